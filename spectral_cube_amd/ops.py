"""Functional layer over the C ABI: one Python function per entry point of
include/spcube_hip.h, operating on :class:`DeviceArray` cubes.

Each function names the reference code it stands in for (paths relative to the
reference tree).  There is no CPU fallback here.
"""
import ctypes as C
import os
import threading
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from . import _lib, moments_forms
from .device import DeviceArray, _sh
from .moments_forms import _MomentsList, _MomentsVlist, _bits_lock, _cube_key, _switch_on, list_is_kept, vlist_is_kept


@dataclass
class MaskSpec:
    """Device-evaluable mask (AND of the enabled terms); see SPC_MASK_* in
    include/spcube_hip.h and spectral_cube/masks.py:105-116, 425-435.

    A spec that is used again is taken to describe the same mask, and one used again on the same cube the same samples:
    moments() then reads the array term as bits, as a list of the included lane segments, as a list of the included voxels
    (moments_forms has the rules, the keys and the costs; the slots below are its state, changed under its lock).  Bytes or
    samples changed behind the library's back - through the raw pointer, by a kernel of the caller's - after a spec's second
    use need invalidate()."""
    flags: int = 0
    thr_lo: float = 0.0
    thr_hi: float = 0.0
    array: Optional[DeviceArray] = None      # uint8, same shape as the cube
    # the packed form of the array term (moments()): not part of what the spec says, so neither compared nor printed
    _bits: Optional[DeviceArray] = field(default=None, init=False, compare=False, repr=False)
    _bits_key: Optional[tuple] = field(default=None, init=False, compare=False, repr=False)
    _bits_uses: int = field(default=0, init=False, compare=False, repr=False)
    _bits_failed: bool = field(default=False, init=False, compare=False, repr=False)   # no form / no memory: stay with the bytes
    # the list of the lane segments the bits include in ONE cube (moments_forms.select): beside the bits, under their lock
    _list: Optional[object] = field(default=None, init=False, compare=False, repr=False)
    _list_key: Optional[tuple] = field(default=None, init=False, compare=False, repr=False)      # the cube of the launch before
    _list_root: Optional[object] = field(default=None, init=False, compare=False, repr=False)    # weakref to that cube's root array
    _list_failed: bool = field(default=False, init=False, compare=False, repr=False)   # refused / no form / no memory: the bits march
    # the voxel list made from _list (moments_forms.select): dropped wherever the list is, under the same lock
    _vlist: Optional[object] = field(default=None, init=False, compare=False, repr=False)
    _vlist_failed: bool = field(default=False, init=False, compare=False, repr=False)  # refused / switched off / no memory: the list

    def invalidate(self):
        """forget the packed form of the array term and the list made from it, and start counting uses again: after the
        array's bytes - or the samples of the cube a list was made of - were changed by something other than upload() or an
        operator of this package"""
        with _bits_lock:
            self._drop_bits()

    def _drop_bits(self):
        self._bits = None                    # (the buffer goes back through spc_free, which waits for the launches that read it)
        self._bits_key = None
        self._bits_uses = 0
        self._bits_failed = False
        self._drop_list()                    # the list holds what THESE bits include

    def _drop_list(self):
        self._list = None
        self._list_key = None
        self._list_root = None
        self._list_failed = False
        self._vlist = None                   # the voxel list holds what THIS list holds
        self._vlist_failed = False

    def to_c(self, wide=False):
        """spc_mask_f32, or (*wide*) spc_mask_f64: the thresholds as they are (a float64 cube is compared in float64)"""
        m = _lib.SpcMask64() if wide else _lib.SpcMask()
        m.flags, m.thr_lo, m.thr_hi = self.flags, self.thr_lo, self.thr_hi
        m.row_stride = m.plane_stride = 0
        if self.flags & _lib.MASK_ARRAY:
            if self.array is None:
                raise ValueError("MASK_ARRAY set without an array")
            m.d_array = self.array.ptr
            # always the array's OWN strides: 0 would mean "the cube's" on the C side, which walks a contiguous mask
            # with the strides of a rows() / planes() view of a larger cube
            shp = self.array.shape
            m.row_stride = getattr(self.array, "row_stride", shp[-1])
            m.plane_stride = getattr(self.array, "plane_stride", shp[-2] * shp[-1] if len(shp) >= 2 else shp[-1])
        return m

    def rows(self, y0, y1):
        """the same mask restricted to rows [y0, y1) (strided view of the array term)"""
        return MaskSpec(self.flags, self.thr_lo, self.thr_hi,
                        self.array.rows(y0, y1) if self.array is not None else None)

    def swap01(self):
        """the same mask for DeviceArray.swap01() views"""
        return MaskSpec(self.flags, self.thr_lo, self.thr_hi, self.array.swap01() if self.array is not None else None)

    def planes(self, z0, z1):
        """the same mask restricted to channels [z0, z1)"""
        return MaskSpec(self.flags, self.thr_lo, self.thr_hi,
                        self.array.planes(z0, z1) if self.array is not None else None)


_F32, _F64 = np.dtype(np.float32), np.dtype(np.float64)


def _written(a):
    """the operator has queued a write into *a*, an array the caller may have given (or None): a MaskSpec that has packed
    its bytes packs them again, and one that holds the list of a cube's included samples builds it again
    (DeviceArray.mark_written; arrays that are no DeviceArray keep no count)"""
    mark = getattr(a, "mark_written", None)
    if mark is not None:
        mark()


def _cube_c(cube, dtype=None):
    """spc_cube_f32 / spc_cube_f64 (one layout) of a float32 or float64 cube; *dtype*: the one sample type an operator
    without the other form takes"""
    ok = (_F32, _F64) if dtype is None else (dtype,)
    if cube.dtype not in ok or len(cube.shape) != 3:
        raise TypeError("cube must be a %s DeviceArray of shape (nz, ny, nx)" % " or ".join(d.name for d in ok))
    c = _lib.SpcCube()
    c.d_data = cube.ptr
    c.nz, c.ny, c.nx = cube.shape
    c.row_stride = getattr(cube, "row_stride", cube.shape[2])          # DeviceArray.rows() views
    c.plane_stride = getattr(cube, "plane_stride", cube.shape[1] * cube.shape[2])
    return c


def _mask_c(mask, cube):
    if mask is None:
        mask = MaskSpec()
    if mask.array is not None:
        if mask.array.shape != cube.shape or mask.array.dtype.itemsize != 1:
            raise ValueError("mask array must be 1-byte and match the cube shape")
    return mask.to_c(wide=cube.dtype == _F64)


def _entry(base, cube, f32="_f32"):
    """(exported symbol, output dtype) of operator *base* on *cube*: spc_<base>_f32 and float32, or spc_<base>_f64 and
    float64 for a float64 cube (the reference keeps a float64 cube in float64, masks.py:225)"""
    if cube.dtype == _F64:
        return "spc_%s_f64" % base, _F64
    return "spc_%s%s" % (base, f32), _F32


def _kern(k):
    k = np.ascontiguousarray(k, dtype=np.float64).ravel()
    return k, k.ctypes.data_as(C.POINTER(C.c_double))


# ---- device scratch: one reusable buffer per (device, stream, host thread) ---------------------------
# The C ABI never allocates (include/spcube_hip.h): every call gets its scratch from the caller.  Calls
# queued on one stream run one after the other, so they can share ONE buffer that only ever grows; two
# streams, or two host threads (dask `threads` workers), get their own.  Growing replaces the buffer -
# the old one goes back through spc_free, which waits for the work still using it.
_ws_lock = threading.Lock()
_ws_cache = {}


def workspace(device, stream, kind, nz, ny, nx, p0=0, p1=0, explicit=None):
    """(c_void_p, nbytes) of a device scratch buffer large enough for entry point *kind* (a
    _lib.WS_* constant) - *explicit* (a DeviceArray) when the caller manages its own."""
    need = int(_lib.load().spc_workspace_bytes(int(kind), int(nz), int(ny), int(nx), int(p0), int(p1)))
    if explicit is not None:
        if explicit.nbytes < need:
            raise ValueError("workspace of %d bytes given, %d needed" % (explicit.nbytes, need))
        return C.c_void_p(explicit.ptr), explicit.nbytes
    return _pooled_scratch(device, stream, need)


def _pooled_scratch(device, stream, need):
    """(c_void_p, nbytes) of the (device, stream, thread) scratch buffer, grown to *need* bytes: for the entries that size
    their scratch with a function of their own (spc_percentile_groups_workspace_bytes) as for the kinds of workspace()"""
    h = _sh(stream)
    key = (device, getattr(h, "value", h) or 0, threading.get_ident())
    with _ws_lock:
        buf = _ws_cache.get(key)
        if buf is None or buf.nbytes < need:
            buf = DeviceArray((max(need, 1 << 16),), np.uint8, device)
            _ws_cache[key] = buf
    return C.c_void_p(buf.ptr), buf.nbytes


def release_workspaces():
    """drop every cached scratch buffer (they return to the pool of spc_malloc)"""
    with _ws_lock:
        _ws_cache.clear()


_WANT_ALL = ("m0", "m1", "m2")


def _moment_outputs(shape2d, device, want, out=None):
    types = dict(m0=np.float64, m1=np.float64, m2=np.float64, mu=np.float64, s0=np.float64,
                 argmax=np.int64, argmin=np.int64, vmax=np.float32, vmin=np.float32,
                 nvalid=np.int32)
    bufs = {}
    o = _lib.SpcMomentOutputs()
    for name in want:
        if name not in types:
            raise ValueError("unknown moment output %r" % name)
        if out is not None and name in out:
            bufs[name] = out[name]
            if bufs[name].shape != tuple(shape2d) or bufs[name].dtype != np.dtype(types[name]):
                raise ValueError("preallocated output %r has wrong shape/dtype" % name)
            _written(bufs[name])
        else:
            bufs[name] = DeviceArray(shape2d, types[name], device)
        setattr(o, "d_" + name, bufs[name].ptr)
    o.out_row_stride = 0
    return o, bufs


def moments(cube, cen, dv=1.0, m1_add=0.0, mask=None, want=_WANT_ALL, stream=None, workspace=None,
            out=None):
    """Fused masked moment 0/1/2 (+argmax/argmin/max/min/count) along axis 0.

    Stands in for DaskSpectralCubeMixin.moment arithmetic
    (spectral_cube/dask_spectral_cube.py:1083-1104), moment_cubewise /
    slicewise / raywise (spectral_cube/_moments.py:30-193), allbadtonan
    (np_compat.py:3-27) and argmax/argmin (spectral_cube.py:793-819).

    cen: DeviceArray of nz float64 = pix_cen[z] - c_ref.  Returns a dict of
    (ny, nx) DeviceArrays for the names in *want*.
    """
    nz, ny, nx = cube.shape
    if cen.dtype != np.float64 or cen.shape != (nz,):
        raise TypeError("cen must be a float64 DeviceArray of length nz")
    o, bufs = _moment_outputs((ny, nx), cube.device, want, out)
    need = _lib.load().spc_moments_workspace_bytes(nz, ny, nx)
    ws = workspace
    if need and (ws is None or ws.nbytes < need):
        ws = DeviceArray((need,), np.uint8, cube.device)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    wsp = (C.c_void_p(ws.ptr if ws is not None else 0), ws.nbytes if ws is not None else 0)
    common = (cube.device, _sh(stream), C.byref(c), C.byref(m), C.c_void_p(cen.ptr), float(dv), float(m1_add), C.byref(o)) + wsp
    # the form a reused mask and cube are read in; *held* keeps its buffers from being freed by a drop in another thread
    # until the launch that reads them has been queued (spc_free then waits for that launch)
    entry, extra, held = moments_forms.select(mask, cube, stream, c, m, o, wsp)
    _lib.call(entry, *common, *extra)
    del held
    bufs["_workspace"] = ws
    return bufs


_WANT_F64 = ("m0", "m1", "m2", "mu", "s0", "argmax", "argmin", "vmax", "vmin", "nvalid")


def moments_f64(cube, cen, dv=1.0, m1_add=0.0, mask=None, want=("m0", "m1", "m2"), stream=None):
    """Masked moment 0 / 1 / 2 (+ argmax / argmin / max / min / count) along axis 0 of a FLOAT64 cube, in the source's own
    precision: the reference keeps a float64 cube in float64 (masks.py:225) and so are its moment maps
    (_moments.py:30-193, dask_spectral_cube.py:1083-1104).  One pass gives S0, S1, the count and the extrema
    (spc_moments_f64); moment 2 is a second pass about the first moment (spc_moment_order_f64, the reference's own form,
    _moments.py:185-193).  The thresholds of *mask* are compared in float64; ``vmax`` / ``vmin`` are float64 maps."""
    nz, ny, nx = cube.shape
    if cen.dtype != np.float64 or cen.shape != (nz,):
        raise TypeError("cen must be a float64 DeviceArray of length nz")
    types = dict(m0=np.float64, m1=np.float64, mu=np.float64, s0=np.float64, argmax=np.int64, argmin=np.int64,
                 vmax=np.float64, vmin=np.float64, nvalid=np.int32)
    first = [n for n in want if n != "m2"]
    if "m2" in want:
        first += [n for n in ("mu", "s0") if n not in first]
    bufs, o = {}, _lib.SpcMomentOutputs64()
    for name in first:
        if name not in types:
            raise ValueError("unknown moment output %r" % name)
        bufs[name] = DeviceArray((ny, nx), types[name], cube.device)
        setattr(o, "d_" + name, bufs[name].ptr)
    o.out_row_stride = 0
    c, m = _cube_c(cube, _F64), _mask_c(mask, cube)
    _lib.call("spc_moments_f64", cube.device, _sh(stream), C.byref(c), C.byref(m), C.c_void_p(cen.ptr), float(dv), float(m1_add), C.byref(o))
    if "m2" in want:
        bufs["m2"] = moment_order_f64(cube, cen, 2, bufs["mu"], bufs["s0"], mask=mask, stream=stream)
    return {n: bufs[n] for n in want}


def moment_order_f64(cube, cen, order, mu, s0, mask=None, stream=None):
    """sum v (c - mu)^order / S0 of a float64 cube (dask_spectral_cube.py:1094-1099; _moments.py:185-193)"""
    nz, ny, nx = cube.shape
    out = DeviceArray((ny, nx), np.float64, cube.device)
    c, m = _cube_c(cube, _F64), _mask_c(mask, cube)
    _lib.call("spc_moment_order_f64", cube.device, _sh(stream), C.byref(c), C.byref(m), C.c_void_p(cen.ptr), int(order),
              C.c_void_p(mu.ptr), C.c_void_p(s0.ptr), C.c_void_p(out.ptr), 0)
    return out


def sigma_clip_axis0_f64(cube, sigma=3.0, sigma_lower=None, sigma_upper=None, maxiters=5, cenfunc="median", stdfunc="std", mask=None,
                         stream=None):
    """sigma_clip_axis0 of a float64 cube (spc_sigma_clip_axis0_f64): float64 centre, spread and bounds"""
    if cenfunc not in ("median", "mean") or stdfunc not in ("std", "mad_std"):
        raise ValueError("cenfunc must be 'median' or 'mean', stdfunc 'std' or 'mad_std'")
    out = DeviceArray(cube.shape, np.float64, cube.device)
    c, m = _cube_c(cube, _F64), _mask_c(mask, cube)
    lo = float(sigma if sigma_lower is None else sigma_lower)
    hi = float(sigma if sigma_upper is None else sigma_upper)
    _lib.call("spc_sigma_clip_axis0_f64", cube.device, _sh(stream), C.byref(c), C.byref(m), lo, hi,
              -1 if maxiters is None else int(maxiters), 1 if cenfunc == "mean" else 0, 1 if stdfunc == "mad_std" else 0, C.c_void_p(out.ptr))
    return out


def narrow_f64(cube, stream=None, out=None):
    """float32 copy of a float64 DeviceArray (for the operators without a float64 form); *out* may be a strided view"""
    out = _out_cube(out, cube.shape, np.float32, cube.device)
    c = _cube_c(cube, _F64)
    _lib.call("spc_narrow_f64_to_f32", cube.device, _sh(stream), C.byref(c), C.c_void_p(out.ptr), *_strides(out))
    return out


def _given(out, name, shape, dtype, device):
    """out[name] when the caller preallocated it (checked), else a new DeviceArray"""
    a = out.get(name) if out else None
    if a is None:
        return DeviceArray(shape, dtype, device)
    if tuple(a.shape) != tuple(shape) or a.dtype != np.dtype(dtype):
        raise ValueError("preallocated output %r must be %s %s" % (name, tuple(shape), np.dtype(dtype)))
    _written(a)                  # the operator is about to write into the caller's array
    return a


def argextrema_axis(cube, axis, mask=None, want=("argmax", "argmin"), stream=None, out=None):
    """argmax / argmin along a spatial axis (spectral_cube.py:793-819 with axis = 1 or 2): int64
    maps (nz, nx) / (nz, ny); first index on ties, 0 for rays without an included sample."""
    nz, ny, nx = cube.shape
    if axis not in (1, 2):
        raise ValueError("axis must be 1 or 2 (axis 0 comes out of ops.moments)")
    shape = (nz, nx) if axis == 1 else (nz, ny)
    bufs = {n: _given(out, n, shape, np.int64, cube.device) for n in want if n in ("argmax", "argmin")}
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ptr = lambda n: C.c_void_p(bufs[n].ptr) if n in bufs else None  # noqa: E731
    _lib.call("spc_argextrema_axis_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), int(axis),
              ptr("argmin"), ptr("argmax"))
    return bufs


def moment_order(cube, cen, order, mu, s0, mask=None, stream=None):
    """sum v*(c-mu)^order / S0 - second pass for order > 2
    (dask_spectral_cube.py:1094-1099)."""
    nz, ny, nx = cube.shape
    out = DeviceArray((ny, nx), np.float64, cube.device)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    _lib.call("spc_moment_order_f32", cube.device, _sh(stream), C.byref(c), C.byref(m),
              C.c_void_p(cen.ptr), int(order), C.c_void_p(mu.ptr), C.c_void_p(s0.ptr),
              C.c_void_p(out.ptr), 0)
    return out


def moments_spatial(cube, cen2d, axis, pix_size, mask=None, want=_WANT_ALL, stream=None, out=None):
    """moment 0/1/2 along a spatial axis (golden tables
    spectral_cube/tests/test_moments.py:19-49)."""
    nz, ny, nx = cube.shape
    if axis not in (1, 2):
        raise ValueError("axis must be 1 or 2")
    shape = (nz, nx) if axis == 1 else (nz, ny)
    bufs = {n: _given(out, n, shape, np.float64, cube.device) for n in want}
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ptr = lambda n: C.c_void_p(bufs[n].ptr) if n in bufs else None  # noqa: E731
    _lib.call("spc_moments_spatial_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), int(axis),
              C.c_void_p(cen2d.ptr), float(pix_size), ptr("m0"), ptr("m1"), ptr("m2"))
    return bufs


def moment_order_spatial(cube, cen2d, axis, order, mu, mask=None, stream=None, out=None):
    """sum v (c - mu)^order / sum v along a spatial axis: the second pass for order > 2
    (dask_spectral_cube.py:1094-1099 with axis != 0); *mu* = the m1 map of moments_spatial."""
    nz, ny, nx = cube.shape
    if axis not in (1, 2):
        raise ValueError("axis must be 1 or 2")
    out = _given({"o": out} if out is not None else None, "o", (nz, nx) if axis == 1 else (nz, ny), np.float64, cube.device)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    _lib.call("spc_moment_order_spatial_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), int(axis),
              C.c_void_p(cen2d.ptr), int(order), C.c_void_p(mu.ptr), C.c_void_p(out.ptr))
    return out


def spectral_conv(cube, kernel1d, mask=None, out=None, stream=None):
    """NaN-aware convolution along the spectral axis = chunk function of
    spectral_smooth (dask_spectral_cube.py:880-917); the result has the cube's dtype (the Dask class keeps the chunk
    dtype, dask_spectral_cube.py:829)."""
    name, dtype = _entry("spectral_conv", cube)
    out = _out_cube(out, cube.shape, dtype, cube.device)
    k, kp = _kern(kernel1d)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    # (the float64 kernel sizes its scratch by its own kind)
    ws, wsn = workspace(cube.device, stream, _lib.WS_SPECTRAL_CONV_F64 if dtype == _F64 else _lib.WS_SPECTRAL_CONV, *cube.shape, len(k))
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), kp, len(k),
              C.c_void_p(out.ptr), *_strides(out), ws, wsn)
    return out


def downsample_shape(shape, axis, factor, truncate):
    """shape of the downsampled cube: ceil(n / factor) along *axis*, floor(n / factor) when truncating
    (spectral_cube.py:3511-3513)"""
    out = list(shape)
    n = int(shape[axis])
    out[axis] = n // factor if truncate else -(-n // factor)
    return tuple(out)


def _strides(arr):
    return getattr(arr, "row_stride", 0), getattr(arr, "plane_stride", 0)


def _out_cube(out, shape, dtype, device):
    """*out* when the caller preallocated it (checked as _given checks; it may be a strided view of a larger array, whose
    strides travel with it), else a new DeviceArray"""
    return _given({"out": out} if out is not None else None, "out", shape, dtype, device)


def _contiguous_out(out, shape, dtype, device):
    """_out_cube for the entries that address their output as one contiguous block (their C entry takes no output strides,
    or the wrapper offsets the pointer itself): a strided view is refused here, before anything is launched"""
    if out is not None and getattr(out, "_is_view", False):
        raise ValueError("preallocated output must be a contiguous %s %s, not a strided view" % (tuple(shape), np.dtype(dtype)))
    return _out_cube(out, shape, dtype, device)


def _downsample_outputs(cube, axis, factor, truncate, dtype, out, out_mask):
    shape = downsample_shape(cube.shape, axis, factor, truncate)
    if out is None:
        out = DeviceArray(shape, dtype, cube.device)
    else:
        _written(out)
    if out_mask is None:
        out_mask = DeviceArray(shape, np.uint8, cube.device)
    if tuple(out.shape) != shape or out.dtype != np.dtype(dtype) or tuple(out_mask.shape) != shape or out_mask.dtype != np.uint8:
        raise ValueError("preallocated outputs must be %s %s and %s uint8" % (shape, np.dtype(dtype), shape))
    if _strides(out) != _strides(out_mask):
        raise ValueError("out and out_mask must have the same strides")
    return out, out_mask


def downsample(cube, axis, factor, truncate=False, estimator=_lib.DS_NANMEAN, fill=np.nan, mask=None, out=None, out_mask=None,
               stream=None, nan_excluded=False):
    """(data, include) of the cube block-downsampled along *axis* = SpectralCube.downsample_axis's in-memory form
    (spectral_cube.py:3466-3497): estimator (an SPC_DS_* code) over every run of *factor* filled samples, and any(include)
    over the run's voxels, as a DeviceArray of the cube's dtype and a uint8 one.  *out* / *out_mask* may be strided views (rows() /
    planes()) of larger outputs: a strip is written in place.  *nan_excluded*: NaN samples count as excluded (the
    ~isnan mask of the cube's own data, which lowers to no MaskSpec term)."""
    name, dtype = _entry("downsample", cube)
    out, out_mask = _downsample_outputs(cube, axis, factor, truncate, dtype, out, out_mask)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    ors, ops_ = _strides(out)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, float(fill),
              int(axis), int(factor), 1 if truncate else 0, int(estimator), C.c_void_p(out.ptr), ors, ops_, C.c_void_p(out_mask.ptr))
    _written(out_mask)
    return out, out_mask


def _rank_filter(base, cube, sizes, rank, mode, cval, fill, mask, out, stream, nan_excluded):
    name, dtype = _entry(base, cube)
    if mode not in _lib.RANK_MODES:
        raise ValueError("mode must be one of %s (got %r)" % (", ".join(sorted(_lib.RANK_MODES)), mode))
    if out is None:
        out = DeviceArray(cube.shape, dtype, cube.device)
    else:
        _written(out)
    if tuple(out.shape) != tuple(cube.shape) or out.dtype != dtype:
        raise ValueError("preallocated output must be %s %s" % (tuple(cube.shape), dtype))
    c, m = _cube_c(cube), _mask_c(mask, cube)
    ors, ops_ = _strides(out)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, float(fill),
              *[int(s) for s in sizes], int(rank), _lib.RANK_MODES[mode], float(cval), C.c_void_p(out.ptr), ors, ops_)
    return out


def rank_filter_axis0(cube, ksize, rank, mode="reflect", cval=0.0, fill=np.nan, mask=None, out=None, stream=None,
                      nan_excluded=False):
    """element *rank* of the sorted window of *ksize* FILLED samples along the spectral axis, for every voxel = the chunk
    function of spectral_smooth_median / spectral_filter with one of scipy.ndimage's rank filters (spectral_cube.py:2844-2898,
    dask_spectral_cube.py:920-960); *mode* / *cval* as scipy names them.  NaN ranks last (``np.sort(window)[rank]``).  The
    result has the cube's dtype and holds samples of the cube bit for bit.  *nan_excluded* as for ``downsample``."""
    return _rank_filter("rank_filter_axis0", cube, (ksize,), rank, mode, cval, fill, mask, out, stream, nan_excluded)


def rank_filter_plane(cube, ky, kx, rank, mode="reflect", cval=0.0, fill=np.nan, mask=None, out=None, stream=None,
                      nan_excluded=False):
    """rank_filter_axis0 with a window of *ky* x *kx* samples of every image plane: spatial_smooth_median / spatial_filter
    (spectral_cube.py:2749-2806, dask_spectral_cube.py:995-1029)"""
    return _rank_filter("rank_filter_plane", cube, (ky, kx), rank, mode, cval, fill, mask, out, stream, nan_excluded)


def _stack_inputs(cube, idx, shifts, pad, fused):
    """(device idx, device shifts, npos, (pad_lo, pad_hi), workspace) of the two stack operators: the positions are checked on
    the host (the kernel would give an all-NaN row for one outside the map) and travel as int32"""
    idx = np.ascontiguousarray(idx, dtype=np.int64).ravel()
    shifts = np.ascontiguousarray(shifts, dtype=np.float64).ravel()
    nz, ny, nx = cube.shape
    if idx.size < 1 or idx.size != shifts.size:
        raise ValueError("need one shift per position and at least one position (got %d and %d)" % (idx.size, shifts.size))
    if ny * nx > 2**31 - 1:
        raise ValueError("a map of %d x %d spaxels does not index with int32" % (ny, nx))
    if idx.min() < 0 or idx.max() >= ny * nx:
        raise IndexError("position outside the %d x %d map" % (ny, nx))
    pad_lo, pad_hi = int(pad[0]), int(pad[1])
    if pad_lo < 0 or pad_hi < 0:
        raise ValueError("pads must not be negative (got %r)" % (pad,))
    need = int(_lib.load().spc_stack_workspace_bytes(nz, idx.size, min(pad_lo, 2**30), min(pad_hi, 2**30), 1 if fused else 0))
    ws = DeviceArray((max(need, 256),), np.uint8, cube.device)
    d_idx = DeviceArray.from_numpy(idx.astype(np.int32), cube.device)
    d_shift = DeviceArray.from_numpy(shifts, cube.device)
    return d_idx, d_shift, idx.size, (min(pad_lo, 2**30), min(pad_hi, 2**30)), ws


def stack_shift(cube, idx, shifts, pad=(0, 0), fill=np.nan, mask=None, out=None, stream=None, nan_excluded=False):
    """(M, P) float64 DeviceArray of the P filled spectra at the flat spaxel indices *idx* (y * nx + x), zero-padded by
    *pad* = (front, back) channels and Fourier-shifted by *shifts* channels each: column p is
    ``fourier_shift(cube.filled_data[:, y, x], shifts[p], add_pad=True, pad_size=pad)`` (analysis_utilities.py:14-94), M = nz
    + front + back.  A NaN shift or a spectrum without a finite sample gives an all-NaN column.  *idx* and *shifts* are host
    arrays.  M above _lib.STACK_MAX_CHANNELS raises HipUnsupported."""
    name, _ = _entry("stack_shift", cube)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    d_idx, d_shift, npos, (pad_lo, pad_hi), ws = _stack_inputs(cube, idx, shifts, pad, False)
    shape = (cube.shape[0] + pad_lo + pad_hi, npos)
    if out is None:
        out = DeviceArray(shape if shape[0] <= _lib.STACK_MAX_CHANNELS else (1, 1), np.float64, cube.device)
    elif tuple(out.shape) != shape or out.dtype != _F64:
        raise ValueError("preallocated output must be %s float64" % (shape,))
    else:
        _written(out)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, float(fill),
              C.c_void_p(d_idx.ptr), C.c_void_p(d_shift.ptr), npos, pad_lo, pad_hi, C.c_void_p(out.ptr), C.c_void_p(ws.ptr), ws.nbytes)
    if stream is not None:                   # (the inputs and the workspace go back to the pool when this returns)
        _lib.call("spc_stream_sync", cube.device, _sh(stream))
    return out


def stack_sum(cube, idx, shifts, pad=(0, 0), fill=np.nan, mask=None, stream=None, nan_excluded=False):
    """(sum, count, nan_count) over the rows of ``stack_shift`` without writing them: per output channel the float64 sum of
    the rows that are not NaN there, their number and the number of rows that are NaN (int64), as host arrays of length M -
    what np.nanmean / np.mean / np.nansum / np.sum of stack_spectra (analysis_utilities.py:301-304) are finished from.
    Reproducible: partial sums per block, added in a fixed order."""
    name, _ = _entry("stack_sum", cube)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    d_idx, d_shift, npos, (pad_lo, pad_hi), ws = _stack_inputs(cube, idx, shifts, pad, True)
    M = min(cube.shape[0] + pad_lo + pad_hi, _lib.STACK_MAX_CHANNELS)
    total = DeviceArray((M,), np.float64, cube.device)
    count = DeviceArray((M,), np.int64, cube.device)
    nnan = DeviceArray((M,), np.int64, cube.device)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, float(fill),
              C.c_void_p(d_idx.ptr), C.c_void_p(d_shift.ptr), npos, pad_lo, pad_hi, C.c_void_p(total.ptr), C.c_void_p(count.ptr),
              C.c_void_p(nnan.ptr), C.c_void_p(ws.ptr), ws.nbytes)
    return total.get(stream), count.get(stream), nnan.get(stream)


def stack_cube(cube, lo, t, inv_dx, exact, mode="nanmean", fill=np.nan, mask=None, out=None, stream=None, nan_excluded=False):
    """(n0, ny, nx) DeviceArray in the cube's dtype: ``average(cutouts, axis=0)`` of stack_cube (analysis_utilities.py:
    321-432) without a cutout.  Row s of the (S, n0) host tables *lo* / *t* / *inv_dx* is the plan of ``lerp_plan`` for source
    s in absolute channels of *cube* (-1 = outside the slab): cutout s at output channel j is ``a + (b - a) * inv_dx * t`` of
    the samples lo and lo + 1 (excluded ones NaN), NaN replaced by *fill*; a source with ``exact[s]`` set is its filled
    sample lo as it is.  *mode*: nanmean / mean / nansum / sum, numpy's NaN rules, float64 in source order.  More than
    _lib.STACK_CUBE_MAX_LINES sources raise HipUnsupported before any device work."""
    name, dtype = _entry("stack_cube", cube)
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    t = np.ascontiguousarray(t, dtype=np.float64)
    inv_dx = np.ascontiguousarray(inv_dx, dtype=np.float64)
    exact = np.ascontiguousarray(exact, dtype=np.int32).ravel()
    if lo.ndim != 2 or t.shape != lo.shape or inv_dx.shape != lo.shape or exact.size != lo.shape[0]:
        raise ValueError("lo, t and inv_dx must be (S, n0) tables and exact of length S (got %s, %s, %s, %s)"
                         % (lo.shape, t.shape, inv_dx.shape, exact.shape))
    nsrc, n0 = lo.shape
    if nsrc > _lib.STACK_CUBE_MAX_LINES:
        raise _lib.HipUnsupported("%d sources are above the built limit of %d (STACK_CUBE_MAX_LINES)" % (nsrc, _lib.STACK_CUBE_MAX_LINES))
    if mode not in _lib.STACK_CUBE_MODES:
        raise ValueError("mode must be one of %s (got %r)" % (sorted(_lib.STACK_CUBE_MODES), mode))
    c, m = _cube_c(cube), _mask_c(mask, cube)
    shape = (n0,) + tuple(cube.shape[1:])
    if out is None:
        out = DeviceArray(shape if nsrc >= 1 and 2 <= n0 <= cube.shape[0] else (1, 1, 1), dtype, cube.device)
    else:
        out = _contiguous_out(out, shape, dtype, cube.device)          # (the entry takes no output strides)
    ws = DeviceArray((int(_lib.load().spc_stack_cube_workspace_bytes(nsrc, n0)),), np.uint8, cube.device)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, float(fill), nsrc,
              lo.ctypes.data_as(C.c_void_p), t.ctypes.data_as(C.c_void_p), inv_dx.ctypes.data_as(C.c_void_p),
              exact.ctypes.data_as(C.c_void_p), _lib.STACK_CUBE_MODES[mode], n0, C.c_void_p(out.ptr), C.c_void_p(ws.ptr), ws.nbytes)
    if stream is not None:                   # (the workspace goes back to the pool when this returns)
        _lib.call("spc_stream_sync", cube.device, _sh(stream))
    return out


def mosaic(cubes, maps, masks, fills, order, weights=None, out=None, stream=None):
    """(nz, ny_out, nx_out) DeviceArray in the cubes' dtype: the co-added mosaic of mosaic_cubes (cube_utils.py:810-856) in
    one kernel.  *cubes*: S DeviceArrays of one dtype (float32 or float64) and one number of channels; *maps*: per cube its
    ``(xs, ys)`` float64 (ny_out, nx_out) DeviceArrays of source pixel coordinates (``wcs_pixel_map``); *masks*: per cube a
    MaskSpec or None; *fills*: per cube the fill value that replaces excluded voxels (and that the cube contributes outside
    its footprint, NaN counting as 0).  *order*: 1 bilinear, 0 nearest neighbour.  Per output voxel: the float64 sum, in list
    order, of nan_to_num of what ``resample_bilinear`` gives for each cube (the same bits), divided by the number of cubes
    whose footprint holds the pixel (NaN where none does), rounded once.  *weights*: optional int32 (ny_out, nx_out)
    DeviceArray that receives that number."""
    cubes, maps = list(cubes), list(maps)
    nsrc = len(cubes)
    if nsrc < 1:
        raise ValueError("an empty list of cubes")
    masks = [None] * nsrc if masks is None else list(masks)
    fills = list(fills)
    if not (len(maps) == len(masks) == len(fills) == nsrc):
        raise ValueError("cubes, maps, masks and fills must have one entry per cube")
    if int(order) not in (0, 1):
        raise ValueError("order must be 1 (bilinear) or 0 (nearest neighbour), got %r" % (order,))
    first = cubes[0]
    name, dtype = _entry("mosaic", first)
    dev, nz = first.device, first.shape[0]
    shape_yx = tuple(maps[0][0].shape)
    wide = dtype == _F64
    tab = ((_lib.SpcMosaicSource64 if wide else _lib.SpcMosaicSource) * nsrc)()
    for s, (cube, (xs, ys), mask, fill) in enumerate(zip(cubes, maps, masks, fills)):
        if cube.dtype != dtype or len(cube.shape) != 3 or cube.shape[0] != nz:
            raise TypeError("every cube must be a %s DeviceArray with %d channels (cube %d: %s %s)"
                            % (dtype.name, nz, s, cube.dtype, cube.shape))
        for m in (xs, ys):
            if not isinstance(m, DeviceArray) or m.dtype != np.float64 or tuple(m.shape) != shape_yx or len(shape_yx) != 2:
                raise ValueError("maps must be pairs of float64 DeviceArrays of one (ny_out, nx_out) shape (cube %d)" % s)
        tab[s].cube, tab[s].mask = _cube_c(cube), _mask_c(mask, cube)
        tab[s].fill = float(fill)
        tab[s].d_xs, tab[s].d_ys = xs.ptr, ys.ptr
    shape = (nz,) + shape_yx
    if out is None:
        out = DeviceArray(shape, dtype, dev)
    elif tuple(out.shape) != shape or out.dtype != dtype or getattr(out, "_is_view", False):
        raise ValueError("preallocated output must be a contiguous %s %s" % (shape, dtype))
    else:
        _written(out)
    if weights is not None and (tuple(weights.shape) != shape_yx or weights.dtype != np.int32):
        raise ValueError("weights must be an int32 %s DeviceArray" % (shape_yx,))
    ws = DeviceArray((int(_lib.load().spc_mosaic_workspace_bytes(nsrc)),), np.uint8, dev)
    _lib.call(name, dev, _sh(stream), nsrc, tab, nz, shape_yx[0], shape_yx[1], int(order), C.c_void_p(out.ptr),
              C.c_void_p(weights.ptr) if weights is not None else None, C.c_void_p(ws.ptr), ws.nbytes)
    if stream is not None:                   # (the workspace goes back to the pool when this returns)
        _lib.call("spc_stream_sync", dev, _sh(stream))
    return out


def normalize_view(view, shape):
    """(start, step, length) per axis of a tuple of three slices applied to *shape* (``slice.indices``, as numpy indexes)"""
    out = []
    for sl, n in zip(view, shape):
        start, stop, step = sl.indices(int(n))
        out.append((start, step, len(range(start, stop, step))))
    return out


def subcube(cube, start, step, shape, mask=None, out=None, out_mask=None, want_mask=True, filled=False, fill=np.nan,
            stream=None, nan_excluded=False):
    """(data, include) of ``cube[start[a] :: step[a]]`` cut to *shape* = SpectralCube.__getitem__ with three slices
    (spectral_cube.py:1308-1381): output sample (k, j, i) is parent sample (start + (k, j, i) * step), copied bit for bit
    in the cube's dtype (*filled*: excluded voxels become *fill*), and the include byte of the parent's mask there.  ``want_mask=False``
    (a parent without a mask) skips the mask output and returns None for it.  *out* / *out_mask* may be strided views
    of larger outputs."""
    name, dtype = _entry("subcube", cube)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    shape = tuple(int(n) for n in shape)
    if out is None:
        out = DeviceArray(shape, dtype, cube.device)
    else:
        _written(out)
    if out_mask is None and want_mask:
        out_mask = DeviceArray(shape, np.uint8, cube.device)
    if tuple(out.shape) != shape or out.dtype != dtype:
        raise ValueError("preallocated output must be %s %s" % (shape, dtype))
    if out_mask is not None:
        if tuple(out_mask.shape) != shape or out_mask.dtype != np.uint8:
            raise ValueError("preallocated mask output must be %s uint8" % (shape,))
        if _strides(out) != _strides(out_mask):
            raise ValueError("out and out_mask must have the same strides")
    ors, ops_ = _strides(out)
    st3, sp3 = (C.c_int64 * 3)(*[int(v) for v in start]), (C.c_int64 * 3)(*[int(v) for v in step])
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, st3, sp3,
              shape[0], shape[1], shape[2], C.c_void_p(out.ptr), ors, ops_,
              C.c_void_p(out_mask.ptr) if out_mask is not None else None, 1 if filled else 0, float(fill))
    _written(out_mask)
    return out, out_mask


def pv_extract(data, xs, ys, order=1, respect_nan=True, mask_spec=None, fill=np.nan, out=None, count=None, stream=None,
               nan_excluded=False):
    """(nz, npts) DeviceArray in the cube's dtype: the position-velocity diagram of the float32 / float64 cube *data* (a
    strided view is read in place) along the path whose pixel positions are *xs*, *ys* - host arrays or float64
    DeviceArrays of shape (npts,) or (nlines, npts), 0-based - averaged over the lines (spc_pv_extract_f32 / _f64; stands in
    for pvextractor.extract_pv_slice behind SpectralCube.to_pvextractor, spectral_cube.py:2506-2513, and for the
    axis-aligned cube[:, j, :]).  A sample is the FILLED cube's: *fill* where *mask_spec* (the cube's MaskSpec; None: no
    mask; *nan_excluded* as in subcube) excludes the voxel, and such a sample is not fetched.  A point is inside when
    0 <= x <= nx - 1 and 0 <= y <= ny - 1 and NaN otherwise (scipy's mode='constant', cval=nan).  *order* 0: the sample at
    (floor(y + 0.5), floor(x + 0.5)); 1: bilinear in float64, a neighbour of weight exactly 0 neither read nor counted.
    *respect_nan*: a NaN neighbour of non-zero weight makes the line's value NaN; otherwise it adds 0.  The result is the
    mean over the lines whose value is not NaN, added in line order in float64 and rounded once; NaN when there is none.
    *count*: an int32 (nz, npts) DeviceArray that receives the number of such lines.  *out* / *count* may hold anything.
    Two calls give the same bits (no atomics)."""
    name, dtype = _entry("pv_extract", data)
    c, m = _cube_c(data), _mask_c(mask_spec, data)
    if int(order) not in (0, 1) or order != int(order):
        raise ValueError("order %r is not built on the device: 0 (nearest) or 1 (bilinear)" % (order,))
    if isinstance(xs, DeviceArray) and isinstance(ys, DeviceArray):
        if xs.dtype != _F64 or ys.dtype != _F64 or xs.shape != ys.shape or len(xs.shape) not in (1, 2):
            raise ValueError("xs, ys must be float64 arrays of one shape, (npts,) or (nlines, npts)")
        d_xs, d_ys = xs, ys
    else:
        xs, ys = np.ascontiguousarray(xs, dtype=np.float64), np.ascontiguousarray(ys, dtype=np.float64)
        if xs.shape != ys.shape or xs.ndim not in (1, 2):
            raise ValueError("xs, ys must have one shape, (npts,) or (nlines, npts) (got %s and %s)" % (xs.shape, ys.shape))
        d_xs, d_ys = (DeviceArray.from_numpy(a, data.device, stream) if a.size else None for a in (xs, ys))
    shape2 = tuple(int(n) for n in xs.shape)
    nlines, npts = shape2 if len(shape2) == 2 else (1, shape2[0])
    if npts < 1 or nlines < 1:
        raise ValueError("a path needs at least one point and one line (got %d lines of %d points)" % (nlines, npts))
    nz = int(data.shape[0])
    out = _given({"out": out}, "out", (nz, npts), dtype, data.device)
    if count is not None and (tuple(count.shape) != (nz, npts) or count.dtype != np.dtype(np.int32)):
        raise ValueError("count must be an int32 array of shape %s" % ((nz, npts),))
    _lib.call(name, data.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, float(fill), npts, nlines,
              C.c_void_p(d_xs.ptr), C.c_void_p(d_ys.ptr), int(order), 1 if respect_nan else 0, C.c_void_p(out.ptr),
              getattr(out, "row_stride", npts), C.c_void_p(count.ptr) if count is not None else None,
              getattr(count, "row_stride", npts))
    out._plan = (d_xs, d_ys)             # the uploads stay alive until the result goes
    return out


def baseline_abscissa(nz):
    """t_k = (2k - (nz - 1)) / (nz - 1), the channel index on [-1, 1] (float64; t_0 = 0 when nz == 1)"""
    nz = int(nz)
    if nz == 1:
        return np.zeros(1, np.float64)
    return (2.0 * np.arange(nz, dtype=np.float64) - (nz - 1)) / (nz - 1)


def baseline_basis(nz, order):
    """(nz, order + 1) float64: the Legendre table P_j(t_k) the baseline entries take (include/spcube_hip.h), computed on
    the host with numpy.polynomial.legendre.legvander - the device never recomputes a basis value"""
    return np.ascontiguousarray(np.polynomial.legendre.legvander(baseline_abscissa(nz), int(order)), dtype=np.float64)


def _baseline_order(order):
    if isinstance(order, bool) or not isinstance(order, (int, np.integer)) or not 0 <= int(order) <= _lib.BASELINE_MAX_ORDER:
        raise ValueError("order must be an integer from 0 to %d (got %r)" % (_lib.BASELINE_MAX_ORDER, order))
    return int(order)


def baseline_channels(channels, nz):
    """the channel list of a baseline fit as increasing int32 channel numbers: *channels* is None (all), a boolean (nz,)
    array, or integer indices (negative ones count from the end; duplicates are dropped).  ValueError for anything else"""
    nz = int(nz)
    if channels is None:
        return np.arange(nz, dtype=np.int32)
    c = np.asarray(channels)
    if c.dtype == np.bool_:
        if c.shape != (nz,):
            raise ValueError("a boolean channel selection must have shape (%d,) (got %s)" % (nz, c.shape))
        return np.flatnonzero(c).astype(np.int32)
    if c.ndim != 1 or (c.size and c.dtype.kind not in "iu"):
        raise ValueError("channels must be a boolean (nz,) array or a 1-D list of integer indices")
    c = c.astype(np.int64)
    if c.size and (c.min() < -nz or c.max() >= nz):
        raise ValueError("channel index out of range for %d channels" % nz)
    return np.unique(np.where(c < 0, c + nz, c)).astype(np.int32)


def baseline_segments(shape, nfit):
    """how many segments spc_baseline_fit_* cuts a channel list of *nfit* entries into for a cube of *shape*: a fixed rule
    on the plane and nfit (1: the fit kernel solves itself; more: partial sums through the workspace, added in order)"""
    nz, ny, nx = (int(n) for n in shape)
    return int(_lib.load().spc_baseline_segments(nz, ny, nx, int(nfit)))


def baseline_fit(data, order, channels=None, mask_spec=None, coef=None, npts=None, stream=None, workspace=None):
    """(coef, npts): the Legendre coefficients, a float64 (order + 1, ny, nx) DeviceArray, of the polynomial of *order*
    (0 ... 5) fitted by least squares to every spectrum of the float32 / float64 cube *data* (a strided view is read in
    place), and the int32 (ny, nx) number of samples each fit used (spc_baseline_fit_f32 / _f64; stands in for a per-spectrum
    polyfit through apply_function_parallel_spectral, spectral_cube.py:3103, and for CASA's imcontsub fitorder=n).  A
    spectrum is fitted on the channels of *channels* (None: all; a boolean (nz,) array or integer indices, host side)
    whose voxel *mask_spec* (the cube's MaskSpec; None: no mask) includes and whose sample is not NaN; other channels are
    not read.  The abscissa is the channel index mapped to [-1, 1]; sums, the L D L^T solve and the coefficients are
    float64.  Fewer than order + 1 samples, or a pivot that is not positive: NaN coefficients.  *coef*, *npts*: preallocated
    outputs; *workspace*: a uint8 DeviceArray of spc_baseline_workspace_bytes bytes (the stream's pooled scratch
    otherwise).  All three may hold anything.  Two calls give the same bits (no atomics)."""
    name, _ = _entry("baseline_fit", data)
    order = _baseline_order(order)
    c, m = _cube_c(data), _mask_c(mask_spec, data)
    nz, ny, nx = (int(n) for n in data.shape)
    chan = baseline_channels(channels, nz)
    if chan.size < 1:
        raise ValueError("the channel list is empty")
    given = {"coef": coef, "npts": npts}
    for a in (coef, npts):
        if a is not None and getattr(a, "_is_view", False):
            raise ValueError("coef and npts must be contiguous arrays, not strided views")
    coef = _given(given, "coef", (order + 1, ny, nx), np.float64, data.device)
    npts = _given(given, "npts", (ny, nx), np.int32, data.device)
    d_basis = DeviceArray.from_numpy(baseline_basis(nz, order), data.device, stream)
    d_chan = None if channels is None else DeviceArray.from_numpy(chan, data.device, stream)
    need = int(_lib.load().spc_baseline_workspace_bytes(nz, ny, nx, int(chan.size), order))
    ws, wsn = _scratch(need, workspace, data.device, stream) if need else (None, 0)
    _lib.call(name, data.device, _sh(stream), C.byref(c), C.byref(m), order, C.c_void_p(d_chan.ptr) if d_chan is not None else None,
              int(chan.size), C.c_void_p(d_basis.ptr), C.c_void_p(coef.ptr), C.c_void_p(npts.ptr), ws, wsn)
    coef._plan = (d_basis, d_chan)       # the uploads stay alive until the result goes
    return coef, npts


def baseline_apply(data, coef, subtract=True, out=None, stream=None):
    """A DeviceArray of the cube's shape and dtype: *data* minus the baseline model of *coef* (the (order + 1, ny, nx)
    float64 Legendre coefficients of baseline_fit), or - *subtract* False - the model itself (spc_baseline_apply_f32 / _f64).
    model_k = sum_j c_j P_j(t_k) in float64 for every channel and every voxel, whatever any mask says; a NaN sample stays
    NaN in the difference, NaN coefficients give a NaN spectrum.  *out*: a preallocated array, which may be a strided
    view and may hold anything, but not the cube itself."""
    name, dtype = _entry("baseline_apply", data)
    c = _cube_c(data)
    nz, ny, nx = (int(n) for n in data.shape)
    if coef.dtype != _F64 or len(coef.shape) != 3 or tuple(coef.shape[1:]) != (ny, nx) or getattr(coef, "_is_view", False):
        raise ValueError("coef must be a contiguous float64 (order + 1, %d, %d) DeviceArray" % (ny, nx))
    order = _baseline_order(int(coef.shape[0]) - 1)
    out = _out_cube(out, (nz, ny, nx), dtype, data.device)
    ors, ops_ = _strides(out)
    d_basis = DeviceArray.from_numpy(baseline_basis(nz, order), data.device, stream)
    _lib.call(name, data.device, _sh(stream), C.byref(c), order, C.c_void_p(d_basis.ptr), C.c_void_p(coef.ptr),
              0 if subtract else 1, C.c_void_p(out.ptr), ors, ops_)
    out._plan = (d_basis, coef)
    return out


def arith_operand_strides(shape, cube_shape, strides=None):
    """element strides (z, y, x) of an operand of *shape* broadcast against *cube_shape* by numpy's rules, 0 along a
    broadcast axis; *strides*: the operand's own element strides per axis (C-contiguous when None).  ValueError in
    numpy's words when the shapes do not broadcast to the cube's."""
    shape = tuple(int(n) for n in shape)
    if len(shape) > 3 or any(n != 1 and n != m for n, m in zip(shape[::-1], tuple(cube_shape)[::-1])):
        raise ValueError("operands could not be broadcast together with shapes %s %s" % (tuple(cube_shape), shape))
    if strides is None:
        strides = [int(np.prod(shape[a + 1:], dtype=np.int64)) for a in range(len(shape))]
    full = [0] * (3 - len(shape)) + [0 if n == 1 else int(s) for n, s in zip(shape, strides)]
    return tuple(full)


def arith(cube, steps, mask=None, fill=np.nan, out=None, stream=None, nan_excluded=False):
    """A chain of + - * / ** steps over the cube in one pass (SpectralCube.__add__ ... __pow__, spectral_cube.py:2237-2361,
    through _apply_everywhere :912-942 and _cube_on_cube_operation :944-1003): a DeviceArray of the cube's dtype.
    *steps*: up to _lib.ARITH_MAX_STEPS tuples ``(op, operand, refill)``; op a key of _lib.ARITH_OPCODES; operand a Python
    scalar, or a DeviceArray of the cube's dtype whose shape broadcasts to the cube's by numpy's rules (a (ny, nx) map, a
    (nz, 1, 1) spectrum, a cube, ...), or None for the exact power forms square / sqrt / recip / one.  Per voxel the
    include bit of *mask* is taken once on the source sample; a step with *refill* first sets the excluded voxels to
    *fill* (the filled data the reference's _apply_everywhere starts from), then applies op.  + - * / and the exact forms
    are single IEEE operations (no FMA): the result equals numpy's stepwise one bit for bit."""
    name, dtype = _entry("arith", cube)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    steps = list(steps)
    prog = _lib.SpcArithProgram()
    prog.n_steps = len(steps)
    if len(steps) > _lib.ARITH_MAX_STEPS:
        raise _lib.HipInvalidArgument("an arithmetic program holds at most %d steps (got %d)" % (_lib.ARITH_MAX_STEPS, len(steps)))
    keep = []
    for s, (op, operand, refill) in zip(prog.steps, steps):
        if op not in _lib.ARITH_OPCODES:
            raise ValueError("unknown arithmetic step %r (one of %s)" % (op, sorted(_lib.ARITH_OPCODES)))
        s.opcode, s.refill = _lib.ARITH_OPCODES[op], 1 if refill else 0
        if isinstance(operand, DeviceArray):
            if op in _lib.ARITH_UNARY:
                raise ValueError("step %r takes no operand" % op)
            if operand.dtype != dtype:
                raise TypeError("operand of %r must be a %s DeviceArray like the cube (got %s)" % (op, dtype, operand.dtype))
            own = None
            if len(operand.shape) == 3 and hasattr(operand, "row_stride"):
                own = (operand.plane_stride, operand.row_stride, 1)
            s.stride_z, s.stride_y, s.stride_x = arith_operand_strides(operand.shape, cube.shape, own)
            s.is_scalar, s.d_data = 0, operand.ptr
            keep.append(operand)
        else:
            if operand is None and op not in _lib.ARITH_UNARY:
                raise ValueError("step %r needs an operand" % op)
            s.is_scalar, s.scalar, s.d_data = 1, float(0.0 if operand is None else operand), None
    if out is None:
        out = DeviceArray(cube.shape, dtype, cube.device)
    elif tuple(out.shape) != tuple(cube.shape) or out.dtype != dtype:
        raise ValueError("preallocated output must be %s %s" % (tuple(cube.shape), dtype))
    else:
        _written(out)
    ors, ops_ = _strides(out)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, float(fill), C.byref(prog),
              C.c_void_p(out.ptr), ors, ops_)
    return out


def _bbox_result(box, device, stream):
    if stream is not None:
        _lib.call("spc_stream_sync", device, _sh(stream))
    b = [int(v) for v in box.get()]
    if b[0] > b[1]:
        return None
    return ((b[0], b[1]), (b[2], b[3]), (b[4], b[5]))


def mask_bbox(cube, mask=None, stream=None, nan_excluded=False):
    """bounding box of the included voxels, ((zmin, zmax), (ymin, ymax), (xmin, xmax)) with inclusive bounds, or None
    when nothing is included: ``ndimage.find_objects(include.astype(int))[0]`` of subcube_slices_from_mask
    (spectral_cube.py:1925-1938) in one pass over the mask terms."""
    box = DeviceArray((6,), np.int64, cube.device)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    _lib.call(_entry("mask_bbox", cube)[0], cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0, C.c_void_p(box.ptr))
    return _bbox_result(box, cube.device, stream)


def spectral_conv_moments(cube, kernel1d, cen, dv=1.0, m1_add=0.0, mask=None, want=_WANT_ALL,
                          stream=None, out=None, cen_host=None):
    """fused spectral_smooth -> moment (smoothed cube never written).
    cen_host: optional host copy of *cen* (lets the kernel use the linear-axis form)."""
    nz, ny, nx = cube.shape
    o, bufs = _moment_outputs((ny, nx), cube.device, want, out)
    k, kp = _kern(kernel1d)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    hc = None
    if cen_host is not None:
        cen_host = np.ascontiguousarray(cen_host, dtype=np.float64)
        hc = cen_host.ctypes.data_as(C.POINTER(C.c_double))
    ws, wsn = workspace(cube.device, stream, _lib.WS_SPECTRAL_CONV_MOMENTS, *cube.shape, len(k))
    _lib.call("spc_spectral_conv_moments_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), kp,
              len(k), C.c_void_p(cen.ptr), hc, float(dv), float(m1_add), C.byref(o), ws, wsn)
    return bufs


def separable_factors(kernel2d, rtol=1e-12):
    """Return (ky, kx) with outer(ky, kx) == kernel2d, or None."""
    k = np.asarray(kernel2d, dtype=np.float64)
    iy, ix = np.unravel_index(np.argmax(np.abs(k)), k.shape)
    piv = k[iy, ix]
    if piv == 0:
        return None
    ky = k[:, ix].copy()
    kx = k[iy, :] / piv
    if not np.allclose(np.outer(ky, kx), k, rtol=rtol, atol=rtol * abs(piv)):
        return None
    if piv > 0:
        # split the scale evenly: for a symmetric kernel (every Gaussian2DKernel with one stddev)
        # both factors then coincide, and handing the library IDENTICAL arrays lets it pick the
        # kernels that keep one set of weights in scalar registers for both passes
        s = np.sqrt(piv)
        ky, kx = ky / s, kx * s
        if ky.shape == kx.shape and np.allclose(ky, kx, rtol=rtol, atol=rtol * np.abs(ky).max()):
            kx = ky.copy()
    return ky, kx


MASKED_SPATIAL_ARITHMETIC = ("f16-split", "f32")
_SPATIAL_FORM = {"f16-split": _lib.SPATIAL_FORM_SPLIT, "f32": _lib.SPATIAL_FORM_RING}


class masked_spatial_arithmetic:
    """Scope in which the masked separable spatial stencil runs in the named arithmetic (the precision
    policy): "f16-split" (default) = every product on the fp16 matrix instruction with the samples, the taps and the x-pass
    result split hi + lo, float32 accumulation - 1e-6 of the data range against astropy's float64, inside the 1e-5 contract;
    "f32" = the ring kernels, float32 multiply-adds on the vector ALU - 2.5e-7 of the range, 1.2 - 1.5 x the time.
    A setting of the calling thread (spc_set_masked_spatial_form): it holds for the library calls this thread makes inside
    the scope, wins over SPC_SPATIAL_RING in the environment, nests, and no other thread sees it."""

    def __init__(self, name):
        if name is not None and name not in MASKED_SPATIAL_ARITHMETIC:
            raise ValueError("arithmetic must be one of %r, got %r" % (MASKED_SPATIAL_ARITHMETIC, name))
        self.name = name

    def __enter__(self):
        if self.name is not None:
            self._old = _lib.load().spc_set_masked_spatial_form(_SPATIAL_FORM[self.name])
        return self

    def __exit__(self, *exc):
        if self.name is not None:
            _lib.load().spc_set_masked_spatial_form(self._old)
        return False


def spatial_conv(cube, kernel2d, mask=None, out=None, stream=None, arithmetic=None):
    """NaN-aware per-channel 2-D convolution = chunk function of
    spatial_smooth (dask_spectral_cube.py:962-993, :540-547): an outer-product kernel in two passes, any other kernel
    summed directly; the result has the cube's dtype.  *arithmetic*: None (the library's default) or one of
    MASKED_SPATIAL_ARITHMETIC for the masked separable stencil of a float32 cube (see masked_spatial_arithmetic)."""
    wide = cube.dtype == _F64
    if arithmetic is not None and not wide:          # (the float64 stencils have one arithmetic)
        with masked_spatial_arithmetic(arithmetic):
            return spatial_conv(cube, kernel2d, mask=mask, out=out, stream=stream)
    out = _out_cube(out, cube.shape, cube.dtype, cube.device)
    k2 = np.ascontiguousarray(kernel2d, dtype=np.float64)
    if k2.ndim != 2:
        raise ValueError("kernel must be 2-D")
    c, m = _cube_c(cube), _mask_c(mask, cube)
    sep = separable_factors(k2)
    if wide:
        # float64: ONE entry point with a separable flag (the two factors, or the whole kernel and no second pointer) and one
        # workspace kind
        (ky, kyp), (kx, kxp) = (_kern(sep[0]), _kern(sep[1])) if sep is not None else (_kern(k2), (None, None))
        ws, wsn = workspace(cube.device, stream, _lib.WS_SPATIAL_CONV_F64, *cube.shape, k2.shape[0], k2.shape[1])
        _lib.call("spc_spatial_conv_f64", cube.device, _sh(stream), C.byref(c), C.byref(m), kyp, k2.shape[0], kxp, k2.shape[1],
                  0 if sep is None else 1, C.c_void_p(out.ptr), *_strides(out), ws, wsn)
    elif sep is not None:
        (ky, kyp), (kx, kxp) = _kern(sep[0]), _kern(sep[1])
        ws, wsn = workspace(cube.device, stream, _lib.WS_SPATIAL_CONV_SEP, *cube.shape, len(ky), len(kx))
        _lib.call("spc_spatial_conv_sep_f32", cube.device, _sh(stream), C.byref(c), C.byref(m),
                  kyp, len(ky), kxp, len(kx), C.c_void_p(out.ptr), *_strides(out), ws, wsn)
    else:
        k, kp = _kern(k2)
        ws, wsn = workspace(cube.device, stream, _lib.WS_SPATIAL_CONV2D, *cube.shape, k2.shape[0], k2.shape[1])
        _lib.call("spc_spatial_conv2d_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), kp,
                  k2.shape[0], k2.shape[1], C.c_void_p(out.ptr), *_strides(out), ws, wsn)
    return out


def lerp_plan(inaxis, grid, fill_value=None):
    """Host-side plan for spectral_lerp restating scipy interp1d's index
    arithmetic (dask_spectral_cube.py:1291-1353).  Returns
    (lo int32, t float64, inv_dx float64, reverse_in, reverse_out, fill)."""
    inaxis = np.asarray(inaxis, dtype=np.float64)
    grid = np.asarray(grid, dtype=np.float64)
    reverse_in = np.mean(np.diff(inaxis)) < 0
    reverse_out = np.mean(np.diff(grid)) < 0
    if reverse_in:
        inaxis = inaxis[::-1]
    if reverse_out:
        grid = grid[::-1]
    if not (np.all(np.diff(grid) > 0) and np.all(np.diff(inaxis) > 0)):
        raise AssertionError("spectral axes must be strictly monotonic")
    np.testing.assert_allclose(np.diff(grid), np.mean(np.diff(grid)),
                               err_msg="Output grid must be linear")
    idx = np.clip(np.searchsorted(inaxis, grid), 1, len(inaxis) - 1)
    lo = (idx - 1).astype(np.int32)
    t = grid - inaxis[lo]
    inv_dx = 1.0 / (inaxis[lo + 1] - inaxis[lo])
    oob = (grid < inaxis[0]) | (grid > inaxis[-1])
    lo[oob] = -1
    fill = np.nan if fill_value is None else float(fill_value)
    return lo, t, inv_dx, bool(reverse_in), bool(reverse_out), fill


def spectral_lerp(cube, lo, t, inv_dx, fill=np.nan, mask=None, out=None, stream=None):
    """per-spaxel linear interpolation onto nz_out channels (chunk function
    of spectral_interpolate, dask_spectral_cube.py:1342-1353), in the cube's dtype.  *cube* must
    already be in ascending spectral order."""
    nz_out = len(lo)
    dev = cube.device
    d_lo = DeviceArray.from_numpy(np.asarray(lo, dtype=np.int32), dev)
    d_t = DeviceArray.from_numpy(np.asarray(t, dtype=np.float64), dev)
    d_inv = DeviceArray.from_numpy(np.asarray(inv_dx, dtype=np.float64), dev)
    name, dtype = _entry("spectral_lerp", cube)
    out = _out_cube(out, (nz_out,) + tuple(cube.shape[1:]), dtype, dev)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    _lib.call(name, dev, _sh(stream), C.byref(c), C.byref(m), nz_out,
              C.c_void_p(d_lo.ptr), C.c_void_p(d_t.ptr), C.c_void_p(d_inv.ptr), float(fill),
              C.c_void_p(out.ptr), *_strides(out))
    out._plan = (d_lo, d_t, d_inv)     # keep alive until the stream has consumed them
    return out


def _wcs_struct(w):
    code, crpix, lin, inv, ap, dp, php, pv1, plane0, (sip_order, sip_a, sip_b) = w.celestial_params()
    s = _lib.SpcCelestialWcs()
    s.proj = code
    s.pv1 = pv1
    s.plane0[0], s.plane0[1] = plane0
    s.sip_order = int(sip_order)
    for i in range(len(sip_a)):
        s.sip_a[i], s.sip_b[i] = sip_a[i], sip_b[i]
    s.crpix[0], s.crpix[1] = crpix
    for i in range(4):
        s.lin[i], s.lin_inv[i] = lin[i], inv[i]
    s.alpha_p, s.delta_p, s.phi_p = ap, dp, php
    return s


def wcs_pixel_map(wcs_in, wcs_out, shape_out, device=0, stream=None):
    """(xs, ys) float64 DeviceArrays: source-grid pixel coordinates of every pixel of the target grid,
    computed on the device (spc_wcs_pixel_map_f64; the host version is wcs.reproject_pixel_map).
    Pixels that cannot be projected hold -1e30."""
    ny, nx = (int(n) for n in shape_out)
    d_xs, d_ys = DeviceArray((ny, nx), np.float64, device), DeviceArray((ny, nx), np.float64, device)
    so, si = _wcs_struct(wcs_out), _wcs_struct(wcs_in)
    # target frame -> source frame (ICRS / FK5 / Galactic; NotImplementedError for pairs that are not built; None = same)
    # (ABI 4: 15 doubles - rotation, E-terms removed before it (FK4 target), E-terms added after it (FK4 source))
    from .wcs import frame_transform
    tr = frame_transform(getattr(wcs_out, "frame", None), getattr(wcs_in, "frame", None))
    rp = None
    if tr is not None:
        remove, rot, add = tr
        vals = list(np.ascontiguousarray(rot, dtype=np.float64).ravel())
        vals += list(remove) if remove is not None else [0.0, 0.0, 0.0]
        vals += list(add) if add is not None else [0.0, 0.0, 0.0]
        rp = (C.c_double * 15)(*vals)
    _lib.call("spc_wcs_pixel_map_f64", device, _sh(stream), C.byref(so), C.byref(si), rp, ny, nx,
              C.c_void_p(d_xs.ptr), C.c_void_p(d_ys.ptr))
    return d_xs, d_ys


def _pixel_map_on_device(xs, ys, dev):
    """(d_xs, d_ys, ny_out, nx_out) of a pixel map given as float64 DeviceArrays (wcs_pixel_map: used where they are) or as
    host arrays (uploaded to *dev*)"""
    if isinstance(xs, DeviceArray) and isinstance(ys, DeviceArray):
        if xs.dtype != np.float64 or ys.dtype != np.float64 or xs.shape != ys.shape or len(xs.shape) != 2:
            raise ValueError("xs, ys must be 2-D float64 maps of identical shape")
        return (xs, ys) + tuple(xs.shape)
    xs = np.ascontiguousarray(xs, dtype=np.float64)
    ys = np.ascontiguousarray(ys, dtype=np.float64)
    if xs.shape != ys.shape or xs.ndim != 2:
        raise ValueError("xs, ys must be 2-D maps of identical shape")
    return (DeviceArray.from_numpy(xs, dev), DeviceArray.from_numpy(ys, dev)) + xs.shape


def resample_bilinear(cube, xs, ys, fill=np.nan, mask=None, stream=None, want_footprint=True, out=None,
                      order=1, any_valid=None):
    """bilinear spatial resample of every channel at (xs, ys) source pixel
    coordinates (resampler of reproject_interp, spectral_cube.py:2726-2732).  xs, ys: host arrays or
    float64 DeviceArrays (wcs_pixel_map).  order: 1 bilinear, 0 nearest neighbour.  any_valid: optional
    1-element uint32 DeviceArray, set to 1 iff some output value is not NaN.  A float64 cube: float64 weights and result."""
    dev = cube.device
    name, dtype = _entry("resample_bilinear", cube)
    d_xs, d_ys, ny_out, nx_out = _pixel_map_on_device(xs, ys, dev)
    out = _out_cube(out, (cube.shape[0], ny_out, nx_out), dtype, dev)          # (a strided view carries its strides)
    foot = DeviceArray((ny_out, nx_out), np.uint8, dev) if want_footprint else None
    c, m = _cube_c(cube), _mask_c(mask, cube)
    # (the float32 kernel alone takes a workspace)
    scratch = workspace(dev, stream, _lib.WS_RESAMPLE_BILINEAR, *cube.shape, ny_out, nx_out) if dtype == _F32 else ()
    _lib.call(name, dev, _sh(stream), C.byref(c), C.byref(m), float(fill),
              ny_out, nx_out, C.c_void_p(d_xs.ptr), C.c_void_p(d_ys.ptr), C.c_void_p(out.ptr), *_strides(out),
              C.c_void_p(foot.ptr) if foot is not None else None, int(order),
              C.c_void_p(any_valid.ptr) if any_valid is not None else None, *scratch)
    out._plan = (d_xs, d_ys)
    return out, foot


def lerp_plan_folds(lo):
    """a plan resample_bilinear_lerp accepts: monotone either way (a descending one is run reversed)"""
    lo = np.asarray(lo)
    return lerp_plan_is_foldable(lo) or lerp_plan_is_foldable(lo[::-1])


def lerp_plan_is_foldable(lo):
    """True when a spectral_lerp plan can ride in the resampling kernel (resample_bilinear_lerp): its non-negative
    entries ascend and are contiguous (an ascending grid on ascending channels)"""
    lo = np.asarray(lo)
    ok = np.nonzero(lo >= 0)[0]
    if len(ok) == 0:
        return False
    return bool(ok[-1] - ok[0] + 1 == len(ok) and np.all(np.diff(lo[ok]) >= 0))


def resample_bilinear_lerp(cube, xs, ys, lo, t, inv_dx, fill=np.nan, mask=None, stream=None, want_footprint=True, out=None,
                           order=1, any_valid=None):
    """resample_bilinear with the spectral interpolation folded in (spc_resample_bilinear_lerp_f32): output channel j is the
    linear blend (spectral_lerp's plan *lo*, *t*, *inv_dx*) of the RESAMPLED input planes lo[j], lo[j] + 1 - one read of the
    cube, one write of the result, for spectral_interpolate(...).reproject(...) (dask_spectral_cube.py:1342-1353 +
    spectral_cube.py:2700-2732) and for reproject onto a cube header with its own spectral axis.  Channels with lo < 0 are
    NaN planes.  Returns (cube of len(lo) channels, footprint)."""
    dev = cube.device
    lo = np.ascontiguousarray(lo, dtype=np.int32)
    t, inv_dx = np.asarray(t, dtype=np.float64), np.asarray(inv_dx, dtype=np.float64)
    flip = False
    if not lerp_plan_is_foldable(lo):
        # a descending plan (a reversed output grid, or a reversed input axis): the same kernel on the reversed plan, its
        # output planes written from the last one down (a negative plane stride)
        if not lerp_plan_is_foldable(lo[::-1]):
            raise _lib.HipUnsupported("resample_bilinear_lerp: the plan's channels must be monotone and contiguous (run the two passes)")
        lo, t, inv_dx, flip = lo[::-1].copy(), t[::-1].copy(), inv_dx[::-1].copy(), True
    if cube.shape[0] < 2:
        raise _lib.HipUnsupported("resample_bilinear_lerp: at least two input channels")
    d_xs, d_ys, ny_out, nx_out = _pixel_map_on_device(xs, ys, dev)
    nz_out = len(lo)
    d_lo = DeviceArray.from_numpy(lo, dev)
    d_t = DeviceArray.from_numpy(np.asarray(t, dtype=np.float64), dev)
    d_inv = DeviceArray.from_numpy(np.asarray(inv_dx, dtype=np.float64), dev)
    if out is None:
        out = DeviceArray((nz_out, ny_out, nx_out), np.float32, dev)
    elif out.shape != (nz_out, ny_out, nx_out) or out.dtype != np.float32 or getattr(out, "_is_view", False):
        raise ValueError("out must be a contiguous float32 (nz_out, ny_out, nx_out) DeviceArray")
    else:
        _written(out)
    foot = DeviceArray((ny_out, nx_out), np.uint8, dev) if want_footprint else None
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ws, wsn = workspace(dev, stream, _lib.WS_RESAMPLE_BILINEAR_LERP, *cube.shape, ny_out, nx_out)
    plane = ny_out * nx_out
    _lib.call("spc_resample_bilinear_lerp_f32", dev, _sh(stream), C.byref(c), C.byref(m), float(fill),
              ny_out, nx_out, C.c_void_p(d_xs.ptr), C.c_void_p(d_ys.ptr), nz_out, C.c_void_p(d_lo.ptr), C.c_void_p(d_t.ptr),
              C.c_void_p(d_inv.ptr), C.c_void_p(out.ptr + ((nz_out - 1) * plane * 4 if flip else 0)), nx_out, -plane if flip else plane,
              C.c_void_p(foot.ptr) if foot is not None else None, int(order),
              C.c_void_p(any_valid.ptr) if any_valid is not None else None, ws, wsn)
    out._plan = (d_xs, d_ys, d_lo, d_t, d_inv)
    return out, foot


def spatial_conv_mfma(cube, kernel2d, mask=None, stream=None, out=None, want_cube=True, want_m0=False, dv=1.0, m0=None):
    """masked separable spatial_smooth with the denominator on the matrix cores (spc_spatial_conv_sep_mfma_f32), optionally
    fused with moment 0 of the smoothed cube under the ORIGINAL mask (the cube is then never written when want_cube is
    False).  Returns (smoothed cube or None, m0 map float64 or None).  HipUnsupported: kernels of more than 29 taps per axis,
    non-separable or negative kernels, mask terms other than the array / isfinite - the caller falls back to spatial_conv
    (+ moments)."""
    k = np.asarray(kernel2d, dtype=np.float64)
    fac = separable_factors(k)
    if fac is None:
        raise _lib.HipUnsupported("spatial_conv_mfma: the kernel is not an outer product")
    ky, kx = (np.ascontiguousarray(f, dtype=np.float64) for f in fac)
    dev = cube.device
    nz, ny, nx = cube.shape
    if want_cube:
        out = _contiguous_out(out, (nz, ny, nx), np.float32, dev)
    if want_m0 and m0 is None:
        m0 = DeviceArray((ny, nx), np.float64, dev)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ws, wsn = workspace(dev, stream, _lib.WS_SPATIAL_CONV_MFMA, nz, ny, nx)
    _lib.call("spc_spatial_conv_sep_mfma_f32", dev, _sh(stream), C.byref(c), C.byref(m),
              ky.ctypes.data_as(C.POINTER(C.c_double)), len(ky), kx.ctypes.data_as(C.POINTER(C.c_double)), len(kx),
              C.c_void_p(out.ptr) if want_cube else None, 0, 0, float(dv), C.c_void_p(m0.ptr) if want_m0 else None, 0, ws, wsn)
    return (out if want_cube else None), (m0 if want_m0 else None)


def spatial_conv_mfma_moments(cube, kernel2d, d_cen, dv=1.0, m1_add=0.0, mask=None, want=("m0", "m1", "m2"), stream=None,
                              out=None, want_cube=False):
    """masked separable spatial_smooth fused with moments 0 / 1 / 2 of the smoothed cube under the ORIGINAL mask
    (spc_spatial_conv_sep_mfma_moments_f32): the smoothed cube is never written unless want_cube.  *d_cen*: DeviceArray of
    nz doubles (channel coordinates about the reference, as for moments()).  Returns (cube or None, {"m0": ..}) with
    float64 DeviceArray maps.  HipUnsupported as spatial_conv_mfma, and where the split form does not apply."""
    k = np.asarray(kernel2d, dtype=np.float64)
    fac = separable_factors(k)
    if fac is None:
        raise _lib.HipUnsupported("spatial_conv_mfma: the kernel is not an outer product")
    ky, kx = (np.ascontiguousarray(f, dtype=np.float64) for f in fac)
    dev = cube.device
    nz, ny, nx = cube.shape
    if want_cube:
        out = _contiguous_out(out, (nz, ny, nx), np.float32, dev)
    maps = {w: DeviceArray((ny, nx), np.float64, dev) for w in want}
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    higher = ("m1" in maps) or ("m2" in maps)
    ws, wsn = workspace(dev, stream, _lib.WS_SPATIAL_CONV_MFMA, nz, ny, nx, 3 if higher else 1)
    ptr = lambda w: C.c_void_p(maps[w].ptr) if w in maps else None
    _lib.call("spc_spatial_conv_sep_mfma_moments_f32", dev, _sh(stream), C.byref(c), C.byref(m),
              ky.ctypes.data_as(C.POINTER(C.c_double)), len(ky), kx.ctypes.data_as(C.POINTER(C.c_double)), len(kx),
              C.c_void_p(out.ptr) if want_cube else None, 0, 0, C.c_void_p(d_cen.ptr), float(dv), float(m1_add),
              ptr("m0"), ptr("m1"), ptr("m2"), 0, ws, wsn)
    return (out if want_cube else None), maps


def map_check(counts=None, expect=0, values=None, stream=None):
    """device-side checks of the algebraic smooth -> moment paths (spc_map_check): bit 0 = a count differs from *expect*, bit 1 = a
    value is not finite.  Returns the flags (an int; reads back four bytes)."""
    ref = counts if counts is not None else values
    n = int(np.prod(ref.shape, dtype=np.int64))
    flags = DeviceArray((1,), np.uint32, ref.device)
    _lib.call("spc_map_check", ref.device, _sh(stream), C.c_void_p(counts.ptr) if counts is not None else None, int(expect),
              C.c_void_p(values.ptr) if values is not None else None, n, C.c_void_p(flags.ptr))
    return int(flags.get(stream)[0])


def resample_spline(cube, xs, ys, order, stream=None, want_footprint=True, out=None, slab_bytes=2 << 30):
    """biquadratic (order 2) / bicubic (order 3) spatial resample of every channel at (xs, ys): scipy's
    map_coordinates(order, mode='constant', cval=nan) on the border-replicated planes, the resampler of
    reproject_interp(order='biquadratic' | 'bicubic') (spectral_cube.py:2667-2676, 2726-2732).  The cube must hold
    finite samples only (the caller checks: scipy's prefilter makes everything NaN otherwise).  The float64 spline
    coefficients of a slab of channels at a time live in a scratch buffer of at most *slab_bytes*."""
    dev = cube.device
    if order not in (2, 3):
        raise ValueError("spline order 2 or 3")
    if isinstance(xs, DeviceArray) and isinstance(ys, DeviceArray):
        d_xs, d_ys = xs, ys
        ny_out, nx_out = xs.shape
    else:
        xs = np.ascontiguousarray(xs, dtype=np.float64)
        ys = np.ascontiguousarray(ys, dtype=np.float64)
        ny_out, nx_out = xs.shape
        d_xs, d_ys = DeviceArray.from_numpy(xs, dev), DeviceArray.from_numpy(ys, dev)
    nz, ny, nx = cube.shape
    out = _contiguous_out(out, (nz, ny_out, nx_out), np.float32, dev)       # (written a slab of planes at a time, from out.ptr)
    foot = DeviceArray((ny_out, nx_out), np.uint8, dev) if want_footprint else None
    per_plane = (ny + 2) * (nx + 2) * 8
    planes = int(max(1, min(nz, slab_bytes // per_plane, 65535)))
    coef = DeviceArray((planes * per_plane,), np.uint8, dev)
    for z0 in range(0, nz, planes):
        z1 = min(nz, z0 + planes)
        c = _cube_c(cube.planes(z0, z1), _F32)
        _lib.call("spc_resample_spline_f32", dev, _sh(stream), C.byref(c), int(order), ny_out, nx_out, C.c_void_p(d_xs.ptr),
                  C.c_void_p(d_ys.ptr), C.c_void_p(out.ptr + z0 * ny_out * nx_out * 4), 0, 0,
                  C.c_void_p(foot.ptr) if (foot is not None and z0 == 0) else None, C.c_void_p(coef.ptr), C.c_size_t(coef.nbytes))
    if stream is not None:
        _lib.call("spc_stream_sync", dev, _sh(stream))
    else:
        _lib.call("spc_stream_sync", dev, None)          # `coef` goes back to the pool: the kernels must be done with it
    out._plan = (d_xs, d_ys)
    return out, foot


# ---- statistics ----------------------------------------------
STAT_KEYS = ("count", "min", "max", "sum", "sumsq")
_STAT_DTYPES = {"count": np.int32, "min": np.float32, "max": np.float32, "sum": np.float64, "sumsq": np.float64, "m2": np.float64}


def stats_global(cube, mask=None, stream=None):
    """{npts, min, max, sum, sumsq} of the included samples of the whole cube in ONE pass
    (per-chunk compute_stats + aggregation of statistics(), dask_spectral_cube.py:769-814).
    Returns python floats (min / max of a float64 cube are its float64 samples); synchronises."""
    name, dtype = _entry("stats_global", cube)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    h = (C.c_double * 5)()
    # (the float64 kernel sizes its scratch by its own kind)
    ws, wsn = workspace(cube.device, stream, _lib.WS_STATS_GLOBAL_F64 if dtype == _F64 else _lib.WS_STATS_GLOBAL, *cube.shape)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), h, ws, wsn)
    return {"npts": h[0], "min": h[1], "max": h[2], "sum": h[3], "sumsq": h[4]}


def stats_planes(cube, mask=None, stream=None):
    """{count, min, max, sum, sumsq} -> float64 arrays of length nz: the statistics of every channel's
    plane in ONE pass (nan-reductions with axis=(1, 2): spectra).  Synchronises."""
    nz = cube.shape[0]
    buf = (C.c_double * (5 * nz))()
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ws, wsn = workspace(cube.device, stream, _lib.WS_STATS_PLANES, *cube.shape)
    _lib.call("spc_stats_planes_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), buf, ws, wsn)
    a = np.frombuffer(buf, dtype=np.float64).reshape(nz, 5)
    return {"count": a[:, 0].copy(), "min": a[:, 1].copy(), "max": a[:, 2].copy(), "sum": a[:, 3].copy(), "sumsq": a[:, 4].copy()}


def stats_axis(cube, axis, mask=None, want=STAT_KEYS, stream=None, out=None):
    """count / min / max / sum / sumsq maps along *axis* in ONE pass (the nan-reductions behind
    sum / mean / std / max / min, dask_spectral_cube.py:641-767).  Returns DeviceArrays
    (*out*: dict of preallocated ones, reused); min / max have the cube's dtype.

    ``"m2"`` in *want* (not one of the five of the single pass): sum (x - mean)^2 of every ray about its OWN mean, from a
    second read of the cube (csrc/spc_stats_m2.hip) - what std is made of: sumsq / n - mean^2 is lost on a pedestal.
    Comes with count and sum, which it is computed from."""
    if axis not in (0, 1, 2):
        raise ValueError("axis must be 0, 1 or 2")
    name, dtype = _entry("stats_axis", cube)
    types = dict(_STAT_DTYPES, min=dtype, max=dtype)
    shp = tuple(n for i, n in enumerate(cube.shape) if i != axis)
    res = {}
    m2 = "m2" in want
    want = tuple(k for k in want if k != "m2") + (tuple(k for k in ("count", "sum") if k not in want) if m2 else ())
    for k in want + (("m2",) if m2 else ()):
        a = out.get(k) if out else None
        if a is None:
            a = DeviceArray(shp, types[k], cube.device)
        elif tuple(a.shape) != shp or a.dtype != types[k]:
            raise ValueError("out[%r] must be %s %s" % (k, shp, types[k]))
        else:
            _written(a)
        res[k] = a
    o = _lib.SpcStatsOutputs()
    for k in want:
        setattr(o, "d_" + k, res[k].ptr)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), int(axis), C.byref(o))
    if m2:
        _lib.call(_entry("stats_m2_axis", cube)[0], cube.device, _sh(stream), C.byref(c), C.byref(m), int(axis),
                  C.c_void_p(res["count"].ptr), C.c_void_p(res["sum"].ptr), C.c_void_p(res["m2"].ptr))
    return res


def stats_dev_axis(cube, axis, center, mask=None, stream=None):
    """(s1, s2) DeviceArrays: sum (x - center) and sum (x - center)^2 of every ray along *axis* about ONE number - the second
    pass of the whole cube's std, whose mean stats_global gave (csrc/spc_stats_m2.hip)"""
    if axis not in (0, 1, 2):
        raise ValueError("axis must be 0, 1 or 2")
    shp = tuple(n for i, n in enumerate(cube.shape) if i != axis)
    s1, s2 = DeviceArray(shp, np.float64, cube.device), DeviceArray(shp, np.float64, cube.device)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    _lib.call(_entry("stats_dev_axis", cube)[0], cube.device, _sh(stream), C.byref(c), C.byref(m), int(axis), float(center),
              C.c_void_p(s1.ptr), C.c_void_p(s2.ptr))
    return s1, s2


def map_conv2d(dmap, kernel2d, stream=None, out=None):
    """zero-filled, sum-normalised 2-D convolution of one float64 (ny, nx) DeviceArray (the map
    form of spatial_smooth used by the algebraic smooth -> moment path)."""
    if dmap.dtype != np.float64 or len(dmap.shape) != 2:
        raise TypeError("map must be a 2-D float64 DeviceArray")
    k = np.ascontiguousarray(kernel2d, dtype=np.float64)
    if k.ndim != 2:
        raise ValueError("kernel must be 2-D")
    if out is None:
        out = DeviceArray(dmap.shape, np.float64, dmap.device)
    else:
        _written(out)
    ws, wsn = workspace(dmap.device, stream, _lib.WS_MAP_CONV2D, 1, dmap.shape[0], dmap.shape[1], k.shape[0], k.shape[1])
    _lib.call("spc_map_conv2d_f64", dmap.device, _sh(stream), C.c_void_p(dmap.ptr), dmap.shape[0], dmap.shape[1],
              k.ctypes.data_as(C.POINTER(C.c_double)), k.shape[0], k.shape[1], C.c_void_p(out.ptr), ws, wsn)
    return out


def map_arith(op, a, b, c=None, s=0.0, out=None, stream=None):
    """elementwise arithmetic on float64 maps (spc_map_arith_f64; op one of _lib.MAP_*): the algebra around
    map_conv2d without a trip to the host."""
    for m in (a, b, c):
        if m is not None and (m.dtype != np.float64 or tuple(m.shape) != tuple(a.shape)):
            raise TypeError("maps must be float64 DeviceArrays of one shape")
    if out is None:
        out = DeviceArray(a.shape, np.float64, a.device)
    else:
        _written(out)
    _lib.call("spc_map_arith_f64", a.device, _sh(stream), int(op), C.c_void_p(a.ptr), C.c_void_p(b.ptr),
              C.c_void_p(c.ptr) if c is not None else None, float(s), C.c_void_p(out.ptr), int(np.prod(a.shape, dtype=np.int64)))
    return out


MAD_TO_STD = 1.482602218505602          # 1 / Phi^-1(3/4), astropy.stats.mad_std


def percentile_axis0(cube, q, mask=None, center=None, scale=1.0, stream=None, out=None):
    """q-th percentile along the spectral axis per spaxel (median: q = 50), numpy 'linear'
    interpolation, NaN / masked samples ignored (dask_spectral_cube.py:657-693); with *center*
    (a (ny, nx) DeviceArray of the cube's dtype) of |x - center| times *scale* (mad_std, :711-731).  The map has the
    cube's dtype.  Selection along y: pass ``cube.swap01()`` (and ``mask.swap01()``); the result is (nz, nx).
    A float64 cube: HipUnsupported beyond 4096 samples per ray."""
    name, dtype = _entry("percentile_axis0", cube)
    if out is None:
        out = DeviceArray(cube.shape[1:], dtype, cube.device)
    else:
        _written(out)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    if center is not None and (center.dtype != dtype or tuple(center.shape) != tuple(cube.shape[1:])):
        raise TypeError("center must be a %s (ny, nx) DeviceArray" % dtype)
    _lib.call(name, cube.device, _sh(stream), C.byref(c), C.byref(m), float(q),
              C.c_void_p(center.ptr) if center is not None else None, float(scale), C.c_void_p(out.ptr))
    return out


def fill_masked(cube, mask=None, fill=np.nan, stream=None, out=None):
    """device copy with excluded voxels replaced by *fill* (MaskBase._filled, masks.py:197-237)."""
    out = _out_cube(out, cube.shape, np.float32, cube.device)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    _lib.call("spc_fill_masked_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), float(fill), C.c_void_p(out.ptr), *_strides(out))
    return out


def mask_include(cube, mask=None, nan_excluded=False, stream=None):
    """uint8 (nz, ny, nx) DeviceArray: 1 where *mask* (a MaskSpec evaluated on *cube*'s values) includes
    the voxel (spc_mask_include_u8 / _f64: the one pair named irregularly) - a lazy mask bound to another device-resident cube is lowered
    like this instead of through a host copy of that cube."""
    out = DeviceArray(cube.shape, np.uint8, cube.device)
    c, m = _cube_c(cube), _mask_c(mask, cube)
    _lib.call(_entry("mask_include", cube, "_u8")[0], cube.device, _sh(stream), C.byref(c), C.byref(m), 1 if nan_excluded else 0,
              C.c_void_p(out.ptr))
    return out


_ELEM = {np.dtype(np.float32): _lib.ELEM_F32, np.dtype(np.float64): _lib.ELEM_F64, np.dtype(np.uint8): _lib.ELEM_U8,
         np.dtype(bool): _lib.ELEM_U8}


def mask_eval(program, shape, device, dtype, out=None, stream=None):
    """uint8 (nz, ny, nx) DeviceArray: 1 where the mask tree compiled into *program* (masks.compile_mask, with the
    DeviceArrays of sample type *dtype* as its slots) includes the voxel - CompositeMask / InvertedMask over comparison,
    isfinite and boolean-array terms (masks.py:239-250, 399-455, 670-758) in one pass over the cubes it names
    (spc_mask_eval_f32 / _f64).  Host operands are uploaded un-broadcast; they stay alive with the result.  *out* may be
    a strided view of a larger array."""
    shape = tuple(int(n) for n in shape)
    name, dtype = _entry("mask_eval", np.empty(0, dtype=np.dtype(dtype)))
    if np.dtype(dtype) not in (_F32, _F64) or len(shape) != 3:
        raise TypeError("mask_eval runs on float32 or float64 cubes of shape (nz, ny, nx)")
    if (len(program.slots) > _lib.MASK_PROG_MAX_SLOTS or len(program.operands) > _lib.MASK_PROG_MAX_OPERANDS
            or len(program.instr) > _lib.MASK_PROG_MAX_INSTR):
        raise ValueError("mask program beyond the limits of spc_mask_program (%d slots, %d operands, %d instructions)"
                         % (_lib.MASK_PROG_MAX_SLOTS, _lib.MASK_PROG_MAX_OPERANDS, _lib.MASK_PROG_MAX_INSTR))
    p = _lib.SpcMaskProgram()
    p.n_slots, p.n_operands, p.n_instr = len(program.slots), len(program.operands), len(program.instr)
    for i, s in enumerate(program.slots):
        if s.dtype != dtype or tuple(s.shape) != shape:
            raise TypeError("data slot %d must be a %s DeviceArray of shape %s" % (i, np.dtype(dtype).name, shape))
        p.slots[i].d_data = s.ptr
        p.slots[i].row_stride, p.slots[i].plane_stride = _strides(s)
    held = []
    for i, (a, strides) in enumerate(program.operands):
        if not isinstance(a, DeviceArray):
            a = DeviceArray.from_numpy(a, device, stream)
        if a.dtype not in _ELEM:
            raise TypeError("operand %d: float32, float64 or uint8 elements, not %s" % (i, a.dtype))
        held.append(a)
        o = p.operands[i]
        o.d_data, o.elem = a.ptr, _ELEM[a.dtype]
        o.stride_z, o.stride_y, o.stride_x = (int(v) for v in strides)
    for i, (opcode, slot, cmp_, operand, imm) in enumerate(program.instr):
        q = p.instr[i]
        q.opcode, q.slot, q.cmp, q.operand, q.imm = int(opcode), int(slot), int(cmp_), int(operand), float(imm)
    if out is None:
        out = DeviceArray(shape, np.uint8, device)
    elif tuple(out.shape) != shape or out.dtype != np.uint8:
        raise ValueError("preallocated output must be %s uint8" % (shape,))
    ors, ops_ = _strides(out)
    _lib.call(name, device, _sh(stream), shape[0], shape[1], shape[2], C.byref(p), C.c_void_p(out.ptr), ors, ops_)
    _written(out)
    out._mask_operands = held       # the kernel may still be queued: the operands live as long as the result
    return out


def mask_morph(inp, offsets, op, iterations=1, mask=None, border_value=0, out=None, stream=None, workspace=None,
               return_iterations=False):
    """uint8 (nz, ny, nx) DeviceArray: the include array *inp* (uint8 / bool, any non-zero byte True; a rows() / planes()
    view is read where it is) eroded (*op* = _lib.MORPH_ERODE) or dilated (_lib.MORPH_DILATE) with the structuring element
    whose True entries sit at the (n, 3) integer *offsets* (dz, dy, dx) = index - size // 2, each within
    +-_lib.MORPH_MAX_REACH (spc_mask_morph_u8: scipy.ndimage.binary_erosion / binary_dilation / binary_propagation, which
    users of the reference run on the host on get_mask_array(), spectral_cube.py:552).  *iterations* >= 1: that many
    steps; < 1: until a step changes nothing.  *mask*: a uint8 array of *inp*'s shape, voxels outside it keep their
    value at every step.  *border_value*: the samples outside the array.  *out*: a contiguous uint8 array that is neither
    input; *workspace*: a uint8 DeviceArray of spc_mask_morph_workspace_bytes bytes (the stream's pooled scratch
    otherwise).  Only the change words of a repetition to the fixed point (a few bytes per batch of sweeps) come back to
    the host, inside the call.  *return_iterations*: (result, steps or sweeps run)."""
    if inp.dtype.itemsize != 1 or inp.dtype.kind not in "ub" or len(inp.shape) != 3:
        raise TypeError("mask_morph runs on a uint8 / bool DeviceArray of shape (nz, ny, nx)")
    shape = tuple(int(n) for n in inp.shape)
    if mask is not None and (tuple(mask.shape) != shape or mask.dtype.itemsize != 1 or mask.dtype.kind not in "ub"):
        raise ValueError("mask must be a uint8 / bool array of the input's shape %s (got %s %s)" % (shape, tuple(mask.shape), mask.dtype))
    if op not in (_lib.MORPH_ERODE, _lib.MORPH_DILATE):
        raise ValueError("op must be _lib.MORPH_ERODE or _lib.MORPH_DILATE (got %r)" % (op,))
    offs = np.asarray(offsets)
    if offs.ndim != 2 or offs.shape[1] != 3 or not 1 <= offs.shape[0] <= _lib.MORPH_MAX_OFFSETS:
        raise ValueError("offsets must be 1 to %d rows of (dz, dy, dx) (got shape %s)" % (_lib.MORPH_MAX_OFFSETS, offs.shape))
    if np.abs(offs).max() > _lib.MORPH_MAX_REACH:
        raise ValueError("offsets reach beyond +-%d" % _lib.MORPH_MAX_REACH)
    offs = np.ascontiguousarray(offs, dtype=np.int8)
    out = _contiguous_out(out, shape, np.uint8, inp.device)           # (the entry writes a compact array)
    ws, wsn = _scratch(int(_lib.load().spc_mask_morph_workspace_bytes(*shape)), workspace, inp.device, stream)
    run = C.c_int64(0)
    mrs, mps = _strides(mask) if mask is not None else (0, 0)
    _lib.call("spc_mask_morph_u8", inp.device, _sh(stream), shape[0], shape[1], shape[2], C.c_void_p(inp.ptr), *_strides(inp),
              C.c_void_p(mask.ptr) if mask is not None else None, mrs, mps, int(op), offs.ctypes.data_as(C.c_void_p),
              int(offs.shape[0]), int(iterations), int(border_value), C.c_void_p(out.ptr), ws, wsn, C.byref(run))
    _written(out)
    return (out, run.value) if return_iterations else out


def _scratch(need, workspace, device, stream):
    """(c_void_p, nbytes) of *workspace* (a uint8 DeviceArray of at least *need* bytes) or of the stream's pooled scratch"""
    if workspace is not None:
        if workspace.nbytes < need:
            raise ValueError("workspace of %d bytes given, %d needed" % (workspace.nbytes, need))
        return C.c_void_p(workspace.ptr), workspace.nbytes
    return _pooled_scratch(device, stream, need)


def _label_map(labels, nlabels):
    """(shape, nlabels) of an int32 label array of shape (nz, ny, nx) with labels 0 ... *nlabels*"""
    if labels.dtype != np.int32 or len(labels.shape) != 3:
        raise TypeError("labels must be an int32 DeviceArray of shape (nz, ny, nx)")
    if getattr(labels, "_is_view", False):
        raise ValueError("labels must be a contiguous array, not a strided view")
    nlabels = int(nlabels)
    if not 0 <= nlabels <= _lib.LABEL_MAX_VOXELS:
        raise ValueError("nlabels must be 0 to 2**31 - 1 (got %d)" % nlabels)
    return tuple(int(n) for n in labels.shape), nlabels


def label_structure(structure):
    """27 uint8: the (3, 3, 3) *structure* as spc_label_u8 takes it, checked as scipy.ndimage.label checks it"""
    s = np.asarray(structure)
    if s.shape != (3, 3, 3):
        raise ValueError("structure must have shape (3, 3, 3) (got %s)" % (s.shape,))
    s = np.ascontiguousarray(s != 0, dtype=np.uint8).ravel()
    if not np.array_equal(s, s[::-1]):
        raise ValueError("structure must be centrosymmetric: entry o and entry -o of every offset o agree (scipy.ndimage.label "
                         "refuses any other)")
    return s


def label(inp, structure, out=None, stream=None, workspace=None):
    """(int32 (nz, ny, nx) DeviceArray, n): the connected components of the include array *inp* (uint8 / bool, any non-zero
    byte True; a rows() / planes() view is read where it is) under the centrosymmetric (3, 3, 3) *structure*, whose centre
    is ignored - scipy.ndimage.label(inp != 0, structure), numbering included (spc_label_u8).  At most 2**31 - 1 voxels.
    *out*: a contiguous int32 array that is not the input; *workspace*: a uint8 DeviceArray of spc_label_workspace_bytes
    bytes (the stream's pooled scratch otherwise).  Only n (8 bytes) comes back to the host, inside the call."""
    if inp.dtype.itemsize != 1 or inp.dtype.kind not in "ub" or len(inp.shape) != 3:
        raise TypeError("label runs on a uint8 / bool DeviceArray of shape (nz, ny, nx)")
    shape = tuple(int(n) for n in inp.shape)
    s = label_structure(structure)
    if shape[0] * shape[1] * shape[2] > _lib.LABEL_MAX_VOXELS:
        raise NotImplementedError("%s voxels: linear indices are int32, at most 2**31 - 1 voxels are labelled" % (shape,))
    out = _contiguous_out(out, shape, np.int32, inp.device)
    ws, wsn = _scratch(int(_lib.load().spc_label_workspace_bytes(*shape)), workspace, inp.device, stream)
    n = C.c_int64(0)
    _lib.call("spc_label_u8", inp.device, _sh(stream), shape[0], shape[1], shape[2], C.c_void_p(inp.ptr), *_strides(inp),
              s.ctypes.data_as(C.c_void_p), C.c_void_p(out.ptr), ws, wsn, C.byref(n))
    return out, n.value


def label_objects(labels, nlabels, out=None, stream=None, workspace=None):
    """(sizes, bbox): int64 (nlabels + 1,) and int32 (nlabels + 1, 6) DeviceArrays of the int32 label array *labels* with
    labels 0 ... *nlabels* - sizes[k] = the voxels with label k (entry 0: the background), bbox[k] = zlo, zhi, ylo, yhi,
    xlo, xhi with hi exclusive, the slices of scipy.ndimage.find_objects (spc_label_objects_i32).  A label outside
    0 ... nlabels raises ValueError; nothing is written past the tables.  *out*: {"sizes": ..., "bbox": ...}."""
    shape, nlabels = _label_map(labels, nlabels)
    sizes = _given(out, "sizes", (nlabels + 1,), np.int64, labels.device)
    bbox = _given(out, "bbox", (nlabels + 1, 6), np.int32, labels.device)
    ws, wsn = _scratch(_lib.LABEL_OBJECTS_WORKSPACE_BYTES, workspace, labels.device, stream)
    _lib.call("spc_label_objects_i32", labels.device, _sh(stream), shape[0], shape[1], shape[2], C.c_void_p(labels.ptr), nlabels,
              C.c_void_p(sizes.ptr), C.c_void_p(bbox.ptr), ws, wsn)
    return sizes, bbox


def label_select(labels, nlabels, keep, out=None, stream=None):
    """uint8 (nz, ny, nx) DeviceArray: 1 where *keep*[labels] is non-zero - *keep*: a uint8 / bool table of *nlabels* + 1
    entries, a DeviceArray or a host array that is uploaded (spc_label_select_i32).  *out*: a contiguous uint8 array."""
    shape, nlabels = _label_map(labels, nlabels)
    if not isinstance(keep, DeviceArray):
        keep = np.ascontiguousarray(keep)
        if keep.dtype.kind not in "ub" or keep.dtype.itemsize != 1:
            raise TypeError("keep must be a uint8 / bool table (got %s)" % keep.dtype)
        if keep.shape != (nlabels + 1,):
            raise ValueError("keep must have nlabels + 1 = %d entries (got shape %s)" % (nlabels + 1, keep.shape))
        keep = DeviceArray.from_numpy(keep.view(np.uint8), labels.device, stream)
    elif keep.dtype.itemsize != 1 or keep.dtype.kind not in "ub" or tuple(keep.shape) != (nlabels + 1,):
        raise ValueError("keep must be a uint8 / bool table of nlabels + 1 = %d entries (got %s %s)"
                         % (nlabels + 1, tuple(keep.shape), keep.dtype))
    out = _contiguous_out(out, shape, np.uint8, labels.device)
    _lib.call("spc_label_select_i32", labels.device, _sh(stream), shape[0], shape[1], shape[2], C.c_void_p(labels.ptr), nlabels,
              C.c_void_p(keep.ptr), C.c_void_p(out.ptr))
    _written(out)
    out._keep_table = keep          # the kernel may still be queued: the table lives as long as the result
    return out


MEASURE_GROUPS = {"sums": _lib.MEASURE_SUMS, "extrema": _lib.MEASURE_EXTREMA, "first": _lib.MEASURE_FIRST,
                  "second": _lib.MEASURE_SECOND}
# table -> (its group, the columns after the label axis, dtype; None: the cube's)
_MEASURE_TABLES = {"count": ("sums", (), np.int64), "sums": ("sums", (2,), np.float64),
                   "min": ("extrema", (), None), "max": ("extrema", (), None),
                   "min_pos": ("extrema", (), np.int64), "max_pos": ("extrema", (), np.int64),
                   "first": ("first", (4,), np.float64), "second": ("second", (6,), np.float64)}


def label_measure(data, labels, nlabels, mask_spec=None, origin=None, want=("sums", "extrema", "first"), out=None, stream=None,
                  workspace=None):
    """{table: DeviceArray} of nlabels + 1 rows each (row 0: the background, never measured): the float32 / float64 cube
    *data* (a strided view is read in place) measured through the int32 label array *labels* with labels 0 ... *nlabels*
    (spc_label_measure_f32 / _f64: the sums behind scipy.ndimage.sum_labels, mean, variance, minimum, maximum, their
    positions and center_of_mass).  A voxel counts when its label is above 0, *mask_spec* (the cube's MaskSpec; None: no mask)
    includes it and its sample is not NaN.  *origin*: (nlabels + 1, 4) float64, v0, z0, y0, x0 of every label, a DeviceArray or a host array that is
    uploaded; None: all zero.  *want*: the groups of tables, each computed only when asked for -
    "sums": count (int64), sums (n + 1, 2) = sum (v - v0), sum (v - v0)^2;
    "extrema": min, max (the cube's dtype), min_pos, max_pos (int64 linear C-order index of the FIRST extreme; NaN and -1
    for a label with nothing measured);
    "first": first (n + 1, 4) = sum v, sum v (z - z0), sum v (y - y0), sum v (x - x0);
    "second": second (n + 1, 6) = sum v dz^2, v dy^2, v dx^2, v dz dy, v dz dx, v dy dx.
    All sums are float64; their atomic order is not fixed, so they are reproducible to float64 rounding only.  A label
    outside 0 ... nlabels raises ValueError.  *out*: {table: preallocated DeviceArray}; *workspace*: a uint8 DeviceArray of
    spc_label_measure_workspace_bytes bytes (the stream's pooled scratch otherwise).  Tables and workspace may hold
    anything.  Only the status reaches the host, inside the call."""
    shape, nlabels = _label_map(labels, nlabels)
    name, dtype = _entry("label_measure", data)
    c = _cube_c(data)
    if tuple(int(n) for n in data.shape) != shape:
        raise ValueError("labels %s and the cube %s must have one shape" % (shape, tuple(data.shape)))
    if isinstance(want, str):
        want = (want,)
    unknown = [g for g in want if g not in MEASURE_GROUPS]
    if unknown or not want:
        raise ValueError("want must name at least one of %s (got %r)" % (sorted(MEASURE_GROUPS), tuple(want)))
    bits = 0
    for g in want:
        bits |= MEASURE_GROUPS[g]
    m = _mask_c(mask_spec, data)
    nt = nlabels + 1
    if origin is not None and not isinstance(origin, DeviceArray):
        origin = np.ascontiguousarray(origin, dtype=np.float64)
        if origin.shape != (nt, 4):
            raise ValueError("origin must have shape (nlabels + 1, 4) = (%d, 4) (got %s)" % (nt, origin.shape))
        origin = DeviceArray.from_numpy(origin, labels.device, stream)
    elif origin is not None and (tuple(origin.shape) != (nt, 4) or origin.dtype != _F64):
        raise ValueError("origin must be a float64 table of shape (%d, 4) (got %s %s)" % (nt, tuple(origin.shape), origin.dtype))
    res = {}
    o = _lib.SpcLabelMeasureOutputs()
    for table, (group, cols, dt) in _MEASURE_TABLES.items():
        if group in want:
            res[table] = _given(out, table, (nt,) + cols, dtype if dt is None else dt, labels.device)
            setattr(o, "d_" + table, res[table].ptr)
    ws, wsn = _scratch(int(_lib.load().spc_label_measure_workspace_bytes(nlabels, bits)), workspace, labels.device, stream)
    _lib.call(name, labels.device, _sh(stream), C.byref(c), C.byref(m), C.c_void_p(labels.ptr), nlabels,
              C.c_void_p(origin.ptr) if origin is not None else None, bits, C.byref(o), ws, wsn)
    return res


def percentile_axis2(cube, q, mask=None, center=None, scale=1.0, stream=None, out=None):
    """q-th percentile along x per (z, y) row, no transposed copy (spc_percentile_axis2_f32); *center*: a (nz, ny)
    float32 DeviceArray.  Raises HipUnsupported for rows of more than 4096 samples."""
    nz, ny, nx = cube.shape
    if out is None:
        out = DeviceArray((nz, ny), np.float32, cube.device)
    else:
        _written(out)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    if center is not None and (center.dtype != np.float32 or tuple(center.shape) != (nz, ny)):
        raise TypeError("center must be a float32 (nz, ny) DeviceArray")
    _lib.call("spc_percentile_axis2_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), float(q),
              C.c_void_p(center.ptr) if center is not None else None, float(scale), C.c_void_p(out.ptr))
    return out


def percentile_global(cube, q, mask=None, center=None, stream=None, keep=None, scale=1.0, out=None):
    """q-th percentile of all included samples of the cube (np.nanpercentile(..., axis=None));
    with *center* of |x - center|.  Returns a python float (NaN when nothing is included).

    *keep* = 0 | 1: the same selection over the two OTHER axes, one result per index of the kept axis
    (spc_percentile_groups_f32; spectral_cube.py:730-764, 1172-1257 with a two-axis tuple): per plane z (axis=(1, 2)) or per
    row index y (axis=(0, 2)).  *center* is then a float32 DeviceArray of one centre per group (or None), the result -
    multiplied by *scale* - a float32 DeviceArray of (ngroups,), *out* when given.  Nothing comes back to the host and
    nothing waits: the result of one call may be the centre of the next (mad_std)."""
    if keep is not None:
        return _percentile_groups(cube, q, mask, center, stream, keep, scale, out)
    if scale != 1.0 or out is not None:
        raise ValueError("scale= and out= go with keep=0 | 1: the whole-cube statistic comes back as a python float")
    out = C.c_double(0.0)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ws, wsn = workspace(cube.device, stream, _lib.WS_PERCENTILE_GLOBAL, *cube.shape)
    _lib.call("spc_percentile_global_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), float(q),
              0 if center is None else 1, 0.0 if center is None else float(center), C.byref(out), ws, wsn)
    return out.value


def _percentile_groups(cube, q, mask, center, stream, keep, scale, out):
    """percentile_global's keep=0 | 1 mode"""
    if keep not in (0, 1):
        raise ValueError("keep must be None (the whole cube), 0 (one result per plane) or 1 (one per row index)")
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ngroups = int(cube.shape[keep])
    if center is not None and (not isinstance(center, DeviceArray) or center.dtype != np.float32 or tuple(center.shape) != (ngroups,)):
        raise TypeError("center must be a float32 (%d,) DeviceArray: one centre per group" % ngroups)
    if out is None:
        out = DeviceArray((ngroups,), np.float32, cube.device)
    elif tuple(out.shape) != (ngroups,) or out.dtype != np.float32:
        raise ValueError("preallocated output must be (%d,) float32" % ngroups)
    else:
        _written(out)
    ws, wsn = _pooled_scratch(cube.device, stream, int(_lib.load().spc_percentile_groups_workspace_bytes(ngroups)))
    _lib.call("spc_percentile_groups_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), int(keep), float(q),
              C.c_void_p(center.ptr) if center is not None else None, float(scale), C.c_void_p(out.ptr), ws, wsn)
    out._group_center = center       # the kernels may still be queued: the centre lives as long as the result
    return out


def key_histogram(cube, prefix, pmask, shift, mask=None, center=None, stream=None):
    """One pass of the whole-cube selection on THIS rank's part of a cube (spc_key_histogram_f32): the 256 counters
    of the key byte at bit *shift* among the included samples whose key agrees with *prefix* on *pmask*.
    Returns a uint64 ndarray of 256."""
    h = np.zeros(256, np.uint64)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ws, wsn = workspace(cube.device, stream, _lib.WS_PERCENTILE_GLOBAL, *cube.shape)
    _lib.call("spc_key_histogram_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), int(prefix), int(pmask), int(shift),
              0 if center is None else 1, 0.0 if center is None else float(center),
              h.ctypes.data_as(C.POINTER(C.c_uint64)), None, ws, wsn)
    return h


def key_next(cube, prefix, mask=None, center=None, stream=None):
    """smallest sample key above *prefix* on this rank's part (0xffffffff when there is none)."""
    nxt = C.c_uint32(0)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    ws, wsn = workspace(cube.device, stream, _lib.WS_PERCENTILE_GLOBAL, *cube.shape)
    _lib.call("spc_key_histogram_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), int(prefix), 0xffffffff, 0,
              0 if center is None else 1, 0.0 if center is None else float(center), None, C.byref(nxt), ws, wsn)
    return nxt.value


def key_to_float(key):
    """the float32 sample an order-preserving key stands for (spc_key_to_f32)."""
    return float(_lib.load().spc_key_to_f32(C.c_uint32(int(key))))


def fill_masked_transposed(cube, mask=None, fill=np.nan, stream=None):
    """(nz, nx, ny) device copy: excluded voxels replaced by *fill*, spatial axes exchanged
    (spc_fill_masked_transpose_f32) - rays along x become rays along y."""
    nz, ny, nx = cube.shape
    out = DeviceArray((nz, nx, ny), np.float32, cube.device)
    c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
    _lib.call("spc_fill_masked_transpose_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), float(fill), C.c_void_p(out.ptr))
    return out


def sigma_clip_axis0(cube, sigma=3.0, sigma_lower=None, sigma_upper=None, maxiters=5, cenfunc="median",
                     stdfunc="std", mask=None, stream=None):
    """astropy.stats.sigma_clip(axis=0, masked=False, copy=True) on the device
    (DaskSpectralCubeMixin.sigma_clip_spectrally, dask_spectral_cube.py:851-878): returns a new
    float32 DeviceArray with masked and clipped samples set to NaN.  Every iteration is one
    selection (median), one statistics pass (std) and one clip pass; it stops when a pass clips
    nothing or after *maxiters* (None: until convergence)."""
    lo_s = sigma if sigma_lower is None else sigma_lower
    hi_s = sigma if sigma_upper is None else sigma_upper
    if cenfunc not in ("median", "mean") or stdfunc not in ("std", "mad_std"):
        raise NotImplementedError("cenfunc must be 'median' or 'mean', stdfunc 'std' or 'mad_std' on the device path")
    # the whole loop in one kernel, rays resident in registers (<= 4096 channels)
    if cube.shape[0] <= 4096 and os.environ.get("SPC_SIGMA_CLIP_FUSED", "1") != "0":
        out = DeviceArray(cube.shape, np.float32, cube.device)
        c, m = _cube_c(cube, _F32), _mask_c(mask, cube)
        ws, wsn = workspace(cube.device, stream, _lib.WS_SIGMA_CLIP, *cube.shape)
        try:
            _lib.call("spc_sigma_clip_axis0_f32", cube.device, _sh(stream), C.byref(c), C.byref(m), float(lo_s), float(hi_s),
                      -1 if maxiters is None else int(maxiters), 1 if cenfunc == "mean" else 0, 1 if stdfunc == "mad_std" else 0,
                      C.c_void_p(out.ptr), ws, wsn)
            return out
        except _lib.HipUnsupported:
            del out                    # planes beyond what the register-resident kernel addresses: the loop of kernels below
    work = fill_masked(cube, mask, np.nan, stream)
    nz, ny, nx = work.shape
    dev = work.device
    d_lo, d_hi = DeviceArray((ny, nx), np.float32, dev), DeviceArray((ny, nx), np.float32, dev)
    need_stats = cenfunc == "mean" or stdfunc == "std"
    st = None
    it = 0
    while maxiters is None or it < maxiters:
        it += 1
        if need_stats:
            st = stats_axis(work, 0, want=("count", "sum", "sumsq"), stream=stream, out=st)
        med = percentile_axis0(work, 50.0, stream=stream) if (cenfunc == "median" or stdfunc == "mad_std") else None
        spread = percentile_axis0(work, 50.0, center=med, scale=MAD_TO_STD, stream=stream) if stdfunc == "mad_std" else None
        center = med if cenfunc == "median" else None
        if center is None and spread is not None:          # mean centre with a mad_std spread: the mean map itself
            n = st["count"].get().astype(np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                center = DeviceArray.from_numpy(np.where(n > 0, st["sum"].get() / n, np.nan).astype(np.float32), dev)
        ptr = lambda a: C.c_void_p(a.ptr) if a is not None else None  # noqa: E731
        use_stats = need_stats and (center is None or spread is None)
        _lib.call("spc_clip_bounds_f32", dev, _sh(stream), ny * nx,
                  ptr(st["count"]) if use_stats else None, ptr(st["sum"]) if use_stats else None,
                  ptr(st["sumsq"]) if use_stats else None, ptr(center), ptr(spread), float(lo_s), float(hi_s),
                  C.c_void_p(d_lo.ptr), C.c_void_p(d_hi.ptr))
        nch = C.c_uint64(0)
        ws, wsn = workspace(dev, stream, _lib.WS_CLIP_OUTSIDE, nz, ny, nx)
        _lib.call("spc_clip_outside_f32", dev, _sh(stream), C.c_void_p(work.ptr), nz, ny, nx,
                  C.c_void_p(d_lo.ptr), C.c_void_p(d_hi.ptr), C.byref(nch), ws, wsn)
        if nch.value == 0:
            break
    return work


def scale_inplace(arr, factor, stream=None):
    """arr *= factor on the device (contiguous float32 or float64 DeviceArray)."""
    if arr.dtype not in (_F32, _F64) or getattr(arr, "_is_view", False):
        raise TypeError("scale_inplace needs a contiguous float32 or float64 DeviceArray")
    _written(arr)
    _lib.call(_entry("scale", arr)[0], arr.device, _sh(stream), C.c_void_p(arr.ptr), int(np.prod(arr.shape, dtype=np.int64)), float(factor))
    return arr


# ---- names bench.py still calls: each pair was folded into the function it now names (the dtype comes from the cube)
percentile_axis0_f64 = percentile_axis0
spatial_conv_f64 = spatial_conv
spectral_conv_f64 = spectral_conv
spectral_lerp_f64 = spectral_lerp
stats_global_f64 = stats_global
