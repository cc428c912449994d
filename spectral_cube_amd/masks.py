"""Host-side mask algebra mirroring spectral_cube/masks.py, plus the lowering
of a mask tree to the device-evaluable :class:`~spectral_cube_amd.ops.MaskSpec`.

Semantics restated from the reference:
  * ``include`` / ``exclude`` (masks.py:105-138);
  * ``_filled``: ``where(include, data.astype(result_type(dtype, 0.0)), fill)``
    (masks.py:197-237);
  * ``&`` ``|`` ``^`` ``~`` composition (masks.py:239-250, 399-455);
  * BooleanArrayMask (masks.py:457-584), LazyMask (:586-668),
    LazyComparisonMask (:670-758), FunctionMask (:760-803).
A tree that is not an AND of device terms is compiled into a postfix program
(:func:`compile_mask`) that the device evaluates once (ops.mask_eval); only
what has no device form is evaluated here, by numpy (:func:`lower_mask`).
WCS consistency checks between mask and cube are not reproduced (metadata
bookkeeping, out of scope).
"""
import operator

import threading

import numpy as np

from . import _lib

_substitute = threading.local()     # .host = (data identity, host array) while lower_mask() evaluates a host term


class MaskBase:
    def include(self, data=None, view=()):
        """True where the voxel takes part in computations."""
        return self._include(data=data, view=view)

    def exclude(self, data=None, view=()):
        return np.logical_not(self._include(data=data, view=view))

    def _include(self, data=None, view=()):
        raise NotImplementedError

    def any(self):
        return np.any(self.include())

    def _filled(self, data, fill=np.nan, view=()):
        dt = np.result_type(data.dtype, 0.0)
        sliced = np.array(data[view], dtype=dt, copy=True)
        sliced[self.exclude(data=data, view=view)] = fill
        return sliced

    def _flattened(self, data, view=()):
        return data[view][self.include(data=data, view=view)]

    def __and__(self, other):
        return CompositeMask(self, other, operation="and")

    def __or__(self, other):
        return CompositeMask(self, other, operation="or")

    def __xor__(self, other):
        return CompositeMask(self, other, operation="xor")

    def __invert__(self):
        return InvertedMask(self)

    # ---- device lowering --------------------------------------------------
    def _device_terms(self, data):
        """Return (flags, thr_lo, thr_hi, host_bool_array_or_None) when this
        mask can be expressed as an AND of device terms evaluated on *data*
        (the array the kernel will read); otherwise None."""
        return None


class InvertedMask(MaskBase):
    def __init__(self, mask):
        self._mask = mask

    def _include(self, data=None, view=()):
        return np.logical_not(self._mask.include(data=data, view=view))

    def __invert__(self):
        return self._mask


class CompositeMask(MaskBase):
    def __init__(self, mask1, mask2, operation="and"):
        if operation not in ("and", "or", "xor"):
            raise ValueError("Operation '{0}' not supported".format(operation))
        self._mask1, self._mask2, self._operation = mask1, mask2, operation

    def _include(self, data=None, view=()):
        a = self._mask1._include(data=data, view=view)
        b = self._mask2._include(data=data, view=view)
        if self._operation == "and":
            return np.bitwise_and(a, b)
        if self._operation == "or":
            return np.bitwise_or(a, b)
        return np.bitwise_xor(a, b)

    def _device_terms(self, data):
        if self._operation != "and":
            return None
        a = self._mask1._device_terms(data)
        b = self._mask2._device_terms(data)
        if a is None or b is None:
            return None
        return _and_terms(a, b)


class BooleanArrayMask(MaskBase):
    def __init__(self, mask, wcs=None, shape=None, include=True):
        mask = np.asarray(mask)
        if mask.dtype != bool:
            mask = mask.astype(bool)
        self._mask = mask
        self._wcs = wcs
        self._include_flag = include
        if shape is not None:
            np.broadcast_shapes(mask.shape, tuple(shape))   # raises like the reference on mismatch
        self._shape = tuple(shape) if shape is not None else mask.shape

    @property
    def shape(self):
        return self._shape

    def _include(self, data=None, view=()):
        m = np.broadcast_to(self._mask, self._shape)[view]
        return m if self._include_flag else np.logical_not(m)

    def _device_terms(self, data):
        m = np.broadcast_to(self._mask, self._shape)
        if not self._include_flag:
            m = np.logical_not(m)
        return (0, -np.inf, np.inf, m)


class DeviceBooleanMask(BooleanArrayMask):
    """A BooleanArrayMask whose array lives in HBM as uint8 (1 = include): the mask of a cube computed on the device
    (downsample_axis).  *source* is the DeviceArray, or a callable that produces it on first use.  Kernels take the
    device array as it is (cube._mask_spec); the host copy is made only when ``include()`` / ``exclude()`` or a host
    composition asks for it."""

    def __init__(self, source, wcs=None, shape=None):
        self._source = source
        self._host = None
        self._wcs = wcs
        self._include_flag = True
        self._shape = tuple(shape) if shape is not None else tuple(source.shape)

    def device_array(self):
        if callable(self._source):
            self._source = self._source()
        return self._source

    @property
    def _mask(self):
        if self._host is None:
            self._host = self.device_array().get().view(bool)
        return self._host


class LazyMask(MaskBase):
    """mask = function(data), evaluated lazily on the data it was created for
    (masks.py:586-668).  ``np.isfinite`` lowers to SPC_MASK_FINITE."""

    def __init__(self, function, cube=None, data=None):
        self._function = function
        if cube is not None:
            self._data_ref = cube
        elif data is not None:
            self._data_ref = _Holder(data)
        else:
            raise ValueError("Either a cube or (data & wcs) is required.")

    def _own_data(self):
        # lower_mask() evaluating on behalf of a view of the SAME data (cube._WideView: the float64 samples of a wide
        # FITS image) hands its host array over here, so that the predicate is decided on the samples the kernel will
        # read and not on the cube's float32-narrowed copy
        sub = getattr(_substitute, "host", None)
        if sub is not None and getattr(self._data_ref, "_data_id", self._data_ref) is sub[0]:
            return sub[1]
        return self._data_ref._host_data()

    def _include(self, data=None, view=()):
        return self._function(self._own_data()[view])

    def _device_terms(self, data):
        if self._function is np.isfinite and self._data_ref._is_same_data(data):
            return (_lib.MASK_FINITE, -np.inf, np.inf, None)
        return None


class NotNaNMask(LazyMask):
    """``~np.isnan(data)`` of the cube's own data - the mask spectral_interpolate
    and reproject attach (dask_spectral_cube.py:1364; spectral_cube.py:2741-2746
    with NaN outside the footprint).  Redundant on the device: NaN samples never
    take part in a reduction."""

    def __init__(self, cube):
        super().__init__(lambda x: ~np.isnan(x), cube=cube)

    def _device_terms(self, data):
        if self._data_ref._is_same_data(data):
            return (0, -np.inf, np.inf, None)
        return None


_CMP = {operator.gt: _lib.MASK_GT, operator.ge: _lib.MASK_GE,
        operator.lt: _lib.MASK_LT, operator.le: _lib.MASK_LE}


class LazyComparisonMask(LazyMask):
    """``cube > value`` etc. (masks.py:670-758)."""

    def __init__(self, function, comparison_value, cube=None, data=None):
        self._cmp = function
        self._value = comparison_value
        super().__init__(lambda x: function(x, comparison_value), cube=cube, data=data)

    def _device_terms(self, data):
        if self._cmp in _CMP and np.isscalar(self._value) and self._data_ref._is_same_data(data):
            v = float(self._value)
            # The device compares float32 data with a float32 threshold.  numpy does
            # the same for "weak" python scalars (NEP 50); typed float64 scalars are
            # compared in float64, so only lower those when exactly representable.
            weak = type(self._value) in (float, int)
            if v != v:
                return None          # a NaN threshold includes nothing: left to the host form (all False)
            if getattr(data, "_wide", False):
                # the float64 kernels (cube._mask_spec64): float64 samples against a float64 threshold, as numpy compares them
                flag = _CMP[self._cmp]
                return (flag, v, np.inf, None) if flag in (_lib.MASK_GT, _lib.MASK_GE) else (flag, -np.inf, v, None)
            if weak or float(np.float32(v)) == v or not np.isfinite(v):
                v = float(np.float32(v))          # +-inf stay +-inf: `cube > -inf` is a real comparison
                flag = _CMP[self._cmp]
                if flag in (_lib.MASK_GT, _lib.MASK_GE):
                    return (flag, v, np.inf, None)
                return (flag, -np.inf, v, None)
        return None


class FunctionMask(MaskBase):
    """mask = function(data[view]) (masks.py:760-803)."""

    def __init__(self, function):
        self._function = function

    def _include(self, data=None, view=()):
        out = self._function(data[view])
        if out.shape != data[view].shape:
            raise ValueError("Function did not return mask with correct shape - expected "
                             "{0}, got {1}".format(data[view].shape, out.shape))
        return out


class _Holder:
    def __init__(self, data):
        self._d = data

    def _host_data(self):
        return self._d

    def _is_same_data(self, data):
        return data is self._d


def _and_terms(a, b):
    fa, la, ha, ma = a
    fb, lb, hb, mb = b
    flags = (fa | fb) & _lib.MASK_FINITE
    # lower bound: the stricter of the two (GT beats GE at equal thresholds)
    lo, lof = -np.inf, 0
    for f, l in ((fa & (_lib.MASK_GT | _lib.MASK_GE), la), (fb & (_lib.MASK_GT | _lib.MASK_GE), lb)):
        if f and (not lof or l > lo or (l == lo and f == _lib.MASK_GT)):
            lo, lof = l, f
    hi, hif = np.inf, 0
    for f, h in ((fa & (_lib.MASK_LT | _lib.MASK_LE), ha), (fb & (_lib.MASK_LT | _lib.MASK_LE), hb)):
        if f and (not hif or h < hi or (h == hi and f == _lib.MASK_LT)):
            hi, hif = h, f
    if ma is None:
        m = mb
    elif mb is None:
        m = ma
    else:
        m = np.logical_and(ma, mb)
    return (flags | lof | hif, lo, hi, m)


def lower_mask(mask, data, shape):
    """Lower *mask* for kernels that read *data* (host ndarray identity used to
    decide whether lazy predicates may run on the device).

    Returns (flags, thr_lo, thr_hi, host_uint8_array_or_None).  Anything that
    cannot be expressed as an AND of device terms is materialised on the host
    into the array term - results are identical, only the traffic differs.
    """
    if mask is None:
        return (0, 0.0, 0.0, None)
    terms = mask._device_terms(data)
    if terms is None:
        # host form: FunctionMask and friends index the voxel ARRAY (masks.py:760-803), not the cube object
        host = data._host_data() if hasattr(data, "_host_data") else data
        ident = getattr(data, "_data_id", None)
        _substitute.host = (ident, host) if ident is not None else None
        try:
            inc = np.asarray(mask.include(data=host))
        finally:
            _substitute.host = None
        terms = (0, -np.inf, np.inf, np.broadcast_to(inc, shape))
    flags, lo, hi, m = terms
    arr = None
    if m is not None:
        flags |= _lib.MASK_ARRAY
        arr = np.ascontiguousarray(np.broadcast_to(m, shape)).view(np.uint8)
    # a bound that is not in force is passed as 0; one that is keeps its value, infinities included
    lo = float(lo) if flags & (_lib.MASK_GT | _lib.MASK_GE) else 0.0
    hi = float(hi) if flags & (_lib.MASK_LT | _lib.MASK_LE) else 0.0
    return (flags, lo, hi, arr)


# ---- mask tree -> postfix program for ops.mask_eval (spc_mask_eval_f32 / _f64) -------------------------------------
_PROG_CMP = {operator.gt: _lib.CMP_GT, operator.ge: _lib.CMP_GE, operator.lt: _lib.CMP_LT, operator.le: _lib.CMP_LE,
             operator.eq: _lib.CMP_EQ, operator.ne: _lib.CMP_NE}
_PROG_OP = {"and": _lib.MOP_AND, "or": _lib.MOP_OR, "xor": _lib.MOP_XOR}


class MaskProgram:
    """A mask tree in the postfix form the device evaluates (spc_mask_program, include/spcube_hip.h).

    slots:    the cubes the comparison terms read, in slot order - as compile_mask() returns it the cube objects
              themselves; ops.mask_eval() wants their DeviceArrays of the path's sample type in their place
    operands: [(array, (stride_z, stride_y, stride_x))]: un-broadcast C-contiguous host arrays (float32, float64 or
              uint8) or uint8 DeviceArrays, element strides, 0 = broadcast along that axis
    instr:    [(opcode, slot, cmp, operand, imm)], _lib.MOP_* / _lib.CMP_*; operand -1 = compare with imm"""
    __slots__ = ("slots", "operands", "instr")

    def __init__(self):
        self.slots, self.operands, self.instr = [], [], []


class _NotCompilable(Exception):
    pass


def _bcast_strides(arr_shape, shape):
    """(3-D shape, element strides) of a C-contiguous array of *arr_shape* read as (nz, ny, nx): missing leading axes and
    axes of length 1 get stride 0"""
    s3 = (1,) * (3 - len(arr_shape)) + tuple(arr_shape)
    strides, run = [0, 0, 0], 1
    for a in (2, 1, 0):
        if s3[a] != 1:
            strides[a] = run
        run *= s3[a]
    return s3, tuple(strides)


def _threshold_ok(dtype):
    # longdouble is 'f' with more than 8 bytes: numpy would compare in extended precision, which no kernel does
    return dtype.kind in "biu" or (dtype.kind == "f" and dtype.itemsize <= 8)


def compile_mask(mask, data, shape, wide):
    """*mask* as a :class:`MaskProgram` for kernels that read *data* (the cube, or its float64 view) on the float32 or
    (*wide*) the float64 path, or None when a term has no device form: FunctionMask, LazyMask of a function other than
    np.isfinite, a threshold of another dtype or shape, a term bound to a bare array that is not the cube's own, a
    cube that cannot hand out device samples of the path's type as they are, or a tree beyond the program's limits.

    Thresholds follow numpy (NEP 50): a Python float / int is rounded to the sample type, every other scalar is used
    as an exact double; arrays stay un-broadcast, float32 as it is and bool / integer / float16 / float64 as float64 -
    the device compares sample and threshold as doubles, which is numpy's result for each of these."""
    shape = tuple(int(n) for n in shape)
    cube = getattr(data, "_cube", data)
    prog = MaskProgram()
    seen = {}                                   # id(source array) -> operand index

    def slot_of(ref):
        if isinstance(ref, _Holder):
            own = getattr(cube, "_data", None)
            if own is None or ref._d is not own:
                raise _NotCompilable
            ref = cube
        elif ref._is_same_data(data):
            ref = cube
        for i, c in enumerate(prog.slots):
            if c is ref or c._is_same_data(ref):
                return i
        ok = (hasattr(ref, "_device_data") and tuple(ref._shape) == shape and ref._stream_source() is None
              and (ref._wide_resident() if wide else not ref._is_wide()))
        if not ok or len(prog.slots) == _lib.MASK_PROG_MAX_SLOTS:
            raise _NotCompilable
        prog.slots.append(ref)
        return len(prog.slots) - 1

    def operand_of(src, arr, arr_shape):
        if id(src) in seen:
            return seen[id(src)]
        try:
            if np.broadcast_shapes(tuple(arr_shape), shape) != shape:
                raise _NotCompilable
        except ValueError:
            raise _NotCompilable
        if len(prog.operands) == _lib.MASK_PROG_MAX_OPERANDS:
            raise _NotCompilable
        prog.operands.append((arr, _bcast_strides(arr_shape, shape)[1]))
        seen[id(src)] = len(prog.operands) - 1
        return seen[id(src)]

    def walk(m):
        if isinstance(m, CompositeMask):
            walk(m._mask1)
            walk(m._mask2)
            prog.instr.append((_PROG_OP[m._operation], 0, 0, -1, 0.0))
        elif isinstance(m, InvertedMask):
            walk(m._mask)
            prog.instr.append((_lib.MOP_NOT, 0, 0, -1, 0.0))
        elif isinstance(m, DeviceBooleanMask):
            dev = m.device_array()
            if tuple(dev.shape) != shape:
                raise _NotCompilable
            if len(prog.operands) == _lib.MASK_PROG_MAX_OPERANDS:
                raise _NotCompilable
            prog.operands.append((dev, (getattr(dev, "plane_stride", shape[1] * shape[2]), getattr(dev, "row_stride", shape[2]), 1)))
            prog.instr.append((_lib.MOP_LOAD, 0, 0, len(prog.operands) - 1, 0.0))
        elif isinstance(m, BooleanArrayMask):
            b = m._mask
            prog.instr.append((_lib.MOP_LOAD, 0, 0, operand_of(b, np.ascontiguousarray(b).view(np.uint8), b.shape), 0.0))
            if not m._include_flag:
                prog.instr.append((_lib.MOP_NOT, 0, 0, -1, 0.0))
        elif isinstance(m, NotNaNMask):
            # v <= +inf: false for NaN alone - a term of its own, so the include array is complete without nan_excluded
            prog.instr.append((_lib.MOP_CMP, slot_of(m._data_ref), _lib.CMP_LE, -1, float("inf")))
        elif isinstance(m, LazyComparisonMask):
            if m._cmp not in _PROG_CMP:
                raise _NotCompilable
            slot, v = slot_of(m._data_ref), m._value
            if type(v) in (float, int):
                try:
                    imm = float(v) if wide else float(np.float32(v))
                except OverflowError:
                    raise _NotCompilable
                prog.instr.append((_lib.MOP_CMP, slot, _PROG_CMP[m._cmp], -1, imm))
                return
            try:
                a = np.asarray(v)
            except Exception:
                raise _NotCompilable
            if not _threshold_ok(a.dtype):
                raise _NotCompilable
            if a.ndim == 0:
                prog.instr.append((_lib.MOP_CMP, slot, _PROG_CMP[m._cmp], -1, float(a)))
                return
            up = np.ascontiguousarray(a, dtype=np.float32 if a.dtype == np.float32 else np.float64)
            prog.instr.append((_lib.MOP_CMP, slot, _PROG_CMP[m._cmp], operand_of(v, up, a.shape), 0.0))
        elif type(m) is LazyMask and m._function is np.isfinite:
            prog.instr.append((_lib.MOP_FINITE, slot_of(m._data_ref), 0, -1, 0.0))
        else:
            raise _NotCompilable

    try:
        walk(mask)
    except _NotCompilable:
        return None
    if len(prog.instr) > _lib.MASK_PROG_MAX_INSTR:
        return None
    depth = deepest = 0
    for op in prog.instr:
        depth += {_lib.MOP_NOT: 0, _lib.MOP_AND: -1, _lib.MOP_OR: -1, _lib.MOP_XOR: -1}.get(op[0], 1)
        deepest = max(deepest, depth)
    if deepest > _lib.MASK_PROG_MAX_STACK:
        return None
    return prog


def contains(mask, cls):
    """True when a term of the mask tree is an instance of *cls*"""
    if isinstance(mask, cls):
        return True
    if isinstance(mask, CompositeMask):
        return contains(mask._mask1, cls) or contains(mask._mask2, cls)
    if isinstance(mask, InvertedMask):
        return contains(mask._mask, cls)
    return False


def foreign_owner(mask):
    """The ONE other cube whose data every lazy term of *mask* is bound to (e.g. the parent of a
    smoothed cube, which keeps the parent's mask object: dask_spectral_cube.py:836-840), or None
    when there is no such single cube.  cube._mask_spec() then evaluates the mask on that cube's
    device data instead of copying it to the host."""
    owners = []

    def walk(m):
        if isinstance(m, CompositeMask):
            walk(m._mask1); walk(m._mask2)
        elif isinstance(m, InvertedMask):
            walk(m._mask)
        elif isinstance(m, LazyMask):
            owners.append(m._data_ref)
        elif isinstance(m, FunctionMask):
            owners.append(None)
    walk(mask)
    first = owners[0] if owners else None
    if first is None or isinstance(first, _Holder) or any(o is not first for o in owners):
        return None
    return first
