"""Host-side mirror of the reference's operator interface for the hot path.

``SpectralCube`` keeps the reference's method names, argument meaning and
error behaviour for

    moment / moment0 / moment1 / moment2 / linewidth_sigma / linewidth_fwhm
    argmax / argmin / max / min (axis=0)
    spectral_smooth / spatial_smooth / spectral_interpolate / reproject
    with_mask / with_fill_value / filled_data / spectral_axis

(reference: spectral_cube/spectral_cube.py:1614-1763, 793-819, 2649-2842,
3186-3332; spectral_cube/dask_spectral_cube.py:880-993, 1031-1132, 1250-1373)
while every voxel is touched only by the HIP kernels behind the C ABI
(include/spcube_hip.h).  There is no CPU fallback: without the library or a
GPU the compute methods raise ``HipLibraryError``.

Differences by design: results of cube->cube operations are
float32 device-resident cubes (the Dask class keeps float32 too; only
spectral_interpolate returns float64 there); 2-D maps are float64 like the
reference; units are plain strings unless astropy is importable.  The 1e8-voxel
``warn_slow`` guard (utils.py:41-75) is kept where BOTH reference classes have it
(``reproject``, ``convolve_to``): set ``cube.allow_huge_operations = True`` for
cubes above the threshold, exactly as with the reference.
"""
import functools
import math
import operator
import os
import warnings

import numpy as np

from . import _lib, masks as M, ops
from .beam import Beam, BeamError
from .device import DeviceArray
from .kernels import kernel_array
from .pending import Pending
from .wcs import (SimpleWCS, check_same_spectral_kind, join_celestial_spectral, pix_cen_spatial, pix_size, reproject_pixel_map,
                  spectral_unit_scale)

SIGMA2FWHM = 2. * np.sqrt(2. * np.log(2.))      # spectral_cube.py:66


class VarianceWarning(UserWarning):
    pass


class PrecisionWarning(UserWarning):
    """the source holds samples float32 cannot represent exactly (a float64 array, a BITPIX = -64 / 32 / 64 FITS image): the
    reference keeps such a cube in float64 (``np.result_type(dtype, 0.0)``, masks.py:225).  The moments along the spectral
    axis (moment 0 / 1 / 2 / N, argmax / argmin, moments012) of a resident cube are computed from the float64 samples
    (spc_moments_f64); every other operator stages the cube as float32 (sums are carried in float64, the SAMPLES are
    rounded to 24 bits: ~6e-8 relative per sample, inside the 1e-5 contract of the float32 configurations, but not the
    reference's float64 result).  Raised once per source, the first time its samples are narrowed."""


_NARROWED = "%s samples are narrowed to float32 on their way to HBM (the reference would keep float64, masks.py:225): results " \
            "agree with a float64 computation to ~1e-7 relative, not to float64 precision"


def _is_wide_dtype(dtype):
    dt = np.dtype(dtype)
    return (dt.kind == "f" and dt.itemsize > 4) or (dt.kind in "iu" and dt.itemsize >= 4)


def _warn_if_narrowed(dtype=None, bitpix=None, stacklevel=3):
    if dtype is not None:
        wide, what = _is_wide_dtype(dtype), str(np.dtype(dtype))
    else:
        wide = bitpix in (-64, 32, 64)
        what = "BITPIX = %s" % bitpix
    if wide:
        warnings.warn(_NARROWED % what, PrecisionWarning, stacklevel=stacklevel)


class _DataToken:
    """identity of a cube's voxel values, shared by the cubes derived from it without touching them (with_mask,
    with_fill_value, with_spectral_unit): lazy masks compare it (``_is_same_data``), and a wide source keeps what its
    float64 path needs here - the FITS image the samples come from, the float64 device copy, whether the narrowing to
    float32 has been announced."""
    __slots__ = ("wide_file", "dev64", "warned", "lazy64", "derived64")

    def __init__(self):
        self.wide_file = None        # (path, hdu, bitpix) of a resident BITPIX = -64 / 32 / 64 image
        self.dev64 = None            # float64 DeviceArray, staged by the first spectral moment
        self.warned = False
        self.lazy64 = None           # pending float64 operator of a cube DERIVED from a wide one (spectral_smooth, ...)
        self.derived64 = False       # the values exist as a float64 DeviceArray only (dev64 / lazy64): no host array, no file


def _token_dev64(tok):
    """the float64 DeviceArray of a DERIVED wide cube's data token (pending operator run once)"""
    if tok.dev64 is None:
        _lib.require_gpu()
        tok.dev64 = tok.lazy64()
        tok.lazy64 = None
    return tok.dev64


class _WideView:
    """what a mask is lowered against for the float64 kernels: the cube's identity (lazy masks bound to the cube stay
    device terms), ``_wide`` (comparison thresholds keep their float64 value: numpy compares a float64 cube in float64),
    and the float64 samples for the terms that are evaluated on the host"""
    _wide = True

    def __init__(self, cube):
        self._cube, self._data_id = cube, cube._data_id

    def _host_data(self):
        c = self._cube
        if c._data_id.wide_file is None and c._data is not None:
            return c._data
        return c._device_data64().get()


_ALL_NAN = ("All values in reprojected cube are nan.  This can be caused"
            " by an error in which coordinates do not 'round-trip'.  Try "
            "setting ``roundtrip_coords=False``.  You might also check "
            "whether the WCS transformation produces valid pixel->world "
            "and world->pixel coordinates in each axis.")


def _channel_plan(zs, nz):
    """reproject onto a header with a spectral axis of its own (oracle_np.reproject_separable): target channels at the source
    channel positions *zs*.  Positions inside [-0.5, nz - 0.5] are clipped to the cube and each output channel is the linear
    blend of the two source planes around it.  Returns ops.spectral_lerp's plan: ``inside`` (bool per output channel),
    ``lo`` (int32 lower plane, -1 outside: a NaN plane), ``t`` (weight of plane lo + 1) and ``ones`` (its unit spacing)."""
    inside = (zs >= -0.5) & (zs <= nz - 0.5)
    zc = np.clip(np.where(inside, zs, 0.0), 0.0, nz - 1.0)
    z0 = np.minimum(np.floor(zc).astype(np.int64), nz - 2)
    return inside, np.where(inside, z0, -1).astype(np.int32), zc - z0, np.ones(len(zs))


class SliceWarning(UserWarning):
    """a spectral slab whose two limits fall on the same channel (utils.py:86)"""


class SmoothingWarning(UserWarning):
    pass


class UnitsError(ValueError):
    """stands in for astropy.units.UnitsError"""


class WCSCelestialError(ValueError):
    """spectral_cube.utils.WCSCelestialError (utils.py:95): an image without two celestial axes was asked for a
    celestial operation (lower_dimensional_structures.py:450-538)."""


class BeamUnitsError(Exception):
    """spectral_cube.utils.BeamUnitsError (base_class.py:134-137)"""


_VARIANCE_MSG = ("Note that the second moment returned will be a "
                 "variance map. To get a linewidth map, use the "
                 "SpectralCube.linewidth_fwhm() or "
                 "SpectralCube.linewidth_sigma() methods instead.")


MEMORY_THRESHOLD = 1e8        # voxels: cube_utils.py:266-274


def warn_slow(function):
    """utils.py:41-75: operations the reference refuses on huge cubes unless
    ``allow_huge_operations`` is set (they load the whole cube there; here they need the whole cube
    resident in HBM, plus an output of the same size).  Same switch, same ValueError."""
    @functools.wraps(function)
    def wrapper(self, *args, **kwargs):
        if self._is_huge and not self.allow_huge_operations:
            raise ValueError("This function ({0}) requires loading the entire "
                             "cube into memory, and the cube is large ({1} "
                             "pixels), so by default we disable this operation. "
                             "To enable the operation, set "
                             "`cube.allow_huge_operations=True` and try again.  "
                             "See {2} for details.".format(str(function), self.size,
                                                           "https://spectral-cube.readthedocs.io/en/latest/big_data.html"))
        return function(self, *args, **kwargs)
    return wrapper


def _check_convolve(convolve):
    """The ``convolve=`` seam of spectral_smooth / spatial_smooth / convolve_to
    (dask_spectral_cube.py:883, 963; spectral_cube.py:2810, 3188, 3335).  The device stencils ARE
    astropy's normalised, NaN-interpolating convolution, so astropy's own ``convolve`` (the default of
    the smoothing methods) and ``convolve_fft`` (the default of convolve_to; same mathematics through
    an FFT) are accepted as naming it; any other callable cannot run on the device."""
    if convolve is None:
        return
    mod, name = getattr(convolve, "__module__", "") or "", getattr(convolve, "__name__", "")
    if mod.startswith("astropy.convolution") and name in ("convolve", "convolve_fft"):
        return
    raise NotImplementedError("custom `convolve` callables cannot run on the device; the HIP stencils "
                              "implement astropy.convolution.convolve (pass that, convolve_fft, or nothing)")


def _unit_mul(a, b):
    a, b = (a or "").strip(), (b or "").strip()
    return (a + " " + b).strip()


def _unit_pow(a, n):
    a = (a or "").strip()
    if not a or n == 1:
        return a
    return "(%s)%d" % (a, n) if " " in a or "/" in a else "%s%d" % (a, n)


def _unit_div(a, b):
    a, b = (a or "").strip(), (b or "").strip()
    if a == b:
        return ""
    if not b:
        return a
    return "%s / %s" % (a or "1", "(%s)" % b if " " in b or "/" in b else b)


class WCSMismatchWarning(UserWarning):
    """spectral_cube.utils.WCSMismatchWarning: arithmetic on two cubes of one shape whose WCSs differ (spectral_cube.py:979-982)"""


def _same_fill(a, b):
    a, b = float(a), float(b)
    return a == b or (a != a and b != b)


class _ArithPending:
    """A pending chain of arithmetic steps over ``source`` (its samples and its mask): what ``cube + a``, ``- a``, ``* a``,
    ``/ a`` and ``** a`` return carries one, and an operator applied to such a result before anything has used it extends
    a COPY of the chain - ``(cube - cont) / rms * 1e3`` reads the cube once and writes once (ops.arith, spc_arith_f32 /
    _f64).  ``steps``: a tuple (never mutated: the parent result keeps its own) of ``(op, operand, refill)``; operand a
    Python float, a host array already in the sample type and broadcastable to the cube, a DeviceArray, or the right-hand
    SpectralCube of a cube-on-cube step."""

    def __init__(self, source, steps, wide, mask, fill):
        self.source, self.steps, self.wide, self.mask, self.fill = source, tuple(steps), bool(wide), mask, fill

    def _samples(self, cube):
        """device samples of a right-hand cube in this program's sample type"""
        if not self.wide:
            return cube._device_data()
        if cube._is_wide():
            return cube._device_data64()
        return DeviceArray.from_numpy(cube._host_data(), self.source.device, dtype=np.float64)

    def __call__(self):
        src = self.source
        data, mspec, view = src._operand(self.wide)
        steps = []
        for op, operand, refill in self.steps:
            if isinstance(operand, SpectralCube):
                operand = self._samples(operand)
            elif isinstance(operand, np.ndarray):
                operand = DeviceArray.from_numpy(operand, src.device)
            steps.append((op, operand, refill))
        return ops.arith(data, steps, mask=mspec, fill=self.fill, nan_excluded=_nan_term_dropped(src, view))


# numpy's fast paths of ``x ** p`` for a scalar p (x * x, sqrt, 1 / x, a copy, ones): exact, where pow() is not
_EXACT_POWERS = {2.0: ("square", None), 0.5: ("sqrt", None), -1.0: ("recip", None), 1.0: ("mul", 1.0), 0.0: ("one", None)}


# downsample_axis estimators, recognised by identity (np.max is np.amax, np.min is np.amin)
_DS_ESTIMATORS = ((np.nanmean, _lib.DS_NANMEAN), (np.nansum, _lib.DS_NANSUM), (np.nanmax, _lib.DS_NANMAX),
                  (np.nanmin, _lib.DS_NANMIN), (np.mean, _lib.DS_MEAN), (np.sum, _lib.DS_SUM), (np.max, _lib.DS_MAX),
                  (np.amax, _lib.DS_MAX), (np.min, _lib.DS_MIN), (np.amin, _lib.DS_MIN))


def _ds_estimator(estimator):
    for fn, code in _DS_ESTIMATORS:
        if estimator is fn:
            return code
    raise NotImplementedError("downsample_axis estimator %r is not built: np.nanmean, np.nansum, np.nanmax, np.nanmin, "
                              "np.mean, np.sum, np.max (np.amax), np.min (np.amin)" % (getattr(estimator, "__name__", estimator),))


# scipy.ndimage's rank family, recognised by name (the package never imports scipy)
_RANK_FILTERS = ("median_filter", "minimum_filter", "maximum_filter", "percentile_filter", "rank_filter")
_RANK_IGNORED = ("use_memmap", "verbose", "num_cores", "parallel", "update_function", "save_to_tmp_dir")


def _rank_filter_name(filter):
    name = filter if isinstance(filter, str) else getattr(filter, "__name__", None)
    if name not in _RANK_FILTERS:
        raise NotImplementedError("filter %r is not built: the device runs scipy.ndimage's rank family - %s (the function or "
                                  "its name)" % (name if name is not None else filter, ", ".join(_RANK_FILTERS)))
    return name


def _rank_filter_options(filter, w, kwargs):
    """(rank, mode, cval) of a rank filter over a window of *w* samples: the one integer rank into the sorted window that
    scipy's median / minimum / maximum / percentile / rank filter selects (ndimage/_filters.py, _rank_filter), and the
    boundary keywords.  Keywords the device does not honour raise; the reference's scheduling keywords are dropped."""
    name = _rank_filter_name(filter)
    kw = {k: v for k, v in kwargs.items() if k not in _RANK_IGNORED}
    mode, cval = kw.pop("mode", "reflect"), kw.pop("cval", 0.0)
    origin = kw.pop("origin", 0)
    if np.any(np.asarray(origin) != 0):
        raise NotImplementedError("origin other than 0 is not built on the device (got %r)" % (origin,))
    if kw.pop("footprint", None) is not None:
        raise NotImplementedError("a footprint is not built on the device: rectangular windows (ksize) only")
    if mode not in _lib.RANK_MODES:
        raise ValueError("mode must be one of %s (got %r)" % (", ".join(sorted(_lib.RANK_MODES)), mode))
    if name == "rank_filter":
        if "rank" not in kw:
            raise TypeError("rank_filter needs rank=")
        rank = operator.index(kw.pop("rank"))
        if rank < 0:
            rank += w
        if rank < 0 or rank >= w:
            raise ValueError("rank not within the window of %d samples" % w)
    elif name == "percentile_filter":
        if "percentile" not in kw:
            raise TypeError("percentile_filter needs percentile=")
        p = kw.pop("percentile")
        if p < 0:
            p += 100
        if p < 0 or p > 100:
            raise ValueError("invalid percentile (got %r)" % (kwargs["percentile"],))
        rank = w - 1 if p == 100 else int(float(w) * p / 100.0)
    else:
        rank = {"median_filter": w // 2, "minimum_filter": 0, "maximum_filter": w - 1}[name]
    if kw:
        raise TypeError("unexpected keyword arguments for %s: %s" % (name, sorted(kw)))
    return rank, mode, float(cval)


def _nan_term_dropped(cube, view):
    """True when the cube's mask goes to the kernels as device terms (``_device_terms(view)``, *view* what it is lowered
    against) and names ~isnan of the cube's own data.  That term lowers to nothing (NotNaNMask: a reduction skips NaN
    anyway), so an operator that fills excluded voxels or reports the include map must exclude NaN samples itself - as
    reproject and streaming.original_include do"""
    m = cube._mask
    return (m is not None and not isinstance(m, M.DeviceBooleanMask) and M.contains(m, M.NotNaNMask)
            and m._device_terms(view) is not None)


def _check_downsample_fits(cube, shape):
    """the downsampled result of a streamed cube is made resident: its data + mask must fit the HBM budget"""
    from . import streaming
    need = 5 * int(np.prod(shape, dtype=np.int64))
    budget = streaming.hbm_budget(cube.device)
    if need > budget:
        raise streaming.HugeCubeError(
            "downsample_axis of an out-of-core cube keeps its result in HBM: the result (data + mask) takes %d bytes "
            "(%.2f GiB) against a budget of %d bytes (%.2f GiB, SPC_HBM_BUDGET); use a larger factor"
            % (need, need / 2**30, budget, budget / 2**30))
    return need, budget


def _downsample_streamed(cube, axis, factor, truncate, est, fill, shape):
    """ops.downsample of a cube larger than the HBM budget into a resident result: along the spectral axis strip by strip
    (every spaxel whole), along y or x slab by slab (every image plane whole); the kernel writes each part in place"""
    from . import streaming
    from .device import Stream
    need, budget = _check_downsample_fits(cube, shape)
    data = DeviceArray(shape, np.float32, cube.device)
    inc = DeviceArray(shape, np.uint8, cube.device)
    src = cube._stream_source()
    terms = streaming._mask_terms(cube)
    has_arr = terms is not None and terms[3] is not None
    nan_ex = _nan_term_dropped(cube, cube)
    left = max(budget - need, 1)
    compute = Stream(cube.device)
    if axis == 0:
        rows = streaming.plan_rows(src.shape, left, mask_array=has_arr, max_strip_mb=getattr(src, "max_strip_mb", 0))
        for y0, y1, dev, mspec in streaming.Strips(cube, compute, rows):
            ops.downsample(dev, 0, factor, truncate, est, fill, mask=mspec, out=data.rows(y0, y1), out_mask=inc.rows(y0, y1),
                           stream=compute, nan_excluded=nan_ex)
    else:
        planes = streaming.plan_planes(src.shape, left, mask_array=has_arr, out_factor=0.0)
        for z0, z1, dev, mspec in streaming.Strips(cube, compute, planes, axis=0):
            ops.downsample(dev, axis, factor, truncate, est, fill, mask=mspec, out=data.planes(z0, z1), out_mask=inc.planes(z0, z1),
                           stream=compute, nan_excluded=nan_ex)
    compute.synchronize()
    return data, inc


def _check_cut_fits(cube, shape, has_mask):
    """the cut of a streamed cube is made resident: its data (+ mask) must fit the HBM budget"""
    from . import streaming
    need = (5 if has_mask else 4) * int(np.prod(shape, dtype=np.int64))
    budget = streaming.hbm_budget(cube.device)
    if need > budget:
        raise streaming.HugeCubeError(
            "a cut of an out-of-core cube keeps its result in HBM: the result %s (data%s) takes %d bytes (%.2f GiB) against a "
            "budget of %d bytes (%.2f GiB, SPC_HBM_BUDGET); cut a smaller range"
            % (tuple(shape), " + mask" if has_mask else "", need, need / 2**30, budget, budget / 2**30))
    return need, budget


def _cut_window(spec):
    """(z0, z1, y0, y1): the channel and row range of the parent that the view *spec* ((start, step, length) per axis)
    touches - what a streamed cut stages; channels and rows outside it never leave the host"""
    lo, hi = [], []
    for (start, step, n) in spec[:2]:
        last = start + (n - 1) * step
        lo.append(min(start, last))
        hi.append(max(start, last) + 1)
    return lo[0], hi[0], lo[1], hi[1]


def _subcube_streamed(cube, spec, shape, has_mask):
    """ops.subcube of a cube larger than the HBM budget into a resident result: slabs of planes of the window the view
    touches go through the strip pipeline, and the kernel writes each slab's selected channels in place"""
    from . import streaming
    from .device import Stream
    need, budget = _check_cut_fits(cube, shape, has_mask)
    data = DeviceArray(shape, np.float32, cube.device)
    inc = DeviceArray(shape, np.uint8, cube.device) if has_mask else None
    z0, z1, y0, y1 = window = _cut_window(spec)
    terms = streaming._mask_terms(cube)
    has_arr = terms is not None and terms[3] is not None
    nan_ex = _nan_term_dropped(cube, cube)
    compute = Stream(cube.device)
    wshape = (z1 - z0, y1 - y0, cube._shape[2])
    planes = streaming.plan_planes(wshape, max(budget - need, 1), mask_array=has_arr, out_factor=0.0)
    (zs, zstep, nzo), (ys, ystep, _), (xs, xstep, _) = spec
    chan = zs + zstep * np.arange(nzo, dtype=np.int64)           # parent channel of every output plane
    for a, b, dev, mspec in streaming.Strips(cube, compute, planes, axis=0, window=window):
        sel = np.nonzero((chan >= z0 + a) & (chan < z0 + b))[0]
        if sel.size == 0:
            continue
        k0, k1 = int(sel[0]), int(sel[-1]) + 1
        ops.subcube(dev, (int(chan[k0]) - z0 - a, ys - y0, xs), (zstep, ystep, xstep), (k1 - k0,) + tuple(shape[1:]), mask=mspec,
                    out=data.planes(k0, k1), out_mask=inc.planes(k0, k1) if inc is not None else None, want_mask=has_mask,
                    stream=compute, nan_excluded=nan_ex)
    compute.synchronize()
    return data, inc


def _bbox_streamed(cube):
    """ops.mask_bbox of a streamed cube: one box per row strip, merged on the host"""
    from . import streaming
    from .device import Stream
    compute = Stream(cube.device)
    nan_ex = _nan_term_dropped(cube, cube)
    box = None
    for y0, y1, dev, mspec in streaming.Strips(cube, compute):
        b = ops.mask_bbox(dev, mask=mspec, stream=compute, nan_excluded=nan_ex)
        if b is None:
            continue
        b = (b[0], (b[1][0] + y0, b[1][1] + y0), b[2])
        box = b if box is None else tuple((min(p[0], q[0]), max(p[1], q[1])) for p, q in zip(box, b))
    compute.synchronize()
    return box


_AXIS_NAMES = ("spectral axis (0)", "y axis (1)", "x axis (2)")


class Projection(np.ndarray):
    """2-D result map (stands in for lower_dimensional_structures.Projection
    :246-292): an ndarray carrying unit, wcs and meta."""

    def __new__(cls, value, unit="", wcs=None, meta=None, beam=None, device=0, header=None):
        obj = np.asarray(value).view(cls)
        obj.unit = unit
        obj.wcs = wcs
        obj.header = dict(header) if header is not None else dict(getattr(wcs, "header", None) or {})
        obj.meta = dict(meta or {})
        obj.beam = beam if beam is not None else obj.meta.get("beam")
        obj._spc_device = device
        return obj

    def __array_finalize__(self, obj):
        if obj is None:
            return
        self.unit = getattr(obj, "unit", "")
        self.wcs = getattr(obj, "wcs", None)
        self.header = getattr(obj, "header", {})
        self.meta = getattr(obj, "meta", {})
        self.beam = getattr(obj, "beam", None)
        self._spc_device = getattr(obj, "_spc_device", 0)

    def _celestial(self):
        if self.ndim != 2 or self.wcs is None or getattr(self.wcs, "naxis", 0) < 2:
            raise WCSCelestialError("WCS does not contain two spatial axes.")      # _raise_wcs_no_celestial
        return self.wcs

    def convolve_to(self, beam, convolve=None, **kwargs):
        """Convolve the image to *beam* (lower_dimensional_structures.py:450-494): the kernel
        ``beam.deconvolve(self.beam).as_kernel(pixscale)`` through the same NaN-aware 2-D stencils as
        the cube (one channel), astropy's normalised 'interpolate' treatment."""
        treat = kwargs.pop("nan_treatment", "interpolate")
        _check_convolve(convolve)
        if treat not in ("interpolate", "fill") or kwargs.pop("fill_value", 0.0) != 0.0 or kwargs:
            raise NotImplementedError("the device stencil is astropy.convolution.convolve with boundary='fill', "
                                      "fill_value=0, normalize_kernel=True and nan_treatment 'interpolate' or 'fill'")
        w = self._celestial()
        if self.beam is None:
            raise ValueError("No beam is contained in Projection.meta.")
        if beam == self.beam:
            warnings.warn("The given beam is identical to the current beam. Skipping convolution.")
            return self
        psm = w.pixel_scale_matrix
        pixscale = math.sqrt(abs(psm[0, 0] * psm[1, 1] - psm[0, 1] * psm[1, 0]))
        karr = beam.deconvolve(self.beam).as_kernel(pixscale)
        _lib.require_gpu()
        pix = np.asarray(self, dtype=np.float32)
        if treat == "fill":                  # astropy: NaN -> fill_value (0), plain normalised convolution
            pix = np.where(np.isnan(pix), np.float32(0.0), pix)
        img = DeviceArray.from_numpy(pix[None], self._spc_device)
        out = ops.spatial_conv(img, karr).get()[0].astype(self.dtype if self.dtype.kind == "f" else np.float32)
        return Projection(out, unit=self.unit, wcs=self.wcs, meta=dict(self.meta, beam=beam), beam=beam, device=self._spc_device)

    def reproject(self, header, order="bilinear"):
        """Reproject the image onto the celestial WCS of *header* (lower_dimensional_structures.py:496-538):
        bilinear, NaN outside the footprint - the cube's resampling kernel on one channel."""
        if order not in ("bilinear", 1):
            raise NotImplementedError("only order='bilinear' is built on the GPU path")
        w = self._celestial()
        newwcs = header if isinstance(header, SimpleWCS) else SimpleWCS(header, naxis=2)
        hdr = newwcs.header
        ny_out, nx_out = (int(hdr["NAXIS2"]), int(hdr["NAXIS1"])) if ("NAXIS1" in hdr and "NAXIS2" in hdr) else self.shape
        _lib.require_gpu()
        xs, ys = ops.wcs_pixel_map(w, newwcs, (ny_out, nx_out), self._spc_device)
        img = DeviceArray.from_numpy(np.asarray(self, dtype=np.float32)[None], self._spc_device)
        dev, _ = ops.resample_bilinear(img, xs, ys, fill=np.nan, want_footprint=False)
        out = dev.get()[0].astype(self.dtype if self.dtype.kind == "f" else np.float32)
        return Projection(out, unit=self.unit, wcs=newwcs, meta=dict(self.meta), beam=self.beam, device=self._spc_device)

    @property
    def value(self):
        return np.asarray(self)

    def quantity(self):
        """astropy Quantity when astropy is importable."""
        from astropy import units as u
        return u.Quantity(np.asarray(self), u.Unit(self.unit))


class SpectralCube:
    """(nz, ny, nx) float32 cube with a lazily lowered mask, device resident."""

    def __init__(self, data=None, wcs=None, mask=None, meta=None, fill_value=np.nan,
                 header=None, unit=None, device=0, allow_huge_operations=False, _dev=None,
                 _lazy=None, _shape=None, _data_id=None, _source=None):
        if data is None and _dev is None and _lazy is None and _source is None:
            raise ValueError("data is required")
        if data is not None:
            data = np.asarray(data)
            if data.ndim != 3:
                raise ValueError("SpectralCube needs a 3-D (spectral, y, x) array")
        self._data = data                 # host ndarray or None
        self._dev = _dev                  # DeviceArray float32 or None
        # the Pending record of a result that has not been computed yet (pending.py), or None; a bare callable is its run()
        self._lazy = _lazy if _lazy is None or isinstance(_lazy, Pending) else Pending(run=_lazy)
        self._source = _source            # streaming.FitsSource / NdarraySource of an out-of-core cube, or None
        self._shape = tuple(data.shape) if data is not None else (
            tuple(_dev.shape) if _dev is not None else tuple(_shape))
        # (strict=False: a header with celestial keywords the minimal WCS does not model still gives a cube - moments along the
        # spectral axis need no celestial transform; the first celestial USE raises, naming the keyword: wcs.py)
        if wcs is None and header is not None:
            wcs = SimpleWCS(header, strict=False)
        elif wcs is not None and not isinstance(wcs, SimpleWCS):
            wcs = SimpleWCS(wcs, strict=False)
        self._wcs = wcs
        self._header = dict(wcs.header) if wcs is not None else {}
        self._mask = mask
        self._meta = dict(meta or {})
        self._fill_value = fill_value
        if unit is None:
            unit = str(self._header.get("BUNIT", "")).strip()
        self._unit = unit
        self.device = device
        self.allow_huge_operations = allow_huge_operations
        self._mask_cache = None
        self._cen_cache = {}
        # cubes that share the same voxel values (with_mask, with_fill_value) share
        # this token; lazy masks use it to decide whether their predicate may be
        # evaluated by the kernel on the data it is reading
        self._data_id = _data_id if _data_id is not None else _DataToken()
        self._mask64_cache = None
        self._arith = None                # the _ArithPending this cube is the result of (arithmetic operators), or None

    # ---- construction helpers ------------------------------------------------
    @classmethod
    def read(cls, data, header=None, device=0, hdu=None, **kw):
        """``SpectralCube.read``: a FITS file name (streamed to HBM through pinned staging
        buffers and decoded on the device, ``io_fits.load_cube``), or an in-memory array +
        header.  Like the FITS reader (spectral_cube/io/fits.py:171-260) it attaches
        ``LazyMask(np.isfinite)`` and copies ``BUNIT`` into ``meta``."""
        if isinstance(data, (str, os.PathLike)):
            from . import io_fits, streaming
            img = io_fits.find_image(os.fspath(data), hdu)
            fshape = tuple(io_fits.cube_shape(img))
            _lib.require_gpu()
            if 4 * int(np.prod(fshape, dtype=np.int64)) > streaming.hbm_budget(device):
                _warn_if_narrowed(bitpix=img.bitpix)         # the strips are staged as float32
                # larger than the HBM budget: the cube stays in the file and goes through the device in row
                # strips (streaming.py; the role of _moments.py:89-125 / cube_utils.py:277-301 in the reference)
                src = streaming.FitsSource(os.fspath(data), hdu)
                hdr = io_fits.cube_header(img)
                meta = dict(kw.pop("meta", None) or {})
                if "BUNIT" in hdr:
                    meta["BUNIT"] = hdr["BUNIT"]
                table = cls._beams_table_for(os.fspath(data), fshape[0]) if "beams" not in kw else None
                if table is not None:            # a BEAMS extension makes it a varying-resolution cube (io/fits.py:216-228)
                    cls, kw = VaryingResolutionSpectralCube, dict(kw, beam_table=table)
                cube = cls(None, header=hdr, device=device, meta=meta, _source=src, _shape=fshape, **kw)
                finite = M.LazyMask(np.isfinite, cube=cube)
                beam_mask = cube._mask if isinstance(cube, VaryingResolutionSpectralCube) else None
                cube._mask = finite if beam_mask is None else (finite & beam_mask)
                return cube
            wide = img.bitpix in (-64, 32, 64)
            if wide:
                # samples float32 cannot hold: nothing is staged yet - the spectral moments read the image as float64
                # (_device_data64), any other operator as float32 (with a PrecisionWarning), whichever comes first
                dev, hdr = None, io_fits.cube_header(img)
            else:
                dev, hdr = io_fits.load_cube(os.fspath(data), device=device, hdu=hdu)
            meta = dict(kw.pop("meta", None) or {})
            if "BUNIT" in hdr:
                meta["BUNIT"] = hdr["BUNIT"]
            table = cls._beams_table_for(os.fspath(data), fshape[0]) if "beams" not in kw else None
            if table is not None:            # a BEAMS extension makes it a varying-resolution cube (io/fits.py:216-228)
                cls, kw = VaryingResolutionSpectralCube, dict(kw, beam_table=table)
            if wide:
                path_, hdu_ = os.fspath(data), hdu
                cube = cls(None, header=hdr, device=device, meta=meta, _shape=fshape,
                           _lazy=lambda: io_fits.load_cube(path_, device=device, hdu=hdu_)[0], **kw)
                cube._data_id.wide_file = (path_, hdu_, img.bitpix)
            else:
                cube = cls(None, header=hdr, device=device, _dev=dev, meta=meta, **kw)
        else:
            cube = cls(np.asarray(data), header=header, device=device, **kw)
        finite = M.LazyMask(np.isfinite, cube=cube)
        beam_mask = cube._mask if isinstance(cube, VaryingResolutionSpectralCube) else None
        cube._mask = finite if beam_mask is None else (finite & beam_mask)
        return cube

    @staticmethod
    def _beams_table_for(path, nchan):
        """the file's BEAMS table when it has one row per channel (io/fits.py:216-228), else None"""
        from . import io_fits
        table = io_fits.read_beams_table(path)
        if table is not None and len(table["BMAJ"]) != nchan and "POL" in table:
            # full-polarisation tables list every channel once per Stokes plane (cube_utils._split_stokes
            # hands each component its rows); this path reads one plane: keep the first polarisation's rows
            keep = table["POL"] == table["POL"][0]
            table = {k: v[keep] for k, v in table.items()}
        if table is not None and len(table["BMAJ"]) != nchan:
            warnings.warn("BEAMS table with %d rows does not match the %d channels of the cube: ignored"
                          % (len(table["BMAJ"]), nchan), BeamWarning)
            table = None
        return table

    def write(self, filename, overwrite=False, format=None, filled=True):
        """Write the cube as FITS (io/fits.py:262-294; device byte swap, pinned read-back, no host
        arithmetic).  Like the reference's ``hdu`` (dask_spectral_cube.py:1405,1502:
        ``_get_filled_data(fill=self._fill_value)``) what goes to disk is the FILLED data: excluded
        voxels carry the fill value (NaN by default).  ``filled=False`` writes the raw voxels."""
        from . import io_fits
        if self._runs_wide():
            # a float64 cube goes to disk as BITPIX = -64 (the reference writes the array it holds, io/fits.py:262-294)
            path = os.fspath(filename)
            if os.path.exists(path) and not overwrite:
                raise OSError("File %r already exists (use overwrite=True)" % path)
            # the float64 samples explicitly: _host_data() returns the float32-narrowed copy once a float32-only operator has
            # staged one, and the written precision must not depend on the call history
            if self._data is not None and getattr(self._data, "dtype", None) == np.float64:
                data = self._data
            else:
                data = self._device_data64().get()
            if filled and self._mask is not None:
                data = self._mask._filled(data, fill=self._fill_value)
            hdr = {k: v for k, v in self._header.items() if k != "WCSAXES"}
            io_fits.write_fits(path, np.asarray(data, dtype=np.float64), header=hdr)
            return
        plan = self._strip_plan(filled)
        if plan is not None:             # out of core: strips in, operator, strips out (streaming.map_strips / map_slabs)
            from . import streaming
            sink = streaming.FitsSink(os.fspath(filename), self._header, tuple(self._shape), overwrite=overwrite)
            self._run_plan(plan, sink)
            return
        dev = self._device_data()
        if filled and self._mask is not None:
            dev = ops.fill_masked(dev, self._mask_spec(), self._fill_value)
        io_fits.save_cube(os.fspath(filename), dev, header=self._header, overwrite=overwrite)

    def _strip_plan(self, filled=True):
        """(streamed source cube, fn(strip, mask spec, stream) -> result strip, result channels) when this cube is - or
        is a pending operator with an out-of-core route (``Pending.strips`` / ``Pending.slabs``) on - a cube that does not
        fit the HBM budget; None otherwise.  ``_run_plan`` chooses the route."""
        fill = self._fill_value
        if self._stream_source() is not None:
            if filled and self._mask is not None:
                return self, (lambda dev, mspec, stream: ops.fill_masked(dev, mspec, fill, stream)), self._shape[0]
            # (the strip buffer itself is recycled by the pipeline: hand out a copy)
            return self, (lambda dev, mspec, stream: ops.fill_masked(dev, None, fill, stream)), self._shape[0]
        lz = self._lazy
        if self._dev is not None or lz is None or not (lz.slabs or lz.strips) or lz.parent._stream_source() is None:
            return None
        parent, fn = lz.parent, lz.fn
        if filled and self._mask is not None and lz.keeps_mask and self._mask is parent._mask:
            def fn(dev, mspec, stream):      # the parent's mask, evaluated on the parent's voxels (as _mask_spec does)
                from . import streaming
                keep = streaming.original_include(parent, dev, mspec, stream)
                return ops.fill_masked(lz.fn(dev, mspec, stream), keep, fill, stream)
        # (otherwise the data are their own fill: NaN outside a reprojection's footprint, ~isnan(result) of spectral_interpolate)
        return parent, fn, self._shape[0]

    def stream_into(self, out):
        """Out-of-core counterpart of ``filled_data``: fill the float32 (nz, ny, nx) host array / memory map *out* with
        the filled data of this cube, strip by strip (the cube, or the pending per-spaxel operator on a cube, larger than
        the HBM budget).  Returns *out*."""
        from . import streaming
        plan = self._strip_plan(True)
        if plan is None:
            raise ValueError("this cube fits the device: use filled_data")
        self._run_plan(plan, streaming.NdarraySink(out))
        return out

    def _run_plan(self, plan, sink):
        from . import streaming
        src, fn, nz_out = plan
        if self._lazy is not None and self._lazy.slabs and self._dev is None:
            # per-channel operator: slabs of whole planes (a record with both routes too: no halo rows to read twice)
            streaming.map_slabs(src, fn, tuple(self._shape[1:]), sink)
        else:
            streaming.map_strips(src, fn, nz_out, sink, halo=self._strip_halo())

    def _strip_halo(self):
        return self._lazy.halo if (self._lazy is not None and self._dev is None) else 0

    @classmethod
    def from_device(cls, dev, wcs=None, header=None, mask=None, **kw):
        if dev.dtype != np.float32 or len(dev.shape) != 3:
            raise TypeError("device cube must be float32 (nz, ny, nx)")
        return cls(None, wcs=wcs, header=header, mask=mask, device=dev.device, _dev=dev, **kw)

    def _new_cube_with(self, data=None, dev=None, wcs=None, mask=None, meta=None, fill_value=None,
                       lazy=None, shape=None, unit=None, same_data=False):
        return SpectralCube(data, wcs=self._wcs if wcs is None else wcs,
                            mask=self._mask if mask is None else mask,
                            meta=self._meta if meta is None else meta,
                            fill_value=self._fill_value if fill_value is None else fill_value,
                            unit=self._unit if unit is None else unit, device=self.device,
                            allow_huge_operations=self.allow_huge_operations, _dev=dev,
                            _lazy=lazy, _shape=shape, _data_id=self._data_id if same_data else None,
                            _source=self._source if same_data else None)

    # ---- identity used by lazy masks -------------------------------------------
    def _host_data(self):
        if self._data is None:
            if self._data_id.derived64 or (self._data_id.wide_file is not None and self._dev is None and self._wide_resident()):
                # the result of a float64 operator / a resident BITPIX = -64 / 32 / 64 image: float64 on the host as well
                # (what the reference holds, masks.py:225 - host-evaluated mask terms compare these samples)
                self._data = self._device_data64().get()
            else:
                self._data = self._device_data().get()
        return self._data

    def _stream_source(self):
        """streaming source of a cube that is NOT resident and larger than the HBM budget (a FITS file, a memory
        map, a host array), else None.  Such a cube runs its spectral-axis reductions strip by strip
        (streaming.py) and refuses the operators that need it whole."""
        if self._dev is not None or self._lazy is not None:
            return None
        if self._source is not None:
            return self._source
        if self._data is not None:
            from . import streaming
            if 4 * self._data.size > streaming.hbm_budget(self.device):
                self._source = streaming.NdarraySource(self._data)
        return self._source

    def _is_same_data(self, data):
        return getattr(data, "_data_id", None) is self._data_id

    # ---- basic properties --------------------------------------------------------
    @property
    def shape(self):
        return self._shape

    @property
    def ndim(self):
        return 3

    @property
    def size(self):
        return int(np.prod(self._shape, dtype=np.int64))

    @property
    def _is_huge(self):
        return self.size > MEMORY_THRESHOLD                  # cube_utils.is_huge

    @property
    def unit(self):
        return self._unit

    @property
    def wcs(self):
        return self._wcs

    @property
    def header(self):
        return self._header

    @property
    def meta(self):
        return self._meta

    @property
    def mask(self):
        return self._mask

    @property
    def fill_value(self):
        return self._fill_value

    @property
    def spectral_axis(self):
        """world coordinate of every channel, in CUNIT3 (base_class.py:276-281)."""
        return self._wcs.spectral_pix2world(np.arange(self._shape[0]))

    @property
    def spectral_unit(self):
        return self._wcs.spectral_unit if self._wcs is not None else ""

    def with_spectral_unit(self, unit, velocity_convention=None, rest_value=None):
        """The same cube with its spectral axis in another unit OF THE SAME KIND (m/s <-> km/s, Hz <-> GHz, ...:
        spectral_cube.py:1345-1388 for that case; base_class.py `with_spectral_unit`): the WCS is rescaled, the voxels and the mask
        are shared.  Moments then come out in the new unit (tests/test_moments.py:145-155).  Changing the KIND of axis
        (frequency <-> velocity, another velocity convention or rest value) is the reference's spectral_axis machinery, outside
        the dense path: NotImplementedError."""
        unit = str(getattr(unit, "to_string", lambda: unit)()).replace(" ", "")
        if velocity_convention is not None or rest_value is not None:
            raise NotImplementedError("changing the velocity convention / rest value is not built: only same-kind unit changes are")
        try:
            scale = spectral_unit_scale(self.spectral_unit, unit)
        except ValueError as exc:
            raise NotImplementedError(str(exc))
        w = self._wcs
        newwcs = w.with_spectral(w.crval[2] * scale, w.cdelt[2] * w.pc[2, 2] * scale, w.crpix[2], cunit=unit)
        out = self._new_cube_with(data=self._data, dev=self._dev, wcs=newwcs, lazy=self._lazy, shape=self._shape, same_data=True)
        out._mask_cache = self._mask_cache
        return out

    def with_mask(self, mask, inherit_mask=True):
        """spectral_cube.py:1390-1441: AND the new mask with the existing one."""
        if isinstance(mask, np.ndarray):
            np.broadcast_shapes(mask.shape, self._shape)
            mask = M.BooleanArrayMask(mask, self._wcs, shape=self._shape)
        if self._mask is not None and inherit_mask:
            mask = self._mask & mask
        out = self._new_cube_with(data=self._data, dev=self._dev, mask=mask, lazy=self._lazy,
                                  shape=self._shape, same_data=True)
        return out

    def with_mask_dilated(self, structure=None, iterations=1):
        """the cube with its include map dilated on the device (morphology.binary_dilation; scipy.ndimage.binary_dilation
        on get_mask_array() for users of the reference): the new mask replaces the old one"""
        from . import morphology
        return self.with_mask(morphology.binary_dilation(self, structure=structure, iterations=iterations), inherit_mask=False)

    def with_mask_eroded(self, structure=None, iterations=1):
        """the cube with its include map eroded on the device (morphology.binary_erosion)"""
        from . import morphology
        return self.with_mask(morphology.binary_erosion(self, structure=structure, iterations=iterations), inherit_mask=False)

    def with_mask_pruned(self, min_size=64, min_channels=1, structure=None):
        """the cube with the small islands of its include map removed on the device (labelling.remove_small_objects;
        scipy.ndimage.label + np.bincount + find_objects on get_mask_array() for users of the reference): components of
        fewer than *min_size* voxels or spanning fewer than *min_channels* channels leave the mask"""
        from . import labelling
        return self.with_mask(labelling.remove_small_objects(self, min_size=min_size, structure=structure,
                                                             min_channels=min_channels), inherit_mask=False)

    def with_fill_value(self, fill_value):
        out = self._new_cube_with(data=self._data, dev=self._dev, fill_value=fill_value,
                                  lazy=self._lazy, shape=self._shape, same_data=True)
        out._mask_cache = self._mask_cache
        return out

    def _cmp(self, op, value):
        value = getattr(value, "value", value)
        return M.LazyComparisonMask(op, value, cube=self)

    def __gt__(self, value):
        return self._cmp(operator.gt, value)

    def __ge__(self, value):
        return self._cmp(operator.ge, value)

    def __lt__(self, value):
        return self._cmp(operator.lt, value)

    def __le__(self, value):
        return self._cmp(operator.le, value)

    # ---- arithmetic: + - * / ** (spectral_cube.py:2298-2361) -------------------------------------------
    def _pending_arith_steps(self):
        """number of steps of the arithmetic program this cube is the pending result of; None once it has been run (or
        for any other cube).  For tests and for the curious: a following operator extends the program while this is
        below _lib.ARITH_MAX_STEPS."""
        P = self._arith_pending()
        return len(P.steps) if P is not None else None

    def _arith_pending(self):
        P = self._arith
        if P is None or self._dev is not None:
            return None
        if (self._data_id.dev64 is not None) if P.wide else (self._lazy is None):
            return None
        return P

    def _arith_value(self, name, value):
        """the operand of ``cube <name> value`` for a value that is not a cube, checked against the cube's unit as
        _val_to_own_unit does for + and - (spectral_cube.py:2237-2261): (a Python float, a host array in the sample type of
        the path, or a DeviceArray; the operand's unit string or None)"""
        unit = getattr(value, "unit", None)
        unit = None if unit is None else str(unit).strip()
        if name in ("add", "sub"):
            if unit is None:
                if self._unit.strip():
                    raise ValueError("Can only %s cube objects from SpectralCubes or Quantities with a unit attribute."
                                     % ("add" if name == "add" else "subtract"))
            elif unit != self._unit.strip():
                if not hasattr(value, "to"):
                    raise UnitsError("%s is not equivalent to %s" % (self._unit or "dimensionless", unit or "dimensionless"))
                value = value.to(self._unit)
        if isinstance(value, DeviceArray):
            ops.arith_operand_strides(value.shape, self._shape)
            return value, unit
        arr = np.asarray(getattr(value, "value", value))
        if arr.dtype.kind not in "fiub":
            raise TypeError("cube arithmetic takes real numbers and arrays of them (got %s)" % arr.dtype)
        if arr.ndim == 0:
            return float(arr), unit
        ops.arith_operand_strides(arr.shape, self._shape)      # numpy's own ValueError: a (nz,) spectrum does not broadcast
        if self._runs_wide():
            return np.ascontiguousarray(arr, dtype=np.float64), unit
        _warn_if_narrowed(dtype=arr.dtype, stacklevel=5)
        return np.ascontiguousarray(arr, dtype=np.float32), unit

    def _arith_cube(self, name, other):
        """the checks of _cube_on_cube_operation (spectral_cube.py:959-1003); the unit of the result"""
        if tuple(other._shape) != tuple(self._shape):       # (the reference's `assert cube.shape == self.shape`; kept under -O)
            raise AssertionError("cube shapes differ: %s and %s" % (tuple(self._shape), tuple(other._shape)))
        a, b = self._unit.strip(), other._unit.strip()
        if a != b:
            raise UnitsError("%s is not equivalent to %s" % (a or "dimensionless", b or "dimensionless"))
        if (self._wcs is None) != (other._wcs is None) or (self._wcs is not None and dict(self._wcs.header) != dict(other._wcs.header)):
            warnings.warn("Cube WCSs do not match, but their shapes do", WCSMismatchWarning, stacklevel=4)
        if name == "pow":
            if a:
                raise AssertionError("Function %r could not be applied to a pair of simple cube.  The error was: %s ** %s has "
                                     "no unit" % (operator.pow, a, b))
            raise NotImplementedError("cube ** cube is not built")
        return {"mul": _unit_pow(a, 2), "div": ""}.get(name, a)

    def _arith_op(self, name, value):
        if isinstance(value, SpectralCube):
            unit = self._arith_cube(name, value)
            return self._arith_result((name, value, False), unit)
        operand, ounit = self._arith_value(name, value)
        unit = self._unit
        if name == "mul":
            unit = _unit_pow(unit, 2) if (ounit and ounit == unit.strip()) else _unit_mul(unit, ounit)
        elif name == "div":
            unit = _unit_div(unit, ounit)
        elif name == "pow":
            if ounit:
                raise UnitsError("an exponent cannot carry a unit (got %s)" % ounit)
            if not isinstance(operand, float):
                if unit.strip():
                    raise NotImplementedError("an array exponent on a cube with a unit (%s)" % unit)
            else:
                if operand.is_integer():
                    unit = _unit_pow(unit, int(operand)) if operand != 0 else ""
                elif operand == 0.5:
                    unit = unit.strip() + "(1/2)" if unit.strip() else unit
                elif unit.strip():
                    raise NotImplementedError("%s ** %r: only integer exponents and 0.5 are built for a cube with a unit" % (unit, operand))
                if operand in _EXACT_POWERS:
                    name, operand = _EXACT_POWERS[operand]
        return self._arith_result((name, operand, True), unit)

    def _arith_result(self, step, unit):
        """the pending result of one more step: the program of a pending arithmetic result is extended (in a copy) while
        nothing has run it, mask and fill value are the ones it was planned with, it has room, and the right-hand side is
        not itself a pending program; anything else starts a new program on this cube, which is materialised by its
        first use.  New data token, this cube's mask, fill value, WCS, meta and beams."""
        P = self._arith_pending()
        right = step[1]
        right_pending = isinstance(right, SpectralCube) and right._arith_pending() is not None
        if (P is not None and P.mask is self._mask and _same_fill(P.fill, self._fill_value)
                and len(P.steps) < _lib.ARITH_MAX_STEPS and not right_pending):
            pending = _ArithPending(P.source, P.steps + (step,), P.wide, P.mask, P.fill)
        else:
            pending = _ArithPending(self, (step,), self._runs_wide(), self._mask, self._fill_value)
        out = self._result_cube(pending, pending.wide)
        out._unit = unit
        out._arith = pending
        return out

    @warn_slow
    def __add__(self, value):
        return self._arith_op("add", value)

    @warn_slow
    def __sub__(self, value):
        return self._arith_op("sub", value)

    @warn_slow
    def __mul__(self, value):
        return self._arith_op("mul", value)

    @warn_slow
    def __truediv__(self, value):
        return self._arith_op("div", value)

    @warn_slow
    def __pow__(self, value):
        return self._arith_op("pow", value)

    @warn_slow
    def __floordiv__(self, value):
        raise NotImplementedError("Floor-division (division with truncation) is not supported.")

    # ---- data access -----------------------------------------------------------------
    def _device_data(self):
        """float32 DeviceArray of the cube values (uploads / materialises lazily)."""
        if self._dev is None:
            self._note_narrowed()
            if self._lazy is not None:
                self._dev = self._lazy()
                self._lazy = None
            else:
                _lib.require_gpu()
                if self._stream_source() is not None:
                    from . import streaming
                    nbytes = 4 * int(np.prod(self._shape, dtype=np.int64))
                    raise streaming.HugeCubeError(
                        "this operation needs the whole cube in HBM: %.2f GiB against a budget of %.2f GiB (SPC_HBM_BUDGET). "
                        "Out-of-core cubes stream moments, argmax / argmin, the nan-reductions and median / percentile / mad_std along any "
                        "axis and over the pair (1, 2), statistics(), and spectral_smooth / spatial_smooth / spectral_interpolate / sigma_clip_spectrally / reproject "
                        "(celestial) into write(), stream_into() or a following moment"
                        % (nbytes / 2**30, streaming.hbm_budget(self.device) / 2**30))
                self._dev = DeviceArray.from_numpy(self._data, self.device, dtype=np.float32)
        return self._dev

    # ---- wide sources (float64 arrays, BITPIX = -64 / 32 / 64 images): the spectral moments in their own precision ------
    def _is_wide(self):
        if self._data_id.wide_file is not None or self._data_id.derived64:
            return True
        return self._data is not None and _is_wide_dtype(self._data.dtype)

    def _note_narrowed(self, stacklevel=4):
        """PrecisionWarning, once per source, when a wide source is about to be used as float32"""
        tok = self._data_id
        if tok.warned or not self._is_wide():
            return
        tok.warned = True
        if tok.wide_file is not None:
            _warn_if_narrowed(bitpix=tok.wide_file[2], stacklevel=stacklevel)
        elif tok.derived64:
            _warn_if_narrowed(dtype=np.float64, stacklevel=stacklevel)
        else:
            _warn_if_narrowed(dtype=self._data.dtype, stacklevel=stacklevel)

    def _wide_resident(self):
        """True when the spectral moments of this cube run on its float64 samples: a wide source whose values this cube
        still is (no pending operator) and whose float64 copy fits the HBM budget"""
        if self._data_id.derived64:
            return True
        if not self._is_wide() or (self._lazy is not None and self._data_id.wide_file is None):
            return False
        if self._data_id.dev64 is not None:
            return True
        from . import streaming
        return 8 * int(np.prod(self._shape, dtype=np.int64)) <= streaming.hbm_budget(self.device)

    def _device_data64(self):
        """float64 DeviceArray of a wide source (uploaded / decoded from the FITS image once, shared by the cubes that share
        the data)"""
        tok = self._data_id
        if tok.dev64 is None:
            _lib.require_gpu()
            if tok.lazy64 is not None:
                tok.dev64 = tok.lazy64()
                tok.lazy64 = None
            elif tok.wide_file is not None:
                from . import io_fits
                path, hdu, _ = tok.wide_file
                tok.dev64 = io_fits.load_cube(path, device=self.device, hdu=hdu, dtype=np.float64)[0]
            else:
                tok.dev64 = DeviceArray.from_numpy(self._data, self.device, dtype=np.float64)
        return tok.dev64

    def _lower_mask(self, wide):
        """the mask tree lowered for the float32 kernels or (*wide*) the float64 ones: thresholds in float64, host-evaluated
        terms on the float64 samples.  The uint8 array term stays resident in HBM."""
        view = _WideView if wide else (lambda cube: cube)
        owner = M.foreign_owner(self._mask) if self._mask is not None else None
        if isinstance(self._mask, M.DeviceBooleanMask) and tuple(self._mask.shape) == tuple(self._shape):
            # computed on the device (downsample_axis, a cut): the kernels read its uint8 array where it is
            return ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, self._mask.device_array())
        if (owner is not None and not owner._is_same_data(self) and tuple(owner._shape) == tuple(self._shape)
                and (not wide or getattr(owner, "_wide_resident", lambda: False)())
                and self._mask._device_terms(view(owner)) is not None):
            # every lazy term belongs to ANOTHER cube's data (a smoothed cube keeps its parent's mask): evaluate it there,
            # on the device, on the samples of this path - no host copy of either cube
            flags, lo, hi, arr = M.lower_mask(self._mask, view(owner), self._shape)
            darr = DeviceArray.from_numpy(arr, self.device) if arr is not None else None
            inc = ops.mask_include(owner._device_data64() if wide else owner._device_data(), ops.MaskSpec(flags, lo, hi, darr),
                                   nan_excluded=M.contains(self._mask, M.NotNaNMask))
            return ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, inc)
        if self._mask is not None:
            terms = self._mask._device_terms(view(self))
            if ((terms is None or (terms[3] is not None and 0 in np.asarray(terms[3]).strides and np.size(terms[3]) > 1))
                    and self._stream_source() is None):
                # not an AND of device terms (a map / spectrum / cube threshold, | ^ ~, == !=, terms on several cubes), or
                # an array term smaller than the cube: compiled and evaluated once on the device (ops.mask_eval) - no
                # host copy of any cube, no broadcast upload.  What compile_mask cannot express takes the host form below
                prog = M.compile_mask(self._mask, view(self), self._shape, wide)
                if prog is not None:
                    prog.slots = [c._device_data64() if wide else c._device_data() for c in prog.slots]
                    inc = ops.mask_eval(prog, self._shape, self.device, np.float64 if wide else np.float32)
                    return ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, inc)
        flags, lo, hi, arr = M.lower_mask(self._mask, view(self), self._shape)
        darr = DeviceArray.from_numpy(arr, self.device) if arr is not None else None
        return ops.MaskSpec(flags, lo, hi, darr)

    def _mask_spec(self):
        """the mask lowered for the float32 kernels, once"""
        if self._mask_cache is None:
            self._mask_cache = self._lower_mask(False)
        return self._mask_cache

    def _mask_spec64(self):
        """the mask lowered for the float64 kernels, once (both lowerings of one mask may be live)"""
        if self._mask64_cache is None:
            self._mask64_cache = self._lower_mask(True)
        return self._mask64_cache

    def _runs_wide(self):
        """True when a cube -> cube operator of this cube runs on float64 samples: a wide cube that is resident (or fits).
        Decided without a device where it can be (a float32 cube never asks); no device at all = the float32 plan, which
        raises when it is run"""
        if not self._is_wide():
            return False
        try:
            return self._stream_source() is None and self._wide_resident()
        except _lib.HipLibraryError:
            return False

    def _operand(self, wide=None):
        """(device data, lowered mask, view) for the path this cube's operators run on (*wide*: a decision of
        ``_runs_wide()`` taken earlier): the float64 samples, the float64 lowering and ``_WideView(self)``, or the float32
        ones and the cube itself.  The view is what ``_nan_term_dropped`` and the mask lowering evaluate against."""
        if self._runs_wide() if wide is None else wide:
            return self._device_data64(), self._mask_spec64(), _WideView(self)
        return self._device_data(), self._mask_spec(), self

    def _result_cube(self, run, wide, shape=None, wcs=None, mask=None, plain=False):
        """the result cube of a cube -> cube operator, pending until first used: run() gives its DeviceArray, a float64 one
        when *wide*.  *plain*: a SpectralCube whatever the subclass (no beams)."""
        if wide:
            return self._new_wide_cube(run, shape=shape, wcs=wcs, mask=mask, plain=plain)
        make = (lambda **kw: SpectralCube._new_cube_with(self, **kw)) if plain else self._new_cube_with
        return make(lazy=Pending(run=run), shape=tuple(shape) if shape is not None else self._shape, wcs=wcs, mask=mask)

    def _derived(self, fn, **kw):
        """_result_cube of *fn*(data, mask, view) applied to ``_operand()``, on the path decided now"""
        wide = self._runs_wide()
        return self._result_cube(lambda: fn(*self._operand(wide)), wide, **kw)

    def _new_wide_cube(self, fn64, shape=None, wcs=None, mask=None, plain=False):
        """the result of a float64 operator on this (wide, resident) cube: a cube whose values exist as a float64 DeviceArray
        (pending until first used; the Dask class keeps the chunk dtype, dask_spectral_cube.py:829).  Its spectral moments,
        reductions, statistics() and further smoothing / interpolation run in float64; an operator without a float64 form
        narrows it with a PrecisionWarning, like a float64 source."""
        # the narrowing record holds the result's DATA TOKEN, never the cube: out._lazy -> record -> out was a reference cycle
        # that kept a dropped float64 cube (8 B / voxel of HBM) and its parent alive until a generation-2 collection
        tokens = []
        narrow = Pending(run=lambda: ops.narrow_f64(_token_dev64(tokens[0])))
        make = (lambda **kw: SpectralCube._new_cube_with(self, **kw)) if plain else self._new_cube_with      # plain: not the subclass's (beams)
        out = make(lazy=narrow, shape=tuple(shape) if shape is not None else self._shape, wcs=wcs, mask=mask)
        out._data_id.lazy64 = fn64
        out._data_id.derived64 = True
        tokens.append(out._data_id)
        return out

    @property
    def filled_data(self):
        """host copy with excluded voxels replaced by fill_value
        (base_class.py:389-417 / masks.py:197-237)."""
        d = self._host_data()
        if self._mask is None:
            return d
        return self._mask._filled(d, fill=self._fill_value)

    unitless_filled_data = filled_data

    def get_mask_array(self):
        """the include map of the cube's mask as a host bool array, all True without a mask (spectral_cube.py:552).  Of a
        resident cube it is evaluated on the device (the lowered mask as it is, ops.mask_include or ops.mask_eval) and
        only the map comes down; an out-of-core cube evaluates the tree on the host."""
        if self._mask is None:
            return np.ones(self._shape, dtype=bool)
        if self._stream_source() is not None:
            return np.array(np.broadcast_to(self._mask.include(data=self._host_data()), self._shape), dtype=bool)
        data, mspec, view = self._operand()
        nan_ex = _nan_term_dropped(self, view)
        if mspec.flags == _lib.MASK_ARRAY and not nan_ex:
            return mspec.array.get().view(bool)
        return ops.mask_include(data, mspec, nan_excluded=nan_ex).get().view(bool)

    @property
    def unmasked_data(self):
        return self._host_data()

    # ---- coordinates fed to the kernels -------------------
    def _pix_size_slice(self, axis):
        return pix_size(self._wcs, axis)

    def _pix_cen_axis(self, axis):
        if axis not in self._cen_cache:
            if axis == 0:
                spec = self.spectral_axis
                self._cen_cache[0] = spec - spec[0]          # spectral_cube.py:1473-1475
            else:
                y, x = pix_cen_spatial(self._wcs, self._shape)
                self._cen_cache[1], self._cen_cache[2] = y, x
        return self._cen_cache[axis]

    # ---- moments -----------------------------------------------------------------------
    def _moment_device(self, want, fused_kernel=None):
        nz = self._shape[0]
        cen = self._pix_cen_axis(0)
        cref = cen[nz // 2]
        spec0 = self.spectral_axis[0]
        d_cen = DeviceArray.from_numpy(cen - cref, self.device)
        dv = self._pix_size_slice(0)
        if fused_kernel is None and self._wide_resident():
            # a float64 source: its own precision (the reference's maps are float64 sums of float64 samples)
            return ops.moments_f64(self._device_data64(), d_cen, dv=dv, m1_add=cref + spec0, mask=self._mask_spec64(), want=want)
        if fused_kernel is None and self._is_wide():
            self._note_narrowed()
        if fused_kernel is not None and fused_kernel[0]._stream_source() is not None:
            from . import streaming                     # out-of-core parent: the fused kernels, strip by strip
            try:
                return streaming.moments(fused_kernel[0], want, d_cen, dv, cref + spec0, kernel=fused_kernel[1], cen_host=cen - cref)
            except _lib.HipUnsupported:
                # a kernel wider than the rings on a strip that holds an invalid sample (or an extremum requested): the
                # resident path materialises the smoothed cube; here the smoothed STRIP is materialised, then reduced.
                # The maps are rebuilt from the first strip on (a strip's rows are written whole, nothing is accumulated).
                lz = self._lazy
                return streaming.moments(lz.parent, want, d_cen, dv, cref + spec0, pre=lz.fn, halo=lz.halo)
        if fused_kernel is None and self._stream_source() is not None:
            from . import streaming
            return streaming.moments(self, want, d_cen, dv, cref + spec0)
        lz = self._lazy
        if (fused_kernel is None and self._dev is None and lz is not None and lz.strips and lz.parent._stream_source() is not None
                and lz.parent._mask is self._mask and tuple(lz.parent._shape) == tuple(self._shape)):
            # out-of-core parent and a pending cube -> cube operator that keeps the parent's mask (spatial_smooth outside the
            # all-valid algebraic case: strip + halo rows, the strip's own rows reduced; sigma_clip_spectrally; a
            # spectral_smooth too wide to fuse): operator and reduction strip by strip
            from . import streaming
            return streaming.moments(lz.parent, want, d_cen, dv, cref + spec0, pre=lz.fn, halo=lz.halo)
        if fused_kernel is not None:
            parent, karr = fused_kernel
            try:
                return ops.spectral_conv_moments(parent._device_data(), karr, d_cen, dv=dv,
                                                 m1_add=cref + spec0, mask=parent._mask_spec(), want=want,
                                                 cen_host=cen - cref)
            except _lib.HipUnsupported:
                pass        # e.g. a wide kernel on a cube with invalid samples: materialise, then reduce
        return ops.moments(self._device_data(), d_cen, dv=dv, m1_add=cref + spec0,
                           mask=self._mask_spec(), want=want)

    def _fusable(self):
        """pending spectral_smooth whose parent shares this cube's mask object:
        smooth -> moment can run fused (dask_spectral_cube.py:836-840 keeps the
        original mask, so the semantics are identical)."""
        lz = self._lazy
        if (lz is not None and lz.op == "spectral_smooth" and self._dev is None
                and lz.parent._mask is self._mask and lz.fusable):
            return (lz.parent, lz.kernel)
        return None

    def _moments_of_spatially_smoothed(self, want):
        """spatial_smooth -> moment without smoothing nz planes.  With every voxel valid astropy's
        convolution is linear (zero fill, division by the kernel sum: dask_spectral_cube.py:
        962-993), so it commutes with the sums along the spectral axis (:1083-1104):
        S_n' = conv2d(S_n).  One pass over the UNSMOOTHED cube gives S0, S1, S2 (float64), three
        small map convolutions give the moments of the smoothed cube.  Returns None when the
        shortcut does not apply (mask terms other than isfinite, any invalid voxel, S0 == 0) -
        the caller then materialises the smoothed cube."""
        lz = self._lazy
        if not (lz is not None and lz.op == "spatial_smooth" and self._dev is None
                and lz.parent._mask is self._mask):
            return None
        parent = lz.parent
        spec = parent._mask_spec()
        split_ok = lz.arithmetic != "f32"        # (asked for float32 multiply-adds: the fused forms are split-form kernels)
        if not split_ok and spec.array is not None:
            return None
        if tuple(want) == ("m0",) and parent._stream_source() is None and (spec.array is not None or (spec.flags & ~_lib.MASK_FINITE) == 0):
            fused = self._fused_masked_smooth_moment0(parent, spec, lz.kernel)
            if fused is not None:
                return {"m0": fused}
        elif (set(want) <= {"m0", "m1", "m2"} and parent._stream_source() is None and spec.array is not None
              and self._prefer_fused_higher_moments()):
            fused = self._fused_masked_smooth_moments(parent, spec, lz.kernel, want)
            if fused is not None:
                return fused
        if spec.array is not None or (spec.flags & ~_lib.MASK_FINITE):
            return None
        nz = self._shape[0]
        higher = ("m1" in want) or ("m2" in want)
        # moment 0 alone: the kernel scales by the channel width (m0 = dv * S0), the convolved map is the result
        r = parent._moment_device((("s0", "mu", "m2") if higher else ("m0",)) + ("nvalid",))
        if not higher:
            # every spaxel has nz valid voxels, and no NaN / Inf sum anywhere (cannot happen when the mask keeps finite samples
            # only): both checked on the device - four bytes come back instead of the count map and a host reduction of the
            # result (17.5 -> 14 ms at C4)
            c0d = ops.map_conv2d(r["m0"], lz.kernel)             # the sums never leave the device
            if ops.map_check(r["nvalid"], nz, None if (spec.flags & _lib.MASK_FINITE) else c0d):
                return None
            return {"m0": c0d.get()}
        if ops.map_check(r["nvalid"], nz):
            return None
        # S1 = mu * S0 and S2 = (m2 + mu^2) * S0 about the reference channel are smoothed like S0; the moments of the
        # smoothed cube are their ratios.  All of it on the device: only the requested maps come back.  A spaxel whose
        # spectrum sums to zero (0/0 in mu), a zero smoothed sum or a non-finite sample shows up as a non-finite value
        # in the result: not this path.
        s0, mu, m2 = r["s0"], r["mu"], r["m2"]
        c0d = ops.map_conv2d(s0, lz.kernel)
        c1d = ops.map_conv2d(ops.map_arith(_lib.MAP_MUL, mu, s0), lz.kernel)
        cen = self._pix_cen_axis(0)
        cref = cen[nz // 2]
        out = {}
        if "m1" in want:
            out["m1"] = ops.map_arith(_lib.MAP_DIV_ADD, c1d, c0d, s=cref + self.spectral_axis[0]).get()
        if "m2" in want:
            c2d = ops.map_conv2d(ops.map_arith(_lib.MAP_SECOND_MOMENT_SUM, m2, mu, s0), lz.kernel)
            mupd = ops.map_arith(_lib.MAP_DIV_ADD, c1d, c0d, s=0.0)
            out["m2"] = ops.map_arith(_lib.MAP_DIV_SUB_SQ, c2d, c0d, mupd).get()
        if "m0" in want:
            out["m0"] = self._pix_size_slice(0) * c0d.get()
        if not all(np.isfinite(m.sum()) for m in out.values()):
            return None
        return out

    def _prefer_fused_higher_moments(self):
        """Measured at 4096 x 2048^2 + uint8 mask (round 6): the fused moments 0 / 1 / 2 take 55 ms (eight channel-parallel
        waves per block, bands of 96 rows; round 5: 71 ms with 16-row wave regions) against 39 + 14 ms for smoothing into a
        second cube (whole-column march) and reducing that.  So the fused form remains for cubes whose smoothed copy does not
        fit beside them in HBM (SPC_FUSED_SMOOTH_MOMENTS=1 / 0 forces / forbids it)."""
        env = os.environ.get("SPC_FUSED_SMOOTH_MOMENTS")
        if env is not None:
            return env == "1"
        from .device import device_info
        nz, ny, nx = self._shape
        return device_info(self.device)["free_mem"] < 1.05 * 4 * nz * ny * nx

    def _fused_masked_smooth_moments(self, parent, spec, kernel2d, want):
        """masked spatial_smooth -> moment 1 / 2 (and 0) in ONE kernel, like _fused_masked_smooth_moment0: the split form of
        spc_spatial_conv_sep_mfma_moments_f32 keeps sum v, sum c v, sum c^2 v of the smoothed values per spaxel
        (dask_spectral_cube.py:962-993 then :1083-1104).  None when the kernel does not take the case."""
        nz = self._shape[0]
        cen = self._pix_cen_axis(0)
        cref = cen[nz // 2]
        d_cen = DeviceArray.from_numpy(cen - cref, self.device)
        try:
            _, maps = ops.spatial_conv_mfma_moments(parent._device_data(), kernel2d, d_cen, dv=self._pix_size_slice(0),
                                                    m1_add=cref + self.spectral_axis[0], mask=spec, want=tuple(want))
        except _lib.HipUnsupported:
            return None
        return {k: v.get() for k, v in maps.items()}

    def _fused_masked_smooth_moment0(self, parent, spec, kernel2d):
        """masked spatial_smooth -> moment0 in ONE kernel that never writes the smoothed cube (the lazy Dask graph of the
        reference does not materialise it either: dask_spectral_cube.py:962-993 then :1083-1104): numerator and denominator of
        the NaN-aware convolution on the matrix cores, moment sums in registers / LDS (spc_spatial_conv_sep_mfma_f32).
        None when the kernel does not take the case (more than 29 taps per axis, non-separable or negative kernels, mask
        terms other than the array / isfinite): the caller materialises.  Only tried where it pays: a mask ARRAY (an
        all-valid cube takes the algebraic path below, which is cheaper still)."""
        if spec.array is None:
            return None
        try:
            _, m0 = ops.spatial_conv_mfma(parent._device_data(), kernel2d, mask=spec, want_cube=False, want_m0=True,
                                          dv=self._pix_size_slice(0))
        except _lib.HipUnsupported:
            return None
        return m0.get()

    def moment(self, order=0, axis=0, how="auto", **kwargs):
        """Compute moments along an axis (spectral_cube.py:1614-1720;
        dask_spectral_cube.py:1031-1132).  ``how`` is accepted for interface
        compatibility; every strategy maps onto the same one-pass HIP kernel."""
        if how not in ("auto", "cube", "slice", "ray"):
            raise ValueError("Invalid how. Must be in %r" % sorted(["auto", "cube", "slice", "ray"]))
        if axis not in (0, 1, 2):
            raise ValueError("Cubes have 3 axes.")
        order = int(order)
        if order < 0:
            raise ValueError("order must be >= 0")
        if axis == 0 and order == 2:
            warnings.warn(_VARIANCE_MSG, VarianceWarning)
        if axis == 0:
            key = {0: "m0", 1: "m1", 2: "m2"}.get(order)
            alg = self._moments_of_spatially_smoothed((key,)) if key is not None else None
            if alg is not None:
                out = alg[key]
            elif key is not None:
                out = self._moment_device((key,), self._fusable())[key].get()
            else:
                r = self._moment_device(("mu", "s0"))
                cen = self._pix_cen_axis(0)
                cref = cen[self._shape[0] // 2]
                d_cen = DeviceArray.from_numpy(cen - cref, self.device)
                if self._wide_resident():
                    out = ops.moment_order_f64(self._device_data64(), d_cen, order, r["mu"], r["s0"], mask=self._mask_spec64()).get()
                else:
                    out = ops.moment_order(self._device_data(), d_cen, order, r["mu"], r["s0"], mask=self._mask_spec()).get()
                # dv cancels: sum(I dv (c-M1)^N) / sum(I dv)
            axunit = self.spectral_unit
        else:
            cen = self._pix_cen_axis(axis)
            d_cen = DeviceArray.from_numpy(cen, self.device)
            size = self._pix_size_slice(axis)
            key = {0: "m0", 1: "m1", 2: "m2"}.get(order)
            if self._stream_source() is not None:
                # out of core: the image planes are whole in a slab of channels, the (nz, nx) / (nz, ny) map grows slab by slab
                from . import streaming
                width, f64 = self._shape[2 if axis == 1 else 1], {"m0": np.float64, "m1": np.float64, "m2": np.float64, "o": np.float64}
                first = key or "m1"
                mu = streaming.slab_maps(self, lambda dev, ms, st, o, z0, z1: ops.moments_spatial(
                    dev, d_cen, axis, size, mask=ms, want=(first,), stream=st, out=o), (first,), width, f64)[first]
                if key is None:
                    mu = streaming.slab_maps(self, lambda dev, ms, st, o, z0, z1: ops.moment_order_spatial(
                        dev, d_cen, axis, order, streaming._rows_view(mu, z0, z1), mask=ms, stream=st, out=o["o"]), ("o",), width, f64)["o"]
                out = mu.get()
            elif key is None:          # order > 2: second pass about the first moment (_moments.py:185-193)
                mu = ops.moments_spatial(self._device_data(), d_cen, axis, size, mask=self._mask_spec(),
                                         want=("m1",))["m1"]
                out = ops.moment_order_spatial(self._device_data(), d_cen, axis, order, mu,
                                               mask=self._mask_spec()).get()
            else:
                out = ops.moments_spatial(self._device_data(), d_cen, axis, size, mask=self._mask_spec(),
                                          want=(key,))[key].get()
            axunit = self._wcs.cunit[2 - axis] if self._wcs is not None else ""
        if order == 0:
            unit = _unit_mul(self._unit, axunit)
        else:
            unit = _unit_pow(axunit, max(order, 1))
        meta = {"moment_order": order, "moment_axis": axis}
        meta.update(self._meta)
        new_wcs = self._wcs.drop_spectral() if (self._wcs is not None and axis == 0) else None
        beam = None if isinstance(self, VaryingResolutionSpectralCube) else self.beam
        return Projection(out, unit=unit, wcs=new_wcs, meta=meta, beam=beam, device=self.device)

    def moment0(self, axis=0, how="auto"):
        return self.moment(axis=axis, order=0, how=how)

    def moment1(self, axis=0, how="auto"):
        return self.moment(axis=axis, order=1, how=how)

    def moment2(self, axis=0, how="auto"):
        return self.moment(axis=axis, order=2, how=how)

    def moments012(self, keep_on_device=False):
        """moment 0, 1 and 2 along the spectral axis from ONE pass over the cube
        (the reference needs three graph executions, dask_spectral_cube.py
        :1090,1097,1104)."""
        r = self._moment_device(("m0", "m1", "m2"), self._fusable())
        if keep_on_device:
            return r["m0"], r["m1"], r["m2"]
        return tuple(self._wrap0(r[k].get(), o) for o, k in enumerate(("m0", "m1", "m2")))

    def _wrap0(self, arr, order):
        unit = _unit_mul(self._unit, self.spectral_unit) if order == 0 else _unit_pow(self.spectral_unit, max(order, 1))
        meta = {"moment_order": order, "moment_axis": 0}
        meta.update(self._meta)
        beam = None if isinstance(self, VaryingResolutionSpectralCube) else self.beam
        return Projection(arr, unit=unit, wcs=self._wcs.drop_spectral() if self._wcs is not None else None,
                          meta=meta, beam=beam, device=self.device)

    def linewidth_sigma(self, how="auto"):
        """sqrt(moment 2), no VarianceWarning (spectral_cube.py:1746-1753)."""
        with np.errstate(invalid="ignore"), warnings.catch_warnings():
            warnings.simplefilter("ignore", VarianceWarning)
            m2 = self.moment(order=2, axis=0, how=how)
            out = np.sqrt(m2)
        return Projection(out, unit=self.spectral_unit, wcs=m2.wcs, meta=m2.meta)

    def linewidth_fwhm(self, how="auto"):
        """linewidth_sigma * sqrt(8 ln 2) (spectral_cube.py:1755-1763)."""
        s = self.linewidth_sigma(how=how)
        return Projection(np.asarray(s) * SIGMA2FWHM, unit=s.unit, wcs=s.wcs, meta=s.meta)

    def _extremum(self, key, axis, how):
        if axis == 0:
            return self._moment_device((key,))[key].get()
        if axis in (1, 2):
            if self._stream_source() is not None:
                from . import streaming
                return streaming.slab_maps(self, lambda dev, ms, st, o, z0, z1: ops.argextrema_axis(dev, axis, mask=ms, want=(key,), stream=st, out=o),
                                           (key,), self._shape[2 if axis == 1 else 1], {key: np.int64})[key].get()
            return ops.argextrema_axis(self._device_data(), axis, mask=self._mask_spec(), want=(key,))[key].get()
        if axis is not None:
            raise ValueError("axis must be None, 0, 1 or 2")
        # whole cube: flat C-order index of the first extreme voxel, from the per-spaxel extreme and
        # its first channel (one pass of the fused kernel)
        vkey = "vmax" if key == "argmax" else "vmin"
        r = self._moment_device((key, vkey))
        val, idx = r[vkey].get().astype(np.float64), r[key].get()
        fill = -np.inf if key == "argmax" else np.inf
        val = np.where(np.isnan(val), fill, val)               # rays without an included sample
        best = val.max() if key == "argmax" else val.min()
        if best == fill:
            return np.int64(0)
        nz, ny, nx = self._shape
        yy, xx = np.nonzero(val == best)
        return np.int64(np.min(idx[yy, xx] * (ny * nx) + yy * nx + xx))

    def argmax(self, axis=None, how="auto", **kwargs):
        """index of the maximum along *axis* (spectral_cube.py:793-804: nanargmax of the data filled
        with -inf); first index on ties, 0 for fully masked rays; int64.  ``axis=None``: flat index
        into the cube."""
        return self._extremum("argmax", axis, how)

    def argmin(self, axis=None, how="auto", **kwargs):
        """spectral_cube.py:806-819 (fill +inf)"""
        return self._extremum("argmin", axis, how)

    # ---- statistics / nan-reductions -----------------------------
    def _reduce(self, op, axis, ddof=0):
        """sum / mean / std / max / min (dask_spectral_cube.py:641-767): sum / mean / max / min come
        out of ONE pass over the cube (the reference: one pass per statistic); std takes two,
        like the reference's nanstd (_reduce_std)."""
        axis = self._reduced_axes(axis)
        if op == "std":
            return self._reduce_std(axis, ddof)
        need = {"sum": ("count", "sum"), "mean": ("count", "sum"), "max": ("count", "max"), "min": ("count", "min")}[op]
        if axis is None:
            if self._stream_source() is not None:
                from . import streaming
                st = streaming.statistics(self)
            else:
                data, mask, _ = self._operand()
                st = ops.stats_global(data, mask=mask)
            n = st["npts"]
            vals = {"count": np.float64(n), "sum": np.float64(st["sum"]), "max": np.float64(st["max"]), "min": np.float64(st["min"])}
        elif isinstance(axis, tuple):
            # two axes at once (e.g. the mean spectrum, axis=(1, 2)): one device pass removes the first
            # of them, the small (5 statistics x one map) remainder is finished on the host
            axes = list(axis)
            if axes == [1, 2] and not (self._stream_source() is None and self._wide_resident()):
                # per channel (spectra): one dedicated pass, nz records (a float64 cube: its rows on the device, the rest here)
                if self._stream_source() is not None:
                    from . import streaming
                    vals = streaming.stats_planes(self)
                else:
                    vals = ops.stats_planes(self._device_data(), mask=self._mask_spec())
                axis = (1, 2)
                return self._finish_reduce(op, vals, axis, ddof)
            first, second = axes[1], axes[0]            # drop the higher axis on the device, the lower one here
            r = self._stats_axis_maps(first, need)
            part = {k: r[k].get().astype(np.float64) for k in need}
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", RuntimeWarning)
                vals = {"count": part["count"].sum(axis=second)}
                for k in need:
                    if k == "sum":
                        vals[k] = np.nansum(part[k], axis=second)
                    elif k == "max":
                        vals[k] = np.nanmax(np.where(part["count"] > 0, part[k], -np.inf), axis=second)
                    elif k == "min":
                        vals[k] = np.nanmin(np.where(part["count"] > 0, part[k], np.inf), axis=second)
        else:
            r = self._stats_axis_maps(axis, need)
            vals = {k: r[k].get().astype(np.float64) for k in need}
        return self._finish_reduce(op, vals, axis, ddof)

    @staticmethod
    def _reduced_axes(axis):
        """None (all three), one of 0 / 1 / 2, or a sorted pair of them"""
        if isinstance(axis, (tuple, list)):
            axes = sorted(set(int(a) for a in axis))
            if any(a not in (0, 1, 2) for a in axes) or not axes:
                raise ValueError("axis must be None, 0, 1, 2 or a tuple of these")
            return None if len(axes) == 3 else axes[0] if len(axes) == 1 else tuple(axes)
        if axis is not None and axis not in (0, 1, 2):
            raise ValueError("axis must be None, 0, 1 or 2")
        return axis

    def _reduce_std(self, axis, ddof):
        """nanstd is two-pass in the reference (the mean, then the deviations), and so is this: per ray along ONE axis the
        device gives count, sum and m2 = sum (x - mean)^2 about the ray's own mean (a second read, csrc/spc_stats_m2.hip);
        a second axis, or all three, merges those rays here (distributed.merge_m2).  sumsq / n - mean^2 - the formula of
        statistics()['sigma'], which is the reference's there - loses (mean / sigma)^2 ulps: noise or 0 on a pedestal."""
        from .distributed import merge_m2
        need = ("count", "sum", "m2")
        src = self._stream_source()
        if src is not None and self._is_wide():
            from . import streaming
            if streaming.wide_source(self) is None:
                self._note_narrowed()              # a wide FITS image streams as float32: std of THOSE samples, said once
        if axis is None and src is None:
            # resident, the whole cube: ONE mean, known after the single pass of statistics(); the second pass sums the
            # deviations about it per ray of the longest axis, the rays are added here - nothing to merge
            data, mask, _ = self._operand()
            st = ops.stats_global(data, mask=mask)
            n = st["npts"]
            q = np.nan
            if n > 0:
                first = max((0, 1, 2), key=lambda a: (self._shape[a], a))
                s1, s2 = ops.stats_dev_axis(data, first, st["sum"] / n, mask=mask)
                s1, s2 = float(s1.get().sum()), float(s2.get().sum())
                q = max(s2 - s1 * s1 / n, 0.0) if s2 == s2 else np.nan
            vals = {"count": np.float64(n), "sum": np.float64(st["sum"]), "m2": np.float64(q)}
        elif axis is None or isinstance(axis, tuple):
            # the device reduces the LONGEST of the axes (the fewest rays come back: what is merged here is the cube over
            # that axis - (4096, 4096, 4) along x would leave 16 M rows of 4 samples), the host the rest
            over = (0, 1, 2) if axis is None else axis
            first = max(over, key=lambda a: (self._shape[a], a))
            r = self._stats_axis_maps(first, need, wide=True)
            if axis is None:
                second = None
            else:
                other = over[0] if over[1] == first else over[1]
                second = other - (1 if other > first else 0)           # its place in the map that has lost `first`
            n, s, q = merge_m2(*(r[k].get() for k in need), axis=second)
            vals = {"count": n, "sum": s, "m2": q}
        else:
            r = self._stats_axis_maps(axis, need, wide=True)
            vals = {k: r[k].get().astype(np.float64) for k in need}
        return self._finish_reduce("std", vals, axis, ddof)

    def _stats_axis_maps(self, axis, need, wide=False):
        if self._stream_source() is not None:          # out of core: strips (axis 0) or slabs of planes (axis 1 / 2)
            from . import streaming                    # (*wide*: float64 strips of a float64 host array - std asks for them)
            return streaming.stats_axis(self, axis, need, wide=wide)
        data, mask, _ = self._operand()
        return ops.stats_axis(data, axis, mask=mask, want=need)

    def _finish_reduce(self, op, vals, axis, ddof=0):
        n = vals["count"]
        with np.errstate(invalid="ignore", divide="ignore"):
            if op == "sum":
                out = np.where(n > 0, vals["sum"], np.nan)            # nansum_allbadtonan
            elif op == "mean":
                out = np.where(n > 0, vals["sum"] / n, np.nan)
            elif op == "std":
                out = np.where((n > 0) & (n - ddof > 0), np.sqrt(vals["m2"] / (n - ddof)), np.nan)
            else:
                out = np.where(n > 0, vals[op], np.nan)
        if axis is None:
            return float(out)
        wcs = self._wcs.drop_spectral() if (axis == 0 and self._wcs is not None) else None
        return Projection(out, unit=self._unit, wcs=wcs, meta=dict(self._meta))

    def sum(self, axis=None, how="auto", **kwargs):
        """nansum_allbadtonan of the masked data (dask_spectral_cube.py:641-647)."""
        return self._reduce("sum", axis)

    def mean(self, axis=None, how="auto", **kwargs):
        """nanmean (dask_spectral_cube.py:649-655)."""
        return self._reduce("mean", axis)

    def std(self, axis=None, how="auto", ddof=0, **kwargs):
        """nanstd with ddof (dask_spectral_cube.py:695-709)."""
        return self._reduce("std", axis, ddof=ddof)

    def max(self, axis=None, how="auto", **kwargs):
        """nanmax (dask_spectral_cube.py:733-739)."""
        return self._reduce("max", axis)

    def min(self, axis=None, how="auto", **kwargs):
        """nanmin (dask_spectral_cube.py:741-747)."""
        return self._reduce("min", axis)

    def _order_stat(self, q, axis, what, center=None, scale=1.0):
        if axis not in (0, 1, 2):
            raise ValueError("axis must be None, 0, 1 or 2")
        if axis in (0, 1) and self._shape[axis] <= 4096 and self._runs_wide():
            # a float64 cube: sorted rays of float64 keys (spc_percentile_axis0_f64), a float64 map
            # (longer rays have no float64 kernel: they go the float32 way below, with a PrecisionWarning)
            d64, ms, _ = self._operand(True)
            if axis == 1:
                d64, ms = d64.swap01(), ms.swap01()
            return ops.percentile_axis0(d64, q, mask=ms, center=center, scale=scale)
        if axis in (1, 2) and self._stream_source() is not None:
            # out of core: the rays along y / x are whole in a slab of channels; row z of the (nz, nx) / (nz, ny) map per slab row
            from . import streaming

            def one(dev, ms, st, o, z0, z1):
                cen = streaming._rows_view(center, z0, z1) if center is not None else None
                if axis == 1:
                    ops.percentile_axis0(dev.swap01(), q, mask=ms.swap01() if ms is not None else None, center=cen, scale=scale, stream=st, out=o["q"])
                    return
                try:
                    ops.percentile_axis2(dev, q, mask=ms, center=cen, scale=scale, stream=st, out=o["q"])
                except _lib.HipUnsupported:
                    flipped = ops.fill_masked_transposed(dev, ms, np.nan, stream=st)
                    ops.percentile_axis0(flipped.swap01(), q, center=cen, scale=scale, stream=st, out=o["q"])
                    st.synchronize()
            return streaming.slab_maps(self, one, ("q",), self._shape[2 if axis == 1 else 1], {"q": np.float32})["q"]
        if axis == 1:            # rays along y: the same kernels on a view with the first two axes exchanged
            return ops.percentile_axis0(self._device_data().swap01(), q, mask=self._mask_spec().swap01(),
                                        center=center, scale=scale)
        if axis == 2:            # rays along x: the rows themselves (contiguous samples, lanes walk along the ray) ...
            try:
                return ops.percentile_axis2(self._device_data(), q, mask=self._mask_spec(), center=center, scale=scale)
            except _lib.HipUnsupported:
                pass             # ... or, for rows of more than 4096 samples, a NaN-filled transposed copy, then as along y
            flipped = ops.fill_masked_transposed(self._device_data(), self._mask_spec(), np.nan)
            return ops.percentile_axis0(flipped.swap01(), q, center=center, scale=scale)
        if axis != 0:
            raise ValueError("axis must be None, 0, 1 or 2")
        if self._stream_source() is not None:       # out of core: per spaxel, so strip by strip
            from . import streaming
            return streaming.percentile_axis0(self, q, center=center, scale=scale)
        return ops.percentile_axis0(self._device_data(), q, mask=self._mask_spec(), center=center, scale=scale)

    def _order_wcs(self, axis):
        return self._wcs.drop_spectral() if (axis == 0 and self._wcs is not None) else None

    def _order_stat_global(self, q, center=None):
        """whole-cube statistic (axis=None): float32 like numpy's result for a float32 cube"""
        return np.float32(ops.percentile_global(self._device_data(), q, mask=self._mask_spec(), center=center))

    def _order_stat_pair(self, q, pair, center=None, scale=1.0, operand=None):
        """the statistic over two axes (spectral_cube.py:730-764, 1172-1257 with a two-axis tuple): a float32 DeviceArray
        with one value per index of the third axis (ops.percentile_global's keep mode: per-group histograms, the descent of
        every group on the device).  *center*: the device result of an earlier call (mad_std).  A float64 cube goes the way
        median(axis=None) goes: its float32 samples, with a PrecisionWarning."""
        if operand is None:
            operand = self._pair_operand(pair)
        if operand is None:
            # out of core: every plane is whole in a slab of channels; the slab's results are rows z0:z1 of the spectrum
            from . import streaming
            self._note_narrowed()                  # (a wide source streams as float32: said once, as a resident one says it)
            return streaming.percentile_planes(self, q, center=center, scale=scale)
        data, mask, keep = operand
        return ops.percentile_global(data, q, mask=mask, center=center, keep=keep, scale=scale)

    def _pair_operand(self, pair):
        """(device data, mask, kept axis) that ops.percentile_global's keep mode reduces for *pair* - mad_std's two calls share
        it; None for the planes of a streamed cube, which go slab by slab"""
        if pair == (1, 2) and self._stream_source() is not None:
            return None
        data, mask = self._device_data(), self._mask_spec()
        if pair == (0, 1):
            # one value per x: the NaN-filled copy with the spatial axes exchanged has x as its row index.  No mask goes
            # with it: NaN is never a sample, and an infinity the mask included stays one (as in numpy's nanmedian)
            return ops.fill_masked_transposed(data, mask, np.nan), None, 1
        return data, mask, 0 if pair == (1, 2) else 1

    def _pair_projection(self, dev):
        """a statistic over two axes as mean(axis=pair) returns it"""
        return Projection(dev.get(), unit=self._unit, wcs=None, meta=dict(self._meta))

    def median(self, axis=None, **kwargs):
        """nanmedian along an axis, over two axes or of the whole cube (dask_spectral_cube.py:657-671;
        spectral_cube.py:1172-1213 for a pair): digit descent on order-preserving keys, no sort (csrc/spc_select.hip,
        spc_select_groups.hip)."""
        axis = self._reduced_axes(axis)
        if axis is None:
            return float(self._order_stat_global(50.0))
        if isinstance(axis, tuple):
            return self._pair_projection(self._order_stat_pair(50.0, axis))
        return Projection(self._order_stat(50.0, axis, "median").get(), unit=self._unit,
                          wcs=self._order_wcs(axis), meta=dict(self._meta))

    def percentile(self, q, axis=None, **kwargs):
        """np.nanpercentile along an axis, over two axes or of the whole cube (dask_spectral_cube.py:673-693;
        spectral_cube.py:1215-1257 for a pair)."""
        axis = self._reduced_axes(axis)
        if axis is None:
            return float(self._order_stat_global(float(q)))
        if isinstance(axis, tuple):
            return self._pair_projection(self._order_stat_pair(float(q), axis))
        return Projection(self._order_stat(float(q), axis, "percentile").get(), unit=self._unit,
                          wcs=self._order_wcs(axis), meta=dict(self._meta))

    def mad_std(self, axis=None, ignore_nan=True, **kwargs):
        """astropy mad_std along an axis, over two axes - axis=(1, 2): the noise of every channel - or of the whole cube
        (dask_spectral_cube.py:711-731; spectral_cube.py:730-764): two selections (median, then median of |x - median|)
        without leaving the device."""
        axis = self._reduced_axes(axis)
        if axis is None:
            med = self._order_stat_global(50.0)
            return float(np.float32(self._order_stat_global(50.0, center=med) * np.float32(ops.MAD_TO_STD)))
        if isinstance(axis, tuple):
            operand = self._pair_operand(axis)
            med = self._order_stat_pair(50.0, axis, operand=operand)
            return self._pair_projection(self._order_stat_pair(50.0, axis, center=med, scale=ops.MAD_TO_STD, operand=operand))
        med = self._order_stat(50.0, axis, "mad_std")
        out = self._order_stat(50.0, axis, "mad_std", center=med, scale=ops.MAD_TO_STD)
        return Projection(out.get(), unit=self._unit, wcs=self._order_wcs(axis), meta=dict(self._meta))

    def sigma_clip_spectrally(self, threshold, **kwargs):
        """astropy's sigma clipper along the spectral axis, clipped (and excluded) values -> NaN
        (dask_spectral_cube.py:851-878); kwargs: maxiters, cenfunc ('median' | 'mean'), stdfunc
        ('std' | 'mad_std'), sigma_lower, sigma_upper.  Runs on the device (ops.sigma_clip_axis0)."""
        allowed = {"maxiters", "cenfunc", "stdfunc", "sigma_lower", "sigma_upper"}
        extra = set(kwargs) - allowed
        if extra:
            raise NotImplementedError("sigma_clip options not built on the device path: %s" % sorted(extra))
        if self._stream_source() is not None:
            # out of core: a pending operator; write() / stream_into() run it strip by strip
            parent, sig = self, float(threshold)
            lazy = Pending(lambda dev, mspec, stream: ops.sigma_clip_axis0(dev, sigma=sig, mask=mspec, stream=stream, **kwargs),
                           op="sigma_clip_spectrally", parent=parent, strips=True, keeps_mask=True)
            return self._new_cube_with(lazy=lazy, shape=self._shape)
        if self._shape[0] <= 4096 and self._runs_wide():
            parent, kw = self, dict(kwargs)
            return self._new_wide_cube(lambda: ops.sigma_clip_axis0_f64(parent._device_data64(), sigma=float(threshold),
                                                                        mask=parent._mask_spec64(), **kw))
        dev = ops.sigma_clip_axis0(self._device_data(), sigma=float(threshold), mask=self._mask_spec(), **kwargs)
        return self._new_cube_with(dev=dev)

    def statistics(self):
        """global basic statistics in ONE pass (dask_spectral_cube.py:769-814): npts, min, max,
        sum, sumsq, mean, sigma (the reference's textbook formula), rms."""
        if self._stream_source() is not None:
            from . import streaming
            return streaming.statistics(self)           # per-strip records, combined (same formulae)
        data, mask, _ = self._operand()
        st = ops.stats_global(data, mask=mask)
        n = st["npts"]
        with np.errstate(invalid="ignore", divide="ignore"):
            st["mean"] = st["sum"] / n if n else np.nan
            st["sigma"] = float(np.sqrt((st["sumsq"] - st["sum"] ** 2 / n) / (n - 1))) if n > 1 else np.nan
            st["rms"] = float(np.sqrt(st["sumsq"] / n)) if n else np.nan
        return st

    # ---- downsampling ------------------------------------------------------------------------
    def downsample_axis(self, factor, axis, estimator=np.nanmean, truncate=False, use_memmap=True, progressbar=True):
        """Block-downsample the cube by an integer *factor* along *axis* (spectral_cube.py:3421-3557, the in-memory form
        ``use_memmap=False``; ``use_memmap`` / ``progressbar`` are accepted and ignored).  Every run of *factor* samples of
        the FILLED data (masked voxels -> fill_value, NaN by default: ``with_fill_value(0)`` counts them as zeros)
        becomes ``estimator(run)``; the new mask is a boolean array, True where any voxel of the run is included.  A
        last run shorter than *factor* is dropped when *truncate*, otherwise padded with NaN like the reference pads it:
        the nan-estimators skip the padding, ``np.mean`` / ``np.sum`` / ``np.max`` / ``np.min`` give NaN there.
        The WCS follows ``wcs_utils.slice_wcs`` with a step (``SimpleWCS.downsampled``): output pixel k is the centre of
        its parent block.

        Estimators (by identity): np.nanmean (default), np.nansum, np.nanmax, np.nanmin, np.mean, np.sum, np.max /
        np.amax, np.min / np.amin; any other raises NotImplementedError (there is no CPU path).

        dtype, by design: a float32 cube gives float32 (sums and means are carried in float64 and rounded once), a
        float64 cube float64 throughout - the reference's dtype depends on its code path (float32 unpadded, float64
        padded or memory-mapped).

        The result is pending like ``spectral_smooth``: shape, wcs and header need no device; data and mask come from
        one kernel pass on first use, and stay in HBM.  A parent larger than the HBM budget streams through the device
        (row strips along the spectral axis, slabs of planes along y / x) into a resident result, which must fit."""
        if isinstance(factor, (bool, np.bool_)) or not isinstance(factor, (int, np.integer)) or factor < 1:
            raise ValueError("factor must be an integer >= 1 (got %r)" % (factor,))
        factor = int(factor)
        if isinstance(axis, (bool, np.bool_)) or not isinstance(axis, (int, np.integer)) or axis not in (0, 1, 2):
            raise ValueError("axis must be 0, 1 or 2 (got %r)" % (axis,))
        axis = int(axis)
        est = _ds_estimator(estimator)
        shape = ops.downsample_shape(self._shape, axis, factor, truncate)
        if shape[axis] < 1:
            raise ValueError("downsampling %d samples along axis %d by %d with truncate=True leaves an empty cube"
                             % (self._shape[axis], axis, factor))
        newwcs = self._wcs.downsampled(axis, factor, shape) if self._wcs is not None else None
        parent, fill, wide = self, self._fill_value, self._runs_wide()
        if not wide:
            try:
                streamed = self._stream_source() is not None
            except _lib.HipLibraryError:
                streamed = False
            if streamed:
                _check_downsample_fits(self, shape)

        def run():
            # (a ~isnan mask of the parent's own data lowers to no term: the kernel is told to exclude NaN samples, which the
            # reference fills with fill_value and leaves out of the new mask)
            if not wide and parent._stream_source() is not None:
                return _downsample_streamed(parent, axis, factor, truncate, est, fill, shape)
            data, mask, view = parent._operand(wide)
            return ops.downsample(data, axis, factor, truncate, est, fill, mask=mask, nan_excluded=_nan_term_dropped(parent, view))

        result = _Once(run)
        mask = M.DeviceBooleanMask(lambda: result()[1], wcs=newwcs, shape=shape)
        return self._result_cube(lambda: result()[0], wide, shape=shape, wcs=newwcs, mask=mask)

    # ---- cutting: slicing, spectral_slab, subcube, minimal_subcube ---------------------------------
    def _normalize_view(self, view):
        """*view* as a tuple of three entries, slices kept, integers normalised to 0 .. n - 1 (spectral_cube.py:1310-1316)"""
        if not isinstance(view, tuple):
            view = (view,)
        if len(view) > 3:
            raise IndexError("Too many indices")
        view = view + (slice(None),) * (3 - len(view))
        out = []
        for axis, (s, n) in enumerate(zip(view, self._shape)):
            if isinstance(s, slice):
                out.append(s)
            elif isinstance(s, (int, np.integer)) and not isinstance(s, (bool, np.bool_)):
                k = int(s)
                if not -n <= k < n:
                    raise IndexError("index %d is out of bounds for the %s with size %d" % (k, _AXIS_NAMES[axis], n))
                out.append(k + n if k < 0 else k)
            else:
                raise IndexError("a cube is indexed with integers and slices (got %r)" % (s,))
        return tuple(out)

    def __getitem__(self, view):
        """``cube[view]`` (spectral_cube.py:1308-1381): an integer or slice, or a tuple of up to three.

        Slices only: a new cube that owns compact memory (never a view of the parent's), its unmasked data equal to
        ``parent_data[view]`` bit for bit, its mask to ``parent.mask.include()[view]``, the WCS from ``SimpleWCS.sliced``;
        ``meta['slice']`` records the view.  The result is pending like ``downsample_axis``: one gather pass makes data and
        mask on first use, and the mask stays in HBM.  A parent larger than the HBM budget streams only the channel and
        row range the view touches; the cut itself must fit the budget (HugeCubeError).
        An empty selection (``cube[5:5]``) raises ValueError - the reference returns a (0, ...) cube.

        ``cube[k]`` / ``cube[k, ys, xs]``: the FILLED channel as a 2-D Projection with the celestial WCS, its header
        carrying CRVAL3 / CDELT3 / CUNIT3 of that channel.  ``cube[zs, j, i]``: the filled spectrum as a 1-D Projection
        whose wcs is the spectral axis alone.  Integers that include the spectral axis and another:
        NotImplementedError as the reference; one integer on y or x (a position-velocity slice): NotImplementedError
        (``pv_slice(y=j)`` / ``pv_slice(x=i)`` give it)."""
        view = self._normalize_view(view)
        meta = dict(self._meta)
        slice_data = [(s.start, s.stop, s.step) if isinstance(s, slice) else s for s in view]
        meta["slice"] = list(meta.get("slice", [])) + [slice_data]
        ints = [axis for axis, s in enumerate(view) if not isinstance(s, slice)]
        if not ints:
            return self._cut(view, meta)
        if len(ints) > 1:
            if 0 in ints:
                raise NotImplementedError("1D slices along non-spectral axes are not yet implemented.")
            return self._spectrum(view, meta)
        if ints[0] != 0:
            raise NotImplementedError("a single integer index on a spatial axis (a position-velocity slice) is not built "
                                      "as an index: cube.pv_slice(y=j) / cube.pv_slice(x=i) give it as a Projection")
        return self._channel(view, meta)

    def _view_spec(self, view):
        """(start, step, length) per axis of three slices; an empty selection raises (the kernels have no zero-size form)"""
        spec = ops.normalize_view(view, self._shape)
        for axis, (start, step, n) in enumerate(spec):
            if n < 1:
                raise ValueError("the view %r selects nothing along the %s of a cube of shape %s"
                                 % (view[axis], _AXIS_NAMES[axis], self._shape))
        return spec

    def _gather(self, spec, shape, filled=False):
        """(data, include or None) of the view on the device, in the cube's dtype path"""
        starts, steps = [a[0] for a in spec], [a[1] for a in spec]
        has_mask = self._mask is not None
        wide = self._runs_wide()
        if not wide and self._stream_source() is not None:
            data, inc = _subcube_streamed(self, spec, shape, has_mask)
            if filled and has_mask:
                data = ops.fill_masked(data, ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, inc), self._fill_value)
            return data, inc
        data, mask, view = self._operand(wide)
        return ops.subcube(data, starts, steps, shape, mask=mask if has_mask else None, want_mask=has_mask, filled=filled,
                           fill=self._fill_value, nan_excluded=_nan_term_dropped(self, view))

    def _cut_finish(self, new, view):
        return new

    def _cut(self, view, meta):
        spec = self._view_spec(view)
        shape = tuple(a[2] for a in spec)
        newwcs = self._wcs.sliced(view, self._shape) if self._wcs is not None else None
        if newwcs is None:
            for axis, (start, step, n) in enumerate(spec):
                if step < 0 and (axis != 0 or step != -1):
                    raise NotImplementedError("Haven't dealt with resampling & reversing.")
        parent, wide, has_mask = self, self._runs_wide(), self._mask is not None
        if not wide:
            try:
                streamed = self._stream_source() is not None
            except _lib.HipLibraryError:
                streamed = False
            if streamed:
                _check_cut_fits(self, shape, has_mask)
        result = _Once(lambda: parent._gather(spec, shape))
        mask = M.DeviceBooleanMask(lambda: result()[1], wcs=newwcs, shape=shape) if has_mask else None
        new = self._result_cube(lambda: result()[0], wide, shape=shape, wcs=newwcs, mask=mask, plain=True)
        new._meta = meta
        return self._cut_finish(new, view)

    def _channel_beam(self, k):
        return self.beam

    def _spectrum_meta(self, meta, view):
        return meta

    def _channel(self, view, meta):
        """cube[k, ys, xs]: the filled channel as a 2-D Projection (spectral_cube.py:1351-1370)"""
        k = view[0]
        full = (slice(k, k + 1),) + tuple(view[1:])
        spec = self._view_spec(full)
        shape = tuple(a[2] for a in spec)
        w2, header = None, {}
        if self._wcs is not None:
            w2 = self._wcs.sliced(full, self._shape).drop_spectral()
            header = dict(w2.header)
            header["CRVAL3"] = float(self._wcs.spectral_pix2world(k))
            header["CDELT3"] = float(self._wcs.cdelt[2] * self._wcs.pc[2, 2])
            header["CUNIT3"] = self.spectral_unit
        data, _ = self._gather(spec, shape, filled=True)
        beam = self._channel_beam(k)
        if beam is not None:
            meta = dict(meta, beam=beam)
        return Projection(data.get()[0], unit=self._unit, wcs=w2, meta=meta, beam=beam, device=self.device, header=header)

    def _spectrum(self, view, meta):
        """cube[zs, j, i]: the filled spectrum as a 1-D Projection whose wcs is the spectral axis alone (:1331-1349)"""
        j, i = view[1], view[2]
        full = (view[0], slice(j, j + 1), slice(i, i + 1))
        spec = self._view_spec(full)
        shape = tuple(a[2] for a in spec)
        w1 = self._wcs.sliced(full, self._shape).spectral_only() if self._wcs is not None else None
        data, _ = self._gather(spec, shape, filled=True)
        meta = self._spectrum_meta(meta, view)
        return Projection(data.get()[:, 0, 0], unit=self._unit, wcs=w1, meta=meta, device=self.device)

    def pv_slice(self, path=None, y=None, x=None, **kwargs):
        """The position-velocity diagram along *path* (a ``pvextract.Path`` or a list of ``(x, y)`` pixel positions) as a
        Projection of shape ``(nz, npts)``: ``pvextract.extract_pv_slice(self, path, **kwargs)`` (spacing, order - 1 by
        default, not pvextractor's 3 -, respect_nan, nlines), computed on the device; stands in for ``to_pvextractor()``
        (spectral_cube.py:2506-2513).  ``pv_slice(y=j)`` / ``pv_slice(x=i)``: the axis-aligned cut, an exact copy of
        ``filled_data[:, j, :]`` / ``filled_data[:, :, i]`` (negative indices as in numpy)."""
        from . import pvextract
        if path is None:
            if kwargs:
                raise TypeError("pv_slice(y=...) / pv_slice(x=...) take no other keyword (got %s)" % sorted(kwargs))
            return pvextract.axis_cut(self, y=y, x=x)
        if y is not None or x is not None:
            raise ValueError("give a path, or one of y= and x=, not both")
        return pvextract.extract_pv_slice(self, path, **kwargs)

    def fit_baseline(self, order=1, fit_mask=None, channels=None, exclude=None):
        """A ``baseline.BaselineFit``: a polynomial of degree *order* (0 ... 5) fitted on the device to the line-free
        channels of every spectrum - ``baseline.fit_baseline(self, ...)``, which documents *fit_mask* (anything with_mask
        accepts, ``~signal``), *channels* and *exclude* (``(lo, hi)`` spectral ranges left out).  Stands in for a polyfit per
        spectrum through ``apply_function_parallel_spectral`` (spectral_cube.py:3103)."""
        from . import baseline
        return baseline.fit_baseline(self, order=order, fit_mask=fit_mask, channels=channels, exclude=exclude)

    def subtract_baseline(self, order=1, fit_mask=None, channels=None, exclude=None):
        """The cube minus the polynomial baseline of ``fit_baseline(...)``, subtracted in every voxel; it keeps this cube's
        mask, WCS, unit, meta and beam(s)."""
        from . import baseline
        return baseline.subtract_baseline(self, order=order, fit_mask=fit_mask, channels=channels, exclude=exclude)

    def _spectral_value(self, value):
        """a spectral coordinate in the cube's spectral unit: plain numbers are taken to be in it, an object with
        ``.value`` and ``.unit`` is converted (same kind of unit only, spectral_cube.py:1794-1819)"""
        if not hasattr(value, "unit"):
            return float(value)
        unit = value.unit
        unit = str(getattr(unit, "to_string", lambda: unit)()).replace(" ", "")
        try:
            return float(value.value) * spectral_unit_scale(unit, self.spectral_unit)
        except ValueError:
            from .wcs import _SPECTRAL_SI
            mine = _SPECTRAL_SI.get(self.spectral_unit, (None,))[0]
            theirs = _SPECTRAL_SI.get(unit, (None,))[0]
            if theirs in ("freq", "length") and mine == "speed":
                raise UnitsError("Spectral axis is in velocity units and 'value' is in frequency-equivalent units - use "
                                 "SpectralCube.with_spectral_unit first to convert the cube to frequency-equivalent units, or "
                                 "search for a velocity instead")
            if theirs == "speed" and mine in ("freq", "length"):
                raise UnitsError("Spectral axis is in frequency-equivalent units and 'value' is in velocity units - use "
                                 "SpectralCube.with_spectral_unit first to convert the cube to frequency-equivalent units, or "
                                 "search for a velocity instead")
            if theirs in ("freq", "length") and mine in ("freq", "length"):
                raise NotImplementedError("converting between frequency and wavelength is a change of spectral representation: "
                                          "not built, give the value in %s" % self.spectral_unit)
            if theirs is not None:
                raise UnitsError("Unexpected spectral axis units: {0}".format(self.spectral_unit))
            raise UnitsError("'value' should be in frequency equivalent or velocity units (got {0})".format(unit))

    def closest_spectral_channel(self, value):
        """index of the channel closest to the spectral coordinate *value* (spectral_cube.py:1780-1821)"""
        return int(np.argmin(np.abs(self.spectral_axis - self._spectral_value(value))))

    def spectral_slab(self, lo, hi):
        """the cube between two spectral coordinates, both ends included (spectral_cube.py:1823-1879); limits in either
        order, plain numbers in the cube's spectral unit"""
        ilo, ihi = self.closest_spectral_channel(lo), self.closest_spectral_channel(hi)
        if ilo == ihi:
            warnings.warn("The maxmimum and minimum spectral channel in the spectral"
                          "slab are identical; this indicates that one or both are "
                          "likely incorrect and/or out of range.", SliceWarning)
        if ilo > ihi:
            ilo, ihi = ihi, ilo
        return self[ilo:ihi + 1]

    def subcube(self, xlo="min", xhi="max", ylo="min", yhi="max", zlo="min", zhi="max", rest_value=None):
        """Extract a sub-cube spatially and spectrally (spectral_cube.py:1947-2036).  Limits are 'min' / 'max', pixel
        integers, or - *zlo* / *zhi* only - spectral coordinates (objects with ``.unit``; the upper one is end-inclusive).
        Spatial limits as world coordinates (the reference's joint corner solve): NotImplementedError."""
        nz, ny, nx = self._shape
        given = {"xlo": xlo, "xhi": xhi, "ylo": ylo, "yhi": yhi, "zlo": zlo, "zhi": zhi}
        ends = {"xlo": 0, "xhi": nx, "ylo": 0, "yhi": ny, "zlo": 0, "zhi": nz}
        lim, united = {}, []
        for key, v in given.items():
            if isinstance(v, str):
                if v != ("min" if key.endswith("lo") else "max"):
                    raise ValueError("%s must be %r, a pixel index or a quantity (got %r)" % (key, "min" if key.endswith("lo") else "max", v))
                lim[key] = ends[key]
            elif hasattr(v, "unit"):
                if key[0] != "z":
                    raise NotImplementedError("spatial limits given as world coordinates are not built: give %s in pixels" % key)
                try:
                    lim[key] = self.closest_spectral_channel(v)
                except UnitsError:
                    raise UnitsError("Spectral units are not equivalent to the spectral slice.  Use `.with_spectral_unit` to "
                                     "convert to equivalent units first")
                united.append(key)
            elif isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_)):
                lim[key] = int(v)
            else:
                raise ValueError("%s must be 'min' / 'max', a pixel index or (spectral limits) a quantity (got %r)" % (key, v))
        if lim["zhi"] < lim["zlo"]:
            lim["zlo"], lim["zhi"] = lim["zhi"], lim["zlo"]
        if "zhi" in united:
            lim["zhi"] += 1
        for xx in "zyx":
            if lim[xx + "hi"] == lim[xx + "lo"]:
                raise ValueError("The slice in the {0} direction will remove "
                                 "all elements.  If you want a single-channel "
                                 "slice, you need a different approach.".format(xx))
        return self[tuple(slice(lim[xx + "lo"], lim[xx + "hi"]) for xx in "zyx")]

    def subcube_slices_from_mask(self, region_mask, spatial_only=False):
        """the slices of the smallest subcube that holds every voxel *region_mask* includes (spectral_cube.py:1901-1945):
        a boolean ndarray broadcastable to the cube, or a mask object, lowered against this cube's data and reduced to
        its bounding box on the device.  ``(slice(0),) * 3`` when nothing is included."""
        if isinstance(region_mask, np.ndarray):
            ok = region_mask.ndim <= 3 and all(a in (1, b) for a, b in zip(region_mask.shape[::-1], self._shape[::-1]))
            if not ok:
                raise ValueError("Mask shape does not match cube shape.")
            region_mask = M.BooleanArrayMask(region_mask, self._wcs, shape=self._shape)
        if region_mask is self._mask:
            probe = self
        else:
            if self._lazy is not None and not self._runs_wide():
                self._device_data()                     # a pending cube is materialised once and shared with the probe
            probe = SpectralCube._new_cube_with(self, data=self._data, dev=self._dev, mask=region_mask, lazy=self._lazy,
                                                shape=self._shape, same_data=True)
        wide = probe._runs_wide()
        if not wide and probe._stream_source() is not None:
            box = _bbox_streamed(probe)
        else:
            data, mask, view = probe._operand(wide)
            box = ops.mask_bbox(data, mask=mask, nan_excluded=_nan_term_dropped(probe, view))
        if box is None:
            return (slice(0),) * 3
        slices = tuple(slice(lo, hi + 1) for lo, hi in box)
        if spatial_only:
            slices = (slice(None),) + slices[1:]
        return slices

    def subcube_from_mask(self, region_mask):
        """the minimal subcube that encloses *region_mask* (spectral_cube.py:1890-1899)"""
        return self[self.subcube_slices_from_mask(region_mask)]

    def minimal_subcube(self, spatial_only=False):
        """the minimum enclosing subcube where the mask is valid (spectral_cube.py:1881-1888); a cube without a mask: a
        copy of itself.  With nothing included the empty selection raises ValueError."""
        if self._mask is None:
            return self[:]
        return self[self.subcube_slices_from_mask(self._mask, spatial_only=spatial_only)]

    def mask_channels(self, goodchannels):
        """mask out whole channels: *goodchannels* a 1-D boolean array with one entry per channel (spectral_cube.py:3394)"""
        goodchannels = np.asarray(goodchannels, dtype="bool")
        if goodchannels.ndim != 1:
            raise ValueError("goodchannels mask must be one-dimensional")
        if goodchannels.size != self._shape[0]:
            raise ValueError("goodchannels must have a length equal to the "
                             "cube's spectral dimension.")
        return self.with_mask(goodchannels[:, None, None])

    # ---- smoothing ---------------------------------------------------------------------------
    def spectral_smooth(self, kernel, convolve=None, **kwargs):
        """Smooth along the spectral axis; the mask is left unchanged
        (dask_spectral_cube.py:880-917).  Lazy like the Dask class: a following
        ``moment`` runs fused with the stencil, any other access materialises."""
        karr = kernel_array(kernel, 1)
        _check_convolve(convolve)
        parent = self
        if self._runs_wide():
            # a float64 cube stays float64 (the Dask class keeps the chunk dtype, dask_spectral_cube.py:829) and is resident:
            # none of what the float32 record below carries for a following moment or an out-of-core parent applies
            return self._derived(lambda data, mask, view: ops.spectral_conv(data, karr, mask=mask))
        lazy = Pending(lambda dev, mspec, stream: ops.spectral_conv(dev, karr, mask=mspec, stream=stream),
                       op="spectral_smooth", parent=parent, strips=True, keeps_mask=True, kernel=karr, fusable=True)
        return self._new_cube_with(lazy=lazy, shape=self._shape)

    def spatial_smooth(self, kernel, convolve=None, raise_error_jybm=True, arithmetic=None, **kwargs):
        """Smooth every channel with a 2-D kernel (dask_spectral_cube.py:962-993).  Extra keyword
        arguments are accepted and not used - exactly what the Dask class does with them (its
        convolve_wrapper only receives ``kernel``, :990-993; spectral_smooth likewise, :912-917).
        ``arithmetic`` (this package's own): None, "f16-split" or "f32" - which arithmetic the MASKED separable stencil of a
        float32 cube runs in (ops.masked_spatial_arithmetic; DESIGN section 5: both are inside the 1e-5 contract, the
        reference computes in float64)."""
        self.check_jybeam_smoothing(raise_error_jybm=raise_error_jybm)
        karr = kernel_array(kernel, 2)
        _check_convolve(convolve)
        if arithmetic is not None and arithmetic not in ops.MASKED_SPATIAL_ARITHMETIC:
            raise ValueError("arithmetic must be one of %r, got %r" % (ops.MASKED_SPATIAL_ARITHMETIC, arithmetic))
        parent = self
        if self._runs_wide():        # (resident: no strip / slab form; the float64 stencils have one arithmetic)
            return self._derived(lambda data, mask, view: ops.spatial_conv(data, karr, mask=mask))
        # both routes: cube -> cube (write / stream_into) of an out-of-core parent goes in slabs of whole planes - no halo rows
        # to read twice (29 x 29 taps, 8 GiB host array: 8.3 GB/s each way in halo strips, the link's rate in slabs); the
        # strips, with the halo rows they need from their neighbours, remain for a following moment, which needs whole spaxels
        lazy = Pending(lambda dev, mspec, stream: ops.spatial_conv(dev, karr, mask=mspec, stream=stream, arithmetic=arithmetic),
                       op="spatial_smooth", parent=parent, strips=True, slabs=True, halo=karr.shape[0] // 2, keeps_mask=True,
                       kernel=karr, arithmetic=arithmetic)
        return self._new_cube_with(lazy=lazy, shape=self._shape)

    # ---- median and rank filters -----------------------------------------------------------------
    def _rank_filtered(self, sizes, axis_lengths, filter, kwargs):
        """the pending result of a rank filter with a window of *sizes* samples ((ksize,) along the spectral axis, (ky, kx)
        per plane) on the FILLED data; mask, fill value, WCS, unit, meta and beams stay the parent's"""
        rank, mode, cval = _rank_filter_options(filter, int(np.prod(sizes)), kwargs)
        spectral = len(sizes) == 1
        limit = _lib.RANK_FILTER_MAX_KSIZE if spectral else _lib.RANK_FILTER_MAX_KSIZE_SPATIAL
        for k, n in zip(sizes, axis_lengths):
            if k < 1:
                raise ValueError("ksize must be at least 1 (got %d)" % k)
            if k > limit:
                raise ValueError("ksize %d is above the built limit of %d %s" % (k, limit, "channels" if spectral else "pixels per axis"))
            if k // 2 > n:
                raise ValueError("ksize %d reaches more than one axis length (%d samples) past the edge: the limit is "
                                 "ksize // 2 <= %d (scipy's own versions disagree beyond it)" % (k, n, n))
        parent, fill = self, self._fill_value
        fn = ops.rank_filter_axis0 if spectral else ops.rank_filter_plane

        def run(data, mask, view, stream=None):
            return fn(data, *sizes, rank, mode=mode, cval=cval, fill=fill, mask=mask, stream=stream,
                      nan_excluded=_nan_term_dropped(parent, view))
        if self._runs_wide():            # (resident, float64 throughout)
            return self._derived(run)
        # (of an out-of-core parent: strips of whole spaxels along the spectral axis, slabs of whole planes per plane)
        lazy = Pending(lambda dev, mspec, stream: run(dev, mspec, parent, stream), op="spectral_filter" if spectral else "spatial_filter",
                       parent=parent, strips=spectral, slabs=not spectral, keeps_mask=True)
        return self._new_cube_with(lazy=lazy, shape=self._shape)

    def spectral_filter(self, ksize, filter, **kwargs):
        """Filter every spectrum with one of scipy.ndimage's rank filters over a window of *ksize* channels
        (spectral_cube.py:2844-2868, dask_spectral_cube.py:926-960).  *filter*: ``median_filter``, ``minimum_filter``,
        ``maximum_filter``, ``percentile_filter`` (with ``percentile=``) or ``rank_filter`` (with ``rank=``) - the scipy
        function itself (recognised by its name; scipy is never imported here) or that name as a string; anything else
        raises NotImplementedError.  Keywords ``mode`` ('reflect', the default, 'constant', 'nearest', 'mirror', 'wrap')
        and ``cval`` are scipy's; ``origin`` other than 0 and ``footprint`` are not built; ``use_memmap``, ``verbose``,
        ``num_cores``, ``parallel``, ``update_function`` and ``save_to_tmp_dir`` are accepted and ignored.

        The filter runs on the filled data (masked samples -> fill_value) and the mask is left unchanged.  An even
        *ksize* behaves as in scipy: ``ksize // 2`` samples back, the rest forward, the median the upper middle sample.
        A spectrum without one included sample is left as it is (:147-159).  By design a NaN ranks LAST in its window
        (numpy's sort order: the result is ``np.sort(window)[rank]``), where scipy's result depends on its version; on
        windows without a NaN the two agree bit for bit.  Limits: ksize 1 ... 129 and ``ksize // 2 <= nz``.

        Pending like ``spectral_smooth``; a parent larger than the HBM budget runs strip by strip."""
        if isinstance(ksize, (bool, np.bool_)):
            raise TypeError("ksize should be an integer (got {0})".format(ksize))
        try:
            integral = float(ksize).is_integer()
        except (TypeError, ValueError):
            integral = False
        if not integral:
            raise TypeError("ksize should be an integer (got {0})".format(ksize))
        return self._rank_filtered((int(ksize),), self._shape[:1], filter, kwargs)

    def spectral_smooth_median(self, ksize, **kwargs):
        """Median-filter every spectrum over *ksize* channels (spectral_cube.py:2870-2898): ``spectral_filter`` with
        ``median_filter`` (a ``filter=`` keyword names another member of the family, as in the reference)."""
        return self.spectral_filter(ksize, kwargs.pop("filter", "median_filter"), **kwargs)

    def spatial_filter(self, ksize, filter, raise_error_jybm=True, **kwargs):
        """Filter every image plane with one of scipy.ndimage's rank filters over a window of *ksize* pixels, one integer
        or ``(ky, kx)`` (spectral_cube.py:2775-2806, dask_spectral_cube.py:995-1021).  Filters, keywords, the filled data,
        the unchanged mask and the NaN-last rule as ``spectral_filter``; a plane without one included sample is left as
        it is (:161-172).  Limits: ky, kx 1 ... 15 and ``k // 2`` at most the axis length.  A parent larger than the HBM
        budget runs in slabs of whole planes."""
        self.check_jybeam_smoothing(raise_error_jybm=raise_error_jybm)
        sizes = tuple(ksize) if isinstance(ksize, (tuple, list, np.ndarray)) else (ksize, ksize)
        if len(sizes) != 2 or any(isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer, float, np.floating))
                                  or not float(k).is_integer() for k in sizes):
            raise TypeError("ksize should be an integer or a pair of integers (got {0})".format(ksize))
        return self._rank_filtered(tuple(int(k) for k in sizes), self._shape[1:], filter, kwargs)

    def spatial_smooth_median(self, ksize, raise_error_jybm=True, **kwargs):
        """Median-filter every image plane (spectral_cube.py:2749-2772): ``spatial_filter`` with ``median_filter``."""
        return self.spatial_filter(ksize, kwargs.pop("filter", "median_filter"), raise_error_jybm=raise_error_jybm, **kwargs)

    @property
    def beam(self):
        """the restoring beam from BMAJ / BMIN / BPA (None when the header has no beam)."""
        from .beam import Beam
        if getattr(self, "_beam", None) is None:
            self._beam = Beam.from_header(self._header)
        return self._beam

    def with_beam(self, beam, raise_error_jybm=True):
        new = self._new_cube_with(data=self._data, dev=self._dev, lazy=self._lazy, shape=self._shape, same_data=True)
        new._beam = beam
        new._header = dict(self._header, BMAJ=beam.major, BMIN=beam.minor, BPA=beam.pa)
        return new

    @warn_slow
    def convolve_to(self, beam, convolve=None, **kwargs):
        """Convolve every channel to *beam* (dask_spectral_cube.py:1412-1464): kernel = beam.deconvolve(
        self.beam).as_kernel(pixscale) through the 2-D stencils (separable when the kernel is, else the
        LDS-tiled direct kernel), Jy/beam data scaled by the ratio of the beam areas."""
        _check_convolve(convolve)
        if self.beam is None:
            raise ValueError("cube has no beam (BMAJ / BMIN / BPA) to convolve from")
        if beam == self.beam:
            warnings.warn("The given beam is identical to the current beam. Skipping convolution.")
            return self
        if self._wcs is None:
            raise ValueError("convolve_to needs the celestial pixel scale of a WCS")
        psm = self._wcs.pixel_scale_matrix                     # proj_plane_pixel_area(wcs.celestial) ** 0.5
        pixscale = math.sqrt(abs(psm[0, 0] * psm[1, 1] - psm[0, 1] * psm[1, 0]))
        karr = beam.deconvolve(self.beam).as_kernel(pixscale)
        is_jybm = str(self._unit).replace(" ", "").upper() in ("JY/BEAM", "JYBEAM-1", "JY/BM")
        ratio = beam.sr / self.beam.sr if is_jybm else 1.0
        def run(data, mask, view=None, stream=None):
            res = ops.spatial_conv(data, karr, mask=mask, stream=stream)
            return ops.scale_inplace(res, ratio, stream=stream) if ratio != 1.0 else res
        if self._runs_wide():        # (pending, like every float64 result; the float32 result below is made at once)
            return self._derived(run).with_beam(beam, raise_error_jybm=False)
        if self._stream_source() is not None:
            # out of core: one kernel for every channel, so slabs of whole planes; pending until write() / stream_into()
            # (never resident: materialising asks the parent for its samples, which raises HugeCubeError with the budget)
            lazy = Pending(lambda dev, mspec, stream: run(dev, mspec, None, stream), op="convolve_to", parent=self, slabs=True,
                           keeps_mask=True)
            return self._new_cube_with(lazy=lazy, shape=self._shape).with_beam(beam, raise_error_jybm=False)
        new = self._new_cube_with(dev=run(self._device_data(), self._mask_spec()))
        return new.with_beam(beam, raise_error_jybm=False)

    def check_jybeam_smoothing(self, raise_error_jybm=True):
        """base_class.py:116-140"""
        if str(self._unit).replace(" ", "").upper() in ("JY/BEAM", "JYBEAM-1", "JY/BM"):
            if raise_error_jybm:
                raise BeamUnitsError("Attempting to change the spatial resolution of a cube with "
                                     "Jy/beam units. To ignore this error, set "
                                     "`raise_error_jybm=False`.")

    # ---- regridding -----------------------------------------------------------------------------
    def spectral_interpolate(self, spectral_grid, suppress_smooth_warning=False, fill_value=None,
                             force_rechunk=True):
        """Resample onto a linear spectral grid, Dask semantics
        (dask_spectral_cube.py:1250-1373): NaN outside the input range (or
        ``fill_value``), NaN when either bracketing channel is NaN/masked,
        new mask = ~isnan(result)."""
        grid = np.asarray(getattr(spectral_grid, "value", spectral_grid), dtype=np.float64)
        inaxis = self.spectral_axis
        lo, t, inv_dx, rin, rout, fill = ops.lerp_plan(inaxis, grid, fill_value)
        g_sorted = grid[::-1] if rout else grid
        in_sorted = inaxis[::-1] if rin else inaxis
        indiff = np.mean(np.diff(in_sorted))
        outdiff = np.mean(np.diff(g_sorted))
        if outdiff > 2 * indiff and not suppress_smooth_warning:
            warnings.warn("Input grid has too small a spacing. The data should "
                          "be smoothed prior to resampling.", SmoothingWarning)
        nz = self._shape[0]
        if rin:          # cubedata[::-1]: channel k of the flipped cube is nz-1-k
            lo_dev = np.where(lo >= 0, nz - 2 - lo, -1).astype(np.int32)
            # bracketing pair (lo, lo+1) of the flipped axis = (nz-1-lo, nz-2-lo) here:
            # interpolate from the upper neighbour downwards
            t_dev = (in_sorted[np.clip(lo, 0, nz - 2) + 1] - g_sorted)
            plan = (lo_dev, np.where(lo >= 0, t_dev, 0.0), inv_dx)
        else:
            plan = (lo, t, inv_dx)
        if rout:
            plan = tuple(p[::-1].copy() for p in plan)

        def lerp(dev, mspec, stream=None):
            return ops.spectral_lerp(dev, plan[0], plan[1], plan[2], fill, mask=mspec, stream=stream)

        crval = g_sorted[0] if not rout else g_sorted[-1]
        cdelt = outdiff if not rout else -outdiff
        newwcs = self._wcs.with_spectral(crval, cdelt, 1.0)
        if self._runs_wide():
            out = self._derived(lambda data, mask, view: lerp(data, mask), shape=(len(grid),) + self._shape[1:], wcs=newwcs, mask=False)
            out._mask = M.NotNaNMask(out)
            return out
        # float32: the record also carries what an out-of-core parent needs (row strips) and what a following reproject
        # needs to fold the interpolation into its resampling kernel (the plan)
        lazy = Pending(lerp, op="spectral_interpolate", parent=self, strips=True, lerp=(plan, fill))
        out = self._new_cube_with(lazy=lazy, shape=(len(grid),) + self._shape[1:], wcs=newwcs, mask=False)
        out._mask = M.NotNaNMask(out)
        return out

    @warn_slow
    def reproject(self, header, order="bilinear", use_memmap=False, filled=True, **kwargs):
        """Reproject onto the WCS of *header* (spectral_cube.py:2649-2746 -> reproject_interp).

        The celestial plane of every channel is resampled at the source positions of the target pixels
        (``order`` 'bilinear' / 1 or 'nearest-neighbor' / 0; the pixel map is formed on the device by
        this package's WCS, validated against astropy.wcs).  Like the reference, a cube header also
        carries the output's spectral axis: ``NAXIS3`` channels at the target's spectral coordinates,
        linearly interpolated between the source channels (reproject_interp's one trilinear call for a
        separable cube WCS, restated as oracle_np.reproject_separable and pinned against scipy).  A
        2-axis header keeps this cube's spectral axis.  Masked voxels enter as ``fill_value`` when
        ``filled``; the new mask is the footprint; an output without a single non-NaN value raises the
        reference's ValueError."""
        order = {"nearest-neighbor": 0, "bilinear": 1, "biquadratic": 2, "bicubic": 3}.get(order, order)
        if order not in (0, 1, 2, 3):
            raise ValueError("order %r: 'nearest-neighbor' (0), 'bilinear' (1), 'biquadratic' (2) or 'bicubic' (3)" % (order,))
        newwcs = header if isinstance(header, SimpleWCS) else SimpleWCS(header)
        if self._wcs is not None:
            self._wcs._require_celestial()     # (a cube is read with a lenient WCS: keywords it does not model are refused here)
        newwcs._require_celestial()
        hdr = newwcs.header
        if "NAXIS1" in hdr and "NAXIS2" in hdr:
            ny_out, nx_out = int(hdr["NAXIS2"]), int(hdr["NAXIS1"])
        else:
            ny_out, nx_out = self._shape[1:]
        nz = self._shape[0]
        zs = None
        if newwcs.naxis >= 3 and self._wcs is not None and self._wcs.naxis >= 3:
            nz_out = int(hdr.get("NAXIS3", nz))
            check_same_spectral_kind(self._wcs, newwcs)
            scale = spectral_unit_scale(newwcs.spectral_unit or self.spectral_unit, self.spectral_unit)
            zs = self._wcs.spectral_world2pix(newwcs.spectral_pix2world(np.arange(nz_out)) * scale)
            if nz_out == nz and np.all(np.abs(zs - np.arange(nz)) <= 1e-9 * max(nz, 1)):
                zs = None                         # the same channels: a purely spatial reprojection
        elif self._wcs is not None and self._wcs.naxis >= 3:
            newwcs = join_celestial_spectral(newwcs, self._wcs, nz)
        if zs is not None and (order != 1 or nz < 2):
            raise NotImplementedError("resampling the spectral axis as well needs order='bilinear' and at least two channels "
                                      "(spectral_interpolate first, then reproject with order %r)" % (order,))
        if order >= 2 and self._stream_source() is not None:
            from . import streaming
            raise streaming.HugeCubeError("order 'biquadratic' / 'bicubic' of a cube above the HBM budget (SPC_HBM_BUDGET) is not built: "
                                          "the spline prefilter couples every sample of the cube")
        if os.environ.get("SPC_WCS_HOST_MAP", "0") == "1":         # cross-check: the numpy map (0.8 s per 1024^2 pixels)
            xs, ys = reproject_pixel_map(self._wcs, newwcs, (ny_out, nx_out))
            xs = np.where(np.isfinite(xs), xs, -1e30)
            ys = np.where(np.isfinite(ys), ys, -1e30)
        else:
            _lib.require_gpu()
            xs, ys = ops.wcs_pixel_map(self._wcs, newwcs, (ny_out, nx_out), self.device)
        if self._stream_source() is not None:
            if zs is not None:
                return self._reproject_streamed_with_spectral_axis(newwcs, zs, (ny_out, nx_out), order, filled)
            return self._reproject_streamed(newwcs, xs, ys, order, filled)
        if order in (0, 1) and self._runs_wide():
            return self._reproject_f64(newwcs, xs, ys, zs, order, filled)
        folded = self._pending_interpolation(order) if zs is None else None
        if folded is not None:
            return self._reproject_folded(newwcs, xs, ys, order, *folded)
        if order >= 2:
            return self._reproject_spline(newwcs, xs, ys, order, filled)
        return self._reproject_bilinear(newwcs, xs, ys, zs, order, filled)

    def _resample_mask(self, filled, wide):
        """the mask a resampler fills under (None when not *filled*), lowered for the float32 or (*wide*) float64 kernels"""
        if not filled:
            return None
        data, mspec, _ = self._operand(wide)
        if not np.isnan(float(self._fill_value)) and self._mask is not None and M.contains(self._mask, M.NotNaNMask) \
                and not M.contains(self._mask, M.InvertedMask):
            # ~isnan(data) lowers to nothing (NaN samples never take part in a reduction), but HERE the excluded voxels are
            # replaced by a fill value that is a number (spectral_cube.py:2709-2712): the NaN samples must be named
            return ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, ops.mask_include(data, mspec, nan_excluded=True))
        return mspec

    def _reprojected(self, dev, footprint, inside, newwcs, shape=None):
        """the result cube of a reprojection: *dev* its float32 or float64 DeviceArray, or the Pending record of a result
        that is never resident (with its *shape*); the new mask is the *footprint*, on the output channels *inside* the
        source's spectral range (None: all of them); ``_footprint`` keeps the 2-D map"""
        if isinstance(dev, Pending):
            out = self._new_cube_with(lazy=dev, wcs=newwcs, mask=False, shape=shape)
        elif dev.dtype == np.float64:
            out = self._new_wide_cube(lambda: dev, shape=dev.shape, wcs=newwcs, mask=False)
        else:
            out = self._new_cube_with(dev=dev, wcs=newwcs, mask=False, shape=dev.shape)
        valid3d = footprint[None] if inside is None or inside.all() else footprint[None] & inside[:, None, None]
        out._mask = M.BooleanArrayMask(valid3d, newwcs, shape=out._shape)
        out._footprint = footprint
        return out

    def _reproject_streamed(self, newwcs, xs, ys, order, filled):
        """out of core: every channel is resampled on its own, so the cube goes through the device in slabs of whole
        planes; the result stays pending until write() / stream_into() (it does not fit the budget either, so
        materialising it raises the parent's HugeCubeError).  Footprint and all-NaN error: a one-plane probe of the map."""
        probe = DeviceArray.from_numpy(np.zeros((1,) + tuple(self._shape[1:]), np.float32), self.device)
        _, foot = ops.resample_bilinear(probe, xs, ys, fill=np.nan, order=order)
        footprint = foot.get().astype(bool)
        if not footprint.any():
            raise ValueError(_ALL_NAN)
        fill = float(self._fill_value)
        lazy = Pending(lambda dev, mspec, stream: ops.resample_bilinear(dev, xs, ys, fill=fill, mask=mspec if filled else None,
                                                                        order=order, stream=stream, want_footprint=False)[0],
                       op="reproject", parent=self, slabs=True)
        return self._reprojected(lazy, footprint, None, newwcs, shape=(self._shape[0],) + tuple(xs.shape))

    def _reproject_f64(self, newwcs, xs, ys, zs, order, filled):
        """a float64 cube: float64 weights and results (reproject_interp computes in float64); a cube header's own spectral
        axis is blended from the resampled float64 planes afterwards"""
        flag = DeviceArray((1,), np.uint32, self.device)
        mask64 = self._resample_mask(filled, True)
        dev64, foot = ops.resample_bilinear(self._device_data64(), xs, ys, fill=float(self._fill_value), mask=mask64, order=order,
                                            any_valid=flag)
        footprint = foot.get().astype(bool)
        nothing, inside = int(flag.get()[0]) == 0, None
        if zs is not None:
            inside, lo, t, ones = _channel_plan(zs, self._shape[0])
            dev64 = ops.spectral_lerp(dev64, lo, t, ones, np.nan)
            nothing = nothing or not inside.any()
        if nothing:
            raise ValueError(_ALL_NAN)
        return self._reprojected(dev64, footprint, inside, newwcs)

    def _reproject_folded(self, newwcs, xs, ys, order, parent, plan):
        """spectral_interpolate(...).reproject(...): both are linear interpolations with NaN propagation, so they commute -
        every INPUT plane is resampled once and the output channels are blended from neighbouring resampled planes in the
        same kernel (ops.resample_bilinear_lerp): one read of the parent, one write of the result, the interpolated cube
        is never formed"""
        flag = DeviceArray((1,), np.uint32, self.device)
        dev, foot = ops.resample_bilinear_lerp(parent._device_data(), xs, ys, plan[0], plan[1], plan[2], fill=np.nan,
                                               mask=parent._mask_spec(), order=order, any_valid=flag)
        footprint = foot.get().astype(bool)
        if int(flag.get()[0]) == 0:
            raise ValueError(_ALL_NAN)
        return self._reprojected(dev, footprint, None, newwcs)

    def _reproject_spline(self, newwcs, xs, ys, order, filled):
        """order 2 / 3 of a resident float32 cube (the planner has refused a spectral axis of the target's own)"""
        mask = self._resample_mask(filled, False)
        # scipy's recursive spline prefilter (which reproject_interp runs along all three axes of the NaN-filled cube)
        # turns ONE non-finite sample into NaN everywhere: the reference then raises "All values ... are nan"
        src = self._device_data()
        if mask is not None:
            src = ops.fill_masked(src, mask, float(self._fill_value))
        finite = ops.stats_global(src, mask=ops.MaskSpec(_lib.MASK_FINITE))["npts"]
        if int(finite) != int(np.prod(self._shape, dtype=np.int64)):
            raise ValueError(_ALL_NAN)
        dev, foot = ops.resample_spline(src, xs, ys, order)
        footprint = foot.get().astype(bool)
        if not footprint.any():
            raise ValueError(_ALL_NAN)
        return self._reprojected(dev, footprint, None, newwcs)

    def _reproject_bilinear(self, newwcs, xs, ys, zs, order, filled):
        """order 0 / 1 of a resident float32 cube; *zs*: the target's channels in source channel units when the header
        carries a spectral axis of its own (reproject_separable: each output channel is the linear blend of the two
        resampled planes around it)"""
        fill, mask = float(self._fill_value), self._resample_mask(filled, False)
        flag = DeviceArray((1,), np.uint32, self.device)
        inside = None
        if zs is not None:
            inside, lo, t, ones = _channel_plan(zs, self._shape[0])
        if zs is not None and ops.lerp_plan_folds(lo) and os.environ.get("SPC_REPROJECT_FOLD", "1") != "0":
            # ascending target channels: the blend rides in the resampling kernel (one pass, no resampled copy of the cube)
            dev, foot = ops.resample_bilinear_lerp(self._device_data(), xs, ys, lo, t, ones, fill=fill, mask=mask, order=order,
                                                   any_valid=flag)
            folded = True
        else:
            dev, foot = ops.resample_bilinear(self._device_data(), xs, ys, fill=fill, mask=mask, order=order, any_valid=flag)
            folded = False
        footprint = foot.get().astype(bool)
        if zs is not None and not folded:
            dev = ops.spectral_lerp(dev, lo, t, ones, np.nan)
            nothing = (not inside.any()) or ops.stats_global(dev)["npts"] == 0
        else:
            nothing = (zs is not None and not inside.any()) or int(flag.get()[0]) == 0
        if nothing:
            raise ValueError(_ALL_NAN)
        return self._reprojected(dev, footprint, inside, newwcs)

    def _pending_interpolation(self, order):
        """(parent, plan) when this cube is a spectral_interpolate result that has not been formed yet and a reprojection of
        order 0 / 1 may fold the interpolation in: the parent is resident (or fits), nothing replaced the NaN fill or the
        ~isnan mask in between, the plan's channels ascend"""
        lz = self._lazy
        if self._dev is not None or lz is None or lz.lerp is None or order not in (0, 1):
            return None
        if os.environ.get("SPC_REPROJECT_FOLD", "1") == "0":
            return None
        plan, fill = lz.lerp
        parent = lz.parent
        if not (np.isnan(fill) and np.isnan(float(self._fill_value))) or parent._stream_source() is not None:
            return None
        if not (isinstance(self._mask, M.NotNaNMask) and self._mask._data_ref._is_same_data(self)):
            return None
        if parent._shape[0] < 2 or not ops.lerp_plan_folds(plan[0]):
            return None
        return parent, plan

    def _reproject_streamed_with_spectral_axis(self, newwcs, zs, shape_yx, order, filled):
        """reproject of a cube above the HBM budget onto a CUBE header whose spectral axis differs from this cube's: the
        reference's one reproject_interp call (spectral_cube.py:2726-2732) resamples all three axes at once; for a separable
        WCS that is the celestial resampling of every source channel followed by the linear blend of the two resampled
        planes around every output channel (oracle_np.reproject_separable).  Out of core the two steps run one after the
        other: source slabs -> resampled planes in a float32 HOST array (nz x ny_out x nx_out: host memory, not HBM), then
        row strips of that array -> output channels, pending until write() / stream_into() / a reduction."""
        nz = self._shape[0]
        ny_out, nx_out = shape_yx
        celestial = join_celestial_spectral(newwcs, self._wcs, nz)          # the target's sky grid, this cube's channels
        spatial = self.reproject(celestial, order=order, filled=filled)      # (pending; raises the all-NaN ValueError itself)
        mid = np.empty((nz, ny_out, nx_out), dtype=np.float32)
        spatial.stream_into(mid)
        midcube = SpectralCube(mid, wcs=celestial, device=self.device, allow_huge_operations=self.allow_huge_operations)
        inside, lo, t, ones = _channel_plan(zs, nz)
        if not inside.any():
            raise ValueError(_ALL_NAN)
        lazy = Pending(lambda dev, mspec, stream: ops.spectral_lerp(dev, lo, t, ones, np.nan, mask=mspec, stream=stream),
                       op="reproject", parent=midcube, strips=True)
        return self._reprojected(lazy, spatial._footprint, inside, newwcs, shape=(len(zs), ny_out, nx_out))

    def __repr__(self):
        return "SpectralCube(hip) with shape=%s%s" % (self._shape, " and unit=%s" % self._unit if self._unit else "")


class BeamWarning(UserWarning):
    """spectral_cube.utils.BeamWarning"""


class NonFiniteBeamsWarning(UserWarning):
    """spectral_cube.utils.NonFiniteBeamsWarning"""


class VaryingResolutionSpectralCube(SpectralCube):
    """Cube with one beam per channel (spectral_cube.py:3776-3872, the Dask flavour at
    dask_spectral_cube.py:1467-1645).  What the accelerated path serves is ``convolve_to``: every
    channel is brought to a common beam with its own deconvolved kernel, runs of channels that share
    a beam going through the 2-D stencils in one launch.  Channels with non-finite beams are masked
    out, as the reference does; the beam-area checks around spectral reductions
    (base_class.py:673-790) are not mirrored."""

    def __init__(self, *args, beams=None, beam_table=None, goodbeams_mask=None, beam_threshold=0.01, **kw):
        if beams is None and beam_table is None:
            raise ValueError("Must give either a beam table or a list of beams to "
                             "initialize a VaryingResolutionSpectralCube")
        super().__init__(*args, **kw)
        if beam_table is not None:          # {"BMAJ", "BMIN", "BPA"} in degrees (io_fits.read_beams_table)
            beams = [Beam(a, b, p) for a, b, p in zip(beam_table["BMAJ"], beam_table["BMIN"], beam_table["BPA"])]
        beams = list(beams)
        if len(beams) != self._shape[0]:
            raise ValueError("Beam list must have same size as spectral dimension")
        self._beams = beams
        self.beam_threshold = beam_threshold
        good = np.array([b.isfinite for b in beams], dtype=bool)
        if goodbeams_mask is not None:
            good &= np.asarray(goodbeams_mask, dtype=bool)
        self._goodbeams_mask = good
        if not good.all():
            if goodbeams_mask is None:
                warnings.warn("There were {0} non-finite beams; layers with non-finite beams will be "
                              "masked out.".format(int(np.count_nonzero(~good))), NonFiniteBeamsWarning)
            bm = M.BooleanArrayMask(good[:, None, None], wcs=self._wcs, shape=self._shape)
            self._mask = bm if self._mask is None else (self._mask & bm)

    @property
    def beams(self):
        """the beams of the channels whose beam is good (base_class.py:497-501)"""
        return [b for b, g in zip(self._beams, self._goodbeams_mask) if g]

    @property
    def unmasked_beams(self):
        return self._beams

    @property
    def goodbeams_mask(self):
        return self._goodbeams_mask

    @property
    def beam(self):
        raise AttributeError("VaryingResolutionSpectralCubes have a `beams` list, not a single `beam`")

    def with_beams(self, beams, goodbeams_mask=None, raise_error_jybm=True):
        new = self._new_cube_with(data=self._data, dev=self._dev, lazy=self._lazy, shape=self._shape, same_data=True)
        beams = list(beams)
        if len(beams) != self._shape[0]:
            raise ValueError("Beam list must have same size as spectral dimension")
        new._beams = beams
        if goodbeams_mask is not None:
            new._goodbeams_mask = np.asarray(goodbeams_mask, dtype=bool)
        return new

    def downsample_axis(self, factor, axis, estimator=np.nanmean, truncate=False, use_memmap=True, progressbar=True):
        """spatial axes as SpectralCube.downsample_axis (the beams table is kept); along the spectral axis the beams of a
        run cannot be averaged: NotImplementedError"""
        if not isinstance(axis, (bool, np.bool_)) and isinstance(axis, (int, np.integer)) and axis == 0:
            raise NotImplementedError("downsampling the spectral axis of a VaryingResolutionSpectralCube would have to average "
                                      "the channels' beams: bring the cube to one beam with convolve_to() first")
        return SpectralCube.downsample_axis(self, factor, axis, estimator=estimator, truncate=truncate)

    def _cut_finish(self, new, view):
        """a cut along the spectral axis cuts the beams table with the same slice (spectral_cube.py:3873-3967)"""
        new.__class__ = VaryingResolutionSpectralCube
        new._beams = list(self._beams[view[0]])
        new._goodbeams_mask = self._goodbeams_mask[view[0]].copy()
        new.beam_threshold = self.beam_threshold
        return new

    def _channel_beam(self, k):
        return self._beams[k]

    def _spectrum_meta(self, meta, view):
        return dict(meta, beams=list(self._beams[view[0]]))

    def _new_cube_with(self, **kw):
        new = SpectralCube._new_cube_with(self, **kw)
        if new._shape[0] == len(self._beams):
            new.__class__ = VaryingResolutionSpectralCube
            new._beams = self._beams
            new._goodbeams_mask = self._goodbeams_mask
            new.beam_threshold = self.beam_threshold
        return new

    def write(self, filename, overwrite=False, format=None):
        """the cube followed by its BEAMS table (hdulist, dask_spectral_cube.py:1493-1509)"""
        from . import io_fits
        SpectralCube.write(self, filename, overwrite=overwrite, format=format)
        io_fits.append_beams_table(os.fspath(filename), [b.major for b in self._beams],
                                   [b.minor for b in self._beams], [b.pa for b in self._beams])

    @warn_slow
    def convolve_to(self, beam, allow_smaller=False, convolve=None, **kwargs):
        """Convolve each channel to *beam* (dask_spectral_cube.py:1511-1630): channel k gets the kernel
        ``beam.deconvolve(beams[k]).as_kernel(pixscale)`` and, for Jy/beam data, the factor
        ``beam.sr / beams[k].sr``; channels whose beam is masked, equals the target, or (with
        ``allow_smaller``) cannot be deconvolved are passed through as filled data.  Returns a
        single-beam SpectralCube."""
        _check_convolve(convolve)
        if self._wcs is None:
            raise ValueError("convolve_to needs the celestial pixel scale of a WCS")
        psm = self._wcs.pixel_scale_matrix
        if psm[0, 1] != 0 or psm[1, 0] != 0:
            warnings.warn("The beams will produce convolution kernels that are not aware of any "
                          "misaligment between pixel and world coordinates, and there are off-diagonal "
                          "elements of the WCS spatial transformation matrix.  Unexpected results are "
                          "likely.", BeamWarning)
        pixscale = math.sqrt(abs(psm[0, 0] * psm[1, 1] - psm[0, 1] * psm[1, 0]))
        is_jybm = str(self._unit).replace(" ", "").upper() in ("JY/BEAM", "JYBEAM-1", "JY/BM")
        plans = []                                  # per channel: None (pass through) or (source beam, kernel, ratio)
        for bm, valid in zip(self._beams, self._goodbeams_mask):
            if not valid or beam == bm:
                plans.append(None)
                continue
            try:
                dk = beam.deconvolve(bm)
            except (BeamError, ValueError):
                if allow_smaller:
                    plans.append(None)
                    continue
                raise
            if plans and plans[-1] is not None and plans[-1][0] == bm:
                plans.append(plans[-1])             # same beam as the previous channel: share the launch
            else:
                plans.append((bm, dk.as_kernel(pixscale), beam.sr / bm.sr if is_jybm else 1.0))
        def runs(src, spec, zbase, stream=None):
            """channels zbase .. of the cube held in `src` (their mask in `spec`): runs of channels that share a plan, one launch
            each, in the dtype of `src`"""
            n = src.shape[0]
            out = DeviceArray(src.shape, src.dtype, self.device)
            a = 0
            while a < n:
                b = a + 1
                while b < n and plans[zbase + b] is plans[zbase + a]:
                    b += 1
                o, m = out.planes(a, b), (spec.planes(a, b) if spec is not None else None)
                if plans[zbase + a] is None and src.dtype == np.float32:
                    ops.fill_masked(src.planes(a, b), m, np.nan, out=o, stream=stream)
                else:
                    # (fill_masked has no float64 form: a float64 pass-through channel = the 1 x 1 kernel, the filled sample)
                    _, karr, ratio = plans[zbase + a] or (None, np.ones((1, 1)), 1.0)
                    ops.spatial_conv(src.planes(a, b), karr, mask=m, out=o, stream=stream)
                    if ratio != 1.0:
                        ops.scale_inplace(o, ratio, stream=stream)
                a = b
            return out

        if self._runs_wide():
            # a float64 cube: the same runs on the float64 samples
            return self._derived(lambda data, mask, view: runs(data, mask, 0), plain=True).with_beam(beam, raise_error_jybm=False)
        if self._stream_source() is not None:
            # out of core: slabs of whole planes (every channel has its own kernel, the slab knows its first channel);
            # pending until write() / stream_into()
            # (never resident: materialising asks the parent for its samples, which raises HugeCubeError with the budget)
            lazy = Pending(lambda dev, mspec, stream: runs(dev, mspec, int(getattr(dev, "z0", 0)), stream), op="convolve_to",
                           parent=self, slabs=True, keeps_mask=True)
            new = SpectralCube._new_cube_with(self, lazy=lazy, shape=self._shape)
            return new.with_beam(beam, raise_error_jybm=False)
        new = SpectralCube._new_cube_with(self, dev=runs(self._device_data(), self._mask_spec(), 0))
        return new.with_beam(beam, raise_error_jybm=False)

    def spectral_interpolate(self, *args, **kwargs):
        raise AttributeError("VaryingResolutionSpectralCubes can't be spectrally interpolated.  Convolve "
                             "to a common resolution with `convolve_to` before attempting spectral "
                             "interpolation.")

    def spectral_smooth(self, *args, **kwargs):
        raise AttributeError("VaryingResolutionSpectralCubes can't be spectrally smoothed.  Convolve to "
                             "a common resolution with `convolve_to` before attempting spectral "
                             "smoothed.")

    def __repr__(self):
        return "VaryingResolutionSpectralCube(hip) with shape=%s%s" % (
            self._shape, " and unit=%s" % self._unit if self._unit else "")


class _Once:
    """fn() run once, its result kept (the one kernel pass behind a downsampled cube's data AND mask)"""

    def __init__(self, fn):
        self._fn, self._res = fn, None

    def __call__(self):
        if self._fn is not None:
            _lib.require_gpu()
            self._res = self._fn()
            self._fn = None
        return self._res
