"""The mask predicate is one piece of code (csrc/spc_common.h): its semantics, pinned through every operator that takes a
mask and a fill value, in float32 and float64 -
  * NaN never passes a predicate; without one it follows the array term, unless nan_excluded says otherwise,
  * >= / <= include the threshold itself and nothing beyond its neighbouring float,
  * a NaN threshold rejects everything, >= -inf / <= +inf reject only NaN.
Every operator runs in an identity configuration, so the expected result is numpy's own evaluation of the mask in the
cube's dtype and every comparison is exact: no tolerance appears in this file."""
import functools

import numpy as np
import pytest

from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

SHAPES = [(5, 6, 7), (8, 8, 16)]          # odd nx: the scalar paths; aligned rows: the 16-byte paths
DTYPES = [np.float32, np.float64]
T = 1.5
FILL = -7.0


def _samples(dtype):
    t, inf = dtype(T), dtype(np.inf)
    special = [np.nan, inf, -inf, 0.0, -0.0, t, np.nextafter(t, -inf), np.nextafter(t, inf), -t, np.finfo(dtype).max]
    return np.array(special, dtype=dtype), np.array([0.25, -3.0, 2.0], dtype=dtype)


@functools.lru_cache(maxsize=None)
def _case(dtype, shape):
    """(host cube, device cube, host array term, device array term): the samples repeat with period 13 (coprime to every extent, so
    each lands in every column), the array term has a zero at the first copy of every special sample"""
    special, plain = _samples(dtype)
    vals = np.concatenate([special, plain])
    n = int(np.prod(shape))
    d = vals[np.arange(n) % vals.size].reshape(shape)
    arr = np.ones(shape, np.uint8)
    arr.reshape(-1)[:special.size] = 0
    d.setflags(write=False)
    arr.setflags(write=False)
    return d, DeviceArray.from_numpy(d, 0), arr, DeviceArray.from_numpy(arr, 0)


def _masks():
    """(name, flags, thr_lo, thr_hi, numpy predicate or None)"""
    L = _lib
    nan, inf = float("nan"), float("inf")
    base = [
        ("none", 0, 0.0, 0.0, None),
        ("finite", L.MASK_FINITE, 0.0, 0.0, lambda v, t: np.isfinite(v)),
        ("gt t", L.MASK_GT, T, 0.0, lambda v, t: v > t(T)),
        ("ge t", L.MASK_GE, T, 0.0, lambda v, t: v >= t(T)),
        ("lt t", L.MASK_LT, 0.0, T, lambda v, t: v < t(T)),
        ("le t", L.MASK_LE, 0.0, T, lambda v, t: v <= t(T)),
        ("ge -t & le t", L.MASK_GE | L.MASK_LE, -T, T, lambda v, t: (v >= t(-T)) & (v <= t(T))),
        ("ge -inf", L.MASK_GE, -inf, 0.0, lambda v, t: v >= t(-inf)),
        ("le +inf", L.MASK_LE, 0.0, inf, lambda v, t: v <= t(inf)),
        ("gt nan", L.MASK_GT, nan, 0.0, lambda v, t: v > t(nan)),
        ("lt nan", L.MASK_LT, 0.0, nan, lambda v, t: v < t(nan)),
    ]
    for name, flags, lo, hi, pred in base:
        for with_array in (False, True):
            for nan_excluded in (False, True):
                yield ("%s%s%s" % (name, " & array" if with_array else "", ", nan excluded" if nan_excluded else ""),
                       flags, lo, hi, pred, with_array, nan_excluded)


MASKS = list(_masks())


def _expected(d, arr, pred, with_array, nan_excluded):
    """the include set as numpy evaluates the mask, thresholds in the cube's dtype"""
    inc = np.ones(d.shape, bool)
    with np.errstate(invalid="ignore"):
        if pred is not None:
            inc &= pred(d, d.dtype.type)
    if with_array:
        inc &= arr != 0
    if nan_excluded:
        inc &= ~np.isnan(d)
    return inc


def _each_mask(dtype, shape):
    """(name, MaskSpec or None, nan_excluded, expected include set, host cube, device cube) per mask"""
    d, dev, arr, dev_arr = _case(dtype, shape)
    for name, flags, lo, hi, pred, with_array, nan_excluded in MASKS:
        spec = ops.MaskSpec(flags | (_lib.MASK_ARRAY if with_array else 0), lo, hi, dev_arr if with_array else None)
        if name == "none":
            spec = None
        yield "%s %s: %s" % (np.dtype(dtype).name, shape, name), spec, nan_excluded, _expected(d, arr, pred, with_array, nan_excluded), d, dev


def _same_bits(got, exp, what):
    """bit for bit where exp is not NaN, NaN exactly where exp is"""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what + ": NaN pattern"
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    ok = ~np.isnan(exp)
    assert np.array_equal(got.view(u)[ok], exp.view(u)[ok]), what + ": samples differ"


def _filled(d, inc, fill):
    return np.where(inc, d, d.dtype.type(fill))


grid = pytest.mark.parametrize("dtype,shape", [(t, s) for t in DTYPES for s in SHAPES],
                               ids=["%s-%dx%dx%d" % ((np.dtype(t).name,) + s) for t in DTYPES for s in SHAPES])


def test_the_cases_hold_every_special_sample_and_every_mask():
    for dtype in DTYPES:
        special, _ = _samples(dtype)
        assert special.dtype == dtype and np.isnan(special[0]) and np.signbit(special[4]) and special[6] < special[5] < special[7]
        assert special[7] - special[6] == 2 * np.spacing(special[6])       # the neighbouring floats of this dtype, not of another
    assert len(MASKS) == 11 * 2 * 2


@grid
def test_mask_include(gpu, dtype, shape):
    for what, spec, nx_, inc, d, dev in _each_mask(dtype, shape):
        got = ops.mask_include(dev, spec, nan_excluded=nx_).get()
        assert got.dtype == np.uint8 and np.array_equal(got, inc.astype(np.uint8)), what


@grid
def test_subcube_filled(gpu, dtype, shape):
    for what, spec, nx_, inc, d, dev in _each_mask(dtype, shape):
        out, om = ops.subcube(dev, (0, 0, 0), (1, 1, 1), shape, mask=spec, filled=True, fill=FILL, nan_excluded=nx_)
        exp = _filled(d, inc, FILL)
        _same_bits(out.get(), exp, what)
        assert np.array_equal(om.get(), inc.astype(np.uint8)), what + ": mask"


@grid
def test_mask_bbox(gpu, dtype, shape):
    for what, spec, nx_, inc, d, dev in _each_mask(dtype, shape):
        got = ops.mask_bbox(dev, spec, nan_excluded=nx_)
        if " nan" in what.split(": ")[1].split(",")[0]:               # a NaN threshold: nothing is included
            assert not inc.any(), what
        if not inc.any():
            assert got is None, what
            continue
        exp = tuple((int(np.flatnonzero(inc.any(axis=tuple(b for b in range(3) if b != a)))[0]),
                     int(np.flatnonzero(inc.any(axis=tuple(b for b in range(3) if b != a)))[-1])) for a in range(3))
        assert got == exp, what


@grid
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_downsample_by_one(gpu, dtype, shape, axis):
    for what, spec, nx_, inc, d, dev in _each_mask(dtype, shape):
        out, om = ops.downsample(dev, axis, 1, estimator=_lib.DS_MAX, fill=np.nan, mask=spec, nan_excluded=nx_)
        _same_bits(out.get(), _filled(d, inc, np.nan), what)
        assert np.array_equal(om.get(), inc.astype(np.uint8)), what + ": mask"


@grid
def test_rank_filters_of_one_sample(gpu, dtype, shape):
    for what, spec, nx_, inc, d, dev in _each_mask(dtype, shape):
        exp = _filled(d, inc, np.nan)
        _same_bits(ops.rank_filter_axis0(dev, 1, 0, mask=spec, nan_excluded=nx_).get(), exp, what + " (axis 0)")
        _same_bits(ops.rank_filter_plane(dev, 1, 1, 0, mask=spec, nan_excluded=nx_).get(), exp, what + " (plane)")


@grid
def test_stack_sum_counts(gpu, dtype, shape):
    npos = shape[1] * shape[2]
    for what, spec, nx_, inc, d, dev in _each_mask(dtype, shape):
        _, count, nnan = ops.stack_sum(dev, np.arange(npos), np.zeros(npos), fill=np.nan, mask=spec, nan_excluded=nx_)
        exp = np.isfinite(_filled(d, inc, np.nan)).sum(axis=(1, 2))          # a row is NaN where its filled sample is not finite
        assert count.dtype == np.int64 and np.array_equal(count, exp), what
        assert np.array_equal(nnan, npos - exp), what
