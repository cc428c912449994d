"""std, the sums next to it and sigma clipping on cubes far from zero (far_from_zero.py holds the cases and the references;
test_far_from_zero_host.py shows that the single-pass formula sumsq / n - mean^2 misses every tolerance here by a factor of
100 to 1e9).  Cube-level API throughout.

Shapes - the smallest that still reach every kernel form:
  float32  (48, 9, 37)    scalar paths                      float64  (33, 5, 7)   small odd extents
           (40, 8, 64)    16-byte loads                              (9, 3, 130)  wide rows
           (3, 50, 1366)  ragged linear groups of the global kernel  (64, 6, 8)   even extents
           (515, 2, 37)   rays split across waves
Masks: none, a uint8 include array drawn at 70 %, `cube > thr` with thr just below the pedestal, both."""
import functools
import warnings

import numpy as np
import pytest

import far_from_zero as Z
from conftest import assert_close
from spectral_cube_amd import SpectralCube, ops
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5, "CUNIT3": "km/s",
       "CRPIX1": 1, "CRPIX2": 1, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}


def _masked(cube, arr, thr, mask):
    if "array" in mask:
        cube = cube.with_mask(arr.astype(bool))
    if "predicate" in mask:
        cube = cube.with_mask(cube > thr)
    return cube


@functools.lru_cache(maxsize=None)
def _filled(case, mask):
    d, arr, thr = Z.case(*case)
    f = Z.filled_of(d, Z.include_of(d, arr, thr, mask))
    f.setflags(write=False)
    return f


def _check_std(cube, f, family, d, what, axes=Z.AXES):
    for axis in axes:
        for ddof in (0, 1):
            got = cube.std(axis=axis, ddof=ddof)
            assert_close(got, Z.ref_std(f, axis, ddof), rtol=Z.RTOL, atol=Z.std_atol(family, d), what="%s: std axis %s ddof %d" % (what, axis, ddof))


def _check_sums(cube, f, family, what):
    """sum and mean at rtol 1e-12 OF THE VALUE, every family, every element - also where the baselines of `per_ray` and
    `constant` have both signs and a row of the plane cancels (sum |x| up to 3.5e4 |sum x|).  The whole-cube sums against
    math.fsum; the maps against long-double sums of the same samples, whose own error n 2^-64 sum |x| is far below that
    bound (a Python call per ray of the widest map would take the test's time): the bound itself is the one asked"""
    for axis in Z.AXES:
        n, s, a = Z.wide_sums(f, axis)
        if axis is None:
            ex = Z.exact_sums(f)
            s = np.longdouble(ex["sum"])
        with np.errstate(all="ignore"):
            s = np.where(n > 0, s, np.nan)
            scale = np.abs(s)
            for name, exp, tol in (("sum", s, 1e-12 * scale), ("mean", s / n, 1e-12 * scale / n)):
                got = np.asarray(getattr(cube, name)(axis=axis), np.float64)
                exp = np.asarray(exp)
                assert got.shape == exp.shape and np.array_equal(np.isnan(got), np.isnan(exp)), (what, name, axis)
                ok = ~np.isnan(exp)
                err = np.abs(got.astype(np.longdouble) - exp)
                assert np.all(err[ok] <= np.asarray(tol)[ok]), "%s: %s axis %s off by %.3e of its bound" % (
                    what, name, axis, float(np.max(err[ok] / np.maximum(np.asarray(tol)[ok], np.longdouble(1e-300)))))


@pytest.mark.parametrize("case", Z.all_cases(), ids=Z.case_id)
def test_std_mean_and_sum_far_from_zero(gpu, case):
    """cube.std(axis, ddof) for every axis form and ddof 0 / 1, under every mask, against the two-pass long-double reference of
    np.where(include, d, nan): NaN pattern identical, rtol 1e-9 per element (`constant`: plus 8 eps64 max |d|).  1e-9 because
    any two-pass evaluation, or one shifted by an included sample of its own population, is bounded by about n eps64 <= 1e-10
    at these n, while the textbook form is >= 1e-7 away.  `per_ray` is the case that one cube-wide pivot cannot pass.
    cube.mean and cube.sum of the same cubes at 1e-12: the route to std must not cost them anything."""
    family, dtype, shape = case
    d, arr, thr = Z.case(*case)
    cube = SpectralCube.read(d.copy(), HDR)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for mask in Z.MASKS:
            c, f = _masked(cube, arr, thr, mask), _filled(case, mask)
            what = "%s, mask %s" % (Z.case_id(case), mask)
            _check_std(c, f, family, d, what)
            _check_sums(c, f, family, what)


@pytest.mark.parametrize("case", Z.all_cases(), ids=Z.case_id)
def test_statistics_far_from_zero(gpu, case):
    """cube.statistics(): npts, min, max exact; sum, sumsq, mean, rms within 1e-12 of the exact sums (math.fsum).
    NO assertion on 'sigma': it stays the reference's textbook formula of those sums (dask_spectral_cube.py:810), and on these
    inputs the reference's own value is noise - std() is the number to use, and test_std_mean_and_sum_far_from_zero holds it."""
    family, dtype, shape = case
    d, arr, thr = Z.case(*case)
    cube = SpectralCube.read(d.copy(), HDR)
    for mask in Z.MASKS:
        st, ex = _masked(cube, arr, thr, mask).statistics(), Z.exact_sums(_filled(case, mask))
        for k in ("npts", "min", "max"):
            assert st[k] == ex[k], (mask, k, st[k], ex[k])
        for k in ("sum", "sumsq", "mean", "rms"):
            assert abs(st[k] - ex[k]) <= 1e-12 * abs(ex[k]), (mask, k, st[k], ex[k])
        assert "sigma" in st


def test_counts_read_through_a_bitpix_32_image(gpu, tmp_path):
    """`counts64` once more, read through a real BITPIX = 32 image with BZERO = 2^30 and BLANK: the cube is float64 and its std
    is that of the integers the file means (the textbook form gives 0 or noise at 2^30 +- 30)"""
    shape = Z.SHAPES[Z.F64][0]
    blob, d = Z.counts_fits(shape)
    path = tmp_path / "counts.fits"
    path.write_bytes(blob)
    cube = SpectralCube.read(str(path))
    assert np.array_equal(np.asarray(cube.unmasked_data), d, equal_nan=True) and np.asarray(cube.unmasked_data).dtype == np.float64
    _, arr, thr = Z.case("counts64", Z.F64, shape)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for mask in Z.MASKS:
            _check_std(_masked(cube, arr, thr, mask), _filled(("counts64", Z.F64, shape), mask), "counts64", d, "BITPIX 32, mask %s" % mask)


@pytest.mark.parametrize("family, dtype", [("pedestal32", Z.F32), ("baseline64", Z.F64)])
def test_out_of_core_std_merges_its_strips(gpu, monkeypatch, family, dtype):
    """the HBM budget lowered (as test_out_of_core_moments_and_argmax_equal_the_resident_result lowers it) until the cube goes
    through the device in at least three strips / slabs: std(axis=None), std(axis=0) and std(axis=(1, 2)) at the tolerance of
    the resident cube - this is where per-strip records are merged.  The float64 array goes up as float64 strips for this
    (streaming.wide_source): its float32 copy has a std of its own, 6e-7 away on this baseline"""
    from spectral_cube_amd import streaming
    shape = (24, 40, 16)
    d, arr, thr = Z.case(family, dtype, shape)
    monkeypatch.setenv("SPC_HBM_BUDGET", str(d.size))           # a quarter of the float32 cube
    big = SpectralCube.read(d.copy(), HDR)
    assert big._stream_source() is not None and big._dev is None
    assert streaming.plan_rows(shape, streaming.hbm_budget(0)) * 3 <= shape[1] and streaming.plan_planes(shape, streaming.hbm_budget(0), out_factor=0.0) * 3 <= shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        for mask in ("none", "array & predicate"):
            c, f = _masked(big, arr, thr, mask), Z.filled_of(d, Z.include_of(d, arr, thr, mask))
            _check_std(c, f, family, d, "out of core %s, mask %s" % (family, mask), axes=(None, 0, (1, 2)))
            assert big._dev is None, "the cube was never made resident"


def test_streamed_wide_fits_image_says_that_std_is_of_its_float32_copy(gpu, tmp_path, monkeypatch):
    """a BITPIX = 32 image larger than the HBM budget streams through the device as float32 (it is decoded there): its std is
    that of the float32 samples, and the user is told - a PrecisionWarning on the way to that number (once per source: when
    the image is opened for streaming, or else by std itself), not a silent one"""
    from spectral_cube_amd import PrecisionWarning
    shape = Z.SHAPES[Z.F64][0]
    blob, d = Z.counts_fits(shape)
    path = tmp_path / "counts.fits"
    path.write_bytes(blob)
    monkeypatch.setenv("SPC_HBM_BUDGET", str(d.size))
    with pytest.warns(PrecisionWarning):
        big = SpectralCube.read(str(path), device=0)
        assert big._stream_source() is not None
        got = big.std(axis=0)
    assert np.asarray(got).shape == shape[1:] and big._dev is None


@pytest.mark.parametrize("dtype", [Z.F32, Z.F64], ids=["float32", "float64"])
def test_strided_row_views_give_the_std_of_the_copied_rows(gpu, dtype):
    """ops.stats_axis (with "m2", what std is made of) and ops.stats_global on rows(a, b) of a `per_ray` cube - a strided view,
    as a strip of a larger cube is - against the same rows copied out: identical maps, and the std of the reference"""
    shape = Z.SHAPES[dtype][1 if dtype == Z.F32 else 0]             # (40, 8, 64): rows 1 .. 6; (33, 5, 7): rows 1 .. 3
    d, arr, thr = Z.case("per_ray", dtype, shape)
    a, b = 1, shape[1] - 1
    whole, part = DeviceArray.from_numpy(d), DeviceArray.from_numpy(np.ascontiguousarray(d[:, a:b]))
    marr, mpart = DeviceArray.from_numpy(arr), DeviceArray.from_numpy(np.ascontiguousarray(arr[:, a:b]))
    from spectral_cube_amd import _lib
    f = np.where(arr[:, a:b] != 0, d[:, a:b], np.nan)
    for axis in (0, 1, 2):
        view = ops.stats_axis(whole.rows(a, b), axis, mask=ops.MaskSpec(_lib.MASK_ARRAY, array=marr.rows(a, b)), want=("count", "sum", "m2"))
        copy = ops.stats_axis(part, axis, mask=ops.MaskSpec(_lib.MASK_ARRAY, array=mpart), want=("count", "sum", "m2"))
        for k in ("count", "sum", "m2"):
            assert np.array_equal(view[k].get(), copy[k].get(), equal_nan=True), (axis, k)
        with np.errstate(all="ignore"):
            got = np.sqrt(view["m2"].get() / view["count"].get())
        assert_close(got, Z.ref_std(f, axis, 0), rtol=Z.RTOL, what="rows view, axis %d" % axis)
    gv = ops.stats_global(whole.rows(a, b), mask=ops.MaskSpec(_lib.MASK_ARRAY, array=marr.rows(a, b)))
    gc = ops.stats_global(part, mask=ops.MaskSpec(_lib.MASK_ARRAY, array=mpart))
    ex = Z.exact_sums(f)
    for g in (gv, gc):
        assert g["npts"] == ex["npts"] and g["min"] == ex["min"] and g["max"] == ex["max"]
        assert abs(g["sum"] - ex["sum"]) <= 1e-12 * abs(ex["sum"]) and abs(g["sumsq"] - ex["sumsq"]) <= 1e-12 * ex["sumsq"]


@pytest.mark.parametrize("route", ["one kernel", "loop of kernels"])
@pytest.mark.parametrize("cen", ["median", "mean"])
@pytest.mark.parametrize("case", Z.clip_cases(), ids=Z.clip_id)
def test_sigma_clip_off_zero(gpu, monkeypatch, case, cen, route):
    """cube.sigma_clip_spectrally(3, maxiters=5, cenfunc, stdfunc='std') of float32 cubes on a pedestal - dense (the loop over
    the registers) and under a signal mask that leaves at most 128 valid samples per ray (the packed-ray loop): the NaN pattern
    equals O.sigma_clip's exactly and the survivors are bit-equal.  The kernels' bounds are float32, so a ray in which some
    oracle iteration has a valid sample within 4 ulp32(|bound|) + 1e-6 std of a bound is left out: at most 10 % of a case's
    rays (measured on the 320 rays of each case here, the oracle alone leaves out 0 to 8.4 %, test_far_from_zero_host.py).
    A pin: the variance of these loops is sumsq / n - mean^2 in float64, whose error eps64 r^2 stays under the bound's own
    rounding eps32 r at these pedestals.  *route*: the whole loop in one kernel (rays in registers, packed or not), and the
    loop of kernels that rays of more than 4096 samples take - stats_axis, spc_clip_bounds_f32, spc_clip_outside_f32 -
    which SPC_SIGMA_CLIP_FUSED=0 selects at any length."""
    if route == "loop of kernels":
        monkeypatch.setenv("SPC_SIGMA_CLIP_FUSED", "0")
    d, inc = Z.clip_case(*case)
    exp, left_out = Z.clip_oracle(d, inc, cen)
    assert left_out.mean() <= Z.CLIP_CAP
    cube = SpectralCube.read(d.copy(), HDR)
    if inc is not None:
        cube = cube.with_mask(inc)
    got = cube.sigma_clip_spectrally(3.0, maxiters=5, cenfunc=cen, stdfunc="std")._device_data().get()
    keep = ~left_out
    bad = (np.isnan(got) != np.isnan(exp)) & keep[None]
    assert not bad.any(), "%d samples in %d rays clipped differently, first %s" % (bad.sum(), bad.any(axis=0).sum(), np.argwhere(bad)[:4].tolist())
    both = ~np.isnan(exp) & keep[None]
    assert np.array_equal(got[both], exp[both])
