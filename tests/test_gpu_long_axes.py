"""Every public SpectralCube operator on cubes with one axis longer than 65535 (the largest gridDim.y / gridDim.z of a launch),
against oracle/oracle_np.py or a float64 numpy restatement written here - never against the library itself.

Shapes (float32 data 0.3 + N(0, 1), ~5 % NaN, one all-NaN spaxel, one fully masked row in the boolean mask):

    long spectra   (131075, 3, 5)   > 2 x 65535: a grid-stride loop over channels runs three times; nx % 4 != 0 (scalar paths)
                   (65536, 2, 8)    first size past the limit; 16-byte rows (vector paths)
    tall planes    (3, 131075, 5), (2, 65536, 8)
    long rows      (2, 3, 200003), (2, 2, 131072)
    at the limit   (65535, 2, 8), (2, 65535, 8)
    float64        float64 copies of the long-spectra and tall-plane shapes; (1048577, 1, 4) for the float64 spectral stencil
                   that works in runs of 16 channels (more than 65535 runs)

Mask kinds: none, isfinite (read), comparison (cube > 0.1), boolean array; with_fill_value(0.0) where the operator reads
filled data.  Each operator keeps the bound of its small-shape parity test:

    operator                          shapes        compared with                        tolerance (source)
    mask.include / filled_data /      all, f64      numpy where(include, data, fill)     exact (test_gpu_downsample::test_every_fixture_case...)
      unmasked_data
    moment order 0-2, axes 0/1/2      all           O.moment                             rtol 1e-8, atol 1e-9 max|exp| (test_gpu_cube::test_consistent_mask_handling)
    moment order 3                    all           O.moment                             rtol 1e-7, atol 1e-9 max|exp| (test_gpu_cube::test_moment_order_3)
      (orders >= 1: rays whose |moment 0| is below 1e-3 of the largest divide by a cancelled sum and are compared for NaN only)
    moments012                        all           O.moments012                         1e-5 max|m0|, 1e-5 span, 1e-5 max|m2| (test_gpu_cube::test_c1_config...)
    linewidth_sigma / _fwhm           all           sqrt(O.moment order 2) (x FWHM)      atol 1e-6 max (test_gpu_cube::test_c1_config...)
    argmax / argmin, axes 0/1/2/None  all           O.argmax / O.argmin                  exact (test_gpu_cube::test_argmax_argmin_every_axis)
    sum/mean/std/max/min, None/0/1/2  all           O.reduce                             atol 1e-9 max|exp| (test_gpu_cube::test_statistics_and_reductions)
      axes (1, 2) / (0, 1) / (0, 2)   all           O.reduce                             atol 1e-6 max|exp| (same test, two axes)
    median, axes None/0/1/2           all           O.median (float32 nanmedian)         exact (test_gpu_cube::test_median_percentile_mad_std)
    percentile 10 / 90                all           O.percentile (float64)               axis 0: atol 2e-6 max; 1/2: rtol 2e-6 + atol 2e-6 max;
                                                                                         None: 2e-6 max(1, |e|) (same test)
    mad_std                           all           O.mad_std                            axis 0: atol 2e-6 max; 1/2: rtol 3e-6 + atol 3e-6 max;
                                                                                         None: 3e-6 |e| (same test)
    sigma_clip_spectrally(3)          all           O.sigma_clip                         < 2e-5 of samples disagree on clipping, kept
                                                                                         samples exact (test_gpu_fullsize::test_c2_sigma_clip...)
    statistics()                      all           O.statistics                         npts / min / max exact; rel 1e-9
                                                                                         (test_gpu_cube::test_statistics_and_reductions)
    downsample_axis, every axis,      all           restate (test_gpu_downsample)        extrema exact, others 1 ulp of the float64 value
      f = 2, 3, 1000, 1001, 4096, n                                                      (test_gpu_downsample::test_random_shapes...)
      (those up to the axis length n)
    spectral_smooth 9 / 33 taps, box  all           O.spectral_smooth                    atol 1e-5 max|exp| (test_gpu_cube::test_spectral_smooth)
    spatial_smooth 9x9, 73x73,        all           _spatial_restated (O's arithmetic,   atol 1e-5 max|exp| (test_gpu_cube::test_spatial_smooth)
      non-separable 7x7                             separable sums for the 73x73 kernel)
    spectral_interpolate              long spectra  O.spectral_interpolate               atol 1e-5 max|exp| (test_gpu_cube::test_spectral_interpolate)
    reproject (bilinear)              long spectra  O.resample_bilinear                  atol 1e-5 max|exp| (test_gpu_cube::test_reproject)
    write / read (FITS)               long spectra, the cube's filled data               exact (test_gpu_downsample::test_write_read_round_trip)
                                      tall, rows
    out of core: moment0,             (131075,3,5)  the resident cube's result           bit-identical (test_gpu_downsample::test_out_of_core...)
      downsample_axis(axis=0)
    float64: masks, moments 0-2,      f64 shapes    as above, float64                    rel 1e-12 of max|exp| (test_gpu_round5::test_float64_cube_
      reductions, statistics, both                                                       stays_float64...); downsample rtol 1e-14 + atol 1e-15 max
      smooths, downsample, clip                                                          (test_gpu_downsample::test_float64_cube_stays_float64);
                                                                                         spectral_smooth runs / ring 1e-13 (test_gpu_round6::
                                                                                         test_float64_spectral_smooth_ring_form); clip exact
"""
import warnings

import numpy as np
import pytest

import oracle_np as O
from conftest import assert_close
from spectral_cube_amd import Box1DKernel, Gaussian1DKernel, Gaussian2DKernel, SpectralCube
from test_gpu_downsample import EST, EXTREMA, restate, within_one_ulp

pytestmark = pytest.mark.gpu

LONG = [(131075, 3, 5), (65536, 2, 8)]
TALL = [(3, 131075, 5), (2, 65536, 8)]
ROWS = [(2, 3, 200003), (2, 2, 131072)]
BOUNDARY = [(65535, 2, 8), (2, 65535, 8)]
ALL = LONG + TALL + ROWS + BOUNDARY
F64 = LONG + TALL
SIGMA2FWHM = np.sqrt(8 * np.log(2))


def _hdr(shape):
    # 1e-6 deg pixels: a 200003-pixel row stays well inside the TAN projection
    nz, ny, nx = shape
    return {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-6, "CDELT2": 1e-6, "CDELT3": 0.5,
            "CUNIT3": "km/s", "CRPIX1": (nx + 1) / 2.0, "CRPIX2": (ny + 1) / 2.0, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0,
            "CRVAL3": -16.0, "BUNIT": "K"}


def _data(shape, dtype=np.float32):
    rng = np.random.default_rng(sum(shape))
    d = rng.normal(0.3, 1.0, shape).astype(np.float32)
    d[rng.random(shape, dtype=np.float32) < 0.05] = np.nan
    d[:, 0, 1] = np.nan                                      # one spaxel with no valid sample
    keep = rng.random(shape, dtype=np.float32) < 0.7
    keep[:, 1, :] = False                                   # one fully masked row
    return d.astype(dtype), keep


_CUBES = {}


def _cubes(shape, dtype=np.float32):
    """(data, {kind: (cube, include)}) - built once per shape, so each cube is uploaded once"""
    key = (shape, np.dtype(dtype).str)
    if key not in _CUBES:
        _CUBES.clear()                                      # one shape at a time in HBM and host memory
        d, keep = _data(shape, dtype)
        hdr = _hdr(shape)
        finite = SpectralCube.read(d, hdr)
        with np.errstate(invalid="ignore"):
            _CUBES[key] = (d, {"none": (SpectralCube(d, header=hdr), np.ones(shape, bool)),
                               "finite": (finite, np.isfinite(d)),
                               "cmp": (finite.with_mask(finite > 0.1), np.isfinite(d) & (d > 0.1)),
                               "array": (SpectralCube(d, header=hdr).with_mask(keep), keep)})
    return _CUBES[key]


def _ids(shapes):
    return ["x".join(map(str, s)) for s in shapes]


@pytest.fixture
def quiet():
    old = np.seterr(all="ignore")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        yield
    np.seterr(**old)


def _exact(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert np.array_equal(got, exp, equal_nan=True), "%s: %d samples differ" % (what, (got != exp).sum())


def _rel(got, exp, rtol, what):
    """float64 result: NaN pattern exact, at most rtol * max|exp| apart"""
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape and np.array_equal(np.isnan(got), np.isnan(exp)), what + ": NaN pattern"
    ok = ~np.isnan(exp)
    if ok.any():
        err = np.abs(got[ok] - exp[ok]).max()
        assert err <= rtol * np.abs(exp[ok]).max(), (what, err)


# ---- masks --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_mask_filled_unmasked(gpu, shape):
    d, kinds = _cubes(shape)
    for kind, (cube, inc) in kinds.items():
        _exact(cube.mask.include() if cube.mask is not None else np.ones(shape, bool), inc, kind + " include")
        _exact(cube.filled_data, np.where(inc, d, np.nan), kind + " filled_data")
        _exact(cube.unmasked_data, d, kind + " unmasked_data")
        _exact(cube.with_fill_value(0.0).filled_data, np.where(inc, d, np.float32(0)), kind + " filled 0")


# ---- moments and arg-extrema -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_moments_every_axis(gpu, shape, quiet):
    d, kinds = _cubes(shape)
    for kind in ("finite", "array"):
        cube, inc = kinds[kind]
        for axis in (0, 1, 2):
            cen = cube._pix_cen_axis(axis)
            size = cube._pix_size_slice(axis)
            e0 = O.moment(d, inc, 0, cen, size, axis=axis)
            scale0 = np.nanmax(np.abs(e0))
            well = np.abs(e0) >= 1e-3 * scale0
            for order in (0, 1, 2, 3):
                what = "%s moment %d axis %d" % (kind, order, axis)
                got = np.asarray(cube.moment(order=order, axis=axis), dtype=np.float64)
                exp = O.moment(d, inc, order, cen, size, axis=axis, world0=cube.spectral_axis[0])
                assert got.shape == exp.shape and np.array_equal(np.isnan(got), np.isnan(exp)), what + ": NaN pattern"
                ok = well if order else np.ones(exp.shape, bool)
                rtol = 1e-7 if order == 3 else 1e-8
                assert_close(got[ok], exp[ok], rtol=rtol, atol=1e-9 * np.nanmax(np.abs(exp[ok])), what=what)
        cen0 = cube._pix_cen_axis(0)
        dv = cube._pix_size_slice(0)
        e0, e1, e2 = O.moments012(d, inc, cen0, dv, cube.spectral_axis[0])
        m0, m1, m2 = (np.asarray(m, dtype=np.float64) for m in cube.moments012())
        span = float(np.ptp(cube.spectral_axis)) + dv
        assert_close(m0, e0, atol=1e-5 * np.nanmax(np.abs(e0)), what=kind + " moments012 m0")
        assert_close(m1, e1, atol=1e-5 * span, what=kind + " moments012 m1")
        assert_close(m2, e2, atol=1e-5 * np.nanmax(np.abs(e2)), what=kind + " moments012 m2")
        sig = np.sqrt(O.moment(d, inc, 2, cen0, dv))
        assert_close(cube.linewidth_sigma(), sig, atol=1e-6 * np.nanmax(sig), what=kind + " linewidth_sigma")
        assert_close(cube.linewidth_fwhm(), sig * SIGMA2FWHM, atol=1e-6 * np.nanmax(sig * SIGMA2FWHM), what=kind + " fwhm")


@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_argmax_argmin_every_axis(gpu, shape):
    d, kinds = _cubes(shape)
    for kind, (cube, inc) in kinds.items():
        for axis in (0, 1, 2):
            _exact(cube.argmax(axis=axis), O.argmax(d, inc, axis=axis), "%s argmax axis %d" % (kind, axis))
            _exact(cube.argmin(axis=axis), O.argmin(d, inc, axis=axis), "%s argmin axis %d" % (kind, axis))
        assert cube.argmax() == int(O.argmax(d.ravel(), inc.ravel(), axis=0)), kind + " argmax flat"
        assert cube.argmin() == int(O.argmin(d.ravel(), inc.ravel(), axis=0)), kind + " argmin flat"


# ---- reductions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_reductions_every_axis(gpu, shape, quiet):
    d, kinds = _cubes(shape)
    for kind, (cube, inc) in kinds.items():
        axes = (None, 0, 1, 2, (1, 2), (0, 1), (0, 2)) if kind in ("finite", "array") else (0, 1, (1, 2))
        for op in ("sum", "mean", "std", "max", "min"):
            for axis in axes:
                what = "%s %s axis=%s" % (kind, op, axis)
                got = np.asarray(getattr(cube, op)(axis=axis), dtype=np.float64)
                exp = np.asarray(O.reduce(d, inc, op, axis=axis), dtype=np.float64)
                if op in ("max", "min"):
                    _exact(got, exp, what)
                    continue
                tol = 1e-6 if isinstance(axis, tuple) else 1e-9
                assert_close(got, exp, atol=tol * np.nanmax(np.abs(exp)), what=what)
        st, es = cube.statistics(), O.statistics(d, inc)
        for k in ("npts", "min", "max"):
            assert st[k] == es[k], (kind, k, st[k], es[k])
        for k in ("sum", "sumsq", "mean", "sigma", "rms"):
            assert st[k] == pytest.approx(es[k], rel=1e-9), (kind, k)


# ---- order statistics ----------------------------------------------------------------------------------------------
def _nanpercentile(x, q, axis):
    """np.nanpercentile(x, q, axis) ('linear': numpy's _lerp, numpy/lib/_function_base_impl.py) without its per-ray Python
    loop: NaN sorts last, the virtual index (n - 1) q / 100 counts the non-NaN samples of each ray"""
    x = np.sort(np.moveaxis(np.asarray(x, dtype=np.float64), axis, -1), axis=-1)
    n = np.sum(~np.isnan(x), axis=-1)
    vi = (n - 1) * (q / 100.0)
    lo = np.clip(np.floor(vi).astype(np.int64), 0, None)
    hi = np.minimum(lo + 1, np.maximum(n - 1, 0))
    t = vi - np.floor(vi)
    a = np.take_along_axis(x, lo[..., None], -1)[..., 0]
    b = np.take_along_axis(x, hi[..., None], -1)[..., 0]
    diff = b - a
    out = np.where(t >= 0.5, b - diff * (1 - t), a + diff * t)
    return np.where(n > 0, out, np.nan)


def test_percentile_restatement_is_numpy_s(gpu, quiet):
    d, keep = _data((7, 9, 301))
    f = np.where(keep, d, np.nan).astype(np.float64)
    f[:, 2, :] = np.nan
    for q in (0.0, 10.0, 37.5, 50.0, 90.0, 100.0):
        for axis in (0, 1, 2):
            _exact(_nanpercentile(f, q, axis), np.nanpercentile(f, q, axis=axis), "q %g axis %d" % (q, axis))


@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_median_percentile_mad_std_every_axis(gpu, shape, quiet):
    d, kinds = _cubes(shape)
    for kind in ("finite", "array"):
        cube, inc = kinds[kind]
        f32 = np.where(inc, d, np.nan)
        f64 = f32.astype(np.float64)
        assert cube.median() == float(np.nanmedian(f32)), kind + " median"
        for q in (10.0, 90.0):
            e = float(np.nanpercentile(f64, q))
            assert abs(cube.percentile(q) - e) <= 2e-6 * max(1.0, abs(e)), (kind, q)
        em = float(np.nanmedian(np.abs(f32 - np.nanmedian(f32)))) * 1.482602218505602
        assert abs(cube.mad_std() - em) <= 3e-6 * em, kind + " mad_std"
        for axis in (0, 1, 2):
            what = "%s axis %d" % (kind, axis)
            _exact(np.asarray(cube.median(axis=axis)), O.median(d, inc, axis=axis), what + " median")
            for q in (10.0, 90.0):
                got = np.asarray(cube.percentile(q, axis=axis), dtype=np.float64)
                exp = _nanpercentile(f64, q, axis)
                scale = np.nanmax(np.abs(exp))
                assert_close(got, exp, rtol=0.0 if axis == 0 else 2e-6, atol=2e-6 * scale, what="%s percentile %g" % (what, q))
            got = np.asarray(cube.mad_std(axis=axis), dtype=np.float64)
            exp = O.mad_std(d, inc, axis=axis)
            if axis == 0:
                assert_close(got, exp, atol=2e-6 * np.nanmax(np.abs(exp)), what=what + " mad_std")
            else:
                assert_close(got, exp, rtol=3e-6, atol=3e-6 * np.nanmax(exp), what=what + " mad_std")


@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_sigma_clip_spectrally(gpu, shape):
    d, kinds = _cubes(shape)
    for kind in ("finite", "array"):
        cube, inc = kinds[kind]
        got = np.asarray(cube.sigma_clip_spectrally(3.0).unmasked_data)
        exp = O.sigma_clip(d, inc & ~np.isnan(d), 3.0)
        assert np.mean(np.isnan(got) != np.isnan(exp)) < 2e-5, kind
        ok = ~np.isnan(got) & ~np.isnan(exp)
        assert np.array_equal(got[ok], exp[ok]), kind


# ---- downsample_axis -------------------------------------------------------------------------------------------------
def _check_downsample(ds, er, em, est, what):
    got = np.asarray(ds.unmasked_data)
    assert got.shape == er.shape, what
    assert np.array_equal(ds.mask.include(), em), what + ": mask"
    if est in EXTREMA:
        assert np.array_equal(got, er.astype(got.dtype), equal_nan=True), what
    else:
        within_one_ulp(got, er, what)


@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_downsample_every_axis(gpu, shape):
    """boolean mask: every estimator at f = 3 and 1001, a sum-type and an extremum estimator at the other factors; the other
    mask kinds and fill 0 at f = 3 and 1001.  Along a long x axis, factors above 512 run ds_axis2_run_kernel: f % 4 == 0
    (1000, 4096) with 16-byte loads on 16-byte rows, 1001 without"""
    d, kinds = _cubes(shape)
    for axis in (0, 1, 2):
        n = shape[axis]
        for f in sorted(f for f in {2, 3, 1000, 1001, 4096, n} if f <= n):      # (a longer run is the whole axis, padded)
            for trunc in (False, True):
                cube, inc = kinds["array"]
                for est in (EST if f in (3, 1001) else ("nanmean", "max")):
                    er, em = restate(d, inc, np.nan, axis, f, trunc, est)
                    _check_downsample(cube.downsample_axis(f, axis, estimator=EST[est], truncate=trunc), er, em, est,
                                      "array %s axis %d f %d trunc %s" % (est, axis, f, trunc))
                if f not in (3, 1001) or trunc:
                    continue
                for kind in ("none", "finite", "cmp"):
                    cube, inc = kinds[kind]
                    for est in ("nanmean", "max"):
                        er, em = restate(d, inc, np.nan, axis, f, trunc, est)
                        _check_downsample(cube.downsample_axis(f, axis, estimator=EST[est], truncate=trunc), er, em, est,
                                          "%s %s axis %d f %d" % (kind, est, axis, f))
                cube, inc = kinds["array"]
                for est in ("nansum", "nanmin"):
                    er, em = restate(d, inc, 0.0, axis, f, trunc, est)
                    _check_downsample(cube.with_fill_value(0.0).downsample_axis(f, axis, estimator=EST[est], truncate=trunc),
                                      er, em, est, "fill 0 %s axis %d f %d" % (est, axis, f))


# ---- smoothing ---------------------------------------------------------------------------------------------------------
def _spatial_restated(d, inc, kernel2d):
    """O.spatial_smooth's arithmetic (convolve_fill_interp of every plane, float64) on the whole cube at once.  Zero
    padding is a valid zero there, so top = conv(data with NaN -> 0) and weight = sum(k) - conv(isnan); taps that never
    overlap the plane multiply zeros and are left out; a separable kernel outer(a, b) runs as two 1-D passes"""
    f = O.filled(d, inc, np.nan).astype(np.float64)
    k = np.asarray(kernel2d, dtype=np.float64)
    nz, ny, nx = f.shape
    py, px = min(k.shape[0] // 2, ny - 1), min(k.shape[1] // 2, nx - 1)
    kc = k[k.shape[0] // 2 - py:k.shape[0] // 2 + py + 1, k.shape[1] // 2 - px:k.shape[1] // 2 + px + 1][::-1, ::-1]
    u, s, vt = np.linalg.svd(kc)

    def conv(x):
        xp = np.pad(x, ((0, 0), (py, py), (px, px)))
        if s[1] <= 1e-14 * s[0]:
            a, b = u[:, 0] * s[0], vt[0]
            t = sum(b[j] * xp[:, :, j:j + nx] for j in range(2 * px + 1))
            return sum(a[i] * t[:, i:i + ny, :] for i in range(2 * py + 1))
        return sum(kc[i, j] * xp[:, i:i + ny, j:j + nx] for i in range(2 * py + 1) for j in range(2 * px + 1))

    isn = np.isnan(f)
    top = conv(np.where(isn, 0.0, f))
    bot = k.sum() - conv(isn.astype(np.float64)) if isn.any() else np.full(f.shape, k.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(bot != 0.0, top / np.where(bot != 0.0, bot, 1.0), f)


SPECTRAL_KERNELS = {"gauss9": Gaussian1DKernel(1.0), "gauss33": Gaussian1DKernel(4.0), "box5": Box1DKernel(5)}
SPATIAL_KERNELS = {"gauss9x9": Gaussian2DKernel(1.0), "gauss73x73": Gaussian2DKernel(9.0),
                   "ellipse": Gaussian2DKernel(1.5, 0.7, theta=0.6, x_size=7, y_size=7)}


@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_spectral_smooth(gpu, shape, quiet):
    assert [len(k.array) for k in SPECTRAL_KERNELS.values()] == [9, 33, 5]
    d, kinds = _cubes(shape)
    for kind in ("finite", "array"):
        cube, inc = kinds[kind]
        for name, k in SPECTRAL_KERNELS.items():
            got = cube.spectral_smooth(k)._device_data().get()
            exp = O.spectral_smooth(d, inc, k.array)
            assert_close(got, exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="%s spectral_smooth %s" % (kind, name))


@pytest.mark.parametrize("shape", ALL, ids=_ids(ALL))
def test_spatial_smooth(gpu, shape, quiet):
    """a boolean-array mask takes the split form (separable kernels), the isfinite mask the fused one"""
    assert SPATIAL_KERNELS["gauss73x73"].array.shape == (73, 73)
    d, kinds = _cubes(shape)
    for kind in ("finite", "array"):
        cube, inc = kinds[kind]
        for name, k in SPATIAL_KERNELS.items():
            got = cube.spatial_smooth(k)._device_data().get()
            exp = _spatial_restated(d, inc, k.array).astype(np.float32)
            assert_close(got, exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="%s spatial_smooth %s" % (kind, name))


def test_spatial_restatement_is_the_oracle(gpu):
    """the whole-cube restatement above equals O.spatial_smooth plane by plane (small cube)"""
    d, keep = _data((6, 17, 23))
    for k in SPATIAL_KERNELS.values():
        exp = O.spatial_smooth(d, keep, k.array)
        got = _spatial_restated(d, keep, k.array).astype(np.float32)
        assert_close(got, exp, rtol=1e-6, atol=1e-7 * np.nanmax(np.abs(exp)))


# ---- spectral axis, reprojection, files -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LONG, ids=_ids(LONG))
def test_spectral_interpolate(gpu, shape, quiet):
    d, kinds = _cubes(shape)
    cube, inc = kinds["array"]
    sa = cube.spectral_axis
    grid = np.linspace(sa[0] - 3.3, sa[-1] + 2.1, 57)                # a long cube onto a short grid (ends outside)
    got = cube.spectral_interpolate(grid, suppress_smooth_warning=True).filled_data
    exp, _ = O.spectral_interpolate(d, inc, sa, grid)
    assert_close(got, exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="long -> short")
    short = np.ascontiguousarray(d[:40])
    sc = SpectralCube.read(short, _hdr(short.shape)).with_mask(inc[:40])
    ssa = sc.spectral_axis
    grid = np.linspace(ssa[0] - 0.2, ssa[-1] + 0.2, 70001)           # a short cube onto more than 65535 channels
    got = sc.spectral_interpolate(grid, suppress_smooth_warning=True).filled_data
    exp, _ = O.spectral_interpolate(short, inc[:40] & np.isfinite(short), ssa, grid)
    assert_close(got, exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="short -> long")


@pytest.mark.parametrize("shape", LONG, ids=_ids(LONG))
def test_reproject_bilinear(gpu, shape):
    """the target is the source shifted by a fraction of a pixel (same projection and reference point): source x = x - dx"""
    d, kinds = _cubes(shape)
    cube, _ = kinds["none"]
    h = _hdr(shape)
    dx, dy = 0.3, -0.45
    target = {k: h[k] for k in ("CTYPE1", "CTYPE2", "CDELT1", "CDELT2", "CRVAL1", "CRVAL2")}
    target.update(CRPIX1=h["CRPIX1"] + dx, CRPIX2=h["CRPIX2"] + dy, NAXIS=2, NAXIS1=shape[2], NAXIS2=shape[1])
    result = cube.reproject(target)
    ys, xs = np.mgrid[0:shape[1], 0:shape[2]].astype(np.float64)
    exp, foot = O.resample_bilinear(d, xs - dx, ys - dy)
    assert result.shape == shape
    assert_close(result._device_data().get(), exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="reproject")
    assert np.array_equal(result.mask.include()[0], foot[0])


@pytest.mark.parametrize("shape", LONG + TALL[:1] + ROWS[:1], ids=_ids(LONG + TALL[:1] + ROWS[:1]))
def test_write_read_round_trip(gpu, shape, tmp_path):
    d, kinds = _cubes(shape)
    cube, inc = kinds["array"]
    path = str(tmp_path / "long.fits")
    cube.write(path)
    back = SpectralCube.read(path)
    assert back.shape == shape
    _exact(back.unmasked_data, np.where(inc, d, np.nan), "round trip")


def test_out_of_core_equals_resident(gpu, monkeypatch):
    shape = LONG[0]
    d, _ = _data(shape)
    res = SpectralCube.read(d, _hdr(shape))
    monkeypatch.setenv("SPC_HBM_BUDGET", str(d.nbytes // 4))
    big = SpectralCube.read(d.copy(), _hdr(shape))
    assert big._stream_source() is not None and big._dev is None
    for cs, cr in ((big, res), (big.with_mask(big > 0.2), res.with_mask(res > 0.2))):
        monkeypatch.setenv("SPC_HBM_BUDGET", str(d.nbytes // 4))
        m0 = np.asarray(cs.moment0(), dtype=np.float64)
        ds = cs.downsample_axis(1001, 0)
        got, ginc = np.asarray(ds.unmasked_data), ds.mask.include()
        assert cs._dev is None
        monkeypatch.setenv("SPC_HBM_BUDGET", str(1 << 40))
        assert np.array_equal(m0.view(np.uint64), np.asarray(cr.moment0(), dtype=np.float64).view(np.uint64))
        r = cr.downsample_axis(1001, 0)
        assert np.array_equal(got.view(np.uint32), np.asarray(r.unmasked_data).view(np.uint32))
        assert np.array_equal(ginc, r.mask.include())


# ---- float64 ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", F64, ids=_ids(F64))
def test_float64_operators(gpu, shape, quiet):
    d, kinds = _cubes(shape, np.float64)
    for kind in ("finite", "array"):
        cube, inc = kinds[kind]
        _exact(cube.mask.include(), inc, kind + " include")
        filled = cube.filled_data
        assert filled.dtype == np.float64
        _exact(filled, np.where(inc, d, np.nan), kind + " filled")
        cen0, dv = cube._pix_cen_axis(0), cube._pix_size_slice(0)
        for order in (0, 1, 2):
            exp = O.moment(d, inc, order, cen0, dv, world0=cube.spectral_axis[0])
            _rel(cube.moment(order=order, axis=0), exp, 1e-12, "%s f64 moment %d" % (kind, order))
        for op in ("sum", "mean", "max", "min"):
            for axis in (None, 0, 1, 2, (1, 2)):
                _rel(getattr(cube, op)(axis=axis), O.reduce(d, inc, op, axis=axis), 1e-12, "%s f64 %s axis %s" % (kind, op, axis))
        st, es = cube.statistics(), O.statistics(d, inc)
        assert (st["npts"], st["min"], st["max"]) == (es["npts"], es["min"], es["max"]), kind
        for k in ("sum", "sumsq", "mean", "rms"):
            assert abs(st[k] - es[k]) <= 1e-12 * abs(es[k]), (kind, k)
        for name, k in SPECTRAL_KERNELS.items():
            sm = cube.spectral_smooth(k).unmasked_data
            assert sm.dtype == np.float64
            _rel(sm, O.spectral_smooth(d, inc, k.array), 1e-12, "%s f64 spectral_smooth %s" % (kind, name))
        for name, k in SPATIAL_KERNELS.items():
            sp = cube.spatial_smooth(k).unmasked_data
            assert sp.dtype == np.float64
            _rel(sp, _spatial_restated(d, inc, k.array), 1e-12, "%s f64 spatial_smooth %s" % (kind, name))
        scale = float(np.nanmax(np.abs(d)))
        for axis in (0, 1, 2):
            for f in (f for f in (3, 1001) if f <= shape[axis]):
                for est in ("nanmean", "max"):
                    ds = cube.downsample_axis(f, axis, estimator=EST[est])
                    er, em = restate(d, inc, np.nan, axis, f, False, est)
                    got = np.asarray(ds.unmasked_data)
                    assert got.dtype == np.float64 and np.array_equal(ds.mask.include(), em)
                    assert_close(got, er, rtol=1e-14, atol=1e-15 * scale, what="%s f64 downsample %s axis %d f %d" % (kind, est, axis, f))
        if shape[0] <= 4096:                                   # the float64 clip (longer spectra narrow to float32)
            got = cube.sigma_clip_spectrally(3.0).unmasked_data
            exp = O.sigma_clip(d, inc & ~np.isnan(d), 3.0, out_dtype=np.float64)
            assert got.dtype == np.float64
            _exact(got, exp, kind + " f64 sigma clip")


@pytest.mark.parametrize("ring", ["default", "0"])
def test_float64_spectral_smooth_more_than_65535_runs(gpu, monkeypatch, ring, quiet):
    """(1048577, 1, 4): more than 65535 runs of 16 channels for the float64 stencil that works in runs"""
    if ring != "default":
        monkeypatch.setenv("SPC_SPECTRAL64_RING", ring)
    shape = (1048577, 1, 4)
    rng = np.random.default_rng(5)
    d = 1000.0 + 50.0 * rng.standard_normal(shape)
    d[rng.random(shape) < 0.02] = np.nan
    keep = rng.random(shape) < 0.8
    cube = SpectralCube.read(d, _hdr(shape)).with_mask(keep)
    inc = keep & ~np.isnan(d)
    for name in ("gauss9", "gauss33"):
        k = SPECTRAL_KERNELS[name].array
        got = cube.spectral_smooth(SPECTRAL_KERNELS[name]).unmasked_data
        assert got.dtype == np.float64
        _rel(got, O.spectral_smooth(d, inc, k), 1e-13, "f64 runs %s ring %s" % (name, ring))
