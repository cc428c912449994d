"""SpectralCube.downsample_axis on the device (spc_downsample_f32 / _f64), checked against the reference's results
(tests/golden/downsample_axis.npz) and a float64 numpy restatement written here - never against the library itself."""
import os
import warnings

import numpy as np
import pytest

import oracle_np as O
from conftest import assert_close, golden
from spectral_cube_amd import SpectralCube
from spectral_cube_amd.cube import PrecisionWarning
from spectral_cube_amd.wcs import parse_header

pytestmark = pytest.mark.gpu

EST = {"nanmean": np.nanmean, "nansum": np.nansum, "nanmax": np.nanmax, "nanmin": np.nanmin,
       "mean": np.mean, "sum": np.sum, "max": np.max, "min": np.min}
EXTREMA = ("nanmax", "nanmin", "max", "min")
HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 24, "CRPIX2": 16, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}


def restate(d, inc, fill, axis, f, truncate, est):
    """float64 numpy statement of the reference's in-memory downsample_axis (spectral_cube.py:3466-3497):
    (data, include) of the result"""
    x = np.where(inc, np.asarray(d, dtype=np.float64), fill)
    m = np.asarray(inc, dtype=bool)
    x, m = np.moveaxis(x, axis, 0), np.moveaxis(m, axis, 0)
    n = x.shape[0]
    if truncate:
        x, m = x[:n - n % f], m[:n - n % f]
    elif n % f:
        pad = f - n % f
        x = np.concatenate([x, np.full((pad,) + x.shape[1:], np.nan)])
        m = np.concatenate([m, np.zeros((pad,) + m.shape[1:], dtype=bool)])
    x = x.reshape((x.shape[0] // f, f) + x.shape[1:])
    m = m.reshape((m.shape[0] // f, f) + m.shape[1:])
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore", RuntimeWarning)
        r = EST[est](x, axis=1)
    return np.moveaxis(r, 0, axis), np.moveaxis(m.any(axis=1), 0, axis)


def within_one_ulp(got, exp64, what):
    """float32 result vs the float64 restatement rounded once: NaN pattern exact, at most 1 ulp apart"""
    exp = np.asarray(exp64).astype(np.float32)
    got = np.asarray(got)
    assert got.dtype == np.float32, what
    assert np.array_equal(np.isnan(got), np.isnan(exp)), what + ": NaN pattern"
    ok = np.isfinite(exp)
    assert np.array_equal(got[~ok & ~np.isnan(exp)], exp[~ok & ~np.isnan(exp)]), what + ": inf"
    diff = np.abs(got[ok].astype(np.float64) - exp[ok].astype(np.float64))
    assert diff.size == 0 or (diff <= np.spacing(np.abs(exp[ok])).astype(np.float64)).all(), what + ": more than 1 ulp"


# ---- against the reference ------------------------------------------------------------------------------
def _golden_cube(G, kind, fill):
    d = G["data"]
    cube = SpectralCube.read(d, parse_header(str(G["header"])))
    if kind == "bool":
        cube = cube.with_mask(G["keep"], inherit_mask=False)
    elif kind == "cmp":
        cube = cube.with_mask(cube > float(G["threshold"]))
    if fill == fill:
        cube = cube.with_fill_value(fill)
    return cube


def test_every_fixture_case_matches_the_reference(gpu):
    G = golden("downsample_axis.npz")
    names, offs = [str(s) for s in G["case_names"]], G["case_offsets"]
    inc_all = np.unpackbits(G["include"])[:offs[-1]].astype(bool)
    scale = float(np.nanmax(np.abs(G["data"])))
    variants = {"bool": ("bool", np.nan), "finite": ("finite", np.nan), "cmp": ("cmp", np.nan), "bool_fill0": ("bool", 0.0)}
    cubes = {k: _golden_cube(G, *v) for k, v in variants.items()}
    assert len(names) >= 200
    for i, name in enumerate(names):
        vname, rest = name.split("_a")
        a, f, t, est = rest.split("_")
        axis, factor, trunc = int(a), int(f[1:]), bool(int(t[1:]))
        ds = cubes[vname].downsample_axis(factor, axis, estimator=EST[est], truncate=trunc)
        sl = slice(offs[i], offs[i + 1])
        filled = np.asarray(ds.filled_data)
        unmasked = np.asarray(ds.unmasked_data)
        inc = ds.mask.include()
        assert filled.dtype == np.float32
        assert np.array_equal(inc.ravel(), inc_all[sl]), name + ": mask"
        for got, key in ((filled, "filled"), (unmasked, "unmasked")):
            exp = G[key][sl].reshape(got.shape)
            if est in EXTREMA:
                assert np.array_equal(got, exp, equal_nan=True), "%s %s: extrema not bit-exact" % (name, key)
            else:
                assert_close(got, exp, rtol=2e-6, atol=1e-6 * scale, what="%s %s" % (name, key))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_reference_downsample_table(gpu, dtype):
    """test_regrid.py::test_downsample on data_255 (np.arange(50.).reshape(2, 5, 5), conftest.py:422): float64 runs the
    float64 kernel, then once more as float32"""
    data = np.arange(50.).reshape(2, 5, 5).astype(dtype)
    hdr = dict(HDR, CRPIX1=3, CRPIX2=3)
    cube = SpectralCube.read(data, hdr)
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)
        ds = cube.downsample_axis(factor=2, axis=0)
        got = np.asarray(ds.filled_data)
    assert got.dtype == dtype
    np.testing.assert_almost_equal(data.mean(axis=0)[None], got)
    ds = cube.downsample_axis(factor=2, axis=1)
    exp = np.array([data[:, :2, :].mean(axis=1), data[:, 2:4, :].mean(axis=1), data[:, 4:, :].mean(axis=1)]).swapaxes(0, 1)
    assert ds.shape == (2, 3, 5)
    np.testing.assert_almost_equal(exp, np.asarray(ds.filled_data))
    ds = cube.downsample_axis(factor=2, axis=1, truncate=True)
    exp = np.array([data[:, :2, :].mean(axis=1), data[:, 2:4, :].mean(axis=1)]).swapaxes(0, 1)
    np.testing.assert_almost_equal(exp, np.asarray(ds.filled_data))


# ---- against the restatement ----------------------------------------------------------------------------
def _random_cube(shape, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(0.3, 1.0, shape).astype(np.float32)
    d[rng.random(shape) < 0.05] = np.nan
    d[:, 3, 5] = np.nan
    keep = rng.random(shape) < 0.7
    keep[:, 7, :] = False
    return d, keep


def _mask_kinds(d, keep):
    """(cube, include as the reference would see it) for the four mask kinds: none, isfinite, comparison, boolean array"""
    plain = SpectralCube(d, header=HDR)
    finite = SpectralCube.read(d, HDR)
    cmp_ = finite.with_mask(finite > 0.1)
    arr = SpectralCube(d, header=HDR).with_mask(keep)
    with np.errstate(invalid="ignore"):
        return {"none": (plain, np.ones(d.shape, bool)), "finite": (finite, np.isfinite(d)),
                "cmp": (cmp_, np.isfinite(d) & (d > 0.1)), "array": (arr, keep)}


@pytest.mark.parametrize("shape", [(37, 53, 61), (24, 32, 64)])
def test_random_shapes_every_axis_factor_mask_estimator(gpu, shape):
    d, keep = _random_cube(shape, 7 + shape[0])
    for kind, (cube, inc) in _mask_kinds(d, keep).items():
        for axis in (0, 1, 2):
            for f in (1, 2, 3, 4, 5, 6, 7, 64):
                for trunc in (False, True):
                    if trunc and f > shape[axis]:
                        continue
                    for est in EST:
                        ds = cube.downsample_axis(f, axis, estimator=EST[est], truncate=trunc)
                        er, em = restate(d, inc, np.nan, axis, f, trunc, est)
                        what = "%s %s axis %d f %d trunc %s" % (kind, est, axis, f, trunc)
                        got = np.asarray(ds.unmasked_data)
                        assert got.shape == er.shape, what
                        assert np.array_equal(ds.mask.include(), em), what + ": mask"
                        if est in EXTREMA:
                            assert np.array_equal(got, er.astype(np.float32), equal_nan=True), what
                        else:
                            within_one_ulp(got, er, what)


def test_fill_value_zero_and_infinities(gpu):
    d, keep = _random_cube((9, 10, 12), 3)
    d[2, 4, 4], d[3, 4, 4] = np.inf, -np.inf            # inf + -inf -> NaN, as numpy
    d[0, 0, 1] = np.inf
    cube = SpectralCube(d, header=HDR).with_mask(keep).with_fill_value(0.0)
    for axis in (0, 1, 2):
        for est in EST:
            ds = cube.downsample_axis(3, axis, estimator=EST[est])
            er, em = restate(d, keep, 0.0, axis, 3, False, est)
            got = np.asarray(ds.unmasked_data)
            assert np.array_equal(ds.mask.include(), em)
            if est in EXTREMA:
                assert np.array_equal(got, er.astype(np.float32), equal_nan=True), est
            else:
                within_one_ulp(got, er, "fill 0 %s axis %d" % (est, axis))


def test_float64_cube_stays_float64(gpu):
    d, keep = _random_cube((21, 18, 30), 11)
    d64 = d.astype(np.float64) * (1.0 + 1e-9)
    scale = float(np.nanmax(np.abs(d64)))
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)
        cube = SpectralCube.read(d64, HDR).with_mask(keep)
        for axis in (0, 1, 2):
            for est in ("nanmean", "nansum", "max", "nanmin"):
                ds = cube.downsample_axis(4, axis, estimator=EST[est])
                got = np.asarray(ds.unmasked_data)
                er, em = restate(d64, keep & np.isfinite(d64), np.nan, axis, 4, False, est)
                assert got.dtype == np.float64
                assert np.array_equal(ds.mask.include(), em)
                assert_close(got, er, rtol=1e-14, atol=1e-15 * scale, what="float64 %s axis %d" % (est, axis))
        m0 = cube.downsample_axis(2, 0).moment0()
    assert np.asarray(m0).dtype == np.float64


# ---- chaining ---------------------------------------------------------------------------------------------
def test_moments_of_the_downsampled_cube(gpu):
    d, keep = _random_cube((40, 24, 36), 5)
    cube = SpectralCube.read(d, HDR).with_mask(keep)
    ds = cube.downsample_axis(2, 0)
    er, em = restate(d, keep & np.isfinite(d), np.nan, 0, 2, False, "nanmean")
    cen = ds.spectral_axis - ds.spectral_axis[0]
    dv = abs(ds.wcs.cdelt[2] * ds.wcs.pc[2, 2])
    e0, e1, e2 = O.moments012(er, em, cen, dv, ds.spectral_axis[0])
    with np.errstate(all="ignore"):
        m0 = np.asarray(ds.moment0())
        got = [np.asarray(m) for m in ds.moments012()]
    assert_close(m0, e0, atol=1e-5 * np.nanmax(np.abs(e0)), what="moment0")
    assert_close(got[0], e0, atol=1e-5 * np.nanmax(np.abs(e0)), what="moments012 m0")
    ok = np.isfinite(e1) & (np.abs(e0) > 1e-2 * np.nanmax(np.abs(e0)))
    assert np.array_equal(np.isnan(got[1]), np.isnan(e1))
    assert np.abs(got[1][ok] - e1[ok]).max() <= 1e-3 * float(np.ptp(cen) + 1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("fill", [np.nan, 0.0])
def test_downsample_of_a_spectrally_interpolated_cube(gpu, dtype, fill):
    """spectral_interpolate attaches ~isnan(result) (NotNaNMask), which lowers to no kernel term: the NaN channels outside
    the input range and the NaN samples inside are EXCLUDED - filled with the fill value and left out of the new mask, as
    the reference's mask.include() / unitless_filled_data have them"""
    d, _ = _random_cube((20, 12, 14), 21)
    cube = SpectralCube.read(d.astype(dtype), HDR)
    sa = cube.spectral_axis
    grid = sa[0] + (sa[1] - sa[0]) * np.arange(-6, 26, dtype=np.float64)      # 6 channels beyond each end of the input
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        si = cube.spectral_interpolate(grid, suppress_smooth_warning=True)
        x = np.asarray(si.unmasked_data)
    inc = ~np.isnan(x)
    assert not inc[:6].any() and not inc[-6:].any() and inc.any()
    src = si if fill != fill else si.with_fill_value(fill)
    scale = float(np.nanmax(np.abs(x)))
    for axis in (0, 1, 2):
        for est in ("nanmean", "mean", "nansum", "max"):
            ds = src.downsample_axis(4, axis, estimator=EST[est])
            er, em = restate(x, inc, fill, axis, 4, False, est)
            what = "%s fill %s %s axis %d" % (np.dtype(dtype), fill, est, axis)
            assert np.array_equal(ds.mask.include(), em), what + ": mask"
            got = np.asarray(ds.unmasked_data)
            assert got.dtype == dtype, what
            if est == "max":
                assert np.array_equal(got, er.astype(dtype), equal_nan=True), what
            elif dtype == np.float32:
                within_one_ulp(got, er, what)
            else:
                assert_close(got, er, rtol=1e-14, atol=1e-15 * scale, what=what)
            if est == "max":
                assert np.array_equal(np.asarray(ds.filled_data), np.where(em, er, fill).astype(dtype), equal_nan=True), what


def test_spatial_binning_in_two_steps_equals_one(gpu):
    d, keep = _random_cube((6, 20, 24), 9)
    cube = SpectralCube(d, header=HDR).with_mask(keep)
    two = cube.downsample_axis(2, 1, estimator=np.nansum).downsample_axis(2, 2, estimator=np.nansum)
    x = np.where(keep, d.astype(np.float64), np.nan)
    exp = np.nansum(x.reshape(6, 10, 2, 12, 2), axis=(2, 4))
    assert np.array_equal(two.mask.include(), keep.reshape(6, 10, 2, 12, 2).any(axis=(2, 4)))
    assert_close(np.asarray(two.unmasked_data), exp, rtol=2e-6, atol=1e-6 * float(np.nanmax(np.abs(d))), what="2x2 nansum")
    full = np.abs(d[np.isfinite(d)]).max()
    dense = np.where(np.isfinite(d), d, 0.5).astype(np.float32)
    two = SpectralCube(dense, header=HDR).downsample_axis(2, 1).downsample_axis(2, 2)
    exp = dense.astype(np.float64).reshape(6, 10, 2, 12, 2).mean(axis=(2, 4))
    assert_close(np.asarray(two.unmasked_data), exp, rtol=4e-7, atol=4e-7 * full, what="2x2 mean")


def test_write_read_round_trip(gpu, tmp_path):
    d, keep = _random_cube((12, 14, 18), 13)
    ds = SpectralCube.read(d, HDR).with_mask(keep).downsample_axis(3, 2)
    path = str(tmp_path / "ds.fits")
    ds.write(path)
    back = SpectralCube.read(path)
    exp = np.asarray(ds.filled_data)
    assert np.array_equal(np.asarray(back.unmasked_data), exp, equal_nan=True)
    assert back.shape == ds.shape
    for k in ("CRPIX1", "CDELT1", "CRVAL1", "CRPIX3", "CDELT3"):
        assert float(back.header[k]) == pytest.approx(float(ds.header[k]), rel=1e-12, abs=1e-12), k


# ---- out of core ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["fits", "ndarray"])
def test_out_of_core_equals_resident(gpu, tmp_path, monkeypatch, source):
    from spectral_cube_amd import io_fits, streaming
    nz, ny, nx = 96, 200, 64
    d, keep = _random_cube((nz, ny, nx), 17)
    res = SpectralCube.read(d, HDR)
    budget = d.nbytes // 4
    monkeypatch.setenv("SPC_HBM_BUDGET", str(budget))
    if source == "fits":
        p = str(tmp_path / "big.fits")
        io_fits.write_fits(p, d, HDR)
        big = SpectralCube.read(p)
    else:
        big = SpectralCube.read(d.copy(), HDR)
    assert big._stream_source() is not None and big._dev is None
    for cube_s, cube_r in ((big, res), (big.with_mask(big > 0.2), res.with_mask(res > 0.2))):
        for axis in (0, 2):
            for est in (np.nanmean, np.max):
                monkeypatch.setenv("SPC_HBM_BUDGET", str(budget))
                s = cube_s.downsample_axis(8, axis, estimator=est)
                got, ginc = np.asarray(s.unmasked_data), s.mask.include()
                assert cube_s._dev is None, "the parent was never made resident"
                monkeypatch.setenv("SPC_HBM_BUDGET", str(1 << 40))
                r = cube_r.downsample_axis(8, axis, estimator=est)
                assert np.array_equal(got.view(np.uint32), np.asarray(r.unmasked_data).view(np.uint32)), (axis, est)
                assert np.array_equal(ginc, r.mask.include())
    monkeypatch.setenv("SPC_HBM_BUDGET", str(budget))
    with pytest.raises(streaming.HugeCubeError, match="bytes"):
        big.downsample_axis(2, 0)


# ---- full size --------------------------------------------------------------------------------------------
def test_full_size_1024_cubed(gpu):
    n = 1024
    rng = np.random.default_rng(2026)
    d = rng.standard_normal((n, n, n), dtype=np.float32)
    d[rng.integers(0, n, 4096), rng.integers(0, n, 4096), rng.integers(0, n, 4096)] = np.nan
    keep = rng.random((n, n, n), dtype=np.float32) < 0.8
    cube = SpectralCube(d, header=HDR).with_mask(keep)
    picks = rng.integers(0, n, (64, 2))
    for axis in (0, 1, 2):
        ds = cube.downsample_axis(2, axis)
        got = ds._device_data().get()
        inc = ds.mask.device_array().get().view(bool)
        again = cube.downsample_axis(2, axis)._device_data().get()
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32)), "two runs differ"
        del again
        for a, b in picks:
            if axis == 0:
                er, em = restate(d[:, a, b], keep[:, a, b], np.nan, 0, 2, False, "nanmean")
                g, gi = got[:, a, b], inc[:, a, b]
            else:
                er, em = restate(d[a], keep[a], np.nan, axis - 1, 2, False, "nanmean")
                g, gi = got[a], inc[a]
            assert np.array_equal(gi, em)
            within_one_ulp(g, er, "full size axis %d at %d %d" % (axis, a, b))
        del got, inc, ds
