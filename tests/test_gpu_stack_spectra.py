"""stack_spectra on the device (spc_stack_shift_* / spc_stack_sum_*), checked against the reference's results
(tests/golden/stack_spectra.npz) and against a float64 numpy restatement written here - the reference's own lines
(fft, phase ramp over fftfreq, ifft, real part; NaN indicator shifted alongside and cut at 0.5), never the library.

Tolerance: 1e-10 * max |finite sample|, absolute: float64 sums of at most 8192 products with |h| <= 1 give about 1e-12;
loose by 100x for the device's sin / tan and the order of summation, 600x tighter than a float32 accumulation would pass.
NaN patterns must match exactly; the random cases may leave out samples whose float64 indicator lies within 1e-9 of 0.5
(at most 1e-4 of a case's samples), the committed fixture none."""
import warnings

import numpy as np
import pytest

from conftest import golden
from spectral_cube_amd import SpectralCube, BadVelocitiesWarning, HipUnsupported, ops, stack_spectra
from spectral_cube_amd.analysis_utilities import stack_plan
from spectral_cube_amd.cube import PrecisionWarning
from spectral_cube_amd.device import DeviceArray
from spectral_cube_amd.wcs import parse_header

pytestmark = pytest.mark.gpu

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 24, "CRPIX2": 16, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}
RTOL = 1e-10
NX = 7


def restate(filled, idx, shifts, pad):
    """(rows (P, M), indicator (P, M), has_nan (P,)): fourier_shift of every filled spectrum, in float64"""
    nz = filled.shape[0]
    x = filled.reshape(nz, -1)[:, np.asarray(idx)].T.astype(np.float64)
    bad = ~np.isfinite(x)
    shifts = np.asarray(shifts, dtype=np.float64)
    s = np.where(np.isfinite(shifts), shifts, 0.0)
    xp = np.pad(np.where(bad, 0.0, x), ((0, 0), tuple(pad)))
    bp = np.pad(bad.astype(np.float64), ((0, 0), tuple(pad)))
    phase = np.exp(-2j * np.pi * np.fft.fftfreq(xp.shape[1])[None, :] * s[:, None])
    rows = np.real(np.fft.ifft(np.fft.fft(xp, axis=1) * phase, axis=1))
    ind = np.real(np.fft.ifft(np.fft.fft(bp, axis=1) * phase, axis=1))
    some = bad.any(axis=1)
    rows[(ind > 0.5) & some[:, None]] = np.nan
    rows[bad.all(axis=1) | ~np.isfinite(shifts)] = np.nan
    return rows, ind, some


def scale_of(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.abs(a[np.isfinite(a)]).max())


def close(got, exp, scale, what, skip=None):
    got, exp = np.asarray(got, dtype=np.float64), np.asarray(exp, dtype=np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    use = np.ones(exp.shape, bool) if skip is None else ~skip
    assert np.array_equal(np.isnan(got)[use], np.isnan(exp)[use]), what + ": NaN pattern"
    ok = np.isfinite(exp) & use
    err = np.abs(got[ok] - exp[ok]).max() if ok.any() else 0.0
    assert err <= RTOL * scale, "%s: %.3e above %.3e" % (what, err, RTOL * scale)


def near_half(ind, some, cap=1e-4):
    skip = (np.abs(ind - 0.5) < 1e-9) & some[:, None]
    assert skip.mean() <= cap
    return skip


def dev_rows(cube, idx, shifts, pad, **kw):
    data, mask, view = cube._operand()
    return ops.stack_shift(data, idx, shifts, pad, fill=cube.fill_value, mask=mask, **kw).get().T


def dev_sums(cube, idx, shifts, pad, **kw):
    data, mask, view = cube._operand()
    return ops.stack_sum(data, idx, shifts, pad, fill=cube.fill_value, mask=mask, **kw)


# ---- against the reference ------------------------------------------------------------------------------------
def _fixture():
    G = golden("stack_spectra.npz")
    stops = np.cumsum(G["npos"])
    pkeys = [str(k) for k in G["pkeys"]]
    funcs = [str(f) for f in G["funcs"]]
    offs = np.concatenate([[0], np.cumsum(np.repeat(G["naxis1"], len(funcs)))])
    out = []
    for i, key in enumerate(str(k) for k in G["keys"]):
        variant, case = key.split("|")
        d = G[variant + "|data"]
        cube = SpectralCube(d, header=parse_header(str(G[variant + "|header"])))
        filled = d
        if case == "bool0":
            cube = cube.with_mask(G[variant + "|keep"]).with_fill_value(0.0)
            filled = np.where(G[variant + "|keep"], d, np.float32(0.0))
        idx, shifts = G["idx"][stops[i] - G["npos"][i]:stops[i]], G["shifts"][stops[i] - G["npos"][i]:stops[i]]
        kw = {}
        if G["explicit_posns"][i]:
            kw["xy_posns"] = (idx // NX, idx % NX)
        if np.isfinite(G["v0"][i]):
            kw["v0"] = float(G["v0"][i])
        for j, pkey in enumerate(pkeys):
            if pkey.startswith(key + "|"):
                stacks = {f: G["stacks"][offs[j * len(funcs) + k]:offs[j * len(funcs) + k + 1]] for k, f in enumerate(funcs)}
                out.append((pkey, cube, filled, G["vels"][i], idx, shifts, kw, tuple(int(p) for p in G["pads"][j]),
                            float(G["crpix1"][j]), int(G["naxis1"][j]), stacks, G[pkey + "|rows"] if pkey + "|rows" in G.files else None))
    return G, out


def test_fixture_through_stack_spectra(gpu):
    G, cases = _fixture()
    assert len(cases) == 30 and float(G["indicator_min_distance"]) >= 1e-6
    for pkey, cube, filled, vel, idx, shifts, kw, pad, crpix1, naxis1, stacks, rows in cases:
        scale = scale_of(filled)
        for fname, exp in stacks.items():
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                got = stack_spectra(cube, vel, stack_function=getattr(np, fname), pad_edges=pkey.endswith("pad1"), **kw)
            assert got.dtype == np.float64 and got.ndim == 1 and got.unit == cube.unit
            close(got, exp, scale, pkey + " " + fname)
            assert got.wcs.header["CRPIX1"] == crpix1 and got.wcs.header["NAXIS1"] == naxis1 == got.size
            assert got.header["CRPIX1"] == crpix1 and got.wcs.spectral_unit == cube.spectral_unit
            if pad[0]:
                assert np.allclose(got.wcs.spectral_pix2world(pad[0]), cube.spectral_axis[0])


def test_fixture_through_the_ops_wrappers(gpu):
    G, cases = _fixture()
    seen = 0
    for pkey, cube, filled, vel, idx, shifts, kw, pad, crpix1, naxis1, stacks, rows in cases:
        scale = scale_of(filled)
        total, count, nnan = dev_sums(cube, idx, shifts, pad)
        assert np.array_equal(count + nnan, np.full(naxis1, idx.size))
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            close(np.where(count > 0, total / np.maximum(count, 1), np.nan), stacks["nanmean"], scale, pkey + " sums")
        if rows is not None:
            got = dev_rows(cube, idx, shifts, pad)
            close(got, rows, scale, pkey + " rows")
            assert np.array_equal(count, np.isfinite(rows).sum(axis=0))
            seen += 1
    assert seen == 4


# ---- against the restatement ----------------------------------------------------------------------------------
def _random(shape, seed, dtype=np.float32, nan=0.05):
    rng = np.random.default_rng(seed)
    nz = shape[0]
    z = np.arange(nz)[:, None, None]
    cen = nz / 2.0 + (rng.random(shape[1:]) - 0.5) * min(8.0, nz / 3.0)
    d = (np.exp(-0.5 * ((z - cen) / 1.5) ** 2) + 0.05 * rng.normal(size=shape)).astype(dtype)
    if dtype == np.float64:
        d *= 1.0 + 1e-9                                     # samples that are no float32 numbers
    d[rng.random(shape) < nan] = np.nan
    keep = rng.random(shape) < 0.85
    return d, keep, cen


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("nz", [37, 64])
def test_random_cubes_odd_and_even_lengths(gpu, dtype, nz):
    shape = (nz, 9, 13)
    d, keep, cen = _random(shape, 100 + nz, dtype)
    d[:, 2, 3] = np.nan
    rng = np.random.default_rng(nz)
    n = shape[1] * shape[2]
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)
        for cube, filled in ((SpectralCube.read(d, HDR), d),
                             (SpectralCube(d, header=HDR).with_mask(keep).with_fill_value(0.0), np.where(keep, d, dtype(0.0)))):
            idx = rng.permutation(n)[:n - 5]
            shifts = np.round(rng.normal(0.0, 3.0, idx.size), 3)
            shifts[::7] = np.round(shifts[::7])                 # integer shifts among the fractional ones
            shifts[3] = np.nan
            shifts[4], shifts[5] = 0.5, -0.5
            for pad in ((0, 0), (int(-np.floor(np.nanmin(shifts))), int(np.ceil(np.nanmax(shifts)))), (1, 0)):   # M odd and even
                exp, ind, some = restate(filled, idx, shifts, pad)
                skip = near_half(ind, some)
                what = "%s nz %d pad %s" % (np.dtype(dtype), nz, pad)
                close(dev_rows(cube, idx, shifts, pad), exp, scale_of(filled), what, skip)
                total, count, nnan = dev_sums(cube, idx, shifts, pad)
                quiet = ~skip.any(axis=0)                       # channels where no row is undecided
                assert np.array_equal(count[quiet], np.isfinite(exp).sum(axis=0)[quiet]), what
                assert np.array_equal((count + nnan)[quiet], np.full(exp.shape[1], idx.size)[quiet])
                close(total[quiet], np.nansum(exp, axis=0)[quiet], scale_of(filled) * idx.size, what + " sum")


def test_integer_shifts_are_a_roll_and_zero_shifts_the_mean(gpu):
    nz, ny, nx = 20, 5, 6
    d, _, _ = _random((nz, ny, nx), 7, nan=0.0)
    cube = SpectralCube(d, header=HDR)
    rng = np.random.default_rng(3)
    idx = np.arange(ny * nx)
    shifts = rng.integers(-4, 6, idx.size).astype(np.float64)
    pad = (4, 5)
    got = dev_rows(cube, idx, shifts, pad)
    padded = np.pad(d.reshape(nz, -1).T.astype(np.float64), ((0, 0), pad))
    exp = np.stack([np.roll(padded[p], int(shifts[p])) for p in idx])
    assert np.array_equal(got, exp), "an integer shift moves samples bit for bit"
    got0 = dev_rows(cube, idx, shifts, (0, 0))
    assert np.array_equal(got0, np.stack([np.roll(d.reshape(nz, -1).T[p].astype(np.float64), int(shifts[p])) for p in idx]))
    vel = np.full((ny, nx), cube.spectral_axis.mean())
    for fn in (np.nanmean, np.mean, np.nansum, np.sum, np.nanmedian):
        s = stack_spectra(cube, vel, stack_function=fn)
        assert s.size == nz and s.wcs.header["CRPIX1"] == cube.wcs.spectral_only().header["CRPIX1"]
        close(s, fn(d.reshape(nz, -1).T.astype(np.float64), axis=0), scale_of(d) * (idx.size if "sum" in fn.__name__ else 1), fn.__name__)


def test_longest_spectra_and_the_limit(gpu):
    d, _, _ = _random((4096, 3, 5), 41, nan=0.002)
    cube = SpectralCube.read(d, HDR)
    idx = np.arange(15)
    shifts = np.linspace(-2047.3, 2047.6, 15)
    shifts[7] = 1024.0
    pad = (2048, 2048)
    exp, ind, some = restate(d, idx, shifts, pad)
    assert exp.shape == (15, 8192)
    skip = near_half(ind, some)
    close(dev_rows(cube, idx, shifts, pad), exp, scale_of(d), "M = 8192", skip)
    total, count, nnan = dev_sums(cube, idx, shifts, pad)
    quiet = ~skip.any(axis=0)
    assert np.array_equal(count[quiet], np.isfinite(exp).sum(axis=0)[quiet])
    close(total[quiet], np.nansum(exp, axis=0)[quiet], 15 * scale_of(d), "M = 8192 sum")
    for op in (dev_rows, dev_sums):
        with pytest.raises(HipUnsupported, match="8192"):
            op(cube, idx, shifts, (2048, 2049))
    # the most LDS a block takes: float64 samples, 8192 channels without a pad
    d64, _, _ = _random((8192, 1, 3), 43, np.float64, nan=0.001)
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)
        c64 = SpectralCube.read(d64, HDR)
        s64 = np.array([0.25, -1000.75, 4095.5])
        exp, ind, some = restate(d64, np.arange(3), s64, (0, 0))
        close(dev_rows(c64, np.arange(3), s64, (0, 0)), exp, scale_of(d64), "float64, 8192 channels", near_half(ind, some))


def test_more_than_65535_positions(gpu):
    shape = (8, 1, 70001)
    d, keep, _ = _random(shape, 5, nan=0.03)
    cube = SpectralCube.read(d, HDR).with_mask(keep)
    filled = np.where(keep, d, np.float32(np.nan))
    rng = np.random.default_rng(9)
    idx = np.arange(shape[2])
    shifts = np.round(rng.normal(0.0, 1.2, idx.size), 2)
    pad = (int(-np.floor(shifts.min())), int(np.ceil(shifts.max())))
    exp, ind, some = restate(filled, idx, shifts, pad)
    skip = near_half(ind, some)
    close(dev_rows(cube, idx, shifts, pad), exp, scale_of(d), "P = 70001 rows", skip)
    total, count, nnan = dev_sums(cube, idx, shifts, pad)
    quiet = ~skip.any(axis=0)
    assert np.array_equal(count[quiet], np.isfinite(exp).sum(axis=0)[quiet]) and np.array_equal(count + nnan, np.full(count.size, idx.size))
    close(total[quiet], np.nansum(exp, axis=0)[quiet], scale_of(d) * idx.size, "P = 70001 sum")


def test_fused_equals_the_reduction_of_the_rows_and_runs_are_bit_identical(gpu):
    shape = (48, 40, 50)
    d, keep, cen = _random(shape, 13)
    cube = SpectralCube.read(d, HDR).with_mask(keep)
    vel = cube.spectral_axis[0] + 0.5 * cen
    vel[3, 4] = np.nan
    idx, shifts, pad = stack_plan(cube, vel)
    rows = dev_rows(cube, idx, shifts, pad)
    total, count, nnan = dev_sums(cube, idx, shifts, pad)
    assert np.array_equal(count, np.isfinite(rows).sum(axis=0)) and np.array_equal(nnan, np.isnan(rows).sum(axis=0))
    close(total, np.nansum(rows, axis=0), scale_of(d) * idx.size, "fused sum against the rows")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for fn in (np.nanmean, np.mean, np.nansum, np.sum):
            close(stack_spectra(cube, vel, stack_function=fn), fn(rows, axis=0), scale_of(d) * (idx.size if "sum" in fn.__name__ else 1),
                  fn.__name__)
        for fn in (np.nanmedian, np.median, lambda a, axis: np.nanmax(a, axis=axis)):
            assert np.array_equal(stack_spectra(cube, vel, stack_function=fn), fn(rows, axis=0), equal_nan=True)
    again = dev_sums(cube, idx, shifts, pad)
    assert total.tobytes() == again[0].tobytes() and np.array_equal(count, again[1]) and np.array_equal(nnan, again[2])
    assert dev_rows(cube, idx, shifts, pad).tobytes() == rows.tobytes()
    a, b = (np.asarray(stack_spectra(cube, vel)).tobytes() for _ in range(2))
    assert a == b


def test_out_of_core_equals_resident(gpu, monkeypatch):
    from spectral_cube_amd.streaming import HugeCubeError
    nz, ny, nx = 32, 200, 64
    d, _, cen = _random((nz, ny, nx), 17)
    vel = -16.0 + 0.5 * cen
    res = SpectralCube.read(d, HDR)
    monkeypatch.setenv("SPC_HBM_BUDGET", str(d.nbytes // 4))
    big = SpectralCube.read(d.copy(), HDR)
    assert big._stream_source() is not None and big._dev is None
    for cube_s, cube_r in ((big, res), (big.with_mask(big > 0.02), res.with_mask(res > 0.02))):
        for fn in (np.nanmean, np.sum):
            monkeypatch.setenv("SPC_HBM_BUDGET", str(d.nbytes // 4))
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                s = stack_spectra(cube_s, vel, stack_function=fn)
                assert cube_s._dev is None, "the parent was not made resident"
                monkeypatch.setenv("SPC_HBM_BUDGET", str(1 << 40))
                r = stack_spectra(cube_r, vel, stack_function=fn)
            # (the strips add their partial sums in another order than one resident run: equal to the tolerance, NaN exactly)
            close(s, r, scale_of(d) * (ny * nx if fn is np.sum else 1), "out of core " + fn.__name__)
            assert s.wcs.header == r.wcs.header
    monkeypatch.setenv("SPC_HBM_BUDGET", str(d.nbytes // 4))
    with pytest.raises(HugeCubeError):
        stack_spectra(big, vel, stack_function=np.nanmedian)


def test_moment1_is_accepted_as_the_surface(gpu):
    shape = (40, 12, 14)
    d, _, cen = _random(shape, 23, nan=0.0)
    cube = SpectralCube.read(d, HDR)
    with np.errstate(all="ignore"):
        cube = cube.with_mask(cube > 0.2)
        m1 = cube.moment1()
    assert hasattr(m1, "unit") and m1.shape == shape[1:]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", BadVelocitiesWarning)
        s = stack_spectra(cube, m1)
        idx, shifts, pad = stack_plan(cube, np.asarray(m1))
    filled = np.where(d > 0.2, d, np.float32(np.nan))
    exp, ind, some = restate(filled, idx, shifts, pad)
    skip = near_half(ind, some)
    quiet = ~skip.any(axis=0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        close(np.asarray(s)[quiet], np.nanmean(exp, axis=0)[quiet], scale_of(d), "moment1 surface")
    # aligned lines: the stack peaks at the channel of v0
    assert abs(int(np.nanargmax(s)) - (pad[0] + (shape[0] - 1) / 2.0)) <= 1.0
