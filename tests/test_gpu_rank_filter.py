"""spectral_smooth_median / spectral_filter / spatial_smooth_median / spatial_filter on the device
(spc_rank_filter_axis0_* / _plane_*), checked against the reference's results (tests/golden/rank_filter.npz) and against a
numpy restatement written here - pad, sliding_window_view, np.sort, take the rank - never against the library itself.
The restatement equals scipy bit for bit on NaN-free input (tools/gen_golden_rank_filter.py asserts it before it writes the
fixture); with a NaN in the window it IS the package's rule: NaN ranks last.  Every comparison is exact."""
import warnings

import numpy as np
import pytest

from conftest import golden
from spectral_cube_amd import SpectralCube, Gaussian1DKernel
from spectral_cube_amd.cube import PrecisionWarning
from spectral_cube_amd.wcs import parse_header

pytestmark = pytest.mark.gpu

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 24, "CRPIX2": 16, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}
MODES = ("reflect", "constant", "nearest", "mirror", "wrap")
PAD = {"reflect": "symmetric", "mirror": "reflect", "nearest": "edge", "wrap": "wrap", "constant": "constant"}


def restate(x, sizes, rank, mode="reflect", cval=0.0):
    """np.sort(window)[rank] of every window of *sizes* samples: (ksize,) along axis 0, (ky, kx) along axes 1 and 2 (or
    the two axes of a plane); scipy's origin-0 window (size // 2 back, the rest forward) and boundary modes"""
    axes = (0,) if len(sizes) == 1 else tuple(range(x.ndim - 2, x.ndim))
    pads = [(0, 0)] * x.ndim
    for k, a in zip(sizes, axes):
        pads[a] = (k // 2, k - 1 - k // 2)
    kw = {"constant_values": cval} if mode == "constant" else {}
    win = np.lib.stride_tricks.sliding_window_view(np.pad(x, pads, mode=PAD[mode], **kw), sizes, axis=axes)
    return np.sort(win.reshape(x.shape + (-1,)), axis=-1)[..., rank]


def expected(d, inc, fill, sizes, rank, mode="reflect", cval=0.0):
    """the filter of the filled data; a spectrum (plane) without one included sample stays as filled
    (_apply_spectral_function / _apply_spatial_function, spectral_cube.py:147-172)"""
    x = np.where(inc, d, np.asarray(fill, dtype=d.dtype))
    r = restate(x, sizes, rank, mode, cval)
    if len(sizes) == 1:
        dead = ~inc.any(axis=0)
        r[:, dead] = x[:, dead]
    else:
        dead = ~inc.any(axis=(1, 2))
        r[dead] = x[dead]
    return r


def rank_of(name, w, extra):
    if name in ("median", "minimum", "maximum"):
        return {"median": w // 2, "minimum": 0, "maximum": w - 1}[name]
    if name == "rank":
        return extra + w if extra < 0 else extra
    p = extra + 100 if extra < 0 else extra
    return w - 1 if p == 100 else int(float(w) * p / 100.0)


def run(cube, sizes, name="median", extra=None, **kw):
    if name == "percentile":
        kw["percentile"] = extra
    if name == "rank":
        kw["rank"] = extra
    if len(sizes) == 1:
        return cube.spectral_smooth_median(sizes[0], **kw) if name == "median" else cube.spectral_filter(sizes[0], name + "_filter", **kw)
    ks = sizes[0] if sizes[0] == sizes[1] else list(sizes)
    return cube.spatial_smooth_median(ks, **kw) if name == "median" else cube.spatial_filter(ks, name + "_filter", **kw)


def same(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = ~((got == exp) | (np.isnan(got) & np.isnan(exp)))
    assert not bad.any(), "%s: %d of %d voxels differ, first at %s: got %r, expected %r" % (
        what, bad.sum(), bad.size, np.argwhere(bad)[0].tolist(), got[bad][:4].tolist(), exp[bad][:4].tolist())


# ---- against the reference ------------------------------------------------------------------------------------
def _fixture():
    G = golden("rank_filter.npz")
    hdr = parse_header(str(G["header"]))
    holes, clean, sparse, keep = G["holes"], G["clean"], G["sparse"], G["keep"]
    variants = {"finite0": (SpectralCube.read(holes, hdr).with_fill_value(0.0), holes, np.isfinite(holes), 0.0),
                "bool0": (SpectralCube(clean, header=hdr).with_mask(keep).with_fill_value(0.0), clean, keep, 0.0),
                "finitenan": (SpectralCube.read(sparse, hdr), sparse, np.isfinite(sparse), np.nan)}
    cases = []
    for i, tag in enumerate(str(s) for s in G["case_names"]):
        variant, size, name, extra, mode = tag.split("|")
        cases.append((i, tag, variant, tuple(int(k) for k in size.split("x")), name, float(extra) if extra else None, mode))
    return G, variants, cases


def test_every_fixture_case_matches_the_reference_where_scipy_is_defined(gpu):
    G, variants, cases = _fixture()
    n = G["clean"].size
    ref_all = G["filtered"].reshape(len(cases), *G["clean"].shape)
    flags = np.unpackbits(G["comparable"])[:len(cases) * n].astype(bool).reshape(ref_all.shape)
    assert len(cases) >= 120 and {c[2] for c in cases} == set(variants)
    for i, tag, variant, sizes, name, extra, mode in cases:
        cube, d, inc, fill = variants[variant]
        if extra is not None and name == "rank":
            extra = int(extra)
        out = run(cube, sizes, name, extra, mode=mode, cval=float(G["cval"]))
        got = np.asarray(out.unmasked_data)
        assert got.dtype == np.float32
        # the comparable set is recomputed from the data (windows of the filled input without a NaN) and must be the
        # recorded one: a bug cannot hide by shrinking it
        x = np.where(inc, d, np.float32(fill))
        ok = ~restate(np.isnan(x), sizes, int(np.prod(sizes)) - 1, mode, False)
        assert np.array_equal(ok, flags[i]) and int(ok.sum()) == int(G["comparable_count"][i]), tag
        assert ok.all() if variant != "finitenan" else ok.mean() >= 0.5, tag
        assert np.array_equal(got[ok], ref_all[i][ok]), "%s: %d comparable voxels differ" % (tag, (got[ok] != ref_all[i][ok]).sum())
        filled = np.asarray(out.filled_data)
        assert np.array_equal(filled[ok], np.where(inc, ref_all[i], np.float32(fill))[ok], equal_nan=True), tag + ": filled"
        assert np.array_equal(out.mask.include(), inc), tag + ": mask"


def test_every_fixture_case_matches_the_restatement_on_all_voxels(gpu):
    G, variants, cases = _fixture()
    for i, tag, variant, sizes, name, extra, mode in cases:
        cube, d, inc, fill = variants[variant]
        rank = rank_of(name, int(np.prod(sizes)), int(extra) if name == "rank" else extra)
        out = run(cube, sizes, name, int(extra) if name == "rank" else extra, mode=mode, cval=float(G["cval"]))
        same(out.unmasked_data, expected(d, inc, fill, sizes, rank, mode, float(G["cval"])), tag)


def test_reference_table(gpu):
    """spectral_cube/tests/test_spectral_cube.py:2448-2519 on data_adv"""
    adv = golden("adv_argmax.npz")["data"].astype(np.float32)
    hdr = dict(HDR, CRPIX1=1, CRPIX2=1)
    cube = SpectralCube.read(adv, hdr)
    med = np.asarray(cube.spatial_smooth_median(3).filled_data)
    np.testing.assert_almost_equal(med[0], np.array([[0.8172354, 0.9038805], [0.7068793, 0.8172354], [0.7068793, 0.7068793]]))
    np.testing.assert_almost_equal(med[2], np.array([[0.3038468, 0.3038468], [0.303744, 0.3038468], [0.1431722, 0.303744]]))

    class maximum_filter:                           # a stand-in: only the name is read
        __name__ = "maximum_filter"
    mx = np.asarray(cube.spatial_filter([3, 3], filter=maximum_filter(), num_cores=1).filled_data)
    np.testing.assert_almost_equal(mx[0], np.array([[0.90950237, 0.90950237], [0.90950237, 0.90950237], [0.90388047, 0.90388047]]))
    smx = np.asarray(cube.spectral_filter(3, filter="maximum_filter", num_cores=None).filled_data)
    np.testing.assert_almost_equal(smx[:, 1, 1], np.array([0.90388047, 0.90388047, 0.96629004, 0.96629004]))
    smed = np.asarray(cube.spectral_smooth_median(3, num_cores=1).filled_data)
    np.testing.assert_almost_equal(smed[:, 1, 1], np.array([0.9038805, 0.1431722, 0.1431722, 0.9662900]))


# ---- against the restatement ----------------------------------------------------------------------------------
def _random(shape, seed, dtype=np.float32, nan=0.10):
    rng = np.random.default_rng(seed)
    d = rng.normal(0.3, 1.0, shape).astype(dtype)
    if dtype == np.float64:
        d *= 1.0 + 1e-9                                     # samples that are no float32 numbers
    d[rng.random(shape) < nan] = np.nan
    d.flat[::17] = d.flat[min(3, d.size - 1)]                                # ties
    keep = rng.random(shape) < 0.7
    return d, keep


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_spectral_every_size_and_mode(gpu, dtype):
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)
        for shape, sizes in (((37, 29, 43), list(range(1, 13)) + [33, 65]), ((70, 9, 11), [10, 33, 65, 129]), ((131, 5, 8), [129, 64])):
            d, _ = _random(shape, 11 + shape[0], dtype)
            cube = SpectralCube.read(d, HDR)                # isfinite mask, NaN fill: windows with NaN all over
            inc = np.isfinite(d)
            for n, k in enumerate(sizes):
                mode = MODES[n % 5]
                for name, extra in (("median", None), ("rank", -1 if n % 2 else 0), ("percentile", 25.0)):
                    out = run(cube, (k,), name, extra, mode=mode, cval=-0.5)
                    same(out.unmasked_data, expected(d, inc, np.nan, (k,), rank_of(name, k, extra), mode, -0.5),
                         "%s %s ksize %d %s %s" % (np.dtype(dtype), shape, k, name, mode))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_spatial_every_size_and_mode(gpu, dtype):
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)
        shape = (5, 37, 43)
        d, _ = _random(shape, 23, dtype)
        cube = SpectralCube.read(d, HDR)
        inc = np.isfinite(d)
        sizes = [(k, k) for k in (1, 2, 3, 4, 5, 6, 7, 11, 15)] + [(3, 5), (5, 3), (1, 7), (15, 2), (4, 9)]
        for n, s in enumerate(sizes):
            mode = MODES[n % 5]
            w = s[0] * s[1]
            for name, extra in (("median", None), ("rank", -1 if n % 2 else 0), ("percentile", 70.0)):
                out = run(cube, s, name, extra, mode=mode, cval=1.25)
                same(out.unmasked_data, expected(d, inc, np.nan, s, rank_of(name, w, extra), mode, 1.25),
                     "%s %s ksize %s %s %s" % (np.dtype(dtype), shape, s, name, mode))


def test_axes_of_length_one_two_three(gpu):
    for shape in ((1, 5, 6), (2, 5, 6), (3, 4, 5), (4, 1, 7), (4, 2, 3), (4, 3, 1), (1, 1, 1), (2, 2, 2)):
        d, _ = _random(shape, sum(shape), nan=0.15)
        cube = SpectralCube.read(d, HDR)
        inc = np.isfinite(d)
        for mode in MODES:
            for k in range(1, 2 * shape[0] + 2):
                same(run(cube, (k,), mode=mode, cval=0.5).unmasked_data, expected(d, inc, np.nan, (k,), k // 2, mode, 0.5),
                     "%s spectral %d %s" % (shape, k, mode))
            for ky in range(1, min(2 * shape[1] + 2, 8)):
                for kx in range(1, min(2 * shape[2] + 2, 8)):
                    same(run(cube, (ky, kx), mode=mode, cval=0.5).unmasked_data,
                         expected(d, inc, np.nan, (ky, kx), ky * kx // 2, mode, 0.5), "%s spatial %dx%d %s" % (shape, ky, kx, mode))


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_masks_and_fill_values(gpu, dtype):
    shape = (21, 18, 30)
    d, keep = _random(shape, 31, dtype)
    keep[:, 3, 4] = False
    keep[6] = False
    d[:, 7, 9] = np.nan
    d[11] = np.nan
    plain = SpectralCube(d, header=HDR)
    finite = SpectralCube.read(d, HDR)
    with np.errstate(invalid="ignore"):
        kinds = {"none": (plain, np.ones(shape, bool)), "finite": (finite, np.isfinite(d)),
                 "cmp": (finite.with_mask(finite > 0.1), np.isfinite(d) & (d > 0.1)),
                 "array": (plain.with_mask(keep), keep),
                 "array+cmp": (finite.with_mask(keep).with_mask(finite < 1.0), keep & np.isfinite(d) & (d < 1.0))}
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)
        for kind, (cube, inc) in kinds.items():
            for fill in (np.nan, 0.0, np.inf):
                c = cube if fill != fill else cube.with_fill_value(fill)
                for sizes, mode in (((3,), "reflect"), ((4,), "constant"), ((9,), "constant"), ((17,), "mirror"),
                                    ((3, 3), "constant"), ((5, 5), "wrap"), ((2, 7), "constant")):
                    w = int(np.prod(sizes))
                    for name, extra in (("median", None), ("maximum", None)):
                        out = run(c, sizes, name, extra, mode=mode, cval=2.5)
                        exp = expected(d, inc, fill, sizes, rank_of(name, w, extra), mode, 2.5)
                        what = "%s %s fill %s %s %s %s" % (np.dtype(dtype), kind, fill, sizes, name, mode)
                        same(out.unmasked_data, exp, what)
                        same(out.filled_data, np.where(inc, exp, np.asarray(fill, dtype=dtype)), what + " filled")
                        assert out.mask is c.mask and (c.mask is None or np.array_equal(out.mask.include(), inc))


def test_pending_and_cut_parents_and_chaining(gpu):
    d, keep = _random((40, 24, 36), 5, nan=0.03)
    cube = SpectralCube.read(d, HDR).with_mask(keep)
    inc = keep & np.isfinite(d)
    with np.errstate(all="ignore"):
        sm = cube.spectral_smooth(Gaussian1DKernel(1.5))
        smd = np.asarray(sm.unmasked_data)
        same(cube.spectral_smooth(Gaussian1DKernel(1.5)).spectral_smooth_median(3).unmasked_data,
             expected(smd, inc, np.nan, (3,), 1), "median of a pending smooth")
    cut = cube[3:20, 2:, ::2]
    dc, ic = d[3:20, 2:, ::2], inc[3:20, 2:, ::2]
    same(cut.spectral_smooth_median(5).unmasked_data, expected(dc, ic, np.nan, (5,), 2), "cut parent, spectral")
    same(cut.spatial_smooth_median(3).unmasked_data, expected(dc, ic, np.nan, (3, 3), 4), "cut parent, spatial")
    first = expected(d, inc, np.nan, (5,), 2)
    chain = cube.spectral_smooth_median(5).spatial_smooth_median((3, 5), mode="nearest")
    same(chain.unmasked_data, expected(first, inc, np.nan, (3, 5), 7, "nearest"), "spectral then spatial")
    assert np.array_equal(chain.mask.include(), inc)
    m0 = np.asarray(cube.spectral_smooth_median(3).moment0())
    assert m0.shape == (24, 36) and np.isfinite(m0).any()


# ---- long axes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(131075, 3, 5), (65536, 2, 8), (3, 131075, 5), (2, 65536, 8), (2, 3, 200003), (2, 2, 131072)],
                         ids=lambda s: "x".join(map(str, s)))
def test_axes_longer_than_65535(gpu, shape):
    d, keep = _random(shape, sum(shape), nan=0.05)
    cube = SpectralCube.read(d, HDR).with_mask(keep)
    inc = keep & np.isfinite(d)
    spectral = [k for k in (2, 5, 33) if k // 2 <= shape[0]]
    spatial = [s for s in ((3, 3), (2, 5), (5, 5), (7, 1)) if s[0] // 2 <= shape[1] and s[1] // 2 <= shape[2]]
    for k in spectral:
        for mode in ("reflect", "constant"):
            same(run(cube, (k,), mode=mode, cval=1.0).unmasked_data, expected(d, inc, np.nan, (k,), k // 2, mode, 1.0),
                 "%s spectral %d %s" % (shape, k, mode))
    for s in spatial:
        for mode in ("mirror", "constant"):
            same(run(cube, s, mode=mode, cval=1.0).unmasked_data, expected(d, inc, np.nan, s, s[0] * s[1] // 2, mode, 1.0),
                 "%s spatial %s %s" % (shape, s, mode))


# ---- out of core ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["fits", "ndarray"])
def test_out_of_core_equals_resident(gpu, tmp_path, monkeypatch, source):
    from spectral_cube_amd import io_fits
    nz, ny, nx = 96, 200, 64
    d, _ = _random((nz, ny, nx), 17, nan=0.05)
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
        for sizes, mode in (((5,), "reflect"), ((12,), "constant"), ((3, 3), "reflect"), ((4, 7), "constant")):
            monkeypatch.setenv("SPC_HBM_BUDGET", str(budget))
            s = run(cube_s, sizes, mode=mode, cval=0.75)
            got = np.empty((nz, ny, nx), np.float32)
            s.stream_into(got)
            assert cube_s._dev is None and s._dev is None, "neither the parent nor the result was made resident"
            monkeypatch.setenv("SPC_HBM_BUDGET", str(1 << 40))
            r = np.asarray(run(cube_r, sizes, mode=mode, cval=0.75).filled_data)
            assert np.array_equal(got.view(np.uint32), r.view(np.uint32)), (sizes, mode)


# ---- full size ------------------------------------------------------------------------------------------------
def test_full_size_1024_cubed(gpu):
    n = 1024
    rng = np.random.default_rng(2026)
    d = rng.standard_normal((n, n, n), dtype=np.float32)
    d[rng.integers(0, n, 4096), rng.integers(0, n, 4096), rng.integers(0, n, 4096)] = np.nan
    keep = rng.random((n, n, n), dtype=np.float32) < 0.8
    cube = SpectralCube(d, header=HDR).with_mask(keep)
    got = cube.spectral_smooth_median(5)._device_data().get()
    for a, b in rng.integers(0, n, (64, 2)):
        col, inc = d[:, a:a + 1, b:b + 1], keep[:, a:a + 1, b:b + 1]
        same(got[:, a:a + 1, b:b + 1], expected(col, inc, np.nan, (5,), 2), "1024^3 spectral at %d %d" % (a, b))
    del got
    got = cube.spatial_smooth_median(3)._device_data().get()
    for z in rng.integers(0, n, 8):
        same(got[z:z + 1], expected(d[z:z + 1], keep[z:z + 1], np.nan, (3, 3), 4), "1024^3 spatial plane %d" % z)
