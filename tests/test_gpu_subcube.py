"""Cutting a cube on the device (spc_subcube_f32 / _f64, spc_mask_bbox_f32 / _f64), checked against the reference's results
(tests/golden/subcube.npz) and against numpy indexing of the host arrays - a cut is a copy, so every comparison of
samples is bit for bit."""
import warnings

import numpy as np
import pytest

import oracle_np as O
from conftest import assert_close, golden
from spectral_cube_amd import Gaussian1DKernel, SpectralCube
from spectral_cube_amd.cube import PrecisionWarning
from spectral_cube_amd.wcs import parse_header
from test_subcube_host import CUTS, Q

pytestmark = pytest.mark.gpu

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 24, "CRPIX2": 16, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}
LOWER = {"chan3": (3,), "chan_box": (-2, slice(1, 6), slice(2, 9)), "spectrum": (slice(None), 2, 3), "spec_part": (slice(2, 9), 5, 0)}


def same_bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    assert np.array_equal(np.ascontiguousarray(got).view(u), np.ascontiguousarray(exp).view(u)), what + ": samples differ"


def check_cut(cut, d, inc, view, what, fill=np.nan):
    """the cut against numpy indexing of the parent's host data and include map"""
    same_bits(cut.unmasked_data, d[view], what)
    if inc is None:
        assert cut.mask is None, what
        return
    assert np.array_equal(cut.mask.include(), inc[view]), what + ": mask"
    exp = np.where(inc[view], d[view], np.asarray(fill, dtype=d.dtype))
    assert np.array_equal(np.asarray(cut.filled_data), exp, equal_nan=True), what + ": filled"


# ---- against the reference ------------------------------------------------------------------------------
def _golden_cube(G, kind, dtype=np.float32):
    d = np.asarray(G["data"]).astype(dtype)
    hdr = parse_header(str(G["header"]))
    if kind == "none":
        return SpectralCube(d, header=hdr)
    cube = SpectralCube.read(d, hdr)
    if kind == "bool":
        cube = cube.with_mask(np.asarray(G["keep"]), inherit_mask=False)
    elif kind == "cmp":
        cube = cube.with_mask(cube > float(G["threshold"]))
    return cube


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_every_fixture_view_matches_the_reference(gpu, dtype):
    G = golden("subcube.npz")
    names, offs = [str(s) for s in G["case_names"]], G["case_offsets"]
    inc_all = np.unpackbits(G["include"])[:offs[-1]].astype(bool)
    assert len(names) >= 40
    cubes = {k: _golden_cube(G, k, dtype) for k in ("none", "finite", "cmp", "bool")}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        warnings.simplefilter("error", PrecisionWarning)
        for i, name in enumerate(names):
            kind, cutname = name.split("_", 1)
            cut = CUTS[cutname](cubes[kind])
            sl = slice(offs[i], offs[i + 1])
            shape = tuple(G["shape_" + name])
            assert cut.shape == shape, name
            got = np.asarray(cut.unmasked_data)
            assert got.dtype == dtype, name
            exp = G["unmasked"][sl].reshape(shape)
            assert np.array_equal(got, exp.astype(dtype), equal_nan=True), name + ": unmasked"
            inc = cut.mask.include() if cut.mask is not None else np.ones(shape, bool)
            assert np.array_equal(inc.ravel(), inc_all[sl]), name + ": mask"
            assert np.array_equal(np.asarray(cut.filled_data), G["filled"][sl].reshape(shape).astype(dtype), equal_nan=True), name + ": filled"


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lower_dimensional_results_match_the_reference(gpu, dtype):
    G = golden("subcube.npz")
    for kind in ("none", "finite", "cmp", "bool"):
        cube = _golden_cube(G, kind, dtype)
        for name, view in LOWER.items():
            with warnings.catch_warnings():
                warnings.simplefilter("error", PrecisionWarning)
                r = cube[view]
            exp = G["lower_filled_%s_%s" % (kind, name)]
            assert r.shape == tuple(G["lower_shape_" + name]) and r.dtype == dtype, (kind, name)
            assert np.array_equal(np.asarray(r), exp.astype(dtype), equal_nan=True), (kind, name)
            assert r.unit == "K"
    cube = _golden_cube(G, "finite")
    ch = cube[3]
    crpix, cdelt, crval = G["lower_wcs_chan3"]
    assert ch.wcs.naxis == 2
    np.testing.assert_allclose(ch.wcs.crpix, crpix)
    np.testing.assert_allclose(ch.wcs.cdelt * np.diag(ch.wcs.pc), cdelt)
    np.testing.assert_allclose(ch.wcs.crval, crval)
    assert ch.header["CRVAL3"] == pytest.approx(cube.spectral_axis[3]) and ch.header["CDELT3"] == 0.5 and ch.header["CUNIT3"] == "km/s"
    # (cube[k, ys, xs]: the celestial WCS follows the slice here; the reference leaves CRPIX where it was)
    np.testing.assert_allclose(cube[-2, 1:6, 2:9].wcs.crpix, [crpix[0] - 2, crpix[1] - 1])
    sp = cube[:, 2, 3]
    crpix, cdelt, crval = G["lower_wcs_spectrum"]
    assert sp.wcs.naxis == 1
    np.testing.assert_allclose([sp.wcs.crpix[0], sp.wcs.cdelt[0] * 1e3, sp.wcs.crval[0] * 1e3], [crpix[0], cdelt[0], crval[0]])
    np.testing.assert_allclose(cube[2:9, 5, 0].wcs.spectral_pix2world(np.arange(7)), cube.spectral_axis[2:9])


def test_bounding_boxes_match_the_reference(gpu):
    G = golden("subcube.npz")
    cube = _golden_cube(G, "finite")

    def rec(sl):
        return [[-1 if s.start is None else s.start, -1 if s.stop is None else s.stop] for s in sl]

    assert rec(cube.subcube_slices_from_mask(cube > float(G["bbox_threshold"]))) == G["bbox_cmp"].tolist()
    region = np.asarray(G["bbox_region"])
    assert rec(cube.subcube_slices_from_mask(region)) == G["bbox_array"].tolist()
    assert rec(cube.subcube_slices_from_mask(region, spatial_only=True)) == G["bbox_array_spatial"].tolist()
    empty = cube.subcube_slices_from_mask(np.zeros(cube.shape, bool))
    assert empty == (slice(0),) * 3 and rec(empty) == G["bbox_empty"].tolist()
    mc = cube.with_mask(cube > float(G["bbox_threshold"])).minimal_subcube()
    assert mc.shape == tuple(G["minimal_shape"])
    assert np.array_equal(np.asarray(mc.filled_data), G["minimal_filled"], equal_nan=True)
    np.testing.assert_allclose(mc.wcs.crpix, G["minimal_wcs"][0])
    sub = cube.subcube_from_mask(region)
    assert sub.shape == (6, 3, 7)
    with pytest.raises(ValueError, match="selects nothing"):
        cube.subcube_from_mask(np.zeros(cube.shape, bool))
    with pytest.raises(ValueError, match="selects nothing"):
        cube.with_mask(np.zeros(cube.shape, bool)).minimal_subcube()


# ---- against numpy indexing -----------------------------------------------------------------------------
def _random_cube(shape, seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(0.3, 1.0, shape).astype(np.float32)
    d[rng.random(shape) < 0.05] = np.nan
    d[:, 3, 5] = np.nan
    d.view(np.uint32)[0, 0, :3] = (0x7fc00001, 0xffc12345, 0x7f800001)        # NaN payloads travel unchanged
    keep = rng.random(shape) < 0.7
    keep[:, 7, :] = False
    return d, keep


def _mask_kinds(d, keep):
    """(cube, include as the reference would see it) for the mask kinds: none, isfinite, comparison, boolean array, composite"""
    hdr = dict(HDR)
    plain = SpectralCube(d, header=hdr)
    finite = SpectralCube.read(d, hdr)
    with np.errstate(invalid="ignore"):
        return {"none": (plain, None), "finite": (finite, np.isfinite(d)),
                "cmp": (finite.with_mask(finite > 0.1), np.isfinite(d) & (d > 0.1)),
                "array": (SpectralCube(d, header=hdr).with_mask(keep), keep),
                "composite": (finite.with_mask(keep).with_mask(finite < 1.5), np.isfinite(d) & keep & (d < 1.5))}


def _random_view(rng, shape, x_aligned=None):
    view = []
    for axis, n in enumerate(shape):
        step = int(rng.integers(1, 4)) if rng.random() < 0.5 else 1
        a = int(rng.integers(0, n - 1))
        b = int(rng.integers(a + 1, n + 1))
        if axis == 0 and rng.random() < 0.25:
            view.append(slice(b - 1, a - 1 if a > 0 else None, -1))
            continue
        if axis == 2 and x_aligned is not None:
            step = 1
            a = (a // 4) * 4 if x_aligned else (a // 4) * 4 + 1 + int(rng.integers(0, 3))
            a = min(a, n - 2)
            b = max(b, a + 1)
        view.append(slice(a, b, step if step > 1 else None))
    return tuple(view)


@pytest.mark.parametrize("shape,x_aligned", [((23, 19, 61), None), ((17, 22, 64), True), ((17, 22, 64), False), ((17, 22, 64), None)],
                         ids=["odd-nx", "aligned-x", "unaligned-x", "any-x"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_random_views(gpu, shape, x_aligned, dtype):
    d, keep = _random_cube(shape, 3 + shape[2])
    d = d.astype(dtype)
    rng = np.random.default_rng(shape[0] + (0 if x_aligned is None else 1 + int(x_aligned)))
    for kind, (cube, inc) in _mask_kinds(d, keep).items():
        for trial in range(12):
            view = _random_view(rng, shape, x_aligned)
            with warnings.catch_warnings():
                warnings.simplefilter("error", PrecisionWarning)
                check_cut(cube[view], d, inc, view, "%s %s %s" % (np.dtype(dtype), kind, view))
        fill = cube.with_fill_value(-3.5)[2:9, 1:, :-1]
        check_cut(fill, d, inc, (slice(2, 9), slice(1, None), slice(None, -1)), kind + " fill", fill=-3.5)
        assert fill.fill_value == -3.5


def test_cut_of_a_cut_and_a_full_copy(gpu):
    d, keep = _random_cube((20, 16, 24), 5)
    cube = SpectralCube.read(d, HDR).with_mask(keep)
    inc = keep & np.isfinite(d)
    a = cube[3:18:2]
    b = a[1:6, ::2, 4:20]
    check_cut(b, d[3:18:2], inc[3:18:2], (slice(1, 6), slice(None, None, 2), slice(4, 20)), "cut of a cut")
    full = cube[:]
    check_cut(full, d, inc, (slice(None),) * 3, "full")
    assert full._device_data().ptr != cube._device_data().ptr, "a cut owns its memory"
    assert full.mask.device_array().shape == cube.shape


def test_cut_of_pending_results(gpu):
    d, keep = _random_cube((24, 14, 20), 8)
    cube = SpectralCube.read(d, HDR).with_mask(keep)
    view = (slice(4, 20, 3), slice(2, 12), slice(4, 16))
    sm = cube.spectral_smooth(Gaussian1DKernel(1.5))
    cut = sm[view]
    assert sm._dev is None and cut._dev is None, "still pending"
    got, ginc = np.asarray(cut.unmasked_data), cut.mask.include()
    x, xinc = np.asarray(sm.unmasked_data), sm.mask.include()
    same_bits(got, x[view], "cut of a pending spectral_smooth")
    assert np.array_equal(ginc, xinc[view])
    # spectral_interpolate attaches ~isnan(result): NaN channels outside the input range are excluded (nan_excluded)
    sa = cube.spectral_axis
    grid = sa[0] + (sa[1] - sa[0]) * np.arange(-4, 28, dtype=np.float64)
    for dtype in (np.float32, np.float64):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            si = SpectralCube.read(d.astype(dtype), HDR).spectral_interpolate(grid, suppress_smooth_warning=True)
            cut = si[2:30:2, 1:, 3:]
            got, ginc, gfill = np.asarray(cut.unmasked_data), cut.mask.include(), np.asarray(cut.with_fill_value(9.0).filled_data)
            x = np.asarray(si.unmasked_data)
        v = (slice(2, 30, 2), slice(1, None), slice(3, None))
        same_bits(got, x[v], "cut of a pending spectral_interpolate")
        assert got.dtype == dtype and not ginc[0].any() and ginc.any()
        assert np.array_equal(ginc, ~np.isnan(x[v]))
        assert np.array_equal(gfill, np.where(np.isnan(x[v]), 9.0, x[v]).astype(dtype))


def test_moments_of_a_spectral_slab(gpu):
    d, keep = _random_cube((40, 24, 36), 5)
    cube = SpectralCube.read(d, HDR).with_mask(keep)
    sa = cube.spectral_axis
    slab = cube.spectral_slab(Q(float(sa[9]) * 1e3, "m/s"), Q(float(sa[30]), "km/s"))
    assert slab.shape == (22, 24, 36)
    dd, ii = d[9:31], (keep & np.isfinite(d))[9:31]
    cen = slab.spectral_axis - slab.spectral_axis[0]
    np.testing.assert_allclose(slab.spectral_axis, sa[9:31])
    e0, e1, e2 = O.moments012(dd, ii, cen, 0.5, slab.spectral_axis[0])
    with np.errstate(all="ignore"):
        m0 = np.asarray(slab.moment0())
        got = [np.asarray(m) for m in slab.moments012()]
        box = cube[9:31, 4:20, 8:28].moment0()
    assert_close(m0, e0, atol=1e-5 * np.nanmax(np.abs(e0)), what="moment0")
    assert_close(got[0], e0, atol=1e-5 * np.nanmax(np.abs(e0)), what="moments012 m0")
    assert_close(np.asarray(box), e0[4:20, 8:28], atol=1e-5 * np.nanmax(np.abs(e0)), what="moment0 of a box")
    ok = np.isfinite(e1) & (np.abs(e0) > 1e-2 * np.nanmax(np.abs(e0)))
    assert np.array_equal(np.isnan(got[1]), np.isnan(e1))
    assert np.abs(got[1][ok] - e1[ok]).max() <= 1e-3 * float(np.ptp(cen) + 1)
    assert np.array_equal(slab.argmax(axis=0), O.argmax(dd, ii))


# ---- bounding boxes -----------------------------------------------------------------------------------------
def np_box(inc, spatial_only=False):
    """numpy restatement of ndimage.find_objects(include)[0]"""
    if not inc.any():
        return (slice(0),) * 3
    out = []
    for axis in range(3):
        hit = np.where(inc.any(axis=tuple(a for a in range(3) if a != axis)))[0]
        out.append(slice(int(hit[0]), int(hit[-1]) + 1))
    if spatial_only:
        out[0] = slice(None)
    return tuple(out)


@pytest.mark.parametrize("shape", [(23, 19, 61), (17, 22, 64)])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_minimal_subcube_boxes(gpu, shape, dtype):
    d, keep = _random_cube(shape, 31)
    d = d.astype(dtype)
    region = np.zeros(shape, bool)
    region[4:9, 5:12, 7:40] = keep[4:9, 5:12, 7:40]
    region[9, 6, 41] = True
    with np.errstate(invalid="ignore"):
        hot = d > 2.6
    finite = SpectralCube.read(d, HDR)
    dnan = d.copy()
    dnan[:3] = np.nan
    dnan[:, :, -5:] = np.nan
    dnan[:, :2] = np.nan
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cases = {"array": (SpectralCube(d, header=HDR).with_mask(region), region),
                 "predicate": (finite.with_mask(finite > 2.6), hot),
                 "composite": (finite.with_mask(region).with_mask(finite > 0.0), region & np.isfinite(d) & (d > 0.0)),
                 "finite": (SpectralCube.read(dnan, HDR), np.isfinite(dnan))}
        for name, (cube, inc) in cases.items():
            for spatial in (False, True):
                box = np_box(inc, spatial)
                assert cube.subcube_slices_from_mask(cube.mask, spatial_only=spatial) == box, name
                mc = cube.minimal_subcube(spatial_only=spatial)
                check_cut(mc, np.asarray(cube.unmasked_data), inc, box, "minimal_subcube " + name)
        plain = SpectralCube(d, header=HDR)
        assert plain.minimal_subcube().shape == shape
        # the NotNaN mask of an interpolated cube: NaN channels fall outside the box
        sa = finite.spectral_axis
        grid = sa[0] + (sa[1] - sa[0]) * np.arange(-3, shape[0] + 2, dtype=np.float64)
        si = SpectralCube(np.where(np.isnan(d), 0.25, d).astype(dtype), header=HDR).spectral_interpolate(grid, suppress_smooth_warning=True)
        assert si.subcube_slices_from_mask(si.mask)[0] == slice(3, 3 + shape[0])
        assert si.minimal_subcube().shape == shape
    for corner in ((0, 0, 0), (shape[0] - 1, shape[1] - 1, shape[2] - 1), (0, shape[1] - 1, 0), (5, 0, shape[2] - 1)):
        one = np.zeros(shape, bool)
        one[corner] = True
        assert plain.subcube_slices_from_mask(one) == tuple(slice(c, c + 1) for c in corner)
        assert plain.with_mask(one).minimal_subcube().shape == (1, 1, 1)
    assert plain.subcube_slices_from_mask(np.zeros(shape, bool)) == (slice(0),) * 3
    assert plain.subcube_slices_from_mask(np.ones((shape[0], 1, 1), bool)) == tuple(slice(0, n) for n in shape)


# ---- axes longer than a launch dimension ------------------------------------------------------------------
LONG = [(131075, 3, 5), (65536, 2, 8), (3, 131075, 5), (2, 65536, 8), (3, 5, 131075), (2, 2, 65536)]


@pytest.mark.parametrize("shape", LONG, ids=["x".join(map(str, s)) for s in LONG])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_long_axes(gpu, shape, dtype):
    rng = np.random.default_rng(sum(shape))
    d = rng.normal(0.3, 1.0, shape).astype(dtype)
    d[rng.random(shape) < 0.05] = np.nan
    keep = rng.random(shape) < 0.7
    axis = int(np.argmax(shape))
    n = shape[axis]
    cube = SpectralCube(d, header=HDR).with_mask(keep)
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)
        for sl in (slice(None), slice(1, n - 1), slice(3, None, 2), slice(70000 if n > 70000 else 65530, None)):
            view = tuple(sl if a == axis else slice(None) for a in range(3))
            check_cut(cube[view], d, keep, view, "%s %s" % (shape, sl))
        if axis == 0:
            view = (slice(None, None, -1), slice(None), slice(1, None))
            check_cut(cube[view], d, keep, view, "%s reversed" % (shape,))
        region = np.zeros(shape, bool)
        lo, hi = n // 2 - 3, n - 2
        for p in (lo, hi):
            idx = [0, 0, 0]
            idx[axis] = p
            region[tuple(idx)] = True
        box = cube.subcube_slices_from_mask(region)
        assert box == np_box(region)
        assert cube.subcube_slices_from_mask(cube.mask) == np_box(keep)


# ---- out of core ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["fits", "ndarray"])
def test_out_of_core_equals_resident(gpu, tmp_path, monkeypatch, source):
    from spectral_cube_amd import io_fits, streaming
    nz, ny, nx = 96, 200, 64
    d, keep = _random_cube((nz, ny, nx), 17)
    budget = d.nbytes // 4
    monkeypatch.setenv("SPC_HBM_BUDGET", str(budget))
    if source == "fits":
        p = str(tmp_path / "big.fits")
        io_fits.write_fits(p, d, HDR)
        big = SpectralCube.read(p)
    else:
        big = SpectralCube.read(d.copy(), HDR)
    assert big._stream_source() is not None and big._dev is None
    fin = np.isfinite(d)
    with np.errstate(invalid="ignore"):
        cases = [(big, fin), (big.with_mask(big > 0.2), fin & (d > 0.2)), (big.with_mask(keep), fin & keep)]
    views = [(slice(10, 25), slice(None), slice(None)), (slice(5, 90, 7), slice(20, 61), slice(None)),
             (slice(None), slice(100, 120), slice(8, 40)), (slice(80, 3, -1), slice(0, 200, 9), slice(1, 64, 3))]
    for cube, inc in cases:
        for view in views:
            cut = cube[view]
            check_cut(cut, d, inc, view, "%s %s" % (source, view))
            assert cube._dev is None, "the parent was never made resident"
        assert cube.subcube_slices_from_mask(cube.mask) == np_box(inc)
    reg = np.zeros(d.shape, bool)
    reg[40:50, 150:190, 3:9] = True
    assert big.subcube_slices_from_mask(reg) == np_box(reg)
    mc = big.with_mask(reg).minimal_subcube()
    check_cut(mc, d, fin & reg, np_box(fin & reg), "minimal_subcube out of core")
    assert np.array_equal(np.asarray(big[40]), np.where(fin[40], d[40], np.nan), equal_nan=True)
    with pytest.raises(streaming.HugeCubeError, match="bytes"):
        big[:]
    with pytest.raises(streaming.HugeCubeError, match="budget"):
        big[2:]


# ---- full size --------------------------------------------------------------------------------------------
def test_full_size_1024_cubed(gpu):
    n = 1024
    rng = np.random.default_rng(2026)
    d = rng.standard_normal((n, n, n), dtype=np.float32)
    d[rng.integers(0, n, 4096), rng.integers(0, n, 4096), rng.integers(0, n, 4096)] = np.nan
    keep = rng.random((n, n, n), dtype=np.float32) < 0.8
    keep[:100] = False
    keep[:, :, 900:] = False
    cube = SpectralCube(d, header=HDR).with_mask(keep)
    for view in ((slice(256, 512), slice(None), slice(None)), (slice(None), slice(255, 767), slice(257, 769)),
                 (slice(None, None, 2), slice(None, None, 2), slice(None, None, 2))):
        cut = cube[view]
        got = cut._device_data().get()
        inc = cut.mask.device_array().get().view(bool)
        assert np.array_equal(got.view(np.uint32), d[view].view(np.uint32)), view
        assert np.array_equal(inc, keep[view]), view
        del got, inc, cut
    assert cube.subcube_slices_from_mask(cube.mask) == (slice(100, n), slice(0, n), slice(0, 900))
    mc = cube.minimal_subcube()
    assert mc.shape == (n - 100, n, 900)
    assert np.array_equal(mc._device_data().get().view(np.uint32), d[100:, :, :900].view(np.uint32))
