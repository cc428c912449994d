"""CPU: combine_headers / mosaic_cubes (spectral_cube_amd/cube_utils.py) without a device - the header arithmetic against the
recorded pairs of tests/golden/mosaic.npz (tools/gen_golden_mosaic.py: the reference's combine_headers / mosaic_cubes on top
of this project's stand-in for the reproject package), a float64 numpy restatement of the accumulation against the
recorded mosaics, routing, keyword errors, exports."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_np as O
from conftest import REPO, golden
from spectral_cube_amd import (_lib, cube_utils, ops, SpectralCube, SimpleWCS, HipLibraryError, combine_headers,
                               mosaic_cubes)
from spectral_cube_amd.wcs import parse_header, reproject_pixel_map

G = golden("mosaic.npz")
PAIRS = [str(n) for n in G["pairs"]]
KEYS = [str(k) for k in G["keys"]]
MOSAICS = [("three", "nearest-neighbor"), ("three", "bilinear"), ("split", "nearest-neighbor")]
ORDER = {"nearest-neighbor": 0, "bilinear": 1}
# tests/test_wcs_strict.py: positions on the sky within 2e-12 degrees (1e-9 pixel of a 2 arcsec grid), pixels within 1e-9
SKY_TOL, PIX_TOL = 2e-12, 1e-9


def pair(name):
    key = "pair|%s|" % name
    kw = {}
    if key + "kwargs" in G.files:
        res, lon, lat = (float(v) for v in G[key + "kwargs"])
        kw = {"projection": str(G[key + "projection"]), "resolution": res, "reference": (lon, lat)}
    return parse_header(str(G[key + "h1"])), parse_header(str(G[key + "h2"])), kw, key


def corners(h):
    w = SimpleWCS(h, naxis=2)
    nx, ny = int(h["NAXIS1"]), int(h["NAXIS2"])
    return w.celestial_pix2world(np.array([-0.5, nx - 0.5, nx - 0.5, -0.5]), np.array([-0.5, -0.5, ny - 0.5, ny - 0.5]))


@pytest.mark.parametrize("name", PAIRS)
def test_combine_headers_against_the_recorded_pairs(name):
    h1, h2, kw, key = pair(name)
    res = combine_headers(h1, h2, **kw)
    exp = dict(zip(KEYS, G[key + "values"]))
    assert [res["CTYPE1"], res["CTYPE2"]] == [str(c) for c in G[key + "ctype"]]
    assert [res["NAXIS1"], res["NAXIS2"]] == [int(n) for n in G[key + "naxis"]]             # exact
    assert res["NAXIS"] == 3 and res["WCSAXES"] == 3 and res["NAXIS3"] == h1["NAXIS3"]
    coslat = np.cos(np.radians(exp["CRVAL2"]))
    assert abs(res["CRVAL1"] - exp["CRVAL1"]) * coslat <= SKY_TOL and abs(res["CRVAL2"] - exp["CRVAL2"]) <= SKY_TOL
    assert abs(res["CRPIX1"] - exp["CRPIX1"]) <= PIX_TOL and abs(res["CRPIX2"] - exp["CRPIX2"]) <= PIX_TOL
    assert abs(res["CDELT1"] - exp["CDELT1"]) <= SKY_TOL and abs(res["CDELT2"] - exp["CDELT2"]) <= SKY_TOL
    assert res["CTYPE3"] == h1["CTYPE3"] and res["CRVAL3"] == h1["CRVAL3"] and res["BUNIT"] == h1["BUNIT"]
    assert not any(re.match(r"^(PC|CD)\d_\d$|^CROTA\d$", k) for k in res)                  # the target is unrotated
    # astropy's pixel maps of both inputs on the recorded grid, through this package's WCS on ITS grid
    wout = SimpleWCS(res)
    for tag, h in (("1", h1), ("2", h2)):
        xs, ys = reproject_pixel_map(SimpleWCS(h, naxis=2), wout, (res["NAXIS2"], res["NAXIS1"]))
        assert np.abs(xs - G[key + "xs" + tag]).max() <= 2 * PIX_TOL and np.abs(ys - G[key + "ys" + tag]).max() <= 2 * PIX_TOL


def test_a_header_combined_with_itself_keeps_its_grid():
    """the reference test's assertion (tests/test_regrid.py:613, 627-631) for an unrotated TAN header"""
    h1, _, _, _ = pair("identical")
    res = combine_headers(h1, h1)
    assert (res["NAXIS1"], res["NAXIS2"], res["NAXIS3"]) == (h1["NAXIS1"], h1["NAXIS2"], h1["NAXIS3"])
    for k in KEYS:
        assert abs(res[k] - h1[k]) <= (PIX_TOL if k.startswith("CRPIX") else SKY_TOL), k
    assert (res["CTYPE1"], res["CTYPE2"]) == (h1["CTYPE1"], h1["CTYPE2"])


@pytest.mark.parametrize("name", PAIRS)
def test_the_corners_of_both_inputs_lie_inside_the_result(name):
    """The near edge of the result is the smallest corner coordinate exactly (0-based -0.5).  The far edge follows from
    NAXISn = round(max - min): the largest corner coordinate lies within half a pixel of n - 0.5 - at or inside it when
    the extent rounds up (so for a header combined with itself), up to half a pixel beyond it when it rounds down (the
    recorded ``offset`` pair: an extent of 18.17 x 12.50 pixels gives 18 x 13, the far corner in x at n - 0.5 + 0.17).
    'Inside [-0.5, n - 0.5]' without that half pixel cannot hold together with round(); the reference has round()."""
    h1, h2, kw, _ = pair(name)
    res = combine_headers(h1, h2, **kw)
    w = SimpleWCS(res, naxis=2)
    assert SimpleWCS(h1, naxis=2).frame == SimpleWCS(h2, naxis=2).frame == w.frame        # (the recorded pairs share a frame)
    both = np.concatenate([np.stack(w.celestial_world2pix(*corners(h))) for h in (h1, h2)], axis=1)
    for c, n in ((both[0], res["NAXIS1"]), (both[1], res["NAXIS2"])):
        assert abs(c.min() + 0.5) <= PIX_TOL
        assert n == int(round(c.max() - c.min())) and abs(c.max() - (n - 0.5)) <= 0.5 + PIX_TOL
        if (c.max() - c.min()) % 1.0 >= 0.5 or name == "identical":
            assert c.max() <= n - 0.5 + PIX_TOL


@pytest.mark.parametrize("name", [n for n in PAIRS if n != "sin_tan"])
def test_the_result_is_symmetric_in_its_arguments(name):
    h1, h2, kw, _ = pair(name)
    a, b = combine_headers(h1, h2, **kw), combine_headers(h2, h1, **kw)
    for k in KEYS + ["NAXIS1", "NAXIS2", "CTYPE1", "CTYPE2", "CUNIT1", "CUNIT2"]:
        assert a[k] == b[k] or abs(a[k] - b[k]) <= 1e-12, k


def test_keyword_errors():
    h1, h2, _, _ = pair("offset")
    with pytest.raises(NotImplementedError, match="frame"):
        combine_headers(h1, h2, frame="galactic")
    with pytest.raises(NotImplementedError, match="bogus"):
        combine_headers(h1, h2, bogus=1)
    with pytest.raises(TypeError, match="auto_rotate"):
        combine_headers(h1, h2, auto_rotate=False)
    with pytest.raises(NotImplementedError, match="ZPN"):
        combine_headers(h1, h2, projection="ZPN")
    cube = SpectralCube(np.zeros((2, 3, 4), np.float32), header=h1)
    with pytest.raises(ValueError, match="empty"):
        mosaic_cubes([])
    with pytest.raises(TypeError, match="bogus"):
        mosaic_cubes([cube], bogus=1)
    with pytest.raises(ValueError, match="order"):
        mosaic_cubes([cube], order="quintic")


# ---- the accumulation, restated in float64 numpy ------------------------------------------------------------------
def restate_mosaic(sources, header, order, zs=None):
    """(mosaic, weight) of cube_utils.py:810-856 in float64: *sources* = [(data, header, include or None, fill)], include
    None = the finite-value mask; per source the filled data resampled with the oracle at this package's pixel map, the
    cube's fill value outside its footprint, nan_to_num, summed in list order; the weight is the footprint of channel 0.
    *zs*: optional per-source fractional channel positions of the target's channels (None = the same channels)."""
    wout = SimpleWCS(header)
    shape_yx = (int(header["NAXIS2"]), int(header["NAXIS1"]))
    final, weight = None, np.zeros(shape_yx)
    for s, (data, h, include, fill) in enumerate(sources):
        d = np.asarray(data, dtype=np.float64)
        inc = np.isfinite(d) if include is None else np.asarray(include, dtype=bool)
        filled = np.where(inc, d, fill)
        xs, ys = reproject_pixel_map(SimpleWCS(h, naxis=2), wout, shape_yx)
        if zs is not None and zs[s] is not None:
            assert order == 1
            res, foot = O.reproject_separable(filled, xs, ys, zs[s])
        else:
            res, foot = (O.resample_nearest if order == 0 else O.resample_bilinear)(filled, xs, ys)
        term = np.nan_to_num(np.where(foot, res, fill))
        final = term if final is None else final + term
        weight += foot[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        return final / weight, weight


def recorded_sources(name):
    key = "mos|%s|" % name
    out = []
    for s in range(int(G[key + "n"])):
        keep = G[key + "keep%d" % s]
        out.append((G[key + "data%d" % s], parse_header(str(G[key + "header%d" % s])), keep if keep.size else None,
                    float(G[key + "fill%d" % s])))
    return out, parse_header(str(G[key + "header"])), key


@pytest.mark.parametrize("name,order", MOSAICS)
def test_the_restatement_reproduces_the_recorded_mosaics(name, order):
    sources, header, key = recorded_sources(name)
    exp = G[key + "result|" + order]
    got, weight = restate_mosaic(sources, header, ORDER[order])
    assert np.array_equal(weight, G[key + "weight"])
    assert np.array_equal(np.isnan(got), np.isnan(exp))                                   # the NaN pattern exactly
    ok = np.isfinite(exp)
    assert np.abs(got[ok] - exp[ok]).max() <= 1e-5 * np.abs(exp[ok]).max()
    if name == "three":
        w = G[key + "weight"]
        assert (w >= 2).mean() >= 0.10 and w.max() == 3 and (w == 0).mean() >= 0.10 and float(G["margin"]) >= 1e-6


def test_the_header_of_the_recorded_mosaic_is_the_pairwise_combination_in_list_order():
    sources, header, _ = recorded_sources("three")
    h = sources[0][1]
    for _, hs, _, _ in sources[1:]:
        h = combine_headers(h, hs)
    assert (h["NAXIS1"], h["NAXIS2"], h["NAXIS3"]) == (header["NAXIS1"], header["NAXIS2"], header["NAXIS3"])
    # the reference writes every intermediate header as text of 14 significant digits: half a unit of the 14th digit per
    # value and step, carried into the CRPIX of the next step through the grid spacing
    for k in KEYS:
        digits = 2 * 5e-14 * max(abs(header["CRVAL1"]), abs(header["CRPIX1"]))
        tol = (PIX_TOL + digits / abs(header["CDELT2"])) if k.startswith("CRPIX") else (SKY_TOL + digits)
        assert abs(h[k] - header[k]) <= tol, k


# ---- routing ------------------------------------------------------------------------------------------------------
class _StandInArray:
    """what ops.py reads of a DeviceArray, without a device"""

    def __init__(self, shape, dtype, device=0):
        self.shape, self.dtype, self.device, self.ptr = tuple(int(n) for n in shape), np.dtype(dtype), device, 0x1000
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize

    @classmethod
    def from_numpy(cls, arr, device=0, stream=None, dtype=None):
        a = np.asarray(arr, dtype=dtype)
        return cls(a.shape, a.dtype, device)


class _Reprojected:
    def __init__(self, shape):
        self.shape = shape
        self.filled_data = np.ones(shape, np.float32)

    def get_mask_array(self):
        return np.ones(self.shape, bool)


@pytest.fixture
def recorded(monkeypatch):
    import spectral_cube_amd.device as D
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)
    monkeypatch.setattr(ops, "DeviceArray", _StandInArray)
    monkeypatch.setattr(D, "DeviceArray", _StandInArray)
    monkeypatch.setattr(SpectralCube, "_device_data", lambda self: _StandInArray(self.shape, np.float32))
    monkeypatch.setattr(SpectralCube, "_runs_wide", lambda self: False)
    monkeypatch.setattr(SpectralCube, "_stream_source", lambda self: None)

    def fake_reproject(self, header, order="bilinear", filled=True, **kw):
        w = header if isinstance(header, SimpleWCS) else SimpleWCS(header)
        calls.append(("reproject", (order, filled)))
        return _Reprojected((int(w.header["NAXIS3"]), int(w.header["NAXIS2"]), int(w.header["NAXIS1"])))
    monkeypatch.setattr(SpectralCube, "reproject", fake_reproject)
    return calls


def _two_cubes(shift=0.0, nz=5):
    h1, h2, _, _ = pair("offset")
    h1, h2 = dict(h1, NAXIS3=nz), dict(h2, NAXIS3=nz, CRVAL3=h2["CRVAL3"] + shift)
    a = SpectralCube(np.zeros((nz, h1["NAXIS2"], h1["NAXIS1"]), np.float32), header=h1)
    b = SpectralCube(np.zeros((nz, h2["NAXIS2"], h2["NAXIS1"]), np.float32), header=h2)
    return a, b


def test_routing_one_kernel_or_reproject_per_cube(recorded):
    calls = recorded
    a, b = _two_cubes()
    for order in ("nearest-neighbor", "bilinear", 0, 1):
        del calls[:]
        out = mosaic_cubes([a, b], order=order, spectral_block_size=None, use_memmap=False, roundtrip_coords=False, block_size=None)
        names = [c[0] for c in calls]
        assert names == ["spc_wcs_pixel_map_f64", "spc_wcs_pixel_map_f64", "spc_mosaic_f32"], (order, names)
        args = calls[-1][1]
        assert len(args) == len(_lib.SIGNATURES["spc_mosaic_f32"][1]) and args[2] == 2
        assert isinstance(args[3], C.Array) and isinstance(args[3][0], _lib.SpcMosaicSource) and len(args[3]) == 2
        assert args[4:8] == (5, out.shape[1], out.shape[2], {"nearest-neighbor": 0, "bilinear": 1}.get(order, order))
        assert type(out) is SpectralCube and out.shape[0] == 5 and out.unit == a.unit and out.meta == {}
        assert np.isnan(out.fill_value) and out.wcs.header["NAXIS1"] == out.shape[2]
    for order in ("biquadratic", "bicubic", 2, 3):                                      # spline orders
        del calls[:]
        mosaic_cubes([a, b], order=order)
        assert [c[0] for c in calls] == ["reproject", "reproject"]
    del calls[:]
    a2, b2 = _two_cubes(shift=0.4)                                                       # another spectral axis
    out = mosaic_cubes([a2, b2])
    assert [c for c in calls] == [("reproject", (1, True)), ("reproject", (1, True))] and out.shape[0] == 5
    assert cube_utils.mosaic_route([a2, b2], SimpleWCS(dict(a2.header, NAXIS3=5)), 1) == "composed"
    assert cube_utils.mosaic_route([a, b], SimpleWCS(dict(a.header, NAXIS3=5)), 1) == "fused"
    del calls[:]
    out = mosaic_cubes([a], filled=False)                                                # a single cube is allowed
    assert [c[0] for c in calls] == ["spc_wcs_pixel_map_f64", "spc_mosaic_f32"] and out.shape == a.shape
    assert calls[-1][1][3][0].mask.flags == 0


def test_mixed_sample_types_take_the_composed_route(recorded, monkeypatch):
    calls = recorded
    a, b = _two_cubes()
    monkeypatch.setattr(SpectralCube, "_runs_wide", lambda self: self is b)
    mosaic_cubes([a, b])
    assert [c[0] for c in calls] == ["reproject", "reproject"]


def test_different_units_warn_and_the_first_wins(recorded):
    a, b = _two_cubes()
    b = SpectralCube(np.zeros(b.shape, np.float32), header=dict(b.header, BUNIT="Jy/beam"))
    with pytest.warns(UserWarning, match="different units"):
        out = mosaic_cubes([a, b])
    assert out.unit == "K"


def test_an_out_of_core_cube_is_refused(recorded, monkeypatch):
    from spectral_cube_amd import streaming
    a, b = _two_cubes()
    monkeypatch.setattr(SpectralCube, "_stream_source", lambda self: object() if self is b else None)
    with pytest.raises(streaming.HugeCubeError):
        mosaic_cubes([a, b])
    with pytest.raises(streaming.HugeCubeError):
        mosaic_cubes([a, b], order="bicubic")


def test_ops_mosaic_checks_its_arguments_before_any_call(recorded):
    calls = recorded
    c32, c64 = _StandInArray((4, 5, 6), np.float32), _StandInArray((4, 5, 6), np.float64)
    xy = (_StandInArray((3, 4), np.float64), _StandInArray((3, 4), np.float64))
    out = ops.mosaic([c64, c64], [xy, xy], [None, ops.MaskSpec(_lib.MASK_GT, thr_lo=0.1)], [np.nan, 0.0], 1)
    assert [c[0] for c in calls] == ["spc_mosaic_f64"] and out.dtype == np.float64 and out.shape == (4, 3, 4)
    tab = calls[0][1][3]
    assert isinstance(tab[1], _lib.SpcMosaicSource64) and tab[1].mask.thr_lo == 0.1 and tab[1].fill == 0.0 and np.isnan(tab[0].fill)
    del calls[:]
    with pytest.raises(TypeError):
        ops.mosaic([c32, c64], [xy, xy], None, [0.0, 0.0], 1)
    with pytest.raises(TypeError):
        ops.mosaic([c32, _StandInArray((3, 5, 6), np.float32)], [xy, xy], None, [0.0, 0.0], 1)
    with pytest.raises(ValueError):
        ops.mosaic([c32], [(xy[0], _StandInArray((3, 5), np.float64))], None, [0.0], 1)
    with pytest.raises(ValueError):
        ops.mosaic([c32], [xy], None, [0.0], 2)
    with pytest.raises(ValueError):
        ops.mosaic([], [], None, [], 1)
    with pytest.raises(ValueError):
        ops.mosaic([c32], [xy], None, [0.0], 1, weights=_StandInArray((3, 4), np.float32))
    assert calls == []


# ---- exports, and no CPU fallback -----------------------------------------------------------------------------------
def test_new_symbols_are_declared_exported_and_bound():
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name in ("spc_mosaic_f32", "spc_mosaic_f64", "spc_mosaic_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr) and hasattr(lib, name) and name in _lib.SIGNATURES
    assert "cube_utils.py:810-856" in hdr and lib.spc_abi_version() == 8
    assert C.sizeof(_lib.SpcMosaicSource) == 112 and C.sizeof(_lib.SpcMosaicSource64) == 120
    assert lib.spc_mosaic_workspace_bytes(1000) >= 1000 * 120                            # no built limit on the sources
    # argument checking happens before any device work
    tab = (_lib.SpcMosaicSource * 1)()
    assert lib.spc_mosaic_f32(0, None, 1, tab, 1, 1, 1, 1, None, None, None, 0) == _lib.SPC_ERR_INVALID
    assert lib.spc_mosaic_f32(0, None, 0, tab, 1, 1, 1, 1, None, None, None, 0) == _lib.SPC_ERR_INVALID


def test_no_cpu_fallback_without_a_gpu():
    if _lib.device_count() > 0:
        return
    sources, _, _ = recorded_sources("split")
    cubes = [SpectralCube.read(d, h) for d, h, _, _ in sources]
    with pytest.raises(HipLibraryError):
        mosaic_cubes(cubes, order="nearest-neighbor")
    with pytest.raises(HipLibraryError):
        mosaic_cubes(cubes, order="bicubic")
