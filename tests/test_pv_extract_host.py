"""CPU: position-velocity diagrams - the numpy restatement of the kernel's rule against the scipy oracle on the case table
(pv_cases.py), Path sampling, the header, every refusal, and the ABI.  The kernel itself: test_gpu_pv_extract.py."""
import ctypes as C
import inspect
import math
import os
import re

import numpy as np
import pytest

import pv_cases as P
import spectral_cube_amd as S
from spectral_cube_amd import _lib, ops, pvextract, SimpleWCS, SpectralCube
from spectral_cube_amd.pvextract import Path, extract_pv_slice

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(got, exp):
    got, exp = np.asarray(got), np.asarray(exp)
    return got.dtype == exp.dtype and got.shape == exp.shape and bool(
        np.all((got == exp) & (np.signbit(got) == np.signbit(exp)) | (np.isnan(got) & np.isnan(exp))))


def check_against_oracle(got, count, scale, fdata, xs, ys, order, respect_nan, dtype, what):
    """*got* (the device's or the restatement's diagram) against scipy: order 0 equal, order 1 the NaN pattern equal and the
    finite values within pv_cases.bound; the count equal"""
    exp, ecount = P.oracle(fdata, xs, ys, order, respect_nan)
    got64 = np.asarray(got, np.float64)
    assert np.array_equal(np.isnan(got64), np.isnan(exp)), (what, "NaN pattern", np.argwhere(np.isnan(got64) != np.isnan(exp))[:4].tolist())
    if count is not None:
        assert np.array_equal(count, ecount), (what, "count")
    fin = ~np.isnan(exp)
    if order == 0:
        assert np.array_equal(got64[fin], exp.astype(dtype).astype(np.float64)[fin]), (what, "order 0 is a copy")
        return
    err = np.abs(got64 - exp)
    b = P.bound(scale, np.atleast_2d(xs).shape[0], dtype, exp)
    print("%s: max error %.3e, max error / bound %.3f" % (what, err[fin].max() if fin.any() else 0.0,
                                                          (err[fin] / np.maximum(b[fin], 1e-300)).max() if fin.any() else 0.0))
    assert (err[fin] <= b[fin]).all(), (what, float(err[fin].max()), np.argwhere(fin & ~(err <= b))[:4].tolist())


# ---- restatement against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("respect_nan", (True, False))
@pytest.mark.parametrize("order", (0, 1))
def test_the_restated_rule_is_scipys_on_the_case_table(order, respect_nan):
    for cid, plane, nz, npts, nlines in P.cases():
        shape = (nz,) + plane
        for masked in (False, True):
            f = P.filled(P.cube(shape, np.float64), P.include(shape) if masked else None)
            xs, ys = P.points(plane, npts, nlines)
            got, count, scale = P.restate(f, xs, ys, order, respect_nan)
            check_against_oracle(got, count, scale, f, xs, ys, order, respect_nan, np.float64, (cid, order, respect_nan, masked))


@pytest.mark.parametrize("order", (0, 1))
def test_restated_rule_on_a_path_that_leaves_and_re_enters_and_on_zero_weight_holes(order):
    f = P.cube((3, 7, 9), np.float64)
    xs, ys = P.zigzag((7, 9), 130)
    inside = (xs >= 0) & (xs <= 8) & (ys >= 0) & (ys <= 6)
    assert np.count_nonzero(np.diff(inside[0].astype(int))) >= 4, "the sweep crosses the border several times"
    got, count, scale = P.restate(f, xs, ys, order, True)
    check_against_oracle(got, count, scale, f, xs, ys, order, True, np.float64, "zigzag")
    assert np.isnan(got[:, ~inside[0]]).all()
    d, xs, ys = P.zero_weight_holes((2, 5, 6), np.float64)
    got, count, scale = P.restate(d, xs, ys, order, True)
    check_against_oracle(got, count, scale, d, xs, ys, order, True, np.float64, "holes")
    on_finite = (xs[0] % 1 == 0) & (ys[0] % 1 == 0) & ((xs[0] + ys[0]) % 2 == 0)
    assert on_finite.sum() >= 15 and np.array_equal(got[:, on_finite], d[:, ys[0][on_finite].astype(int), xs[0][on_finite].astype(int)])


def test_the_domain_is_closed_and_1e_9_beyond_it_is_outside():
    f = np.arange(2 * 3 * 4, dtype=np.float64).reshape(2, 3, 4)
    xs = np.array([[0.0, 3.0, -1e-9, 3.0 + 1e-9, 0.0, 0.0, 3.0, 1.5]])
    ys = np.array([[0.0, 2.0, 0.0, 0.0, -1e-9, 2.0 + 1e-9, 2.0 - 1e-9, np.nan]])
    for order in (0, 1):
        got, count, _ = P.restate(f, xs, ys, order, True)
        assert np.array_equal(np.isnan(got[0]), [False, False, True, True, True, True, False, True])
        assert got[1, 0] == f[1, 0, 0] and got[1, 1] == f[1, 2, 3]
        assert np.array_equal(count[0], [1, 1, 0, 0, 0, 0, 1, 0])


def test_a_whole_line_outside_does_not_count_and_all_outside_is_nan():
    f = P.cube((2, 7, 9), np.float64, nan_frac=0.0)
    xs, ys = P.points((7, 9), 65, 5)
    got, count, _ = P.restate(f, xs, ys, 1, True)
    assert count.max() <= 4                                    # (the last line of points() lies outside)
    alone, c1, _ = P.restate(f, xs[-1:], ys[-1:], 1, True)
    assert np.isnan(alone).all() and not c1.any()


# ---- Path -----------------------------------------------------------------------------------------------------------------
def test_point_counts_at_integer_and_fractional_length_over_spacing():
    p = Path([(0, 0), (3, 4), (3, 10)])                        # lengths 5 and 6
    assert p.length == 11.0
    assert len(p.sample_points(1.0)) == 12                     # L / spacing an integer: both ends are points
    assert len(p.sample_points(2.0)) == 6                      # 5.5: floor + 1
    assert len(p.sample_points(11.0)) == 2 and len(p.sample_points(11.5)) == 1
    assert len(Path([(0, 0), (0.3, 0)]).sample_points(0.1)) == 4        # 0.3 / 0.1 = 2.9999999999999996: the 1e-9 of the rule
    pts = p.sample_points(1.0)
    assert np.array_equal(pts[5], [3.0, 4.0]), "a vertex hit exactly"
    assert np.array_equal(pts[0], [0.0, 0.0]) and np.array_equal(pts[-1], [3.0, 10.0])
    assert np.allclose(pts[1], [0.6, 0.8], atol=1e-15) and np.array_equal(pts[7], [3.0, 6.0])
    assert pts.dtype == np.float64 and np.allclose(np.hypot(*np.diff(pts[:6], axis=0).T), 1.0, atol=1e-15)
    assert np.array_equal(Path([(0, 0), (4, 0)]).sample_points(1.0), np.stack([np.arange(5.0), np.zeros(5)], 1))


def test_direction_at_vertices_and_at_the_last_point_and_symmetric_offsets():
    p = Path([(0, 0), (3, 4), (3, 10)], width=4)
    xs, ys = p.sample_lines(1.0)
    assert xs.shape == ys.shape == (4, 12) and xs.flags.c_contiguous
    mid = p.sample_points(1.0)
    assert np.allclose(xs.mean(axis=0), mid[:, 0], atol=1e-14) and np.allclose(ys.mean(axis=0), mid[:, 1], atol=1e-14)
    off = ((np.arange(4) + 0.5) / 4 - 0.5) * 4
    assert np.array_equal(off, [-1.5, -0.5, 0.5, 1.5])
    for k, normal in ((0, (-0.8, 0.6)), (4, (-0.8, 0.6)), (5, (-1.0, 0.0)), (8, (-1.0, 0.0)), (11, (-1.0, 0.0))):
        # point 5 is the vertex: the FOLLOWING segment's direction (0, 1); point 11 the last: the last segment's
        assert np.allclose(xs[:, k] - mid[k, 0], off * normal[0], atol=1e-14), k
        assert np.allclose(ys[:, k] - mid[k, 1], off * normal[1], atol=1e-14), k
    assert np.allclose(xs[::-1] - mid[:, 0], -(xs - mid[:, 0]), atol=1e-14), "line l mirrors line nlines - 1 - l"
    assert Path([(0, 0), (5, 0)], width=2.2).sample_lines(1.0)[0].shape[0] == 3          # ceil(width)
    assert Path([(0, 0), (5, 0)], width=0.4).sample_lines(1.0)[0].shape[0] == 1
    assert Path([(0, 0), (5, 0)]).sample_lines(1.0)[0].shape == (1, 6)
    xs1, ys1 = Path([(0, 0), (5, 0)], width=3).sample_lines(1.0, nlines=1)
    assert np.array_equal(ys1, np.zeros((1, 6))), "one line lies on the path whatever the width"
    xs7, ys7 = Path([(0, 0), (5, 0)], width=3).sample_lines(1.0, nlines=7)
    assert ys7.shape == (7, 6) and np.allclose(ys7[:, 0], ((np.arange(7) + 0.5) / 7 - 0.5) * 3)


def test_from_world_round_trip():
    w = SimpleWCS(dict(P.HDR, NAXIS1=9, NAXIS2=7, NAXIS3=4))
    px, py = np.array([0.25, 3.0, 7.75]), np.array([5.5, 2.0, 0.125])
    lon, lat = w.celestial_pix2world(px, py)
    p = Path.from_world(lon, lat, w, width=2)
    assert np.abs(p.points - np.stack([px, py], 1)).max() <= 1e-9 and p.width == 2.0


def test_path_refusals():
    for bad in ([(1, 1)], [], [(1, 1), (1, 1)], [(0, 0), (1, 0), (1, 0), (2, 0)], [(0, 0), (np.nan, 1)], [1, 2, 3], [(0, 0, 0), (1, 1, 1)]):
        with pytest.raises(ValueError):
            Path(bad)
    with pytest.raises(ValueError, match="zero length"):
        Path([(0, 0), (2, 0), (2, 0)])
    with pytest.raises(ValueError, match="two distinct"):
        Path([(4, 4)])
    p = Path([(0, 0), (5, 0)], width=2)
    for spacing in (0, -1.0, np.nan, np.inf):
        with pytest.raises(ValueError, match="spacing"):
            p.sample_points(spacing)
    for n in (0, -2, 1.5):
        with pytest.raises(ValueError, match="nlines"):
            p.sample_lines(1.0, nlines=n)
    with pytest.raises(ValueError, match="width"):
        Path([(0, 0), (5, 0)], width=-1)


# ---- the public layer without a device ----------------------------------------------------------------------------------
def host_cube(shape=(4, 7, 9), hdr=P.HDR, cls=SpectralCube, **kw):
    return cls.read(np.zeros(shape, np.float32), dict(hdr) if hdr is not None else None, **kw)


def test_header_keywords():
    cube = host_cube()
    h = pvextract.pv_header(cube, 11, 2.5)
    assert (h["CTYPE1"], h["CRPIX1"], h["CRVAL1"], h["CUNIT1"]) == ("OFFSET", 1.0, 0.0, "deg")
    assert h["CDELT1"] == 2.5 * math.sqrt(abs(-2e-3 * 2e-3))                      # pvextractor: spacing x sqrt|det psm|
    assert (h["CTYPE2"], h["CRVAL2"], h["CDELT2"], h["CRPIX2"], h["CUNIT2"]) == ("VRAD", -16.0, 0.5, 1.0, "km/s")
    assert h["RESTFRQ"] == P.HDR["RESTFRQ"] and h["BUNIT"] == "K"
    assert (h["NAXIS"], h["NAXIS1"], h["NAXIS2"]) == (2, 11, 4)
    rot = dict(P.HDR, PC1_1=math.cos(0.5), PC1_2=-math.sin(0.5), PC2_1=math.sin(0.5), PC2_2=math.cos(0.5))
    assert pvextract.pv_header(host_cube(hdr=rot), 3, 1.0)["CDELT1"] == pytest.approx(2e-3, rel=1e-14)      # a rotation keeps the scale
    no_rest = {k: v for k, v in P.HDR.items() if k != "RESTFRQ"}
    assert "RESTFRQ" not in pvextract.pv_header(host_cube(hdr=no_rest), 3, 1.0)


def test_deliberate_limits_say_what_to_do_instead(monkeypatch):
    cube = host_cube()
    for order in (2, 3):
        with pytest.raises(NotImplementedError, match="order=1"):
            extract_pv_slice(cube, [(0, 0), (5, 5)], order=order)
        with pytest.raises(NotImplementedError, match="order=1"):
            cube.pv_slice([(0, 0), (5, 5)], order=order)
    for order in (-1, 4, 0.5, "cubic"):
        with pytest.raises(ValueError, match="order"):
            extract_pv_slice(cube, [(0, 0), (5, 5)], order=order)
    monkeypatch.setenv("SPC_HBM_BUDGET", "64")                     # bytes: the cube is an out-of-core source
    big = host_cube()
    with pytest.raises(NotImplementedError, match="cut"):
        extract_pv_slice(big, [(0, 0), (5, 5)])
    with pytest.raises(NotImplementedError, match="cut"):
        big.pv_slice(y=2)


def test_pv_slice_argument_errors_and_getitem_is_unchanged():
    cube = host_cube()
    with pytest.raises(NotImplementedError, match="pv_slice"):
        cube[:, 3]
    with pytest.raises(NotImplementedError, match="pv_slice"):
        cube[:, :, 3]
    for kw in ({}, {"y": 1, "x": 2}):
        with pytest.raises(ValueError, match="exactly one"):
            cube.pv_slice(**kw)
    for kw in ({"y": 7}, {"y": -8}, {"x": 9}, {"x": -10}):
        with pytest.raises(IndexError):
            cube.pv_slice(**kw)
    with pytest.raises(TypeError):
        cube.pv_slice(y=1.5)
    with pytest.raises(TypeError):
        cube.pv_slice(y=1, order=1)
    with pytest.raises(ValueError, match="not both"):
        cube.pv_slice([(0, 0), (1, 1)], y=1)
    with pytest.raises(ValueError):
        cube.pv_slice([(0, 0)])


# ---- the ABI --------------------------------------------------------------------------------------------------------------
def test_symbols_prototypes_and_abi_version():
    assert S.Path is Path and S.extract_pv_slice is extract_pv_slice and S.pvextract is pvextract
    assert callable(SpectralCube.pv_slice) and callable(ops.pv_extract)
    lib = _lib.load()
    assert lib.spc_abi_version() == 8 == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    assert "#define SPC_ABI_VERSION 8" in text
    for name in ("spc_pv_extract_f32", "spc_pv_extract_f64"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(re.findall(r"\bint %s\(" % name, text)) == 1
    # the comment above the prototypes cites what they replace
    head = text[:text.index("int spc_pv_extract_f32(")]
    comment = head[head.rindex("/* ----"):]
    assert "spectral_cube.py:2506-2513" in comment and "to_pvextractor" in comment
    src = open(os.path.join(REPO, "spectral_cube_amd", "csrc", "spc_pv_extract.hip")).read()
    assert "spectral_cube.py:2506-2513" in src and "to_pvextractor" in src
    sig = inspect.signature(ops.pv_extract)
    assert list(sig.parameters)[:3] == ["data", "xs", "ys"]
    assert (sig.parameters["order"].default, sig.parameters["respect_nan"].default) == (1, True)
    assert inspect.signature(extract_pv_slice).parameters["order"].default == 1


def _entry_args(npts=3, nlines=1, order=1, xs=0x1000, out=0x1000, ors=0, count=None, crs=0, wide=False):
    """arguments of spc_pv_extract_* that no check before the device switch dereferences (fake device addresses)"""
    c = _lib.SpcCube()
    c.d_data, c.nz, c.ny, c.nx, c.row_stride, c.plane_stride = 0x1000, 2, 3, 4, 4, 12
    m = _lib.SpcMask64() if wide else _lib.SpcMask()
    return (1 << 20, None, C.byref(c), C.byref(m), 0, float("nan"), npts, nlines, C.c_void_p(xs), C.c_void_p(xs), order, 1,
            C.c_void_p(out), ors, C.c_void_p(count), crs), (c, m)


@pytest.mark.parametrize("wide", (False, True))
def test_argument_errors_are_invalid_with_a_message(wide):
    name = "spc_pv_extract_f64" if wide else "spc_pv_extract_f32"
    for kw, words in (({"npts": 0}, "at least one point"), ({"npts": -3}, "at least one point"), ({"nlines": 0}, "at least one line"),
                      ({"order": 2}, "order 2"), ({"order": 3}, "order 3"), ({"order": -1}, "order -1"), ({"xs": None}, "d_xs"),
                      ({"out": None}, "d_out"), ({"ors": 2}, "out_row_stride"), ({"count": 0x1000, "crs": 2}, "count_row_stride")):
        args, keep = _entry_args(wide=wide, **kw)
        with pytest.raises(_lib.HipInvalidArgument, match=words):
            _lib.call(name, *args)
    # valid arguments pass every check and stop at the device switch (device 2^20 does not exist): nothing is launched
    args, keep = _entry_args(wide=wide, count=0x1000, ors=5, crs=3)
    with pytest.raises(_lib.HipLibraryError):
        _lib.call(name, *args)


def test_wrapper_refuses_before_any_launch():
    class Fake:
        shape, dtype, device, ptr = (2, 3, 4), np.dtype(np.float32), 0, 0x1000
    with pytest.raises(ValueError, match="order"):
        ops.pv_extract(Fake(), [0.0], [0.0], order=2)
    with pytest.raises(ValueError, match="one shape"):
        ops.pv_extract(Fake(), [0.0, 1.0], [0.0])
    with pytest.raises(ValueError, match="one shape"):
        ops.pv_extract(Fake(), np.zeros((1, 2, 2)), np.zeros((1, 2, 2)))
    with pytest.raises(ValueError, match="at least one point"):
        ops.pv_extract(Fake(), [], [])
