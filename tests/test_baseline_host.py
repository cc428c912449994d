"""CPU: polynomial baselines - the numpy restatement of the kernels' rule against the np.linalg.lstsq oracle on the case
table (baseline_cases.py), the conditioning cap, polynomial() against np.polyfit, channel / exclude resolution, every
refusal, and the ABI.  The kernels themselves: test_gpu_baseline.py."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import baseline_cases as B
import spectral_cube_amd as S
from spectral_cube_amd import _lib, baseline, ops, SpectralCube

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 1, "CRPIX2": 1, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}


def check_model(got_model, got_npts, case, o, order, what, dtype=np.float64):
    """*got_model* (model values at all channels, the restatement's or the device's) against the oracle: npts equal, the NaN
    pattern equal, every value finite where fitted, and within ``bound`` on the spaxels the toleranced comparison covers"""
    assert np.array_equal(got_npts, o["npts"]), (what, "npts")
    fitted = o["npts"] >= order + 1
    got = np.asarray(got_model, np.float64)
    assert np.array_equal(np.isnan(got).all(axis=0), ~fitted), (what, "NaN pattern")
    assert np.isfinite(got[:, fitted]).all(), (what, "finite")
    tol = B.toleranced(o, order)
    if not tol.any():
        return 0.0
    b = B.bound(o["npts"], order, o["kappa"], o["scale"], expected=o["model"], dtype=dtype)
    err = np.abs(got - o["model"])
    worst = float((err[:, tol] / b[:, tol]).max())
    assert (err[:, tol] <= b[:, tol]).all(), (what, "error / bound", worst)
    return worst


# ---- restatement against the oracle ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("plane", B.PLANES, ids=lambda p: "%dx%d" % p)
def test_restatement_against_lstsq_on_the_case_table(plane):
    worst = 0.0
    for pl, nz, order, dt, mask, lst in B.case_ids():
        if pl != plane or dt != "float64":
            continue                       # (the float32 cases differ in the samples only: the GPU test runs both)
        c = B.make_case(pl, nz, order, dt, mask, lst)
        o = B.case_oracle(pl, nz, order, dt, mask, lst)
        coef, npts = B.restate_fit(c["data"], c["include"], c["chan"], order)
        model = B.restate_apply(np.zeros(c["data"].shape), coef, subtract=False)
        worst = max(worst, check_model(model, npts, c, o, order, (pl, nz, order, dt, mask, lst)))
    print("plane %s: largest error / bound %.3g" % (plane, worst))


def test_at_most_two_percent_of_the_fitted_spaxels_are_beyond_the_conditioning_cap():
    seen = 0
    for key in B.case_ids():
        if key[3] != "float64":
            continue
        order = key[2]
        o = B.case_oracle(*key)
        fitted = o["npts"] >= order + 1
        beyond = fitted & ~B.toleranced(o, order)
        assert beyond.sum() <= 0.02 * fitted.sum(), (key, int(beyond.sum()), int(fitted.sum()), float(np.nanmax(o["kappa"])))
        seen += 1
    assert seen > 300


def test_special_spaxels_have_n_0_p_and_p_plus_1():
    for key in (((7, 9), 37, 3, "float64", "bytes", "all"), ((1, 5), 7, 2, "float32", "none", "all"), ((3, 130), 64, 5, "float32", "gt", "ends")):
        order = key[2]
        o = B.case_oracle(*key)
        n = o["npts"].ravel()
        assert (n[0], n[1], n[2]) == (0, order, order + 1)
        m = o["model"].reshape(key[1], -1)
        assert np.isnan(m[:, 0]).all() and np.isnan(m[:, 1]).all() and np.isfinite(m[:, 2]).all()


def test_segmented_restatement_matches_the_plain_one_within_the_bound():
    rng = np.random.default_rng(3)
    nz, order = 200, 3
    data = 5.0 + rng.standard_normal((nz, 2, 3))
    chan = np.arange(nz)
    c1, n1 = B.restate_fit(data, None, chan, order, nseg=1)
    c3, n3 = B.restate_fit(data, None, chan, order, nseg=3)
    assert B.segment_slices(nz, 3) == [(0, 67), (67, 134), (134, 200)]
    assert np.array_equal(n1, n3) and not B.same_bits(c1, c3)       # another order of the same sums
    o = B.oracle(data, None, chan, order)
    for coef in (c1, c3):
        model = B.restate_apply(np.zeros_like(data), coef, subtract=False)
        assert (np.abs(model - o["model"]) <= B.bound(o["npts"], order, o["kappa"], o["scale"])).all()


def test_power_basis_is_what_the_issue_says_it_is():
    """the reason for Legendre: the Gram matrix of 1, k ... k^5 at nz = 257 is beyond float64, Legendre's is about 11"""
    k = np.arange(257.0)
    V = np.vander(k, 6, increasing=True)
    assert np.linalg.cond(V.T @ V) > 1e20
    L = B.basis(257, 5)
    assert np.linalg.cond(L.T @ L) < 12


# ---- the public layer without a device ------------------------------------------------------------------------------------
class _Fit(baseline.BaselineFit):
    """a BaselineFit whose coefficients are a host array"""

    def legendre(self):
        return self.coefficients


def test_polynomial_against_polyfit():
    rng = np.random.default_rng(11)
    nz, order = 23, 3
    cube = SpectralCube.read(np.zeros((nz, 2, 3), np.float32), dict(HDR))
    k = np.arange(nz, dtype=np.float64)
    data = (2.0 - 0.3 * k + 0.02 * k ** 2 - 4e-4 * k ** 3)[:, None, None] * rng.uniform(0.5, 2.0, (1, 2, 3))
    coef, npts = B.restate_fit(data, None, np.arange(nz), order)
    fit = _Fit(cube, order, coef, None, np.arange(nz))
    poly = fit.polynomial()
    assert poly.shape == (order + 1, 2, 3)
    for y in range(2):
        for x in range(3):
            exp = np.polyfit(k, data[:, y, x], order)[::-1]
            assert np.allclose(poly[:, y, x], exp, rtol=1e-8, atol=1e-12), (poly[:, y, x], exp)
    # the band centre is t = 0, channel (nz - 1) / 2
    cen = fit.continuum()
    exp = sum(poly[j] * ((nz - 1) / 2.0) ** j for j in range(order + 1))
    assert np.allclose(np.asarray(cen), exp, rtol=1e-12) and cen.unit == "K"
    assert np.allclose(np.asarray(fit.continuum(4)), sum(poly[j] * 4.0 ** j for j in range(order + 1)), rtol=1e-10)
    one = _Fit(SpectralCube.read(np.zeros((1, 1, 1), np.float32), dict(HDR)), 0, np.full((1, 1, 1), 3.5), None, np.arange(1))
    assert one.polynomial().tolist() == [[[3.5]]] and np.asarray(one.continuum(0)).item() == 3.5


@pytest.mark.parametrize("cdelt", (0.5, -0.5))
def test_channels_and_exclude_resolution(cdelt):
    nz = 20
    cube = SpectralCube.read(np.zeros((nz, 2, 2), np.float32), dict(HDR, CDELT3=cdelt))
    axis = np.asarray(cube.spectral_axis, np.float64)
    assert (np.diff(axis) > 0).all() == (cdelt > 0)
    r = baseline.resolve_channels
    assert r(cube).tolist() == list(range(nz)) and r(cube).dtype == np.int32
    assert r(cube, channels=[3, 1, -1, 3]).tolist() == [1, 3, 19]
    sel = np.zeros(nz, bool)
    sel[[2, 5, 7]] = True
    assert r(cube, channels=sel).tolist() == [2, 5, 7]
    # a range in the spectral unit: the closest channel to each end, both included, whichever way the axis runs
    lo, hi = sorted((axis[4], axis[9]))
    gone = set(range(4, 10))
    assert r(cube, exclude=[(lo, hi)]).tolist() == [k for k in range(nz) if k not in gone]
    assert r(cube, exclude=[(lo + 0.1, hi - 0.1)]).tolist() == [k for k in range(nz) if k not in gone]      # rounds to the closest
    assert r(cube, channels=[3, 4, 5, 12], exclude=[(lo, hi)]).tolist() == [3, 12]                          # they combine
    lo2, hi2 = sorted((axis[15], axis[16]))
    assert r(cube, exclude=[(lo, hi), (lo2, hi2)]).tolist() == [k for k in range(nz) if k not in gone | {15, 16}]
    same = cube.spectral_slab(lo, hi)
    assert same.shape[0] == len(gone)                                                                       # spectral_slab's rule
    for bad in ([nz], [-nz - 1], [1.5], np.zeros(nz + 1, bool), [[1, 2]]):
        with pytest.raises(ValueError):
            r(cube, channels=bad)
    with pytest.raises(ValueError, match="lo must not be above hi"):
        r(cube, exclude=[(hi, lo)])
    with pytest.raises(ValueError, match="list of"):
        r(cube, exclude=(lo, hi))


def test_refusals_come_before_any_device_call(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "call", lambda *a, **k: called.append(a))
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: called.append("require_gpu"))
    cube = SpectralCube.read(np.zeros((8, 3, 4), np.float32), dict(HDR))
    axis = np.asarray(cube.spectral_axis, np.float64)
    for order in (-1, 6, 1.0, 2.5, "1", None, True):
        with pytest.raises(ValueError, match="order"):
            cube.fit_baseline(order=order)
        with pytest.raises(ValueError, match="order"):
            S.subtract_baseline(cube, order=order)
    with pytest.raises(ValueError, match="at least 4 channels and 3 are left"):
        cube.fit_baseline(order=3, channels=[0, 1, 2])
    with pytest.raises(ValueError, match="at least 2 channels and 1 are left"):
        cube.fit_baseline(order=1, exclude=[(axis[1], axis[7])])
    with pytest.raises(ValueError, match="out of range"):
        cube.fit_baseline(order=1, channels=[0, 8])
    with pytest.raises(ValueError, match="lo must not be above hi"):
        cube.subtract_baseline(order=1, exclude=[(axis[5], axis[2])])
    monkeypatch.setenv("SPC_HBM_BUDGET", "64")
    with pytest.raises(NotImplementedError, match="out-of-core"):
        cube.fit_baseline(order=1)
    with pytest.raises(NotImplementedError, match="out-of-core"):
        cube.subtract_baseline(order=0)
    assert not called


def test_wrappers_refuse_before_any_launch(monkeypatch):
    called = []
    monkeypatch.setattr(_lib, "call", lambda *a, **k: called.append(a))

    class Fake:
        shape, dtype, device, ptr, nbytes = (4, 3, 5), np.dtype(np.float32), 0, 0x1000, 240

    class Coef:
        shape, dtype, device, ptr = (7, 3, 5), np.dtype(np.float64), 0, 0x2000

    for order in (-1, 6, 1.5, True):
        with pytest.raises(ValueError, match="order"):
            ops.baseline_fit(Fake(), order)
    with pytest.raises(ValueError, match="out of range"):
        ops.baseline_fit(Fake(), 1, channels=[0, 4])
    with pytest.raises(ValueError, match="empty"):
        ops.baseline_fit(Fake(), 0, channels=np.zeros(4, bool))
    with pytest.raises(ValueError, match="order"):
        ops.baseline_apply(Fake(), Coef())
    Coef.shape = (2, 3, 4)
    with pytest.raises(ValueError, match="coef must be"):
        ops.baseline_apply(Fake(), Coef())
    assert not called
    sig = inspect.signature(ops.baseline_fit)
    assert list(sig.parameters)[:7] == ["data", "order", "channels", "mask_spec", "coef", "npts", "stream"]
    assert list(inspect.signature(ops.baseline_apply).parameters) == ["data", "coef", "subtract", "out", "stream"]
    for f in (ops.baseline_fit, ops.baseline_apply):
        assert not {"cube", "mask"} & set(inspect.signature(f).parameters)


# ---- the ABI --------------------------------------------------------------------------------------------------------------
NAMES = ("spc_baseline_fit_f32", "spc_baseline_fit_f64", "spc_baseline_apply_f32", "spc_baseline_apply_f64")


def test_symbols_prototypes_and_abi_version():
    assert S.fit_baseline is baseline.fit_baseline and S.subtract_baseline is baseline.subtract_baseline
    assert S.BaselineFit is baseline.BaselineFit and S.baseline is baseline
    assert callable(SpectralCube.fit_baseline) and callable(SpectralCube.subtract_baseline)
    lib = _lib.load()
    assert lib.spc_abi_version() == 8 == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    assert "#define SPC_ABI_VERSION 8" in text and "#define SPC_BASELINE_MAX_ORDER 5" in text
    assert _lib.BASELINE_MAX_ORDER == 5 == baseline.MAX_ORDER == B.MAX_ORDER
    for name in NAMES:
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert len(re.findall(r"\bint %s\(" % name, text)) == 1
    for name in ("spc_baseline_segments", "spc_baseline_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES and name + "(" in text
    head = text[:text.index("int spc_baseline_fit_f32(")]
    comment = head[head.rindex("/* ----"):]
    for words in ("t_k = (2k - (nz - 1)) / (nz - 1)", "Legendre", "legvander", "L D L^T", "No atomics", "mode 0", "mode 1"):
        assert words in comment, words
    mk = open(os.path.join(REPO, "spectral_cube_amd", "csrc", "Makefile")).read()
    assert "spc_baseline.hip" in mk and "EXTRA_spc_baseline := -ffp-contract=off" in mk
    assert len(_lib.SIGNATURES["spc_baseline_fit_f32"][1]) == 12 and len(_lib.SIGNATURES["spc_baseline_apply_f64"][1]) == 10


def test_segment_rule_and_workspace_size():
    seg = ops.baseline_segments
    # a plane that fills the device, or a short list, is not split
    assert seg((4096, 256, 256), 4096) == 1 and seg((127, 7, 9), 127) == 1 and seg((4096, 7, 9), 100) == 1
    assert seg((128, 7, 9), 128) == 2 and seg((200, 7, 9), 200) == 3
    assert seg((4096, 64, 64), 4096) == 32                    # the single-dish map: 64 waves become 2048
    assert seg((70001, 1, 3), 70001) == 64
    lib = _lib.load()
    assert lib.spc_baseline_workspace_bytes(127, 7, 9, 127, 5) == 0
    for order in range(6):
        nacc = (order + 1) * (order + 2) // 2 + order + 1
        need = lib.spc_baseline_workspace_bytes(200, 7, 9, 200, order)
        assert 3 * 63 * (8 * nacc + 4) <= need <= 3 * 63 * (8 * nacc + 4) + 512
    # the rule restated: the segments are ceil(nfit / s) long and none is empty
    for nfit in (128, 129, 191, 192, 200, 1000, 4096, 70001):
        s = seg((nfit, 1, 3), nfit)
        sl = B.segment_slices(nfit, s)
        assert len(sl) == s and sl[-1][1] == nfit and all(b > a for a, b in sl)


def _entry_args(fit, wide, order=1, nfit=6, chan=None, basis=0x9000, coef=0x20000, npts=0x30000, data=0x1000, strides=(5, 20),
                marr=None, mstrides=(0, 0), ws=None, wsn=0, mode=0, out=0x40000, ostrides=(0, 0), shape=(6, 4, 5)):
    """arguments of the baseline entries that no check before the device switch dereferences (fake device addresses)"""
    c = _lib.SpcCube()
    c.d_data = data
    c.nz, c.ny, c.nx = shape
    c.row_stride, c.plane_stride = strides
    m = _lib.SpcMask64() if wide else _lib.SpcMask()
    if marr is not None:
        m.flags, m.d_array = _lib.MASK_ARRAY, marr
        m.row_stride, m.plane_stride = mstrides
    if fit:
        return (1 << 20, None, C.byref(c), C.byref(m), order, C.c_void_p(chan), nfit, C.c_void_p(basis), C.c_void_p(coef),
                C.c_void_p(npts), C.c_void_p(ws), wsn), (c, m)
    return (1 << 20, None, C.byref(c), order, C.c_void_p(basis), C.c_void_p(coef), mode, C.c_void_p(out), ostrides[0],
            ostrides[1]), (c, m)


@pytest.mark.parametrize("wide", (False, True))
def test_argument_errors_are_invalid_with_a_message(wide):
    it = 8 if wide else 4
    fit = "spc_baseline_fit_f64" if wide else "spc_baseline_fit_f32"
    for kw, words in (({"order": -1}, "order -1"), ({"order": 6}, "order 6"), ({"basis": None}, "d_basis"), ({"coef": None}, "d_coef"),
                      ({"data": None}, "cube pointer"), ({"nfit": 0}, "nfit"), ({"nfit": 5}, "must be nz"), ({"strides": (4, 20)}, "row_stride"),
                      ({"strides": (5, 19)}, "plane_stride"), ({"marr": 0x50000, "mstrides": (4, 20)}, "mask row_stride"),
                      ({"marr": 0x50000, "mstrides": (5, 19)}, "mask plane_stride"),
                      ({"coef": 0x1000 + 10 * it}, "d_coef overlaps the cube"), ({"npts": 0x9000 + 8}, "d_npts overlaps d_basis"),
                      ({"npts": 0x20000 + 16}, "d_coef overlaps d_npts"), ({"marr": 0x20000 + 1}, "d_coef overlaps the mask array"),
                      ({"chan": 0x30000 + 4, "nfit": 3}, "d_npts overlaps d_channels")):
        args, keep = _entry_args(True, wide, **kw)
        with pytest.raises(_lib.HipInvalidArgument, match=words):
            _lib.call(fit, *args)
    # the segmented path: a workspace that is short, NULL, or on an output
    shape, need = (200, 2, 3), _lib.load().spc_baseline_workspace_bytes(200, 2, 3, 200, 1)
    assert need > 0
    seg = dict(shape=shape, strides=(3, 6), nfit=200, data=0x100000, coef=0x20000, npts=0x30000)
    for kw, words in (({"ws": 0x800000, "wsn": need - 1}, "d_workspace too small"), ({"ws": None, "wsn": need}, "d_workspace too small"),
                      ({"ws": 0x20000, "wsn": need}, "d_coef overlaps d_workspace")):
        args, keep = _entry_args(True, wide, **dict(seg, **kw))
        with pytest.raises(_lib.HipInvalidArgument, match=words):
            _lib.call(fit, *args)
    # valid arguments pass every check and stop at the device switch (device 2^20 does not exist): nothing is launched
    for kw in ({}, {"marr": 0x50000}, {"marr": 0x50000, "mstrides": (7, 30)}, {"chan": 0x60000, "nfit": 2}, {"npts": None}, {"order": 5},
               dict(seg, ws=0x800000, wsn=need)):
        args, keep = _entry_args(True, wide, **kw)
        with pytest.raises(_lib.HipLibraryError) as e:
            _lib.call(fit, *args)
        assert not isinstance(e.value, _lib.HipInvalidArgument), (kw, str(e.value))
    apply_ = "spc_baseline_apply_f64" if wide else "spc_baseline_apply_f32"
    for kw, words in (({"order": 6}, "order 6"), ({"basis": None}, "d_basis"), ({"coef": None}, "d_coef"), ({"out": None}, "d_out"),
                      ({"mode": 2}, "mode 2"), ({"ostrides": (4, 0)}, "out_row_stride"), ({"ostrides": (5, 19)}, "out_plane_stride"),
                      ({"out": 0x1000}, "d_out overlaps the cube"), ({"out": 0x1000 + 100 * it}, "d_out overlaps the cube"),
                      ({"out": 0x20000 - 8}, "d_out overlaps d_coef"), ({"out": 0x9000}, "d_out overlaps d_basis")):
        args, keep = _entry_args(False, wide, **kw)
        with pytest.raises(_lib.HipInvalidArgument, match=words):
            _lib.call(apply_, *args)
    for kw in ({}, {"mode": 1}, {"ostrides": (7, 30)}, {"order": 0}):
        args, keep = _entry_args(False, wide, **kw)
        with pytest.raises(_lib.HipLibraryError) as e:
            _lib.call(apply_, *args)
        assert not isinstance(e.value, _lib.HipInvalidArgument), (kw, str(e.value))
