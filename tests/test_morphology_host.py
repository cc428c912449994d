"""CPU: the host side of binary mask morphology (spectral_cube_amd/morphology.py, ops.mask_morph, spc_mask_morph_u8): the
numpy restatement of its rules (tests/morphology.py) against scipy.ndimage, argument checking, the C ABI, what reaches the
entry point.  No kernel runs here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import morphology as R
from conftest import REPO
from spectral_cube_amd import _lib, morphology, ops, SpectralCube
from spectral_cube_amd import masks as M

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 4, "CRPIX2": 3, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}


scipy_morph = R.scipy_morph
CASES = R.cases()


def test_the_table_covers_what_it_should():
    names = {c.split("-")[0] for c, _ in CASES}
    for want in ("point", "conn1", "conn2", "conn3", "box2x1x1", "box1x2x3", "box3x1x5", "box4x3x2", "box5x5x5", "box1x7x1",
                 "box7x2x3", "asym1x2x3", "asym7x2x3", "hollow5x5x5", "back2x1x1", "back4x3x2"):
        assert want in names
    assert {tuple(kw["x"].shape) for _, kw in CASES} == set(R.SHAPES)
    assert {kw["iterations"] for _, kw in CASES} == {0, 1, 2}
    assert {kw["border_value"] for _, kw in CASES} == {0, 1}
    assert any(kw["mask"] is not None for _, kw in CASES) and any(kw["mask"] is None for _, kw in CASES)
    # asymmetric: a structure that is not its own reflection; a repetition to the fixed point without the centre
    assert any(not np.array_equal(kw["structure"], kw["structure"][::-1, ::-1, ::-1]) for _, kw in CASES)
    assert any(kw["iterations"] < 1 and not kw["structure"][tuple(n // 2 for n in kw["structure"].shape)] for _, kw in CASES)


@pytest.mark.parametrize("name", sorted({c.split("-")[0] for c, _ in CASES}))
def test_restatement_equals_scipy(name):
    n = 0
    for cid, kw in CASES:
        if cid.split("-")[0] != name:
            continue
        exp = scipy_morph(**kw)
        got = R.morph(kw["x"], kw["structure"], kw["op"], kw["iterations"], kw["mask"], kw["border_value"])
        assert np.array_equal(got, exp), cid
        n += 1
    assert n >= 64


@pytest.mark.parametrize("shape", R.SHAPES)
def test_opening_closing_propagation_equal_scipy(shape):
    x, mask = R.field(shape, 3, 0.6), R.field(shape, 4, 0.7)
    for s in (None, np.ones((2, 1, 1), bool), R.generate_binary_structure(3, 2), np.ones((1, 2, 3), bool)):
        fits = all(a <= n for a, n in zip((3, 3, 3) if s is None else s.shape, shape))
        for border in (0, 1):
            for m in (None, mask):
                for it in (1, 2) if fits else (1,):
                    kw = dict(structure=s, iterations=it, mask=m, border_value=border)
                    assert np.array_equal(R.binary_opening(x, **kw), ndi.binary_opening(x, **kw)), (s, kw)
                    assert np.array_equal(R.binary_closing(x, **kw), ndi.binary_closing(x, **kw)), (s, kw)
        if fits:
            seed = x & mask & R.field(shape, 5, 0.1)
            for border in (0, 1):
                assert np.array_equal(R.binary_propagation(seed, s, mask=mask, border_value=border),
                                      ndi.binary_propagation(seed, structure=s, mask=mask, border_value=border))


def test_serpentine_is_one_long_path():
    m, seed = R.serpentine()
    x = np.zeros(m.shape, bool)
    x[seed] = True
    for c in (1, 3):
        got = R.binary_propagation(x, R.generate_binary_structure(3, c), mask=m)
        assert np.array_equal(got, ndi.binary_propagation(x, structure=ndi.generate_binary_structure(3, c), mask=m))
        assert np.array_equal(got, m) and m.sum() > 500        # the whole corridor is reached from the one seed


@pytest.mark.parametrize("rank", [2, 3])
@pytest.mark.parametrize("connectivity", [1, 2, 3])
def test_generate_binary_structure(rank, connectivity):
    exp = ndi.generate_binary_structure(rank, connectivity)
    for f in (morphology.generate_binary_structure, R.generate_binary_structure):
        got = f(rank, connectivity)
        assert got.dtype == bool and np.array_equal(got, exp)


def test_offsets_of_a_structure():
    off = morphology._offsets(None, 0)
    assert off.dtype == np.int8 and sorted(map(tuple, off)) == sorted(map(tuple, R.offsets(R.generate_binary_structure(3, 1))))
    assert morphology._offsets(np.ones((2, 1, 1), bool), 0).tolist() == [[-1, 0, 0], [0, 0, 0]]       # centre = size // 2
    assert morphology._offsets(np.ones((1, 7), bool), 0).tolist() == [[0, 0, d] for d in range(-3, 4)]  # 2-D: per plane
    assert morphology._offsets(np.ones((7, 7, 7), bool), (0, 0, 0)).shape == (343, 3)
    s = np.zeros((4, 3, 2), int)
    s[3, 0, 1] = 5
    assert morphology._offsets(s, 0).tolist() == [[1, -1, 0]]


# ---- argument errors, all without a device --------------------------------------------------------------------------
def _cube(shape=(6, 5, 4)):
    return SpectralCube.read(np.random.default_rng(3).normal(size=shape).astype(np.float32), HDR)


ALL = (morphology.binary_dilation, morphology.binary_erosion, morphology.binary_opening, morphology.binary_closing,
       morphology.binary_propagation)


@pytest.mark.parametrize("f", ALL)
def test_argument_errors(f, monkeypatch):
    x = np.ones((6, 5, 4), bool)
    with pytest.raises(NotImplementedError, match="origin"):
        f(x, origin=1)
    with pytest.raises(NotImplementedError, match="origin"):
        f(x, origin=(0, -1, 0))
    with pytest.raises(ValueError, match="1 to 7"):
        f(x, structure=np.ones((8, 1, 1), bool))
    with pytest.raises(ValueError, match="1 to 7"):
        f(x, structure=np.ones((3, 8), bool))
    for empty in (np.zeros((3, 3, 3), bool), np.zeros((0, 3, 3), bool)):
        with pytest.raises(ValueError, match="empty"):
            f(x, structure=empty)
    with pytest.raises(ValueError, match=r"reshape\(-1, 1, 1\)"):
        f(x, structure=np.ones(3, bool))
    with pytest.raises(ValueError, match="does not match"):
        f(x, mask=np.ones((6, 5, 5), bool))
    with pytest.raises(ValueError, match="does not match"):
        f(_cube(), mask=_cube((6, 5, 3)) > 0)
    with pytest.raises(ValueError, match="shape"):
        f(np.ones((5, 4), bool))
    with pytest.raises(TypeError, match="cube="):
        f(M.FunctionMask(lambda d: d > 0))
    with pytest.raises(TypeError):
        f(x, brute_force=True)
    with pytest.raises(TypeError):
        f(x, output=np.empty_like(x))
    monkeypatch.setenv("SPC_HBM_BUDGET", "64")
    with pytest.raises(NotImplementedError, match="out-of-core"):
        f(_cube())
    with pytest.raises(NotImplementedError, match="out-of-core"):
        f(x, mask=_cube() > 0)


def test_cube_conveniences_go_through_the_same_checks(monkeypatch):
    cube = _cube()
    with pytest.raises(ValueError, match="1 to 7"):
        cube.with_mask_dilated(np.ones((1, 1, 9), bool))
    with pytest.raises(ValueError, match="empty"):
        cube.with_mask_eroded(np.zeros((3, 3, 3), bool))
    monkeypatch.setenv("SPC_HBM_BUDGET", "64")
    with pytest.raises(NotImplementedError, match="out-of-core"):
        cube.with_mask_dilated()


def test_the_package_does_not_import_scipy():
    import subprocess
    import sys
    code = ("import sys; import spectral_cube_amd as s, numpy as np; "
            "assert s.generate_binary_structure(3, 2).sum() == 19; s.morphology._offsets(np.ones((2, 1, 1), bool), 0); "
            "assert s.binary_propagation is s.morphology.binary_propagation; "
            "assert not any(m == 'scipy' or m.startswith('scipy.') for m in sys.modules)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_entry_points_declared_exported_and_bound():
    import spectral_cube_amd as pkg
    lib = _lib.load()
    assert lib.spc_abi_version() == 8 == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    assert re.search(r"\bint\s+spc_mask_morph_u8\s*\(", text) and re.search(r"\bsize_t\s+spc_mask_morph_workspace_bytes\s*\(", text)
    for name in ("spc_mask_morph_u8", "spc_mask_morph_workspace_bytes"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert re.search(r"#define\s+SPC_MORPH_MAX_REACH\s+%d\b" % _lib.MORPH_MAX_REACH, text)
    assert re.search(r"#define\s+SPC_MORPH_MAX_OFFSETS\s+%d\b" % _lib.MORPH_MAX_OFFSETS, text)
    assert re.search(r"SPC_MORPH_ERODE\s*=\s*%d\b" % _lib.MORPH_ERODE, text) and re.search(r"SPC_MORPH_DILATE\s*=\s*%d\b" % _lib.MORPH_DILATE, text)
    assert "spc_mask_morph.hip" in open(os.path.join(REPO, "spectral_cube_amd", "csrc", "Makefile")).read()
    for name in ("binary_dilation", "binary_erosion", "binary_opening", "binary_closing", "binary_propagation",
                 "generate_binary_structure"):
        assert getattr(pkg, name) is getattr(morphology, name)
    assert callable(SpectralCube.with_mask_dilated) and callable(SpectralCube.with_mask_eroded)


def test_workspace_holds_three_packed_arrays():
    lib = _lib.load()
    for shape in ((9, 7, 11), (5, 6, 70), (1, 1, 1), (3, 2, 64), (1024, 1024, 1024)):
        words = shape[0] * shape[1] * ((shape[2] + 31) // 32)
        need = lib.spc_mask_morph_workspace_bytes(*shape)
        assert 3 * 4 * words <= need <= 3 * 4 * words + 2048, shape
    assert lib.spc_mask_morph_workspace_bytes(0, 4, 4) == 0
    assert lib.spc_mask_morph_workspace_bytes(1024, 1024, 1024) < (1 << 30) // 2      # 3/8 of the uint8 array


def test_invalid_arguments_are_reported_before_any_device_work():
    lib = _lib.load()
    nz, ny, nx = 3, 4, 40
    n = nz * ny * nx
    src, msk, dst = (C.c_uint8 * (2 * n))(), (C.c_uint8 * n)(), (C.c_uint8 * n)()
    wsn = lib.spc_mask_morph_workspace_bytes(nz, ny, nx)
    ws = (C.c_uint8 * wsn)()
    off = (C.c_int8 * 6)(0, 0, 0, 0, 0, 1)
    P = lambda a, at=0: C.c_void_p(C.addressof(a) + at)             # noqa: E731

    def call(shape=(nz, ny, nx), d_in=P(src), istr=(0, 0), d_mask=None, mstr=(0, 0), op=1, offs=P(off), noff=2, it=1, border=0,
             d_out=P(dst), w=P(ws), wn=wsn):
        return lib.spc_mask_morph_u8(0, None, shape[0], shape[1], shape[2], d_in, istr[0], istr[1], d_mask, mstr[0], mstr[1], op,
                                     offs, noff, it, border, d_out, w, wn, None)

    far = (C.c_int8 * 3)(0, 4, 0)
    for kw, word in ((dict(d_in=None), b"d_in is NULL"), (dict(d_out=None), b"d_out is NULL"), (dict(offs=None), b"h_offsets is NULL"),
                     (dict(shape=(nz, 0, nx)), b"positive"), (dict(shape=(nz, ny, -1)), b"positive"),
                     (dict(noff=0), b"1 to 343"), (dict(noff=344), b"1 to 343"), (dict(offs=P(far), noff=1), b"beyond"),
                     (dict(op=2), b"unknown op"), (dict(border=2), b"border_value"),
                     (dict(istr=(nx - 1, 0)), b"stride smaller than nx"), (dict(istr=(nx, nx)), b"overlapping"),
                     (dict(d_mask=P(msk), mstr=(8, 0)), b"d_mask: row / plane stride"),
                     (dict(d_out=P(src)), b"overlaps d_in"), (dict(d_out=P(src, n - 1)), b"overlaps d_in"),
                     (dict(d_in=P(src), istr=(2 * nx, 0), d_out=P(src, nx)), b"overlaps d_in"),
                     (dict(d_mask=P(msk), d_out=P(msk)), b"overlaps d_mask"),
                     (dict(w=None), b"d_workspace too small"), (dict(wn=wsn // 2), b"d_workspace too small"),
                     (dict(w=P(dst)), b"d_workspace overlaps")):
        assert call(**kw) == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (kw, lib.spc_last_error())


# ---- what ops.mask_morph hands to the entry point -------------------------------------------------------------------
class _StandInArray:
    """what ops.py reads of a DeviceArray, without a device"""

    def __init__(self, shape, dtype, device=0, ptr=None, owner=None):
        self.shape, self.dtype, self.device = tuple(int(n) for n in np.atleast_1d(shape)), np.dtype(dtype), device
        self.ptr = 0x1000 if ptr is None else ptr
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize


@pytest.fixture
def recorded_calls(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "DeviceArray", _StandInArray)
    monkeypatch.setattr(ops, "_ws_cache", {})
    return calls


def test_ops_passes_strides_and_offsets_as_specified(recorded_calls):
    shape = (6, 5, 40)
    inp = _StandInArray(shape, np.uint8, ptr=0x2000)
    inp.row_stride, inp.plane_stride, inp._is_view = 48, 48 * 9, True            # a rows() / x-window view
    mask = _StandInArray(shape, bool, ptr=0x9000)
    offs = morphology._offsets(np.ones((2, 1, 3), bool), 0)
    out = ops.mask_morph(inp, offs, _lib.MORPH_ERODE, iterations=-1, mask=mask, border_value=1)
    assert out.shape == shape and out.dtype == np.uint8
    (name, a), = recorded_calls
    assert name == "spc_mask_morph_u8" and len(a) == len(_lib.SIGNATURES[name][1]) == 20
    # device, stream, nz, ny, nx, d_in, strides, d_mask, strides, op, h_offsets, noffsets, iterations, border, d_out, ws, n, run
    assert a[:5] == (0, None, 6, 5, 40)
    assert (a[5].value, a[6], a[7]) == (0x2000, 48, 48 * 9)
    assert (a[8].value, a[9], a[10]) == (0x9000, 0, 0)                            # contiguous: 0 = the shape's own strides
    assert a[11] == _lib.MORPH_ERODE and a[13:16] == (6, -1, 1)
    got = np.ctypeslib.as_array(C.cast(a[12], C.POINTER(C.c_int8)), shape=(6, 3))
    assert got.tolist() == [[dz, 0, dx] for dz in (-1, 0) for dx in (-1, 0, 1)]
    assert a[16].value == out.ptr and a[18] >= _lib.load().spc_mask_morph_workspace_bytes(*shape)
    del recorded_calls[:]
    out2, run = ops.mask_morph(mask, [[0, 0, 0]], _lib.MORPH_DILATE, return_iterations=True)
    (name, a), = recorded_calls
    assert a[8] is None and a[9:11] == (0, 0) and a[11] == _lib.MORPH_DILATE and a[13:16] == (1, 1, 0) and run == 0


def test_ops_refuses_what_the_entry_would(recorded_calls):
    x = _StandInArray((6, 5, 40), np.uint8)
    for bad, exc in ((dict(offsets=[[0, 0, 4]]), ValueError), (dict(offsets=[[0, 0]]), ValueError), (dict(offsets=np.zeros((0, 3))), ValueError),
                     (dict(offsets=np.zeros((344, 3))), ValueError), (dict(op=2), ValueError),
                     (dict(mask=_StandInArray((6, 5, 41), np.uint8)), ValueError), (dict(mask=_StandInArray((6, 5, 40), np.float32)), ValueError),
                     (dict(out=_StandInArray((6, 5, 40), np.float32)), ValueError),
                     (dict(workspace=_StandInArray((16,), np.uint8)), ValueError)):
        kw = dict(offsets=[[0, 0, 0]], op=_lib.MORPH_DILATE)
        kw.update(bad)
        with pytest.raises(exc):
            ops.mask_morph(x, kw.pop("offsets"), kw.pop("op"), **kw)
    with pytest.raises(TypeError):
        ops.mask_morph(_StandInArray((6, 5, 40), np.float32), [[0, 0, 0]], _lib.MORPH_DILATE)
    view = _StandInArray((6, 5, 40), np.uint8)
    view._is_view = True
    with pytest.raises(ValueError, match="contiguous"):
        ops.mask_morph(x, [[0, 0, 0]], _lib.MORPH_DILATE, out=view)
    assert recorded_calls == []
