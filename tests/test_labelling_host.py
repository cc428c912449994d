"""CPU: the host side of connected-component labelling (spectral_cube_amd/labelling.py, ops.label / label_objects /
label_select, spc_label_u8 / spc_label_objects_i32 / spc_label_select_i32): structure parsing, argument checking, the C
ABI, the keep table against scipy.  No kernel runs here."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import labelling as R
from conftest import REPO
from spectral_cube_amd import _lib, labelling, ops, SpectralCube
from spectral_cube_amd import masks as M

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 4, "CRPIX2": 3, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}


def _cube(shape=(6, 5, 4)):
    return SpectralCube.read(np.random.default_rng(3).normal(size=shape).astype(np.float32), HDR)


# ---- structures ---------------------------------------------------------------------------------------------------------
def test_structure_becomes_thirteen_pair_bits():
    assert labelling.pair_bits(None) == labelling.pair_bits(ndi.generate_binary_structure(3, 1)) == (1 << 4) | (1 << 10) | (1 << 12)
    assert labelling.pair_bits(ndi.generate_binary_structure(3, 3)) == (1 << 13) - 1
    assert labelling.pair_bits(np.zeros((3, 3, 3), bool)) == 0
    for name, s in R.structures():
        full = R.full_structure(s)
        bits = labelling.pair_bits(s)
        assert bits == sum(1 << t for t in range(13) if full.ravel()[t]), name
        flipped = full.copy()
        flipped[1, 1, 1] ^= True                                        # the centre is not part of the connectivity
        assert labelling.pair_bits(flipped) == bits
        assert np.array_equal(ops.label_structure(full), full.ravel().astype(np.uint8))
    # a (3, 3) structure is the middle plane: no bit of another plane (t < 9), the in-plane bits as they are
    assert labelling.pair_bits(np.ones((3, 3), bool)) == 0b1111 << 9
    assert np.array_equal(labelling._structure([[0, 1, 0], [1, 1, 1], [0, 1, 0]])[1], ndi.generate_binary_structure(2, 1))
    assert not labelling._structure(np.ones((3, 3)))[[0, 2]].any()
    assert labelling._structure(np.full((3, 3, 3), 7)).all()            # any non-zero entry is True


def test_structures_that_are_refused():
    x = np.ones((4, 4, 4), bool)
    asym = ndi.generate_binary_structure(3, 1).copy()
    asym[0, 1, 1] = False
    for f in (lambda s: labelling.label(x, structure=s), lambda s: labelling.remove_small_objects(x, structure=s),
              lambda s: _cube().with_mask_pruned(structure=s)):
        with pytest.raises(ValueError, match="centrosymmetric"):
            f(asym)
        with pytest.raises(ValueError, match="centrosymmetric"):
            f(np.array([[0, 1, 0], [0, 1, 1], [0, 0, 0]]))
        for bad in (np.ones(3, bool), np.ones((1, 1, 3), bool), np.ones((5, 5, 5), bool), np.ones((3, 5), bool), np.ones((3, 3, 3, 3), bool)):
            with pytest.raises(ValueError, match=r"\(3, 3, 3\)"):
                f(bad)
    with pytest.raises(ValueError, match="centrosymmetric"):
        ops.label_structure(asym)
    with pytest.raises(ValueError, match=r"\(3, 3, 3\)"):
        ops.label_structure(np.ones((3, 3), bool))
    with pytest.raises(AssertionError, match="not symmetric"):           # what scipy does with the same structure
        ndi.label(x, structure=asym)


def test_other_argument_errors(monkeypatch):
    with pytest.raises(ValueError, match="shape"):
        labelling.label(np.ones((5, 4), bool))
    with pytest.raises(TypeError, match="cube="):
        labelling.label(M.FunctionMask(lambda d: d > 0))
    monkeypatch.setenv("SPC_HBM_BUDGET", "64")
    for f in (lambda: labelling.label(_cube()), lambda: labelling.remove_small_objects(_cube() > 0), lambda: _cube().with_mask_pruned()):
        with pytest.raises(NotImplementedError, match="out-of-core"):
            f()


def test_the_package_does_not_import_scipy():
    import subprocess
    import sys
    code = ("import sys; import spectral_cube_amd as s, numpy as np; "
            "assert s.labelling.pair_bits(None) == 5136; s.labelling.keep_table(np.ones(3, np.int64), np.zeros((3, 6), np.int32)); "
            "assert s.label is s.labelling.label and s.remove_small_objects is s.labelling.remove_small_objects; "
            "assert not any(m == 'scipy' or m.startswith('scipy.') for m in sys.modules)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=REPO)


# ---- the keep table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(9, 8, 70), (6, 40, 40)])
def test_keep_table_equals_the_scipy_pipeline(shape):
    for seed, (p, conn) in enumerate(((0.31, 1), (0.2, 3), (0.5, 1))):
        x = R.field(shape, seed, p)
        s = ndi.generate_binary_structure(3, conn)
        lab, n = R.scipy_label(x, s)
        sizes, objs = R.scipy_objects(lab, n)
        bbox = np.array([[0] * 6] + [[v for sl in o for v in (sl.start, sl.stop)] for o in objs], np.int32)
        for min_size, min_channels in ((1, 1), (4, 1), (4, 2), (2, 3), (10 ** 9, 1)):
            mask, keep = R.scipy_remove_small(x, min_size, s, min_channels)
            got = labelling.keep_table(sizes, bbox, min_size, min_channels)
            assert got.dtype == bool and np.array_equal(got, keep) and not got[0], (p, conn, min_size, min_channels)
            assert np.array_equal(got[lab], mask)
        assert labelling.keep_table(sizes, bbox, 1, 1)[1:].all() and not labelling.keep_table(sizes, bbox, 10 ** 9)[1:].any()
        some = labelling.keep_table(sizes, bbox, 4, 2)
        assert some[1:].any() and not some[1:].all()
    with pytest.raises(ValueError, match="one entry per label"):
        labelling.keep_table(np.ones(3), np.zeros((4, 6)))
    assert labelling.keep_table(np.array([5]), np.zeros((1, 6), np.int32)).tolist() == [False]          # no label at all


# ---- the C ABI ----------------------------------------------------------------------------------------------------------
NAMES = ("spc_label_u8", "spc_label_objects_i32", "spc_label_select_i32", "spc_label_workspace_bytes")


def test_entry_points_declared_exported_and_bound():
    import spectral_cube_amd as pkg
    lib = _lib.load()
    assert lib.spc_abi_version() == 8 == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name in NAMES:
        kind = "size_t" if name.endswith("_bytes") else "int"
        assert re.search(r"\b%s\s+%s\s*\(" % (kind, name), text), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert re.search(r"#define\s+SPC_LABEL_OBJECTS_WORKSPACE_BYTES\s+%d\b" % _lib.LABEL_OBJECTS_WORKSPACE_BYTES, text)
    assert "2^31 - 1" in text and _lib.LABEL_MAX_VOXELS == 2 ** 31 - 1
    assert "spc_label.hip" in open(os.path.join(REPO, "spectral_cube_amd", "csrc", "Makefile")).read()
    for name in ("label", "remove_small_objects", "LabelMap"):
        assert getattr(pkg, name) is getattr(labelling, name)
    assert callable(SpectralCube.with_mask_pruned)
    assert callable(ops.label) and callable(ops.label_objects) and callable(ops.label_select)


def test_workspace_query():
    q = _lib.load().spc_label_workspace_bytes
    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (0, 0, 0)):
        assert q(*shape) == 0
    last = 0
    for n in (1, 2, 7, 64, 255, 256, 257, 1000, 1024, 4096, 70000):
        need = q(n, n, n)
        assert need >= max(last, _lib.LABEL_OBJECTS_WORKSPACE_BYTES), n          # monotone, and enough for label_objects too
        last = need
    for a, b in (((3, 4, 40), (3, 4, 41)), ((3, 4, 40), (3, 5, 40)), ((3, 4, 40), (4, 4, 40)), ((1, 1, 70000), (2, 1, 70000))):
        assert q(*a) <= q(*b)
    assert q(1024, 1024, 1024) <= 1 << 20                                # counts per chunk, nothing per voxel
    assert q(2 ** 40, 2 ** 40, 2 ** 40) >= q(1024, 1024, 1024)           # no overflow in the product


def _buffers(nz=3, ny=4, nx=40):
    lib = _lib.load()
    n = nz * ny * nx
    wsn = lib.spc_label_workspace_bytes(nz, ny, nx)
    return dict(n=n, src=(C.c_uint8 * (2 * n))(), lab=(C.c_int32 * (2 * n))(), ws=(C.c_uint8 * wsn)(), wsn=wsn,
                out=(C.c_uint8 * n)(), st=(C.c_uint8 * 27)(*ndi.generate_binary_structure(3, 1).ravel().astype(int)),
                sizes=(C.c_int64 * 8)(), bbox=(C.c_int32 * 48)(), keep=(C.c_uint8 * 1024)(), count=C.c_int64(-5))


def P(a, at=0):
    return C.c_void_p(C.addressof(a) + at)


def test_invalid_arguments_are_reported_before_any_device_work():
    lib = _lib.load()
    nz, ny, nx = 3, 4, 40
    B = _buffers(nz, ny, nx)
    n = B["n"]

    def lab(shape=(nz, ny, nx), d_in=P(B["src"]), istr=(0, 0), st=P(B["st"]), d_lab=P(B["lab"]), w=P(B["ws"]), wn=B["wsn"],
            count=C.byref(B["count"])):
        return lib.spc_label_u8(0, None, shape[0], shape[1], shape[2], d_in, istr[0], istr[1], st, d_lab, w, wn, count)

    asym = (C.c_uint8 * 27)(*([1] + [0] * 26))
    for kw, word in ((dict(d_in=None), b"d_in is NULL"), (dict(d_lab=None), b"d_labels is NULL"), (dict(st=None), b"h_structure is NULL"),
                     (dict(count=None), b"h_nlabels is NULL"), (dict(shape=(nz, 0, nx)), b"positive"), (dict(shape=(nz, ny, -1)), b"positive"),
                     (dict(istr=(nx - 1, 0)), b"stride smaller than nx"), (dict(istr=(nx, nx)), b"overlapping rows"),
                     (dict(st=P(asym)), b"centrosymmetric"),
                     (dict(d_lab=P(B["src"])), b"overlaps d_in"), (dict(d_in=P(B["lab"], 4 * n - 1)), b"overlaps d_in"),
                     (dict(w=None), b"d_workspace too small"), (dict(wn=B["wsn"] // 2), b"d_workspace too small"), (dict(wn=0), b"too small"),
                     (dict(w=P(B["lab"], 16)), b"d_workspace overlaps")):
        assert lab(**kw) == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (kw, lib.spc_last_error())
    assert B["count"].value == -5

    def obj(shape=(nz, ny, nx), d_lab=P(B["lab"]), nl=7, sizes=P(B["sizes"]), bbox=P(B["bbox"]), w=P(B["ws"]), wn=B["wsn"]):
        return lib.spc_label_objects_i32(0, None, shape[0], shape[1], shape[2], d_lab, nl, sizes, bbox, w, wn)

    for kw, word in ((dict(d_lab=None), b"d_labels is NULL"), (dict(sizes=None), b"d_sizes is NULL"), (dict(bbox=None), b"d_bbox is NULL"),
                     (dict(shape=(0, ny, nx)), b"positive"), (dict(nl=-1), b"nlabels"), (dict(nl=2 ** 31), b"nlabels"),
                     (dict(sizes=P(B["lab"])), b"overlap"), (dict(bbox=P(B["sizes"], 8)), b"overlap"),
                     (dict(w=None), b"d_workspace too small"), (dict(wn=3), b"d_workspace too small"), (dict(w=P(B["bbox"])), b"d_workspace overlaps")):
        assert obj(**kw) == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (kw, lib.spc_last_error())

    def sel(shape=(nz, ny, nx), d_lab=P(B["lab"]), nl=7, keep=P(B["keep"]), out=P(B["out"])):
        return lib.spc_label_select_i32(0, None, shape[0], shape[1], shape[2], d_lab, nl, keep, out)

    for kw, word in ((dict(d_lab=None), b"d_labels is NULL"), (dict(keep=None), b"d_keep is NULL"), (dict(out=None), b"d_out is NULL"),
                     (dict(shape=(nz, ny, 0)), b"positive"), (dict(nl=-1), b"nlabels"),
                     (dict(out=P(B["lab"], 5)), b"overlaps d_labels"), (dict(out=P(B["keep"])), b"overlaps d_keep")):
        assert sel(**kw) == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (kw, lib.spc_last_error())


def test_more_than_int32_voxels_is_refused_by_shape_alone():
    lib = _lib.load()
    B = _buffers()                                                       # nothing of the large shapes is allocated: the refusal
    for shape in ((2048, 1024, 1024), (4096, 2048, 2048), (1, 1, 2 ** 31), (2 ** 31, 2 ** 31, 2 ** 31), (2 ** 62, 2, 2)):      # comes first
        assert lib.spc_label_u8(0, None, *shape, P(B["src"]), 0, 0, P(B["st"]), P(B["lab"]), P(B["ws"]), B["wsn"],
                                C.byref(B["count"])) == _lib.SPC_ERR_UNSUPPORTED
        assert b"2^31 - 1" in lib.spc_last_error()
        assert lib.spc_label_objects_i32(0, None, *shape, P(B["lab"]), 7, P(B["sizes"]), P(B["bbox"]), P(B["ws"]), B["wsn"]) == _lib.SPC_ERR_UNSUPPORTED
        assert lib.spc_label_select_i32(0, None, *shape, P(B["lab"]), 7, P(B["keep"]), P(B["out"])) == _lib.SPC_ERR_UNSUPPORTED
    # 2^31 - 1 voxels pass the limit (and fail the next check: the workspace is that of a small shape)
    assert lib.spc_label_u8(0, None, 1, 1, 2 ** 31 - 1, P(B["src"]), 0, 0, P(B["st"]), P(B["lab"]), P(B["ws"]), B["wsn"],
                            C.byref(B["count"])) == _lib.SPC_ERR_INVALID
    assert b"2^31" not in lib.spc_last_error()


# ---- what ops hands to the entry points -------------------------------------------------------------------------------
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


def test_ops_passes_strides_structure_and_tables_as_specified(recorded_calls):
    shape = (6, 5, 40)
    inp = _StandInArray(shape, np.uint8, ptr=0x2000)
    inp.row_stride, inp.plane_stride, inp._is_view = 48, 48 * 9, True            # a rows() / x-window view
    s = ndi.generate_binary_structure(3, 2)
    out, n = ops.label(inp, s)
    assert out.shape == shape and out.dtype == np.int32 and n == 0
    (name, a), = recorded_calls
    assert name == "spc_label_u8" and len(a) == len(_lib.SIGNATURES[name][1]) == 13
    # device, stream, nz, ny, nx, d_in, strides, h_structure, d_labels, ws, n, h_nlabels
    assert a[:5] == (0, None, 6, 5, 40) and (a[5].value, a[6], a[7]) == (0x2000, 48, 48 * 9)
    assert np.ctypeslib.as_array(C.cast(a[8], C.POINTER(C.c_uint8)), shape=(27,)).tolist() == s.ravel().astype(int).tolist()
    assert a[9].value == out.ptr and a[11] >= _lib.load().spc_label_workspace_bytes(*shape)
    del recorded_calls[:]
    lab = _StandInArray(shape, np.int32, ptr=0x3000)
    sizes, bbox = ops.label_objects(lab, 9)
    (name, a), = recorded_calls
    assert name == "spc_label_objects_i32" and len(a) == len(_lib.SIGNATURES[name][1]) == 11
    assert a[:5] == (0, None, 6, 5, 40) and a[5].value == 0x3000 and a[6] == 9
    assert (sizes.shape, sizes.dtype, bbox.shape, bbox.dtype) == ((10,), np.int64, (10, 6), np.int32)
    assert a[10] >= _lib.LABEL_OBJECTS_WORKSPACE_BYTES
    del recorded_calls[:]
    keep = _StandInArray((10,), np.uint8, ptr=0x5000)
    sel = ops.label_select(lab, 9, keep)
    (name, a), = recorded_calls
    assert name == "spc_label_select_i32" and len(a) == len(_lib.SIGNATURES[name][1]) == 9
    assert a[5].value == 0x3000 and a[6] == 9 and a[7].value == 0x5000 and a[8].value == sel.ptr
    assert sel.shape == shape and sel.dtype == np.uint8


def test_ops_refuses_what_the_entries_would(recorded_calls):
    x = _StandInArray((6, 5, 40), np.uint8)
    s = np.ones((3, 3, 3), bool)
    view = _StandInArray((6, 5, 40), np.int32)
    view._is_view = True
    with pytest.raises(TypeError):
        ops.label(_StandInArray((6, 5, 40), np.float32), s)
    with pytest.raises(TypeError):
        ops.label(_StandInArray((5, 40), np.uint8), s)
    with pytest.raises(ValueError, match="contiguous"):
        ops.label(x, s, out=view)
    with pytest.raises(ValueError):
        ops.label(x, s, out=_StandInArray((6, 5, 40), np.uint8))
    with pytest.raises(ValueError, match="workspace"):
        ops.label(x, s, workspace=_StandInArray((16,), np.uint8))
    with pytest.raises(NotImplementedError, match="int32"):
        ops.label(_StandInArray((2048, 1024, 1024), np.uint8), s)
    lab = _StandInArray((6, 5, 40), np.int32)
    for f in (lambda a, n: ops.label_objects(a, n), lambda a, n: ops.label_select(a, n, np.ones(max(n, 0) + 1, bool))):
        with pytest.raises(TypeError):
            f(x, 3)
        with pytest.raises(ValueError, match="contiguous"):
            f(view, 3)
        with pytest.raises(ValueError, match="nlabels"):
            f(lab, -1)
    with pytest.raises(ValueError, match="preallocated"):
        ops.label_objects(lab, 3, out={"sizes": _StandInArray((3,), np.int64)})
    with pytest.raises(ValueError, match="entries"):
        ops.label_select(lab, 3, np.ones(3, bool))
    with pytest.raises(TypeError):
        ops.label_select(lab, 3, np.ones(4, np.int32))
    with pytest.raises(ValueError, match="entries"):
        ops.label_select(lab, 3, _StandInArray((5,), np.uint8))
    # LabelMap.select: a uint8 array could be a table or label numbers
    lm = labelling.LabelMap(lab, 3)
    with pytest.raises(TypeError, match="uint8"):
        lm.select(np.array([0, 1, 1, 0], np.uint8))
    with pytest.raises(ValueError, match="n \\+ 1"):
        lm.select(np.ones(3, bool))
    with pytest.raises(ValueError, match="0 to 3"):
        lm.select([4])
    assert recorded_calls == []
