"""The voxel list (include/spcube_hip.h, spc_moments_vlist_*) without a GPU: the numpy restatement of
tests/moments_vlist_layout.py against a direct per-column walk of small random masks, a walk of the voxel list against a
walk of the planes bit for bit, the keep-or-refuse rule, the struct sizes, and the tier's rules in ops.MaskSpec with
``_lib.call`` recorded."""
import ctypes as C

import numpy as np
import pytest

import moments_list_layout as L
import moments_vlist_layout as V
from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray

PLANS = [(4, 1, 37), (1, 1, 37), (8, 1, 37), (4, 3, 13), (8, 2, 19)]      # (zw, nsplit, zchunk) over 37 planes


def _inputs(shape=(37, 6, 40), p=0.15, seed=3):
    rng = np.random.default_rng(seed)
    cube = rng.normal(size=shape).astype(np.float32)
    mask = rng.random(shape) < p
    cube[rng.random(shape) < 0.02] = np.nan                    # under included and excluded voxels alike
    return cube, mask


@pytest.mark.parametrize("p", [0.03, 0.15, 0.6])
@pytest.mark.parametrize("zw, nsplit, zchunk", PLANS)
def test_the_restatement_is_a_direct_walk_of_the_columns(zw, nsplit, zchunk, p):
    cube, mask = _inputs(p=p)
    lst = L.build(cube, mask, zw, nsplit, zchunk)
    vl = V.build(lst)
    want = V.direct(cube, mask, zw, nsplit, zchunk)
    nblocks, nsub = vl["vlen"].shape
    assert (nblocks, nsub) == lst["len"].shape and vl["vrows"] == int(vl["vlen"].sum())
    flat = vl["vlen"].reshape(-1).astype(np.uint64)
    assert np.array_equal(vl["voff"].reshape(-1), np.cumsum(flat) - flat)
    total = 0
    for b in range(nblocks):
        for j in range(nsub):
            o, n = int(vl["voff"][b, j]), int(vl["vlen"][b, j])
            assert n == max(len(want[b, j, l]) for l in range(64))
            for l in range(64):
                pairs = want[b, j, l]
                got = vl["entries"][o:o + n, l]
                assert [(int(a), int(m)) for a, m in got[:len(pairs)]] == pairs
                assert not got[len(pairs):].any(), "padding is all zero: bit 30 clear"
                total += len(pairs)
    assert total == int(mask.sum()), "every included voxel exactly once"
    assert total == int(((vl["entries"][:, :, 1] >> 30) & 1).sum())
    # excluded voxels of an included segment never enter
    col = (vl["entries"][:, :, 1] >> 28) & 3
    assert col[vl["entries"][:, :, 1] == 0].sum() == 0 and vl["entries"][:, :, 1].max(initial=0) < (1 << 31)


@pytest.mark.parametrize("zw, nsplit, zchunk", PLANS)
def test_a_walk_of_the_voxel_list_is_a_walk_of_the_planes_bit_for_bit(zw, nsplit, zchunk):
    cube, mask = _inputs()
    nz = cube.shape[0]
    cen = (np.arange(nz) - nz // 2) * 500.0                     # negative coordinates too: 0 * c is then -0.0
    vl = V.build(L.build(cube, mask, zw, nsplit, zchunk))
    a, b = L.walk_planes(cube, mask, cen, zw, nsplit, zchunk), V.walk_vlist(vl, cen, nz, zw, nsplit, zchunk)
    assert len(a) == len(b) == vl["vlen"].size
    for x, y in zip(a, b):
        for k in ("s0", "s1", "s2"):
            assert np.array_equal(x[k].view(np.uint64), y[k].view(np.uint64)), k      # the sign of zero included
        assert np.array_equal(x["n"], y["n"]) and np.array_equal(x["bmax"], y["bmax"], equal_nan=True)
        assert np.array_equal(x["imax"], y["imax"])


def test_keep_or_refuse():
    shape = (64, 4, 64)                                        # one block of 64 lanes
    cube = np.zeros(shape, dtype=np.float32)

    def rule(mask):
        lst = L.build(cube, mask, 4, 1, 64)
        vl = V.build(lst)
        return V.keep(vl["vrows"], lst["rows"]), lst["rows"], vl["vrows"]
    z, g = np.arange(64).reshape(64, 1, 1), np.arange(64).reshape(1, 64, 1)
    col = np.arange(4).reshape(1, 1, 4)
    seg = (z // 8 + g) % 8 == 0
    assert rule((seg & (col == g % 4)).reshape(shape)) == (True, 8, 8)         # one voxel of a segment: 512 against 1280
    assert rule((seg & (col != g % 4)).reshape(shape)) == (False, 8, 24)       # three: 1536 against 1280
    assert rule((seg & (col < 2)).reshape(shape)) == (False, 8, 16)            # two: 1024 is more than half of 1280
    assert rule(np.ones(shape, dtype=bool)) == (False, 64, 256)
    assert ops.vlist_is_kept(5, 4) and V.keep(5, 4) and not ops.vlist_is_kept(6, 4) and not V.keep(6, 4)   # the boundary is kept
    assert ops.vlist_is_kept(0, 0)


def test_the_entries_are_additions_within_abi_8():
    assert _lib.ABI_VERSION == 8 and _lib.load().spc_abi_version() == 8
    for name in ("spc_moments_vlist_count_f32", "spc_moments_vlist_fill_f32", "spc_moments_vlist_f32"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["spc_moments_vlist_f32"][1][:13] == _lib.SIGNATURES["spc_moments_list_f32"][1]
    assert C.sizeof(_lib.SpcMomentsListDesc) == 32 and C.sizeof(_lib.SpcMomentsList) == 32 + 8 * 8     # nothing existing moved
    assert C.sizeof(_lib.SpcMomentsVlist) == 32 + 6 * 8
    assert _lib.SpcMomentsVlist.d_entries.offset == 32 and _lib.SpcMomentsVlist.rows.offset == 72


# ---- the tier's rules, on a recorded library ---------------------------------------------------------------------------

@pytest.fixture
def recorded(monkeypatch):
    """``_lib.call`` recorded (test_moments_list_host.py's fake): spc_malloc hands out made-up addresses and the list's plan is
    one block and one sublist.  The counts read back are ``recorded.counts``, in the order they are read: the list's len, its
    lines, then the voxel list's vlen.  (2, 40, 2): a list of 2 rows, kept (2560 * 2 <= 128 * 40 + 32 * 8), and a voxel list
    of 2 rows, kept (1024 * 2 <= 1280 * 2)"""
    class Rec(list):
        counts = [2, 40, 2]
    calls, nxt, reads = Rec(), [1 << 32], [0]

    def call(name, *a):
        calls.append(name)
        if name == "spc_malloc":
            a[2]._obj.value = nxt[0]
            nxt[0] += (int(a[1]) + 255) // 256 * 256 + 4096
        if name in ("spc_moments_list_plan_f32", "spc_moments_list_count_f32"):
            d = a[-1]._obj
            d.zw, d.nsplit, d.zchunk, d.nblocks, d.nsub = 1, 1, 8, 1, 1
        if name == "spc_moments_list_count_f32":
            reads[0] = 0

    def get(self, stream=None):
        v = calls.counts[min(reads[0], len(calls.counts) - 1)]
        reads[0] += 1
        return np.full(self.shape, v, dtype=self.dtype)

    class _Lib:
        spc_moments_workspace_bytes = staticmethod(lambda *a: 0)
        spc_mask_bits_bytes = staticmethod(lambda nz, ny, nx: -(-(ny * (nx // 4)) // 64) * nz * 32)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "load", lambda: _Lib)
    monkeypatch.setattr(DeviceArray, "get", get)
    for name in ("SPC_MOMENTS_LIST", "SPC_MOMENTS_MASK_BITS", "SPC_MOMENTS_VLIST"):
        monkeypatch.delenv(name, raising=False)
    return calls


def _launch(cube, spec, calls):
    del calls[:]
    ops.moments(cube, DeviceArray((cube.shape[0],), np.float64), mask=spec)
    return [n for n in calls if n.startswith("spc_m") and n != "spc_malloc" and not n.startswith("spc_memcpy")]


SHAPE = (8, 4, 16)
LIST_BUILD = ["spc_moments_list_plan_f32", "spc_moments_list_count_f32", "spc_moments_list_fill_f32", "spc_moments_list_f32"]
VLIST_BUILD = ["spc_moments_vlist_count_f32", "spc_moments_vlist_fill_f32", "spc_moments_vlist_f32"]


def _pair():
    return DeviceArray(SHAPE, np.float32), ops.MaskSpec(_lib.MASK_ARRAY, array=DeviceArray(SHAPE, np.uint8))


def _built(recorded, cube=None, spec=None):
    if cube is None:
        cube, spec = _pair()
    assert _launch(cube, spec, recorded) == ["spc_moments_f32"]
    assert _launch(cube, spec, recorded) == ["spc_mask_pack_bits", "spc_moments_bits_f32"]
    assert _launch(cube, spec, recorded) == LIST_BUILD and spec._list.rows == 2 and spec._vlist is None and not spec._vlist_failed
    assert _launch(cube, spec, recorded) == VLIST_BUILD
    return cube, spec


def test_the_fourth_launch_compacts_a_kept_list_and_the_fifth_only_reads(recorded):
    cube, spec = _built(recorded)
    vl, lst = spec._vlist, spec._list
    assert vl is not None and vl.rows == 2 and vl.nbytes == 1024 and vl.entries.nbytes == 1024 and not spec._vlist_failed
    assert bytes(vl.c.desc) == bytes(lst.c.desc) and vl.c.nsublists == 1 and vl.c.entries_bytes == 1024
    assert _launch(cube, spec, recorded) == ["spc_moments_vlist_f32"]
    assert _launch(cube, spec, recorded) == ["spc_moments_vlist_f32"]
    assert spec._vlist is vl and spec._list is lst and lst.samples is not None, "the list's arrays stay"


def test_a_refusal_is_remembered_and_does_not_count_again(recorded):
    recorded.counts = [2, 40, 6]                               # three voxels of a segment: 1024 * 6 > 1280 * 2
    cube, spec = _pair()
    for _ in range(3):
        _launch(cube, spec, recorded)
    lst = spec._list
    assert _launch(cube, spec, recorded) == ["spc_moments_vlist_count_f32", "spc_moments_list_f32"]
    assert spec._vlist is None and spec._vlist_failed and spec._list is lst
    assert _launch(cube, spec, recorded) == ["spc_moments_list_f32"]
    assert _launch(cube, spec, recorded) == ["spc_moments_list_f32"] and spec._list is lst
    cube.mark_written()
    _launch(cube, spec, recorded)
    assert not spec._vlist_failed                              # another key: the question is open again


def test_the_switch_at_zero_builds_and_passes_nothing(recorded, monkeypatch):
    monkeypatch.setenv("SPC_MOMENTS_VLIST", "0")
    cube, spec = _pair()
    for expect in (["spc_moments_f32"], ["spc_mask_pack_bits", "spc_moments_bits_f32"], LIST_BUILD, ["spc_moments_list_f32"],
                   ["spc_moments_list_f32"]):
        assert _launch(cube, spec, recorded) == expect
    assert spec._vlist is None and spec._vlist_failed and spec._list is not None


def test_an_empty_list_is_never_compacted(recorded):
    recorded.counts = [0, 0, 0]
    cube, spec = _pair()
    for _ in range(3):
        _launch(cube, spec, recorded)
    assert spec._list is not None and spec._list.rows == 0
    for _ in range(3):
        assert _launch(cube, spec, recorded) == ["spc_moments_list_f32"]
    assert spec._vlist is None and not spec._vlist_failed


def test_a_refused_list_has_no_voxel_list(recorded):
    recorded.counts = [5, 5, 5]                                # the list itself is refused
    cube, spec = _pair()
    for _ in range(3):
        _launch(cube, spec, recorded)
    assert spec._list is None and spec._list_failed
    assert _launch(cube, spec, recorded) == ["spc_moments_bits_f32"] and spec._vlist is None and not spec._vlist_failed


def test_whatever_drops_the_list_drops_the_voxel_list(recorded):
    cube, spec = _built(recorded)
    bits = spec._bits
    cube.mark_written()                                        # upload(), an operator's out=, scale_inplace
    assert _launch(cube, spec, recorded) == ["spc_moments_bits_f32"]
    assert (spec._list, spec._vlist, spec._vlist_failed) == (None, None, False) and spec._bits is bits
    assert _launch(cube, spec, recorded) == LIST_BUILD and spec._vlist is None
    assert _launch(cube, spec, recorded) == VLIST_BUILD and spec._vlist is not None
    other = DeviceArray(SHAPE, np.float32)                     # another cube
    assert _launch(other, spec, recorded) == ["spc_moments_bits_f32"] and spec._list is None and spec._vlist is None
    assert _launch(other, spec, recorded) == LIST_BUILD
    assert _launch(other, spec, recorded) == VLIST_BUILD
    spec.array.mark_written()                                  # a rewritten mask
    assert _launch(other, spec, recorded) == ["spc_moments_f32"]
    assert (spec._bits, spec._list, spec._vlist) == (None, None, None)
    assert _launch(other, spec, recorded) == ["spc_mask_pack_bits", "spc_moments_bits_f32"]
    assert _launch(other, spec, recorded) == LIST_BUILD
    assert _launch(other, spec, recorded) == VLIST_BUILD
    spec.invalidate()
    assert (spec._list, spec._vlist, spec._vlist_failed, spec._bits) == (None, None, False, None)
    assert _launch(other, spec, recorded) == ["spc_moments_f32"]
    spec._vlist_failed = True
    spec._drop_bits()
    assert not spec._vlist_failed


def test_the_slots_for_the_voxel_list_are_no_part_of_what_a_spec_says():
    a, b = ops.MaskSpec(_lib.MASK_GT, 1.0, 0.0), ops.MaskSpec(_lib.MASK_GT, 1.0, 0.0)
    b._vlist_failed, b._vlist = True, object()
    assert a == b and repr(a) == repr(b) and "_vlist" not in repr(a)
