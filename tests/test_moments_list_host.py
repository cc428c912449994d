"""The list of included lane segments (include/spcube_hip.h, spc_moments_list_*) without a GPU: the numpy restatement of
tests/moments_list_layout.py against its own invariants, a walk of the list against a walk of the planes bit for bit, the
keep-or-refuse rule on constructed masks, the plan the library reports (spc_moments_list_plan_f32 needs no device), and the
key rules of ops.MaskSpec with ``_lib.call`` recorded."""
import ctypes as C
import gc

import numpy as np
import pytest

import moments_list_layout as L
from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray

PLANS = [(4, 1, 37), (1, 1, 37), (8, 1, 37), (4, 3, 13), (8, 2, 19)]      # (zw, nsplit, zchunk) over 37 planes


def _inputs(shape=(37, 6, 40), p=0.15, seed=3):
    rng = np.random.default_rng(seed)
    cube = rng.normal(size=shape).astype(np.float32)
    mask = rng.random(shape) < p
    cube[rng.random(shape) < 0.02] = np.nan                    # under included and excluded voxels alike
    return cube, mask


@pytest.mark.parametrize("zw, nsplit, zchunk", PLANS)
def test_every_included_lane_plane_appears_once_in_ascending_order(zw, nsplit, zchunk):
    cube, mask = _inputs()
    nz = cube.shape[0]
    lst = L.build(cube, mask, zw, nsplit, zchunk)
    nib, lan = L.nibbles(mask), L.lanes_of(cube)
    nblocks, nsub = lst["len"].shape
    assert nsub == zw * nsplit and lst["rows"] == int(lst["len"].sum())
    assert np.array_equal(lst["off"].reshape(-1), np.cumsum(lst["len"].reshape(-1).astype(np.uint64)) - lst["len"].reshape(-1))
    seen = np.zeros(nib.shape, dtype=np.int64)
    subs = L.sublist_planes(nz, zw, nsplit, zchunk)
    assert sorted(np.concatenate(subs).tolist()) == list(range(nz)), "the sublists cover every plane once"
    for b in range(nblocks):
        for j in range(nsub):
            o, n = int(lst["off"][b, j]), int(lst["len"][b, j])
            meta, samples = lst["meta"][o:o + n], lst["samples"][o:o + n]
            for l in range(64):
                real = meta[:, l] != 0
                k = int(real.sum())
                assert real[:k].all() and not real[k:].any(), "a lane's entries come first, padding after them"
                assert not samples[k:, l].view(np.uint32).any(), "padding samples are zero"
                z = (meta[:k, l] & 0x0fffffff).astype(np.int64)
                assert np.all(np.diff(z) > 0) and np.isin(z, subs[j]).all()
                g = b * 64 + l
                assert np.array_equal(meta[:k, l] >> 28, nib[z, g]) and (nib[z, g] != 0).all()
                assert np.array_equal(samples[:k, l].view(np.uint32), lan[z, g].view(np.uint32))
                seen[z, g] += 1
            assert n == max(int((meta[:, l] != 0).sum()) for l in range(64)) if n else True
    assert np.array_equal(seen, (nib != 0).astype(np.int64)), "every included lane-plane exactly once, nothing else"
    assert not seen[:, mask.shape[1] * (mask.shape[2] // 4):].any(), "dead lanes hold only padding"


@pytest.mark.parametrize("zw, nsplit, zchunk", PLANS)
def test_a_walk_of_the_list_is_a_walk_of_the_planes_bit_for_bit(zw, nsplit, zchunk):
    cube, mask = _inputs()
    nz = cube.shape[0]
    cen = (np.arange(nz) - nz // 2) * 500.0                     # negative coordinates too: 0 * c is then -0.0
    lst = L.build(cube, mask, zw, nsplit, zchunk)
    a, b = L.walk_planes(cube, mask, cen, zw, nsplit, zchunk), L.walk_list(lst, cen, nz, zw, nsplit, zchunk)
    assert len(a) == len(b) == lst["len"].size
    for x, y in zip(a, b):
        for k in ("s0", "s1", "s2"):
            assert np.array_equal(x[k].view(np.uint64), y[k].view(np.uint64)), k      # the sign of zero included
        assert np.array_equal(x["n"], y["n"]) and np.array_equal(x["bmax"], y["bmax"], equal_nan=True)
        assert np.array_equal(x["imax"], y["imax"])


def test_keep_or_refuse_on_constructed_masks():
    shape = (64, 4, 64)                                        # one block of 64 lanes
    cube = np.zeros(shape, dtype=np.float32)

    def rule(mask):
        lst = L.build(cube, mask, 4, 1, 64)
        return L.keep(lst["rows"], lst["lines"], 1, 64), lst
    kept, lst = rule(np.zeros(shape, dtype=bool))
    assert kept and lst["rows"] == 0 and lst["lines"] == 0     # empty: nothing to read is at most half of the bits
    kept, lst = rule(np.ones(shape, dtype=bool))
    assert not kept and lst["rows"] == 64 and lst["lines"] == 8 * 64   # all ones: 1280 bytes a plane against 1056
    one = np.zeros(shape, dtype=bool)
    one[:, 0, 0:4] = True                                      # one lane full beside 63 empty: a row of padding per plane
    kept, lst = rule(one)
    assert not kept and lst["rows"] == 64 and lst["lines"] == 64
    assert not lst["meta"][:, 1:].any() and (lst["meta"][:, 0] >> 28 == 15).all()
    # every line of every plane fetched for one lane segment of its eight, the lanes equally long: an eighth of the rows
    z, g = np.arange(64).reshape(64, 1), np.arange(64).reshape(1, 64)
    diag = np.repeat(((z // 8 + g) % 8 == 0)[:, :, None], 4, axis=2).reshape(shape)
    kept, lst = rule(diag)
    assert kept and lst["rows"] == 8 and lst["lines"] == 8 * 64
    assert ops.list_is_kept(8, 512, 1, 64) and not ops.list_is_kept(64, 512, 1, 64)
    # the boundary itself is kept: 1280 * rows == (128 * lines + 32 * nblocks * nz) / 2
    assert ops.list_is_kept(1, 18, 1, 8) and L.keep(1, 18, 1, 8) and not ops.list_is_kept(1, 18, 1, 7)


# ---- the plan, from the library --------------------------------------------------------------------------------------

def _plan(shape, want=("m0", "m1", "m2"), ws_bytes=None, flags=_lib.MASK_ARRAY):
    nz, ny, nx = shape
    c = _lib.SpcCube()
    c.d_data, c.nz, c.ny, c.nx, c.row_stride, c.plane_stride = 4096, nz, ny, nx, nx, ny * nx      # made-up addresses: no device
    m = _lib.SpcMask()
    m.flags, m.d_array = flags, 8192 if flags & _lib.MASK_ARRAY else None
    o = _lib.SpcMomentOutputs()
    for k in want:
        setattr(o, "d_" + k, 16384)
    need = int(_lib.load().spc_moments_workspace_bytes(nz, ny, nx)) if ws_bytes is None else ws_bytes
    desc = _lib.SpcMomentsListDesc()
    _lib.call("spc_moments_list_plan_f32", C.byref(c), C.byref(m), C.byref(o), C.c_void_p(32768 if need else None), need, C.byref(desc))
    return desc.zw, desc.nsplit, desc.zchunk, desc.nblocks, desc.nsub


def test_the_plan_the_library_reports(monkeypatch):
    for name in ("SPC_MOMENTS_ZW", "SPC_MOMENTS_NSPLIT", "SPC_MOMENTS_MASK_FIRST", "SPC_MOMENTS_MASK_BITS", "SPC_MOMENTS_LIST"):
        monkeypatch.delenv(name, raising=False)
    assert _plan((4096, 2048, 2048)) == (4, 1, 4096, 16384, 4)                 # the headline launch
    assert _plan((1024, 1024, 1024)) == (8, 1, 1024, 4096, 8)
    assert _plan((37, 6, 40)) == (4, 1, 37, 1, 4)
    assert _plan((9, 4, 16)) == (1, 1, 9, 1, 1)
    assert _plan((520, 4, 64)) == (8, 8, 65, 1, 64)
    assert _plan((520, 4, 64), want=("m0", "argmax")) == (4, 8, 65, 1, 32)     # extrema: four waves
    assert _plan((520, 4, 64), ws_bytes=0) == (8, 1, 520, 1, 8)                # no workspace: one z range
    assert _plan((300, 4, 64)) == (4, 4, 75, 1, 16)
    assert _plan((66000, 2, 8)) == (8, 16, 4125, 1, 128)
    monkeypatch.setenv("SPC_MOMENTS_NSPLIT", "3")
    assert _plan((37, 6, 40)) == (4, 3, 13, 1, 12)


@pytest.mark.parametrize("why, shape, flags, env", [("no mask array", (37, 6, 40), 0, {}), ("8-byte lanes", (37, 6, 42), _lib.MASK_ARRAY, {}),
                                                    ("mask-first off", (37, 6, 40), _lib.MASK_ARRAY, {"SPC_MOMENTS_MASK_FIRST": "0"}),
                                                    ("bits off", (37, 6, 40), _lib.MASK_ARRAY, {"SPC_MOMENTS_MASK_BITS": "0"}),
                                                    ("list off", (37, 6, 40), _lib.MASK_ARRAY, {"SPC_MOMENTS_LIST": "0"})])
def test_where_there_is_no_list(monkeypatch, why, shape, flags, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    with pytest.raises(_lib.HipUnsupported):
        _plan(shape, flags=flags)


def test_the_entries_are_additions_within_abi_8():
    assert _lib.ABI_VERSION == 8 and _lib.load().spc_abi_version() == 8
    for name in ("spc_moments_list_plan_f32", "spc_moments_list_count_f32", "spc_moments_list_fill_f32", "spc_moments_list_f32"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["spc_moments_list_f32"][1][:12] == _lib.SIGNATURES["spc_moments_bits_f32"][1]
    assert C.sizeof(_lib.SpcMomentsListDesc) == 32 and C.sizeof(_lib.SpcMomentsList) == 32 + 8 * 8


# ---- the key rules of the spec, on a recorded library ------------------------------------------------------------------

@pytest.fixture
def recorded(monkeypatch):
    """``_lib.call`` recorded (test_dirty_memory_host.py's fake): spc_malloc hands out made-up addresses, the list's plan is
    one block and one sublist, and the counts read back are whatever the host memory held, so ``get`` is replaced by zeros:
    an empty list, which the rule keeps"""
    calls, nxt = [], [1 << 32]

    def call(name, *a):
        calls.append(name)
        if name == "spc_malloc":
            a[2]._obj.value = nxt[0]
            nxt[0] += (int(a[1]) + 255) // 256 * 256 + 4096
        if name in ("spc_moments_list_plan_f32", "spc_moments_list_count_f32"):
            d = a[-1]._obj
            d.zw, d.nsplit, d.zchunk, d.nblocks, d.nsub = 1, 1, 8, 1, 1

    class _Lib:
        spc_moments_workspace_bytes = staticmethod(lambda *a: 0)
        spc_mask_bits_bytes = staticmethod(lambda nz, ny, nx: -(-(ny * (nx // 4)) // 64) * nz * 32)
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(_lib, "load", lambda: _Lib)
    monkeypatch.setattr(DeviceArray, "get", lambda self, stream=None: np.zeros(self.shape, dtype=self.dtype))
    monkeypatch.delenv("SPC_MOMENTS_LIST", raising=False)
    monkeypatch.delenv("SPC_MOMENTS_MASK_BITS", raising=False)
    return calls


def _launch(cube, spec, calls):
    del calls[:]
    ops.moments(cube, DeviceArray((cube.shape[0],), np.float64), mask=spec)
    return [n for n in calls if n.startswith("spc_m") and n != "spc_malloc" and not n.startswith("spc_memcpy")]


SHAPE = (8, 4, 16)
BUILD = ["spc_mask_pack_bits"], ["spc_moments_list_plan_f32", "spc_moments_list_count_f32", "spc_moments_list_fill_f32", "spc_moments_list_f32"]


def _pair():
    return DeviceArray(SHAPE, np.float32), ops.MaskSpec(_lib.MASK_ARRAY, array=DeviceArray(SHAPE, np.uint8))


def test_nothing_changes_for_the_first_two_uses_and_the_third_builds(recorded):
    cube, spec = _pair()
    assert _launch(cube, spec, recorded) == ["spc_moments_f32"]
    assert _launch(cube, spec, recorded) == ["spc_mask_pack_bits", "spc_moments_bits_f32"] and spec._list is None
    assert _launch(cube, spec, recorded) == BUILD[1] and spec._list is not None and spec._list.rows == 0
    assert _launch(cube, spec, recorded) == ["spc_moments_list_f32"]


def test_the_switch_at_zero_builds_and_passes_nothing(recorded, monkeypatch):
    cube, spec = _pair()
    monkeypatch.setenv("SPC_MOMENTS_LIST", "0")
    for expect in (["spc_moments_f32"], ["spc_mask_pack_bits", "spc_moments_bits_f32"], ["spc_moments_bits_f32"], ["spc_moments_bits_f32"]):
        assert _launch(cube, spec, recorded) == expect
    assert spec._list is None and not spec._list_failed


def test_a_written_cube_another_cube_and_invalidate_drop_the_list(recorded):
    cube, spec = _pair()
    for _ in range(3):
        _launch(cube, spec, recorded)
    bits = spec._bits
    assert spec._list is not None
    cube.mark_written()                                        # upload(), an operator's out=, scale_inplace
    assert _launch(cube, spec, recorded) == ["spc_moments_bits_f32"] and spec._list is None and spec._bits is bits
    assert _launch(cube, spec, recorded) == BUILD[1]           # the same cube as the launch before, the bits packed
    other = DeviceArray(SHAPE, np.float32)
    assert _launch(other, spec, recorded) == ["spc_moments_bits_f32"] and spec._list is None and spec._bits is bits
    assert _launch(cube, spec, recorded) == ["spc_moments_bits_f32"]      # alternating cubes never build
    assert _launch(other, spec, recorded) == ["spc_moments_bits_f32"]
    assert _launch(other, spec, recorded) == BUILD[1]
    rows = other.rows(1, 3)                                    # a view is another key, its write is the root's
    spec2 = ops.MaskSpec(_lib.MASK_ARRAY, array=spec.array.rows(1, 3))
    for _ in range(3):
        _launch(rows, spec2, recorded)
    assert spec2._list is not None
    other.mark_written()
    assert _launch(rows, spec2, recorded) == ["spc_moments_bits_f32"] and spec2._list is None
    spec.invalidate()
    assert (spec._list, spec._list_key, spec._list_root, spec._list_failed, spec._bits) == (None, None, None, False, None)
    assert _launch(other, spec, recorded) == ["spc_moments_f32"]


def test_a_rewritten_mask_drops_the_bits_and_the_list(recorded):
    cube, spec = _pair()
    for _ in range(3):
        _launch(cube, spec, recorded)
    spec.array.mark_written()
    assert _launch(cube, spec, recorded) == ["spc_moments_f32"] and spec._list is None and spec._bits is None
    assert _launch(cube, spec, recorded) == ["spc_mask_pack_bits", "spc_moments_bits_f32"]
    assert _launch(cube, spec, recorded) == BUILD[1]


def test_a_new_array_at_a_freed_cubes_address_never_matches(recorded):
    cube, spec = _pair()
    for _ in range(3):
        _launch(cube, spec, recorded)
    assert spec._list is not None
    ptr, key = cube.ptr, spec._list_key
    cube._owns = False                                         # (nothing to free on a recorded library)
    del cube
    gc.collect()
    assert spec._list_root() is None
    again = DeviceArray(SHAPE, np.float32, ptr=ptr)            # the same address, shape, strides and generation 0
    assert (spec._bits_key,) + ops._cube_key(again) == key
    assert _launch(again, spec, recorded) == ["spc_moments_bits_f32"] and spec._list is None
    assert _launch(again, spec, recorded) == BUILD[1]


def test_a_refusal_is_remembered_and_silent(recorded, monkeypatch):
    cube, spec = _pair()
    monkeypatch.setattr(DeviceArray, "get", lambda self, stream=None: np.full(self.shape, 5, dtype=self.dtype))   # 5 rows, 5 lines
    _launch(cube, spec, recorded)
    _launch(cube, spec, recorded)
    assert _launch(cube, spec, recorded) == ["spc_moments_list_plan_f32", "spc_moments_list_count_f32", "spc_moments_bits_f32"]
    assert spec._list is None and spec._list_failed
    assert _launch(cube, spec, recorded) == ["spc_moments_bits_f32"]          # it does not count again
    cube.mark_written()
    _launch(cube, spec, recorded)
    assert not spec._list_failed                               # another key: the question is open again


def test_the_slots_for_the_list_are_no_part_of_what_a_spec_says():
    a, b = ops.MaskSpec(_lib.MASK_GT, 1.0, 0.0), ops.MaskSpec(_lib.MASK_GT, 1.0, 0.0)
    b._list_failed, b._list_key = True, (1, 2)
    assert a == b and repr(a) == repr(b) and "_list" not in repr(a)
