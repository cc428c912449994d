"""tests/dirty_memory.py without a GPU: what ``dirty`` does, call by call, on a recorded ``_lib.call`` (the fake library of
test_views_host.py, with an spc_malloc that hands out made-up pointers), and what ``same_under_every_pattern`` can and
cannot see, pattern by pattern, on a toy operator in numpy that is wrong in the three ways a kernel depends on memory."""
import ctypes as C

import numpy as np
import pytest

import dirty_memory as DM
from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray


@pytest.fixture
def recorded(monkeypatch):
    calls, nxt = [], [1 << 32]

    def call(name, *a):
        calls.append((name, a))
        if name == "spc_malloc":
            a[2]._obj.value = nxt[0]
            nxt[0] += (int(a[1]) + 255) // 256 * 256 + 4096
    monkeypatch.setattr(_lib, "call", call)
    monkeypatch.setattr(ops, "_ws_cache", {})
    return calls


def _val(p):
    return getattr(p, "value", p)


def _fills(calls):
    """(pointer, bytes, value or None for an upload) of every fill"""
    out = []
    for name, a in calls:
        if name == "spc_memset":
            out.append((_val(a[1]), int(a[3]), int(a[2])))
        elif name == "spc_memcpy_h2d":
            out.append((_val(a[1]), int(a[3]), None))
    return out


@pytest.mark.parametrize("pattern", DM.PATTERNS, ids=[str(p) for p in DM.PATTERNS])
def test_dirty_fills_every_cached_scratch_buffer_once_and_syncs(recorded, pattern):
    a, b = DeviceArray((1 << 16,), np.uint8, 0), DeviceArray((3 << 16,), np.uint8, 0)
    ops._ws_cache[(0, 0, 1)], ops._ws_cache[(0, 77, 2)] = a, b
    del recorded[:]
    with DM.dirty(pattern):
        got = list(recorded)
    fills = _fills(got)
    value = None if pattern == "random" else pattern
    assert sorted(fills) == sorted([(a.ptr, a.nbytes, value), (b.ptr, b.nbytes, value)])
    # the device is synchronised after the fills, before the block runs
    assert got[-1] == ("spc_device_sync", (0,)) and [n for n, _ in got].count("spc_device_sync") == 1
    assert all(_val(args[4]) is None for name, args in got if name in ("spc_memset", "spc_memcpy_h2d")), "fills run on the null stream"


@pytest.mark.parametrize("pattern", DM.PATTERNS, ids=[str(p) for p in DM.PATTERNS])
def test_dirty_fills_every_owning_allocation_and_no_view(recorded, pattern):
    value = None if pattern == "random" else pattern
    with DM.dirty(pattern):
        del recorded[:]
        own = DeviceArray((5, 6, 7), np.float32, 0)
        assert _fills(recorded) == [(own.ptr, 5 * 6 * 7 * 4, value)]
        assert recorded[-1][0] == "spc_stream_sync" and _val(recorded[-1][1][1]) is None, "the null stream is drained after the fill"
        del recorded[:]
        for view in (own.rows(1, 3), own.planes(1, 2), own.swap01(), own.reshape((30, 7)), DeviceArray((4,), np.uint8, 0, ptr=own.ptr + 8, owner=own)):
            assert not view._owns
        assert _fills(recorded) == [] and not recorded, "a view (ptr= given) is not filled"
        # from_numpy and zeros: filled, then overwritten as they are today - the fill comes first
        z = DeviceArray.zeros((9,), np.float64, 0)
        assert _fills(recorded) == [(z.ptr, 72, value), (z.ptr, 72, 0)]
        del recorded[:]
        u = DeviceArray.from_numpy(np.arange(6, dtype=np.int32), 0)
        assert _fills(recorded) == [(u.ptr, 24, value), (u.ptr, 24, None)]
        del recorded[:]
        DeviceArray((0, 3), np.float32, 0)
        assert _fills(recorded) == [], "nothing to fill in an empty array"


def test_a_scratch_buffer_that_grows_inside_the_block_is_filled(recorded, monkeypatch):
    class _Lib:
        @staticmethod
        def spc_workspace_bytes(*a):
            return 1 << 20
    monkeypatch.setattr(_lib, "load", lambda: _Lib)
    with DM.dirty(0x7F):
        del recorded[:]
        ptr, n = ops.workspace(0, None, 0, 1, 1, 1)
        assert _fills(recorded) == [(ptr.value, n, 0x7F)] and n >= 1 << 20


def test_random_fills_differ_from_one_allocation_to_the_next_and_repeat_from_run_to_run(recorded):
    seen = []
    for _ in range(2):
        with DM.dirty("random") as f:
            DeviceArray((64,), np.uint8, 0)
            DeviceArray((64,), np.uint8, 0)
            assert f.count == 2
        seen.append([bytes(C.string_at(_val(a[2]), 64)) for n, a in recorded if n == "spc_memcpy_h2d"][-2:])
    assert seen[0] == seen[1] and seen[0][0] != seen[0][1]
    assert seen[0][0] == DM.pattern_bytes("random", 64, 0).tobytes() and seen[0][1] == DM.pattern_bytes("random", 64, 1).tobytes()


def test_dirty_restores_the_constructor_after_a_normal_exit_and_after_an_exception(recorded):
    original = DeviceArray.__init__
    with DM.dirty(0xFF):
        assert DeviceArray.__init__ is not original
    assert DeviceArray.__init__ is original
    with pytest.raises(RuntimeError, match="inside"):
        with DM.dirty("random"):
            assert DeviceArray.__init__ is not original
            raise RuntimeError("inside")
    assert DeviceArray.__init__ is original
    del recorded[:]
    DeviceArray((8,), np.float32, 0)
    assert _fills(recorded) == []
    with pytest.raises(ValueError, match="unknown pattern"):
        with DM.dirty(0x55):
            pass
    assert DeviceArray.__init__ is original


def test_patterns_read_as_the_table_says():
    for p, f32, f64, i32, byte in ((0x00, 0.0, 0.0, 0, 0), (0xFF, np.nan, np.nan, -1, 255), (0x7F, 3.39e38, 1.4e306, 2139062143, 127)):
        b = DM.pattern_bytes(p, 8)
        assert b.view(np.int32)[0] == i32 and b[0] == byte
        for got, exp in ((b.view(np.float32)[0], f32), (b.view(np.float64)[0], f64)):
            assert (np.isnan(got) and np.isnan(exp)) or abs(got - exp) <= 0.02 * abs(exp)     # (the table rounds to two or three digits)
    assert np.isfinite(DM.pattern_bytes(0x7F, 8).view(np.float32)).all()


# ---- sensitivity of the comparison rule: a toy operator (column sums of a (7, 10) array in tiles of 4 columns: 4, 4 and a
# ragged 2) with a "scratch" array and a fresh output that `enter` fills the way dirty() fills device memory -----------------------
DEFECTS = ("accumulates into uncleared scratch", "skips the last tile of its output", "nonzero status byte taken for done")


class _Toy:
    """scratch: 10 float64 partial sums + 3 status bytes, one per tile.  The producer adds the tile's column sums to the
    partial sums and marks the tile done; the finish pass writes a done tile's sums to the output and NaN ("no data") for a
    tile that is not done.  Written right, it clears the partial sums, marks every tile and writes every output cell.
    The three defects: the clear of the partial sums is missing; the finish pass walks 10 // 4 tiles; the producer marks
    10 // 4 tiles and the finish pass takes whatever nonzero byte it finds at the third for 'done'."""

    def __init__(self, defect=None):
        assert defect is None or defect in DEFECTS
        self.defect = defect
        self.x = np.arange(70, dtype=np.float64).reshape(7, 10) - 20.0
        self.pattern = 0

    def enter(self, pattern):
        import contextlib
        self.pattern = pattern
        return contextlib.nullcontext()

    def _alloc(self, n, dtype, counter):
        return DM.pattern_bytes(self.pattern, n * np.dtype(dtype).itemsize, counter).view(dtype).copy()

    def run(self):
        partial, status, out = self._alloc(10, np.float64, 0), self._alloc(3, np.uint8, 1), self._alloc(10, np.float64, 2)
        tiles = [(0, 4), (4, 8), (8, 10)]
        if self.defect != "accumulates into uncleared scratch":
            partial[:] = 0.0
        marked = tiles[:2] if self.defect == "nonzero status byte taken for done" else tiles
        if self.defect != "nonzero status byte taken for done":
            status[:] = 0
        with np.errstate(all="ignore"):
            partial += self.x.sum(axis=0)
        for t in range(len(marked)):
            status[t] = 1
        finished = tiles[:2] if self.defect == "skips the last tile of its output" else tiles
        for t, (a, b) in enumerate(finished):
            out[a:b] = partial[a:b] if status[t] != 0 else np.nan
        return {"sums": out}

    def check(self, first):
        assert np.array_equal(first["sums"], self.x.sum(axis=0))


def _exposing(defect):
    """the patterns under which the toy's result differs from the right one"""
    toy = _Toy(defect)
    right = toy.x.sum(axis=0)
    bad = []
    for p in DM.PATTERNS:
        with toy.enter(p):
            got = toy.run()["sums"]
        if not np.array_equal(got, right):
            bad.append(p)
    return bad


def test_the_toy_operator_without_a_defect_passes():
    toy = _Toy()
    first = DM.same_under_every_pattern(toy.run, toy.check, enter=toy.enter)
    assert first["sums"].dtype == np.float64 and _exposing(None) == []


# Which patterns expose which defect.  The accumulate form is invisible under 0x00: zeroed memory is what it assumes.  The
# status form is invisible under 0xFF and 0x7F (and under the random bytes, which are nonzero here): a set byte is what it
# assumes.  The skipped tile is wrong under every pattern - under 0x00 it reads as a plausible 0.0.  No single pattern shows
# all three, and none of 0x00 / 0xFF alone shows two of them against each other: hence four.
EXPOSED_BY = {
    "accumulates into uncleared scratch": [0xFF, 0x7F, "random"],
    "skips the last tile of its output": [0x00, 0xFF, 0x7F, "random"],
    "nonzero status byte taken for done": [0x00],
}


@pytest.mark.parametrize("defect", DEFECTS)
def test_every_way_to_depend_on_memory_is_reported(defect):
    toy = _Toy(defect)
    with pytest.raises(AssertionError, match="depends on what memory held") as hit:
        DM.same_under_every_pattern(toy.run, toy.check, enter=toy.enter)
    text = str(hit.value)
    assert "sums under" in text and "places, first [[" in text, text
    assert _exposing(defect) == EXPOSED_BY[defect]
    # the comparison alone reports it, without a reference
    with pytest.raises(AssertionError, match="depends on what memory held"):
        DM.same_under_every_pattern(toy.run, enter=toy.enter)


def test_one_pattern_hides_half_the_ways():
    """under 0x00 alone the accumulating operator passes its reference check, under 0xFF, 0x7F and both together the
    status form does: each is caught only because the other kind of pattern runs too"""
    toy = _Toy("accumulates into uncleared scratch")
    DM.same_under_every_pattern(toy.run, toy.check, patterns=(0x00,), enter=toy.enter)
    toy = _Toy("nonzero status byte taken for done")
    for patterns in ((0xFF,), (0x7F,), (0xFF, 0x7F)):
        DM.same_under_every_pattern(toy.run, toy.check, patterns=patterns, enter=toy.enter)
    with pytest.raises(AssertionError):
        DM.same_under_every_pattern(toy.run, toy.check, patterns=(0x00,), enter=toy.enter)       # (its reference check)


def test_the_comparison_reads_nan_as_equal_and_dtype_and_shape_as_part_of_the_result():
    a = {"m": np.array([1.0, np.nan, -0.0], np.float32)}
    assert DM.compare(a, {"m": np.array([1.0, np.nan, -0.0], np.float32)}, 0xFF) == []
    assert len(DM.compare(a, {"m": np.array([1.0, np.nan, -0.0], np.float64)}, 0xFF)) == 1
    assert len(DM.compare(a, {"m": np.array([[1.0, np.nan, -0.0]], np.float32)}, 0xFF)) == 1
    assert len(DM.compare(a, {"n": a["m"]}, 0xFF)) == 1
    msg = DM.compare(a, {"m": np.array([1.0, 2.0, 3.0], np.float32)}, "random")
    assert len(msg) == 1 and "2 places" in msg[0] and "[[1], [2]]" in msg[0] and "'random'" in msg[0]
    assert len(DM.compare({"s": np.float64(2.0)}, {"s": np.float64(3.0)}, 0x7F)) == 1
    assert DM.compare({"s": np.float64(np.nan)}, {"s": np.float64(np.nan)}, 0x7F) == []
