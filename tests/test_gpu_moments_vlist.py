"""GPU: a kept list of included lane segments is compacted, on a spec's fourth use of one cube, into a VOXEL list of one
8-byte entry per included voxel (spc_moments_vlist_* / ops.MaskSpec): the device-built voxel list is the layout of
include/spcube_hip.h byte for byte, padding included; the maps of the launch that reads it are those of the byte march bit
for bit; it is kept only where it halves the list's bytes, and dropped with the list.

Shapes: those of tests/test_gpu_moments_list.py (the smallest that reach each path of the loader), and one whose sublists are
longer than two batches of 16 rows.  Mask bytes are drawn from {1, 2, 128, 255}.  Every array of the C-entry tests is allocated
on dirty memory: each such test opens ONE DM.dirty("random") block (opening it fills every cached scratch buffer, which is what
costs time late in a long run)."""
import ctypes as C

import numpy as np
import pytest

import dirty_memory as DM
import moments_list_layout as L
import moments_vlist_layout as V
from spectral_cube_amd import _lib, ops, synth
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

VLIST, LIST, FIRST = "SPC_MOMENTS_VLIST", "SPC_MOMENTS_LIST", "SPC_MOMENTS_MASK_FIRST"
SUMS, COUNT = ("m0", "m1", "m2"), ("m0", "m1", "m2", "nvalid")
EXTREMA = ("m0", "m1", "m2", "nvalid", "argmax", "argmin", "vmax", "vmin")
WANTS = {"sums": SUMS, "count": COUNT, "extrema": EXTREMA}
ARRAY, THRESHOLDS = (0, 0.0, 0.0), (_lib.MASK_FINITE | _lib.MASK_GT | _lib.MASK_LE, -0.25, 3.0)

# shape, switches, what it reaches
SHAPES = [((37, 6, 40), {}, "ZW = 4, sublists shorter than a batch, dead lanes (60 lane groups)"),
          ((9, 4, 16), {}, "ZW = 1"),
          ((520, 4, 64), {}, "ZW = 8 with a z split"),
          ((300, 4, 64), {}, "nsplit > 1, ZW = 4"),
          ((37, 6, 40), {"SPC_MOMENTS_NSPLIT": "3"}, "a forced split"),
          ((66000, 2, 8), {}, "more than 65535 planes")]
_ids = [("x".join(map(str, s)) + ("," + ",".join("%s=%s" % (k[12:], v) for k, v in e.items()) if e else "")) for s, e, _ in SHAPES]


def _segments(d):
    """(nz, ngroups, 1): lane group g includes the planes z with (z // 8 + g) % 8 == 0 (test_gpu_moments_list.py's _diagonal:
    every 128-byte line of every plane holds one included lane segment, so the LIST is kept at (37, 6, 40), (300, 4, 64)
    and (520, 4, 64)), and g itself"""
    nz, ny, nx = d.shape
    g = np.arange(ny * (nx // 4)).reshape(1, -1, 1)
    z = np.arange(nz).reshape(nz, 1, 1)
    return (z // 8 + g) % 8 == 0, g


def _one_per_segment(d):
    """one voxel of every kept segment, its column varying by lane: the voxel list has exactly the list's rows and is KEPT
    (1024 <= 1280)"""
    seg, g = _segments(d)
    return (seg & (np.arange(4).reshape(1, 1, 4) == g % 4)).reshape(d.shape)


def _one_to_four(d):
    """1 .. 4 voxels of every kept segment, by lane: lanes of unequal length, refused by the rule"""
    seg, g = _segments(d)
    return (seg & (np.arange(4).reshape(1, 1, 4) <= g % 4)).reshape(d.shape)


def _diagonal(d):
    """test_gpu_moments_list.py's: three voxels of every kept segment - the list is kept, the voxel list refused (3 * 1024 > 1280)"""
    seg, g = _segments(d)
    return (seg & (np.arange(4).reshape(1, 1, 4) != g % 4)).reshape(d.shape)


def _one_voxel(d):
    m = np.zeros(d.shape, dtype=bool)
    m[d.shape[0] // 2, -1, -1] = True
    return m


def _one_lane(d):
    """lane group 1 holds every plane, all other lanes nothing: maximal padding"""
    m = np.zeros(d.shape, dtype=bool)
    m[:, 0, 4:8] = True
    return m


MASKS = {"one per segment": _one_per_segment, "one to four per segment": _one_to_four,
         "empty": lambda d: np.zeros(d.shape, dtype=bool), "one voxel": _one_voxel, "one lane with every plane": _one_lane,
         "all ones": lambda d: np.ones(d.shape, dtype=bool)}


def _cube(shape, seed=7):
    return synth.gaussian_line_cube(shape, seed + shape[0])


def _bytes(arr, seed=1):
    rng = np.random.default_rng(seed)
    return np.where(arr, rng.choice(np.array([1, 2, 128, 255], dtype=np.uint8), size=arr.shape), np.uint8(0)).astype(np.uint8)


def _spec(arr, flags=0, lo=0.0, hi=0.0):
    return ops.MaskSpec(flags | _lib.MASK_ARRAY, lo, hi, DeviceArray.from_numpy(_bytes(arr)))


def _axis(nz):
    v = synth.spectral_axis(nz)
    cen = v - v[0]
    return v, cen, cen[nz // 2]


def _maps(dcube, spec, want):
    nz = dcube.shape[0]
    v, cen, cref = _axis(nz)
    r = ops.moments(dcube, DeviceArray.from_numpy(cen - cref), dv=500.0, m1_add=cref + v[0], mask=spec, want=want)
    return {k: r[k].get() for k in want}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


# ---- through the C entries alone ------------------------------------------------------------------------------------------

class _Native:
    """the bits of a mask and, per launch plan, the list and the voxel list made through the C entries alone (no keep-or-refuse
    rule); the caller holds DM.dirty("random") open, so every array is allocated dirty"""

    def __init__(self, dcube, dmask, pred=ARRAY):
        self.dcube, self.shape = dcube, dcube.shape
        nz, ny, nx = self.shape
        self.spec = ops.MaskSpec(pred[0] | _lib.MASK_ARRAY, pred[1], pred[2], dmask)
        self.c, self.m = ops._cube_c(dcube, np.dtype(np.float32)), self.spec.to_c()
        self.need = int(_lib.load().spc_mask_bits_bytes(nz, ny, nx))
        v, cen, cref = _axis(nz)
        self.m1_add = float(cref + v[0])
        self.ws = DeviceArray((max(int(_lib.load().spc_moments_workspace_bytes(nz, ny, nx)), 1),), np.uint8)
        self.bits = DeviceArray((self.need,), np.uint8)
        self.d_cen = DeviceArray.from_numpy(cen - cref)
        _lib.call("spc_mask_pack_bits", 0, None, nz, ny, nx, C.byref(self.m), C.c_void_p(self.bits.ptr), self.need)
        self.plans = {}

    def lists(self, o):
        """(list, voxel list) for the plan of a launch with outputs *o*"""
        desc = _lib.SpcMomentsListDesc()
        wsp = C.c_void_p(self.ws.ptr)
        _lib.call("spc_moments_list_plan_f32", C.byref(self.c), C.byref(self.m), C.byref(o), wsp, self.ws.nbytes, C.byref(desc))
        key = bytes(desc)
        if key in self.plans:
            return self.plans[key]
        n = int(desc.nblocks * desc.nsub)
        d_len, d_lines, d_vlen = (DeviceArray((n,), np.uint32) for _ in range(3))
        _lib.call("spc_moments_list_count_f32", 0, None, C.byref(self.c), C.byref(self.m), C.byref(o), wsp, self.ws.nbytes,
                  C.c_void_p(self.bits.ptr), self.need, C.c_void_p(d_len.ptr), C.c_void_p(d_lines.ptr), n, C.byref(desc))
        length = d_len.get().astype(np.uint64)
        rows = int(length.sum())
        off = DeviceArray.from_numpy(np.cumsum(length) - length)
        samples, meta = DeviceArray((max(rows, 1) * 1024,), np.uint8), DeviceArray((max(rows, 1) * 256,), np.uint8)
        lst = ops._MomentsList(desc, off, d_len, samples, meta, rows)
        _lib.call("spc_moments_list_fill_f32", 0, None, C.byref(self.c), C.c_void_p(self.bits.ptr), self.need, C.byref(lst.c))
        _lib.call("spc_moments_vlist_count_f32", 0, None, C.byref(lst.c), C.c_void_p(d_vlen.ptr), n)
        vlen = d_vlen.get().astype(np.uint64)
        vrows = int(vlen.sum())
        voff = DeviceArray.from_numpy(np.cumsum(vlen) - vlen)
        entries = DeviceArray((max(vrows, 1) * 512,), np.uint8)
        vl = ops._MomentsVlist(desc, voff, d_vlen, entries, vrows)
        _lib.call("spc_moments_vlist_fill_f32", 0, None, C.byref(lst.c), C.byref(vl.c))
        self.plans[key] = lst, vl
        return lst, vl

    def device_vlist(self, vl):
        d = vl.desc
        return dict(vlen=vl.len.get().reshape(d.nblocks, d.nsub), voff=vl.off.get().reshape(d.nblocks, d.nsub), vrows=vl.rows,
                    entries=vl.entries.get()[:vl.rows * 512].view(np.uint32).reshape(vl.rows, 64, 2))

    def launch(self, want, zero_entries=False):
        """the maps of spc_moments_vlist_f32 for *want*, and the voxel list it read"""
        ny, nx = self.shape[1:]
        o, bufs = ops._moment_outputs((ny, nx), 0, want)
        lst, vl = self.lists(o)
        if zero_entries:
            _lib.call("spc_memset", 0, C.c_void_p(vl.entries.ptr), 0, vl.entries.nbytes, None)
        _lib.call("spc_moments_vlist_f32", 0, None, C.byref(self.c), C.byref(self.m), C.c_void_p(self.d_cen.ptr), 500.0, self.m1_add,
                  C.byref(o), C.c_void_p(self.ws.ptr), self.ws.nbytes, C.c_void_p(self.bits.ptr), self.need, C.byref(lst.c), C.byref(vl.c))
        return {k: bufs[k].get() for k in want}, lst, vl


def _assert_is_the_layout(got, want):
    assert got["vrows"] == want["vrows"]
    assert np.array_equal(got["vlen"], want["vlen"]) and np.array_equal(got["voff"], want["voff"])
    assert np.array_equal(got["entries"], want["entries"]), np.argwhere(got["entries"] != want["entries"])[:4]


@pytest.mark.parametrize("mask_kind", sorted(MASKS))
@pytest.mark.parametrize("shape, env, _why", SHAPES, ids=_ids)
def test_voxel_list_is_the_layout_and_the_maps_are_the_march(gpu, monkeypatch, shape, env, _why, mask_kind):
    """per shape and mask, kept by the rule or not: vlen, voff and every entry byte against the numpy restatement for each plan
    the three forms launch, and the maps of the launch that reads the voxel list against a fresh spec's byte march, for
    SUMS, COUNT and EXTREMA and both predicate forms; zeroed entries then turn m0 all NaN"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.delenv(VLIST, raising=False)
    d = _cube(shape)
    arr = MASKS[mask_kind](d)
    dcube, dmask = DeviceArray.from_numpy(d), DeviceArray.from_numpy(_bytes(arr))
    with DM.dirty("random"):
        _layout_and_maps(shape, env, mask_kind, d, arr, dcube, dmask)


def _layout_and_maps(shape, env, mask_kind, d, arr, dcube, dmask):
    checked = set()
    for pred in (ARRAY, THRESHOLDS):
        nat = _Native(dcube, dmask, pred)
        for name, want in WANTS.items():
            maps, lst, vl = nat.launch(want)
            desc = vl.desc
            if not env:
                assert desc.zw == {37: 4, 9: 1, 520: 4 if want is EXTREMA else 8, 300: 4, 66000: 4 if want is EXTREMA else 8}[shape[0]]
                assert (desc.nsplit > 1) == (shape[0] >= 256)
            else:
                assert desc.nsplit == 3
            if bytes(desc) not in checked:
                checked.add(bytes(desc))
                want_list = L.build(d, arr, desc.zw, desc.nsplit, desc.zchunk)
                want_vl = V.build(want_list)
                _assert_is_the_layout(nat.device_vlist(vl), want_vl)
                assert want_list["rows"] <= want_vl["vrows"] <= 4 * want_list["rows"]
                if mask_kind == "empty":
                    assert want_vl["vrows"] == 0 and not want_vl["vlen"].any()
                if mask_kind == "one per segment":
                    assert want_vl["vrows"] == want_list["rows"] and V.keep(want_vl["vrows"], want_list["rows"])
                if mask_kind in ("all ones", "one lane with every plane"):
                    assert want_vl["vrows"] == 4 * want_list["rows"] and not V.keep(want_vl["vrows"], want_list["rows"])
                if mask_kind == "one to four per segment":
                    assert len(set(np.count_nonzero(want_vl["entries"][:, l, 1]) for l in range(8))) > 1, "lanes of unequal length"
            fresh = _maps(dcube, ops.MaskSpec(pred[0] | _lib.MASK_ARRAY, pred[1], pred[2], dmask), want)
            _same(maps, fresh, "%s, %s: the launch that reads the voxel list" % (name, "thresholds" if pred[0] else "array"))
        # the same launch once the entries are zeroed: every entry is then padding, so a launch that did not read the voxel
        # list (the list form, the bits march) would show here
        if mask_kind != "empty":
            assert not np.isnan(nat.launch(SUMS)[0]["m0"]).all()
        assert np.isnan(nat.launch(SUMS, zero_entries=True)[0]["m0"]).all(), "the launch did not read the voxel list"


@pytest.mark.parametrize("under", ["excluded", "included"])
def test_nan_and_inf_in_included_lane_segments(gpu, under):
    """NaN, +Inf and -Inf under voxels the mask excludes inside a lane segment it includes (they travel in the list and never
    enter the voxel list), and under voxels it includes (they reach the sums as they do in the march)"""
    shape = (37, 6, 40)
    d = _cube(shape).copy()
    arr = _one_to_four(d)
    seg = arr.reshape(shape[0], -1, 4).any(axis=2, keepdims=True).repeat(4, axis=2).reshape(shape)
    where = (seg & ~arr) if under == "excluded" else arr
    idx = np.flatnonzero(where)
    pick = np.random.default_rng(3).choice(idx, size=max(3, idx.size // 5), replace=False)
    d.reshape(-1)[pick] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), pick.size)
    dcube, dmask = DeviceArray.from_numpy(d), DeviceArray.from_numpy(_bytes(arr))
    with DM.dirty("random"):
        _nan_and_inf(under, d, arr, pick, dcube, dmask)


def _nan_and_inf(under, d, arr, pick, dcube, dmask):
    nat = _Native(dcube, dmask)
    for want in (COUNT, EXTREMA):
        maps, lst, vl = nat.launch(want)
        got = nat.device_vlist(vl)
        _assert_is_the_layout(got, V.build(L.build(d, arr, vl.desc.zw, vl.desc.nsplit, vl.desc.zchunk)))
        real = (got["entries"][:, :, 1] >> 30) & 1 != 0
        values = got["entries"][:, :, 0].copy().view(np.float32)[real]
        listed = lst.samples.get()[:lst.rows * 1024].view(np.float32)
        assert not np.isfinite(listed).all(), "the list carries them either way"
        # the entries are the included voxels' samples and nothing else, whatever lies beside them
        assert np.array_equal(np.sort(values.view(np.uint32)), np.sort(d[arr].view(np.uint32)))
        if under == "excluded":
            assert np.isfinite(values).all(), "a sample of an excluded voxel entered the voxel list"
        else:
            assert np.count_nonzero(~np.isfinite(values)) == pick.size
        _same(maps, _maps(dcube, ops.MaskSpec(_lib.MASK_ARRAY, array=dmask), want), under)


@pytest.mark.parametrize("rows_in_flight", ["8", "16"])
def test_both_batch_sizes(gpu, monkeypatch, rows_in_flight):
    """SPC_MOMENTS_VLIST_U: without a z split every sublist holds 33 rows here (66 with extrema: four waves), so two batches of
    16 and the tail of either form run"""
    monkeypatch.setenv("SPC_MOMENTS_VLIST_U", rows_in_flight)
    monkeypatch.setenv("SPC_MOMENTS_NSPLIT", "1")
    shape = (2100, 4, 64)
    d = _cube(shape)
    arr = _one_per_segment(d)
    dcube, dmask = DeviceArray.from_numpy(d), DeviceArray.from_numpy(_bytes(arr))
    with DM.dirty("random"):
        _batches(rows_in_flight, d, arr, dcube, dmask)


def _batches(rows_in_flight, d, arr, dcube, dmask):
    nat = _Native(dcube, dmask)
    for want in (SUMS, EXTREMA):
        maps, lst, vl = nat.launch(want)
        assert (vl.desc.zw, vl.desc.nsplit) == ((4, 1) if want is EXTREMA else (8, 1))
        want_vl = V.build(L.build(d, arr, vl.desc.zw, 1, vl.desc.zchunk))
        vlen = want_vl["vlen"]
        assert (vlen >= 2 * 16).all() and (vlen % 16 != 0).all() and (vlen % 8 != 0).all(), "two batches and a remainder"
        _assert_is_the_layout(nat.device_vlist(vl), want_vl)
        _same(maps, _maps(dcube, ops.MaskSpec(_lib.MASK_ARRAY, array=dmask), want), "U = " + rows_in_flight)


# ---- through ops --------------------------------------------------------------------------------------------------------------

def _device_vlist(spec):
    vl = spec._vlist
    d = vl.desc
    return dict(vlen=vl.len.get().reshape(d.nblocks, d.nsub), voff=vl.off.get().reshape(d.nblocks, d.nsub), vrows=vl.rows,
                entries=vl.entries.get()[:vl.rows * 512].view(np.uint32).reshape(vl.rows, 64, 2))


def _six(monkeypatch, dcube, spec, want, kept=True):
    """calls 1 .. 6 through one spec, then the voxel list, the list and the mask-first march switched off: all bit-identical;
    the list appears with the third call, the voxel list with the fourth and not before"""
    for name in (VLIST, LIST, FIRST):
        monkeypatch.delenv(name, raising=False)
    calls, lst = [], None
    for n in range(6):
        calls.append(_maps(dcube, spec, want))
        assert (spec._list is not None) == (n >= 2), "after call %d" % (n + 1)
        lst = spec._list if n == 2 else lst
        assert spec._list is lst, "the list stays the same object"
        assert (spec._vlist is not None) == (kept and n >= 3), "after call %d" % (n + 1)
        assert spec._vlist_failed == (not kept and n >= 3), "after call %d" % (n + 1)
    others = {}
    for name in (VLIST, LIST, FIRST):
        monkeypatch.setenv(name, "0")
        others[name + "=0"] = _maps(dcube, spec, want)
        monkeypatch.delenv(name)
    for n in range(1, 6):
        _same(calls[n], calls[0], "call %d against the first" % (n + 1))
    for what, maps in others.items():
        _same(maps, calls[0], what)
    return calls[0]


def _restated(spec, d, arr):
    desc = spec._list.desc
    lst = L.build(d, arr, desc.zw, desc.nsplit, desc.zchunk)
    assert L.keep(lst["rows"], lst["lines"], desc.nblocks, d.shape[0]), "the list is kept by its rule"
    return lst, V.build(lst)


@pytest.mark.parametrize("pred", [ARRAY, THRESHOLDS], ids=["array", "array+thresholds"])
@pytest.mark.parametrize("want", [SUMS, COUNT, EXTREMA], ids=["sums", "count", "extrema"])
@pytest.mark.parametrize("shape", [(37, 6, 40), (520, 4, 64)], ids=["37x6x40", "520x4x64"])
def test_six_calls_are_bit_identical_and_both_tiers_are_kept(gpu, monkeypatch, shape, want, pred):
    d = _cube(shape)
    arr = _one_per_segment(d)
    spec = _spec(arr, *pred)
    first = _six(monkeypatch, DeviceArray.from_numpy(d), spec, want)
    lst, vl = _restated(spec, d, arr)
    assert V.keep(vl["vrows"], lst["rows"])
    _assert_is_the_layout(_device_vlist(spec), vl)
    assert bytes(spec._vlist.desc) == bytes(spec._list.desc)
    if "nvalid" in want and not pred[0]:
        assert np.array_equal(first["nvalid"], (arr & ~np.isnan(d)).sum(axis=0))


@pytest.mark.parametrize("shape", [(37, 6, 40), (520, 4, 64)], ids=["37x6x40", "520x4x64"])
def test_three_voxels_of_a_segment_are_refused_and_stay_on_the_list(gpu, monkeypatch, shape):
    d = _cube(shape)
    arr = _diagonal(d)
    dcube, spec = DeviceArray.from_numpy(d), _spec(arr)
    _six(monkeypatch, dcube, spec, COUNT, kept=False)
    lst, vl = _restated(spec, d, arr)
    assert not V.keep(vl["vrows"], lst["rows"]) and vl["vrows"] == 3 * lst["rows"]
    assert spec._vlist is None and spec._vlist_failed
    rows = spec._list.rows
    assert rows == lst["rows"]
    assert np.array_equal(spec._list.samples.get()[:rows * 1024].view(np.uint32), lst["samples"].view(np.uint32).reshape(-1))
    assert np.array_equal(spec._list.meta.get()[:rows * 256].view(np.uint32), lst["meta"].reshape(-1))
    # a later call does not count again
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    _maps(dcube, spec, COUNT)
    assert "spc_moments_vlist_count_f32" not in seen and "spc_moments_list_f32" in seen


def test_row_view(gpu, monkeypatch):
    """rows 3 .. 10 of a taller cube with the rows() spec of its mask"""
    shape = (77, 14, 52)
    d = _cube(shape)
    sub = np.ascontiguousarray(d[:, 3:11])
    arr = _one_per_segment(sub)                                  # the lane groups of the VIEW
    full = np.zeros(shape, dtype=bool)
    full[:, 3:11] = arr
    dmask = DeviceArray.from_numpy(_bytes(full))
    view = ops.MaskSpec(_lib.MASK_ARRAY, array=dmask).rows(3, 11)
    first = _six(monkeypatch, DeviceArray.from_numpy(d).rows(3, 11), view, COUNT)
    lst, vl = _restated(view, sub, arr)
    assert V.keep(vl["vrows"], lst["rows"])
    _assert_is_the_layout(_device_vlist(view), vl)
    _same(_maps(DeviceArray.from_numpy(sub), _spec(arr), COUNT), first, "contiguous copy")


def test_a_launch_with_another_plan_reads_the_bits_and_keeps_both_lists(gpu):
    """built by sums launches at (520, 4, 64), ZW = 8; argmax on the same spec launches ZW = 4"""
    shape = (520, 4, 64)
    d = _cube(shape)
    arr = _one_per_segment(d)
    dcube, spec = DeviceArray.from_numpy(d), _spec(arr)
    for _ in range(4):
        sums = _maps(dcube, spec, SUMS)
    lst, vl = spec._list, spec._vlist
    assert lst is not None and vl is not None and vl.desc.zw == 8
    ext = _maps(dcube, spec, EXTREMA)
    assert spec._list is lst and spec._vlist is vl
    _same(ext, _maps(dcube, _spec(arr), EXTREMA), "extrema through lists made for another plan")
    _same(_maps(dcube, spec, SUMS), sums, "the next sums call")
    assert spec._list is lst and spec._vlist is vl


def test_upload_into_the_cube_drops_both_lists(gpu):
    shape = (37, 6, 40)
    d, other = _cube(shape), _cube(shape, seed=99)
    arr = _one_per_segment(d)
    dcube, spec = DeviceArray.from_numpy(d), _spec(arr)
    for _ in range(4):
        _maps(dcube, spec, COUNT)
    assert spec._vlist is not None
    dcube.upload(other)
    fresh = _maps(DeviceArray.from_numpy(other), _spec(arr), COUNT)
    _same(_maps(dcube, spec, COUNT), fresh, "first call after upload()")
    assert spec._list is None and spec._vlist is None and spec._bits is not None
    for call in range(3):
        _same(_maps(dcube, spec, COUNT), fresh, "call %d after upload()" % (call + 2))
    assert spec._vlist is not None
