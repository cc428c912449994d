"""GPU: a cube reduced again under the same mask is read as a list of the lane segments the mask includes
(spc_moments_list_* / ops.MaskSpec): the device-built list is the layout of include/spcube_hip.h byte for byte, padding
included; the maps of the list form are those of the bits march and of the byte loop bit for bit; the list is built on a
spec's third use of one cube and not before, refused where it would not halve the bytes, and dropped when the cube, its
samples or the mask change.

Shapes: the smallest that reach each path of the loader (see SHAPES).  Mask bytes are drawn from {1, 2, 128, 255}."""
import ctypes as C
import gc

import numpy as np
import pytest

import dirty_memory as DM
import moments_list_layout as L
from spectral_cube_amd import _lib, ops, synth
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

LIST, FIRST = "SPC_MOMENTS_LIST", "SPC_MOMENTS_MASK_FIRST"
SUMS, COUNT = ("m0", "m1", "m2"), ("m0", "m1", "m2", "nvalid")
EXTREMA = ("m0", "m1", "m2", "nvalid", "argmax", "argmin", "vmax", "vmin")
THRESHOLDS = (_lib.MASK_FINITE | _lib.MASK_GT | _lib.MASK_LE, -0.25, 3.0)

# shape, switches, what it reaches
SHAPES = [((37, 6, 40), {}, "ZW = 4, a tail shorter than a batch, dead lanes (60 lane groups)"),
          ((9, 4, 16), {}, "ZW = 1"),
          ((520, 4, 64), {}, "ZW = 8: sublists of 65 planes over eight waves"),
          ((300, 4, 64), {}, "nsplit > 1"),
          ((37, 6, 40), {"SPC_MOMENTS_NSPLIT": "3"}, "a forced split"),
          ((66000, 2, 8), {}, "more than 65535 planes")]
_ids = [("x".join(map(str, s)) + ("," + ",".join("%s=%s" % (k[12:], v) for k, v in e.items()) if e else "")) for s, e, _ in SHAPES]


def _bench(d):
    return synth.boolean_mask(d, 5).astype(bool)


def _one_voxel(d):
    m = np.zeros(d.shape, dtype=bool)
    m[d.shape[0] // 2, -1, -1] = True
    return m


def _one_lane(d):
    """lane group 1 holds every plane, all other lanes nothing: maximal padding"""
    m = np.zeros(d.shape, dtype=bool)
    m[:, 0, 4:8] = True
    return m


def _diagonal(d):
    """lane group g includes the planes z with (z // 8 + g) % 8 == 0, three of its four voxels: every 128-byte line of every
    plane holds one included lane segment, and the lanes of a block hold equally many - the bits march fetches every line for
    an eighth of its samples, so the list is KEPT at every shape here (most masks are refused at these sizes: with one or
    two blocks a row of 64 lanes is rarely worth its 1280 bytes)"""
    nz, ny, nx = d.shape
    g = np.arange(ny * (nx // 4)).reshape(1, ny, nx // 4, 1)
    z = np.arange(nz).reshape(nz, 1, 1, 1)
    return (((z // 8 + g) % 8 == 0) & (np.arange(4).reshape(1, 1, 1, 4) != g % 4)).reshape(d.shape)


MASKS = {"bench mask": _bench, "diagonal": _diagonal, "empty": lambda d: np.zeros(d.shape, dtype=bool), "one voxel": _one_voxel,
         "one lane with every plane": _one_lane}


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


def _four(monkeypatch, dcube, spec, want, builds=True):
    """calls 1 .. 4 through one spec, then the list switched off and the mask-first march switched off: all bit-identical;
    the list appears with the third call and not before"""
    monkeypatch.delenv(LIST, raising=False)
    calls = []
    for n in range(4):
        calls.append(_maps(dcube, spec, want))
        assert (spec._list is not None) == (builds and n >= 2), "after call %d" % (n + 1)
    monkeypatch.setenv(LIST, "0")
    no_list = _maps(dcube, spec, want)
    monkeypatch.delenv(LIST)
    monkeypatch.setenv(FIRST, "0")
    loop = _maps(dcube, spec, want)
    monkeypatch.delenv(FIRST)
    for n in range(1, 4):
        _same(calls[n], calls[0], "call %d against the first" % (n + 1))
    _same(no_list, calls[0], LIST + "=0")
    _same(loop, calls[0], FIRST + "=0")
    return calls[0]


def _device_list(spec):
    lst = spec._list
    n = int(lst.desc.nblocks * lst.desc.nsub)
    rows = lst.rows
    return dict(len=lst.len.get()[:n].reshape(lst.desc.nblocks, lst.desc.nsub), off=lst.off.get()[:n].reshape(lst.desc.nblocks, lst.desc.nsub),
                samples=lst.samples.get()[:rows * 1024].view(np.float32).reshape(rows, 64, 4),
                meta=lst.meta.get()[:rows * 256].view(np.uint32).reshape(rows, 64), rows=rows)


def _assert_list_is_the_layout(spec, d, arr):
    desc = spec._list.desc
    want = L.build(d, arr, desc.zw, desc.nsplit, desc.zchunk)
    got = _device_list(spec)
    assert got["rows"] == want["rows"]
    assert np.array_equal(got["len"], want["len"]) and np.array_equal(got["off"], want["off"])
    assert np.array_equal(got["meta"], want["meta"]), np.argwhere(got["meta"] != want["meta"])[:4]
    assert np.array_equal(got["samples"].view(np.uint32), want["samples"].view(np.uint32))
    return want


# ---- the list, byte for byte, and the maps ------------------------------------------------------------------------------

def _native_list(dcube, dmask, want=SUMS):
    """count, fill and launch through the C entries alone (no keep-or-refuse rule), every array allocated dirty: the desc, the
    device's len, lines, off, samples and meta on the host, and the maps of the launch that reads them"""
    nz, ny, nx = dcube.shape
    spec = ops.MaskSpec(_lib.MASK_ARRAY, array=dmask)
    c, m = ops._cube_c(dcube, np.dtype(np.float32)), spec.to_c()
    ws = DeviceArray((max(int(_lib.load().spc_moments_workspace_bytes(nz, ny, nx)), 1),), np.uint8)
    need = int(_lib.load().spc_mask_bits_bytes(nz, ny, nx))
    bits = DeviceArray((need,), np.uint8)
    _lib.call("spc_mask_pack_bits", 0, None, nz, ny, nx, C.byref(m), C.c_void_p(bits.ptr), need)
    v, cen, cref = _axis(nz)
    d_cen = DeviceArray.from_numpy(cen - cref)
    with DM.dirty("random"):
        o, bufs = ops._moment_outputs((ny, nx), 0, want)
        desc, counted = _lib.SpcMomentsListDesc(), _lib.SpcMomentsListDesc()
        _lib.call("spc_moments_list_plan_f32", C.byref(c), C.byref(m), C.byref(o), C.c_void_p(ws.ptr), ws.nbytes, C.byref(desc))
        n = int(desc.nblocks * desc.nsub)
        d_len, d_lines = DeviceArray((n,), np.uint32), DeviceArray((n,), np.uint32)
        _lib.call("spc_moments_list_count_f32", 0, None, C.byref(c), C.byref(m), C.byref(o), C.c_void_p(ws.ptr), ws.nbytes,
                  C.c_void_p(bits.ptr), need, C.c_void_p(d_len.ptr), C.c_void_p(d_lines.ptr), n, C.byref(counted))
        assert bytes(counted) == bytes(desc)
        length = d_len.get().astype(np.uint64)
        rows = int(length.sum())
        off = DeviceArray.from_numpy(np.cumsum(length) - length)
        samples, meta = DeviceArray((max(rows, 1) * 1024,), np.uint8), DeviceArray((max(rows, 1) * 256,), np.uint8)
        lst = ops._MomentsList(desc, off, d_len, samples, meta, rows)
        _lib.call("spc_moments_list_fill_f32", 0, None, C.byref(c), C.c_void_p(bits.ptr), need, C.byref(lst.c))
        got = dict(desc=desc, rows=rows, len=d_len.get().reshape(desc.nblocks, desc.nsub), lines=int(d_lines.get().astype(np.uint64).sum()),
                   off=off.get().reshape(desc.nblocks, desc.nsub), samples=samples.get()[:rows * 1024].view(np.float32).reshape(rows, 64, 4),
                   meta=meta.get()[:rows * 256].view(np.uint32).reshape(rows, 64))

        def launch():
            _lib.call("spc_moments_list_f32", 0, None, C.byref(c), C.byref(m), C.c_void_p(d_cen.ptr), 500.0, float(cref + v[0]),
                      C.byref(o), C.c_void_p(ws.ptr), ws.nbytes, C.c_void_p(bits.ptr), need, C.byref(lst.c))
            return {k: bufs[k].get() for k in want}
        got["maps"] = launch()
        # the same launch once the metas are zeroed: every entry is then an excluded plane, so a launch that did not read the
        # list (the bits march) would show here
        _lib.call("spc_memset", 0, C.c_void_p(meta.ptr), 0, meta.nbytes, None)
        assert np.isnan(launch()["m0"]).all(), "the launch did not read the list"
    return got


@pytest.mark.parametrize("mask_kind", sorted(MASKS) + ["all ones"])
@pytest.mark.parametrize("shape, env, _why", SHAPES, ids=_ids)
def test_list_is_the_layout_and_the_maps_are_the_march(gpu, monkeypatch, shape, env, _why, mask_kind):
    """the C entries on every shape and mask, kept by the rule or not: the list's bytes against the numpy restatement, the maps
    of the launch that reads it against the byte march; then ops on the same inputs: kept or refused as the rule says on the
    third call, the maps the march's either way"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = _cube(shape)
    arr = np.ones(shape, dtype=bool) if mask_kind == "all ones" else MASKS[mask_kind](d)
    dcube, spec = DeviceArray.from_numpy(d), _spec(arr)
    fresh = _maps(dcube, _spec(arr), COUNT)                    # a first call: the byte march
    got = _native_list(dcube, spec.array, COUNT)
    desc = got["desc"]
    if not env:
        assert desc.zw == {37: 4, 9: 1, 520: 8, 300: 4, 66000: 8}[shape[0]]
        assert (desc.nsplit > 1) == (shape[0] >= 256)
    else:
        assert desc.nsplit == 3
    want = L.build(d, arr, desc.zw, desc.nsplit, desc.zchunk)
    assert got["rows"] == want["rows"] and got["lines"] == want["lines"]
    assert np.array_equal(got["len"], want["len"]) and np.array_equal(got["off"], want["off"])
    assert np.array_equal(got["meta"], want["meta"]), np.argwhere(got["meta"] != want["meta"])[:4]
    assert np.array_equal(got["samples"].view(np.uint32), want["samples"].view(np.uint32))
    if mask_kind == "empty":
        assert want["rows"] == 0 and not want["len"].any()
    _same(got["maps"], fresh, "the launch that reads the list")
    kept = L.keep(want["rows"], want["lines"], desc.nblocks, shape[0])
    if mask_kind in ("all ones", "one lane with every plane"):
        assert not kept
    if mask_kind == "empty" or (mask_kind == "diagonal" and not env and shape[0] in (37, 300, 520)):
        assert kept                                            # (9 and 66000 channels: 16 and 4 lane groups, never worth a row)
    for call in range(4):
        _same(_maps(dcube, spec, COUNT), fresh, "call %d" % (call + 1))
        assert (spec._list is not None) == (kept and call >= 2) and spec._list_failed == (not kept and call >= 2)
    if kept:
        _assert_list_is_the_layout(spec, d, arr)


@pytest.mark.parametrize("want", [SUMS, EXTREMA], ids=["sums", "extrema"])
@pytest.mark.parametrize("mask_kind", ["bench mask", "diagonal"])
def test_the_other_forms_read_the_list(gpu, mask_kind, want):
    """the sums form (any-valid bit) and the extrema form (its own plan: ZW = 4 at 520 channels) through the C entries"""
    shape = (520, 4, 64)
    d = _cube(shape)
    arr = MASKS[mask_kind](d)
    dcube, spec = DeviceArray.from_numpy(d), _spec(arr)
    got = _native_list(dcube, spec.array, want)
    assert got["desc"].zw == (4 if want is EXTREMA else 8)
    _same(got["maps"], _maps(dcube, _spec(arr), want), "the launch that reads the list")


@pytest.mark.parametrize("flags, lo, hi", [(0, 0.0, 0.0), THRESHOLDS], ids=["array", "array+thresholds"])
@pytest.mark.parametrize("want", [SUMS, COUNT, EXTREMA], ids=["sums", "count", "extrema"])
@pytest.mark.parametrize("shape", [(37, 6, 40), (520, 4, 64)], ids=["37x6x40", "520x4x64"])
def test_four_calls_are_bit_identical(gpu, monkeypatch, shape, want, flags, lo, hi):
    d = _cube(shape)
    arr = _diagonal(d)
    first = _four(monkeypatch, DeviceArray.from_numpy(d), _spec(arr, flags, lo, hi), want)
    if "nvalid" in want and not flags:
        assert np.array_equal(first["nvalid"], (arr & ~np.isnan(d)).sum(axis=0))


@pytest.mark.parametrize("rows_in_flight", ["4", "8"])
def test_both_batch_sizes(gpu, monkeypatch, rows_in_flight):
    """SPC_MOMENTS_LIST_U: without a z split a sublist holds 20 rows here (10 with extrema), so the batches and the tail of
    either form run"""
    monkeypatch.setenv("SPC_MOMENTS_LIST_U", rows_in_flight)
    monkeypatch.setenv("SPC_MOMENTS_NSPLIT", "1")
    shape = (640, 24, 136)
    d = _cube(shape)
    for want in (SUMS, EXTREMA):
        _four(monkeypatch, DeviceArray.from_numpy(d), _spec(_diagonal(d)), want)


@pytest.mark.parametrize("under", ["excluded", "included"])
def test_nan_and_inf_in_included_lane_segments(gpu, monkeypatch, under):
    """NaN, +Inf and -Inf under voxels the mask excludes inside a lane segment it includes (they travel in the list and must
    not reach a sum), and under voxels it includes (they must reach the sums as they do in the march)"""
    shape = (37, 6, 40)
    d = _cube(shape).copy()
    arr = _diagonal(d)
    seg = arr.reshape(shape[0], -1, 4).any(axis=2, keepdims=True).repeat(4, axis=2).reshape(shape)
    where = (seg & ~arr) if under == "excluded" else arr
    idx = np.flatnonzero(where)
    pick = np.random.default_rng(3).choice(idx, size=max(3, idx.size // 5), replace=False)
    d.reshape(-1)[pick] = np.resize(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), pick.size)
    for want in (COUNT, EXTREMA):
        _four(monkeypatch, DeviceArray.from_numpy(d), _spec(arr), want)


def test_row_view(gpu, monkeypatch):
    """rows 3 .. 10 of a taller cube with the rows() spec of its mask: the fill addresses the cube with the view's strides"""
    shape = (77, 14, 52)
    d = _cube(shape)
    arr = _diagonal(d)
    dmask = DeviceArray.from_numpy(_bytes(arr))
    view = ops.MaskSpec(_lib.MASK_ARRAY, array=dmask).rows(3, 11)
    dcube = DeviceArray.from_numpy(d).rows(3, 11)
    first = _four(monkeypatch, dcube, view, COUNT)
    _assert_list_is_the_layout(view, np.ascontiguousarray(d[:, 3:11]), np.ascontiguousarray(arr[:, 3:11]))
    _same(_maps(DeviceArray.from_numpy(np.ascontiguousarray(d[:, 3:11])), _spec(np.ascontiguousarray(arr[:, 3:11])), COUNT), first,
          "contiguous copy")


# ---- keep or refuse -----------------------------------------------------------------------------------------------------

def test_all_ones_is_refused(gpu, monkeypatch):
    shape = (37, 6, 40)
    d = _cube(shape)
    dcube, spec = DeviceArray.from_numpy(d), _spec(np.ones(shape, dtype=bool))
    first = _four(monkeypatch, dcube, spec, COUNT, builds=False)
    assert spec._list is None and spec._list_failed and first["nvalid"].all()
    # a later call does not count again
    seen = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (seen.append(name), real(name, *a))[1])
    _maps(dcube, spec, COUNT)
    assert "spc_moments_list_count_f32" not in seen and "spc_moments_bits_f32" in seen


# ---- plan mismatch ------------------------------------------------------------------------------------------------------

def test_a_launch_with_another_plan_reads_the_bits_and_keeps_the_list(gpu, monkeypatch):
    """built by a sums launch at (520, 4, 64), ZW = 8; argmax on the same spec launches ZW = 4"""
    shape = (520, 4, 64)
    d = _cube(shape)
    arr = _diagonal(d)
    dcube, spec = DeviceArray.from_numpy(d), _spec(arr)
    for _ in range(3):
        sums = _maps(dcube, spec, SUMS)
    lst = spec._list
    assert lst is not None and lst.desc.zw == 8
    ext = _maps(dcube, spec, EXTREMA)
    assert spec._list is lst
    _same(ext, _maps(dcube, _spec(arr), EXTREMA), "extrema through a list made for another plan")
    _same(_maps(dcube, spec, SUMS), sums, "the next sums call")
    assert spec._list is lst


# ---- staleness ----------------------------------------------------------------------------------------------------------

def _used(dcube, arr, n=3):
    spec = _spec(arr)
    for _ in range(n):
        _maps(dcube, spec, COUNT)
    assert spec._list is not None
    return spec


def _fresh_three_times(dcube, spec, fresh, what):
    for call in range(3):
        _same(_maps(dcube, spec, COUNT), fresh, "call %d after %s" % (call + 1, what))


def test_upload_into_the_cube_drops_the_list(gpu):
    shape = (37, 6, 40)
    d, other = _cube(shape), _cube(shape, seed=99)
    arr = _diagonal(d)
    dcube = DeviceArray.from_numpy(d)
    spec = _used(dcube, arr)
    dcube.upload(other)
    fresh = _maps(DeviceArray.from_numpy(other), _spec(arr), COUNT)
    _same(_maps(dcube, spec, COUNT), fresh, "first call after upload()")
    assert spec._list is None and spec._bits is not None       # only the list is dropped
    _fresh_three_times(dcube, spec, fresh, "upload()")
    assert spec._list is not None


def test_an_operator_writing_into_the_cube_drops_the_list(gpu):
    shape = (37, 6, 40)
    d, other = _cube(shape), _cube(shape, seed=99)
    arr = _diagonal(d)
    dcube = DeviceArray.from_numpy(d)
    spec = _used(dcube, arr)
    ops.fill_masked(DeviceArray.from_numpy(other), out=dcube)  # no mask: a copy of `other` into the cube
    fresh = _maps(DeviceArray.from_numpy(other), _spec(arr), COUNT)
    _fresh_three_times(dcube, spec, fresh, "fill_masked(out=cube)")


def test_a_second_cube_with_the_same_spec(gpu):
    shape = (37, 6, 40)
    d, other = _cube(shape), _cube(shape, seed=99)
    arr = _diagonal(d)
    dcube, dother = DeviceArray.from_numpy(d), DeviceArray.from_numpy(other)
    spec = _used(dcube, arr)
    fresh = _maps(dother, _spec(arr), COUNT)
    _same(_maps(dother, spec, COUNT), fresh, "the other cube")
    assert spec._list is None
    _same(_maps(dcube, spec, COUNT), _maps(dcube, _spec(arr), COUNT), "back to the first cube")
    _fresh_three_times(dother, spec, fresh, "changing cubes")


def test_a_freed_cube_whose_address_comes_back(gpu):
    shape = (37, 6, 40)
    d, other = _cube(shape), _cube(shape, seed=99)
    arr = _diagonal(d)
    dcube = DeviceArray.from_numpy(d)
    spec = _used(dcube, arr)
    ptr = dcube.ptr
    del dcube
    gc.collect()
    again = None
    for _ in range(8):
        cand = DeviceArray.from_numpy(other)
        if cand.ptr == ptr:
            again = cand
            break
        del cand
        gc.collect()
    if again is None:
        pytest.skip("the address did not come back")
    _same(_maps(again, spec, COUNT), _maps(again, _spec(arr), COUNT), "a new cube at the freed cube's address")


def test_invalidate_drops_the_list(gpu):
    shape = (37, 6, 40)
    d = _cube(shape)
    arr = _diagonal(d)
    dcube = DeviceArray.from_numpy(d)
    spec = _used(dcube, arr)
    other = _cube(shape, seed=99)
    _lib.call("spc_memcpy_h2d", 0, C.c_void_p(dcube.ptr), other.ctypes.data_as(C.c_void_p), other.nbytes, None)   # behind the library's back
    _same(_maps(dcube, spec, COUNT), _maps(DeviceArray.from_numpy(d), _spec(arr), COUNT), "the list made before the raw write")
    spec.invalidate()
    assert spec._list is None and spec._bits is None
    _fresh_three_times(dcube, spec, _maps(DeviceArray.from_numpy(other), _spec(arr), COUNT), "invalidate()")
