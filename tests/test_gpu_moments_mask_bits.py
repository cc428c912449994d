"""GPU: the moment kernel reads a reused uint8 mask array as bits (spc_mask_pack_bits / spc_moments_bits_f32, ops.MaskSpec):
the packed form is the layout of include/spcube_hip.h byte for byte, the maps of the bits form are those of the byte form
bit for bit, a spec packs on its second use and not before, and a rewritten array is packed again.

Shapes, launch forms, mask patterns and the poisoned cubes are those of tests/test_gpu_moments_mask_first.py (the smallest
that hit each path of the march); the mask bytes here are drawn from {1, 2, 128, 255} where the pattern includes a voxel:
non-zero, not 1, means included."""
import ctypes as C

import numpy as np
import pytest

import oracle_np as O
from conftest import assert_close
from mask_bits_layout import bits_bytes, pack_bits
from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray, Stream
from test_gpu_moments_mask_first import LAUNCHES, MASKS, SHAPES, _axis, _case

pytestmark = pytest.mark.gpu

BITS, FIRST = "SPC_MOMENTS_MASK_BITS", "SPC_MOMENTS_MASK_FIRST"
SUMS, COUNT = ("m0", "m1", "m2"), ("m0", "m1", "m2", "nvalid")
EXTREMA = ("m0", "m1", "m2", "nvalid", "argmax", "argmin", "vmax", "vmin")
_ids = dict(ids=lambda s: "x".join(map(str, s)))


def _bytes(arr, seed):
    """the boolean pattern *arr* as mask bytes: 0 where excluded, one of 1, 2, 128, 255 where included"""
    rng = np.random.default_rng(seed)
    return np.where(arr, rng.choice(np.array([1, 2, 128, 255], dtype=np.uint8), size=arr.shape), np.uint8(0)).astype(np.uint8)


def _spec(arr, flags=0, lo=0.0, hi=0.0, seed=1):
    return ops.MaskSpec(flags | _lib.MASK_ARRAY, lo, hi, DeviceArray.from_numpy(_bytes(arr, seed)))


def _maps(dcube, spec, want, stream=None):
    nz = dcube.shape[0]
    v, cen, cref = _axis(nz)
    r = ops.moments(dcube, DeviceArray.from_numpy(cen - cref), dv=500.0, m1_add=cref + v[0], mask=spec, want=want, stream=stream)
    return {k: r[k].get(stream) for k in want}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def _packed(dmask):
    """spc_mask_pack_bits of a (view of a) uint8 DeviceArray, on the host"""
    nz, ny, nx = dmask.shape
    need = int(_lib.load().spc_mask_bits_bytes(nz, ny, nx))
    assert need == bits_bytes(nz, ny, nx) > 0
    bits = DeviceArray.from_numpy(np.full(need, 0xA5, dtype=np.uint8))       # every byte must be written
    m = ops.MaskSpec(_lib.MASK_ARRAY, array=dmask).to_c()
    _lib.call("spc_mask_pack_bits", 0, None, nz, ny, nx, C.byref(m), C.c_void_p(bits.ptr), need)
    return bits.get()


# ---- the packed form ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mask_kind", sorted(MASKS))
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[2] % 4 == 0], **_ids)
def test_pack_is_the_layout_byte_for_byte(gpu, shape, mask_kind):
    arr = _case(shape, mask_kind)[2]
    host = _bytes(arr, 5)
    got = _packed(DeviceArray.from_numpy(host))
    want = pack_bits(host)
    assert got.shape == want.shape and np.array_equal(got, want), np.flatnonzero(got != want)[:8]


def test_pack_of_a_row_view(gpu):
    """rows 3 .. 10 of a taller mask: the plane stride is not ny * nx"""
    arr = _case((77, 14, 52), "bench mask")[2]
    host = _bytes(arr, 6)
    got = _packed(DeviceArray.from_numpy(host).rows(3, 11))
    assert np.array_equal(got, pack_bits(host[:, 3:11]))


def test_no_packed_form_for_a_width_that_is_no_multiple_of_four(gpu):
    assert int(_lib.load().spc_mask_bits_bytes(530, 9, 50)) == 0
    d = DeviceArray.from_numpy(np.ones((4, 3, 50), dtype=np.uint8))
    m = ops.MaskSpec(_lib.MASK_ARRAY, array=d).to_c()
    bits = DeviceArray((64,), np.uint8)
    with pytest.raises(_lib.HipUnsupported):
        _lib.call("spc_mask_pack_bits", 0, None, 4, 3, 50, C.byref(m), C.c_void_p(bits.ptr), 64)


# ---- bit identity -----------------------------------------------------------------------------------------------------

def _four_ways(monkeypatch, dcube, arr, flags, lo, hi, want, packs):
    """the maps of a fresh spec's first call (bytes), second and third (bits where the form exists) and of the switch at 0,
    all equal; the spec holds bits after the second call, not after the first"""
    monkeypatch.delenv(BITS, raising=False)
    spec = _spec(arr, flags, lo, hi)
    first = _maps(dcube, spec, want)
    assert spec._bits is None and not spec._bits_failed
    second = _maps(dcube, spec, want)
    assert (spec._bits is not None) == packs and spec._bits_failed == (not packs)
    third = _maps(dcube, spec, want)
    monkeypatch.setenv(BITS, "0")
    off = _maps(dcube, spec, want)
    monkeypatch.delenv(BITS)
    _same(second, first, "second call (bits) against the first (bytes)")
    _same(third, first, "third call (bits) against the first (bytes)")
    _same(off, first, BITS + "=0 against the first call")
    return first


@pytest.mark.parametrize("mask_kind", sorted(MASKS))
@pytest.mark.parametrize("launch", LAUNCHES, ids=lambda s: ",".join("%s=%s" % (k[12:], v) for k, v in s.items()) or "default")
@pytest.mark.parametrize("shape", SHAPES, **_ids)
def test_bits_are_bit_identical_to_bytes(gpu, monkeypatch, shape, launch, mask_kind):
    for k, v in launch.items():
        monkeypatch.setenv(k, v)
    nz = shape[0]
    d, _zeroed, arr, flags, lo, hi = _case(shape, mask_kind)
    dcube = DeviceArray.from_numpy(d)
    packs = shape[2] % 4 == 0                                  # (530, 9, 50): 8-byte lanes, no packed form, nothing changes
    for want in (SUMS, COUNT):
        new = _four_ways(monkeypatch, dcube, arr, flags, lo, hi, want, packs)
    if mask_kind == "all zero":
        assert np.isnan(new["m0"]).all() and np.isnan(new["m1"]).all() and np.isnan(new["m2"]).all() and not new["nvalid"].any()
    if not launch:
        # the third call of a spec, against the oracle at the tolerances of test_mask_first_is_bit_identical
        inc = arr & ~np.isnan(d)
        if flags:
            inc &= np.isfinite(d) & (np.nan_to_num(d) > np.float32(lo)) & (np.nan_to_num(d) <= np.float32(hi))
        v, cen, _ = _axis(nz)
        e0, e1, e2 = O.moments012(d, inc, cen, 500.0, v[0])
        assert np.array_equal(new["nvalid"], inc.sum(axis=0))
        with np.errstate(all="ignore"):
            scale = np.nanmax(np.abs(e0)) if inc.any() else 1.0
            assert_close(new["m0"], e0, atol=1e-12 * scale, what="m0")
            assert_close(new["m1"], e1, atol=1e-9 * 500.0 * nz, what="m1")
            okm = np.isfinite(e2) & (np.abs(e0) > 1e-3 * scale)
            assert np.array_equal(np.isnan(new["m2"]), np.isnan(e2))
            assert np.all(np.abs(new["m2"][okm] - e2[okm]) <= 1e-8 * (500.0 * nz) ** 2)


@pytest.mark.parametrize("mask_kind", ["bench mask", "70 % random + isfinite + (lo, hi]"])
def test_bits_extrema_are_bit_identical(gpu, monkeypatch, mask_kind):
    """the extrema form (argmax, argmin, vmax, vmin beside the sums and the count), without and with the threshold terms
    (PRED = 0 / 1)"""
    shape = (77, 13, 52)
    d, _zeroed, arr, flags, lo, hi = _case(shape, mask_kind)
    new = _four_ways(monkeypatch, DeviceArray.from_numpy(d), arr, flags, lo, hi, EXTREMA, True)
    inc = arr & ~np.isnan(d)
    if flags:
        inc &= np.isfinite(d) & (np.nan_to_num(d) > np.float32(lo)) & (np.nan_to_num(d) <= np.float32(hi))
    assert np.array_equal(new["argmax"], O.argmax(d, inc)) and np.array_equal(new["argmin"], O.argmin(d, inc))


def test_bits_on_row_views(gpu, monkeypatch):
    """rows 3 .. 10 of a taller cube and mask: the view's spec packs the rows it shows"""
    shape = (77, 14, 52)
    d, _zeroed, arr, _flags, _lo, _hi = _case(shape, "bench mask")
    dmask = DeviceArray.from_numpy(_bytes(arr, 2))
    view = ops.MaskSpec(_lib.MASK_ARRAY, array=dmask).rows(3, 11)
    dcube = DeviceArray.from_numpy(d).rows(3, 11)
    first = _maps(dcube, view, COUNT)
    assert view._bits is None
    second = _maps(dcube, view, COUNT)
    assert view._bits is not None and view._bits.nbytes == bits_bytes(77, 8, 52)
    _same(second, first, "bits against bytes on a row view")
    contiguous = _spec(np.ascontiguousarray(arr[:, 3:11]))
    _same(_maps(DeviceArray.from_numpy(np.ascontiguousarray(d[:, 3:11])), contiguous, COUNT), first, "contiguous copy")


def test_the_third_call_reads_the_bits_not_the_bytes(gpu, monkeypatch):
    """the contract from the other side: bytes zeroed behind the library's back (a raw copy, no upload()) after the spec has
    packed are not seen - the launch reads the bits - until invalidate(); so a silent return to the byte kernels would fail here"""
    shape = (77, 13, 52)
    d, _zeroed, arr, _flags, _lo, _hi = _case(shape, "bench mask")
    dcube = DeviceArray.from_numpy(d)
    spec = _spec(arr)
    first = _maps(dcube, spec, COUNT)
    _maps(dcube, spec, COUNT)
    assert spec._bits is not None and first["nvalid"].any()
    zeros = np.zeros(shape, dtype=np.uint8)
    _lib.call("spc_memcpy_h2d", 0, C.c_void_p(spec.array.ptr), zeros.ctypes.data_as(C.c_void_p), zeros.nbytes, None)
    _same(_maps(dcube, spec, COUNT), first, "bits packed before the raw write")
    spec.invalidate()
    assert spec._bits is None
    assert not _maps(dcube, spec, COUNT)["nvalid"].any()


# ---- staleness --------------------------------------------------------------------------------------------------------

def _used_twice(dcube, arr):
    spec = _spec(arr)
    _maps(dcube, spec, COUNT)
    _maps(dcube, spec, COUNT)
    assert spec._bits is not None
    return spec


def _other_mask(shape):
    return np.random.default_rng(99).random(shape) < 0.2


def test_upload_of_another_mask_drops_the_bits(gpu):
    shape = (77, 13, 52)
    d, _zeroed, arr, _flags, _lo, _hi = _case(shape, "bench mask")
    dcube = DeviceArray.from_numpy(d)
    spec = _used_twice(dcube, arr)
    other = _other_mask(shape)
    spec.array.upload(_bytes(other, 3))
    fresh = _maps(dcube, _spec(other, seed=3), COUNT)
    _same(_maps(dcube, spec, COUNT), fresh, "first call after upload()")
    assert spec._bits is None                                  # the count starts again
    _same(_maps(dcube, spec, COUNT), fresh, "second call after upload()")
    assert spec._bits is not None
    _same(_maps(dcube, spec, COUNT), fresh, "third call after upload()")


def test_an_operator_writing_through_out_drops_the_bits(gpu):
    """ops.mask_morph(out=the spec's array): a dilation by the centre voxel alone copies its input"""
    shape = (77, 13, 52)
    d, _zeroed, arr, _flags, _lo, _hi = _case(shape, "bench mask")
    dcube = DeviceArray.from_numpy(d)
    spec = _used_twice(dcube, arr)
    other = _other_mask(shape)
    ops.mask_morph(DeviceArray.from_numpy(other.astype(np.uint8)), [[0, 0, 0]], _lib.MORPH_DILATE, out=spec.array)
    fresh = _maps(dcube, _spec(other), COUNT)
    for call in range(3):
        _same(_maps(dcube, spec, COUNT), fresh, "call %d after mask_morph(out=)" % (call + 1))
    assert spec._bits is not None


def test_invalidate_after_a_raw_write(gpu):
    shape = (77, 13, 52)
    d, _zeroed, arr, _flags, _lo, _hi = _case(shape, "bench mask")
    dcube = DeviceArray.from_numpy(d)
    spec = _used_twice(dcube, arr)
    other = _other_mask(shape)
    raw = _bytes(other, 4)
    _lib.call("spc_memcpy_h2d", 0, C.c_void_p(spec.array.ptr), raw.ctypes.data_as(C.c_void_p), raw.nbytes, None)
    spec.invalidate()
    fresh = _maps(dcube, _spec(other, seed=4), COUNT)
    for call in range(3):
        _same(_maps(dcube, spec, COUNT), fresh, "call %d after invalidate()" % (call + 1))
    assert spec._bits is not None


# ---- switches and fallback --------------------------------------------------------------------------------------------

def test_mask_first_off_with_bits_present_is_the_byte_loop(gpu, monkeypatch):
    shape = (77, 13, 52)
    d, _zeroed, arr, _flags, _lo, _hi = _case(shape, "bench mask")
    dcube = DeviceArray.from_numpy(d)
    monkeypatch.setenv(FIRST, "0")
    loop = _maps(dcube, _spec(arr), COUNT)                     # a first call: no bits anywhere
    monkeypatch.delenv(FIRST)
    spec = _used_twice(dcube, arr)
    monkeypatch.setenv(FIRST, "0")
    zeros = np.zeros(shape, dtype=np.uint8)
    _same(_maps(dcube, spec, COUNT), loop, FIRST + "=0 with bits present")
    # and it is the byte loop that ran: it sees bytes written behind the bits' back
    _lib.call("spc_memcpy_h2d", 0, C.c_void_p(spec.array.ptr), zeros.ctypes.data_as(C.c_void_p), zeros.nbytes, None)
    assert spec._bits is not None and not _maps(dcube, spec, COUNT)["nvalid"].any()


def test_a_spec_whose_allocation_failed_keeps_working(gpu):
    """what ops.moments leaves on a spec when the bits cannot be allocated (HipLibraryError / MemoryError): the mark alone,
    and the byte kernels from then on"""
    shape = (77, 13, 52)
    d, _zeroed, arr, _flags, _lo, _hi = _case(shape, "bench mask")
    dcube = DeviceArray.from_numpy(d)
    spec = _spec(arr)
    want = _maps(dcube, spec, COUNT)
    spec._bits_failed = True
    for call in range(3):
        _same(_maps(dcube, spec, COUNT), want, "call %d of a spec marked failed" % (call + 2))
        assert spec._bits is None and spec._bits_failed


# ---- a second stream --------------------------------------------------------------------------------------------------

def test_pack_on_one_stream_launch_on_another(gpu):
    shape = (640, 24, 136)
    d, _zeroed, arr, _flags, _lo, _hi = _case(shape, "bench mask")
    dcube = DeviceArray.from_numpy(d)
    a, b = Stream(0), Stream(0)
    spec = _spec(arr)
    first = _maps(dcube, spec, COUNT, stream=a)
    second = _maps(dcube, spec, COUNT, stream=a)               # packs on a
    assert spec._bits is not None
    _same(_maps(dcube, spec, COUNT, stream=b), first, "launch on the other stream")
    _same(second, first, "the packing call")
