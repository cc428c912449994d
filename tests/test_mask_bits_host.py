"""CPU: the packed form of a mask array - the numpy restatement of the layout (tests/mask_bits_layout.py) against a
hand-written two-block example, spc_mask_bits_bytes against it (the library loads without a device), and the host side of
ops.MaskSpec's slot for the bits: equality and printing unchanged, the write generation on the root of a view chain, the
switch read the way spc_switch reads it."""
import numpy as np
import pytest

from mask_bits_layout import bits_bytes, pack_bits
from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray


def test_layout_against_a_hand_written_two_block_example():
    """(2, 3, 96): 24 lane groups per row, 72 in all = block 0 (64 lanes) and block 1 (8 live lanes); plane z of block b at
    (b * 2 + z) * 32"""
    m = np.zeros((2, 3, 96), dtype=np.uint8)
    want = np.zeros(2 * 2 * 32, dtype=np.uint8)
    m[0, 0, 0] = 1          # g 0: block 0, lane 0, voxel 0 -> byte 0, low nibble, bit 0
    m[0, 0, 7] = 200        # g 1: block 0, lane 1, voxel 3 -> byte 0, high nibble, bit 3
    want[0] = 0x81
    m[0, 2, 60:64] = 1      # g 63: block 0, lane 63, all four -> byte 31, high nibble
    want[31] = 0xF0
    m[1, 1, 10] = 1         # g 26: block 0, lane 26, voxel 2 -> plane 1, byte 13, low nibble, bit 2
    want[32 + 13] = 0x04
    m[1, 2, 64] = 2         # g 64: block 1, lane 0, voxel 0 -> plane 1 of block 1, byte 0
    want[(1 * 2 + 1) * 32 + 0] = 0x01
    m[1, 2, 95] = 255       # g 71: block 1, lane 7, voxel 3 -> plane 1 of block 1, byte 3, high nibble, bit 3
    want[(1 * 2 + 1) * 32 + 3] = 0x80
    got = pack_bits(m)
    assert got.dtype == np.uint8 and got.shape == (bits_bytes(2, 3, 96),) == (128,)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    # lanes 8 .. 63 of block 1 do not exist: their nibbles stay zero whatever the mask holds
    full = pack_bits(np.full((2, 3, 96), 7, dtype=np.uint8))
    assert (full.reshape(2, 2, 32)[0] == 0xFF).all()
    assert (full.reshape(2, 2, 32)[1, :, :4] == 0xFF).all() and not full.reshape(2, 2, 32)[1, :, 4:].any()


def test_a_view_packs_the_rows_it_shows():
    rng = np.random.default_rng(3)
    m = rng.choice(np.array([0, 1, 2, 128, 255], dtype=np.uint8), size=(5, 14, 52))
    assert np.array_equal(pack_bits(m[:, 3:11]), pack_bits(np.ascontiguousarray(m[:, 3:11])))
    assert not np.array_equal(pack_bits(m[:, 3:11]), pack_bits(m[:, 2:10]))


@pytest.mark.parametrize("shape", [(77, 13, 52), (640, 24, 136), (9, 5, 256), (530, 9, 50), (4096, 2048, 2048), (1, 1, 4), (3, 7, 5),
                                   (0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4)])
def test_size_against_the_library(shape):
    got = int(_lib.load().spc_mask_bits_bytes(*shape))
    assert got == bits_bytes(*shape)
    if shape == (4096, 2048, 2048):
        assert got == 2 << 30                      # an eighth of the 16 GiB mask
    if shape[2] % 4 or min(shape) <= 0:
        assert got == 0


def test_the_abi_version_did_not_move():
    assert _lib.ABI_VERSION == 8 and _lib.load().spc_abi_version() == 8
    for name in ("spc_mask_bits_bytes", "spc_mask_pack_bits", "spc_moments_bits_f32"):
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["spc_moments_bits_f32"][1][:10] == _lib.SIGNATURES["spc_moments_f32"][1]


def test_the_slot_for_the_bits_is_no_part_of_what_a_spec_says():
    a = ops.MaskSpec(_lib.MASK_GT, 1.0, 0.0)
    b = ops.MaskSpec(_lib.MASK_GT, 1.0, 0.0)
    b._bits_uses, b._bits_failed, b._bits_key = 5, True, (1, 2)
    assert a == b and repr(a) == repr(b) and "_bits" not in repr(a)
    assert ops.MaskSpec(3, 0.5, 2.0, None) == ops.MaskSpec(flags=3, thr_lo=0.5, thr_hi=2.0, array=None)
    b.invalidate()
    assert (b._bits, b._bits_key, b._bits_uses, b._bits_failed) == (None, None, 0, False)
    with pytest.raises(TypeError):
        ops.MaskSpec(0, 0.0, 0.0, None, None)      # the slot is not a constructor argument


def test_write_generation_lives_on_the_root_of_the_owner_chain():
    root = DeviceArray((4, 6, 8), np.uint8, ptr=4096)          # a made-up address: nothing is launched
    rows = root.rows(1, 5)
    planes = rows.planes(1, 3)
    other = DeviceArray((4, 6, 8), np.uint8, ptr=8192)
    g0 = root.write_generation
    assert rows.write_generation == planes.write_generation == g0
    planes.mark_written()
    assert root.write_generation == rows.write_generation == planes.write_generation == g0 + 1
    root.mark_written()
    assert planes.write_generation == g0 + 2 and other.write_generation == 0


@pytest.mark.parametrize("text, on", [(None, True), ("1", True), ("0", False), ("", False), ("2", True), ("no", False), (" 1", True),
                                      ("1x", True), ("-1", True), ("+0", False)])
def test_the_switch_is_read_as_the_library_reads_it(monkeypatch, text, on):
    if text is None:
        monkeypatch.delenv("SPC_MOMENTS_MASK_BITS", raising=False)
    else:
        monkeypatch.setenv("SPC_MOMENTS_MASK_BITS", text)
    assert ops._switch_on("SPC_MOMENTS_MASK_BITS") is on
