"""The packed form of a uint8 mask array (include/spcube_hip.h, spc_mask_pack_bits) restated in numpy, never the library:
shared by tests/test_mask_bits_host.py and tests/test_gpu_moments_mask_bits.py.

Lane group g = y * (nx / 4) + x / 4 over the array as the call sees it, block b = g / 64, lane l = g % 64; the bits of plane z
of block b are the 32 bytes at (b * nz + z) * 32; lane l owns nibble (l & 1) of byte l >> 1; bit i of the nibble is "mask byte
of voxel x + i != 0"; lanes past the last group have zero bits."""
import numpy as np


def bits_bytes(nz, ny, nx):
    if nz <= 0 or ny <= 0 or nx <= 0 or nx % 4:
        return 0
    return -(-(ny * (nx // 4)) // 64) * nz * 32


def pack_bits(mask):
    """uint8 vector of bits_bytes(*mask.shape) bytes from a (nz, ny, nx) array (any dtype: non-zero means included)"""
    nz, ny, nx = mask.shape
    assert nx % 4 == 0
    ngroups = ny * (nx // 4)
    nblocks = -(-ngroups // 64)
    inc = (np.asarray(mask) != 0).reshape(nz, ngroups, 4).astype(np.uint8)
    nib = inc[..., 0] | (inc[..., 1] << 1) | (inc[..., 2] << 2) | (inc[..., 3] << 3)         # (nz, ngroups)
    lanes = np.zeros((nz, nblocks * 64), dtype=np.uint8)
    lanes[:, :ngroups] = nib
    lanes = lanes.reshape(nz, nblocks, 32, 2)
    byte = lanes[..., 0] | (lanes[..., 1] << 4)                                              # (nz, nblocks, 32)
    return np.ascontiguousarray(byte.transpose(1, 0, 2)).reshape(-1)
