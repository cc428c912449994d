"""The voxel list made from a list of included lane segments (include/spcube_hip.h, spc_moments_vlist_*) restated in numpy,
never the library: shared by tests/test_moments_vlist_host.py and tests/test_gpu_moments_vlist.py.

It is formed from moments_list_layout.build(...)'s output, for the same sublists (block, split * zw + w).  An entry is
{ float v; uint32 meta } with meta = z | col << 28 | 1 << 30 (col: the voxel's place in the lane's 16-byte segment).  A lane's
entries are the voxels whose bit is set in the nibbles of its list entries, in the list's order and in ascending col within
a list entry.  vlen[b][j] is the longest lane's count, voff its exclusive prefix sum over (b, j) in entry rows of 64 x 8
bytes; shorter and dead lanes are padded with all-zero entries."""
import numpy as np

import moments_list_layout as L

ENTRY = np.uint32(1 << 30)


def keep(vrows, rows):
    """the voxel list is kept only where it reads at most half of what the list does: 512 bytes a row against 1280"""
    return 2 * 512 * int(vrows) <= 1280 * int(rows)


def build(lst):
    """dict(vlen (nblocks, nsub) uint32, voff (nblocks, nsub) uint64, entries (vrows, 64, 2) uint32 - [..., 0] the bits of v,
    [..., 1] the meta -, vrows) from moments_list_layout.build's dict"""
    ln, off, meta, samples = lst["len"], lst["off"], lst["meta"], lst["samples"].view(np.uint32)
    nblocks, nsub = ln.shape
    cols = np.arange(4, dtype=np.uint32)
    lanes = {}
    vlen = np.zeros((nblocks, nsub), dtype=np.uint32)
    for b in range(nblocks):
        for j in range(nsub):
            o, n = int(off[b, j]), int(ln[b, j])
            if not n:
                continue
            m = meta[o:o + n]                                           # (n, 64)
            bit = ((m[:, :, None] >> (28 + cols)) & 1).astype(bool)     # (n, 64, 4): row-major (row, col) is the entry order
            per_lane = []
            for l in range(64):
                r, c = np.nonzero(bit[:, l, :])
                z = m[r, l] & np.uint32(0x0fffffff)
                per_lane.append((samples[o + r, l, c], z | (c.astype(np.uint32) << 28) | ENTRY))
            lanes[b, j] = per_lane
            vlen[b, j] = max(v.size for v, _ in per_lane)
    flat = vlen.reshape(-1).astype(np.uint64)
    voff = (np.cumsum(flat) - flat).reshape(nblocks, nsub)
    vrows = int(flat.sum())
    entries = np.zeros((vrows, 64, 2), dtype=np.uint32)
    for (b, j), per_lane in lanes.items():
        o = int(voff[b, j])
        for l, (v, mt) in enumerate(per_lane):
            entries[o:o + v.size, l, 0] = v
            entries[o:o + v.size, l, 1] = mt
    return dict(vlen=vlen, voff=voff, entries=entries, vrows=vrows)


def direct(cube, mask, zw, nsplit, zchunk):
    """per (block, sublist, lane) the (bits of v, meta) pairs from the cube and the mask alone: a walk of the sublist's planes in
    ascending order and of the lane's four columns within a plane"""
    nz, ny, nx = mask.shape
    ngroups = ny * (nx // 4)
    nblocks = -(-ngroups // 64)
    inc = (np.asarray(mask) != 0).reshape(nz, ngroups, 4)
    val = np.asarray(cube, dtype=np.float32).reshape(nz, ngroups, 4).view(np.uint32)
    out = {}
    for b in range(nblocks):
        for j, zs in enumerate(L.sublist_planes(nz, zw, nsplit, zchunk)):
            for l in range(64):
                g = b * 64 + l
                pairs = []
                if g < ngroups:
                    for z in zs:
                        for col in range(4):
                            if inc[z, g, col]:
                                pairs.append((int(val[z, g, col]), int(z) | (col << 28) | (1 << 30)))
                out[b, j, l] = pairs
    return out


def walk_vlist(vl, cen, nz, zw, nsplit, zchunk):
    """the sums of moments_list_layout.walk_planes from the voxel list's entry rows alone: every entry goes through all four
    columns, three of them with ok false"""
    nblocks, nsub = vl["vlen"].shape
    subs = L.sublist_planes(nz, zw, nsplit, zchunk)
    out = []
    for b in range(nblocks):
        for j in range(nsub):
            acc = L._new_acc(int(subs[j][0]) if subs[j].size else 0)
            o = int(vl["voff"][b, j])
            for r in range(o, o + int(vl["vlen"][b, j])):
                mt = vl["entries"][r, :, 1]
                z = np.minimum((mt & 0x0fffffff).astype(np.int64), nz - 1)
                v = np.repeat(vl["entries"][r, :, 0].copy().view(np.float32)[:, None], 4, axis=1)
                nib = (((mt >> 30) & 1) << ((mt >> 28) & 3)).astype(np.uint8)
                L._add(acc, v, nib, cen[z], z)
            out.append(acc)
    return out
