"""The list of included lane segments of a cube under a mask (include/spcube_hip.h, spc_moments_list_*) restated in numpy,
never the library: shared by tests/test_moments_list_host.py and tests/test_gpu_moments_list.py.

Lane group g = y * (nx / 4) + x / 4, block b = g / 64, lane l = g % 64 (the layout of the packed bits).  For a launch plan
(zw, nsplit, zchunk) sublist j = split * zw + w of block b holds the planes z = zb + w, zb + w + zw, ... < ze of split
`split` (zb = split * zchunk, ze = min(nz, zb + zchunk)); a lane keeps those where its nibble of the bits is not zero, in
ascending order.  len[b][j] is the longest lane's count, off the exclusive prefix sum of len over (b, j) in entry rows; an
entry row is 64 float4 of samples (as they lie in the cube) and 64 uint32 of meta (z | nibble << 28); shorter lanes and
dead lanes are padded with zero samples and zero meta."""
import numpy as np


def nibbles(mask):
    """(nz, nblocks * 64) uint8: every lane's four mask bits per plane, dead lanes zero"""
    nz, ny, nx = mask.shape
    assert nx % 4 == 0
    ngroups = ny * (nx // 4)
    nblocks = -(-ngroups // 64)
    inc = (np.asarray(mask) != 0).reshape(nz, ngroups, 4).astype(np.uint8)
    nib = np.zeros((nz, nblocks * 64), dtype=np.uint8)
    nib[:, :ngroups] = inc[..., 0] | (inc[..., 1] << 1) | (inc[..., 2] << 2) | (inc[..., 3] << 3)
    return nib


def lanes_of(cube):
    """(nz, nblocks * 64, 4) float32: every lane's float4 per plane, dead lanes zero"""
    nz, ny, nx = cube.shape
    ngroups = ny * (nx // 4)
    nblocks = -(-ngroups // 64)
    out = np.zeros((nz, nblocks * 64, 4), dtype=np.float32)
    out[:, :ngroups] = np.asarray(cube, dtype=np.float32).reshape(nz, ngroups, 4)
    return out


def sublist_planes(nz, zw, nsplit, zchunk):
    """the planes of sublist j = split * zw + w, for every j"""
    out = []
    for split in range(nsplit):
        zb = split * zchunk
        ze = min(nz, zb + zchunk)
        for w in range(zw):
            out.append(np.arange(zb + w, ze, zw, dtype=np.int64))
    return out


def fetched_lines(mask):
    """128-byte cube lines the bits march fetches: the non-zero 32-bit words of the bits (eight lanes each)"""
    nib = nibbles(mask)
    return int(np.count_nonzero(nib.reshape(nib.shape[0], -1, 8).any(axis=2)))


def keep(total_rows, lines, nblocks, nz):
    """the list is kept only where it reads at most half of what the bits march fetches"""
    return 2 * 1280 * int(total_rows) <= 128 * int(lines) + 32 * int(nblocks) * int(nz)


def build(cube, mask, zw, nsplit, zchunk):
    """dict(len (nblocks, nsub) uint32, off (nblocks, nsub) uint64, samples (rows, 64, 4) float32, meta (rows, 64) uint32,
    lines)"""
    nz = mask.shape[0]
    nib, lan = nibbles(mask), lanes_of(cube)
    nblocks = nib.shape[1] // 64
    subs = sublist_planes(nz, zw, nsplit, zchunk)
    nsub = len(subs)
    ln = np.zeros((nblocks, nsub), dtype=np.uint32)
    for b in range(nblocks):
        for j, zs in enumerate(subs):
            if zs.size:
                ln[b, j] = np.count_nonzero(nib[zs, b * 64:(b + 1) * 64], axis=0).max()
    flat = ln.reshape(-1).astype(np.uint64)
    off = (np.cumsum(flat) - flat).reshape(nblocks, nsub)
    rows = int(flat.sum())
    samples = np.zeros((rows, 64, 4), dtype=np.float32)
    meta = np.zeros((rows, 64), dtype=np.uint32)
    for b in range(nblocks):
        for j, zs in enumerate(subs):
            if not ln[b, j]:
                continue
            o = int(off[b, j])
            for l in range(64):
                g = b * 64 + l
                zsel = zs[nib[zs, g] != 0]
                samples[o:o + zsel.size, l] = lan[zsel, g]
                meta[o:o + zsel.size, l] = zsel.astype(np.uint32) | (nib[zsel, g].astype(np.uint32) << 28)
    return dict(len=ln, off=off, samples=samples, meta=meta, lines=fetched_lines(mask), rows=rows)


def _add(acc, v, nibble, c, z):
    """one plane of every lane into the running sums, as acc_add does it: select in float32, widen, three sums, the valid
    count and the first-index extrema (mask bits only: the samples of these tests carry no threshold term)"""
    for i in range(4):
        ok = ((nibble >> i) & 1).astype(bool) & ~np.isnan(v[:, i])
        w = np.where(ok, v[:, i], np.float32(0)).astype(np.float64)
        acc["s0"][:, i] += w
        acc["s1"][:, i] += w * c
        acc["s2"][:, i] += w * (c * c)
        acc["n"][:, i] += ok
        hi = np.where(ok, v[:, i], -np.inf)
        up = hi > acc["bmax"][:, i]
        acc["bmax"][:, i] = np.where(up, hi, acc["bmax"][:, i])
        acc["imax"][:, i] = np.where(up, z, acc["imax"][:, i])


def _new_acc(z0):
    return dict(s0=np.zeros((64, 4)), s1=np.zeros((64, 4)), s2=np.zeros((64, 4)), n=np.zeros((64, 4), dtype=np.int64),
                bmax=np.full((64, 4), -np.inf), imax=np.full((64, 4), z0, dtype=np.int64))


def walk_planes(cube, mask, cen, zw, nsplit, zchunk):
    """per (block, sublist): the sums a wave of the bits march carries after its planes"""
    nib, lan = nibbles(mask), lanes_of(cube)
    nblocks = nib.shape[1] // 64
    out = []
    for b in range(nblocks):
        for zs in sublist_planes(mask.shape[0], zw, nsplit, zchunk):
            acc = _new_acc(int(zs[0]) if zs.size else 0)
            for z in zs:
                m = nib[z, b * 64:(b + 1) * 64]
                v = np.where((m != 0)[:, None], lan[z, b * 64:(b + 1) * 64], np.float32(0))   # lanes the mask excludes hold 0.f
                _add(acc, v, m, np.full(64, cen[z]), np.full(64, z))
            out.append(acc)
    return out


def walk_list(lst, cen, nz, zw, nsplit, zchunk):
    """the same sums from the list's entry rows alone"""
    nblocks, nsub = lst["len"].shape
    subs = sublist_planes(nz, zw, nsplit, zchunk)
    out = []
    for b in range(nblocks):
        for j in range(nsub):
            acc = _new_acc(int(subs[j][0]) if subs[j].size else 0)
            o = int(lst["off"][b, j])
            for r in range(o, o + int(lst["len"][b, j])):
                z = (lst["meta"][r] & 0x0fffffff).astype(np.int64)
                _add(acc, lst["samples"][r], (lst["meta"][r] >> 28).astype(np.uint8), cen[z], z)
            out.append(acc)
    return out
