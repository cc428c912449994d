"""Shared by test_mask_patterns_host.py (CPU) and test_gpu_mask_patterns.py (GPU): the include sets, the byte values and the
poison that every masked entry point is run on.  Nothing here touches the GPU.

The uint8 include array is read in several ways by the kernels - single bytes, dwords decoded with ``(m >> 8 c) & 0xff``, the
sign-extended bit 0 of each byte after a wave-wide "every byte is 0 or 1" test, a SWAR "byte != 0" reduction, "dword != 0, so
skip the 16-byte cube load" - and its contract is one line: any non-zero byte includes, a byte is never a weight, and no
sample the array excludes reaches a result.  Three things pin that:

PATTERNS   include sets for a shape (nz, ny, nx): what the 70 % random mask of views.data never has - an empty or a full
           mask, a single voxel, empty dwords, empty 16-byte groups, empty rows, planes and rays, one byte lane per dword.
BYTES      how an include set becomes bytes: 1, 2 (bit 0 clear), 0x80 (the sign bit alone), 0xFF, and a seeded mix.
poison     NaN, +inf, -inf, +max, -max and the smallest subnormal under a seeded quarter of the excluded voxels, next to the
           same cube with 0 there: the two must give the same bits.

``properties`` states what each pattern claims to contain; the host test asserts it for every shape of SHAPES."""
import functools

import numpy as np

import views as V

PATTERNS = ("all zero", "all one", "one voxel", "sparse", "segments", "slabs", "lanes")
BYTES = ("canonical", "two", "sign", "ones", "mixed")
MIXED_VALUES = (1, 2, 4, 8, 16, 32, 64, 128, 254, 255)
SHAPES = (V.BASE, (21, 9, 1024))          # the two base shapes of the view matrix (views.BASE, test_gpu_views.BASE_WIDE)
POISON_FRACTION = 0.25

# the units a pattern claims to hold BOTH empty and not empty: aligned dwords (4 bytes) and 16-byte groups of the flat array,
# rows (z, y), planes z and rays (y, x)
UNITS = ("dword", "group16", "row", "plane", "ray")
CLAIMS = {"all zero": (), "all one": (), "one voxel": UNITS, "sparse": ("dword", "group16"), "segments": ("dword", "group16"),
          "slabs": UNITS, "lanes": ()}


def _seed(name, shape):
    return 1000 * PATTERNS.index(name) + sum(int(n) for n in shape)


@functools.lru_cache(maxsize=None)
def include(name, shape):
    """the include set of pattern *name* on *shape*: bool, seeded, read-only"""
    shape = tuple(int(n) for n in shape)
    nz, ny, nx = shape
    rng = np.random.default_rng(_seed(name, shape))
    z, y, x = np.arange(nz)[:, None, None], np.arange(ny)[None, :, None], np.arange(nx)[None, None, :]
    if name == "all zero":
        m = np.zeros(shape, bool)
    elif name == "all one":
        m = np.ones(shape, bool)
    elif name == "one voxel":                 # the last column of the last row of the last plane
        m = np.zeros(shape, bool)
        m[-1, -1, -1] = True
    elif name == "sparse":
        m = rng.random(shape) < 0.04
    elif name == "segments":                  # whole aligned 32-voxel x-segments empty: the even ones on odd planes, the odd ones on even planes
        m = rng.random(shape) < 0.3
        m[np.broadcast_to(((x // 32) + z) % 2 == 1, shape)] = False
    elif name == "slabs":
        # empty planes (z % 3 == 0), empty rows (y % 4 == 1), and the rays of the region x < nx // 3 on even y: those at even x
        # empty in every plane, those at odd x empty in every plane but the last, where the 70 % stay
        m = rng.random(shape) < 0.7
        m[np.broadcast_to(z % 3 == 0, shape)] = False
        m[np.broadcast_to(y % 4 == 1, shape)] = False
        region = np.broadcast_to((x < nx // 3) & (y % 2 == 0), shape)
        m[region & np.broadcast_to((x % 2 == 0) | (z < nz - 1), shape)] = False
    elif name == "lanes":                     # exactly one voxel of every aligned group of four x: the byte-lane decode
        m = np.broadcast_to(x % 4 == (z + y + x // 4) % 4, shape).copy()
    else:
        raise KeyError(name)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def _mix(shape):
    v = np.random.default_rng(77 + sum(shape)).choice(np.array(MIXED_VALUES, np.uint8), size=shape)
    v.setflags(write=False)
    return v


def to_bytes(inc, kind):
    """the uint8 array that states include set *inc* with the byte values of *kind*; every excluded voxel is 0"""
    inc = np.asarray(inc, bool)
    if kind == "mixed":
        val = _mix(tuple(inc.shape))
    else:
        val = np.uint8({"canonical": 1, "two": 2, "sign": 0x80, "ones": 0xFF}[kind])
    out = np.where(inc, val, np.uint8(0)).astype(np.uint8)
    out.setflags(write=False)
    return out


def poison_values(dtype):
    fi = np.finfo(dtype)
    return np.array([np.nan, np.inf, -np.inf, fi.max, -fi.max, fi.smallest_subnormal], dtype=dtype)


def poison_set(inc):
    """the voxels that ``poison`` overwrites: a seeded quarter of those *inc* excludes, never none where it excludes any"""
    inc = np.asarray(inc, bool)
    rng = np.random.default_rng(4242 + int(inc.sum()) + sum(inc.shape))
    pick = ~inc & (rng.random(inc.shape) < POISON_FRACTION)
    if not pick.any() and not inc.all():
        pick.reshape(-1)[np.flatnonzero(~inc.reshape(-1))[0]] = True
    return pick


def poison(d, inc, dtype=None):
    """(poisoned, zeroed): *d* with NaN, +inf, -inf, +max, -max and the smallest subnormal (in turn, from a seeded start) in the
    voxels of ``poison_set(inc)``, and *d* with 0 there; both read-only, everything else of *d* unchanged"""
    dtype = np.dtype(d.dtype if dtype is None else dtype)
    pick = poison_set(inc)
    vals = poison_values(dtype.type)
    n = int(pick.sum())
    bad, zero = np.array(d, dtype=dtype), np.array(d, dtype=dtype)
    bad[pick] = vals[(np.arange(n) + int(inc.sum())) % vals.size]
    zero[pick] = 0
    bad.setflags(write=False)
    zero.setflags(write=False)
    return bad, zero


def _units(m):
    """{unit: bool array, True where the unit holds an included voxel}"""
    nz, ny, nx = m.shape
    flat = m.reshape(-1)
    out = {}
    for unit, n in (("dword", 4), ("group16", 16)):
        out[unit] = np.pad(flat, (0, -flat.size % n)).reshape(-1, n).any(axis=1)        # (a last group may be short)
    out["row"], out["plane"], out["ray"] = m.any(axis=2).ravel(), m.any(axis=(1, 2)), m.any(axis=0).ravel()
    return out


def properties(name, shape):
    """the facts the GPU tests rely on, for pattern *name* on *shape*:
    ``empty`` / ``occupied``: {unit: how many of the unit hold no / some included voxel}; ``claims``: the units the pattern is
    there to show both ways; ``lanes``: the byte lanes (x % 4) of the dwords that hold exactly one included voxel;
    ``last_plane_only``: rays whose only included voxels lie in the last plane; ``included`` / ``excluded`` / ``poisoned``: counts"""
    m = include(name, shape)
    u = _units(m)
    nx = m.shape[2]
    lanes = set()
    if nx % 4 == 0:
        d = m.reshape(-1, 4)
        lanes = set(np.argmax(d[d.sum(axis=1) == 1], axis=1).tolist())
    return {"empty": {k: int((~v).sum()) for k, v in u.items()}, "occupied": {k: int(v.sum()) for k, v in u.items()},
            "claims": CLAIMS[name], "lanes": lanes, "last_plane_only": int((m[-1] & ~m[:-1].any(axis=0)).sum()),
            "included": int(m.sum()), "excluded": int((~m).sum()), "poisoned": int(poison_set(m).sum())}
