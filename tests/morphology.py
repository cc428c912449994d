"""Binary morphology restated in numpy, and the case table the host and the GPU tests share (no test here, and nothing of
the package's kernels: test_morphology_host.py holds the restatement against scipy.ndimage, test_gpu_morphology.py the
kernels against scipy.ndimage on the same table).

The rules, for the offsets o = index - size // 2 of a structure's True entries and samples outside the array equal to
border_value:
    dilation  r[p] = OR  over o of in[p - o]
    erosion   r[p] = AND over o of in[p + o]
    out[p] = mask[p] ? r[p] : in[p]            (every step)
    iterations >= 1: that many synchronous steps; iterations < 1: until a step changes nothing.
"""
import itertools

import numpy as np

REACH = 3                     # the widest structure is 7: offsets within +-3
ERODE, DILATE = 0, 1


def generate_binary_structure(rank, connectivity):
    """scipy.ndimage.generate_binary_structure: True within *connectivity* city-block steps of the centre of a 3**rank box"""
    connectivity = max(int(connectivity), 1)
    if rank < 1:
        return np.array(True, dtype=bool)
    out = np.fabs(np.indices([3] * rank) - 1)
    return np.add.reduce(out, 0) <= connectivity


def offsets(structure):
    """(n, 3) int array: index - size // 2 of every True entry"""
    s = np.asarray(structure, dtype=bool)
    return np.argwhere(s) - np.array(s.shape) // 2


def step(x, offs, op, border_value=0, mask=None):
    nz, ny, nx = x.shape
    R = REACH
    xp = np.full((nz + 2 * R, ny + 2 * R, nx + 2 * R), bool(border_value))
    xp[R:R + nz, R:R + ny, R:R + nx] = x
    r = np.zeros(x.shape, bool) if op == DILATE else np.ones(x.shape, bool)
    for dz, dy, dx in offs:
        if op == DILATE:
            r |= xp[R - dz:R - dz + nz, R - dy:R - dy + ny, R - dx:R - dx + nx]
        else:
            r &= xp[R + dz:R + dz + nz, R + dy:R + dy + ny, R + dx:R + dx + nx]
    return r if mask is None else np.where(mask, r, x)


def morph(x, structure, op, iterations=1, mask=None, border_value=0, limit=100000):
    x = np.asarray(x, dtype=bool)
    offs = offsets(structure)
    mask = None if mask is None else np.asarray(mask, dtype=bool)
    if iterations >= 1:
        for _ in range(iterations):
            x = step(x, offs, op, border_value, mask)
        return x
    for _ in range(limit):
        y = step(x, offs, op, border_value, mask)
        if np.array_equal(x, y):
            return y
        x = y
    raise AssertionError("no fixed point in %d steps" % limit)


def binary_dilation(x, structure=None, iterations=1, mask=None, border_value=0):
    return morph(x, _default(structure), DILATE, iterations, mask, border_value)


def binary_erosion(x, structure=None, iterations=1, mask=None, border_value=0):
    return morph(x, _default(structure), ERODE, iterations, mask, border_value)


def binary_opening(x, structure=None, iterations=1, mask=None, border_value=0):
    s = _default(structure)
    return morph(morph(x, s, ERODE, iterations, mask, border_value), s, DILATE, iterations, mask, border_value)


def binary_closing(x, structure=None, iterations=1, mask=None, border_value=0):
    s = _default(structure)
    return morph(morph(x, s, DILATE, iterations, mask, border_value), s, ERODE, iterations, mask, border_value)


def binary_propagation(x, structure=None, mask=None, border_value=0):
    return morph(x, _default(structure), DILATE, -1, mask, border_value)


def _default(structure):
    return generate_binary_structure(3, 1) if structure is None else np.asarray(structure, dtype=bool)


def scipy_morph(x, structure, op, iterations=1, mask=None, border_value=0):
    """scipy.ndimage's result.  Its default path (the one that tracks the voxels changed last) corrupts the heap of the
    process when iterations != 1 and the structure is larger than the array (scipy 1.15: 1x7x1 and 7x2x3 on (5, 6, 70) end
    in `double free or corruption`); brute_force=True is scipy's plain loop over whole arrays, the same result by its
    documentation, and is what such a case is compared with.  Every other case takes the default path."""
    import scipy.ndimage as ndi
    f = ndi.binary_dilation if op == DILATE else ndi.binary_erosion
    brute = iterations != 1 and any(s > n for s, n in zip(np.shape(structure), np.shape(x)))
    return f(x, structure=structure, iterations=iterations, mask=mask, border_value=border_value, brute_force=brute)


# ---- the case table ---------------------------------------------------------------------------------------------
def _pattern(shape, seed, centre):
    """a random structure of *shape*, about half True; its centre entry forced to *centre*"""
    s = np.random.default_rng(seed).random(shape) < 0.5
    c = tuple(n // 2 for n in shape)
    s[c] = centre
    if not s.any():
        s.flat[0] = True
    return s


def _one_sided(shape, seed):
    """a structure that only reaches back along z (every offset has dz < 0, shape[0] >= 2): plane z of a step's result
    depends on earlier planes alone, so repeating it settles plane by plane whatever the mask and the border are,
    although the structure does not hold its centre"""
    s = np.zeros(shape, bool)
    s[:shape[0] // 2] = np.random.default_rng(seed).random((shape[0] // 2,) + tuple(shape[1:])) < 0.6
    s[0].flat[0] = True
    return s


def structures():
    """[(name, structure, settles)]: *settles* = repeating a step is certain to reach a fixed point (the structure holds
    its centre: the sequence is monotone; or it is one-sided).  A structure without either can cycle for ever, in scipy too"""
    out = [("point", np.ones((1, 1, 1), bool), True)]
    for c in (1, 2, 3):
        out.append(("conn%d" % c, generate_binary_structure(3, c), True))
    for shape in ((2, 1, 1), (1, 2, 3), (3, 1, 5), (4, 3, 2), (5, 5, 5), (1, 7, 1), (7, 2, 3)):
        name = "x".join(str(n) for n in shape)
        out.append(("box" + name, np.ones(shape, bool), True))
        if np.prod(shape) > 2:
            out.append(("asym" + name, _pattern(shape, 11 + sum(shape), True), True))
            out.append(("hollow" + name, _pattern(shape, 23 + sum(shape), False), False))
    out.append(("back2x1x1", np.array([True, False]).reshape(2, 1, 1), True))
    out.append(("back4x3x2", _one_sided((4, 3, 2), 5), True))
    return out


SHAPES = ((9, 7, 11), (5, 6, 70), (1, 4, 5), (6, 1, 1))


def field(shape, seed, fill):
    return np.random.default_rng(seed).random(shape) < fill


def cases():
    """every (id, kwargs) of the table: x, structure, op, iterations, mask, border_value"""
    out = []
    for (sname, s, settles), shape, op, iterations, masked, border in itertools.product(
            structures(), SHAPES, (ERODE, DILATE), (1, 2, 0), (False, True), (0, 1)):
        if iterations < 1 and not settles:
            continue
        seed = len(out)
        x = field(shape, seed, 0.75 if op == ERODE else 0.2)
        mask = field(shape, seed + 100000, 0.7) if masked else None
        cid = "%s-%s-%s-it%d-%s-b%d" % (sname, "x".join(map(str, shape)), "erode" if op == ERODE else "dilate", iterations,
                                        "mask" if masked else "nomask", border)
        out.append((cid, dict(x=x, structure=s, op=op, iterations=iterations, mask=mask, border_value=border)))
    return out


def serpentine(shape=(6, 40, 200), gap=4):
    """(corridor mask, seed voxel): one voxel-wide corridor that runs along x, steps *gap* rows on at alternating ends, and
    at the end of a plane steps one plane on - a single path of several hundred voxels through every part of the cube"""
    nz, ny, nx = shape
    m = np.zeros(shape, bool)
    rows = list(range(1, ny - 1, gap))
    for k in range(0, nz, 2):
        order = rows if (k // 2) % 2 == 0 else rows[::-1]
        for i, j in enumerate(order):
            m[k, j, 1:nx - 1] = True
            if i + 1 < len(order):
                a, b = sorted((j, order[i + 1]))
                m[k, a:b + 1, (nx - 2) if i % 2 == 0 else 1] = True
        if k + 2 < nz:
            # the odd plane above holds one voxel, over the end of this plane's last row
            m[k + 1, order[-1], 1 if (len(order) - 1) % 2 else nx - 2] = True
    return m, (0, rows[0], 1)
