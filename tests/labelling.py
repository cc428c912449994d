"""Shared by the labelling tests (test_labelling_host.py, test_gpu_labelling.py): the structures and the case table of
connected-component labelling, scipy.ndimage as the reference, and the scipy restatement of remove_small_objects.  No tests."""
import functools
import itertools

import numpy as np
import scipy.ndimage as ndi

from morphology import field, serpentine  # noqa: F401  (re-exported for the tests)

SHAPES = ((5, 6, 7), (9, 8, 70), (3, 17, 33), (1, 1, 40), (12, 1, 1), (6, 40, 40))
DENSITIES = (0.1, 0.31, 0.5, 0.9)


def random_structure(seed):
    """a seeded random centrosymmetric 3x3x3 structure: 13 pair bits and a centre"""
    rng = np.random.default_rng(1000 + seed)
    half = rng.random(13) < 0.35
    s = np.zeros(27, bool)
    s[:13] = half
    s[26:13:-1] = half
    s[13] = rng.random() < 0.5
    return s.reshape(3, 3, 3)


def _only(*offsets):
    s = np.zeros((3, 3, 3), bool)
    for o in offsets:
        s[tuple(np.add(o, 1))] = True
        s[tuple(np.subtract(1, o))] = True
    return s


def structures():
    """[(name, structure as label() takes it)]: a (3, 3) entry labels every plane on its own"""
    out = [("conn%d" % c, ndi.generate_binary_structure(3, c)) for c in (1, 2, 3)]
    out.append(("none", np.zeros((3, 3, 3), bool)))
    out.append(("centre", _only((0, 0, 0))))
    out.append(("zpairs", _only((1, 0, 0))))
    out.append(("plane2d", ndi.generate_binary_structure(2, 2)))
    out += [("random%d" % k, random_structure(k)) for k in range(8)]
    return out


def full_structure(s):
    """the 3x3x3 structure a (3, 3) one stands for: its middle plane, the other planes False"""
    s = np.asarray(s) != 0
    if s.ndim == 2:
        full = np.zeros((3, 3, 3), bool)
        full[1] = s
        return full
    return s


def scipy_label(x, structure=None):
    """(labels int32, n) of scipy.ndimage.label; an all-False structure, which scipy also accepts, numbers the True voxels"""
    s = ndi.generate_binary_structure(3, 1) if structure is None else full_structure(structure)
    lab, n = ndi.label(np.asarray(x) != 0, structure=s)
    return lab.astype(np.int32), int(n)


def scipy_objects(lab, n):
    """(sizes int64 (n + 1,), the list scipy.ndimage.find_objects gives)"""
    return np.bincount(lab.ravel(), minlength=n + 1).astype(np.int64), ndi.find_objects(lab, max_label=n)


def scipy_remove_small(x, min_size=64, structure=None, min_channels=1):
    """the host pipeline remove_small_objects replaces: label, bincount, find_objects, a keep table, a gather"""
    lab, n = scipy_label(x, structure)
    sizes, objs = scipy_objects(lab, n)
    keep = np.zeros(n + 1, bool)
    for k, sl in enumerate(objs, start=1):
        keep[k] = sizes[k] >= min_size and sl[0].stop - sl[0].start >= min_channels
    return keep[lab], keep


@functools.lru_cache(maxsize=None)
def cases():
    """((id, x, structure), ...) over SHAPES x DENSITIES x structures(); the arrays are read-only"""
    out = []
    for (sname, s), shape, p in itertools.product(structures(), SHAPES, DENSITIES):
        x = field(shape, len(out), p)
        x.setflags(write=False)
        out.append(("%s-%s-p%g" % (sname, "x".join(map(str, shape)), p), x, s))
    return tuple(out)


def shells(n=40):
    """*n* nested one-voxel shells (the faces of concentric boxes) with a one-voxel gap between them, in a cube of
    4 n - 1 voxels a side: n components under every connectivity, each crossing every part of the array, and the raster
    order of their first voxels (outermost first) is not the order in which any tiling meets them"""
    side = 4 * n - 1
    x = np.zeros((side,) * 3, bool)
    for k in range(n):
        lo, hi = 2 * k, side - 2 * k
        box = x[lo:hi, lo:hi, lo:hi]
        box[[0, -1]] = True
        box[:, [0, -1]] = True
        box[:, :, [0, -1]] = True
    return x


def checkerboard(shape):
    z, y, x = np.indices(shape, sparse=True)
    return ((x + y + z) % 2).astype(bool)


def line_cube(dtype):
    """the line cube of the morphology test: a Gaussian line over noise, NaN borders"""
    shape = (24, 20, 70)
    rng = np.random.default_rng(12)
    z = np.arange(shape[0])[:, None, None]
    amp = 6.0 * np.exp(-0.5 * (((np.arange(shape[1])[:, None] - 9) / 4.0) ** 2 + ((np.arange(shape[2])[None, :] - 35) / 12.0) ** 2))
    d = (rng.normal(size=shape) + amp[None] * np.exp(-0.5 * ((z - 11) / 2.5) ** 2)).astype(dtype)
    d[:, :2] = d[:, -2:] = np.nan
    d[:, :, :3] = d[:, :, -3:] = np.nan
    return d
