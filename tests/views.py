"""Shared by test_views_host.py (CPU) and test_gpu_views.py (GPU): the strided, offset and misaligned layouts a cube, a mask
or an output may have inside a larger allocation, as ``(offset_elements, shape, row_stride, plane_stride)``, applied to a
numpy array (the reference always works on the numpy slice) or to a DeviceArray (built the way DeviceArray.rows() builds
its views).  Nothing here touches the GPU until ``device_view`` / ``upload`` are called.

Every view lies strictly inside its parent: two planes before and after it in z (``rows``: none, as rows() views), three rows before and at least two after it
in y, at least three elements after the last x of every row - a tile that over-reads one vector stays inside the
allocation, and what it reads there is poison: 1e30 / 1e300 in a cube (finite: no predicate drops it), 1 in a mask (the
sample counts), so a kernel that uses what it over-read shows in the result.  Output parents are pre-filled with -7e33
(uint8 / integer outputs: a byte pattern) and must still hold it outside the view after the call.

BASE = (21, 9, 132): one 128-column tile and a 4-element tail; the ``xwin_tail`` layout has nx = 131.  The parents are
(25, 14, 140) and, for ``xwin_oddstride``, (25, 15, 139): 15 rows, because 14 * 139 is even and the layout is there for
an odd plane stride as well as a row stride that is no multiple of 4."""
import collections
import functools

import numpy as np

Layout = collections.namedtuple("Layout", "name parent_shape offset shape row_stride plane_stride x0")

BASE = (21, 9, 132)
Z0, Y0 = 2, 3
CUBE_POISON = {np.dtype(np.float32): 1e30, np.dtype(np.float64): 1e300}
OUT_POISON = -7e33

CUBE_LAYOUTS = ("contig", "rows", "planes_of_rows", "xwin_aligned", "xwin_off1", "xwin_oddstride", "xwin_tail")
MASK_LAYOUTS = ("mask_same", "mask_contig", "mask_phase")
OUT_LAYOUTS = ("contig", "out_xwin_aligned", "out_xwin_off1")


def _window(name, shape, x0, pad_x, extra_rows=0):
    nz, ny, nx = shape
    pnx = x0 + nx + pad_x
    parent = (nz + 2 * Z0, ny + Y0 + 2 + extra_rows, pnx)
    rs, ps = pnx, parent[1] * pnx
    return Layout(name, parent, Z0 * ps + Y0 * rs + x0, tuple(shape), rs, ps, x0)


def layout(name, base=BASE):
    """the named layout of a view of *base* = (nz, ny, nx), nx a multiple of 4 (``xwin_tail``: of (nz, ny, nx - 1))"""
    nz, ny, nx = (int(n) for n in base)
    name = {"out_xwin_aligned": "xwin_aligned", "out_xwin_off1": "xwin_off1"}.get(name, name)
    if name == "contig":
        return Layout(name, (nz, ny, nx), 0, (nz, ny, nx), nx, ny * nx, 0)
    assert nx % 4 == 0, "the base extent along x is a multiple of 4: the layouts decide the alignment"
    if name == "rows":                       # parent.rows(Y0, Y0 + ny) of a parent with the view's nx and nz
        parent = (nz, ny + Y0 + 2, nx)
        return Layout(name, parent, Y0 * nx, (nz, ny, nx), nx, parent[1] * nx, 0)
    if name == "planes_of_rows":             # .planes(Z0, Z0 + nz) of such a rows() view
        parent = (nz + 2 * Z0, ny + Y0 + 2, nx)
        ps = parent[1] * nx
        return Layout(name, parent, Z0 * ps + Y0 * nx, (nz, ny, nx), nx, ps, 0)
    if name == "xwin_aligned":               # base and strides 16-byte aligned, row_stride != nx
        return _window(name, (nz, ny, nx), 4, 4)
    if name == "xwin_off1":                  # nx % 4 == 0 and aligned strides, the base one element off
        return _window(name, (nz, ny, nx), 1, 7)
    if name == "xwin_oddstride":             # row_stride % 4 == 3, plane_stride odd
        lay = _window(name, (nz, ny, nx), 4, 3, extra_rows=1)
        assert lay.row_stride % 4 == 3 and lay.plane_stride % 2 == 1
        return lay
    if name == "xwin_tail":                  # general form (odd nx) plus an offset
        return _window(name, (nz, ny, nx - 1), 3, 6)
    if name == "swap01":                     # DeviceArray.swap01() of xwin_aligned
        a = layout("xwin_aligned", base)
        return a._replace(name=name, shape=(ny, nz, nx), row_stride=a.plane_stride, plane_stride=a.row_stride)
    raise KeyError(name)


def mask_layout(name, cube_layout):
    """the layout of the uint8 mask array that goes with a cube in *cube_layout*"""
    shape = cube_layout.shape
    if name == "mask_same":
        return cube_layout
    if name == "mask_contig":                # a fresh array of the view's shape, whatever the cube's strides
        return Layout(name, shape, 0, shape, shape[2], shape[1] * shape[2], 0)
    if name == "mask_phase":                 # an x-window whose x0 mod 4 differs from the cube's
        if cube_layout.name == "swap01":
            raise KeyError("mask_phase goes with the (nz, ny, nx) layouts")
        return _window(name, shape, (cube_layout.x0 + 1) % 4 + 4, 3)
    raise KeyError(name)


def parent_size(lay):
    return int(np.prod(lay.parent_shape, dtype=np.int64))


def _strided(flat, lay):
    it = flat.dtype.itemsize
    strides = (lay.plane_stride * it, lay.row_stride * it, it)
    return np.lib.stride_tricks.as_strided(flat[lay.offset:], shape=lay.shape, strides=strides)


def footprint(lay):
    """flat element indices of the parent that the view covers"""
    idx = np.arange(parent_size(lay), dtype=np.int64)
    return np.ascontiguousarray(_strided(idx, lay)).ravel()


def fits_parent(lay):
    """the view lies inside its parent, touches neither its first nor its last element's neighbourhood (three elements after
    the last sample of a non-contiguous layout), and no two of its elements coincide"""
    f = footprint(lay)
    n = parent_size(lay)
    inside = f.min() >= 0 and f.max() < n
    if lay.name not in ("contig", "mask_contig"):
        inside = inside and f.max() + 3 < n
    return bool(inside and np.unique(f).size == f.size)


def check_cube_conditions(lay, any_order=False):
    """spc_check_cube (csrc/spc_common.h) restated on a layout: None when it passes, else the message the entry gives.
    *any_order*: spc_check_cube_any_order, which also takes a view with its first two axes exchanged"""
    nz, ny, nx = lay.shape
    rs, ps = lay.row_stride, lay.plane_stride
    if min(nz, ny, nx) <= 0:
        return "cube shape must be positive"
    if any_order:
        if not (rs >= nx and ps >= nx):
            return "row / plane stride smaller than nx"
        if not (ps >= rs * (ny - 1) + nx or rs >= ps * (nz - 1) + nx):
            return "overlapping rows and planes"
        return None
    if rs < nx:
        return "row_stride %d < nx %d" % (rs, nx)
    if ps < rs * (ny - 1) + nx:
        return "plane_stride too small"
    return None


def place(lay, data, poison, dtype=None):
    """flat parent array: *poison* everywhere, *data* (of the layout's shape) in the view"""
    data = np.asarray(data, dtype=dtype)
    assert data.shape == lay.shape, (data.shape, lay.shape)
    flat = np.full(parent_size(lay), poison, dtype=data.dtype)
    _strided(flat, lay)[...] = data
    return flat


def extract(lay, flat):
    """a copy of the view's samples out of the flat parent"""
    return np.ascontiguousarray(_strided(np.asarray(flat).ravel(), lay))


def outside(lay, flat):
    """the parent's elements that are not part of the view, in flat order"""
    keep = np.ones(parent_size(lay), bool)
    keep[footprint(lay)] = False
    return np.asarray(flat).ravel()[keep]


def device_view(lay, parent, cls=None):
    """the layout as a DeviceArray view of the (flat) DeviceArray *parent*, built as DeviceArray.rows() builds its views; a
    contiguous layout is an ordinary array of the view's shape on the parent's memory.  *cls*: the host test's stand-in"""
    if cls is None:
        from spectral_cube_amd.device import DeviceArray as cls
    v = cls(lay.shape, parent.dtype, parent.device, ptr=parent.ptr + lay.offset * parent.dtype.itemsize, owner=parent)
    if lay.name in ("contig", "mask_contig"):
        return v
    v.row_stride, v.plane_stride = lay.row_stride, lay.plane_stride
    v.nbytes = 0
    v._is_view = True
    return v


def upload(lay, data, poison, device=0, dtype=None):
    """(view, parent): *data* placed in a poisoned parent on the device"""
    from spectral_cube_amd.device import DeviceArray
    parent = DeviceArray.from_numpy(place(lay, data, poison, dtype), device)
    return device_view(lay, parent), parent


def out_poison(dtype):
    """the pattern an output parent is filled with: -7e33 for floats, bytes of 0xA5 for the integer types"""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return dtype.type(OUT_POISON)
    return np.frombuffer(b"\xa5" * dtype.itemsize, dtype=dtype)[0]


def output(lay, dtype, device=0):
    """(view, parent) of an output in layout *lay*, the parent pre-filled with the poison pattern"""
    return upload(lay, np.full(lay.shape, out_poison(dtype), dtype=dtype), out_poison(dtype), device, dtype)


def read_output(lay, parent):
    """(the view's samples, True when everything outside the view still holds the poison pattern bit for bit)"""
    flat = parent.get().ravel()
    rest = outside(lay, flat)
    want = np.full(rest.shape, out_poison(flat.dtype), dtype=flat.dtype)
    return extract(lay, flat), bool(rest.tobytes() == want.tobytes())


# ---- data ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def data(dtype, shape=BASE, seed=5, nan_frac=0.05, include_frac=0.7, pedestal=0.0):
    """(cube, uint8 mask): seeded normal samples with 5 % NaN, about 70 % of the voxels included; read-only.  *pedestal*: added
    to every sample - the moment and statistics parity tests, whose tolerances the view matrix takes over, run on samples
    of one sign (5 + N(0, 1) in test_moments_f64_kernel_against_the_oracle): a weighted mean over weights that cancel has
    no conditioning to hold a tolerance against"""
    rng = np.random.default_rng(seed)
    d = (pedestal + rng.standard_normal(shape)).astype(dtype)
    d[rng.random(shape) < nan_frac] = np.nan
    m = (rng.random(shape) < include_frac).astype(np.uint8)
    d.setflags(write=False)
    m.setflags(write=False)
    return d, m


def crop(a, lay):
    """*a* (made for the base shape) cut to the layout's nx (``xwin_tail`` has one column less), axes exchanged for swap01"""
    a = np.asarray(a)
    if lay.name == "swap01":
        return np.ascontiguousarray(np.swapaxes(a, 0, 1))
    return np.ascontiguousarray(a[..., :lay.shape[-1]])
