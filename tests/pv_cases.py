"""Shared by the position-velocity tests (test_pv_extract_host.py, test_gpu_pv_extract.py): the scipy oracle, the numpy
restatement of the kernel's rule (include/spcube_hip.h, csrc/spc_pv_extract.hip), the error bound, and the case table.
No tests; nothing here touches the GPU.

oracle       per channel, on the FILLED plane: map_coordinates(nan_to_num(plane), [y, x], order, mode='constant', cval=nan),
             then (respect_nan) NaN where map_coordinates(isnan(plane).astype(float), ..., cval=0) is non-zero; the mean over
             the lines that are not NaN (np.nanmean, NaN and no warning where there is none) and their count.
restate      the kernel's rule in float64 numpy, the same operations in the same order: bit-identical for a float64 cube.
bound        the derived distance between the two at order 1, see its docstring.
"""
import functools
import itertools
import warnings

import numpy as np
import scipy.ndimage as ndi

U = 2.0 ** -53

PLANES = ((2, 2), (1, 5), (7, 9))
NZS = (1, 2, 7, 37)
NPTS = (1, 63, 64, 65, 130)
NLINES = (1, 2, 5)


def filled(data, include=None, fill=np.nan):
    """the cube's filled data: *fill* where *include* (bool, or None: everything) excludes the voxel"""
    d = np.array(data, copy=True)
    if include is not None:
        d[~np.asarray(include, bool)] = fill
    return d


def oracle_lines(fdata, xs, ys, order, respect_nan):
    """(nz, nlines, npts) float64: every line's value by scipy, on filled data"""
    f = np.asarray(fdata, np.float64)
    xs, ys = np.atleast_2d(xs), np.atleast_2d(ys)
    out = np.empty((f.shape[0],) + xs.shape)
    coords = [ys, xs]
    for k in range(f.shape[0]):
        hole = np.isnan(f[k])
        v = ndi.map_coordinates(np.where(hole, 0.0, f[k]), coords, order=order, mode="constant", cval=np.nan)
        if respect_nan:
            bad = ndi.map_coordinates(hole.astype(np.float64), coords, order=order, mode="constant", cval=0.0)
            v = np.where(bad != 0, np.nan, v)
        out[k] = v
    return out


def mean_lines(lines):
    """(np.nanmean over the line axis with all-NaN -> NaN and no warning, the count of lines that are not NaN)"""
    count = (~np.isnan(lines)).sum(axis=1).astype(np.int32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        mean = np.nanmean(lines, axis=1)
    return mean, count


def oracle(fdata, xs, ys, order, respect_nan):
    """(diagram (nz, npts) float64, count (nz, npts) int32) by scipy + np.nanmean"""
    return mean_lines(oracle_lines(fdata, xs, ys, order, respect_nan))


def restate(fdata, xs, ys, order, respect_nan, dtype=None):
    """(diagram in *dtype* (the cube's by default), count int32, scale): the kernel's rule restated.  *scale*: the pair
    (S, V) that ``bound`` multiplies, per output the mean over the counted lines of sum |w_i v_i| and of sum |v_i| over the
    neighbours of non-zero weight that are not NaN."""
    fdata = np.asarray(fdata)
    dtype = np.dtype(dtype or fdata.dtype)
    f = fdata.astype(np.float64)
    xs, ys = np.atleast_2d(np.asarray(xs, np.float64)), np.atleast_2d(np.asarray(ys, np.float64))
    nz, ny, nx = f.shape
    nlines, npts = xs.shape
    total = np.zeros((nz, npts))
    scale = np.zeros((nz, npts))
    vscale = np.zeros((nz, npts))
    count = np.zeros((nz, npts), np.int32)
    raw = np.full((nz, npts), np.nan)
    with np.errstate(invalid="ignore"):
        for l in range(nlines):
            x, y = xs[l], ys[l]
            inside = (x >= 0.0) & (x <= nx - 1.0) & (y >= 0.0) & (y <= ny - 1.0)
            xi, yi = np.where(inside, x, 0.0), np.where(inside, y, 0.0)
            if order == 0:
                nbrs = [(np.floor(yi + 0.5).astype(np.int64), np.floor(xi + 0.5).astype(np.int64), np.ones(npts))]
            else:
                xf, yf = np.floor(xi), np.floor(yi)
                fx, fy = xi - xf, yi - yf
                x0, y0 = xf.astype(np.int64), yf.astype(np.int64)
                x1, y1 = np.minimum(x0 + 1, nx - 1), np.minimum(y0 + 1, ny - 1)
                gx, gy = 1.0 - fx, 1.0 - fy
                nbrs = [(y0, x0, gy * gx), (y0, x1, gy * fx), (y1, x0, fy * gx), (y1, x1, fy * fx)]
            val = np.zeros((nz, npts))
            mag = np.zeros((nz, npts))
            vmag = np.zeros((nz, npts))
            hole = np.zeros((nz, npts), bool)
            for jy, jx, w in nbrs:
                v = f[:, jy, jx]
                use = (w != 0.0)[None, :]
                nan = np.isnan(v)
                hole |= use & nan
                term = w[None, :] * np.where(nan, 0.0, v)
                add = use & ~nan
                val = np.where(add, val + term, val)
                mag = np.where(add, mag + np.abs(term), mag)
                vmag = np.where(add, vmag + np.abs(np.where(nan, 0.0, v)), vmag)
            counted = inside[None, :] & ~(hole & bool(respect_nan))
            first = counted & (count == 0)
            total = np.where(first, val, np.where(counted, total + val, total))
            scale = np.where(counted, scale + mag, scale)
            vscale = np.where(counted, vscale + vmag, vscale)
            raw = np.where(counted, np.where(hole, 0.0, f[:, nbrs[0][0], nbrs[0][1]]), raw)
            count = count + counted.astype(np.int32)
        if order == 0 and nlines == 1:
            out = raw
        else:
            out = np.where(count > 0, total / np.maximum(count, 1), np.nan)
        scale, vscale = scale / np.maximum(count, 1), vscale / np.maximum(count, 1)
    return out.astype(dtype), count, (scale, vscale)


def bound(scale, nlines, dtype, expected=None):
    """The largest |device - oracle| at order 1 that float64 rounding explains, per output; U = 2^-53, (S, V) = *scale*
    as ``restate`` returns it: the mean over the counted lines of sum |w_i v_i| and of sum |v_i| (neighbours of non-zero
    weight that are not NaN).

    The device's line.  fx = x - floor(x) is exact and 1 - fx carries one rounding, so a weight - a product of two such
    factors - carries at most 3; the product w v one more; the three additions of the four terms at most one each, on
    partial sums no larger than sum |w_i v_i|.  That is 7 roundings: |line - exact| <= 8 U sum |w_i v_i|, the eighth unit
    covering the terms of second order.
    scipy's line.  Its products and additions are bounded the same way, 4 U sum |w_i v_i|, but not its weights: along an
    axis it forms 1 - fx and then the other weight as the remainder 1 - (1 - fx), which is off from fx by up to U
    ABSOLUTE (measured: map_coordinates at fy = 1e-9 is off by 2.8e-8 relative).  A product of two such weights, each
    <= 1, is off by at most 3 U absolute, 4 U with the second order: 4 U sum |v_i| over the neighbours.
    The mean over n lines: n - 1 additions and one division, each at most U relative on a partial sum no larger than the
    sum over the lines of sum |w_i v_i|; divided by n that is n U S on either side, 2 n U S.  The line errors pass through
    the mean unchanged.  Together
        b = (12 + 2 n) U S + 4 U V.
    A float32 cube rounds the device's float64 result d once: |fl32(d) - d| <= 2^-24 |d| <= 2^-24 (|expected| + b) for a
    normal result, 2^-150 for a subnormal one (*expected*: the oracle's float64 values)."""
    s, v = scale
    b = (12.0 + 2.0 * nlines) * U * np.asarray(s, np.float64) + 4.0 * U * np.asarray(v, np.float64)
    if np.dtype(dtype) == np.float32:
        b = b + 2.0 ** -24 * (np.abs(np.nan_to_num(np.asarray(expected, np.float64))) + b) + 2.0 ** -150
    return b


# ---- data and points -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cube(shape, dtype, seed=0, nan_frac=0.08):
    """seeded normal samples with NaN holes; read-only"""
    rng = np.random.default_rng(100 + seed + sum(shape))
    d = rng.standard_normal(shape).astype(dtype)
    d[rng.random(shape) < nan_frac] = np.nan
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def include(shape, seed=0, frac=0.75):
    rng = np.random.default_rng(200 + seed + sum(shape))
    m = rng.random(shape) < frac
    m.setflags(write=False)
    return m


def edge_values(n):
    """coordinates along an axis of length n that the domain rule turns on: the ends, 1e-9 on either side of them, integers,
    halves, and far outside"""
    last = float(n - 1)
    vals = [0.0, last, -1e-9, last + 1e-9, 1e-9, last - 1e-9, -0.5, last + 0.5, -40.0, last + 1e6, 0.5 * last]
    vals += [float(k) for k in range(n)] + [k + 0.5 for k in range(n - 1)] + [k + 0.25 for k in range(n - 1)]
    return vals


def points(plane, npts, nlines, seed=0):
    """(xs, ys), each (nlines, npts): every pair of edge values first (as many as fit), then seeded random positions of
    which about a sixth lie outside the plane and a quarter on integer x or y; the last line, when there are several, lies
    wholly outside (it never counts)"""
    ny, nx = plane
    rng = np.random.default_rng(300 + seed + 7 * npts + nlines + nx)
    n = nlines * npts
    x = rng.uniform(-0.1 * nx - 0.5, 1.1 * nx - 0.5, n)
    y = rng.uniform(-0.1 * ny - 0.5, 1.1 * ny - 0.5, n)
    onx, ony = rng.random(n) < 0.25, rng.random(n) < 0.25
    x[onx] = np.clip(np.rint(x[onx]), 0, nx - 1)
    y[ony] = np.clip(np.rint(y[ony]), 0, ny - 1)
    pairs = list(itertools.product(edge_values(nx), edge_values(ny)))
    rng.shuffle(pairs)
    m = min(len(pairs), n // 2 if n > 1 else 1)
    x[:m] = [p[0] for p in pairs[:m]]
    y[:m] = [p[1] for p in pairs[:m]]
    order = rng.permutation(n)
    xs, ys = x[order].reshape(nlines, npts), y[order].reshape(nlines, npts)
    if nlines > 1:
        xs[-1] = nx + 3.0 + np.arange(npts)
    return xs, ys


def zigzag(plane, npts):
    """one line that leaves the plane and re-enters it several times: a straight sweep from (-2, -1) to (nx + 1, ny)"""
    ny, nx = plane
    t = np.linspace(0.0, 1.0, npts) if npts > 1 else np.array([0.5])
    x = -2.0 + (nx + 3.0) * t
    y = (ny - 1.0) * 0.5 + (0.5 * ny + 1.0) * np.sin(6.0 * np.pi * t)
    return x[None], y[None]


def zero_weight_holes(shape, dtype):
    """(cube, xs, ys): a NaN at every voxel with x + y odd, and points exactly on the finite voxels' integer coordinates and
    on the lines x = integer / y = integer between them - each has zero-weight neighbours that are NaN and must not count"""
    nz, ny, nx = shape
    d = np.arange(nz * ny * nx, dtype=np.float64).reshape(shape).astype(dtype) + 1
    yy, xx = np.mgrid[:ny, :nx]
    d[:, (yy + xx) % 2 == 1] = np.nan
    gx, gy = np.meshgrid(np.arange(nx, dtype=np.float64), np.arange(ny, dtype=np.float64))
    on = ((gy + gx) % 2 == 0).ravel()
    xs = np.concatenate([gx.ravel()[on], gx.ravel()[:-1] + 0.5, gx.ravel()])
    ys = np.concatenate([gy.ravel()[on], gy.ravel()[:-1], np.minimum(gy.ravel() + 0.5, ny - 1.0)])
    keep = xs <= nx - 1
    return d, xs[keep][None], ys[keep][None]


def cases():
    """[(id, plane (ny, nx), nz, npts, nlines)]: every plane with every nz, every npts and every nlines at least once, not
    the full product"""
    out = []
    for i, plane in enumerate(PLANES):
        for j, nz in enumerate(NZS):
            npts = NPTS[(i + j) % len(NPTS)]
            nlines = NLINES[(i + 2 * j) % len(NLINES)]
            out.append(("%dx%d-nz%d-p%d-l%d" % (plane + (nz, npts, nlines)), plane, nz, npts, nlines))
        for npts, nlines in ((1, 5), (63, 1), (64, 2), (65, 5), (130, 1), (130, 2)):
            out.append(("%dx%d-nz3-p%d-l%d" % (plane + (npts, nlines)), plane, 3, npts, nlines))
    return out


HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -2e-3, "CDELT2": 2e-3, "CDELT3": 0.5,
       "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s", "CRPIX1": 5.0, "CRPIX2": 4.0, "CRPIX3": 1.0, "CRVAL1": 10.0,
       "CRVAL2": 20.0, "CRVAL3": -16.0, "RESTFRQ": 1.420405752e9, "BUNIT": "K"}
