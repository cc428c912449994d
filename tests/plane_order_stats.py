"""Inputs and expected values shared by the tests of test_gpu_plane_order_stats.py: median / percentile / mad_std over two
axes.  Importing this module touches no GPU; the expected values are oracle/oracle_np.py on the host, computed once per
(shape, mask) and handed out read-only.

Data: float32 samples 0.3 + N(0, 1), about 5 % NaN, and a few infinities of each sign, placed so that no plane z, no row
index y and no column index x holds more than one of a sign.  (Where an order statistic that a percentile interpolates
FROM is infinite, numpy's lerp - ``a + (b - a) t`` below t = 0.5, ``b - (b - a)(1 - t)`` from there - and the kernels'
``a + (b - a) t`` give different non-finite answers; with one infinity per group that needs a group of at most ten
samples.  Where a column x has no more than that, the infinity is its only sample - the median is the infinity, the lerp
between two equal infinities NaN in numpy and here.  ``expected`` asserts that a NaN in an expected array is a group
without a sample or such a column.)

Masks: ``finite`` - the isfinite predicate (SpectralCube.read); ``threshold`` - ``cube > 0.1`` alone, which keeps +inf;
``array`` - a boolean array including about 70 %, which keeps both infinities."""
import functools

import numpy as np

import oracle_np as O

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 1, "CRPIX2": 1, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}
PAIRS = ((1, 2), (0, 2), (0, 1))
QS = (10.0, 37.5, 90.0)
MASKS = ("finite", "threshold", "array")
THRESHOLD = 0.1
# the smallest shapes at which each mechanism of the kernel can go wrong (see test_gpu_plane_order_stats.py)
SHAPES = ((5, 7, 9), (4, 64, 64), (3, 70, 531), (700, 5, 7), (2, 3, 70001))


@functools.lru_cache(maxsize=None)
def data(shape, seed=11):
    rng = np.random.default_rng(seed + sum(shape))
    d = (0.3 + rng.standard_normal(shape)).astype(np.float32)
    d[rng.random(shape) < 0.05] = np.nan
    nz, ny, nx = shape
    for i in range(min(3, min(shape))):
        hi, lo = (i, i, (2 * i + 1) % nx), (i, ny - 1 - i, (nx - 2 - 2 * i) % nx)
        assert hi != lo
        if nz * ny <= 10:                      # (its column would be such a group: the infinity is the column's only sample)
            d[:, :, hi[2]] = d[:, :, lo[2]] = np.nan
        d[hi], d[lo] = np.inf, -np.inf
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def include_array(shape, seed=11):
    m = np.random.default_rng(seed + 1000 + sum(shape)).random(shape) < 0.7
    m.setflags(write=False)
    return m


def include(shape, kind):
    """the voxels the mask *kind* includes, as numpy evaluates it"""
    d = data(shape)
    with np.errstate(invalid="ignore"):
        return {"finite": np.isfinite(d), "threshold": d > np.float32(THRESHOLD), "array": include_array(shape)}[kind]


def cube(shape, kind, d=None):
    """the SpectralCube of the case (a copy of the data: the cached arrays are read-only)"""
    from spectral_cube_amd import SpectralCube
    d = data(shape).copy() if d is None else d
    if kind == "finite":
        return SpectralCube.read(d, HDR)
    c = SpectralCube(d, header=HDR)
    return c.with_mask(c > THRESHOLD) if kind == "threshold" else c.with_mask(include_array(shape))


def oracle(d, inc, pair):
    """{"median", "p10", "p37.5", "p90", "mad_std"}: oracle_np over *pair*"""
    out = {"median": O.median(d, inc, axis=pair), "mad_std": O.mad_std(d, inc, axis=pair)}
    # (one call for the three percentiles: np.nanpercentile walks the groups in Python, 70001 of them for a long row)
    for q, v in zip(QS, O.percentile(d, inc, list(QS), axis=pair)):
        out["p%g" % q] = v
    return out


@functools.lru_cache(maxsize=None)
def expected(shape, kind):
    """{pair: oracle(...)} of the case, read-only"""
    d, inc = data(shape), include(shape, kind)
    out = {}
    for pair in PAIRS:
        e = oracle(d, inc, pair)
        n = (inc & ~np.isnan(d)).sum(axis=pair)
        lone = (n > 0) & ((inc & np.isfinite(d)).sum(axis=pair) == 0)          # nothing but an infinity
        for k, v in e.items():
            v = np.asarray(v)
            nan = (n == 0) if k == "median" else (n == 0) | lone
            assert np.array_equal(np.isnan(v), nan), (shape, kind, pair, k, "a non-finite order statistic meets numpy's lerp")
            v.setflags(write=False)
        out[pair] = e
    return out


def check(got, exp, what):
    """the bounds of the one-axis forms (test_gpu_long_axes.py:28-32): median exact (signed zeros compare equal: numpy's
    partition does not order them either), percentile rtol 2e-6 + atol 2e-6 max|exp|, mad_std 3e-6 likewise; NaN and
    infinities in the same places"""
    from conftest import assert_close
    assert set(got) == set(exp), what
    for k, e in exp.items():
        g = np.asarray(got[k])
        e = np.asarray(e)
        assert g.dtype == np.float32 and g.shape == e.shape, (what, k, g.dtype, g.shape, e.shape)
        fin = np.isfinite(e)
        top = float(np.abs(e[fin]).max()) if fin.any() else 0.0
        tol = 0.0 if k == "median" else 3e-6 if k == "mad_std" else 2e-6
        assert_close(g, e, rtol=tol, atol=tol * top, what="%s %s" % (what, k))


# ---- planted groups: (12, 6, 10), one plane each ---------------------------------------------------------------------
PLANTED = ("empty", "one", "two", "equal", "zeros", "signs", "last_byte", "even_tie")


@functools.lru_cache(maxsize=None)
def planted():
    """(data, include) of shape (12, 6, 10): planes 0 .. 7 hold the groups of PLANTED, the rest ordinary samples"""
    rng = np.random.default_rng(5)
    shape = (12, 6, 10)
    d = (0.3 + rng.standard_normal(shape)).astype(np.float32)
    inc = rng.random(shape) < 0.8
    n = shape[1] * shape[2]
    inc[0] = False                                                      # no included sample: NaN out
    inc[1] = False
    inc[1, 3, 4] = True                                                 # one sample
    inc[2] = False
    inc[2, 0, 1] = inc[2, 5, 9] = True                                  # two different samples: the next-key pass, the mean
    d[2, 0, 1], d[2, 5, 9] = 1.25, -3.5
    d[3], inc[3] = 2.5, True                                            # all samples equal
    d[4] = np.where(rng.random(shape[1:]) < 0.5, np.float32(0.0), np.float32(-0.0))       # only +0.0 and -0.0
    inc[4] = True
    d[5] = (rng.integers(-3, 4, shape[1:]) * np.float32(1e-3)).astype(np.float32)          # mixed signs around zero
    d[5, 0, :3] = (1e-42, -1e-42, -0.0)                                 # (subnormals of both signs)
    inc[5] = True
    d[6] = (1.0 + rng.permutation(n).reshape(shape[1:]) * 2.0 ** -23).astype(np.float32)  # keys agree down to the last byte
    inc[6] = True
    v = np.sort(rng.standard_normal(n).astype(np.float32))
    v[n // 2 - 1] = v[n // 2]                                           # an even count whose two middle values are equal
    d[7] = rng.permutation(v).reshape(shape[1:])
    inc[7] = True
    assert len(np.unique(d[6])) == n and inc[7].sum() % 2 == 0
    d.setflags(write=False)
    inc.setflags(write=False)
    return d, inc
