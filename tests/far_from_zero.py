"""Shared by test_gpu_far_from_zero.py (GPU) and test_far_from_zero_host.py (CPU): cubes whose samples lie far from zero
compared with their spread - a pedestal, a 1000 K baseline, counts near 2^30, a baseline of its own per spaxel - the
high-precision reference of std on them, and the formula that fails on them.  Nothing here touches the GPU.

Why: sumsq / n - mean^2 evaluated in float64 loses (mean / sigma)^2 ulps.  Zero-mean unit-variance noise, which every other
test of std and of sigma clipping feeds, never shows that; a cube on a pedestal gets noise or 0.  The reference's std is
nanstd, which is two-pass (dask_spectral_cube.py:699-710, spectral_cube.py:667-724)."""
import functools
import math
from fractions import Fraction

import numpy as np

import oracle_np as O

F32, F64 = np.float32, np.float64
EPS64 = float(np.finfo(np.float64).eps)
RTOL = 1e-9                     # of std on the GPU: a two-pass or well-shifted evaluation is bounded by about n eps64 <= 1e-10 for
#                                 the n used here; the textbook form is >= 1e-7 away on every family (test_far_from_zero_host.py)
BLANK32 = -2 ** 31              # the BLANK of the BITPIX = 32 image of `counts64`


# ---- the references -------------------------------------------------------------------------------------------------------
def _axes(axis, ndim=3):
    if axis is None:
        return tuple(range(ndim))
    return tuple(sorted(int(a) for a in (axis if isinstance(axis, (tuple, list)) else (axis,))))


def ref_std(filled, axis=None, ddof=0):
    """nanstd of *filled* (NaN = excluded) in long double, two-pass: the mean, then sqrt(sum (x - mean)^2 / (n - ddof)) over the
    non-NaN samples; NaN where n == 0 or n - ddof <= 0.  *axis*: None, an int or a tuple.  float64 out"""
    x = np.asarray(filled).astype(np.longdouble)
    ax = _axes(axis, x.ndim)
    ok = ~np.isnan(x)
    n = ok.sum(axis=ax)
    with np.errstate(all="ignore"):
        mean = np.where(ok, x, 0).sum(axis=ax, keepdims=True) / ok.sum(axis=ax, keepdims=True)
        dev = np.where(ok, x - mean, 0)
        var = (dev * dev).sum(axis=ax) / (n - ddof)
        out = np.where((n > 0) & (n - ddof > 0), np.sqrt(var), np.nan)
    return out.astype(np.float64) if out.ndim else float(out)


def textbook_std(filled, axis=None, ddof=0):
    """THE WRONG NEIGHBOUR (host check only): sqrt((sumsq - sum^2 / n) / (n - ddof)) in float64 with numpy's pairwise sums,
    what std was before it became two-pass, and still what statistics()['sigma'] is (the reference's own formula there)"""
    x = np.asarray(filled).astype(np.float64)
    ax = _axes(axis, x.ndim)
    ok = ~np.isnan(x)
    n = ok.sum(axis=ax).astype(np.float64)
    x0 = np.where(ok, x, 0.0)
    with np.errstate(all="ignore"):
        s, q = x0.sum(axis=ax), (x0 * x0).sum(axis=ax)
        var = (q - s * s / n) / (n - ddof)
        out = np.where((n > 0) & (n - ddof > 0), np.sqrt(np.maximum(var, 0.0)), np.nan)
    return out if out.ndim else float(out)


def exact_std(samples, ddof=0):
    """std of a short list of samples in exact rational arithmetic, the square root alone taken in long double"""
    v = [Fraction(float(s)) for s in samples if s == s]
    n = len(v)
    if n == 0 or n - ddof <= 0:
        return float("nan")
    mean = sum(v) / n
    var = sum((s - mean) ** 2 for s in v) / (n - ddof)
    hi = float(var)
    lo = float(var - Fraction(hi))
    return float(np.sqrt(np.longdouble(hi) + np.longdouble(lo)))


def wide_sums(filled, axis):
    """(count, sum, sum |x|) per output element of *axis* in long double: what the sum / mean MAPS are held to.  Its own error,
    n 2^-64 of sum |x|, is four decades under the 1e-12 asked; math.fsum (exact_sums) takes a Python call per output element,
    which the 68 300 rays of the widest case do not have the time for - the whole-cube sums do go through it"""
    x = np.asarray(filled).astype(np.longdouble)
    ax = _axes(axis, x.ndim)
    ok = ~np.isnan(x)
    x = np.where(ok, x, 0)
    return ok.sum(axis=ax), x.sum(axis=ax), np.abs(x).sum(axis=ax)


def exact_sums(filled, axis=None):
    """what statistics() / sum / mean are held to: {npts, min, max, sum, sumsq, mean, rms} of the non-NaN samples with math.fsum
    over the float64-widened samples and over their squares, per output element of *axis* (None: the whole cube, floats)"""
    x = np.asarray(filled).astype(np.float64)
    ax = _axes(axis, x.ndim)
    keep = tuple(a for a in range(x.ndim) if a not in ax)
    rays = np.transpose(x, keep + ax).reshape(int(np.prod([x.shape[a] for a in keep], dtype=np.int64)), -1)
    out = {k: np.full(rays.shape[0], np.nan) for k in ("npts", "min", "max", "sum", "sumsq", "mean", "rms")}
    for i, r in enumerate(rays):
        r = r[~np.isnan(r)]
        out["npts"][i] = r.size
        out["sum"][i], out["sumsq"][i] = math.fsum(r), math.fsum(r * r)
        if r.size:
            out["min"][i], out["max"][i] = r.min(), r.max()
            out["mean"][i], out["rms"][i] = out["sum"][i] / r.size, math.sqrt(out["sumsq"][i] / r.size)
    shape = tuple(x.shape[a] for a in keep)
    return {k: (v.reshape(shape) if shape else float(v[0])) for k, v in out.items()}


# ---- the case families: (dtype, shape, seed) -> (data, uint8 include array, threshold of the `cube > thr` predicate) -------------
def _baselines(dtype, ny, nx):
    """one baseline per spaxel, log-spaced from -top to +top across the plane (top 1e6; float32: 3e4), never zero"""
    top = 1e6 if dtype == F64 else 3e4
    n = ny * nx
    neg = n // 3                # (not half: the sums over the plane must not cancel, or no float64 sum could be held to 1e-12)
    mag = np.concatenate([np.logspace(np.log10(top), 0.0, neg), np.logspace(0.0, np.log10(top), n - neg)])
    sign = np.concatenate([-np.ones(neg), np.ones(n - neg)])
    return (sign * mag).astype(dtype).reshape(ny, nx)


def _include(rng, shape, frac=0.7):
    return (rng.random(shape) < frac).astype(np.uint8)


def _sprinkle(d, arr):
    """a NaN block, one all-NaN ray, one ray the include array excludes entirely (every family but `constant`)"""
    nz, ny, nx = d.shape
    d[nz // 3:nz // 3 + 3, ny // 2:ny // 2 + 2, nx // 3:nx // 3 + 4] = np.nan
    d[:, ny - 1, nx // 2] = np.nan
    arr[:, 0, nx - 1] = 0


def _below(dtype, x):
    """a threshold the cube's dtype holds exactly (the predicate is evaluated in that dtype)"""
    return float(dtype(x))


def pedestal32(dtype, shape, seed):
    rng = np.random.default_rng([1, seed])
    d = (3e4 + 0.05 * rng.standard_normal(shape)).astype(dtype)
    return d, _include(rng, shape), _below(dtype, 3e4 - 0.05)


def negative32(dtype, shape, seed):
    rng = np.random.default_rng([2, seed])
    d = (-1e4 + 0.02 * rng.standard_normal(shape)).astype(dtype)
    return d, _include(rng, shape), _below(dtype, -1e4 - 0.02)


def baseline64(dtype, shape, seed):
    rng = np.random.default_rng([3, seed])
    d = (1000.0 + 1e-3 * rng.standard_normal(shape)).astype(dtype)
    z0 = shape[0] // 2
    d[z0:z0 + 3] += 0.5                                        # a 0.5-high line in a few channels
    return d, _include(rng, shape), _below(dtype, 1000.0 - 1e-3)


def counts_raw(shape, seed):
    """the int32 samples of `counts64` (the image adds BZERO = 2^30): integers in [-30, 30]"""
    return np.random.default_rng([4, seed]).integers(-30, 30, size=shape, endpoint=True).astype(np.int32)


def counts64(dtype, shape, seed):
    rng = np.random.default_rng([5, seed])
    d = (counts_raw(shape, seed).astype(np.float64) + 2.0 ** 30).astype(dtype)
    return d, _include(rng, shape), _below(dtype, 2.0 ** 30 - 10.5)


def per_ray(dtype, shape, seed):
    """every spaxel on a baseline of its own: ONE cube-wide pivot cannot condition these rays - the case that catches a half fix"""
    rng = np.random.default_rng([6, seed])
    base = _baselines(dtype, shape[1], shape[2]).astype(np.float64)
    noise = 1e-6 if dtype == F64 else 1e-5
    d = (base[None] * (1.0 + noise * rng.standard_normal(shape))).astype(dtype)
    pick = base.ravel()[(3 * base.size) // 4]                   # a ray on the positive side: it is cut, the rays below it go
    return d, _include(rng, shape), _below(dtype, pick * (1.0 - noise))


def constant(dtype, shape, seed):
    """every sample of a ray equals its baseline: std is 0, held to 8 eps64 |baseline| (no NaN, no special ray)"""
    rng = np.random.default_rng([7, seed])
    base = _baselines(dtype, shape[1], shape[2])
    d = np.ascontiguousarray(np.broadcast_to(base[None], shape)).astype(dtype)
    return d, _include(rng, shape), _below(dtype, base.ravel()[(3 * base.size) // 4])


def sparse(dtype, shape, seed):
    """rays with 0, 1 and 2 included samples (in turn, then the 70 % draw) on a pedestal: the NaN rules of ddof = 1"""
    rng = np.random.default_rng([8, seed])
    top, sd = (1e3, 0.05) if dtype == F64 else (3e4, 0.05)          # (two samples a hair apart: numpy's own nanstd is off by (eps mean / gap)^2)
    d = (top + sd * rng.standard_normal(shape)).astype(dtype)
    arr = _include(rng, shape)
    nz, ny, nx = shape
    kind = (np.arange(ny * nx) % 4).reshape(ny, nx)             # 0, 1, 2 samples; 3: the draw
    for k in (0, 1, 2):
        sel = kind == k
        arr[:, sel] = 0
        for j in range(k):
            arr[(5 * j + 2) % nz, sel] = 1
    return d, arr, _below(dtype, top - 3 * sd)


FAMILIES = {"pedestal32": (pedestal32, (F32,)), "negative32": (negative32, (F32,)), "baseline64": (baseline64, (F64,)),
            "counts64": (counts64, (F64,)), "per_ray": (per_ray, (F32, F64)), "constant": (constant, (F32, F64)),
            "sparse": (sparse, (F32, F64))}
# the smallest shapes that still reach every kernel form (test_gpu_far_from_zero.py says which)
SHAPES = {F32: ((48, 9, 37), (40, 8, 64), (3, 50, 1366), (515, 2, 37)), F64: ((33, 5, 7), (9, 3, 130), (64, 6, 8))}
MIXED_SIGNS = ("per_ray", "constant")         # baselines of both signs: a sum over the plane can cancel (see wide_sums' users)
AXES = (None, 0, 1, 2, (1, 2), (0, 1), (0, 2))
MASKS = ("none", "array", "predicate", "array & predicate")


@functools.lru_cache(maxsize=None)
def case(family, dtype, shape, seed=0):
    """(data, uint8 include array, threshold) of a family, with its sprinkles; read-only"""
    fn, dtypes = FAMILIES[family]
    assert dtype in dtypes
    d, arr, thr = fn(dtype, shape, seed)
    if family != "constant":
        _sprinkle(d, arr)
    d.setflags(write=False)
    arr.setflags(write=False)
    return d, arr, thr


def include_of(d, arr, thr, mask):
    """the include set of one of MASKS as numpy evaluates it in the cube's dtype (NaN > thr is False), or None"""
    if mask == "none":
        return None
    inc = np.ones(d.shape, bool)
    if "array" in mask:
        inc &= arr != 0
    if "predicate" in mask:
        with np.errstate(invalid="ignore"):
            inc &= d > d.dtype.type(thr)
    return inc


def filled_of(d, inc):
    return d if inc is None else np.where(inc, d, np.nan)


def std_atol(family, d):
    """rtol alone, but for `constant`: 8 eps64 max |d| (a ray of equal samples has no spread to be relative to)"""
    return 8 * EPS64 * float(np.nanmax(np.abs(d))) if family == "constant" else 0.0


def all_cases():
    """(family, dtype, shape) of every case"""
    return [(f, dt, s) for f, (_, dts) in FAMILIES.items() for dt in dts for s in SHAPES[dt]]


def case_id(c):
    return "%s-%s-%s" % (c[0], np.dtype(c[1]).name, "x".join(map(str, c[2])))


def counts_fits(shape, seed=0):
    """(bytes of a BITPIX = 32 image with BZERO = 2^30 and BLANK, the float64 cube it means): `counts64` read through a real
    image; the NaN sprinkles are BLANK pixels"""
    from fits_edges import to_payload
    d, _, _ = case("counts64", F64, shape, seed)
    raw = counts_raw(shape, seed).copy()
    raw[np.isnan(d)] = BLANK32
    cards = ["SIMPLE  =                    T", "BITPIX  = %20d" % 32, "NAXIS   =                    3", "NAXIS1  = %20d" % shape[2],
             "NAXIS2  = %20d" % shape[1], "NAXIS3  = %20d" % shape[0], "BSCALE  =                    1", "BZERO   =           1073741824",
             "BLANK   = %20d" % BLANK32, "CTYPE1  = 'RA---TAN'", "CTYPE2  = 'DEC--TAN'", "CTYPE3  = 'VRAD    '", "CUNIT3  = 'km/s    '",
             "CDELT1  =               -1.0E-3", "CDELT2  =                1.0E-3", "CDELT3  =                  0.5", "CRPIX1  =                    1",
             "CRPIX2  =                    1", "CRPIX3  =                    1", "CRVAL1  =                 10.0", "CRVAL2  =                 20.0",
             "CRVAL3  =                -16.0", "BUNIT   = 'K       '"]
    text = "".join(c.ljust(80) for c in cards + ["END"])
    text += " " * ((-len(text)) % 2880)
    payload = to_payload(raw)
    return text.encode("ascii") + payload + b"\0" * ((-len(payload)) % 2880), d


# ---- sigma clipping off zero (the float32 kernels, both loops) ---------------------------------------------------------------
CLIP_PEDESTALS = ((1000.0, 0.5), (-3e4, 2.0), (1e4, 1.0), (250.0, 0.02))
CLIP_NZ = (60, 200, 515)
CLIP_PLANE = (8, 40)
CLIP_CAP = 0.10                 # at most this share of the rays of a case may be left out of the comparison


def clip_cases():
    return [(p, s, nz, masked) for p, s in CLIP_PEDESTALS for nz in CLIP_NZ for masked in (False, True)]


def clip_id(c):
    return "%g+-%g-nz%d-%s" % (c[0], c[1], c[2], "masked" if c[3] else "dense")


@functools.lru_cache(maxsize=None)
def clip_case(pedestal, sd, nz, masked, seed=0, plane=CLIP_PLANE):
    """(float32 cube, bool include or None): pedestal +- sd noise, three outliers of 4 to 40 sigma and two NaN per ray; *masked*:
    a signal mask that leaves at most 128 valid samples per ray (the packed-ray loop takes such rays)"""
    ny, nx = plane
    rng = np.random.default_rng([9, seed, nz, int(masked), int(abs(pedestal))])
    d = pedestal + sd * rng.standard_normal((nz, ny, nx))
    for y in range(ny):
        for x in range(nx):
            z = rng.choice(nz, 5, replace=False)
            d[z[:3], y, x] += sd * rng.uniform(4.0, 40.0, 3) * rng.choice((-1.0, 1.0), 3)
            d[z[3:], y, x] = np.nan
    d = d.astype(np.float32)
    inc = None
    if masked:
        keep = rng.integers(20, 129, size=(ny, nx))
        inc = np.argsort(rng.random((nz, ny, nx)), axis=0) < keep[None]          # `keep` samples of every ray, at random places
    d.setflags(write=False)
    return d, inc


def clip_oracle(d, inc, cenfunc, sigma=3.0, maxiters=5):
    """(O.sigma_clip's result, bool (ny, nx): the rays left out of the comparison).  The kernels' bounds are float32, the
    oracle's float64: a ray is left out when in SOME oracle iteration a valid sample lies within 4 ulp32(|bound|) + 1e-6 std
    of a bound - there the rounding of the bound, not the variance, decides.  The iteration restates O.sigma_clip (asserted)"""
    f = O.filled(d, inc, np.nan).astype(np.float64)
    out_ray = np.zeros(f.shape[1:], bool)
    with np.errstate(invalid="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            for _ in range(maxiters):
                cen = np.nanmedian(f, axis=0) if cenfunc == "median" else np.nanmean(f, axis=0)
                std = np.nanstd(f, axis=0)
                for b in (cen - sigma * std, cen + sigma * std):
                    gap = 4 * np.spacing(np.abs(b).astype(np.float32)).astype(np.float64) + 1e-6 * std
                    out_ray |= (np.abs(f - b) <= gap).any(axis=0)
                out = (f < cen - sigma * std) | (f > cen + sigma * std)
                if not out.any():
                    break
                f[out] = np.nan
    exp = O.sigma_clip(d, inc, sigma, maxiters=maxiters, cenfunc=cenfunc)
    assert np.array_equal(exp, f.astype(np.float32), equal_nan=True), "clip_oracle no longer restates O.sigma_clip"
    return exp, out_ray
