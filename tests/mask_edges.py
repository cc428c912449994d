"""Shared by test_gpu_mask_edges.py (GPU) and test_mask_edges_host.py (CPU): the samples, the masks, the ONE function that
evaluates a mask the way numpy does in the cube's dtype, the cubes that put one special sample in every ray / plane, and
per operator family the float64 reference (oracle_np fed with that include set) with the tolerance of the existing parity
test of the same entry point.  Nothing here touches the GPU.

The NaN rule of the operators without ``nan_excluded`` (every family below), as numpy states it: a mask term is evaluated as
numpy evaluates it (``nan > t`` is False, ``isfinite(nan)`` is False), a mask without such a term follows the array term;
the excluded voxels become NaN (``np.where(include, d, nan)``) and the operator then ignores NaN as the nan-reductions and
astropy's ``nan_treatment='interpolate'`` do - so a sample counts iff ``include & ~isnan(d)`` and an included NaN is never
valid, whatever the mask says.  The resamplers do not ignore NaN: it propagates through every blend that touches it."""
import collections
import functools

import numpy as np

import oracle_np as O
from spectral_cube_amd import _lib as L          # the MASK_* constants only (importing the package may build the library once)
from test_gpu_mask_layer import _masks, _samples

Mask = collections.namedtuple("Mask", "name flags lo hi with_array")
THRESHOLD_FLAGS = L.MASK_GT | L.MASK_GE | L.MASK_LT | L.MASK_LE

# the neighbouring wrong predicates of the host check (test_mask_edges_host.py)
WRONG = ("strictness flipped", "bound one ulp down", "bound one ulp up", "NaN through the threshold", "array term ignored",
         "inf through isfinite")


def samples(dtype):
    """the special samples of the mask-layer test and its plain values, then what the added thresholds need: the smallest
    denormals, dtype(0.1) and both neighbours, the float below max, -max"""
    special, plain = _samples(dtype)
    fi, inf = np.finfo(dtype), dtype(np.inf)
    dn, p1 = fi.smallest_subnormal, dtype(0.1)
    extra = np.array([dn, -dn, p1, np.nextafter(p1, -inf), np.nextafter(p1, inf), np.nextafter(fi.max, -inf), -fi.max], dtype=dtype)
    return np.concatenate([special, plain, extra])


@functools.lru_cache(maxsize=None)
def masks(dtype):
    """the mask-layer test's 11 masks x {without, with} the array term, then 0.0, -0.0, the smallest denormal, 0.1 and max,
    each as > >= < <=, and >= +inf, <= -inf (one infinity each), again without and with the array term"""
    out = [Mask(name, flags, lo, hi, with_array) for name, flags, lo, hi, _, with_array, nan_excluded in _masks() if not nan_excluded]
    fi = np.finfo(dtype)
    thr = [("0.0", 0.0), ("-0.0", -0.0), ("denorm", float(fi.smallest_subnormal)), ("0.1", 0.1), ("max", float(fi.max))]
    cmp_ = [("gt", L.MASK_GT, True), ("ge", L.MASK_GE, True), ("lt", L.MASK_LT, False), ("le", L.MASK_LE, False)]
    added = [("%s %s" % (cn, tn), flag, tv if is_lo else 0.0, 0.0 if is_lo else tv) for tn, tv in thr for cn, flag, is_lo in cmp_]
    added += [("ge +inf", L.MASK_GE, float("inf"), 0.0), ("le -inf", L.MASK_LE, 0.0, -float("inf"))]
    for name, flags, lo, hi in added:
        for with_array in (False, True):
            out.append(Mask(name + (" & array" if with_array else ""), flags, lo, hi, with_array))
    return tuple(out)


def include(d, arr, m, wrong=None):
    """THE include set: numpy's own evaluation of mask *m* on *d*, thresholds in the cube's dtype.  *wrong*: one of WRONG,
    the same mask as a subtly wrong kernel would evaluate it (host check only)"""
    t = d.dtype.type
    flags, lo, hi = m.flags, t(m.lo), t(m.hi)
    if wrong == "strictness flipped":
        swap = {L.MASK_GT: L.MASK_GE, L.MASK_GE: L.MASK_GT, L.MASK_LT: L.MASK_LE, L.MASK_LE: L.MASK_LT}
        flags = (flags & ~THRESHOLD_FLAGS) | sum(v for k, v in swap.items() if flags & k)
    if wrong in ("bound one ulp down", "bound one ulp up"):
        to = t(-np.inf if wrong.endswith("down") else np.inf)
        with np.errstate(over="ignore"):
            lo, hi = np.nextafter(lo, to), np.nextafter(hi, to)
    inc = np.ones(d.shape, bool)
    with np.errstate(invalid="ignore"):
        if flags & L.MASK_FINITE:
            inc &= ~np.isnan(d) if wrong == "inf through isfinite" else np.isfinite(d)
        if flags & L.MASK_GT:
            inc &= d > lo
        if flags & L.MASK_GE:
            inc &= d >= lo
        if flags & L.MASK_LT:
            inc &= d < hi
        if flags & L.MASK_LE:
            inc &= d <= hi
    if wrong == "NaN through the threshold" and flags & THRESHOLD_FLAGS:
        inc |= np.isnan(d)
    if m.with_array and wrong != "array term ignored":
        inc &= arr != 0
    return inc


def wrong_case(d, arr, m, wrong):
    """(data, include set) as the wrong predicate sees them, or None when it includes exactly what the right one does.  A NaN
    that a wrong kernel takes for valid poisons every sum it enters; the oracle would skip it, so it enters as +inf here"""
    inc, bad = include(d, arr, m), include(d, arr, m, wrong)
    if np.array_equal(inc, bad):
        return None
    leak = bad & ~inc & np.isnan(d)
    if leak.any():
        d = d.copy()
        d[leak] = np.inf
    return d, bad


# ---- cubes -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ray_cube(dtype, shape, axis, lines=False, no_max=False, const=False):
    """(cube, array term): ONE special sample per ray along *axis*, sample (r mod 20) in ray r at a position that moves with r.
    Rays come in four kinds, 20 each in turn: a background of 0.25 and 2.0 in a checkerboard (exactly representable, every
    partial sum exact in float64 whatever the order) with the array term set / clear at the special sample, then the same
    two with a NaN background (the special sample alone decides whether the ray is empty).  *lines*: the array term is also
    clear on the whole aligned group of four x around the sample, so that the mask-first loads skip those cube lines.
    *no_max*: max, the float below it and -max give way to 0.5, 0.75 and -0.5 (see GLOBAL_CASES).  *const*: two more kinds, a
    ray that holds the special sample at EVERY position, the array term set / clear all along it - what an interpolation
    needs: it blends neighbours, and under most masks one of two background values is excluded (see RESAMPLE_CASES)"""
    s = samples(dtype)
    if no_max:
        s = s.copy()
        s[np.isfinite(s) & (np.abs(s) > 1e30)] = np.array([0.5, 0.75, -0.5], dtype=dtype)
    ns, n = s.size, shape[axis]
    other = tuple(shape[a] for a in range(3) if a != axis)
    nr = other[0] * other[1]
    nk = 6 if const else 4
    assert nr >= nk * ns, "every sample needs a ray of each kind"
    pos, r = np.arange(n)[:, None], np.arange(nr)[None, :]
    kind = (r[0] // ns) % nk
    a = np.where((pos + r) % 2 == 0, dtype(0.25), dtype(2.0)).astype(dtype)
    a[:, (kind == 2) | (kind == 3)] = np.nan
    p = 1 + (3 * r[0] + r[0] // 5) % (n - 1)          # never 0: what argmax / argmin give for an empty ray
    a[p, r[0]] = s[r[0] % ns]
    arr = np.ones((n, nr), np.uint8)
    off = kind % 2 == 1
    arr[p[off], r[0][off]] = 0
    a[:, kind >= 4] = s[r[0] % ns][kind >= 4]
    arr[:, kind == 5] = 0
    if lines:
        assert axis == 0 and shape[2] % 4 == 0
        for k in range(4):
            arr[p[off], (r[0][off] & ~3) + k] = 0
    d = np.ascontiguousarray(np.moveaxis(a.reshape((n,) + other), 0, axis))
    arr = np.ascontiguousarray(np.moveaxis(arr.reshape((n,) + other), 0, axis))
    d.setflags(write=False)
    arr.setflags(write=False)
    return d, arr


@functools.lru_cache(maxsize=None)
def plane_cube(dtype, shape, const=False, pairs=False):
    """(cube, array term): ONE special sample per plane, sample (z mod 20) at a spot that moves with z, the four kinds of
    ray_cube per plane: no window of a 2-D stencil ever holds two special samples.  *pairs*: every plane twice in a row, for the
    operator that also blends neighbouring planes"""
    if pairs:
        d, arr = plane_cube(dtype, (shape[0] // 2,) + tuple(shape[1:]), const)
        d, arr = np.repeat(d, 2, axis=0), np.repeat(arr, 2, axis=0)
        d.setflags(write=False)
        arr.setflags(write=False)
        return d, arr
    s = samples(dtype)
    ns = s.size
    nz, ny, nx = shape
    nk = 6 if const else 4                  # (*const*: planes that hold the sample everywhere, as in ray_cube)
    assert nz >= nk * ns
    z, y, x = np.arange(nz)[:, None, None], np.arange(ny)[None, :, None], np.arange(nx)[None, None, :]
    d = np.where((y + x + z) % 2 == 0, dtype(0.25), dtype(2.0)).astype(dtype)
    zz = np.arange(nz)
    kind = (zz // ns) % nk
    d[(kind == 2) | (kind == 3)] = np.nan
    py, px = (3 * zz + 1) % ny, (5 * zz + 2) % nx
    d[zz, py, px] = s[zz % ns]
    arr = np.ones(shape, np.uint8)
    off = kind % 2 == 1
    arr[zz[off], py[off], px[off]] = 0
    d[kind >= 4] = s[zz % ns][kind >= 4, None, None]
    arr[kind == 5] = 0
    d.setflags(write=False)
    arr.setflags(write=False)
    return d, arr


@functools.lru_cache(maxsize=None)
def flat_cube(dtype, shape):
    """(cube, array term) in the layout of the mask-layer test: the samples repeat along the flat index (20 of them: coprime
    to the odd extents), the array term is clear at the first copy of each"""
    s = samples(dtype)
    n = int(np.prod(shape))
    d = s[np.arange(n) % s.size].reshape(shape)
    arr = np.ones(shape, np.uint8)
    arr.reshape(-1)[:s.size] = 0
    d.setflags(write=False)
    arr.setflags(write=False)
    return d, arr


# ---- tolerances: a reference gives, per output, (expected, [(selection, atol, rtol), ...]); atol None = exact --------------
def _all(e):
    return np.ones(np.shape(e), bool)


def exact(e):
    return np.asarray(e), [(_all(e), None, 0.0)]


def within(e, atol, rtol=0.0, where=None):
    return np.asarray(e), [(_all(e) if where is None else where, atol, rtol)]


def of_max(e, frac, rtol=0.0):
    """atol = frac * max |expected|, the form of the parity tests - taken apart for the outputs that hold the dtype's max
    (above 1e30) and for the rest, so that one huge sample does not loosen the check of every other output: each group is
    held to frac of ITS largest finite value, never more than frac of the whole map's"""
    e = np.asarray(e)
    e64 = e.astype(np.float64)
    fin = np.isfinite(e64)
    big = fin & (np.abs(e64) > 1e30)
    groups = []
    for sel in (big, ~big):
        f = sel & fin
        groups.append((sel, frac * (np.abs(e64[f]).max() if f.any() else 0.0), rtol))
    return e, groups


def _infs(a):
    """+1 / -1 where *a* is +inf / -inf, 0 elsewhere (NaN too)"""
    a = np.asarray(a, np.float64)
    return np.where(np.isposinf(a), 1, 0) - np.where(np.isneginf(a), 1, 0)


def check(got, ref, what):
    """the GPU result against a reference of this module: NaN and inf patterns exactly, the rest per group"""
    from conftest import assert_close
    for name, (e, groups) in ref.items():
        g = np.asarray(got[name])
        assert g.shape == e.shape, (what, name, g.shape, e.shape)
        for kind, a, b in (("NaN", np.isnan(g), np.isnan(e)), ("inf", _infs(g), _infs(e))):
            bad = np.argwhere(a != b)
            assert not len(bad), "%s: %s %s pattern differs at %d places, first %s: got %s, expected %s" % (
                what, name, kind, len(bad), bad[:6].tolist(), [g[tuple(i)] for i in bad[:6]], [e[tuple(i)] for i in bad[:6]])
        for sel, atol, rtol in groups:
            if atol is None:
                bad = np.argwhere(sel & ~((g == e) | ((g != g) & (e != e))))
                assert not len(bad), "%s: %s differs at %d places, first %s: got %s, expected %s" % (
                    what, name, len(bad), bad[:6].tolist(), [g[tuple(i)] for i in bad[:6]], [e[tuple(i)] for i in bad[:6]])
            else:
                with np.errstate(all="ignore"):
                    assert_close(g[sel], e[sel], rtol=rtol, atol=atol, what="%s: %s" % (what, name))


def differs(ref, bad, factor=100.0):
    """True when reference *bad* (a wrong predicate's) misses *ref* by more than *factor* x the tolerance in some output, or
    in a NaN / inf pattern, or in an exact (integer, selected) output"""
    for name, (e, groups) in ref.items():
        e, b = np.asarray(e, np.float64), np.asarray(bad[name][0], np.float64)
        if not np.array_equal(np.isnan(e), np.isnan(b)) or not np.array_equal(_infs(e), _infs(b)):
            return True
        for sel, atol, rtol in groups:
            fin = sel & np.isfinite(e) & np.isfinite(b)
            err = np.abs(e[fin] - b[fin])
            if atol is None:
                if (err > 0).any():
                    return True
            elif (err > factor * (atol + rtol * np.abs(e[fin]))).any():
                return True
    return False


# ---- references ----------------------------------------------------------------------------------------------------------------
def spectral_centres(nz):
    """channel centres for the moments: dyadic (products with the samples are exact in float64), never zero (inf * 0 would be
    a NaN that nansum skips and a plain sum does not), span nz / 64"""
    return (np.arange(nz) + 0.5 - nz / 2) / 64.0


M1_ADD = 2.0


def dv_of(dtype):
    """the channel width of the moments: 0.5 for float32 cubes; 1.0 for float64 ones, where the reference's own
    ``d * pix_size`` underflows to 0 for the smallest denormal (its first moment is then 0 / 0, the kernel's sum(v c) / sum(v)
    is not): the configuration that keeps the reference exact, not another tolerance"""
    return 0.5 if np.dtype(dtype) == np.float32 else 1.0


def _valid(d, inc):
    return inc & ~np.isnan(d)


def _extrema(d, inc, axis):
    with np.errstate(all="ignore"):
        v = _valid(d, inc)
        vmax = np.where(v.any(axis=axis), np.max(np.where(v, d, -np.inf), axis=axis), np.nan).astype(d.dtype)
        vmin = np.where(v.any(axis=axis), np.min(np.where(v, d, np.inf), axis=axis), np.nan).astype(d.dtype)
    return vmax, vmin


def ref_moments(d, inc, want):
    """ops.moments / ops.moments_f64 along axis 0.  float32: m0 exact (see ray_cube), m1 and m2 at the bounds of
    test_mask_first_is_bit_identical (1e-9 span, 1e-8 span^2; no ray here has the small m0 that test sets aside);
    float64: test_moments_f64 of test_gpu_round4.py (1e-13; its third moment 1e-12)"""
    nz = d.shape[0]
    cen, span = spectral_centres(nz), nz / 64.0
    wide = d.dtype == np.float64
    out = {}
    with np.errstate(all="ignore"):
        for o in range(3):
            if "m%d" % o in want:
                e = O.moment(d, inc, o, cen, dv_of(d.dtype), world0=M1_ADD)
                if wide:
                    out["m%d" % o] = within(e, 1e-13, 1e-13)
                else:
                    out["m%d" % o] = exact(e) if o == 0 else within(e, (1e-9 * span) if o == 1 else (1e-8 * span * span))
    if "nvalid" in want:
        out["nvalid"] = exact(_valid(d, inc).sum(axis=0).astype(np.int32))
    if "argmax" in want:
        out["argmax"], out["argmin"] = exact(O.argmax(d, _valid(d, inc))), exact(O.argmin(d, _valid(d, inc)))
        vmax, vmin = _extrema(d, inc, 0)
        out["vmax"], out["vmin"] = exact(vmax), exact(vmin)
    return out


def ref_moment_order(d, inc, order=3):
    """ops.moment_order / moment_order_f64: test_moment_order (rtol 1e-9, atol 1e-9 max) / test_moments_f64 (1e-12)"""
    with np.errstate(all="ignore"):
        e = O.moment(d, inc, order, spectral_centres(d.shape[0]), 1.0)
    return {"m%d" % order: within(e, 1e-12, 1e-12) if d.dtype == np.float64 else of_max(e, 1e-9, 1e-9)}


def spatial_centres(shape, axis):
    ny, nx = shape[1:]
    n = shape[axis]
    c = (np.arange(n) + 0.5 - n / 2) / 64.0
    return np.ascontiguousarray(np.broadcast_to(c[:, None] if axis == 1 else c[None, :], (ny, nx)))


def ref_moments_spatial(d, inc, axis):
    """ops.moments_spatial and moment_order_spatial (order 3): test_moments_spatial_axes (rtol 1e-9, atol 1e-7 max)"""
    cen = spatial_centres(d.shape, axis)
    out = {}
    with np.errstate(all="ignore"):
        for o in (0, 1, 2, 3):
            out["m%d" % o] = of_max(O.moment(d, inc, o, cen[None], dv_of(d.dtype), axis=axis), 1e-7, 1e-9)
    return out


def ref_argextrema(d, inc, axis):
    v = _valid(d, inc)
    return {"argmax": exact(O.argmax(d, v, axis)), "argmin": exact(O.argmin(d, v, axis))}


def ref_stats_axis(d, inc, axis):
    """ops.stats_axis (axis 0, 1, 2; an empty ray sums to NaN) and stats_planes (axis (1, 2); an empty plane sums to 0):
    test_stats_global_and_axes and test_stats_planes - count, min, max exact, sum and sumsq rtol 1e-12"""
    empty = np.nan if isinstance(axis, int) else 0.0
    v = _valid(d, inc)
    f = np.where(v, d, 0).astype(np.float64)
    cnt = v.sum(axis=axis)
    vmax, vmin = _extrema(d, inc, axis)
    with np.errstate(all="ignore"):
        return {"count": exact(cnt.astype(np.int32)), "min": exact(vmin), "max": exact(vmax),
                "sum": within(np.where(cnt > 0, f.sum(axis=axis), empty), 0.0, 1e-12),
                "sumsq": within(np.where(cnt > 0, (f * f).sum(axis=axis), empty), 0.0, 1e-12)}


def ref_stats_global(d, inc):
    """ops.stats_global: O.statistics, as test_stats_global_and_axes holds it (npts, min, max exact; sum, sumsq rel 1e-12)"""
    with np.errstate(all="ignore"):
        st = O.statistics(d, inc)
    return {"npts": exact(np.float64(st["npts"])), "min": exact(np.float64(st["min"])), "max": exact(np.float64(st["max"])),
            "sum": within(np.float64(st["sum"]), 0.0, 1e-12), "sumsq": within(np.float64(st["sumsq"]), 0.0, 1e-12)}


def ref_spectral_conv(d, inc, kernel):
    """ops.spectral_conv: test_spectral_conv_vs_oracle (atol 1e-5 max)"""
    with np.errstate(all="ignore"):
        return {"out": of_max(O.spectral_smooth(d, inc, kernel), 1e-5)}


def ref_spectral_conv_moments(d, inc, kernel):
    """ops.spectral_conv_moments: test_spectral_conv_moments_fused - the smoothed cube under the ORIGINAL mask; m0 1e-5 max, m1
    1e-5 span, m2 1e-5 max where |m0| > 1e-2 max (that test's well-conditioned rays), its NaN pattern everywhere"""
    nz = d.shape[0]
    cen = spectral_centres(nz)
    with np.errstate(all="ignore"):
        sm = O.spectral_smooth(d, inc, kernel)
        e0, e1, e2 = O.moments012(sm, inc, cen, dv_of(d.dtype), M1_ADD)
        fin0 = np.isfinite(e0)
        small = fin0 & (np.abs(e0) <= 1e30)
        top = np.abs(e0[small]).max() if small.any() else 0.0
        wc = np.isfinite(e2) & small & (np.abs(e0) > 1e-2 * top)
        return {"m0": of_max(e0, 1e-5), "m1": within(e1, 1e-5 * nz / 64.0),
                "m2": within(e2, 1e-5 * (np.abs(e2[wc]).max() if wc.any() else 0.0), where=wc)}


def ref_spatial_conv(d, inc, kernel2d):
    """ops.spatial_conv: test_spatial_conv_sep_vs_oracle and its kin (atol 1e-5 max)"""
    with np.errstate(all="ignore"):
        return {"out": of_max(O.spatial_smooth(d, inc, kernel2d), 1e-5)}


def lerp_axes(nz, shift):
    x = np.arange(nz, dtype=np.float64)
    return x, x[:nz - 1] + shift


def ref_spectral_lerp(d, inc, shift):
    """ops.spectral_lerp: test_spectral_lerp (atol 1e-5 max)"""
    x, grid = lerp_axes(d.shape[0], shift)
    with np.errstate(all="ignore"):
        e, _ = O.spectral_interpolate(d, inc, x, grid, out_dtype=d.dtype)
    return {"out": of_max(e, 1e-5)}


def bilinear_maps(shape, shift):
    yy, xx = np.mgrid[0:shape[1], 0:shape[2]].astype(np.float64)
    return xx + shift, yy + shift


def ref_resample_bilinear(d, inc, shift):
    """ops.resample_bilinear: test_resample_bilinear (atol 1e-5 max, the footprint exact)"""
    xs, ys = bilinear_maps(d.shape, shift)
    with np.errstate(all="ignore"):
        e, foot = O.resample_bilinear(O.filled(d, inc), xs, ys)
    return {"out": of_max(e.astype(d.dtype), 1e-5), "foot": exact(foot[0].astype(np.uint8))}


def ref_resample_bilinear_lerp(d, inc, shift):
    """ops.resample_bilinear_lerp: O.resample_bilinear of the filled cube, then O.spectral_interpolate of its planes, at the
    1e-5 max of test_bilinear_lerp_equals_the_two_passes (test_gpu_round5.py); the footprint exact"""
    xs, ys = bilinear_maps(d.shape, shift)
    x, grid = lerp_axes(d.shape[0], shift)
    with np.errstate(all="ignore"):
        planes, foot = O.resample_bilinear(O.filled(d, inc), xs, ys)
        # the resampled planes in the cube's dtype, as the reprojected cube is: the interpolation then takes the difference of
        # two neighbours in that dtype (scipy's _call_linear on a float32 y, which O.spectral_interpolate restates by keeping
        # the dtype of its data), so max next to -max gives -inf there, as in the kernel
        e, _ = O.spectral_interpolate(planes.astype(d.dtype), None, x, grid, out_dtype=d.dtype)
    return {"out": of_max(e, 1e-5), "foot": exact(foot[0].astype(np.uint8))}


# ---- kernels of the stencil cases ---------------------------------------------------------------------------------------------
def taps(n, sym=True, zero_centre=False):
    """n positive taps around a broad peak (every tap carries weight, so a sample that enters or leaves a window moves it by far
    more than the tolerance), optionally lopsided or with a zero centre tap"""
    k = np.hanning(n + 2)[1:-1] + 0.25
    if not sym:
        k = k * np.linspace(0.5, 1.5, n)
    if zero_centre:
        k[n // 2] = 0.0
    return k / k.sum()          # sum 1: the float32 stencils form sum(k v) in float32, which max times a tap above 1 leaves


# (operator, path, dtype, shape, parameters): the table both test files walk.  Shapes: see the docstring of
# test_gpu_mask_edges.py for the dispatch rule that each one meets
F32, F64 = np.float32, np.float64
SUMS, COUNT, EXTREMA = ("m0", "m1", "m2"), ("m0", "m1", "m2", "nvalid"), ("m0", "m1", "m2", "nvalid", "argmax", "argmin", "vmax", "vmin")
Case = collections.namedtuple("Case", "op path dtype shape par")

MOMENT_CASES = [Case("moments", path, F32, shape, (want, lines))
                for path, shape, lines in (("one spaxel per lane (odd nx)", (40, 12, 7), False),
                                           ("two spaxels per lane (nx % 4 == 2)", (40, 9, 10), False),
                                           ("four spaxels per lane, mask-first with a mask array", (40, 8, 16), False),
                                           ("four per lane, whole mask dwords clear at the samples (lines never loaded)", (40, 8, 16), True),
                                           ("z split in four + combine kernel (nz >= 256, small map)", (256, 6, 16), False))
                for want in (SUMS, COUNT, EXTREMA)]
MOMENT_CASES += [Case("moments_f64", path, F64, shape, (EXTREMA, False))
                 for path, shape in (("one spaxel per lane (odd nx)", (40, 12, 7)), ("two spaxels per lane (even nx)", (40, 8, 16)))]
ORDER_CASES = [Case("moment_order", "scalar kernel (spc_pred)", F32, (40, 12, 7), None),
               Case("moment_order", "v4 kernel (spc_pred_valid)", F32, (40, 8, 16), None),
               Case("moment_order_f64", "odd nx", F64, (40, 12, 7), None), Case("moment_order_f64", "even nx", F64, (40, 8, 16), None)]
SPATIAL_MOMENT_CASES = [Case("moments_spatial", "axis %d, %s" % (axis, path), F32, shape, axis)
                        for axis in (1, 2) for path, shape in (("odd nx", (12, 12, 7) if axis == 1 else (12, 7, 13)),
                                                               ("nx % 4 == 0", (7, 12, 16)))]
ARGEXTREMA_CASES = [Case("argextrema_axis", "axis %d, %s" % (axis, path), F32, shape, axis)
                    for axis in (1, 2) for path, shape in (("odd nx", (12, 12, 7) if axis == 1 else (12, 7, 13)), ("nx % 4 == 0", (7, 12, 16)))]
STATS_CASES = [Case("stats_axis", "axis %d, %s" % (axis, path), dtype, shape, axis)
               for dtype in (F32, F64) for axis in (0, 1, 2)
               for path, shape in (("ragged rows (nx = 67)", {0: (5, 3, 67), 1: (3, 5, 67), 2: (3, 27, 67)}[axis]),
                                   ("contiguous groups (nx = 16)", {0: (8, 8, 16), 1: (10, 8, 16), 2: (8, 10, 16)}[axis]))]
STATS_CASES += [Case("stats_planes", path, F32, shape, (1, 2)) for path, shape in (("ragged rows", (3, 27, 67)), ("aligned rows", (8, 10, 16)))]
# stats_global of a float64 cube holds every sample in ONE float64 sum: max + (max - 1 ulp) - max overflows or not with the
# order of the additions, in numpy's pairwise sum as in the kernel's tree - the reference itself overflows in the cube's
# dtype, so these two cases leave the three samples of magnitude max out.  (A float32 cube is summed in float64: nothing
# overflows, nothing is left out; along an axis every ray holds one such sample.)
GLOBAL_CASES = [Case("stats_global", path, dtype, shape, None) for dtype in (F32, F64)
                for path, shape in (("ragged tail", (3, 27, 67)), ("aligned", (8, 10, 16)))]

SPECTRAL_CASES = [
    Case("spectral_conv", "9-tap ring; general kernel under a threshold, fast pass + redo under isfinite", F32, (40, 9, 9), taps(9)),
    Case("spectral_conv", "17-tap ring, two spaxels per lane", F32, (40, 8, 10), taps(17)),
    Case("spectral_conv", "33-tap ring", F32, (40, 9, 9), taps(33)),
    Case("spectral_conv", "no ring (zero centre tap), 7 taps: per-output loop (spc_pred)", F32, (40, 9, 9), taps(7, zero_centre=True)),
    Case("spectral_conv", "35 lopsided taps: runs-of-16 kernel, numerator-only pass first under isfinite", F32, (48, 8, 10), taps(35, sym=False)),
    Case("spectral_conv", "41 symmetric taps: all-valid 49 ring first under isfinite, wide ring after", F32, (48, 8, 10), taps(41)),
    Case("spectral_conv", "9-tap ring split in two along z (nz >= 8 R)", F32, (80, 9, 9), taps(9)),
    Case("spectral_conv", "float64, 9-tap ring", F64, (40, 9, 9), taps(9)),
    Case("spectral_conv", "float64, 33-tap ring", F64, (40, 8, 10), taps(33)),
    Case("spectral_conv", "float64, zero centre tap", F64, (40, 9, 9), taps(7, zero_centre=True)),
]
FUSED_CASES = [Case("spectral_conv_moments", "9-tap ring", F32, (40, 9, 9), taps(9)),
               Case("spectral_conv_moments", "33-tap ring, two spaxels per lane", F32, (40, 8, 10), taps(33))]     # (no ring, no fused form)


def _k2(ny, nx, separable=True):
    k = np.outer(taps(ny), taps(nx))
    if not separable:
        k = k + np.linspace(0.0, 0.1 / (ny * nx), ny * nx).reshape(ny, nx)
    return k / k.sum()


# spatial_conv: par = (kernel, arithmetic)
SPATIAL_CASES = [
    Case("spatial_conv", "9-tap separable ring (f32 form), nx < 64: no fast pass", F32, (80, 12, 14), (_k2(9, 9), "f32")),
    Case("spatial_conv", "9-tap separable ring (f32 form), nx = 64: fast pass + redo under isfinite", F32, (80, 10, 64), (_k2(9, 9), "f32")),
    Case("spatial_conv", "17-tap separable ring (f32 form)", F32, (80, 18, 20), (_k2(17, 17), "f32")),
    Case("spatial_conv", "default form: split (matrix cores) under array (+ isfinite), ring otherwise", F32, (80, 12, 14), (_k2(9, 9), None)),
    Case("spatial_conv", "two-pass wide form (67 x 3 taps) on a plane just larger", F32, (80, 70, 8), (_k2(67, 3), None)),
    Case("spatial_conv", "tiled 2-D (9 x 3, not separable), all-valid pass under isfinite", F32, (80, 12, 14), (_k2(9, 3, False), None)),
    Case("spatial_conv", "generic 2-D (3 x 3, not separable)", F32, (80, 7, 9), (_k2(3, 3, False), None)),
    Case("spatial_conv", "separable, zero centre tap: the filled centre under an empty window", F32, (80, 7, 9),
         (np.outer(taps(3, zero_centre=True), taps(3, zero_centre=True)), "f32")),
    Case("spatial_conv", "float64 separable ring", F64, (80, 12, 14), (_k2(9, 9), None)),
    Case("spatial_conv", "float64 2-D (3 x 3, not separable)", F64, (80, 7, 9), (_k2(3, 3, False), None)),
]
# the resamplers blend neighbours: a special sample between two background values shows only under the masks that keep both,
# so these cubes also hold rays / planes that are the sample throughout (120 rays / planes: six kinds of 20)
# par = (shift, library switches): SPC_BILINEAR_LDS=0 sends every tile to the gather kernel (otherwise it only redoes flagged
# tiles, and nothing here flags one), SPC_LERP_TILES=0 takes spectral_lerp off its tiled form - as test_gpu_ops.py and
# test_gpu_round2.py force them.  resample_bilinear_lerp blends neighbouring planes too: its cube holds every plane twice
RESAMPLE_CASES = [Case(op, "%s%s, %s" % (path, "".join(", %s=%s" % kv for kv in env), "identity" if shift == 0.0 else "half-sample shift"),
                       dtype, shape, (shift, env))
                  for op, dtype, path, shape, env in (
                      ("spectral_lerp", F32, "odd nx", (40, 11, 11), ()), ("spectral_lerp", F32, "nx % 4 == 0", (40, 8, 16), ()),
                      ("spectral_lerp", F32, "nx % 4 == 0", (40, 8, 16), (("SPC_LERP_TILES", "0"),)),
                      ("spectral_lerp", F64, "float64", (40, 11, 11), ()),
                      ("resample_bilinear", F32, "LDS-staged kernel", (120, 9, 11), ()),
                      ("resample_bilinear", F32, "gather kernel", (120, 9, 11), (("SPC_BILINEAR_LDS", "0"),)),
                      ("resample_bilinear", F64, "float64", (120, 9, 11), ()),
                      ("resample_bilinear_lerp", F32, "LDS-staged kernel, LERP", (240, 9, 11), ()),
                      ("resample_bilinear_lerp", F32, "gather kernel, LERP", (240, 9, 11), (("SPC_BILINEAR_LDS", "0"),)))
                  for shift in (0.0, 0.5)]

CASES = (MOMENT_CASES + ORDER_CASES + SPATIAL_MOMENT_CASES + ARGEXTREMA_CASES + STATS_CASES + GLOBAL_CASES + SPECTRAL_CASES + FUSED_CASES
         + SPATIAL_CASES + RESAMPLE_CASES)


# What no data can show (the host check counts these with the identical ones).  WEIGHTS_ONLY: every output is a weighted sum
# over a sum of weights - a sample equal to zero weighs nothing in either, an infinite or NaN sample makes the quotient NaN,
# which is what a ray without a valid sample gives too; a wrong predicate that moves only such samples shows in the counts
# and sums of the pass that feeds these operators (ops.moments), not in them.  BLENDS: a NaN or infinite sample blended with a
# NaN neighbour, or with itself (inf - inf), is NaN whether the mask kept it or not.
WEIGHTS_ONLY = ("moment_order", "moment_order_f64")
BLENDS = ("spectral_lerp", "resample_bilinear", "resample_bilinear_lerp")


def cannot_show(op, moved):
    """True when a wrong predicate that moved exactly the samples *moved* in or out cannot change any output of *op*"""
    if op in WEIGHTS_ONLY:
        return bool(((moved == 0) | ~np.isfinite(moved)).all())
    return op in BLENDS and bool((~np.isfinite(moved)).all())


def case_id(c):
    return "%s-%s-%s-%s" % (c.op, np.dtype(c.dtype).name, "x".join(map(str, c.shape)), c.path.split(":")[0].split(",")[0].replace(" ", "_")[:40])


def case_data(c):
    """(cube, array term) of a case"""
    if c.op in ("moments", "moments_f64"):
        return ray_cube(c.dtype, c.shape, 0, c.par[1])
    if c.op in ("moments_spatial", "argextrema_axis", "stats_axis"):
        return ray_cube(c.dtype, c.shape, c.par)
    if c.op in ("stats_planes", "stats_global"):
        return ray_cube(c.dtype, c.shape, 2, no_max=c.op == "stats_global" and c.dtype == F64)
    if c.op in ("spatial_conv", "resample_bilinear", "resample_bilinear_lerp"):
        return plane_cube(c.dtype, c.shape, c.op != "spatial_conv", c.op == "resample_bilinear_lerp")
    return ray_cube(c.dtype, c.shape, 0, const=c.op == "spectral_lerp")


def case_ref(c, d, inc):
    """the reference of a case for include set *inc*"""
    if c.op in ("moments", "moments_f64"):
        return ref_moments(d, inc, c.par[0])
    if c.op in ("moment_order", "moment_order_f64"):
        return ref_moment_order(d, inc)
    if c.op == "moments_spatial":
        return ref_moments_spatial(d, inc, c.par)
    if c.op == "argextrema_axis":
        return ref_argextrema(d, inc, c.par)
    if c.op in ("stats_axis", "stats_planes"):
        return ref_stats_axis(d, inc, c.par)
    if c.op == "stats_global":
        return ref_stats_global(d, inc)
    if c.op == "spectral_conv":
        return ref_spectral_conv(d, inc, c.par)
    if c.op == "spectral_conv_moments":
        return ref_spectral_conv_moments(d, inc, c.par)
    if c.op == "spatial_conv":
        return ref_spatial_conv(d, inc, c.par[0])
    return {"spectral_lerp": ref_spectral_lerp, "resample_bilinear": ref_resample_bilinear,
            "resample_bilinear_lerp": ref_resample_bilinear_lerp}[c.op](d, inc, c.par[0])


class RefCache:
    """references of one case by include set: many masks (and most wrong predicates) include the same voxels"""

    def __init__(self, c):
        self.c, self.d, self.arr = c, *case_data(c)
        self.memo = {}

    def ref(self, d, inc):
        key = (inc.tobytes(), None if d is self.d else d.tobytes())
        if key not in self.memo:
            self.memo[key] = case_ref(self.c, d, inc)
        return self.memo[key]

    def expected(self, m):
        return self.ref(self.d, include(self.d, self.arr, m))


# ---- the order-statistics cases of test_order_statistics_mask_predicates_as_key_intervals (test_gpu_round2.py), for the
# operators that share its key-interval test but are not in it ---------------------------------------------------------------
def order_statistic_data(dtype=np.float32):
    """that test's cube: seeded normal samples, 40 % replaced by its special values"""
    rng = np.random.default_rng(77)
    d = rng.standard_normal((96, 3, 40)).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, -1e-45, 1e38, -1e38, 0.3, -0.3], np.float32)
    pick = rng.random(d.shape) < 0.4
    d[pick] = special[rng.integers(0, len(special), int(pick.sum()))]
    return d.astype(dtype)


def order_statistic_masks():
    """that test's masks as (flags, lo, hi)"""
    one = (L.MASK_GT, L.MASK_GE, L.MASK_LT, L.MASK_LE)
    thr = [0.0, -0.0, np.inf, -np.inf, np.nan, 1e-45, 3.4028235e38, 0.3, -0.3]
    out = [(f, t, 0.0) if f in (L.MASK_GT, L.MASK_GE) else (f, 0.0, t) for f in one for t in thr]
    out += [(L.MASK_GT | L.MASK_LT, -0.3, 0.3), (L.MASK_GE | L.MASK_LE, -0.0, 0.0), (L.MASK_GE | L.MASK_LT, 0.0, np.inf),
            (L.MASK_GT | L.MASK_LE | L.MASK_FINITE, -np.inf, np.inf), (L.MASK_FINITE, 0.0, 0.0), (0, 0.0, 0.0)]
    return [Mask("flags %d, lo %r, hi %r" % m, m[0], m[1], m[2], False) for m in out]
