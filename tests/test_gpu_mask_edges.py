"""The mask predicate at its edges, through every hot-path operator that takes a mask: 66 masks per case (the 11 of
test_gpu_mask_layer.py and > >= < <= against 0.0, -0.0, the smallest denormal, 0.1, max, >= +inf, <= -inf; each without and
with the array term) on cubes that hold NaN, +-inf, +-0, +-denormal, the thresholds, their neighbouring floats and +-max.
The expected include set is numpy's own evaluation in the cube's dtype (mask_edges.include, the one place), the expected
result is oracle_np in float64 fed with it, the tolerance is that of the existing parity test of the same entry point
(named beside each reference in mask_edges.py) - and test_mask_edges_host.py shows on the CPU that every neighbouring wrong
predicate misses that tolerance by a factor of 100, changes a NaN / inf pattern or an exact output.

Every cube has ONE special sample per ray (reductions, spectral stencils, spectral interpolation) or per plane (spatial
stencils, reprojection) in a background of 0.25 and 2.0 - sums of it are exact in float64 in any order - or of NaN, with
the array term set or clear at the sample: 20 samples x 4 kinds = 80 rays / planes at least.  No sample is left out of any
operator: the oracle computes in float64, where max overflows nowhere (the float64 cubes give inf where the reference's
own float64 arithmetic does, compared as a pattern).

Dispatch paths and the shapes that reach them (mask_edges.CASES; all 66 masks run on each, a path taken only under some
masks is named with them):
  moments (spc_moments_f32), each as sums / + nvalid / + extrema
    (40, 12, 7)   odd nx: one spaxel per lane
    (40, 9, 10)   nx % 4 == 2: two spaxels per lane
    (40, 8, 16)   four spaxels per lane; with the array term the mask-first march, special samples under kept dwords
    (40, 8, 16)*  the same with whole mask dwords clear around the samples: their cube lines are never loaded
    (256, 6, 16)  nz >= 256 on a small map: z split in four and the combine kernel
  moment_order            (40, 12, 7) scalar kernel (spc_pred), (40, 8, 16) v4 kernel (spc_pred_valid)
  moments_f64, moment_order_f64        (40, 12, 7) one spaxel per lane, (40, 8, 16) two
  moments_spatial + moment_order_spatial, argextrema_axis     axis 1: (12, 12, 7), axis 2: (12, 7, 13) scalar; (7, 12, 16) vector
  stats_axis (float32, float64; the one-compare form under none / isfinite / array, three compares under a threshold)
    axis 0 (5, 3, 67) / (8, 8, 16), axis 1 (3, 5, 67) / (10, 8, 16), axis 2 (3, 27, 67) / (8, 10, 16): ragged rows / contiguous groups
  stats_planes, stats_global           (3, 27, 67) ragged tail, (8, 10, 16) aligned
  spectral_conv
    (40, 9, 9)  9 taps, (40, 8, 10) 17 taps, (40, 9, 9) 33 taps: the rings - general kernel under a threshold or the array
                term, speculative fast pass + redo of flagged tiles under none / isfinite
    (40, 9, 9)  7 taps, zero centre: no ring, per-output loop (spc_pred); an empty window gives the filled centre
    (48, 8, 10) 35 lopsided taps: runs-of-16 kernel (numerator-only pass first under none / isfinite)
    (48, 8, 10) 41 symmetric taps: all-valid 49 ring first under none / isfinite; the rest by the wide 49 ring under a mask
                with isfinite, by the runs-of-16 kernel under one that lets +-inf through (the kernel does not fill the ring)
    (80, 9, 9)  9 taps, nz >= 8 R: split in two along z
    float64: (40, 9, 9) 9 taps, (40, 8, 10) 33 taps, (40, 9, 9) zero centre
  spectral_conv_moments   (40, 9, 9) 9 taps, (40, 8, 10) 33 taps (a kernel without a ring has no fused form)
  spatial_conv
    (80, 12, 14) 9 x 9 separable ring, arithmetic="f32"; (80, 10, 64) the same at nx = 64: fast pass under none / isfinite
    (80, 18, 20) 17 x 17 ring; (80, 12, 14) default form: the split (matrix-core) form under array (+ isfinite)
    (80, 70, 8)  67 x 3 taps: two-pass wide form;  (80, 12, 14) 9 x 3 not separable: tiled 2-D, all-valid pass under none / isfinite
    (80, 7, 9)   3 x 3 not separable: generic 2-D;  (80, 7, 9) zero centre taps: empty windows over included and excluded centres,
                 the 9 ring under a mask with isfinite, the per-output 2-D kernel under the others
    float64: (80, 12, 14) separable, (80, 7, 9) 2-D
  spectral_lerp (40, 11, 11), (40, 8, 16) tiled form and SPC_LERP_TILES=0, float64 (40, 11, 11);
  resample_bilinear (120, 9, 11): the LDS-staged kernel, the gather kernel alone (SPC_BILINEAR_LDS=0), float64;
  resample_bilinear_lerp (240, 9, 11, every plane twice: it blends neighbouring planes too): the LERP forms of both kernels;
    each at the identity and at a half-sample shift; these cubes also hold rays / planes that are one special sample
    throughout (an interpolation blends neighbours, and most masks exclude one of two background values)
  fill_masked, fill_masked_transposed, percentile_axis2, percentile_global, percentile_axis0 in float64: the cube and the masks
    of test_order_statistics_mask_predicates_as_key_intervals, bit for bit
  arith (* 1), stack_shift (zero shift), stack_cube (one slab on its own grid), mosaic (one field on its own grid): the
    identity scheme of test_gpu_mask_layer.py on (5, 6, 7) and (8, 8, 16), nan_excluded both ways where the operator has it

What these cases found, beside the predicates: the float32 ring, split and wide stencils multiply every tap of their window,
a zero tap too, and 0 * inf is NaN where the oracle, the float64 kernels and the per-output kernels - which skip zero taps -
give a finite value.  Before the fix spectral_conv with 41 taps (padded with zeros to the 49 ring) gave 94 NaN against 59
expected under "none" on (48, 8, 10), the 35 extra ones on the four outputs either side of the kernel around each +-inf
sample, and spatial_conv with 3 x 3 taps and a zero centre gave 208 NaN outputs that should be finite on (80, 7, 9).  Under a
mask that lets +-inf through, the first now leaves its flagged tiles to the runs-of-16 kernel (which never multiplies the
PADDING; a zero tap inside the kernel it still multiplies) and the second takes the per-output 2-D kernel, which skips every
zero tap (see spc_spectral_conv_f32 and spc_spatial_conv_sep_f32).  Kernels padded into the 9 / 17 / 33 rings keep the defect:
test_padded_ring_defect_is_confined pins where it shows.  The float32 ring and split stencils and the float64 spatial ones
also gave inf for a window that holds max alone (k * max * (1 / k) rounds one step above max); with non-negative taps the
quotient is a weighted mean and is now held at max while the numerator is finite."""
import warnings

import numpy as np
import pytest

import mask_edges as E
from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray
from test_gpu_mask_layer import _same_bits

pytestmark = pytest.mark.gpu


def _dev(a):
    return DeviceArray.from_numpy(np.ascontiguousarray(a), 0)


def _spec(m, dev_arr):
    if not m.flags and not m.with_array:
        return None
    return ops.MaskSpec(m.flags | (_lib.MASK_ARRAY if m.with_array else 0), m.lo, m.hi, dev_arr if m.with_array else None)


def _host(r, names):
    return {k: r[k].get() for k in names}


def _run(c, dev, spec, aux):
    """the outputs of case *c* under *spec*, named as its reference names them"""
    op, shape = c.op, c.shape
    if op == "moments":
        return _host(ops.moments(dev, aux["cen"], dv=E.dv_of(c.dtype), m1_add=E.M1_ADD, mask=spec, want=c.par[0]), c.par[0])
    if op == "moments_f64":
        return _host(ops.moments_f64(dev, aux["cen"], dv=E.dv_of(c.dtype), m1_add=E.M1_ADD, mask=spec, want=c.par[0]), c.par[0])
    if op == "moment_order":
        r = ops.moments(dev, aux["cen"], mask=spec, want=("mu", "s0"))
        return {"m3": ops.moment_order(dev, aux["cen"], 3, r["mu"], r["s0"], mask=spec).get()}
    if op == "moment_order_f64":
        r = ops.moments_f64(dev, aux["cen"], mask=spec, want=("mu", "s0"))
        return {"m3": ops.moment_order_f64(dev, aux["cen"], 3, r["mu"], r["s0"], mask=spec).get()}
    if op == "moments_spatial":
        r = ops.moments_spatial(dev, aux["cen2d"], c.par, E.dv_of(c.dtype), mask=spec)
        out = _host(r, ("m0", "m1", "m2"))
        out["m3"] = ops.moment_order_spatial(dev, aux["cen2d"], c.par, 3, r["m1"], mask=spec).get()
        return out
    if op == "argextrema_axis":
        return _host(ops.argextrema_axis(dev, c.par, mask=spec), ("argmax", "argmin"))
    if op == "stats_axis":
        return _host(ops.stats_axis(dev, c.par, mask=spec), ops.STAT_KEYS)
    if op == "stats_planes":
        return ops.stats_planes(dev, mask=spec)
    if op == "stats_global":
        return {k: np.float64(v) for k, v in ops.stats_global(dev, mask=spec).items()}
    if op == "spectral_conv":
        return {"out": ops.spectral_conv(dev, c.par, mask=spec).get()}
    if op == "spectral_conv_moments":
        return _host(ops.spectral_conv_moments(dev, c.par, aux["cen"], dv=E.dv_of(c.dtype), m1_add=E.M1_ADD, mask=spec, want=E.SUMS,
                                               cen_host=E.spectral_centres(shape[0])), E.SUMS)
    if op == "spatial_conv":
        return {"out": ops.spatial_conv(dev, c.par[0], mask=spec, arithmetic=c.par[1]).get()}
    if op == "spectral_lerp":
        lo, t, inv, _, _, fill = ops.lerp_plan(*E.lerp_axes(shape[0], c.par[0]))
        return {"out": ops.spectral_lerp(dev, lo, t, inv, fill, mask=spec).get()}
    xs, ys = E.bilinear_maps(shape, c.par[0])
    if op == "resample_bilinear":
        out, foot = ops.resample_bilinear(dev, xs, ys, mask=spec)
    else:
        lo, t, inv, _, _, fill = ops.lerp_plan(*E.lerp_axes(shape[0], c.par[0]))
        out, foot = ops.resample_bilinear_lerp(dev, xs, ys, lo, t, inv, fill=fill, mask=spec)
    return {"out": out.get(), "foot": foot.get()}


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_operator_at_the_mask_edges(gpu, monkeypatch, case):
    if case.op in E.BLENDS:
        for name, value in case.par[1]:
            monkeypatch.setenv(name, value)
    cache = E.RefCache(case)
    dev, dev_arr = _dev(cache.d), _dev(cache.arr)
    aux = {"cen": _dev(E.spectral_centres(case.shape[0]))}
    if case.op == "moments_spatial":
        aux["cen2d"] = _dev(E.spatial_centres(case.shape, case.par))
    failed = []
    for m in E.masks(case.dtype):
        got = _run(case, dev, _spec(m, dev_arr), aux)
        try:
            E.check(got, cache.expected(m), "%s (%s) %s: %s" % (case.op, case.path, case.shape, m.name))
        except AssertionError as err:                # every mask is tried: the report names all that miss
            failed.append(str(err).splitlines()[0])
    assert not failed, "%d of %d masks: %s" % (len(failed), len(E.masks(case.dtype)), "\n".join(failed[:8]))


def test_padded_ring_defect_is_confined(gpu):
    """KNOWN DEFECT, pinned: a 13-tap kernel sits in the 17-tap ring between two zero taps on either side, which the ring
    kernel multiplies: around an included +-inf sample the outputs 7 and 8 channels away (inside the ring, outside the kernel)
    are NaN where the oracle is finite.  Everything else matches the oracle at the tolerance of test_spectral_conv_vs_oracle.
    Whoever repairs the rings replaces this test by a 13-tap entry in mask_edges.SPECTRAL_CASES."""
    case = E.Case("spectral_conv", "13 taps in the 17 ring", np.float32, (40, 9, 9), E.taps(13))
    cache = E.RefCache(case)
    d, arr = cache.d, cache.arr
    dev, dev_arr = _dev(d), _dev(arr)
    z = np.arange(40)[:, None, None]
    seen = 0
    for m in E.masks(np.float32):
        inc = E.include(d, arr, m)
        zone = np.zeros(d.shape, bool)
        for zi, y, x in np.argwhere(inc & np.isinf(d)):
            zone[:, y, x] |= (np.abs(z[:, 0, 0] - zi) > 6) & (np.abs(z[:, 0, 0] - zi) <= 8)
        got = ops.spectral_conv(dev, case.par, mask=_spec(m, dev_arr)).get()
        exp = cache.expected(m)["out"][0]
        assert np.isnan(got[zone]).all(), m.name
        seen += int((zone & ~np.isnan(exp)).sum())
        E.check({"out": np.where(zone, np.float32(0), got)}, {"out": E.of_max(np.where(zone, np.float32(0), exp), 1e-5)}, m.name)
    assert seen > 0


# ---- the operators that share the key-interval test of the order statistics -------------------------------------------------------
FILL = -7.0


def _order_statistic_case(dtype):
    d = E.order_statistic_data(dtype)
    return d, _dev(d), [(m, E.include(d, None, m)) for m in E.order_statistic_masks()]


def _spec_of(m):
    return ops.MaskSpec(m.flags, m.lo, m.hi) if m.flags else None


def test_fill_masked_and_its_transpose(gpu):
    d, dev, cases = _order_statistic_case(np.float32)
    for m, inc in cases:
        exp = np.where(inc, d, np.float32(FILL))
        _same_bits(ops.fill_masked(dev, _spec_of(m), fill=FILL).get(), exp, m.name)
        _same_bits(ops.fill_masked_transposed(dev, _spec_of(m), fill=FILL).get(), np.ascontiguousarray(exp.transpose(0, 2, 1)), m.name + " (transposed)")


def test_percentiles_along_x_and_of_the_whole_cube(gpu):
    d, dev, cases = _order_statistic_case(np.float32)
    for m, inc in cases:
        f = np.where(inc, d, np.nan).astype(np.float32)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            exp2, expg = np.nanmedian(f, axis=2), np.nanmedian(f)
        assert np.array_equal(ops.percentile_axis2(dev, 50.0, mask=_spec_of(m)).get(), exp2, equal_nan=True), m.name
        got = np.float32(ops.percentile_global(dev, 50.0, mask=_spec_of(m)))
        assert got == expg or (np.isnan(got) and np.isnan(expg)), (m.name, got, expg)


def test_float64_percentile_along_the_spectral_axis(gpu):
    d, dev, cases = _order_statistic_case(np.float64)
    for m, inc in cases:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            exp = np.nanmedian(np.where(inc, d, np.nan), axis=0)
        got = ops.percentile_axis0(dev, 50.0, mask=_spec_of(m)).get()
        assert got.dtype == np.float64 and np.array_equal(got, exp, equal_nan=True), m.name


# ---- the spc_include operators that test_gpu_mask_layer.py leaves out: its identity scheme, bit for bit ----------------------------
IDENTITY = [(t, s) for t in (np.float32, np.float64) for s in ((5, 6, 7), (8, 8, 16))]
identity = pytest.mark.parametrize("dtype,shape", IDENTITY, ids=["%s-%dx%dx%d" % ((np.dtype(t).name,) + s) for t, s in IDENTITY])


def _each(dtype, shape, both=True):
    """(name, MaskSpec, nan_excluded, include set, host cube, device cube) per mask, nan_excluded both ways"""
    d, arr = E.flat_cube(dtype, shape)
    dev, dev_arr = _dev(d), _dev(arr)
    for m in E.masks(dtype):
        for nan_excluded in (False, True) if both else (False,):
            inc = E.include(d, arr, m)
            if nan_excluded:
                inc = inc & ~np.isnan(d)
            yield "%s%s" % (m.name, ", nan excluded" if nan_excluded else ""), _spec(m, dev_arr), nan_excluded, inc, d, dev


@identity
def test_arith_times_one(gpu, dtype, shape):
    for what, spec, nx_, inc, d, dev in _each(dtype, shape):
        out = ops.arith(dev, [("mul", 1.0, True)], mask=spec, fill=FILL, nan_excluded=nx_).get()
        _same_bits(out, np.where(inc, d, dtype(FILL)), what)


@identity
def test_stack_shift_by_zero(gpu, dtype, shape):
    """a zero shift is a gather: column p is the filled spectrum in float64, NaN where it is not finite, all NaN where none is"""
    npos = shape[1] * shape[2]
    for what, spec, nx_, inc, d, dev in _each(dtype, shape):
        out = ops.stack_shift(dev, np.arange(npos), np.zeros(npos), fill=np.nan, mask=spec, nan_excluded=nx_).get()
        f = np.where(inc, d, np.nan).astype(np.float64).reshape(shape[0], npos)
        exp = np.where(np.isfinite(f), f, np.nan)
        assert out.dtype == np.float64 and np.array_equal(out, exp, equal_nan=True), what


@identity
def test_stack_cube_of_one_slab_on_its_own_grid(gpu, dtype, shape):
    nz = shape[0]
    lo, t, inv = np.arange(nz, dtype=np.int32)[None], np.zeros((1, nz)), np.ones((1, nz))
    for what, spec, nx_, inc, d, dev in _each(dtype, shape):
        out = ops.stack_cube(dev, lo, t, inv, [1], mode="sum", fill=np.nan, mask=spec, nan_excluded=nx_).get()
        # (by value: the sum starts from +0.0, so a lone -0.0 comes back as +0.0)
        assert out.dtype == dtype and np.array_equal(out, np.where(inc, d, dtype(np.nan)), equal_nan=True), what


@identity
@pytest.mark.parametrize("order", [0, 1])
def test_mosaic_of_one_field_on_its_own_grid(gpu, dtype, shape, order):
    """nan_to_num of the resampled filled cube over a weight of 1 (cube_utils.py:810-856); nearest neighbour is the filled cube
    itself, bilinear at integer positions is oracle_np.resample_bilinear (a NaN or inf neighbour reaches through its zero weight)"""
    import oracle_np as O
    xs, ys = E.bilinear_maps(shape, 0.0)
    dxs, dys = _dev(xs), _dev(ys)
    for what, spec, nx_, inc, d, dev in _each(dtype, shape, both=False):
        out = ops.mosaic([dev], [(dxs, dys)], [spec], [FILL], order).get()
        f = np.where(inc, d, dtype(FILL))
        with np.errstate(all="ignore"):
            r = f if order == 0 else O.resample_bilinear(f, xs, ys)[0].astype(dtype)
            exp = (np.nan_to_num(r.astype(np.float64)) / 1.0).astype(dtype)
        assert out.dtype == dtype and np.array_equal(out, exp), what
