"""Every operator on strided, offset and misaligned views of a cube, a mask and an output (tests/views.py).

Contiguous, 256-byte aligned allocations hide four kinds of defect: a dispatch condition that forgets one stride or one
pointer, a 16-byte form that steps by nx where it means row_stride, a tile that over-reads past nx and then uses what
it read, a vector store that overruns a strided output row.  Here the cube is a view of a parent that holds 1e30 / 1e300
outside it, the mask a view of a parent that holds 1 outside it, the output a view of a parent filled with -7e33, which
must still be there after the call.  The reference is always numpy on the numpy slice of the same data.

TABLE lists, per operator, the entry point, the line that chooses between its 16-byte and its general form, which of the
layouts fall on which side of it, and what the result is held to: "exact" (bit for bit against numpy) or the tolerance
of the operator's existing parity test, cited.  "aligned" = contig, rows, planes_of_rows, xwin_aligned; "general" =
xwin_off1 (base one element off), xwin_oddstride (row stride 139, plane stride 2085), xwin_tail (nx = 131, base three
elements off).  mask_phase moves the mask's base off the cube's phase: the entries that test the mask's alignment go
general with it, the others must not care.  A float64 cube in xwin_off1 is 8-byte aligned only: general in every entry."""
import collections
import contextlib
import os
import re
import warnings

import numpy as np
import pytest

import mask_edges as E
import oracle_np as O
import views as V
from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
ALIGNED = ("contig", "rows", "planes_of_rows", "xwin_aligned")
GENERAL = ("xwin_off1", "xwin_oddstride", "xwin_tail")

# (operator, entry points, dispatch line, kind, tolerance and where it comes from).  Fast form: ALIGNED (with mask_same /
# mask_contig); general form: GENERAL, and ALIGNED with mask_phase where the line tests the mask - unless noted.
TABLE = [
    ("moments", "spc_moments_f32", "spc_moments.hip make_plan (aligned(v), v = 4, 2, 1; mask base and strides too)", "summing",
     "m0 1e-5 max, m1 1e-5 span, m2 1e-5 scale on rays with signal; extrema, counts exact: test_gpu_ops.py:56-72"),
    ("moments_f64", "spc_moments_f64 + spc_moment_order_f64", "spc_moments_f64.hip:186 (spc_pairs_ok_f64, spc_wide.h:39)", "summing",
     "1e-13: mask_edges.py:301 (test_moments_f64, test_gpu_round4.py)"),
    ("moment_order", "spc_moment_order_f32 / _f64", "spc_moments.hip spc_moment_order_f32 (v4); spc_moments_f64.hip:186", "summing",
     "rtol 1e-9, atol 1e-9 max: test_gpu_ops.py:116; float64 1e-12: mask_edges.py:317"),
    ("stats_axis", "spc_stats_axis_f32 / _f64, axes 0 1 2", "spc_stats.hip:855-856 (v4)", "summing",
     "count, min, max exact; sum, sumsq rtol 1e-12: test_gpu_ops.py:460-465"),
    ("stats_m2", "spc_stats_m2_axis_f32 / _f64 (the m2 route of std)", "spc_stats_m2.hip:111-140 (no 16-byte form: one load per sample on every layout)", "summing",
     "std = sqrt(m2 / n) at far_from_zero.RTOL: test_gpu_far_from_zero.py:182"),
    ("stats_dev_axis", "spc_stats_dev_axis_f32 / _f64", "spc_stats_m2.hip:111-140 (no 16-byte form)", "summing",
     "the whole cube's std from s1, s2 at far_from_zero.RTOL: test_gpu_far_from_zero.py:48"),
    ("percentile_axis0", "spc_percentile_axis0_f32 (register, radix-16, bisection) / _f64 (register form; its LDS form, a "
     "once-per-process switch, in a fresh process)", "spc_select.hip:377 (v4); takes swap01 (spc_check_cube_any_order)", "exact",
     "median and MAD equal np.nanmedian: test_gpu_round2.py:327-334"),
    ("sigma_clip_axis0", "spc_sigma_clip_axis0_f32 (fused: packed rays, rays in registers) / the loop of kernels (SPC_SIGMA_CLIP_FUSED=0) / _f64", "spc_sigma_clip.hip:68 (no 16-byte form; takes swap01)",
     "exact against contig", "kept values equal the oracle's, NaN pattern differs on < 2e-4 of the samples: test_gpu_round2.py:529-531"),
    ("moments_spatial", "spc_moments_spatial_f32 + spc_moment_order_spatial_f32, axes 1 2",
     "spc_moments_spatial.hip:152 (per row), :184 (v4)", "summing", "rtol 1e-9, atol 1e-7 max: test_gpu_ops.py:142"),
    ("argextrema_axis", "spc_argextrema_axis_f32, axes 1 2", "spc_stats.hip:906-907 (v4, axis 1; axis 2 per row)", "exact", "-"),
    ("stats_planes", "spc_stats_planes_f32", "spc_stats.hip:191-205 (flat planes / row by row)", "summing",
     "sum, sumsq rtol 1e-12: test_gpu_ops.py:746-747"),
    ("stats_global", "spc_stats_global_f32 / _f64", "spc_stats.hip:120-129 (one run / rows of a view); spc_stats_f64.hip:161 (vec2: spc_pairs_ok_f64)",
     "summing", "npts, min, max exact; sum, sumsq rtol 1e-12: test_gpu_ops.py:441-465"),
    ("percentile_axis2", "spc_percentile_axis2_f32", "spc_select.hip:419-440 (no 16-byte form: lanes take consecutive samples of a row; takes "
     "swap01)", "exact", "-"),
    ("percentile_global", "spc_percentile_global_f32", "spc_select_global.hip:86-92 (gsel_geometry: one run / rows of a view)", "exact", "-"),
    ("key_histogram", "spc_key_histogram_f32 (+ key_next)", "spc_select_global.hip:86-92", "exact", "-"),
    ("spectral_conv", "spc_spectral_conv_f32 (9, 17, 33, 49, 65 taps; masked, all valid) / _f64",
     "spc_spectral_conv.hip:377-380 (two spaxels per lane: cube, mask and output)", "summing", "1e-5 max: test_gpu_ops.py:169"),
    ("spectral_conv_moments", "spc_spectral_conv_moments_f32", "spc_spectral_conv.hip:329-331 (algebraic form: the "
     "all-valid row on the ALIGNED layouts; never with a mask array, never on GENERAL), :377-380", "summing",
     "m0 1e-5 max, m1 1e-5 span, m2 1e-5 max on well-conditioned rays: mask_edges.py:382-383 (test_gpu_ops.py:246-251)"),
    ("spatial_conv", "spc_spatial_conv_sep_f32 (split / matrix-core form, ring form), spc_spatial_conv2d_f32, spc_spatial_conv_f64 "
     "(ring, two-pass)", "spc_spatial_split.hip:709-710; spc_spatial_conv.hip:636; spc_spatial_conv_impl.h:398,489,602 (nx = 1024, BASE_WIDE: :398 holds on "
     "the last strip of the ALIGNED layouts and of out_xwin_aligned, fails on whole strips, on xwin_tail and on out_xwin_off1; :168, :404, :592 "
     "edge_cols false on the inner strips)", "summing",
     "1e-5 max: test_gpu_ops.py:273"),
    ("spatial_conv_mfma", "spc_spatial_conv_sep_mfma_f32: cube, cube + moment 0, moment 0 alone; split form, form 2, form 1 "
     "(SPC_SPATIAL_MFMA_FORM)", "spc_spatial_moment.hip:812-813 with spc_spatial_split.hip:709-710 (split: multiples of 4 - ALIGNED with "
     "mask_same / mask_contig hold, GENERAL and mask_phase fail), :836-839 (older forms: column pairs - GENERAL and mask_phase are "
     "refused, HipUnsupported), :762-766 (form 2: mask strides equal the cube's - mask_same holds, mask_contig on a view fails)", "summing",
     "cube 1e-5 max: test_gpu_mfma.py:40; m0 1e-5 max: test_gpu_mfma.py:65"),
    ("spatial_conv_mfma_moments", "spc_spatial_conv_sep_mfma_moments_f32: m0 m1 m2, with and without the cube", "spc_spatial_moment.hip:812-813, "
     ":830 (no split form: refused, HipUnsupported - GENERAL, mask_phase, every layout under SPC_SPATIAL_MFMA_FORM=1)", "summing",
     "m0 1e-5 max, m1 1e-5 * 500 nz, m2 1e-5 max: test_gpu_round5.py:80-82"),
    ("spectral_lerp", "spc_spectral_lerp_f32 (tiled, untiled) / _f64", "spc_resample.hip:937-939 (v4: cube and output)", "summing",
     "1e-5 max: test_gpu_ops.py:344"),
    ("resample_bilinear", "spc_resample_bilinear_f32 (LDS, gather) / _f64, spc_resample_bilinear_lerp_f32",
     "spc_resample.hip:484 (vector store: output base and strides)", "summing", "1e-5 max, footprint exact: test_gpu_ops.py:356; "
     "the identity map at order 0 exact"),
    ("resample_spline", "spc_resample_spline_f32", "spc_resample.hip:993-1019 (no 16-byte form)", "summing", "1e-5 of the data range: test_gpu_round4.py:151"),
    ("fill_masked", "spc_fill_masked_f32, spc_fill_masked_transpose_f32, spc_mask_include_u8 / _f64, spc_narrow_f64_to_f32",
     "spc_stats.hip:1024 / spc_convert_f64.hip:18 (scalar)", "exact", "-"),
    ("downsample", "spc_downsample_f32 / _f64, axes 0 1 2", "spc_downsample.hip:347-350 (ds_vec_ok: cube, mask, output)", "summing",
     "float32 within 1 ulp of the float64 restatement: test_gpu_downsample.py:45; float64 rtol 1e-14, atol 1e-15 max: :194"),
    ("subcube", "spc_subcube_f32 / _f64 (step 1, step 2), spc_mask_bbox_f32 / _f64", "spc_subcube.hip:258, :294", "exact", "-"),
    ("rank_filter", "spc_rank_filter_axis0_f32 / _f64, spc_rank_filter_plane_f32 / _f64", "spc_rank_filter.hip:375 (rf_vec_ok)", "exact", "-"),
    ("stack_shift", "spc_stack_shift_f32 / _f64, spc_stack_sum_f32 / _f64", "spc_stack.hip:315 (gather of single spectra: no 16-byte form)", "summing",
     "1e-10 of the data scale: test_gpu_stack_spectra.py:26,52"),
    ("stack_cube", "spc_stack_cube_f32 / _f64", "spc_stack_cube.hip:220", "summing", "2^-23 (float64: 1e-11) of the data scale: "
     "test_gpu_stack_cube.py:32"),
    ("mosaic", "spc_mosaic_f32 / _f64, two sources in different views", "spc_mosaic.hip:222 (gather: no 16-byte form)", "exact", "nearest neighbour on the cube's own grid"),
    ("arith", "spc_arith_f32 / _f64, the cube and a cube operand in different views", "spc_arith.hip:100 (phase per row), :234", "exact", "-"),
    ("mask_eval", "spc_mask_eval_f32 / _f64, slots in different views", "spc_mask_eval.hip:113 (phase of the output row)", "exact", "-"),
]

# refuses: (operator, layout) -> (source line of the check, exception, message)
REFUSES = [
    ("every entry but percentile_axis0, percentile_axis2 and the fused sigma_clip_axis0 (float32)", "swap01", "spc_common.h:206 (spc_check_cube)",
     _lib.HipInvalidArgument, "plane_stride too small"),
    ("spatial_conv_mfma", "GENERAL, mask_phase", "spc_spatial_moment.hip:836-839", _lib.HipUnsupported, "8-byte column pairs / odd mask strides"),
    ("spatial_conv_mfma_moments", "GENERAL, mask_phase", "spc_spatial_moment.hip:830", _lib.HipUnsupported, "moments 1 / 2 need the split form"),
    ("mosaic", "out_xwin_*", "ops.py (mosaic): the output is contiguous by contract", ValueError, "contiguous"),
    ("resample_bilinear_lerp, stack_cube, spatial_conv_mfma, spatial_conv_mfma_moments, resample_spline", "out_xwin_*",
     "ops.py (_contiguous_out; resample_bilinear_lerp its own check): asserted in test_views_host.py", ValueError, "contiguous"),
]
# (spc_clip_outside_f32 takes a bare pointer to a contiguous cube - the copy fill_masked made: no view can reach it)


# ---- plumbing -------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _env(pairs):
    old = {k: os.environ.get(k) for k, _ in pairs}
    os.environ.update({k: v for k, v in pairs})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _dev(a):
    return DeviceArray.from_numpy(np.ascontiguousarray(a), 0)


def _bits(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    bad = np.argwhere(~((got == exp) | ((got != got) & (exp != exp))))
    assert not len(bad), "%s: differs at %d places, first %s: got %s, expected %s" % (
        what, len(bad), bad[:4].tolist(), [got[tuple(i)] for i in bad[:4]], [exp[tuple(i)] for i in bad[:4]])


class Ctx:
    """one case: the host slice, the device views and what reads an output back"""

    def __init__(self, dtype, cname, mname, oname, base=V.BASE, masked=True, finite=False, pedestal=0.0, data=None, mask=None):
        """*data*, *mask*: (tag, array of the base shape) in place of the samples / the include bytes of views.data; the tags
        join the key of the reference cache (a mask's tag names its include set, whatever its byte values)"""
        self.dtype = dtype = np.dtype(dtype)
        self.lay = V.layout(cname, base)
        d, m = V.data(dtype.type, base, pedestal=pedestal)
        self.given = {"data": data, "mask": mask}
        if data is not None:
            d = np.asarray(data[1], dtype)
        if mask is not None:
            m = np.asarray(mask[1], np.uint8)
        if finite:
            d = np.where(np.isnan(d), dtype.type(0.25), d)
        self.d, self.m = V.crop(d, self.lay), V.crop(m, self.lay)
        self.cube, self._cparent = V.upload(self.lay, self.d, V.CUBE_POISON[dtype])
        self.inc = self.m.astype(bool) if masked else np.ones(self.d.shape, bool)
        self.spec = None
        if masked:
            self.mlay = V.mask_layout(mname, self.lay)
            self.marr, self._mparent = V.upload(self.mlay, self.m, 1)
            self.spec = ops.MaskSpec(_lib.MASK_ARRAY, array=self.marr)
        self.oname = oname
        self.key = (dtype, self.lay.shape, masked, finite, pedestal) + tuple(g[0] for g in (data, mask) if g is not None)
        self._outs = []

    def out(self, shape, dtype):
        """an output in this case's output layout, checked for stray writes by ``finish``"""
        lay = V.layout(self.oname, shape)
        view, parent = V.output(lay, dtype)
        self._outs.append((lay, parent))
        return view

    def read(self, view):
        """the host copy of an output this case made with ``out`` (through its parent), or of a fresh array"""
        for lay, parent in self._outs:
            if view.ptr == parent.ptr + lay.offset * parent.dtype.itemsize:
                got, clean = V.read_output(lay, parent)
                assert clean, "wrote outside the output view (%s)" % lay.name
                return got
        return view.get()


_REF = {}


def _ref(name, ctx, fn):
    key = (name,) + ctx.key
    if key not in _REF:
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            _REF[key] = fn()
    return _REF[key]


def _cen(nz):
    return _dev(E.spectral_centres(nz))


# ---- the operators: run(ctx) -> {name: host array}, ref(ctx) -> {name: (expected, groups)} as mask_edges.check reads them --------
Op = collections.namedtuple("Op", "name dtypes run ref env out masked finite same any_order base pedestal declines")
# one strip of every spatial stencil and a second one.  Along x the ring kernels work in strips of 248 (9 taps) or 240 (17 taps)
# output columns from 256 input columns, the all-valid pass in strips of 504 from 512, the matrix-core forms in strips of 480
# from 512; a run is 8 columns.  At nx = 1024 each of them has whole strips, a strip that lies inside the row on both sides
# (its unclamped loads run: edge_cols false) and a last strip of an even number of whole runs (32, 64 or 16 columns: the
# paired stores of spc_spatial_conv_impl.h:398 hold); xwin_tail (nx = 1023) ends on a ragged run (they fail)
BASE_WIDE = (21, 9, 1024)
OPS = collections.OrderedDict()


def op(name, dtypes=(F32, F64), env=(), out=False, masked=True, finite=False, same=ALIGNED, any_order=(), base=V.BASE, pedestal=0.0,
       declines=None):
    """register run / ref for one row of the matrix.  *same*: the layouts whose result equals the contiguous one bit for bit
    (the same form runs, on the same samples in the same order); *out*: the operator writes a cube the caller may hand in;
    *any_order*: the sample types whose entry calls spc_check_cube_any_order and so meets swap01; *pedestal*: see views.data;
    *declines*: ``declines(ctx)`` -> a regular expression when the entry refuses this combination by design (HipUnsupported with
    that message, asserted), else None"""
    def deco(pair):
        run, ref = pair()
        OPS[name] = Op(name, dtypes, run, ref, tuple(env), out, masked, finite, same, any_order, base, pedestal, declines)
        return pair
    return deco


def _moments32_ref(d, inc):
    nz = d.shape[0]
    cen = E.spectral_centres(nz)
    e0, e1, e2 = O.moments012(d, inc, cen, 0.5, E.M1_ADD)
    okm = np.isfinite(e2)
    span = nz / 64.0                                    # (the centres of mask_edges.spectral_centres span nz / 64)
    scale = max(np.nanmax(np.abs(e2[okm])) if okm.any() else 1.0, span ** 2 * 1e-3)
    wc = okm & (np.abs(e0) > 1e-3 * np.nanmax(np.abs(e0)))
    f = O.filled(d, inc)
    v = inc & ~np.isnan(d)
    vmax, vmin = E._extrema(d, inc, 0)
    return {"m0": E.of_max(e0, 1e-5), "m1": E.within(e1, 1e-5 * span), "m2": E.within(e2, 1e-5 * scale, where=wc),
            "argmax": E.exact(O.argmax(d, v)), "argmin": E.exact(O.argmin(d, v)), "nvalid": E.exact((~np.isnan(f)).sum(axis=0).astype(np.int32)),
            "vmax": E.exact(vmax), "vmin": E.exact(vmin)}


@op("moments", (F32,), pedestal=5.0)
def _():
    def run(c):
        r = ops.moments(c.cube, _cen(c.d.shape[0]), dv=0.5, m1_add=E.M1_ADD, mask=c.spec, want=E.EXTREMA)
        return {k: r[k].get() for k in E.EXTREMA}
    return run, lambda c: _moments32_ref(c.d, c.inc)


@op("moments_f64", (F64,), pedestal=5.0)
def _():
    def run(c):
        r = ops.moments_f64(c.cube, _cen(c.d.shape[0]), dv=1.0, m1_add=E.M1_ADD, mask=c.spec, want=E.EXTREMA)
        return {k: r[k].get() for k in E.EXTREMA}
    return run, lambda c: E.ref_moments(c.d, c.inc, E.EXTREMA)


@op("moment_order", pedestal=5.0)
def _():
    def run(c):
        cen = _cen(c.d.shape[0])
        if c.dtype == F64:
            r = ops.moments_f64(c.cube, cen, mask=c.spec, want=("mu", "s0"))
            return {"m3": ops.moment_order_f64(c.cube, cen, 3, r["mu"], r["s0"], mask=c.spec).get()}
        r = ops.moments(c.cube, cen, mask=c.spec, want=("mu", "s0"))
        return {"m3": ops.moment_order(c.cube, cen, 3, r["mu"], r["s0"], mask=c.spec).get()}
    return run, lambda c: E.ref_moment_order(c.d, c.inc)


def _stats_axis(axis):
    def run(c):
        r = ops.stats_axis(c.cube, axis, mask=c.spec)
        return {k: r[k].get() for k in ops.STAT_KEYS}
    return run, lambda c: E.ref_stats_axis(c.d, c.inc, axis)


for _a in (0, 1, 2):
    op("stats_axis%d" % _a, pedestal=5.0)(lambda _a=_a: _stats_axis(_a))


def _std_ref(c, axis):
    import far_from_zero as Z
    return {"std": E.within(Z.ref_std(np.where(c.inc, c.d, np.nan), axis, 0), 0.0, Z.RTOL)}


def _stats_m2(axis):
    def run(c):
        r = ops.stats_axis(c.cube, axis, mask=c.spec, want=("count", "sum", "m2"))
        with np.errstate(all="ignore"):
            return {"std": np.sqrt(r["m2"].get() / r["count"].get())}
    return run, lambda c: _std_ref(c, axis)


for _a in (0, 1, 2):
    op("stats_m2_axis%d" % _a, pedestal=5.0)(lambda _a=_a: _stats_m2(_a))


@op("stats_dev_axis", pedestal=5.0)
def _():
    def run(c):
        n = float(c.inc.sum() - (np.isnan(c.d) & c.inc).sum())
        out = {}
        for axis in (0, 1, 2):
            s1, s2 = (a.get() for a in ops.stats_dev_axis(c.cube, axis, 0.125, mask=c.spec))
            t1, t2 = np.nansum(s1), np.nansum(s2)
            out["std%d" % axis] = np.float64(np.sqrt((t2 - t1 * t1 / n) / n))
        return out

    def ref(c):
        e = _std_ref(c, None)["std"]
        return {"std%d" % a: e for a in (0, 1, 2)}
    return run, ref


def _percentile0(env=()):
    def run(c):
        med = ops.percentile_axis0(c.cube, 50.0, mask=c.spec)
        return {"median": med.get(), "mad": ops.percentile_axis0(c.cube, 50.0, mask=c.spec, center=med).get()}

    def ref(c):
        f = np.where(c.inc, c.d, np.nan).astype(c.dtype)
        med = np.nanmedian(f, axis=0)
        return {"median": E.exact(med), "mad": E.exact(np.nanmedian(np.abs(f - med[None]), axis=0))}
    return run, ref


op("percentile_axis0", any_order=(F32, F64))(_percentile0)
op("percentile_axis0[radix16]", (F32,), env=(("SPC_SELECT_REG", "0"),), any_order=(F32,))(_percentile0)
op("percentile_axis0[bisection]", (F32,), env=(("SPC_SELECT_REG", "0"), ("SPC_SELECT_RADIX16", "0")), any_order=(F32,))(_percentile0)
op("percentile_axis0[no descriptors]", (F32,), env=(("SPC_SELECT_DESC", "0"),), any_order=(F32,))(_percentile0)


def _sigma_clip():
    def run(c):
        f = ops.sigma_clip_axis0 if c.dtype == F32 else ops.sigma_clip_axis0_f64
        return {"out": f(c.cube, sigma=2.5, mask=c.spec).get()}

    def ref(c):
        return {"out": (O.sigma_clip(c.d, c.inc & ~np.isnan(c.d), 2.5, out_dtype=c.dtype), "sigma_clip")}
    return run, ref


op("sigma_clip_axis0", any_order=(F32,))(_sigma_clip)           # (spc_sigma_clip.hip:68; the float64 entry and the loop refuse)
op("sigma_clip_axis0[loop]", (F32,), env=(("SPC_SIGMA_CLIP_FUSED", "0"),))(_sigma_clip)
# (rays of at most 128 valid samples are packed into LDS by default - every ray of these cubes; SPC_SELECT_COMPACT=0 keeps them
# in registers)
op("sigma_clip_axis0[not packed]", (F32,), env=(("SPC_SELECT_COMPACT", "0"),), any_order=(F32,))(_sigma_clip)


def _moments_spatial(axis):
    def run(c):
        cen = _dev(E.spatial_centres(c.d.shape, axis))
        r = ops.moments_spatial(c.cube, cen, axis, 0.5, mask=c.spec)
        out = {k: r[k].get() for k in ("m0", "m1", "m2")}
        out["m3"] = ops.moment_order_spatial(c.cube, cen, axis, 3, r["m1"], mask=c.spec).get()
        return out
    return run, lambda c: E.ref_moments_spatial(c.d, c.inc, axis)


for _a in (1, 2):
    op("moments_spatial_axis%d" % _a, (F32,), pedestal=5.0)(lambda _a=_a: _moments_spatial(_a))


def _argextrema(axis):
    def run(c):
        r = ops.argextrema_axis(c.cube, axis, mask=c.spec)
        return {k: r[k].get() for k in ("argmax", "argmin")}
    return run, lambda c: E.ref_argextrema(c.d, c.inc, axis)


for _a in (1, 2):
    op("argextrema_axis%d" % _a, (F32,))(lambda _a=_a: _argextrema(_a))


@op("stats_planes", (F32,), same=(), pedestal=5.0)
def _():
    return (lambda c: ops.stats_planes(c.cube, mask=c.spec)), (lambda c: E.ref_stats_axis(c.d, c.inc, (1, 2)))


@op("stats_global", same=(), pedestal=5.0)
def _():
    return ((lambda c: {k: np.float64(v) for k, v in ops.stats_global(c.cube, mask=c.spec).items()}),
            (lambda c: E.ref_stats_global(c.d, c.inc)))


@op("percentile_axis2", (F32,), any_order=(F32,))                # (spc_select.hip:419)
def _():
    return ((lambda c: {"median": ops.percentile_axis2(c.cube, 50.0, mask=c.spec).get()}),
            (lambda c: {"median": E.exact(np.nanmedian(np.where(c.inc, c.d, np.nan).astype(np.float32), axis=2))}))


@op("percentile_global", (F32,))
def _():
    return ((lambda c: {"median": np.float32(ops.percentile_global(c.cube, 50.0, mask=c.spec))}),
            (lambda c: {"median": E.exact(np.float32(np.nanmedian(np.where(c.inc, c.d, np.nan).astype(np.float32))))}))


def _keys(x):
    u = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return np.where(u >> 31, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


@op("key_histogram", (F32,))
def _():
    def run(c):
        return {"hist": ops.key_histogram(c.cube, 0, 0, 24, mask=c.spec), "next": np.uint32(ops.key_next(c.cube, 0x80000000, mask=c.spec))}

    def ref(c):
        x = c.d[c.inc & ~np.isnan(c.d)]
        k = _keys(x)
        for v, kk in zip(x[:8], k[:8]):                     # the key is the library's own (a host function)
            assert np.float32(ops.key_to_float(int(kk))) == v
        above = k[k > 0x80000000]
        nxt = above.min() if above.size else 0xffffffff     # (ops.key_next: 0xffffffff when there is none)
        return {"hist": E.exact(np.bincount(k >> 24, minlength=256).astype(np.uint64)), "next": E.exact(np.uint32(nxt))}
    return run, ref


def _spectral_conv(ntaps):
    k = E.taps(ntaps)

    def run(c):
        return {"out": c.read(ops.spectral_conv(c.cube, k, mask=c.spec, out=c.out(c.d.shape, c.dtype)))}
    return run, lambda c: E.ref_spectral_conv(c.d, c.inc, k)


for _n in (9, 17, 33, 49, 65):
    op("spectral_conv[%d]" % _n, (F32, F64) if _n in (9, 33) else (F32,), out=True)(lambda _n=_n: _spectral_conv(_n))
    op("spectral_conv[%d, all valid]" % _n, (F32,), out=True, masked=False)(lambda _n=_n: _spectral_conv(_n))


def _spectral_conv_moments():
    k = E.taps(9)

    def run(c):
        nz = c.d.shape[0]
        r = ops.spectral_conv_moments(c.cube, k, _cen(nz), dv=0.5, m1_add=E.M1_ADD, mask=c.spec, want=E.SUMS, cen_host=E.spectral_centres(nz))
        return {n: r[n].get() for n in E.SUMS}
    return run, lambda c: E.ref_spectral_conv_moments(c.d, c.inc, k)


op("spectral_conv_moments", (F32,), pedestal=5.0)(_spectral_conv_moments)
# (without a mask array the aligned layouts take the algebraic form, spc_spectral_conv.hip:329-331; the others the stencil)
op("spectral_conv_moments[all valid]", (F32,), pedestal=5.0, masked=False)(_spectral_conv_moments)


def _spatial_conv(k2, arithmetic=None):
    def run(c):
        return {"out": c.read(ops.spatial_conv(c.cube, k2, mask=c.spec, out=c.out(c.d.shape, c.dtype), arithmetic=arithmetic))}
    return run, lambda c: E.ref_spatial_conv(c.d, c.inc, k2)


op("spatial_conv[separable, default form]", (F32,), out=True, base=BASE_WIDE)(lambda: _spatial_conv(E._k2(9, 9)))
op("spatial_conv[separable, f32 ring]", (F32,), out=True, base=BASE_WIDE)(lambda: _spatial_conv(E._k2(9, 9), "f32"))
op("spatial_conv[17 taps, f32 ring]", (F32,), out=True, base=BASE_WIDE)(lambda: _spatial_conv(E._k2(17, 17), "f32"))
op("spatial_conv[17 taps, all valid]", (F32,), out=True, masked=False, base=BASE_WIDE)(lambda: _spatial_conv(E._k2(17, 17)))
op("spatial_conv[separable, all valid]", (F32,), out=True, masked=False, base=BASE_WIDE)(lambda: _spatial_conv(E._k2(9, 9)))
op("spatial_conv[9 x 3, not separable]", (F32,), out=True, base=BASE_WIDE)(lambda: _spatial_conv(E._k2(9, 3, False)))
op("spatial_conv[3 x 3, not separable]", (F32, F64), out=True, base=BASE_WIDE)(lambda: _spatial_conv(E._k2(3, 3, False)))
op("spatial_conv[float64 ring]", (F64,), out=True, base=BASE_WIDE)(lambda: _spatial_conv(E._k2(9, 9)))
op("spatial_conv[float64 two passes]", (F64,), out=True, env=(("SPC_SPATIAL64_RING", "0"),), base=BASE_WIDE)(lambda: _spatial_conv(E._k2(9, 9)))


# ---- the matrix-core stencils called directly: ops.spatial_conv_mfma (cube and / or moment 0) and ops.spatial_conv_mfma_moments
def _aligned_to(lay, n, itemsize_units=1):
    return lay.shape[2] % n == 0 and lay.row_stride % n == 0 and lay.plane_stride % n == 0 and lay.offset % n == 0


def _mfma_declines(form, moments):
    """the entry's own conditions (spc_spatial_moment.hip:812-813 with spc_spatial_split.hip:709-710, then :832-839), restated
    on the layouts: the split form wants nx, the strides and the bases of cube and mask multiples of 4 samples / bytes; the
    older forms column pairs (multiples of 2); moments 1 / 2 exist in the split form only"""
    def declines(c):
        split = form == 3 and _aligned_to(c.lay, 4) and _aligned_to(c.mlay, 4)
        if split:
            return None
        if moments:
            return "moments 1 / 2 need the split form"
        if not _aligned_to(c.lay, 2):
            return "8-byte column pairs"
        return None if _aligned_to(c.mlay, 2) else "odd mask strides"
    return declines


_MFMA_DV, _MFMA_M1 = 500.0, 77.0


def _mfma_cen(nz):
    return (np.arange(nz) - nz // 2) * 500.0


def _mfma_ref(c, k2, want):
    """test_mfma_fused_moment0_against_the_oracle (test_gpu_mfma.py:49-65) and test_gpu_round5.py:69-82: the smoothed cube of
    the mask array's samples, its sums under the same mask"""
    sm = _ref("mfma smoothed cube", c, lambda: O.spatial_smooth(c.d, c.inc, k2))          # (one kernel: shared by the rows)
    filled = np.where(c.inc, sm, np.nan)
    e0 = _MFMA_DV * np.nansum(filled, axis=0)
    e0[np.all(np.isnan(filled), axis=0)] = np.nan
    f0, cen = np.nan_to_num(filled, nan=0.0), _mfma_cen(c.d.shape[0])
    s0, s1, s2 = f0.sum(0), (f0 * cen[:, None, None]).sum(0), (f0 * (cen ** 2)[:, None, None]).sum(0)
    e1, e2 = s1 / s0 + _MFMA_M1, s2 / s0 - (s1 / s0) ** 2
    ref = {"out": E.of_max(sm.astype(np.float32), 1e-5), "m0": E.of_max(e0, 1e-5), "m1": E.within(e1, 1e-5 * 500.0 * c.d.shape[0]),
           "m2": E.of_max(e2, 1e-5)}
    return {k: ref[k] for k in want}


def _mfma(want_cube, want_m0):
    k2 = E._k2(9, 9)

    def run(c):
        out, m0 = ops.spatial_conv_mfma(c.cube, k2, mask=c.spec, want_cube=want_cube, want_m0=want_m0, dv=_MFMA_DV)
        return dict(([("out", out.get())] if want_cube else []) + ([("m0", m0.get())] if want_m0 else []))
    return run, lambda c: _mfma_ref(c, k2, (("out",) if want_cube else ()) + (("m0",) if want_m0 else ()))


def _mfma_moments(want_cube):
    k2 = E._k2(9, 9)

    def run(c):
        out, maps = ops.spatial_conv_mfma_moments(c.cube, k2, _dev(_mfma_cen(c.d.shape[0])), dv=_MFMA_DV, m1_add=_MFMA_M1, mask=c.spec,
                                                  want_cube=want_cube)
        res = {k: maps[k].get() for k in ("m0", "m1", "m2")}
        if want_cube:
            res["out"] = out.get()
        return res
    return run, lambda c: _mfma_ref(c, k2, ("m0", "m1", "m2") + (("out",) if want_cube else ()))


# (the sums of a chunk of channels are float32 partials, the forms differ with the mask's strides: against the contiguous cube
# at the tolerance, never bit for bit; 2 + N(0, 1) samples as in test_gpu_mfma.py)
for _form in (3, 2, 1):
    _e = (("SPC_SPATIAL_MFMA_FORM", str(_form)),)
    _t = {3: "split form", 2: "form 2", 1: "form 1"}[_form]
    op("spatial_conv_mfma[%s, cube]" % _t, (F32,), env=_e, base=BASE_WIDE, same=(), pedestal=2.0,
       declines=_mfma_declines(_form, False))(lambda: _mfma(True, False))
    op("spatial_conv_mfma[%s, cube + m0]" % _t, (F32,), env=_e, base=BASE_WIDE, same=(), pedestal=2.0,
       declines=_mfma_declines(_form, False))(lambda: _mfma(True, True))
    op("spatial_conv_mfma[%s, m0 alone]" % _t, (F32,), env=_e, base=BASE_WIDE, same=(), pedestal=2.0,
       declines=_mfma_declines(_form, False))(lambda: _mfma(False, True))
op("spatial_conv_mfma_moments", (F32,), base=BASE_WIDE, same=(), pedestal=2.0, declines=_mfma_declines(3, True))(lambda: _mfma_moments(False))
op("spatial_conv_mfma_moments[with the cube]", (F32,), base=BASE_WIDE, same=(), pedestal=2.0,
   declines=_mfma_declines(3, True))(lambda: _mfma_moments(True))
op("spatial_conv_mfma_moments[older forms: refused]", (F32,), env=(("SPC_SPATIAL_MFMA_FORM", "1"),), base=BASE_WIDE, same=(), pedestal=2.0,
   declines=_mfma_declines(1, True))(lambda: _mfma_moments(False))


def _lerp():
    def run(c):
        lo, t, inv, _, _, fill = ops.lerp_plan(*E.lerp_axes(c.d.shape[0], 0.5))
        return {"out": c.read(ops.spectral_lerp(c.cube, lo, t, inv, fill, mask=c.spec, out=c.out((len(lo),) + c.d.shape[1:], c.dtype)))}
    return run, lambda c: E.ref_spectral_lerp(c.d, c.inc, 0.5)


op("spectral_lerp", out=True)(_lerp)
op("spectral_lerp[untiled]", (F32,), out=True, env=(("SPC_LERP_TILES", "0"),))(_lerp)


def _bilinear(shift, order=1):
    def run(c):
        xs, ys = E.bilinear_maps(c.d.shape, shift)
        out, foot = ops.resample_bilinear(c.cube, xs, ys, mask=c.spec, out=c.out(c.d.shape, c.dtype), order=order)
        return {"out": c.read(out), "foot": foot.get()}

    def ref(c):
        if order == 0:                                   # nearest neighbour on the cube's own grid: the filled cube
            return {"out": E.exact(O.filled(c.d, c.inc).astype(c.dtype)), "foot": E.exact(np.ones(c.d.shape[1:], np.uint8))}
        return E.ref_resample_bilinear(c.d, c.inc, shift)
    return run, ref


op("resample_bilinear[LDS]", out=True)(lambda: _bilinear(0.5))
op("resample_bilinear[gather]", (F32,), out=True, env=(("SPC_BILINEAR_LDS", "0"),))(lambda: _bilinear(0.5))
op("resample_bilinear[nearest, identity]", out=True)(lambda: _bilinear(0.0, 0))


def _bilinear_lerp():
    def run(c):
        xs, ys = E.bilinear_maps(c.d.shape, 0.5)
        lo, t, inv, _, _, fill = ops.lerp_plan(*E.lerp_axes(c.d.shape[0], 0.5))
        out, foot = ops.resample_bilinear_lerp(c.cube, xs, ys, lo, t, inv, fill=fill, mask=c.spec)
        return {"out": out.get(), "foot": foot.get()}
    return run, lambda c: E.ref_resample_bilinear_lerp(c.d, c.inc, 0.5)


op("resample_bilinear_lerp[LDS]", (F32,))(_bilinear_lerp)
op("resample_bilinear_lerp[gather]", (F32,), env=(("SPC_BILINEAR_LDS", "0"),))(_bilinear_lerp)


@op("resample_spline", (F32,), masked=False, finite=True)
def _():
    def run(c):
        xs, ys = E.bilinear_maps(c.d.shape, 0.3)
        out, foot = ops.resample_spline(c.cube, xs, ys, 3)
        return {"out": out.get(), "foot": foot.get()}

    def ref(c):
        xs, ys = E.bilinear_maps(c.d.shape, 0.3)
        e, foot = O.resample_spline(c.d.astype(np.float64), xs, ys, 3)
        return {"out": E.within(e.astype(np.float32), 1e-5 * np.abs(c.d).max()), "foot": E.exact(foot[0].astype(np.uint8))}
    return run, ref


FILL = -7.0


@op("fill_masked", (F32,), out=True)
def _():
    return ((lambda c: {"out": c.read(ops.fill_masked(c.cube, c.spec, FILL, out=c.out(c.d.shape, F32)))}),
            (lambda c: {"out": E.exact(np.where(c.inc, c.d, np.float32(FILL)))}))


@op("fill_masked_transposed", (F32,))
def _():
    return ((lambda c: {"out": ops.fill_masked_transposed(c.cube, c.spec, FILL).get()}),
            (lambda c: {"out": E.exact(np.ascontiguousarray(np.where(c.inc, c.d, np.float32(FILL)).transpose(0, 2, 1)))}))


@op("mask_include")
def _():
    return ((lambda c: {"out": ops.mask_include(c.cube, c.spec, nan_excluded=True).get()}),
            (lambda c: {"out": E.exact((c.inc & ~np.isnan(c.d)).astype(np.uint8))}))


@op("narrow_f64", (F64,), out=True, masked=False)
def _():
    return ((lambda c: {"out": c.read(ops.narrow_f64(c.cube, out=c.out(c.d.shape, F32)))}),
            (lambda c: {"out": E.exact(c.d.astype(np.float32))}))


def _downsample(axis):
    import test_gpu_downsample as DS

    def run(c):
        shape = ops.downsample_shape(c.d.shape, axis, 3, False)
        out = c.out(shape, c.dtype)
        omask = None
        if hasattr(out, "row_stride"):                                   # the two outputs share their geometry
            omask = c.out(shape, np.uint8)
        out, omask = ops.downsample(c.cube, axis, 3, mask=c.spec, out=out, out_mask=omask, nan_excluded=True)
        return {"out": c.read(out), "mask": c.read(omask)}

    def ref(c):
        v = c.inc & ~np.isnan(c.d)
        er, em = DS.restate(c.d, v, np.nan, axis, 3, False, "nanmean")
        return {"out": (er, "one ulp") if c.dtype == F32 else E.within(er, 1e-15 * float(np.nanmax(np.abs(c.d))), 1e-14),
                "mask": E.exact(em.astype(np.uint8))}
    return run, ref


for _a in (0, 1, 2):
    op("downsample_axis%d" % _a, out=True)(lambda _a=_a: _downsample(_a))


_NO_BOX = ((-1, -1),) * 3           # ops.mask_bbox gives None when nothing is included


def _subcube(step):
    def geometry(shape):
        start = (1, 2, 4 if step == 1 else 1)
        return start, (step,) * 3, tuple(len(range(s, n, step)) for s, n in zip(start, shape))

    def run(c):
        start, steps, shape = geometry(c.d.shape)
        shape = shape[:2] + (shape[2] // 4 * 4,)
        out = c.out(shape, c.dtype)
        omask = c.out(shape, np.uint8) if hasattr(out, "row_stride") else None
        out, omask = ops.subcube(c.cube, start, steps, shape, mask=c.spec, out=out, out_mask=omask, nan_excluded=True)
        res = {"out": c.read(out), "mask": c.read(omask)}
        box = ops.mask_bbox(c.cube, mask=c.spec, nan_excluded=True)
        res["bbox"] = np.array(box if box is not None else _NO_BOX, np.int64)
        return res

    def ref(c):
        start, steps, shape = geometry(c.d.shape)
        shape = shape[:2] + (shape[2] // 4 * 4,)
        sl = tuple(slice(s, s + n * step, step) for s, n in zip(start, shape))
        v = c.inc & ~np.isnan(c.d)
        w = np.argwhere(v)
        box = np.array([(w[:, a].min(), w[:, a].max()) for a in range(3)] if len(w) else _NO_BOX, np.int64)
        return {"out": E.exact(c.d[sl]), "mask": E.exact(v[sl].astype(np.uint8)), "bbox": E.exact(box)}
    return run, ref


op("subcube[step 1]", out=True)(lambda: _subcube(1))
op("subcube[step 2]", out=True)(lambda: _subcube(2))


def _rank(sizes):
    import test_gpu_rank_filter as RF
    rank = int(np.prod(sizes)) // 2

    def run(c):
        f = ops.rank_filter_axis0 if len(sizes) == 1 else ops.rank_filter_plane
        return {"out": c.read(f(c.cube, *sizes, rank, mask=c.spec, out=c.out(c.d.shape, c.dtype)))}
    return run, lambda c: {"out": E.exact(RF.expected(c.d, c.inc, np.nan, sizes, rank))}


op("rank_filter_axis0", out=True)(lambda: _rank((5,)))
op("rank_filter_plane", out=True)(lambda: _rank((3, 3)))


def _stack_positions(shape):
    ny, nx = shape[1:]
    idx = np.array([0, nx - 1, nx, (ny - 1) * nx, ny * nx - 1, 3 * nx + 64, 5 * nx + 127, 4 * nx + 128], np.int64)
    return idx, np.linspace(-2.25, 3.5, idx.size)


@op("stack_shift")
def _():
    import test_gpu_stack_spectra as SS

    def run(c):
        idx, shifts = _stack_positions(c.d.shape)
        rows = ops.stack_shift(c.cube, idx, shifts, pad=(1, 2), mask=c.spec).get()
        total, count, nnan = ops.stack_sum(c.cube, idx, shifts, pad=(1, 2), mask=c.spec)
        return {"rows": rows, "sum": total, "count": count, "nan": nnan}

    def ref(c):
        idx, shifts = _stack_positions(c.d.shape)
        f = np.where(c.inc, c.d, np.nan)
        rows, ind, some = SS.restate(f, idx, shifts, (1, 2))
        assert not SS.near_half(ind, some).any(), "an indicator too close to one half for a reference to decide"
        tol = SS.RTOL * (SS.scale_of(f) if np.isfinite(f).any() else 0.0)          # (a mask that includes nothing: every row NaN)
        ok = ~np.isnan(rows)
        return {"rows": E.within(rows.T, tol), "sum": E.within(np.where(ok, rows, 0.0).sum(axis=0), tol * idx.size),
                "count": E.exact(ok.sum(axis=0).astype(np.int64)), "nan": E.exact((~ok).sum(axis=0).astype(np.int64))}
    return run, ref


def _stack_cube_tables(nz):
    n0 = 6
    lo = np.stack([np.arange(n0), np.arange(n0) + 5, np.arange(n0) + nz - n0 - 1]).astype(np.int32)
    t = np.stack([np.full(n0, 0.25), np.zeros(n0), np.full(n0, 0.5)])
    return lo, t, np.ones((3, n0)), np.array([0, 1, 0], np.int32)


@op("stack_cube")
def _():
    import test_gpu_stack_cube as SC
    import test_stack_cube_host as SH
    P = collections.namedtuple("P", "lo t inv_dx exact")

    def run(c):
        lo, t, inv, exact = _stack_cube_tables(c.d.shape[0])
        return {"out": ops.stack_cube(c.cube, lo, t, inv, exact, "nanmean", mask=c.spec, nan_excluded=True).get()}

    def ref(c):
        cuts = SH.emulate(c.d, c.inc & ~np.isnan(c.d), np.nan, P(*_stack_cube_tables(c.d.shape[0])))
        return {"out": E.within(SH.average("nanmean", cuts), SC.bound(c.dtype, SC.scale_of(c.d), "nanmean", 3))}
    return run, ref


def _other(c, name, instead):
    """the layout of a second cube next to *c*'s: *name*, *instead* where *c* has it itself; the one layout of c's shape for
    xwin_tail"""
    if c.lay.name == "xwin_tail":
        return "xwin_tail"
    return instead if c.lay.name == name else name


@op("mosaic")
def _():
    def run(c):
        other = Ctx(c.dtype, _other(c, "xwin_oddstride", "xwin_off1"), "mask_contig", None, **c.given)
        xs, ys = (_dev(a) for a in E.bilinear_maps(c.d.shape, 0.0))
        weights = DeviceArray(c.d.shape[1:], np.int32, 0)
        out = ops.mosaic([c.cube, other.cube], [(xs, ys)] * 2, [c.spec, other.spec], [FILL, FILL], 0, weights=weights)
        return {"out": out.get(), "weights": weights.get()}

    def ref(c):
        f = np.where(c.inc, c.d, c.dtype.type(FILL))
        return {"out": E.exact(np.nan_to_num(f.astype(np.float64)).astype(c.dtype)), "weights": E.exact(np.full(c.d.shape[1:], 2, np.int32))}
    return run, ref


@op("arith", out=True)
def _():
    def operand(c):
        return np.round(V.data(c.dtype.type, V.BASE, seed=9)[0][..., :c.d.shape[2]] * 8) / 8

    def run(c):
        lay = V.layout(_other(c, "xwin_off1", "xwin_aligned"))
        b, _parent = V.upload(lay, operand(c), V.CUBE_POISON[c.dtype])
        steps = [("add", b, True), ("mul", 1.5, False), ("sub", b, False)]
        return {"out": c.read(ops.arith(c.cube, steps, mask=c.spec, fill=FILL, out=c.out(c.d.shape, c.dtype)))}

    def ref(c):
        b = operand(c).astype(c.dtype)
        with np.errstate(all="ignore"):
            return {"out": E.exact((np.where(c.inc, c.d, c.dtype.type(FILL)) + b) * c.dtype.type(1.5) - b)}
    return run, ref


@op("mask_eval", out=True)
def _():
    import types

    def second(c):
        return V.data(c.dtype.type, V.BASE, seed=9)[0][..., :c.d.shape[2]]

    def run(c):
        lay = V.layout(_other(c, "xwin_oddstride", "rows"))
        b, _parent = V.upload(lay, second(c), V.CUBE_POISON[c.dtype])
        prog = types.SimpleNamespace(slots=[c.cube, b], operands=[],
                                     instr=[(_lib.MOP_CMP, 0, _lib.CMP_GT, -1, 0.25), (_lib.MOP_CMP, 1, _lib.CMP_LE, -1, 0.5),
                                            (_lib.MOP_NOT, 0, 0, -1, 0.0), (_lib.MOP_OR, 0, 0, -1, 0.0)])
        return {"out": c.read(ops.mask_eval(prog, c.d.shape, 0, c.dtype, out=c.out(c.d.shape, np.uint8)))}

    def ref(c):
        with np.errstate(invalid="ignore"):
            return {"out": E.exact(((c.d > 0.25) | ~(second(c) <= 0.5)).astype(np.uint8))}
    return run, ref


# ---- the matrix -----------------------------------------------------------------------------------------------------
def _combos(o, dtype):
    """(cube layout, mask layout, output layout): every cube layout with mask_same, every mask layout with xwin_aligned and
    xwin_off1, every output layout with xwin_aligned"""
    swap = dtype in o.any_order
    cubes = V.CUBE_LAYOUTS + (("swap01",) if swap else ())
    combos = [(c, "mask_same", "contig") for c in cubes]
    if o.masked:
        combos += [(c, m, "contig") for c in ("xwin_aligned", "xwin_off1") for m in ("mask_contig", "mask_phase")]
        if swap:
            combos.append(("swap01", "mask_contig", "contig"))
    if o.out:
        combos += [("xwin_aligned", "mask_same", oname) for oname in V.OUT_LAYOUTS[1:]]
    return combos


def _one_ulp(got, exp64, what):
    import test_gpu_downsample as DS
    DS.within_one_ulp(got, exp64, what)


def _sigma_rule(got, exp, what):
    """test_sigma_clip_fused_kernel's: float32-against-float64 bounds move borderline samples only"""
    assert got.shape == exp.shape and np.mean(np.isnan(got) != np.isnan(exp)) < 2e-4, what + ": clipped set"
    ok = ~np.isnan(got) & ~np.isnan(exp)
    assert np.array_equal(got[ok], exp[ok].astype(got.dtype)), what + ": kept values"


def _check(got, ref, what):
    plain = {}
    for k, (e, groups) in ref.items():
        if groups == "one ulp":
            _one_ulp(got[k], e, "%s: %s" % (what, k))
        elif groups == "sigma_clip":
            _sigma_rule(got[k], e, "%s: %s" % (what, k))
        else:
            plain[k] = (e, groups)
    E.check(got, plain, what)


def _against_contig(o, got, base, ref, same, what):
    """the view's result against the contiguous one: bit for bit where the same form ran (and for every exact output), else at
    the reference's tolerance"""
    for k, (e, groups) in ref.items():
        g, b = np.asarray(got[k]), np.asarray(base[k])
        exact = same or groups == "sigma_clip" or (not isinstance(groups, str) and all(a is None for _, a, _ in groups))
        if exact:
            _bits(g, b, "%s: %s against the contiguous cube" % (what, k))
        elif groups == "one ulp":
            with np.errstate(invalid="ignore"):
                assert np.array_equal(np.isnan(g), np.isnan(b)) and (np.abs(g - b)[~np.isnan(b)] <= np.spacing(np.abs(b[~np.isnan(b)]))).all(), what
        else:
            E.check({k: g}, {k: (b, groups)}, what + " against the contiguous cube")


CASES = [(name, dt) for name, o in OPS.items() for dt in o.dtypes]


@pytest.mark.parametrize("name,dtype", CASES, ids=["%s-%s" % (n.replace(" ", "_"), d.name) for n, d in CASES])
def test_operator_on_every_view(gpu, name, dtype):
    o = OPS[name]
    failed = []
    base = None
    with _env(o.env):
        for cname, mname, oname in _combos(o, dtype):
            what = "%s %s: cube %s, mask %s, out %s" % (name, dtype.name, cname, mname if o.masked else "-", oname if o.out else "-")
            c = Ctx(dtype, cname, mname, oname, base=o.base, masked=o.masked, finite=o.finite, pedestal=o.pedestal)
            why = o.declines(c) if o.declines else None
            if why is not None:                                 # refused by design: the message, and nothing else to check
                try:
                    o.run(c)
                    failed.append(what + ": ran, where the entry declines (%s)" % why)
                except _lib.HipUnsupported as err:
                    if not re.search(why, str(err)):
                        failed.append(what + ": refused with %r, not %r" % (str(err)[:200], why))
                continue
            ref = _ref(name, c, lambda: o.ref(c))
            got = o.run(c)
            for lay, parent in c._outs:                         # (an output the runner did not read back itself)
                assert V.read_output(lay, parent)[1], what + ": wrote outside the output view"
            try:
                _check(got, ref, what)
                if cname == "contig" and mname == "mask_same" and oname == "contig":
                    base = got
                elif base is not None and c.lay.shape == V.layout("contig", o.base).shape:
                    same = cname in o.same and mname in ("mask_same", "mask_contig") and oname in ("contig", "out_xwin_aligned")
                    _against_contig(o, got, base, ref, same, what)
            except AssertionError as err:                       # every layout is tried: the report names all that miss
                failed.append("%s: %s" % (what, str(err).splitlines()[0][:300]))
    assert not failed, "%d of %d layouts:\n%s" % (len(failed), len(_combos(o, dtype)), "\n".join(failed[:12]))


def test_float64_percentile_with_its_keys_in_lds(gpu):
    """SPC_SELECT64 is read once per process (spc_select_f64.hip:632): the float64 selection that keeps its keys in LDS runs
    the same row of the matrix in a fresh process"""
    import subprocess
    import sys
    env = dict(os.environ, SPC_SELECT64="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-p", "no:cacheprovider",
                        "-k", "test_operator_on_every_view and percentile_axis0-float64"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "1 passed" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]


def _row_of(name):
    stem = name.split("[")[0]
    for a in ("_axis0", "_axis1", "_axis2"):
        if stem.endswith(a) and stem not in ("percentile_axis0", "percentile_axis2", "sigma_clip_axis0", "rank_filter_axis0"):
            stem = stem[:-len(a)]
    return {"stats": "stats_axis", "argextrema": "argextrema_axis", "fill_masked_transposed": "fill_masked", "mask_include": "fill_masked",
            "narrow_f64": "fill_masked", "rank_filter_axis0": "rank_filter", "rank_filter_plane": "rank_filter",
            "resample_bilinear_lerp": "resample_bilinear"}.get(stem, stem)


# ops functions with a cube parameter -> the TABLE row that runs them (None: no device work on the cube's samples)
ROW_OF_OPS_FUNCTION = {
    "moments": "moments", "moments_f64": "moments_f64", "moment_order": "moment_order", "moment_order_f64": "moment_order",
    "sigma_clip_axis0": "sigma_clip_axis0", "sigma_clip_axis0_f64": "sigma_clip_axis0", "narrow_f64": "fill_masked",
    "argextrema_axis": "argextrema_axis", "moments_spatial": "moments_spatial", "moment_order_spatial": "moments_spatial",
    "spectral_conv": "spectral_conv", "downsample": "downsample", "rank_filter_axis0": "rank_filter", "rank_filter_plane": "rank_filter",
    "stack_shift": "stack_shift", "stack_sum": "stack_shift", "stack_cube": "stack_cube", "subcube": "subcube", "arith": "arith",
    "mask_bbox": "subcube", "spectral_conv_moments": "spectral_conv_moments", "spatial_conv": "spatial_conv",
    "spatial_conv_mfma": "spatial_conv_mfma", "spatial_conv_mfma_moments": "spatial_conv_mfma_moments", "spectral_lerp": "spectral_lerp",
    "resample_bilinear": "resample_bilinear", "resample_bilinear_lerp": "resample_bilinear", "resample_spline": "resample_spline",
    "stats_global": "stats_global", "stats_planes": "stats_planes", "stats_axis": "stats_axis", "stats_dev_axis": "stats_dev_axis",
    "percentile_axis0": "percentile_axis0", "fill_masked": "fill_masked", "mask_include": "fill_masked", "percentile_axis2": "percentile_axis2",
    "percentile_global": "percentile_global", "key_histogram": "key_histogram", "key_next": "key_histogram",
    "fill_masked_transposed": "fill_masked",
}


def test_table_names_every_operator_of_the_matrix_and_every_ops_function_that_takes_a_cube():
    import inspect
    rows = {r[0] for r in TABLE}
    assert {_row_of(name) for name in OPS} == rows
    for n, f in vars(ops).items():
        if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_") and "cube" in inspect.signature(f).parameters:
            assert ROW_OF_OPS_FUNCTION.get(f.__name__) in rows, "ops.%s takes a cube and has no row" % n
    # (mosaic and mask_eval take their cubes as lists / slots)
    assert {"mosaic", "mask_eval"} <= rows


# ---- refusals: decided by the entry's SPC_REQUIREs, before any launch --------------------------------------------------------
def test_swap01_is_refused_by_the_entries_that_check_plane_order(gpu, monkeypatch):
    """spc_check_cube (spc_common.h:206) refuses a view whose rows lie a plane apart; only the entries that call
    spc_check_cube_any_order (percentile_axis0 float32 and float64, percentile_axis2, the fused sigma_clip_axis0) take it: the
    matrix runs those on swap01.  The loop form of sigma clipping starts with fill_masked and refuses with it"""
    monkeypatch.setenv("SPC_SIGMA_CLIP_FUSED", "0")
    for dtype in (F32, F64):
        c = Ctx(dtype, "swap01", "mask_same", "contig")
        calls = [lambda: ops.stats_axis(c.cube, 0, mask=c.spec), lambda: ops.stats_global(c.cube, mask=c.spec),
                 lambda: ops.spectral_conv(c.cube, E.taps(9), mask=c.spec), lambda: ops.spatial_conv(c.cube, E._k2(3, 3), mask=c.spec),
                 lambda: ops.mask_include(c.cube, c.spec), lambda: ops.downsample(c.cube, 0, 3, mask=c.spec),
                 lambda: ops.arith(c.cube, [("mul", 2.0, False)], mask=c.spec)]
        if dtype == F32:
            calls += [lambda: ops.moments(c.cube, _cen(c.d.shape[0]), mask=c.spec), lambda: ops.fill_masked(c.cube, c.spec),
                      lambda: ops.stats_planes(c.cube, mask=c.spec), lambda: ops.percentile_global(c.cube, 50.0, mask=c.spec),
                      lambda: ops.sigma_clip_axis0(c.cube, mask=c.spec)]
        else:
            calls += [lambda: ops.moments_f64(c.cube, _cen(c.d.shape[0]), mask=c.spec), lambda: ops.narrow_f64(c.cube),
                      lambda: ops.sigma_clip_axis0_f64(c.cube, mask=c.spec)]
        for i, call in enumerate(calls):
            with pytest.raises(_lib.HipInvalidArgument, match="plane_stride too small") as hit:
                call()
            assert hit.type is _lib.HipInvalidArgument, "%s call %d" % (dtype.name, i)


def test_mosaic_output_is_contiguous_by_contract(gpu):
    c = Ctx(F32, "xwin_aligned", "mask_same", "out_xwin_aligned")
    xs, ys = (_dev(a) for a in E.bilinear_maps(c.d.shape, 0.0))
    with pytest.raises(ValueError, match="contiguous"):
        ops.mosaic([c.cube], [(xs, ys)], [c.spec], [FILL], 0, out=c.out(c.d.shape, F32))
