"""Every operator on dirty scratch and recycled device memory (tests/dirty_memory.py).

``ops.workspace()`` hands every entry the leftovers of the operator before it, ``spc_malloc`` hands freed blocks out again:
what a clean test run sees depends on test order.  Every row below runs once per pattern of ``dirty_memory.PATTERNS`` - the
cached scratch and every fresh allocation hold 0x00, 0xFF, 0x7F or seeded random bytes - and is held to ONE rule: the
results are bit-identical under the four patterns (NaN equal to NaN, dtype and shape too), and the first result passes the
existing reference check of that case at its existing tolerance.  No new tolerance is introduced here: each row names the
test its data and reference are taken from.

  A  every dispatch route of the hot-path operators: mask_edges.CASES through test_gpu_mask_edges._run, under five masks
     chosen by their flags (none, isfinite, > 0.1, the array term alone, isfinite & array: between them every kernel variant
     the 66 masks select)
  B  every ops function that takes a cube: test_gpu_views.CASES on the contiguous layout, with FRESH outputs (the views
     matrix hands every operator a prepared out= array; here the operator allocates its own, which arrives dirty)
  C  routes with more than one chunk, tile or partial record, which neither views.BASE nor the mask-edge shapes reach
  D  chains through SpectralCube, where one operator's scratch is the next one's

The audit that goes with these rows - who writes and who reads every scratch region and fresh allocation - is the table
"What memory an entry may assume" in docs/DESIGN_NOTES.md."""
import collections
import re
import warnings

import numpy as np
import pytest

import dirty_memory as DM
import mask_edges as E
import oracle_np as O
import test_gpu_mask_edges as ME
import test_gpu_views as V
from conftest import assert_close, golden
from spectral_cube_amd import Gaussian1DKernel, Gaussian2DKernel, SpectralCube, _lib, ops
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

F32, F64 = V.F32, V.F64


def _dev(a):
    return DeviceArray.from_numpy(np.ascontiguousarray(a), 0)


def _quiet(fn):
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        return fn()


# ---- the helper itself, on the device: the fills land where the operators will look ------------------------------------------------
@pytest.mark.parametrize("pattern", DM.PATTERNS, ids=[str(p) for p in DM.PATTERNS])
def test_dirty_reaches_the_cached_scratch_and_every_fresh_allocation(gpu, pattern):
    ops.workspace(0, None, _lib.WS_STATS_PLANES, 3, 130, 130)           # (a cached scratch buffer of this thread exists)
    with DM.dirty(pattern) as f:
        cached = list(ops._ws_cache.values())
        assert cached and f.count == len(cached)
        for i, buf in enumerate(cached):
            view = DeviceArray((buf.nbytes,), np.uint8, buf.device, ptr=buf.ptr, owner=buf)
            assert np.array_equal(view.get(), DM.pattern_bytes(pattern, buf.nbytes, i)), "cached scratch %d" % i
        fresh = DeviceArray((37, 5), np.float32, 0)
        assert fresh.get().tobytes() == DM.pattern_bytes(pattern, fresh.nbytes, len(cached)).tobytes()
        assert (DeviceArray.zeros((9,), np.float64, 0).get() == 0).all()
        assert np.array_equal(_dev(np.arange(7.0)).get(), np.arange(7.0))
        # a request larger than every cached buffer: the scratch grows inside the block, and the new block is filled too
        nx, held = 256, max(b.nbytes for b in cached)
        while int(_lib.load().spc_workspace_bytes(_lib.WS_SPATIAL_CONV_MFMA, 8, 256, nx, 1, 0)) <= held:
            nx *= 2
        grown, n = ops.workspace(0, None, _lib.WS_SPATIAL_CONV_MFMA, 8, 256, nx, 1, 0)
        assert n > held and grown.value not in {b.ptr for b in cached}
        view = DeviceArray((n,), np.uint8, 0, ptr=grown.value)
        assert np.array_equal(view.get(), DM.pattern_bytes(pattern, n, f.count - 1)), "scratch grown inside the block"
    ops.release_workspaces()                 # (the grown scratch would be refilled on every later entry: back to the pool)


# ---- A: every dispatch route of the hot-path operators -----------------------------------------------------------------------
FIVE = (("no mask", lambda m: m.flags == 0 and not m.with_array),
        ("isfinite", lambda m: m.flags == _lib.MASK_FINITE and not m.with_array),
        ("one threshold (> 0.1)", lambda m: m.flags == _lib.MASK_GT and m.lo == 0.1 and not m.with_array),
        ("the array term alone", lambda m: m.flags == 0 and m.with_array),
        ("isfinite & array", lambda m: m.flags == _lib.MASK_FINITE and m.with_array))


def five_masks(dtype):
    """the five masks of mask_edges.masks, selected by flags, never by position"""
    out = []
    for what, pred in FIVE:
        hits = [m for m in E.masks(dtype) if pred(m)]
        assert len(hits) == 1, (what, [m.name for m in hits])
        out.append(hits[0])
    return out


A_CASES = list(E.CASES)


@pytest.mark.parametrize("case", A_CASES, ids=E.case_id)
def test_hot_path_route_on_dirty_memory(gpu, monkeypatch, case):
    if case.op in E.BLENDS:
        for name, value in case.par[1]:
            monkeypatch.setenv(name, value)
    cache = E.RefCache(case)
    dev, dev_arr = _dev(cache.d), _dev(cache.arr)
    aux = {"cen": _dev(E.spectral_centres(case.shape[0]))}
    if case.op == "moments_spatial":
        aux["cen2d"] = _dev(E.spatial_centres(case.shape, case.par))
    masks = five_masks(case.dtype)

    def run():
        out = {}
        for m in masks:
            for k, v in ME._run(case, dev, ME._spec(m, dev_arr), aux).items():
                out["%s: %s" % (m.name, k)] = v
        return out

    def check(first):
        for m in masks:
            ref = cache.expected(m)
            E.check({k: first["%s: %s" % (m.name, k)] for k in ref}, ref, "%s (%s) %s: %s" % (case.op, case.path, case.shape, m.name))

    DM.same_under_every_pattern(run, check)


def test_matrix_a_covers_every_mask_edge_case_and_five_kinds_of_mask():
    assert len(A_CASES) == len(E.CASES) and all(a is b for a, b in zip(A_CASES, E.CASES))
    assert len({id(c) for c in A_CASES}) == len(E.CASES)
    for dtype in (np.float32, np.float64):
        got = five_masks(dtype)
        assert len({m.name for m in got}) == 5
        assert [(bool(m.flags & _lib.MASK_FINITE), bool(m.flags & E.THRESHOLD_FLAGS), m.with_array) for m in got] == [
            (False, False, False), (True, False, False), (False, True, False), (False, False, True), (True, False, True)]


# ---- B: every ops function that takes a cube ---------------------------------------------------------------------------------
class FreshOutputs(V.Ctx):
    """the contiguous case of the views matrix, with outputs the operator allocates itself (they arrive dirty)"""

    def out(self, shape, dtype):
        return None


@pytest.mark.parametrize("name,dtype", V.CASES, ids=["%s-%s" % (n.replace(" ", "_"), d.name) for n, d in V.CASES])
def test_operator_on_dirty_memory(gpu, name, dtype):
    o = V.OPS[name]
    what = "%s %s on dirty memory" % (name, dtype.name)
    with V._env(o.env):
        c = FreshOutputs(dtype, "contig", "mask_same", "contig", base=o.base, masked=o.masked, finite=o.finite, pedestal=o.pedestal)
        why = o.declines(c) if o.declines else None
        if why is not None:                                     # refused by design, whatever memory holds
            for p in DM.PATTERNS:
                with DM.dirty(p), pytest.raises(_lib.HipUnsupported) as hit:
                    o.run(c)
                assert re.search(why, str(hit.value)), (p, str(hit.value)[:200], why)
            return
        ref = V._ref(name, c, lambda: o.ref(c))
        fresh = DM.same_under_every_pattern(lambda: o.run(c), lambda first: V._check(first, ref, what))
        if o.out:                                               # and as the views matrix calls it, into a prepared out= array
            given = V.Ctx(dtype, "contig", "mask_same", "contig", base=o.base, masked=o.masked, finite=o.finite, pedestal=o.pedestal)
            first = DM.same_under_every_pattern(lambda: o.run(given), lambda r: V._check(r, ref, what + ", out= given"))
            for lay, parent in given._outs:
                assert V.V.read_output(lay, parent)[1], what + ": wrote outside the output it was given"
            assert DM.compare(fresh, first, "out= given", "a fresh output") == [], "a fresh output and a given one differ"


def test_matrix_b_covers_every_operator_of_the_views_matrix():
    assert {n for n, _ in V.CASES} == set(V.OPS) and len(V.CASES) == sum(len(o.dtypes) for o in V.OPS.values())
    rows = {r[0] for r in V.TABLE}
    assert {V._row_of(n) for n, _ in V.CASES} == rows, "a row of test_gpu_views.TABLE has no case here"
    declined = [n for n, d in V.CASES if V.OPS[n].declines is not None]
    assert declined and all(n.startswith("spatial_conv_mfma") for n in declined)


# ---- C: routes with more than one chunk, tile or partial record ------------------------------------------------------------------
Row = collections.namedtuple("Row", "name env build")
ROWS = collections.OrderedDict()
_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = _quiet(fn)
    return _MEMO[key]


def row(name, env=()):
    """``build()`` -> (run, check): run() gives {output: host array}, check(first result) is the named test's own check"""
    def deco(build):
        assert name not in ROWS
        ROWS[name] = Row(name, tuple(env), build)
        return build
    return deco


def _array_spec(m, flags=0):
    return ops.MaskSpec(_lib.MASK_ARRAY | flags, array=_dev(m.astype(np.uint8)))


# split / matrix-core stencil with nchunk > 1: test_mfma_many_channels_several_chunks (test_gpu_mfma.py), moments 0 1 2 as
# test_split_form_fused_moments_012_against_the_oracle (test_gpu_round5.py)
def _chunks_case():
    import test_gpu_mfma as MF
    shape = (150, 16, 96)
    d, m = MF._case(shape, 5, valid=0.6)
    k2 = Gaussian2DKernel(2.0).array
    sm = _memo("mfma chunks", lambda: O.spatial_smooth(d, m, k2))
    return shape, d, m, k2, sm


def _chunks(want_cube, want_m0, moments=False):
    def build():
        shape, d, m, k2, sm = _chunks_case()
        cube, spec = _dev(d), _array_spec(m)
        filled = np.where(m, sm, np.nan)
        if moments:
            cen = (np.arange(shape[0]) - shape[0] // 2) * 500.0
            dcen = _dev(cen)

            def run():
                _, maps = ops.spatial_conv_mfma_moments(cube, k2, dcen, dv=500.0, m1_add=77.0, mask=spec)
                return {k: maps[k].get() for k in ("m0", "m1", "m2")}

            def check(r):
                e0 = 500.0 * np.nansum(filled, axis=0)
                e0[np.all(np.isnan(filled), axis=0)] = np.nan
                f0 = np.nan_to_num(filled, nan=0.0)
                s0, s1, s2 = f0.sum(0), (f0 * cen[:, None, None]).sum(0), (f0 * (cen ** 2)[:, None, None]).sum(0)
                with np.errstate(all="ignore"):
                    e1, e2 = s1 / s0 + 77.0, s2 / s0 - (s1 / s0) ** 2
                assert_close(r["m0"], e0, atol=1e-5 * np.nanmax(np.abs(e0)), what="fused m0")
                assert_close(r["m1"], e1, atol=1e-5 * 500.0 * shape[0], what="fused m1")
                assert_close(r["m2"], e2, atol=1e-5 * np.nanmax(np.abs(e2)), what="fused m2")
            return run, check

        def run():
            out, m0 = ops.spatial_conv_mfma(cube, k2, mask=spec, want_cube=want_cube, want_m0=want_m0, dv=2.0)
            return dict(([("out", out.get())] if want_cube else []) + ([("m0", m0.get())] if want_m0 else []))

        def check(r):
            if want_cube:
                assert_close(r["out"], sm.astype(np.float32), atol=1e-5 * np.nanmax(np.abs(sm)), what="mfma smooth 17 taps")
            if want_m0:
                exp = 2.0 * np.nansum(filled, axis=0)
                exp[np.all(np.isnan(filled), axis=0)] = np.nan
                assert_close(r["m0"], exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="mfma moment0 chunks")
        return run, check
    return build


for _form, _t in ((3, "split form"), (2, "form 2"), (1, "form 1")):
    _e = (("SPC_SPATIAL_MFMA_FORM", str(_form)),)
    row("matrix-core stencil, several chunks [%s, m0 alone]" % _t, _e)(_chunks(False, True))
    row("matrix-core stencil, several chunks [%s, cube + m0]" % _t, _e)(_chunks(True, True))
row("matrix-core stencil, several chunks [split form, m0 m1 m2]")(_chunks(False, True, moments=True))


@row("fused moment on a sparse mask: unseen spaxels")                  # test_split_form_zero_sums_are_not_taken_for_unseen_spaxels
def _():
    import test_gpu_round5 as R5
    d = np.zeros((6, 32, 64), np.float32)
    d[:, 16:] = -0.0
    d[:, :, 40:] = 1.5
    m = np.ones(d.shape, bool)
    m[:, 5:9, 5:9] = False
    cube, spec = _dev(d), _array_spec(m)

    def run():
        return {"m0": ops.spatial_conv_mfma(cube, R5.K8, mask=spec, want_cube=False, want_m0=True, dv=2.0)[1].get()}

    def check(r):
        got = r["m0"]
        assert np.isnan(got[5:9, 5:9]).all() and np.isnan(got).sum() == 16
        assert (got[:, :20][~np.isnan(got[:, :20])] == 0.0).all()
        exp = 2.0 * np.nansum(np.where(m, _memo("zero sums", lambda: O.spatial_smooth(d, m, R5.K8)), np.nan), axis=0)
        exp[5:9, 5:9] = np.nan
        assert_close(got, exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="zero sums")
    return run, check


def _wide_ring():                                                       # test_spectral_smooth_wide_symmetric_rings, 41 taps
    ntaps = 41
    shape = (3 * ntaps + 5, 6, 300)
    assert shape == (128, 6, 300)
    rng = np.random.default_rng(ntaps)
    d = rng.standard_normal(shape).astype(np.float32) + 1.0
    d[ntaps, 2, 17] = np.nan                 # one flagged 128-column status tile, the others stay on the ring
    d[0, 5, 299] = np.nan
    k = np.exp(-0.5 * ((np.arange(ntaps) - ntaps // 2) / (ntaps / 8.0)) ** 2)
    cube, spec = _dev(d), ops.MaskSpec(_lib.MASK_FINITE)

    def check(r):
        exp = _memo("wide ring", lambda: O.spectral_smooth(d, np.isfinite(d), k))
        assert np.array_equal(np.isnan(r["out"]), np.isnan(exp))
        np.testing.assert_allclose(r["out"], exp, rtol=1e-6, atol=1e-6, equal_nan=True)
    return (lambda: {"out": ops.spectral_conv(cube, k, mask=spec).get()}), check


row("spectral stencil, 41 taps, several status tiles, one flagged")(_wide_ring)
row("spectral stencil, 41 taps, the runs-of-16 kernel alone", (("SPC_CONV_FAST", "0"),))(_wide_ring)


def _flag_tiles(shape):                                                 # test_fused_smooth_moments_rows_across_flag_tiles
    def build():
        rng = np.random.default_rng(shape[2])
        nz = shape[0]
        d = (rng.standard_normal(shape) * 3 + 1).astype(np.float32)
        d[rng.random(shape) < 0.02 / max(nz // 4, 1)] = np.nan
        k = np.abs(rng.standard_normal(15)) + 0.05
        cen = np.cumsum(rng.uniform(0.5, 1.5, nz))
        cref = cen[nz // 2]
        cube, dcen = _dev(d), _dev(cen - cref)

        def run():                                                      # (fresh output maps: they arrive dirty)
            r = ops.spectral_conv_moments(cube, k, dcen, dv=1.3, m1_add=cref + 10.0, want=("m0", "m1"), cen_host=cen - cref)
            return {"m0": r["m0"].get(), "m1": r["m1"].get()}

        def check(r):
            sm = O.spectral_smooth(d, None, k)
            e0 = O.moment(sm, None, 0, cen, 1.3)
            e1 = O.moment(sm, None, 1, cen, 1.3, world0=10.0)
            assert_close(r["m0"], e0, atol=1e-5 * np.nanmax(np.abs(e0)), what="fused m0")
            wc = np.abs(e0) > 1e-2 * np.nanmax(np.abs(e0))
            assert_close(np.where(wc, r["m1"], 0.0), np.where(wc, e1, 0.0), atol=1e-5 * max(cen[-1] - cen[0], 1.0), what="fused m1")
        return run, lambda r: _quiet(lambda: check(r))
    return build


for _s in ((1, 68, 76), (7, 33, 100), (40, 9, 260)):
    row("fused smooth -> moments across flag tiles %s" % (_s,))(_flag_tiles(_s))


@row("spectral stencil, masked table denominators, z split (300, 5, 7), 17 taps")  # test_spectral_smooth_masked_table_denominators
def _():
    shape, ntaps = (300, 5, 7), 17
    rng = np.random.default_rng(ntaps * 7 + shape[0])
    d = rng.standard_normal(shape).astype(np.float32) + 3.0
    d[rng.random(shape) < 0.03] = np.nan
    inc = rng.random(shape) < 0.6
    inc[40:40 + 2 * ntaps, 1, 2] = False
    inc[:ntaps, 0, 0] = False
    inc[:, 2, 3] = True
    k = np.exp(-0.5 * (np.arange(ntaps) - ntaps // 2) ** 2 / (ntaps / 6.0) ** 2)
    cen = (np.arange(shape[0]) - shape[0] // 2) * 0.5
    cube, dcen, spec = _dev(d), _dev(cen), _array_spec(inc, _lib.MASK_FINITE)

    def run():
        r = ops.spectral_conv_moments(cube, k, dcen, mask=spec, cen_host=cen, want=("m0", "m1"))
        return {"out": ops.spectral_conv(cube, k, mask=spec).get(), "m0": r["m0"].get(), "m1": r["m1"].get()}

    def check(r):
        exp = O.spectral_smooth(d, inc, k)
        assert np.array_equal(np.isnan(r["out"]), np.isnan(exp))
        ok = ~np.isnan(exp)
        np.testing.assert_allclose(r["out"][ok], exp[ok], rtol=1e-6, atol=1e-6)
        einc = inc & np.isfinite(d)
        e0 = O.moment(exp.astype(np.float32), einc, 0, cen, 1.0)
        e1 = O.moment(exp.astype(np.float32), einc, 1, cen, 1.0)
        assert_close(r["m0"], e0, atol=1e-5 * np.nanmax(np.abs(e0)), what="fused m0")
        wc = np.abs(e0) > 1e-3 * np.nanmax(np.abs(e0))
        assert_close(np.where(wc, r["m1"], 0.0), np.where(wc, e1, 0.0), atol=1e-5 * np.abs(cen).max(), what="fused m1")
    return run, lambda r: _quiet(lambda: check(r))


def _wide_spatial(array_mask):                                          # test_spatial_smooth_wide_rings, taps (41, 41)
    def build():
        ny_t = nx_t = 41
        rng = np.random.default_rng(ny_t + nx_t)
        shape = (3, 90, 900)
        d = rng.standard_normal(shape).astype(np.float32) + 2.0
        d[1, 40, 300] = np.nan
        g = np.exp(-0.5 * ((np.arange(ny_t) - ny_t // 2) / (ny_t / 8.0)) ** 2)
        k2 = np.outer(g, g)
        inc = rng.random(shape) < 0.7
        cube = _dev(d)
        spec = _array_spec(inc, _lib.MASK_FINITE) if array_mask else ops.MaskSpec(_lib.MASK_FINITE)
        valid = (inc & np.isfinite(d)) if array_mask else np.isfinite(d)

        def check(r):
            exp = _memo(("wide spatial", array_mask), lambda: O.spatial_smooth(d, valid, k2))
            assert_close(r["out"], exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="41 x 41 taps, %s" % ("array mask" if array_mask else "finite mask"))
        return (lambda: {"out": ops.spatial_conv(cube, k2, mask=spec).get()}), check
    return build


row("spatial stencil, 41 x 41 taps, one NaN, isfinite mask")(_wide_spatial(False))
row("spatial stencil, 41 x 41 taps, one NaN, array mask")(_wide_spatial(True))


@row("spatial stencil, rotated 13 x 13 kernel, all-valid pass and flagged tiles")     # test_nonseparable_stencil_all_valid_pass
def _():
    rng = np.random.default_rng(8)
    shape = (2, 75, 330)
    d = rng.standard_normal(shape).astype(np.float32) + 1.0
    d[1, 40, 200] = np.nan
    yy, xx = np.mgrid[-6:7, -6:7]
    kn = np.exp(-0.5 * (((xx + 0.5 * yy) / 2.0) ** 2 + (yy / 1.2) ** 2))
    cube, spec = _dev(d), ops.MaskSpec(_lib.MASK_FINITE)

    def check(r):
        exp = _memo("rotated", lambda: O.spatial_smooth(d, np.isfinite(d), kn))
        assert_close(r["out"], exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="two-pass 2-D stencil")
    return (lambda: {"out": ops.spatial_conv(cube, kn, mask=spec).get()}), check


def _bilinear(scale, angle):                                            # test_resample_bilinear_lds_and_gather_paths_agree
    def build():
        rng = np.random.default_rng(17)
        nz, ny, nx = 9, 150, 170
        d = rng.standard_normal((nz, ny, nx)).astype(np.float32)
        d[3, 40:45, 50:60] = np.nan
        inc = rng.random((nz, ny, nx)) > 0.15
        nyo, nxo = 131, 157
        yy, xx = np.mgrid[0:nyo, 0:nxo].astype(np.float64)
        a = np.deg2rad(angle)
        xs = scale * (np.cos(a) * (xx - nxo / 2) - np.sin(a) * (yy - nyo / 2)) + nx / 2 + 0.123
        ys = scale * (np.sin(a) * (xx - nxo / 2) + np.cos(a) * (yy - nyo / 2)) + ny / 2 - 0.371
        cube = _dev(d)
        specs = (("no mask", None), ("array", _array_spec(inc)), ("predicate", ops.MaskSpec(_lib.MASK_GT | _lib.MASK_FINITE, -0.5)))

        def run():
            out = {}
            for what, spec in specs:
                o, f = ops.resample_bilinear(cube, xs, ys, mask=spec, fill=np.nan)
                out[what + ": out"], out[what + ": foot"] = o.get(), f.get()
            return out

        def check(r):
            exp, ef = _memo(("bilinear", scale, angle), lambda: O.resample_bilinear(np.where(inc, d, np.nan).astype(np.float32), xs, ys))
            assert_close(r["array: out"], exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="bilinear vs oracle")
            assert np.array_equal(r["array: foot"].astype(bool), ef[0])
        return run, check
    return build


for _scale, _angle in ((1.0, 30.0), (3.0, 20.0)):            # (the second overflows the LDS footprint: flagged tiles go to the gather kernel)
    for _lds in ("1", "0"):
        row("resample_bilinear, scale %g, angle %g, SPC_BILINEAR_LDS=%s" % (_scale, _angle, _lds), (("SPC_BILINEAR_LDS", _lds),))(
            _bilinear(_scale, _angle))


@row("resample_bilinear_lerp, 17 -> 40 channels, 64 x 64 tiles")         # test_bilinear_with_the_spectral_interpolation_folded_in, first case
def _():
    import test_gpu_round5 as R5
    shape, (nzo, nyo, nxo) = (17, 90, 130), (40, 150, 170)
    rng = np.random.default_rng(90 + shape[0])
    nz, ny, nx = shape
    d = (rng.standard_normal(shape) * 2 + 1).astype(np.float32)
    d[rng.random(d.shape) < 0.01] = np.nan
    inc = rng.random(d.shape) > 0.15
    xs, ys = R5._rot_map(nyo, nxo, ny, nx, 30.0, 1.0, (1.3, -0.7))
    xin = np.cumsum(rng.uniform(0.5, 1.5, nz))
    xout = np.linspace(xin[0], xin[-1], nzo)
    lo, t, inv, _, _, _ = ops.lerp_plan(xin, xout)
    cube, spec = _dev(d), _array_spec(inc)

    def run():
        got, foot = ops.resample_bilinear_lerp(cube, xs, ys, lo, t, inv, mask=spec, order=1)
        return {"out": got.get(), "foot": foot.get()}

    def check(r):
        ei, _ = O.spectral_interpolate(d, inc, xin, xout)
        exp, ef = O.resample_bilinear(ei, xs, ys)
        assert r["out"].shape == (nzo, nyo, nxo) and np.array_equal(r["foot"].astype(bool), ef[0])
        assert_close(r["out"], exp.astype(np.float32), atol=1e-5 * np.nanmax(np.abs(exp)), what="folded interpolation vs oracle")
    return run, lambda r: _quiet(lambda: check(r))


def _noisy(shape, dtype=np.float32, seed=None):
    """the data of test_stats_planes (test_gpu_ops.py): normal samples, a tenth NaN, a mask array that keeps 70 % and no
    sample of plane 1"""
    rng = np.random.default_rng(sum(shape) if seed is None else seed)
    d = rng.standard_normal(shape).astype(dtype)
    d[rng.random(shape) < 0.1] = np.nan
    inc = rng.random(shape) < 0.7
    inc[1] = False
    return d, inc


@row("stats_planes, two segments per plane (3, 130, 130)")              # (nseg = 2 needs ny * nx > 16384) test_stats_planes
def _():
    d, inc = _noisy((3, 130, 130))
    assert d.shape[1] * d.shape[2] > 16384
    cube, spec = _dev(d), _array_spec(inc)

    def run():
        out = {}
        for what, s in (("no mask", None), ("array", spec)):
            out.update({"%s: %s" % (what, k): v for k, v in ops.stats_planes(cube, mask=s).items()})
        return out

    def check(r):
        for what, include in (("no mask", np.ones(d.shape, bool)), ("array", inc)):
            ref = E.ref_stats_axis(d, include, (1, 2))
            E.check({k: r["%s: %s" % (what, k)] for k in ref}, ref, "stats_planes, " + what)
    return run, check


def _global(dtype):                                                     # test_stats_global_and_axes' bounds (mask_edges.ref_stats_global)
    def build():
        import test_gpu_ops as TO
        shape = (64, 16, 256)
        assert shape in TO.SHAPES
        d, inc = _noisy(shape, dtype)
        cube, spec = _dev(d), _array_spec(inc)

        def run():
            out = {}
            for what, s in (("no mask", None), ("array", spec)):
                out.update({"%s: %s" % (what, k): np.float64(v) for k, v in ops.stats_global(cube, mask=s).items()})
            return out

        def check(r):
            for what, include in (("no mask", np.ones(d.shape, bool)), ("array", inc)):
                ref = E.ref_stats_global(d, include)
                E.check({k: r["%s: %s" % (what, k)] for k in ref}, ref, "stats_global %s, %s" % (np.dtype(dtype).name, what))
        return run, check
    return build


row("stats_global (64, 16, 256)")(_global(np.float32))
row("stats_global_f64 (64, 16, 256)")(_global(np.float64))


def _sigma(shape, dtype=np.float32):                                    # test_sigma_clip_fused_kernel's cube (test_gpu_round2.py)
    def build():
        rng = np.random.default_rng(shape[0] + 1)
        d = rng.standard_normal(shape).astype(dtype)
        d[rng.random(shape) < 0.03] *= 12.0
        d[rng.random(shape) < 0.02] = np.nan
        d[:, 0, 0] = np.nan
        d[:, 0, 1] = 4.25
        d[0, 1, 2] = np.inf
        inc = rng.random(shape) < 0.85
        cube, spec = _dev(d), _array_spec(inc)
        f = ops.sigma_clip_axis0 if dtype == np.float32 else ops.sigma_clip_axis0_f64

        def check(r):
            V._sigma_rule(r["out"], O.sigma_clip(d, inc & ~np.isnan(d), 2.5, out_dtype=np.dtype(dtype)), "sigma clip %s" % (shape,))
        return (lambda: {"out": f(cube, sigma=2.5, mask=spec).get()}), check
    return build


# (nz in 513 .. 1024 and at least 256 rays: the wide block shape with the probe of 64 rays, spc_sigma_clip.hip wide_ok / kProbeRays;
# see test_sigma_clip_block_shape_follows_the_mask)
row("sigma clipping, fused with the probe (515, 8, 37)")(_sigma((515, 8, 37)))
row("sigma clipping, the loop of kernels (60, 3, 70)", (("SPC_SIGMA_CLIP_FUSED", "0"),))(_sigma((60, 3, 70)))
row("sigma clipping, float64 (60, 3, 70)")(_sigma((60, 3, 70), np.float64))


@row("percentile_global, key_histogram and key_next with ties (40, 3, 70)")
def _():
    rng = np.random.default_rng(40)
    d = np.round(rng.standard_normal((40, 3, 70)) * 4).astype(np.float32) / 4          # quarter steps: many ties
    d[rng.random(d.shape) < 0.05] = np.nan
    inc = rng.random(d.shape) < 0.8
    cube, spec = _dev(d), _array_spec(inc)

    def run():
        return {"median": np.float32(ops.percentile_global(cube, 50.0, mask=spec)), "q90": np.float32(ops.percentile_global(cube, 90.0, mask=spec)),
                "hist": ops.key_histogram(cube, 0, 0, 24, mask=spec), "next": np.uint32(ops.key_next(cube, 0x80000000, mask=spec))}

    def check(r):
        x = d[inc & ~np.isnan(d)]
        k = V._keys(x)
        assert r["median"] == np.float32(np.median(x)), (r["median"], np.median(x))
        # (q90 goes through the second selection pass: held to the four patterns, its value is test_gpu_cube.py's business)
        assert np.array_equal(r["hist"], np.bincount(k >> 24, minlength=256).astype(np.uint64))
        assert r["next"] == np.uint32(k[k > 0x80000000].min())
    return run, check


@row("stack_shift and stack_sum, the smallest recorded case with rows")  # test_fixture_through_the_ops_wrappers
def _():
    import test_gpu_stack_spectra as SS
    _, cases = SS._fixture()
    with_rows = [c for c in cases if c[11] is not None]
    pkey, cube, filled, vel, idx, shifts, kw, pad, crpix1, naxis1, stacks, rows = min(with_rows, key=lambda c: (c[2].size + c[9], c[0]))

    def run():
        total, count, nnan = SS.dev_sums(cube, idx, shifts, pad)
        return {"rows": SS.dev_rows(cube, idx, shifts, pad), "sum": total, "count": count, "nan": nnan}

    def check(r):
        scale = SS.scale_of(filled)
        assert np.array_equal(r["count"] + r["nan"], np.full(naxis1, idx.size))
        SS.close(np.where(r["count"] > 0, r["sum"] / np.maximum(r["count"], 1), np.nan), stacks["nanmean"], scale, pkey + " sums")
        SS.close(r["rows"], rows, scale, pkey + " rows")
        assert np.array_equal(r["count"], np.isfinite(rows).sum(axis=0))
    return run, lambda r: _quiet(lambda: check(r))


@row("stack_cube with three slabs, the smallest recorded case")          # test_goldens_through_stack_cube
def _():
    import test_gpu_stack_cube as SC
    import test_stack_cube_host as SH
    from spectral_cube_amd import stack_cube
    G, cases = SH.fixture()
    vmin, vmax = float(G["vmin"]), float(G["vmax"])
    three = [c for c in cases if len(SH.restate(c[2], c[3], c[4], c[5], c[6], vmin, vmax)[0]) == 3]
    key, cube, d, inc, fill, freq, lines = min(three, key=lambda c: (SH.restate(c[2], c[3], c[4], c[5], c[6], vmin, vmax)[0][0].size, c[0]))
    fitting, _ = SH.restate(d, inc, fill, freq, lines, vmin, vmax)

    def run():
        return {f: SC.values(stack_cube(cube, lines, vmin, vmax, average=getattr(np, f))) for f in ("nanmean", "sum")}

    def check(r):
        for f in r:
            SC.close(r[f], SH.average(f, fitting), SC.bound(np.float32, SH.scale_of(d), f, 3), "%s %s" % (key, f))
    return run, check


@row("mosaic of two fields, the recorded split cube")                    # test_split_cube_round_trip_is_exact_with_nearest
def _():
    import test_gpu_mosaic as MO
    from spectral_cube_amd import mosaic_cubes
    sources, _, key = MO.recorded_sources("split")
    assert len(sources) == 2
    whole = MO.G[key + "whole"]

    def run():
        near = mosaic_cubes([MO.make_cube(*s) for s in sources], order="nearest-neighbor", roundtrip_coords=False, spectral_block_size=None)
        lin = mosaic_cubes([MO.make_cube(*s) for s in sources], order="bilinear", roundtrip_coords=False)
        return {"nearest": MO.host(near), "bilinear": MO.host(lin)}

    def check(r):
        assert r["nearest"].shape == whole.shape and np.array_equal(r["nearest"], whole)
        exp = MO.G[key + "result|bilinear"] if key + "result|bilinear" in MO.G.files else None
        if exp is not None:                                             # (test_recorded_mosaics' bound)
            ok = np.isfinite(exp)
            assert np.array_equal(np.isnan(r["bilinear"]), np.isnan(exp)) and np.abs(r["bilinear"][ok] - exp[ok]).max() <= 1e-5 * np.abs(exp[ok]).max()
    return run, check


@pytest.mark.parametrize("name", list(ROWS), ids=[re.sub(r"[^A-Za-z0-9_.=+-]+", "_", n).strip("_") for n in ROWS])
def test_route_with_several_chunks_tiles_or_partial_records(gpu, name):
    r = ROWS[name]
    with V._env(r.env):
        run, check = r.build()
        DM.same_under_every_pattern(run, check)


# ---- D: chains through SpectralCube: one operator's scratch is the next one's ----------------------------------------------------
HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5, "CUNIT3": "km/s",
       "CRPIX1": 1, "CRPIX2": 1, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -16.0, "BUNIT": "K"}


def test_chain_spatial_smooth_then_moment0_fused(gpu, monkeypatch):
    """test_cube_level_masked_spatial_smooth_moment0_runs_fused (test_gpu_mfma.py): its cube, its kernel, its reference"""
    import test_gpu_mfma as MF
    shape = (20, 64, 160)
    d, m = MF._case(shape, 17, valid=0.6)
    m[:, 10:13, 20:24] = False
    k = Gaussian2DKernel(8 / 2.3548200450309493)
    calls = []
    real = ops.spatial_conv_mfma
    monkeypatch.setattr(ops, "spatial_conv_mfma", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])

    def run():
        return {"m0": np.asarray(SpectralCube.read(d, dict(HDR)).with_mask(m).spatial_smooth(k).moment0())}

    def check(r):
        assert len(calls) == len(DM.PATTERNS), "the fused kernel was not used"
        filled = np.where(m, O.spatial_smooth(d, m, k.array), np.nan)
        exp = 0.5 * np.nansum(filled, axis=0)
        exp[np.all(np.isnan(filled), axis=0)] = np.nan
        assert np.isnan(exp).sum() == 12
        assert_close(r["m0"], exp, atol=1e-5 * np.nanmax(np.abs(exp)), what="cube-level fused smooth -> moment0")
    DM.same_under_every_pattern(run, check)


def test_chain_spectral_smooth_then_moment1(gpu):
    """spectral_smooth(Gaussian1DKernel(4)).moment1() on the cube of the smoke run with a NaN run longer than the kernel: the
    33-tap ring fused with the moments.  Reference and bound as test_c3_spectral_smooth_moment1_2048cubed (test_gpu_fullsize.py):
    NaN pattern exact, 1e-5 * dv * nz on the spaxels whose smoothed S0 is well conditioned"""
    from spectral_cube_amd import synth
    shape = (64, 32, 48)
    d = synth.gaussian_line_cube(shape, 11)
    d[20:60, 3, 5] = np.nan
    inc = synth.boolean_mask(d, 11).astype(bool)
    k = Gaussian1DKernel(4)
    assert k.array.size == 33

    def run():
        return {"m1": np.asarray(SpectralCube.read(d, dict(HDR)).with_mask(inc).spectral_smooth(k).moment1())}

    def check(r):
        cube = SpectralCube.read(d, dict(HDR))
        v = np.asarray(cube.spectral_axis)
        cen = v - v[0]
        valid = inc & np.isfinite(d)
        sm = O.spectral_smooth(d, valid, k.array)
        exp = O.moment(sm, valid, 1, cen, 0.5, world0=v[0])
        assert np.array_equal(np.isnan(r["m1"]), np.isnan(exp))
        s0 = O.moment(sm, valid, 0, cen, 1.0)
        wc = np.isfinite(exp) & (np.abs(s0) > 1e-2 * np.nanmax(np.abs(s0)))
        assert wc.mean() > 0.5
        assert np.abs(r["m1"][wc] - exp[wc]).max() <= 1e-5 * 0.5 * shape[0]
    DM.same_under_every_pattern(run, lambda r: _quiet(lambda: check(r)))


def test_chain_interpolate_then_reproject_in_one_pass(gpu, monkeypatch):
    """the small case of test_cube_level_interpolate_then_reproject_is_one_pass (test_gpu_round5.py)"""
    import test_gpu_round5 as R5
    rng = np.random.default_rng(77)
    nz, ny, nx = 21, 70, 90
    d = rng.standard_normal((nz, ny, nx)).astype(np.float32)
    d[5, 20:24, 30:33] = np.nan
    hdr = R5._cube_hdr(nz, ny, nx)
    a = np.deg2rad(30.0)
    tgt = {k: hdr[k] for k in ("CTYPE1", "CTYPE2", "CDELT1", "CDELT2", "CRVAL1", "CRVAL2")}
    tgt.update(NAXIS=2, NAXIS1=80, NAXIS2=76, CRPIX1=40.5, CRPIX2=38.5, PC1_1=np.cos(a), PC1_2=-np.sin(a), PC2_1=np.sin(a), PC2_2=np.cos(a))
    calls = []
    real = ops.resample_bilinear_lerp
    monkeypatch.setattr(ops, "resample_bilinear_lerp", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    seen = {}

    def run():
        cube = SpectralCube.read(d, hdr)
        cube = cube.with_mask(cube > -1.2)
        v = cube.spectral_axis
        grid = np.linspace(v[0], v[-1], 50)
        res = cube.spectral_interpolate(grid, suppress_smooth_warning=True).reproject(tgt)
        seen.update(cube=cube, res=res, v=np.asarray(v), grid=grid)
        return {"out": res._device_data().get(), "foot": np.asarray(res._footprint)}

    def check(r):
        assert calls == [1] * len(DM.PATTERNS), "the interpolation was not folded into the resampling kernel"
        ei, _ = O.spectral_interpolate(d, d > -1.2, seen["v"], seen["grid"])
        xs, ys = ops.wcs_pixel_map(seen["cube"].wcs, seen["res"].wcs, (76, 80))
        exp, _ = O.resample_bilinear(ei, xs.get(), ys.get())
        assert_close(r["out"], exp.astype(np.float32), atol=1e-5 * np.nanmax(np.abs(exp)), what="cube-level folded chain vs oracle")
    DM.same_under_every_pattern(run, lambda r: _quiet(lambda: check(r)))


def test_chain_median_mad_std_statistics_on_one_cube(gpu):
    """median(axis=0), mad_std(axis=0), statistics() one after the other: the selection's scratch, then the reduction's.  The
    cube and bounds of test_median_percentile_mad_std (test_gpu_cube.py: the median bit for bit, mad_std 2e-6 max) and of
    test_stats_global_and_axes (npts, min, max exact; sum, sumsq 1e-12)"""
    g = golden("order_stats.npz")
    d, inc = g["data"], g["include"]
    hdr = str(golden("c1_moments.npz")["header"])

    def run():
        cube = SpectralCube.read(d, hdr).with_mask(inc)
        out = {"median": np.asarray(cube.median(axis=0)), "mad_std": np.asarray(cube.mad_std(axis=0))}
        out.update({"stat " + k: np.float64(v) for k, v in cube.statistics().items()})
        return out

    def check(r):
        exp = g["median"]
        assert np.array_equal(np.isnan(r["median"]), np.isnan(exp))
        assert np.array_equal(r["median"][~np.isnan(exp)], exp[~np.isnan(exp)].astype(np.float32))
        assert_close(r["mad_std"], g["mad_std"], atol=2e-6 * np.nanmax(np.abs(g["mad_std"])), what="mad_std")
        es = O.statistics(d, inc.astype(bool))
        for k in ("npts", "min", "max"):
            assert r["stat " + k] == es[k], k
        for k in ("sum", "sumsq"):
            assert r["stat " + k] == pytest.approx(es[k], rel=1e-12), k
    DM.same_under_every_pattern(run, lambda r: _quiet(lambda: check(r)))


def test_chain_out_of_core_moment0_and_spatial_smooth_with_halo_rows(gpu, monkeypatch):
    """the cube, mask and kernel of test_out_of_core_spatial_smooth_with_halo_rows (test_gpu_round3.py) streamed through a
    budget of a quarter of the cube: moment0, the smoothed cube and its moment 0 equal the resident results bit for bit,
    whatever the strips' buffers, the per-strip scratch and the maps held before"""
    import test_gpu_round3 as R3
    from spectral_cube_amd import synth
    monkeypatch.setenv("SPC_MOMENTS_NSPLIT", "1")
    nz, ny, nx = 24, 90, 70
    d = synth.gaussian_line_cube((nz, ny, nx), 34)
    d[:, 40:43, 10:13] = np.nan
    inc = synth.boolean_mask(d, 34).astype(bool)
    hdr = R3._c1_header()
    k2 = Gaussian2DKernel(1.5)
    assert k2.array.shape == (13, 13)
    monkeypatch.setenv("SPC_HBM_BUDGET", str(1 << 40))
    res = SpectralCube.read(d, hdr).with_mask(inc)
    sm = res.spatial_smooth(k2)
    resident = {"m0": np.asarray(res.moment0()), "smooth": np.asarray(sm.filled_data), "smooth m0": np.asarray(sm.moment0())}
    monkeypatch.setenv("SPC_HBM_BUDGET", str(d.nbytes // 4))

    def run():
        big = SpectralCube.read(d.copy(), hdr).with_mask(inc)
        assert big._stream_source() is not None
        out = {"m0": np.asarray(big.moment0()),
               "smooth": big.spatial_smooth(k2).stream_into(np.empty((nz, ny, nx), np.float32)),
               "smooth m0": np.asarray(big.spatial_smooth(k2).moment0())}
        assert big._dev is None, "the cube was made resident"
        return out

    def check(r):
        for k, e in resident.items():
            V._bits(np.asarray(r[k], dtype=e.dtype), e, "out of core %s against the resident result" % k)
    DM.same_under_every_pattern(run, check)
