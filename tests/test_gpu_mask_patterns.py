"""Every masked operator on the mask patterns, byte values and poison of tests/mask_patterns.py.

The rows are those of test_gpu_views.py (``OPS``: run, ref, env, base, dtypes - every row with ``masked=True``) and their
references and tolerances are the ones cited there; nothing here has a tolerance of its own.  One test id per (row, sample
type, pattern), on the row's own base shape, checks three things:

a. canonical bytes (1) against the row's reference fed with the pattern as include set (mask_edges.check: NaN and inf patterns
   exactly, the rest at the cited tolerance; the sigma-clip and one-ulp rules of the views matrix as they are there);
b. every other byte value - 2, 0x80, 0xFF, the seeded mix - bit for bit against the canonical run (a NaN equals a NaN): the
   include set is the same, so there is nothing to tolerate;
c. the poisoned cube bit for bit against the cube with 0 in the same voxels, with canonical and with mixed bytes (not for
   ``all one``, which excludes nothing).

All of it runs on a contiguous cube with a contiguous mask; ``segments`` and ``lanes`` run again, mixed bytes and poison, on
xwin_off1 with mask_phase, where every entry takes its byte-at-a-time form (against the same reference: the include set and
the included samples are the same).

Masks an entry WRITES hold only 0 and 1, whatever bytes came in: spc_mask_eval_*, spc_mask_include_u8, the downsample mask,
the bilinear footprint, the morphology outputs, label_select - and subcube's ``out_mask`` too (spc_subcube.hip:83 packs
``inc ? 1 : 0``), so no entry passes input bytes on.  Every uint8 output of every run is held to that.

EXEMPT lists the rows that by design show raw excluded samples; they are held to (a) on the poisoned cube instead of (c).
spc_mask_morph_u8 and spc_label_u8 take masks and no cube: patterns and byte values against scipy on ``mask != 0``."""
import collections
import functools
import types

import numpy as np
import pytest

import labelling as RL
import mask_edges as E
import mask_patterns as P
import morphology as RM
import oracle_np as O
import test_gpu_views as TV
import views as V
from spectral_cube_amd import _lib, labelling, masks, ops
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

F32, F64 = TV.F32, TV.F64

# operator -> (outputs that may differ under excluded voxels, the source line that makes it so).  (c) then compares those
# outputs where the output mask includes, everything else bit for bit, and holds the poisoned run to the reference
EXEMPT = {
    "subcube": (("out",), "spc_subcube.hip:84, :108: ``if (A.filled) v = inc ? v : A.fill`` - without *filled* the sample is copied as it is"),
}

# rows of the views matrix that take no include array although ``masked`` is their default: the row here that does
REPLACED = {"mask_eval": "mask_eval[array term]"}

OPS = collections.OrderedDict((n, o) for n, o in TV.OPS.items() if o.masked and n not in REPLACED)


def _extra(name, dtypes, pair):
    run, ref = pair()
    OPS[name] = TV.Op(name, dtypes, run, ref, (), False, True, False, TV.ALIGNED, (), V.BASE, 0.0, None)


def _percentile_groups():
    """spc_percentile_groups_f32 (ops.percentile_global with keep=0 | 1), the row the views matrix does not have: numpy's
    nanmedian / nanpercentile over the two other axes, at the bounds plane_order_stats.check cites (median exact, a
    percentile rtol 2e-6 and 2e-6 of the largest expected value: test_gpu_long_axes.py:28-32)"""
    def run(c):
        out = {}
        for keep in (0, 1):
            out["median, keep=%d" % keep] = ops.percentile_global(c.cube, 50.0, mask=c.spec, keep=keep).get()
            out["p37.5, keep=%d" % keep] = ops.percentile_global(c.cube, 37.5, mask=c.spec, keep=keep).get()
        return out

    def ref(c):
        out = {}
        for keep, pair in ((0, (1, 2)), (1, (0, 2))):
            out["median, keep=%d" % keep] = E.exact(O.median(c.d, c.inc, axis=pair))
            p = np.asarray(O.percentile(c.d, c.inc, [37.5], axis=pair)[0])
            fin = np.isfinite(p)
            out["p37.5, keep=%d" % keep] = E.within(p, 2e-6 * (float(np.abs(p[fin]).max()) if fin.any() else 0.0), 2e-6)
        return out
    return run, ref


def _mask_eval():
    """spc_mask_eval_f32 / _f64 with the include bytes as a uint8 operand (SPC_MOP_LOAD pushes ``operand != 0``):
    ((cube > 0.25) AND array) OR (array XOR (second <= 0.5))"""
    def second(c):
        return V.data(c.dtype.type, V.BASE, seed=9)[0][..., :c.d.shape[2]]

    def run(c):
        lay = V.layout(TV._other(c, "xwin_oddstride", "rows"))
        b, _parent = V.upload(lay, second(c), V.CUBE_POISON[c.dtype])
        rs, ps = c.mlay.row_stride, c.mlay.plane_stride              # (an operand's strides are explicit: 0 broadcasts)
        prog = types.SimpleNamespace(slots=[c.cube, b], operands=[(c.marr, (ps, rs, 1))],
                                     instr=[(_lib.MOP_CMP, 0, _lib.CMP_GT, -1, 0.25), (_lib.MOP_LOAD, 0, 0, 0, 0.0), (_lib.MOP_AND, 0, 0, -1, 0.0),
                                            (_lib.MOP_LOAD, 0, 0, 0, 0.0), (_lib.MOP_CMP, 1, _lib.CMP_LE, -1, 0.5), (_lib.MOP_XOR, 0, 0, -1, 0.0),
                                            (_lib.MOP_OR, 0, 0, -1, 0.0)])
        return {"out": c.read(ops.mask_eval(prog, c.d.shape, 0, c.dtype, out=c.out(c.d.shape, np.uint8)))}

    def ref(c):
        with np.errstate(invalid="ignore"):
            return {"out": E.exact((((c.d > 0.25) & c.inc) | (c.inc ^ (second(c) <= 0.5))).astype(np.uint8))}
    return run, ref


_extra("percentile_groups", (F32,), _percentile_groups)
_extra("mask_eval[array term]", (F32, F64), _mask_eval)

CASES = [(name, dt, pattern) for name, o in OPS.items() for dt in o.dtypes for pattern in P.PATTERNS]


@functools.lru_cache(maxsize=None)
def _cubes(dtype, base, pedestal, pattern):
    """(poisoned, zeroed) of the row's samples under the pattern's excluded voxels"""
    return P.poison(V.data(dtype.type, base, pedestal=pedestal)[0], P.include(pattern, base))


def _only_0_and_1(got, what):
    for k, v in got.items():
        v = np.asarray(v)
        if v.dtype == np.uint8:
            assert v.size == 0 or v.max() <= 1, "%s: %s, a mask the entry writes, holds byte %d" % (what, k, v.max())


def _same_bits(got, exp, what):
    assert set(got) == set(exp), what
    for k in exp:
        TV._bits(got[k], exp[k], "%s: %s" % (what, k))


def _same_where_included(got, exp, loose, what):
    """(c) of an exempt row: the outputs *loose* where the output mask includes, every other output bit for bit"""
    for k in exp:
        g, e = np.asarray(got[k]), np.asarray(exp[k])
        if k in loose:
            inc = np.asarray(exp["mask"]) != 0
            g, e = np.where(inc, g, 0), np.where(inc, e, 0)
        TV._bits(g, e, "%s: %s" % (what, k))


def _ids(cases):
    return ["%s-%s-%s" % (n.replace(" ", "_"), d.name, p.replace(" ", "_")) for n, d, p in cases]


@pytest.mark.parametrize("name,dtype,pattern", CASES, ids=_ids(CASES))
def test_operator_on_every_mask_pattern(gpu, name, dtype, pattern):
    o = OPS[name]
    inc = P.include(pattern, o.base)
    exempt = EXEMPT.get(name.split("[")[0])
    failed = []

    def ctx(cname, mname, kind, data=None):
        given = None if data is None else ("%s: %s" % (data, pattern), _cubes(dtype, o.base, o.pedestal, pattern)[data == "zeroed"])
        return TV.Ctx(dtype, cname, mname, "contig", base=o.base, masked=True, finite=o.finite, pedestal=o.pedestal, data=given,
                      mask=(pattern, P.to_bytes(inc, kind)))

    def run(c, what):
        got = o.run(c)
        for lay, parent in c._outs:
            assert V.read_output(lay, parent)[1], what + ": wrote outside the output view"
        _only_0_and_1(got, what)
        return got

    def attempt(what, check):
        try:
            check()
        except AssertionError as err:                           # every cell is tried: the report names all that miss
            failed.append("%s: %s" % (what, str(err).splitlines()[0][:300]))

    def refused(c, what):
        """True when the entry declines this layout by design (asserted, as in the views matrix)"""
        why = o.declines(c) if o.declines else None
        if why is None:
            return False
        with pytest.raises(_lib.HipUnsupported, match=why):
            o.run(c)
        return True

    def poison_check(cname, mname, kind, what):
        cz, cp = ctx(cname, mname, kind, "zeroed"), ctx(cname, mname, kind, "poison")
        gz, gp = run(cz, what), run(cp, what)
        if exempt is None:
            attempt(what, lambda: _same_bits(gp, gz, what))
        else:
            attempt(what, lambda: _same_where_included(gp, gz, exempt[0], what))
            attempt(what, lambda: TV._check(gp, TV._ref(name, cp, lambda: o.ref(cp)), what + " against the reference"))

    with TV._env(o.env):
        for cname, mname, kinds in (("contig", "mask_contig", P.BYTES), ("xwin_off1", "mask_phase", ("mixed",))):
            if cname != "contig" and pattern not in ("segments", "lanes"):
                continue
            where = "%s %s, %s: cube %s, mask %s" % (name, dtype.name, pattern, cname, mname)
            c0 = ctx(cname, mname, kinds[0])
            if refused(c0, where):
                continue
            ref = TV._ref(name, c0, lambda: o.ref(c0))
            got0 = run(c0, where)
            attempt(where + ", %s bytes (a)" % kinds[0], lambda: TV._check(got0, ref, where))
            for kind in kinds[1:]:
                what = "%s, %s bytes against canonical (b)" % (where, kind)
                got = run(ctx(cname, mname, kind), what)
                attempt(what, lambda: _same_bits(got, got0, what))
            if pattern != "all one":
                for kind in sorted({kinds[0], "mixed"}):
                    poison_check(cname, mname, kind, "%s, %s bytes, poisoned against zeroed (c)" % (where, kind))
    assert not failed, "%d checks:\n%s" % (len(failed), "\n".join(failed[:12]))


def test_the_matrix_covers_every_masked_row_of_the_views_matrix():
    """a new masked row of test_gpu_views.OPS cannot stay out: every one is here under its own name, or replaced by name"""
    masked = {n for n, o in TV.OPS.items() if o.masked}
    assert set(REPLACED) <= masked and set(REPLACED.values()) <= set(OPS)
    assert masked - set(REPLACED) <= set(OPS)
    assert {(n, d) for n, d, _ in CASES} == {(n, d) for n, o in OPS.items() for d in o.dtypes}
    assert {p for _, _, p in CASES} == set(P.PATTERNS) and len(CASES) == len(P.PATTERNS) * sum(len(o.dtypes) for o in OPS.values())
    assert {o.base for o in OPS.values()} == set(P.SHAPES) == {V.BASE, TV.BASE_WIDE}
    rows = {TV._row_of(n) for n in OPS if n not in ("percentile_groups",)}
    assert rows == {TV._row_of(n) for n in masked}, "a masked row of test_gpu_views.TABLE has no case here"
    assert set(EXEMPT) <= {n.split("[")[0] for n in OPS} and all(":" in why for _, why in EXEMPT.values())
    # every ops function that takes mask= is run by a row (through the table of the views matrix) or named here
    import inspect
    for n, f in vars(ops).items():
        if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_") and "mask" in inspect.signature(f).parameters:
            # (mask_morph: test_morphology_on_every_mask_pattern_and_byte_value below)
            assert n == "mask_morph" or TV.ROW_OF_OPS_FUNCTION.get(f.__name__) in rows, "ops.%s takes a mask and has no row" % n


# ---- entries that take masks and no cube -----------------------------------------------------------------------------------------
MORPH_SHAPE = (5, 6)
MORPH_STRIDE = 80                    # rows 16-byte aligned at x offset 0, 4-byte aligned at 4, unaligned at 1


def _mask_view(a, x0):
    """*a* (uint8) as an x-window at offset *x0* of a parent whose rows are MORPH_STRIDE bytes apart and hold 1 around it"""
    lay = V._window("xwin", a.shape, x0, MORPH_STRIDE - a.shape[2] - x0)
    assert lay.row_stride == MORPH_STRIDE and lay.plane_stride % 16 == 0
    return V.upload(lay, a, 1)


@functools.lru_cache(maxsize=None)
def _morph_expected(shape, pattern, variant):
    x, m = P.include(pattern, shape), RM.field(shape, 4, 0.7)
    s = RM.generate_binary_structure(3, 1)
    if variant == "dilate":
        return RM.scipy_morph(x, s, RM.DILATE)
    if variant == "erode":
        return RM.scipy_morph(x, s, RM.ERODE, 1, m, 1)
    return RM.scipy_morph(x, s, RM.DILATE, -1, m, 0)


@pytest.mark.parametrize("x0", (0, 4, 1))
@pytest.mark.parametrize("nx", (64, 68, 67), ids=("32n", "32n+4", "odd"))
def test_morphology_on_every_mask_pattern_and_byte_value(gpu, nx, x0):
    """mm_pack_kernel (spc_mask_morph.hip:115-135) reads a row's words as 16 bytes (x offset 0), as dwords (4) or byte by
    byte (1, and every last word of a row of 32 n + 4 or of odd length): input and mask in every byte value, the result scipy's
    on ``!= 0`` and 0 / 1 bytes"""
    shape = MORPH_SHAPE + (nx,)
    offs = RM.offsets(RM.generate_binary_structure(3, 1))
    field = RM.field(shape, 4, 0.7)
    failed = []
    for pattern in P.PATTERNS:
        for kind in P.BYTES:
            xv, _xp = _mask_view(P.to_bytes(P.include(pattern, shape), kind), x0)
            mv, _mp = _mask_view(P.to_bytes(field, kind), x0)
            for variant, kw in (("dilate", {}), ("erode", dict(mask=mv, border_value=1)), ("propagate", dict(mask=mv, iterations=-1))):
                op = _lib.MORPH_ERODE if variant == "erode" else _lib.MORPH_DILATE
                got = ops.mask_morph(xv, offs, op, **kw).get()
                if got.max(initial=0) > 1 or not np.array_equal(got != 0, _morph_expected(shape, pattern, variant)):
                    failed.append((pattern, kind, variant, int(got.max(initial=0))))
    assert not failed, "%d of %d differ from scipy on mask != 0: %s" % (len(failed), 3 * len(P.PATTERNS) * len(P.BYTES), failed[:8])


@pytest.mark.parametrize("x0", (0, 1))
def test_labelling_on_every_mask_pattern_and_byte_value(gpu, x0):
    """spc_label_u8 on every pattern and byte value against scipy.ndimage.label(mask != 0); the mask label_select writes from
    a keep table of mixed bytes holds 0 and 1, and so does remove_small_objects of a device mask of the same bytes"""
    shape = MORPH_SHAPE + (68,)
    conn = RL.ndi.generate_binary_structure(3, 2)
    failed = []
    for pattern in P.PATTERNS:
        inc = P.include(pattern, shape)
        exp, n = RL.scipy_label(inc, conn)
        sizes, _ = RL.scipy_objects(exp, n)
        keep = sizes >= 2
        keep[0] = False
        table = np.where(keep, np.resize(np.array(P.MIXED_VALUES, np.uint8), n + 1), 0).astype(np.uint8)
        for kind in P.BYTES:
            xv, _xp = _mask_view(P.to_bytes(inc, kind), x0)
            lab, m = ops.label(xv, conn)
            if m != n or not np.array_equal(lab.get(), exp):
                failed.append((pattern, kind, "label", m, n))
                continue
            sel = ops.label_select(lab, m, table).get()
            if sel.dtype != np.uint8 or not np.array_equal(sel, keep[exp].astype(np.uint8)):
                failed.append((pattern, kind, "select", int(sel.max(initial=0))))
            if x0 == 0:                          # remove_small_objects itself, on a device mask of these bytes
                dev = masks.DeviceBooleanMask(DeviceArray.from_numpy(np.ascontiguousarray(P.to_bytes(inc, kind))))
                small = labelling.remove_small_objects(dev, min_size=2, structure=conn).device_array().get()
                if small.dtype != np.uint8 or not np.array_equal(small, RL.scipy_remove_small(inc, 2, conn)[0].astype(np.uint8)):
                    failed.append((pattern, kind, "remove_small_objects", int(small.max(initial=0))))
    assert not failed, failed[:8]
