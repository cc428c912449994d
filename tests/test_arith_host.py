"""CPU: the host side of cube arithmetic (+ - * / **, spectral_cube.py:912-1003 and 2237-2361) against
tests/golden/arith.npz, the reference's results through both of its classes (tools/gen_golden_arith.py).

``restate`` is the step program of include/spcube_hip.h in numpy, never the library: the include bit is taken once on the
source sample; a step with ``refill`` first sets the excluded voxels to the fill value, then applies one numpy operation in
the cube's dtype.  It must reproduce every recorded array bit for bit (the general powers excepted: two libm's), and the
programs SpectralCube plans - pending, so no device is needed - must be the ones restated here.  The GPU tests
(tests/test_gpu_arith.py) run the same table through the kernels."""
import os
import re
import warnings

import numpy as np
import pytest

from conftest import REPO, golden
from spectral_cube_amd import PrecisionWarning, Projection, SpectralCube, UnitsError, _lib, ops
from spectral_cube_amd.wcs import parse_header


class Q:
    """a quantity as far as the operators look: a value and a unit"""

    def __init__(self, value, unit):
        self.value, self.unit = value, unit


def K(v):
    return Q(v, "K")


# case -> (the expression on the product, its step program (op, operand, refill); a string names a recorded array)
TABLE = {
    "add_q": (lambda c, o: c + K(1.5), [("add", 1.5, 1)]),
    "sub_q": (lambda c, o: c - K(0.25), [("sub", 0.25, 1)]),
    "mul_s": (lambda c, o: c * 2.5, [("mul", 2.5, 1)]),
    "mul_i": (lambda c, o: c * 2, [("mul", 2.0, 1)]),
    "div_s": (lambda c, o: c / 3.0, [("div", 3.0, 1)]),
    "pow_2": (lambda c, o: c ** 2, [("square", None, 1)]),
    "pow_half": (lambda c, o: c ** 0.5, [("sqrt", None, 1)]),
    "pow_m1": (lambda c, o: c ** -1, [("recip", None, 1)]),
    "pow_1": (lambda c, o: c ** 1, [("mul", 1.0, 1)]),
    "pow_0": (lambda c, o: c ** 0, [("one", None, 1)]),
    "sub_map": (lambda c, o: c - Projection(o["map"], unit="K"), [("sub", "map", 1)]),
    "div_map2": (lambda c, o: c / o["map2"], [("div", "map2", 1)]),
    "mul_spec3": (lambda c, o: c * o["spec"][:, None, None], [("mul", "spec3", 1)]),
    "sub_row": (lambda c, o: c - K(o["row"]), [("sub", "row", 1)]),
    "add_col": (lambda c, o: c + K(o["col"]), [("add", "col", 1)]),
    "mul_zy": (lambda c, o: c * o["zy"], [("mul", "zy", 1)]),
    "mul_jy": (lambda c, o: c * Q(2, "Jy"), [("mul", 2.0, 1)]),
    "sub_cube": (lambda c, o: c - o["cube2"], [("sub", "data2", 0)]),
    "add_cube": (lambda c, o: c + o["cube2"], [("add", "data2", 0)]),
    "mul_cube": (lambda c, o: c * o["cube2"], [("mul", "data2", 0)]),
    "div_cube": (lambda c, o: c / o["cube2"], [("div", "data2", 0)]),
    "chain3": (lambda c, o: (c - K(o["map"])) / o["map2"] * 1e3, [("sub", "map", 1), ("div", "map2", 1), ("mul", 1e3, 1)]),
    "chain_mul_add": (lambda c, o: c * o["map2"] + K(o["map"]), [("mul", "map2", 1), ("add", "map", 1)]),
    "bare_add_1": (lambda c, o: c + 1, [("add", 1.0, 1)]),
    "bare_sub_1": (lambda c, o: c - 1, [("sub", 1.0, 1)]),
    "pow_1p7": (lambda c, o: c ** 1.7, [("pow", 1.7, 1)]),
    "pow_m2p5": (lambda c, o: c ** -2.5, [("pow", -2.5, 1)]),
}
# the unit of every case by the product's rules (strings; the reference's astropy spelling where it differs is in the file)
UNITS = {"pow_2": "K2", "pow_half": "K(1/2)", "pow_m1": "K-1", "pow_0": "", "mul_jy": "K Jy", "mul_cube": "K2", "div_cube": "",
         "bare_add_1": "", "bare_sub_1": "", "pow_1p7": "", "pow_m2p5": ""}
GENERAL_POW = ("pow_1p7", "pow_m2p5")
BARE, POWBASE = ("bare_add_1", "bare_sub_1"), GENERAL_POW      # on the unitless cube / on the unitless abs(cube) + 0.1
RAISING = {
    "add_plain": lambda c, o: c + 1,
    "sub_plain": lambda c, o: c - 1,
    "sub_spec1": lambda c, o: c - K(o["spec"]),
    "floordiv": lambda c, o: c // 2,
    "pow_cube": lambda c, o: c ** o["cube2"],
    "rmul": lambda c, o: 2 * c,
    "neg": lambda c, o: -c,
    "sub_shape": lambda c, o: c - o["cube2"][:, :, :5],
}
NUMPY_OP = {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide, "pow": np.power,
            "square": lambda v, b: v * v, "sqrt": lambda v, b: np.sqrt(v), "recip": lambda v, b: v.dtype.type(1) / v,
            "one": lambda v, b: np.ones_like(v)}


def restate(d, inc, fill, steps, arrays):
    """the step program per voxel, in numpy and in d's dtype"""
    t = d.dtype.type
    v = d.copy()
    with np.errstate(all="ignore"):
        for op, b, refill in steps:
            if refill:
                v = np.where(inc, v, t(fill))
            b = arrays[b].astype(d.dtype) if isinstance(b, str) else (None if b is None else t(b))
            v = NUMPY_OP[op](v, b)
            assert v.dtype == d.dtype
    return v


def arrays_of(G, dtype=np.float32):
    a = {k: G[k].astype(dtype) for k in ("map", "map2", "spec", "row", "col", "zy", "data2")}
    a["spec3"] = a["spec"][:, None, None]
    return a


def header_of(G, unit="K"):
    h = parse_header(str(G["header"]))
    h["BUNIT"] = unit
    return h


def cubes_of(G, fill, dtype=np.float32):
    """(the cube in K, the unitless one, the unitless abs(cube) + 0.1, the operands) as the generator made them: the boolean
    mask alone (no isfinite term: the NaN sample is included)"""
    keep = G["keep"]

    def make(d, unit):
        return SpectralCube(d.astype(dtype), header=header_of(G, unit), mask=_mask(keep), fill_value=fill)
    o = {k: G[k].astype(dtype) for k in ("map", "map2", "spec", "row", "col", "zy")}
    o["cube2"] = SpectralCube(G["data2"].astype(dtype), header=header_of(G), mask=_mask(G["keep2"]))
    return make(G["data"], "K"), make(G["data"], ""), make(G["powbase"], ""), o


def _mask(keep):
    from spectral_cube_amd import BooleanArrayMask
    return BooleanArrayMask(keep, None, shape=keep.shape)


def recorded(G, cls, fname):
    """{case: (raw, filled, include, unit)} of one class and fill value.  The generator checked for every case that the
    include map is ``keep`` and the filled data ``where(keep, raw, fill)``; the file holds raw data and units"""
    g = "%s|%s|" % (cls, fname)
    keep, fill = G["keep"], np.float32(fname)
    return {str(n): (G[g + "raw"][i], np.where(keep, G[g + "raw"][i], fill), keep, str(G[g + "units"][i]))
            for i, n in enumerate(G[g + "names"])}


def groups(G):
    for cls in (str(c) for c in G["classes"]):
        for fname in (str(f) for f in G["fills"]):
            yield cls, fname, float(fname)


def source_of(G, case):
    return G["powbase"] if case in POWBASE else G["data"]


def pick(case, cube, bare, powbase):
    return powbase if case in POWBASE else bare if case in BARE else cube


def ulp_distance(a, b):
    """largest distance in units of the last place between two float arrays of one dtype with equal NaN patterns"""
    a, b = np.asarray(a), np.asarray(b)
    it = np.int32 if a.dtype == np.float32 else np.int64
    ok = ~np.isnan(a)
    ia, ib = a[ok].view(it).astype(np.int64), b[ok].view(it).astype(np.int64)
    top = np.int64(np.iinfo(it).min)
    ia, ib = np.where(ia < 0, top - ia, ia), np.where(ib < 0, top - ib, ib)
    return int(np.abs(ia - ib).max()) if ia.size else 0


# ---- the restatement against the reference -------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_bit_for_bit():
    G = golden("arith.npz")
    arrays, keep = arrays_of(G), G["keep"]
    assert G["data"].shape == (7, 5, 6) and G["data"].dtype == np.float32 and np.isnan(G["data"]).sum() == 1
    assert keep[np.isnan(G["data"])].all(), "the NaN sample is included"
    seen = 0
    for cls, fname, fill in groups(G):
        rec = recorded(G, cls, fname)
        assert set(rec) == set(TABLE) - ({"mul_jy"} if cls == "dask" else set()), (cls, fname)
        for case, (raw, filled, include, unit) in rec.items():
            mine = restate(source_of(G, case), keep, fill, TABLE[case][1], arrays)
            what = (cls, fname, case)
            assert raw.dtype == np.float32 and np.array_equal(include, keep), what
            assert np.array_equal(filled, np.where(keep, raw, np.float32(fill)), equal_nan=True), what
            if case in GENERAL_POW:                            # numpy's powf here and the one that wrote the file
                assert np.array_equal(np.isnan(mine), np.isnan(raw)), what
                np.testing.assert_allclose(mine, raw, rtol=2.0 ** -20, atol=0.0)
            else:
                assert np.array_equal(mine, raw, equal_nan=True), what
            seen += 1
    assert seen == 4 * len(TABLE) - 2
    # what an excluded voxel holds after a chain with fill 0: op_last(0, b), not the chain applied to 0
    raw = recorded(G, "np", "0")["chain3"][0]
    assert np.array_equal(raw[~keep], np.zeros(keep.shape, np.float32)[~keep]), "0 * 1e3"
    raw = recorded(G, "np", "0")["chain_mul_add"][0]
    assert np.array_equal(raw[~keep], np.broadcast_to(G["map"], keep.shape)[~keep]), "0 + map, not 0 * map2 + map"
    raw = recorded(G, "np", "0")["sub_cube"][0]                # cube on cube: raw samples, nothing refilled
    assert np.array_equal(raw, G["data"] - G["data2"], equal_nan=True)


# ---- the programs the product plans ----------------------------------------------------------------------------------
def test_planned_programs_units_and_metadata():
    G = golden("arith.npz")
    arrays = arrays_of(G)
    for fill in (np.nan, 0.0):
        cube, bare, powbase, o = cubes_of(G, fill)
        for case, (expr, steps) in TABLE.items():
            left = pick(case, cube, bare, powbase)
            r = expr(left, o)
            assert type(r) is SpectralCube and r.shape == left.shape, case
            assert r._pending_arith_steps() == len(steps) and r._dev is None and r._data is None, case
            P = r._arith
            assert P.source is left and P.mask is left.mask and not P.wide, case
            for (op, b, refill), (gop, gb, grefill) in zip(steps, P.steps):
                assert (op, bool(refill)) == (gop, bool(grefill)), case
                if b == "data2":
                    assert gb is o["cube2"], case
                elif isinstance(b, str):
                    assert gb.dtype == np.float32 and np.array_equal(np.broadcast_to(gb, left.shape), np.broadcast_to(arrays[b], left.shape)), case
                else:
                    assert gb == b and (gb is None or type(gb) is float), case
            assert r.unit == UNITS.get(case, "K"), (case, r.unit)
            # mask, fill value, WCS and meta are the left cube's; the values are new
            assert r.mask is left.mask and r.wcs is left.wcs and r.meta == left.meta, case
            assert np.array_equal(r.fill_value, left.fill_value, equal_nan=True), case
            assert not left._is_same_data(r), case
    # where the reference's unit strings are spelled the same way they agree
    rec = recorded(G, "np", "nan")
    for case in TABLE:
        if case not in ("pow_m1", "mul_jy"):
            assert rec[case][3] == UNITS.get(case, "K"), case
    assert rec["pow_m1"][3] == "1 / K" and rec["mul_jy"][3] == "Jy K"
    # the other unit rules
    cube = cubes_of(G, np.nan)[0]
    assert (cube ** 3).unit == "K3" and (cube / K(2.0)).unit == "" and (cube / Q(2.0, "s")).unit == "K / s"
    assert (cube * K(2.0)).unit == "K2" and (cube * 2).unit == "K" and (cube / 2).unit == "K"
    with pytest.raises(NotImplementedError):
        cube ** 1.7
    with pytest.raises(UnitsError):
        cube + Q(1.0, "Jy")
    with pytest.raises(UnitsError):
        cube - SpectralCube(G["data"], header=header_of(G, "Jy"))

    class Convertible(Q):
        def to(self, unit):
            assert unit == "K" and self.unit == "mK"
            return Q(self.value / 1e3, unit)
    assert (cube - Convertible(250.0, "mK"))._arith.steps == (("sub", 0.25, True),)


def test_error_rows_raise_what_the_reference_raises():
    G = golden("arith.npz")
    cube, bare, powbase, o = cubes_of(G, np.nan)
    builtin = {e.__name__: e for e in (ValueError, NotImplementedError, AssertionError, TypeError)}
    for cls, fname, fill in groups(G):
        g = "%s|%s|" % (cls, fname)
        names = [str(n) for n in G[g + "raising"]]
        assert set(names) == set(RAISING) | ({"mul_jy"} if cls == "dask" else set())
        for name, exc, msg in zip(names, G[g + "raises"], G[g + "messages"]):
            if name == "mul_jy":                               # the Dask class alone: units are strings here, 'K Jy' is one
                continue
            with pytest.raises(builtin[str(exc)]) as info:
                RAISING[name](cube, o)
            if name in ("add_plain", "sub_plain", "floordiv"):
                assert str(info.value) == str(msg), name
    with pytest.raises(ValueError, match="could not be broadcast"):
        cube * np.ones(7, np.float32)                          # a (nz,) spectrum: it has to be (nz, 1, 1)
    assert (bare + 1).unit == "" and (cube * np.ones((7, 1, 1), np.float32))._pending_arith_steps() == 1


def test_operand_shapes_and_narrowing():
    shape = (7, 5, 6)
    exp = {(): None, (6,): (0, 0, 1), (5, 6): (0, 6, 1), (5, 1): (0, 1, 0), (7, 1, 1): (1, 0, 0), (7, 5, 1): (5, 1, 0),
           (1, 5, 6): (0, 6, 1), (7, 1, 6): (6, 0, 1), (7, 5, 6): (30, 6, 1), (1, 1, 1): (0, 0, 0), (1,): (0, 0, 0)}
    for s, strides in exp.items():
        if strides is not None:
            assert ops.arith_operand_strides(s, shape) == strides, s
    for bad in ((7,), (5,), (7, 5), (7, 5, 5), (1, 7, 5, 6), (2, 1, 1)):
        with pytest.raises(ValueError, match="could not be broadcast"):
            ops.arith_operand_strides(bad, shape)
    G = golden("arith.npz")
    cube = cubes_of(G, np.nan)[0]
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cube * G["map2"]                                       # float32: nothing to say
        cube * 1e3
        cube * np.float64(2.5)                                 # a scalar follows the cube (numpy's value-based casting)
    with pytest.warns(PrecisionWarning):
        r = cube * G["map2"].astype(np.float64)                # the reference would return float64
    assert r._arith.steps[0][1].dtype == np.float32
    with pytest.raises(TypeError):
        cube * (1 + 2j)


# ---- fusion ----------------------------------------------------------------------------------------------------------
def test_fusion_planning():
    G = golden("arith.npz")
    cube, bare, powbase, o = cubes_of(G, np.nan)
    assert cube._pending_arith_steps() is None
    a = cube - K(o["map"])
    b = a / o["map2"]
    c = b * 1e3
    assert [x._pending_arith_steps() for x in (a, b, c)] == [1, 2, 3]
    assert c._arith.source is cube and b._arith.source is cube
    # extending a result leaves the parent's own program as it was
    assert len(a._arith.steps) == 1 and len(b._arith.steps) == 2 and a._arith.steps == b._arith.steps[:1]
    assert isinstance(a._arith.steps, tuple) and a._arith is not b._arith
    b2 = a + K(1.0)                                            # a second branch off the same parent
    assert b2._pending_arith_steps() == 2 and b._arith.steps[1][0] == "div" and b2._arith.steps[1][0] == "add"
    # a fifth step starts a new program on the four-step result
    d4 = c + K(1.0)
    e5 = d4 - K(1.0)
    assert d4._pending_arith_steps() == _lib.ARITH_MAX_STEPS == 4 and e5._pending_arith_steps() == 1
    assert e5._arith.source is d4 and len(d4._arith.steps) == 4
    # a changed fill value or mask in between breaks the chain
    f = b.with_fill_value(0.0) * 2
    assert f._pending_arith_steps() == 1 and f._arith.source._is_same_data(b) and f._arith.fill == 0.0
    m = b.with_mask(G["keep2"]) * 2
    assert m._pending_arith_steps() == 1 and m._arith.mask is not b.mask
    # cube on cube extends the left chain; a right-hand side that is itself pending does not (it is materialised first)
    g = a - o["cube2"]
    assert g._pending_arith_steps() == 2 and g._arith.steps[1] == ("sub", o["cube2"], False)
    h = a - (o["cube2"] * 2)
    assert h._pending_arith_steps() == 1 and h._arith.source is a
    # the exact power forms inside a chain
    assert [s[0] for s in ((cube * 2) ** 2)._arith.steps] == ["mul", "square"]
    assert [s[0] for s in (((cube * 2) ** 1) ** 0.5)._arith.steps] == ["mul", "mul", "sqrt"]


def test_lazy_mask_terms_stay_on_the_original_cube():
    G = golden("arith.npz")
    cube = SpectralCube(G["data"], header=header_of(G))
    lz = cube.with_mask(cube > 0.2)
    r = lz + K(5.0)
    r2 = r * 2 - K(1.0)
    from spectral_cube_amd import masks as M
    for res in (r, r2):
        assert res.mask is lz.mask and M.foreign_owner(res.mask)._is_same_data(cube) and not res._is_same_data(cube)
    assert np.array_equal(lz.mask.include(data=G["data"]), G["np|lazy|include"])


def test_cube_on_cube_checks():
    G = golden("arith.npz")
    cube, bare, powbase, o = cubes_of(G, np.nan)
    from spectral_cube_amd.cube import WCSMismatchWarning
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        cube - o["cube2"]                                      # one header: nothing to say
    moved = SpectralCube(G["data2"], header=dict(header_of(G), CRVAL1=31.0))
    with pytest.warns(WCSMismatchWarning, match="WCSs do not match"):
        r = cube - moved
    assert r._pending_arith_steps() == 1 and r.wcs is cube.wcs, "the left cube's WCS is kept"
    # shapes are compared by an explicit raise (it survives python -O), units must be equal for every operator - the
    # reference's is_equivalent test comes before the operator is looked at (spectral_cube.py:976-978)
    with pytest.raises(AssertionError, match="shapes differ"):
        cube * SpectralCube(G["data2"][:, :, :5], header=header_of(G))
    jy = SpectralCube(G["data2"], header=header_of(G, "Jy"))
    for fn in (lambda: cube * jy, lambda: cube / jy, lambda: cube + jy):
        with pytest.raises(UnitsError, match="K is not equivalent to Jy"):
            fn()


# ---- the ABI ---------------------------------------------------------------------------------------------------------
def test_entry_points_exported_and_declared():
    lib = _lib.load()
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name in ("spc_arith_f32", "spc_arith_f64"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name + " is not declared in include/spcube_hip.h"
    assert _lib.ARITH_MAX_STEPS == int(re.search(r"#define SPC_ARITH_MAX_STEPS (\d+)", text).group(1)) == 4
    enum = dict((k.lower(), int(v)) for k, v in re.findall(r"SPC_AOP_(\w+) = (\d+)", text))
    assert enum == _lib.ARITH_OPCODES and len(enum) == 9
    assert lib.spc_abi_version() == 8
    import ctypes as C
    assert C.sizeof(_lib.SpcArithStep) == 56 and C.sizeof(_lib.SpcArithProgram) == 8 + 4 * 56
    for op in ("__add__", "__sub__", "__mul__", "__truediv__", "__pow__", "__floordiv__"):
        assert op in SpectralCube.__dict__, op
    for op in ("__radd__", "__rsub__", "__rmul__", "__rtruediv__", "__neg__", "__pos__"):
        assert not hasattr(SpectralCube, op), op + ": the reference has no reflected or unary operators"
    src = open(os.path.join(REPO, "spectral_cube_amd", "csrc", "spc_arith.hip")).read()
    assert "#pragma clang fp contract(off)" in src
    mk = open(os.path.join(REPO, "spectral_cube_amd", "csrc", "Makefile")).read()
    assert "spc_arith.hip" in mk
