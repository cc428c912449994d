"""Cube arithmetic on the device (spc_arith_f32 / _f64 behind SpectralCube's + - * / **), checked against the reference's
recorded results (tests/golden/arith.npz) and the numpy restatement of the step program in tests/test_arith_host.py.

Bounds.  + - * / and the exact power forms (** 2, 0.5, -1, 1, 0: x * x, sqrt, 1 / x, a copy, ones) are single correctly
rounded IEEE operations on both sides: every comparison of them is ``np.array_equal(..., equal_nan=True)``.  A general
power goes through the device's pow: the bound is twice the largest distance measured on an MI355X over these inputs
(profiles/arith_pow_ulp.txt), for float32 against the recorded reference and for float64 against numpy's pow on this host:
1 ulp was measured for both, so 2 ulp is asserted for both (the golden's libm, the host's and the device pow are each within
a couple of ulp of the true value and the fixture is small)."""
import ctypes as C
import warnings

import numpy as np
import pytest

from conftest import assert_close, golden
from test_arith_host import (BARE, GENERAL_POW, K, TABLE, UNITS, arrays_of, cubes_of, groups, header_of, pick, recorded, restate,
                             source_of, ulp_distance)
from spectral_cube_amd import PrecisionWarning, SpectralCube, _lib, ops
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

POW_ULP_F32 = 2          # 2 x the 1 ulp measured (profiles/arith_pow_ulp.txt)
POW_ULP_F64 = 2          # likewise


def values(cube):
    return (cube._device_data64() if cube._runs_wide() else cube._device_data()).get()


# ---- against the reference -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_goldens_through_spectral_cube(gpu, dtype):
    G = golden("arith.npz")
    keep, arrays = G["keep"], arrays_of(G, dtype)
    worst = 0
    with warnings.catch_warnings():
        warnings.simplefilter("error", PrecisionWarning)       # nothing is narrowed on either path
        for fname, fill in (("nan", np.nan), ("0", 0.0)):
            cube, bare, powbase, o = cubes_of(G, fill, dtype)
            rec = recorded(G, "np", fname)
            for case, (expr, steps) in TABLE.items():
                left = pick(case, cube, bare, powbase)
                r = expr(left, o)
                assert r._pending_arith_steps() == len(steps)
                raw = values(r)
                assert r._pending_arith_steps() is None and raw.dtype == dtype, case
                exp = restate(source_of(G, case).astype(dtype), keep, fill, steps, arrays)
                what = "%s fill %s %s" % (np.dtype(dtype).name, fname, case)
                assert np.array_equal(np.isnan(raw), np.isnan(exp)), what
                if case in GENERAL_POW:
                    ref = rec[case][0] if dtype == np.float32 else exp
                    dist = ulp_distance(raw, ref)
                    worst = max(worst, dist)
                    print("%s: %d ulp from the %s" % (what, dist, "recorded reference" if dtype == np.float32 else "host's pow"))
                    assert dist <= (POW_ULP_F32 if dtype == np.float32 else POW_ULP_F64), what
                else:
                    assert np.array_equal(raw, exp, equal_nan=True), what
                    if dtype == np.float32:                    # both reference classes, bit for bit
                        assert np.array_equal(raw, rec[case][0], equal_nan=True), what
                        if case != "mul_jy":
                            assert np.array_equal(raw, recorded(G, "dask", fname)[case][0], equal_nan=True), what
                filled = r.filled_data
                assert filled.dtype == dtype and np.array_equal(filled, np.where(keep, raw, dtype(fill)), equal_nan=True), what
                if dtype == np.float32 and case not in GENERAL_POW:
                    assert np.array_equal(filled, rec[case][1], equal_nan=True), what
                assert np.array_equal(r.get_mask_array(), rec[case][2]), what
                assert r.unit == UNITS.get(case, "K"), what
    print("general pow, %s: %d ulp at most" % (np.dtype(dtype).name, worst))


def test_excluded_voxels_after_a_chain_with_fill_0(gpu):
    G = golden("arith.npz")
    keep = G["keep"]
    cube, bare, powbase, o = cubes_of(G, 0.0)
    raw = values(TABLE["chain_mul_add"][0](cube, o))
    assert np.array_equal(raw[~keep], np.broadcast_to(G["map"], keep.shape)[~keep]), "op2(0, b): 0 + map"
    assert np.array_equal(raw, recorded(G, "np", "0")["chain_mul_add"][0], equal_nan=True)
    raw = values(TABLE["chain3"][0](cube, o))
    assert (raw[~keep] == 0).all() and np.array_equal(raw, recorded(G, "np", "0")["chain3"][0], equal_nan=True)
    # (cube - 1 K) - 1 K: an excluded voxel holds 0 - 1, not (0 - 1) - 1
    raw = values(cube - K(1.0) - K(1.0))
    assert (raw[~keep] == -1).all() and np.array_equal(raw[keep], (G["data"] - np.float32(1) - np.float32(1))[keep], equal_nan=True)


def test_the_mask_reads_the_original_data(gpu):
    G = golden("arith.npz")
    cube = SpectralCube(G["data"], header=header_of(G))
    r = cube.with_mask(cube > 0.2) + K(5.0)
    assert np.array_equal(r.get_mask_array(), G["np|lazy|include"]) and np.array_equal(r.get_mask_array(), G["data"] > 0.2)
    for cls in ("np", "dask"):
        exp = float(G[cls + "|lazy|sum"])
        assert abs(float(r.sum()) - exp) <= 1e-5 * abs(exp)
        m0 = G[cls + "|lazy|moment0"]
        assert_close(r.moment0(), m0, atol=1e-5 * np.nanmax(np.abs(m0)), what="moment 0 after + 5 K")
    # a chained result, fused and past the end of a program: the terms are still evaluated on the original samples
    assert r._pending_arith_steps() is None, "sum() and moment0() have run the program"
    r4 = r * 2 * 2 * 2 * 2                                     # a new program on the materialised result
    assert r4._pending_arith_steps() == 4 and r4._arith.source is r
    assert np.array_equal(r4.get_mask_array(), G["data"] > 0.2)
    fresh = cube.with_mask(cube > 0.2) + K(5.0)
    r5 = fresh * 2 * 2 * 2 * 2                                 # the fifth step starts a program on the pending four-step result
    assert r5._pending_arith_steps() == 1 and r5._arith.source._pending_arith_steps() == 4
    assert np.array_equal(r5.get_mask_array(), G["data"] > 0.2)
    inc = G["data"] > 0.2
    for res in (r4, r5):
        assert np.array_equal(values(res)[inc], ((G["data"] + np.float32(5)) * np.float32(16))[inc])


# ---- fusion ----------------------------------------------------------------------------------------------------------
def test_fused_chain_equals_the_steps_one_by_one(gpu):
    G = golden("arith.npz")
    for fname, fill in (("nan", np.nan), ("0", 0.0)):
        cube, bare, powbase, o = cubes_of(G, fill)
        fused = TABLE["chain3"][0](cube, o)
        assert fused._pending_arith_steps() == 3
        a = cube - K(o["map"])
        a._device_data()
        b = a / o["map2"]
        assert a._pending_arith_steps() is None and b._pending_arith_steps() == 1 and b._arith.source is a
        b._device_data()
        c = b * 1e3
        assert c._pending_arith_steps() == 1 and c._arith.source is b
        got = values(fused)
        assert np.array_equal(got, values(c), equal_nan=True)
        assert np.array_equal(got, recorded(G, "np", fname)["chain3"][0], equal_nan=True)
        assert np.array_equal(fused.get_mask_array(), c.get_mask_array())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_multiply_then_add_is_not_contracted(gpu, dtype):
    rng = np.random.default_rng(5)
    shape = (6, 9, 37)
    d, m, a = (rng.normal(size=s).astype(dtype) for s in (shape, shape[1:], shape[1:]))
    cube = SpectralCube(d, header=dict(header_of(golden("arith.npz"), "")))
    r = cube * m + a
    assert r._pending_arith_steps() == 2
    got = values(r)
    prod = d * m
    exp = prod + a
    fma = (d.astype(np.longdouble) * m + a).astype(dtype)      # one rounding: what a fused multiply-add gives
    assert (fma != exp).sum() > exp.size // 20, "the data tell an FMA from two roundings"
    assert np.array_equal(got, exp), "%d voxels differ from numpy's stepwise result" % (got != exp).sum()
    # scalars the same way: x * s + t
    got = values(cube * 1.1 + 0.3)
    assert np.array_equal(got, d * dtype(1.1) + dtype(0.3))


# ---- cube on cube ----------------------------------------------------------------------------------------------------
def test_cube_on_cube(gpu):
    G = golden("arith.npz")
    cube, bare, powbase, o = cubes_of(G, 0.0)
    for name, fn in (("sub", np.subtract), ("add", np.add), ("mul", np.multiply), ("div", np.divide)):
        r = TABLE[name + "_cube"][0](cube, o)
        with np.errstate(all="ignore"):
            exp = fn(G["data"], G["data2"])
        assert np.array_equal(values(r), exp, equal_nan=True), name + ": the raw samples of both cubes, nothing filled"
        assert r.mask is cube.mask and np.array_equal(r.get_mask_array(), G["keep"]), "only the left mask"
    with pytest.raises(AssertionError):
        cube - o["cube2"][:, :, :5]
    # a pending right-hand side is materialised, a pending left-hand side extended
    r = (cube * 2) - (o["cube2"] * 2)
    assert np.array_equal(values(r), np.where(G["keep"], G["data"], np.float32(0)) * np.float32(2)
                          - np.where(G["keep2"], G["data2"], np.float32(np.nan)) * np.float32(2), equal_nan=True)


# ---- shapes where indexing can go wrong --------------------------------------------------------------------------------
SHAPES = [(3, 2, 67), (2, 3, 1), (5, 4, 3), (2, 2, 8), (1, 1, 70001), (70001, 1, 2), (2, 70001, 1)]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(n) for n in s))
def test_shapes_and_operand_kinds(gpu, shape, dtype):
    rng = np.random.default_rng(sum(shape))
    nz, ny, nx = shape
    d = rng.normal(size=shape).astype(dtype)
    d[rng.random(shape) < 0.02] = np.nan
    inc = rng.random(shape) < 0.8
    arrays = {"row": rng.normal(size=(nx,)), "map": rng.normal(size=(ny, nx)), "col": rng.normal(size=(ny, 1)),
              "spec": 1.0 + rng.random((nz, 1, 1)), "zy": 1.0 + rng.random((nz, ny, 1)), "full": rng.normal(size=shape),
              "zx": rng.normal(size=(nz, 1, nx)), "one": rng.normal(size=(1, 1, 1))}
    arrays = {k: v.astype(dtype) for k, v in arrays.items()}
    dev = {k: DeviceArray.from_numpy(v) for k, v in arrays.items()}
    cube = DeviceArray.from_numpy(d)
    mask = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, DeviceArray.from_numpy(inc.astype(np.uint8)))
    programs = [[("add", "row", 1), ("mul", "col", 1), ("sub", "spec", 1), ("div", "full", 0)],
                [("mul", "map", 1), ("add", "zy", 1), ("mul", 0.75, 1), ("square", None, 1)],
                [("sub", "zx", 1), ("div", "one", 0), ("recip", None, 0)],
                [("sub", "full", 0)], [("mul", -1.5, 1)]]
    for fill in (0.0, np.nan):
        for steps in programs:
            got = ops.arith(cube, [(op, dev.get(b, b) if isinstance(b, str) else b, r) for op, b, r in steps], mask=mask, fill=fill).get()
            exp = restate(d, inc, fill, steps, arrays)
            assert np.array_equal(got, exp, equal_nan=True), (shape, steps, int((~np.isclose(got, exp, equal_nan=True)).sum()))
    # without a mask every voxel is included
    got = ops.arith(cube, [("add", dev["row"], 1), ("mul", dev["spec"], 1)]).get()
    assert np.array_equal(got, (d + arrays["row"]) * arrays["spec"], equal_nan=True)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_padded_rows_and_a_misaligned_first_element(gpu, dtype):
    """row_stride = nx + 3 and a first element one sample past a 16-byte boundary, for the cube, the mask, a cube operand and
    the output, each at its own phase: heads, tails and rows that cannot use the 16-byte forms"""
    rng = np.random.default_rng(11)
    nz, ny, nx = 3, 5, 21
    rs, ps = nx + 3, (nx + 3) * ny + 5
    n = ps * nz + 8

    def view(buf, first, dt):
        v = DeviceArray((nz, ny, nx), dt, ptr=buf.ptr + first * np.dtype(dt).itemsize, owner=buf)
        v.row_stride, v.plane_stride = rs, ps
        return v

    def strided(host, first):
        return np.lib.stride_tricks.as_strided(host[first:], (nz, ny, nx), tuple(s * host.itemsize for s in (ps, rs, 1)))

    hd, hb, hm = rng.normal(size=n).astype(dtype), rng.normal(size=n).astype(dtype), (rng.random(n) < 0.7).astype(np.uint8)
    bd, bb, bm = (DeviceArray.from_numpy(h) for h in (hd, hb, hm))
    sentinel = np.full(n, -77.0, dtype)
    for firsts in ((1, 2, 3, 1), (0, 0, 0, 0), (3, 3, 3, 3), (2, 0, 1, 2)):
        fd, fb, fm, fo = firsts
        bo = DeviceArray.from_numpy(sentinel)
        out = view(bo, fo, dtype)
        mask = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, view(bm, fm, np.uint8))
        steps = [("mul", view(bb, fb, dtype), 1), ("add", 0.5, 1)]
        ops.arith(view(bd, fd, dtype), steps, mask=mask, fill=0.0, out=out)
        got = bo.get()
        d, b, inc = strided(hd, fd), strided(hb, fb), strided(hm, fm) != 0
        exp = np.where(inc, np.where(inc, d, dtype(0)) * b, dtype(0)) + dtype(0.5)
        assert np.array_equal(strided(got, fo), exp), firsts
        touched = np.zeros(n, bool)
        strided(touched, fo)[...] = True
        assert (got[~touched] == -77.0).all(), "nothing outside the output view is written"


# ---- validation through the C ABI --------------------------------------------------------------------------------------
def test_invalid_programs_are_refused_before_anything_is_queued(gpu):
    lib = _lib.load()
    shape = (3, 4, 5)
    d = np.arange(60, dtype=np.float32).reshape(shape)
    cube, other = DeviceArray.from_numpy(d), DeviceArray.from_numpy(d + 1)
    out = DeviceArray.from_numpy(np.full(shape, -77.0, np.float32))
    c = ops._cube_c(cube)

    def program(*steps):
        p = _lib.SpcArithProgram()
        p.n_steps = len(steps)
        for s, (op, is_scalar, ptr, strides) in zip(p.steps, steps[:_lib.ARITH_MAX_STEPS]):
            s.opcode, s.refill, s.is_scalar, s.scalar, s.d_data = op, 1, is_scalar, 2.0, ptr
            s.stride_z, s.stride_y, s.stride_x = strides
        return p

    def run(prog, dst):
        return lib.spc_arith_f32(0, None, C.byref(c), None, 0, C.c_float(0.0), C.byref(prog), C.c_void_p(dst), 0, 0)

    full, scalar = (20, 5, 1), (0, 0, 0)
    ok = program((_lib.AOP_ADD, 1, None, scalar))
    bad = {
        "d_out is the cube": (ok, cube.ptr),
        "d_out overlaps the cube": (ok, cube.ptr + 4 * 59),
        "d_out is an operand": (program((_lib.AOP_ADD, 0, out.ptr, full)), out.ptr),
        "an operand pointer with the scalar flag": (program((_lib.AOP_ADD, 1, other.ptr, full)), out.ptr),
        "an array operand without a pointer": (program((_lib.AOP_ADD, 0, None, full)), out.ptr),
        "an array operand of a unary opcode": (program((_lib.AOP_SQRT, 0, other.ptr, full)), out.ptr),
        "no steps": (program(), out.ptr),
        "too many steps": (program(*[(_lib.AOP_ADD, 1, None, scalar)] * 5), out.ptr),
        "an unknown opcode": (program((9, 1, None, scalar)), out.ptr),
        "stride_x 2": (program((_lib.AOP_ADD, 0, other.ptr, (20, 5, 2))), out.ptr),
        "a negative stride": (program((_lib.AOP_ADD, 0, other.ptr, (-20, 5, 1))), out.ptr),
    }
    for what, (prog, dst) in bad.items():
        assert run(prog, dst) == _lib.SPC_ERR_INVALID, what
        assert _lib.last_error(), what
    with pytest.raises(_lib.HipInvalidArgument, match="d_out overlaps the cube"):
        ops.arith(cube, [("add", 1.0, 1)], out=cube)
    with pytest.raises(_lib.HipInvalidArgument, match="at least one step"):
        ops.arith(cube, [])
    with pytest.raises(_lib.HipInvalidArgument, match="at most 4"):
        ops.arith(cube, [("add", 1.0, 1)] * 5)
    _lib.call("spc_device_sync", 0)
    assert (out.get() == -77.0).all() and np.array_equal(cube.get(), d), "no kernel ran"
    assert run(ok, out.ptr) == _lib.SPC_OK and np.array_equal(out.get(), d + 2)
