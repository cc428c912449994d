"""masks.compile_mask without a device: a mask tree becomes a postfix program (slots, un-broadcast operands, instructions)
whose meaning - worked out by the small numpy interpreter below, test code only - is numpy's own ``mask.include()``, voxel
for voxel: every comparison, thresholds of every shape class and accepted dtype, | ^ ~ &, a region map, a second cube,
NaN / inf / signed zeros and samples equal to the thresholds.  The GPU tests run the same trees (``case()``)."""
import operator

import numpy as np
import pytest

from spectral_cube_amd import SpectralCube, _lib
from spectral_cube_amd import masks as M
from spectral_cube_amd.cube import _WideView

SHAPE = (5, 4, 7)
OPS = {"gt": operator.gt, "ge": operator.ge, "lt": operator.lt, "le": operator.le, "eq": operator.eq, "ne": operator.ne}
DTYPES = ("bool", "int8", "int16", "int32", "int64", "uint8", "uint16", "uint32", "uint64", "float16", "float32", "float64")


@pytest.fixture(autouse=True)
def _budget(monkeypatch):
    monkeypatch.setenv("SPC_HBM_BUDGET", "1G")       # "does this cube fit" is asked of the device otherwise


def samples(shape, dtype, seed):
    """multiples of 0.25 in [-2, 2] (so that samples EQUAL thresholds), a few float32(0.1), NaN, +-inf and +-0"""
    rng = np.random.default_rng(seed)
    d = (rng.integers(-8, 9, size=shape) * 0.25).astype(dtype)
    flat = d.reshape(-1)
    n = flat.size
    special = [np.nan, np.inf, -np.inf, 0.0, -0.0, np.float32(0.1), np.nan, np.float32(0.1)]
    for i, v in enumerate(special):
        flat[(i * 7 + 3) % n] = v
    flat[:: max(n // 5, 1)] = np.float32(0.1)
    return d


def case(shape, dtype, seed=3, data=None, other=None):
    """(cube, other cube, {name: mask tree}) over host cubes of *shape* / *dtype* (or over the arrays given)"""
    nz, ny, nx = shape
    rng = np.random.default_rng(seed + 100)
    cube = SpectralCube(samples(shape, dtype, seed) if data is None else data)
    oth = SpectralCube(samples(shape, dtype, seed + 1) if other is None else other)

    def thr(*s):
        return rng.integers(-4, 5, size=s) * 0.25

    def cmp(op, v, c=cube):
        return M.LazyComparisonMask(OPS[op], v, cube=c)

    shapes = {"spectrum": (nz, 1, 1), "map": (ny, nx), "row": (1, nx), "x": (nx,), "full": (nz, ny, nx)}
    t = {}
    for op in OPS:
        t["%s_weak" % op] = cmp(op, 0.25)
        t["%s_map" % op] = cmp(op, thr(ny, nx).astype(np.float32))
    for name, s in shapes.items():
        t["gt_f32_" + name] = cmp("gt", thr(*s).astype(np.float32))
        t["le_f64_" + name] = cmp("le", thr(*s) + 0.1)
    for dt in DTYPES:
        a = rng.integers(0, 2, size=(ny, nx)) if dt == "bool" or dt.startswith("u") else rng.integers(-2, 3, size=(ny, nx))
        t["ge_map_" + dt] = cmp("ge", (a * (0.25 if dt.startswith("f") else 1)).astype(dt))
    t["gt_f64_scalar"] = cmp("gt", np.float64(0.1))
    t["gt_weak_tenth"] = cmp("gt", 0.1)
    t["le_f32_scalar"] = cmp("le", np.float32(0.1))
    t["ge_f16_scalar"] = cmp("ge", np.float16(0.25))
    t["lt_i64_scalar"] = cmp("lt", np.int64(1))
    t["ge_weak_int"] = cmp("ge", 1)
    t["gt_0d"] = cmp("gt", np.array(-0.5))
    t["eq_zero"] = cmp("eq", 0.0)
    t["ne_zero"] = cmp("ne", 0.0)
    t["gt_nan"] = cmp("gt", float("nan"))
    t["ne_nan"] = cmp("ne", np.float64("nan"))
    t["gt_minus_inf"] = cmp("gt", -np.inf)
    t["le_inf"] = cmp("le", np.inf)
    t["ne_map_with_nan"] = cmp("ne", np.where(thr(ny, nx) > 0.5, np.nan, thr(ny, nx)))
    t["finite"] = M.LazyMask(np.isfinite, cube=cube)
    t["notnan"] = M.NotNaNMask(cube)
    rms = np.abs(thr(ny, nx)) + 0.25
    region = rng.integers(0, 2, size=(ny, nx)).astype(bool)
    t["or"] = cmp("gt", 5 * rms) | cmp("lt", -5 * rms)
    t["wing"] = cmp("gt", rms) | cmp("lt", -rms)
    t["xor"] = cmp("gt", rms) ^ cmp("ge", 0.5)
    t["not"] = ~cmp("gt", 3 * rms)
    t["and_finite_map"] = M.LazyMask(np.isfinite, cube=cube) & cmp("gt", rms.astype(np.float32))
    t["region"] = M.BooleanArrayMask(region, shape=shape)
    t["region_excluded"] = M.BooleanArrayMask(region, shape=shape, include=False)
    t["finite_and_region"] = M.LazyMask(np.isfinite, cube=cube) & M.BooleanArrayMask(region, shape=shape)
    t["other_cube"] = cmp("gt", 2 * rms, oth)
    t["two_cubes"] = (cmp("gt", rms) & cmp("le", 0.75, oth)) | M.NotNaNMask(oth)
    t["depth4"] = ~(((cmp("gt", rms) | cmp("lt", thr(nz, 1, 1))) ^ M.BooleanArrayMask(region, shape=shape, include=False))
                    & (M.LazyMask(np.isfinite, cube=cube) | ~cmp("eq", 0.25, oth)))
    t["own_array"] = M.LazyComparisonMask(operator.ge, 0.5, data=cube._data)
    return cube, oth, t


def compiled(mask, cube, wide):
    return M.compile_mask(mask, _WideView(cube) if wide else cube, cube.shape, wide)


def operand_view(arr, strides, shape):
    """operand (a C-contiguous un-broadcast array + element strides) as the kernel addresses it"""
    return np.lib.stride_tricks.as_strided(arr.reshape(-1), shape, [s * arr.itemsize for s in strides], writeable=False)


def interpret(prog, slot_data, shape):
    """what spc_mask_eval computes, in numpy: samples and thresholds compared as doubles"""
    stack = []
    for opcode, slot, cmp_, operand, imm in prog.instr:
        if opcode == _lib.MOP_CMP:
            x = slot_data[slot].astype(np.float64)
            th = np.float64(imm) if operand < 0 else operand_view(*prog.operands[operand], shape).astype(np.float64)
            fn = [operator.gt, operator.ge, operator.lt, operator.le, operator.eq, operator.ne][cmp_]
            with np.errstate(invalid="ignore"):
                stack.append(np.broadcast_to(fn(x, th), shape))
        elif opcode == _lib.MOP_FINITE:
            stack.append(np.isfinite(slot_data[slot]))
        elif opcode == _lib.MOP_LOAD:
            arr, strides = prog.operands[operand]
            assert arr.dtype == np.uint8
            stack.append(operand_view(arr, strides, shape) != 0)
        elif opcode == _lib.MOP_NOT:
            stack.append(~stack.pop())
        else:
            b, a = stack.pop(), stack.pop()
            stack.append({_lib.MOP_AND: a & b, _lib.MOP_OR: a | b, _lib.MOP_XOR: a ^ b}[opcode])
        assert len(stack) <= _lib.MASK_PROG_MAX_STACK
    out, = stack
    return out


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_compiled_program_means_what_numpy_computes(dtype):
    wide = dtype is np.float64
    cube, oth, trees = case(SHAPE, dtype)
    d = cube._data
    assert np.isnan(d).any() and np.isposinf(d).any() and np.isneginf(d).any() and (d == 0.25).any()
    assert np.signbit(d[d == 0]).any() and not np.signbit(d[d == 0]).all()
    for name, mask in trees.items():
        prog = compiled(mask, cube, wide)
        assert prog is not None, name
        assert len(prog.slots) <= 4 and len(prog.operands) <= 8 and len(prog.instr) <= 16
        for c in prog.slots:
            assert c is cube or c is oth, name
        with np.errstate(invalid="ignore"):
            want = np.broadcast_to(mask.include(), SHAPE)
        got = interpret(prog, [c._data for c in prog.slots], SHAPE)
        assert got.dtype == bool and np.array_equal(got, want), name
    assert len(compiled(trees["two_cubes"], cube, wide).slots) == 2
    assert compiled(trees["other_cube"], cube, wide).slots == [oth]
    assert compiled(trees["own_array"], cube, wide).slots == [cube]
    assert compiled(trees["wing"], cube, wide).slots == [cube]            # two terms, one slot: the cube is read once


def test_operands_stay_unbroadcast():
    nz, ny, nx = SHAPE
    cube, _, trees = case(SHAPE, np.float32)
    expect = {"gt_f32_spectrum": ((nz, 1, 1), (1, 0, 0)), "gt_f32_map": ((ny, nx), (0, nx, 1)), "gt_f32_row": ((1, nx), (0, 0, 1)),
              "gt_f32_x": ((nx,), (0, 0, 1)), "gt_f32_full": ((nz, ny, nx), (ny * nx, nx, 1))}
    for name, (shape, strides) in expect.items():
        (arr, got), = compiled(trees[name], cube, False).operands
        assert arr.shape == shape and arr.dtype == np.float32 and arr.flags.c_contiguous and got == strides, name
    for dt in DTYPES:
        (arr, got), = compiled(trees["ge_map_" + dt], cube, False).operands
        assert arr.dtype == (np.float32 if dt == "float32" else np.float64) and arr.shape == (ny, nx) and got == (0, nx, 1)
    prog = compiled(trees["region_excluded"], cube, False)
    (arr, got), = prog.operands
    assert arr.dtype == np.uint8 and arr.shape == (ny, nx) and got == (0, nx, 1)
    assert [i[0] for i in prog.instr] == [_lib.MOP_LOAD, _lib.MOP_NOT]
    assert compiled(trees["gt_weak"], cube, False).operands == []         # a scalar is an immediate
    # one term, never dropped: ~isnan of the cube's own data
    assert compiled(trees["notnan"], cube, False).instr == [(_lib.MOP_CMP, 0, _lib.CMP_LE, -1, float("inf"))]


def test_weak_scalar_is_rounded_to_the_sample_type_and_a_typed_one_is_not():
    cube, _, trees = case(SHAPE, np.float32)
    d = cube._data
    weak, typed = compiled(trees["gt_weak_tenth"], cube, False), compiled(trees["gt_f64_scalar"], cube, False)
    assert weak.instr[0][4] == float(np.float32(0.1)) and typed.instr[0][4] == 0.1
    a, b = interpret(weak, [d], SHAPE), interpret(typed, [d], SHAPE)
    with np.errstate(invalid="ignore"):
        na, nb = d > 0.1, d > np.float64(0.1)
    assert np.array_equal(a, na) and np.array_equal(b, nb)
    assert np.array_equal(a != b, na != nb) and np.array_equal(a != b, d == np.float32(0.1)) and (a != b).sum() >= 5
    # float64 samples: the Python scalar keeps its value
    cube64, _, trees64 = case(SHAPE, np.float64)
    assert compiled(trees64["gt_weak_tenth"], cube64, True).instr[0][4] == 0.1


def test_what_has_no_device_form_is_left_to_the_host():
    cube, oth, trees = case(SHAPE, np.float32)

    def cmp(v, op=operator.gt, c=cube):
        return M.LazyComparisonMask(op, v, cube=c)

    assert compiled(M.FunctionMask(lambda x: x > 0), cube, False) is None
    assert compiled(cmp(0.5) & M.FunctionMask(lambda x: x > 0), cube, False) is None
    assert compiled(M.LazyMask(np.isnan, cube=cube), cube, False) is None
    assert compiled(cmp(np.longdouble(0.5)), cube, False) is None
    assert compiled(cmp(np.ones(SHAPE[1:], dtype=np.longdouble)), cube, False) is None
    assert compiled(cmp(np.ones(SHAPE[1:], dtype=np.complex64)), cube, False) is None
    assert compiled(cmp(np.ones((3, 3))), cube, False) is None                     # not broadcastable to the cube
    assert compiled(cmp(0.5, operator.add), cube, False) is None
    assert compiled(M.LazyComparisonMask(operator.gt, 0.5, data=oth._data), cube, False) is None     # a bare array of another cube
    long = cmp(0.0)
    for i in range(1, 9):
        long = long | cmp(0.25 * i)
    assert compiled(long, cube, False) is None                                      # 9 terms + 8 operators > 16 instructions
    nine = cmp(np.zeros(SHAPE[2]))
    for i in range(8):
        nine = cmp(np.full(SHAPE[2], float(i))) & nine
    assert compiled(nine, cube, False) is None                                      # 9 operands
    five = cmp(0.0)
    for i in range(4):
        five = five & cmp(0.0, c=SpectralCube(samples(SHAPE, np.float32, 20 + i)))
    assert compiled(five, cube, False) is None                                      # 5 cubes
    assert compiled(cmp(0.0, c=SpectralCube(samples((5, 4, 6), np.float32, 9))), cube, False) is None   # another shape
    # a cube that would have to be narrowed (float32 path) or widened (float64 path) to be read
    cube64, _, _ = case(SHAPE, np.float64)
    assert compiled(cmp(0.0, c=cube64), cube, False) is None
    assert compiled(cmp(0.0, c=cube), cube64, True) is None
    assert compiled(cmp(0.0, c=cube64), cube64, False) is None
