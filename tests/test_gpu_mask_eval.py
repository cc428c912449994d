"""Mask expressions evaluated on the device (ops.mask_eval, spc_mask_eval_f32 / _f64; SpectralCube._lower_mask).

    what                               shapes                                      compared with               tolerance
    ops.mask_eval, every tree of       (7,5,19) odd rows: head + tail; (3,6,64)     numpy mask.include()        exact
      test_mask_program_host.case()    aligned; (4,3,1); planes(1,3) / rows(1,6)
                                       / swap01() views of a slot; a strided out;
                                       float32 and float64
    long axes, (c > map) | (c < -map)  (2,65540,5), (65540,2,3)                     numpy                       exact
    malformed programs                 (2,3,4)                                     SPC_ERR_INVALID + message,  d_out untouched
    cube level: the six idioms of a    (9,6,10) resident cube, _host_data raising  the same calls on a host    masks exact; values rtol 1e-8 +
      signal mask: moment0, statistics,                                             cube masked by the numpy    atol 1e-9 max|exp| (the bound of
      median(axis=0), get_mask_array                                                boolean array               test_gpu_cube::test_consistent_
                                                                                                                mask_handling: same kernels, same mask)
    reference pin                      tests/golden/mask_eval.npz                  the reference's             exact
                                                                                    get_mask_array()
"""
import ctypes as C
import operator

import numpy as np
import pytest

from conftest import assert_close, golden
from spectral_cube_amd import Gaussian1DKernel, SpectralCube, _lib, ops
from spectral_cube_amd import cube as cube_module
from spectral_cube_amd import masks as M
from spectral_cube_amd.device import DeviceArray
from spectral_cube_amd.wcs import parse_header
from test_mask_program_host import case, compiled, samples

pytestmark = pytest.mark.gpu

HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5,
       "CUNIT3": "km/s", "CRPIX1": 5, "CRPIX2": 3, "CRPIX3": 1, "CRVAL1": 10.0, "CRVAL2": 20.0, "CRVAL3": -2.0, "BUNIT": "K"}

# name -> (shape of the array in memory, host view of it, the same view of its DeviceArray)
LAYOUTS = {
    "odd_rows": ((7, 5, 19), lambda a: a, lambda d: d),
    "aligned": ((3, 6, 64), lambda a: a, lambda d: d),
    "one_column": ((4, 3, 1), lambda a: a, lambda d: d),
    "planes_view": ((5, 5, 19), lambda a: a[1:3], lambda d: d.planes(1, 3)),
    "rows_view": ((3, 8, 12), lambda a: a[:, 1:6], lambda d: d.rows(1, 6)),
    "swap01_view": ((4, 3, 9), lambda a: a.transpose(1, 0, 2), lambda d: d.swap01()),
    "strided_out": ((3, 4, 10), lambda a: a, lambda d: d),
}


def _expected(mask, shape):
    with np.errstate(invalid="ignore"):
        return np.broadcast_to(mask.include(), shape).astype(np.uint8)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_mask_eval_equals_numpy_on_every_tree(gpu, layout, dtype):
    wide = dtype is np.float64
    mem_shape, host_view, dev_view = LAYOUTS[layout]
    big = samples(mem_shape, dtype, 5)
    sub = host_view(big)
    shape = sub.shape
    other = samples(shape, dtype, 6)
    cube, oth, trees = case(shape, dtype, data=sub, other=other)
    big_dev = DeviceArray.from_numpy(big, gpu, dtype=dtype)
    dev = {id(cube): dev_view(big_dev), id(oth): DeviceArray.from_numpy(other, gpu, dtype=dtype)}
    assert tuple(dev[id(cube)].shape) == shape
    frame = None
    for name, mask in trees.items():
        prog = compiled(mask, cube, wide)
        assert prog is not None, name
        prog.slots = [dev[id(c)] for c in prog.slots]
        if layout == "strided_out":
            nz, ny, nx = shape
            frame = DeviceArray.from_numpy(np.full((nz, ny + 3, nx), 7, dtype=np.uint8), gpu)
            ops.mask_eval(prog, shape, gpu, dtype, out=frame.rows(2, ny + 2))
            whole = frame.get()
            got = whole[:, 2:ny + 2]
            assert (whole[:, :2] == 7).all() and (whole[:, ny + 2:] == 7).all(), name + ": wrote outside the view"
        else:
            got = ops.mask_eval(prog, shape, gpu, dtype).get()
        want = _expected(mask, shape)
        assert got.dtype == np.uint8 and np.array_equal(got, want), "%s: %d voxels differ, first at %s" % (
            name, (got != want).sum(), np.argwhere(got != want)[:4].tolist())


@pytest.mark.parametrize("shape", [(2, 65540, 5), (65540, 2, 3)], ids=["tall_planes", "long_spectra"])
def test_axes_longer_than_a_grid_dimension(gpu, shape):
    rng = np.random.default_rng(11)
    d = (rng.integers(-8, 9, size=shape) * 0.25).astype(np.float32)
    d[rng.random(shape) < 0.05] = np.nan
    thr = (rng.integers(1, 5, size=shape[1:]) * 0.25).astype(np.float32)
    cube = SpectralCube(d)
    mask = M.LazyComparisonMask(operator.gt, thr, cube=cube) | M.LazyComparisonMask(operator.lt, -thr, cube=cube)
    prog = compiled(mask, cube, False)
    prog.slots = [DeviceArray.from_numpy(d, gpu)]
    got = ops.mask_eval(prog, shape, gpu, np.float32).get()
    with np.errstate(invalid="ignore"):
        want = ((d > thr) | (d < -thr)).astype(np.uint8)
    assert np.array_equal(got, want), np.argwhere(got != want)[:4].tolist()
    assert 0 < want[-1].sum() < want[-1].size and 0 < want[:, -1].sum() < want[:, -1].size


def _program(instr, slots, operands, n_slots=None, n_operands=None, n_instr=None):
    p = _lib.SpcMaskProgram()
    p.n_slots = len(slots) if n_slots is None else n_slots
    p.n_operands = len(operands) if n_operands is None else n_operands
    p.n_instr = len(instr) if n_instr is None else n_instr
    for i, ptr in enumerate(slots):
        p.slots[i].d_data = ptr
    for i, (ptr, elem, strides) in enumerate(operands):
        p.operands[i].d_data, p.operands[i].elem = ptr, elem
        p.operands[i].stride_z, p.operands[i].stride_y, p.operands[i].stride_x = strides
    for i, (opcode, slot, cmp_, operand, imm) in enumerate(instr[:_lib.MASK_PROG_MAX_INSTR]):
        q = p.instr[i]
        q.opcode, q.slot, q.cmp, q.operand, q.imm = opcode, slot, cmp_, operand, imm
    return p


def test_malformed_programs_are_refused_before_any_device_work(gpu):
    shape = (2, 3, 4)
    data = DeviceArray.from_numpy(np.zeros(shape, np.float32), gpu)
    fmap = DeviceArray.from_numpy(np.zeros(shape[1:], np.float32), gpu)
    bmap = DeviceArray.from_numpy(np.ones(shape[1:], np.uint8), gpu)
    out = DeviceArray.from_numpy(np.full(shape, 9, np.uint8), gpu)
    F, U = (fmap.ptr, _lib.ELEM_F32, (0, 4, 1)), (bmap.ptr, _lib.ELEM_U8, (0, 4, 1))
    CMP, FIN, LOAD, NOT, AND = _lib.MOP_CMP, _lib.MOP_FINITE, _lib.MOP_LOAD, _lib.MOP_NOT, _lib.MOP_AND
    fin, cmp0, load1 = (FIN, 0, 0, -1, 0.0), (CMP, 0, _lib.CMP_GT, 0, 0.0), (LOAD, 0, 0, 1, 0.0)
    both = dict(slots=[data.ptr], operands=[F, U])

    def run(p, d_out=out.ptr, name="spc_mask_eval_f32"):
        _lib.call(name, gpu, None, shape[0], shape[1], shape[2], C.byref(p) if p is not None else None,
                  C.c_void_p(d_out) if d_out else None, 0, 0)

    run(_program([cmp0, load1, (AND, 0, 0, -1, 0.0), (NOT, 0, 0, -1, 0.0)], **both))        # the well-formed one runs
    assert (out.get() == 1).all()                                                           # ~((0 > 0) & 1)
    out.upload(np.full(shape, 9, np.uint8))
    bad = {
        "unknown opcode": _program([(99, 0, 0, -1, 0.0)], **both),
        "negative opcode": _program([(-1, 0, 0, -1, 0.0)], **both),
        "binary operator on one value": _program([fin, (AND, 0, 0, -1, 0.0)], **both),
        "NOT on an empty stack": _program([(NOT, 0, 0, -1, 0.0)], **both),
        "nine values on the stack": _program([fin] * 9 + [(AND, 0, 0, -1, 0.0)] * 7, **both),
        "two values left": _program([fin, fin], **both),
        "no instruction": _program([], **both),
        "too many instructions": _program([fin] * 16, n_instr=17, **both),
        "slot past the last": _program([(FIN, 1, 0, -1, 0.0)], **both),
        "negative slot": _program([(CMP, -1, _lib.CMP_GT, -1, 0.0)], **both),
        "slot of a program without slots": _program([fin], slots=[], operands=[F, U]),
        "too many slots": _program([fin], n_slots=5, **both),
        "operand past the last": _program([(CMP, 0, _lib.CMP_GT, 2, 0.0)], **both),
        "operand -2": _program([(CMP, 0, _lib.CMP_GT, -2, 0.0)], **both),
        "LOAD without an operand": _program([(LOAD, 0, 0, -1, 0.0)], **both),
        "too many operands": _program([fin], n_operands=9, **both),
        "NULL slot": _program([fin], slots=[None], operands=[F, U]),
        "NULL operand": _program([fin], slots=[data.ptr], operands=[(None, _lib.ELEM_F32, (0, 4, 1))]),
        "float operand under LOAD": _program([(LOAD, 0, 0, 0, 0.0)], **both),
        "uint8 operand under CMP": _program([(CMP, 0, _lib.CMP_GT, 1, 0.0)], **both),
        "unknown comparison": _program([(CMP, 0, 6, 0, 0.0)], **both),
        "unknown element type": _program([fin], slots=[data.ptr], operands=[(fmap.ptr, 3, (0, 4, 1))]),
        "negative operand stride": _program([fin], slots=[data.ptr], operands=[(fmap.ptr, _lib.ELEM_F32, (0, -4, 1))]),
    }
    for what, p in bad.items():
        for name in ("spc_mask_eval_f32", "spc_mask_eval_f64"):
            with pytest.raises((_lib.HipInvalidArgument, _lib.HipLibraryError)) as err:
                run(p, name=name)
            assert isinstance(err.value, _lib.HipInvalidArgument) and str(err.value).strip(), what
    good = _program([fin], **both)
    for kw in (dict(p=None), dict(p=good, d_out=None)):
        with pytest.raises(_lib.HipInvalidArgument) as err:
            run(**kw)
        assert str(err.value).strip()
    # and through ops.mask_eval: the description reaches the same checks
    prog = M.MaskProgram()
    prog.slots, prog.instr = [data], [(FIN, 0, 0, -1, 0.0), (FIN, 0, 0, -1, 0.0)]
    with pytest.raises(_lib.HipInvalidArgument, match="stack"):
        ops.mask_eval(prog, shape, gpu, np.float32, out=out)
    assert (out.get() == 9).all()


# ---- cube level ---------------------------------------------------------------------------------------------------------
def _idioms(cube, rms, region):
    """the six ways into a signal mask; numpy's statement of each on the samples d (and those of the smoothed cube)"""
    smooth = cube.spectral_smooth(Gaussian1DKernel(2))
    return smooth, {
        "sig": (lambda: cube > 3 * rms, lambda d, s: d > 3 * rms),
        "wing": (lambda: (cube > 5 * rms) | (cube < -5 * rms), lambda d, s: (d > 5 * rms) | (d < -5 * rms)),
        "off": (lambda: ~(cube > 3 * rms), lambda d, s: ~(d > 3 * rms)),
        "dil": (lambda: smooth > 2 * rms, lambda d, s: s > 2 * rms),
        "roi": (lambda: region, lambda d, s: np.broadcast_to(region, d.shape)),
        "finite_roi": (lambda: M.LazyMask(np.isfinite, cube=cube) & M.BooleanArrayMask(region, shape=cube.shape),
                       lambda d, s: np.isfinite(d) & region),
    }


def _signal_cube(dtype):
    rng = np.random.default_rng(23)
    shape = (9, 6, 10)
    d = rng.normal(0.0, 1.0, shape)
    d[3:6, 1:5, 2:8] += 4.0
    d = d.astype(dtype)
    d[rng.random(shape) < 0.04] = np.nan
    d[:, 0, 0] = np.nan                      # a spaxel without a sample: its noise is NaN, no threshold includes it
    d[2, 3, 3], d[7, 4, 1] = np.inf, -np.inf
    return d, rng.random(shape[1:]) < 0.6


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_signal_masks_never_bring_the_cube_to_the_host(gpu, monkeypatch, dtype):
    d, region = _signal_cube(dtype)
    if dtype is np.float32:
        cube = SpectralCube.from_device(DeviceArray.from_numpy(d, gpu), header=HDR)
    else:
        cube = SpectralCube(d, header=HDR)               # float64 samples: every operator below runs on the float64 path
    rms = cube.mad_std(axis=0)
    smooth, idioms = _idioms(cube, rms, region)
    sm = (smooth._device_data64() if dtype is np.float64 else smooth._device_data()).get()
    assert sm.dtype == dtype

    def no_host(self):
        raise AssertionError("the cube was copied to the host to evaluate a mask")

    monkeypatch.setattr(SpectralCube, "_host_data", no_host)
    monkeypatch.setattr(cube_module._WideView, "_host_data", no_host)
    for name, (make, restate) in idioms.items():
        with np.errstate(invalid="ignore"):
            inc = np.array(restate(d, sm))
        assert 0 < inc.sum() < inc.size, name
        got = cube.with_mask(make())
        ref = SpectralCube(d, header=HDR).with_mask(inc)
        g = got.get_mask_array()
        assert g.dtype == bool and g.shape == d.shape and np.array_equal(g, inc), name
        assert np.array_equal(ref.get_mask_array(), inc)
        e0 = np.asarray(ref.moment0())
        assert_close(got.moment0(), e0, rtol=1e-8, atol=1e-9 * np.nanmax(np.abs(e0)), what=name + " moment0")
        em = np.asarray(ref.median(axis=0))
        assert_close(got.median(axis=0), em, rtol=1e-8, atol=1e-9 * np.nanmax(np.abs(em)), what=name + " median")
        gs, es = got.statistics(), ref.statistics()
        assert sorted(gs) == sorted(es)
        assert gs["npts"] == es["npts"] == int((inc & ~np.isnan(d)).sum()), name
        for k in es:
            assert_close(gs[k], es[k], rtol=1e-8, atol=1e-9 * abs(es[k]) if np.isfinite(es[k]) else 0.0, what="%s statistics %s" % (name, k))
    assert SpectralCube.from_device(DeviceArray.from_numpy(d.astype(np.float32), gpu), header=HDR).get_mask_array().all()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_include_maps_of_the_reference(gpu, dtype):
    G = golden("mask_eval.npz")
    d, rms, region = G["data"].astype(dtype), G["rms"], G["region"]
    hdr = parse_header(str(G["header"]))
    if dtype is np.float32:
        cube = SpectralCube.from_device(DeviceArray.from_numpy(d, gpu), header=hdr)
        other = SpectralCube.from_device(DeviceArray.from_numpy(G["smooth"], gpu), header=hdr)
    else:
        cube, other = SpectralCube(d, header=hdr), SpectralCube(G["smooth"].astype(dtype), header=hdr)

    def ne(c, v):
        return M.LazyComparisonMask(operator.ne, v, cube=c)

    def eq(c, v):
        return M.LazyComparisonMask(operator.eq, v, cube=c)

    idioms = {
        "sig": lambda: cube > 3 * rms,
        "wing": lambda: (cube > 5 * rms) | (cube < -5 * rms),
        "off": lambda: ~(cube > 3 * rms),
        "dil": lambda: other > 2 * rms,
        "roi": lambda: region,
        "ge_or_eq": lambda: (cube >= 3 * rms) ^ eq(cube, -5 * rms),
        "ne": lambda: ne(cube, 3 * rms),
    }
    assert sorted(idioms) == [str(s) for s in G["names"]]
    for name, make in idioms.items():
        got = cube.with_mask(make()).get_mask_array()
        want = np.unpackbits(G["include_" + name])[:d.size].reshape(d.shape).astype(bool)
        assert np.array_equal(got, want), "%s: %d voxels differ" % (name, (got != want).sum())
