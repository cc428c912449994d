"""The cube and mask checks every two-width operator shares (csrc/spc_common.h), driven through the C ABI on a host-backed
view: each malformed input is refused with SPC_ERR_INVALID and names its fault, before any kernel could be launched.
No GPU is needed: every call here fails its validation, and validation comes before the first HIP call."""
import ctypes as C

import pytest

from spectral_cube_amd import _lib

NZ = NY = NX = 4
F32, F64 = "_f32", "_f64"


def _buffers(suffix):
    elem = C.c_float if suffix == F32 else C.c_double
    return (elem * 64)(), (elem * 64)()


def _entry(name, suffix):
    """name + suffix -> call(cube_ptr, mask_ptr, **fault): every other argument valid unless `fault` names one to break"""
    lib = _lib.load()
    fn = getattr(lib, name + suffix) if name not in ("spc_moments_f64", "spc_stats_axis_f64") else getattr(lib, name)
    _, out = _buffers(suffix)
    keep = [out]
    o = C.c_void_p(C.addressof(out))
    three = C.c_int64 * 3
    start, step = three(0, 0, 0), three(1, 1, 1)
    idx, shift, box = (C.c_int32 * 1)(0), (C.c_double * 1)(0.0), (C.c_int64 * 6)()
    ws = (C.c_char * 4096)()
    keep += [start, step, idx, shift, box, ws]
    p = lambda a: C.c_void_p(C.addressof(a))

    def call(cube, mask, null=None):
        dst = None if null == "out" else o
        if name == "spc_downsample":
            return fn(0, None, cube, mask, 0, 0.0, 0, 2, 0, _lib.DS_MAX, dst, 0, 0, None)
        if name == "spc_subcube":
            return fn(0, None, cube, mask, 0, None if null == "start" else start, step, 2, 2, 2, dst, 0, 0, None, 0, 0.0)
        if name == "spc_mask_bbox":
            return fn(0, None, cube, mask, 0, None if null == "box" else p(box))
        if name == "spc_rank_filter_axis0":
            return fn(0, None, cube, mask, 0, 0.0, 3, 1, 0, 0.0, dst, 0, 0)
        if name == "spc_rank_filter_plane":
            return fn(0, None, cube, mask, 0, 0.0, 3, 3, 4, 0, 0.0, dst, 0, 0)
        if name == "spc_stack_shift":
            return fn(0, None, cube, mask, 0, 0.0, p(idx), p(shift), 1, 0, 0, dst, p(ws), 4096)
        if name == "spc_stack_sum":
            return fn(0, None, cube, mask, 0, 0.0, None if null == "idx" else p(idx), p(shift), 1, 0, 0, o, o, o, p(ws), 4096)
        if name == "spc_moments_f64":
            outs = _lib.SpcMomentOutputs64()
            outs.d_m0 = C.addressof(out)
            return fn(0, None, cube, mask, o, 1.0, 0.0, C.byref(outs))
        assert name == "spc_stats_axis_f64"
        outs = _lib.SpcStatsOutputs()
        outs.d_count = C.addressof(out)
        return fn(0, None, cube, mask, 0, C.byref(outs))
    call.keep = keep
    return call


def _cube(suffix, **over):
    buf, _ = _buffers(suffix)
    c = _lib.SpcCube()
    c.d_data = C.addressof(buf)
    c.nz, c.ny, c.nx, c.row_stride, c.plane_stride = NZ, NY, NX, NX, NY * NX
    for k, v in over.items():
        setattr(c, k, v)
    c.keep = buf
    return c


def _mask(suffix, flags, d_array=None):
    m = (_lib.SpcMask if suffix == F32 else _lib.SpcMask64)()
    m.flags, m.thr_lo, m.thr_hi, m.d_array = flags, 0.0, 1.0, d_array
    return m


# ---- the malformed inputs: case -> (cube fields to override or None for a NULL cube, mask or None, word of the message)
COMMON = {
    "null cube": (None, None, b"cube pointer is NULL"),
    "null d_data": ({"d_data": None}, None, b"cube pointer is NULL"),
    "zero nz": ({"nz": 0}, None, b"shape must be positive"),
    "zero ny": ({"ny": 0}, None, b"shape must be positive"),
    "zero nx": ({"nx": 0}, None, b"shape must be positive"),
    "unknown mask flags": ({}, (0x40, None), b"unknown mask flags 0x40"),
    "mask array without d_array": ({}, (_lib.MASK_ARRAY, None), b"d_array is NULL"),
}
# what spc_check_cube says of bad strides; a view with the first two axes exchanged (row_stride 16, plane_stride 4) is refused
ORDERED = dict(COMMON, **{
    "row_stride < nx": ({"row_stride": NX - 1}, None, b"row_stride 3 < nx 4"),
    "plane_stride one short": ({"plane_stride": NY * NX - 1}, None, b"plane_stride too small"),
    "axes exchanged": ({"row_stride": NZ * NX, "plane_stride": NX}, None, b"plane_stride too small"),
})
# the float64 rank filter and stack refuse the same views, two of them in the words of spc_check_cube_any_order
ORDERED_WIDE_WORDS = dict(ORDERED, **{
    "row_stride < nx": ({"row_stride": NX - 1}, None, b"row / plane stride smaller than nx"),
    "plane_stride one short": ({"plane_stride": NY * NX - 1}, None, b"overlapping rows and planes"),
})
NZ_BOUND = {"nz": 1 << 21}
MOMENT_BOUND = b"nz too large for the float64 moment kernel (2097152)"

# entry point -> (its table, {case: (cube fields, argument to NULL, word)} beyond the table)
ENTRIES = {
    ("spc_downsample", F32): (ORDERED, {}),
    ("spc_downsample", F64): (ORDERED, {"nz = 2^21": (NZ_BOUND, None, MOMENT_BOUND)}),
    ("spc_subcube", F32): (ORDERED, {}),
    ("spc_subcube", F64): (ORDERED, {"nz = 2^21": (NZ_BOUND, "start", b"start / step is NULL")}),
    ("spc_mask_bbox", F32): (ORDERED, {}),
    ("spc_mask_bbox", F64): (ORDERED, {"nz = 2^21": (NZ_BOUND, "box", b"d_box is NULL")}),
    ("spc_rank_filter_axis0", F32): (ORDERED, {}),
    ("spc_rank_filter_axis0", F64): (ORDERED_WIDE_WORDS, {"nz = 2^21": (NZ_BOUND, "out", b"d_out is NULL")}),
    ("spc_rank_filter_plane", F32): (ORDERED, {}),
    ("spc_rank_filter_plane", F64): (ORDERED_WIDE_WORDS, {"nz = 2^21": (NZ_BOUND, "out", b"d_out is NULL")}),
    ("spc_stack_shift", F32): (ORDERED, {}),
    ("spc_stack_shift", F64): (ORDERED_WIDE_WORDS, {"nz = 2^21": (NZ_BOUND, "out", b"d_out is NULL")}),
    ("spc_stack_sum", F32): (ORDERED, {}),
    ("spc_stack_sum", F64): (ORDERED_WIDE_WORDS, {"nz = 2^21": (NZ_BOUND, "idx", b"d_idx / d_shift is NULL")}),
    ("spc_moments_f64", F64): (ORDERED, {"nz = 2^21": (NZ_BOUND, None, MOMENT_BOUND)}),
    ("spc_stats_axis_f64", F64): (ORDERED, {"nz = 2^21": (NZ_BOUND, None, MOMENT_BOUND)}),
}


def _cases():
    for (name, suffix), (table, extra) in ENTRIES.items():
        for case, (fields, mask, word) in table.items():
            yield pytest.param(name, suffix, fields, mask, None, word, id="%s-%s" % (name if name.endswith(F64) else name + suffix, case))
        for case, (fields, null, word) in extra.items():
            yield pytest.param(name, suffix, fields, None, null, word, id="%s-%s" % (name if name.endswith(F64) else name + suffix, case))


@pytest.mark.parametrize("name,suffix,fields,mask,null,word", list(_cases()))
def test_malformed_input_is_refused_before_any_launch(name, suffix, fields, mask, null, word):
    lib = _lib.load()
    call = _entry(name, suffix)
    cube = None if fields is None else _cube(suffix, **fields)
    m = None if mask is None else _mask(suffix, *mask)
    rc = call(None if cube is None else C.byref(cube), None if m is None else C.byref(m), null=null)
    assert rc == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (rc, word, lib.spc_last_error())


def test_float32_entries_have_no_nz_bound_of_the_float64_moment_kernel():
    """nz = 2^21 passes every float32 cube check too: the calls fail on the later fault chosen above, never on nz"""
    lib = _lib.load()
    for name, suffix in ENTRIES:
        if suffix == F64:
            continue
        null, word = {"spc_downsample": ("out", b"d_out is NULL"), "spc_subcube": ("start", b"start / step is NULL"),
                      "spc_mask_bbox": ("box", b"d_box is NULL"), "spc_rank_filter_axis0": ("out", b"d_out is NULL"),
                      "spc_rank_filter_plane": ("out", b"d_out is NULL"), "spc_stack_shift": ("out", b"d_out is NULL"),
                      "spc_stack_sum": ("idx", b"d_idx / d_shift is NULL")}[name]
        cube = _cube(suffix, **NZ_BOUND)
        rc = _entry(name, suffix)(C.byref(cube), None, null=null)
        assert rc == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (name, lib.spc_last_error())
