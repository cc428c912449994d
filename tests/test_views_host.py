"""What reaches the C ABI when a cube, a mask or an output is a strided, offset or misaligned view (tests/views.py): for
every ``ops`` wrapper that takes one, the struct and the arguments handed to ``_lib.call`` carry exactly the layout's
pointer and strides - the cube's, the mask's and the output's separately.  No GPU: ``_lib.call`` is recorded, the arrays
are stand-ins with made-up pointers.

Two defects this pins: a contiguous mask array next to a strided cube went out with strides 0 ("the cube's" on the C
side: the kernel would walk the mask past its end), and eight ``out=`` call sites wrote a strided output as if it were
contiguous."""
import ctypes as C
import types

import numpy as np
import pytest

import views as V
from spectral_cube_amd import _lib, ops
from spectral_cube_amd.device import DeviceArray

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)


class _Arr(DeviceArray):
    """a DeviceArray without a device: a made-up 256-byte aligned pointer, no transfers; rows() / planes() / swap01() are
    the real ones"""
    _next = [1 << 32]

    def __init__(self, shape, dtype, device=0, ptr=None, owner=None):
        if ptr is None:
            n = int(np.prod(np.atleast_1d(shape), dtype=np.int64)) * np.dtype(dtype).itemsize
            ptr = _Arr._next[0]
            _Arr._next[0] += (n + 4096 + 255) // 256 * 256
        super().__init__(shape, dtype, device, ptr=ptr, owner=owner)

    def upload(self, arr, stream=None):
        pass

    def get(self, stream=None):
        return np.zeros(self.shape, self.dtype)


@pytest.fixture
def recorded(monkeypatch):
    import spectral_cube_amd.device as D
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "DeviceArray", _Arr)
    monkeypatch.setattr(D, "DeviceArray", _Arr)
    return calls


def _view(lay, dtype):
    parent = _Arr((V.parent_size(lay),), dtype)
    return V.device_view(lay, parent, cls=_Arr), parent


def _expect_strides(lay):
    return lay.row_stride, lay.plane_stride


# ---- the layouts themselves -----------------------------------------------------------------------------------------
ALL_LAYOUTS = V.CUBE_LAYOUTS + ("swap01",)


@pytest.mark.parametrize("name", ALL_LAYOUTS)
def test_layout_fits_its_parent_and_passes_the_cube_check(name):
    lay = V.layout(name)
    assert V.fits_parent(lay)
    assert V.check_cube_conditions(lay, any_order=True) is None
    # swap01 is the one layout spc_check_cube refuses (its rows lie a plane apart)
    assert (V.check_cube_conditions(lay) is None) == (name != "swap01")
    for mname in V.MASK_LAYOUTS:
        if name == "swap01" and mname == "mask_phase":
            continue
        ml = V.mask_layout(mname, lay)
        assert ml.shape == lay.shape and V.fits_parent(ml) and V.check_cube_conditions(ml, any_order=True) is None
        if mname == "mask_phase":
            assert ml.x0 % 4 != lay.x0 % 4
    for oname in V.OUT_LAYOUTS:
        ol = V.layout(oname, (20, 9, 132))
        assert V.fits_parent(ol) and V.check_cube_conditions(ol) is None


def test_layout_alignment_is_what_its_name_says():
    for dtype in (F32, F64):
        per16 = 16 // dtype.itemsize
        lay = {n: V.layout(n) for n in V.CUBE_LAYOUTS}
        for n in ("contig", "rows", "planes_of_rows", "xwin_aligned"):
            assert lay[n].offset % per16 == 0 and lay[n].row_stride % per16 == 0 and lay[n].plane_stride % per16 == 0, n
        assert lay["xwin_aligned"].row_stride != lay["xwin_aligned"].shape[2]
        assert lay["xwin_off1"].offset % 4 == 1 and lay["xwin_off1"].shape[2] % 4 == 0 and lay["xwin_off1"].row_stride % 4 == 0
        assert lay["xwin_oddstride"].row_stride % 4 == 3 and lay["xwin_oddstride"].plane_stride % 2 == 1
        assert lay["xwin_tail"].shape[2] % 4 == 3 and lay["xwin_tail"].offset % 4 == 3


def test_place_extract_outside_round_trip():
    d, m = V.data(np.float32)
    for name in ALL_LAYOUTS:
        lay = V.layout(name)
        x = V.crop(d, lay)
        flat = V.place(lay, x, V.CUBE_POISON[F32])
        assert np.array_equal(V.extract(lay, flat), x, equal_nan=True)
        rest = V.outside(lay, flat)
        assert rest.size == V.parent_size(lay) - x.size and (rest == np.float32(1e30)).all()


def test_device_view_is_what_rows_and_planes_build():
    """the generator's views carry the pointer and strides DeviceArray.rows() / planes() / swap01() give"""
    for dtype in (F32, F64):
        lay = V.layout("planes_of_rows")
        v, parent = _view(lay, dtype)
        import spectral_cube_amd.device as D
        real = D.DeviceArray
        D.DeviceArray = _Arr
        try:
            cube = _Arr(lay.parent_shape, dtype, ptr=parent.ptr)
            w = cube.rows(V.Y0, V.Y0 + lay.shape[1]).planes(V.Z0, V.Z0 + lay.shape[0])
            a, pa = _view(V.layout("xwin_aligned"), dtype)
            s = a.swap01()
        finally:
            D.DeviceArray = real
        assert (w.ptr, w.shape, w.row_stride, w.plane_stride) == (v.ptr, v.shape, v.row_stride, v.plane_stride)
        sl = V.layout("swap01")
        assert (s.ptr - pa.ptr, s.shape, s.row_stride, s.plane_stride) == (sl.offset * dtype.itemsize, sl.shape, sl.row_stride, sl.plane_stride)


# ---- the wrappers ---------------------------------------------------------------------------------------------------
def _cen(n):
    return _Arr((n,), np.float64)


def _map(shape, dtype=np.float64):
    return _Arr(shape, dtype)


_K9 = np.hanning(11)[1:-1]
_K2SEP = np.outer(_K9, _K9)
_K2GEN = _K2SEP + np.linspace(0, 1e-3, 81).reshape(9, 9)


def _same(c):
    return tuple(c.shape)


def _lerp_plan(nz):
    return np.arange(nz - 1, dtype=np.int32), np.full(nz - 1, 0.5), np.ones(nz - 1)


def _xy(c):
    ny, nx = c.shape[1:]
    return _map((ny, nx)), _map((ny, nx))


def _prog(slots):
    p = types.SimpleNamespace(slots=list(slots), operands=[], instr=[(_lib.MOP_CMP, i, _lib.CMP_GT, -1, 0.0) for i in range(len(slots))])
    p.instr += [(_lib.MOP_AND, 0, 0, -1, 0.0)] * (len(slots) - 1)
    return p


# name -> (sample types, takes a mask, shape of out= (None: no out=) and its dtype, call(cube, mask, out))
W = {}


def _w(name, dtypes, mask, out, fn):
    W[name] = (dtypes, mask, out, fn)


_BOTH, _ONLY32, _ONLY64 = (F32, F64), (F32,), (F64,)
_w("moments", _ONLY32, True, None, lambda c, m, o: ops.moments(c, _cen(c.shape[0]), mask=m, want=("m0", "m1", "m2", "argmax")))
_w("moments_f64", _ONLY64, True, None, lambda c, m, o: ops.moments_f64(c, _cen(c.shape[0]), mask=m))
_w("moment_order", _ONLY32, True, None, lambda c, m, o: ops.moment_order(c, _cen(c.shape[0]), 3, _map(c.shape[1:]), _map(c.shape[1:]), mask=m))
_w("moment_order_f64", _ONLY64, True, None, lambda c, m, o: ops.moment_order_f64(c, _cen(c.shape[0]), 3, _map(c.shape[1:]), _map(c.shape[1:]), mask=m))
_w("sigma_clip_axis0", _ONLY32, True, None, lambda c, m, o: ops.sigma_clip_axis0(c, mask=m))
_w("sigma_clip_axis0_f64", _ONLY64, True, None, lambda c, m, o: ops.sigma_clip_axis0_f64(c, mask=m))
_w("narrow_f64", _ONLY64, False, (_same, F32), lambda c, m, o: ops.narrow_f64(c, out=o))
_w("argextrema_axis", _ONLY32, True, None, lambda c, m, o: [ops.argextrema_axis(c, a, mask=m) for a in (1, 2)])
_w("moments_spatial", _ONLY32, True, None, lambda c, m, o: [ops.moments_spatial(c, _map(c.shape[1:]), a, 1.0, mask=m) for a in (1, 2)])
_w("moment_order_spatial", _ONLY32, True, None,
   lambda c, m, o: ops.moment_order_spatial(c, _map(c.shape[1:]), 2, 3, _map(c.shape[:2]), mask=m))
_w("spectral_conv", _BOTH, True, (_same, None), lambda c, m, o: ops.spectral_conv(c, _K9, mask=m, out=o))
_w("spectral_conv_moments", _ONLY32, True, None, lambda c, m, o: ops.spectral_conv_moments(c, _K9, _cen(c.shape[0]), mask=m))
_w("downsample", _BOTH, True, (lambda c: ops.downsample_shape(c.shape, 0, 3, False), None),
   lambda c, m, o: ops.downsample(c, 0, 3, mask=m, out=o, out_mask=None if o is None else _twin(o)))
_w("rank_filter_axis0", _BOTH, True, (_same, None), lambda c, m, o: ops.rank_filter_axis0(c, 5, 2, mask=m, out=o))
_w("rank_filter_plane", _BOTH, True, (_same, None), lambda c, m, o: ops.rank_filter_plane(c, 3, 3, 4, mask=m, out=o))
_w("stack_shift", _BOTH, True, None, lambda c, m, o: ops.stack_shift(c, [0, 5], [0.5, -1.25], mask=m))
_w("stack_sum", _BOTH, True, None, lambda c, m, o: ops.stack_sum(c, [0, 5], [0.5, -1.25], mask=m))
_w("stack_cube", _BOTH, True, None,
   lambda c, m, o: ops.stack_cube(c, np.zeros((2, 4), np.int32), np.zeros((2, 4)), np.ones((2, 4)), [0, 0], mask=m))
_w("subcube", _BOTH, True, (_same, None),
   lambda c, m, o: ops.subcube(c, (0, 0, 0), (1, 1, 1), c.shape, mask=m, out=o, out_mask=None if o is None else _twin(o)))
_w("arith", _BOTH, True, (_same, None), lambda c, m, o: ops.arith(c, [("add", 1.0, False)], mask=m, out=o))
_w("mask_bbox", _BOTH, True, None, lambda c, m, o: ops.mask_bbox(c, mask=m))
_w("spatial_conv_sep", _BOTH, True, (_same, None), lambda c, m, o: ops.spatial_conv(c, _K2SEP, mask=m, out=o))
_w("spatial_conv_2d", _BOTH, True, (_same, None), lambda c, m, o: ops.spatial_conv(c, _K2GEN, mask=m, out=o))
_w("spatial_conv_mfma", _ONLY32, True, None, lambda c, m, o: ops.spatial_conv_mfma(c, _K2SEP, mask=m, want_m0=True))
_w("spatial_conv_mfma_moments", _ONLY32, True, None, lambda c, m, o: ops.spatial_conv_mfma_moments(c, _K2SEP, _cen(c.shape[0]), mask=m))
_w("spectral_lerp", _BOTH, True, (lambda c: (c.shape[0] - 1,) + tuple(c.shape[1:]), None),
   lambda c, m, o: ops.spectral_lerp(c, *_lerp_plan(c.shape[0]), mask=m, out=o))
_w("resample_bilinear", _BOTH, True, (_same, None), lambda c, m, o: ops.resample_bilinear(c, *_xy(c), mask=m, out=o))
_w("resample_bilinear_lerp", _ONLY32, True, None, lambda c, m, o: ops.resample_bilinear_lerp(c, *_xy(c), *_lerp_plan(c.shape[0]), mask=m))
_w("resample_spline", _ONLY32, False, None, lambda c, m, o: ops.resample_spline(c, *_xy(c), 3))
_w("stats_global", _BOTH, True, None, lambda c, m, o: ops.stats_global(c, mask=m))
_w("stats_planes", _ONLY32, True, None, lambda c, m, o: ops.stats_planes(c, mask=m))
_w("stats_axis", _BOTH, True, None, lambda c, m, o: [ops.stats_axis(c, a, mask=m, want=ops.STAT_KEYS + ("m2",)) for a in (0, 1, 2)])
_w("stats_dev_axis", _BOTH, True, None, lambda c, m, o: [ops.stats_dev_axis(c, a, 0.5, mask=m) for a in (0, 1, 2)])
_w("percentile_axis0", _BOTH, True, None, lambda c, m, o: ops.percentile_axis0(c, 50.0, mask=m))
_w("percentile_axis2", _ONLY32, True, None, lambda c, m, o: ops.percentile_axis2(c, 50.0, mask=m))
_w("percentile_global", _ONLY32, True, None, lambda c, m, o: ops.percentile_global(c, 50.0, mask=m))
_w("key_histogram", _ONLY32, True, None, lambda c, m, o: (ops.key_histogram(c, 0, 0, 24, mask=m), ops.key_next(c, 0, mask=m)))
_w("fill_masked", _ONLY32, True, (_same, F32), lambda c, m, o: ops.fill_masked(c, m, 0.0, out=o))
_w("fill_masked_transposed", _ONLY32, True, None, lambda c, m, o: ops.fill_masked_transposed(c, m, 0.0))
_w("mask_include", _BOTH, True, None, lambda c, m, o: ops.mask_include(c, m))

# the entries that call spc_check_cube_any_order (percentile_axis0 both widths, spc_percentile_axis2_f32, the fused
# spc_sigma_clip_axis0_f32): they alone meet swap01
ANY_ORDER = ("percentile_axis0", "percentile_axis2", "sigma_clip_axis0")


def _twin(o):
    """the uint8 output that shares *o*'s geometry (downsample / subcube want the two outputs to have the same strides)"""
    t = _Arr(o.shape, np.uint8, ptr=o.ptr + (1 << 24))
    for k in ("row_stride", "plane_stride", "_is_view"):
        if hasattr(o, k):
            setattr(t, k, getattr(o, k))
    return t


def _combos(name):
    """(cube layout, mask layout, output layout) as the GPU matrix walks them"""
    dtypes, takes_mask, out, _ = W[name]
    cube_layouts = V.CUBE_LAYOUTS + (("swap01",) if name in ANY_ORDER else ())
    out_layouts = V.OUT_LAYOUTS if out is not None else (None,)
    combos = [(c, "mask_same", None) for c in cube_layouts]
    if takes_mask:
        combos += [(c, m, None) for c in ("xwin_aligned", "xwin_off1") + (("swap01",) if name in ANY_ORDER else ())
                   for m in V.MASK_LAYOUTS if not (c == "swap01" and m == "mask_phase")]
    combos += [("xwin_aligned", "mask_same", o) for o in out_layouts if o is not None]
    return combos


def _structs(args, kind):
    return [a._obj for a in args if hasattr(a, "_obj") and isinstance(a._obj, kind)]


def _check_cube_struct(c, view, parent, lay, what):
    it = parent.dtype.itemsize
    assert c.d_data == parent.ptr + lay.offset * it == view.ptr, what
    assert (c.nz, c.ny, c.nx) == lay.shape, what
    assert (c.row_stride, c.plane_stride) == _expect_strides(lay), (what, c.row_stride, c.plane_stride)


def _check_mask_struct(m, mparent, mlay, what):
    assert m.flags & _lib.MASK_ARRAY, what
    assert m.d_array == mparent.ptr + mlay.offset, what
    # never 0 with an array present: 0 means "the cube's strides" on the C side
    assert (m.row_stride, m.plane_stride) == _expect_strides(mlay), (what, m.row_stride, m.plane_stride)


def _check_out_args(args, out, olay, what):
    at = [i for i, a in enumerate(args) if isinstance(a, C.c_void_p) and a.value == out.ptr]
    assert len(at) == 1, (what, "the output pointer must reach the call once")
    got = tuple(int(v) for v in args[at[0] + 1:at[0] + 3])
    want = _expect_strides(olay)
    assert got == want or (olay.name == "contig" and got == (0, 0)), (what, "output strides", got, want)


@pytest.mark.parametrize("name", sorted(W))
def test_wrapper_hands_the_layout_to_the_library(recorded, name):
    dtypes, takes_mask, out_spec, fn = W[name]
    for dtype in dtypes:
        for cname, mname, oname in _combos(name):
            what = "%s %s cube %s mask %s out %s" % (name, dtype.name, cname, mname, oname)
            lay = V.layout(cname)
            cube, parent = _view(lay, dtype)
            mask = mlay = mparent = None
            if takes_mask:
                mlay = V.mask_layout(mname, lay)
                marr, mparent = _view(mlay, np.uint8)
                mask = ops.MaskSpec(_lib.MASK_ARRAY | _lib.MASK_FINITE, 0.0, 0.0, marr)
            out = olay = None
            if oname is not None:
                shape_of, odtype = out_spec
                olay = V.layout(oname, shape_of(cube))
                out, _ = _view(olay, odtype or dtype)
            del recorded[:]
            fn(cube, mask, out)
            seen_cube = seen_out = 0
            for cname_, args in recorded:
                for c in _structs(args, _lib.SpcCube):
                    _check_cube_struct(c, cube, parent, lay, what + " " + cname_)
                    seen_cube += 1
                    if takes_mask:
                        ms = _structs(args, (_lib.SpcMask, _lib.SpcMask64))
                        assert len(ms) == 1 and isinstance(ms[0], _lib.SpcMask64 if dtype == F64 else _lib.SpcMask), what
                        _check_mask_struct(ms[0], mparent, mlay, what + " " + cname_)
                    if out is not None:
                        _check_out_args(args, out, olay, what + " " + cname_)
                        seen_out += 1
            assert seen_cube >= 1 and (out is None or seen_out == 1), what


@pytest.mark.parametrize("name", sorted(n for n in W if W[n][2] is not None))
def test_wrapper_checks_a_given_output(recorded, name):
    """a preallocated output of another shape or dtype is refused before anything reaches the library"""
    dtypes, takes_mask, (shape_of, odtype), fn = W[name]
    dtype = dtypes[0]
    cube, _ = _view(V.layout("contig"), dtype)
    good = shape_of(cube)
    for shape, dt in (((good[0] + 1,) + tuple(good[1:]), odtype or dtype), (good, np.int16)):
        del recorded[:]
        with pytest.raises((ValueError, TypeError)):
            fn(cube, None, _Arr(shape, dt))
        assert not [c for c in recorded if c[0] not in ("spc_malloc",)], name


def test_mosaic_sources_carry_their_own_strides(recorded):
    for dtype in (F32, F64):
        lays = [V.layout("xwin_off1"), V.layout("xwin_oddstride")]
        mlays = [V.mask_layout("mask_contig", lays[0]), V.mask_layout("mask_phase", lays[1])]
        views = [_view(l, dtype) for l in lays]
        mviews = [_view(l, np.uint8) for l in mlays]
        maps = [(_map((7, 12)), _map((7, 12))) for _ in lays]
        masks = [ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, mv[0]) for mv in mviews]
        del recorded[:]
        ops.mosaic([v[0] for v in views], maps, masks, [np.nan, 0.0], 1)
        (name, args), = [c for c in recorded if c[0].startswith("spc_mosaic")]
        tab = args[3]
        for s in range(2):
            _check_cube_struct(tab[s].cube, views[s][0], views[s][1], lays[s], "mosaic source %d" % s)
            _check_mask_struct(tab[s].mask, mviews[s][1], mlays[s], "mosaic source %d" % s)
        out, _ = _view(V.layout("out_xwin_aligned", (21, 7, 12)), dtype)
        with pytest.raises(ValueError, match="contiguous"):          # the mosaic's output is contiguous by contract
            ops.mosaic([v[0] for v in views], maps, masks, [np.nan, 0.0], 1, out=out)


# the wrappers whose entry writes one contiguous block: name -> (sample type, output shape of a cube, call(cube, out))
_STACK = (np.zeros((2, 4), np.int32), np.zeros((2, 4)), np.ones((2, 4)), [0, 0])
CONTIGUOUS_OUT = {
    "stack_cube": (F32, lambda c: (4,) + tuple(c.shape[1:]), lambda c, o: ops.stack_cube(c, *_STACK, out=o)),
    "stack_cube_f64": (F64, lambda c: (4,) + tuple(c.shape[1:]), lambda c, o: ops.stack_cube(c, *_STACK, out=o)),
    "spatial_conv_mfma": (F32, _same, lambda c, o: ops.spatial_conv_mfma(c, _K2SEP, out=o)),
    "spatial_conv_mfma_moments": (F32, _same, lambda c, o: ops.spatial_conv_mfma_moments(c, _K2SEP, _cen(c.shape[0]), out=o, want_cube=True)),
    "resample_spline": (F32, _same, lambda c, o: ops.resample_spline(c, *_xy(c), 3, out=o)),
    "resample_bilinear_lerp": (F32, lambda c: (c.shape[0] - 1,) + tuple(c.shape[1:]),
                               lambda c, o: ops.resample_bilinear_lerp(c, *_xy(c), *_lerp_plan(c.shape[0]), out=o)),
}


@pytest.mark.parametrize("name", sorted(CONTIGUOUS_OUT))
def test_contiguous_only_outputs_refuse_views_and_check_what_they_are_given(recorded, name):
    """stack_cube's entry takes no output strides, the matrix-core stencils are handed 0, 0, the spline resampler offsets the
    output pointer by whole contiguous planes, the lerp resampler addresses it from its last plane: a strided view, another
    shape or another dtype is refused before anything reaches the library; a contiguous output reaches it as it is"""
    dtype, shape_of, fn = CONTIGUOUS_OUT[name]
    cube, _ = _view(V.layout("xwin_aligned"), dtype)
    shape = shape_of(cube)
    for oname in V.OUT_LAYOUTS[1:]:
        out, _ = _view(V.layout(oname, shape), dtype)
        del recorded[:]
        with pytest.raises(ValueError, match="contiguous"):
            fn(cube, out)
        assert not [c for c in recorded if c[0] not in ("spc_malloc",)], (name, oname)
    for bad_shape, bad_dtype in (((shape[0] + 1,) + tuple(shape[1:]), dtype), (shape, np.int16)):
        del recorded[:]
        with pytest.raises((ValueError, TypeError)):
            fn(cube, _Arr(bad_shape, bad_dtype))
        assert not [c for c in recorded if c[0] not in ("spc_malloc",)], name
    out = _Arr(shape, dtype)
    del recorded[:]
    fn(cube, out)
    hits = [a for n, args in recorded for a in args if isinstance(a, C.c_void_p) and a.value == out.ptr]
    assert len(hits) >= 1, name


def test_rows_of_an_x_window_start_whole_row_strides_on(recorded):
    """rows() / planes() / MaskSpec.rows() compose with a window in x of a wider parent: y0 rows on is y0 * row_stride"""
    for dtype in (F32, np.dtype(np.uint8)):
        lay = V.layout("xwin_off1")
        v, parent = _view(lay, dtype)
        r = v.rows(2, 7).planes(3, 9)
        it = dtype.itemsize
        assert r.ptr == parent.ptr + (lay.offset + 3 * lay.plane_stride + 2 * lay.row_stride) * it
        assert (r.shape, r.row_stride, r.plane_stride) == ((6, 5, lay.shape[2]), lay.row_stride, lay.plane_stride)
    m = ops.MaskSpec(_lib.MASK_ARRAY, array=v).rows(2, 7).to_c()
    assert m.d_array == parent.ptr + lay.offset + 2 * lay.row_stride and (m.row_stride, m.plane_stride) == (lay.row_stride, lay.plane_stride)


def test_resample_bilinear_lerp_output_is_contiguous_by_contract(recorded):
    """its output is addressed from its last plane for a descending plan: a view is refused before anything is launched"""
    cube, _ = _view(V.layout("xwin_aligned"), F32)
    out, _ = _view(V.layout("out_xwin_aligned", (20, 9, 132)), F32)
    del recorded[:]
    with pytest.raises(ValueError, match="contiguous"):
        ops.resample_bilinear_lerp(cube, *_xy(cube), *_lerp_plan(21), out=out)
    assert not [c for c in recorded if c[0].startswith("spc_resample")]


def test_arith_operand_and_mask_eval_slots_carry_their_own_strides(recorded):
    for dtype in (F32, F64):
        lay, olay = V.layout("xwin_aligned"), V.layout("xwin_oddstride")
        cube, parent = _view(lay, dtype)
        operand, oparent = _view(olay, dtype)
        del recorded[:]
        ops.arith(cube, [("mul", operand, False)])
        (name, args), = [c for c in recorded if c[0].startswith("spc_arith")]
        _check_cube_struct(_structs(args, _lib.SpcCube)[0], cube, parent, lay, "arith cube")
        step = _structs(args, _lib.SpcArithProgram)[0].steps[0]
        assert step.d_data == oparent.ptr + olay.offset * dtype.itemsize and not step.is_scalar
        assert (step.stride_z, step.stride_y, step.stride_x) == (olay.plane_stride, olay.row_stride, 1)

        slots = [_view(V.layout(n), dtype) for n in ("xwin_off1", "rows", "contig")]
        out, _ = _view(V.layout("out_xwin_off1"), np.uint8)
        del recorded[:]
        ops.mask_eval(_prog([s[0] for s in slots]), V.BASE, 0, dtype, out=out)
        (name, args), = [c for c in recorded if c[0].startswith("spc_mask_eval")]
        p = _structs(args, _lib.SpcMaskProgram)[0]
        for i, (n, (v, par)) in enumerate(zip(("xwin_off1", "rows", "contig"), slots)):
            l = V.layout(n)
            assert p.slots[i].d_data == par.ptr + l.offset * dtype.itemsize
            got = (p.slots[i].row_stride, p.slots[i].plane_stride)
            assert got == _expect_strides(l) or (n == "contig" and got == (0, 0)), (n, got)
        _check_out_args(args, out, V.layout("out_xwin_off1"), "mask_eval out")


def test_every_cube_wrapper_is_in_the_table():
    """an ``ops`` function with a ``cube`` parameter that this module does not walk is a gap"""
    import inspect
    covered = set(W) | {"spatial_conv", "mosaic", "mask_eval", "key_next", "scale_inplace", "workspace"}
    covered |= {"spatial_conv_sep", "spatial_conv_2d"}
    missing = []
    for n, f in vars(ops).items():
        if inspect.isfunction(f) and f.__module__ == ops.__name__ and not n.startswith("_"):
            # (the aliases at the foot of ops.py are the functions above under their former names: f.__name__)
            if "cube" in inspect.signature(f).parameters and f.__name__ not in covered:
                missing.append(n)
    assert not missing, missing
