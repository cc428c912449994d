"""CPU: median / percentile / mad_std over two axes (axis=(1, 2): one value per channel; (0, 2); (0, 1)).

* the oracle (oracle/oracle_np.py takes an axis tuple as numpy does) against the vectors the reference produced
  (tests/golden/plane_order_stats.npz, tools/gen_golden_plane_order_stats.py), at the bounds test_oracle_golden.py uses for
  the one-axis forms;
* the C ABI: spc_percentile_groups_f32 and its size function are exported, declared and documented;
* what ``ops.percentile_global`` hands to the library: today's call without ``keep``, the new entry with the view's own
  pointer and strides with ``keep=0 | 1`` (the layouts of tests/views.py, ``_lib.call`` recorded as test_views_host.py
  records it);
* how ``SpectralCube`` normalises an axis argument."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_np as O
import views as V
from conftest import REPO, assert_close, golden
from spectral_cube_amd import SpectralCube, _lib, ops
from test_views_host import _Arr, _check_cube_struct, _check_mask_struct, _view, recorded  # noqa: F401

PAIRS = ((1, 2), (0, 2), (0, 1))
GONE = {(1, 2): 4, (0, 2): 7, (0, 1): 2}          # the channel, row index and column index the golden mask excludes whole
NEW = ("spc_percentile_groups_workspace_bytes", "spc_percentile_groups_f32")


@pytest.mark.parametrize("pair", PAIRS)
def test_oracle_reproduces_the_reference_over_two_axes(pair):
    g = golden("plane_order_stats.npz")
    d, inc = g["data"], g["include"]
    tag = "a%d%d" % pair
    assert d.dtype == np.float32 and d.shape == (9, 11, 13) and np.isnan(d).any()
    assert 0.25 < 1.0 - inc.mean() < 0.45
    assert bool(g["mad_std_from_reference"][PAIRS.index(pair)])
    assert_close(O.median(d, inc, axis=pair), g["median_" + tag], what="median %s" % (pair,))          # exact
    for q in (10.0, 37.5, 90.0):
        exp = g["p%g_%s" % (q, tag)]
        assert_close(O.percentile(d, inc, q, axis=pair), exp, atol=2e-6 * np.nanmax(np.abs(exp)), what="percentile %g %s" % (q, pair))
    exp = g["mad_std_" + tag]
    assert_close(O.mad_std(d, inc, axis=pair), exp, atol=2e-6 * np.nanmax(exp), what="mad_std %s" % (pair,))
    # the group without an included sample
    for k in ("median_", "p10_", "p37.5_", "p90_", "mad_std_"):
        nan = np.isnan(g[k + tag])
        assert nan[GONE[pair]] and nan.sum() == 1, k


def test_new_entry_is_exported_declared_and_documented():
    lib = _lib.load()
    hdr = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name), "libspcube_hip.so does not export " + name
        assert name in _lib.SIGNATURES, name + " is not declared in _lib.py"
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, hdr), name + " is not declared in include/spcube_hip.h"
    # the comment above the declarations names the reference lines the entry replaces and what it promises
    doc = hdr[:hdr.index("size_t spc_percentile_groups_workspace_bytes")].rsplit("/*", 1)[1]
    for word in ("spectral_cube.py:1172-1257", ":730-764", "keep_axis = 0", "keep_axis = 1", "d_center", "workspace"):
        assert word in doc, word
    assert lib.spc_abi_version() == 8
    assert lib.spc_workspace_bytes(99, 4, 4, 4, 0, 0) == 0            # no new kind: the entry has a size function of its own


def test_workspace_size_grows_with_the_groups():
    lib = _lib.load()
    sizes = [int(lib.spc_percentile_groups_workspace_bytes(n)) for n in (0, 1, 2, 3, 7, 64, 700, 65536, 1 << 20)]
    assert all(s > 0 for s in sizes)
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert sizes[6] >= 700 * 256 * 8                                   # 256 64-bit counters per group


def _mask(lay, mname):
    mlay = V.mask_layout(mname, lay)
    marr, mparent = _view(mlay, np.uint8)
    return ops.MaskSpec(_lib.MASK_ARRAY | _lib.MASK_FINITE, 0.0, 0.0, marr), mlay, mparent


def test_without_keep_the_call_is_the_one_it_was(recorded):
    lay = V.layout("xwin_off1")
    cube, parent = _view(lay, np.float32)
    mask, mlay, mparent = _mask(lay, "mask_phase")
    del recorded[:]
    ops.percentile_global(cube, 50.0, mask=mask)
    (name, a), = recorded
    assert name == "spc_percentile_global_f32" and len(a) == len(_lib.SIGNATURES[name][1]) == 10
    assert a[0] == cube.device and a[1] is None
    _check_cube_struct(a[2]._obj, cube, parent, lay, "cube")
    _check_mask_struct(a[3]._obj, mparent, mlay, "mask")
    assert a[4:7] == (50.0, 0, 0.0) and isinstance(a[7]._obj, C.c_double)
    assert isinstance(a[8], C.c_void_p) and a[9] >= _lib.load().spc_workspace_bytes(_lib.WS_PERCENTILE_GLOBAL, *cube.shape, 0, 0)
    del recorded[:]
    ops.percentile_global(cube, 25.0, mask=mask, center=1.5)
    (name, a), = recorded
    assert name == "spc_percentile_global_f32" and a[4:7] == (25.0, 1, 1.5)


@pytest.mark.parametrize("keep", [0, 1])
def test_keep_hands_the_layout_to_the_new_entry(recorded, keep):
    combos = [(c, "mask_same") for c in V.CUBE_LAYOUTS]
    combos += [(c, m) for c in ("xwin_aligned", "xwin_off1") for m in V.MASK_LAYOUTS]
    for cname, mname in combos:
        what = "keep=%d cube %s mask %s" % (keep, cname, mname)
        lay = V.layout(cname)
        cube, parent = _view(lay, np.float32)
        mask, mlay, mparent = _mask(lay, mname)
        n = lay.shape[keep]
        center = _Arr((n,), np.float32)
        del recorded[:]
        got = ops.percentile_global(cube, 37.5, mask=mask, center=center, keep=keep, scale=1.25)
        (name, a), = recorded
        assert name == "spc_percentile_groups_f32" and len(a) == len(_lib.SIGNATURES[name][1]), what
        _check_cube_struct(a[2]._obj, cube, parent, lay, what)
        _check_mask_struct(a[3]._obj, mparent, mlay, what)
        assert a[4:6] == (keep, 37.5) and a[6].value == center.ptr and a[7] == 1.25, what
        assert a[8].value == got.ptr and got.shape == (n,) and got.dtype == np.float32, what
        assert isinstance(a[9], C.c_void_p) and a[10] >= _lib.load().spc_percentile_groups_workspace_bytes(n), what
    # out= is used when it fits and refused when it does not; a centre of another length or type is refused
    cube, _ = _view(V.layout("contig"), np.float32)
    n = cube.shape[keep]
    out = _Arr((n,), np.float32)
    del recorded[:]
    assert ops.percentile_global(cube, 50.0, keep=keep, out=out) is out
    (name, a), = recorded
    assert a[6] is None and a[7] == 1.0 and a[8].value == out.ptr
    del recorded[:]
    for bad in (_Arr((n + 1,), np.float32), _Arr((n,), np.float64)):
        with pytest.raises((ValueError, TypeError)):
            ops.percentile_global(cube, 50.0, keep=keep, out=bad)
        with pytest.raises((ValueError, TypeError)):
            ops.percentile_global(cube, 50.0, keep=keep, center=bad)
    with pytest.raises((ValueError, TypeError)):
        ops.percentile_global(cube, 50.0, keep=keep, center=0.5)
    with pytest.raises(ValueError):
        ops.percentile_global(cube, 50.0, keep=2)
    assert recorded == []


def test_scale_and_out_need_keep(recorded):
    cube, _ = _view(V.layout("contig"), np.float32)
    with pytest.raises(ValueError):
        ops.percentile_global(cube, 50.0, scale=2.0)
    with pytest.raises(ValueError):
        ops.percentile_global(cube, 50.0, out=_Arr((cube.shape[0],), np.float32))
    assert recorded == []


def test_axis_arguments_are_normalised():
    r = SpectralCube._reduced_axes
    assert r([1]) == 1 and r((2, 1)) == (1, 2) and r((0, 1, 2)) is None and r((1, 1)) == 1
    assert r((2, 0)) == (0, 2) and r([1, 0]) == (0, 1) and r(None) is None and r(2) == 2
    with pytest.raises(ValueError):
        r((0, 3))
    with pytest.raises(ValueError):
        r(3)
