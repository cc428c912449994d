"""GPU: median / percentile / mad_std over two axes - ``cube.mad_std(axis=(1, 2))`` is the noise of every channel - and the
kernel underneath, ``ops.percentile_global(..., keep=0 | 1)`` (spc_percentile_groups_f32: per-group histograms, the digit
descent of all groups on the device).  Expected values: oracle/oracle_np.py on the host (tests/plane_order_stats.py), at the
bounds of the one-axis forms (test_gpu_long_axes.py:28-32): median exact, percentile 10 / 37.5 / 90 rtol 2e-6 + atol 2e-6
max|exp|, mad_std 3e-6 likewise, NaN in the same places.

Shapes, each with no mask (the isfinite predicate), a threshold predicate and a uint8 include array, NaN and both
infinities in the data, all three axis pairs:

    (5, 7, 9)        nothing aligned: the scalar tail only
    (4, 64, 64)      the vector path
    (3, 70, 531)     a plane larger than one block's piece: several blocks flush into one group's counters
    (700, 5, 7)      far more groups than blocks resident at once, tiny groups
    (2, 3, 70001)    a row longer than 65535

Planted groups (12, 6, 10), one plane each and again with z and y exchanged: no sample, one, two different ones (the next-key
pass and the mean), all equal, only +0.0 and -0.0, mixed signs around zero with subnormals, 1 + k 2^-23 (keys that agree down
to the last byte), an even count whose middle values are equal.

Then: every cube and mask layout of tests/views.py against the contiguous copy bit for bit; dirty scratch and recycled
memory (tests/dirty_memory.py); a second call; the reference's recorded results (tests/golden/plane_order_stats.npz); the
cube-level result's type; a signal mask built from the noise spectrum; a streamed cube; a float64 source."""
import warnings

import numpy as np
import pytest

import dirty_memory as DM
import plane_order_stats as P
import views as V
from conftest import golden
from spectral_cube_amd import PrecisionWarning, SpectralCube, _lib, ops
from spectral_cube_amd.device import DeviceArray
from spectral_cube_amd.wcs import parse_header

pytestmark = pytest.mark.gpu

MAD = 1.482602218505602


def _cube_stats(cube, pair):
    out = {"median": cube.median(axis=pair), "mad_std": cube.mad_std(axis=pair)}
    for q in P.QS:
        out["p%g" % q] = cube.percentile(q, axis=pair)
    return out


def _ops_stats(dev, mask, keep):
    """the five statistics through the binding: mad_std's centre never leaves the device"""
    med = ops.percentile_global(dev, 50.0, mask=mask, keep=keep)
    out = {"median": med.get(), "mad_std": ops.percentile_global(dev, 50.0, mask=mask, center=med, keep=keep, scale=MAD).get()}
    for q in P.QS:
        out["p%g" % q] = ops.percentile_global(dev, q, mask=mask, keep=keep).get()
    return out


def _bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("kind", P.MASKS)
@pytest.mark.parametrize("shape", P.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_pair_against_the_oracle(gpu, shape, kind):
    exp = P.expected(shape, kind)
    cube = P.cube(shape, kind)
    for pair in P.PAIRS:
        P.check({k: np.asarray(v) for k, v in _cube_stats(cube, pair).items()}, exp[pair], "%s %s axis=%s" % (shape, kind, pair))


@pytest.mark.parametrize("keep", [0, 1])
def test_planted_groups(gpu, keep):
    d, inc = P.planted()
    if keep == 1:                                   # the same groups as rows y of a (6, 12, 10) cube
        d, inc = np.ascontiguousarray(np.swapaxes(d, 0, 1)), np.ascontiguousarray(np.swapaxes(inc, 0, 1))
    pair = (1, 2) if keep == 0 else (0, 2)
    exp = P.oracle(d, inc, pair)
    assert np.isnan(exp["median"][0]) and exp["median"][1] == P.planted()[0][1, 3, 4] and exp["median"][2] == np.float32(-1.125)
    assert exp["median"][3] == 2.5 and exp["median"][4] == 0 and exp["mad_std"][3] == 0 and 1 < exp["median"][6] < 1 + 2.0 ** -17
    dev = DeviceArray.from_numpy(d, gpu)
    mask = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, DeviceArray.from_numpy(inc.view(np.uint8), gpu))
    P.check(_ops_stats(dev, mask, keep), exp, "planted keep=%d" % keep)
    # and through the cube, the third pair included
    cube = SpectralCube(d.copy(), header=P.HDR).with_mask(inc)
    for pr in P.PAIRS:
        P.check({k: np.asarray(v) for k, v in _cube_stats(cube, pr).items()}, P.oracle(d, inc, pr), "planted cube axis=%s" % (pr,))


def _view_combos():
    combos = [(c, "mask_same") for c in V.CUBE_LAYOUTS]
    combos += [(c, m) for c in ("xwin_aligned", "xwin_off1") for m in V.MASK_LAYOUTS]
    return combos


@pytest.mark.parametrize("keep", [0, 1])
def test_views_match_the_contiguous_copy_bit_for_bit(gpu, keep):
    """the walk test_gpu_views.py's table cannot do for the keep mode: every cube layout, every mask layout, a predicate on
    top of the array, with and without a centre"""
    d, m = V.data(np.float32)
    ref = {}
    for cname, mname in _view_combos():
        lay = V.layout(cname)
        x, mk = V.crop(d, lay), V.crop(m, lay)
        key = x.shape
        if key not in ref:
            cd, cm = DeviceArray.from_numpy(x, gpu), DeviceArray.from_numpy(mk, gpu)
            spec = ops.MaskSpec(_lib.MASK_ARRAY | _lib.MASK_GT, -0.5, 0.0, cm)
            ref[key] = _ops_stats(cd, spec, keep)
            P.check(ref[key], P.oracle(x, (mk != 0) & (x > np.float32(-0.5)), (1, 2) if keep == 0 else (0, 2)), "contiguous keep=%d" % keep)
        view, parent = V.upload(lay, x, V.CUBE_POISON[np.dtype(np.float32)], gpu)
        mview, mparent = V.upload(V.mask_layout(mname, lay), mk, 1, gpu)
        got = _ops_stats(view, ops.MaskSpec(_lib.MASK_ARRAY | _lib.MASK_GT, -0.5, 0.0, mview), keep)
        for k in ref[key]:
            assert _bits(got[k], ref[key][k]), "keep=%d cube %s mask %s: %s differs from the contiguous copy" % (keep, cname, mname, k)


def test_result_does_not_depend_on_what_memory_held(gpu):
    shape = (3, 70, 531)
    d, inc = P.data(shape), P.include_array(shape)
    exp = P.expected(shape, "array")

    def run():
        dev = DeviceArray.from_numpy(d, gpu)
        mask = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, DeviceArray.from_numpy(inc.view(np.uint8), gpu))
        out = {"keep0_" + k: v for k, v in _ops_stats(dev, mask, 0).items()}
        out.update({"keep1_" + k: v for k, v in _ops_stats(dev, mask, 1).items()})
        out["cube_mad_std"] = np.asarray(P.cube(shape, "array").mad_std(axis=(1, 2)))
        return out

    def check(first):
        P.check({k[6:]: v for k, v in first.items() if k.startswith("keep0_")}, exp[(1, 2)], "dirty keep=0")
        P.check({k[6:]: v for k, v in first.items() if k.startswith("keep1_")}, exp[(0, 2)], "dirty keep=1")
        assert _bits(first["cube_mad_std"], first["keep0_mad_std"])

    DM.same_under_every_pattern(run, check)


def test_second_call_is_bit_identical(gpu):
    """integer counters are the only reduction"""
    shape = (3, 70, 531)
    dev = DeviceArray.from_numpy(P.data(shape), gpu)
    mask = ops.MaskSpec(_lib.MASK_GT, P.THRESHOLD, 0.0, None)
    for keep in (0, 1):
        a, b = _ops_stats(dev, mask, keep), _ops_stats(dev, mask, keep)
        for k in a:
            assert _bits(a[k], b[k]), (keep, k)


def test_reference_results_are_reproduced(gpu):
    g = golden("plane_order_stats.npz")
    cube = SpectralCube.read(g["data"].copy(), parse_header(str(g["header"]))).with_mask(g["include"])
    for pair in P.PAIRS:
        tag = "a%d%d" % pair
        exp = {k: g["%s_%s" % (k, tag)] for k in ("median", "mad_std", "p10", "p37.5", "p90")}
        P.check({k: np.asarray(v) for k, v in _cube_stats(cube, pair).items()}, exp, "golden axis=%s" % (pair,))


def test_cube_level_result_is_built_like_the_mean(gpu):
    shape = (5, 7, 9)
    cube = P.cube(shape, "array")
    for pair in P.PAIRS + ([2, 1], (2, 0), [1, 0]):
        norm = tuple(sorted(pair))
        like = cube.mean(axis=norm)
        for got in (cube.median(axis=pair), cube.percentile(25, axis=pair), cube.mad_std(axis=pair),
                    cube.median(axis=pair, how="slice", iterate_rays=True), cube.mad_std(axis=pair, ignore_nan=True)):
            assert type(got) is type(like) and got.shape == like.shape and got.ndim == 1
            assert got.unit == like.unit and got.meta == like.meta and got.wcs is None and like.wcs is None
            assert np.asarray(got).dtype == np.float32
    # a list or tuple of one axis is that axis; all three are None
    assert np.array_equal(np.asarray(cube.median(axis=[1])), np.asarray(cube.median(axis=1)), equal_nan=True)
    assert np.array_equal(np.asarray(cube.mad_std(axis=(0,))), np.asarray(cube.mad_std(axis=0)), equal_nan=True)
    assert cube.percentile(30, axis=(0, 1, 2)) == cube.percentile(30)
    for q in (101, -1):
        with pytest.raises(ValueError):
            cube.percentile(q, axis=(1, 2))
    with pytest.raises(ValueError):
        cube.median(axis=(0, 3))


def test_signal_mask_from_the_noise_spectrum(gpu):
    """the recipe the feature is for: cube > 5 sigma per channel, evaluated on the device"""
    shape = (6, 16, 20)
    rng = np.random.default_rng(3)
    d = (rng.standard_normal(shape) * np.linspace(0.5, 3.0, shape[0])[:, None, None]).astype(np.float32)
    d[rng.random(shape) < 0.02] *= 40                                   # signal
    d[rng.random(shape) < 0.03] = np.nan
    cube = SpectralCube.read(d.copy(), P.HDR)
    noise = cube.mad_std(axis=(1, 2))
    exp_noise = P.O.mad_std(d, np.isfinite(d), axis=(1, 2))
    P.check({"mad_std": np.asarray(noise)}, {"mad_std": exp_noise}, "noise spectrum")
    masked = cube.with_mask(cube > 5 * noise[:, None, None])
    with np.errstate(invalid="ignore"):
        exp = np.isfinite(d) & (d > 5 * np.asarray(noise)[:, None, None])
    assert 0 < exp.sum() < exp.size // 10
    assert np.array_equal(masked.get_mask_array(), exp)


def test_out_of_core_planes_equal_the_resident_result(gpu, monkeypatch):
    """the HBM budget lowered (as test_gpu_far_from_zero.py lowers it) until the cube goes through the device in at least
    three slabs of channels: axis=(1, 2) is bit-identical to the resident cube's, the other pairs need the whole cube"""
    from spectral_cube_amd import streaming
    shape = (24, 40, 16)
    rng = np.random.default_rng(8)
    d = (0.3 + rng.standard_normal(shape)).astype(np.float32)
    d[rng.random(shape) < 0.05] = np.nan
    inc = rng.random(shape) < 0.7
    inc[5] = False
    resident = {}
    for kind in ("finite", "array"):
        c = SpectralCube.read(d.copy(), P.HDR)
        c = c.with_mask(inc) if kind == "array" else c
        resident[kind] = (c.median(axis=(1, 2)), c.percentile(90, axis=(1, 2)), c.mad_std(axis=(1, 2)))
    P.check({"median": np.asarray(resident["array"][0]), "mad_std": np.asarray(resident["array"][2])},
            {k: v for k, v in P.oracle(d, inc & np.isfinite(d), (1, 2)).items() if k in ("median", "mad_std")}, "resident")
    monkeypatch.setenv("SPC_HBM_BUDGET", str(d.size))           # a quarter of the float32 cube
    assert streaming.plan_planes(shape, streaming.hbm_budget(0), out_factor=0.0) * 3 <= shape[0]
    for kind in ("finite", "array"):
        big = SpectralCube.read(d.copy(), P.HDR)
        assert big._stream_source() is not None and big._dev is None
        big = big.with_mask(inc) if kind == "array" else big
        got = (big.median(axis=(1, 2)), big.percentile(90, axis=(1, 2)), big.mad_std(axis=(1, 2)))
        for a, b, name in zip(got, resident[kind], ("median", "percentile 90", "mad_std")):
            assert type(a) is type(b) and _bits(np.asarray(a), np.asarray(b)), (kind, name)
        assert big._dev is None, "the cube was never made resident"
        for pair in ((0, 2), (0, 1)):
            with pytest.raises(streaming.HugeCubeError, match=r"\(1, 2\)"):
                big.median(axis=pair)


def test_float64_source_gives_the_float32_result_and_says_so_once(gpu, monkeypatch):
    shape = (5, 7, 9)
    d = P.data(shape)
    narrow = SpectralCube.read(d.copy(), P.HDR)
    exp = {pair: narrow.mad_std(axis=pair) for pair in P.PAIRS}
    exp_median = np.asarray(narrow.median(axis=(1, 2)))
    _float64_resident(d, narrow, exp)
    # streamed: the planes go through the device as float32 slabs, and that is said as well
    monkeypatch.setenv("SPC_HBM_BUDGET", str(d.size))
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        big = SpectralCube.read(d.astype(np.float64), P.HDR)
        assert big._stream_source() is not None
        got = (big.mad_std(axis=(1, 2)), big.median(axis=(1, 2)))
    assert len([w for w in seen if issubclass(w.category, PrecisionWarning)]) == 1, [str(w.message) for w in seen]
    assert _bits(np.asarray(got[0]), np.asarray(exp[(1, 2)])) and _bits(np.asarray(got[1]), exp_median)


def _float64_resident(d, narrow, exp):
    wide = SpectralCube.read(d.astype(np.float64), P.HDR)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        got = {pair: wide.mad_std(axis=pair) for pair in P.PAIRS}
        med = wide.median(axis=(1, 2))
    assert len([w for w in seen if issubclass(w.category, PrecisionWarning)]) == 1, [str(w.message) for w in seen]
    for pair in P.PAIRS:
        assert _bits(np.asarray(got[pair]), np.asarray(exp[pair])), pair
    assert _bits(np.asarray(med), np.asarray(narrow.median(axis=(1, 2))))
