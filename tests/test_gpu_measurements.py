"""GPU: per-label measurements (csrc/spc_label_measure.hip through ops.label_measure, spectral_cube_amd.measurements,
LabelMap.measure / catalog) against scipy.ndimage and against the numpy restatement of the kernel's tables
(test_measurements_host.restate).

Tolerances are derived, not tuned.  Counts, extrema and positions are integers and samples: they must be EQUAL.
A float64 sum of m terms t_i, added in any order, obeys |err| <= (m - 1) U sum |t_i| with U = 2^-53.  Every term is made
in float64 from exact inputs (a float32 sample widens exactly, coordinates are small integers) by at most 3 roundings:
the subtraction of the origin, and one per multiply - 1 for (v - v0)^2, 2 for v dz dy.  The restatement forms the terms
with the same operations in the same order, so against it only the order of the additions differs; scipy's terms may
differ by those <= 3 roundings.  Two summation orders, ours and the other's, therefore differ by at most

    sum_bound = 2 (m + 3) U sum |t_i|     per label,

with sum |t_i| computed per label in numpy (the "abs_*" tables of restate).  For a second pass (variance about the means,
second moments about the centroids) the restatement is given the origin table the first DEVICE pass returned, so the bound
holds without an extra term; against scipy, which has its own means, check_against_scipy (test_measurements_host.py) adds
the first-order term of the difference of the means.  Quotients - the mean, the centroid - get the bound propagated
through the division.  The atomic order is not fixed: two calls agree to sum_bound too, and exactly in everything else."""
import functools

import numpy as np
import pytest
import scipy.ndimage as ndi

import dirty_memory
import labelling as R
import views
from spectral_cube_amd import _lib, labelling, measurements as MS, ops, SpectralCube
from spectral_cube_amd.device import DeviceArray
from test_measurements_host import (GROUPS, HDR, U, assert_catalogs_agree, catalog_loop, check_against_scipy, field_case,
                                    positive_blobs, restate, sum_bound)

pytestmark = pytest.mark.gpu

EXACT = ("count", "min_pos", "max_pos")
SAMPLES = ("min", "max")


def label_map(labels, n):
    return labelling.LabelMap(DeviceArray.from_numpy(np.ascontiguousarray(labels, dtype=np.int32)), n)


def cube_of(data, include=None):
    c = SpectralCube.read(data, dict(HDR))
    return c if include is None else c.with_mask(np.asarray(include, bool))


class Device:
    """the ten public functions on (cube, labels), as check_against_scipy asks for them"""

    def __init__(self, cube, lab):
        self.cube, self.lab = cube, lab

    def __getattr__(self, name):
        return lambda index: getattr(MS, name)(self.cube, self.lab, index)


def raw(data, include, labels, n, origin=None, want=GROUPS, mask=None, **kw):
    """the device's tables as host arrays, through ops.label_measure; *include*: a bool array (uploaded as 0 / 1)"""
    d = data if isinstance(data, DeviceArray) else DeviceArray.from_numpy(data)
    if mask is None and include is not None:
        mask = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, DeviceArray.from_numpy(np.asarray(include, bool).astype(np.uint8)))
    lab = DeviceArray.from_numpy(np.ascontiguousarray(labels, dtype=np.int32))
    return {k: v.get() for k, v in ops.label_measure(d, lab, n, mask_spec=mask, origin=origin, want=want, **kw).items()}


def within(got, exp, bound, what):
    got, exp = np.asarray(got, np.float64), np.asarray(exp, np.float64)
    fin = np.isfinite(exp)
    assert (np.abs(got[fin] - exp[fin]) <= np.broadcast_to(bound, exp.shape)[fin]).all(), \
        (what, np.abs(got[fin] - exp[fin]).max(), np.argwhere(fin & ~(np.abs(got - exp) <= bound))[:4].tolist())
    assert np.array_equal(got[~fin], exp[~fin], equal_nan=True), (what, "inf / NaN sums")


def check_raw(got, exp, what=""):
    """the device's tables against the restated ones: exact where the header says exact, sum_bound for the sums"""
    for key, g in got.items():
        e = exp[key]
        assert g.shape == e.shape and g.dtype == e.dtype, (what, key, g.shape, g.dtype)
        if key in EXACT:
            assert np.array_equal(g, e), (what, key, np.argwhere(g != e)[:4].tolist())
        elif key in SAMPLES:
            assert np.array_equal(g, e, equal_nan=True) and np.array_equal(np.signbit(g), np.signbit(e)), (what, key)
        else:
            within(g, e, sum_bound(exp["count"][:, None], exp["abs_" + key]), (what, key))
    assert exp["count"][0] == 0 and all(np.isnan(got[k][0]) for k in SAMPLES if k in got)       # the background: never measured


def random_origin(n, shape, seed=0):
    rng = np.random.default_rng(seed)
    return np.concatenate([rng.normal(size=(n + 1, 1)), rng.uniform(0, 1, (n + 1, 3)) * np.asarray(shape)], axis=1)


# ---- the case table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n, _ in R.structures()])
def test_case_table(gpu, name):
    done = 0
    for j, (cid, x, s) in enumerate(R.cases()):
        if cid.split("-")[0] != name:
            continue
        done += 1
        data, include, labels, n = field_case(x, s, j, np.float32 if j % 2 else np.float64)
        got = raw(data, include, labels, n)
        check_raw(got, restate(data, include, labels, n), cid)
        if n == 0:
            continue
        Q = Device(cube_of(data, include), label_map(labels, n))
        several = np.random.default_rng(j).integers(1, n + 1, size=min(n, 5))
        for index in (int(several[0]), np.concatenate([several, several[:2]]).tolist(), None):
            check_against_scipy(Q, data, include, labels, n, index, (cid, index))
    assert done == len(R.SHAPES) * len(R.DENSITIES)


# ---- row lengths around a wave's 64 voxels --------------------------------------------------------------------------------
@pytest.mark.parametrize("nx", [1, 63, 64, 65, 130])
def test_row_lengths(gpu, nx):
    shape = (3, 4, nx)
    row = np.arange(12).reshape(3, 4, 1)
    x = np.arange(nx).reshape(1, 1, nx)
    # two runs a row; the last voxel of every row and the first of the next carry different labels
    labels = np.where(x < nx // 2, 1 + (2 * row) % 5, 1 + (2 * row + 1) % 5).astype(np.int32)
    flat = labels.reshape(12, nx)
    assert (flat[:-1, -1] != flat[1:, 0]).all()
    rng = np.random.default_rng(nx)
    holes = np.where(rng.random(shape) < 0.2, 0, labels)                 # the same with background inside the runs
    holes[:, :, -1], holes[:, :, 0] = labels[:, :, -1], labels[:, :, 0]
    for dtype in (np.float32, np.float64):
        data = rng.normal(size=shape).astype(dtype)
        for lab in (labels, holes):
            o = random_origin(5, shape, nx)
            check_raw(raw(data, None, lab, 5, origin=o), restate(data, None, lab, 5, o), "nx=%d" % nx)
            for want in (("sums",), ("extrema",), ("first",), ("second",), ("sums", "second")):    # every group on its own kernel
                got = raw(data, None, lab, 5, origin=o, want=want)
                assert sorted(got) == sorted(k for k, (g, _, _) in ops._MEASURE_TABLES.items() if g in want)
                check_raw(got, restate(data, None, lab, 5, o), "nx=%d %s" % (nx, want))
    Q = Device(cube_of(data), label_map(labels, 5))
    for index in (3, [1, 2, 3, 4, 5], None):
        check_against_scipy(Q, data, None, labels, 5, index, ("nx=%d" % nx, index))


# ---- one run through the whole array, and no run at all ---------------------------------------------------------------------
def test_one_label_filling_the_array(gpu):
    shape = (3, 17, 130)
    rng = np.random.default_rng(1)
    labels = np.ones(shape, np.int32)
    for dtype in (np.float32, np.float64):
        data = rng.normal(size=shape).astype(dtype)
        o = random_origin(1, shape)
        check_raw(raw(data, None, labels, 1, origin=o), restate(data, None, labels, 1, o), "one label")
        Q = Device(cube_of(data), label_map(labels, 1))
        for index in (1, [1], None):
            check_against_scipy(Q, data, None, labels, 1, index, ("one label", index))
    # carried across blocks: more voxels than one block's span (rounds: test_walk_of_more_rounds_than_one)
    shape = (5, 40, 130)
    data = rng.normal(size=shape).astype(np.float32)
    check_raw(raw(data, None, np.ones(shape, np.int32), 1), restate(data, None, np.ones(shape, np.int32), 1), "one label, many blocks")


def test_walk_of_more_rounds_than_one(gpu):
    """The sizes the kernel is made for.  A wave walks `chunks` x 64 consecutive voxels a round, chunks = 16 doubled while
    2 x 2048 blocks are still filled, and the grid is 2048 blocks at most: at 40 x 512 x 1024 = 20 971 520 voxels chunks is
    32, a block's span 8192 voxels, and 2560 spans go to 2048 blocks - a quarter of the blocks walk a second round, 16.7
    million voxels further on, with the run they carried out of the first.  (chunks = 64 ... 256 take 6.7e7 ... 2.7e8 voxels,
    a GiB of labels: the same loop with another bound, timed by tools/time_label_measure.py and not run here.)
    Three large regions - one of them in the second round's part of the array - and 2e5 single voxels between them."""
    shape = (40, 512, 1024)
    rng = np.random.default_rng(9)
    labels = np.zeros(shape, np.int32)
    labels[2:6, 50:150, 100:900], labels[15:18, 100:200, :], labels[33:39, 400:450, 512:] = 1, 2, 3
    lone = np.flatnonzero((labels.ravel() == 0) & (rng.random(labels.size, dtype=np.float32) < 0.01))
    labels.ravel()[lone] = 4 + np.arange(lone.size, dtype=np.int32)
    n = 3 + lone.size
    data = rng.standard_normal(shape, dtype=np.float32)
    data[rng.random(shape, dtype=np.float32) < 0.02] = np.nan
    exp = restate(data, None, labels, n)
    assert exp["count"][1:4].min() > 1e5 and n > 1e5 and labels[33:].any() and data.size > 2048 * 8192
    got = raw(data, None, labels, n)
    check_raw(got, exp, "two rounds")
    assert got["count"][1] + got["count"][2] + got["count"][3] == (~np.isnan(data[(labels > 0) & (labels < 4)])).sum()


def test_every_voxel_a_label_of_its_own(gpu):
    shape = (6, 40, 40)
    lab, n = labelling.label(np.ones(shape, bool), structure=np.zeros((3, 3, 3), bool))
    assert n == 9600
    labels = np.arange(1, n + 1, dtype=np.int32).reshape(shape)
    assert np.array_equal(lab.get(), labels)
    rng = np.random.default_rng(2)
    data = rng.normal(size=shape).astype(np.float32)
    data[rng.random(shape) < 0.05] = np.nan
    o = random_origin(n, shape)
    check_raw(raw(data, None, labels, n, origin=o), restate(data, None, labels, n, o), "singletons")
    idx = np.flatnonzero(~np.isnan(data.ravel())) + 1
    cube = cube_of(data)
    assert np.array_equal(MS.sum_labels(cube, lab, idx), data.ravel()[idx - 1].astype(np.float64))       # one term: exact
    assert np.array_equal(MS.maximum(cube, lab, idx), data.ravel()[idx - 1])
    assert MS.maximum_position(cube, lab, idx[:50]) == [tuple(int(c) for c in np.unravel_index(i - 1, shape)) for i in idx[:50]]
    assert (MS.variance(cube, lab, idx) == 0).all()


def test_no_label_at_all(gpu):
    shape = (5, 6, 7)
    data = np.random.default_rng(3).normal(size=shape).astype(np.float32)
    got = raw(data, None, np.zeros(shape, np.int32), 0)
    check_raw(got, restate(data, None, np.zeros(shape, np.int32), 0), "n = 0")
    assert got["count"].tolist() == [0] and got["min_pos"].tolist() == [-1] and not got["first"].any()
    lab = label_map(np.zeros(shape, np.int32), 0)
    cube = cube_of(data)
    assert MS.sum_labels(cube, lab) == 0.0 and np.isnan(MS.mean(cube, lab)) and MS.maximum_position(cube, lab) == (-1, -1, -1)
    assert MS.sum_labels(cube, lab, []).shape == (0,)
    cat = lab.catalog(cube)
    assert all(len(v) == 0 for k, v in cat.items() if k != "meta") and cat["meta"]["flux_unit"] == "K km/s"
    with pytest.raises(ValueError, match="background"):
        MS.sum_labels(cube, lab, 1)


def test_a_label_out_of_range_is_skipped_and_reported(gpu):
    shape = (3, 4, 70)
    labels = np.random.default_rng(4).integers(0, 4, shape).astype(np.int32)
    data = np.ones(shape, np.float32)
    for bad in (4, -1, 2 ** 31 - 1):
        lab = labels.copy()
        lab[1, 2, 33] = bad
        with pytest.raises(ValueError, match="outside 0"):
            raw(data, None, lab, 3)
    check_raw(raw(data, None, labels, 3), restate(data, None, labels, 3), "after the refusals")


# ---- ties -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_ties_zeros_and_infinities(gpu, dtype):
    shape = (4, 5, 70)
    rng = np.random.default_rng(5)
    labels = np.zeros(shape, np.int32)
    labels[0, 1:4, 10:60], labels[1, :, 3:69], labels[2, 2:, :], labels[3, 0, 5:40], labels[3, 3, 5:40] = 1, 2, 3, 4, 5
    data = rng.normal(size=shape).astype(dtype)
    data[labels == 1] = 2.5                                              # constant: both positions are the first voxel
    zero = rng.random(shape) < 0.3                                       # both zeros among positive samples: the minimum
    data[labels == 2] = np.abs(data[labels == 2]) + 1
    data[(labels == 2) & zero] = 0.0
    data[1, 0, 20], data[1, 0, 7] = -0.0, 0.0
    data[1, 0, 3:7] = 1.0
    data[2, 3, 17], data[2, 2, 60], data[2, 4, 1] = np.inf, -np.inf, np.inf
    data[3, 0, 30] = data[3, 0, 12] = np.inf                             # label 4: +inf twice, label 5: -0.0 the maximum
    data[labels == 5] = -np.abs(data[labels == 5]) - 1
    data[3, 3, 22], data[3, 3, 31] = -0.0, 0.0
    got = raw(data, None, labels, 5)
    check_raw(got, restate(data, None, labels, 5), "ties")
    first = lambda k: int(np.flatnonzero(labels.ravel() == k)[0])  # noqa: E731
    assert got["min_pos"][1] == got["max_pos"][1] == first(1) and got["min"][1] == got["max"][1] == dtype(2.5)
    assert got["min"][2] == 0 and got["min_pos"][2] == np.ravel_multi_index((1, 0, 7), shape)            # +0.0 at 7, -0.0 at 20
    assert got["max"][5] == 0 and got["max_pos"][5] == np.ravel_multi_index((3, 3, 22), shape)           # -0.0 first
    assert got["max"][3] == np.inf and got["min"][3] == -np.inf and np.isnan(got["sums"][3, 0]) and got["sums"][3, 1] == np.inf and got["count"][3] == 210
    assert got["max_pos"][3] == np.ravel_multi_index((2, 3, 17), shape) and got["min_pos"][3] == np.ravel_multi_index((2, 2, 60), shape)
    assert got["sums"][4, 0] == np.inf and got["max_pos"][4] == np.ravel_multi_index((3, 0, 12), shape)
    cube, lab = cube_of(data), label_map(labels, 5)
    idx = [1, 2, 3, 4, 5]
    # through the cube: its own mask keeps finite samples only (LazyMask(np.isfinite), as the reference's), so the
    # infinities leave.  scipy finds positions with an unstable argsort - among equal samples its choice is arbitrary -
    # so the positions of tied extremes are held to the first voxel, the restatement, and only the values to scipy
    fin = np.isfinite(data)
    exp = restate(data, fin, labels, 5)
    lab2, dnat = np.where(fin, labels, 0), np.where(fin, data, dtype(0))
    unravel = lambda p: [tuple(int(c) for c in np.unravel_index(q, shape)) for q in p]  # noqa: E731
    assert MS.minimum_position(cube, lab, idx) == unravel(exp["min_pos"][1:])
    assert MS.maximum_position(cube, lab, idx) == unravel(exp["max_pos"][1:])
    assert np.array_equal(MS.minimum(cube, lab, idx), ndi.minimum(dnat, lab2, idx))
    assert np.array_equal(MS.maximum(cube, lab, idx), ndi.maximum(dnat, lab2, idx))
    for f, fp, sv in ((MS.minimum, MS.minimum_position, ndi.minimum), (MS.maximum, MS.maximum_position, ndi.maximum)):
        v = f(cube, lab)
        assert v == sv(dnat, lab2)
        assert fp(cube, lab) == unravel([np.flatnonzero((lab2.ravel() > 0) & (dnat.ravel() == v))[0]])[0]


# ---- the mask ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_mask_bytes_thresholds_and_nan(gpu, dtype):
    shape = (5, 9, 67)
    rng = np.random.default_rng(6)
    labels, n = R.scipy_label(R.field(shape, 11, 0.55))
    data = rng.normal(size=shape).astype(dtype)
    data[rng.random(shape) < 0.1] = np.nan
    some = int(np.argmax(np.bincount(labels.ravel())[1:])) + 1
    inside = np.flatnonzero(labels.ravel() == some)
    data.ravel()[inside[::2]] = np.nan                                   # every second voxel of the largest label
    assert np.isnan(data[labels == some]).sum() >= inside.size // 2
    # any non-zero byte includes
    byte = rng.choice(np.array([0, 1, 2, 0x80, 0xFF], np.uint8), size=shape)
    gone = int(labels[labels > 0][5])
    byte[labels == gone] = 0                                             # a label whose voxels are all excluded
    spec = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, DeviceArray.from_numpy(byte))
    got = raw(data, None, labels, n, mask=spec)
    check_raw(got, restate(data, byte != 0, labels, n), "mask bytes")
    assert got["count"][gone] == 0 and np.isnan(got["max"][gone]) and got["max_pos"][gone] == -1 and not got["first"][gone].any()
    # threshold terms, with and without the array
    for flags, lo, hi, inc in ((_lib.MASK_GT, 0.25, 0.0, data > dtype(0.25)), (_lib.MASK_LE | _lib.MASK_GE, -0.5, 1.0, (data >= dtype(-0.5)) & (data <= dtype(1.0))),
                               (_lib.MASK_ARRAY | _lib.MASK_LT, 0.0, 0.1, (byte != 0) & (data < dtype(0.1)))):
        spec = ops.MaskSpec(flags, lo, hi, DeviceArray.from_numpy(byte) if flags & _lib.MASK_ARRAY else None)
        with np.errstate(invalid="ignore"):
            check_raw(raw(data, None, labels, n, mask=spec), restate(data, inc, labels, n), "threshold %d" % flags)
    # through the cube: with_mask(bool array) and a lazy threshold
    cube = cube_of(data, byte != 0)
    lab = label_map(labels, n)
    live = np.flatnonzero(restate(data, byte != 0, labels, n)["count"])
    check_against_scipy(Device(cube, lab), data, byte != 0, labels, n, live[:7].tolist(), "with_mask")
    assert MS.sum_labels(cube, lab, gone) == 0.0 and np.isnan(MS.mean(cube, lab, gone)) and np.isnan(MS.variance(cube, lab, gone))
    assert MS.minimum_position(cube, lab, gone) == (-1, -1, -1) and np.isnan(MS.maximum(cube, lab, [gone]))[0]
    plain = cube_of(data)
    with np.errstate(invalid="ignore"):
        check_against_scipy(Device(plain.with_mask(plain > 0.25), lab), data, data > dtype(0.25), labels, n, None, "cube > 0.25")


# ---- strided and offset views -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("name,mname", [("rows", "mask_same"), ("xwin_off1", "mask_contig"), ("xwin_oddstride", "mask_phase"),
                                        ("xwin_tail", "mask_same")])
def test_views_of_the_cube_and_the_mask(gpu, dtype, name, mname):
    base = (5, 9, 132)
    lay = views.layout(name, base)
    d, m = views.data(np.dtype(dtype), base)
    d, m = views.crop(d, lay), views.crop(m, lay)
    labels, n = R.scipy_label(R.field(lay.shape, 21, 0.5))
    cube, _p1 = views.upload(lay, d, views.CUBE_POISON[np.dtype(dtype)])
    marr, _p2 = views.upload(views.mask_layout(mname, lay), m, 1)
    spec = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, marr)
    o = random_origin(n, lay.shape)
    check_raw(raw(cube, None, labels, n, origin=o, mask=spec), restate(d, m != 0, labels, n, o), "%s %s" % (name, mname))
    check_raw(raw(cube, None, labels, n, want=("sums",)), restate(d, None, labels, n), "%s sums, no mask" % name)


# ---- data far from zero -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_variance_on_a_pedestal(gpu, dtype):
    shape = (6, 40, 40)
    rng = np.random.default_rng(8)
    labels, n = R.scipy_label(R.field(shape, 5, 0.45), ndi.generate_binary_structure(3, 2))
    data = (1000.0 + rng.normal(size=shape)).astype(dtype)               # a 1000 K baseline, unit noise
    Q = Device(cube_of(data), label_map(labels, n))
    big = np.argsort(np.bincount(labels.ravel())[1:])[-6:] + 1
    for index in (int(big[-1]), big.tolist(), None):
        check_against_scipy(Q, data, None, labels, n, index, ("pedestal", index))
    v = MS.variance(Q.cube, Q.lab, int(big[-1]))
    assert 0.5 < v < 1.5                                                 # (sum v^2 / m - mean^2 in float32 would be ~0 or negative)


# ---- what memory held -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_dirty_tables_and_workspace(gpu, dtype):
    shape = (5, 9, 67)
    x = R.field(shape, 31, 0.5)
    data, include, labels, n = field_case(x, None, 31, dtype)
    o = random_origin(n, shape)
    exp = restate(data, include, labels, n, o)
    firsts = None
    for pattern in dirty_memory.PATTERNS:
        with dirty_memory.dirty(pattern):
            out = {k: DeviceArray((n + 1,) + cols, dtype if dt is None else dt) for k, (_, cols, dt) in ops._MEASURE_TABLES.items()}
            ws = DeviceArray((int(_lib.load().spc_label_measure_workspace_bytes(n, 15)),), np.uint8)
            got = raw(data, include, labels, n, origin=o, out=out, workspace=ws)
            pooled = raw(data, include, labels, n, origin=o)             # the stream's scratch, dirtied on entry
        for g in (got, pooled):
            check_raw(g, exp, "dirty %r" % (pattern,))
            if firsts is None:
                firsts = g
            for k in EXACT + SAMPLES:
                assert np.array_equal(g[k], firsts[k], equal_nan=True), (pattern, k)


# ---- the atomic order is not fixed ------------------------------------------------------------------------------------------
def test_two_calls_agree(gpu):
    shape = (6, 40, 40)
    data, include, labels, n = field_case(R.field(shape, 41, 0.5), None, 41)
    exp = restate(data, include, labels, n)
    a, b = raw(data, include, labels, n), raw(data, include, labels, n)
    for k in EXACT + SAMPLES:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
    for k in ("sums", "first", "second"):
        within(a[k], b[k], sum_bound(exp["count"][:, None], exp["abs_" + k]), ("twice", k))


# ---- label -> catalogue ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def line_case(dtype):
    data = R.line_cube(dtype)
    data.setflags(write=False)
    with np.errstate(invalid="ignore"):
        include = data > 2.0
    labels, n = R.scipy_label(include)
    return data, include, labels, n


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_label_to_catalogue(gpu, dtype):
    data, include, labels, n = line_case(dtype)
    cube = SpectralCube.read(np.array(data), dict(HDR))
    masked = cube.with_mask(cube > 2.0)
    lab, got_n = labelling.label(masked)
    assert got_n == n >= 3 and np.array_equal(lab.get(), labels)
    cat = lab.catalog(masked)
    exp = catalog_loop(data, include, labels, n, channel_width=0.5)
    # every float column within the bound catalog_loop derives for it (samples above 2: weights of one sign, tight bounds)
    assert_catalogs_agree({k: v for k, v in cat.items() if k != "meta"}, exp, "line cube")
    assert cat["meta"]["flux_unit"] == "K km/s" and cat["meta"]["channel_width"] == 0.5 and cat["peak"].dtype == dtype
    ok = np.isfinite(cat["centroid"]).all(axis=1)
    assert ok.all() and np.allclose(cat["v_cen"], -16.0 + 0.5 * cat["centroid"][:, 0], rtol=0, atol=1e-12)
    lon, lat = cube.wcs.celestial_pix2world(cat["centroid"][:, 2], cat["centroid"][:, 1])
    assert np.array_equal(cat["lon"], lon) and np.array_equal(cat["lat"], lat)
    assert np.array_equal(cat["sigma_v"], 0.5 * cat["sigma_z"], equal_nan=True)
    t = lab.measure(masked)
    assert np.array_equal(t["count"][1:], cat["npix"]) and sorted(t) == ["count", "first", "max", "max_pos", "min", "min_pos", "sums"]
    # the same flux the slow way: one full pass of the cube per label
    k = int(np.argmax(cat["npix"])) + 1
    one = float(masked.with_mask(lab.select([k])).sum())
    v = data[labels == k].astype(np.float64)
    # cube.sum() adds in float64 in an order of its own (sum_bound) and may hand the total back in the cube's precision
    assert abs(one - MS.sum_labels(masked, lab, k)) <= sum_bound(v.size, np.abs(v).sum()) + 2.0 ** -23 * abs(v.sum())
    assert abs(MS.sum_labels(masked, lab, k) - v.sum()) <= sum_bound(v.size, np.abs(v).sum())
    blobs = positive_blobs((12, 20, 33), 1, dtype)
    cat = label_map(blobs[2], blobs[3]).catalog(cube_of(blobs[0], blobs[1]))
    assert_catalogs_agree({k: v for k, v in cat.items() if k != "meta"}, catalog_loop(*blobs, channel_width=0.5), "blobs")
