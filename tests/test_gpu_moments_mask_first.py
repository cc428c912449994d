"""GPU: the mask-first march of the moment kernel (16-byte lanes with a uint8 mask array: the mask dwords of a batch are
loaded first and a lane loads its four samples only where its dword is not zero) gives, bit for bit, the maps of the loop
that loads every sample (SPC_MOMENTS_MASK_FIRST=0), whatever lies under the excluded voxels."""
import functools

import numpy as np
import pytest

import oracle_np as O
from conftest import assert_close
from spectral_cube_amd import _lib, ops, synth
from spectral_cube_amd.device import DeviceArray

pytestmark = pytest.mark.gpu

SWITCH = "SPC_MOMENTS_MASK_FIRST"
SHAPES = [(77, 13, 52),      # 13 lane groups per row: a wave's lanes straddle rows and 128-byte lines; nz has a tail
          (640, 24, 136),
          (530, 9, 50),      # 8-byte lanes (VEC = 2): the switch changes nothing
          (9, 5, 256)]       # nine planes: one batch and a tail at the default launch (ZW = 1, U = 8), the tail loop alone at ZW = 8 and ZW = 4
LAUNCHES = [{}, {"SPC_MOMENTS_ZW": "8"}, {"SPC_MOMENTS_ZW": "1", "SPC_MOMENTS_NSPLIT": "1"},
            {"SPC_MOMENTS_ZW": "4", "SPC_MOMENTS_U": "4", "SPC_MOMENTS_XCD": "1", "SPC_MOMENTS_NSPLIT": "3"}, {"SPC_MOMENTS_U": "2"}]
THRESHOLDS = (_lib.MASK_FINITE | _lib.MASK_GT | _lib.MASK_LE, -0.25, 3.0)


def _segments(d, rng):
    """30 % random, with whole 32-voxel x-segments empty: the even ones on odd planes, the odd ones on even planes"""
    nz, ny, nx = d.shape
    m = rng.random(d.shape) < 0.3
    z, x = np.arange(nz)[:, None, None], np.arange(nx)[None, None, :]
    m[np.broadcast_to(((x // 32) + z) % 2 == 1, d.shape)] = False
    return m


def _single(d, rng):
    m = np.zeros(d.shape, dtype=bool)
    m[-1, -1, -1] = True
    return m


MASKS = {
    "all zero": lambda d, rng: np.zeros(d.shape, dtype=bool),
    "all one": lambda d, rng: np.ones(d.shape, dtype=bool),
    "4 % random": lambda d, rng: rng.random(d.shape) < 0.04,
    "empty 32-voxel segments on alternate planes": _segments,
    "one voxel, last column of the last row of the last plane": _single,
    "bench mask": lambda d, rng: synth.boolean_mask(d, 5).astype(bool),
    "70 % random + isfinite + (lo, hi]": lambda d, rng: rng.random(d.shape) < 0.7,
}


@functools.lru_cache(maxsize=None)
def _cube(shape):
    d = synth.gaussian_line_cube(shape, 40 + shape[0])
    d.setflags(write=False)
    return d


def _case(shape, mask_kind):
    """(poisoned cube, the same with the poisoned voxels zeroed, mask array, flags, lo, hi): NaN, +Inf and -Inf at a seeded
    5 % of the voxels that the mask array excludes"""
    rng = np.random.default_rng(shape[0] + shape[2] + len(mask_kind))
    clean = _cube(shape)
    arr = MASKS[mask_kind](clean, rng)
    poison = ~arr & (rng.random(shape) < 0.05)
    d = clean.copy()
    d[poison] = rng.choice(np.array([np.nan, np.inf, -np.inf], dtype=np.float32), size=int(poison.sum()))
    zeroed = d.copy()
    zeroed[poison] = 0.0
    flags, lo, hi = THRESHOLDS if "isfinite" in mask_kind else (0, 0.0, 0.0)
    return d, zeroed, arr, flags, lo, hi


def _axis(nz):
    v = synth.spectral_axis(nz)
    cen = v - v[0]
    return v, cen, cen[nz // 2]


def _maps(monkeypatch, switch, dcube, spec, nz, want):
    monkeypatch.setenv(SWITCH, switch)
    v, cen, cref = _axis(nz)
    r = ops.moments(dcube, DeviceArray.from_numpy(cen - cref), dv=500.0, m1_add=cref + v[0], mask=spec, want=want)
    return {k: r[k].get() for k in want}


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


@pytest.mark.parametrize("mask_kind", sorted(MASKS))
@pytest.mark.parametrize("launch", LAUNCHES, ids=lambda s: ",".join("%s=%s" % (k[12:], v) for k, v in s.items()) or "default")
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mask_first_is_bit_identical(gpu, monkeypatch, shape, launch, mask_kind):
    """SPC_MOMENTS_MASK_FIRST=0 and =1 in one process: m0, m1, m2 (the sums alone) and with nvalid (the count) are equal
    bit for bit; so are the maps of the cube whose poisoned excluded voxels are zeroed: no value that the mask-first loop
    does not read reaches a sum.  With the default launch also against the oracle, at the tolerances of
    test_moment_kernel_template_space."""
    for k, v in launch.items():
        monkeypatch.setenv(k, v)
    nz = shape[0]
    d, zeroed, arr, flags, lo, hi = _case(shape, mask_kind)
    spec = ops.MaskSpec(flags | _lib.MASK_ARRAY, lo, hi, DeviceArray.from_numpy(arr.astype(np.uint8)))
    dcube, dzero = DeviceArray.from_numpy(d), DeviceArray.from_numpy(zeroed)
    for want in (("m0", "m1", "m2"), ("m0", "m1", "m2", "nvalid")):
        old = _maps(monkeypatch, "0", dcube, spec, nz, want)
        new = _maps(monkeypatch, "1", dcube, spec, nz, want)
        _same(new, old, "switch 1 against switch 0")
        _same(_maps(monkeypatch, "1", dzero, spec, nz, want), new, "poisoned voxels zeroed")
    if mask_kind == "all zero":
        assert np.isnan(new["m0"]).all() and np.isnan(new["m1"]).all() and np.isnan(new["m2"]).all() and not new["nvalid"].any()
    if not launch:
        inc = arr & ~np.isnan(d)
        if flags:
            inc &= np.isfinite(d) & (np.nan_to_num(d) > np.float32(lo)) & (np.nan_to_num(d) <= np.float32(hi))
        v, cen, _ = _axis(nz)
        e0, e1, e2 = O.moments012(d, inc, cen, 500.0, v[0])
        assert np.array_equal(new["nvalid"], inc.sum(axis=0))
        with np.errstate(all="ignore"):
            scale = np.nanmax(np.abs(e0)) if inc.any() else 1.0
            assert_close(new["m0"], e0, atol=1e-12 * scale, what="m0")
            assert_close(new["m1"], e1, atol=1e-9 * 500.0 * nz, what="m1")
            okm = np.isfinite(e2) & (np.abs(e0) > 1e-3 * scale)
            assert np.array_equal(np.isnan(new["m2"]), np.isnan(e2))
            assert np.all(np.abs(new["m2"][okm] - e2[okm]) <= 1e-8 * (500.0 * nz) ** 2)


@pytest.mark.parametrize("mask_kind", ["bench mask", "70 % random + isfinite + (lo, hi]"])
def test_mask_first_extrema_are_bit_identical(gpu, monkeypatch, mask_kind):
    """the extrema form of the kernel (argmax, argmin, vmax, vmin beside the sums and the count)"""
    shape = (77, 13, 52)
    want = ("m0", "m1", "m2", "nvalid", "argmax", "argmin", "vmax", "vmin")
    d, zeroed, arr, flags, lo, hi = _case(shape, mask_kind)
    spec = ops.MaskSpec(flags | _lib.MASK_ARRAY, lo, hi, DeviceArray.from_numpy(arr.astype(np.uint8)))
    old = _maps(monkeypatch, "0", DeviceArray.from_numpy(d), spec, shape[0], want)
    new = _maps(monkeypatch, "1", DeviceArray.from_numpy(d), spec, shape[0], want)
    _same(new, old, "switch 1 against switch 0")
    _same(_maps(monkeypatch, "1", DeviceArray.from_numpy(zeroed), spec, shape[0], want), new, "poisoned voxels zeroed")
    inc = arr & ~np.isnan(d)
    if flags:
        inc &= np.isfinite(d) & (np.nan_to_num(d) > np.float32(lo)) & (np.nan_to_num(d) <= np.float32(hi))
    assert np.array_equal(new["argmax"], O.argmax(d, inc)) and np.array_equal(new["argmin"], O.argmin(d, inc))


def test_mask_first_on_row_views(gpu, monkeypatch):
    """rows 3..10 of a taller cube and mask: the plane stride is not ny * nx.  nx = 52 keeps every row of the views 16-byte
    (cube) and 4-byte (mask) aligned, so the launch is the 16-byte lane form, the one the switch selects between"""
    shape = (77, 14, 52)
    want = ("m0", "m1", "m2", "nvalid")
    d, zeroed, arr, flags, lo, hi = _case(shape, "bench mask")
    dmask = DeviceArray.from_numpy(arr.astype(np.uint8))
    spec = ops.MaskSpec(_lib.MASK_ARRAY, array=dmask.rows(3, 11))
    dcube, dzero = DeviceArray.from_numpy(d), DeviceArray.from_numpy(zeroed)
    old = _maps(monkeypatch, "0", dcube.rows(3, 11), spec, shape[0], want)
    new = _maps(monkeypatch, "1", dcube.rows(3, 11), spec, shape[0], want)
    _same(new, old, "switch 1 against switch 0")
    _same(_maps(monkeypatch, "1", dzero.rows(3, 11), spec, shape[0], want), new, "poisoned voxels zeroed")
    # and the views are the rows they say: the contiguous copy of the same rows gives the same maps
    spec_c = ops.MaskSpec(_lib.MASK_ARRAY, array=DeviceArray.from_numpy(np.ascontiguousarray(arr[:, 3:11]).astype(np.uint8)))
    _same(_maps(monkeypatch, "1", DeviceArray.from_numpy(np.ascontiguousarray(d[:, 3:11])), spec_c, shape[0], want), new, "contiguous copy")
