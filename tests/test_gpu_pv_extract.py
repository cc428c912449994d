"""GPU: position-velocity diagrams (csrc/spc_pv_extract.hip through ops.pv_extract, pvextract.extract_pv_slice,
SpectralCube.pv_slice) against the scipy oracle and the numpy restatement of the kernel's rule (pv_cases.py).

Nothing is tuned.  Order 0 copies samples: EQUAL to the oracle.  Order 1: the NaN pattern and the count are EQUAL to the
oracle's, and every finite value lies within pv_cases.bound of it - derived there from float64 rounding:

    b = (12 + 2 n) U S + 4 U V,   U = 2^-53, n lines,
    S = the mean over the counted lines of sum |w_i v_i|, V = that of sum |v_i| over the neighbours read,

8 U S for the device's line (3 roundings in a weight, 1 in the product, 3 additions, second order), 4 U S + 4 U V for
scipy's (its products and additions; its second weight along an axis is the remainder 1 - (1 - fx), off by up to U
absolute), 2 n U S for the two means over the lines; a float32 cube adds one rounding of the result, 2^-24 (|expected| + b).
Against the restatement, which performs the same float64 operations in the same order (the unit is built without fused
multiply-adds), the result is EQUAL bit for bit, for float32 cubes too: the one rounding to float32 is the same."""
import math

import numpy as np
import pytest

import dirty_memory
import pv_cases as P
import views as V
from spectral_cube_amd import _lib, ops, Beam, SpectralCube, VaryingResolutionSpectralCube
from spectral_cube_amd.device import DeviceArray
from spectral_cube_amd.pvextract import Path, extract_pv_slice
from test_pv_extract_host import check_against_oracle, same_bits

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)
ODD_BYTES = np.array([1, 2, 0x80, 0xFF, 37, 254], np.uint8)          # any non-zero byte includes


def spec_of(include, seed=0):
    """a MaskSpec whose uint8 array holds bytes other than 0 / 1 where *include* is set"""
    b = ODD_BYTES[np.random.default_rng(seed).integers(0, len(ODD_BYTES), include.shape)]
    return ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, DeviceArray.from_numpy(np.where(include, b, 0).astype(np.uint8)))


def run(data, xs, ys, order=1, respect_nan=True, mask=None, fill=np.nan, want_count=True, **kw):
    """(diagram, count) as host arrays; *data* a host array (uploaded) or a DeviceArray"""
    d = data if isinstance(data, DeviceArray) else DeviceArray.from_numpy(np.ascontiguousarray(data))
    npts = np.atleast_2d(xs).shape[-1]
    count = DeviceArray((d.shape[0], npts), np.int32, d.device) if want_count else None
    out = ops.pv_extract(d, xs, ys, order=order, respect_nan=respect_nan, mask_spec=mask, fill=fill, count=count, **kw)
    assert out.shape == (d.shape[0], npts) and out.dtype == d.dtype
    return out.get(), count.get() if want_count else None


def check(data, include, xs, ys, order, respect_nan, what, fill=np.nan, mask=None):
    """the device on (data, include) against the restatement (bits) and the oracle (pv_cases.bound)"""
    dtype = data.dtype
    if mask is None and include is not None:
        mask = spec_of(include)
    got, count = run(data, xs, ys, order, respect_nan, mask=mask, fill=fill)
    f = P.filled(data, include, fill)
    exp, ecount, scale = P.restate(f, xs, ys, order, respect_nan)
    assert same_bits(got, exp), (what, "restatement", np.argwhere(~((got == exp) | (np.isnan(got) & np.isnan(exp))))[:4].tolist())
    assert np.array_equal(count, ecount), (what, "count against the restatement")
    check_against_oracle(got, count, scale, f, xs, ys, order, respect_nan, dtype, what)
    return got


# ---- the case table: planes 2x2, 1x5, 7x9; nz 1, 2, 7, 37; npts 1, 63, 64, 65, 130; nlines 1, 2, 5 ------------------------
@pytest.mark.parametrize("order", (0, 1))
@pytest.mark.parametrize("dtype", DTYPES)
def test_case_table(gpu, dtype, order):
    for cid, plane, nz, npts, nlines in P.cases():
        shape = (nz,) + plane
        xs, ys = P.points(plane, npts, nlines)
        for respect_nan in (True, False):
            check(P.cube(shape, dtype), None, xs, ys, order, respect_nan, (cid, "no mask", respect_nan))
            check(P.cube(shape, dtype), P.include(shape), xs, ys, order, respect_nan, (cid, "mask", respect_nan))


@pytest.mark.parametrize("dtype", DTYPES)
def test_leaving_and_re_entering_zero_weight_holes_and_a_line_outside(gpu, dtype):
    for order in (0, 1):
        xs, ys = P.zigzag((7, 9), 130)
        got = check(P.cube((7, 7, 9), dtype), None, xs, ys, order, True, ("zigzag", order))
        inside = (xs[0] >= 0) & (xs[0] <= 8) & (ys[0] >= 0) & (ys[0] <= 6)
        assert np.isnan(got[:, ~inside]).all() and (~inside).sum() > 20
        d, xs, ys = P.zero_weight_holes((2, 5, 6), dtype)
        got = check(d, None, xs, ys, order, True, ("holes", order))
        on = (xs[0] % 1 == 0) & (ys[0] % 1 == 0) & ((xs[0] + ys[0]) % 2 == 0)
        assert same_bits(got[:, on], d[:, ys[0][on].astype(int), xs[0][on].astype(int)]), "NaN neighbours of weight 0 do not count"
        # every line outside: count 0, NaN
        xs, ys = np.full((2, 65), 9.0 + 1e-9), np.tile(np.linspace(0, 6, 65), (2, 1))
        got, count = run(P.cube((7, 7, 9), dtype), xs, ys, order)
        assert np.isnan(got).all() and not count.any()


# ---- both grid dimensions past 65535 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_a_path_of_70000_points_and_a_cube_of_70000_channels(gpu, dtype):
    rng = np.random.default_rng(5)
    d = rng.standard_normal((2, 3, 70001)).astype(dtype)
    d[rng.random(d.shape) < 0.05] = np.nan
    p = Path([(0.0, 0.25), (70000.0, 1.75)], width=2)
    xs, ys = p.sample_lines(70000.0 / 69999.0)
    assert xs.shape == (2, 70000)
    for order in (0, 1):
        check(d, None, xs, ys, order, True, ("70000 points", order))
    d = rng.standard_normal((70000, 2, 2)).astype(dtype)
    d[rng.random(d.shape) < 0.05] = np.nan
    inc = rng.random(d.shape) < 0.8
    xs, ys = np.array([[0.0, 0.5, 1.0]]), np.array([[0.25, 1.0, 0.0]])
    for order in (0, 1):
        got, count = run(d, xs, ys, order, mask=spec_of(inc))
        exp, ecount, scale = P.restate(P.filled(d, inc), xs, ys, order, True)
        assert same_bits(got, exp) and np.array_equal(count, ecount), ("70000 channels", order)
        some = np.r_[0:40, 32760:32800, 65520:65560, 69960:70000]                 # scipy runs channel by channel
        check_against_oracle(got[some], count[some], (scale[0][some], scale[1][some]), P.filled(d, inc)[some], xs, ys, order, True,
                             dtype, ("70000 channels", order))


# ---- masks ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_mask_terms_fill_values_and_count(gpu, dtype):
    shape = (7, 7, 9)
    d, inc = P.cube(shape, dtype), P.include(shape)
    xs, ys = P.points((7, 9), 130, 2, seed=3)
    xs[-1], ys[-1] = P.points((7, 9), 130, 1, seed=4)                              # (both lines inside: counts of 0, 1 and 2)
    for order in (0, 1):
        for fill in (np.nan, -5.0, 0.0):
            for respect_nan in (True, False):
                check(d, inc, xs, ys, order, respect_nan, ("array", order, fill), fill=fill)
        # a predicate term: data > 0.1 and finite, alone and with the array
        thr = 0.1
        pred = _lib.MASK_GT | _lib.MASK_FINITE
        with np.errstate(invalid="ignore"):
            keep = d > dtype(thr) if dtype == np.float32 else d > thr
        check(d, keep, xs, ys, order, True, ("predicate", order), fill=-1.0, mask=ops.MaskSpec(pred, thr, 0.0, None))
        both = spec_of(inc)
        both.flags |= pred
        both.thr_lo = thr
        check(d, keep & inc, xs, ys, order, True, ("predicate and array", order), fill=2.5, mask=both)
        # nan_excluded: a NaN sample counts as excluded and takes the fill value
        got, _ = run(d, xs, ys, order, mask=spec_of(inc), fill=7.0, nan_excluded=True)
        exp, _, _ = P.restate(P.filled(d, inc & ~np.isnan(d), 7.0), xs, ys, order, True)
        assert same_bits(got, exp)


@pytest.mark.parametrize("dtype", DTYPES)
def test_poison_under_excluded_voxels_does_not_reach_the_output(gpu, dtype):
    shape = (7, 7, 9)
    inc = P.include(shape, frac=0.6)
    clean = np.array(P.cube(shape, dtype, nan_frac=0.0))
    xs, ys = P.points((7, 9), 130, 2, seed=9)
    xs[-1], ys[-1] = P.points((7, 9), 130, 1, seed=10)
    for poison in (1e30, np.inf, -np.inf, np.nan):
        bad = clean.copy()
        bad[~inc] = poison
        zero = clean.copy()
        zero[~inc] = 0
        for order in (0, 1):
            for fill in (np.nan, 0.0):
                a, ca = run(bad, xs, ys, order, mask=spec_of(inc), fill=fill)
                b, cb = run(zero, xs, ys, order, mask=spec_of(inc), fill=fill)
                assert same_bits(a, b) and np.array_equal(ca, cb), (poison, order, fill)
                assert np.isfinite(a[~np.isnan(a)]).all() and (np.abs(a[~np.isnan(a)]) < 1e3).all()


# ---- views, dirty memory, determinism ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_offset_and_misaligned_views(gpu, dtype):
    d, m = V.data(np.dtype(dtype))
    nz, ny, nx = V.BASE
    p = Path([(1.5, 0.0), (nx - 1.0, ny - 1.0), (3.25, 2.5)], width=3)
    xs, ys = p.sample_lines(1.0)
    for cname in V.CUBE_LAYOUTS:
        lay = V.layout(cname)
        dc, mc = V.crop(d, lay), V.crop(m, lay)
        cube, cparent = V.upload(lay, dc, V.CUBE_POISON[np.dtype(dtype)])
        for mname in V.MASK_LAYOUTS:
            mlay = V.mask_layout(mname, lay)
            marr, mparent = V.upload(mlay, mc, 1)
            spec = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, marr)
            for order in (0, 1):
                got, count = run(cube, xs, ys, order, mask=spec, fill=-3.0)
                exp, ecount, _ = P.restate(P.filled(dc, mc != 0, -3.0), xs, ys, order, True)
                assert same_bits(got, exp) and np.array_equal(count, ecount), (cname, mname, order)
    # an output and a count that are windows of wider arrays: nothing outside them is written
    npts = xs.shape[1]
    for dt, name in ((dtype, "out"), (np.int32, "count")):
        parent = DeviceArray.from_numpy(np.full((nz, npts + 7), V.out_poison(dt), dt))
        view = DeviceArray((nz, npts), dt, ptr=parent.ptr + 3 * np.dtype(dt).itemsize, owner=parent)
        view.row_stride = npts + 7
        cube = DeviceArray.from_numpy(d)
        ops.pv_extract(cube, xs, ys, **{name: view})
        ref, rcount = run(d, xs, ys)
        host = parent.get()
        assert same_bits(host[:, 3:3 + npts], ref if name == "out" else rcount)
        rest = np.delete(host, np.s_[3:3 + npts], axis=1)
        assert rest.tobytes() == np.full(rest.shape, V.out_poison(dt), dt).tobytes()


@pytest.mark.parametrize("dtype", DTYPES)
def test_dirty_and_recycled_outputs_and_two_calls_agree(gpu, dtype):
    shape = (37, 7, 9)
    d, inc = DeviceArray.from_numpy(np.array(P.cube(shape, dtype))), P.include(shape)
    xs, ys = P.points((7, 9), 130, 5, seed=2)
    spec = spec_of(inc)
    for order in (0, 1):
        def once():
            got, count = run(d, xs, ys, order, mask=spec)
            return {"out": got, "count": count}
        first = dirty_memory.same_under_every_pattern(once)
        again = once()
        assert same_bits(first["out"], again["out"]) and np.array_equal(first["count"], again["count"])
        exp, ecount, _ = P.restate(P.filled(np.array(P.cube(shape, dtype)), inc), xs, ys, order, True)
        assert same_bits(first["out"], exp) and np.array_equal(first["count"], ecount)


# ---- the public layer ---------------------------------------------------------------------------------------------------------
def cube_of(data, include=None, fill=None, hdr=P.HDR):
    c = SpectralCube.read(data, dict(hdr) if hdr is not None else None)
    if include is not None:
        c = c.with_mask(np.asarray(include, bool))
    return c if fill is None else c.with_fill_value(fill)


@pytest.mark.parametrize("dtype", DTYPES)
def test_axis_aligned_cuts_are_filled_data(gpu, dtype):
    shape = (7, 7, 9)
    d, inc = np.array(P.cube(shape, dtype)), P.include(shape)
    for include, fill in ((None, None), (inc, None), (inc, -5.0), (inc, 0.0)):
        cube = cube_of(d, include, fill)
        f = np.asarray(cube.filled_data)
        assert f.dtype == dtype
        for j in (0, 3, 6, -1, -7):
            got = cube.pv_slice(y=j)
            assert got.shape == (7, 9) and same_bits(np.asarray(got), f[:, j, :]), ("y", j, fill)
        for i in (0, 4, 8, -1, -9):
            got = cube.pv_slice(x=i)
            assert got.shape == (7, 7) and same_bits(np.asarray(got), f[:, :, i]), ("x", i, fill)
        assert got.unit == "K" and got.meta["pv_order"] == 0 and got.header["CTYPE1"] == "OFFSET"
    thin = cube_of(np.ascontiguousarray(d[:, :, :1]), inc[:, :, :1])                      # one column: a row of one point
    assert same_bits(np.asarray(thin.pv_slice(y=2)), np.asarray(thin.filled_data)[:, 2, :])


@pytest.mark.parametrize("dtype", DTYPES)
def test_extract_pv_slice_and_cube_pv_slice(gpu, dtype):
    shape = (7, 7, 9)
    d, inc = np.array(P.cube(shape, dtype)), P.include(shape)
    cube = cube_of(d, inc)
    path = Path([(0.5, 0.25), (7.75, 5.5), (2.0, 6.0)], width=3)
    xs, ys = path.sample_lines(0.5)
    f = P.filled(d, inc)
    for order in (0, 1):
        for respect_nan in (True, False):
            got = extract_pv_slice(cube, path, spacing=0.5, order=order, respect_nan=respect_nan)
            exp, _, scale = P.restate(f, xs, ys, order, respect_nan)
            assert got.shape == (7, xs.shape[1]) and same_bits(np.asarray(got), exp)
            check_against_oracle(np.asarray(got), None, scale, f, xs, ys, order, respect_nan, dtype, ("public", order, respect_nan))
            assert same_bits(np.asarray(cube.pv_slice(path, spacing=0.5, order=order, respect_nan=respect_nan)), np.asarray(got))
    got = extract_pv_slice(cube, path, spacing=0.5)
    assert got.unit == "K" and got.dtype == dtype and got.beam is None
    assert got.meta["pv_path"] == [(0.5, 0.25), (7.75, 5.5), (2.0, 6.0)]
    assert (got.meta["pv_spacing"], got.meta["pv_width"], got.meta["pv_order"]) == (0.5, 3.0, 1)
    h = got.header
    assert (h["CTYPE1"], h["CRPIX1"], h["CRVAL1"], h["CDELT1"], h["CUNIT1"]) == ("OFFSET", 1.0, 0.0, 0.5 * math.sqrt(abs(-2e-3 * 2e-3)), "deg")
    assert (h["CTYPE2"], h["CRVAL2"], h["CDELT2"], h["CRPIX2"], h["CUNIT2"]) == ("VRAD", -16.0, 0.5, 1.0, "km/s")
    assert h["RESTFRQ"] == P.HDR["RESTFRQ"] and (h["NAXIS1"], h["NAXIS2"]) == (xs.shape[1], 7)
    # nlines, a plain list of points, a world-coordinate path equal to its pixel twin
    one = extract_pv_slice(cube, path, spacing=0.5, nlines=1)
    plain = extract_pv_slice(cube, [(0.5, 0.25), (7.75, 5.5), (2.0, 6.0)], spacing=0.5)
    assert same_bits(np.asarray(one), np.asarray(plain)) and plain.meta["pv_width"] is None
    lon, lat = cube.wcs.celestial_pix2world(path.points[:, 0], path.points[:, 1])
    world = Path.from_world(lon, lat, cube.wcs, width=3)
    assert np.abs(world.points - path.points).max() <= 1e-9
    twin = extract_pv_slice(cube, Path(world.points, width=3), spacing=0.5)
    assert same_bits(np.asarray(extract_pv_slice(cube, world, spacing=0.5)), np.asarray(twin))
    # without a WCS: no header, offsets in pixels
    bare = extract_pv_slice(cube_of(d, inc, hdr=None), path, spacing=0.5)
    assert bare.header == {} and bare.meta["pv_spacing"] == 0.5 and same_bits(np.asarray(bare), np.asarray(got))


def test_a_varying_resolution_cube_gives_no_beam_and_a_beam_is_kept(gpu):
    d = np.array(P.cube((3, 7, 9), np.float32))
    beams = [Beam(3 * 2e-3), Beam(4 * 2e-3), Beam(5 * 2e-3)]
    vr = VaryingResolutionSpectralCube(d, header=dict(P.HDR), beams=beams)
    got = vr.pv_slice([(0, 0), (8, 6)])
    assert got.beam is None and "beam" not in got.meta
    assert vr.pv_slice(y=1).beam is None
    one = SpectralCube.read(d, dict(P.HDR, BMAJ=6e-3, BMIN=6e-3, BPA=0.0))
    assert one.pv_slice([(0, 0), (8, 6)]).beam == one.beam and one.beam is not None
