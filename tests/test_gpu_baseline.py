"""GPU: polynomial baselines (csrc/spc_baseline.hip through ops.baseline_fit / ops.baseline_apply, baseline.fit_baseline,
SpectralCube.fit_baseline / subtract_baseline) against the numpy restatement of the kernels' rule and the np.linalg.lstsq
oracle (baseline_cases.py).

Nothing is tuned.  The unit is built WITHOUT contraction (-ffp-contract=off), so the restatement - the same float64
products, sums, divisions and casts in the same order - is held to EQUAL BITS: coefficients, counts, the difference and
the model, for float32 cubes too (the one rounding to float32 is the same).  Against the oracle: npts and the NaN pattern
equal, every fitted value finite, and the model at all channels within baseline_cases.bound on the spaxels whose Gram
matrix has kappa_2 <= 1e6 (test_baseline_host.py asserts that these are at least 98 % of the fitted spaxels of every case)."""
import numpy as np
import pytest

import baseline_cases as B
import dirty_memory
import views as V
from spectral_cube_amd import _lib, baseline, ops, Beam, SpectralCube, VaryingResolutionSpectralCube
from spectral_cube_amd.device import DeviceArray
from test_baseline_host import HDR, check_model

pytestmark = pytest.mark.gpu

DTYPES = (np.float32, np.float64)


def up(a):
    return a if isinstance(a, DeviceArray) else DeviceArray.from_numpy(np.ascontiguousarray(a))


def spec_of(kind, arr=None):
    """the MaskSpec of a case's mask"""
    if kind == "none":
        return None
    if kind == "bytes":
        return ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, up(arr))
    if kind == "finite":
        return ops.MaskSpec(_lib.MASK_FINITE, 0.0, 0.0, None)
    if kind == "gt":
        return ops.MaskSpec(_lib.MASK_GT, B.GT_THRESHOLD, 0.0, None)
    raise KeyError(kind)


def bytes_of(include, seed=0):
    b = B.BYTES[np.random.default_rng(seed).integers(0, len(B.BYTES), include.shape)]
    return np.where(include, b, 0).astype(np.uint8)


def fit(data, order, chan=None, mask=None, **kw):
    """(coef, npts) as host arrays, and the device coefficients"""
    d = up(data)
    coef, npts = ops.baseline_fit(d, order, channels=chan, mask_spec=mask, **kw)
    assert coef.shape == (order + 1,) + tuple(d.shape[1:]) and coef.dtype == np.float64
    assert npts.shape == tuple(d.shape[1:]) and npts.dtype == np.int32
    return coef.get(), npts.get(), coef


def apply(data, coef, subtract=True, **kw):
    d = up(data)
    out = ops.baseline_apply(d, up(coef), subtract=subtract, **kw)
    assert out.shape == d.shape and out.dtype == d.dtype
    return out.get()


def check(data, include, chan, order, mask, what, o=None, full_list=False):
    """the device on (data, mask, chan) against the restatement (bits: coefficients, counts, difference, model) and the
    oracle (the model within the bound); returns the device's host results"""
    d = up(data)
    nseg = ops.baseline_segments(data.shape, len(chan))
    coef, npts, dcoef = fit(d, order, None if full_list else chan, mask)
    ecoef, enpts = B.restate_fit(data, include, chan, order, nseg=nseg)
    assert np.array_equal(npts, enpts), (what, "npts")
    assert B.differing(coef, ecoef) == 0, (what, "coefficients against the restatement", B.differing(coef, ecoef))
    diff, model = apply(d, dcoef, True), apply(d, dcoef, False)
    assert B.differing(diff, B.restate_apply(data, ecoef, True)) == 0, (what, "difference against the restatement")
    assert B.differing(model, B.restate_apply(data, ecoef, False)) == 0, (what, "model against the restatement")
    if o is None:
        o = B.oracle(data, include, chan, order)
    worst = check_model(model, npts, None, o, order, what, dtype=data.dtype)
    # the difference: NaN where the sample is, v - model elsewhere, within the bound plus its own rounding
    exp = data.astype(np.float64) - o["model"]
    tol = B.toleranced(o, order)
    b = B.bound(o["npts"], order, o["kappa"], o["scale"], expected=exp, dtype=data.dtype)
    ok = np.isfinite(exp) & tol[None]
    with np.errstate(invalid="ignore"):                                  # (an infinite sample under MASK_FINITE: inf - inf)
        err = np.abs(diff.astype(np.float64) - exp)
    assert (err[ok] <= b[ok]).all(), (what, "difference against the oracle")
    assert np.array_equal(np.isnan(diff), np.isnan(data) | np.isnan(model)), (what, "NaN samples stay NaN")
    return dict(coef=coef, npts=npts, diff=diff, model=model, worst=worst)


# ---- the case table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("float32", "float64"))
@pytest.mark.parametrize("plane", B.PLANES, ids=lambda p: "%dx%d" % p)
def test_case_table_against_restatement_and_oracle(gpu, plane, dtype):
    worst, seen = 0.0, 0
    for key in B.case_ids():
        if key[0] != plane or key[3] != dtype:
            continue
        pl, nz, order, dt, mask, lst = key
        c = B.make_case(*key)
        o = B.case_oracle(*key)
        r = check(c["data"], c["include"], c["chan"], order, spec_of(*c["mask"]), key, o=o, full_list=len(c["chan"]) == nz)
        worst = max(worst, r["worst"])
        seen += 1
        if pl[0] * pl[1] >= 3:                              # n = 0, order, order + 1: NaN, NaN, finite
            n, cf = r["npts"].ravel(), r["coef"].reshape(order + 1, -1)
            assert (n[0], n[1], n[2]) == (0, order, order + 1), key
            assert np.isnan(cf[:, :2]).all() and np.isfinite(cf[:, 2]).all(), key
    assert seen == 21 * len(B.MASKS) * len(B.LISTS)
    print("plane %s %s: %d cases, largest error / bound %.3g" % (plane, dtype, seen, worst))


@pytest.mark.parametrize("dtype", DTYPES)
def test_order_equal_to_nz_gives_nan_coefficients_and_the_wrapper_refuses(gpu, dtype):
    rng = np.random.default_rng(1)
    for nz in (1, 3, 5):
        data = (5.0 + rng.standard_normal((nz, 2, 4))).astype(dtype)
        coef, npts, _ = fit(data, nz)
        assert coef.shape == (nz + 1, 2, 4) and np.isnan(coef).all() and (npts == nz).all()
        assert np.isnan(apply(data, coef)).all() and np.isnan(apply(data, coef, subtract=False)).all()
        with pytest.raises(ValueError, match="at least %d channels" % (nz + 1)):
            SpectralCube.read(data, dict(HDR)).fit_baseline(order=nz)


# ---- poison ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_poison_under_excluded_voxels_and_in_unlisted_channels_reaches_nothing(gpu, dtype):
    key = ((7, 9), 64, 3, np.dtype(dtype).name, "bytes", "ends")
    c = B.make_case(*key)
    clean, arr, chan, listed = np.array(c["data"]), c["mask"][1], c["chan"], c["listed"]
    hidden = (arr == 0) | ~listed[:, None, None]                     # excluded by the mask, or in no listed channel
    spec = spec_of("bytes", arr)
    big = np.finfo(dtype).max
    coef0, npts0, dc0 = fit(clean, 3, chan, spec)
    model0, diff0 = apply(clean, dc0, False), apply(clean, dc0, True)
    assert np.isfinite(coef0[:, 2:].reshape(4, -1)[:, 1:]).any()
    for poison in (np.nan, np.inf, -np.inf, big, -big):
        bad = clean.copy()
        bad[hidden] = poison
        coef, npts, dc = fit(bad, 3, chan, spec)
        assert B.same_bits(coef, coef0) and B.same_bits(npts, npts0), poison
        assert B.same_bits(apply(bad, dc, False), model0), poison
        assert B.same_bits(apply(bad, dc, True)[~hidden], diff0[~hidden]), poison
    # the predicate masks: the excluded samples ARE the poison (non-finite under MASK_FINITE, below the threshold under GT)
    for mask in ("finite", "gt"):
        k2 = ((7, 9), 64, 3, np.dtype(dtype).name, mask, "ends")
        c2 = B.make_case(*k2)
        check(c2["data"], c2["include"], c2["chan"], 3, spec_of(mask), k2, o=B.case_oracle(*k2))


# ---- views, dirty memory, determinism -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_strided_offset_and_misaligned_views(gpu, dtype):
    d, m = V.data(np.dtype(dtype), pedestal=5.0)
    order = 2
    for cname in V.CUBE_LAYOUTS:
        lay = V.layout(cname)
        dc, mc = V.crop(d, lay), V.crop(m, lay)
        nz = dc.shape[0]
        chan = B.channel_list("ends", nz, order)
        cube, cparent = V.upload(lay, dc, V.CUBE_POISON[np.dtype(dtype)])
        ecoef = None
        for mname in V.MASK_LAYOUTS:
            marr, mparent = V.upload(V.mask_layout(mname, lay), mc, 1)
            coef, npts, dcoef = fit(cube, order, chan, ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, marr))
            if ecoef is None:
                ecoef, enpts = B.restate_fit(dc, mc != 0, chan, order)
            assert B.differing(coef, ecoef) == 0 and np.array_equal(npts, enpts), (cname, mname)
        for oname in V.OUT_LAYOUTS:
            if dc.shape[2] % 4 and oname != "contig":
                continue                                                  # (the windows are laid out for nx a multiple of 4)
            olay = V.layout(oname, dc.shape)
            for subtract in (True, False):
                out, oparent = V.output(olay, dtype)
                ops.baseline_apply(cube, dcoef, subtract=subtract, out=out)
                got, untouched = V.read_output(olay, oparent)
                assert untouched, (cname, oname, "written outside the view")
                assert B.differing(got, B.restate_apply(dc, ecoef, subtract)) == 0, (cname, oname, subtract)
    whole = up(np.array(V.crop(d, V.layout(V.CUBE_LAYOUTS[-1]))))
    with pytest.raises(_lib.HipInvalidArgument, match="d_out overlaps the cube"):
        ops.baseline_apply(whole, dcoef, out=whole)


@pytest.mark.parametrize("dtype", DTYPES)
def test_dirty_and_recycled_memory_and_two_calls_agree(gpu, dtype):
    rng = np.random.default_rng(5)
    for shape, order in (((37, 7, 9), 3), ((200, 7, 9), 2)):             # one segment; three, through the workspace
        data = (5.0 + rng.standard_normal(shape)).astype(dtype)
        inc = rng.random(shape) < 0.6
        d, spec = up(data), ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, up(bytes_of(inc)))
        assert ops.baseline_segments(shape, shape[0]) == (1 if shape[0] == 37 else 3)

        def once():
            coef, npts, dc = fit(d, order, None, spec)
            return {"coef": coef, "npts": npts, "diff": apply(d, dc, True), "model": apply(d, dc, False)}
        first = dirty_memory.same_under_every_pattern(once)
        again = once()
        for name in first:
            assert B.same_bits(first[name], again[name]), name
        # outputs and workspace the caller pre-filled with 0xFF bytes
        need = int(_lib.load().spc_baseline_workspace_bytes(shape[0], shape[1], shape[2], shape[0], order))
        ff = lambda shp, dt: DeviceArray.from_numpy(np.frombuffer(b"\xff" * (int(np.prod(shp)) * np.dtype(dt).itemsize), dt).reshape(shp))  # noqa: E731
        coef, npts, ws = ff((order + 1,) + shape[1:], np.float64), ff(shape[1:], np.int32), ff((max(need, 1),), np.uint8)
        out = ff(shape, dtype)
        ops.baseline_fit(d, order, mask_spec=spec, coef=coef, npts=npts, workspace=ws)
        ops.baseline_apply(d, coef, out=out)
        assert B.same_bits(coef.get(), first["coef"]) and B.same_bits(npts.get(), first["npts"]) and B.same_bits(out.get(), first["diff"])
        ecoef, enpts = B.restate_fit(data, inc, np.arange(shape[0]), order, nseg=ops.baseline_segments(shape, shape[0]))
        assert B.differing(first["coef"], ecoef) == 0 and np.array_equal(first["npts"], enpts)


# ---- launches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ((3, 1, 70001), (3, 70001, 1), (70001, 1, 3)), ids=lambda s: "x".join(map(str, s)))
def test_axes_longer_than_a_launch_grid(gpu, shape):
    rng = np.random.default_rng(7)
    nz = shape[0]
    t = B.abscissa(nz)[:, None, None]
    data = (3.0 + 2.0 * t - t * t + 0.01 * rng.standard_normal(shape)).astype(np.float32)
    data[rng.random(shape) < 0.1] = np.nan
    chan = np.arange(nz)
    nseg = ops.baseline_segments(shape, nz)
    assert nseg == (64 if nz > 3 else 1)
    d = up(data)
    for order in (1, 2):
        coef, npts, dcoef = fit(d, order)
        ecoef, enpts = B.restate_fit(data, None, chan, order, nseg=nseg)
        assert np.array_equal(npts, enpts) and B.differing(coef, ecoef) == 0, order
        assert B.differing(apply(d, dcoef, True), B.restate_apply(data, ecoef, True)) == 0, order
        if nz > 3:                                                       # three spectra: the oracle too
            o = B.oracle(data, None, chan, order)
            check_model(apply(d, dcoef, False), npts, None, o, order, (shape, order), dtype=np.float32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_segmented_path_on_both_sides_of_the_rule(gpu, dtype):
    rng = np.random.default_rng(9)
    for nz, nseg in ((127, 1), (128, 2), (200, 3)):                      # 200: segments of 67, 67 and 66
        shape = (nz, 7, 9)
        assert ops.baseline_segments(shape, nz) == nseg
        t = B.abscissa(nz)[:, None, None]
        data = (4.0 - t + 0.5 * t ** 3 + 0.05 * rng.standard_normal(shape)).astype(dtype)
        inc = rng.random(shape) < 0.5
        for order in (0, 3, 5):
            check(data, inc, np.arange(nz), order, ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, up(bytes_of(inc, nz))), (nz, order),
                  full_list=True)
    # a list short enough for one segment on a long axis, and one cut in two with a shorter last segment
    shape = (300, 7, 9)
    data = (4.0 + rng.standard_normal(shape)).astype(dtype)
    for chan in (np.arange(0, 300, 3), np.concatenate([np.arange(70), np.arange(211, 300)])):
        assert ops.baseline_segments(shape, len(chan)) == (1 if len(chan) == 100 else 2)
        check(data, None, chan, 2, None, ("list", len(chan)))


# ---- far from zero ----------------------------------------------------------------------------------------------------------
def test_far_from_zero_float32(gpu):
    nz = 64
    k = np.arange(nz, dtype=np.float64)
    win = (k >= 24) & (k < 40)
    spec = 1000.0 + 1e-3 * k / nz + np.where(win, 1.0, 0.0)
    data = np.repeat(spec[:, None, None], 6, axis=2).astype(np.float32)
    chan = np.flatnonzero(~win)
    r = check(data, None, chan, 1, None, "far from zero")                # slope and level: the model within the bound
    o = B.oracle(data, None, chan, 1)
    assert o["kappa"].max() < 12
    exp = data.astype(np.float64) - o["model"]
    b = B.bound(o["npts"], 1, o["kappa"], o["scale"], expected=exp, dtype=np.float32)
    assert b.max() < 1e-7                                                # (a float32 step at 1000 is 6e-5: the bound is not slack)
    resid = r["diff"].astype(np.float64)
    assert (np.abs(resid - exp)[~win] <= b[~win]).all()
    # the samples are within half a float32 step, h = 2^-15, of the exact line: the fit of the rounded samples is off the
    # exact line by at most sqrt(m kappa) h at any channel (see test_quadratic_baseline_under_a_gaussian_line), the model's
    # own rounding to float32 adds h: level and slope are recovered to that, the residual outside the window to one h more
    h = 2.0 ** -15
    off = np.sqrt(2 * o["kappa"].max()) * h + h
    truth = (1000.0 + 1e-3 * k / nz)[:, None, None]
    assert np.abs(r["model"].astype(np.float64) - truth).max() <= off
    assert np.abs(resid[~win]).max() <= off + h


# ---- apply ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_apply_modes_nan_and_masked_voxels(gpu, dtype):
    rng = np.random.default_rng(13)
    shape, order = (9, 3, 5), 2
    data = (2.0 + rng.standard_normal(shape)).astype(dtype)
    data[4, 1, 2] = np.nan                                               # a NaN sample
    inc = np.ones(shape, bool)
    inc[:, 0, 0] = False                                                 # a spectrum the mask excludes entirely: NaN coefficients
    inc[2:5, 2, 3] = False                                               # masked voxels of a fitted spectrum
    coef, npts, dcoef = fit(data, order, None, ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, up(bytes_of(inc))))
    assert np.isnan(coef[:, 0, 0]).all() and npts[0, 0] == 0 and npts[2, 3] == 6 and npts[1, 2] == 8
    diff, model = apply(data, dcoef, True), apply(data, dcoef, False)
    assert diff.dtype == model.dtype == np.dtype(dtype)
    assert np.isnan(diff[:, 0, 0]).all() and np.isnan(model[:, 0, 0]).all()
    assert np.isnan(diff[4, 1, 2]) and np.isfinite(model[4, 1, 2])        # the model does not read the samples
    rest = np.ones(shape, bool)
    rest[:, 0, 0] = False
    rest[4, 1, 2] = False
    assert np.isfinite(diff[rest]).all() and np.isfinite(model[rest]).all()
    # masked voxels are subtracted like any other: diff + model gives the sample back to rounding
    back = diff[2:5, 2, 3].astype(np.float64) + model[2:5, 2, 3].astype(np.float64)
    eps = np.finfo(dtype).eps
    assert (np.abs(back - data[2:5, 2, 3]) <= 2 * eps * (np.abs(model[2:5, 2, 3]) + np.abs(data[2:5, 2, 3]))).all()
    assert B.differing(diff, B.restate_apply(data, coef, True)) == 0 and B.differing(model, B.restate_apply(data, coef, False)) == 0


# ---- the public layer -------------------------------------------------------------------------------------------------------
def test_order_zero_against_cube_minus_its_mean(gpu):
    rng = np.random.default_rng(17)
    shape = (37, 7, 9)
    data = 5.0 + rng.standard_normal(shape)
    data[rng.random(shape) < 0.05] = np.nan
    cube = SpectralCube.read(data, dict(HDR))
    got = np.asarray(cube.subtract_baseline(0).filled_data, np.float64)
    route = np.asarray((cube - cube.mean(axis=0)).filled_data, np.float64)
    assert got.dtype == route.dtype == np.float64
    o = B.oracle(data, None, np.arange(37), 0)
    exp = data - o["model"]
    # each route is within the bound of the exact least-squares answer (the mean is one sum of n terms and a division, the
    # difference one rounding: less than the bound allows the fit), so they are within twice the bound of each other
    b = B.bound(o["npts"], 0, o["kappa"], o["scale"], expected=exp, dtype=np.float64)
    fin = np.isfinite(exp)
    assert np.array_equal(np.isnan(got), np.isnan(route)) and np.array_equal(np.isnan(got), ~fin)
    assert (np.abs(got - exp)[fin] <= b[fin]).all() and (np.abs(got - route)[fin] <= 2 * b[fin]).all()


def test_quadratic_baseline_under_a_gaussian_line(gpu):
    nz, ny, nx, order = 64, 4, 5, 2
    rng = np.random.default_rng(19)
    k = np.arange(nz, dtype=np.float64)[:, None, None]
    amp = rng.uniform(0.5, 2.0, (1, ny, nx))
    quad = 3.0 + 0.05 * k - 4e-4 * k * k * rng.uniform(0.5, 1.5, (1, ny, nx))
    line = amp * np.exp(-0.5 * ((k - 30.0) / 1.5) ** 2)
    win = (k[:, 0, 0] >= 12) & (k[:, 0, 0] <= 48)                        # 12 sigma either side: the line is 0 outside
    assert line[~win].max() < 1e-30
    data = quad + line
    cube = SpectralCube.read(data, dict(HDR))
    axis = np.asarray(cube.spectral_axis, np.float64)
    dv = abs(float(HDR["CDELT3"]))
    fitres = cube.fit_baseline(order=order, exclude=[(axis[12], axis[48])])
    assert fitres.channels.tolist() == np.flatnonzero(~win).tolist() and fitres.order == order
    flat = fitres.subtract()
    got = np.asarray(flat.filled_data, np.float64)
    o = B.oracle(data, None, np.flatnonzero(~win), order)
    exp = data - o["model"]
    b = B.bound(o["npts"], order, o["kappa"], o["scale"], expected=exp, dtype=np.float64)
    assert (np.abs(got - exp) <= b).all()                                # the residual, outside the window and inside
    # the oracle fits ROUNDED samples (r_k <= u |data|): its model is off the exact quadratic by at most
    # sqrt(m kappa) u max|data| at any channel (||dc||_2 <= ||r||_2 / sigma_min(A), sigma_min^2 = lambda_min(G) >= n / kappa)
    m = order + 1
    off = np.sqrt(m * o["kappa"].max()) * B.U * np.abs(data).max()
    assert np.abs(o["model"] - quad).max() <= off
    assert np.abs(got[~win]).max() <= b.max() + off + B.U * np.abs(data).max()
    # moment 0 of the result is the line's own sum: nz channels, each off by at most the bound, the oracle's offset and
    # the rounding of the sample, times the channel width; plus the moment's own sum of nz terms
    m0 = np.asarray(flat.moment0(), np.float64)
    analytic = line.sum(axis=0) * dv
    tol = nz * dv * (b.max() + off + B.U * np.abs(data).max()) + (nz + 2) * B.U * np.abs(got).sum(axis=0).max() * dv
    assert m0.shape == (ny, nx) and (np.abs(m0 - analytic) <= tol).all(), (float(np.abs(m0 - analytic).max()), float(tol))
    assert tol < 1e-9 * analytic.min()                                   # (the tolerance says something: the sums are 1 to 8)
    # model(), continuum(), legendre(), polynomial()
    model = np.asarray(fitres.model().filled_data, np.float64)
    assert (np.abs(model - o["model"]) <= B.bound(o["npts"], order, o["kappa"], o["scale"])).all()
    leg = fitres.legendre()
    assert leg.shape == (m, ny, nx) and np.allclose(leg, o["coef"], rtol=1e-9)
    poly = fitres.polynomial()
    assert np.allclose(poly[0], 3.0, atol=1e-9) and np.allclose(poly[1], 0.05, atol=1e-9)
    cen = fitres.continuum()                                             # the band centre, channel 31.5
    q2 = (3.0 + 0.05 * k - quad)[1] / 1.0                                # the quadratic coefficient of every spaxel
    assert cen.shape == (ny, nx) and cen.unit == "K" and np.allclose(np.asarray(cen), 3.0 + 0.05 * 31.5 - q2 * 31.5 ** 2, atol=1e-9)
    assert np.allclose(np.asarray(fitres.continuum(10)), quad[10], atol=1e-9)
    same = cube.subtract_baseline(order=order, exclude=[(axis[12], axis[48])])
    assert B.same_bits(np.asarray(same.filled_data), np.asarray(flat.filled_data))
    import spectral_cube_amd as S
    assert B.same_bits(np.asarray(S.subtract_baseline(cube, order, channels=~win).filled_data), np.asarray(flat.filled_data))


def test_fit_mask_pending_arithmetic_and_what_the_result_carries(gpu):
    rng = np.random.default_rng(23)
    nz, ny, nx = 16, 5, 6
    k = np.arange(nz, dtype=np.float32)[:, None, None]
    data = (1.0 + 0.1 * k + 0.01 * rng.standard_normal((nz, ny, nx))).astype(np.float32)
    data[6:9] += 5.0                                                     # the line
    beams = [Beam((3 + 0.1 * i) * 1e-3) for i in range(nz)]
    own = rng.random((nz, ny, nx)) < 0.8
    vr = VaryingResolutionSpectralCube(data, header=dict(HDR), beams=beams).with_mask(own)
    signal = vr > 4.0
    fitres = vr.fit_baseline(order=1, fit_mask=~signal)
    npts = fitres.npts
    inc = own & ~(data > 4.0)
    assert npts.dtype == np.int32 and npts.shape == (ny, nx) and np.array_equal(np.asarray(npts), inc.sum(axis=0))
    assert type(npts).__name__ == "Projection" and npts.unit == "" and npts.meta["baseline_order"] == 1
    ecoef, enpts = B.restate_fit(data, inc, np.arange(nz), 1)
    assert B.differing(fitres.legendre(), ecoef) == 0
    for out, subtract in ((fitres.subtract(), True), (fitres.model(), False), (vr.subtract_baseline(1, fit_mask=~signal), True)):
        assert isinstance(out, VaryingResolutionSpectralCube) and out.unmasked_beams == beams
        assert out.unit == "K" and out.shape == vr.shape and out.header["CTYPE3"] == "VRAD" and out.meta == vr.meta
        assert np.array_equal(out.get_mask_array(), own)                 # the cube's own mask, not the fit mask
        assert B.differing(np.asarray(out.unmasked_data), B.restate_apply(data, ecoef, subtract)) == 0
    # pending arithmetic is materialised first
    plain = SpectralCube.read(data, dict(HDR, BMAJ=6e-3, BMIN=6e-3, BPA=0.0))
    shifted = plain * 3.0 / 7.0
    got = shifted.subtract_baseline(1, channels=[0, 1, 2, 3, 12, 13, 14, 15])
    twice = (data * np.float32(3.0) / np.float32(7.0)).astype(np.float32)
    c2, _ = B.restate_fit(twice, None, [0, 1, 2, 3, 12, 13, 14, 15], 1)
    assert B.differing(np.asarray(got.unmasked_data), B.restate_apply(twice, c2, True)) == 0
    assert got.beam == plain.beam and plain.beam is not None
    assert isinstance(fitres, baseline.BaselineFit)
