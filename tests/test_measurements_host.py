"""CPU: the host side of the per-label measurements (spectral_cube_amd/measurements.py, ops.label_measure,
spc_label_measure_f32 / _f64): the arithmetic after the kernel - means, variances, centroids, dispersions, index handling,
the union of index None - held to scipy.ndimage through a numpy restatement of the kernel's tables, the catalogue against a
direct per-label loop, the C ABI and what ops hands to it.  No kernel runs here.

restate() below IS the specification of the tables (include/spcube_hip.h): test_gpu_measurements.py compares the device
with it.  Tolerances: U = 2^-53; a float64 sum of m terms t_i in any order is within (m - 1) U sum |t_i| of the exact sum
(and a term carries at most 3 roundings of its own), so two orders differ by at most sum_bound = 2 (m + 3) U sum |t_i|.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.ndimage as ndi

import labelling as R
from conftest import REPO
from spectral_cube_amd import _lib, labelling, measurements as MS, ops, SpectralCube
from test_labelling_host import HDR, P, _StandInArray

U = 2.0 ** -53
GROUPS = ("sums", "extrema", "first", "second")


# ---- the tables, restated in numpy --------------------------------------------------------------------------------------
def restate(data, include, labels, n, origin=None):
    """the raw tables of spc_label_measure (rows 0 ... n) of *data* under the bool *include* (None: all) through
    *labels*, about *origin* ((n + 1, 4): v0, z0, y0, x0; None: zero), every group; with them "abs_sums", "abs_first",
    "abs_second": the same sums of the terms' absolute values, which the error bounds are made of"""
    data, labels = np.asarray(data), np.asarray(labels)
    inc = np.ones(data.shape, bool) if include is None else np.asarray(include, bool)
    meas = (labels > 0) & inc & ~np.isnan(data)
    k = labels[meas].astype(np.int64)
    v = data[meas].astype(np.float64)
    z, y, x = (c.astype(np.float64) for c in np.nonzero(meas))
    pos = np.flatnonzero(meas)
    o = np.zeros((n + 1, 4)) if origin is None else np.asarray(origin, np.float64)
    dv, dz, dy, dx = v - o[k, 0], z - o[k, 1], y - o[k, 2], x - o[k, 3]

    def per_label(terms):
        with np.errstate(invalid="ignore"):
            return np.stack([np.bincount(k, weights=t, minlength=n + 1) for t in terms], axis=1).astype(np.float64)

    t = {"count": np.bincount(k, minlength=n + 1).astype(np.int64)}
    with np.errstate(invalid="ignore", over="ignore"):
        groups = {"sums": [dv, dv * dv], "first": [v, v * dz, v * dy, v * dx],
                  "second": [(v * dz) * dz, (v * dy) * dy, (v * dx) * dx, (v * dz) * dy, (v * dz) * dx, (v * dy) * dx]}
        for name, terms in groups.items():
            t[name] = per_label(terms)
            t["abs_" + name] = per_label([np.abs(q) for q in terms])
    vz = data[meas] + data.dtype.type(0)                               # -0.0 -> +0.0: the two compare equal
    for key, order in (("min", np.lexsort((pos, vz, k))), ("max", np.lexsort((pos, -vz, k)))):
        val, where = np.full(n + 1, np.nan, data.dtype), np.full(n + 1, -1, np.int64)
        ks = k[order]
        head = np.ones(ks.size, bool)
        head[1:] = ks[1:] != ks[:-1]                                   # the first of every label's sorted voxels
        val[ks[head]], where[ks[head]] = vz[order][head], pos[order][head]
        t[key], t[key + "_pos"] = val, where
    return t


def sum_bound(count, abs_sum):
    """|our sum - another order's| <= 2 (m + 3) U sum |t_i| (the module docstring)"""
    return 2.0 * (np.asarray(count, np.float64) + 3.0) * U * np.asarray(abs_sum, np.float64)


def measured_labels(data, include, labels):
    """the labels scipy is run with: 0 where a voxel is not measured"""
    inc = True if include is None else np.asarray(include, bool)
    return np.where(inc & ~np.isnan(data), labels, 0).astype(np.int32)


def filled(data, include):
    return np.where(True if include is None else include, data, data.dtype.type(0))


def field_case(x, structure, seed, dtype=np.float32, nan=0.03, excluded=0.2, offset=0.0):
    """(data, include, labels, n) on the bool field *x*: seeded noise with NaN samples and an include array"""
    rng = np.random.default_rng(7000 + seed)
    labels, n = R.scipy_label(x, structure)
    data = (offset + rng.normal(size=x.shape)).astype(dtype)
    data[rng.random(x.shape) < nan] = np.nan
    include = rng.random(x.shape) >= excluded
    return data, include, labels, n


def host_cases():
    """every 7th case of the labelling case table (all shapes, densities and kinds of structure come up)"""
    return [(cid, x, s, j) for j, (cid, x, s) in enumerate(R.cases()) if j % 7 == 0]


# ---- derivations against scipy ------------------------------------------------------------------------------------------
class FromTables:
    """the ten public quantities derived from raw tables: tables_of(origin) -> the tables of a pass about origin"""

    def __init__(self, tables_of, n, shape):
        self.of, self.n, self.shape, self.t = tables_of, n, shape, tables_of(None)

    def sum_labels(self, index):
        return MS.sum_from(self.t, index, self.n)

    def mean(self, index):
        return MS.mean_from(self.t, index, self.n)

    def variance(self, index):
        return MS.variance_from(self.of(MS.variance_origin(self.t, index, self.n)), index, self.n)

    def standard_deviation(self, index):
        return np.sqrt(self.variance(index))

    def minimum(self, index):
        return MS.extreme_from(self.t, index, self.n, False)

    def maximum(self, index):
        return MS.extreme_from(self.t, index, self.n, True)

    def minimum_position(self, index):
        return MS.position_from(self.t, index, self.n, self.shape, False)

    def maximum_position(self, index):
        return MS.position_from(self.t, index, self.n, self.shape, True)

    def extrema(self, index):
        return MS.extrema_from(self.t, index, self.n, self.shape)

    def center_of_mass(self, index):
        return MS.center_of_mass_from(self.t, index, self.n)


def check_against_scipy(Q, data, include, labels, n, index, what):
    """the ten public quantities of *Q* (FromTables, or the device's) for *index* against scipy.ndimage on the measured
    labels, within the bounds the restated tables give; labels without a measured voxel are left to
    test_empty_label_conventions"""
    lab2 = measured_labels(data, include, labels)
    d64 = filled(data, include).astype(np.float64)
    dnat = filled(data, include)
    cnt_all = np.bincount(lab2.ravel(), minlength=n + 1)
    t = restate(data, include, labels, n)
    scalar = index is None or np.ndim(index) == 0
    if index is None:
        if cnt_all[1:].sum() == 0:
            return
        live = None
    else:
        live = cnt_all[np.atleast_1d(index)] > 0
        if scalar and not live.all():
            return
    sel = (lambda a: np.asarray(a)) if scalar else (lambda a: np.asarray(a)[live])
    # what the bounds are made of, for the region(s) of index
    if index is None:
        m, asum = t["count"][1:].sum(), t["abs_sums"][1:, 0].sum()
    else:
        m, asum = t["count"][index], t["abs_sums"][index, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        bs = sum_bound(m, asum)
        got, exp = Q.sum_labels(index), ndi.sum_labels(d64, lab2, index)
        assert np.shape(got) == np.shape(exp) and (np.abs(sel(got) - sel(exp)) <= sel(bs)).all(), (what, "sum")
        got, exp = Q.mean(index), ndi.mean(d64, lab2, index)
        # the quotient: both divide sums within bs of each other by the same m, one rounding each
        bm = bs / m + 2 * U * np.abs(exp)
        assert np.shape(got) == np.shape(exp) and (np.abs(sel(got) - sel(exp)) <= sel(bm)).all(), (what, "mean")
        # variance: the second pass is about OUR means c, scipy sums (v - mu)^2 about its own mu, |mu - c| <= bm:
        # |sum (v - mu)^2 - sum (v - c)^2| <= 2 bm sum |v - c| + m bm^2; the subtractions v - c and v - mu round once each
        # (2 U of the square, each side: 4 U sum (v - c)^2); then the two orders of summation, and the quotient by m
        t2 = restate(data, include, labels, n, MS.variance_origin(t, index, n))
        if index is None:
            a1, a2 = t2["abs_sums"][1:, 0].sum(), t2["abs_sums"][1:, 1].sum()
        else:
            a1, a2 = t2["abs_sums"][index, 0], t2["abs_sums"][index, 1]
        got, exp = Q.variance(index), ndi.variance(d64, lab2, index)
        bv = (sum_bound(m, a2) + 4 * U * a2 + 2 * bm * a1 + m * bm * bm) / m + 2 * U * np.abs(exp)
        assert np.shape(got) == np.shape(exp) and (np.abs(sel(got) - sel(exp)) <= sel(bv)).all(), (what, "variance", got, exp, bv)
        # the square root: d sqrt(x) = dx / (2 sqrt(x)), with x >= exp - bv; one rounding
        got, exp_sd = Q.standard_deviation(index), np.sqrt(exp)
        bsd = bv / (2 * np.sqrt(np.maximum(exp - bv, 0.0))) + 2 * U * exp_sd
        ok_sd = sel(exp > 4 * bv)                                        # (a variance of 0: the root has no derivative)
        assert (np.abs(sel(got) - sel(exp_sd))[ok_sd] <= sel(bsd)[ok_sd]).all(), (what, "standard_deviation")
        # extrema and positions: equal
        pairs = ((Q.minimum, Q.minimum_position, ndi.minimum, ndi.minimum_position),
                 (Q.maximum, Q.maximum_position, ndi.maximum, ndi.maximum_position))
        ex = Q.extrema(index)
        for which, (fv, fp, sv, sp) in enumerate(pairs):
            got, exp = fv(index), sv(dnat, lab2, index)
            assert np.asarray(got).dtype == data.dtype and np.array_equal(sel(got), sel(exp)), (what, "extreme", which)
            assert np.array_equal(sel(ex[which]), sel(exp)), (what, "extrema", which)
            got, exp = fp(index), sp(dnat, lab2, index)
            assert ex[2 + which] == got, (what, "extrema positions", which)
            if scalar:
                assert got == tuple(int(c) for c in exp), (what, "position", which)
            else:
                assert isinstance(got, list) and len(got) == len(exp)
                assert [g for g, ok in zip(got, live) if ok] == [tuple(int(c) for c in e) for e, ok in zip(exp, live) if ok], (what, "position", which)
        # centre of mass: sum v coord / sum v; numerator and denominator within their bounds, propagated through the quotient
        got, exp = np.asarray(Q.center_of_mass(index), np.float64), np.asarray(ndi.center_of_mass(d64, lab2, index), np.float64)
        assert got.shape == exp.shape, (what, "center_of_mass")
        if index is None:
            f, af = t["first"][1:].sum(axis=0), t["abs_first"][1:].sum(axis=0)
        else:
            f, af = t["first"][index], t["abs_first"][index]
        f, af = np.atleast_2d(f), np.atleast_2d(af)
        bf = sum_bound(np.atleast_1d(m)[:, None], af)
        w = np.abs(f[:, :1])
        ok = (bf[:, :1] < 0.5 * w).ravel()                              # where the quotient is conditioned at all
        bc = (bf[:, 1:] + np.abs(f[:, 1:]) / w * bf[:, :1]) / (w - bf[:, :1]) + 2 * U * np.abs(np.atleast_2d(exp))
        err = np.abs(np.atleast_2d(got) - np.atleast_2d(exp))
        keep = ok if scalar else ok & live
        assert (err[keep] <= bc[keep]).all(), (what, "center_of_mass")


@pytest.mark.parametrize("cid,x,s,j", host_cases(), ids=[c[0] for c in host_cases()])
def test_derivations_equal_scipy_on_the_case_table(cid, x, s, j):
    data, include, labels, n = field_case(x, s, j, np.float32 if j % 2 else np.float64)
    if n == 0:
        return
    rng = np.random.default_rng(j)
    Q = FromTables(lambda origin: restate(data, include, labels, n, origin), n, x.shape)
    several = rng.integers(1, n + 1, size=min(n, 6))
    for index in (int(several[0]), several.tolist(), np.concatenate([several, several[:2]]), np.arange(1, n + 1), None):
        check_against_scipy(Q, data, include, labels, n, index, (cid, index))


def test_index_forms_and_errors():
    x = R.field((5, 6, 7), 3, 0.4)
    data, include, labels, n = field_case(x, None, 3)
    assert n >= 3
    t = restate(data, include, labels, n)
    assert np.ndim(MS.sum_from(t, 2, n)) == 0 and np.ndim(MS.sum_from(t, np.int64(2), n)) == 0 and np.ndim(MS.sum_from(t, None, n)) == 0
    assert MS.sum_from(t, [2], n).shape == (1,) and MS.sum_from(t, [2, 2, 1], n).shape == (3,)
    assert MS.sum_from(t, [2, 2, 1], n)[0] == MS.sum_from(t, [2, 2, 1], n)[1] == MS.sum_from(t, 2, n)
    assert MS.sum_from(t, [], n).shape == (0,) and MS.position_from(t, [], n, x.shape, True) == []
    assert isinstance(MS.position_from(t, 1, n, x.shape, False), tuple) and isinstance(MS.position_from(t, [1], n, x.shape, False), list)
    assert isinstance(MS.center_of_mass_from(t, 1, n), tuple) and len(MS.center_of_mass_from(t, [1, 2], n)) == 2
    assert MS.sum_from(t, 2.0, n) == MS.sum_from(t, 2, n)
    for bad in (0, n + 1, -1, [1, 0], [n + 1], np.array([1, n + 7])):
        for f in (MS.sum_from, MS.mean_from, MS.variance_from, MS.center_of_mass_from):
            with pytest.raises(ValueError, match="1 to %d" % n):
                f(t, bad, n)
        with pytest.raises(ValueError, match="background"):
            MS.extreme_from(t, bad, n, True)
        with pytest.raises(ValueError):
            MS.position_from(t, bad, n, x.shape, True)
    for bad in (1.5, [[1, 2]], "1", True, [True, False]):
        with pytest.raises(ValueError):
            MS.parse_index(bad, n)
    # the public functions refuse a bad index before any device work (no device here: anything else would raise differently)
    lm = labelling.LabelMap(_StandInArray(x.shape, np.int32), n)
    for f in (MS.sum_labels, MS.mean, MS.variance, MS.standard_deviation, MS.minimum, MS.maximum, MS.minimum_position,
              MS.maximum_position, MS.extrema, MS.center_of_mass):
        with pytest.raises(ValueError, match="background"):
            f(None, lm, 0)


def test_empty_label_conventions():
    shape = (3, 4, 9)
    labels = np.zeros(shape, np.int32)
    labels[0, 0, :4], labels[1, 1, 2:6], labels[2, 3, 5:] = 1, 2, 3
    data = np.random.default_rng(5).normal(size=shape).astype(np.float32)
    data[1, 1, 2:4] = np.nan                                             # label 2: NaN samples and excluded voxels only
    include = np.ones(shape, bool)
    include[1, 1, 4:6] = False
    n = 4                                                                # label 4 has no voxel at all
    t = restate(data, include, labels, n)
    assert t["count"].tolist() == [0, 4, 0, 4, 0]
    for k in (2, 4):
        assert MS.sum_from(t, k, n) == 0.0 and np.isnan(MS.mean_from(t, k, n))
        t2 = restate(data, include, labels, n, MS.variance_origin(t, k, n))
        assert np.isnan(MS.variance_from(t2, k, n))
        assert np.isnan(MS.extreme_from(t, k, n, False)) and np.isnan(MS.extreme_from(t, k, n, True))
        assert MS.position_from(t, k, n, shape, False) == (-1, -1, -1) == MS.position_from(t, k, n, shape, True)
        assert np.isnan(MS.center_of_mass_from(t, k, n)).all()
    got = MS.mean_from(t, [1, 2, 3, 4], n)
    assert np.isnan(got).tolist() == [False, True, False, True]
    assert MS.position_from(t, [2, 3], n, shape, True)[0] == (-1, -1, -1)
    assert np.isfinite(MS.variance_origin(t, [1, 2], n)).all()           # the origin table never carries a NaN to the device
    # nothing measured anywhere: the union
    t0 = restate(data, np.zeros(shape, bool), labels, n)
    assert MS.sum_from(t0, None, n) == 0.0 and np.isnan(MS.mean_from(t0, None, n)) and np.isnan(MS.extreme_from(t0, None, n, True))
    assert MS.position_from(t0, None, n, shape, True) == (-1, -1, -1)
    assert np.isnan(MS.variance_from(t0, None, n))
    # the union passes over labels without a measured voxel, and its variance is about ONE mean
    assert MS.extreme_from(t, None, n, True) == np.nanmax(np.where(labels > 0, filled(data, include), np.nan)[include])
    o = MS.variance_origin(t, None, n)
    assert np.unique(o[1:, 0]).size == 1 and (o[:, 1:] == 0).all() and o[0, 0] == 0


# ---- the catalogue ------------------------------------------------------------------------------------------------------
def catalog_loop(data, include, labels, n, channel_width=1.0):
    """the catalogue by a direct loop over the labels, what catalog_from and the device are held to, and with every float
    column X a column "b_X": how far another correct float64 evaluation may be from it.  Derived as in the module docstring:
    W = sum v and N_a = sum v a are sums (sum_bound, of |v| and |v a|; the device sums v (a - box corner), whose terms are
    no larger); the centroid c_a = N_a / W is a quotient, b_c = (b_N + |c| b_W) / (|W| - b_W) and 4 U |c| for its own
    roundings.  S_ab = sum v (a - c_a)(b - c_b) about a centroid that is off by b_c: sum_bound of its terms, 8 U of
    them for the roundings inside a term on either side, and b_ca sum |v||b - c_b| + b_cb sum |v||a - c_a| + sum |v| b_ca b_cb
    for the shift; mu = S / W is a quotient again.  sigma = sqrt(mu): |sqrt x - sqrt y| <= min(sqrt |x - y|, |x - y| / (2 sqrt
    min(x, y))).  The angle is that of the vector (mu_xx - mu_yy, 2 mu_yx) halved; a vector of length A moved by d turns
    by at most asin(d / A) <= (pi / 2) d / A: a round region (A <= 2 d) has no angle and is not compared."""
    meas = measured_labels(data, include, labels)
    names = ("flux", "centroid", "sigma_z", "sigma_y", "sigma_x", "position_angle")
    cols = {k: [] for k in ("npix", "peak", "peak_position") + names + tuple("b_" + k for k in names)}
    cw = abs(channel_width)
    for k in range(1, n + 1):
        zz, yy, xx = np.nonzero(meas == k)
        v = data[zz, yy, xx].astype(np.float64)
        m = v.size
        cols["npix"].append(m)
        if m == 0:
            cols["flux"].append(0.0)
            cols["b_flux"].append(0.0)
            cols["peak"].append(np.nan)
            cols["peak_position"].append((-1, -1, -1))
            for c in names[1:]:
                cols[c].append((np.nan,) * 3 if c == "centroid" else np.nan)
                cols["b_" + c].append((np.nan,) * 3 if c == "centroid" else np.nan)
            continue
        j = int(np.argmax(v))                                            # nonzero is in C order: the first maximum
        cols["peak"].append(data[zz[j], yy[j], xx[j]])
        cols["peak_position"].append((zz[j], yy[j], xx[j]))
        av = np.abs(v)
        with np.errstate(invalid="ignore", divide="ignore"):
            w, bw = v.sum(), sum_bound(m, av.sum())
            cols["flux"].append(w * cw)
            cols["b_flux"].append(bw * cw + 2 * U * abs(w * cw))
            room = abs(w) - bw if abs(w) > 2 * bw else np.nan            # (a sum v of about 0: no quotient is conditioned)
            c, bc = [], []
            for a in (zz, yy, xx):
                c.append((v * a).sum() / w)
                bc.append((sum_bound(m, (av * a).sum()) + abs(c[-1]) * bw) / room + 4 * U * abs(c[-1]))
            cols["centroid"].append(c)
            cols["b_centroid"].append(bc)
            mu, bmu = {}, {}
            for ab, (a, i, b, j_) in {"zz": (zz, 0, zz, 0), "yy": (yy, 1, yy, 1), "xx": (xx, 2, xx, 2), "yx": (yy, 1, xx, 2)}.items():
                da, db = a - c[i], b - c[j_]
                t = av * np.abs(da) * np.abs(db)
                bs = (sum_bound(m, t.sum()) + 8 * U * t.sum() + bc[i] * (av * np.abs(db)).sum() + bc[j_] * (av * np.abs(da)).sum()
                      + av.sum() * bc[i] * bc[j_])
                mu[ab] = (v * da * db).sum() / w
                bmu[ab] = (bs + abs(mu[ab]) * bw) / room + 2 * U * abs(mu[ab])
            for c_, ab in (("sigma_z", "zz"), ("sigma_y", "yy"), ("sigma_x", "xx")):
                sig = np.sqrt(mu[ab])
                cols[c_].append(sig)
                cols["b_" + c_].append(min(np.sqrt(bmu[ab]), bmu[ab] / (2 * np.sqrt(max(mu[ab] - bmu[ab], 1e-300)))) + 2 * U * abs(sig))
            cols["position_angle"].append(0.5 * np.arctan2(2 * mu["yx"], mu["xx"] - mu["yy"]))
            length, moved = np.hypot(2 * mu["yx"], mu["xx"] - mu["yy"]), np.hypot(2 * bmu["yx"], bmu["xx"] + bmu["yy"])
            cols["b_position_angle"].append(0.5 * (np.pi / 2) * moved / length + 4 * U if length > 2 * moved else np.nan)
    return {k: np.asarray(v) for k, v in cols.items()}


def catalog_by_restatement(data, include, labels, n, wcs=None, channel_width=1.0):
    sizes = np.bincount(labels.ravel(), minlength=n + 1)
    bbox = np.zeros((n + 1, 6), np.int32)
    bbox[:, 0::2] = np.iinfo(np.int32).max
    for k, sl in enumerate(ndi.find_objects(labels, max_label=n), start=1):
        if sl is not None:
            bbox[k] = [q for s in sl for q in (s.start, s.stop)]
    o1 = MS.box_origin(sizes, bbox)
    t1 = restate(data, include, labels, n, o1)
    cen = MS.centroid_table(t1["first"], o1)
    o2 = np.zeros((n + 1, 4))
    o2[:, 1:] = np.where(np.isfinite(cen), cen, 0.0)
    return MS.catalog_from(t1, o1, restate(data, include, labels, n, o2), cen, labels.shape, channel_width=channel_width, wcs=wcs)


def assert_catalogs_agree(got, exp, what=""):
    """a catalogue against catalog_loop's: integers and samples equal, every float column within the loop's "b_" column;
    where a bound is NaN (no measured voxel, sum v of about 0, a round region's angle) the column is not compared"""
    assert np.array_equal(got["npix"], exp["npix"]) and got["npix"].dtype == np.int64, what
    assert np.array_equal(got["peak"], exp["peak"], equal_nan=True), what
    assert np.array_equal(got["peak_position"], np.asarray(exp["peak_position"]).reshape(-1, 3)), what
    for key in ("flux", "centroid", "sigma_z", "sigma_y", "sigma_x", "position_angle"):
        shape = np.shape(got[key])
        g, e, b = (np.asarray(a, np.float64).reshape(shape) for a in (got[key], exp[key], exp["b_" + key]))
        ok = ~np.isnan(b) & ~np.isnan(e)
        if key.startswith("sigma"):
            # a second moment within its bound of 0 may come out below 0 on one side: NaN there is as good as sigma <= bound
            g = np.where(np.isnan(g) & ok & (e <= b), 0.0, g)
        d = np.abs(g[ok] - e[ok])
        if key == "position_angle":
            d = np.minimum(d, np.pi - d)                                 # an axis: the angle is modulo pi
        assert not np.isnan(g[ok]).any() and (d <= b[ok]).all(), (what, key, float(np.max(d - b[ok])))
        empty = np.asarray(exp["npix"]) == 0
        assert np.isnan(g[empty]).all() or key == "flux", (what, key, "a label with nothing measured")
    assert (~np.isnan(np.asarray(exp["b_centroid"], np.float64))).any(), what


def positive_blobs(shape, seed, dtype=np.float32):
    """(data, include, labels, n): positive samples (weights of one sign: centroids and widths are well conditioned, so the
    bounds of catalog_loop are tight and every column is compared) over a thresholded smooth field"""
    rng = np.random.default_rng(seed)
    smooth = ndi.gaussian_filter(rng.normal(size=shape), 1.5)
    labels, n = R.scipy_label(smooth > 0.6 * smooth.std())
    data = (1.0 + 5.0 * np.abs(smooth) / smooth.std() + rng.random(shape)).astype(dtype)
    data[rng.random(shape) < 0.02] = np.nan
    include = rng.random(shape) > 0.1
    return data, include, labels, n


@pytest.mark.parametrize("shape,seed", [((12, 20, 33), 1), ((6, 40, 40), 2), ((9, 8, 70), 3)])
def test_catalogue_arithmetic_against_a_direct_loop(shape, seed):
    data, include, labels, n = positive_blobs(shape, seed)
    assert n >= 3
    cube = SpectralCube.read(np.zeros(shape, np.float32), dict(HDR))
    cat = catalog_by_restatement(data, include, labels, n, wcs=cube.wcs, channel_width=0.5)
    exp = catalog_loop(data, include, labels, n, channel_width=0.5)
    for v in cat.values():
        assert len(v) == n
    assert_catalogs_agree(cat, exp)
    ok = np.isfinite(cat["centroid"]).all(axis=1)
    assert np.allclose(cat["v_cen"][ok], -16.0 + 0.5 * cat["centroid"][ok, 0], rtol=0, atol=1e-12)
    assert np.allclose(cat["sigma_v"][ok], 0.5 * cat["sigma_z"][ok], rtol=1e-15, atol=0, equal_nan=True)
    lon, lat = cube.wcs.celestial_pix2world(cat["centroid"][ok, 2], cat["centroid"][ok, 1])
    assert np.array_equal(cat["lon"][ok], lon) and np.array_equal(cat["lat"][ok], lat)
    # one elongated region: the angle of its long axis, from +x towards +y
    lab = np.zeros((1, 21, 21), np.int32)
    for i in range(-8, 9):
        lab[0, 10 + i // 2, 10 + i] = 1                                  # slope 1 / 2
    one = catalog_by_restatement(np.ones(lab.shape, np.float32), None, lab, 1)
    assert 0.3 < one["position_angle"][0] < 0.6 and abs(one["position_angle"][0] - np.arctan(0.5)) < 0.05
    assert one["sigma_x"][0] > one["sigma_y"][0] > 0 and one["sigma_z"][0] == 0 and "v_cen" not in one


# ---- the C ABI ------------------------------------------------------------------------------------------------------------
NAMES = ("spc_label_measure_f32", "spc_label_measure_f64", "spc_label_measure_workspace_bytes")


def test_entry_points_declared_exported_and_bound():
    import spectral_cube_amd as pkg
    lib = _lib.load()
    assert lib.spc_abi_version() == 8 == _lib.ABI_VERSION
    text = open(os.path.join(REPO, "include", "spcube_hip.h")).read()
    for name in NAMES:
        kind = "size_t" if name.endswith("_bytes") else "int"
        assert re.search(r"\b%s\s+%s\s*\(" % (kind, name), text), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    for name, bit in (("SUMS", 1), ("EXTREMA", 2), ("FIRST", 4), ("SECOND", 8)):
        assert re.search(r"#define\s+SPC_MEASURE_%s\s+%du\b" % (name, bit), text) and getattr(_lib, "MEASURE_" + name) == bit
    fields = re.search(r"typedef struct \{([^}]*)\} spc_label_measure_outputs;", text).group(1)
    assert re.findall(r"\b(d_\w+);", fields) == [f for f, _ in _lib.SpcLabelMeasureOutputs._fields_]
    assert C.sizeof(_lib.SpcLabelMeasureOutputs) == 8 * 8
    assert "spc_label_measure.hip" in open(os.path.join(REPO, "spectral_cube_amd", "csrc", "Makefile")).read()
    assert "not fixed" in text.lower() or "NOT FIXED" in text                 # the header says the sums are not bit-stable
    for name in MS.__all__:
        assert getattr(pkg, name) is getattr(MS, name), name
    assert pkg.measurements is MS and callable(ops.label_measure)
    assert callable(labelling.LabelMap.measure) and callable(labelling.LabelMap.catalog)
    assert "are not built" not in labelling.__doc__


def test_workspace_query():
    q = _lib.load().spc_label_measure_workspace_bytes
    assert q(-1, 15) == 0 and q(2 ** 31, 15) == 0
    for want in range(1, 16):
        last = 0
        for n in (0, 1, 7, 255, 256, 10 ** 4, 10 ** 6):
            need = q(n, want)
            assert need >= max(last, 256)
            assert (need >= 16 * (n + 1)) == bool(want & 2) or n < 64        # two 64-bit keys per label, for the extrema only
            last = need
    assert q(10 ** 6, 1) == q(0, 1) < 2048


def _buffers(nz=3, ny=4, nx=40, nl=7):
    lib = _lib.load()
    n = nz * ny * nx
    wsn = lib.spc_label_measure_workspace_bytes(nl, 15)
    B = dict(n=n, data=(C.c_float * (2 * n))(), lab=(C.c_int32 * (2 * n))(), ws=(C.c_uint8 * wsn)(), wsn=wsn, arr=(C.c_uint8 * n)(),
             origin=(C.c_double * (4 * (nl + 1) + 256))())                  # (room behind the table: a workspace may be laid over it)
    for name, per in (("count", 8), ("sums", 16), ("min", 8), ("max", 8), ("min_pos", 8), ("max_pos", 8), ("first", 32), ("second", 48)):
        B[name] = (C.c_uint8 * (per * (nl + 1)))()
    return B


def test_invalid_arguments_are_reported_before_any_device_work():
    lib = _lib.load()
    nz, ny, nx, nl = 3, 4, 40, 7
    B = _buffers(nz, ny, nx, nl)

    def run(entry="spc_label_measure_f32", shape=(nz, ny, nx), data=P(B["data"]), strides=(nx, ny * nx), d_lab=P(B["lab"]), n=nl,
            origin=None, want=15, w=P(B["ws"]), wn=B["wsn"], out=True, mask_arr=None, device=0, **tables):
        c = _lib.SpcCube()
        c.d_data, (c.nz, c.ny, c.nx), (c.row_stride, c.plane_stride) = data.value if data else None, shape, strides
        m = (_lib.SpcMask64 if entry.endswith("64") else _lib.SpcMask)()
        if mask_arr is not None:
            m.flags, m.d_array = _lib.MASK_ARRAY, mask_arr.value
        o = _lib.SpcLabelMeasureOutputs()
        for f, _ in o._fields_:
            p = tables.get(f, P(B[f[2:]]))
            setattr(o, f, p.value if p is not None else None)
        return getattr(lib, entry)(device, None, C.byref(c), C.byref(m), d_lab, n, origin, want, C.byref(o) if out else None, w, wn)

    for entry in ("spc_label_measure_f32", "spc_label_measure_f64"):
        for kw, word in ((dict(data=None), b"cube pointer is NULL"), (dict(d_lab=None), b"d_labels is NULL"), (dict(out=False), b"out is NULL"),
                         (dict(shape=(nz, 0, nx)), b"positive"), (dict(shape=(nz, ny, -1)), b"positive"),
                         (dict(strides=(nx - 1, ny * nx)), b"stride smaller than nx"), (dict(strides=(nx, nx)), b"overlapping rows"),
                         (dict(n=-1), b"nlabels"), (dict(n=2 ** 31), b"nlabels"), (dict(want=0), b"want"), (dict(want=16), b"want"),
                         (dict(want=31), b"want"),
                         (dict(d_count=None), b"SPC_MEASURE_SUMS"), (dict(d_sums=None), b"SPC_MEASURE_SUMS"),
                         (dict(d_min=None), b"SPC_MEASURE_EXTREMA"), (dict(d_max_pos=None), b"SPC_MEASURE_EXTREMA"),
                         (dict(d_first=None), b"SPC_MEASURE_FIRST"), (dict(d_second=None), b"SPC_MEASURE_SECOND"),
                         (dict(d_sums=P(B["lab"], 8)), b"d_sums overlaps d_labels"), (dict(d_first=P(B["data"])), b"d_first overlaps the cube"),
                         (dict(d_min=P(B["max"])), b"overlaps"), (dict(d_second=P(B["first"], 16)), b"d_first overlaps d_second"),
                         (dict(d_count=P(B["origin"]), origin=P(B["origin"])), b"d_count overlaps d_origin"),
                         (dict(d_max=P(B["arr"]), mask_arr=P(B["arr"])), b"d_max overlaps the mask array"),
                         (dict(w=None), b"d_workspace too small"), (dict(wn=B["wsn"] // 2), b"d_workspace too small"), (dict(wn=0), b"too small"),
                         (dict(w=P(B["lab"], 16)), b"d_workspace overlaps d_labels"), (dict(w=P(B["second"])), b"overlaps")):
            assert run(entry, **kw) == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (entry, kw, lib.spc_last_error())
        # the fullest call - all four groups, a mask array and an origin table: 13 buffers are held against each other, the
        # last of them too; with everything in order the call gets as far as a device no machine has
        full = dict(want=15, mask_arr=P(B["arr"]), origin=P(B["origin"]))
        for kw, word in ((dict(d_count=P(B["origin"], 8)), b"d_count overlaps d_origin"), (dict(d_second=P(B["arr"], 8)), b"d_second overlaps the mask array"),
                         (dict(w=P(B["origin"])), b"d_workspace overlaps d_origin")):
            assert run(entry, **full, **kw) == _lib.SPC_ERR_INVALID and word in lib.spc_last_error(), (entry, kw, lib.spc_last_error())
        for want in range(1, 16):
            assert run(entry, device=2 ** 20, **dict(full, want=want)) == _lib.SPC_ERR_HIP and b"hipSetDevice" in lib.spc_last_error()
        # a group that is not wanted is not looked at: its NULL pointers pass the checks (what fails next is the device)
        assert run(entry, want=1, d_min=None, d_first=None, d_second=None, n=-1) == _lib.SPC_ERR_INVALID
        assert b"nlabels" in lib.spc_last_error()
        # more than 2^31 - 1 voxels: refused by shape alone
        for shape in ((2048, 1024, 1024), (1, 1, 2 ** 31), (2 ** 31, 2 ** 31, 2 ** 31)):
            assert run(entry, shape=shape, strides=(shape[2], shape[1] * shape[2])) == _lib.SPC_ERR_UNSUPPORTED
            assert b"2^31 - 1" in lib.spc_last_error()


# ---- what ops hands to the entry points -------------------------------------------------------------------------------
@pytest.fixture
def recorded_calls(monkeypatch):
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    monkeypatch.setattr(ops, "DeviceArray", _StandInArray)
    monkeypatch.setattr(ops, "_ws_cache", {})
    return calls


def test_ops_passes_cube_mask_origin_and_tables_as_specified(recorded_calls):
    shape = (6, 5, 40)
    lab = _StandInArray(shape, np.int32, ptr=0x3000)
    data = _StandInArray(shape, np.float32, ptr=0x2000)
    data.row_stride, data.plane_stride = 48, 48 * 9                       # a strided view of the cube
    arr = _StandInArray(shape, np.uint8, ptr=0x7000)
    origin = _StandInArray((10, 4), np.float64, ptr=0x9000)
    res = ops.label_measure(data, lab, 9, mask_spec=ops.MaskSpec(_lib.MASK_ARRAY | _lib.MASK_GT, 0.5, 0.0, arr), origin=origin,
                            want=("sums", "extrema", "first", "second"))
    (name, a), = recorded_calls
    assert name == "spc_label_measure_f32" and len(a) == len(_lib.SIGNATURES[name][1]) == 11
    # device, stream, cube, mask, d_labels, nlabels, d_origin, want, out, ws, n
    c, m, o = a[2]._obj, a[3]._obj, a[8]._obj
    assert a[:2] == (0, None) and (c.d_data, c.nz, c.ny, c.nx, c.row_stride, c.plane_stride) == (0x2000, 6, 5, 40, 48, 48 * 9)
    assert isinstance(m, _lib.SpcMask) and (m.flags, m.thr_lo, m.d_array) == (_lib.MASK_ARRAY | _lib.MASK_GT, 0.5, 0x7000)
    assert a[4].value == 0x3000 and a[5] == 9 and a[6].value == 0x9000 and a[7] == 15
    assert a[10] >= _lib.load().spc_label_measure_workspace_bytes(9, 15)
    expect = {"count": ((10,), np.int64), "sums": ((10, 2), np.float64), "min": ((10,), np.float32), "max": ((10,), np.float32),
              "min_pos": ((10,), np.int64), "max_pos": ((10,), np.int64), "first": ((10, 4), np.float64), "second": ((10, 6), np.float64)}
    assert {k: (v.shape, v.dtype) for k, v in res.items()} == {k: (s, np.dtype(d)) for k, (s, d) in expect.items()}
    for k, v in res.items():
        assert getattr(o, "d_" + k) == v.ptr
    # a float64 cube, sums only, no origin, no mask: the other entry, NULL for what is not wanted
    del recorded_calls[:]
    given = {"count": _StandInArray((10,), np.int64, ptr=0xA000)}
    res = ops.label_measure(_StandInArray(shape, np.float64, ptr=0x2000), lab, 9, want="sums", out=given)
    (name, a), = recorded_calls
    o = a[8]._obj
    assert name == "spc_label_measure_f64" and isinstance(a[3]._obj, _lib.SpcMask64) and a[6] is None and a[7] == _lib.MEASURE_SUMS
    assert sorted(res) == ["count", "sums"] and res["count"] is given["count"] and o.d_count == 0xA000
    assert o.d_min is None and o.d_first is None and o.d_second is None and o.d_max_pos is None
    del recorded_calls[:]
    res = ops.label_measure(_StandInArray(shape, np.float64), lab, 9, want=("extrema",))
    assert res["min"].dtype == res["max"].dtype == np.float64 and recorded_calls[0][1][7] == _lib.MEASURE_EXTREMA
    # a host origin table is uploaded
    del recorded_calls[:]
    up = []
    monkey_from = classmethod(lambda cls, arr, device=0, stream=None, dtype=None: up.append(arr) or _StandInArray(arr.shape, arr.dtype, ptr=0xB000))
    _StandInArray.from_numpy = monkey_from
    try:
        ops.label_measure(data, lab, 9, origin=np.arange(40).reshape(10, 4), want=("first",))
    finally:
        del _StandInArray.from_numpy
    assert up[0].dtype == np.float64 and up[0].shape == (10, 4) and recorded_calls[0][1][6].value == 0xB000


def test_ops_refuses_what_the_entry_would(recorded_calls):
    shape = (6, 5, 40)
    lab, data = _StandInArray(shape, np.int32), _StandInArray(shape, np.float32)
    view = _StandInArray(shape, np.int32)
    view._is_view = True
    with pytest.raises(TypeError):
        ops.label_measure(data, _StandInArray(shape, np.uint8), 3)
    with pytest.raises(ValueError, match="contiguous"):
        ops.label_measure(data, view, 3)
    with pytest.raises(ValueError, match="nlabels"):
        ops.label_measure(data, lab, -1)
    with pytest.raises(TypeError, match="float32 or float64"):
        ops.label_measure(_StandInArray(shape, np.int16), lab, 3)
    with pytest.raises(ValueError, match="one shape"):
        ops.label_measure(_StandInArray((6, 5, 41), np.float32), lab, 3)
    for want in ((), ("sum",), ("sums", "moments"), 3):
        with pytest.raises((ValueError, TypeError)):
            ops.label_measure(data, lab, 3, want=want)
    with pytest.raises(ValueError, match="origin"):
        ops.label_measure(data, lab, 3, origin=np.zeros((3, 4)))
    with pytest.raises(ValueError, match="origin"):
        ops.label_measure(data, lab, 3, origin=_StandInArray((4, 4), np.float32))
    with pytest.raises(ValueError, match="preallocated"):
        ops.label_measure(data, lab, 3, out={"sums": _StandInArray((4,), np.float64)})
    with pytest.raises(ValueError, match="preallocated"):
        ops.label_measure(data, lab, 3, want=("extrema",), out={"min": _StandInArray((4,), np.float64)})
    with pytest.raises(ValueError, match="workspace"):
        ops.label_measure(data, lab, 3, workspace=_StandInArray((16,), np.uint8))
    with pytest.raises(ValueError, match="mask array"):
        ops.label_measure(data, lab, 3, mask_spec=ops.MaskSpec(_lib.MASK_ARRAY, 0, 0, _StandInArray((6, 5, 4), np.uint8)))
    assert recorded_calls == []


def test_measuring_refuses_an_out_of_core_cube_and_another_shape(monkeypatch):
    cube = SpectralCube.read(np.zeros((6, 5, 4), np.float32), dict(HDR))
    lm = labelling.LabelMap(_StandInArray((6, 5, 5), np.int32), 2)
    with pytest.raises(ValueError, match="one shape"):
        lm.measure(cube)
    monkeypatch.setenv("SPC_HBM_BUDGET", "64")
    lm = labelling.LabelMap(_StandInArray((6, 5, 4), np.int32), 2)
    lm._objects = (np.array([100, 10, 10]), np.zeros((3, 6), np.int32))
    for f in (lambda: lm.measure(cube), lambda: lm.catalog(cube), lambda: MS.sum_labels(cube, lm, 1), lambda: MS.center_of_mass(cube, lm)):
        with pytest.raises(NotImplementedError, match="out-of-core"):
            f()
