"""The references and the cases of test_gpu_far_from_zero.py, checked on the CPU: the long-double reference of std against
exact rational arithmetic and against numpy's nanstd, the textbook formula (today's statistics()['sigma'], yesterday's std)
missing the GPU tolerance by a wide margin on every family - so a kernel that still used it could not pass - and the share of
rays that the sigma-clip comparison leaves out.  No GPU."""
import warnings

import numpy as np
import pytest

import far_from_zero as Z


@pytest.mark.parametrize("family", sorted(Z.FAMILIES))
def test_ref_std_agrees_with_exact_rational_arithmetic(family):
    """a few short rays of every family (axis 0 of the smallest shape, under the array mask: 0, 1, 2 and more samples) in
    fractions.Fraction, the square root in long double: 4 eps64"""
    for dtype in Z.FAMILIES[family][1]:
        shape = min(Z.SHAPES[dtype], key=lambda s: s[0] * s[1] * s[2])
        d, arr, thr = Z.case(family, dtype, shape)
        f = Z.filled_of(d, Z.include_of(d, arr, thr, "array"))
        for ddof in (0, 1):
            got = Z.ref_std(f, 0, ddof)
            for y, x in [(0, 0), (0, 1), (0, 2), (0, 3), (shape[1] - 1, shape[2] // 2), (0, shape[2] - 1), (shape[1] // 2, shape[2] // 3)]:
                exp = Z.exact_std(f[:, y, x], ddof)
                assert np.isnan(exp) == np.isnan(got[y, x]), (family, y, x, ddof)
                if not np.isnan(exp):
                    assert abs(got[y, x] - exp) <= 4 * Z.EPS64 * abs(exp), (family, dtype, y, x, ddof, got[y, x], exp)
        # ... and one whole-cube value, which takes the other branch of the axis handling
        small = f[:5, :2, :3]
        exp = Z.exact_std(small.ravel(), 1)
        assert abs(Z.ref_std(small, None, 1) - exp) <= 4 * Z.EPS64 * abs(exp)
        assert abs(Z.ref_std(small, (0, 1, 2), 1) - exp) <= 4 * Z.EPS64 * abs(exp)


@pytest.mark.parametrize("case", Z.all_cases(), ids=Z.case_id)
def test_ref_std_agrees_with_nanstd_of_the_float64_samples(case):
    """np.nanstd is two-pass too (good to about 1e-15 here): 1e-13, the NaN pattern exact, every axis, mask and ddof.  The
    `constant` rays, whose std is 0, are held to the absolute bound of the GPU test"""
    family, dtype, shape = case
    d, arr, thr = Z.case(*case)
    for mask in Z.MASKS:
        f = Z.filled_of(d, Z.include_of(d, arr, thr, mask))
        for axis in Z.AXES:
            for ddof in (0, 1):
                with warnings.catch_warnings(), np.errstate(all="ignore"):
                    warnings.simplefilter("ignore", RuntimeWarning)
                    exp = np.nanstd(f.astype(np.float64), axis=axis, ddof=ddof)
                got = np.asarray(Z.ref_std(f, axis, ddof))
                assert np.array_equal(np.isnan(got), np.isnan(exp)), (mask, axis, ddof)
                ok = ~np.isnan(exp)
                assert np.all(np.abs(got - exp)[ok] <= 1e-13 * np.abs(got)[ok] + Z.std_atol(family, d)), (mask, axis, ddof)


def _teeth(case):
    """the largest miss of textbook_std over masks, axes and ddof, in units of the GPU tolerance"""
    family, dtype, shape = case
    d, arr, thr = Z.case(*case)
    worst = 0.0
    for mask in Z.MASKS:
        f = Z.filled_of(d, Z.include_of(d, arr, thr, mask))
        for axis in Z.AXES:
            for ddof in (0, 1):
                ref, bad = np.asarray(Z.ref_std(f, axis, ddof)), np.asarray(Z.textbook_std(f, axis, ddof))
                ok = ~np.isnan(ref) & ((ref > 0) | (family == "constant"))        # (equal counts: 0 against 0 + rtol 0)
                if ok.any():
                    worst = max(worst, float(np.max(np.abs(bad - ref)[ok] / (Z.RTOL * np.abs(ref)[ok] + Z.std_atol(family, d)))))
    return worst


# the one case the textbook formula gets right: three equal float32 samples per ray - 3 b, 3 b^2 and 9 b^2 / 3 are exact in
# float64 - and along the other axes the baselines differ by more than their rounding
NO_TEETH = {("constant", Z.F32, (3, 50, 1366))}


@pytest.mark.parametrize("case", [c for c in Z.all_cases() if c[0] != "sparse"], ids=Z.case_id)
def test_the_textbook_formula_misses_the_gpu_tolerance_by_a_factor_100(case):
    """every case has teeth: sqrt((sumsq - sum^2 / n) / (n - ddof)) in float64 - numpy's pairwise sums, the best case for a
    kernel - is off by >= 100 x the tolerance of test_gpu_far_from_zero.py in every case but the one of NO_TEETH, which is
    held to having none (`sparse` is there for the NaN rules)"""
    with np.errstate(all="ignore"):
        worst = _teeth(case)
    print(Z.case_id(case), "%.1e" % worst)
    assert (worst < 1.0) if case in NO_TEETH else (worst >= 100.0), worst


def test_counts_image_means_the_counts_cube():
    """the BITPIX = 32 image of `counts64` decodes (numpy model: raw + BZERO in float64, BLANK -> NaN) to the array form"""
    shape = Z.SHAPES[Z.F64][0]
    blob, d = Z.counts_fits(shape)
    assert len(blob) % 2880 == 0 and blob[:6] == b"SIMPLE"
    n = int(np.prod(shape))
    raw = np.frombuffer(blob[2880:2880 + 4 * n], ">i4").reshape(shape)
    got = np.where(raw == Z.BLANK32, np.nan, raw.astype(np.float64) + 2.0 ** 30)
    assert np.array_equal(got, d, equal_nan=True) and np.isnan(d).any()


@pytest.mark.parametrize("cen", ["median", "mean"])
@pytest.mark.parametrize("case", Z.clip_cases(), ids=Z.clip_id)
def test_sigma_clip_cases_leave_out_few_rays(case, cen):
    """the oracle alone: the share of rays with a sample inside the float32 rounding of a bound stays under the cap, every ray
    holds its outliers and NaN, and the masked form leaves at most 128 valid samples per ray"""
    d, inc = Z.clip_case(*case)
    exp, out = Z.clip_oracle(d, inc, cen)
    assert out.mean() <= Z.CLIP_CAP, out.mean()
    valid = ~np.isnan(d) if inc is None else (inc & ~np.isnan(d))
    assert (np.isnan(d).sum(axis=0) == 2).all()
    if case[3]:
        assert valid.sum(axis=0).max() <= 128
    clipped = valid & np.isnan(exp)
    assert clipped.any() and (clipped.sum(axis=0) <= 0.2 * case[2] + 3).all()          # it clips, and no ray is emptied


@pytest.mark.parametrize("case", Z.all_cases(), ids=Z.case_id)
def test_the_sums_are_well_conditioned_where_they_are_held_relative(case):
    """sum and mean are held to 1e-12 of their value where every sample has one sign (sum |x| = |sum x|: any float64 sum meets
    it), and to 1e-12 of sum |x| in the two families whose baselines have both signs, where a row of the plane can cancel to
    any degree; the whole-cube sums of those, which statistics() is held to relatively, lose less than a decade"""
    family, dtype, shape = case
    d, arr, thr = Z.case(*case)
    for mask in Z.MASKS:
        f = Z.filled_of(d, Z.include_of(d, arr, thr, mask))
        for axis in Z.AXES:
            n, s, a = Z.wide_sums(f, axis)
            if family not in Z.MIXED_SIGNS:
                assert np.array_equal(np.abs(s), a), (mask, axis)
            elif axis is None:
                assert a <= 10 * abs(s), (mask, float(a / abs(s)))
        ex = Z.exact_sums(f)
        n, s, a = Z.wide_sums(f, None)
        assert ex["npts"] == n and abs(ex["sum"] - float(s)) <= 1e-15 * float(a)
