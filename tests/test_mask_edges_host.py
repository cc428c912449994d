"""CPU companion of test_gpu_mask_edges.py: the cases there can fail.  For every (operator, path shape, mask) of
mask_edges.CASES the oracle's result under each neighbouring WRONG predicate (strictness flipped, the bound one ulp either
way, NaN let through a threshold, the array term ignored, +-inf let through isfinite) must miss the expected result by
more than 100 x the tolerance that the GPU test applies, or in a NaN / inf pattern, or in an exact output - unless the
wrong predicate includes exactly the same voxels on this data.  The oracle only; no GPU."""
import numpy as np
import pytest

import mask_edges as E
from test_gpu_mask_layer import _masks


def test_the_masks_and_samples_are_those_of_the_issue():
    for dtype in (np.float32, np.float64):
        s = E.samples(dtype)
        fi = np.finfo(dtype)
        assert s.dtype == dtype and s.size == 20 and len(set(s.view(np.uint32 if dtype == np.float32 else np.uint64))) == 20
        for v in (fi.smallest_subnormal, -fi.smallest_subnormal, dtype(0.1), np.nextafter(dtype(0.1), dtype(1)), np.nextafter(dtype(0.1), dtype(0)),
                  fi.max, -fi.max, dtype(1.5), np.nextafter(dtype(1.5), dtype(2)), np.nextafter(dtype(1.5), dtype(1)), dtype(np.inf), -dtype(np.inf)):
            assert (s == v).any(), v
        assert np.isnan(s).sum() == 1 and (np.signbit(s) & (s == 0)).sum() == 1
        ms = E.masks(dtype)
        assert len(ms) == 11 * 2 + (5 * 4 + 2) * 2 and len({m.name for m in ms}) == len(ms)


def test_include_is_the_numpy_expression_of_the_mask_layer_test():
    """the flag-driven evaluation of mask_edges.include against the lambdas of test_gpu_mask_layer._masks, mask by mask"""
    for dtype in (np.float32, np.float64):
        d, arr = E.flat_cube(dtype, (5, 6, 7))
        for name, flags, lo, hi, pred, with_array, nan_excluded in _masks():
            if nan_excluded:
                continue
            exp = np.ones(d.shape, bool)
            with np.errstate(invalid="ignore"):
                if pred is not None:
                    exp &= pred(d, dtype)
            if with_array:
                exp &= arr != 0
            assert np.array_equal(E.include(d, arr, E.Mask(name, flags, lo, hi, with_array)), exp), name


def test_every_kind_of_ray_holds_every_sample():
    for dtype in (np.float32, np.float64):
        d, arr = E.ray_cube(dtype, (40, 12, 7), 0)
        s = E.samples(dtype)
        u = np.uint32 if dtype == np.float32 else np.uint64
        rays, marr = d.reshape(40, -1), arr.reshape(40, -1)
        for r in range(80):
            special = np.arange(40) == 1 + (3 * r + r // 5) % 39
            assert rays[special, r].view(u)[0] == s[r % 20:r % 20 + 1].view(u)[0]
            assert marr[special, r][0] == (0 if (r // 20) % 2 else 1) and marr[~special, r].all()
            rest = rays[~special, r]
            assert np.isnan(rest).all() if (r // 20) % 4 >= 2 else (np.isin(rest, (0.25, 2.0)).all() and 18 <= (rest == 0.25).sum() <= 21)


@pytest.mark.parametrize("case", E.CASES, ids=E.case_id)
def test_a_wrong_predicate_would_fail(case):
    cache = E.RefCache(case)
    d, arr = cache.d, cache.arr
    identical, excused, caught, missed = 0, 0, 0, []
    for m in E.masks(case.dtype):
        ref = cache.expected(m)
        E.check({k: v[0] for k, v in ref.items()}, ref, m.name)          # (the checker accepts the expected result itself)
        assert not E.differs(ref, ref)
        for wrong in E.WRONG:
            w = E.wrong_case(d, arr, m, wrong)
            if w is None:
                identical += 1
                continue
            if not E.differs(ref, cache.ref(*w)):
                if E.cannot_show(case.op, d[w[1] != E.include(d, arr, m)]):
                    excused += 1                # identical in every output, whatever the data
                    continue
                missed.append((m.name, wrong))
            else:
                caught += 1
    assert not missed, "%d wrong predicates would pass: %s" % (len(missed), missed[:12])
    total = len(E.masks(case.dtype)) * len(E.WRONG)
    print("%s: %d wrong predicates, %d caught, %d identical include sets, %d that cannot show" % (E.case_id(case), total, caught, identical, excused))
    assert caught + identical + excused == total and caught > 0
    # what cannot show is a property of the operator (mask_edges.cannot_show), none for most: where there is some it stays
    # below the caught ones and below a quarter of all
    assert excused == 0 or case.op in E.WEIGHTS_ONLY + E.BLENDS
    assert excused <= caught and 4 * excused <= total, (caught, identical, excused)
