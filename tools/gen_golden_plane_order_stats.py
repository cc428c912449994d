"""Generate tests/golden/plane_order_stats.npz from the REFERENCE's median / percentile / mad_std over two axes
(in-memory class: apply_numpy_function(np.nanmedian / np.nanpercentile / astropy.stats.mad_std, axis=pair)).

Run with the reference environment, like tools/gen_golden_rank_filter.py:

    /opt/conda/bin/python3.9 -B tools/gen_golden_plane_order_stats.py

One float32 cube of 9 x 11 x 13 with a header: normal samples around 0.4, about 4 % NaN, under a BooleanArrayMask that
excludes about a third of the samples, one whole channel (z = 4), one whole row index (y = 7) and one whole column index
(x = 2) - the groups of each axis pair that must come out NaN.  Recorded: data, include, and for each of the pairs (1, 2),
(0, 2) and (0, 1) the reference's median, percentile(q) for q = 10, 37.5 and 90, and mad_std (how='slice' where the
reference takes it, its default otherwise; ``mad_std_from_reference`` says per pair whether the reference gave it).

Before anything is written, the numpy restatement the tests use (oracle/oracle_np.py: np.nanmedian, np.nanpercentile and
1.482602218505602 * nanmedian(|d - nanmedian(d, keepdims)|) on the NaN-filled data) is checked against every recorded
array: the median exactly, percentile and mad_std within 2e-6 of the largest value.  No test imports this file; only its
output is committed.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle", "ref_env"))

from bootstrap import load_reference  # noqa: E402

load_reference()
warnings.simplefilter("ignore")

from astropy import units as u  # noqa: E402
from astropy.wcs import WCS  # noqa: E402
from spectral_cube import SpectralCube, BooleanArrayMask  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "plane_order_stats.npz")
HEADER = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s",
          "CDELT1": -2e-3, "CDELT2": 2e-3, "CDELT3": 0.5, "CRPIX1": 7.0, "CRPIX2": 6.0, "CRPIX3": 2.0,
          "CRVAL1": 30.0, "CRVAL2": -20.0, "CRVAL3": 4.0, "BUNIT": "K"}
SHAPE = (9, 11, 13)
PAIRS = ((1, 2), (0, 2), (0, 1))
QS = (10.0, 37.5, 90.0)
GONE = {"z": 4, "y": 7, "x": 2}
MAD = 1.482602218505602


def header_text(h):
    return "\n".join("%-8s= %r" % (k, v) if isinstance(v, str) else "%-8s= %s" % (k, repr(float(v))) for k, v in h.items())


def make_data():
    rng = np.random.default_rng(20261019)
    d = rng.normal(0.4, 1.0, SHAPE).astype(np.float32)
    d[rng.random(SHAPE) < 0.04] = np.nan
    inc = rng.random(SHAPE) < 0.9
    inc[GONE["z"], :, :] = False
    inc[:, GONE["y"], :] = False
    inc[:, :, GONE["x"]] = False
    return d, inc


def plain(r):
    return np.asarray(getattr(r, "value", r), dtype=np.float64)


def restated(d, inc, pair):
    f = np.where(inc, d, np.float32(np.nan))
    out = {"median": np.nanmedian(f, axis=pair)}
    for q in QS:
        out["p%g" % q] = np.nanpercentile(f, q, axis=pair)
    med = np.nanmedian(f, axis=pair, keepdims=True)
    out["mad_std"] = MAD * np.nanmedian(np.abs(f - med), axis=pair)
    return out


def same(a, b, atol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.array_equal(np.isnan(a), np.isnan(b)), what + ": NaN pattern"
    ok = ~np.isnan(a)
    assert np.all(np.abs(a[ok] - b[ok]) <= atol), (what, np.abs(a[ok] - b[ok]).max(), atol)


def main():
    d, inc = make_data()
    w = WCS(HEADER)
    cube = SpectralCube(data=d * u.K, wcs=w, mask=BooleanArrayMask(inc, wcs=w))
    out = {"header": np.array(header_text(HEADER)), "data": d, "include": inc}
    from_ref = []
    for pair in PAIRS:
        tag = "a%d%d" % pair
        rec = {"median": plain(cube.median(axis=pair))}
        for q in QS:
            rec["p%g" % q] = plain(cube.percentile(q, axis=pair))
        mad = None
        for kw in ({"how": "slice"}, {}):
            try:
                mad = plain(cube.mad_std(axis=pair, **kw))
                print("mad_std axis=%s %s: the reference gave it" % (pair, kw or "(default how)"))
                break
            except Exception as exc:                      # noqa: BLE001 - what the reference refuses is the finding
                print("mad_std axis=%s %s: the reference refuses: %s: %s" % (pair, kw, type(exc).__name__, exc))
        exp = restated(d, inc, pair)
        from_ref.append(mad is not None)
        rec["mad_std"] = mad if mad is not None else np.asarray(exp["mad_std"], np.float64)
        n_out = SHAPE[({0, 1, 2} - set(pair)).pop()]
        for k, v in rec.items():
            assert v.shape == (n_out,), (pair, k, v.shape)
            atol = 0.0 if k == "median" else 2e-6 * np.nanmax(np.abs(v))
            same(exp[k], v, atol, "%s axis=%s" % (k, pair))
            out["%s_%s" % (k, tag)] = v
        gone = GONE["zyx"[({0, 1, 2} - set(pair)).pop()]]
        assert np.isnan(rec["median"][gone]) and np.isnan(rec["mad_std"][gone]) and np.isnan(rec["median"]).sum() == 1
    out["mad_std_from_reference"] = np.array(from_ref)
    frac = 1.0 - inc.mean()
    assert 0.28 < frac < 0.4, frac
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes; excluded %.0f %% of the samples" % (100 * frac))


if __name__ == "__main__":
    main()
