"""Generate tests/golden/arith.npz from the REFERENCE's cube arithmetic (spectral_cube.py:912-1003, 2237-2361).

Run with the reference environment, like tools/gen_golden_stack_cube.py (the same ``beam`` override):

    /opt/conda/bin/python3.9 -B tools/gen_golden_arith.py

A (7, 5, 6) float32 cube in K with one NaN (which the boolean mask INCLUDES) and a BooleanArrayMask, with fill value NaN and
0, through the NumPy class (``np``) and the Dask class (``dask``).  Every expression of CASES is recorded under
``<class>|<fill>|...``: for the ones that return a cube ``names`` and, stacked in that order, ``raw`` (unmasked_data) and
``units``; for the ones that raise ``raising`` (their names), ``raises`` (the exceptions' class names) and ``messages``.
The include map of every result is checked to be ``keep`` and its filled_data to be ``where(keep, raw, fill)`` before the
file is written, so neither is stored per case.
The operands - all float32, so that an exact comparison is meaningful - are recorded once (``map``, ``map2``, ``spec``,
``row``, ``col``, ``zy``, ``cube2`` with its own mask ``keep2``), as are the unitless cube of the general powers
(``powbase`` = abs(cube) + 0.1) and the case of a lazy mask that must keep testing the original samples (``lazy|...``).
The file holds arrays and strings only.  No test imports this file; only its output is committed.
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
import spectral_cube.base_class as B  # noqa: E402
from spectral_cube import SpectralCube, BooleanArrayMask  # noqa: E402

B.BeamMixinClass.beam = property(lambda self: None, lambda self, v: None)

OUT = os.path.join(REPO, "tests", "golden", "arith.npz")
HEADER = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "m/s",
          "CDELT1": -2e-3, "CDELT2": 2e-3, "CDELT3": 500.0, "CRPIX1": 3.0, "CRPIX2": 3.0, "CRPIX3": 2.0,
          "CRVAL1": 30.0, "CRVAL2": -20.0, "CRVAL3": 0.0, "BUNIT": "K"}
NZ, NY, NX = 7, 5, 6
K = u.K

# name -> expression of (cube, operands); `o` holds the recorded float32 arrays and the second cube
CASES = {
    "add_q": lambda c, o: c + 1.5 * K,
    "sub_q": lambda c, o: c - 0.25 * K,
    "mul_s": lambda c, o: c * 2.5,
    "mul_i": lambda c, o: c * 2,
    "div_s": lambda c, o: c / 3.0,
    "pow_2": lambda c, o: c ** 2,
    "pow_half": lambda c, o: c ** 0.5,
    "pow_m1": lambda c, o: c ** -1,
    "pow_1": lambda c, o: c ** 1,
    "pow_0": lambda c, o: c ** 0,
    "sub_map": lambda c, o: c - o["map"] * K,
    "div_map2": lambda c, o: c / o["map2"],
    "mul_spec3": lambda c, o: c * o["spec"][:, None, None],
    "sub_row": lambda c, o: c - o["row"] * K,
    "add_col": lambda c, o: c + o["col"] * K,
    "mul_zy": lambda c, o: c * o["zy"],
    "mul_jy": lambda c, o: c * (2 * u.Jy),
    "sub_cube": lambda c, o: c - o["cube2"],
    "add_cube": lambda c, o: c + o["cube2"],
    "mul_cube": lambda c, o: c * o["cube2"],
    "div_cube": lambda c, o: c / o["cube2"],
    "chain3": lambda c, o: (c - o["map"] * K) / o["map2"] * 1e3,
    "chain_mul_add": lambda c, o: c * o["map2"] + o["map"] * K,
    # the rows that raise
    "add_plain": lambda c, o: c + 1,
    "sub_plain": lambda c, o: c - 1,
    "sub_spec1": lambda c, o: c - o["spec"] * K,
    "floordiv": lambda c, o: c // 2,
    "pow_cube": lambda c, o: c ** o["cube2"],
    "rmul": lambda c, o: 2 * c,
    "neg": lambda c, o: -c,
    "sub_shape": lambda c, o: c - o["cube2"][:, :, :5],
}
POWERS = {"pow_1p7": 1.7, "pow_m2p5": -2.5}


def header_text(h):
    return "\n".join("%-8s= %r" % (k, v) if isinstance(v, str) else "%-8s= %s" % (k, repr(float(v))) for k, v in h.items())


def arr(q):
    q = q[:] if hasattr(q, "__getitem__") else q
    return np.asarray(getattr(q, "value", q))


def record(out, key, fn):
    try:                                                      # (the Dask class raises for some units only when the data are asked for)
        r = fn()
        raw, filled = arr(r.unmasked_data), arr(r.filled_data)
    except Exception as exc:                                  # noqa: BLE001 - the class name is what is recorded
        out[key + "|raises"] = np.array(type(exc).__name__)
        out[key + "|message"] = np.array(str(exc))
        return None
    assert raw.dtype == np.float32 and filled.dtype == np.float32, (key, raw.dtype, filled.dtype)
    out[key + "|raw"] = raw
    out[key + "|filled"] = filled
    out[key + "|include"] = np.asarray(r.mask.include(), dtype=bool)
    out[key + "|unit"] = np.array(str(r.unit))
    out[key + "|fill"] = np.float64(r.fill_value)
    return r


def pack(out):
    """the per-case entries of every <class>|<fill> stacked into a few arrays (an .npz member costs more than a small cube)"""
    packed = {k: v for k, v in out.items() if k.count("|") < 3}
    for group in sorted({k.rsplit("|", 2)[0] for k in out if k.count("|") == 3}):
        cases = [k.split("|")[2] for k in out if k.startswith(group + "|") and k.count("|") == 3]
        cases = list(dict.fromkeys(cases))
        ok = [c for c in cases if "%s|%s|raw" % (group, c) in out]
        bad = [c for c in cases if "%s|%s|raises" % (group, c) in out]
        assert sorted(ok + bad) == sorted(cases)
        fill = {float(out["%s|%s|fill" % (group, c)]) for c in ok}
        assert len(fill) == 1 or all(np.isnan(f) for f in fill)
        packed[group + "|names"] = np.array(ok)
        packed[group + "|raw"] = np.array([out["%s|%s|raw" % (group, c)] for c in ok])
        # every result keeps the left cube's mask and its filled data are its raw data with the fill value outside it:
        # checked here for every case, so neither is stored per case (`keep` and the fill value say both)
        fv = np.float32(group.split("|")[1])
        for c in ok:
            raw, inc = out["%s|%s|raw" % (group, c)], out["%s|%s|include" % (group, c)]
            assert np.array_equal(inc, out["keep"]), (group, c)
            assert np.array_equal(out["%s|%s|filled" % (group, c)], np.where(inc, raw, fv), equal_nan=True), (group, c)
        packed[group + "|units"] = np.array([str(out["%s|%s|unit" % (group, c)]) for c in ok])
        packed[group + "|raising"] = np.array(bad)
        packed[group + "|raises"] = np.array([str(out["%s|%s|raises" % (group, c)]) for c in bad])
        packed[group + "|messages"] = np.array([str(out["%s|%s|message" % (group, c)]) for c in bad])
    return packed


def main():
    rng = np.random.default_rng(20261018)
    d = rng.normal(size=(NZ, NY, NX)).astype(np.float32)
    d[1, 2, 3] = np.nan
    keep = rng.random(d.shape) < 0.7
    keep[1, 2, 3] = True                                      # the NaN sample is included: it must stay NaN, never the fill
    d2 = (rng.normal(size=d.shape) + 0.5).astype(np.float32)
    d2[4, 0, 1] = np.nan
    keep2 = rng.random(d.shape) < 0.5
    ops = {"map": rng.normal(size=(NY, NX)).astype(np.float32),
           "map2": (0.5 + rng.random((NY, NX))).astype(np.float32),
           "spec": (1.0 + rng.random(NZ)).astype(np.float32),
           "row": rng.normal(size=NX).astype(np.float32),
           "col": rng.normal(size=(NY, 1)).astype(np.float32),
           "zy": (0.5 + rng.random((NZ, NY, 1))).astype(np.float32)}
    powbase = (np.abs(d) + np.float32(0.1)).astype(np.float32)
    w = WCS(HEADER)
    out = {"header": np.array(header_text(HEADER)), "data": d, "keep": keep, "data2": d2, "keep2": keep2, "powbase": powbase,
           "cases": np.array(list(CASES)), "powers": np.array(list(POWERS)), "power_values": np.array(list(POWERS.values())),
           "classes": np.array(["np", "dask"]), "fills": np.array(["nan", "0"])}
    out.update(ops)
    for cls, dask in (("np", False), ("dask", True)):
        cube2 = SpectralCube(d2 * K, wcs=w, use_dask=dask, mask=BooleanArrayMask(keep2, w))
        o = dict(ops, cube2=cube2)
        for fname, fill in (("nan", np.nan), ("0", 0.0)):
            cube = SpectralCube(d * K, wcs=w, use_dask=dask, mask=BooleanArrayMask(keep, w)).with_fill_value(fill)
            for name, fn in CASES.items():
                record(out, "%s|%s|%s" % (cls, fname, name), lambda: fn(cube, o))
            bare = SpectralCube(d * u.dimensionless_unscaled, wcs=w, use_dask=dask, mask=BooleanArrayMask(keep, w)).with_fill_value(fill)
            record(out, "%s|%s|bare_add_1" % (cls, fname), lambda: bare + 1)
            record(out, "%s|%s|bare_sub_1" % (cls, fname), lambda: bare - 1)
            pb = SpectralCube(powbase * u.dimensionless_unscaled, wcs=w, use_dask=dask, mask=BooleanArrayMask(keep, w)).with_fill_value(fill)
            for name, p in POWERS.items():
                record(out, "%s|%s|%s" % (cls, fname, name), lambda: pb ** p)
        # a lazy mask keeps testing the ORIGINAL samples after + 5 K
        plain = SpectralCube(d * K, wcs=w, use_dask=dask)
        r = plain.with_mask(plain > 0.2 * K) + 5 * K
        key = "%s|lazy" % cls
        out[key + "|include"] = np.asarray(r.mask.include(), dtype=bool)
        assert np.array_equal(out[key + "|include"], d > 0.2)
        out[key + "|sum"] = np.float64(r.sum().value)
        out[key + "|moment0"] = np.asarray(r.moment0().value, dtype=np.float64)
        out[key + "|moment0_unit"] = np.array(str(r.moment0().unit))
    raised = sorted(k for k in out if k.endswith("|raises"))
    print("%d entries, %d raise:" % (len(out), len(raised)))
    for k in raised:
        print("   %-28s %s: %s" % (k[:-7], out[k], str(out[k[:-7] + "|message"])[:90]))
    print("units:", sorted({str(out[k]) for k in out if k.endswith("|unit")}))
    np.savez_compressed(OUT, **pack(out))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
