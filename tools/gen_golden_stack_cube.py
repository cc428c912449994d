"""Generate tests/golden/stack_cube.npz from the REFERENCE's analysis_utilities.stack_cube.

Run with the reference environment, like tools/gen_golden_stack_spectra.py (the same ``beam`` override):

    /opt/conda/bin/python3.9 -B tools/gen_golden_stack_cube.py

A small float32 FREQ cube (160 x 5 x 6, 0.5 MHz channels at 100 GHz = 1.5 km/s, 5 % NaN, one all-NaN spaxel) in two
variants, ``inc`` (CDELT3 > 0: the velocity axis decreases) and ``dec`` (CDELT3 < 0).  Cases per variant: ``l3`` (3 lines),
``l5`` (5 lines: one whose window runs off the band edge, one entirely outside the band and therefore skipped) and ``bool0``
(3 lines, a boolean mask, fill value 0), each with np.nanmean / np.mean / np.nansum / np.nanmedian, through the Dask class
(``use_dask=True``: the interpolation this project mirrors).  Recorded per case: the stacked cubes, the included lines, every
surviving line's slab bounds in channels (the reference's own ``closest_spectral_channel``), the output grid and the spectral
WCS keys; the cutouts for two cases; and the plain class's result for one case (``plain|dec|l3``), which clamps at a slab's
ends where the Dask class gives NaN - recorded to document that difference, tested nowhere.

The reference's mask on a decreasing grid.  ``DaskSpectralCubeMixin.spectral_interpolate`` takes ``~isnan(newcube)`` as the
new mask BEFORE it flips ``newcube`` back to a decreasing output grid (dask_spectral_cube.py:1364-1367), so the mask of such
a result is the mirror image, along the spectral axis, of the one that fits its data, and ``filled_data`` - what stack_cube
averages - carries the fill value wherever the data OR its mirror image is NaN.  Every ``inc`` case has a decreasing grid.
The restatement below has that line as the reference has it (``mirror=True``); with ``mirror=False`` it is the operation
this project builds (the mask that fits the data).  ``mirror_differs`` counts the stacked voxels the two disagree on.

Before anything is written the float64 restatement (``mirror=True``) is checked against the reference: equal slab bounds,
identical NaN pattern, and values within 8 * 2**-24 * max |finite input| (``restatement_distance`` is the largest found).
Three margins are asserted, so that the 1e-16-level difference between c (f0 - f) / f0 and astropy's converted linear WCS
cannot flip an integer decision (``margin`` is the smallest found, in channels): no closest-channel decision within 1e-6
channel of a tie, no grid point of a non-reference line within 1e-6 channel of an input node, none within 1e-6 channel of a
slab's end.  No test imports this file; only its output is committed.
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
from spectral_cube.analysis_utilities import stack_cube  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "stack_cube.npz")
HEADER = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "FREQ", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "Hz",
          "CDELT1": -2e-3, "CDELT2": 2e-3, "CDELT3": 0.5e6, "CRPIX1": 3.0, "CRPIX2": 3.0, "CRPIX3": 2.0,
          "CRVAL1": 30.0, "CRVAL2": -20.0, "CRVAL3": 100.0e9, "BUNIT": "K"}
NZ, NY, NX = 160, 5, 6
VMIN, VMAX = -8.3, 9.1                                   # km/s
C_KMS = 299792.458
VARIANTS = {"inc": 0.5e6, "dec": -0.5e6}
# line positions in (fractional) channels; 400.0 lies outside the band, the window of 3.29 runs off its edge
CASES = {"l3": (30.37, 71.81, 118.23), "l5": (30.37, 400.0, 71.81, 3.29, 118.23), "bool0": (30.37, 71.81, 118.23)}
FUNCS = {"nanmean": np.nanmean, "mean": np.mean, "nansum": np.nansum, "nanmedian": np.nanmedian}
CUTOUTS_OF = (("inc", "l5"), ("dec", "bool0"))
PLAIN_OF = ("dec", "l3")


def header_text(h):
    return "\n".join("%-8s= %r" % (k, v) if isinstance(v, str) else "%-8s= %s" % (k, repr(float(v))) for k, v in h.items())


def slab_plan(freq, lines, vmin, vmax):
    """[(line, ilo, ihi, velocity axis of the whole cube)] of the lines whose slab has more than one channel, and the
    smallest distance (in channels) of a closest-channel decision from a tie"""
    out, margin = [], np.inf
    for f0 in lines:
        v = C_KMS * (f0 - freq) / f0
        ends = []
        for bound in (vmin, vmax):
            ends.append(int(np.argmin(np.abs(v - bound))))
            p = (bound - v[0]) / (v[1] - v[0])
            if 0.0 <= p <= len(v) - 1.0:
                margin = min(margin, abs(p - np.floor(p) - 0.5))
        ilo, ihi = min(ends), max(ends)
        if ihi - ilo + 1 > 1:
            out.append((f0, ilo, ihi, v))
    return out, margin


def interp(x, y, grid, mirror):
    """DaskSpectralCubeMixin.spectral_interpolate (dask_spectral_cube.py:1291-1373) on float64: (filled with NaN, include)"""
    rin, rout = np.mean(np.diff(x)) < 0, np.mean(np.diff(grid)) < 0
    if rin:
        x, y = x[::-1], y[::-1]
    if rout:
        grid = grid[::-1]
    idx = np.clip(np.searchsorted(x, grid), 1, len(x) - 1)
    lo = idx - 1
    with np.errstate(invalid="ignore"):
        slope = (y[idx] - y[lo]) / (x[idx] - x[lo])[:, None, None]
        new = slope * (grid - x[lo])[:, None, None] + y[lo]
    new[(grid < x[0]) | (grid > x[-1])] = np.nan
    q = (grid - x[0]) / (x[1] - x[0])                         # grid points in channels of this slab
    margin = min(np.abs(q - np.round(q)).min(), np.abs(q).min(), np.abs(q - (len(x) - 1)).min())
    include = ~np.isnan(new)                                  # :1364, before the flip of :1366-1367
    if rout:
        new = new[::-1]
        if not mirror:
            include = include[::-1]
    return new, include, margin


def restate(d, inc, fill, freq, lines, vmin, vmax, mirror):
    """steps 1 - 4 of stack_cube in float64: (cutouts, plan, smallest margin)"""
    plan, margin = slab_plan(freq, lines, vmin, vmax)
    if not plan:
        raise ValueError("no line survives")
    d64 = d.astype(np.float64)
    f0, ilo, ihi, v = plan[0]
    grid = v[ilo:ihi + 1]
    cuts = [np.where(inc, d64, fill)[ilo:ihi + 1]]
    for f0, ilo, ihi, v in plan[1:]:
        new, include, m = interp(v[ilo:ihi + 1], np.where(inc, d64, np.nan)[ilo:ihi + 1], grid, mirror)
        margin = min(margin, m)
        cuts.append(np.where(include, new, fill))
    return cuts, plan, margin


def make(seed):
    rng = np.random.default_rng(seed)
    z = np.arange(NZ)[:, None, None]
    d = 0.05 * rng.normal(size=(NZ, NY, NX))
    for cen in (30.37, 71.81, 118.23, 3.29):
        d += (0.5 + rng.random((NY, NX))) * np.exp(-0.5 * ((z - cen) / 1.7) ** 2)
    d = d.astype(np.float32)
    d[rng.random(d.shape) < 0.05] = np.nan
    d[:, 3, 4] = np.nan                                  # an all-NaN spaxel
    keep = rng.random(d.shape) < 0.85
    return d, keep


def main():
    out = {"funcs": np.array(list(FUNCS)), "cases": np.array(list(CASES)), "variants": np.array(list(VARIANTS)),
           "vmin": np.float64(VMIN), "vmax": np.float64(VMAX)}
    worst, margin, differs = 0.0, np.inf, 0
    for vi, (variant, cdelt) in enumerate(VARIANTS.items()):
        hdr = dict(HEADER, CDELT3=cdelt)
        w = WCS(hdr)
        d, keep = make(20261018 + vi)
        freq = hdr["CRVAL3"] + cdelt * (np.arange(NZ) + 1.0 - hdr["CRPIX3"])
        scale = float(np.abs(d[np.isfinite(d)]).max())
        out.update({variant + "|header": np.array(header_text(hdr)), variant + "|data": d, variant + "|keep": keep})
        for case, positions in CASES.items():
            key = "%s|%s" % (variant, case)
            lines = np.array([freq[0] + cdelt * p for p in positions])
            inc, fill = np.isfinite(d), np.nan
            if case == "bool0":
                inc, fill = inc & keep, 0.0
            for dask in ((True, False) if (variant, case) == PLAIN_OF else (True,)):
                cube = SpectralCube(d * u.K, wcs=w, use_dask=dask, mask=BooleanArrayMask(inc, wcs=w)).with_fill_value(fill)
                assert np.allclose(cube.spectral_axis.to(u.Hz).value, freq, rtol=1e-15)
                res, ref_cuts = stack_cube(cube, [f * u.Hz for f in lines], VMIN * u.km / u.s, VMAX * u.km / u.s,
                                           return_cutouts=True)
                if not dask:
                    out["plain|" + key] = np.asarray(res.unmasked_data[:].value, dtype=np.float64)
                    continue
                cuts, plan, m = restate(d, inc, fill, freq, lines, VMIN, VMAX, mirror=True)
                honest, _, _ = restate(d, inc, fill, freq, lines, VMIN, VMAX, mirror=False)
                margin = min(margin, m)
                # slab bounds by the reference's own closest-channel search on its velocity axis
                bounds = []
                for f0 in lines:
                    lc = cube.with_spectral_unit(u.km / u.s, velocity_convention="radio", rest_value=f0 * u.Hz)
                    a, b = lc.closest_spectral_channel(VMIN * u.km / u.s), lc.closest_spectral_channel(VMAX * u.km / u.s)
                    if abs(a - b) + 1 > 1:
                        bounds.append((min(a, b), max(a, b)))
                assert bounds == [(p[1], p[2]) for p in plan], (key, bounds, plan)
                included = np.array([q.to(u.Hz).value for q in res.meta["stacked_lines"]])
                assert np.array_equal(included, np.array([p[0] for p in plan])), key
                assert len(ref_cuts) == len(cuts)
                for a, b in zip(ref_cuts, cuts):
                    a = np.asarray(a, dtype=np.float64)
                    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), key
                    ok = np.isfinite(a)
                    worst = max(worst, np.abs(a[ok] - b[ok]).max() / scale)
                grid = plan[0][3][plan[0][1]:plan[0][2] + 1]
                assert np.allclose(res.spectral_axis.to(u.km / u.s).value, grid, rtol=1e-12, atol=0.0), key
                h = res.header
                assert res.wcs.wcs.restfrq == 0.0 and "RESTFRQ" not in h and "RESTFREQ" not in h
                out.update({key + "|lines": lines, key + "|included": included, key + "|bounds": np.array(bounds, dtype=np.int64),
                            key + "|grid": res.spectral_axis.to(u.km / u.s).value,
                            key + "|wcs3": np.array([h["CRPIX3"], h["CRVAL3"], h["CDELT3"]], dtype=np.float64),
                            key + "|ctype3": np.array(h["CTYPE3"]), key + "|cunit3": np.array(h["CUNIT3"])})
                if (variant, case) in CUTOUTS_OF:
                    out[key + "|cutouts"] = np.array([np.asarray(c, dtype=np.float64) for c in ref_cuts])
                stacks = []
                for fname, fn in FUNCS.items():
                    s = stack_cube(cube, [f * u.Hz for f in lines], VMIN * u.km / u.s, VMAX * u.km / u.s, average=fn)
                    val = np.asarray(s.unmasked_data[:].value, dtype=np.float64)
                    mine, mine_honest = fn(cuts, axis=0), fn(honest, axis=0)
                    assert np.array_equal(np.isnan(val), np.isnan(mine)), (key, fname)
                    ok = np.isfinite(val)
                    worst = max(worst, np.abs(val[ok] - mine[ok]).max() / (scale * (len(cuts) if "sum" in fname else 1)))
                    differs += int((~np.isclose(mine, mine_honest, rtol=1e-9, atol=0.0, equal_nan=True)).sum())
                    stacks.append(val)
                out[key + "|stacks"] = np.array(stacks)
    assert worst < 8 * 2.0 ** -24, worst
    assert margin >= 1e-6, margin
    out["restatement_distance"] = np.float64(worst)          # relative to max |finite input| (x lines for the sums)
    out["margin"] = np.float64(margin)
    out["mirror_differs"] = np.int64(differs)
    np.savez_compressed(OUT, **out)
    print("restatement - reference: %.3e of max |input| at most; smallest margin %.3e channel; %d stacked voxels differ with "
          "the mirrored mask" % (worst, margin, differs))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
