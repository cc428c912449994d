"""Generate tests/golden/stack_spectra.npz from the REFERENCE's analysis_utilities.stack_spectra.

Run with the reference environment, like tools/gen_golden_rank_filter.py:

    /opt/conda/bin/python3.9 -B tools/gen_golden_stack_spectra.py

The stub radio_beam of that environment cannot build a beam and stack_spectra reads ``cube.beam``: this process overrides
``spectral_cube.base_class.BeamMixinClass.beam`` with a property returning None.

Three variants of a small float32 cube of Gaussian lines (centres spread over 8 channels, 5 % NaN, one all-NaN spaxel, one
NaN in the velocity map): ``even`` (24 x 6 x 7), ``odd`` (25 channels) and ``decreasing`` (24 channels, CDELT3 < 0).  Per
variant the cases ``default``, ``posns`` (explicit xy_posns), ``v0`` (v0 given), ``oor`` (one velocity outside the axis) and
``bool0`` (a boolean mask with fill value 0), each with pad_edges True / False and np.nanmean / np.mean / np.nanmedian.
Recorded: the stacked spectrum, CRPIX1, NAXIS1, the pixel shifts and positions, and for a few cases the shifted rows (what
the reference hands to stack_function).

Before anything is written the float64 direct-sum restatement the tests use is checked against the reference's rows, and
no shifted NaN indicator may lie within 1e-6 of the 0.5 threshold (the smallest distance is recorded).
No test imports this file; only its output is committed.
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
from spectral_cube.analysis_utilities import stack_spectra  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "stack_spectra.npz")
HEADER = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s",
          "CDELT1": -2e-3, "CDELT2": 2e-3, "CDELT3": 0.5, "CRPIX1": 5.0, "CRPIX2": 4.0, "CRPIX3": 2.0,
          "CRVAL1": 30.0, "CRVAL2": -20.0, "CRVAL3": 4.0, "BUNIT": "K"}
NY, NX = 6, 7
VARIANTS = {"even": (24, 0.5), "odd": (25, 0.5), "decreasing": (24, -0.5)}
CASES = ("default", "posns", "v0", "oor", "bool0")
FUNCS = {"nanmean": np.nanmean, "mean": np.mean, "nanmedian": np.nanmedian}
ROWS_OF = (("even", "default", True), ("odd", "default", True), ("decreasing", "bool0", False), ("even", "oor", False))


def header_text(h):
    return "\n".join("%-8s= %r" % (k, v) if isinstance(v, str) else "%-8s= %s" % (k, repr(float(v))) for k, v in h.items())


def kernel(t, M):
    """h_M(t): the reference's fft / phase ramp / ifft as a circular convolution kernel"""
    t = np.asarray(t, dtype=np.float64)
    a = np.pi * t / M
    with np.errstate(all="ignore"):
        h = np.sin(np.pi * t) / (M * (np.sin(a) if M % 2 else np.tan(a)))
    whole = np.abs(((t + M / 2.0) % M) - M / 2.0) < 1e-12
    return np.where(whole, 1.0, h)


def shift_rows(filled, idx, shifts, pad):
    """the statement the GPU tests check against: (rows (P, M), indicator (P, M)) by the float64 direct sum"""
    nz = filled.shape[0]
    M = nz + pad[0] + pad[1]
    n = np.arange(M)
    flat = filled.reshape(nz, -1)
    rows, inds = np.full((len(idx), M), np.nan), np.zeros((len(idx), M))
    for p, (i, s) in enumerate(zip(idx, shifts)):
        x = flat[:, i].astype(np.float64)
        bad = ~np.isfinite(x)
        if bad.all() or not np.isfinite(s):
            continue
        H = kernel(n[:, None] - n[None, :] - s, M)
        rows[p] = H @ np.pad(np.where(bad, 0.0, x), pad)
        if bad.any():
            inds[p] = H @ np.pad(bad.astype(np.float64), pad)
            rows[p][inds[p] > 0.5] = np.nan
    return rows, inds


def make(nz, seed):
    rng = np.random.default_rng(seed)
    z = np.arange(nz)[:, None, None]
    cen = nz / 2.0 - 4.0 + 8.0 * rng.random((NY, NX))
    d = (np.exp(-0.5 * ((z - cen) / 1.5) ** 2) + 0.01 * rng.normal(size=(nz, NY, NX))).astype(np.float32)
    d[rng.random(d.shape) < 0.05] = np.nan
    d[:, 4, 5] = np.nan                                  # an all-NaN spaxel
    keep = rng.random(d.shape) < 0.85
    return d, cen, keep


def main():
    out = {"funcs": np.array(list(FUNCS)), "cases": np.array(CASES), "variants": np.array(list(VARIANTS))}
    closest, worst, nstack = np.inf, 0.0, 0
    keys, idx_all, shifts_all, vels, v0s, explicit = [], [], [], [], [], []       # per variant|case
    pkeys, pads, crpix1, naxis1, stacks = [], [], [], [], []                      # per variant|case|pad (stacks: x funcs)
    for vi, (variant, (nz, cdelt)) in enumerate(VARIANTS.items()):
        hdr = dict(HEADER, CDELT3=cdelt)
        w = WCS(hdr)
        d, cen, keep = make(nz, 20261017 + vi)
        plain = SpectralCube(d * u.K, wcs=w)
        axis_kms = plain.spectral_axis.to(u.km / u.s).value
        vel = axis_kms[0] + cdelt * cen                  # km/s: the velocity of each line centre
        vel[1, 2] = np.nan
        out.update({variant + "|header": np.array(header_text(hdr)), variant + "|data": d, variant + "|keep": keep})
        for case in CASES:
            cube, filled, v, kw = plain, d, vel.copy(), {}
            if case == "posns":
                ys, xs = np.where(np.isfinite(vel))
                kw["xy_posns"] = (ys[::2][::-1].copy(), xs[::2][::-1].copy())
            if case == "v0":
                kw["v0"] = (axis_kms[nz // 3] + 0.2 * cdelt) * u.km / u.s
            if case == "oor":
                v[2, 3] = axis_kms.max() + 3.7
            if case == "bool0":
                cube = SpectralCube(d * u.K, wcs=w, mask=BooleanArrayMask(keep, wcs=w)).with_fill_value(0.0)
                filled = np.where(keep, d, np.float32(0.0))
            posns = kw.get("xy_posns", np.where(np.isfinite(v)))
            idx = posns[0] * NX + posns[1]
            # the reference's pixel shifts, restated with its quantities (analysis_utilities.py:215-244)
            sa = cube.spectral_axis
            v0 = kw.get("v0", sa.mean())
            size = np.diff(sa[:2])[0]
            sign = -1.0 if size.value > 0 else 1.0
            vq = (v * u.km / u.s).to(sa.unit)
            masked = np.where((vq < sa.max()) & (vq > sa.min()), vq.value, np.nan) * sa.unit
            shifts = sign * ((masked - v0.to(sa.unit)) / np.abs(size)).value[posns]
            key = "%s|%s" % (variant, case)
            keys.append(key)
            idx_all.append(idx.astype(np.int64))
            shifts_all.append(shifts)
            vels.append(v)
            v0s.append(kw["v0"].value if "v0" in kw else np.nan)
            explicit.append("xy_posns" in kw)            # (the positions are then (idx // NX, idx % NX), in this order)
            for pad_edges in (True, False):
                grabbed = []

                def grab(a, axis=0):
                    grabbed.append(np.array(a))
                    return np.nanmean(a, axis=axis)
                stack_spectra(cube, v * u.km / u.s, stack_function=grab, pad_edges=pad_edges, **kw)
                ref_rows = grabbed[0]
                pad = (0, 0)
                if pad_edges:
                    pad = (-min(0, int(np.ceil(np.nanmin(shifts)))), max(0, int(np.ceil(np.nanmax(shifts)))))
                rows, inds = shift_rows(filled, idx, shifts, pad)
                assert rows.shape == ref_rows.shape, (key, rows.shape, ref_rows.shape)
                assert np.array_equal(np.isnan(rows), np.isnan(ref_rows)), key
                ok = np.isfinite(ref_rows)
                worst = max(worst, np.abs(rows[ok] - ref_rows[ok]).max())
                some = inds.any(axis=1)
                if some.any():
                    closest = min(closest, np.abs(inds[some] - 0.5).min())
                pkey = key + "|pad%d" % pad_edges
                pkeys.append(pkey)
                pads.append(pad)
                if (variant, case, pad_edges) in ROWS_OF:
                    out[pkey + "|rows"] = ref_rows
                for fname, fn in FUNCS.items():
                    s = stack_spectra(cube, v * u.km / u.s, stack_function=fn, pad_edges=pad_edges, **kw)
                    val = np.asarray(s.value, dtype=np.float64)
                    assert val.shape == (nz + pad[0] + pad[1],)
                    stacks.append(val)
                    nstack += 1
                crpix1.append(float(s.header["CRPIX1"]))
                naxis1.append(int(s.header.get("NAXIS1", val.size)))
    assert worst <= 1e-12, worst
    assert closest >= 1e-6, closest
    # few, large members: every member of an .npz costs some hundred bytes of headers
    out.update({"keys": np.array(keys), "npos": np.array([a.size for a in idx_all]), "idx": np.concatenate(idx_all),
                "shifts": np.concatenate(shifts_all), "vels": np.array(vels), "v0": np.array(v0s), "explicit_posns": np.array(explicit),
                "pkeys": np.array(pkeys), "pads": np.array(pads, dtype=np.int64), "crpix1": np.array(crpix1),
                "naxis1": np.array(naxis1, dtype=np.int64), "stacks": np.concatenate(stacks)})
    out["indicator_min_distance"] = np.float64(closest)
    out["restatement_max_difference"] = np.float64(worst)
    np.savez_compressed(OUT, **out)
    print("restatement - reference rows: %.2e at most; closest shifted indicator to 0.5: %.2e" % (worst, closest))
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", nstack, "stacks")


if __name__ == "__main__":
    main()
