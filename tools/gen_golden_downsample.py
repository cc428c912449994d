"""Generate tests/golden/downsample_axis.npz from the REFERENCE's SpectralCube.downsample_axis (in-memory form).

Run with the reference environment, like oracle/gen_golden.py:

    /opt/conda/bin/python3.9 -B tools/gen_golden_downsample.py

Small float32 cubes with NaNs (11 x 7 x 9) under four mask / fill variants; for axes 0 / 1 / 2 x factors 2, 3, 4 x
truncate both ways and the estimators of each variant it records the reference's unitless_filled_data, its unmasked
data, mask.include() and the output WCS (crpix / cdelt / crval, FITS order).  A CD-matrix header adds the world
coordinates of the output pixel centres: the parent WCS at parent pixel k * f + (f - 1) / 2 (the block-centre rule).
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
from spectral_cube import SpectralCube, BooleanArrayMask, LazyMask  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "downsample_axis.npz")

HEADER = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s",
          "CDELT1": -2e-3, "CDELT2": 2e-3, "CDELT3": 0.5, "CRPIX1": 5.0, "CRPIX2": 4.0, "CRPIX3": 2.0,
          "CRVAL1": 30.0, "CRVAL2": -20.0, "CRVAL3": 4.0, "BUNIT": "K"}
CD_HEADER = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s",
             "CD1_1": -1.8e-3, "CD1_2": 0.6e-3, "CD2_1": 0.5e-3, "CD2_2": 1.9e-3, "CD3_3": 0.25,
             "CRPIX1": 4.5, "CRPIX2": 3.0, "CRPIX3": 1.0, "CRVAL1": 120.0, "CRVAL2": 35.0, "CRVAL3": -3.0, "BUNIT": "K"}

ESTIMATORS = ("nanmean", "nansum", "nanmax", "nanmin", "mean", "sum", "max", "min")
# variant -> (mask kind, fill, estimators): all eight on the boolean-array mask, the rest on a few
VARIANTS = {"bool": ("bool", np.nan, ESTIMATORS),
            "finite": ("finite", np.nan, ("nanmean", "max")),
            "cmp": ("cmp", np.nan, ("nanmean", "sum", "min")),
            "bool_fill0": ("bool", 0.0, ("nanmean", "mean", "nansum"))}
THRESHOLD = 0.2


def header_text(h):
    return "\n".join("%-8s= %r" % (k, v) if isinstance(v, str) else "%-8s= %s" % (k, repr(float(v))) for k, v in h.items())


def make_data():
    rng = np.random.default_rng(20261016)
    d = rng.normal(0.5, 1.0, (11, 7, 9)).astype(np.float32)
    d[rng.random(d.shape) < 0.08] = np.nan
    d[3, :, 4] = np.nan                   # a whole run of NaN along y
    d[:, 2, 6] = np.nan                   # and along the spectral axis
    d[6, 5, :] = np.nan                   # and along x
    keep = rng.random(d.shape) < 0.75
    keep[:, 1, 2] = False                 # a spaxel masked throughout
    keep[8, :, :] = False                 # a plane masked throughout
    return d, keep


def ref_cube(d, keep, kind, header):
    w = WCS(header)
    cube = SpectralCube(data=d * u.K, wcs=w, mask=LazyMask(np.isfinite, data=d, wcs=w))
    if kind == "bool":
        cube = cube.with_mask(BooleanArrayMask(keep, wcs=w), inherit_mask=False)
    elif kind == "cmp":
        cube = cube.with_mask(cube > THRESHOLD * u.K)
    return cube


def main():
    d, keep = make_data()
    out = {"data": d, "keep": keep, "header": np.array(header_text(HEADER)), "threshold": np.float64(THRESHOLD),
           "variants": np.array(sorted(VARIANTS)), "estimators": np.array(ESTIMATORS)}
    base = ref_cube(d, keep, "finite", HEADER)
    for axis in (0, 1, 2):
        for f in (2, 3, 4):
            for trunc in (False, True):
                tag = "a%d_f%d_t%d" % (axis, f, int(trunc))
                ds = base.downsample_axis(f, axis, truncate=trunc, use_memmap=False)
                out["wcs_" + tag] = np.array([ds.wcs.wcs.crpix, ds.wcs.wcs.cdelt, ds.wcs.wcs.crval], dtype=np.float64)
                out["shape_" + tag] = np.array(ds.shape, dtype=np.int64)
    names, filled, unmasked, include = [], [], [], []
    for vname, (kind, fill, ests) in VARIANTS.items():
        cube = ref_cube(d, keep, kind, HEADER)
        if fill == fill:
            cube = cube.with_fill_value(fill)
        for axis in (0, 1, 2):
            for f in (2, 3, 4):
                for trunc in (False, True):
                    for est in ests:
                        ds = cube.downsample_axis(f, axis, estimator=getattr(np, est), truncate=trunc, use_memmap=False)
                        names.append("%s_a%d_f%d_t%d_%s" % (vname, axis, f, int(trunc), est))
                        filled.append(np.asarray(ds.unitless_filled_data[:], dtype=np.float32).ravel())
                        unmasked.append(np.asarray(ds.unmasked_data[:].value, dtype=np.float32).ravel())
                        include.append(np.asarray(ds.mask.include(), dtype=bool).ravel())
    # (one array per quantity, the cases back to back: a file per case would cost more in zip entries than in data)
    out["case_names"] = np.array(names)
    out["case_offsets"] = np.cumsum([0] + [len(a) for a in filled]).astype(np.int64)
    out["filled"] = np.concatenate(filled)
    out["unmasked"] = np.concatenate(unmasked)
    out["include"] = np.packbits(np.concatenate(include))
    # CD-matrix header: world coordinates of every output pixel centre = the parent WCS at the block centre
    wcd = WCS(CD_HEADER)
    out["cd_header"] = np.array(header_text(CD_HEADER))
    cd_shape = (6, 8, 10)
    out["cd_shape"] = np.array(cd_shape, dtype=np.int64)
    for axis in (0, 1, 2):
        for f in (2, 3):
            n_out = -(-cd_shape[axis] // f)
            grids = [np.arange(s, dtype=np.float64) for s in cd_shape]
            grids[axis] = np.arange(n_out) * f + (f - 1) / 2.0
            zz, yy, xx = np.meshgrid(*grids, indexing="ij")
            world = wcd.wcs_pix2world(np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1), 0)
            out["cdworld_a%d_f%d" % (axis, f)] = world
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
