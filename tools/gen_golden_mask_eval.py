"""Generate tests/golden/mask_eval.npz from the REFERENCE's ``cube.with_mask(...).get_mask_array()`` for the mask
expressions the package evaluates on the device (ops.mask_eval): thresholds that are maps, ``|``, ``~``, a term on a
second cube, a 2-D region map.

Run with the reference environment, like tools/gen_golden_downsample.py:

    /opt/conda/bin/python3.9 -B tools/gen_golden_mask_eval.py

A small float32 cube (9 x 6 x 10, in K, samples on a grid of 1/8 with NaN, +-inf, +-0 and samples equal to the
thresholds), a positive noise map ``rms`` on the same grid and a second cube (the reference's
``spectral_smooth(Gaussian1DKernel(2))`` of the first, stored as data so that the comparison does not depend on how a
smoothing rounds).  Every threshold is a Quantity map in K - the reference compares a cube with a unit against
Quantities only.  Stored per idiom: ``np.packbits`` of the include map.  No test imports this file; only its output is
committed.
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
from astropy.convolution import Gaussian1DKernel  # noqa: E402
from astropy.wcs import WCS  # noqa: E402
from spectral_cube import SpectralCube  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "mask_eval.npz")
HEADER = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s",
          "CDELT1": -2e-3, "CDELT2": 2e-3, "CDELT3": 0.5, "CRPIX1": 5.0, "CRPIX2": 3.0, "CRPIX3": 2.0,
          "CRVAL1": 30.0, "CRVAL2": -20.0, "CRVAL3": 4.0, "BUNIT": "K"}
SHAPE = (9, 6, 10)


def header_text(h):
    return "\n".join("%-8s= %r" % (k, v) if isinstance(v, str) else "%-8s= %s" % (k, repr(float(v))) for k, v in h.items())


def main():
    rng = np.random.default_rng(20261017)
    data = (np.round(rng.normal(0.0, 1.5, SHAPE) * 8) / 8).astype(np.float32)
    rms = (rng.integers(1, 4, size=SHAPE[1:]) / 8).astype(np.float32)           # 1/8, 2/8, 3/8: 3 rms and 5 rms on the grid
    flat = data.reshape(-1)
    for i, v in enumerate((np.nan, np.inf, -np.inf, 0.0, -0.0, np.nan)):
        flat[17 + 41 * i] = v
    data[4] = np.where(rng.random(SHAPE[1:]) < 0.5, 3 * rms, data[4])            # samples EQUAL to a threshold
    data[5] = np.where(rng.random(SHAPE[1:]) < 0.5, -5 * rms, data[5])
    region = rng.random(SHAPE[1:]) < 0.6
    w = WCS(HEADER)
    cube = SpectralCube(data=data * u.K, wcs=w)
    # the smoothed cube as DATA: NaN / inf samples spread, which is as good a second cube as any
    smooth = np.asarray(cube.with_mask(np.isfinite(data)).spectral_smooth(Gaussian1DKernel(2)).unmasked_data[:].value, dtype=np.float32)
    other = SpectralCube(data=smooth * u.K, wcs=w)
    q = lambda a: a * u.K                                                         # noqa: E731
    idioms = {
        "sig": cube.with_mask(cube > q(3 * rms)),
        "wing": cube.with_mask((cube > q(5 * rms)) | (cube < q(-5 * rms))),
        "off": cube.with_mask(~(cube > q(3 * rms))),
        "dil": cube.with_mask(other > q(2 * rms)),
        "roi": cube.with_mask(region),
        "ge_or_eq": cube.with_mask((cube >= q(3 * rms)) ^ (cube == q(-5 * rms))),
        "ne": cube.with_mask(cube != q(3 * rms)),
    }
    out = {"header": np.array(header_text(HEADER)), "data": data, "rms": rms, "smooth": smooth, "region": region,
           "names": np.array(sorted(idioms))}
    for name, c in idioms.items():
        inc = np.asarray(c.get_mask_array())
        assert inc.shape == SHAPE and inc.dtype == bool
        out["include_" + name] = np.packbits(inc)
        print("%-9s includes %3d of %d" % (name, inc.sum(), inc.size))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
