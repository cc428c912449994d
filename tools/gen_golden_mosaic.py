"""Generate tests/golden/mosaic.npz from the REFERENCE's cube_utils.combine_headers / mosaic_cubes.

Run with the reference environment, like tools/gen_golden_stack_cube.py (the same ``beam`` override):

    /opt/conda/bin/python3.9 -B tools/gen_golden_mosaic.py

The reference's two routines run as they are.  The ``reproject`` package they import is not available there: underneath
them sits tools/reproject_standin (on sys.path for this script only), this project's restatement of ``reproject_interp``
and ``mosaicking.find_optimal_celestial_wcs`` from their published steps, with astropy.wcs and scipy.ndimage.  What the
vectors pin is therefore the reference's glue (pairwise headers in list order, filled data, nan_to_num, the channel-0
weight, the division) on top of that restatement, not the package itself.

Header pairs (``pair|<name>|...``): both input headers, the resulting celestial keywords (CRVAL1, CRVAL2, CRPIX1, CRPIX2,
CDELT1, CDELT2: unrounded in ``values``, as the header's 14-digit text gives them in ``header_values``), CTYPE1 / CTYPE2,
NAXIS1 / NAXIS2, and astropy's pixel maps of both inputs on the resulting grid.
``identical`` (an unrotated TAN field with itself), ``offset`` (two offset TAN fields), ``scales`` (different pixel
scales), ``rotated`` (the second field rotated by 30 degrees), ``sin_tan`` (SIN + TAN), ``galactic`` (a Galactic pair) and
``kwargs`` (projection, resolution and reference given).

Mosaics (``mos|<name>|...``): ``three`` - float32 sources of shapes (5, 9, 11), (5, 7, 13) and (5, 12, 6), offset fields, the
second rotated by about 30 degrees, each with about 5 % NaN and one +inf sample; the first and third carry the reader's
finite-value mask, the second a boolean mask (which leaves the +inf sample out and keeps NaN samples) with fill value 0;
orders nearest and bilinear.  ``split`` - the two-thirds split of the reference's test_mosaic_cubes on a (4, 9, 6) cube,
nearest.  Recorded: the sources (data, header, boolean mask, fill value), the target header, the result per order (float64),
the weight map (the sum of the stand-in's footprints) and astropy's pixel maps of every source.

Asserted before anything is written (``three``): at least 10 % of the output pixels have weight >= 2, one has weight 3, at
least 10 % have weight 0, a NaN sample lies inside a footprint, and no source position is within 1e-6 pixel of a
nearest-neighbour tie or of the +-0.5 border (``margin`` is the smallest distance found), so that astropy-versus-SimpleWCS
rounding cannot flip a decision.  No test imports this file; only its output is committed.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle", "ref_env"))
sys.path.insert(0, os.path.join(HERE, "reproject_standin"))

from bootstrap import load_reference  # noqa: E402

load_reference()
warnings.simplefilter("ignore")

from astropy import units as u  # noqa: E402
from astropy.io import fits  # noqa: E402
from astropy.wcs import WCS  # noqa: E402
import spectral_cube.base_class as B  # noqa: E402
from spectral_cube import SpectralCube, BooleanArrayMask, LazyMask  # noqa: E402

B.BeamMixinClass.beam = property(lambda self: None, lambda self, v: None)
from spectral_cube.cube_utils import combine_headers, mosaic_cubes  # noqa: E402
import reproject  # noqa: E402  (the stand-in)
from reproject.mosaicking import find_optimal_celestial_wcs  # noqa: E402

assert reproject.__file__.startswith(HERE), reproject.__file__

OUT = os.path.join(REPO, "tests", "golden", "mosaic.npz")
KEYS = ("CRVAL1", "CRVAL2", "CRPIX1", "CRPIX2", "CDELT1", "CDELT2")


def base(ctype=("RA---TAN", "DEC--TAN"), crval=(30.0, -20.0), crpix=(4.0, 5.0), cdelt=2e-3, shape=(5, 9, 11), rot=None, **kw):
    h = {"NAXIS": 3, "NAXIS1": shape[2], "NAXIS2": shape[1], "NAXIS3": shape[0],
         "CTYPE1": ctype[0], "CTYPE2": ctype[1], "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s",
         "CRVAL1": crval[0], "CRVAL2": crval[1], "CRVAL3": -10.0, "CRPIX1": crpix[0], "CRPIX2": crpix[1], "CRPIX3": 1.0,
         "CDELT1": -cdelt, "CDELT2": cdelt, "CDELT3": 1.5, "BUNIT": "K"}
    if rot is not None:
        c, s = np.cos(np.radians(rot)), np.sin(np.radians(rot))
        h.update({"PC1_1": c, "PC1_2": -s, "PC2_1": s, "PC2_2": c})
    h.update(kw)
    return h


def header_text(h):
    lines = []
    for k in h.keys():
        if k in ("", "COMMENT", "HISTORY"):
            continue
        v = h[k]
        if isinstance(v, str):
            lines.append("%-8s= %r" % (k, v))
        elif isinstance(v, (bool, np.bool_)):
            lines.append("%-8s= %s" % (k, "T" if v else "F"))
        elif isinstance(v, (int, np.integer)):
            lines.append("%-8s= %d" % (k, v))
        else:
            lines.append("%-8s= %s" % (k, repr(float(v))))
    return "\n".join(lines)


def to_fits(h):
    out = fits.Header()
    for k, v in h.items():
        out[k] = v
    return out


PAIRS = {
    "identical": (base(), base(), {}),
    "offset": (base(), base(crval=(30.011, -19.993), crpix=(6.0, 3.0), shape=(5, 7, 13)), {}),
    "scales": (base(), base(crval=(30.006, -20.004), cdelt=1.3e-3, shape=(5, 14, 10)), {}),
    "rotated": (base(), base(crval=(30.009, -19.995), rot=30.0, shape=(5, 7, 13)), {}),
    "sin_tan": (base(ctype=("RA---SIN", "DEC--SIN")), base(crval=(30.008, -20.006), shape=(5, 12, 6)), {}),
    "galactic": (base(ctype=("GLON-TAN", "GLAT-TAN"), crval=(134.37, -31.94)),
                 base(ctype=("GLON-TAN", "GLAT-TAN"), crval=(134.36, -31.93), rot=-17.0, shape=(5, 8, 8)), {}),
    "kwargs": (base(), base(crval=(30.011, -19.993), shape=(5, 7, 13)),
               {"projection": "SIN", "resolution": 1.5e-3, "reference": (30.004, -19.998)}),
}


def do_pairs(out):
    for name, (h1, h2, kw) in PAIRS.items():
        kwargs = dict(kw)
        if "resolution" in kwargs:
            kwargs["resolution"] = kwargs["resolution"] * u.deg
        if "reference" in kwargs:
            from astropy.coordinates import SkyCoord
            kwargs["reference"] = SkyCoord(kwargs["reference"][0], kwargs["reference"][1], unit="deg", frame="icrs")
        res = combine_headers(to_fits(h1), to_fits(h2), **kwargs)
        assert res["NAXIS"] == 3 and res["WCSAXES"] == 3 and res["NAXIS3"] == h1["NAXIS3"]
        key = "pair|%s|" % name
        out[key + "h1"], out[key + "h2"] = np.array(header_text(h1)), np.array(header_text(h2))
        # the header carries astropy's to_header() text: 14 significant digits.  The same call, unrounded, is what the tests
        # compare against; the header's own values are recorded beside it and must be its rounding
        w1, w2 = WCS(to_fits(h1)).celestial, WCS(to_fits(h2)).celestial
        wopt, sopt = find_optimal_celestial_wcs([(w1.array_shape, w1), (w2.array_shape, w2)], auto_rotate=False, **kwargs)
        exact = np.array([wopt.wcs.crval[0], wopt.wcs.crval[1], wopt.wcs.crpix[0], wopt.wcs.crpix[1], wopt.wcs.cdelt[0], wopt.wcs.cdelt[1]])
        rounded = np.array([float(res[k]) for k in KEYS])
        assert np.all(np.abs(exact - rounded) <= 1e-13 * np.abs(exact)), (name, exact, rounded)
        assert (res["NAXIS2"], res["NAXIS1"]) == tuple(sopt)
        out[key + "values"] = exact
        out[key + "header_values"] = rounded
        out[key + "ctype"] = np.array([res["CTYPE1"], res["CTYPE2"]])
        out[key + "naxis"] = np.array([res["NAXIS1"], res["NAXIS2"]], dtype=np.int64)
        if kw:
            out[key + "kwargs"] = np.array([kw["resolution"], kw["reference"][0], kw["reference"][1]])
            out[key + "projection"] = np.array(kw["projection"])
        wout = WCS(res)
        for tag, h in (("1", h1), ("2", h2)):
            xs, ys = reproject.celestial_pixel_map(WCS(to_fits(h)), wout, (res["NAXIS2"], res["NAXIS1"]))
            out[key + "xs" + tag], out[key + "ys" + tag] = xs, ys
        print("pair %-10s -> %s %s naxis %s" % (name, res["CTYPE1"], [float(res[k]) for k in KEYS], (res["NAXIS1"], res["NAXIS2"])))
    hid = combine_headers(to_fits(PAIRS["identical"][0]), to_fits(PAIRS["identical"][1]))
    h0 = PAIRS["identical"][0]
    assert (hid["NAXIS1"], hid["NAXIS2"]) == (h0["NAXIS1"], h0["NAXIS2"])
    assert all(abs(hid[k] - h0[k]) < 1e-9 for k in KEYS)


def make_source(rng, shape, keep_frac=None):
    nz, ny, nx = shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx]
    d = (1.0 + 0.3 * np.sin(0.7 * x + 0.4 * z) + 0.2 * np.cos(0.5 * y) + 0.05 * rng.normal(size=shape)).astype(np.float32)
    d[rng.random(shape) < 0.05] = np.nan
    pos = (int(rng.integers(nz)), int(rng.integers(1, ny - 1)), int(rng.integers(1, nx - 1)))
    d[pos] = np.inf
    keep = None
    if keep_frac is not None:
        keep = rng.random(shape) < keep_frac
        keep[pos] = False
    return d, keep


def margins(xs, ys, shape_yx):
    """smallest distance of an inside source position from a nearest-neighbour tie / from the +-0.5 border (pixels)"""
    ny, nx = shape_yx
    inside = (xs >= -0.5) & (xs <= nx - 0.5) & (ys >= -0.5) & (ys <= ny - 0.5)
    m = np.inf
    for c, n in ((xs, nx), (ys, ny)):
        m = min(m, np.abs(c + 0.5).min(), np.abs(c - (n - 0.5)).min())               # the border, inside or not
        ci = c[inside]
        if ci.size:
            m = min(m, np.abs(ci + 0.5 - np.round(ci + 0.5)).min())                     # ties of floor(c + 0.5)
    return m, inside


def ref_cube(d, h, keep, fill):
    w = WCS(to_fits(h))
    if keep is None:
        mask = LazyMask(np.isfinite, data=d, wcs=w)
    else:
        mask = BooleanArrayMask(keep, wcs=w)
    return SpectralCube(d * u.K, wcs=w, mask=mask, fill_value=fill)


def record_mosaic(out, name, cubes, sources, orders, check):
    key = "mos|%s|" % name
    out[key + "n"] = np.int64(len(sources))
    out[key + "orders"] = np.array(orders)
    margin = np.inf
    for order in orders:
        res = mosaic_cubes(cubes, order=order, roundtrip_coords=False)
        val = np.asarray(res.unmasked_data[:].value, dtype=np.float64)
        assert val.dtype == np.float64
        out[key + "result|" + order] = val
        hdr = res.header
    out[key + "header"] = np.array(header_text(hdr))
    wout = WCS(hdr)
    shape_yx = (hdr["NAXIS2"], hdr["NAXIS1"])
    weight = np.zeros(shape_yx, dtype=np.int64)
    nan_inside = False
    for s, (d, h, keep, fill) in enumerate(sources):
        xs, ys = reproject.celestial_pixel_map(WCS(to_fits(h)), wout, shape_yx)
        m, inside = margins(xs, ys, d.shape[1:])
        margin = min(margin, m)
        weight += inside
        xi = np.clip(np.floor(xs[inside] + 0.5).astype(int), 0, d.shape[2] - 1)
        yi = np.clip(np.floor(ys[inside] + 0.5).astype(int), 0, d.shape[1] - 1)
        nan_inside = nan_inside or bool(np.isnan(d[:, yi, xi]).any())
        out[key + "data%d" % s] = d
        out[key + "header%d" % s] = np.array(header_text(h))
        out[key + "keep%d" % s] = keep if keep is not None else np.zeros((0,), dtype=bool)
        out[key + "fill%d" % s] = np.float64(fill)
        out[key + "xs%d" % s], out[key + "ys%d" % s] = xs, ys
    out[key + "weight"] = weight
    for order in orders:
        val = out[key + "result|" + order]
        assert np.array_equal(np.isnan(val[0]), weight == 0), (name, order)
        assert np.isfinite(val[:, weight > 0]).all() and np.abs(val[np.isfinite(val)]).max() < 1e3, (name, order)
    frac2, frac0 = (weight >= 2).mean(), (weight == 0).mean()
    print("mosaic %-6s grid %s: weight>=2 on %.1f %%, max weight %d, weight 0 on %.1f %%, NaN inside a footprint: %s, margin %.2e"
          % (name, shape_yx, 100 * frac2, weight.max(), 100 * frac0, nan_inside, margin))
    if check:
        assert frac2 >= 0.10 and weight.max() == len(sources) == 3 and frac0 >= 0.10 and nan_inside
    assert margin >= 1e-6, margin
    return margin


def do_mosaics(out):
    rng = np.random.default_rng(20261018)
    specs = [((5, 9, 11), base(crval=(30.0, -20.0), crpix=(5.3, 4.6), shape=(5, 9, 11)), None, np.nan),
             ((5, 7, 13), base(crval=(30.0093, -19.9921), crpix=(6.4, 3.7), rot=30.0, shape=(5, 7, 13)), 0.85, 0.0),
             ((5, 12, 6), base(crval=(30.0139, -20.0068), crpix=(3.2, 6.1), shape=(5, 12, 6)), None, np.nan)]
    sources, cubes = [], []
    for shape, h, keep_frac, fill in specs:
        d, keep = make_source(rng, shape, keep_frac)
        sources.append((d, h, keep, fill))
        cubes.append(ref_cube(d, h, keep, fill))
    margin = record_mosaic(out, "three", cubes, sources, ["nearest-neighbor", "bilinear"], check=True)

    # the reference's test_mosaic_cubes: two overlapping two-thirds of one cube (tests/test_regrid.py:602-634)
    shape = (4, 9, 6)
    h = base(crval=(24.06, 29.0), crpix=(3.0, 4.0), cdelt=1e-3, shape=shape)
    d = (rng.normal(size=shape) + 5.0).astype(np.float32)
    cube = ref_cube(d, h, None, np.nan)
    part1, part2 = cube[:, :round(shape[1] * 2. / 3.), :], cube[:, round(shape[1] / 3.):, :]
    parts = []
    for p in (part1, part2):
        ph = {k: p.header[k] for k in p.header.keys() if k not in ("", "COMMENT", "HISTORY")}
        parts.append((np.asarray(p.unmasked_data[:].value, dtype=np.float32), ph, None, np.nan))
    margin = min(margin, record_mosaic(out, "split", [part1, part2], parts, ["nearest-neighbor"], check=False))
    res = out["mos|split|result|nearest-neighbor"]
    assert res.shape == d.shape and np.array_equal(res, d.astype(np.float64))
    out["mos|split|whole"] = d
    out["mos|split|whole_header"] = np.array(header_text(h))
    out["margin"] = np.float64(margin)


def main():
    out = {"pairs": np.array(list(PAIRS)), "keys": np.array(KEYS), "mosaics": np.array(["three", "split"])}
    do_pairs(out)
    do_mosaics(out)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
