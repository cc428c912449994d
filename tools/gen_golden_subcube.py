"""Generate tests/golden/subcube.npz from the REFERENCE's slicing: SpectralCube.__getitem__, spectral_slab, subcube,
subcube_slices_from_mask and mask_channels.

Run with the reference environment, like tools/gen_golden_downsample.py:

    /opt/conda/bin/python3.9 -B tools/gen_golden_subcube.py

The float32 cube with NaNs (11 x 7 x 9) and the CDELT / CD headers of the downsample generator, under four masks (none,
isfinite, comparison, boolean array).  For each view it records the reference's unmasked data, mask.include(), filled
data and the output WCS (crpix / cdelt / crval, FITS order); the CD header adds the world coordinates of the result's
pixel centres, from the parent WCS.  Only views the reference gets right are recorded: no negative starts, no ``[a:b:-1]``.
No test imports this file; only its output is committed.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle", "ref_env"))
sys.path.insert(0, HERE)

from bootstrap import load_reference  # noqa: E402

load_reference()

from astropy import units as u  # noqa: E402
from astropy.wcs import WCS  # noqa: E402
from spectral_cube import SpectralCube, BooleanArrayMask, LazyMask  # noqa: E402
from spectral_cube.utils import SliceWarning  # noqa: E402

from gen_golden_downsample import CD_HEADER, HEADER, THRESHOLD, header_text, make_data  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "subcube.npz")
KINDS = ("none", "finite", "cmp", "bool")

# name -> how the test builds the same cut (kept in tests/test_gpu_subcube.py / test_subcube_host.py under the same names)
KM = u.km / u.s
CUTS = {
    "step":      lambda c: c[1::2, ::3, 2:8:2],
    "reverse":   lambda c: c[::-1],
    "clipped":   lambda c: c[5:50],
    "full":      lambda c: c[:],
    "box":       lambda c: c[:, 2:6, 1:8],
    "slab":      lambda c: c.spectral_slab(4.2 * KM, 6.4 * KM),
    "slab_swap": lambda c: c.spectral_slab(6.4 * KM, 4.2 * KM),
    "slab_ms":   lambda c: c.spectral_slab(4200.0 * u.m / u.s, 6400.0 * u.m / u.s),
    "slab_one":  lambda c: c.spectral_slab(4.1 * KM, 4.2 * KM),
    "subcube":   lambda c: c.subcube(xlo=2, xhi=7, ylo=1, zlo=4.2 * KM, zhi=6.4 * KM),
    "subcube_z": lambda c: c.subcube(zlo=2, zhi=5),
}
LOWER = {
    "chan3":     lambda c: c[3],
    "chan_box":  lambda c: c[-2, 1:6, 2:9],
    "spectrum":  lambda c: c[:, 2, 3],
    "spec_part": lambda c: c[2:9, 5, 0],
}


LOWER_VIEWS = {"chan3": (3,), "chan_box": (-2, slice(1, 6), slice(2, 9)), "spectrum": (slice(None), 2, 3),
               "spec_part": (slice(2, 9), 5, 0)}


def ref_cube(d, keep, kind, header):
    w = WCS(header)
    if kind == "none":
        return SpectralCube(data=d * u.K, wcs=w)
    cube = SpectralCube(data=d * u.K, wcs=w, mask=LazyMask(np.isfinite, data=d, wcs=w))
    if kind == "bool":
        cube = cube.with_mask(BooleanArrayMask(keep, wcs=w), inherit_mask=False)
    elif kind == "cmp":
        cube = cube.with_mask(cube > THRESHOLD * u.K)
    return cube


def slices_record(sl):
    return np.array([[-1 if s.start is None else s.start, -1 if s.stop is None else s.stop] for s in sl], dtype=np.int64)


def main():
    d, keep = make_data()
    out = {"data": d, "keep": keep, "header": np.array(header_text(HEADER)), "cd_header": np.array(header_text(CD_HEADER)),
           "threshold": np.float64(THRESHOLD), "kinds": np.array(KINDS), "cuts": np.array(sorted(CUTS)),
           "lower": np.array(sorted(LOWER))}
    names, filled, unmasked, include = [], [], [], []
    for kind in KINDS:
        cube = ref_cube(d, keep, kind, HEADER)
        for name in sorted(CUTS):
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                try:
                    r = CUTS[name](cube)
                except ValueError as exc:           # (the reference cannot reverse a comparison mask: "Cannot reverse-index a WCS")
                    print("skipped %s %s: %s" % (kind, name, exc))
                    continue
            tag = "%s_%s" % (kind, name)
            names.append(tag)
            out["shape_" + tag] = np.array(r.shape, dtype=np.int64)
            out["warned_" + tag] = np.bool_(any(issubclass(w.category, SliceWarning) for w in caught))
            if kind == "finite":
                out["wcs_" + name] = np.array([r.wcs.wcs.crpix, r.wcs.wcs.cdelt, r.wcs.wcs.crval], dtype=np.float64)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                filled.append(np.asarray(r.unitless_filled_data[:], dtype=np.float32).ravel())
                unmasked.append(np.asarray(r.unmasked_data[:].value, dtype=np.float32).ravel())
                inc = r.mask.include() if r.mask is not None else np.ones(r.shape, bool)
            include.append(np.asarray(inc, dtype=bool).ravel())
        for name in sorted(LOWER):
            # the FILLED samples of the view are what the reference's 2-D result holds (:1362); its 1-D result holds the
            # unfilled ones, and cube[k, ys, xs] of a cube with a lazy mask fails in the reference ("WCS does not match
            # mask WCS"): the samples are taken from the cube's filled data, shape and WCS from the cube without a mask
            tag = "%s_%s" % (kind, name)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                out["lower_filled_" + tag] = np.asarray(cube.unitless_filled_data[LOWER_VIEWS[name]], dtype=np.float32)
                if kind == "none":
                    r = LOWER[name](cube)
                    out["lower_shape_" + name] = np.array(r.shape, dtype=np.int64)
                    out["lower_wcs_" + name] = np.array([r.wcs.wcs.crpix, r.wcs.wcs.cdelt, r.wcs.wcs.crval], dtype=np.float64)
    out["case_names"] = np.array(names)
    out["case_offsets"] = np.cumsum([0] + [len(a) for a in filled]).astype(np.int64)
    out["filled"] = np.concatenate(filled)
    out["unmasked"] = np.concatenate(unmasked)
    out["include"] = np.packbits(np.concatenate(include))
    # bounding boxes
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        cube = ref_cube(d, keep, "finite", HEADER)
        thr = cube > 2.8 * u.K
        out["bbox_threshold"] = np.float64(2.8)
        out["bbox_cmp"] = slices_record(cube.subcube_slices_from_mask(thr))
        region = np.zeros(d.shape, bool)
        region[2:5, 3, 1:8] = True
        region[7, 1:3, 4] = True
        out["bbox_region"] = region
        out["bbox_array"] = slices_record(cube.subcube_slices_from_mask(region))
        out["bbox_array_spatial"] = slices_record(cube.subcube_slices_from_mask(region, spatial_only=True))
        out["bbox_empty"] = slices_record(cube.subcube_slices_from_mask(np.zeros(d.shape, bool)))
        mc = cube.with_mask(thr).minimal_subcube()
        out["minimal_shape"] = np.array(mc.shape, dtype=np.int64)
        out["minimal_wcs"] = np.array([mc.wcs.wcs.crpix, mc.wcs.wcs.cdelt, mc.wcs.wcs.crval], dtype=np.float64)
        out["minimal_filled"] = np.asarray(mc.unitless_filled_data[:], dtype=np.float32)
        good = np.array([1, 1, 0, 1, 0, 0, 1, 1, 1, 0, 1], dtype=bool)
        ch = cube.mask_channels(good)
        out["goodchannels"] = good
        out["mask_channels_include"] = np.asarray(ch.mask.include(), dtype=bool)
    # CD-matrix header: world coordinates of every pixel centre of the cut = the PARENT WCS at the parent pixel of each
    # result pixel (start + k * step, the block centre + (step - 1) / 2 for a step > 1, start - k reversed), as the
    # downsample generator records them.  The reference's own sliced WCS is not used here: it rescales CDELT, which wcslib
    # ignores beside a CD matrix, so its stepped and reversed CD headers contradict the samples.
    wcd = WCS(CD_HEADER)
    cd_shape = (6, 8, 10)
    out["cd_shape"] = np.array(cd_shape, dtype=np.int64)
    cd_views = {"step": (slice(1, None, 2), slice(None, None, 3), slice(2, 8, 2)), "box": (slice(2, 5), slice(1, 7), slice(3, 9)),
                "reverse": (slice(None, None, -1), slice(None), slice(None))}
    for name, view in cd_views.items():
        grids = []
        for sl, n in zip(view, cd_shape):
            start, stop, step = sl.indices(n)
            k = np.arange(len(range(start, stop, step)), dtype=np.float64)
            grids.append(start + k * step + ((step - 1) / 2.0 if step > 1 else 0.0))
        zz, yy, xx = np.meshgrid(*grids, indexing="ij")
        out["cdworld_" + name] = wcd.wcs_pix2world(np.stack([xx.ravel(), yy.ravel(), zz.ravel()], axis=1), 0)
        out["cdshape_" + name] = np.array(zz.shape, dtype=np.int64)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
