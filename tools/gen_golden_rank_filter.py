"""Generate tests/golden/rank_filter.npz from the REFERENCE's spectral_smooth_median / spectral_filter /
spatial_smooth_median / spatial_filter (in-memory class, scipy.ndimage's rank filters).

Run with the reference environment, like tools/gen_golden_downsample.py:

    /opt/conda/bin/python3.9 -B tools/gen_golden_rank_filter.py

A small float32 cube (11 x 8 x 9, samples on a grid of 1/128 so that the file stays small and windows hold ties) under
three variants:

* ``finite0``: isfinite mask, fill value 0, data with NaN - no NaN reaches the filter, every voxel is compared;
* ``bool0``: boolean-array mask keeping about 75 %, one spaxel and one plane masked throughout, fill value 0 (the data
  are NaN-free) - every voxel compared; covers "a spectrum / plane without an included sample is not filtered";
* ``finitenan``: isfinite mask, the default NaN fill, 2 % NaN - scipy's result with a NaN in the window is undefined, so
  the file records which voxels have a NaN-free window (``comparable``) and only those are compared.

Per case it stores the reference's filter output (the new cube's unmasked data, float32: a rank filter copies samples).
Before anything is written the numpy restatement the GPU tests use (pad, sliding_window_view, sort, take the rank) is
checked against scipy bit for bit on NaN-free input, for every size, mode and rank recorded here and the percentile rule.
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

import scipy  # noqa: E402
from scipy import ndimage  # noqa: E402
from astropy import units as u  # noqa: E402
from astropy.wcs import WCS  # noqa: E402
from spectral_cube import SpectralCube, BooleanArrayMask, LazyMask  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "rank_filter.npz")
HEADER = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s",
          "CDELT1": -2e-3, "CDELT2": 2e-3, "CDELT3": 0.5, "CRPIX1": 5.0, "CRPIX2": 4.0, "CRPIX3": 2.0,
          "CRVAL1": 30.0, "CRVAL2": -20.0, "CRVAL3": 4.0, "BUNIT": "K"}
SHAPE = (11, 8, 9)
CVAL = 2.5
MODES = ("reflect", "constant", "nearest", "mirror", "wrap")
PAD = {"reflect": "symmetric", "mirror": "reflect", "nearest": "edge", "wrap": "wrap", "constant": "constant"}
SPECTRAL = (1, 2, 3, 4, 5, 9)
SPATIAL = ((3, 3), (4, 4), (5, 5), (3, 5))
SUBSET = {"bool0": ((3,), (4,), (3, 3), (3, 5)), "finitenan": ((3,), (5,), (9,), (3, 3), (5, 5))}


def header_text(h):
    return "\n".join("%-8s= %r" % (k, v) if isinstance(v, str) else "%-8s= %s" % (k, repr(float(v))) for k, v in h.items())


def scipy_rank(name, w, extra):
    """the rank scipy's filter *name* selects in a window of w samples (what the package's host code restates)"""
    if name == "median":
        return w // 2
    if name == "minimum":
        return 0
    if name == "maximum":
        return w - 1
    if name == "rank":
        return extra + w if extra < 0 else extra
    p = extra + 100 if extra < 0 else extra
    return w - 1 if p == 100 else int(float(w) * p / 100.0)


def restate(x, sizes, axes, rank, mode, cval=0.0):
    """np.sort(window)[rank] of every window: the statement the GPU tests check against"""
    pads = [(0, 0)] * x.ndim
    for k, a in zip(sizes, axes):
        pads[a] = (k // 2, k - 1 - k // 2)
    kw = {"constant_values": cval} if mode == "constant" else {}
    win = np.lib.stride_tricks.sliding_window_view(np.pad(x, pads, mode=PAD[mode], **kw), sizes, axis=axes)
    return np.sort(win.reshape(x.shape + (-1,)), axis=-1)[..., rank]


def cases():
    """(tag, sizes, filter name, its extra argument, mode) - sizes of length 1 are spectral"""
    out = []
    for kinds in ([(k,) for k in SPECTRAL], SPATIAL):
        for s in kinds:
            for mode in MODES:
                out.append((s, "median", None, mode))
            for name, extra in (("minimum", None), ("maximum", None)):
                out.append((s, name, extra, "reflect"))
            w = int(np.prod(s))
            out.append((s, "percentile", 30 if w % 2 else -40, "reflect" if w % 2 else "constant"))
            out.append((s, "rank", -2 if w > 1 else 0, "nearest" if w % 2 else "wrap"))
            out.append((s, "maximum", None, "constant"))
    return out


def tag_of(variant, s, name, extra, mode):
    return "%s|%s|%s|%s|%s" % (variant, "x".join(str(k) for k in s), name, "" if extra is None else extra, mode)


def ref_filter(cube, s, name, extra, mode):
    fn = getattr(ndimage, name + "_filter")
    kw = dict(mode=mode, cval=CVAL, use_memmap=False, parallel=False)
    if name == "percentile":
        kw["percentile"] = extra
    if name == "rank":
        kw["rank"] = extra
    if len(s) == 1:
        new = cube.spectral_smooth_median(s[0], **kw) if name == "median" else cube.spectral_filter(s[0], filter=fn, **kw)
    else:
        ks = s[0] if s[0] == s[1] else list(s)
        new = cube.spatial_smooth_median(ks, **kw) if name == "median" else cube.spatial_filter(ks, filter=fn, **kw)
    return np.asarray(new.unmasked_data[:].value)


def make_data():
    rng = np.random.default_rng(20261016)
    clean = (np.round(rng.normal(0.5, 1.0, SHAPE) * 128) / 128).astype(np.float32)
    holes = clean.copy()
    holes[rng.random(SHAPE) < 0.08] = np.nan
    holes[:, 2, 6] = np.nan                  # a spaxel of NaN
    sparse = clean.copy()
    sparse[rng.random(SHAPE) < 0.02] = np.nan
    keep = rng.random(SHAPE) < 0.75
    keep[:, 1, 2] = False                    # a spaxel masked throughout
    keep[8, :, :] = False                    # a plane masked throughout
    return clean, holes, sparse, keep


def check_restatement_against_scipy():
    rng = np.random.default_rng(7)
    n = 0
    for shape in ((13,), (4,), (7, 6), (3, 5)):
        x = rng.normal(size=shape).astype(np.float32)
        x.flat[::5] = x.flat[1]              # ties
        sizes_all = [(k,) for k in SPECTRAL if k // 2 <= shape[0]] if len(shape) == 1 else [s for s in SPATIAL + ((2, 2), (1, 3))
                                                                                      if s[0] // 2 <= shape[0] and s[1] // 2 <= shape[1]]
        axes = tuple(range(len(shape)))
        for s in sizes_all:
            w = int(np.prod(s))
            for mode in MODES:
                for rank in range(w):
                    exp = ndimage.rank_filter(x, rank, size=s, mode=mode, cval=CVAL)
                    assert np.array_equal(restate(x, s, axes, rank, mode, CVAL), exp), (shape, s, mode, rank)
                    n += 1
                for name, extra in (("median", None), ("minimum", None), ("maximum", None), ("percentile", 30), ("percentile", -40),
                                    ("percentile", 100), ("percentile", 0), ("percentile", 99.9), ("rank", -1), ("rank", -w)):
                    fn = getattr(ndimage, name + "_filter")
                    args = () if extra is None else (extra,)
                    exp = fn(x, *args, size=s, mode=mode, cval=CVAL)
                    assert np.array_equal(restate(x, s, axes, scipy_rank(name, w, extra), mode, CVAL), exp), (shape, s, mode, name, extra)
                    n += 1
    return n


def main():
    n = check_restatement_against_scipy()
    print("restatement == scipy %s on %d NaN-free filters" % (scipy.__version__, n))
    clean, holes, sparse, keep = make_data()
    w = WCS(HEADER)
    variants = {
        "finite0": (SpectralCube(data=holes * u.K, wcs=w, mask=LazyMask(np.isfinite, data=holes, wcs=w)).with_fill_value(0.0),
                    np.where(np.isfinite(holes), holes, np.float32(0))),
        "bool0": (SpectralCube(data=clean * u.K, wcs=w, mask=BooleanArrayMask(keep, wcs=w)).with_fill_value(0.0),
                  np.where(keep, clean, np.float32(0))),
        "finitenan": (SpectralCube(data=sparse * u.K, wcs=w, mask=LazyMask(np.isfinite, data=sparse, wcs=w)), sparse),
    }
    names, results, flags, nflag = [], [], [], []
    for variant, (cube, filled) in variants.items():
        for (s, name, extra, mode) in cases():
            # every case on finite0; on the other two the median (reflect, constant) and the maximum (constant) of a few sizes
            if variant != "finite0" and (s not in SUBSET[variant] or mode not in ("reflect", "constant")
                                         or not (name == "median" or (name == "maximum" and mode == "constant"))):
                continue
            got = ref_filter(cube, s, name, extra, mode)
            assert got.shape == SHAPE
            got32 = got.astype(np.float32)
            assert np.array_equal(got32.astype(np.float64), got, equal_nan=True), "the filter returned something that is no float32 sample"
            axes = (0,) if len(s) == 1 else (1, 2)
            wn = int(np.prod(s))
            ok = ~restate(np.isnan(filled), s, axes, wn - 1, mode, False)          # no NaN in the window
            if variant == "finitenan":
                assert ok.mean() >= 0.5, (s, mode, ok.mean())
            else:
                assert ok.all()
                # (on NaN-free input the restatement is the reference - apart from rays without an included sample)
            names.append(tag_of(variant, s, name, extra, mode))
            results.append(got32.ravel())
            flags.append(ok.ravel())
            nflag.append(int(ok.sum()))
    out = {"header": np.array(header_text(HEADER)), "clean": clean, "holes": holes, "sparse": sparse, "keep": keep,
           "cval": np.float64(CVAL), "case_names": np.array(names), "filtered": np.concatenate(results),
           "comparable": np.packbits(np.concatenate(flags)), "comparable_count": np.array(nflag, dtype=np.int64),
           "scipy_version": np.array(scipy.__version__)}
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(names), "cases")


if __name__ == "__main__":
    main()
