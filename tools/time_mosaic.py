"""Time mosaic_cubes' fused route (spc_mosaic_f32) against the same mosaic composed from the operators there were before
it, in one run: 4 overlapping 512 x 1024 x 1024 float32 tiles (2 x 2, a quarter of a tile of overlap), one of them rotated
by 30 degrees, every tile with the reader's finite-value mask.

Fused: S device pixel maps (ops.wcs_pixel_map) and one ops.mosaic call - what mosaic_cubes does.  Composed: S x
SpectralCube.reproject onto the common header, then ONE pass of cube arithmetic, ((r0 + r1) + r2 + r3) / weight map (four
steps: the most one arithmetic program holds).  The arithmetic works on the raw samples, so the composed cube is NaN where
any tile does not reach - it is not the mosaic there; it is timed as the least device work a caller without
mosaic_cubes could get away with (nan_to_num per tile would add a pass each).  Both are wall-clock times around a device
synchronise (the composed route blocks on the host for each footprint), alternated --steps times after one warm-up of
each; medians and minima are printed.  Algorithmic bytes of the fused route: the source bytes inside the footprints (each
source voxel the target reaches, once) plus the output once, over the fused median as a fraction of 8 TB/s.

    python tools/time_mosaic.py [--steps 5] [--out profiles/mosaic_timing.txt] [--small]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_TBS = 8.0


def tile_header(shape, dx, dy, rot=None):
    nz, ny, nx = shape
    cd = 1e-4
    h = {"NAXIS": 3, "NAXIS1": nx, "NAXIS2": ny, "NAXIS3": nz, "CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD",
         "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s", "CRVAL1": 30.0 - dx * cd / np.cos(np.radians(-20.0)), "CRVAL2": -20.0 + dy * cd,
         "CRVAL3": 0.0, "CRPIX1": nx / 2 + 0.37, "CRPIX2": ny / 2 + 0.21, "CRPIX3": 1.0, "CDELT1": -cd, "CDELT2": cd, "CDELT3": 1.0,
         "BUNIT": "K"}
    if rot is not None:
        c, s = np.cos(np.radians(rot)), np.sin(np.radians(rot))
        h.update({"PC1_1": c, "PC1_2": -s, "PC2_1": s, "PC2_2": c})
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="32 x 256 x 256 tiles (a quick check of the tool)")
    args = ap.parse_args()
    from spectral_cube_amd import SpectralCube, SimpleWCS, _lib, masks as M, ops
    from spectral_cube_amd.cube_utils import combine_headers, mosaic_route
    from spectral_cube_amd.device import DeviceArray
    _lib.require_gpu()
    shape = (32, 256, 256) if args.small else (512, 1024, 1024)
    nz, ny, nx = shape
    rng = np.random.default_rng(0)
    d = rng.standard_normal(shape, dtype=np.float32)
    d[rng.random(shape, dtype=np.float32) < 0.01] = np.nan
    step = 0.75
    cubes = []
    for k, (ix, iy, rot) in enumerate(((0, 0, None), (1, 0, None), (0, 1, None), (1, 1, 30.0))):
        c = SpectralCube(None, header=tile_header(shape, ix * step * nx, iy * step * ny, rot), _dev=DeviceArray.from_numpy(d, 0),
                         allow_huge_operations=True)
        c._mask = M.LazyMask(np.isfinite, cube=c)
        cubes.append(c)
    del d
    header = dict(cubes[0].header)
    for c in cubes[1:]:
        header = combine_headers(header, c.header)
    wout = SimpleWCS(header)
    shape_out = (nz, int(header["NAXIS2"]), int(header["NAXIS1"]))
    assert mosaic_route(cubes, wout, 1) == "fused"
    datas = [c._device_data() for c in cubes]
    masks = [c._mask_spec() for c in cubes]
    fills = [float(c.fill_value) for c in cubes]
    out = DeviceArray(shape_out, np.float32, 0)
    weights = DeviceArray(shape_out[1:], np.int32, 0)

    def sync():
        _lib.call("spc_device_sync", 0)

    def fused():
        maps = [ops.wcs_pixel_map(c.wcs, wout, shape_out[1:]) for c in cubes]
        ops.mosaic(datas, maps, masks, fills, 1, weights=weights, out=out)
        sync()

    def composed():
        parts = [c.reproject(wout) for c in cubes]
        weight = sum(p._footprint.astype(np.float32) for p in parts)
        total = (((parts[0] + parts[1]) + parts[2]) + parts[3]) / weight
        total._device_data()
        sync()
        return total

    def wall(fn):
        t = time.perf_counter()
        fn()
        return 1e3 * (time.perf_counter() - t)

    fused()
    ref = composed()
    # results must not change: the composed cube is the mosaic wherever it is not NaN (compared on the first two channels)
    a, b = out.planes(0, 2).get(), ref._device_data().planes(0, 2).get()
    both = np.isfinite(a) & np.isfinite(b)
    agree = float(np.abs(a[both] - b[both]).max()) if both.any() else float("nan")
    w = weights.get()
    del a, b, ref
    t_f, t_c = [], []
    for _ in range(args.steps):
        t_f.append(wall(fused))
        t_c.append(wall(composed))
    src_bytes = 0
    for c in cubes:                       # the source pixels that are the nearest one of some target pixel
        xs, ys = (m.get() for m in ops.wcs_pixel_map(c.wcs, wout, shape_out[1:]))
        inside = (xs >= -0.5) & (xs <= nx - 0.5) & (ys >= -0.5) & (ys <= ny - 0.5)
        reached = np.zeros((ny, nx), bool)
        reached[np.clip(np.round(ys[inside]).astype(int), 0, ny - 1), np.clip(np.round(xs[inside]).astype(int), 0, nx - 1)] = True
        src_bytes += int(reached.sum()) * nz * 4
    out_bytes = int(np.prod(shape_out)) * 4
    med_f, med_c = float(np.median(t_f)), float(np.median(t_c))
    rec = dict(workload="4 tiles of %s float32, one rotated by 30 degrees" % (shape,), mosaic_shape=list(shape_out), steps=args.steps,
               fused_ms_median=round(med_f, 2), fused_ms_min=round(min(t_f), 2), composed_ms_median=round(med_c, 2),
               composed_ms_min=round(min(t_c), 2), composed_over_fused=round(med_c / med_f, 2),
               source_bytes_inside_footprints=src_bytes, output_bytes=out_bytes,
               fused_tb_per_s=round((src_bytes + out_bytes) / med_f / 1e9, 3),
               fused_fraction_of_hbm_peak=round((src_bytes + out_bytes) / med_f / 1e9 / HBM_TBS, 3),
               weight_histogram={int(k): int(v) for k, v in zip(*np.unique(w, return_counts=True))},
               max_abs_difference_where_both_finite=agree, measured=True)
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
