"""Time the order statistics over two axes at 1024^3 float32 + uint8 mask (the f4_median configuration of bench.py: one
seeded tile of the synthetic line cube repeated along y, its boolean mask as a uint8 array) next to their yardstick, in one
run, alternating the cases launch by launch:

  (y) cube.median(axis=None)       the whole-cube selection as it was: four reads of the cube with the same loads and the
                                   same LDS histogram, the host walking the counters after every pass (four synchronisations)
  (a) cube.median(axis=(1, 2))     spc_percentile_groups_f32, keep_axis = 0: at most five reads, no synchronisation inside
  (b) cube.mad_std(axis=(1, 2))    two such calls, the first's device result the centre of the second
  (c) cube.median(axis=(0, 2))     keep_axis = 1: the rows of one y, a plane apart

Each is the cube-level call (its result comes back to the host), timed by HIP events on the null stream around it: median /
min / max of --reps rounds after --warmup.  Expectation written down before it ran: (a) <= 5/4 (y) plus the run-to-run spread
of (y) (max - min over the rounds), (b) <= twice that.  The ratios and the spread are printed, whichever way they fall.
The results of (a) - (c) are compared with numpy on the host for the first planes / rows before anything is said of speed.

    python tools/bench_plane_order_stats.py [--n 1024] [--reps 15] [--warmup 3] [--out profiles/plane_order_stats.txt]
"""
import argparse
import os
import sys
import warnings

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402  (tiled_strip_on_device: the benchmark's cube)
from spectral_cube_amd import SpectralCube, _lib, synth  # noqa: E402
from spectral_cube_amd import masks as M  # noqa: E402
from spectral_cube_amd.device import Event, device_info, synchronize  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    device, n = 0, a.n
    shape = (n, n, n)
    dev, maskd, tile, tmask = bench.tiled_strip_on_device(shape, synth.SEEDS["C2"], device)
    cube = SpectralCube.from_device(dev, mask=M.DeviceBooleanMask(maskd))
    cases = (("y", "median(axis=None) [yardstick]", lambda: cube.median()),
             ("a", "median(axis=(1, 2))", lambda: cube.median(axis=(1, 2))),
             ("b", "mad_std(axis=(1, 2))", lambda: cube.mad_std(axis=(1, 2))),
             ("c", "median(axis=(0, 2))", lambda: cube.median(axis=(0, 2))))
    # the answers first: the tile's rows repeat along y, so a plane's samples are the tile's plane taken n / rows times
    inc = tmask.astype(bool) & ~np.isnan(tile)
    filled = np.where(inc, tile, np.float32(np.nan))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        exp_planes = np.nanmedian(filled, axis=(1, 2))
        exp_mad = (1.482602218505602 * np.nanmedian(np.abs(filled - exp_planes[:, None, None]), axis=(1, 2))).astype(np.float32)
        exp_rows = np.nanmedian(filled, axis=(0, 2))
        exp_all = np.nanmedian(filled)
    rows = tile.shape[1]
    whole = n % rows == 0
    got = {tag: np.asarray(fn()) for tag, _, fn in cases}
    checks = []
    if whole:
        checks.append("median(axis=(1, 2)) equals numpy on the tile: %s" % np.array_equal(got["a"], exp_planes, equal_nan=True))
        checks.append("mad_std(axis=(1, 2)) within 3e-6 of numpy on the tile: %s" % bool(
            np.nanmax(np.abs(got["b"] - exp_mad)) <= 3e-6 * np.nanmax(exp_mad)))
        checks.append("median(axis=None) equals numpy on the tile: %s" % bool(got["y"] == exp_all))
    checks.append("median(axis=(0, 2)), first %d rows equal numpy on the tile: %s" % (rows, np.array_equal(got["c"][:rows], exp_rows, equal_nan=True)))
    times = {tag: [] for tag, _, _ in cases}
    for r in range(a.warmup + a.reps):
        for tag, _, fn in cases:
            e0, e1 = Event(device), Event(device)
            e0.record(None)
            fn()
            e1.record(None)
            e1.synchronize()
            if r >= a.warmup:
                times[tag].append(e0.elapsed_ms(e1))
    synchronize(device)
    vox = float(n) ** 3
    lines = ["order statistics over two axes at %d^3 float32 + uint8 mask (%.0f %% of the samples valid), %s" % (
                 n, 100.0 * inc.mean(), device_info(device)["name"] or "HIP device %d" % device),
             "%d rounds after %d warm-ups, the cases alternating inside a round; HIP events around the cube-level call" % (a.reps, a.warmup)]
    lines += checks
    med = {}
    for tag, what, _ in cases:
        t = np.asarray(times[tag])
        med[tag] = float(np.median(t))
        reads = 4 if tag == "y" else (10 if tag == "b" else 5)
        lines.append("(%s) %-32s median %8.3f ms  min %8.3f  max %8.3f   at most %d reads of 5 B per voxel: <= %.2f TB/s" % (
            tag, what, med[tag], t.min(), t.max(), reads, reads * 5.0 * vox / med[tag] / 1e9))
    ty = np.asarray(times["y"])
    spread = float(ty.max() - ty.min())
    lines.append("spread of the yardstick (max - min over the rounds): %.3f ms = %.1f %% of its median" % (spread, 100.0 * spread / med["y"]))
    for tag, factor in (("a", 1.25), ("b", 2.5), ("c", 1.25)):
        bound = factor * med["y"] + (2.0 if tag == "b" else 1.0) * spread
        lines.append("(%s) / (y) = %.3f   expected <= %.2f + spread: %.3f ms against %.3f ms: %s" % (
            tag, med[tag] / med["y"], factor, med[tag], bound, "met" if med[tag] <= bound else "EXCEEDED"))
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
