"""Time the fused moment kernel (ops.moments -> m0, m1, m2) at 1024^3 float32 under five kinds of mask, with the mask-first
march on and off (SPC_MOMENTS_MASK_FIRST=1 / 0, read per call): the benchmark's mask (data > 2 sigma with a 1 % flip), a
signal mask (data > 5 sigma), 80 % random, all ones and no mask array (where the switch selects nothing).  Cube and masks
are one seeded 16-row tile repeated along y, as in bench.py.  One JSON record per mask and setting: median / min / max
of the HIP-event times of the launches, and the algorithmic 5 (4 without an array) bytes per voxel over the median.

    python tools/time_moments_masks.py [--reps 20] [--n 1024] [--out FILE.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import bench  # noqa: E402  (replicate_rows: one upload, device-to-device doubling along y)
from spectral_cube_amd import _lib, ops, synth  # noqa: E402
from spectral_cube_amd.device import DeviceArray, Event, Stream  # noqa: E402

SWITCH = "SPC_MOMENTS_MASK_FIRST"


def timed(fn, st, reps, device):
    for _ in range(3):
        fn()
    times = []
    for _ in range(reps):
        a, b = Event(device), Event(device)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_ms(b))
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    sink = open(args.out, "w") if args.out else None
    n, device = args.n, 0
    shape = (n, n, n)
    tile = synth.gaussian_line_cube((n, 16, n), synth.SEEDS["C2"], chunk_rows=16)
    rng = np.random.default_rng(7)
    masks = [("bench mask (data > 2 sigma, 1 % flip)", synth.boolean_mask(tile, synth.SEEDS["C2"])),
             ("signal mask (data > 5 sigma)", (tile > np.float32(2.5)).view(np.uint8)),
             ("80 % random", (rng.random(tile.shape, dtype=np.float32) < 0.8).view(np.uint8)),
             ("all ones", np.ones(tile.shape, np.uint8)),
             ("no mask array", None)]
    cube = DeviceArray(shape, np.float32, device)
    bench.replicate_rows(cube, tile)
    maskd = DeviceArray(shape, np.uint8, device)
    v = synth.spectral_axis(n)
    cen = v - v[0]
    cref = cen[n // 2]
    d_cen = DeviceArray.from_numpy(cen - cref, device)
    out = {k: DeviceArray((n, n), np.float64, device) for k in ("m0", "m1", "m2")}
    st = Stream(device)
    for label, tmask in masks:
        spec = None
        if tmask is not None:
            bench.replicate_rows(maskd, tmask)
            spec = ops.MaskSpec(_lib.MASK_ARRAY, array=maskd)
        per_voxel = 5 if tmask is not None else 4
        for round_ in range(2):                                 # the two settings alternate: a drift shows as a difference between rounds
            for switch in ("0", "1"):
                os.environ[SWITCH] = switch                     # (the library reads it per call)
                t = timed(lambda: ops.moments(cube, d_cen, dv=500.0, m1_add=cref + v[0], mask=spec, want=("m0", "m1", "m2"),
                                              stream=st, out=out), st, args.reps, device)
                ms = float(np.median(t))
                rec = dict(mask=label, valid_fraction=round(float(np.count_nonzero(tmask)) / tmask.size, 4) if tmask is not None else 1.0,
                           shape=list(shape), mask_first=int(switch), round=round_, launches=len(t), median_ms=round(ms, 4),
                           min_ms=round(float(np.min(t)), 4), max_ms=round(float(np.max(t)), 4),
                           algorithmic_tbps=round(n ** 3 * per_voxel / ms / 1e9, 3))
                line = json.dumps(rec)
                print(line, flush=True)
                if sink:
                    sink.write(line + "\n")
                    sink.flush()
    os.environ.pop(SWITCH, None)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
