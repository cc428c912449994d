"""Time spc_rank_filter_axis0_* / _plane_* (the kernels of spectral_smooth_median / spatial_smooth_median) on the cases of
DESIGN.md: 1024^3 float32 with and without a uint8 mask array, 512 x 1024^2 float64; spectral windows 3, 5, 9, 33, 129,
spatial 3, 5, 9, 15 (the median, mode reflect).  Next to each, in the same run, the yardstick that moves the same bytes:
the materialised spectral_smooth with a kernel of as many taps, the materialised spatial_smooth with the same footprint.
One JSON record per case: the median of the HIP-event times after two warm-up launches, the algorithmic bytes (every
sample and mask byte read once, every output sample written once) and their fraction of 8 TB/s.

    python tools/time_rank_filter.py [--reps 10] [--out profiles/rank_filter_time.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectral_cube_amd import _lib, ops  # noqa: E402
from spectral_cube_amd.device import DeviceArray, Event, Stream  # noqa: E402

SPECTRAL = (3, 5, 9, 33, 129)
SPATIAL = (3, 5, 9, 15)


def gauss(n):
    x = np.arange(n) - n // 2
    k = np.exp(-0.5 * (x / max(n / 6.0, 0.5)) ** 2)
    return k / k.sum()


def timed(fn, st, reps):
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        a, b = Event(st.device), Event(st.device)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_ms(b))
    return float(np.median(times)), float(np.min(times))


def record(op, cube, mask, size, ms, lo, sink):
    e = cube.dtype.itemsize
    n = int(np.prod(cube.shape))
    nbytes = n * (2 * e + (1 if mask is not None else 0))
    rec = dict(op=op, dtype=cube.dtype.name, shape=list(cube.shape), mask="u8" if mask is not None else "none", size=size,
               median_ms=round(ms, 4), min_ms=round(lo, 4), bytes=nbytes, tbps=round(nbytes / ms / 1e9, 3),
               fraction_of_8tbps=round(nbytes / ms / 1e9 / 8.0, 3))
    line = json.dumps(rec)
    print(line, flush=True)
    if sink is not None:
        sink.write(line + "\n")
        sink.flush()
    return ms


def run_cube(cube, mask, reps, sink):
    st = Stream(cube.device)
    out = DeviceArray(cube.shape, cube.dtype, cube.device)
    for k in SPECTRAL:
        t, lo = timed(lambda: ops.rank_filter_axis0(cube, k, k // 2, mask=mask, out=out, stream=st), st, reps)
        record("spectral_median", cube, mask, k, t, lo, sink)
        t, lo = timed(lambda: ops.spectral_conv(cube, gauss(k), mask=mask, out=out, stream=st), st, reps)
        record("spectral_smooth", cube, mask, k, t, lo, sink)
    for k in SPATIAL:
        t, lo = timed(lambda: ops.rank_filter_plane(cube, k, k, k * k // 2, mask=mask, out=out, stream=st), st, reps)
        record("spatial_median", cube, mask, k, t, lo, sink)
        t, lo = timed(lambda: ops.spatial_conv(cube, np.outer(gauss(k), gauss(k)), mask=mask, out=out, stream=st), st, reps)
        record("spatial_smooth", cube, mask, k, t, lo, sink)
    out.free()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    sink = open(args.out, "w") if args.out else None
    rng = np.random.default_rng(0)
    n = 1024
    cube = DeviceArray.from_numpy(rng.standard_normal((n, n, n), dtype=np.float32))
    run_cube(cube, None, args.reps, sink)
    keep = DeviceArray.from_numpy((rng.random((n, n, n), dtype=np.float32) < 0.8).view(np.uint8))
    run_cube(cube, ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, keep), args.reps, sink)
    cube.free()
    keep.free()
    cube64 = DeviceArray.from_numpy(rng.standard_normal((512, n, n)))
    run_cube(cube64, None, args.reps, sink)
    if sink is not None:
        sink.close()


if __name__ == "__main__":
    main()
