"""Time spc_downsample_f32 / _f64 (SpectralCube.downsample_axis's kernel) on the cases of DESIGN.md: 1024^3 float32 with and
without a uint8 mask array, 512 x 1024^2 float64, axes 0 / 1 / 2, factors 2 / 3 / 4.  One JSON record per case: the
median of the HIP-event times, the algorithmic bytes (every input sample read once + its mask byte, every output
sample and its mask byte written once) and their fraction of 8 TB/s.

    python tools/time_downsample.py [--reps 10]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectral_cube_amd import _lib, ops  # noqa: E402
from spectral_cube_amd.device import DeviceArray, Event, Stream  # noqa: E402

PEAK = 8.0e12


def time_case(cube, mask, axis, f, reps, wide):
    fn = ops.downsample
    st = Stream(cube.device)
    shape = ops.downsample_shape(cube.shape, axis, f, False)
    out = DeviceArray(shape, np.float64 if wide else np.float32, cube.device)
    out_mask = DeviceArray(shape, np.uint8, cube.device)
    for _ in range(2):
        fn(cube, axis, f, mask=mask, out=out, out_mask=out_mask, stream=st)
    times = []
    for _ in range(reps):
        a, b = Event(cube.device), Event(cube.device)
        a.record(st)
        fn(cube, axis, f, mask=mask, out=out, out_mask=out_mask, stream=st)
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_ms(b))
    e = 8 if wide else 4
    nin, nout = int(np.prod(cube.shape)), int(np.prod(shape))
    nbytes = nin * (e + (1 if mask is not None else 0)) + nout * (e + 1)
    ms = float(np.median(times))
    return dict(dtype="float64" if wide else "float32", shape=list(cube.shape), mask="u8" if mask is not None else "none",
                axis=axis, factor=f, median_ms=round(ms, 4), min_ms=round(float(np.min(times)), 4), bytes=nbytes,
                tbps=round(nbytes / ms / 1e9, 3), fraction_of_8tbps=round(nbytes / ms / 1e9 / 8.0, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    _lib.require_gpu()
    rng = np.random.default_rng(0)
    n = 1024
    host = rng.standard_normal((n, n, n), dtype=np.float32)
    cube = DeviceArray.from_numpy(host)
    keep = DeviceArray.from_numpy((rng.random((n, n, n), dtype=np.float32) < 0.8).view(np.uint8))
    del host
    mspec = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, keep)
    for mask in (None, mspec):
        for axis in (0, 1, 2):
            for f in (2, 3, 4):
                print(json.dumps(time_case(cube, mask, axis, f, args.reps, False)), flush=True)
    cube.free()
    keep.free()
    cube64 = DeviceArray.from_numpy(rng.standard_normal((512, n, n)))
    for axis in (0, 1, 2):
        for f in (2, 3, 4):
            print(json.dumps(time_case(cube64, None, axis, f, args.reps, True)), flush=True)


if __name__ == "__main__":
    main()
