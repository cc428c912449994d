"""Time spc_mask_eval_f32 (a mask expression evaluated once on the device) at 1024^3 float32 next to its yardstick and to
the host route it replaces:

  (a) ops.mask_eval of ``cube > map``                      one read of the cube, a (ny, nx) float32 map, one byte written
  (b) ops.mask_eval of ``(cube > map) | (cube < -map)``    the same traffic plus a second map: the slot is read once
  (c) ops.mask_include with a scalar threshold             the existing "one read, one byte written" kernel
  (d) the host route of mask (a): masks.lower_mask() in its host form plus the upload of the uint8 array - what
      SpectralCube._mask_spec() did for this mask before masks were compiled (cube to the host, numpy, broadcast, upload);
      wall clock, one run

(a) - (c): median / min / max of HIP-event times over --reps launches after --warmup, operands resident, outputs
preallocated where the entry point allows; algorithmic bytes and their fraction of 8 TB/s.

    python tools/time_mask_eval.py [--n 1024] [--reps 50] [--warmup 5] [--no-host-route] [--out profiles/mask_eval_1024.txt]
"""
import argparse
import operator
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectral_cube_amd import SpectralCube, _lib, ops  # noqa: E402
from spectral_cube_amd import masks as M  # noqa: E402
from spectral_cube_amd.device import DeviceArray, Event, Stream, device_info, synchronize  # noqa: E402

PEAK = 8.0e12


def timed(fn, st, reps, warmup, device):
    for _ in range(warmup):
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


def line(tag, what, times, nbytes):
    ms = float(np.median(times))
    return "(%s) %-46s median %8.3f ms  min %8.3f  max %8.3f  bytes %.4e  %6.3f TB/s  %5.1f %% of 8 TB/s" % (
        tag, what, ms, np.min(times), np.max(times), nbytes, nbytes / ms / 1e9, 100.0 * nbytes / ms / 1e9 / (PEAK / 1e12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-host-route", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.require_gpu()
    device, n = 0, a.n
    shape = (n, n, n)
    rng = np.random.default_rng(5)
    block = rng.standard_normal((min(64, n), n, n), dtype=np.float32)       # the cube: this block of planes, repeated
    dev = DeviceArray(shape, np.float32, device)
    for z0 in range(0, n, block.shape[0]):
        dev.planes(z0, min(z0 + block.shape[0], n)).upload(block[:min(block.shape[0], n - z0)])
    rms = (0.5 + rng.random((n, n))).astype(np.float32)
    cube = SpectralCube.from_device(dev)
    mask_a = M.LazyComparisonMask(operator.gt, rms, cube=cube)
    mask_b = mask_a | M.LazyComparisonMask(operator.lt, -rms, cube=cube)
    st = Stream(device)
    out = DeviceArray(shape, np.uint8, device)
    vox, spaxels = float(n) ** 3, float(n) ** 2
    lines = ["mask expressions at %d^3 float32, %s, %d launches after %d warm-ups, HIP events" % (
        n, device_info(device)["name"], a.reps, a.warmup)]

    def resident(mask):
        prog = M.compile_mask(mask, cube, shape, False)
        prog.slots = [dev]
        prog.operands = [(DeviceArray.from_numpy(arr, device), strides) for arr, strides in prog.operands]
        return prog

    results = {}
    for tag, what, mask, maps in (("a", "mask_eval: cube > map", mask_a, 1), ("b", "mask_eval: (cube > map) | (cube < -map)", mask_b, 2)):
        prog = resident(mask)
        t = timed(lambda: ops.mask_eval(prog, shape, device, np.float32, out=out, stream=st), st, a.reps, a.warmup, device)
        results[tag] = float(np.median(t))
        # every plane re-reads the map(s): 4 B per spaxel, plane and map (from cache after the first plane)
        lines.append(line(tag, what, t, 5.0 * vox + 4.0 * maps * spaxels * n))
    spec = ops.MaskSpec(_lib.MASK_GT, thr_lo=0.75)
    t = timed(lambda: ops.mask_include(dev, spec, stream=st), st, a.reps, a.warmup, device)
    results["c"] = float(np.median(t))
    lines.append(line("c", "mask_include: cube > 0.75 (scalar) [yardstick]", t, 5.0 * vox))
    lines.append("(a) / (c) = %.3f   (b) / (a) = %.3f" % (results["a"] / results["c"], results["b"] / results["a"]))
    # same answer from both routes before anything is said about speed
    got = ops.mask_eval(resident(mask_a), shape, device, np.float32)
    if not a.no_host_route:
        synchronize(device)
        t0 = time.perf_counter()
        flags, lo, hi, arr = M.lower_mask(mask_a, cube, shape)
        t1 = time.perf_counter()
        up = DeviceArray.from_numpy(arr, device)
        synchronize(device)
        t2 = time.perf_counter()
        lines.append("(d) host route of (a): lower_mask %.3f s (cube to host %.2e B, numpy, broadcast) + upload %.3f s (%.2e B) = %.3f s"
                     "  = %.0f x (a)" % (t1 - t0, 4.0 * vox, t2 - t1, vox, t2 - t0, (t2 - t0) * 1e3 / results["a"]))
        same = np.array_equal(got.planes(0, min(8, n)).get(), arr[:min(8, n)])
        lines.append("first planes of (a) equal the host route's array: %s" % same)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
