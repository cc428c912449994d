"""Time the polynomial-baseline kernels (ops.baseline_fit / ops.baseline_apply, csrc/spc_baseline.hip) on resident cubes:
n^3 float32 with and without a uint8 mask array (80 % included), (n/2) x n^2 float64, and 4n x (n/16)^2 float32 - the
single-dish map whose channel list the fit cuts into segments; orders 0, 1, 3, 5; all channels and an 80 % list of two
windows; the fit alone, the apply alone and the two back to back.  One JSON record per case: median / min / max of the
HIP-event times (--reps after 2 warm-ups), the algorithmic bytes - for the fit the mask bytes of the listed channels and the
samples they include, for the apply 2 x the cube - and their fraction of 8 TB/s; at order 5 also the float64 rate of the
fit, 54 operations per included sample (21 + 6 products and as many sums, none fused), against the 78.6 TFLOP/s vector
peak.  The calls go through ops, so a fit includes the upload of its basis table (nz x (order + 1) float64).

Yardsticks, timed the same way in the same process on the n^3 float32 cube: ops.moments (m0, m1, m2: one masked read
pass), ops.arith cube - map (one read and one write pass), and the documented continuum route
cube - cube.with_mask(linefree).median(axis=0) as ops.percentile_axis0 + ops.arith, which needs nothing this unit added.

    python tools/time_baseline.py [--n 1024] [--reps 10] [--out profiles/baseline_time.jsonl]
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
F64_PEAK_TFLOPS = 78.6
ORDERS = (0, 1, 3, 5)


def timed(fn, st, reps, device=0):
    for _ in range(2):
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


def two_windows(nz):
    """80 % of the channels: everything but the middle fifth"""
    k = np.arange(nz)
    return k[(k < (2 * nz) // 5) | (k >= (3 * nz) // 5)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    def record(base, t, nbytes, flops=None):
        ms = float(np.median(t))
        rec = dict(base, median_ms=round(ms, 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4), bytes=int(nbytes),
                   tbps=round(nbytes / ms / 1e9, 4), fraction_of_8tbps=round(nbytes / ms / 1e9 / (PEAK / 1e12), 4))
        if flops is not None:
            rec.update(f64_ops=int(flops), tflops=round(flops / ms / 1e9, 2),
                       fraction_of_f64_vector_peak=round(flops / ms / 1e9 / F64_PEAK_TFLOPS, 3))
        emit(rec)

    n = args.n
    st = Stream(0)
    rng = np.random.default_rng(0)
    cubes = (("f32", (n, n, n), np.float32), ("f64", (n // 2, n, n), np.float64), ("single-dish", (4 * n, n // 16, n // 16), np.float32))
    for cname, shape, dtype in cubes:
        nz, ny, nx = shape
        host = rng.standard_normal(shape, dtype=np.float32)
        cube = DeviceArray.from_numpy(host, dtype=dtype)
        del host
        item = np.dtype(dtype).itemsize
        masks = [("none", None, None)]
        if cname == "f32":
            keep_host = rng.random(shape, dtype=np.float32) < 0.8
            masks.append(("u8", ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, DeviceArray.from_numpy(keep_host.view(np.uint8))), keep_host))
        out = DeviceArray(shape, dtype, 0)
        lists = (("all", None, nz), ("two windows 80 %", two_windows(nz), len(two_windows(nz))))
        for order in ORDERS:
            coef = DeviceArray((order + 1, ny, nx), np.float64, 0)
            npts = DeviceArray((ny, nx), np.int32, 0)
            for lname, chan, nfit in lists:
                for mname, spec, keep_host in masks:
                    base = dict(cube=cname, shape=list(shape), dtype=np.dtype(dtype).name, order=order, channels=lname, mask=mname,
                                segments=ops.baseline_segments(shape, nfit))
                    if keep_host is None:
                        included = nfit * ny * nx
                        fbytes = included * item
                    else:
                        included = int(keep_host[chan].sum() if chan is not None else keep_host.sum())
                        fbytes = nfit * ny * nx + included * item
                    flops = 54 * included if order == 5 else None
                    t = timed(lambda: ops.baseline_fit(cube, order, channels=chan, mask_spec=spec, coef=coef, npts=npts, stream=st),
                              st, args.reps)
                    record(dict(base, kernel="baseline_fit"), t, fbytes, flops)
                    if lname == "all":
                        abytes = 2 * nz * ny * nx * item
                        if mname == "none":
                            t = timed(lambda: ops.baseline_apply(cube, coef, out=out, stream=st), st, args.reps)
                            record(dict(base, kernel="baseline_apply"), t, abytes)

                        def both():
                            ops.baseline_fit(cube, order, channels=chan, mask_spec=spec, coef=coef, npts=npts, stream=st)
                            ops.baseline_apply(cube, coef, out=out, stream=st)
                        t = timed(both, st, args.reps)
                        record(dict(base, kernel="baseline_fit + baseline_apply"), t, fbytes + abytes)
        if cname == "f32":
            # the yardsticks
            cen = DeviceArray.from_numpy(np.arange(nz, dtype=np.float64))
            amap = DeviceArray.from_numpy(np.zeros((ny, nx), np.float32))
            for mname, spec, keep_host in masks:
                base = dict(cube=cname, shape=list(shape), dtype="float32", mask=mname)
                included = nz * ny * nx if keep_host is None else int(keep_host.sum())
                rbytes = included * 4 + (0 if keep_host is None else nz * ny * nx)
                t = timed(lambda: ops.moments(cube, cen, mask=spec, stream=st), st, args.reps)
                record(dict(base, kernel="moments [yardstick: one masked read pass]"), t, rbytes)
                med = DeviceArray((ny, nx), np.float32, 0)

                def route():
                    ops.percentile_axis0(cube, 50.0, mask=spec, stream=st, out=med)
                    ops.arith(cube, [("sub", med, False)], out=out, stream=st)
                t = timed(route, st, max(3, args.reps // 3))
                record(dict(base, kernel="percentile_axis0(50) + arith sub [yardstick: the documented continuum route]"), t,
                       rbytes + 2 * nz * ny * nx * 4)
            t = timed(lambda: ops.arith(cube, [("sub", amap, False)], out=out, stream=st), st, args.reps)
            record(dict(cube=cname, shape=list(shape), dtype="float32", mask="none", kernel="arith cube - map [yardstick: one read + one write pass]"),
                   t, 2 * nz * ny * nx * 4)
        del cube, out, masks
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
