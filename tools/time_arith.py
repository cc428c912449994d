"""Time spc_arith_f32 (the kernel behind SpectralCube's + - * / **) at 1024^3 float32 with a uint8 mask array: one scalar
step, one map step, one cube-on-cube step, the three-step chain (cube - map) / map2 * 1e3 fused into one pass, and the same
chain as three materialised single steps.  HIP-event medians; per case the algorithmic bytes (the cube read once, 4 B, its
mask byte, the output written once, 4 B, plus the operand: a second cube is another 4 B per voxel, a map is noise) and
their fraction of 8 TB/s.  The yardstick is the read-and-write march of profiles/r05_micro_copy_ceiling.txt (a 4096 MiB
copy, 256-thread blocks, plain loads and stores: 6.2 TB/s; 6.6 TB/s non-temporal).

    python tools/time_arith.py [--reps 20] [--n 1024] [--out profiles/arith_1024.txt]
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


def resident(n, rng, dtype, make):
    """an (n, n, n) DeviceArray filled block by block from one 64-plane host block (the values repeat; the kernel does not care)"""
    block = make(rng, (min(64, n), n, n)).astype(dtype)
    dev = DeviceArray((n, n, n), dtype)
    for z in range(0, n, block.shape[0]):
        dev.planes(z, z + block.shape[0]).upload(block)
    return dev


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    _lib.require_gpu()
    n, rng = args.n, np.random.default_rng(0)
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    cube = resident(n, rng, np.float32, lambda r, s: r.standard_normal(s, dtype=np.float32))
    cube2 = resident(n, rng, np.float32, lambda r, s: r.standard_normal(s, dtype=np.float32))
    keep = resident(n, rng, np.uint8, lambda r, s: r.random(s, dtype=np.float32) < 0.8)
    mask = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, keep)
    amap = DeviceArray.from_numpy(rng.standard_normal((n, n), dtype=np.float32))
    amap2 = DeviceArray.from_numpy((0.5 + rng.random((n, n), dtype=np.float32)))
    out, t1, t2 = (DeviceArray((n, n, n), np.float32) for _ in range(3))
    st = Stream(0)
    vox = n ** 3
    chain = [("sub", amap, 1), ("div", amap2, 1), ("mul", 1e3, 1)]

    def stepwise():
        ops.arith(cube, chain[:1], mask=mask, fill=0.0, out=t1, stream=st)
        ops.arith(t1, chain[1:2], mask=mask, fill=0.0, out=t2, stream=st)
        ops.arith(t2, chain[2:], mask=mask, fill=0.0, out=out, stream=st)

    cases = [("one scalar step: cube * 1e3", lambda: ops.arith(cube, chain[2:], mask=mask, fill=0.0, out=out, stream=st), 9 * vox),
             ("one map step: cube - map", lambda: ops.arith(cube, chain[:1], mask=mask, fill=0.0, out=out, stream=st), 9 * vox + 4 * n * n),
             ("one cube-on-cube step: cube - cube2", lambda: ops.arith(cube, [("sub", cube2, 0)], mask=mask, fill=0.0, out=out, stream=st), 13 * vox),
             ("chain (cube - map) / map2 * 1e3, fused: one pass", lambda: ops.arith(cube, chain, mask=mask, fill=0.0, out=out, stream=st),
              9 * vox + 8 * n * n),
             ("the same chain as three materialised steps", stepwise, 27 * vox + 8 * n * n)]
    for what, fn, nbytes in cases:
        t = timed(fn, st, args.reps, 0)
        ms = float(np.median(t))
        emit(dict(kernel="spc_arith_f32", case=what, shape=[n, n, n], mask="u8", median_ms=round(ms, 4), min_ms=round(float(np.min(t)), 4),
                  max_ms=round(float(np.max(t)), 4), bytes=int(nbytes), tbps=round(nbytes / ms / 1e9, 3),
                  fraction_of_8tbps=round(nbytes / ms / 1e9 / (PEAK / 1e12), 3)))
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
