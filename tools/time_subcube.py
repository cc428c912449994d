"""Time spc_subcube_f32 / _f64 and spc_mask_bbox_f32 / _f64 (the kernels behind SpectralCube slicing and minimal_subcube) on
the cases of DESIGN.md: 1024^3 float32 with and without a uint8 mask array, 512 x 1024^2 float64; the full view, a
spectral slab, an aligned and an unaligned spatial box, a strided view; the bounding box of an array mask, a predicate
mask and a single voxel.  Next to them the two yardsticks that exist without this feature, timed the same way in the same
process: ops.downsample(axis=0, factor=1) (the bytes of a full-view gather) and ops.stats_global (one read of cube and
mask ending in a small reduction).  One JSON record per case: median / min / max of the HIP-event times, the algorithmic
bytes (selected samples read once + their mask bytes, output samples + mask bytes written once; for the box the bytes
it reads) and their fraction of 8 TB/s.

    python tools/time_subcube.py [--reps 10] [--out profiles/subcube_time.jsonl]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectral_cube_amd import _lib, ops  # noqa: E402
from spectral_cube_amd.device import DeviceArray, Event, Stream  # noqa: E402

PEAK = 8.0e12
VIEWS = {"full": (slice(None),) * 3,
         "slab": (slice(256, 512), slice(None), slice(None)),
         "box_aligned": (slice(None), slice(256, 768), slice(256, 768)),
         "box_unaligned": (slice(None), slice(255, 767), slice(257, 769)),
         "strided": (slice(None, None, 2),) * 3}


def timed(fn, st, reps, device):
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


def record(what, case, dtype, shape, mask, times, nbytes):
    ms = float(np.median(times))
    return dict(kernel=what, case=case, dtype=dtype, shape=list(shape), mask=mask, median_ms=round(ms, 4),
                min_ms=round(float(np.min(times)), 4), max_ms=round(float(np.max(times)), 4), bytes=int(nbytes),
                tbps=round(nbytes / ms / 1e9, 3), fraction_of_8tbps=round(nbytes / ms / 1e9 / (PEAK / 1e12), 3))


def gather_cases(cube, mask, wide, reps, emit, label):
    e = 8 if wide else 4
    dtype = "float64" if wide else "float32"
    st = Stream(cube.device)
    sub, down = ops.subcube, ops.downsample
    nz = cube.shape[0]
    # yardstick: downsample by a factor of 1 moves the bytes of a full-view gather (always with an output mask)
    out = DeviceArray(cube.shape, np.float64 if wide else np.float32, cube.device)
    out_mask = DeviceArray(cube.shape, np.uint8, cube.device)
    n = int(np.prod(cube.shape))
    t = timed(lambda: down(cube, 0, 1, mask=mask, out=out, out_mask=out_mask, stream=st), st, reps, cube.device)
    emit(record("downsample(axis=0, factor=1) [yardstick]", "full", dtype, cube.shape, label, t, n * (e + (1 if mask is not None else 0)) + n * (e + 1)))
    del out, out_mask
    for name, view in VIEWS.items():
        if name == "slab":
            view = (slice(nz // 4, nz // 2),) + view[1:]
        spec = ops.normalize_view(view, cube.shape)
        shape = tuple(a[2] for a in spec)
        starts, steps = [a[0] for a in spec], [a[1] for a in spec]
        out = DeviceArray(shape, np.float64 if wide else np.float32, cube.device)
        out_mask = DeviceArray(shape, np.uint8, cube.device) if mask is not None else None
        t = timed(lambda: sub(cube, starts, steps, shape, mask=mask, out=out, out_mask=out_mask, want_mask=mask is not None, stream=st),
                  st, reps, cube.device)
        m = int(np.prod(shape))
        per = e + (1 if mask is not None else 0)
        emit(record("subcube", name, dtype, cube.shape, label, t, 2 * m * per))
        del out, out_mask


def bbox_cases(cube, masks, wide, reps, emit):
    e = 8 if wide else 4
    dtype = "float64" if wide else "float32"
    st = Stream(cube.device)
    n = int(np.prod(cube.shape))
    stats = ops.stats_global
    d_box = DeviceArray((6,), np.int64, cube.device)
    c = ops._cube_c(cube)

    def box(cube, mask, stream):
        # (the entry point with a box allocated once, then the 48 bytes read back: stats_global ends in a read-back too)
        m = ops._mask_c(mask, cube)
        _lib.call("spc_mask_bbox_f64" if wide else "spc_mask_bbox_f32", cube.device, stream.handle, C.byref(c), C.byref(m), 0,
                  C.c_void_p(d_box.ptr))
        return d_box.get(stream)

    for label, mask, reads_data in masks:
        per = (e if reads_data else 0) + (1 if mask.array is not None else 0)
        t = timed(lambda: stats(cube, mask=mask, stream=st), st, reps, cube.device)
        emit(record("stats_global [yardstick]", "statistics", dtype, cube.shape, label, t, n * (e + (1 if mask.array is not None else 0))))
        t = timed(lambda: box(cube, mask=mask, stream=st), st, reps, cube.device)
        emit(record("mask_bbox", "box", dtype, cube.shape, label, t, n * per))


def main():
    ap = argparse.ArgumentParser()
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

    rng = np.random.default_rng(0)
    n = 1024
    host = rng.standard_normal((n, n, n), dtype=np.float32)
    cube = DeviceArray.from_numpy(host)
    del host
    keep_host = rng.random((n, n, n), dtype=np.float32) < 0.8
    keep = DeviceArray.from_numpy(keep_host.view(np.uint8))
    one_host = np.zeros((n, n, n), np.uint8)
    one_host[517, 300, 811] = 1
    one = DeviceArray.from_numpy(one_host)
    del keep_host, one_host
    mspec = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, keep)
    gather_cases(cube, None, False, args.reps, emit, "none")
    gather_cases(cube, mspec, False, args.reps, emit, "u8")
    bbox_cases(cube, [("u8 array", mspec, False), ("predicate > 3", ops.MaskSpec(_lib.MASK_GT, 3.0, 0.0, None), True),
                      ("u8 array, one voxel", ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, one), False)], False, args.reps, emit)
    cube.free()
    keep.free()
    one.free()
    cube64 = DeviceArray.from_numpy(rng.standard_normal((512, n, n)))
    gather_cases(cube64, None, True, args.reps, emit, "none")
    bbox_cases(cube64, [("predicate > 3", ops.MaskSpec(_lib.MASK_GT, 3.0, 0.0, None), True)], True, args.reps, emit)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
