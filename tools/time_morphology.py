"""Time binary mask morphology (ops.mask_morph, spc_mask_morph_u8) on a 1024^3 uint8 include array: (a) one dilation at
connectivity 1, at connectivity 3 and with a 5x5x5 box, and the floor of one step with the one-voxel structure (pack, one
step, unpack); (b) the opening with the (2, 1, 1) element of the 4 sigma mask; (c) the propagation of that core into the
2 sigma mask, with the sweeps it took.  Next to them the yardstick that exists without this feature, timed the same way in
the same process: ops.mask_include with a scalar threshold on the same cube (4 B in, 1 B out per voxel).  The cube is
unit noise plus a few Gaussian clouds of peak 8.  One JSON record per case: median / min / max of the HIP-event times of
`--reps` runs after 2 warm-ups, the algorithmic bytes (1 B per voxel of input read, 1 B per voxel of mask read where there
is one, 1 B per voxel written - the intermediate of the opening is not counted) and their fraction of 8 TB/s.

    python tools/time_morphology.py [--n 1024] [--reps 10] [--out profiles/morphology_time.jsonl]
    python tools/time_morphology.py --scipy [--n 256] [--out FILE]     # scipy.ndimage on one host core, for scale: another size
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12


def synthetic(n, seed=0):
    """unit noise plus Gaussian clouds of peak 8 and sigma n / 32 ... n / 16, float32 (n, n, n)"""
    rng = np.random.default_rng(seed)
    d = rng.standard_normal((n, n, n), dtype=np.float32)
    for _ in range(6):
        s = rng.uniform(n / 32, n / 16, 3)
        c = [rng.uniform(4 * s[a], n - 4 * s[a]) for a in range(3)]
        lo = [max(0, int(c[a] - 4 * s[a])) for a in range(3)]
        hi = [min(n, int(c[a] + 4 * s[a]) + 1) for a in range(3)]
        g = [np.exp(-0.5 * ((np.arange(lo[a], hi[a]) - c[a]) / s[a]) ** 2).astype(np.float32) for a in range(3)]
        d[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]] += 8.0 * g[0][:, None, None] * g[1][None, :, None] * g[2][None, None, :]
    return d


def structures():
    from spectral_cube_amd.morphology import generate_binary_structure as gbs
    return {"point": np.ones((1, 1, 1), bool), "connectivity 1": gbs(3, 1), "connectivity 3": gbs(3, 3), "box 5x5x5": np.ones((5, 5, 5), bool),
            "pair (2,1,1)": np.ones((2, 1, 1), bool)}


def record(what, case, shape, times, nbytes, **more):
    ms = float(np.median(times))
    rec = dict(kernel=what, case=case, shape=list(shape), median_ms=round(ms, 4), min_ms=round(float(np.min(times)), 4),
               max_ms=round(float(np.max(times)), 4), bytes=int(nbytes), tbps=round(nbytes / ms / 1e9, 3),
               fraction_of_8tbps=round(nbytes / ms / 1e9 / (PEAK / 1e12), 4))
    rec.update(more)
    return rec


def run_scipy(n, emit):
    import scipy.ndimage as ndi
    d = synthetic(n)
    hi, lo = d > 4.0, d > 2.0
    S = structures()
    vox = n ** 3

    def timed(fn):
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            out = fn()
            t.append(1e3 * (time.perf_counter() - t0))
        return t, out
    for name in ("connectivity 1", "connectivity 3", "box 5x5x5"):
        t, _ = timed(lambda: ndi.binary_dilation(lo, structure=S[name]))
        emit(record("scipy.ndimage.binary_dilation [host, one core]", name, d.shape, t, 2 * vox))
    t, core = timed(lambda: ndi.binary_opening(hi, structure=S["pair (2,1,1)"]))
    emit(record("scipy.ndimage.binary_opening [host, one core]", "pair (2,1,1)", d.shape, t, 2 * vox))
    t, sig = timed(lambda: ndi.binary_propagation(core, mask=lo))
    emit(record("scipy.ndimage.binary_propagation [host, one core]", "4 sigma core into 2 sigma mask", d.shape, t, 3 * vox,
                core_voxels=int(core.sum()), mask_voxels=int(lo.sum()), result_voxels=int(sig.sum())))


def run_device(n, reps, emit):
    from spectral_cube_amd import _lib, ops
    from spectral_cube_amd.device import DeviceArray, Event, Stream
    from spectral_cube_amd.morphology import _offsets
    _lib.require_gpu()
    dev = 0
    st = Stream(dev)

    def timed(fn):
        for _ in range(2):
            fn()
        times = []
        for _ in range(reps):
            a, b = Event(dev), Event(dev)
            a.record(st)
            fn()
            b.record(st)
            b.synchronize()
            times.append(a.elapsed_ms(b))
        return times
    cube = DeviceArray.from_numpy(synthetic(n))
    shape, vox = cube.shape, n ** 3
    t = timed(lambda: ops.mask_include(cube, ops.MaskSpec(_lib.MASK_GT, 2.0, 0.0, None), stream=st))
    emit(record("mask_include [yardstick]", "cube > 2", shape, t, 5 * vox))
    lo = ops.mask_include(cube, ops.MaskSpec(_lib.MASK_GT, 2.0, 0.0, None), stream=st)
    hi = ops.mask_include(cube, ops.MaskSpec(_lib.MASK_GT, 4.0, 0.0, None), stream=st)
    cube.free()
    out, tmp = DeviceArray(shape, np.uint8, dev), DeviceArray(shape, np.uint8, dev)
    ws = DeviceArray((int(_lib.load().spc_mask_morph_workspace_bytes(*shape)),), np.uint8, dev)
    S = {k: _offsets(v, 0) for k, v in structures().items()}
    kw = dict(stream=st, workspace=ws)
    for name in ("point", "connectivity 1", "connectivity 3", "box 5x5x5"):
        t = timed(lambda: ops.mask_morph(lo, S[name], _lib.MORPH_DILATE, out=out, **kw))
        emit(record("mask_morph dilate, 1 step", name, shape, t, 2 * vox))
    pair = S["pair (2,1,1)"]

    def opening():
        ops.mask_morph(hi, pair, _lib.MORPH_ERODE, out=tmp, **kw)
        return ops.mask_morph(tmp, pair, _lib.MORPH_DILATE, out=out, **kw)
    t = timed(opening)
    emit(record("mask_morph opening (erode, dilate)", "pair (2,1,1)", shape, t, 2 * vox))
    core = DeviceArray(shape, np.uint8, dev)
    ops.mask_morph(tmp, pair, _lib.MORPH_DILATE, out=core, **kw)
    sweeps = []
    t = timed(lambda: sweeps.append(ops.mask_morph(core, S["connectivity 1"], _lib.MORPH_DILATE, iterations=-1, mask=lo, out=out,
                                                   return_iterations=True, **kw)[1]))
    st.synchronize()
    count = lambda a: int(np.count_nonzero(a.get(st)))           # noqa: E731
    emit(record("mask_morph propagation (dilate to the fixed point under a mask)", "4 sigma core into 2 sigma mask", shape, t, 3 * vox,
                sweeps=int(sweeps[-1]), core_voxels=count(core), mask_voxels=count(lo), result_voxels=count(out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sink = open(args.out, "a") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()
    if args.scipy:
        run_scipy(args.n or 256, emit)
    else:
        run_device(args.n or 1024, args.reps, emit)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
