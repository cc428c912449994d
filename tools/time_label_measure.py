"""Time the per-label measurements (ops.label_measure, csrc/spc_label_measure.hip) of a 1024^3 float32 cube through the
labels of three of tools/time_label.py's fields:

    sparse   signal: the 4 sigma core grown into the 2 sigma envelope - a few per cent of the voxels, a handful of clouds
    dense    full: every voxel one label, one run through the whole array
    islands  random p = 0.31 at connectivity 1: a hundred million labels, most of a voxel or two

each measured twice: the sums alone (count, sum, sum of squares: what sum_labels / mean / variance need) and all four
groups (sums, extrema with positions, first and second moments).  Next to them, timed the same way in the same process on the
same label array, ops.label_objects, which reads the same 4 B / voxel.  One JSON record per case and call: median / min /
max of the HIP-event times of `--reps` calls after 2 warm-ups (a call = its launches and the 4-byte flag it waits for), the
algorithmic bytes - 4 B of labels per voxel plus the 4 B sample of every labelled voxel (no mask array here) - and their
fraction of 8 TB/s.  The sparse field is measured in two more forms: with a uint8 mask array (the 2 sigma mask, which includes
every labelled voxel: 1 B more per labelled voxel) and on a float64 copy of the cube (8 B samples, and the second launch
that finds the positions of the extrema).  HIP events see a call, not its kernels: the per-kernel times (init, the main
pass, the float64 position launch, finish) are in profiles/label_measure_rocprof_kernel_stats.csv, from

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_label_measure.py --forms --reps 3

    python tools/time_label_measure.py [--n 1024] [--reps 5] [--out profiles/label_measure_time.jsonl]
    python tools/time_label_measure.py --scipy [--n 256] [--out FILE]    # scipy.ndimage.sum_labels etc. on one host core
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_morphology import record, synthetic  # noqa: E402

ALL = ("sums", "extrema", "first", "second")


def run_scipy(n, emit):
    import scipy.ndimage as ndi
    d = synthetic(n)
    core = ndi.binary_opening(d > 4.0, structure=np.ones((2, 1, 1), bool))
    fields = {"sparse (signal)": lambda: ndi.binary_propagation(core, mask=d > 2.0),
              "dense (full)": lambda: np.ones((n, n, n), bool),
              "islands (random p=0.31)": lambda: np.random.default_rng(1).random((n, n, n), dtype=np.float32) < 0.31}
    for name, make in fields.items():
        lab, nl = ndi.label(make())
        index = np.arange(1, nl + 1)
        labelled = int((lab > 0).sum())
        for what, fn in (("scipy.ndimage.sum_labels [host, one core]", lambda: ndi.sum_labels(d, lab, index)),
                         ("scipy.ndimage.variance [host, one core]", lambda: ndi.variance(d, lab, index)),
                         ("scipy.ndimage.extrema + center_of_mass [host, one core]",
                          lambda: (ndi.extrema(d, lab, index), ndi.center_of_mass(d, lab, index)))):
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                fn()
                t.append(1e3 * (time.perf_counter() - t0))
            emit(record(what, name, lab.shape, t, 4 * lab.size + 4 * labelled, labels=int(nl), labelled_fraction=round(labelled / lab.size, 4)))


def run_device(n, reps, emit, only_forms=False):
    from spectral_cube_amd import _lib, ops
    from spectral_cube_amd.device import DeviceArray, Event, Stream
    from spectral_cube_amd.morphology import _offsets, generate_binary_structure as gbs
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

    shape, vox = (n, n, n), n ** 3
    labels = DeviceArray(shape, np.int32, dev)
    ws = DeviceArray((int(_lib.load().spc_label_workspace_bytes(*shape)),), np.uint8, dev)
    cube = DeviceArray.from_numpy(synthetic(n))

    def measure(name, what, data, spec, want, nl, labelled, base, more):
        bits = sum(ops.MEASURE_GROUPS[g] for g in want)
        out = {k: DeviceArray((nl + 1,) + cols, data.dtype if dt is None else dt, dev)
               for k, (g, cols, dt) in ops._MEASURE_TABLES.items() if g in want}
        mws = DeviceArray((int(_lib.load().spc_label_measure_workspace_bytes(nl, bits)),), np.uint8, dev)
        t = timed(lambda: ops.label_measure(data, labels, nl, mask_spec=spec, want=want, out=out, stream=st, workspace=mws))
        per = data.dtype.itemsize + (1 if spec is not None else 0)
        emit(record(what, name, shape, t, 4 * vox + per * labelled, times_label_objects=round(float(np.median(t)) / base, 3), **more))

    def one_case(name, mask, forms=None):
        nl = ops.label(mask, gbs(3, 1), out=labels, stream=st, workspace=ws)[1]
        tables = {"sizes": DeviceArray((nl + 1,), np.int64, dev), "bbox": DeviceArray((nl + 1, 6), np.int32, dev)}
        t_obj = timed(lambda: ops.label_objects(labels, nl, out=tables, stream=st, workspace=ws))
        labelled = vox - int(tables["sizes"].get(st)[0])
        more = dict(labels=int(nl), labelled_fraction=round(labelled / vox, 4))
        emit(record("label_objects [yardstick]", name, shape, t_obj, 4 * vox, **more))
        del tables
        base = float(np.median(t_obj))
        for what, want in (("label_measure sums", ("sums",)), ("label_measure all groups", ALL)):
            if not only_forms:
                measure(name, what, cube, None, want, nl, labelled, base, more)
            for form, (data, spec) in (forms or {}).items():
                measure(name, "%s [%s]" % (what, form), data(), spec, want, nl, labelled, base, more)

    lo = ops.mask_include(cube, ops.MaskSpec(_lib.MASK_GT, 2.0, 0.0, None), stream=st)
    hi = ops.mask_include(cube, ops.MaskSpec(_lib.MASK_GT, 4.0, 0.0, None), stream=st)
    pair = _offsets(np.ones((2, 1, 1), bool), 0)
    core = ops.mask_morph(ops.mask_morph(hi, pair, _lib.MORPH_ERODE, stream=st), pair, _lib.MORPH_DILATE, stream=st)
    signal = ops.mask_morph(core, _offsets(gbs(3, 1), 0), _lib.MORPH_DILATE, iterations=-1, mask=lo, stream=st)
    del hi, core
    ops.release_workspaces()
    wide = []

    def cube64():                                                     # made when it is first asked for, kept for the second want
        if not wide:
            wide.append(DeviceArray.from_numpy(cube.get().astype(np.float64), dev))
        return wide[0]
    one_case("sparse (signal: 4 sigma core grown into the 2 sigma envelope)", signal,
             forms={"u8 mask array": (lambda: cube, ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, lo)), "float64 cube": (cube64, None)})
    del signal, lo, wide[:]
    if only_forms:
        return
    one_case("dense (full)", DeviceArray.from_numpy(np.ones(shape, np.uint8), dev))
    one_case("islands (random p=0.31)",
             DeviceArray.from_numpy((np.random.default_rng(1).random(shape, dtype=np.float32) < 0.31).view(np.uint8), dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scipy", action="store_true")
    ap.add_argument("--forms", action="store_true", help="the sparse field's mask-array and float64 forms only (for a kernel trace)")
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
        run_device(args.n or 1024, args.reps, emit, only_forms=args.forms)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
