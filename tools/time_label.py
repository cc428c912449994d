"""Time connected-component labelling (ops.label / label_objects / label_select, csrc/spc_label.hip) and
labelling.remove_small_objects end to end on 1024^3 uint8 include arrays:

    signal       the README's mask: the 4 sigma core (opened with a (2, 1, 1) element) grown into the 2 sigma envelope
    random       a random field at p = 0.31, connectivity 1: near the site-percolation threshold, the widest size spectrum
    full         every voxel True: one component, the atomic worst case of label_objects
    serpentine   one voxel-wide corridor winding through every second plane: n / 2 components, each crossing the plane
                 hundreds of times
    checkerboard (x + y + z) % 2 at connectivity 1: n^3 / 2 labels (no end-to-end run: its tables alone are 17 GB)

Next to them the yardsticks that exist without this feature, timed the same way in the same process: ops.mask_include with
a scalar threshold (4 B in, 1 B out per voxel) and the propagation of the signal case.  One JSON record per case and
kernel: median / min / max of the HIP-event times of `--reps` runs after 2 warm-ups (remove_small_objects: a host clock
around the call, which ends in device-to-host copies), the algorithmic bytes - label 1 B read + 4 B written per voxel,
label_objects 4 B read, label_select 4 B read + 1 B written - and their fraction of 8 TB/s.

    python tools/time_label.py [--n 1024] [--reps 5] [--out profiles/label_time.jsonl]
    python tools/time_label.py --scipy [--n 256] [--out FILE]     # scipy.ndimage.label + np.bincount on one host core
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


def serpentine(n):
    """every second plane holds one corridor, one voxel wide: rows 4 apart along x, joined at alternating ends"""
    m = np.zeros((n, n, n), bool)
    rows = list(range(1, n - 1, 4))
    m[::2, 1:n - 1:4, 1:n - 1] = True
    for i, j in enumerate(rows[:-1]):
        m[::2, j:j + 5, (n - 2) if i % 2 == 0 else 1] = True
    return m


def host_cases(n):
    """name -> (bool array maker, connectivity); made one at a time: each is n^3 bytes on the host"""
    z, y, x = (a.astype(np.uint8) for a in np.ogrid[:n, :n, :n])          # (parity survives the wrap at 256)
    return {"random p=0.31": (lambda: np.random.default_rng(1).random((n, n, n), dtype=np.float32) < 0.31, 1),
            "full": (lambda: np.ones((n, n, n), bool), 1),
            "serpentine": (lambda: serpentine(n), 1),
            "checkerboard": (lambda: ((x + y + z) & 1).astype(bool), 1)}


def run_scipy(n, emit):
    import scipy.ndimage as ndi
    d = synthetic(n)
    core = ndi.binary_opening(d > 4.0, structure=np.ones((2, 1, 1), bool))
    masks = {"signal": (lambda: ndi.binary_propagation(core, mask=d > 2.0), 1)}
    masks.update(host_cases(n))
    for name, (make, conn) in masks.items():
        x = make()
        t, n_labels = [], 0
        for _ in range(3):
            t0 = time.perf_counter()
            lab, n_labels = ndi.label(x, structure=ndi.generate_binary_structure(3, conn))
            np.bincount(lab.ravel(), minlength=n_labels + 1)
            t.append(1e3 * (time.perf_counter() - t0))
        emit(record("scipy.ndimage.label + np.bincount [host, one core]", name, x.shape, t, 5 * x.size, labels=int(n_labels)))


def run_device(n, reps, emit):
    from spectral_cube_amd import _lib, labelling, ops
    from spectral_cube_amd import masks as M
    from spectral_cube_amd.device import DeviceArray, Event, Stream, synchronize
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

    def wall(fn):
        fn()
        times = []
        for _ in range(max(3, reps // 2)):
            synchronize(dev)
            t0 = time.perf_counter()
            fn()
            synchronize(dev)
            times.append(1e3 * (time.perf_counter() - t0))
        return times
    shape, vox = (n, n, n), n ** 3
    labels = DeviceArray(shape, np.int32, dev)
    out = DeviceArray(shape, np.uint8, dev)
    ws = DeviceArray((int(_lib.load().spc_label_workspace_bytes(*shape)),), np.uint8, dev)

    def one_case(name, mask, conn, end_to_end=True):
        s = gbs(3, conn)
        count = []
        t = timed(lambda: count.append(ops.label(mask, s, out=labels, stream=st, workspace=ws)[1]))
        nl = count[-1]
        emit(record("label", name, shape, t, 5 * vox, labels=int(nl), connectivity=conn))
        tables = {"sizes": DeviceArray((nl + 1,), np.int64, dev), "bbox": DeviceArray((nl + 1, 6), np.int32, dev)}
        t = timed(lambda: ops.label_objects(labels, nl, out=tables, stream=st, workspace=ws))
        sizes = tables["sizes"].get(st) if end_to_end else None
        emit(record("label_objects", name, shape, t, 4 * vox, labels=int(nl),
                    largest=int(sizes[1:].max()) if sizes is not None and nl else None))
        keep = DeviceArray.from_numpy((np.random.default_rng(3).random(nl + 1) < 0.5).astype(np.uint8), dev)
        t = timed(lambda: ops.label_select(labels, nl, keep, out=out, stream=st))
        emit(record("label_select", name, shape, t, 5 * vox, labels=int(nl), table_in_lds=bool(nl + 1 <= 32768)))
        del tables, keep
        if end_to_end:
            src = M.DeviceBooleanMask(mask)
            t = wall(lambda: labelling.remove_small_objects(src, min_size=50, min_channels=2, structure=s).device_array())
            emit(record("remove_small_objects [end to end, host clock]", name, shape, t, 6 * vox, labels=int(nl)))

    cube = DeviceArray.from_numpy(synthetic(n))
    t = timed(lambda: ops.mask_include(cube, ops.MaskSpec(_lib.MASK_GT, 2.0, 0.0, None), stream=st))
    emit(record("mask_include [yardstick]", "cube > 2", shape, t, 5 * vox))
    lo = ops.mask_include(cube, ops.MaskSpec(_lib.MASK_GT, 2.0, 0.0, None), stream=st)
    hi = ops.mask_include(cube, ops.MaskSpec(_lib.MASK_GT, 4.0, 0.0, None), stream=st)
    cube.free()
    pair = _offsets(np.ones((2, 1, 1), bool), 0)
    core = ops.mask_morph(ops.mask_morph(hi, pair, _lib.MORPH_ERODE, stream=st), pair, _lib.MORPH_DILATE, stream=st)
    signal = DeviceArray(shape, np.uint8, dev)
    c1 = _offsets(gbs(3, 1), 0)
    t = timed(lambda: ops.mask_morph(core, c1, _lib.MORPH_DILATE, iterations=-1, mask=lo, out=signal, stream=st))
    emit(record("mask_morph propagation [yardstick]", "4 sigma core into 2 sigma mask", shape, t, 3 * vox))
    del hi, lo, core
    ops.release_workspaces()
    one_case("signal (4 sigma core grown into the 2 sigma envelope)", signal, 1)
    del signal
    for name, (make, conn) in host_cases(n).items():
        mask = DeviceArray.from_numpy(make().view(np.uint8), dev)
        one_case(name, mask, conn, end_to_end=name != "checkerboard")
        del mask


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=None)
    ap.add_argument("--reps", type=int, default=5)
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
