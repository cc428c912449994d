"""Time the fused moment kernel (ops.moments -> m0, m1, m2) at 1024^3 float32 under five kinds of mask: the benchmark's mask
(data > 2 sigma with a 1 % flip), a signal mask (data > 5 sigma), 80 % random, all ones and no mask array (where the
switches select nothing).  Six forms of the launch, alternating in two rounds: "loop" = the loop that loads every sample
(SPC_MOMENTS_MASK_FIRST=0), "bytes" = the mask-first march on the mask's bytes (SPC_MOMENTS_MASK_BITS=0), "bits" = the same
march on the packed form of a reused MaskSpec (SPC_MOMENTS_LIST=0), "vlist" = the reused MaskSpec on the reused cube as the
library runs it by default (the voxel list where it is kept - `vlisted` -, the list of included lane segments where the
voxel list is refused - `vrefused`, `listed` - and the bits march where the list is refused too - `refused`; --vlist-u sets
SPC_MOMENTS_VLIST_U), "list" = the same with SPC_MOMENTS_VLIST=0, which reads the list where it is kept (it runs after
"vlist": a spec remembers that the switch kept it from compacting; --list-u sets SPC_MOMENTS_LIST_U), "fresh" = a new MaskSpec at every call (always its first use: the
byte kernel, what a mask used once costs).  The switches are read per call.  With a mask array also one "pack" record: the
one-off spc_mask_pack_bits launch.  Cube and masks are one seeded 16-row tile repeated along y, as in bench.py.  One JSON
record per mask and form: median / min / max of the HIP-event times of the launches, and the algorithmic 5 (4 without an
array) bytes per voxel over the median.

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

SWITCH, BITS, LIST, LIST_U = "SPC_MOMENTS_MASK_FIRST", "SPC_MOMENTS_MASK_BITS", "SPC_MOMENTS_LIST", "SPC_MOMENTS_LIST_U"
VLIST, VLIST_U = "SPC_MOMENTS_VLIST", "SPC_MOMENTS_VLIST_U"
# form -> the four switches
FORMS = {"loop": ("0", "0", "0", "0"), "bytes": ("1", "0", "0", "0"), "bits": ("1", "1", "0", "0"), "vlist": ("1", "1", "1", "1"),
         "list": ("1", "1", "1", "0"), "fresh": ("1", "1", "1", "1")}


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
    ap.add_argument("--list-u", default=None, choices=("4", "8"), help="entry rows in flight per lane of the list form")
    ap.add_argument("--vlist-u", default=None, choices=("8", "16"), help="entry rows in flight per lane of the voxel-list form")
    args = ap.parse_args()
    _lib.require_gpu()
    if args.list_u:
        os.environ[LIST_U] = args.list_u
    if args.vlist_u:
        os.environ[VLIST_U] = args.vlist_u
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

        def record(form, round_, t, **more):
            ms = float(np.median(t))
            rec = dict(mask=label, valid_fraction=round(float(np.count_nonzero(tmask)) / tmask.size, 4) if tmask is not None else 1.0,
                       shape=list(shape), form=form, mask_first=int(FORMS.get(form, ("1",))[0]), round=round_, launches=len(t),
                       median_ms=round(ms, 4), min_ms=round(float(np.min(t)), 4), max_ms=round(float(np.max(t)), 4),
                       algorithmic_tbps=round(n ** 3 * per_voxel / ms / 1e9, 3), **more)
            line = json.dumps(rec)
            print(line, flush=True)
            if sink:
                sink.write(line + "\n")
                sink.flush()

        def launch(m):
            return ops.moments(cube, d_cen, dv=500.0, m1_add=cref + v[0], mask=m, want=("m0", "m1", "m2"), stream=st, out=out)

        for round_ in range(2):                                 # the forms alternate: a drift shows as a difference between rounds
            for form, (first, bits, lst, vlst) in FORMS.items():
                if spec is None and form in ("bits", "list", "vlist", "fresh"):
                    continue                                    # no mask array: nothing to pack
                os.environ[SWITCH], os.environ[BITS], os.environ[LIST], os.environ[VLIST] = first, bits, lst, vlst   # (read per call)
                if form == "fresh":
                    fn = lambda: launch(ops.MaskSpec(_lib.MASK_ARRAY, array=maskd))     # noqa: E731
                else:
                    fn = lambda: launch(spec)                                           # noqa: E731
                t = timed(fn, st, args.reps, device)
                lists = spec is not None and form in ("list", "vlist")
                record(form, round_, t, packed=bool(spec is not None and spec._bits is not None and form in ("bits", "list", "vlist")),
                       listed=bool(lists and spec._list is not None), refused=bool(lists and spec._list_failed),
                       list_bytes=spec._list.nbytes if lists and spec._list is not None else 0,
                       vlisted=bool(form == "vlist" and spec is not None and spec._vlist is not None),
                       vrefused=bool(form == "vlist" and spec is not None and spec._vlist_failed),
                       vlist_bytes=spec._vlist.nbytes if form == "vlist" and spec is not None and spec._vlist is not None else 0)
        if spec is not None:
            import ctypes as C
            need = int(_lib.load().spc_mask_bits_bytes(n, n, n))
            bits_buf = DeviceArray((need,), np.uint8, device)
            m = spec.to_c()
            t = timed(lambda: _lib.call("spc_mask_pack_bits", device, st.handle, n, n, n, C.byref(m), C.c_void_p(bits_buf.ptr), need),
                      st, args.reps, device)
            record("pack", 0, t, bits_bytes=need)
    os.environ.pop(SWITCH, None)
    os.environ.pop(BITS, None)
    os.environ.pop(LIST, None)
    os.environ.pop(VLIST, None)
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
