"""Time stack_cube's kernel (spc_stack_cube_f32) against the composition it replaces, on the case of DESIGN.md section 3.6f:
a 1024^3 float32 frequency cube with a uint8 mask array, 8 lines, slabs of about 64 channels.

Fused: one ops.stack_cube call.  Composition: per line the subcube gather of its slab (ops.subcube, data + include) and,
for every line but the first, ops.spectral_lerp of that cutout onto the grid - the device work of the general route; the
average over the L cutouts on the host is not timed and would only add to it.  HIP-event medians of --steps runs after two
warm-ups; the algorithmic bytes (every slab once, data + mask bytes, plus the output once) over the fused time as a
fraction of 8 TB/s.

    python tools/time_stack_cube.py [--steps 20] [--out profiles/stack_cube_1024.txt] [--small]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "FREQ", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "Hz",
       "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5e6, "CRPIX1": 1.0, "CRPIX2": 1.0, "CRPIX3": 1.0, "CRVAL1": 10.0, "CRVAL2": 20.0,
       "CRVAL3": 100.0e9, "BUNIT": "K"}
HBM_TBS = 8.0
C_KMS = 299792.458


def timed(fn, st, steps):
    from spectral_cube_amd.device import Event
    for _ in range(2):
        fn()
    times = []
    for _ in range(steps):
        a, b = Event(st.device), Event(st.device)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_ms(b))
    return float(np.median(times)), float(np.min(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="1024 x 256 x 256 (a quick check of the tool)")
    args = ap.parse_args()
    from spectral_cube_amd import SpectralCube, _lib, ops
    from spectral_cube_amd.analysis_utilities import stack_cube_plan
    from spectral_cube_amd.device import Stream
    _lib.require_gpu()
    nz, ny, nx = (1024, 256, 256) if args.small else (1024, 1024, 1024)
    rng = np.random.default_rng(0)
    d = rng.standard_normal((nz, ny, nx), dtype=np.float32)
    keep = rng.random((nz, ny, nx), dtype=np.float32) < 0.9
    cube = SpectralCube(d, header=HDR).with_mask(keep)
    freq = HDR["CRVAL3"] + HDR["CDELT3"] * np.arange(nz)
    lines = [freq[60 + 120 * k] + 0.17e6 * (k + 1) for k in range(8)]
    half = 32 * C_KMS * HDR["CDELT3"] / HDR["CRVAL3"]               # +-32 channels in km/s
    P = stack_cube_plan(cube, lines, -half, half)
    nsrc, n0 = P.lo.shape
    data, mask, _ = cube._operand()
    st = Stream(0)
    out = ops.stack_cube(data, P.lo, P.t, P.inv_dx, P.exact, "nanmean", mask=mask, stream=st)

    def fused():
        ops.stack_cube(data, P.lo, P.t, P.inv_dx, P.exact, "nanmean", mask=mask, out=out, stream=st)

    cuts = [ops.subcube(data, (ilo, 0, 0), (1, 1, 1), (ihi - ilo + 1, ny, nx), mask=mask, stream=st) for ilo, ihi in P.windows]
    rel = [np.where(P.lo[s] >= 0, P.lo[s] - P.windows[s][0], -1).astype(np.int32) for s in range(nsrc)]
    lerped = [None] + [ops.spectral_lerp(cuts[s][0], rel[s], P.t[s], P.inv_dx[s], mask=ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, cuts[s][1]),
                                         stream=st) for s in range(1, nsrc)]

    def composed():
        for s, (ilo, ihi) in enumerate(P.windows):
            ops.subcube(data, (ilo, 0, 0), (1, 1, 1), (ihi - ilo + 1, ny, nx), mask=mask, out=cuts[s][0], out_mask=cuts[s][1], stream=st)
            if s:
                ops.spectral_lerp(cuts[s][0], rel[s], P.t[s], P.inv_dx[s], mask=ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, cuts[s][1]),
                                  out=lerped[s], stream=st)

    slab_channels = sum(ihi - ilo + 1 for ilo, ihi in P.windows)
    nbytes = slab_channels * ny * nx * 5 + n0 * ny * nx * 4
    sink = open(args.out, "w") if args.out else None
    for name, fn in (("fused (spc_stack_cube_f32)", fused), ("composition: gather + spectral_lerp per line", composed)):
        ms, lo = timed(fn, st, args.steps)
        rec = dict(op=name, shape=[nz, ny, nx], mask="u8", lines=nsrc, n0=n0, slab_channels=slab_channels, steps=args.steps,
                   median_ms=round(ms, 3), min_ms=round(lo, 3), measured=True)
        if fn is fused:
            rec.update(algorithmic_bytes=nbytes, tb_per_s=round(nbytes / ms / 1e9, 3), fraction_of_hbm_peak=round(nbytes / ms / 1e9 / HBM_TBS, 3))
        line = json.dumps(rec)
        print(line, flush=True)
        if sink is not None:
            sink.write(line + "\n")
    if sink is not None:
        sink.close()


if __name__ == "__main__":
    main()
