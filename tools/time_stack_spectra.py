"""Time stack_spectra's kernels (spc_stack_sum_* / spc_stack_shift_*) on the cases of DESIGN.md: a float32 cube of Gaussian
lines with a uint8 mask array, 512 x 1024^2 and 1024^3, every spaxel stacked with the shifts of a smooth velocity field
(+-8 channels, padded).  Per case: the fused stack, and shift-then-reduce (the (M, P) float64 rows written, then read back
by the reduction: timed as the shift alone, the reduction would only add to it), HIP-event medians after two warm-ups; the
float64 FMAs the arithmetic needs (P x M x nz, twice for a spectrum with a non-finite sample) over the time, as a
fraction of 78.6 TFLOP/s (a float64 FMA issues at the unpacked float32 vector rate: half of the 157.3 TFLOP/s packed
float32 vector peak); and the end-to-end stack_spectra(np.nanmean) call.

    python tools/time_stack_spectra.py [--reps 5] [--out profiles/stack_spectra_time.jsonl] [--small]

With the reference environment (CPU), the reference's own time on the same kind of cube cut to 512 x 64 x 64:

    /opt/conda/bin/python3.9 -B tools/time_stack_spectra.py --reference [--out FILE]   (appends)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = {"CTYPE1": "RA---TAN", "CTYPE2": "DEC--TAN", "CTYPE3": "VRAD", "CUNIT1": "deg", "CUNIT2": "deg", "CUNIT3": "km/s",
       "CDELT1": -1e-3, "CDELT2": 1e-3, "CDELT3": 0.5, "CRPIX1": 1.0, "CRPIX2": 1.0, "CRPIX3": 1.0, "CRVAL1": 10.0, "CRVAL2": 20.0,
       "CRVAL3": 0.0, "BUNIT": "K"}
F64_PEAK_TFLOPS = 78.6


def make(nz, ny, nx, seed=0):
    """(data, keep, velocity in km/s): lines whose centre follows a smooth field, 1 spectrum in 16 with a NaN"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:ny, 0:nx]
    cen = nz / 2.0 + 8.0 * np.sin(yy / max(ny, 1) * 3.0) * np.cos(xx / max(nx, 1) * 2.0)
    d = np.empty((nz, ny, nx), np.float32)
    for z in range(nz):
        d[z] = np.exp(-0.5 * ((z - cen) / 3.0) ** 2)
    d += 0.05 * rng.standard_normal(d.shape, dtype=np.float32)
    bad = rng.random((ny, nx)) < 1.0 / 16
    d[nz // 3][bad] = np.nan
    keep = rng.random(d.shape, dtype=np.float32) < 0.9
    return d, keep, 0.5 * cen


def emit(rec, sink):
    line = json.dumps(rec)
    print(line, flush=True)
    if sink is not None:
        sink.write(line + "\n")
        sink.flush()


def reference(sink):
    sys.path.insert(0, os.path.join(REPO, "oracle", "ref_env"))
    from bootstrap import load_reference
    load_reference()
    import warnings
    warnings.simplefilter("ignore")
    from astropy import units as u
    from astropy.wcs import WCS
    import spectral_cube.base_class as B
    from spectral_cube import SpectralCube, BooleanArrayMask
    B.BeamMixinClass.beam = property(lambda self: None, lambda self, v: None)
    from spectral_cube.analysis_utilities import stack_spectra
    d, keep, vel = make(512, 64, 64)
    w = WCS(HDR)
    cube = SpectralCube(d * u.K, wcs=w, mask=BooleanArrayMask(keep, wcs=w))
    t0 = time.perf_counter()
    stack_spectra(cube, vel * u.km / u.s)
    dt = time.perf_counter() - t0
    emit(dict(op="reference stack_spectra(nanmean)", shape=[512, 64, 64], seconds=round(dt, 3), us_per_spaxel=round(dt / 4096 * 1e6, 1),
              extrapolated_s_1024x1024=round(dt / 4096 * 1024 * 1024, 1), where="host CPU, reference interpreter"), sink)


def timed(fn, st, reps):
    from spectral_cube_amd.device import Event
    for _ in range(2):
        fn()
    times = []
    for _ in range(reps):
        a, b = Event(st.device), Event(st.device)
        a.record(st)
        fn()
        b.record(st)
        b.synchronize()
        times.append(a.elapsed_ms(b))
    return float(np.median(times)), float(np.min(times))


def device(shape, reps, sink):
    import ctypes as C
    from spectral_cube_amd import SpectralCube, _lib, ops, stack_spectra
    from spectral_cube_amd.analysis_utilities import stack_plan
    from spectral_cube_amd.device import DeviceArray, Stream
    nz, ny, nx = shape
    d, keep, vel = make(nz, ny, nx)
    cube = SpectralCube(d, header=HDR).with_mask(keep)
    idx, shifts, pad = stack_plan(cube, vel)
    M, P = nz + pad[0] + pad[1], idx.size
    filled_bad = ~np.isfinite(np.where(keep, d, np.float32(np.nan)))
    with_nan = int(filled_bad.any(axis=0).sum())
    fma = float(M) * nz * (P + with_nan)
    data, mask, _ = cube._operand()
    st = Stream(0)
    lib = _lib.load()
    c, m = ops._cube_c(data), ops._mask_c(mask, data)
    d_idx, d_shift = DeviceArray.from_numpy(idx.astype(np.int32)), DeviceArray.from_numpy(shifts)
    ws = DeviceArray((int(lib.spc_stack_workspace_bytes(nz, P, pad[0], pad[1], 1)),), np.uint8)
    total, count, nnan = DeviceArray((M,), np.float64), DeviceArray((M,), np.int64), DeviceArray((M,), np.int64)
    rows = DeviceArray((M, P), np.float64)

    def fused():
        _lib.call("spc_stack_sum_f32", 0, st.handle, C.byref(c), C.byref(m), 0, float("nan"), C.c_void_p(d_idx.ptr), C.c_void_p(d_shift.ptr),
                  P, pad[0], pad[1], C.c_void_p(total.ptr), C.c_void_p(count.ptr), C.c_void_p(nnan.ptr), C.c_void_p(ws.ptr), ws.nbytes)

    def shift():
        _lib.call("spc_stack_shift_f32", 0, st.handle, C.byref(c), C.byref(m), 0, float("nan"), C.c_void_p(d_idx.ptr), C.c_void_p(d_shift.ptr),
                  P, pad[0], pad[1], C.c_void_p(rows.ptr), C.c_void_p(ws.ptr), ws.nbytes)
    for name, fn in (("fused stack (spc_stack_sum_f32)", fused), ("shift alone (spc_stack_shift_f32), rows still to be reduced", shift)):
        ms, lo = timed(fn, st, reps)
        emit(dict(op=name, shape=list(shape), mask="u8", M=M, P=P, spectra_with_nan=with_nan, median_ms=round(ms, 3), min_ms=round(lo, 3),
                  f64_fma=fma, tflops=round(2 * fma / ms / 1e9, 2), fraction_of_f64_vector_peak=round(2 * fma / ms / 1e9 / F64_PEAK_TFLOPS, 3),
                  rows_bytes=8 * M * P if fn is shift else 0, measured=True), sink)
    rows.free()
    t0 = time.perf_counter()
    s = stack_spectra(cube, vel)
    dt = time.perf_counter() - t0
    emit(dict(op="stack_spectra(np.nanmean), end to end on a resident cube", shape=list(shape), M=M, P=P, seconds=round(dt, 4),
              peak_channel=int(np.nanargmax(s)), measured=True), sink)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true", help="512 x 256 x 256 only (a quick check of the tool)")
    ap.add_argument("--reference", action="store_true")
    args = ap.parse_args()
    sink = open(args.out, "a" if args.reference else "w") if args.out else None
    if args.reference:
        reference(sink)
    else:
        from spectral_cube_amd import _lib
        _lib.require_gpu()
        for shape in (((512, 256, 256),) if args.small else ((512, 1024, 1024), (1024, 1024, 1024))):
            device(shape, args.reps, sink)
    if sink is not None:
        sink.close()


if __name__ == "__main__":
    main()
