"""Time spc_pv_extract_f32 (the kernel behind extract_pv_slice / SpectralCube.pv_slice) on a resident 1024^3 float32 cube
with and without a uint8 mask array (80 % included): a row-aligned path (y = 512, 1024 points on integer pixels) and a 30
degree diagonal of about 1000 points, widths 1 and 5 (1 and 5 lines), orders 0 and 1.  Next to every order-1 case the same
points through the existing bilinear resampler (ops.resample_bilinear fed the (nlines, npts) pixel map, which writes
(nz, nlines, npts) and leaves the mean over the lines undone) timed the same way in the same process; `--resampler-only`
runs those alone and uses nothing this kernel added, so it also runs on a checkout from before it.  One JSON record per
case: median / min / max of the HIP-event times (median of --reps after 2 warm-ups), the algorithmic bytes - the samples
fetched (neighbours of non-zero weight that the mask includes, counted on the host) + their mask bytes + the output - and
their fraction of 8 TB/s.

    python tools/time_pv_extract.py [--n 1024] [--reps 10] [--out profiles/pv_extract_time.jsonl] [--resampler-only]
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from spectral_cube_amd import _lib, ops  # noqa: E402
from spectral_cube_amd.device import DeviceArray, Event, Stream  # noqa: E402

PEAK = 8.0e12


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


def lines_of(p0, p1, npts, nlines, width):
    """(xs, ys) (nlines, npts): the segment p0 -> p1 in npts equal steps, moved by ((l + 0.5) / nlines - 0.5) width along its
    normal (pvextract.Path.sample_lines on one segment)"""
    t = np.arange(npts, dtype=np.float64) / (npts - 1)
    x, y = p0[0] + t * (p1[0] - p0[0]), p0[1] + t * (p1[1] - p0[1])
    d = np.array([p1[0] - p0[0], p1[1] - p0[1]]) / math.hypot(p1[0] - p0[0], p1[1] - p0[1])
    off = ((np.arange(nlines) + 0.5) / nlines - 0.5) * width
    return np.ascontiguousarray(x[None] - off[:, None] * d[1]), np.ascontiguousarray(y[None] + off[:, None] * d[0])


def neighbours(xs, ys, order, shape):
    """[(jy, jx)] flat index arrays of the neighbours of non-zero weight of the points inside the plane"""
    ny, nx = shape
    x, y = xs.ravel(), ys.ravel()
    inside = (x >= 0) & (x <= nx - 1) & (y >= 0) & (y <= ny - 1)
    x, y = x[inside], y[inside]
    if order == 0:
        return [(np.floor(y + 0.5).astype(np.int64), np.floor(x + 0.5).astype(np.int64))]
    x0, y0 = np.floor(x).astype(np.int64), np.floor(y).astype(np.int64)
    fx, fy = x - x0, y - y0
    out = []
    for dy, dx, w in ((0, 0, (1 - fy) * (1 - fx)), (0, 1, (1 - fy) * fx), (1, 0, fy * (1 - fx)), (1, 1, fy * fx)):
        use = w != 0
        out.append((np.minimum(y0 + dy, ny - 1)[use], np.minimum(x0 + dx, nx - 1)[use]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--resampler-only", action="store_true")
    args = ap.parse_args()
    _lib.require_gpu()
    sink = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    n = args.n
    rng = np.random.default_rng(0)
    host = rng.standard_normal((n, n, n), dtype=np.float32)
    cube = DeviceArray.from_numpy(host)
    del host
    keep_host = rng.random((n, n, n), dtype=np.float32) < 0.8
    keep = DeviceArray.from_numpy(keep_host.view(np.uint8))
    spec = ops.MaskSpec(_lib.MASK_ARRAY, 0.0, 0.0, keep)
    st = Stream(0)
    # the diagonal: 30 degrees from the x axis, about n points one pixel apart, centred on the plane
    half = 0.5 * (n - 24)
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    mid = 0.5 * (n - 1)
    paths = {"row": ((0.0, float(n // 2)), (n - 1.0, float(n // 2)), n),
             "diagonal30": ((mid - half * c, mid - half * s), (mid + half * c, mid + half * s), int(2 * half) + 1)}
    for pname, (p0, p1, npts) in paths.items():
        for nlines in (1, 5):
            xs, ys = lines_of(p0, p1, npts, nlines, float(nlines))
            d_xs, d_ys = DeviceArray.from_numpy(xs), DeviceArray.from_numpy(ys)
            out = DeviceArray((n, npts), np.float32, 0)
            for order in (0, 1):
                nb = neighbours(xs, ys, order, (n, n))
                touched = sum(len(jy) for jy, _ in nb) * n
                for label, mask in (("none", None), ("u8", spec)):
                    base = dict(path=pname, npts=npts, nlines=nlines, order=order, dtype="float32", shape=[n, n, n], mask=label)
                    if mask is None:
                        nbytes = touched * 4 + n * npts * 4
                    else:
                        included = sum(int(keep_host[:, jy, jx].sum()) for jy, jx in nb)
                        nbytes = touched * 1 + included * 4 + n * npts * 4
                    if not args.resampler_only:
                        t = timed(lambda: ops.pv_extract(cube, d_xs, d_ys, order=order, mask_spec=mask, out=out, stream=st), st,
                                  args.reps, 0)
                        ms = float(np.median(t))
                        emit(dict(base, kernel="pv_extract", median_ms=round(ms, 4), min_ms=round(min(t), 4), max_ms=round(max(t), 4),
                                  bytes=int(nbytes), tbps=round(nbytes / ms / 1e9, 4),
                                  fraction_of_8tbps=round(nbytes / ms / 1e9 / (PEAK / 1e12), 4)))
                    if order == 1:
                        # the yardstick: every line as a row of a 2-D output map; (nz, nlines, npts) written, no mean over the lines
                        big = DeviceArray((n, nlines, npts), np.float32, 0)
                        t = timed(lambda: ops.resample_bilinear(cube, d_xs, d_ys, mask=mask, out=big, want_footprint=False, stream=st),
                                  st, args.reps, 0)
                        ms = float(np.median(t))
                        rbytes = nbytes - n * npts * 4 + n * nlines * npts * 4
                        emit(dict(base, kernel="resample_bilinear [yardstick: no mean over the lines]", median_ms=round(ms, 4),
                                  min_ms=round(min(t), 4), max_ms=round(max(t), 4), bytes=int(rbytes), tbps=round(rbytes / ms / 1e9, 4),
                                  fraction_of_8tbps=round(rbytes / ms / 1e9 / (PEAK / 1e12), 4)))
                        del big
    if sink:
        sink.close()


if __name__ == "__main__":
    main()
