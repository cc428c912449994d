"""Which aligned x-segments of the headline cube hold a voxel that the benchmark's uint8 mask includes (CPU only).

    python tools/needed_lines.py [--nz 4096] [--tile FILE]

Builds the (nz, 16, 2048) tile that bench.py repeats along y (synth.gaussian_line_cube + synth.boolean_mask, seed C4) and
prints, per segment size of the float32 cube, the share of aligned segments with at least one included voxel: what a
moment kernel that reads the mask first still has to fetch at that granularity.  --tile writes the mask tile as raw bytes
(the input of `tools/micro/mask_patterns pred`)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from spectral_cube_amd import synth  # noqa: E402

SEGMENTS = (16, 32, 64, 128, 256, 1024)      # bytes of the float32 cube


def bench_mask_tile(nz, rows=16, nx=2048):
    tile = synth.gaussian_line_cube((nz, rows, nx), synth.SEEDS["C4"], chunk_rows=rows)
    return synth.boolean_mask(tile, synth.SEEDS["C4"])


def needed(mask):
    """{segment bytes: share of the aligned segments along x that hold an included voxel}"""
    nz, ny, nx = mask.shape
    out = {}
    for seg in SEGMENTS:
        vox = seg // 4
        assert nx % vox == 0
        out[seg] = float(mask.reshape(nz, ny, nx // vox, vox).any(axis=3).mean())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nz", type=int, default=4096)
    ap.add_argument("--tile", default=None, help="write the uint8 mask tile (nz, 16, 2048) to this file")
    args = ap.parse_args()
    m = bench_mask_tile(args.nz)
    if args.tile:
        m.tofile(args.tile)
    frac = needed(m)
    print("bench mask tile (%d, 16, 2048), seed C4: valid fraction %.4f" % (args.nz, np.count_nonzero(m) / m.size))
    print("| segment | " + " | ".join("%d B" % s if s < 1024 else "1 KiB" for s in SEGMENTS) + " |")
    print("|---|" + "---|" * len(SEGMENTS))
    print("| needed | " + " | ".join("%.4f" % frac[s] for s in SEGMENTS) + " |")
    print("bytes per voxel with the cube fetched per segment (mask 1 + 4 x needed): " +
          ", ".join("%s %.2f" % ("%d B" % s if s < 1024 else "1 KiB", 1 + 4 * frac[s]) for s in SEGMENTS))


if __name__ == "__main__":
    main()
