#!/usr/bin/env python
"""The cubic sampler against the bilinear launch of the same call.

    python tools/bench_warp_interp.py [--cases 64x512 64x2048 16x4096] [--maps subpixel rot30] [--reps 10]

Frames are device-resident float32 noise (uniform in [0, 1)) and the output has the frames' shape.  Two sets of maps:
    subpixel  a 0.5 degree rotation about the centre with a shift of (s % 7 - 3 + 0.37, 2 - s % 5 + 0.61) pixels for frame s:
              what LinearAlign produces for a drifting stack; the taps of a wave fall in a few image rows
    rot30     a 30 degree rotation about the centre with the same shifts: poor gather locality, every wave crosses ~32 rows
Per size and map set, after a warm-up of every form, cubic and bilinear alternate in one process:
    transform     transform_batch(frames, M, off, fills, out="device")
    mean, median  stack_batch(reduce=..., out="device")
    sigma         stack_clip_batch(reject="sigma", kappa=(3, 3), iters=3, out="device")
each with interp="linear" and interp="cubic".  Reported per form: the hipEvent time of the launch in ms (median [min, max] over
the repetitions), the effective rate at 8 bytes per output pixel per frame (one gathered read and, for the warp, one write -- the
bilinear kernel's own traffic model), and cubic / bilinear of the medians.  Needs a device: there is no fallback.
Prints one JSON line.
"""
import argparse
import json
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def maps_of(kind, S, N):
    deg = {"subpixel": 0.5, "rot30": 30.0}[kind]
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    cy = cx = (N - 1) / 2.0
    M = np.tile(np.array([c, -s, s, c], np.float32), (S, 1))
    off = np.array([[cy - c * cy + s * cx + (k % 7 - 3 + 0.37), cx - s * cy - c * cx + (2 - k % 5 + 0.61)] for k in range(S)], np.float32)
    return M, off


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["64x512", "64x2048", "16x4096"], help="SxN: frames x side")
    ap.add_argument("--maps", nargs="+", default=["subpixel", "rot30"], choices=["subpixel", "rot30"])
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_warp_interp: no device; this tool measures kernels and has no fallback")
    import sift_pyocl_amd as sp
    out = {"reps": args.reps, "bytes_per_pixel_per_frame": 8, "cases": {}}
    for case in args.cases:
        S, N = (int(v) for v in case.split("x"))
        torch.manual_seed(0)
        stack = torch.rand((S, N, N), dtype=torch.float32, device="cuda")
        frames = [stack[s] for s in range(S)]
        fills = np.zeros(S, np.float32)
        bp = sp.BatchPlan(shape=(N, N), dtype=np.float32, lanes=1)
        for kind in args.maps:
            M, off = maps_of(kind, S, N)
            forms = {}
            for interp in ("linear", "cubic"):
                forms["transform", interp] = lambda i=interp: (bp.transform_batch(frames, M, off, fills, out="device", interp=i), bp.last_transform_ms)[1]
                forms["mean", interp] = lambda i=interp: (bp.stack_batch(frames, M, off, fills, reduce="mean", out="device", interp=i), bp.last_stack_ms)[1]
                forms["median", interp] = lambda i=interp: (bp.stack_batch(frames, M, off, fills, reduce="median", out="device", interp=i), bp.last_stack_ms)[1]
                forms["sigma", interp] = lambda i=interp: (bp.stack_clip_batch(frames, M, off, fills, reject="sigma", kappa=(3.0, 3.0), iters=3,
                                                                               out="device", interp=i), bp.last_stack_ms)[1]
            for fn in forms.values():                                # warm-up of every form at this shape
                fn(); fn()
            torch.cuda.synchronize()
            kernel = {k: [] for k in forms}
            for _ in range(args.reps):
                for key, fn in forms.items():                        # linear and cubic of every call alternate
                    kernel[key].append(fn())
            res = {}
            for name in ("transform", "mean", "median", "sigma"):
                lin, cub = kernel[name, "linear"], kernel[name, "cubic"]
                rate = lambda v: round(S * N * N * 8 / 1e9 / (float(np.median(v)) / 1e3), 1)      # noqa: E731
                res[name] = {"linear_kernel_ms": stats(lin), "cubic_kernel_ms": stats(cub), "linear_GBps": rate(lin), "cubic_GBps": rate(cub),
                             "cubic_over_linear": round(float(np.median(cub) / np.median(lin)), 3)}
            out["cases"]["S=%d %dx%d %s" % (S, N, N, kind)] = res
            print("S=%d %dx%d %s: %s" % (S, N, N, kind, json.dumps(res)), file=sys.stderr, flush=True)
        del bp, frames, stack, forms
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
