#!/usr/bin/env python
"""BatchPlan.stack_clip_batch against the reductions the library already had and against what it offered for the same result
(DESIGN.md section 7 row 18).

    python tools/bench_stack_clip.py [--cases 64x512 64x2048 16x4096] [--reps 20]

Frames are device-resident float32 noise (uniform in [0, 1)), frame s moved by (s % 7 - 3, 2 - s % 5) pixels (shift-only maps),
the output has the frames' shape: tools/bench_stack.py's stacks.  Per case, after a warm-up of every form, the forms alternate
in one process:
    clip      stack_clip_batch(frames, M, off, fills, reject=..., out="device")   trim (0, 1), trim (2, 2), sigma (3, 3) iters=3
    mean      stack_batch(reduce="mean", out="device")
    median    stack_batch(reduce="median", out="device")
    torch     transform_batch(frames, M, off, fills, out="device") followed by, for a trim, torch.sort(dim=0), a slice and mean(dim=0),
              and for sigma a masked clip: three passes of mean / variance over a mask, the comparison, and the masked mean
with the hipEvent time of the launch (last_stack_ms; the torch form: last_transform_ms, the warp alone) and a host clock around
each form, the device synchronised before the clock stops.  The torch forms ignore coverage (the fill takes part near the
edges): they are a cost yardstick, not a bitwise one.  Uniform noise holds no 3-sigma sample, so the sigma rule stops after its
first pass; --zingers plants one outlier per pixel, which makes most waves run a second pass.
Prints one JSON line; times are median [min, max] in ms over the repetitions.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CLIPS = {"trim0_1": dict(reject="trim", trim=(0, 1)), "trim2_2": dict(reject="trim", trim=(2, 2)),
         "sigma3": dict(reject="sigma", kappa=(3.0, 3.0), iters=3)}


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def torch_trim(planes, lo, hi):
    return planes.sort(dim=0).values[lo:planes.shape[0] - hi].mean(dim=0)


def torch_sigma(planes, kl, kh, iters):
    import torch
    keep = torch.ones_like(planes, dtype=torch.bool)
    for _ in range(iters):
        n = keep.sum(dim=0).to(planes.dtype)
        m = (planes * keep).sum(dim=0) / n
        d = planes - m
        var = (d * d * keep).sum(dim=0) / n
        keep = keep & ~(((d < 0) & (d * d > kl * kl * var)) | ((d > 0) & (d * d > kh * kh * var)))
    return (planes * keep).sum(dim=0) / keep.sum(dim=0).to(planes.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["64x512", "64x2048", "16x4096"], help="SxN: frames x side")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--zingers", action="store_true", help="plant one outlier of 100 per output pixel")
    args = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    out = {"reps": args.reps, "zingers": bool(args.zingers), "cases": {}}
    for case in args.cases:
        S, N = (int(v) for v in case.split("x"))
        torch.manual_seed(0)
        stack = torch.rand((S, N, N), dtype=torch.float32, device="cuda")
        if args.zingers:
            which = torch.randint(0, S, (1, N, N), device="cuda")
            stack.scatter_(0, which, 100.0)
            del which
        frames = [stack[s] for s in range(S)]
        M = np.tile(np.array([1, 0, 0, 1], np.float32), (S, 1))
        off = np.array([[s % 7 - 3, 2 - s % 5] for s in range(S)], np.float32)
        fills = np.zeros(S, np.float32)
        bp = sp.BatchPlan(shape=(N, N), dtype=np.float32, lanes=1)

        def clock(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            return r, 1e3 * (time.perf_counter() - t0)

        def warped():
            return bp.transform_batch(frames, M, off, fills, out="device")

        forms = {name: (lambda p=p: bp.stack_clip_batch(frames, M, off, fills, out="device", **p)) for name, p in CLIPS.items()}
        forms["mean"] = lambda: bp.stack_batch(frames, M, off, fills, reduce="mean", out="device")
        forms["median"] = lambda: bp.stack_batch(frames, M, off, fills, reduce="median", out="device")
        forms["torch_trim0_1"] = lambda: torch_trim(warped(), 0, 1)
        forms["torch_trim2_2"] = lambda: torch_trim(warped(), 2, 2)
        forms["torch_sigma3"] = lambda: torch_sigma(warped(), 3.0, 3.0, 3)
        for fn in forms.values():                                # warm-up of every form at this shape
            fn(); fn()
        wall = {k: [] for k in forms}
        kernel = {k: [] for k in forms}
        for _ in range(args.reps):
            for name, fn in forms.items():
                _, ms = clock(fn)
                wall[name].append(ms)
                kernel[name].append(bp.last_transform_ms if name.startswith("torch") else bp.last_stack_ms)
        res = {}
        for name in forms:
            res[name] = {"kernel_ms": stats(kernel[name]), "wall_ms": stats(wall[name])}
            if not name.startswith("torch"):
                res[name]["kernel_GBps"] = round((S * N * N + N * N) * 4 / 1e9 / (float(np.median(kernel[name])) / 1e3), 1)
        for name in CLIPS:
            res[name]["kernel_over_mean_kernel"] = round(float(np.median(kernel[name]) / np.median(kernel["mean"])), 3)
            res[name]["kernel_over_median_kernel"] = round(float(np.median(kernel[name]) / np.median(kernel["median"])), 3)
            res[name]["torch_wall_over_wall"] = round(float(np.median(wall["torch_" + name]) / np.median(wall[name])), 3)
        out["cases"]["S=%d %dx%d" % (S, N, N)] = res
        print("S=%d %dx%d: %s" % (S, N, N, json.dumps(res)), file=sys.stderr, flush=True)
        del bp, frames, stack, forms
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
