#!/usr/bin/env python
"""StackAccumulator.add against the mean launch of stack_batch, and the two-pass sigma clip against stack_clip_batch (DESIGN.md
section 7 row 20).

    python tools/bench_stack_accum.py [--cases 64x512 64x2048 16x4096] [--reps 20] [--long 512x2048]

Frames are device-resident float32 noise (uniform in [0, 1)), frame s moved by (s % 7 - 3, 2 - s % 5) pixels (shift-only maps),
the output has the frames' shape: tools/bench_stack.py's stacks.  Per case and sampler (bilinear, cubic), after a warm-up of
every form, the forms alternate in one process; the time is the hipEvent time of the launch (last_stack_ms):
    mean      stack_batch(reduce="mean", out="device")
    plain     accumulator.add(frames, ...)                              without second moments
    moments   accumulator.add(frames, ...)                              with them
    clip      accumulator.add(frames, ..., clip=(mean, var))            without moments, the planes of a first pass
    result    accumulator.result(var=True, out="device")                (wall clock: the call has no kernel time of its own to report)
    clip64    stack_clip_batch(reject="sigma", kappa=(3, 3), iters=1)   S <= 64 only: one launch, one pass of the sigma rule
    two_pass  add with moments + result(var=True) + add with clip       the same rule for a stack of any length, three launches
--long SxN: S frames in chunks of 64 against S / 64 mean launches (the chunk is the same 64 frames every time: 64 x 2048^2 is 1 GiB,
four times the last-level cache, so a chunk leaves nothing behind for the next).
Beside every ratio stands the byte model's: (4 S + 32) / (4 S + 4) plain, (4 S + 48) / (4 S + 4) with moments, 8 more bytes with a clip.
Prints one JSON line; times are median [min, max] in ms over the repetitions.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(np.min(v)), 4), "max": round(float(np.max(v)), 4)}


def model(S, extra):
    return round((4.0 * S + extra) / (4.0 * S + 4.0), 3)


def stack_of(S, N):
    import torch
    torch.manual_seed(0)
    stack = torch.rand((S, N, N), dtype=torch.float32, device="cuda")
    M = np.tile(np.array([1, 0, 0, 1], np.float32), (S, 1))
    off = np.array([[s % 7 - 3, 2 - s % 5] for s in range(S)], np.float32)
    return stack, [stack[s] for s in range(S)], M, off, np.zeros(S, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["64x512", "64x2048", "16x4096"], help="SxN: frames x side")
    ap.add_argument("--long", default="512x2048", help="SxN fed in chunks of 64; '' to skip")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    out = {"reps": args.reps, "cases": {}}

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    for case in args.cases:
        S, N = (int(v) for v in case.split("x"))
        stack, frames, M, off, fills = stack_of(S, N)
        bp = sp.BatchPlan(shape=(N, N), dtype=np.float32, lanes=1)
        res = {}
        for interp in (None, "cubic"):
            first = bp.stack_accumulator(moments=True).add(frames, M, off, fills, interp=interp)
            center, var = first.result(var=True, out="device")
            plain, moments, clip = bp.stack_accumulator(), bp.stack_accumulator(moments=True), bp.stack_accumulator()
            forms = {"mean": lambda: bp.stack_batch(frames, M, off, fills, reduce="mean", out="device", interp=interp),
                     "plain": lambda: plain.add(frames, M, off, fills, interp=interp),
                     "moments": lambda: moments.add(frames, M, off, fills, interp=interp),
                     "clip": lambda: clip.add(frames, M, off, fills, interp=interp, clip=(center, var))}
            if S <= 64:
                forms["clip64"] = lambda: bp.stack_clip_batch(frames, M, off, fills, reject="sigma", kappa=(3.0, 3.0), iters=1, out="device",
                                                              interp=interp)
            for fn in forms.values():
                fn(); fn()
            kernel = {k: [] for k in forms}
            walls = {"result": [], "two_pass": [], "clip64": []}
            for _ in range(args.reps):
                for name, fn in forms.items():
                    fn()
                    kernel[name].append(bp.last_stack_ms)
                walls["result"].append(wall(lambda: first.result(var=True, out="device")))

                def two_pass():
                    a = bp.stack_accumulator(moments=True).add(frames, M, off, fills, interp=interp)
                    bp.stack_accumulator().add(frames, M, off, fills, interp=interp, clip=a.result(var=True, out="device")).result(out="device")
                walls["two_pass"].append(wall(two_pass))
                if S <= 64:
                    walls["clip64"].append(wall(forms["clip64"]))
            r = {name: {"kernel_ms": stats(kernel[name])} for name in forms}
            mean_ms = float(np.median(kernel["mean"]))
            for name, extra in (("plain", 32), ("moments", 48), ("clip", 40)):
                r[name]["over_mean"] = round(float(np.median(kernel[name])) / mean_ms, 3)
                r[name]["model"] = model(S, extra)
            r["result_wall_ms"] = stats(walls["result"])
            r["two_pass_wall_ms"] = stats(walls["two_pass"])
            r["two_pass_kernels_ms"] = round(float(np.median(kernel["moments"]) + np.median(kernel["clip"])), 4)
            if S <= 64:
                r["clip64_wall_ms"] = stats(walls["clip64"])
                r["two_pass_kernels_over_clip64_kernel"] = round(r["two_pass_kernels_ms"] / float(np.median(kernel["clip64"])), 3)
            res[interp or "bilinear"] = r
            del first, center, var, plain, moments, clip, forms
        out["cases"]["S=%d %dx%d" % (S, N, N)] = res
        print("S=%d %dx%d: %s" % (S, N, N, json.dumps(res)), file=sys.stderr, flush=True)
        del bp, frames, stack
        torch.cuda.empty_cache()
    if args.long:
        S, N = (int(v) for v in args.long.split("x"))
        calls = (S + 63) // 64
        stack, frames, M, off, fills = stack_of(64, N)
        bp = sp.BatchPlan(shape=(N, N), dtype=np.float32, lanes=1)
        res = {}
        for interp in (None, "cubic"):
            acc_ms, mean_ms = [], []
            for rep in range(max(2, args.reps // 4) + 1):
                acc = bp.stack_accumulator(moments=True)
                a = m = 0.0
                for _ in range(calls):
                    acc.add(frames, M, off, fills, interp=interp)
                    a += acc.last_stack_ms
                for _ in range(calls):
                    bp.stack_batch(frames, M, off, fills, reduce="mean", out="device", interp=interp)
                    m += bp.last_stack_ms
                if rep:                                              # the first round is the warm-up
                    acc_ms.append(a); mean_ms.append(m)
            res[interp or "bilinear"] = {"calls": calls, "accumulate_moments_kernels_ms": stats(acc_ms), "mean_kernels_ms": stats(mean_ms),
                                         "over_mean": round(float(np.median(acc_ms) / np.median(mean_ms)), 3), "model": model(64, 48)}
        out["long"] = {"S=%d %dx%d in chunks of 64" % (S, N, N): res}
        print("long: %s" % json.dumps(res), file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
