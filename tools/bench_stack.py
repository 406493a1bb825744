#!/usr/bin/env python
"""BatchPlan.stack_batch against what the library offered before it.

    python tools/bench_stack.py [--cases 64x512 64x2048 16x4096] [--reps 20]

Frames are device-resident float32 noise, frame s moved by (s % 7 - 3, 2 - s % 5) pixels (shift-only maps), the output has the
frames' shape.  Per case, after a warm-up of every form, the forms alternate in one process:
    stack     stack_batch(frames, M, off, fills, reduce=r, out="device")                    r = mean, median (and sum)
    baseline  transform_batch(frames, M, off, fills, out="device") followed by torch.mean(dim=0) / torch.median(dim=0)
    host      (64 x 512 x 512 only) transform_batch(out="host") followed by numpy.mean / numpy.median
with the hipEvent time of the launch (last_stack_ms, last_transform_ms) and a host clock around each form, the device
synchronised before the clock stops.  The stack kernel's bytes per second are (S * H * W + OH * OW) * 4 / kernel_ms.
The median's selection cost depends on the order of a pixel's values, so its kernel is also timed on frames whose values rise
(every key goes behind the ones kept: the selection costs next to nothing) and fall (every key moves all kept ones) with s.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["64x512", "64x2048", "16x4096"], help="SxN: frames x side")
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    out = {"reps": args.reps, "cases": {}}
    for case in args.cases:
        S, N = (int(v) for v in case.split("x"))
        torch.manual_seed(0)
        stack = torch.rand((S, N, N), dtype=torch.float32, device="cuda")
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

        def stacked(reduce, fr=frames):
            return lambda: bp.stack_batch(fr, M, off, fills, reduce=reduce, out="device")

        def baseline(reduce):
            def run():
                planes = bp.transform_batch(frames, M, off, fills, out="device")
                return planes.mean(dim=0) if reduce == "mean" else (planes.sum(dim=0) if reduce == "sum" else planes.median(dim=0).values)
            return run

        def host(reduce):
            def run():
                planes = bp.transform_batch(frames, M, off, fills, out="host")
                return np.mean(planes, axis=0) if reduce == "mean" else np.median(planes, axis=0)
            return run

        res = {}
        with_host = S * N * N <= 64 * 512 * 512
        for reduce in ("mean", "median", "sum"):
            forms = {"stack": stacked(reduce), "baseline": baseline(reduce)}
            if with_host and reduce != "sum":
                forms["host"] = host(reduce)
            for fn in forms.values():                            # warm-up of every form at this shape
                fn(); fn()
            t = {k: [] for k in forms}
            k_stack, k_warp = [], []
            for _ in range(args.reps):
                for name, fn in forms.items():
                    _, ms = clock(fn)
                    t[name].append(ms)
                    if name == "stack":
                        k_stack.append(bp.last_stack_ms)
                    elif name == "baseline":
                        k_warp.append(bp.last_transform_ms)
            r = {name + "_wall_ms": stats(v) for name, v in t.items()}
            r["stack_kernel_ms"] = stats(k_stack)
            r["transform_batch_kernel_ms"] = stats(k_warp)
            r["stack_kernel_GBps"] = round((S * N * N + N * N) * 4 / 1e9 / (float(np.median(k_stack)) / 1e3), 1)
            r["transform_batch_kernel_GBps"] = round(8.0 * S * N * N / 1e9 / (float(np.median(k_warp)) / 1e3), 1)
            r["stack_kernel_over_transform_kernel"] = round(float(np.median(k_stack) / np.median(k_warp)), 3)
            r["baseline_over_stack_wall"] = round(float(np.median(t["baseline"]) / np.median(t["stack"])), 3)
            res[reduce] = r
        if S <= 64:
            ramp = torch.arange(S, dtype=torch.float32, device="cuda").reshape(S, 1, 1)
            order = {}
            for name, sign in (("rising", 1.0), ("falling", -1.0)):
                moved = stack + sign * ramp
                fr = [moved[s] for s in range(S)]
                fn = stacked("median", fr)
                fn(); fn()
                ks = []
                for _ in range(args.reps):
                    fn()
                    ks.append(bp.last_stack_ms)
                order[name] = stats(ks)
                del moved, fr
            res["median_kernel_ms_by_value_order"] = order
        out["cases"]["S=%d %dx%d" % (S, N, N)] = res
        print("S=%d %dx%d: %s" % (S, N, N, json.dumps(res)), file=sys.stderr, flush=True)
        del bp, frames, stack
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
