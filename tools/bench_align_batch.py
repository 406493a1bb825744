#!/usr/bin/env python
"""LinearAlign.align_batch against the loop of LinearAlign.align calls it replaces.

    python tools/bench_align_batch.py [--cases 64x512 64x1024 64x2048 16x4096] [--reps 5]

Frames are crops of one smoothed plane, as in tools/bench_align.py: frame s is the reference crop moved by (s % 7 - 3, 2 - s % 5)
pixels.  Host frames in, host result out on both sides.  Per case, after a warm-up of every form, the forms alternate in one
process with a host clock around each:
    loop    [align(f, estimate="device", median="device", **kw) for f in frames]
    batch   align_batch(frames, **kw)
for kw = shift_only, affine (the default) and robust; then the warp alone,
    loop    [transform(M_s, off_s, image=f_s, fill=fill_s) for s]         (siftmi_plan_transform per frame)
    batch   BatchPlan.transform_batch(frames, M, off, fills)
with the hipEvent time of the kernels (the batch kernel's bytes per second from 8 B / pixel), and the wall time of every stage of
one align_batch (the same public calls, replayed with a clock around each).  The loop is code this row does not touch.
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
    return {"median": round(float(np.median(v)), 3), "min": round(float(np.min(v)), 3), "max": round(float(np.max(v)), 3)}


def clock(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, 1e3 * (time.perf_counter() - t0)


def stage_times(la, frames):
    """wall time of every stage of one align_batch (affine form), by replaying its public calls"""
    import torch
    t = {}
    bp = la._batch_plan()
    dev, t["upload"] = clock(lambda: (la._device_frames(frames), torch.cuda.synchronize())[0])
    (counts, records), t["keypoints_batch_device"] = clock(lambda: bp.keypoints_batch_device(dev))
    fills, t["minmax_batch"] = clock(lambda: bp.minmax_batch()[0])
    ref = la._ref_dev if la._ref_dev is not None else la.ref_kp
    (pairs, pc), t["match_batch"] = clock(lambda: la.match.match_batch(ref, None, records, counts, out="device"))
    (models, rms, n), t["fit_batch"] = clock(lambda: la.match.fit_batch(ref, None, records, counts, pairs, pc))
    _, t["shift_batch"] = clock(lambda: la.match.shift_batch(ref, None, records, counts, pairs, pc))
    _, t["consensus_batch"] = clock(lambda: la.match.consensus_batch(ref, None, records, counts, pairs, pc, out="device"))
    a, b, c, d, e, f = (models[:, k] for k in range(6))
    M = np.stack([e, d, b, a], axis=1).astype(np.float32)
    off = np.stack([f, c], axis=1).astype(np.float32)
    _, t["transform_batch"] = clock(lambda: bp.transform_batch(dev, M, off, fills, out_shape=la.outshape))
    return {k: round(v, 3) for k, v in t.items()}, M, off, fills


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["64x512", "64x1024", "64x2048", "16x4096"], help="SxN: frames x side")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import sift_pyocl_amd as sp
    from scipy.ndimage import gaussian_filter
    out = {"reps": args.reps, "cases": {}}
    for case in args.cases:
        S, N = (int(v) for v in case.split("x"))
        rng = np.random.default_rng(0)
        big = gaussian_filter(rng.random((N + 64, N + 64), dtype=np.float32), 2.0).astype(np.float32)
        ref = np.ascontiguousarray(big[20:20 + N, 30:30 + N])
        frames = [np.ascontiguousarray(big[20 + (s % 7 - 3):20 + (s % 7 - 3) + N, 30 + (2 - s % 5):30 + (2 - s % 5) + N]) for s in range(S)]
        la = sp.LinearAlign(ref)
        res = {"ref_keypoints": int(len(la.ref_kp))}
        forms = (("shift_only", dict(shift_only=True)), ("affine", dict()), ("robust", dict(robust=True)))
        for name, kw in forms:
            loop = lambda: [la.align(f, estimate="device", median="device", **kw) for f in frames]      # noqa: E731
            batch = lambda: la.align_batch(frames, **kw)                                              # noqa: E731
            looped, batched = loop(), batch()                   # warm-up of both forms at this shape
            worst = max(float(np.abs(a - b).max()) for a, b in zip(looped, batched) if a is not None)
            times = {"loop": [], "batch": []}
            del looped, batched                                 # (one form's result at a time: both are S frames of pinned memory)
            for _ in range(args.reps):
                looped, t = clock(loop); times["loop"].append(t)
                del looped
                batched, t = clock(batch); times["batch"].append(t)
                del batched
            res[name] = {"loop_ms": stats(times["loop"]), "batch_ms": stats(times["batch"]),
                         "loop_over_batch": round(float(np.median(times["loop"]) / np.median(times["batch"])), 3),
                         "batch_wholly_below_loop": bool(max(times["batch"]) < min(times["loop"])),
                         "max_abs_difference_of_the_results": worst}
        stages, M, off, fills = stage_times(la, frames)
        stages, M, off, fills = stage_times(la, frames)          # the second replay: every buffer has its size
        res["align_batch_stage_ms"] = stages
        bp = la._batch_plan()
        times = {"loop": [], "batch": [], "loop_kernel": [], "batch_kernel": []}
        for r in range(args.reps + 1):
            def warp_loop():
                ks = 0.0
                for s in range(S):
                    la.transform(M[s], off[s], image=frames[s], fill=float(fills[s]))
                    ks += la.last_transform_ms
                return ks
            ks, tl = clock(warp_loop)
            _, tb = clock(lambda: bp.transform_batch(frames, M, off, fills, out_shape=la.outshape))
            if r:
                times["loop"].append(tl); times["batch"].append(tb); times["loop_kernel"].append(ks); times["batch_kernel"].append(bp.last_transform_ms)
        k_ms = float(np.median(times["batch_kernel"]))
        res["transform"] = {k + "_ms": stats(v) for k, v in times.items()}
        res["transform"]["batch_kernel_GBps"] = round(8.0 * S * N * N / 1e9 / (k_ms / 1e3), 1)
        res["transform"]["loop_over_batch"] = round(float(np.median(times["loop"]) / np.median(times["batch"])), 3)
        out["cases"]["S=%d %dx%d" % (S, N, N)] = res
        print("S=%d %dx%d: %s" % (S, N, N, json.dumps(res)), file=sys.stderr, flush=True)
        del la, bp, frames
    print(json.dumps(out))


if __name__ == "__main__":
    main()
