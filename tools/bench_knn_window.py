#!/usr/bin/env python
"""Windowed knn against windowed matching and against brute-force knn on the frame pair of
tools/bench_align.py: a 4096^2 frame and the same content moved by +11 / -7 pixels, both keypoint lists resident in HBM.

    python tools/bench_knn_window.py [--size 4096] [--reps 12] [--windows 16 64 256]

match(window=w), knn_window(k, window=w) for k = 1, 2, 4, 8 on both metrics and brute-force knn(2) on both metrics alternate in one
process after warm-up; per variant the median, minimum and maximum of the device time of all kernels of a call
(MatchPlan.kernel_ms) and of the wall time per call.  Then align(max_shift=16) and align(max_shift=16, match_metric="l2",
match_ratio=0.8) alternate the same way.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--windows", type=float, nargs="+", default=[16, 64, 256])
    ap.add_argument("--max-shift", type=float, default=16)
    a = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    from sift_pyocl_amd.match import ratio_filter
    from scipy.ndimage import gaussian_filter
    S = a.size
    rng = np.random.default_rng(0)
    big = gaussian_filter(rng.random((S + 64, S + 64), dtype=np.float32), 2.0).astype(np.float32)
    ref = np.ascontiguousarray(big[20:20 + S, 30:30 + S]); img = np.ascontiguousarray(big[27:27 + S, 19:19 + S])
    la = sp.LinearAlign(ref)
    kp = la.sift.keypoints(img)
    l1 = la._ref_dev if la._ref_dev is not None else la.ref_kp
    l2 = torch.from_numpy(np.ascontiguousarray(kp).view(np.uint8).reshape(-1).copy()).cuda()
    torch.cuda.synchronize()
    mp = sp.MatchPlan()
    variants = []
    for w in a.windows:
        variants.append(("match_w%g" % w, lambda w=w: mp.match(l1, l2, raw_results=True, window=w)))
        for metric in ("l1", "l2"):
            for k in (1, 2, 4, 8):
                variants.append(("knn%d_%s_w%g" % (k, metric, w), lambda w=w, k=k, metric=metric: mp.knn_window(l1, l2, k, metric=metric, window=w)))
    for metric in ("l1", "l2"):
        variants.append(("knn2_%s_brute" % metric, lambda metric=metric: mp.knn(l1, l2, 2, metric=metric)))
    kernel = {n: [] for n, _ in variants}; wall = {n: [] for n, _ in variants}
    results = {}
    for rep in range(a.reps + 2):                          # two warm-up rounds
        for name, call in variants:
            t0 = time.perf_counter()
            got = call()
            dt = 1e3 * (time.perf_counter() - t0)
            if rep >= 2:
                kernel[name].append(mp.kernel_ms()); wall[name].append(dt)
            if rep == 0:
                results[name] = got
    # sanity: ratio_filter of the windowed rows is the windowed match (W1)
    for w in a.windows:
        got = ratio_filter(*results["knn2_l1_w%g" % w]); want = results["match_w%g" % w]
        assert np.array_equal(got[np.lexsort((got[:, 1], got[:, 0]))], want[np.lexsort((want[:, 1], want[:, 0]))])
    out = {"size": S, "keypoints": [int(len(la.ref_kp)), int(len(kp))], "reps": a.reps, "calls": {}}
    for name, _ in variants:
        out["calls"][name] = {"kernel_ms": stats(kernel[name]), "call_ms": stats(wall[name])}
    for w in a.windows:
        m = np.median(kernel["match_w%g" % w])
        out["calls"]["knn2_l1_w%g" % w]["kernel_vs_match"] = round(float(np.median(kernel["knn2_l1_w%g" % w]) / m), 3)
        for metric in ("l1", "l2"):
            out["calls"]["knn2_%s_w%g" % (metric, w)]["kernel_speedup_vs_brute"] = round(
                float(np.median(kernel["knn2_%s_brute" % metric]) / np.median(kernel["knn2_%s_w%g" % (metric, w)])), 2)
    # end to end
    kinds = (("align_max_shift", {"max_shift": a.max_shift}),
             ("align_max_shift_l2_0.8", {"max_shift": a.max_shift, "match_metric": "l2", "match_ratio": 0.8}))
    wall = {n: [] for n, _ in kinds}
    pieces = {}
    for rep in range(a.reps + 2):
        for name, kw in kinds:
            t0 = time.perf_counter()
            la.align(img, **kw)
            dt = 1e3 * (time.perf_counter() - t0)
            if rep >= 2:
                wall[name].append(dt)
            pieces[name] = {"match_kernel_ms": round(la.match.kernel_ms(), 3)}
    for name, kw in kinds:
        r = la.align(img, return_all=True, **kw)
        out[name] = dict(pieces[name], align_ms=stats(wall[name]), matches=int(r["matching"].shape[0]),
                         offset=[float(v) for v in r["offset"]], rms=float(r["rms"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
