#!/usr/bin/env python
"""Windowed matching against the brute-force matcher on the frame pair of tools/bench_align.py:
a 4096^2 frame and the same content moved by +11 / -7 pixels, both keypoint lists resident in HBM.

    python tools/bench_match_window.py [--size 4096] [--reps 12] [--windows 16 64 256]

match() and match(window=w) alternate in one process after warm-up; per variant the median, minimum and maximum of the device
time of all kernels of a call (MatchPlan.kernel_ms) and of the wall time per call, and the pair counts.  Then align(img) and
align(img, max_shift=16) alternate the same way, with the device times of the pieces of the last call.  Prints one JSON line.
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
    variants = [("plain", {})] + [("window_%g" % w, {"window": w}) for w in a.windows]
    kernel = {n: [] for n, _ in variants}; wall = {n: [] for n, _ in variants}; pairs = {}
    for rep in range(a.reps + 2):                          # two warm-up rounds
        for name, kw in variants:
            t0 = time.perf_counter()
            got = mp.match(l1, l2, raw_results=True, **kw)
            dt = 1e3 * (time.perf_counter() - t0)
            if rep >= 2:
                kernel[name].append(mp.kernel_ms()); wall[name].append(dt)
            pairs[name] = int(len(got))
            if kw and rep == 0:                            # sanity: every pair of a windowed call lies inside its window
                assert (np.abs(kp["x"][got[:, 1]] - la.ref_kp["x"][got[:, 0]]) <= np.float32(kw["window"])).all()
    out = {"size": S, "keypoints": [int(len(la.ref_kp)), int(len(kp))], "reps": a.reps, "match": {}}
    for name, _ in variants:
        out["match"][name] = {"kernel_ms": stats(kernel[name]), "call_ms": stats(wall[name]), "pairs": pairs[name],
                              "kernel_speedup": round(float(np.median(kernel["plain"]) / np.median(kernel[name])), 2)}
    # end to end
    wall = {"align": [], "align_max_shift": []}
    pieces = {}
    for rep in range(a.reps + 2):
        for name, kw in (("align", {}), ("align_max_shift", {"max_shift": a.max_shift})):
            t0 = time.perf_counter()
            la.align(img, **kw)
            dt = 1e3 * (time.perf_counter() - t0)
            if rep >= 2:
                wall[name].append(dt)
            pieces[name] = {"match_kernel_ms": round(la.match.kernel_ms(), 3), "transform_kernel_ms": round(la.last_transform_ms, 3)}
    for name in wall:
        r = la.align(img, return_all=True, **({"max_shift": a.max_shift} if name == "align_max_shift" else {}))
        out[name] = dict(pieces[name], align_ms=stats(wall[name]), matches=int(r["matching"].shape[0]),
                         offset=[float(v) for v in r["offset"]], rms=float(r["rms"]))
    t = []
    for _ in range(5):
        t0 = time.perf_counter(); la.sift.keypoints(img); t.append(1e3 * (time.perf_counter() - t0))
    out["keypoints_call_ms"] = stats(t)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
