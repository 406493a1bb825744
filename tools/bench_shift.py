#!/usr/bin/env python
"""Device median timing.

    python tools/bench_shift.py [--matches 5000 200000] [--calls 12] [--size 4096] [--no-align]

(a) MatchPlan.shift on M pairs, lists and pairs resident in HBM: the whole call (host clock, the call ends in a stream
    synchronise) and the hipEvent time from the gather to the last kernel, against the host path it replaces on the same
    pairs with host lists: the two gathers of LinearAlign.align (``_xysa`` heads indexed by the pairs) plus
    ``LinearAlign._median_shift``.  The two variants alternate call by call in one process.
(b) LinearAlign.align(shift_only=True, max_shift=16) on the frame pair of tools/bench_align.py: median="host" against
    median="device", alternating.

`--calls` timed calls each; medians with (min, max).  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def stats(v):
    return {"median": round(float(np.median(v)), 4), "min": round(float(min(v)), 4), "max": round(float(max(v)), 4), "calls": len(v)}


def bench_shift(M, calls):
    import torch
    import sift_pyocl_amd as sp
    from sift_pyocl_amd.alignment import LinearAlign
    from consensus_ref import synthetic_matches
    kp1, kp2, pairs, inlier, truth = synthetic_matches(M, 0.9, 7)
    mp = sp.MatchPlan(profile=True)
    t1 = torch.from_numpy(kp1.view(np.uint8).reshape(-1)).cuda(); t2 = torch.from_numpy(kp2.view(np.uint8).reshape(-1)).cuda()
    tp = torch.from_numpy(pairs).cuda()
    torch.cuda.synchronize()
    heads1 = np.ascontiguousarray(LinearAlign._xysa(kp1))      # align() keeps the reference's heads; the new frame's are packed per call

    def device():
        t0 = time.perf_counter()
        moved, n = mp.shift(t1, t2, tp)
        return 1e3 * (time.perf_counter() - t0), moved

    def host():
        t0 = time.perf_counter()
        g0 = heads1[pairs[:, 0]]
        g1 = np.ascontiguousarray(LinearAlign._xysa(kp2))[pairs[:, 1]]
        t1_ = time.perf_counter()
        matrix, offset = LinearAlign._median_shift(g0, g1)
        t2_ = time.perf_counter()
        return 1e3 * (t2_ - t0), 1e3 * (t1_ - t0), 1e3 * (t2_ - t1_), offset
    for _ in range(5):
        device(); host()
    mp.reset_timer()
    dev_call, host_call, host_gather, host_median = [], [], [], []
    for _ in range(calls):
        ms, moved = device(); dev_call.append(ms)
        ms, g, s, offset = host(); host_call.append(ms); host_gather.append(g); host_median.append(s)
    kernels = [evt.ms for label, evt in mp.events if label == "shift"]
    return {"matches": M, "shift_call_ms": stats(dev_call), "shift_kernels_ms": stats(kernels), "host_path_ms": stats(host_call),
            "host_gathers_ms": stats(host_gather), "host_medians_ms": stats(host_median),
            "saved_ms": round(float(np.median(host_call) - np.median(dev_call)), 4),
            "equal": bool(moved[0] == offset[1] and moved[1] == offset[0])}


def bench_align(size, calls):
    import sift_pyocl_amd as sp
    from scipy.ndimage import gaussian_filter
    S = size
    rng = np.random.default_rng(0)
    big = gaussian_filter(rng.random((S + 64, S + 64), dtype=np.float32), 2.0).astype(np.float32)
    ref = np.ascontiguousarray(big[20:20 + S, 30:30 + S]); img = np.ascontiguousarray(big[27:27 + S, 19:19 + S])
    la = sp.LinearAlign(ref)
    kw = dict(shift_only=True, max_shift=16)
    times = {"host": [], "device": []}
    res = {}
    for med in ("host", "device"):
        res[med] = la.align(img, return_all=True, median=med, **kw)                  # warm-up, and the results to compare
        la.align(img, median=med, **kw)
    for _ in range(calls):
        for med in ("host", "device"):
            t0 = time.perf_counter()
            la.align(img, median=med, **kw)
            times[med].append(1e3 * (time.perf_counter() - t0))
    h, d = res["host"], res["device"]
    return {"size": S, "ref_keypoints": int(len(la.ref_kp)), "matches": int(h["matching"].shape[0]),
            "host_ms": stats(times["host"]), "device_ms": stats(times["device"]),
            "saved_ms": round(float(np.median(times["host"]) - np.median(times["device"])), 3),
            "offset_equal": bool((h["offset"] == d["offset"]).all()), "result_equal": bool(np.array_equal(h["result"], d["result"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, nargs="+", default=[5000, 200000])
    ap.add_argument("--calls", type=int, default=12)
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--no-align", action="store_true")
    a = ap.parse_args()
    out = {"shift": [bench_shift(M, a.calls) for M in a.matches]}
    if not a.no_align:
        out["align"] = bench_align(a.size, a.calls)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
