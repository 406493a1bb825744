#!/usr/bin/env python
"""Device fit timing.

    python tools/bench_fit.py [--matches 5000 200000] [--seconds 0.5] [--size 4096] [--reps 7] [--no-align]

(a) MatchPlan.fit on M pairs, lists and pairs resident in HBM: the whole call (host clock, the call ends in a stream
    synchronise) and the hipEvent time from the gather to the last kernel, against the host path it replaces on the same
    pairs with host lists: the two gathers of LinearAlign.align (``_xysa`` heads indexed by the pairs) plus
    ``utils.affine_least_squares``.  The two variants alternate call by call.
(b) LinearAlign.align on the frame pair of tools/bench_align.py: estimate="host" against "device", alternating, each without
    and with max_shift=16, and with robust=True.

Medians with (min, max).  Prints one JSON line.
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


def bench_fit(M, seconds):
    import torch
    import sift_pyocl_amd as sp
    from sift_pyocl_amd.alignment import LinearAlign
    from sift_pyocl_amd.utils import affine_least_squares
    from consensus_ref import synthetic_matches
    kp1, kp2, pairs, inlier, truth = synthetic_matches(M, 0.9, 7)
    mp = sp.MatchPlan(profile=True)
    t1 = torch.from_numpy(kp1.view(np.uint8).reshape(-1)).cuda(); t2 = torch.from_numpy(kp2.view(np.uint8).reshape(-1)).cuda()
    tp = torch.from_numpy(pairs).cuda()
    torch.cuda.synchronize()
    heads1 = np.ascontiguousarray(LinearAlign._xysa(kp1))      # align() keeps the reference's heads; the new frame's are packed per call

    def device():
        t0 = time.perf_counter()
        model, rms, n = mp.fit(t1, t2, tp)
        return 1e3 * (time.perf_counter() - t0), model

    def host():
        t0 = time.perf_counter()
        g0 = heads1[pairs[:, 0]]
        g1 = np.ascontiguousarray(LinearAlign._xysa(kp2))[pairs[:, 1]]
        t1_ = time.perf_counter()
        model = affine_least_squares(g0[:, 0], g0[:, 1], g1[:, 0], g1[:, 1])
        t2_ = time.perf_counter()
        return 1e3 * (t2_ - t0), 1e3 * (t1_ - t0), 1e3 * (t2_ - t1_), model
    for _ in range(5):
        device(); host()
    mp.reset_timer()
    dev_call, host_call, host_gather, host_solve = [], [], [], []
    t_end = time.perf_counter() + seconds
    while time.perf_counter() < t_end or len(dev_call) < 20:
        ms, model_d = device(); dev_call.append(ms)
        ms, g, s, model_h = host(); host_call.append(ms); host_gather.append(g); host_solve.append(s)
    kernels = [evt.ms for label, evt in mp.events if label == "fit"]
    return {"matches": M, "fit_call_ms": stats(dev_call), "fit_kernels_ms": stats(kernels), "host_path_ms": stats(host_call),
            "host_gathers_ms": stats(host_gather), "host_least_squares_ms": stats(host_solve),
            "saved_ms": round(float(np.median(host_call) - np.median(dev_call)), 4),
            "largest_coefficient_difference": float(np.abs(np.asarray(model_d) - np.asarray(model_h)).max())}


def bench_align(size, reps):
    import sift_pyocl_amd as sp
    from scipy.ndimage import gaussian_filter
    S = size
    rng = np.random.default_rng(0)
    big = gaussian_filter(rng.random((S + 64, S + 64), dtype=np.float32), 2.0).astype(np.float32)
    ref = np.ascontiguousarray(big[20:20 + S, 30:30 + S]); img = np.ascontiguousarray(big[27:27 + S, 19:19 + S])
    la = sp.LinearAlign(ref)
    out = {"size": S, "ref_keypoints": int(len(la.ref_kp)), "variants": []}
    for name, kw in (("brute", dict()), ("max_shift16", dict(max_shift=16)), ("robust", dict(robust=True)),
                     ("max_shift16_robust", dict(max_shift=16, robust=True))):
        times = {"host": [], "device": []}
        res = {}
        for est in ("host", "device"):
            res[est] = la.align(img, return_all=True, estimate=est, **kw)            # warm-up, and the results to compare
        for _ in range(reps):
            for est in ("host", "device"):
                t0 = time.perf_counter()
                la.align(img, estimate=est, **kw)
                times[est].append(1e3 * (time.perf_counter() - t0))
        h, d = res["host"], res["device"]
        out["variants"].append({"name": name, "matches": int(h["matching"].shape[0]), "host_ms": stats(times["host"]),
                                "device_ms": stats(times["device"]),
                                "saved_ms": round(float(np.median(times["host"]) - np.median(times["device"])), 3),
                                "matrix_difference": float(np.abs(h["matrix"].astype(np.float64) - d["matrix"]).max()),
                                "offset_difference": float(np.abs(h["offset"].astype(np.float64) - d["offset"]).max()),
                                "result_equal": bool(np.array_equal(h["result"], d["result"])),
                                "rms_host": float(h["rms"]), "rms_device": float(d["rms"])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, nargs="+", default=[5000, 200000])
    ap.add_argument("--seconds", type=float, default=0.5, help="least time the timed calls of a size fill")
    ap.add_argument("--size", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-align", action="store_true")
    a = ap.parse_args()
    out = {"fit": [bench_fit(M, a.seconds) for M in a.matches]}
    if not a.no_align:
        out["align"] = bench_align(a.size, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
