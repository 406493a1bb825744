#!/usr/bin/env python
"""Consensus filter timing: hipEvent time of consensus_vote_kernel alone and of a whole
MatchPlan.consensus call, lists and pairs resident on the device.

    python tools/bench_consensus.py [--matches 200000 5000] [--hyp 2048] [--seconds 0.5]

A vote is 6 mul + 7 add/sub + 1 compare = 14 f32 lane-operations; the bound it is held against is 79e12 unfused
lane-operations per second (157.3 TFLOPS vector f32 counts an FMA as two).  Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

LANE_OPS_PER_VOTE = 14
LANE_OPS_PER_S = 79e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--matches", type=int, nargs="+", default=[200000, 5000])
    ap.add_argument("--hyp", type=int, default=2048)
    ap.add_argument("--tol", type=float, default=3.0)
    ap.add_argument("--inliers", type=float, default=0.5)
    ap.add_argument("--seconds", type=float, default=0.5, help="least time the timed calls of a size fill")
    a = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    from consensus_ref import synthetic_matches
    L = _lib.lib()
    mp = sp.MatchPlan()
    out = {"n_hyp": a.hyp, "tol": a.tol, "sizes": []}
    for M in a.matches:
        kp1, kp2, pairs, inlier, truth = synthetic_matches(M, a.inliers, 7)
        t1 = torch.from_numpy(kp1.view(np.uint8).reshape(-1)).cuda(); t2 = torch.from_numpy(kp2.view(np.uint8).reshape(-1)).cuda()
        tp = torch.from_numpy(pairs).cuda()
        torch.cuda.synchronize()
        mask = np.zeros(M, np.uint8); model = np.zeros(6, np.float32)
        winner, votes, ms = C.c_int32(), C.c_int32(), C.c_double()

        def call():
            _lib.check(L.siftmi_match_consensus(mp._handle, t1.data_ptr(), len(kp1), 1, t2.data_ptr(), len(kp2), 1, tp.data_ptr(), M, 1,
                                                a.hyp, C.c_float(a.tol), 0, mask.ctypes.data, model.ctypes.data, C.byref(winner),
                                                C.byref(votes), None, None, C.byref(ms)))
            return ms.value
        for _ in range(5):
            call()
        kernel, calls = [], []
        t_end = time.perf_counter() + a.seconds
        while time.perf_counter() < t_end or len(kernel) < 20:
            t0 = time.perf_counter()
            kernel.append(call())
            calls.append(1e3 * (time.perf_counter() - t0))
        k_ms = float(np.median(kernel))
        n_votes = float(M) * a.hyp
        bound_ms = 1e3 * n_votes * LANE_OPS_PER_VOTE / LANE_OPS_PER_S
        out["sizes"].append({"matches": M, "calls": len(kernel), "vote_kernel_ms": round(k_ms, 4),
                             "vote_kernel_ms_min_max": [round(min(kernel), 4), round(max(kernel), 4)],
                             "call_ms": round(float(np.median(calls)), 4), "votes_per_s": round(n_votes / (k_ms / 1e3), 0),
                             "bound_ms": round(bound_ms, 4), "share_of_bound": round(bound_ms / k_ms, 4),
                             "winner": winner.value, "winner_votes": votes.value, "true_inliers": int(inlier.sum())})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
