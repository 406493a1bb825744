#!/usr/bin/env python
"""MatchPlan.match_batch against the loop of match() calls it replaces, on lists made as
tools/bench_match.py makes them: a reference list of n 128-D uint8 descriptors and S segments of n each, half of every segment
within +-8 of a descriptor of the reference, everything resident in HBM.

    python tools/bench_match_batch.py [--segments 8 64] [--sizes 1000 4000 16000] [--min-window 0.3]

Per (S, n) the two forms alternate in one process after two warm-up rounds:
    loop    [match(ref, seg_s, raw_results=True) for s in range(S)]
    batch   match_batch(ref, None, segs, [n] * S, out="host")
A host clock runs around each form; both end in the stream synchronisation the calls contain, with the pairs on the host.  The
repetitions are chosen so that every timed window (all repetitions of one form) is well over a tenth of a second.  The loop is
code the batch call does not touch.  Prints one JSON line: per case the median, minimum and maximum time of one pass over the S
segments in ms for both forms, their ratio (loop / batch, of the medians), the device time of the batch call's kernels and the
number of pairs (checked to be the same rows).
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


def lists(S, n, dtype_kp):
    rng = np.random.default_rng(1)
    a = np.zeros(n, dtype_kp); a["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    rng2 = np.random.default_rng(2)
    b = np.zeros(S * n, dtype_kp)
    half = n // 2
    for s in range(S):
        perm = rng2.permutation(n)
        seg = b[s * n:(s + 1) * n]
        seg["desc"][:half] = np.clip(a["desc"][perm[:half]].astype(np.int16) + rng2.integers(-8, 9, (half, 128)), 0, 255).astype(np.uint8)
        seg["desc"][half:] = rng2.integers(0, 256, (n - half, 128), dtype=np.uint8)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--segments", type=int, nargs="+", default=[8, 64])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1000, 4000, 16000])
    ap.add_argument("--min-window", type=float, default=0.3, help="seconds every timed window must last at least")
    ap.add_argument("--min-reps", type=int, default=5)
    args = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    out = {"min_window_s": args.min_window, "cases": {}}
    for S in args.segments:
        for n in args.sizes:
            a, b = lists(S, n, sp.MatchPlan.dtype_kp)
            ta = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda(); tb = torch.from_numpy(b.view(np.uint8).reshape(-1)).cuda()
            segs = [tb[s * n * 144:(s + 1) * n * 144] for s in range(S)]
            torch.cuda.synchronize()
            mp = sp.MatchPlan(size=n)

            def loop():
                return [mp.match(ta, seg, raw_results=True) for seg in segs]

            def batch():
                return mp.match_batch(ta, None, tb, [n] * S, out="host")

            forms = (("loop", loop), ("batch", batch))
            once = {}
            for _ in range(2):                                 # two warm-up rounds, timed to size the windows
                for name, fn in forms:
                    t0 = time.perf_counter(); res = fn(); once[name] = time.perf_counter() - t0
                    if name == "loop":
                        loop_rows = [r[np.lexsort((r[:, 1], r[:, 0]))] for r in res]
                    else:
                        pairs, counts = res
            assert counts.tolist() == [len(r) for r in loop_rows] and np.array_equal(pairs, np.concatenate(loop_rows)), "match_batch != loop"
            reps = max(args.min_reps, int(np.ceil(args.min_window / min(once.values()))))
            times = {"loop": [], "batch": []}
            kernel = []
            for _ in range(reps):
                for name, fn in forms:
                    t0 = time.perf_counter(); fn(); times[name].append(1e3 * (time.perf_counter() - t0))
                    if name == "batch":
                        kernel.append(mp.kernel_ms())
            res = {"reps": reps, "pairs": int(len(pairs)), "loop_ms": stats(times["loop"]), "batch_ms": stats(times["batch"]),
                   "batch_kernel_ms": stats(kernel), "window_s": {k: round(sum(v) / 1e3, 3) for k, v in times.items()},
                   "loop_over_batch": round(float(np.median(times["loop"]) / np.median(times["batch"])), 3)}
            out["cases"]["S=%d n=%d" % (S, n)] = res
            del mp, ta, tb, segs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
