#!/usr/bin/env python
"""MatchPlan.shift_batch / fit_batch against the loops of shift() / fit() calls they replace.

    python tools/bench_estimate_batch.py [--cases 8x1000 64x1000 ...] [--min-window 0.2]

Everything is resident in HBM.  The lists are made as tools/bench_match_batch.py makes them (a reference list of m descriptors and
S segments of m each, half of every segment within +-8 of a descriptor of the reference) and given positions: the reference's
are uniform in a 4096 x 4096 frame, a matched record sits at its partner's position moved by the segment's own shift plus 0.3 px of
noise, the others anywhere.  The pairs are those of match_batch(out="device") on these lists.  Per case and per estimate the two
forms alternate in one process after two warm-up rounds, a host clock around each:
    loop    [shift(ref, seg_s, pairs_s) for s in range(S)]      (then the same with fit)
    batch   shift_batch(ref, None, segs, counts, pairs, pair_counts)
Both end in the stream synchronisation the calls contain, with the results on the host.  The loop is code the batch call does not
touch.  Prints one JSON line: per case and estimate the median, minimum and maximum of one pass over the S segments in ms for both
forms, their ratio (of the medians), whether the batch's range lies wholly below the loop's, and the hipEvent time of the batch
call's kernels; the results of the two forms are checked to be the same bits.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from bench_match_batch import lists, stats  # noqa: E402

DEFAULT_CASES = ["8x1000", "8x4000", "8x16000", "64x1000", "64x4000", "64x16000", "1x200000"]


def positioned(S, m, dtype_kp):
    """bench_match_batch.lists with positions: segment s's matched half follows the reference moved by (s % 7 - 3, 2 - s % 5)"""
    a, b = lists(S, m, dtype_kp)
    rng = np.random.default_rng(3)
    a["x"] = rng.uniform(0, 4096, m); a["y"] = rng.uniform(0, 4096, m)
    rng2 = np.random.default_rng(2)                            # the stream lists() draws its permutations from
    half = m // 2
    for s in range(S):
        perm = rng2.permutation(m)
        rng2.integers(-8, 9, (half, 128)); rng2.integers(0, 256, (m - half, 128), dtype=np.uint8)
        seg = b[s * m:(s + 1) * m]
        seg["x"] = rng.uniform(0, 4096, m); seg["y"] = rng.uniform(0, 4096, m)
        seg["x"][:half] = a["x"][perm[:half]] + (s % 7 - 3) + rng.normal(0, 0.3, half)
        seg["y"][:half] = a["y"][perm[:half]] + (2 - s % 5) + rng.normal(0, 0.3, half)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=DEFAULT_CASES, help="SxM: segments x keypoints per segment")
    ap.add_argument("--min-window", type=float, default=0.2, help="seconds every timed window must last at least")
    ap.add_argument("--min-reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    out = {"min_window_s": args.min_window, "cases": {}}
    for case in args.cases:
        S, m = (int(v) for v in case.split("x"))
        a, b = positioned(S, m, sp.MatchPlan.dtype_kp)
        ta = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda(); tb = torch.from_numpy(b.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        mp = sp.MatchPlan(size=m, profile=True)
        counts = [m] * S
        pairs, pair_counts = mp.match_batch(ta, None, tb, counts, out="device")
        rows = np.concatenate([[0], np.cumsum(pair_counts)])
        segs = [tb[s * m * 144:(s + 1) * m * 144] for s in range(S)]
        slices = [pairs[rows[s]:rows[s + 1]] for s in range(S)]
        res = {"pairs": int(len(pairs))}
        forms = {
            "shift": (lambda: [mp.shift(ta, segs[s], slices[s], return_ranks=True) for s in range(S)],
                      lambda: mp.shift_batch(ta, None, tb, counts, pairs, pair_counts, return_ranks=True)),
            "fit": (lambda: [mp.fit(ta, segs[s], slices[s], return_moments=True) for s in range(S)],
                    lambda: mp.fit_batch(ta, None, tb, counts, pairs, pair_counts, return_moments=True)),
        }
        for what, (loop, batch) in forms.items():
            once = {}
            for _ in range(2):                                 # two warm-up rounds, timed to size the windows
                t0 = time.perf_counter(); looped = loop(); once["loop"] = time.perf_counter() - t0
                t0 = time.perf_counter(); batched = batch(); once["batch"] = time.perf_counter() - t0
            raw_loop, raw_batch = np.stack([r[-1] for r in looped]), batched[-1]
            same = bool(np.array_equal(np.isnan(raw_loop), np.isnan(raw_batch)) and
                        np.array_equal(raw_loop[~np.isnan(raw_loop)].tobytes(), raw_batch[~np.isnan(raw_batch)].tobytes()))
            assert same, "%s_batch != the loop of %s at %s" % (what, what, case)
            reps = max(args.min_reps, int(np.ceil(args.min_window / min(once.values()))))
            times = {"loop": [], "batch": []}
            kernel = []
            for _ in range(reps):
                t0 = time.perf_counter(); loop(); times["loop"].append(1e3 * (time.perf_counter() - t0))
                mp.reset_timer()
                t0 = time.perf_counter(); batch(); times["batch"].append(1e3 * (time.perf_counter() - t0))
                kernel += [evt.ms for label, evt in mp.events if label == what + "_batch"]
                mp.reset_timer()
            res[what] = {"reps": reps, "loop_ms": stats(times["loop"]), "batch_ms": stats(times["batch"]), "batch_kernel_ms": stats(kernel),
                         "loop_over_batch": round(float(np.median(times["loop"]) / np.median(times["batch"])), 3),
                         "batch_wholly_below_loop": bool(max(times["batch"]) < min(times["loop"])), "same_bits": same}
        out["cases"]["S=%d m=%d" % (S, m)] = res
        print("S=%d m=%d: %s" % (S, m, json.dumps(res)), file=sys.stderr, flush=True)
        del mp, ta, tb, segs, slices, pairs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
