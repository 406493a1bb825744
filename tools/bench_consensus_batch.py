#!/usr/bin/env python
"""MatchPlan.consensus_batch against the loop of consensus() calls it replaces.

    python tools/bench_consensus_batch.py [--cases 8x1000 64x1000 ...] [--min-window 0.2]

Everything is resident in HBM: a reference list of M records with positions uniform in a 4096 x 4096 frame, S segments of M records
each, and S x M pairs (row r of a segment pairs record perm[r] of the reference with record r of the segment).  Half of every
segment's pairs follow the segment's own map (a rotation of up to 3 degrees, a shift of up to 40 px, 0.3 px of noise), the others
lie anywhere.  n_hyp = 2048, tol = 3.  Per case the three forms alternate in one process after two warm-up rounds, a host clock
around each:
    loop          [consensus(ref, seg_s, pairs_s) for s in range(S)]: S stream synchronisations, every mask to the host
    batch host    consensus_batch(ref, None, segs, counts, pairs, pair_counts)
    batch device  the same with out="device": the mask stays in HBM
All end in the stream synchronisation the calls contain.  The loop is code the batch call does not touch.  Prints one JSON line:
per case the median, minimum and maximum of one pass over the S segments in ms for the three forms, the ratios (of the medians),
whether each batch form's range lies wholly below the loop's, and the hipEvent time of the vote kernel: the batch's one launch and
the sum over the loop's S launches; the results of the forms are checked to be the same bits.
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

from bench_match_batch import stats  # noqa: E402

DEFAULT_CASES = ["8x1000", "8x4000", "8x16000", "64x1000", "64x4000", "64x16000", "1x200000"]
N_HYP, TOL = 2048, 3.0


def matches(S, M, dtype_kp):
    rng = np.random.default_rng(5)
    a, b = np.zeros(M, dtype_kp), np.zeros(S * M, dtype_kp)
    a["x"] = rng.uniform(0, 4096, M); a["y"] = rng.uniform(0, 4096, M)
    b["x"] = rng.uniform(0, 4096, S * M); b["y"] = rng.uniform(0, 4096, S * M)
    pairs = np.empty((S * M, 2), np.int32)
    half = M // 2
    for s in range(S):
        perm = rng.permutation(M)
        th, (tx, ty) = np.deg2rad(rng.uniform(-3, 3)), rng.uniform(-40, 40, 2)
        seg = b[s * M:(s + 1) * M]
        x, y = a["x"][perm[:half]], a["y"][perm[:half]]
        seg["x"][:half] = np.cos(th) * x - np.sin(th) * y + tx + rng.normal(0, 0.3, half)
        seg["y"][:half] = np.sin(th) * x + np.cos(th) * y + ty + rng.normal(0, 0.3, half)
        pairs[s * M:(s + 1) * M, 0] = perm
        pairs[s * M:(s + 1) * M, 1] = np.arange(M)
    return a, b, pairs


def same_bits(x, y):
    x, y = np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)
    return bool(np.array_equal(np.isnan(x), np.isnan(y)) and x[~np.isnan(x)].tobytes() == y[~np.isnan(y)].tobytes())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=DEFAULT_CASES, help="SxM: segments x pairs per segment")
    ap.add_argument("--min-window", type=float, default=0.2, help="seconds every timed window must last at least")
    ap.add_argument("--min-reps", type=int, default=7)
    args = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    out = {"n_hyp": N_HYP, "tol": TOL, "min_window_s": args.min_window, "cases": {}}
    for case in args.cases:
        S, M = (int(v) for v in case.split("x"))
        a, b, p = matches(S, M, sp.MatchPlan.dtype_kp)
        ta = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda(); tb = torch.from_numpy(b.view(np.uint8).reshape(-1)).cuda()
        pairs = torch.from_numpy(p).cuda()
        torch.cuda.synchronize()
        mp = sp.MatchPlan(size=M, profile=True)
        counts = pair_counts = [M] * S
        segs = [tb[s * M * 144:(s + 1) * M * 144] for s in range(S)]
        slices = [pairs[s * M:(s + 1) * M] for s in range(S)]
        forms = {
            "loop": lambda: [mp.consensus(ta, segs[s], slices[s], n_hyp=N_HYP, tol=TOL) for s in range(S)],
            "batch_host": lambda: mp.consensus_batch(ta, None, tb, counts, pairs, pair_counts, n_hyp=N_HYP, tol=TOL),
            "batch_device": lambda: mp.consensus_batch(ta, None, tb, counts, pairs, pair_counts, n_hyp=N_HYP, tol=TOL, out="device"),
        }
        once, got = {}, {}
        for _ in range(2):                                     # two warm-up rounds, timed to size the windows
            for name, form in forms.items():
                t0 = time.perf_counter(); got[name] = form(); once[name] = time.perf_counter() - t0
        loop_mask = np.concatenate([r[0] for r in got["loop"]])
        loop_models = np.stack([np.full(6, np.nan, np.float32) if r[1] is None else r[1] for r in got["loop"]])
        same = True
        for name in ("batch_host", "batch_device"):
            mask, models, votes = got[name]
            mask = mask.cpu().numpy() if name == "batch_device" else mask
            same = same and bool(np.array_equal(loop_mask, mask.astype(bool)) and same_bits(loop_models, models) and
                                 [r[2] for r in got["loop"]] == votes.tolist())
        assert same, "consensus_batch != the loop of consensus at %s" % case
        reps = max(args.min_reps, int(np.ceil(args.min_window / min(once.values()))))
        times = {name: [] for name in forms}
        kernel = {name: [] for name in forms}
        for _ in range(reps):
            for name, form in forms.items():
                mp.reset_timer()
                t0 = time.perf_counter(); form(); times[name].append(1e3 * (time.perf_counter() - t0))
                kernel[name].append(sum(evt.ms for label, evt in mp.events))      # the vote kernel: one launch, or the loop's S
        res = {"pairs": S * M, "reps": reps, "votes_of_segment_0": int(got["loop"][0][2]), "same_bits": same}
        for name in forms:
            res[name + "_ms"] = stats(times[name])
            res[name + "_vote_kernel_ms"] = stats(kernel[name])
        for name in ("batch_host", "batch_device"):
            res["loop_over_" + name] = round(float(np.median(times["loop"]) / np.median(times[name])), 3)
            res[name + "_wholly_below_loop"] = bool(max(times[name]) < min(times["loop"]))
        out["cases"]["S=%d M=%d" % (S, M)] = res
        print("S=%d M=%d: %s" % (S, M, json.dumps(res)), file=sys.stderr, flush=True)
        del mp, ta, tb, segs, slices, pairs
    print(json.dumps(out))


if __name__ == "__main__":
    main()
