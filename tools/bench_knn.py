#!/usr/bin/env python
"""k-nearest-neighbour matching against the brute-force matcher on the lists of tools/bench_match.py:
n x n 128-D uint8 descriptors, half of the second list within +-8 of a descriptor of the first, both lists resident in HBM.

    python tools/bench_knn.py [--sizes 100000 10000] [--reps 12] [--ks 1 2 4 8] [--metrics l1 l2]

match() and knn(k, metric) alternate in one process after two warm-up rounds; per variant the median, minimum and maximum of the
device time of the kernels of a call (MatchPlan.kernel_ms: the partial and the merge kernel) and of the wall time of the whole call
(for knn that includes the copy of 2 * n * k int32 to the host), and the kernel time relative to match()'s beside the ratio the
instruction count predicts, (32 + 2k - 2) / (32 + 2).  A squared-Euclidean variant (`knn_l2_<k>`) is also
set against the L1 instance of the same k in the same run, beside (32 + 1 + 2k - 2) / (32 + 2k - 2).  Prints one JSON line.
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


def lists(n, dtype_kp):
    rng = np.random.default_rng(1)
    a = np.zeros(n, dtype_kp); a["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    rng2 = np.random.default_rng(2)
    b = np.zeros(n, dtype_kp)
    perm = rng2.permutation(n); half = n // 2
    b["desc"][:half] = np.clip(a["desc"][perm[:half]].astype(np.int16) + rng2.integers(-8, 9, (half, 128)), 0, 255).astype(np.uint8)
    b["desc"][half:] = rng2.integers(0, 256, (n - half, 128), dtype=np.uint8)
    return a, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[100000, 10000])
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--ks", type=int, nargs="+", default=[1, 2, 4, 8])
    ap.add_argument("--metrics", nargs="+", choices=["l1", "l2"], default=["l1"])
    args = ap.parse_args()
    import torch
    import sift_pyocl_amd as sp
    from sift_pyocl_amd.match import ratio_filter
    out = {"reps": args.reps, "sizes": {}}
    for n in args.sizes:
        a, b = lists(n, sp.MatchPlan.dtype_kp)
        ta = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda(); tb = torch.from_numpy(b.view(np.uint8).reshape(-1)).cuda()
        torch.cuda.synchronize()
        mp = sp.MatchPlan(size=n)
        variants = [("match", None, None)] + [("knn_%d" % k if metric == "l1" else "knn_%s_%d" % (metric, k), k, metric)
                                              for k in args.ks for metric in args.metrics]
        kernel = {name: [] for name, _, _ in variants}; wall = {name: [] for name, _, _ in variants}
        pairs = None
        for rep in range(args.reps + 2):                       # two warm-up rounds
            for name, k, metric in variants:
                t0 = time.perf_counter()
                got = mp.match(ta, tb, raw_results=True) if k is None else mp.knn(ta, tb, k, metric=metric)
                dt = 1e3 * (time.perf_counter() - t0)
                if rep >= 2:
                    kernel[name].append(mp.kernel_ms()); wall[name].append(dt)
                if rep == 0 and k is None:
                    pairs = got
                if rep == 0 and k == 2 and metric == "l1":     # sanity: the ratio test over the two nearest is match()
                    mine = ratio_filter(*got)
                    assert np.array_equal(mine, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]), "knn(2) + ratio_filter != match()"
                if rep == 0 and metric == "l2":                # sanity: the first queries' rows against numpy
                    d = ((a["desc"][:8].astype(np.int64)[:, None, :] - b["desc"].astype(np.int64)[None, :, :]) ** 2).sum(axis=2)
                    order = np.argsort(d, axis=1, kind="stable")[:, :k]
                    assert np.array_equal(got[0][:8], order) and np.array_equal(got[1][:8], np.take_along_axis(d, order, axis=1)), "knn l2 != numpy"
        base = float(np.median(kernel["match"]))
        res = {"pairs": int(len(pairs))}
        for name, k, metric in variants:
            res[name] = {"kernel_ms": stats(kernel[name]), "call_ms": stats(wall[name]), "kernel_vs_match": round(float(np.median(kernel[name])) / base, 3)}
            if k is not None:
                chain = max(2 * k - 2, 1)
                res[name]["metric"] = metric
                res[name]["instruction_ratio"] = round((32 + (metric == "l2") + chain) / 34.0, 3)
                if metric == "l2" and "knn_%d" % k in kernel:
                    res[name]["kernel_vs_l1"] = round(float(np.median(kernel[name])) / float(np.median(kernel["knn_%d" % k])), 3)
                    res[name]["instruction_ratio_vs_l1"] = round((33 + chain) / (32.0 + chain), 3)
        out["sizes"][str(n)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
