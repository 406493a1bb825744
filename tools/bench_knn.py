#!/usr/bin/env python
"""k-nearest-neighbour matching against the brute-force matcher on the lists of tools/bench_match.py:
n x n 128-D uint8 descriptors, half of the second list within +-8 of a descriptor of the first, both lists resident in HBM.

    python tools/bench_knn.py [--sizes 100000 10000] [--reps 12] [--ks 1 2 4 8]

match() and knn(k) alternate in one process after two warm-up rounds; per variant the median, minimum and maximum of the device
time of the kernels of a call (MatchPlan.kernel_ms: the partial and the merge kernel) and of the wall time of the whole call (for
knn that includes the copy of 2 * n * k int32 to the host), and the kernel time relative to match()'s beside the ratio the
instruction count predicts, (32 + 2k - 2) / (32 + 2).  Prints one JSON line.
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
        variants = [("match", None)] + [("knn_%d" % k, k) for k in args.ks]
        kernel = {name: [] for name, _ in variants}; wall = {name: [] for name, _ in variants}
        pairs = None
        for rep in range(args.reps + 2):                       # two warm-up rounds
            for name, k in variants:
                t0 = time.perf_counter()
                got = mp.match(ta, tb, raw_results=True) if k is None else mp.knn(ta, tb, k)
                dt = 1e3 * (time.perf_counter() - t0)
                if rep >= 2:
                    kernel[name].append(mp.kernel_ms()); wall[name].append(dt)
                if rep == 0 and k is None:
                    pairs = got
                if rep == 0 and k == 2:                        # sanity: the ratio test over the two nearest is match()
                    mine = ratio_filter(*got)
                    assert np.array_equal(mine, pairs[np.lexsort((pairs[:, 1], pairs[:, 0]))]), "knn(2) + ratio_filter != match()"
        base = float(np.median(kernel["match"]))
        res = {"pairs": int(len(pairs))}
        for name, k in variants:
            res[name] = {"kernel_ms": stats(kernel[name]), "call_ms": stats(wall[name]), "kernel_vs_match": round(float(np.median(kernel[name])) / base, 3)}
            if k is not None:
                res[name]["instruction_ratio"] = round((32 + max(2 * k - 2, 1)) / 34.0, 3)
        out["sizes"][str(n)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
