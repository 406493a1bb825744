#!/usr/bin/env python
"""MatchPlan.match_window_batch against the two forms it stands between: the loop of
match(window=) calls and the brute-force match_batch, on one reference list of n keypoints and S segments of n each, everything
resident in HBM.

    python tools/bench_match_window_batch.py [--cases 64x1000 64x4000 64x16000 16x200000] [--windows 16 64] [--min-window 0.3]
    python tools/bench_match_window_batch.py --align [--align-cases 64x512 16x4096] [--reps 5]

Lists: n reference keypoints uniform in a square frame with the density of 200 000 keypoints in 4096 x 4096; half of every
segment are partners of reference keypoints (descriptor within +-8, position within +-1.5 px), the rest random.  Per (S, n, window)
the three forms alternate in one process after two warm-up rounds, a host clock around each, every form ending in its own
stream synchronisation with the pairs on the host:
    window_batch   match_window_batch(ref, None, segs, [n] * S, window=w)
    window_loop    [match(ref, seg_s, raw_results=True, window=w) for s in range(S)]
    batch          match_batch(ref, None, segs, [n] * S)
The loop and match_batch are code the new call does not touch.  The rows of window_batch are checked against the loop's.

--align: LinearAlign.align_batch_window(frames, 16) against align_batch(frames) and against the loop of
align(f, max_shift=16, estimate="device", median="device"), host frames in and host result out, on the frames of
tools/bench_align_batch.py.

Prints one JSON line; times are median [min, max] in ms of the whole call.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DENSITY = 200000 / 4096.0 ** 2


def stats(v):
    return {"median": round(float(np.median(v)), 3), "min": round(float(min(v)), 3), "max": round(float(max(v)), 3)}


def lists(S, n, dtype_kp):
    side = float(np.sqrt(n / DENSITY))
    rng = np.random.default_rng(1)
    a = np.zeros(n, dtype_kp); a["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    a["x"] = rng.random(n) * side; a["y"] = rng.random(n) * side
    rng2 = np.random.default_rng(2)
    b = np.zeros(S * n, dtype_kp)
    half = n // 2
    for s in range(S):
        perm = rng2.permutation(n)[:half]
        seg = b[s * n:(s + 1) * n]
        seg["desc"][:half] = np.clip(a["desc"][perm].astype(np.int16) + rng2.integers(-8, 9, (half, 128)), 0, 255).astype(np.uint8)
        seg["desc"][half:] = rng2.integers(0, 256, (n - half, 128), dtype=np.uint8)
        seg["x"] = rng2.random(n) * side; seg["y"] = rng2.random(n) * side
        seg["x"][:half] = a["x"][perm] + rng2.uniform(-1.5, 1.5, half); seg["y"][:half] = a["y"][perm] + rng2.uniform(-1.5, 1.5, half)
    return a, b, side


def alternate(forms, min_window, min_reps, check=None):
    """two warm-up rounds (timed to size the windows), then the forms in turn; {name: [ms]}"""
    once, last = {}, {}
    for _ in range(2):
        for name, fn in forms:
            t0 = time.perf_counter(); last[name] = fn(); once[name] = time.perf_counter() - t0
    if check:
        check(last)
    last.clear()
    reps = max(min_reps, int(np.ceil(min_window / min(once.values()))))
    times = {name: [] for name, _ in forms}
    for _ in range(reps):
        for name, fn in forms:
            t0 = time.perf_counter(); r = fn(); times[name].append(1e3 * (time.perf_counter() - t0))
            del r
    return times


def match_leg(args):
    import torch
    import sift_pyocl_amd as sp
    out = {}
    for case in args.cases:
        S, n = (int(v) for v in case.split("x"))
        a, b, side = lists(S, n, sp.MatchPlan.dtype_kp)
        ta = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda(); tb = torch.from_numpy(b.view(np.uint8).reshape(-1)).cuda()
        segs = [tb[s * n * 144:(s + 1) * n * 144] for s in range(S)]
        torch.cuda.synchronize()
        mp = sp.MatchPlan(size=n)
        for w in args.windows:
            forms = (("window_batch", lambda: mp.match_window_batch(ta, None, tb, [n] * S, window=w)),
                     ("window_loop", lambda: [mp.match(ta, seg, raw_results=True, window=w) for seg in segs]),
                     ("batch", lambda: mp.match_batch(ta, None, tb, [n] * S)))
            found = {}

            def check(last):
                rows = [r[np.lexsort((r[:, 1], r[:, 0]))] for r in last["window_loop"]]
                pairs, counts = last["window_batch"]
                assert counts.tolist() == [len(r) for r in rows] and np.array_equal(pairs, np.concatenate(rows)), "match_window_batch != loop"
                found["pairs"], found["batch_pairs"] = int(len(pairs)), int(len(last["batch"][0]))

            times = alternate(forms, args.min_window, args.min_reps, check)
            med = {k: float(np.median(v)) for k, v in times.items()}
            res = {"frame_side": round(side, 1), "reps": len(times["batch"]), "pairs": found["pairs"], "match_batch_pairs": found["batch_pairs"]}
            res.update({k + "_ms": stats(v) for k, v in times.items()})
            res["window_loop_over_window_batch"] = round(med["window_loop"] / med["window_batch"], 3)
            res["batch_over_window_batch"] = round(med["batch"] / med["window_batch"], 3)
            res["window_batch_wholly_below_both"] = bool(max(times["window_batch"]) < min(min(times["window_loop"]), min(times["batch"])))
            out["S=%d n=%d w=%g" % (S, n, w)] = res
            print("S=%d n=%d w=%g: %s" % (S, n, w, json.dumps(res)), file=sys.stderr, flush=True)
        del mp, ta, tb, segs
    return out


def align_leg(args):
    import sift_pyocl_amd as sp
    from scipy.ndimage import gaussian_filter
    out = {}
    for case in args.align_cases:
        S, N = (int(v) for v in case.split("x"))
        rng = np.random.default_rng(0)
        big = gaussian_filter(rng.random((N + 64, N + 64), dtype=np.float32), 2.0).astype(np.float32)
        ref = np.ascontiguousarray(big[20:20 + N, 30:30 + N])
        frames = [np.ascontiguousarray(big[20 + (s % 7 - 3):20 + (s % 7 - 3) + N, 30 + (2 - s % 5):30 + (2 - s % 5) + N]) for s in range(S)]
        la = sp.LinearAlign(ref)
        forms = (("align_batch_window", lambda: la.align_batch_window(frames, 16)),
                 ("align_loop_max_shift", lambda: [la.align(f, max_shift=16, estimate="device", median="device") for f in frames]),
                 ("align_batch", lambda: la.align_batch(frames)))
        worst = {}

        def check(last):
            worst["window_vs_batch"] = float(np.abs(last["align_batch_window"] - last["align_batch"]).max())

        times = alternate(forms, 0.0, args.reps, check)
        med = {k: float(np.median(v)) for k, v in times.items()}
        res = {"ref_keypoints": int(len(la.ref_kp)), "reps": args.reps, "max_abs_difference_window_vs_align_batch": worst["window_vs_batch"]}
        res.update({k + "_ms": stats(v) for k, v in times.items()})
        res["align_batch_over_window"] = round(med["align_batch"] / med["align_batch_window"], 3)
        res["loop_over_window"] = round(med["align_loop_max_shift"] / med["align_batch_window"], 3)
        out["S=%d %dx%d" % (S, N, N)] = res
        print("S=%d %dx%d: %s" % (S, N, N, json.dumps(res)), file=sys.stderr, flush=True)
        del la, frames
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["64x1000", "64x4000", "64x16000", "16x200000"], help="Sxn: segments x keypoints")
    ap.add_argument("--windows", type=float, nargs="+", default=[16.0, 64.0])
    ap.add_argument("--min-window", type=float, default=0.3, help="seconds every timed window must last at least")
    ap.add_argument("--min-reps", type=int, default=5)
    ap.add_argument("--align", action="store_true", help="time align_batch_window instead of the matcher")
    ap.add_argument("--align-cases", nargs="+", default=["64x512", "16x4096"], help="SxN: frames x side")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    if args.align:
        print(json.dumps({"reps": args.reps, "align": align_leg(args)}))
    else:
        print(json.dumps({"min_window_s": args.min_window, "match": match_leg(args)}))


if __name__ == "__main__":
    main()
