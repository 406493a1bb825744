"""Restatement of the segmented consensus filter and the crafted batches the CPU and GPU tests share.
Nothing here imports the package.  The contract is "segment s gets what the single call gives on that segment alone", so the
restatement slices: estimate_batch_ref.Batch.segment(s) cuts the segment's own two lists and its rows of the pairs out of the batch
and consensus_ref.consensus runs on them with the n_hyp, tol and seed of the whole call.  consensus_ref.gather on the segment's own
lists is the gather rule, and sampling `mod len(pairs_s)` with the row's position inside the segment is what the slice gives.
"""
import numpy as np

import consensus_ref as cr
import estimate_batch_ref as eb


def consensus_batch(batch, n_hyp=2048, tol=3.0, seed=0):
    """dict(mask uint8 (M,), models float32 (S, 6) with NaN rows where there is no winner, winners int32 (S,), winner_votes int32
    (S,), votes_all int32 (S, H), models_all float32 (S, H, 6), valid bool (S, H))"""
    S, M = batch.S, len(batch.pairs)
    out = dict(mask=np.zeros(M, np.uint8), models=np.full((S, 6), np.nan, np.float32), winners=np.full(S, -1, np.int32),
               winner_votes=np.zeros(S, np.int32), votes_all=np.zeros((S, n_hyp), np.int32),
               models_all=np.full((S, n_hyp, 6), np.nan, np.float32), valid=np.zeros((S, n_hyp), bool))
    for s in range(S):
        kp1, kp2, pairs, _ = batch.segment(s)
        r = cr.consensus(kp1, kp2, pairs, n_hyp, tol, seed)
        out["mask"][batch.rows(s)] = r["mask"]
        out["winners"][s], out["winner_votes"][s] = r["winner"], r["winner_votes"]
        out["votes_all"][s], out["models_all"][s], out["valid"][s] = r["votes_all"], r["models_all"], r["valid"]
        if r["model"] is not None:
            out["models"][s] = r["model"]
    return out


def same_bits(got, want):
    """float32 arrays equal as bit patterns, NaN compared as "is NaN" """
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    if got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


# ---------------------------------------------------------------------------------------------- crafted batches
edge_batch, leak_batch, large_batch = eb.edge_batch, eb.leak_batch, eb.large_batch

#: (pairs, inlier share) per segment of tile_batch: more than one tile, exactly one tile, one row into the second tile, less than
#: a tile, two segments that are not active, and a fifth tile of one row; every segment has a map of its own (its seed)
TILE_SEGMENTS = ((1500, 0.6), (1024, 0.4), (1025, 0.9), (300, 0.5), (2, 0.0), (0, 0.0), (4097, 0.3))


@eb.cached
def tile_batch():
    segs = []
    for k, (M, w) in enumerate(TILE_SEGMENTS):
        kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(M, w, 700 + k)
        segs.append((kp1, kp2, pairs))
    return eb.from_segments("tile", segs)


MANY_SEGMENTS = 2048


@eb.cached
def many_batch():
    """the leak batch's segments among one-pair segments, 2048 tiles in all: the size at which the vote grid of a small n_hyp
    drops to one chunk of hypotheses"""
    leak = leak_batch()
    one = eb.case_segment(1, 77)
    segs = [one] * (MANY_SEGMENTS - leak.S)
    for s in range(leak.S):
        segs.insert(400 * s + 7, leak.segment(s)[:3])
    return eb.from_segments("many", segs)


def crafted_batches():
    return [edge_batch(), leak_batch(), large_batch(), tile_batch()]


def leak_model(s):
    """the map every in-range row of segment s of leak_batch follows exactly"""
    dx, dy = eb.leak_displacement(s)
    return np.array([1, 0, dx, 0, 1, dy], np.float32)


def permuted(batch, order, name=None):
    """the segments of `batch` in another order"""
    return eb.from_segments(name or batch.name + " [permuted]", [batch.segment(s)[:3] for s in order])
