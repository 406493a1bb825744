"""numpy restatement of MatchPlan.match_window_batch, by slicing, and the crafted batches the CPU and
GPU tests share.  Nothing here imports the package or the oracle.

Contract: the lists and counts are match_batch's (tests/match_batch_ref.py); segment s gets window_ref.match(kp1_s, kp2_s, window,
shift_s, mutual, float32(ratio ** 2)) -- the rule of tests/window_ref.py over the candidates inside the window -- with indices
local to the segment.  The result is (pairs (M, 2) int32, pair_counts (S,) int64): segments in order, ascending i inside a segment.
A query emits at most one pair, so this fixes the array completely.
"""
import numpy as np

import match_batch_ref as mb
import match_cases as mc
import window_ref as wr

INF = float("inf")


def shifts_of(window_shift, S):
    """(S, 2) float32 from one (sx, sy) or an (S, 2) array"""
    sh = np.asarray(window_shift, np.float32)
    if sh.shape == (2,):
        sh = np.broadcast_to(sh, (S, 2))
    assert sh.shape == (S, 2)
    return sh


def match_window_batch(kp1, counts1, kp2, counts2, window, window_shift=(0.0, 0.0), ratio=None, mutual=False):
    th = mb.threshold(ratio)
    segs = mb.segments(kp1, counts1, kp2, counts2)
    sh = shifts_of(window_shift, len(segs))
    rows = []
    for (a, b), s in zip(segs, sh):
        r = wr.match(a, b, window, (s[0], s[1]), mutual=mutual, ratio_th=th)
        r = r[np.argsort(r[:, 0], kind="stable")]
        assert (np.diff(r[:, 0]) > 0).all()                          # i is unique per pair
        rows.append(r)
    pairs = np.concatenate(rows + [np.zeros((0, 2), np.int32)]).astype(np.int32)
    return pairs, np.array([len(r) for r in rows], np.int64).reshape(-1)


class WBatch(mb.Batch):
    """One match_window_batch call: a match_batch_ref.Batch with a window and shifts"""

    def __init__(self, name, pairs, window, shifts=(0.0, 0.0), shared=None, ratio=None, mutual=False):
        mb.Batch.__init__(self, name, pairs, shared=shared, ratio=ratio, mutual=mutual)
        self.window, self.shifts = window, shifts

    def reference(self, mutual=None, window=None, ratio=-1):
        return match_window_batch(self.kp1, self.counts1, self.kp2, self.counts2, self.window if window is None else window, self.shifts,
                                  self.ratio if ratio == -1 else ratio, self.mutual if mutual is None else mutual)


# ---------------------------------------------------------------------------------------------- lists
def lists(n1, n2, rng, origin=(0.0, 0.0), extent=(120.0, 90.0), shift=(0.0, 0.0), a=None):
    """Two lists for finite windows, as window_ref.crafted makes them but for any sizes: random descriptors, half of min(n1, n2)
    elements of the second list within +-6 of a descriptor of the first and at that keypoint's position plus `shift` (a quarter
    exactly, the rest within +-1.5 px), one exact duplicate of such an element on its twin's position (the tie rule decides),
    every other keypoint at an independent uniform position in origin + [0, extent)."""
    f = np.float32
    if a is None:
        a = mc.records(rng.integers(0, 256, (n1, 128), dtype=np.uint8))
        a["x"] = f(origin[0]) + (rng.random(n1) * extent[0]).astype(f); a["y"] = f(origin[1]) + (rng.random(n1) * extent[1]).astype(f)
    n1 = len(a)
    b = mc.records(rng.integers(0, 256, (n2, 128), dtype=np.uint8))
    b["x"] = f(origin[0]) + (rng.random(n2) * extent[0]).astype(f); b["y"] = f(origin[1]) + (rng.random(n2) * extent[1]).astype(f)
    shared = min(n1, n2) // 2
    idx = rng.permutation(n1)[:shared]
    b["desc"][:shared] = np.clip(a["desc"][idx].astype(int) + rng.integers(-6, 7, (shared, 128)), 0, 255).astype(np.uint8)
    noise = rng.uniform(-1.5, 1.5, (shared, 2)).astype(f)
    noise[::4] = 0
    b["x"][:shared] = a["x"][idx] + f(shift[0]) + noise[:, 0]
    b["y"][:shared] = a["y"][idx] + f(shift[1]) + noise[:, 1]
    if shared + 1 < n2 and shared > 0:
        b[shared + 1] = b[shared - 1]
    return a, b


EDGE_QUERIES = (0, 1, 2, 255, 256, 257, 511, 512, 513, 2)          # both sides of a chunk of 256 queries and of a block of 512 slots
EDGE_LISTS = (129, 0, 1, 63, 64, 65, 128, 129, 1, 0)                # both sides of a tile of 64 elements, 0 and 1
ONE_SPOT = (600, 200)                                               # several chunks of one cell, several tiles of one cell


def edge_batch(window=INF, seed=61):
    """loop and block edges; the last segment has every keypoint of both lists on ONE position"""
    rng = np.random.default_rng(seed)
    segs = [lists(n1, n2, rng) for n1, n2 in zip(EDGE_QUERIES, EDGE_LISTS)]
    a, b = lists(ONE_SPOT[0], ONE_SPOT[1], rng)
    a["x"] = 40.25; a["y"] = 33.5; b["x"] = 40.25; b["y"] = 33.5
    return WBatch("loop and block edges, window %r" % (window,), segs + [(a, b)], window)


LEAK_COUNTS = (257, 130, 513, 64)
LEAK_WINDOW = 4.0


def leak_parts(seed=62):
    """Segment isolation.  Segment s has the queries a_s; its list b_s holds, in shuffled order, a partner for every query of a_s
    (descriptor within +-6, position within +-1.5 px) and an EXACT copy -- descriptor and position -- of every query of a_(s-1) and
    of a_(s+1) (cyclically), but of no query of a_s.  So for every query of segment s its exact descriptor sits inside the
    window, at the query's own position, in the lists of segments s - 1 and s + 1 and not in list s: a scan, a clamp or a cell
    range that reaches into a neighbour's records answers with that copy (distance 0) instead of the partner.
    Returns ([(a_s, b_s)], [partner index of every query of a_s in b_s])."""
    rng = np.random.default_rng(seed)
    S = len(LEAK_COUNTS)
    qs = []
    for s, n in enumerate(LEAK_COUNTS):
        a = mc.records(rng.integers(0, 256, (n, 128), dtype=np.uint8))
        a["x"] = (rng.random(n) * 120).astype(np.float32); a["y"] = (rng.random(n) * 90).astype(np.float32)
        qs.append(a)
    segs, partner = [], []
    for s in range(S):
        own = qs[s].copy()
        own["desc"] = np.clip(own["desc"].astype(int) + rng.integers(-6, 7, own["desc"].shape), 0, 255).astype(np.uint8)
        own["x"] += rng.uniform(-1.5, 1.5, len(own)).astype(np.float32); own["y"] += rng.uniform(-1.5, 1.5, len(own)).astype(np.float32)
        b = np.concatenate([own, qs[s - 1], qs[(s + 1) % S]])
        perm = rng.permutation(len(b))
        inv = np.empty(len(b), np.int64); inv[perm] = np.arange(len(b))
        segs.append((qs[s], b[perm]))
        partner.append(inv[:len(own)])
    return segs, partner


def leak_batch(shared=False):
    """the leak lists with their own first lists, or (shared) with ONE first list, the concatenation of all a_s: the queries of
    a_s then find their partner in segment s, their exact copy in segments s - 1 and s + 1, and nothing elsewhere"""
    segs, _ = leak_parts()
    if shared:
        return WBatch("segment isolation, shared reference", segs, LEAK_WINDOW, shared=np.concatenate([a for a, _ in segs]))
    return WBatch("segment isolation", segs, LEAK_WINDOW)


def extreme_positions(a, b):
    """the last six keypoints of both lists at NaN, +-inf and +-1e30 coordinates (the positions of tests/test_gpu_match_window.py)"""
    n = len(a) - 6
    a["x"][n:] = [np.nan, 1e30, -1e30, 7.0, np.inf, 1e30]; a["y"][n:] = [5.0, 1e30, 3.0, np.nan, 2.0, -1e30]
    n = len(b) - 6
    b["x"][n:] = [1e30, np.nan, -1e30, np.inf, 7.0, 1e30]; b["y"][n:] = [1e30, 5.0, 3.0, 2.0, np.nan, -1e30]
    return a, b


GRID_MAXES = (0, 1, 2, 3, 7, 256)


def grid_batch(seed=63):
    """neighbouring segments whose extents are 0 .. 100, 1e6 .. 1e6 + 50, a single point, one with NaN, +-inf and +-1e30
    coordinates among ordinary ones, and an empty one; then an ordinary one again"""
    rng = np.random.default_rng(seed)
    near = lists(300, 320, rng, extent=(100.0, 100.0))
    far = lists(280, 300, rng, origin=(1e6, 1e6), extent=(50.0, 50.0))
    point = lists(70, 90, rng)
    for l in point:
        l["x"] = 12.5; l["y"] = 7.75
    wild = extreme_positions(*lists(260, 270, rng, extent=(100.0, 100.0)))
    empty = lists(0, 0, rng)
    again = lists(150, 140, rng, extent=(100.0, 100.0))
    return WBatch("per-segment grids", [near, far, point, wild, empty, again], 2.5)


def rule_batch(ratio, n1=12):
    """the prescribed-distance lists of match_cases as segments of one call, on positions that make a finite window bite:
    critical (dist1, dist2) pairs either side of float32(ratio ** 2) and dist2 == 0 spread over match_cases.SPOTS (three queries
    of four see the planted elements, the others a few far candidates or none), tied minima in different cells"""
    th = mb.threshold(ratio)
    cases = mc.ratio_cases(th, n1, seed=31, n2=65, extra=mc.ONE_EXTRA if th == 1 else ())[::2]
    zeros = [c for c in mc.extreme_cases(n1) if ("zero" in c.name and "n2=130" in c.name) or "lone element" in c.name][:10]
    segs = [mc.spread_over_spots(c) for c in cases + zeros]
    ties = [c for c in mc.tie_cases(65, n1) if len(c.planted) > 1][::3]
    segs += [mc.tied_in_different_cells(c) for c in ties]
    return WBatch("the rule, ratio %r" % (ratio,), segs, mc.SPOT_WINDOW, ratio=ratio)


def lone_batch(seed=64):
    """Lone-candidate and no-candidate queries.  The elements of a list stand 50 px apart on a lattice; query 3k and 3k + 1 sit
    within 1 px of element k (exactly ONE candidate for a window of 3: they pair with it whatever the descriptors), query 3k + 2
    sits 25 px away from every element (no candidate: no pair)."""
    rng = np.random.default_rng(seed)
    segs = []
    for n2 in (40, 1, 7):
        b = mc.records(rng.integers(0, 256, (n2, 128), dtype=np.uint8))
        b["x"] = 50.0 * (np.arange(n2) % 8); b["y"] = 50.0 * (np.arange(n2) // 8)
        a = mc.records(rng.integers(0, 256, (3 * n2, 128), dtype=np.uint8))
        k = np.arange(3 * n2) // 3
        off = np.array([0.5, -1.0, 25.0], np.float32)[np.arange(3 * n2) % 3]
        a["x"] = b["x"][k] + off; a["y"] = b["y"][k] + off
        segs.append((a, b))
    return WBatch("lone and no candidates", segs, 3.0)


SHIFTS = np.array([(0.0, 0.0), (3.5, -2.25), (-7.0, 4.0), (0.5, 0.5), (-1.75, -6.0)], np.float32)


def shift_batch(seed=65, mutual=False):
    """every segment's partners lie at their originals plus that segment's own shift, negative and fractional ones included"""
    rng = np.random.default_rng(seed)
    segs = [lists(200 + 30 * s, 260 - 20 * s, rng, shift=SHIFTS[s]) for s in range(len(SHIFTS))]
    return WBatch("per-segment shifts" + (", mutual" if mutual else ""), segs, 2.0, shifts=SHIFTS, mutual=mutual)


MANY = 1100


def many_batch(seed=66):
    """1 100 segments of 0 .. 5 keypoints a side: more than 1 024 blocks and more segments than one pass of the scan"""
    rng = np.random.default_rng(seed)
    n1s = rng.integers(0, 6, MANY); n2s = rng.integers(0, 6, MANY)
    return WBatch("many segments", [lists(int(n1), int(n2), rng, extent=(6.0, 6.0)) for n1, n2 in zip(n1s, n2s)], 2.0)
