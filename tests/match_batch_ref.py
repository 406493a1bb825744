"""numpy restatement of MatchPlan.match_batch, written from the contract text, and the batches the
CPU and GPU tests share.  Nothing here imports the package or the oracle.

Contract: kp2 holds S lists back to back (counts2), kp1 likewise (counts1) or, with counts1 = None, ONE list every segment is
matched against.  Segment s gets the rule of tests/match_cases.py / window_ref.match(a, b, inf) -- nearest and second nearest L1
distance, the earliest index among equal minima, (i, best) emitted iff dist2 != 0 and dist1 / dist2 < float32(ratio ** 2) in
float32, both distances starting at 1e12f; with mutual, i must also be the nearest of j inside the segment, ties to the smallest
i -- with indices local to the segment.  The result is (pairs (M, 2) int32, pair_counts (S,) int64): segments in order,
ascending i inside a segment.  A query emits at most one pair, so this fixes the array completely.
"""
import numpy as np

import match_cases as mc
import window_ref as wr

DEFAULT_RATIO = 0.73                        # par.MatchRatio


def threshold(ratio=None):
    r = DEFAULT_RATIO if ratio is None else ratio
    th = np.float32(r * r)
    if not th <= np.float32(1):
        raise ValueError("ratio ** 2 must be <= 1")
    return th


def segments(kp1, counts1, kp2, counts2):
    """[(a, b)] of the S segment pairs"""
    out, o1, o2 = [], 0, 0
    for s, c2 in enumerate(counts2):
        a = kp1 if counts1 is None else kp1[o1:o1 + counts1[s]]
        out.append((a, kp2[o2:o2 + c2]))
        o1 += 0 if counts1 is None else counts1[s]
        o2 += c2
    assert o2 == len(kp2) and (counts1 is None or o1 == len(kp1))
    return out


def match_batch(kp1, counts1, kp2, counts2, ratio=None, mutual=False):
    th = threshold(ratio)
    rows = [wr.match(a, b, np.inf, mutual=mutual, ratio_th=th) for a, b in segments(kp1, counts1, kp2, counts2)]
    for r in rows:
        assert (np.diff(r[:, 0]) > 0).all()                          # ascending i, one pair a query at most
    pairs = np.concatenate(rows + [np.zeros((0, 2), np.int32)]).astype(np.int32)
    return pairs, np.array([len(r) for r in rows], np.int64).reshape(-1)


def split(pairs, pair_counts):
    """the rows of every segment"""
    edges = np.concatenate([[0], np.cumsum(pair_counts)])
    return [pairs[edges[s]:edges[s + 1]] for s in range(len(pair_counts))]


# ---------------------------------------------------------------------------------------------- batches
class Batch(object):
    """One match_batch call.  dictated: None, or per segment the rows the construction dictates (None where it makes no claim)"""

    def __init__(self, name, pairs, shared=None, ratio=None, mutual=False, dictated=None):
        self.name, self.ratio, self.mutual, self.dictated = name, ratio, mutual, dictated
        self.counts2 = [len(b) for _, b in pairs]
        self.kp2 = np.concatenate([b for _, b in pairs] + [np.zeros(0, mc.DTYPE_KP)])
        if shared is None:
            self.counts1 = [len(a) for a, _ in pairs]
            self.kp1 = np.concatenate([a for a, _ in pairs] + [np.zeros(0, mc.DTYPE_KP)])
        else:
            self.counts1, self.kp1 = None, shared

    def segments(self):
        return segments(self.kp1, self.counts1, self.kp2, self.counts2)

    def args(self):
        return self.kp1, self.counts1, self.kp2, self.counts2

    def reference(self):
        return match_batch(self.kp1, self.counts1, self.kp2, self.counts2, self.ratio, self.mutual)


def planted_lists(n1, n2, rng, a=None):
    """random descriptors with partners planted as window_ref.lists plants them: half of min(n1, n2) elements of the second list
    within +-6 of a descriptor of the first, and one exact duplicate descriptor (tie-breaking matters) where there is room"""
    if a is None:
        a = mc.records(rng.integers(0, 256, (n1, 128), dtype=np.uint8))
    b = mc.records(rng.integers(0, 256, (n2, 128), dtype=np.uint8))
    shared = min(len(a), n2) // 2
    idx = rng.permutation(len(a))[:shared]
    b["desc"][:shared] = np.clip(a["desc"][idx].astype(int) + rng.integers(-6, 7, (shared, 128)), 0, 255).astype(np.uint8)
    if shared + 1 < n2:
        b["desc"][shared + 1] = b["desc"][shared]
    return a, b


EDGE_COUNTS1 = (600, 0, 1, 255, 256, 257, 511, 512, 513)         # 0 and 1, and both sides of a block of 512 queries and of its half
EDGE_COUNTS2 = (0, 1, 2, 63, 64, 65, 130, 257, 320)              # 0 and 1, both sides of a tile of 64, several tiles


def edge_batches(seed=21):
    """segment edges: the two count tables, the tables exchanged, and one segment alone"""
    rng = np.random.default_rng(seed)
    straight = [planted_lists(n1, n2, rng) for n1, n2 in zip(EDGE_COUNTS1, EDGE_COUNTS2)]
    swapped = [planted_lists(n1, n2, rng) for n1, n2 in zip(EDGE_COUNTS2, EDGE_COUNTS1)]
    return [Batch("segment edges", straight), Batch("segment edges, tables exchanged", swapped),
            Batch("one segment", [planted_lists(513, 320, rng)])]


def leak_batch(seed=22):
    """No leak across a boundary.  The queries of segment s are copies of base_s; its list holds an element at distance 100 and
    one at 200 (0.5 < 0.73 ** 2: every query pairs with the first of them) among far ones.  The LAST element of the list before
    and the FIRST of the list after lie at distances 0 and 1 from base_s (cyclically: the first list's first element and the last
    list's last belong to the other end's base), far from their own segment's base: a scan or a clamp that reaches over a
    boundary changes the answer.  Neighbouring segments have different bases and 257 / 513 queries."""
    rng = np.random.default_rng(seed)
    sizes = [65, 130, 257, 64, 5]
    n1s = [257, 513, 257, 513, 257]
    S = len(sizes)
    bases = [mc.make_base(rng) for _ in range(S)]
    for s in range(S):                                               # two random bases are about 16 000 apart
        assert mc.l1(bases[s], bases[(s + 1) % S]) > 9000 and mc.l1(bases[s], bases[s - 1]) > 9000
    spots = [(40, 2), (1, 128), (255, 64), (62, 1), (2, 3)]          # (the element at 100, the element at 200)
    pairs, dictated = [], []
    for s in range(S):
        b = mc.planted(bases[s], sizes[s], {spots[s][0]: 100, spots[s][1]: 200}, rng, far_lo=9000)
        b["desc"][0] = mc.desc_at(bases[s - 1], 1, rng)              # the FIRST of the list after segment s - 1
        b["desc"][-1] = mc.desc_at(bases[(s + 1) % S], 0, rng)       # the LAST of the list before segment s + 1
        assert mc.l1(bases[s], b["desc"][[0, -1]]).min() > 9000
        pairs.append((mc.queries(bases[s], n1s[s]), b))
        dictated.append(np.stack([np.arange(n1s[s]), np.full(n1s[s], spots[s][0])], axis=1).astype(np.int32))
    return Batch("no leak across a boundary", pairs, dictated=dictated)


FOLD_SIZES = (65, 130, 257)


def fold_batch(ratio, n1=3):
    """Partition fold: the tie and placement families of match_cases at 65, 130 and 257 elements as segments of one call.  With
    64 elements a partition the minimum, its tie and the second minimum fall into different partitions.  A ratio above 1 is not
    accepted, so a tie never pairs here: a fold that loses the tie partner, or takes the element one step beyond for the second,
    shows as a pair that must not be (at ratio 1.0 also 1000 / 1001).  The placement lists pair with the planted minimum
    whenever the threshold admits their second distance."""
    th = threshold(ratio)
    pairs, dictated = [], []
    for n2 in FOLD_SIZES:
        for c in mc.tie_cases(n2, n1):
            tied = "constant" in c.name or len(c.planted) > 1        # ("every tile but the first" of two tiles plants ONE minimum)
            pairs.append((c.a, c.b)); dictated.append(mc.Case(c.name, c.a, c.b, th, None if tied else c.planted[0]).expected_rows())
        for c in mc.placement_cases(n2, n1):
            p, q = c.planted if len(c.planted) == 2 else (c.planted[0], None)
            d1 = int(mc.l1(c.a["desc"][0], c.b["desc"][p])); d2 = None if q is None else int(mc.l1(c.a["desc"][0], c.b["desc"][q]))
            best = p if mc.passes(d1, d2, th) else None
            pairs.append((c.a, c.b))
            dictated.append(mc.Case(c.name, c.a, c.b, th, best).expected_rows())
    return Batch("partition fold, ratio %r" % (ratio,), pairs, ratio=ratio, dictated=dictated)


def ratio_batch(ratio, n1=260):
    """every critical (dist1, dist2) of float32(ratio ** 2), one list a segment (both register slots of a lane hold queries)"""
    th = threshold(ratio)
    cases = mc.ratio_cases(th, n1, seed=31, extra=mc.ONE_EXTRA if th == 1 else ())
    return Batch("ratio %r" % (ratio,), [(c.a, c.b) for c in cases], ratio=ratio, dictated=[c.expected_rows() for c in cases])


RATIOS = (0.5, 1.0, None)


def mutual_batches():
    """match_cases.mutual_cases as segments with their own first lists, and ONE first list with duplicates against several lists"""
    cases = mc.mutual_cases()
    own = Batch("mutual, separate first lists", [(c.a, c.b) for c in cases], mutual=True)
    c = cases[11]                                                    # duplicates at (257, 511), a run: both sides of a block's half
    rng = np.random.default_rng(41)
    b = c.b
    lists = [b, b[::-1].copy(), b[:65].copy(), b[:0].copy(), b[70:71].copy(), planted_lists(0, 200, rng, a=c.a)[1], np.concatenate([b, b])]
    shared = Batch("mutual, one shared first list", [(c.a, l) for l in lists], shared=c.a, mutual=True)
    return [own, shared]


def shared_batches(seed=51):
    """one first list against several lists planted from it, a larger call and a smaller one (stale scratch)"""
    rng = np.random.default_rng(seed)
    a = mc.records(rng.integers(0, 256, (600, 128), dtype=np.uint8))
    large = Batch("shared reference", [planted_lists(0, n2, rng, a=a) for n2 in (320, 0, 1, 130, 65, 700)], shared=a)
    a2 = a[:70].copy()
    small = Batch("shared reference, smaller", [planted_lists(0, n2, rng, a=a2) for n2 in (65, 2)], shared=a2)
    return [large, small]


def all_batches():
    """every batch the GPU test runs on crafted lists"""
    out = edge_batches() + [leak_batch()]
    out += [fold_batch(r) for r in (None, 1.0)] + [ratio_batch(r) for r in RATIOS] + mutual_batches() + shared_batches()
    return out
