"""Restatement of the segmented fit and median and the crafted batches the CPU and GPU tests share.
Nothing here imports the package.  The contract is "segment s gets what the single call gives on that segment alone", so the
restatement slices: it cuts the segment's own two lists, its rows of the pairs and of the mask out of the batch and calls
fit_ref.fit / shift_ref.shift on them.  consensus_ref.gather on the segment's own lists is the gather rule: an index outside
[0, counts[s]) gives four NaN, whatever record of a neighbouring segment lies there.
"""
import numpy as np

import fit_ref as fr
import shift_ref as sr
from consensus_ref import DTYPE_KP


class Batch(object):
    """kp1 / kp2: the records of all segments back to back; counts1: S ints, or None for ONE first list shared by every segment;
    pairs (M, 2) int32, local to the segment; pair_counts (S,) int64; mask None or (M,) uint8"""

    def __init__(self, name, kp1, counts1, kp2, counts2, pairs, pair_counts, mask=None):
        self.name = name
        self.kp1, self.kp2 = np.ascontiguousarray(kp1), np.ascontiguousarray(kp2)
        self.counts1 = None if counts1 is None else np.asarray(counts1, np.int64)
        self.counts2 = np.asarray(counts2, np.int64)
        self.pairs = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
        self.pair_counts = np.asarray(pair_counts, np.int64)
        self.mask = None if mask is None else np.ascontiguousarray(mask).astype(np.uint8)
        self.S = len(self.counts2)
        assert len(self.pair_counts) == self.S and self.pair_counts.sum() == len(self.pairs) and self.counts2.sum() == len(self.kp2)
        assert self.counts1 is None or (len(self.counts1) == self.S and self.counts1.sum() == len(self.kp1))
        assert self.mask is None or self.mask.shape == (len(self.pairs),)

    def rows(self, s):
        r0 = int(self.pair_counts[:s].sum())
        return slice(r0, r0 + int(self.pair_counts[s]))

    def segment(self, s):
        """(kp1_s, kp2_s, pairs_s, mask_s): what the single call would be given"""
        o2 = int(self.counts2[:s].sum())
        kp2 = self.kp2[o2:o2 + int(self.counts2[s])]
        if self.counts1 is None:
            kp1 = self.kp1
        else:
            o1 = int(self.counts1[:s].sum())
            kp1 = self.kp1[o1:o1 + int(self.counts1[s])]
        r = self.rows(s)
        return kp1, kp2, self.pairs[r], None if self.mask is None else self.mask[r]

    def with_mask(self, mask, name=None):
        return Batch(name or self.name + "+mask", self.kp1, self.counts1, self.kp2, self.counts2, self.pairs, self.pair_counts, mask)

    def shared(self):
        """The same matches against ONE first list: the first lists concatenated, every in-range i moved by its segment's offset,
        every out-of-range i kept out of range (negative as it is, the others beyond the whole list).  Every row gathers what it
        gathered before, so every result is the one of the batch with separate lists."""
        assert self.counts1 is not None
        pairs = self.pairs.copy()
        n1 = len(self.kp1)
        for s in range(self.S):
            r, c, off = self.rows(s), int(self.counts1[s]), int(self.counts1[:s].sum())
            i = pairs[r, 0].astype(np.int64)
            pairs[r, 0] = np.where(i < 0, i, np.where(i < c, i + off, n1 + (i - c))).astype(np.int32)
        return Batch(self.name + " [shared]", self.kp1, None, self.kp2, self.counts2, pairs, self.pair_counts, self.mask)


def from_segments(name, segs):
    """segs: (kp1, kp2, pairs) or (kp1, kp2, pairs, mask) per segment; a mask of None among masks means all ones"""
    segs = [tuple(s) + (None,) * (4 - len(s)) for s in segs]
    any_mask = any(s[3] is not None for s in segs)
    kp1 = np.concatenate([s[0] for s in segs]) if segs else np.zeros(0, DTYPE_KP)
    kp2 = np.concatenate([s[1] for s in segs]) if segs else np.zeros(0, DTYPE_KP)
    pairs = np.concatenate([np.asarray(s[2], np.int32).reshape(-1, 2) for s in segs]) if segs else np.zeros((0, 2), np.int32)
    mask = None
    if any_mask:
        mask = np.concatenate([np.ones(len(s[2]), np.uint8) if s[3] is None else np.asarray(s[3]).astype(np.uint8) for s in segs])
    return Batch(name, kp1, [len(s[0]) for s in segs], kp2, [len(s[1]) for s in segs], pairs, [len(s[2]) for s in segs], mask)


# ---------------------------------------------------------------------------------------------- the restatement
def fit_batch(batch, blocks=0):
    """(S, 20) float64: fit_ref.fit on every segment's own lists"""
    out = np.empty((batch.S, 20), np.float64)
    for s in range(batch.S):
        kp1, kp2, pairs, mask = batch.segment(s)
        out[s] = fr.fit(kp1, kp2, pairs, mask, blocks)
    return out


def shift_batch(batch, tol=None):
    """out float32 (S, 6), counts int64 (S, 2), keep bool (M,) or None: shift_ref.shift on every segment's own lists"""
    out = np.empty((batch.S, 6), np.float32)
    counts = np.zeros((batch.S, 2), np.int64)
    keep = None if tol is None else np.zeros(len(batch.pairs), bool)
    for s in range(batch.S):
        kp1, kp2, pairs, mask = batch.segment(s)
        out[s], counts[s], k = sr.shift(kp1, kp2, pairs, mask, tol)
        if tol is not None:
            keep[batch.rows(s)] = k
    return out, counts, keep


def same_bits64(got, want):
    return fr.same_bits(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1))


def same_bits32(got, want):
    return sr.same_bits(np.asarray(got).reshape(-1), np.asarray(want).reshape(-1))


# ---------------------------------------------------------------------------------------------- crafted batches
_CACHE = {}


def cached(fn):
    def get():
        if fn.__name__ not in _CACHE:
            _CACHE[fn.__name__] = fn()
        return _CACHE[fn.__name__]
    get.__name__ = fn.__name__
    return get


def case_segment(M, seed, outliers=0.1, extent=16384.0):
    kp1, kp2, pairs, truth = fr.make_case(max(M, 4), seed, outliers, extent)
    return kp1, kp2, pairs[:M]


EDGE_SIZES = (0, 1, 2, 3, 4, 5, 18, 255, 256, 257, 513, 1000)


@cached
def edge_batch():
    return from_segments("edge", [case_segment(M, 300 + M) for M in EDGE_SIZES])


@cached
def large_batch():
    """B_s = 256 and a second row on some lanes only (70 001 = 65 536 + 4 465), between a segment without a pair and one of three"""
    return from_segments("large", [case_segment(0, 41), case_segment(70001, 7), case_segment(3, 42)])


LEAK_SEGMENTS, LEAK_IN_RANGE, LEAK_OUT = 5, 10, 12


def leak_displacement(s):
    return np.float32(s + 0.25), np.float32(-s - 0.5)


@cached
def leak_batch():
    """Every in-range pair of segment s has the displacement (s + 0.25, -s - 0.5) exactly.  LEAK_OUT further rows, more than the
    in-range ones, have i = counts1[s] or j = -1: read across the segment's bounds they would name the first record of the next
    first list or the last record of the previous second list, which no pair of their own segment names and which would give a
    displacement of 1e6.  Dictated: median (s + 0.25, -s - 0.5), n = LEAK_IN_RANGE."""
    segs = []
    for s in range(LEAK_SEGMENTS):
        rng = np.random.default_rng(900 + s)
        n1, n2 = LEAK_IN_RANGE + 4, LEAK_IN_RANGE + 6
        dx, dy = leak_displacement(s)
        kp1, kp2 = np.zeros(n1, DTYPE_KP), np.zeros(n2, DTYPE_KP)
        i = 1 + rng.permutation(n1 - 1)[:LEAK_IN_RANGE]                 # record 0 of the first list is the trap
        j = rng.permutation(n2 - 1)[:LEAK_IN_RANGE]                     # the last record of the second list is the trap
        x0 = rng.integers(0, 64, LEAK_IN_RANGE).astype(np.float32); y0 = rng.integers(0, 64, LEAK_IN_RANGE).astype(np.float32)
        kp1["x"][i] = x0; kp1["y"][i] = y0
        kp2["x"][j] = x0 + dx; kp2["y"][j] = y0 + dy                    # small integers plus a quarter: exact in float32
        kp1["x"][0] = -1e6; kp1["y"][0] = -1e6                          # x1 - (-1e6)
        kp2["x"][n2 - 1] = 1e6; kp2["y"][n2 - 1] = 1e6                  # 1e6 - x0
        rows = [(int(a), int(b)) for a, b in zip(i, j)]
        rows += [(n1, int(j[k % LEAK_IN_RANGE])) for k in range(LEAK_OUT // 2)]
        rows += [(int(i[k % LEAK_IN_RANGE]), -1) for k in range(LEAK_OUT - LEAK_OUT // 2)]
        order = rng.permutation(len(rows))
        segs.append((kp1, kp2, np.asarray(rows, np.int32)[order]))
    return from_segments("leak", segs)


@cached
def degenerate_batch():
    """ordinary, collinear (status 2), ordinary, two pairs (status 2), ordinary"""
    kp1, kp2, pairs = case_segment(20, 52)
    kp1, kp2 = kp1.copy(), kp2.copy()
    t = np.arange(20, dtype=np.float32)
    kp1["x"][pairs[:, 0]] = 3.0 * t + 1.0; kp1["y"][pairs[:, 0]] = 2.0 * t - 5.0
    kp2["x"][pairs[:, 1]] = 3.0 * t + 4.5; kp2["y"][pairs[:, 1]] = 2.0 * t + 0.25
    return from_segments("degenerate", [case_segment(50, 51), (kp1, kp2, pairs), case_segment(300, 53), case_segment(2, 54),
                                        case_segment(40, 55)])


MASKED_SIZES = (300, 200, 257)


@cached
def masked_batch():
    """a random mask, and the mask of the middle segment all zero: EMPTY between two OK ones"""
    b = from_segments("masked", [case_segment(M, 60 + k) for k, M in enumerate(MASKED_SIZES)])
    mask = (np.random.default_rng(61).random(len(b.pairs)) < 0.6).astype(np.uint8)
    mask[mask != 0] = np.random.default_rng(62).integers(1, 256, int(mask.sum()))          # any non-zero byte counts
    mask[b.rows(1)] = 0
    return b.with_mask(mask, "masked")


VALUE_SIZES = (257, 1000)


@cached
def value_batch():
    """every kind of shift_ref.value_sets at n = 257 and n = 1000, as segments of one batch"""
    segs, names = [], []
    for n in VALUE_SIZES:
        for name, dx in sorted(sr.value_sets(n, 70 + n).items()):
            segs.append(sr.lists_from_displacements(dx, seed=n + len(name)))
            names.append((name, n))
    b = from_segments("value", segs)
    b.kinds = names
    return b


@cached
def keep_batch():
    """for the keep mask: a segment with a tied middle (tol = 0 keeps something), one whose x median is NaN (lo = -inf, hi = +inf:
    it keeps nothing), one whose x median is +inf, a segment without a pair and two ordinary ones"""
    kp1, kp2, pairs = case_segment(500, 81)
    kp1, kp2 = kp1.copy(), kp2.copy()
    sel = pairs[np.arange(500) % 5 != 0]
    kp1["x"][sel[:, 0]] = 100.0; kp1["y"][sel[:, 0]] = 200.0; kp2["x"][sel[:, 1]] = 102.0; kp2["y"][sel[:, 1]] = 199.0
    big = np.float32(3e38)
    i1, i2 = np.zeros(6, DTYPE_KP), np.zeros(6, DTYPE_KP)
    i1["x"] = [-big, -big, big, big, 0, 0]; i2["x"] = [big, big, -big, -big, 1, 2]
    i2["y"] = [1, 2, 3, 4, 5, 6]
    idx = np.arange(6, dtype=np.int32); ip = np.stack([idx, idx], axis=1)
    return from_segments("keep", [(kp1, kp2, pairs), (i1, i2, ip[:4]), case_segment(257, 82), (i1, i2, ip[:3]), case_segment(0, 83),
                                  case_segment(18, 84)])


def crafted_batches():
    return [edge_batch(), large_batch(), leak_batch(), degenerate_batch(), masked_batch(), value_batch()]


def cases_batch(limit=5000):
    """the entries of fit_ref.CASES up to `limit` pairs as the segments of one batch"""
    return from_segments("cases", [case_segment(M, seed, outl, ext) for M, seed, outl, ext in fr.CASES if M <= limit])
