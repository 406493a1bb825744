"""Keypoint lists with PRESCRIBED descriptor distances, for the rule both matchers share (matching_cpu.cl:57-109):

    nearest and second nearest L1 distance; among equal minima the earliest index; (i, best) emitted iff
    dist2 != 0 and dist1 / dist2 < ratio_th in float32 (both distances start at 1e12f).

Random descriptors put every distance near 10 900: no (dist1, dist2) comes close to the threshold and a tie for the minimum
never shows (its ratio is 1).  Here every byte of a `base` descriptor is 0 or 255, so a descriptor at ANY L1 distance
0 .. 32 640 from it exists, the query list is n1 copies of `base`, and a list is a set of planted distances among far
elements.  The answer is then all-or-nothing: every query pairs with the same element, or none pairs.

numpy only, deterministic from seeds, nothing here imports the package or the oracle.  The CPU tests
(tests/test_match_cases_host.py) pin the oracle, the numpy restatement (tests/window_ref.py) and the reference's own kernel
(tests/golden/match_crafted.npz) to each other on these lists; the GPU tests (tests/test_gpu_match_cases.py) compare the
kernels with the oracle on the same lists.
"""
import hashlib

import numpy as np

DTYPE_KP = np.dtype([("x", np.float32), ("y", np.float32), ("scale", np.float32), ("angle", np.float32), ("desc", (np.uint8, 128))])
DMAX = 128 * 255                           # 32 640 = 0x7F80: the largest L1 distance of two descriptors
RATIO = np.float32(0.73 * 0.73)            # what MatchPlan.match passes
_INIT = np.float32(1e12)
UNKNOWN = "?"                              # Case.best: the construction makes no claim, the oracle decides


# ---------------------------------------------------------------------------------------------- prescribed distances
def make_base(rng):
    """uint8[128], every byte 0 or 255 (both occur in every dword position)"""
    base = (rng.integers(0, 2, 128) * 255).astype(np.uint8)
    base[:8] = [0, 255, 255, 0, 255, 0, 0, 255]
    return base


def descs_at(base, dists, rng):
    """(n, 128) uint8 descriptors, row k at L1 distance dists[k] from `base` exactly.  The per-byte differences are spread
    irregularly: a cubed uniform draw over a random 70 % of the bytes carries up to three quarters of the distance, the rest is
    poured into the bytes in a random order, each up to 255 -- so some differences are 0 and (from 1 020 on) some are 255, in
    any of the four bytes of a dword, and `base` decides the direction of each |a - b|."""
    d = np.atleast_1d(np.asarray(dists, np.int64))
    assert d.ndim == 1 and (d >= 0).all() and (d <= DMAX).all()
    n = len(d)
    u = rng.random((n, 128)) ** 3 * (rng.random((n, 128)) < 0.7)
    s = u.sum(axis=1)
    s[s == 0] = 1.0
    delta = np.minimum(np.floor(u * (0.75 * d / s)[:, None]), 255).astype(np.int64)
    resid = d - delta.sum(axis=1)                                     # >= 0: the floor never exceeds its share
    order = np.argsort(rng.random((n, 128)), axis=1)
    room = np.take_along_axis(255 - delta, order, axis=1)
    before = np.cumsum(room, axis=1) - room
    add = np.clip(resid[:, None] - before, 0, room)
    np.put_along_axis(delta, order, np.take_along_axis(delta, order, axis=1) + add, axis=1)
    assert (delta.sum(axis=1) == d).all() and delta.min(initial=0) >= 0 and delta.max(initial=0) <= 255
    b = base.astype(np.int64)[None, :]
    return np.where(b == 0, delta, 255 - delta).astype(np.uint8)


def desc_at(base, dist, rng):
    return descs_at(base, [dist], rng)[0]


def l1(base, descs):
    """int64 L1 distances of the rows of `descs` to `base`"""
    return np.abs(np.asarray(descs).astype(np.int64) - np.asarray(base).astype(np.int64)).sum(axis=-1)


def records(descs, x=0.0, y=0.0):
    descs = np.asarray(descs, np.uint8).reshape(-1, 128)
    k = np.zeros(len(descs), DTYPE_KP)
    k["desc"] = descs; k["x"] = x; k["y"] = y; k["scale"] = 1.0
    return k


def queries(base, n1):
    """the query list: n1 copies of `base`"""
    return records(np.repeat(np.asarray(base, np.uint8)[None, :], n1, axis=0))


def far_dists(n, lo, rng):
    """n distances in [lo, DMAX], all of them above every planted one"""
    return rng.integers(min(int(lo), DMAX), DMAX + 1, n)


def planted(base, n2, plant, rng, far_lo=None):
    """a list of n2 elements: element j at distance plant[j] from `base`, every other one far (above the largest planted distance,
    or from `far_lo` on)"""
    lo = (max(plant.values()) + 1 if plant else DMAX // 2) if far_lo is None else far_lo
    d = far_dists(n2, lo, rng)
    for j, v in plant.items():
        d[j] = v
    return records(descs_at(base, d, rng))


def passes(d1, d2, th):
    """the ratio test on two integer distances (None: the 1e12f a missing candidate leaves), in float32"""
    f1 = _INIT if d1 is None else np.float32(d1)
    f2 = _INIT if d2 is None else np.float32(d2)
    with np.errstate(all="ignore"):
        return bool(f2 != 0 and np.float32(f1 / f2) < np.float32(th))


# ---------------------------------------------------------------------------------------------- the threshold edge
def _thin(rows, limit):
    """at most `limit` of the rows, evenly spaced, the first and the last among them"""
    if len(rows) <= limit:
        return rows
    return rows[np.unique(np.linspace(0, len(rows) - 1, limit).round().astype(np.int64))]


def critical_ratio_pairs(th, limit=48):
    """The (d1, d2), 1 <= d2 <= 32 640, d1 = floor(th * d2) + {-1, 0, 1, 2}, 0 <= d1 <= d2, on which a kernel that does not compute
    `f1 / f2 < th` as one correctly rounded float32 division can decide differently:
      exact    the float32 quotient equals th (a quotient off by one ulp lands on the other side), or
      forms    one of  f1 < th * f2,  f1 * (1 / f2) < th,  the binary64 quotient < th  decides differently from it.
    For float32(0.73 ** 2) these are 37 pairs.  Thresholds with a short significand (0.5, 1.0) have an exact quotient for
    thousands of d2: each of the two groups is then thinned to `limit` evenly spaced members (first and last kept)."""
    th = np.float32(th)
    d2 = np.repeat(np.arange(1, DMAX + 1, dtype=np.int64), 4)
    d1 = np.floor(np.float64(th) * d2).astype(np.int64) + np.tile(np.array([-1, 0, 1, 2], np.int64), DMAX)
    ok = (d1 >= 0) & (d1 <= d2)
    d1, d2 = d1[ok], d2[ok]
    f1, f2 = d1.astype(np.float32), d2.astype(np.float32)
    q = f1 / f2
    assert q.dtype == np.float32
    rule = q < th
    forms = (f1 < th * f2) != rule
    forms |= (f1 * (np.float32(1) / f2) < th) != rule
    forms |= (d1.astype(np.float64) / d2.astype(np.float64) < np.float64(th)) != rule
    exact = q == th
    rows = np.stack([d1, d2], axis=1)
    out = np.concatenate([_thin(rows[exact], limit), _thin(rows[forms & ~exact], limit)])
    out = np.unique(out, axis=0)
    return [(int(a), int(b)) for a, b in out]


# ---------------------------------------------------------------------------------------------- where to plant
def edge_positions(n):
    """0, 1, n - 1 and 64k - 1, 64k, 64k + 1 for every k: the tiles are 64 elements and a partition is a whole number of tiles, so
    these lie on both sides of every tile edge and every partition edge whatever the host's partition rule is"""
    pos = {0, 1, n - 1}
    for k in range(64, n + 1, 64):
        pos |= {k - 1, k, k + 1}
    return sorted(p for p in pos if 0 <= p < n)


def placements(n2):
    """[(p_min, p_second)]: neighbours in edge_positions (64k - 1 | 64k: adjacent tiles; 64k | 64k + 1 and 64k + 1 | 64k + 63: one
    tile, for k >= 1 a later tile with everything before it far), the same offset one tile on, and the two ends of the list --
    each in both orders.  n2 == 1: [(0, None)]."""
    if n2 == 1:
        return [(0, None)]
    pos = edge_positions(n2)
    out = []
    for p, q in zip(pos[:-1], pos[1:]):
        out += [(p, q), (q, p)]
    for p in pos:
        if p + 64 < n2:
            out += [(p, p + 64), (p + 64, p)]
    out += [(0, n2 - 1), (n2 - 1, 0)]
    seen, uniq = set(), []
    for e in out:
        if e not in seen:
            seen.add(e); uniq.append(e)
    return uniq


# ---------------------------------------------------------------------------------------------- cases
class Case(object):
    """One matcher call.  best: the list-2 index every query pairs with, None (no pair at all), or UNKNOWN.
    identical: every query is the same record (the result for n1 queries is the result for one, repeated)."""

    def __init__(self, name, a, b, th, best=UNKNOWN, planted=(), identical=True, roi=None, roi_mode=0, mutual=False):
        self.name, self.a, self.b, self.th, self.best = name, a, b, np.float32(th), best
        self.planted, self.identical, self.roi, self.roi_mode, self.mutual = tuple(planted), identical, roi, roi_mode, mutual

    def expected_rows(self, n1=None):
        """(m, 2) int32 from `best` (which must be known)"""
        assert self.best is not UNKNOWN
        n1 = len(self.a) if n1 is None else n1
        if self.best is None:
            return np.zeros((0, 2), np.int32)
        return np.stack([np.arange(n1), np.full(n1, self.best)], axis=1).astype(np.int32)


def _best_of(plant, th):
    """what the rule answers for a list whose smallest distances are the planted ones"""
    order = sorted(plant.items(), key=lambda kv: (kv[1], kv[0]))
    d2 = order[1][1] if len(order) > 1 else None
    return order[0][0] if passes(order[0][1], d2, th) else None


def ratio_cases(th, n1, seed=1, n2=130, extra=()):
    """every critical pair of `th` (and `extra`) planted among far elements, the positions walking through placements(n2)"""
    rng = np.random.default_rng(seed)
    base = make_base(rng)
    a = queries(base, n1)
    pl = placements(n2)
    out = []
    for k, (d1, d2) in enumerate(list(critical_ratio_pairs(th)) + list(extra)):
        p, q = pl[(5 * k) % len(pl)]
        plant = {p: d1, q: d2}
        out.append(Case("ratio th=%r d=(%d, %d) at (%d, %d)" % (float(th), d1, d2, p, q), a, planted(base, n2, plant, rng), th,
                        _best_of(plant, th), (p, q)))
    return out


ONE_EXTRA = [(d - 1, d) for d in (1, 2, 255, 4097, 16385, DMAX)] + [(d, d) for d in (1, 2, 255, 4097, 16385, DMAX)]


def odd_threshold_cases(n1, seed=2):
    """ratio_th = 0, negative, NaN and +inf on a passing pair, a failing pair, a tie, two zeros, a zero and a one-element list"""
    rng = np.random.default_rng(seed)
    base = make_base(rng)
    a = queries(base, n1)
    lists = [("pass", 130, {70: 1000, 3: 4000}), ("fail", 130, {3: 3900, 70: 4000}), ("tie", 130, {64: 500, 63: 500}),
             ("zeros", 130, {129: 0, 0: 0}), ("zero", 130, {5: 0, 100: 9}), ("lone", 1, {0: 777})]
    out = []
    for label, n2, plant in lists:
        b = planted(base, n2, plant, rng)
        order = sorted(plant.items(), key=lambda kv: (kv[1], kv[0]))
        d2 = order[1][1] if len(order) > 1 else None
        for th in (0.0, -0.0, -1.0, np.nan, np.inf, -np.inf):
            best = order[0][0] if passes(order[0][1], d2, th) else None
            out.append(Case("threshold %r on %s" % (th, label), a, b, th, best, tuple(plant)))
    return out


def placement_cases(n2, n1, seed=3):
    """a passing pair (1000 / 4000) and a failing pair (3000 / 4000) at every placement, the rest of the list from 20 000 on"""
    rng = np.random.default_rng(seed + n2)
    base = make_base(rng)
    a = queries(base, n1)
    far = planted(base, n2, {}, rng, far_lo=20000)
    spare = descs_at(base, [1000, 3000, 4000], rng)
    for p, q in placements(n2):
        for label, dmin in (("pass", 0), ("fail", 1)):
            b = far.copy()
            b["desc"][p] = spare[dmin]
            if q is not None:
                b["desc"][q] = spare[2]
            best = p if (q is None or label == "pass") else None
            yield Case("placement n2=%d %s at (%s, %s)" % (n2, label, p, q), a, b, RATIO, best, (p,) if q is None else (p, q))


def tie_cases(n2, n1, seed=4, th=2.0):
    """Ties for the minimum made visible: with ratio_th = 2 a tie (ratio 1) does emit a pair and its second index is the tie-break.
    Two equal minima at every placement; three (a third at the middle or the end of the list); the tie partner only in an
    earlier / only in a later tile while the minimum's own tile holds a slightly larger element; an equal minimum in every tile,
    and in every tile but the first; a list that is one value throughout."""
    rng = np.random.default_rng(seed + n2)
    base = make_base(rng)
    a = queries(base, n1)
    far = planted(base, n2, {}, rng, far_lo=20000)
    same = descs_at(base, [1000] * 8 + [1001], rng)              # eight DIFFERENT descriptors at one distance, one a step beyond

    def make(label, idx, plus=None):
        b = far.copy()
        for k, j in enumerate(idx):
            b["desc"][j] = same[k % 8]
        if plus is not None:
            b["desc"][plus] = same[8]
        return Case("tie n2=%d %s %s" % (n2, label, list(idx)[:4]), a, b, th, min(idx), tuple(idx))

    for p, q in placements(n2):
        if q is None:
            continue
        yield make("two", (p, q))
        for r in (n2 // 2, n2 - 1):
            if r not in (p, q) and p < q:
                yield make("three", (p, q, r))
        # the minimum's own tile offers 1001 as second: the tie partner is the other tile's only word
        if abs(p - q) >= 64:
            plus = p + 1 if (p + 1) // 64 == p // 64 and p + 1 < n2 and p + 1 != q else p - 1
            if 0 <= plus < n2 and plus != q and plus // 64 == p // 64:
                yield make("partner in the %s tile," % ("earlier" if q < p else "later"), (p, q), plus)
    tiles = list(range(0, n2, 64))
    if len(tiles) > 1:
        yield make("every tile", [t + (5 * k + 3) % min(64, n2 - t) for k, t in enumerate(tiles)])
        yield make("every tile but the first", [t + (7 * k + 1) % min(64, n2 - t) for k, t in enumerate(tiles)][1:])
    for value in (1000, 1, DMAX):
        b = records(descs_at(base, [value] * n2, rng))
        yield Case("tie n2=%d constant %d" % (n2, value), a, b, th, 0, (0,))


def extreme_cases(n1, seed=5):
    rng = np.random.default_rng(seed)
    base = make_base(rng)
    a = queries(base, n1)
    out = []

    def add(label, n2, plant, th, far_lo=None):
        out.append(Case("extreme %s th=%r" % (label, float(th)), a, planted(base, n2, plant, rng, far_lo), th, _best_of(plant, th), tuple(plant)))

    for n2 in (2, 130, 320):
        add("zero and 700, n2=%d" % n2, n2, {n2 - 1: 0, 0: 700}, RATIO)
        add("zero and 1, n2=%d" % n2, n2, {0: 0, n2 - 1: 1}, RATIO)
        for th in (RATIO, 1.0, 2.0, np.inf):
            add("two zeros, n2=%d" % n2, n2, {0: 0, n2 - 1: 0}, th)
            add("tie at 1, n2=%d" % n2, n2, {n2 - 1: 1, 0: 1}, th)
    for d in (0, 1, 1000, DMAX):                                      # one element: dist2 stays 1e12, the pair always comes out
        for th in (RATIO, 1.0, 2.0):
            add("lone element at %d" % d, 1, {0: d}, th)
    for n2 in (2, 65, 320):                                           # the largest distance, just under the packed key's sentinel
        for th in (RATIO, 1.0, 2.0):
            add("all at 32640, n2=%d" % n2, n2, {j: DMAX for j in range(n2)}, th)
            for p, q in ((0, n2 - 1), (n2 - 1, 0)):
                plant = {j: DMAX for j in range(n2)}
                plant[p] = DMAX - 1
                add("32639 at %d against 32640, n2=%d" % (p, n2), n2, plant, th)
    return out


SIZES = (1, 2, 63, 64, 65, 257, 320, 1500)
PLAIN_FAMILIES = (["ratio default", "ratio 0.5", "ratio 1.0", "odd thresholds", "extremes"] + ["placement %d" % n for n in SIZES] +
                  ["ties %d" % n for n in SIZES if n > 1])


def family(name, n1):
    """the cases of one family of PLAIN_FAMILIES (a plain match(kp1, kp2, ratio_th): no mask, not mutual), as an iterator: the
    lists of 1 500 are built one at a time"""
    if name == "ratio default":
        return iter(ratio_cases(RATIO, n1, seed=11))
    if name == "ratio 0.5":
        return iter(ratio_cases(np.float32(0.5), n1, seed=12))
    if name == "ratio 1.0":
        return iter(ratio_cases(np.float32(1.0), n1, seed=13, extra=ONE_EXTRA))
    if name == "odd thresholds":
        return iter(odd_threshold_cases(n1))
    if name == "extremes":
        return iter(extreme_cases(n1))
    kind, n2 = name.rsplit(" ", 1)
    return {"placement": placement_cases, "ties": tie_cases}[kind](int(n2), n1)


GOLDEN_FAMILIES = ("ratio default", "ratio 0.5", "ratio 1.0", "odd thresholds", "extremes", "ties 2", "ties 65", "ties 257", "ties 320")


def digest(cases):
    """SHA-256 over the inputs of the cases: both lists' bytes and the threshold's"""
    h = hashlib.sha256()
    for c in cases:
        h.update(np.ascontiguousarray(c.a).tobytes()); h.update(np.ascontiguousarray(c.b).tobytes()); h.update(np.float32(c.th).tobytes())
    return h.hexdigest()


# ---------------------------------------------------------------------------------------------- reverse direction (mutual)
def mutual_cases(seed=6, n1=600, n2=130):
    """Duplicates in list 1: queries i_a < i_b (and, in the `run` form, every query from i_a on) are `base`, the others random
    records far from everything.  All the copies pair with the planted minimum p; in the reverse scan they tie for the nearest of
    p, nearest[p] must be the earliest, so with mutual exactly (i_a, p) survives among them."""
    rng = np.random.default_rng(seed)
    base = make_base(rng)
    b = planted(base, n2, {70: 100, 3: 5000}, rng, far_lo=9000)
    out = []
    for i_a, i_b in [(0, 1), (0, 599), (255, 256), (256, 257), (63, 64), (257, 511), (511, 512), (512, 599), (1, 320), (598, 599)]:
        for run in (False, True):
            a = records(rng.integers(0, 256, (n1, 128), dtype=np.uint8))
            a["desc"][[i_a, i_b]] = base
            if run:
                a["desc"][i_a:] = base
            out.append(Case("mutual duplicates at (%d, %d)%s" % (i_a, i_b, ", a run" if run else ""), a, b, RATIO, UNKNOWN, (i_a, i_b),
                            identical=False, mutual=True))
    return out


# ---------------------------------------------------------------------------------------------- positions for finite windows
SPOTS = np.array([(10.25, 20.5), (210.25, 20.5), (10.25, 320.5), (510.0, 510.0)], np.float32)
SPOT_WINDOW = 3.0


def spread_over_spots(case):
    """(a, b) of the case with every keypoint on one of a few positions 200 px apart: the planted elements and most of the rest on
    spot 0, every fifth far element on spot 1 or 2; three queries of four on spot 0 (their candidates hold the planted ones), the
    others on spot 1 (a few far candidates) or spot 3 (none).  For a window of SPOT_WINDOW."""
    a, b = case.a.copy(), case.b.copy()
    sb = np.zeros(len(b), np.int64)
    free = np.setdiff1d(np.arange(len(b)), np.array(case.planted, np.int64))
    sb[free[4::5]] = 1 + np.arange(len(free[4::5])) % 2
    sa = np.zeros(len(a), np.int64)
    sa[3::4] = np.where(np.arange(len(sa[3::4])) % 2 == 0, 1, 3)
    a["x"], a["y"] = SPOTS[sa, 0], SPOTS[sa, 1]
    b["x"], b["y"] = SPOTS[sb, 0], SPOTS[sb, 1]
    return a, b


def tied_in_different_cells(case):
    """(a, b) of a tie case for a window of SPOT_WINDOW: queries and far elements at x = 0, the tied elements alternately at
    x = +2 and x = -2, the EARLIEST at +2 -- all within the window, in two cells of side 3 from x0 = -2, the earliest index in
    the later cell (a kernel that keeps the first it meets in cell order answers with the wrong one)."""
    a, b = case.a.copy(), case.b.copy()
    for k, j in enumerate(sorted(case.planted)):
        b["x"][j] = 2.0 if k % 2 == 0 else -2.0
    return a, b


# ---------------------------------------------------------------------------------------------- flags (region of interest)
ROI = np.array([[1, 0, 1, 1]], np.int8)          # x in [0, 1): on the mask; [1, 2): masked out; x >= 4: beyond the array
X_ON, X_OFF, X_BEYOND = 0.5, 1.5, 9.5


def flag_cases(n1, seed=7):
    """roi_mode 2 (a keypoint off the mask takes no part) and 1 (`matching_valid`: a list element off the mask is at distance 0, a
    query inside the array and off the mask is dropped); the x position of a keypoint chooses its flag."""
    rng = np.random.default_rng(seed)
    base = make_base(rng)
    out = []

    def add(label, n2, plant, mode, off=(), beyond=(), th=RATIO, q_off=None, best=UNKNOWN, mutual=False):
        a = queries(base, n1)
        a["x"] = X_ON; a["y"] = 0.25
        identical = q_off is None
        if q_off is not None:
            a["x"][q_off(np.arange(n1)) == 1] = X_OFF
            a["x"][q_off(np.arange(n1)) == 2] = X_BEYOND
        b = planted(base, n2, plant, rng, far_lo=20000)
        b["x"] = X_ON; b["y"] = 0.25
        b["x"][list(off)] = X_OFF
        b["x"][list(beyond)] = X_BEYOND
        out.append(Case("flags mode %d %s" % (mode, label), a, b, th, best, tuple(plant), identical, ROI, mode, mutual))

    # the planted minimum excluded: the second becomes the best, the third decides the ratio
    for n2, p, q, r in ((320, 5, 200, 100), (320, 191, 192, 0), (320, 100, 101, 319), (1500, 1499, 0, 700), (65, 64, 63, 0)):
        add("minimum %d excluded, passes" % p, n2, {p: 500, q: 1500, r: 4000}, 2, off=[p], best=q)
        add("minimum %d excluded, fails" % p, n2, {p: 500, q: 1500, r: 1600}, 2, off=[p], best=None)
        add("minimum %d beyond the array, passes" % p, n2, {p: 500, q: 1500, r: 4000}, 2, beyond=[p], best=q)
    # whole aligned runs excluded: a run of 256 (a whole partition of 1500 elements) and of 64 (a whole tile)
    for n2, lo, hi in ((1500, 256, 512), (1500, 0, 256), (1500, 1280, 1500), (320, 128, 192), (320, 0, 64), (320, 256, 320), (512, 256, 512)):
        run = list(range(lo, hi))
        inside, outside, other = lo + 7, (hi + 3) % n2, (lo - 5) % n2
        add("run [%d, %d) excluded with the minimum in it" % (lo, hi), n2, {inside: 300, outside: 1000, other: 4000}, 2, off=run, best=outside)
        add("run [%d, %d) excluded with the second in it" % (lo, hi), n2, {outside: 1000, inside: 1100, other: 4000}, 2, off=run, best=outside)
        add("run [%d, %d) excluded, fails" % (lo, hi), n2, {inside: 300, outside: 3000, other: 4000}, 2, off=run, best=None)
    # every element excluded (every partial is empty), every element but one
    for n2 in (1, 64, 320, 1500):
        add("every element of %d excluded" % n2, n2, {0: 10}, 2, off=range(n2), best=None)
        add("every element of %d excluded, mutual" % n2, n2, {0: 10}, 2, off=range(n2), best=None, mutual=True)
        if n2 > 1:
            add("all of %d but the last excluded" % n2, n2, {n2 - 1: 9000}, 2, off=range(n2 - 1), best=n2 - 1)
            # a threshold above 1 lets 1e12 / 1e12 through: the pair is (i, 0), the index the scan starts from
            add("every element of %d excluded, ratio 2" % n2, n2, {0: 10}, 2, off=range(n2), th=2.0, best=0)
    # matching_valid: a forced zero before and after a true zero (dist1 == dist2 == 0: nothing); alone it takes every query
    for n2, z, f in ((320, 100, 20), (320, 100, 250), (320, 63, 64), (320, 64, 63), (2, 0, 1), (2, 1, 0)):
        add("forced zero %d, true zero %d" % (f, z), n2, {z: 0, f: 6000}, 1, off=[f], best=None)
        add("forced zero %d, true zero %d, ratio 2" % (f, z), n2, {z: 0, f: 6000}, 1, off=[f], th=2.0, best=None)
        add("forced zero %d, minimum 40 at %d" % (f, z), n2, {z: 40, f: 6000}, 1, off=[f], best=f)
        add("forced zero %d beyond the array, minimum 40 at %d" % (f, z), n2, {z: 40, f: 6000}, 1, beyond=[f], best=f)
        add("two forced zeros" , n2, {z: 40, f: 6000}, 1, off=[f], beyond=[z], best=None)
    # dropped queries between kept ones (mode 1 keeps a query beyond the array, mode 2 drops it)
    for mode in (1, 2):
        for mutual in (False, True):
            add("every third query off the mask, every third beyond%s" % (", mutual" if mutual else ""), 320, {191: 1000, 192: 4000}, mode,
                q_off=lambda i: i % 3, mutual=mutual)
            add("only the last query kept%s" % (", mutual" if mutual else ""), 320, {191: 1000, 192: 4000}, mode,
                q_off=lambda i: (i != i.max()).astype(int), mutual=mutual)
    return out


def flags_restated(case):
    """(a', b', rows of a', rows of b') without flags: what the masked call means for lists whose queries all carry ONE descriptor.
    An excluded element or a dropped query is deleted; an element at forced distance 0 gets the queries' descriptor.  Which
    keypoint gets which flag is stated once, in tests/roi_ref.py."""
    import roi_ref
    return roi_ref.restated(case.a, case.b, case.roi, case.roi_mode)
