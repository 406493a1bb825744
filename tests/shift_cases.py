"""Crafted match sets for the two median selects (k_shift.hpp: five launches, a serial 256-bin scan per workgroup; eb_shift_kernel
of k_estimate_batch.hpp: one workgroup per segment, a wave-parallel scan, four bins per lane).
Both are a radix select of four 8-bit digits on the order keys of the contract that tests/shift_ref.py restates, for four selectors
(axis x lo / hi), and both have to give the same bits.

Every result here is DICTATED by construction -- the set is built around the element that was placed in the middle -- and never
read off shift_ref.shift.  A median of an even count is the one float32 sum and halving of the two dictated middles; where a
family is about that arithmetic the bits are written out by hand.  A dictated keep mask comes from exact rational arithmetic on
the float32 values, rounded once (within()).  The y axis of a case carries ANOTHER case's values of the same count, shuffled on
its own, so that a selector that reads the other axis' keys, prefix or bins gives a wrong answer: no case has the same multiset on
both axes.  x0 = y0 = 0, so a displacement is the stored position; +-inf comes only from the overflow of positions of +-3e38.

Families (all_cases() holds 2197 cases; the largest has 1203 rows):
    every_digit       for each level p = 0..3 and digit d = 0..255 a key L whose digit at level p is d, with L - 1, L + 1, the keys
                      one digit below and above d at that level under the same prefix, and L +- 2 where that leaves fewer than two
                      a side: five values with lo = hi = L, and a second instance of six values (one more below) with hi = L and
                      lo = L - 1.  The digits under level p are all 0x00 where d % 8 == 0 and all 0xff where d % 8 == 7, so that
                      L - 1 / L + 1 lie across a carry.  Every key is finite, within [0x00800000, 0xff7fffff]
    divergence        six values, the middle two prescribed: equal; far apart from digit 0, 1, 2, 3 on; adjacent at digit 3;
                      adjacent across a carry (...00ff | ...0100, ...00ffff | ...010000, ...ffffff | the next top byte), so that
                      lo finishes on digits 255 and hi on digits 0; -0.0 | +0.0; the largest negative subnormal | the smallest
                      positive one
    ranks             n = 1..9, 255, 256, 257, 511, 512, 513, 1023, 1024 consecutive distinct keys that run across a byte carry
                      near the middle: a rank off by one changes the bits.  The same counts again, on other keys, with unused rows
                      in between -- mask 0, i = -1, i = n1, j = n2, a NaN or infinite coordinate in either list -- whose
                      displacements, were they counted, lie below every used one: M != n and the ranks follow n.  Up to 1024 - n
                      unused rows, at least one of each kind; n = 1023 and 1024 so have 1031 and 1032 rows
    runs              the middle inside a run of 2, 255, 256, 257 and 600 equal values, at the run's first and at its last
                      element, the other values far away (the bins before the run's are empty at every level) or on the adjacent
                      keys (occupied), on both sides of zero; a run of 600 around the middle of 1024; two runs on adjacent keys
                      with the middle on the seam.  The first or last element of a run of 600 is the middle of 1203 values: the
                      one family above 1024 rows
    top_bins          2^127, 1.5 * 2^127, FLT_MAX and +inf (top digit 255, the digit of the unused rows' key 0xffffffff) as lo, hi
                      and median, with more unused rows than used ones, and the mirror image in bin 0
    median_arithmetic even n: a sum that is inexact (a tie that rounds down, and one that rounds up), sums that overflow to +inf and
                      -inf, -FLT_MAX with +FLT_MAX, subnormal middles of 1 and 2 and of 2 and 3 units of 2^-149 (both halves are
                      ties: 2 units), (-0.0, -0.0) and (-0.0, +0.0); odd n with a middle of -0.0, 3e38 and a subnormal
    keep              displacements at median +- tol and one float32 step inside and outside; tol 0 (median +0.0 keeps -0.0), 0.5,
                      2^-149, inf (a finite median keeps an infinite displacement), 2^24 with a median of 1.0 (dx - mdx rounds
                      onto tol from beyond it); a NaN median (lo -inf, hi +inf) and +-inf medians keep nothing.  Each scenario
                      once on x and once on y, the other axis all within tol; masked rows AT the median, void rows, NaN rows
    lane_edges        for each level and the lanes 0, 1, 62, 63 of the wave scan: a rank equal to the lane's first running count
                      (excl) and to its last (incl - 1).  At the top level that needs n <= 3 with the middle in digits 0..3 / 252..255

numpy only, deterministic, nothing here imports the package.  tests/test_shift_cases_host.py proves on the CPU that every family
reaches what it names, on a plain model of both scans, and that each listed fault of the select changes a dictated result;
tests/test_gpu_shift_cases.py runs every case through siftmi_match_shift, siftmi_match_shift_batch and the two methods.
"""
import zlib
from fractions import Fraction

import numpy as np

import shift_ref as sr
from consensus_ref import gather

F32 = np.float32
U32 = np.uint32
BIG = F32(3e38)
KEY_MIN, KEY_MAX = 0x00800000, 0xFF7FFFFF            # the keys of -FLT_MAX and +FLT_MAX
UNIT = 2.0 ** -149                                   # the smallest subnormal
_CACHE = {}

#: why a row is not used.  The first three are the rows no record stands behind, the rest have one non-finite coordinate
KINDS = ("mask 0", "i = -1", "i = n1", "j = n2", "NaN x0", "inf y1", "-inf x1", "NaN y0")
#: non-keep families run with these in turn, so that both forms write a keep mask for them too (checked against the restatement)
TOLS = (None, 0.0, 0.5, np.inf)


def cached(fn):
    def get():
        if fn.__name__ not in _CACHE:
            _CACHE[fn.__name__] = fn()
        return _CACHE[fn.__name__]
    get.__name__, get.__doc__ = fn.__name__, fn.__doc__
    return get


def val(k):
    """float32 value(s) of order key(s), written here a second time: a key with the top bit set is a non-negative float's bits with
    the sign bit flipped, any other the complement of a negative float's bits"""
    k = np.asarray(k, np.uint64)
    b = np.where(k >> np.uint64(31), k ^ np.uint64(0x80000000), k ^ np.uint64(0xFFFFFFFF))
    return b.astype(U32).view(F32)


def keyof(v):
    b = np.asarray(v, F32).view(U32).astype(np.uint64)
    return np.where(b >> np.uint64(31), b ^ np.uint64(0xFFFFFFFF), b ^ np.uint64(0x80000000)).astype(np.int64)


def bits(v):
    return np.asarray(v, F32).view(U32)


def f32(b):
    return np.asarray(b, U32).view(F32)


def finite_key(k):
    return KEY_MIN <= k <= KEY_MAX


def halve(lo, hi, n):
    """the contract's median of the two dictated middles: lo itself for an odd count, else one float32 sum and one halving"""
    lo, hi = F32(lo), F32(hi)
    if n & 1:
        return lo
    with np.errstate(all="ignore"):
        return F32(F32(lo + hi) * F32(0.5))


def within(v, m, tol):
    """keep's test on one axis in exact arithmetic: |fl(v - m)| <= tol, fl the one rounding to float32; False for a median that
    is not finite"""
    v, m = float(F32(v)), float(F32(m))
    if not np.isfinite(m):
        return False
    if not np.isfinite(v):
        return tol == np.inf
    exact = Fraction(v) - Fraction(m)
    d = float(exact)
    assert Fraction(d) == exact                         # the difference of two float32 of these sets is a binary64 value
    with np.errstate(all="ignore"):
        return bool(abs(F32(d)) <= F32(tol))


class Axis(object):
    """the displacement values of the used rows on one axis and what was placed in their middle"""

    def __init__(self, values, lo, hi, med=None, claims=None):
        self.values = np.array(values, F32).reshape(-1)
        self.n = len(self.values)
        self.lo, self.hi = F32(lo), F32(hi)
        self.med = halve(lo, hi, self.n) if med is None else f32(med).reshape(())[()]
        self.claims = dict(claims or {})

    def negated(self):
        return Axis(-self.values, -self.hi, -self.lo, claims=self.claims)

    def multiset(self):
        return np.sort(bits(self.values)).tobytes()


def from_keys(keys, lo, hi, **kw):
    return Axis(val(keys), val(lo), val(hi), **kw)


class Proto(object):
    """a case before it has its y axis: the x axis, the unused rows as (kind, x value, y value) -- the displacement the row would
    have were it counted -- and tol.  `y`: an axis of its own (the keep family)"""

    def __init__(self, family, name, x, unused=(), tol=None, y=None, keep_family=False):
        self.family, self.name, self.x, self.unused, self.tol, self.y, self.keep_family = family, name, x, list(unused), tol, y, keep_family


class Case(object):
    """dx, dy float32 (M,): the displacement of every row (of an unused row: what it would be); kind: None for a used row, else one
    of KINDS; mask None or uint8 (M,); tol None or a float; n; want float32 (6,) in the order of siftmi_match_shift's `out` (NaN: a
    NaN); keep bool (M,) and n_keep where the family dictates them, else None."""

    def __init__(self, proto, y, seed):
        x = proto.x
        assert x.n == y.n and x.multiset() != y.multiset(), proto.name
        self.family, self.name, self.tol = proto.family, "%s/%s" % (proto.family, proto.name), proto.tol
        self.x, self.y, self.n = x, y, x.n
        rng = np.random.default_rng(seed)
        n, u = x.n, len(proto.unused)
        M = n + u
        # the unused rows spread evenly among the used ones
        is_unused = np.zeros(M, bool)
        if u:
            is_unused[np.unique(((np.arange(u) + 0.5) * M / u).astype(int))] = True
            assert is_unused.sum() == u, proto.name
        self.dx, self.dy = np.zeros(M, F32), np.zeros(M, F32)
        self.dx[~is_unused] = x.values[rng.permutation(n)]
        self.dy[~is_unused] = y.values[rng.permutation(n)]
        self.kind = [None] * M
        for r, (kind, tx, ty) in zip(np.flatnonzero(is_unused), proto.unused):
            assert kind in KINDS
            self.kind[r], self.dx[r], self.dy[r] = kind, tx, ty
        self.mask = None
        if any(k == "mask 0" for k in self.kind):
            self.mask = rng.integers(1, 256, M).astype(np.uint8)            # any non-zero byte counts
            self.mask[[r for r in range(M) if self.kind[r] == "mask 0"]] = 0
        self.used = ~is_unused
        self.want = np.array([x.med, y.med, x.lo, x.hi, y.lo, y.hi], F32)
        self.keep = self.n_keep = None
        if proto.keep_family:
            self.keep = np.array([bool(self.used[r]) and within(self.dx[r], x.med, self.tol) and within(self.dy[r], y.med, self.tol)
                                  for r in range(M)], bool)
            self.n_keep = int(self.keep.sum())

    @property
    def M(self):
        return len(self.dx)

    def lists(self):
        """(kp1, kp2, pairs) from shift_ref.lists_from_displacements, then: an infinite displacement as the overflow of -+3e38
        positions, a non-finite coordinate or an index outside its list for the unused rows"""
        if "_lists" not in self.__dict__:
            fx, fy = np.isfinite(self.dx), np.isfinite(self.dy)
            kp1, kp2, pairs = sr.lists_from_displacements(np.where(fx, self.dx, F32(0)), np.where(fy, self.dy, F32(0)),
                                                          seed=zlib.crc32(self.name.encode()) & 0xFFFF)
            i, j = pairs[:, 0].copy(), pairs[:, 1].copy()
            for r in np.flatnonzero(~fx):
                s = F32(np.sign(self.dx[r]))
                kp1["x"][i[r]] = -s * BIG; kp2["x"][j[r]] = s * BIG
            for r in np.flatnonzero(~fy):
                s = F32(np.sign(self.dy[r]))
                kp1["y"][i[r]] = -s * BIG; kp2["y"][j[r]] = s * BIG
            for r, kind in enumerate(self.kind):
                if kind == "i = -1":
                    pairs[r, 0] = -1
                elif kind == "i = n1":
                    pairs[r, 0] = len(kp1)
                elif kind == "j = n2":
                    pairs[r, 1] = len(kp2)
                elif kind == "NaN x0":
                    kp1["x"][i[r]] = np.nan
                elif kind == "inf y1":
                    kp2["y"][j[r]] = np.inf
                elif kind == "-inf x1":
                    kp2["x"][j[r]] = -np.inf
                elif kind == "NaN y0":
                    kp1["y"][i[r]] = np.nan
            pts = gather(kp1, kp2, pairs)
            used = sr.used_pairs(pts, self.mask)
            assert np.array_equal(used, self.used), self.name
            with np.errstate(all="ignore"):
                gx, gy = pts[:, 2] - pts[:, 0], pts[:, 3] - pts[:, 1]
            assert np.array_equal(bits(gx[used]), bits(self.dx[used])) and np.array_equal(bits(gy[used]), bits(self.dy[used])), self.name
            self._lists = (kp1, kp2, pairs)
        return self._lists

    def segment(self):
        """(kp1, kp2, pairs, mask): a segment for estimate_batch_ref.from_segments"""
        return self.lists() + (self.mask,)


def unused_rows(count, trap_x, trap_y, kinds=KINDS):
    """`count` unused rows of every kind in turn; were one counted, its displacement would be (trap_x, trap_y)"""
    return [(kinds[k % len(kinds)], trap_x, trap_y) for k in range(count)]


# ---------------------------------------------------------------------------------------------- every_digit
def digit_key(p, d):
    """a finite key whose digit at level p (0: the top byte) is d; the digits under it all 0x00 / 0xff for d % 8 == 0 / 7"""
    t = [0x3C + (d & 0x7F), (d * 37 + 11) & 0xFF, (d * 101 + 7 * p + 3) & 0xFF, (d * 59 + 5) & 0xFF]
    if not (p == 0 and d in (0, 255)) and d % 8 in (0, 7):
        for q in range(p + 1, 4):
            t[q] = 0x00 if d % 8 == 0 else 0xFF
    t[p] = d
    if p == 0 and d <= 1:                           # top digit 0 (L itself, or the neighbour below it): finite from 0x0080... on
        t[1] |= 0x80
    if p == 0 and d >= 254:                         # top digit 255: finite up to 0xff7f...
        t[1] &= 0x7F
    return (t[0] << 24) | (t[1] << 16) | (t[2] << 8) | t[3]


def _pad(side, L, sign, need):
    k = 2
    while len(side) < need:
        c = L + sign * k
        assert finite_key(c)
        if c not in side:
            side.append(c)
        k += 1
    return side


def digit_sets(p, d):
    """(L, keys of the odd instance: L in the middle of five, keys of the even instance: one more below, hi = L)"""
    L = digit_key(p, d)
    step = 1 << (8 * (3 - p))
    low = [L - 1] + ([L - step] if d > 0 and L - step != L - 1 else [])
    high = [L + 1] + ([L + step] if d < 255 and L + step != L + 1 else [])
    low, high = _pad(low, L, -1, 2), _pad(high, L, +1, 2)
    odd = low + [L] + high
    even = _pad(list(low), L, -1, 3) + [L] + high
    for keys in (odd, even):
        assert len(set(keys)) == len(keys) and all(finite_key(k) for k in keys), (p, d)
    return L, odd, even


@cached
def every_digit():
    out = []
    for inst in ("lo", "hi"):
        for p in range(4):
            for d in range(256):
                L, odd, even = digit_sets(p, d)
                x = from_keys(odd, L, L, claims=dict(level=p, digit=d, sel="lo")) if inst == "lo" else \
                    from_keys(even, L - 1, L, claims=dict(level=p, digit=d, sel="hi"))
                out.append(Proto("every_digit", "%s p=%d d=%d" % (inst, p, d), x, tol=TOLS[(p + d) % 4]))
    return out


# ---------------------------------------------------------------------------------------------- divergence
#: name -> (key of lo, key of hi, the first digit at which they differ; 4: none)
DIVERGENCE = {
    "equal": (0xC1234567, 0xC1234567, 4),
    "far from digit 0": (0x41C80000, 0xC2480000, 0),
    "far from digit 1": (0xC1100000, 0xC1F00000, 1),
    "far from digit 2": (0xC1201000, 0xC120F000, 2),
    "far at digit 3": (0xC1200010, 0xC12000F0, 3),
    "adjacent at digit 3": (0xC1200040, 0xC1200041, 3),
    "carry into digit 2": (0xC12000FF, 0xC1200100, 2),
    "carry into digit 1": (0xC120FFFF, 0xC1210000, 1),
    "carry into digit 0": (0xC1FFFFFF, 0xC2000000, 0),
    "-0.0 | +0.0": (0x7FFFFFFF, 0x80000000, 0),
    "subnormals either side of zero": (0x7FFFFFFE, 0x80000001, 0),
}


@cached
def divergence():
    out = []
    for k, (name, (a, b, level)) in enumerate(DIVERGENCE.items()):
        keys = [0x12345678 + k, a - 2, a, b, b + 2, 0xEDCBA987 - k]
        out.append(Proto("divergence", name, from_keys(keys, a, b, claims=dict(diverge=level)), tol=TOLS[k % 4]))
    return out


# ---------------------------------------------------------------------------------------------- ranks
RANK_COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 255, 256, 257, 511, 512, 513, 1023, 1024)


def rank_unused(n):
    return max(len(KINDS), min(n, 1024 - n))


@cached
def ranks():
    out = []
    for k, n in enumerate(RANK_COUNTS):
        # positive floats across ...1fffff | ...200000 and negative ones across 0x3e7fffff | 0x3e800000, the carry at the middle
        for name, base, u in (("plain", 0xC1200000 - (n >> 1) - (n & 1), 0), ("unused rows between", 0x3E800000 - (n >> 1), rank_unused(n))):
            keys = base + np.arange(n, dtype=np.int64)
            x = from_keys(keys, keys[(n - 1) >> 1], keys[n >> 1], claims=dict(consecutive=True))
            trap = val(0x20000000 + n)                                      # below every used value on either axis
            out.append(Proto("ranks", "n=%d %s" % (n, name), x, unused=unused_rows(u, trap, trap), tol=TOLS[(k + (u > 0)) % 4]))
    return out


# ---------------------------------------------------------------------------------------------- runs
RUNS = (2, 255, 256, 257, 600)
RUN_KEYS = (0xC1400080, 0x3EBFFF80)                  # 12.000122 and about -12.0


def _others(V, count, side, occupied):
    """`count` distinct keys below (side = -1) or above V: on the adjacent keys, or far away under other top digits"""
    k = np.arange(1, count + 1, dtype=np.int64)
    return V + side * k if occupied else V + side * (0x10000000 + k * 0x00010000)


@cached
def runs():
    out, turn = [], 0
    for R in RUNS:
        for where in ("first", "last"):
            for occupied in (False, True):
                V = RUN_KEYS[turn % 2]
                turn += 1
                # first: the rank of lo is the number of values below, a = R + 1, and 2 lie above; last: 2 below, R + 1 above
                a, b = (R + 1, 2) if where == "first" else (2, R + 1)
                keys = np.concatenate([_others(V, a, -1, occupied), np.full(R, V, np.int64), _others(V, b, +1, occupied)])
                assert len(keys) == 2 * R + 3 and (len(keys) - 1) >> 1 == (a if where == "first" else a + R - 1)
                x = from_keys(keys, V, V, claims=dict(run=R, where=where, occupied=occupied))
                out.append(Proto("runs", "%d %s %s %s" % (R, where, "occupied" if occupied else "empty", "+" if V >> 31 else "-"), x,
                                 tol=TOLS[turn % 4]))
    V = RUN_KEYS[1]
    keys = np.concatenate([_others(V, 212, -1, True), np.full(600, V, np.int64), _others(V, 212, +1, False)])
    out.append(Proto("runs", "600 around the middle of 1024", from_keys(keys, V, V, claims=dict(run=600, where="inside")), tol=0.0))
    for R, V in ((2, RUN_KEYS[0]), (256, RUN_KEYS[1]), (2, 0x7FFFFFFF)):          # the last: -0.0 -0.0 +0.0 +0.0
        keys = np.concatenate([np.full(R, V, np.int64), np.full(R, V + 1, np.int64)])
        out.append(Proto("runs", "seam of two runs of %d at %08x" % (R, V), from_keys(keys, V, V + 1, claims=dict(run=R, where="seam")), tol=0.0))
    return out


# ---------------------------------------------------------------------------------------------- top_bins
P127, P127_15, FLT_MAX = val(0xFF000000)[()], val(0xFF400000)[()], val(KEY_MAX)[()]
INF = F32(np.inf)
#: name -> (values, lo, hi).  Even counts: FLT_MAX + inf = inf; 2^127 + 1.5 * 2^127 overflows to inf
TOP = {
    "median FLT_MAX": ([1.0, P127, FLT_MAX, INF, INF], FLT_MAX, FLT_MAX),
    "median inf": ([P127, FLT_MAX, INF, INF, INF], INF, INF),
    "median 2^127": ([-1.0, 0.5, P127, FLT_MAX, INF], P127, P127),
    "lo FLT_MAX, hi inf": ([1.0, P127, FLT_MAX, INF, INF, INF], FLT_MAX, INF),
    "lo 2^127, hi 1.5 * 2^127": ([-5.0, 1.0, P127, P127_15, FLT_MAX, INF], P127, P127_15),
    "lo 1.5 * 2^127, hi FLT_MAX": ([P127, P127, P127_15, FLT_MAX, INF, INF], P127_15, FLT_MAX),
}


@cached
def top_bins():
    out = []
    for k, (name, (values, lo, hi)) in enumerate(TOP.items()):
        x = Axis(values, lo, hi)
        assert x.med == INF or len(values) & 1
        for mirror in (False, True):
            ax = x.negated() if mirror else x
            trap = F32(-0.25 if mirror else 0.25)                           # finite and on the far side of the middle
            out.append(Proto("top_bins", name + (" mirrored" if mirror else ""), ax, unused=unused_rows(len(values) + 3, trap, trap),
                             tol=(np.inf, None)[(k + mirror) % 2]))
    return out


# ---------------------------------------------------------------------------------------------- median_arithmetic
SUB = lambda units: F32(units * UNIT)               # noqa: E731
#: name -> (values in ascending order with the middle(s) in the middle, the median's bits)
ARITHMETIC = {
    "tie rounds down": ([0.5, f32(0x3F800000), f32(0x3F800001), 7.0], 0x3F800000),          # 2 + 2^-23 -> 2
    "tie rounds up": ([0.5, f32(0x3F800001), f32(0x3F800002), 7.0], 0x3F800002),            # 2 + 3 * 2^-23 -> 2 + 2^-21
    "sum overflows to +inf": ([1.0, 3e38, 3.2e38, 3.3e38], 0x7F800000),
    "sum overflows to -inf": ([-3.3e38, -3.2e38, -3e38, 1.0], 0xFF800000),
    "-FLT_MAX with +FLT_MAX": ([-np.inf, -FLT_MAX, FLT_MAX, np.inf], 0x00000000),
    "subnormal 1 and 2 units": ([-1.0, SUB(1), SUB(2), 1.0], 0x00000002),                   # 1.5 units: a tie, to even
    "subnormal 2 and 3 units": ([-1.0, SUB(2), SUB(3), 1.0], 0x00000002),                   # 2.5 units: a tie, to even
    "subnormal -2 and -3 units": ([-1.0, SUB(-3), SUB(-2), 1.0], 0x80000002),
    "-0.0 and -0.0": ([-1.0, -0.0, -0.0, 1.0], 0x80000000),
    "-0.0 and +0.0": ([-1.0, -0.0, 0.0, 1.0], 0x00000000),
    "odd, -0.0": ([-1.0, -0.0, 1.0], 0x80000000),
    "odd, 3e38": ([1.0, 3e38, 3.2e38], int(bits(F32(3e38)))),
    "odd, -3e38": ([-3.2e38, -3e38, 1.0], int(bits(F32(-3e38)))),
    "odd, subnormal 3 units": ([-1.0, SUB(3), 1.0], 0x00000003),
}


@cached
def median_arithmetic():
    out = []
    for k, (name, (values, med)) in enumerate(ARITHMETIC.items()):
        v = np.array(values, F32)
        n = len(v)
        x = Axis(v, v[(n - 1) >> 1], v[n >> 1], med=med)
        assert np.array_equal(np.sort(keyof(v)), keyof(v)), name
        out.append(Proto("median_arithmetic", name, x, tol=TOLS[k % 4]))
    return out


# ---------------------------------------------------------------------------------------------- keep
def _step(v, towards):
    return np.nextafter(F32(v), F32(towards))


def _around(m, tol):
    """median m in the middle of: m -+ tol, and one float32 step outside and inside each"""
    a, b = F32(m - tol), F32(m + tol)
    return [_step(a, -np.inf), a, _step(a, np.inf), F32(m), _step(b, -np.inf), b, _step(b, np.inf)]


#: name -> (values in ascending order, tol, the values of them that are within tol of the median -- written out, and checked
#: against within())
KEEP = {
    "tol 0.5 about 10": (_around(10.0, 0.5), 0.5, _around(10.0, 0.5)[1:6]),
    "tol 0.5 about -10": (_around(-10.0, 0.5), 0.5, _around(-10.0, 0.5)[1:6]),
    "tol 0.5, even count": ([9.0, 9.5, 10.5, 11.0], 0.5, [9.5, 10.5]),
    "tol 0 about +0.0": ([-1.0, SUB(-1), -0.0, 0.0, SUB(1), 1.0, 2.0], 0.0, [-0.0, 0.0]),
    "tol 2^-149": ([SUB(1), SUB(2), SUB(3), SUB(4), SUB(5)], UNIT, [SUB(2), SUB(3), SUB(4)]),
    # 16777218 - 1 = 2^24 + 1 is a tie and rounds to 2^24 = tol: kept; 16777220 - 1 rounds to 16777220.  -16777216 - 1 likewise
    "difference rounds onto tol": ([-16777218.0, -16777216.0, -16777214.0, 1.0, 16777214.0, 16777218.0, 16777220.0], 2.0 ** 24,
                                   [-16777216.0, -16777214.0, 1.0, 16777214.0, 16777218.0]),
    "tol inf, infinite displacements": ([-np.inf, -5.0, 2.0, 7.0, np.inf], np.inf, [-np.inf, -5.0, 2.0, 7.0, np.inf]),
    "tol inf, NaN median": ([-np.inf, -np.inf, np.inf, np.inf], np.inf, []),
    "tol inf, +inf median": ([1.0, np.inf, np.inf], np.inf, []),
    "tol inf, -inf median": ([-np.inf, -np.inf, 1.0], np.inf, []),
    "tol 0.5, +inf median": ([1.0, np.inf, np.inf], 0.5, []),
}
KEEP_BENIGN = F32(3.25)


@cached
def keep():
    out = []
    for name, (values, tol, kept) in KEEP.items():
        v = np.array(values, F32)
        n = len(v)
        assert np.array_equal(np.sort(keyof(v)), keyof(v)), name
        scen = Axis(v, v[(n - 1) >> 1], v[n >> 1])
        assert sorted(bits([w for w in v if within(w, scen.med, tol)]).tolist()) == sorted(bits(np.array(kept, F32)).tolist()), name
        benign = Axis(np.full(n, KEEP_BENIGN), KEEP_BENIGN, KEEP_BENIGN)
        # a masked row AT both medians, rows without a record, rows with a NaN coordinate: none is kept
        mx = scen.med if np.isfinite(scen.med) else F32(1.0)
        for axis in "xy":
            tx, ty = (mx, KEEP_BENIGN) if axis == "x" else (KEEP_BENIGN, mx)
            unused = unused_rows(6, tx, ty, ("mask 0", "i = -1", "mask 0", "NaN x0", "j = n2", "inf y1"))
            x, y = (scen, benign) if axis == "x" else (benign, scen)
            out.append(Proto("keep", "%s on %s" % (name, axis), x, unused=unused, tol=tol, y=y, keep_family=True))
    return out


# ---------------------------------------------------------------------------------------------- lane_edges
EDGE_LANES = (0, 1, 62, 63)


def edge_key(p, d):
    """digit d at level p under the prefix c1 20 33, finite whatever d"""
    fill = 0x95 if (p == 0 and d == 0) else 0x15 if (p == 0 and d == 255) else 0x55
    t = [0xC1, 0x20, 0x33][:p] + [d] + [fill, 0x55, 0x55][:3 - p]
    return (t[0] << 24) | (t[1] << 16) | (t[2] << 8) | t[3]


@cached
def lane_edges():
    """At level p the keys differ in digit p alone, so the rank that reaches the level is the rank in the whole set.
    excl: the rank equals the number of keys under the lane's four bins; incl - 1: the middle is the lane's last key"""
    out = []
    for p in range(4):
        for lane in EDGE_LANES:
            d0 = 4 * lane
            for edge in ("excl", "incl - 1"):
                if edge == "excl":
                    if lane == 0:
                        digits, lo, hi = [1], 1, 1                                          # n = 1: rank 0
                    else:
                        digits = [d0 - 1, d0 + 2, d0 + 3 if lane == 63 else d0 + 4]         # n = 3: rank 1, one key below the lane
                        lo = hi = d0 + 2
                elif lane == 63:
                    digits, lo, hi = [d0 - 1, d0 + 2], d0 - 1, d0 + 2                       # n = 2: hi has rank 1 = n - 1
                else:
                    below = [d0 - 1] if lane else []
                    digits = below + [d0, d0 + 3] + [d0 + 4 + k for k in range(len(below) + 1)]
                    lo = hi = d0 + 3                                                        # rank b + 1, b + 2 keys up to the lane's end
                keys = [edge_key(p, d) for d in digits]
                x = from_keys(keys, edge_key(p, lo), edge_key(p, hi), claims=dict(level=p, lane=lane, edge=edge))
                out.append(Proto("lane_edges", "p=%d lane %d %s" % (p, lane, edge), x, tol=TOLS[(p + lane) % 4]))
    return out


# ---------------------------------------------------------------------------------------------- all of them
FAMILIES = ("every_digit", "divergence", "ranks", "runs", "top_bins", "median_arithmetic", "keep", "lane_edges")


def family(name):
    """the cases of a family: every proto with the x values of the family's next proto of the same count as its y axis (its own
    values negated where it is the only one of its count)"""
    key = "cases " + name
    if key not in _CACHE:
        protos = globals()[name]()
        by_n = {}
        for q in protos:
            if q.y is None:
                by_n.setdefault(q.x.n, []).append(q)
        cases = []
        for q in protos:
            y = q.y
            if y is None:
                group = by_n[q.x.n]
                y = group[(group.index(q) + 1) % len(group)].x if len(group) > 1 else q.x.negated()
            cases.append(Case(q, y, zlib.crc32(("%s/%s" % (q.family, q.name)).encode())))
        _CACHE[key] = cases
    return _CACHE[key]


def all_cases():
    return [c for name in FAMILIES for c in family(name)]
