"""Crafted match sets for the device fit (k_fit.hpp and its second copy in k_estimate_batch.hpp; DESIGN.md section 7 rows 9 and
13), one family per clause of the solve that tests/fit_ref.py restates:

    DEGENERATE iff n < 3 || !(fabs(det) > 1e-12 * fmax(1.0, scale)),   scale = Sxx*Syy,  det = scale - Sxy*Sxy

On fit_ref.make_case every reading of that rule gives the same status: the sets are well conditioned, and the few degenerate
ones have a determinant of zero or of rounding noise.  Here the status is DICTATED by exact rational arithmetic on the float32
positions (exact()), never read from the restatement, and the sets stand on both sides of the threshold:

    ladder_line   the points t u (1, 1), t = -N .. N (u: a unit), and the two points (0, +k), (0, -k) off the line; list 2 is the exact image
                  under u = 2x - y + 3, v = x + y - 7.  The means are exactly 0 (or the translation), every product and every
                  partial sum is a multiple of 2^-34 below 2^53: the moments are exact in binary64 IN ANY ORDER, so every grid
                  gives the same bits.  ratio = det / (1e-12 max(1, scale)) is about 2 k^2 / (1e-12 sum t^2) and falls by 3 / N
                  per unit of N; the only rounding on the way to det is scale's (2^-53 relative, about 1e-4 of det), far inside
                  a rung.  Four rungs either side of ratio = 1 (LADDERS):
                    diagonal, anti (y = -x), steep (y = 3x)     relative regime, k = 2^-8, u = 1
                    moved 8192, moved 32768, moved apart        the diagonal translated; the means stay exact.  At 32768 sums that
                                                                are not centred lose k^2 below the last bit of sum x^2 (at 8192
                                                                they are still exact); "apart" is (8191, 5003): mx != my, neither
                                                                a power of two, so the order of c = mu - (a*mx + b*my) shows
                    horizontal, vertical                        Sxy == 0, so det == scale and the relative rule cannot trip: these
                                                                two are scaled by u = 2^-17 (k = 2^-16) until det crosses 1e-12
                                                                itself -- the absolute regime, rung by rung
                    big                                         k near 1, N = 14 320 / 14 400: up to 28 803 pairs, moments about
                                                                2e12, default grid 113 workgroups.  Sxy*Sxy rounds here as well
                                                                (2.7e-4 of det in all) and a unit of N is only 2e-4, so the rungs
                                                                step k as well (1 and 1 - 2^-5: k^2 is a multiple of 2^-10,
                                                                exact under sums of 2^42) and stay 0.4 % or more from 1
    tiny_cluster  the corners of a square of side 2^-j at (100, 200), m times over, moved by a translation: powers of two
                  throughout, Sxy == 0, det == scale = m^2 2^-4j < 1.  OK or DEGENERATE by fmax(1.0, scale) ALONE: without it
                  det > 1e-12 det always holds
    exact_fit     sets symmetric about an integer centre with integer offsets, under the integer map: every mean, moment and
                  product of the solve is an integer below 2^53.  Dictated: a .. f == 2, -1, 3, 1, 1, -7 and ssr == +0.0
    min_n         three pairs in a triangle (OK), three on a line, and masks that leave 3, 2 and 1 pairs of 300
    huge          a square of half-side 3e38 and its centre: moments 3.6e77, scale 1.3e155, nothing overflows in binary64; rows with
                  inf / NaN, rows outside their list and masked rows in between add nothing
    rounded_det   points EXACTLY on a line whose direction has 12-bit float32 components near 1/3, 0.1, ... : the exact det is 0, the
                  computed one is what the roundings of the sums leave.  Found by search (ROUNDED_SETS): sets whose computed det
                  is negative, positive and zero.  All DEGENERATE

solve_from_results() recomputes status and model from the RETURNED n, means and moments by the contract's formulas, one rounding
per operation: it pins scale, det, the rule, the six quotients and c = mu - (a*mx + b*my) separately from the order of the sums.

Accuracy (ACCURACY_*): the deviation of an accepted fit's coefficients from the exact rational solution, measured on the CPU by
tests/test_fit_cases_host.py, and the tests' bounds, 8 x the measured values.

Not observable, and not claimed by any family:
    `>=` for `>`            needs det == fl(1e-12 * fmax(1, scale)) exactly
    the clause n < 3 alone  two pairs are collinear: det is rounding noise (exactly 0 when the products are exact), far below the
                            threshold in either regime; one pair has every moment 0
    det without fabs        needs det < -1e-12 max(1, scale).  The computed moments are those of a Gram matrix (det >= 0) up to
                            the roundings of the products and sums, about 2^-53 (M / G + 9) relative: the most negative det / scale
                            the search of rounded_det met is ROUNDED_MOST_NEGATIVE, four orders of magnitude short; float32
                            positions cannot overflow a moment either (scale <= M^2 1.4e154).  tests/test_fit_cases_host.py holds
                            the mutant equal to the contract on every case here, so a set that does show it would be noticed

numpy and fractions only, deterministic, nothing here imports the package.  tests/test_fit_cases_host.py proves on the CPU that
every family is what it claims and that each mutant of the restatement is caught by a named family;
tests/test_gpu_fit_cases.py runs the families through siftmi_match_fit, MatchPlan.fit and both batch entries.
"""
from fractions import Fraction

import numpy as np

import fit_ref as fr
from consensus_ref import DTYPE_KP, gather

F32 = np.float32
_CACHE = {}
MAP = (2.0, -1.0, 3.0, 1.0, 1.0, -7.0)             # u = 2x - y + 3, v = x + y - 7
THRESHOLD = Fraction(float(np.float64(1e-12)))      # the binary64 constant of the rule, as a rational


def cached(fn):
    def get():
        if fn.__name__ not in _CACHE:
            _CACHE[fn.__name__] = fn()
        return _CACHE[fn.__name__]
    get.__name__, get.__doc__ = fn.__name__, fn.__doc__
    return get


# ---------------------------------------------------------------------------------------------- exact arithmetic
def exact(pts, mask=None):
    """The fit of the used rows of float32 `pts` (M, 4) in rational arithmetic: dict(n, means (4), moments (7), scale, det, ratio =
    det / (1e-12 max(1, scale)), status, model (6 Fractions, or None where det == 0 or n == 0)).  Every value is an exact
    Fraction; the moments are centred on the exact means."""
    pts = np.asarray(pts, F32).reshape(-1, 4)
    used = np.isfinite(pts).all(axis=1)
    if mask is not None:
        used &= np.asarray(mask).reshape(-1) != 0
    p = pts[used]
    n = len(p)
    if n == 0:
        return dict(n=0, status=fr.EMPTY, model=None)
    # every float32 is an integer over a power of two: one common denominator, then integer sums
    fracs = [[Fraction(float(v)) for v in row] for row in p]
    den = max(f.denominator for row in fracs for f in row)
    cols = [[f.numerator * (den // f.denominator) for f in col] for col in zip(*fracs)]
    x, y, u, v = cols
    s = [sum(c) for c in cols]
    means = [Fraction(t, n * den) for t in s]

    def moment(a, b, sa, sb):
        return Fraction(n * sum(p_ * q_ for p_, q_ in zip(a, b)) - sa * sb, n * den * den)
    Sxx, Sxy, Syy = moment(x, x, s[0], s[0]), moment(x, y, s[0], s[1]), moment(y, y, s[1], s[1])
    Sxu, Syu, Sxv, Syv = moment(x, u, s[0], s[2]), moment(y, u, s[1], s[2]), moment(x, v, s[0], s[3]), moment(y, v, s[1], s[3])
    scale = Sxx * Syy
    det = scale - Sxy * Sxy
    ratio = det / (THRESHOLD * max(Fraction(1), scale))
    out = dict(n=n, means=means, moments=[Sxx, Sxy, Syy, Sxu, Syu, Sxv, Syv], scale=scale, det=det, ratio=ratio, model=None)
    out["status"] = fr.DEGENERATE if n < 3 or not abs(ratio) > 1 else fr.OK
    if det != 0:
        a = (Sxu * Syy - Syu * Sxy) / det; b = (Syu * Sxx - Sxu * Sxy) / det
        d = (Sxv * Syy - Syv * Sxy) / det; e = (Syv * Sxx - Sxv * Sxy) / det
        out["model"] = [a, b, means[2] - (a * means[0] + b * means[1]), d, e, means[3] - (d * means[0] + e * means[1])]
    return out


def solve_from_results(out):
    """(status, model (6,) float64) recomputed from the n, means and moments that `out` (20 doubles) RETURNS, by the contract's
    formulas in binary64, one rounding per operation in the order written.  Must equal out[STATUS] and out[MODEL] bit for bit."""
    out = np.asarray(out, np.float64)
    model = np.full(6, np.nan, np.float64)
    n = out[fr.N]
    if n == 0:
        return fr.EMPTY, model
    mx, my, mu, mv = out[fr.MEANS]
    Sxx, Sxy, Syy, Sxu, Syu, Sxv, Syv = out[fr.MOMENTS]
    with np.errstate(all="ignore"):
        scale = Sxx * Syy
        det = scale - Sxy * Sxy
        if n < 3 or not (abs(det) > np.float64(1e-12) * max(np.float64(1.0), scale)):
            return fr.DEGENERATE, model
        a = (Sxu * Syy - Syu * Sxy) / det; b = (Syu * Sxx - Sxu * Sxy) / det
        c = mu - (a * mx + b * my)
        d = (Sxv * Syy - Syv * Sxy) / det; e = (Syv * Sxx - Sxv * Sxy) / det
        f = mv - (d * mx + e * my)
    model[:] = a, b, c, d, e, f
    return fr.OK, model


def solved_like(out):
    """does solve_from_results(out) give the status and the model that `out` holds, bit for bit (NaN as "is NaN")?"""
    status, model = solve_from_results(out)
    got = np.asarray(out, np.float64)[fr.MODEL]
    nan = np.isnan(model)
    return bool(status == out[fr.STATUS] and np.array_equal(np.isnan(got), nan)
                and np.array_equal(got[~nan].view(np.uint64), model[~nan].view(np.uint64)))


# ---------------------------------------------------------------------------------------------- a case
class Case(object):
    """pts (M, 4) float32: what the gather has to give, row by row; mask: None or (M,) uint8; void: rows whose pair names a record
    outside its list (they gather four NaN whatever pts holds).  dictated: what exact arithmetic prescribes -- status and n
    always, model / ssr where the family fixes them.  exact_sums: the moments are exact in any order (every grid, the same bits)."""

    def __init__(self, family, name, pts, mask=None, void=(), dictated=None, exact_sums=False, claims=None):
        self.family, self.name = family, "%s/%s" % (family, name)
        self.pts = np.array(pts, F32).reshape(-1, 4)
        self.mask = None if mask is None else np.ascontiguousarray(mask).astype(np.uint8)
        self.void = tuple(sorted(int(r) for r in void))
        self.pts[list(self.void)] = np.nan
        self.exact_sums, self.claims = bool(exact_sums), dict(claims or {})
        self.dictated = dict(dictated or {})
        self._want = {}

    @property
    def M(self):
        return len(self.pts)

    def exact(self):
        if "_exact" not in self.__dict__:
            self._exact = exact(self.pts, self.mask)
            self.dictated.setdefault("status", self._exact["status"])
            self.dictated.setdefault("n", self._exact["n"])
        return self._exact

    def status(self):
        self.exact()
        return self.dictated["status"]

    def want(self, blocks=0):
        """the restatement's 20 doubles"""
        if blocks not in self._want:
            self._want[blocks] = fr.fit_pts(self.pts, self.mask, blocks)
        return self._want[blocks]

    def lists(self):
        """(kp1, kp2, pairs): the rows at random places of two longer lists, as fit_ref.make_case puts them; the records no pair
        names are finite and far away, a void row names a record outside a list"""
        if "_lists" not in self.__dict__:
            M = self.M
            rng = np.random.default_rng(977 + M)
            n1, n2 = M + M // 8 + 5, M + M // 16 + 3
            pairs = np.stack([rng.permutation(n1)[:M], rng.permutation(n2)[:M]], axis=1).astype(np.int32)
            kp1, kp2 = np.zeros(n1, DTYPE_KP), np.zeros(n2, DTYPE_KP)
            for kp in (kp1, kp2):
                kp["x"] = 7777.0; kp["y"] = -7777.0
                kp["scale"] = rng.uniform(1, 8, len(kp)); kp["angle"] = rng.uniform(-3.14, 3.14, len(kp))
                kp["desc"] = rng.integers(0, 256, (len(kp), 128), dtype=np.uint8)
            kp1["x"][pairs[:, 0]] = self.pts[:, 0]; kp1["y"][pairs[:, 0]] = self.pts[:, 1]
            kp2["x"][pairs[:, 1]] = self.pts[:, 2]; kp2["y"][pairs[:, 1]] = self.pts[:, 3]
            for k, r in enumerate(self.void):           # first-list index too large / most negative, second-list -1 / too large
                if k % 2 == 0:
                    pairs[r, 0] = (n1, -2 ** 31)[(k // 2) % 2]
                else:
                    pairs[r, 1] = (-1, n2 + 1000)[(k // 2) % 2]
            got = gather(kp1, kp2, pairs)
            assert np.array_equal(np.isnan(got), np.isnan(self.pts)) and np.array_equal(got[~np.isnan(got)], self.pts[~np.isnan(got)]), self.name
            self._lists = (kp1, kp2, pairs)
        return self._lists

    def segment(self):
        """(kp1, kp2, pairs, mask): a segment for estimate_batch_ref.from_segments"""
        return self.lists() + (self.mask,)


def image(x, y):
    """list 2 under MAP, checked to be exact in float32"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    u, v = MAP[0] * x + MAP[1] * y + MAP[2], MAP[3] * x + MAP[4] * y + MAP[5]
    for a in (x, y, u, v):
        assert np.array_equal(a.astype(F32).astype(np.float64), a)
    return np.stack([x, y, u, v], axis=1).astype(F32)


def shuffled(pts, seed):
    return pts[np.random.default_rng(seed).permutation(len(pts))]


# ---------------------------------------------------------------------------------------------- ladder_line
#: name -> (direction of the line, the axis the two off-line points sit on, k, unit u of the line's points, translation)
LADDERS = {
    "diagonal": ((1, 1), (0, 1), 2.0 ** -8, 1.0, (0.0, 0.0)),
    "anti": ((1, -1), (0, 1), 2.0 ** -8, 1.0, (0.0, 0.0)),
    "steep": ((1, 3), (0, 1), 2.0 ** -8, 1.0, (0.0, 0.0)),
    "horizontal": ((1, 0), (0, 1), 2.0 ** -16, 2.0 ** -17, (0.0, 0.0)),
    "vertical": ((0, 1), (1, 0), 2.0 ** -16, 2.0 ** -17, (0.0, 0.0)),
    "moved 8192": ((1, 1), (0, 1), 2.0 ** -8, 1.0, (8192.0, 8192.0)),
    "moved 32768": ((1, 1), (0, 1), 2.0 ** -8, 1.0, (32768.0, 32768.0)),
    "moved apart": ((1, 1), (0, 1), 2.0 ** -8, 1.0, (8191.0, 5003.0)),
}
RUNGS_PER_SIDE = 4
#: the big ladder's rungs (N, k), ratio falling: two OK, two DEGENERATE; N = 14 400 is the largest set, 28 803 pairs
BIG_RUNGS = ((14320, 1.0), (14400, 1.0), (14160, 1.0 - 2.0 ** -5), (14400, 1.0 - 2.0 ** -5))
BIG_PAIRS = 28803
#: a dictated status needs the exact ratio this far from 1: scale's rounding (and on the big ladder Sxy*Sxy's) moves det by
#: at most 2.7e-4 of itself
RUNG_MARGIN = 2.0 ** -10


def ladder_ratio(name_or_line, N, k=None, unit=None):
    """the exact ratio of a ladder set in closed form: sum t^2 = N (N + 1) (2N + 1) / 3 over t = -N .. N"""
    if isinstance(name_or_line, str):
        line, axis, k0, unit0, _ = LADDERS[name_or_line]
        k, unit = k0 if k is None else k, unit0 if unit is None else unit
    else:
        line, axis = name_or_line
    S = Fraction(N * (N + 1) * (2 * N + 1), 3) * Fraction(unit) ** 2
    kk = 2 * Fraction(k) ** 2
    Sxx, Sxy, Syy = line[0] ** 2 * S + axis[0] * kk, line[0] * line[1] * S, line[1] ** 2 * S + axis[1] * kk
    scale = Sxx * Syy
    return (scale - Sxy * Sxy) / (THRESHOLD * max(Fraction(1), scale))


def ladder_flip(name):
    """the first N on the other side of ratio = 1 than N = 1: the relative ladders fall through it, the absolute ones rise"""
    first, N = ladder_ratio(name, 1) > 1, 2
    while (ladder_ratio(name, N) > 1) == first:
        N += 1
    return N


def ladder_pts(line, axis, k, unit, move, N, seed):
    t = np.arange(-N, N + 1, dtype=np.float64) * unit
    x = np.concatenate([line[0] * t, [axis[0] * k, -axis[0] * k]]) + move[0]
    y = np.concatenate([line[1] * t, [axis[1] * k, -axis[1] * k]]) + move[1]
    return shuffled(image(x, y), seed)


def _rung(name, line, axis, k, unit, move, N):
    ratio = ladder_ratio((line, axis), N, k, unit)
    assert abs(ratio - 1) > RUNG_MARGIN, (name, N, float(ratio))
    status = fr.OK if ratio > 1 else fr.DEGENERATE
    dictated = dict(status=status, n=2 * N + 3, means=(move[0], move[1], MAP[0] * move[0] + MAP[1] * move[1] + MAP[2], MAP[3] * move[0] + MAP[4] * move[1] + MAP[5]))
    return Case("ladder_line", "%s N=%d k=%r" % (name, N, k), ladder_pts(line, axis, k, unit, move, N, N), dictated=dictated,
                exact_sums=True, claims=dict(ladder=name, N=N, ratio=ratio))


def ladder(name):
    """the rungs of LADDERS[name] in ascending N: RUNGS_PER_SIDE on one side of ratio = 1, then RUNGS_PER_SIDE on the other"""
    key = "ladder " + name
    if key not in _CACHE:
        line, axis, k, unit, move = LADDERS[name]
        flip = ladder_flip(name)
        _CACHE[key] = [_rung(name, line, axis, k, unit, move, N) for N in range(flip - RUNGS_PER_SIDE, flip + RUNGS_PER_SIDE)]
    return _CACHE[key]


@cached
def big_ladder():
    return [_rung("big", (1, 1), (0, 1), k, 1.0, (0.0, 0.0), N) for N, k in BIG_RUNGS]


@cached
def ladder_line():
    return [c for name in LADDERS for c in ladder(name)] + big_ladder()


# ---------------------------------------------------------------------------------------------- tiny_cluster
#: (j, m): side 2^-j, m copies of the square; det == scale == m^2 2^-4j
TINY = ((8, 1), (9, 1), (10, 1), (10, 2), (11, 1), (11, 4), (11, 5), (11, 160))
TINY_SHIFT = (3.0, -7.0)


@cached
def tiny_cluster():
    out = []
    for j, m in TINY:
        s = 2.0 ** -j
        x = np.tile([100.0, 100.0 + s, 100.0, 100.0 + s], m); y = np.tile([200.0, 200.0, 200.0 + s, 200.0 + s], m)
        pts = np.stack([x, y, x + TINY_SHIFT[0], y + TINY_SHIFT[1]], axis=1)
        assert np.array_equal(pts.astype(F32).astype(np.float64), pts)
        det = Fraction(m * m, 2 ** (4 * j))
        status = fr.OK if det / THRESHOLD > 1 else fr.DEGENERATE
        dictated = dict(status=status, n=4 * m, means=(100.0 + s / 2, 200.0 + s / 2, 103.0 + s / 2, 193.0 + s / 2))
        if status == fr.OK:
            dictated.update(model=(1.0, 0.0, 3.0, 0.0, 1.0, -7.0), ssr=0.0)
        out.append(Case("tiny_cluster", "j=%d m=%d" % (j, m), shuffled(pts.astype(F32), j + m), dictated=dictated, exact_sums=True,
                        claims=dict(det=det)))
    return out


# ---------------------------------------------------------------------------------------------- exact_fit
#: (used pairs, unused rows in between, masked?)
EXACT_SETS = ((5, 0, False), (49, 0, False), (64, 0, False), (257, 0, False), (701, 0, False), (64, 40, True), (77, 500, True), (257, 300, True),
              (699, 61, True))
EXACT_CENTRE = (1000.0, 2000.0)


def _symmetric(n, rng, reach=31):
    """n distinct integer offsets, symmetric about (0, 0) (with (0, 0) itself when n is odd), not all on a line"""
    seen = set()
    while len(seen) < n // 2:
        dx, dy = (int(v) for v in rng.integers(-reach, reach + 1, 2))
        if (dx, dy) != (0, 0) and (-dx, -dy) not in seen:
            seen.add((dx, dy))
    half = np.array(sorted(seen), np.float64).reshape(-1, 2)
    off = np.concatenate([half, -half] + ([np.zeros((1, 2))] if n % 2 else []))
    return off


@cached
def exact_fit():
    out = []
    for n, extra, masked in EXACT_SETS:
        rng = np.random.default_rng(300 + n)
        off = _symmetric(n, rng)
        used = image(EXACT_CENTRE[0] + off[:, 0], EXACT_CENTRE[1] + off[:, 1])
        M = n + extra
        pts = rng.uniform(-5000, 5000, (M, 4)).astype(F32)          # the unused rows: finite and far off the map
        at = np.sort(rng.permutation(M)[:n])
        pts[at] = shuffled(used, n)
        mask = None
        if masked:
            mask = np.zeros(M, np.uint8)
            mask[at] = rng.integers(1, 256, n)                      # any non-zero byte counts
        cx, cy = EXACT_CENTRE
        dictated = dict(status=fr.OK, n=n, model=MAP, ssr=0.0, means=(cx, cy, MAP[0] * cx + MAP[1] * cy + MAP[2], MAP[3] * cx + MAP[4] * cy + MAP[5]))
        out.append(Case("exact_fit", "n=%d of %d" % (n, M), pts, mask=mask, dictated=dictated, exact_sums=True))
    return out


# ---------------------------------------------------------------------------------------------- min_n
MIN_M = 300
MIN_ROWS = (5, 256, 299)            # lane 5 and lane 0 of workgroup 0 / 1 under the default grid, the last row


@cached
def min_n():
    tri = image([0.0, 3.0, 0.0], [0.0, 0.0, 3.0])                   # means (1, 1): Sxx = Syy = 6, Sxy = -3, det = 27
    line = image([0.0, 1.0, 2.0], [0.0, 1.0, 2.0])
    ok = dict(status=fr.OK, n=3, model=MAP, ssr=0.0)
    out = [Case("min_n", "triangle", tri, dictated=ok, exact_sums=True),
           Case("min_n", "three on a line", line, dictated=dict(status=fr.DEGENERATE, n=3), exact_sums=True)]
    rng = np.random.default_rng(17)
    for left in (3, 2, 1):
        pts = rng.uniform(-5000, 5000, (MIN_M, 4)).astype(F32)
        pts[list(MIN_ROWS)] = tri
        mask = np.zeros(MIN_M, np.uint8)
        mask[list(MIN_ROWS[:left])] = (1, 0x80, 0xff)[:left]
        out.append(Case("min_n", "mask leaves %d" % left, pts, mask=mask, exact_sums=True,
                        dictated=ok if left == 3 else dict(status=fr.DEGENERATE, n=left)))
    return out


# ---------------------------------------------------------------------------------------------- huge
HUGE = float(F32(3e38))
HUGE_COPIES = 20


def _huge_rows():
    x = np.array([HUGE, HUGE, -HUGE, -HUGE, 0.0]); y = np.array([HUGE, -HUGE, HUGE, -HUGE, 0.0])
    return np.stack([x, y, -y, x], axis=1).astype(F32)              # list 2: the quarter turn u = -y, v = x, exact


@cached
def huge():
    """two cases: the five points alone, and HUGE_COPIES of them with six unused rows after each used one: inf, -inf and NaN in
    either list, a pair outside its list, and two masked rows that hold 3e38 and 1e-30"""
    five = _huge_rows()
    turn = (0.0, -1.0, 0.0, 1.0, 0.0, 0.0)
    out = [Case("huge", "five points", five, dictated=dict(status=fr.OK, n=5, model=turn, ssr=0.0, means=(0.0,) * 4), exact_sums=True)]
    used = np.tile(five, (HUGE_COPIES, 1))
    n = len(used)
    pts = np.zeros((7 * n, 4), F32)
    mask = np.ones(7 * n, np.uint8)
    pts[::7] = shuffled(used, 5)
    junk = np.array([[np.inf, 1, 2, 3], [4, -np.inf, 5, 6], [7, 8, np.nan, 9], [1, 2, 3, np.inf], [0, 0, 0, 0], [HUGE, -HUGE, HUGE, 1.0], [1e-30, 1e-30, -1e-30, 5.0]], F32)
    for k in range(1, 7):
        pts[k::7] = junk[k]
    pts[1::14] = junk[0]                                             # rows 1 mod 7 alternate +inf in x0 and -inf in y0
    void = list(range(4, 7 * n, 7))
    mask[5::7] = 0; mask[6::7] = 0
    out.append(Case("huge", "interleaved", pts, mask=mask, void=void, dictated=dict(status=fr.OK, n=n, model=turn, ssr=0.0, means=(0.0,) * 4),
                    exact_sums=True))
    return out


# ---------------------------------------------------------------------------------------------- rounded_det
#: (slope the direction is near, n, seed of the t, sign of the computed det under the default grid): what rounded_search() finds,
#: kept as a list so that building the family costs nothing; the host test repeats the search and checks every sign
ROUNDED_SETS = ((1.0 / 3.0, 600, 0, 0), (0.1, 600, 0, 1), (0.7, 600, 0, 1), (3.0, 600, 0, 0), (3.0, 650, 0, -1), (0.7, 700, 0, -1))
#: the most negative computed det / scale that rounded_search() meets (grids 0, 1, 3 of its 96 sets)
ROUNDED_MOST_NEGATIVE = -4.739764678205612e-16


def rounded_direction(slope):
    """(dx, dy) float32 with 12-bit significands, dy / dx near `slope`: t * dx and t * dy are exact in float32 for |t| < 2^12"""
    def cut(v):
        m, e = np.frexp(v)
        return float(np.ldexp(np.round(m * 4096.0) / 4096.0, e))
    return cut(np.sqrt(2.0)), cut(np.sqrt(2.0) * slope)


def rounded_pts(slope, n, seed):
    dx, dy = rounded_direction(slope)
    t = np.random.default_rng(seed).integers(-4000, 4001, n).astype(np.float64)      # no progression: its mean would be exact
    x, y = t * dx, t * dy
    pts = np.stack([x, y, 0.5 * y + 11.0, 0.25 * x - 5.0], axis=1)
    assert np.array_equal(pts[:, :2].astype(F32).astype(np.float64), pts[:, :2])
    return pts.astype(F32)


def computed_det(out):
    Sxx, Sxy, Syy = np.asarray(out, np.float64)[fr.MOMENTS][:3]
    return Sxx * Syy - Sxy * Sxy


ROUNDED_SLOPES, ROUNDED_N, ROUNDED_SEEDS = (1.0 / 3.0, 0.1, 0.7, 3.0), (600, 650, 700), 8


def rounded_search(want_each=2):
    """([(slope, n, seed, sign)], most negative det / scale): `want_each` sets per sign of the computed det under the default
    grid, in the order the search meets them, and the most negative computed det / scale over grids 0, 1, 3 of every set tried"""
    found, count, worst = [], {-1: 0, 0: 0, 1: 0}, 0.0
    for seed in range(ROUNDED_SEEDS):
        for n in ROUNDED_N:
            for slope in ROUNDED_SLOPES:
                pts = rounded_pts(slope, n, seed)
                for blocks in (0, 1, 3):
                    out = fr.fit_pts(pts, blocks=blocks)
                    worst = min(worst, float(computed_det(out) / (out[fr.MOMENTS][0] * out[fr.MOMENTS][2])))
                    if blocks == 0:
                        sign = int(np.sign(computed_det(out)))
                        if count[sign] < want_each:
                            count[sign] += 1
                            found.append((slope, n, seed, sign))
    return found, worst


@cached
def rounded_det():
    out = []
    for slope, n, seed, sign in ROUNDED_SETS:
        out.append(Case("rounded_det", "slope %.3g n=%d seed=%d" % (slope, n, seed), rounded_pts(slope, n, seed),
                        dictated=dict(status=fr.DEGENERATE, n=n), claims=dict(sign=sign)))
    return out


# ---------------------------------------------------------------------------------------------- all of them
FAMILIES = ("ladder_line", "tiny_cluster", "exact_fit", "min_n", "huge", "rounded_det")


def family(name):
    return globals()[name]()


def all_cases():
    return [c for name in FAMILIES for c in family(name)]


# ---------------------------------------------------------------------------------------------- accuracy
#: Largest |coefficient - exact rational coefficient| of the restatement (default grid) as measured on the CPU by
#: tests/test_fit_cases_host.py, and the tests' bounds: 8 x that, as fit_ref.LSTSQ_BOUND is formed.  Both sides solve the same
#: normal equations, one in binary64 and one exactly, so a small multiple covers the order of other grids without hiding a wrong
#: formula.
#: the ladders' OK rungs: the error of a, b, d, e as a multiple of 2^-53 * scale / |det| * max |a, b, d, e|, and the error of c, f as
#: a multiple of that times the reach 1 + |mx| + |my| (c = mu - (a*mx + b*my) carries the error of a, b that far); the largest of
#: both over grids 0 and 1 (steep, N = 170).  The error has to follow the conditioning, not merely stay small
ACCURACY_LADDER_MULTIPLE_MEASURED = 1.4321556104647244
ACCURACY_LADDER_MULTIPLE_BOUND = 8 * ACCURACY_LADDER_MULTIPLE_MEASURED
#: fit_ref.CASES up to 5000 pairs (well conditioned: scale / det about 1), absolute.  The OK cases of tiny_cluster, exact_fit,
#: min_n and huge are dictated to be exact: their deviation is 0 and nothing is allowed
ACCURACY_GENERIC_MEASURED = 2.616152124138804e-12
ACCURACY_GENERIC_BOUND = 8 * ACCURACY_GENERIC_MEASURED
