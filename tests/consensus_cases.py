"""Crafted match sets for the consensus filter (k_consensus.hpp, k_consensus_batch.hpp), one
family per rule of the contract that tests/consensus_ref.py restates.  On consensus_ref.synthetic_matches the rules' edges are met
by chance or never: no determinant of magnitude exactly 1, a fused solve that changes no model, a handful of errors equal to the
tolerance, no position that is not finite.  Here the sample -- which depends on (seed, h, M) only -- is computed first and the
positions are PLACED on the rows each hypothesis draws:

    det_edge        triples with det exactly +-1 (valid), the largest binary64 and binary32 below 1 in magnitude, +-0.5, 0 from a
                    repeated index and from coincident rows, NaN from a pair outside its list (all void); each below and from h = 256
    solve_rounding  the solve far from the origin on a sheared map: c = x1 - (a*x0 + b*y0) cancels, a fused a*x0 + b*y0 is seen
    vote_ring       probe rows at distance tol from one hypothesis each, stepped by ulps until the unfused vote and ONE fused form
                    disagree, for each of the four fusable places
    vote_equal      exact integer translations and rows off by (3, 4), (0, 5), (5, 0): t == tol2 with tol = 5, and one ulp off
    select_order    most rows out of range, the few valid hypotheses tie: first valid h > 0; >= 512 with an equal one in the same
                    lane of the select; a larger h with strictly more votes than every smaller one
    non_finite      inf, -inf, NaN and 3e38 in the lists, on rows the sample draws and on rows it does not; a set whose valid
                    hypotheses all collect no vote
    tol_range       tol2 = inf, subnormal and 0 on the vote_equal rows

The contraction of det and of the numerators `p*q - r*s` of the solve is NOT covered: through float32 coefficients no input was
found where it can be seen (the quotient absorbs it), and solve_rounding does not claim it.

Then the vote grid: vote_grid() restates the chunk rule of match.hip, and wide_single() / WIDE_BATCH_CASES are the calls whose
workgroups walk more than 256 hypotheses (the second trip of the kernels' fold loop, columns 256..511 of their LDS counters).

numpy and fractions only, deterministic, nothing here imports the package.  tests/test_consensus_cases_host.py proves on the CPU
that every family reaches its rule, with correctly rounded fused variants; tests/test_gpu_consensus_cases.py runs the families.
"""
from fractions import Fraction

import numpy as np

import consensus_ref as cr

F32 = np.float32
_CACHE = {}


def cached(fn):
    def get():
        if fn.__name__ not in _CACHE:
            _CACHE[fn.__name__] = fn()
        return _CACHE[fn.__name__]
    get.__name__, get.__doc__ = fn.__name__, fn.__doc__
    return get


# ---------------------------------------------------------------------------------------------- a case
class Case(object):
    """pts (M, 4) float32: what the gather has to give, row by row; bad: rows whose pair names a record outside its list (they
    gather four NaN whatever pts holds).  The records sit at shuffled places of two longer lists; the records no pair names are
    finite and far away.  claims: what the family says the set reaches (checked by the host test)."""

    def __init__(self, family, name, pts, n_hyp, tol, seed, bad=(), claims=None):
        self.family, self.name = family, "%s/%s" % (family, name)
        self.n_hyp, self.tol, self.seed, self.claims = int(n_hyp), F32(tol), int(seed), dict(claims or {})
        pts = np.array(pts, F32).reshape(-1, 4)
        M = len(pts)
        rng = np.random.default_rng(4242 + M)
        n1, n2 = M + 5, M + 3
        pairs = np.stack([rng.permutation(n1)[:M], rng.permutation(n2)[:M]], axis=1).astype(np.int32)
        kp1, kp2 = np.zeros(n1, cr.DTYPE_KP), np.zeros(n2, cr.DTYPE_KP)
        for kp in (kp1, kp2):
            kp["x"] = 7777.0; kp["y"] = -7777.0
            kp["scale"] = rng.uniform(1, 8, len(kp)); kp["angle"] = rng.uniform(-3.14, 3.14, len(kp))
            kp["desc"] = rng.integers(0, 256, (len(kp), 128), dtype=np.uint8)
        kp1["x"][pairs[:, 0]] = pts[:, 0]; kp1["y"][pairs[:, 0]] = pts[:, 1]
        kp2["x"][pairs[:, 1]] = pts[:, 2]; kp2["y"][pairs[:, 1]] = pts[:, 3]
        for k, r in enumerate(sorted(bad)):             # first-list index too large / most negative, second-list -1 / too large
            if k % 2 == 0:
                pairs[r, 0] = (n1, -2 ** 31)[(k // 2) % 2]
            else:
                pairs[r, 1] = (-1, n2 + 1000)[(k // 2) % 2]
            pts[r] = np.nan
        self.kp1, self.kp2, self.pairs, self.pts, self.bad = kp1, kp2, pairs, pts, tuple(sorted(bad))
        got = cr.gather(kp1, kp2, pairs)
        assert np.array_equal(got.view(np.uint32), pts.view(np.uint32)), self.name

    @property
    def M(self):
        return len(self.pairs)

    @property
    def args(self):
        return self.kp1, self.kp2, self.pairs, self.n_hyp, float(self.tol), self.seed

    def idx(self):
        return cr.sample(self.seed, self.n_hyp, self.M)

    def want(self):
        if "_want" not in self.__dict__:
            self._want = cr.consensus(*self.args)
        return self._want

    def reversed_segment(self):
        """the same matches in reverse order (another sample draws them): the neighbour of the case in a batch.  Its rows follow
        the case's own maps, so they would vote on the case's hypotheses if a read crossed the segment's bounds"""
        return self.kp1, self.kp2, np.ascontiguousarray(self.pairs[::-1])


def distinct(idx):
    return (idx[:, 0] != idx[:, 1]) & (idx[:, 0] != idx[:, 2]) & (idx[:, 1] != idx[:, 2])


def det_of(pts, idx):
    """the determinant of the solve, binary64, the contract's order"""
    p = pts.astype(np.float64)
    i0, i1, i2 = idx[:, 0], idx[:, 1], idx[:, 2]
    with np.errstate(all="ignore"):
        ux = p[i1, 0] - p[i0, 0]; uy = p[i1, 1] - p[i0, 1]; vx = p[i2, 0] - p[i0, 0]; vy = p[i2, 1] - p[i0, 1]
        return ux * vy - vx * uy


# ---------------------------------------------------------------------------------------------- exact fused arithmetic
def _fr(v):
    return Fraction(float(v))


def round_f64(q):
    """a rational to binary64, rounded once to nearest even (int / int is correctly rounded)"""
    return float(q)


def round_f32(q):
    """a rational to binary32, rounded ONCE to nearest even: float(q) -> float32 would round twice"""
    if q == 0:
        return F32(0.0)
    c = F32(float(q))
    with np.errstate(all="ignore"):
        cands = [c, np.nextafter(c, F32(np.inf)), np.nextafter(c, F32(-np.inf))]
    return min(cands, key=lambda v: (abs(_fr(v) - q), int(np.asarray(v).view(np.uint32)) & 1))


def fma64(a, b, c):
    return round_f64(_fr(a) * _fr(b) + _fr(c))


def fma32(a, b, c):
    return round_f32(_fr(a) * _fr(b) + _fr(c))


PLACES = ("unfused", "fma(a,x0,b*y0)", "fma(b,y0,a*x0)", "fma(ex,ex,ey*ey)", "fma(ey,ey,ex*ex)")


def vote_exact(model, row, tol, place):
    """does the match `row` vote for the float32 `model`, with the product-sum of PLACES[place] fused (correctly rounded) and
    everything else rounded operation by operation; place 0 is the contract.  Finite values only."""
    a, b, c, d, e, f = (F32(v) for v in model)
    x0, y0, x1, y1 = (F32(v) for v in row)
    tol = F32(tol)

    def lin(p, q, r, z):
        if place == 1:
            t = fma32(p, x0, q * y0)
        elif place == 2:
            t = fma32(q, y0, p * x0)
        else:
            t = p * x0 + q * y0
        return (t + r) - z
    ex, ey = lin(a, b, c, x1), lin(d, e, f, y1)
    if place == 3:
        t = fma32(ex, ex, ey * ey)
    elif place == 4:
        t = fma32(ey, ey, ex * ex)
    else:
        t = ex * ex + ey * ey
    assert isinstance(t, np.float32)
    return bool(t <= tol * tol)


SOLVE_FORMS = ("fma(a,x0,b*y0)", "fma(b,y0,a*x0)")


def solve_fused(pts, idx, form):
    """consensus_ref.solve with the sum of products in c and f contracted (SOLVE_FORMS[form]), correctly rounded.  Returns the
    float32 models (void rows NaN) and `valid`"""
    models, valid = cr.solve(pts, idx)
    p = pts.astype(np.float64)
    i0, i1, i2 = idx[:, 0], idx[:, 1], idx[:, 2]
    x0, y0, x1, y1 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    with np.errstate(all="ignore"):
        ux = x0[i1] - x0[i0]; uy = y0[i1] - y0[i0]; vx = x0[i2] - x0[i0]; vy = y0[i2] - y0[i0]
        det = ux * vy - vx * uy
        px = x1[i1] - x1[i0]; qx = x1[i2] - x1[i0]; py = y1[i1] - y1[i0]; qy = y1[i2] - y1[i0]
        a = (px * vy - qx * uy) / det; b = (qx * ux - px * vx) / det
        d = (py * vy - qy * uy) / det; e = (qy * ux - py * vx) / det
    out = models.copy()
    for h in np.flatnonzero(valid):
        X, Y = x0[i0[h]], y0[i0[h]]
        for col, (p_, q_, z) in ((2, (a[h], b[h], x1[i0[h]])), (5, (d[h], e[h], y1[i0[h]]))):
            s = fma64(p_, X, q_ * Y) if form == 0 else fma64(q_, Y, p_ * X)
            out[h, col] = F32(z - s)
    return out, valid


# ---------------------------------------------------------------------------------------------- det_edge
BELOW64 = 1.0 - 2.0 ** -53          # the largest binary64 below 1
BELOW32 = 1.0 - 2.0 ** -24          # the largest binary32 below 1
#: class -> (p1 - p0, p2 - p0, det): u = p1 - p0, v = p2 - p0, det = ux vy - vx uy; p0 at the origin where a coordinate needs it
DET_TRIPLES = {
    "+1": ((1.0, 0.0), (0.0, 1.0), 1.0),
    "-1": ((0.0, 1.0), (1.0, 0.0), -1.0),
    "+1 sheared": ((2.0, 1.5), (1.0, 1.25), 1.0),                     # 2 * 1.25 - 1 * 1.5
    "+below64": ((1.0, 2.0 ** -27), (2.0 ** -26, 1.0), BELOW64),       # 1 - 2^-53: one rounding away from 1
    "-below64": ((2.0 ** -26, 1.0), (1.0, 2.0 ** -27), -BELOW64),
    "+below32": ((BELOW32, 0.0), (0.0, 1.0), BELOW32),                 # the row at 1 - 2^-24
    "-below32": ((0.0, 1.0), (BELOW32, 0.0), -BELOW32),
    "+0.5": ((1.0, 0.0), (0.0, 0.5), 0.5),
    "-0.5": ((0.0, 0.5), (1.0, 0.0), -0.5),
    "0 coincident": ((0.0, 0.0), (0.0, 0.0), 0.0),
    "nan": ((1.0, 0.0), (0.0, 1.0), float("nan")),                     # p2's pair is outside its list
}
DET_VALID = ("+1", "-1", "+1 sheared")
DET_M, DET_H, DET_SPLIT = 384, 512, 256
DET_SHIFT = (3.0, -2.0)


@cached
def det_edge():
    """claims: classes = {class: [h, ...]} with every class of DET_TRIPLES and "0 repeated" at some h < 256 and some h >= 256"""
    M, H = DET_M, DET_H
    for seed in range(1000):
        idx = cr.sample(seed, H, M)
        rep = np.flatnonzero(~distinct(idx))
        if (rep < DET_SPLIT).any() and (rep >= DET_SPLIT).any():
            break
    rng = np.random.default_rng(11)
    x0 = rng.integers(0, 32, M) * 0.5; y0 = rng.integers(0, 32, M) * 0.5          # the lattice of step 1 and 1/2
    used = np.zeros(M, bool)
    used[idx[rep].reshape(-1)] = True                   # the repeated-index triples keep their lattice rows
    classes, bad = {"0 repeated": [int(h) for h in rep]}, []
    for half in (range(0, DET_SPLIT), range(DET_SPLIT, H)):
        todo = list(DET_TRIPLES)
        for h in half:
            if not todo:
                break
            t = idx[h]
            if len(set(t.tolist())) < 3 or used[t].any():
                continue
            name = todo.pop(0)
            u, v, _ = DET_TRIPLES[name]
            tiny = "below" in name
            ox, oy = (0.0, 0.0) if tiny else (float(rng.integers(0, 16)), float(rng.integers(0, 16)))
            x0[t] = [ox, ox + u[0], ox + v[0]]; y0[t] = [oy, oy + u[1], oy + v[1]]
            used[t] = True
            if name == "nan":
                bad.append(int(t[2]))
            classes.setdefault(name, []).append(int(h))
        assert not todo, todo
    pts = np.stack([x0, y0, x0 + DET_SHIFT[0], y0 + DET_SHIFT[1]], axis=1)
    return Case("det_edge", "lattice", pts, H, 3.0, seed, bad=bad, claims=dict(classes=classes))


# ---------------------------------------------------------------------------------------------- solve_rounding
SOLVE_MIN_CHANGED = 32


@cached
def solve_rounding():
    """claims: nothing stored -- the host test counts the models that solve_fused changes (at least SOLVE_MIN_CHANGED in c)"""
    rng = np.random.default_rng(5)
    M = 64
    x0 = (1e8 + rng.uniform(0, 4096 * 10, M)).astype(F32).astype(np.float64)
    y0 = (1e8 + rng.uniform(0, 4096 * 10, M)).astype(F32).astype(np.float64)
    x1 = 1.0000001 * x0 - 0.9999999 * y0 + 5
    y1 = 0.9999998 * x0 - 1.0000002 * y0 - 3
    return Case("solve_rounding", "origin 1e8", np.stack([x0, y0, x1, y1], axis=1), 2048, 3.0, 0)


# ---------------------------------------------------------------------------------------------- vote_ring
RING_M, RING_H, RING_TOL, RING_SEED = 1030, 512, 3.0, 7
RING_ROWS = (0, 63, 64, 255, 256, 1023, 1024, RING_M - 1,                     # both register slots of a lane, wave edges, tile 2
             1, 62, 65, 127, 128, 191, 192, 254, 257, 319, 320, 511, 512, 513, 575, 576, 767, 768, 769, 1000, 1022, 1025, 1026, 1027,
             300, 700, 900, 1028)
RING_MIN_PER_PLACE = 8
RING_MAP = (np.cos(0.03) * 1.01, -np.sin(0.03) * 1.01, np.pi + 2.0, np.sin(0.03) * 1.01, np.cos(0.03) * 1.01, np.e + 3.0)


def _steps(v, n):
    """the 2n + 1 float32 values around v > 0, one ulp apart"""
    bits = np.asarray(F32(v)).view(np.int32) + np.arange(-n, n + 1, dtype=np.int32)
    return bits.view(F32)


def _ring_search(model, place, rng):
    """a row (x0, y0, x1, y1) near the origin at distance tol from `model` on which the unfused vote and the vote with
    PLACES[place] fused disagree.  The search is done in binary64 (products of two float32 are exact there); the caller checks
    the row found with vote_exact"""
    a, b, c, d, e, f = (F32(v) for v in model)
    tol2 = F32(RING_TOL) * F32(RING_TOL)
    for _ in range(400):
        x0, y0 = F32(rng.uniform(0.5, 2.0)), F32(rng.uniform(0.5, 2.0))
        pu = ((a * x0 + b * y0) + c, (d * x0 + e * y0) + f)                          # unfused prediction
        if place == 1:
            pf = (fma32(a, x0, b * y0) + c, fma32(d, x0, e * y0) + f)
        elif place == 2:
            pf = (fma32(b, y0, a * x0) + c, fma32(e, y0, d * x0) + f)
        else:
            pf = pu
        if place in (1, 2) and pf == pu:
            continue
        # the error lies along the axis that has to dominate t: x where the fused prediction differs in x, or for fma(ex,ex,.)
        x_major = (pf[0] != pu[0]) if place in (1, 2) else place == 3
        minor = F32(rng.uniform(0.05, 0.2))
        major = F32(np.sqrt(float(tol2) - float(minor) ** 2))
        ex0, ey0 = (major, minor) if x_major else (minor, major)
        if min(pu[0] - ex0, pu[1] - ey0) < 0.25:
            continue
        X1 = _steps(pu[0] - ex0, 4 if x_major else 600)[:, None]
        Y1 = _steps(pu[1] - ey0, 600 if x_major else 4)[None, :]
        ex_u, ey_u = pu[0] - X1, pu[1] - Y1
        ex_f, ey_f = pf[0] - X1, pf[1] - Y1
        t_u = ex_u * ex_u + ey_u * ey_u
        if place == 3:
            t_f = (ex_f.astype(np.float64) ** 2 + (ey_f * ey_f).astype(np.float64)).astype(F32)
        elif place == 4:
            t_f = (ey_f.astype(np.float64) ** 2 + (ex_f * ex_f).astype(np.float64)).astype(F32)
        else:
            t_f = ex_f * ex_f + ey_f * ey_f
        assert t_u.dtype == F32 and t_f.dtype == F32
        hit = np.argwhere((t_u <= tol2) != (t_f <= tol2))
        for i, j in hit[:8]:
            row = (x0, y0, X1[i, 0], Y1[0, j])
            if vote_exact(model, row, RING_TOL, 0) != vote_exact(model, row, RING_TOL, place):
                return row
    raise AssertionError("no probe found for %s" % PLACES[place])


@cached
def vote_ring():
    """claims: probes = [(place, row, h, unfused vote, fused vote), ...], RING_MIN_PER_PLACE or more per place 1..4"""
    M, H, seed = RING_M, RING_H, RING_SEED
    rng = np.random.default_rng(23)
    x0 = rng.uniform(0, 1000, M).astype(F32).astype(np.float64); y0 = rng.uniform(0, 1000, M).astype(F32).astype(np.float64)
    A = RING_MAP
    x1 = A[0] * x0 + A[1] * y0 + A[2] + rng.normal(0, 0.05, M); y1 = A[3] * x0 + A[4] * y0 + A[5] + rng.normal(0, 0.05, M)
    pts = np.stack([x0, y0, x1, y1], axis=1).astype(F32)
    idx = cr.sample(seed, H, M)
    models, valid = cr.solve(pts, idx)          # the models of the triples without a probe row do not depend on the probes
    free = valid & ~np.isin(idx, list(RING_ROWS)).any(axis=1) & (np.abs(models - np.asarray(A, F32)) < 0.5).all(axis=1)
    # the targets spread evenly over the hypotheses, below and from h = 256
    targets = np.flatnonzero(free)
    targets = targets[np.linspace(0, len(targets) - 1, len(RING_ROWS)).astype(int)]
    assert len(set(targets.tolist())) == len(RING_ROWS)
    probes = []
    for k, (row, h) in enumerate(zip(RING_ROWS, targets)):
        place = 1 + k % 4
        pts[row] = _ring_search(models[h], place, rng)
        probes.append((place, int(row), int(h), vote_exact(models[h], pts[row], RING_TOL, 0), vote_exact(models[h], pts[row], RING_TOL, place)))
    return Case("vote_ring", "probes", pts, H, RING_TOL, seed, claims=dict(probes=probes))


# ---------------------------------------------------------------------------------------------- vote_equal, tol_range
EQ_M, EQ_H, EQ_SHIFT = 600, 128, (8.0, -3.0)
TOL5 = F32(5.0)
TOL5_BELOW = np.nextafter(TOL5, F32(0.0))
#: name -> what the row's error (ex, ey) is against the one model (1, 0, 8, 0, 1, -3); rows EQ_M - len(EQ_OFF) ... EQ_M - 1
EQ_OFF = ("(3,4)", "(0,5)", "(5,0)", "(-4,3)", "(3,4)+ulp", "1e-20", "-1e-20 y", "2e-20", "3e38", "inf", "-inf y")
TOL_RANGE = (("inf", F32(3e19)), ("subnormal", F32(1e-20)), ("zero", F32(np.finfo(np.float32).smallest_subnormal)))


@cached
def _equal_rows():
    """(pts, seed, first special row): EQ_M - len(EQ_OFF) rows on an exact integer translation, then
    the EQ_OFF rows; the seed is the first whose EQ_H hypotheses draw none of the EQ_OFF rows, so every valid model is exactly
    (1, 0, tx, 0, 1, ty)"""
    M, n_off = EQ_M, len(EQ_OFF)
    n = M - n_off
    k = np.arange(n, dtype=np.float64)
    x0 = 2.0 * k; y0 = (k * k) % 1009.0                 # distinct x, integers: a det is 0 (void) or at least 1 in magnitude
    tx, ty = EQ_SHIFT
    pts = np.zeros((M, 4), np.float64)
    pts[:n] = np.stack([x0, y0, x0 + tx, y0 + ty], axis=1)
    at = dict((name, n + i) for i, name in enumerate(EQ_OFF))
    for name, r in at.items():
        pts[r] = [40.0 + r, 17.0, 40.0 + r + tx, 17.0 + ty]              # on the map, then moved off it
    pts[at["(3,4)"], 2:] += (-3.0, -4.0)                # ex = pred - x1 = 3, ey = 4
    pts[at["(0,5)"], 3] -= 5.0
    pts[at["(5,0)"], 2] -= 5.0
    pts[at["(-4,3)"], 2:] += (4.0, -3.0)
    pts[at["(3,4)+ulp"], 2:] += (-3.0, -4.0)
    pts = pts.astype(F32)
    r = at["(3,4)+ulp"]
    pts[r, 2] = np.nextafter(pts[r, 2], F32(-np.inf))                    # |ex| one ulp of x1 above 3
    # errors far below one ulp of a position: the prediction is exactly 0 where x0 = -tx, y0 = -ty
    for name, xy in (("1e-20", (-1e-20, 0.0)), ("-1e-20 y", (0.0, 1e-20)), ("2e-20", (-2e-20, 0.0)), ("3e38", (3e38, 0.0)),
                     ("inf", (np.inf, 0.0)), ("-inf y", (0.0, -np.inf))):
        pts[at[name]] = [-tx, -ty, xy[0], xy[1]]
    special = np.arange(n, M)
    for seed in range(100000):
        if not np.isin(cr.sample(seed, EQ_H, M), special).any():
            return pts, seed, n
    raise AssertionError("no seed")


def _equal_case(family, name, tol):
    pts, seed, first = _equal_rows()
    return Case(family, name, pts, EQ_H, tol, seed, claims=dict(rows=dict((n, first + i) for i, n in enumerate(EQ_OFF)), first=first))


@cached
def vote_equal():
    """two cases on the same rows: tol = 5 (t == tol2 votes) and tol one ulp below 5"""
    return [_equal_case("vote_equal", "tol 5", TOL5), _equal_case("vote_equal", "tol 5 - ulp", TOL5_BELOW)]


@cached
def tol_range():
    return [_equal_case("tol_range", name, tol) for name, tol in TOL_RANGE]


# ---------------------------------------------------------------------------------------------- select_order
SELECT_LANES = 256          # consensus_select: lane l scans h = l, l + 256, ...


def _parabola(n, first=0):
    k = np.arange(first, first + n, dtype=np.float64)
    return 3.0 * k, k * k                               # no three points of a parabola lie on a line


def _select_rows(M, groups):
    """groups: [(rows, (tx, ty)), ...] at the head of the set, every other row out of range"""
    pts = np.zeros((M, 4), np.float64)
    at = 0
    for n, (tx, ty) in groups:
        x, y = _parabola(n, at)
        pts[at:at + n] = np.stack([x, y, x + tx, y + ty], axis=1)
        at += n
    # spread the good rows over the set
    order = np.random.default_rng(M).permutation(M)
    out = np.zeros_like(pts)
    out[order] = pts
    bad = sorted(int(r) for r in order[at:])
    return out, bad


@cached
def select_order():
    """three cases; claims: first (the first valid h), valid (all valid h), and for "later maximum" winner"""
    cases = []
    # (a) the first valid h is > 0 and the valid ones all tie
    pts, bad = _select_rows(40, [(10, (8.0, -3.0))])
    for seed in range(10000):
        v = np.flatnonzero(cr.solve(_nan_rows(pts, bad), cr.sample(seed, 256, 40))[1])
        if len(v) >= 3 and v[0] > 0:
            break
    cases.append(Case("select_order", "first valid > 0", pts, 256, 3.0, seed, bad=bad, claims=dict(first=int(v[0]), valid=v.tolist())))
    # (b) the first valid h is >= 512 and an equal one follows in the same lane of the select
    pts, bad = _select_rows(72, [(9, (8.0, -3.0))])
    for seed in range(200000):
        idx = cr.sample(seed, 2048, 72)
        good = ~np.isin(idx, bad).any(axis=1) & distinct(idx)
        v = np.flatnonzero(good)
        if len(v) >= 2 and v[0] >= 512 and ((v[1:] - v[0]) % SELECT_LANES == 0).any():
            break
    cases.append(Case("select_order", "same lane", pts, 2048, 3.0, seed, bad=bad, claims=dict(first=int(v[0]), valid=v.tolist())))
    # (c) a larger h has strictly more votes than every smaller one
    pts, bad = _select_rows(60, [(6, (8.0, -3.0)), (9, (-5.0, 11.0))])
    for seed in range(10000):
        c = Case("select_order", "later maximum", pts, 1024, 3.0, seed, bad=bad)
        w = c.want()
        smaller = w["votes_all"][:max(w["winner"], 0)][w["valid"][:max(w["winner"], 0)]]
        if w["winner"] >= 256 and len(smaller) and smaller.max() >= 6 and w["winner_votes"] > smaller.max():
            break
    c.claims = dict(first=int(np.flatnonzero(w["valid"])[0]), valid=np.flatnonzero(w["valid"]).tolist(), winner=w["winner"])
    cases.append(c)
    return cases


def _nan_rows(pts, bad):
    out = np.array(pts, F32)
    out[list(bad)] = np.nan
    return out


# ---------------------------------------------------------------------------------------------- non_finite
NF_M, NF_H, NF_SEED = 1100, 512, 3
#: (column of (x0, y0, x1, y1), value): second-list inf, -inf, NaN, +-3e38; first-list NaN and inf
NF_KINDS = ((2, np.inf), (3, -np.inf), (2, np.nan), (3, 3e38), (2, -3e38), (0, np.nan), (1, np.inf), (0, -np.inf))


@cached
def non_finite():
    """two cases.  "planted": claims drawn / undrawn = the rows that hold NF_KINDS[k] and are / are not drawn by the sample.
    "no votes": every valid hypothesis collects 0 votes"""
    M, H, seed = NF_M, NF_H, NF_SEED
    rng = np.random.default_rng(31)
    x0 = rng.uniform(0, 1000, M); y0 = rng.uniform(0, 1000, M)
    pts = np.stack([x0, y0, 1.01 * x0 - 0.02 * y0 + 12.5, 0.02 * x0 + 1.01 * y0 - 7.25], axis=1).astype(F32)
    idx = cr.sample(seed, H, M)
    hit = np.zeros(M, bool); hit[idx.reshape(-1)] = True
    undrawn_rows = np.flatnonzero(~hit)
    assert len(undrawn_rows) >= len(NF_KINDS)
    drawn, undrawn = [], []
    for k, (col, val) in enumerate(NF_KINDS):
        # in turn the first index of its triple (it then enters every difference), the second and the third
        h = [h for h in range(H) if distinct(idx[h:h + 1])[0] and not np.isin(idx[h], drawn).any()][3 * k + 1]
        r = int(idx[h, k % 3])
        pts[r, col] = val; drawn.append(r)
        r = int(undrawn_rows[k * (len(undrawn_rows) // len(NF_KINDS))])
        pts[r, col] = val; undrawn.append(r)
    cases = [Case("non_finite", "planted", pts, H, 3.0, seed, claims=dict(drawn=drawn, undrawn=undrawn))]
    # far from the origin and second-list positions near the top of the float32 range: the solve is finite in binary64, c and f
    # overflow float32, and in the vote a*x0 overflows: every error is inf or NaN, for the rows of the triple itself too
    M = 200
    x0 = 1e6 + rng.uniform(0, 10, M); y0 = 1e6 + rng.uniform(0, 10, M)
    x1 = rng.choice([-1.0, 1.0], M) * rng.uniform(1e38, 3.4e38, M); y1 = rng.choice([-1.0, 1.0], M) * rng.uniform(1e38, 3.4e38, M)
    seed = next(s for s in range(10000) if not distinct(cr.sample(s, 256, M)[:1])[0])         # hypothesis 0 is void
    cases.append(Case("non_finite", "no votes", np.stack([x0, y0, x1, y1], axis=1), 256, 3.0, seed))
    return cases


# ---------------------------------------------------------------------------------------------- all of them
FAMILIES = ("det_edge", "solve_rounding", "vote_ring", "vote_equal", "select_order", "non_finite", "tol_range")


def family(name):
    got = globals()[name]()
    return got if isinstance(got, list) else [got]


def all_cases():
    return [c for name in FAMILIES for c in family(name)]


def case_names():
    """(family, index) of every case, without building one"""
    count = dict(det_edge=1, solve_rounding=1, vote_ring=1, vote_equal=2, select_order=3, non_finite=2, tol_range=len(TOL_RANGE))
    return [(name, k) for name in FAMILIES for k in range(count[name])]


# ---------------------------------------------------------------------------------------------- the vote grid
CONS_TILE, CONS_HMAX, CONS_FOLD = 1024, 512, 256        # k_consensus.hpp: SIFT_CONS_TILE, SIFT_CONS_HMAX, SIFT_CONS_THREADS


def vote_grid(tiles, H):
    """match.hip, siftmi_match_consensus and launch_cb_vote: about 2048 workgroups, a chunk of at most CONS_HMAX and at least 16
    hypotheses.  dict(chunks, min_chunks, max_chunks, h_chunk)"""
    chunks = (2048 + tiles - 1) // tiles
    min_chunks, max_chunks = (H + CONS_HMAX - 1) // CONS_HMAX, (H + 15) // 16
    chunks = min(chunks, max_chunks)
    chunks = max(chunks, min_chunks)
    h_chunk = (H + chunks - 1) // chunks
    return dict(chunks=(H + h_chunk - 1) // h_chunk, min_chunks=min_chunks, max_chunks=max_chunks, h_chunk=h_chunk)


def tiles_of(pair_counts):
    """a single call: one count; a batch: tiles never straddle segments"""
    return int(sum(-(-int(m) // CONS_TILE) for m in np.atleast_1d(pair_counts)))


#: the batch cases whose workgroups walk more than CONS_FOLD hypotheses: (batch, n_hyp, h_chunk)
WIDE_BATCH_CASES = [("many", 520, 260), ("many", 1024, 512), ("many", 1025, 342)]
WIDE_SINGLE = dict(M=66561, n_hyp=8224, tol=3.0, seed=5, h_chunk=257)


@cached
def wide_single():
    """(kp1, kp2, pairs): 66 561 matches, about half of them with a pair outside its list"""
    kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(WIDE_SINGLE["M"], 0.6, 8100)
    rng = np.random.default_rng(8101)
    out = rng.random(len(pairs)) < 0.5
    pairs = pairs.copy()
    pairs[out, 0] = np.where(rng.random(out.sum()) < 0.5, len(kp1), -1)
    return kp1, kp2, pairs


def consensus_on_finite(kp1, kp2, pairs, n_hyp, tol, seed):
    """consensus_ref.consensus with the votes counted over the rows that are not NaN only (a NaN row never votes; the sample is
    still taken mod M, and a triple that draws a NaN row is void): the same dict, at the cost of the finite rows"""
    pts = cr.gather(kp1, kp2, pairs)
    M = pts.shape[0]
    assert M >= 3
    models, valid = cr.solve(pts, cr.sample(seed, n_hyp, M))
    finite = ~np.isnan(pts).any(axis=1)
    votes = cr.count_votes(np.ascontiguousarray(pts[finite]), models, tol)
    votes[~valid] = 0
    out = dict(mask=np.zeros(M, np.uint8), model=None, winner=-1, winner_votes=0, votes_all=votes, models_all=models, valid=valid, pts=pts)
    ranked = np.where(valid, votes.astype(np.int64), -1)
    w = int(np.argmax(ranked))
    if ranked[w] >= 0:
        out.update(winner=w, winner_votes=int(votes[w]), model=models[w].copy(), mask=cr.vote_matrix(pts, models[w], tol)[0].astype(np.uint8))
    return out
