"""CPU tests of the crafted match sets of the device fit (tests/fit_cases.py): every family is what it
claims -- the statuses exact rational arithmetic dictates are the restatement's, every ladder stands on both sides of the
threshold, the exact-moment families give the same bits on every grid, rounded_det has both signs -- an accepted fit is as
accurate as its conditioning allows, and every listed one-line mutant of the restatement differs from the contract on a named
family, so the GPU tests on the same sets (tests/test_gpu_fit_cases.py) would notice it in a kernel."""
from fractions import Fraction

import numpy as np
import pytest

import fit_cases as fc
import fit_ref as fr

GRIDS = (0, 1, 3, 7, 1024)


# ---------------------------------------------------------------------------------------------- families are what they claim
def test_dictated_statuses_are_the_restatements():
    for c in fc.all_cases():
        e = c.exact()
        assert e["status"] == c.dictated["status"] and e["n"] == c.dictated["n"], c.name         # the closed forms are exact()'s
        for blocks in (0, 1):
            w = c.want(blocks)
            assert w[fr.STATUS] == c.dictated["status"] and w[fr.N] == c.dictated["n"], (c.name, blocks, float(e.get("ratio", 0)))
            assert fc.solved_like(w), (c.name, blocks)
        if "ratio" in c.claims:
            assert e["ratio"] == c.claims["ratio"], c.name
        if "det" in c.claims:
            assert e["det"] == e["scale"] == c.claims["det"] and e["moments"][1] == 0, c.name
    assert set(c.family for c in fc.all_cases()) == set(fc.FAMILIES)


def test_every_ladder_has_rungs_on_both_sides():
    for name in fc.LADDERS:
        rungs = fc.ladder(name)
        ratios = [float(c.claims["ratio"]) for c in rungs]
        statuses = [c.dictated["status"] for c in rungs]
        print("%-12s N = %d .. %d: ratio %.5f .. %.5f" % (name, rungs[0].claims["N"], rungs[-1].claims["N"], ratios[0], ratios[-1]))
        assert len(rungs) == 2 * fc.RUNGS_PER_SIDE
        assert statuses.count(fr.OK) == fc.RUNGS_PER_SIDE and statuses.count(fr.DEGENERATE) == fc.RUNGS_PER_SIDE
        assert statuses[0] != statuses[-1] and sorted(ratios) in (ratios, ratios[::-1])          # one flip, in step 1
        assert 0.9 < min(ratios) < 1 < max(ratios) < 1.1
        assert all(600 < c.M < 800 for c in rungs) or name == "steep"
    big = fc.big_ladder()
    assert [c.dictated["status"] for c in big] == [fr.OK, fr.OK, fr.DEGENERATE, fr.DEGENERATE]
    assert max(c.M for c in fc.all_cases()) == fc.BIG_PAIRS == big[1].M and fr.default_blocks(fc.BIG_PAIRS) == 113
    assert 1e12 < big[1].want()[fr.MOMENTS][0] < 3e12
    # the regimes: relative (scale far above 1) on the sloped lines, absolute (det == scale below 1) on the axis-parallel ones
    for name in fc.LADDERS:
        for c in fc.ladder(name):
            e = c.exact()
            assert (e["scale"] < 1 and e["det"] == e["scale"]) if name in ("horizontal", "vertical") else e["scale"] > 1e12, c.name


def test_exact_moment_families_give_the_same_bits_on_every_grid():
    n = 0
    for c in fc.all_cases():
        if not c.exact_sums:
            continue
        first = c.want(0)
        for blocks in GRIDS[1:]:
            # status, n, means, moments and model; ssr too where the residuals are exactly 0.  A ladder's accepted model is
            # not exact (see the accuracy test), its residuals round, and their sum follows the grid
            got = c.want(blocks)
            assert fr.same_bits(got[:fr.SSR], first[:fr.SSR]), (c.name, blocks)
            assert fr.same_bits(got, first) or (c.family == "ladder_line" and c.dictated["status"] == fr.OK), (c.name, blocks)
        e = c.exact()                                       # and the bits are the exact values
        assert [Fraction(float(v)) for v in first[fr.MEANS]] == e["means"], c.name
        assert [Fraction(float(v)) for v in first[fr.MOMENTS]] == e["moments"], c.name
        if "means" in c.dictated:
            assert first[fr.MEANS].tolist() == list(c.dictated["means"]), c.name
        n += 1
    assert n >= 80
    assert not any(c.exact_sums for c in fc.rounded_det())


def test_dictated_models_and_residuals():
    n = 0
    for c in fc.all_cases():
        if "model" not in c.dictated:
            continue
        for blocks in GRIDS:
            w = c.want(blocks)
            assert w[fr.MODEL].tolist() == list(c.dictated["model"]), (c.name, blocks, w[fr.MODEL])
            assert w[fr.SSR] == 0.0 and not np.signbit(w[fr.SSR]), (c.name, blocks)
        assert [float(v) for v in c.exact()["model"]] == list(c.dictated["model"]), c.name
        n += 1
    assert n >= len(fc.EXACT_SETS) + 2 + 2


def test_tiny_cluster_turns_on_fmax_alone():
    statuses = {}
    for c in fc.tiny_cluster():
        e = c.exact()
        assert e["det"] == e["scale"] < 1 and e["det"] / (fc.THRESHOLD * e["scale"]) > 1          # without fmax: OK, every one
        statuses[c.name.split("/")[1]] = c.dictated["status"]
    assert statuses["j=8 m=1"] == statuses["j=9 m=1"] == fr.OK and statuses["j=10 m=1"] == statuses["j=11 m=1"] == fr.DEGENERATE
    assert statuses["j=11 m=4"] == fr.DEGENERATE and statuses["j=11 m=5"] == fr.OK
    by = dict((c.name.split("/")[1], float(c.exact()["ratio"])) for c in fc.tiny_cluster())
    print(by)
    assert abs(by["j=9 m=1"] - 14.55) < 0.01 and abs(by["j=10 m=1"] - 0.909) < 0.001


def test_huge_and_min_n_rows():
    five, mixed = fc.huge()
    assert five.want()[fr.MOMENTS][0] == 4 * fc.HUGE ** 2 > 3.5e77 and np.isfinite(five.want()).all()
    assert mixed.want()[fr.N] == 5 * fc.HUGE_COPIES and np.isfinite(mixed.want()).all()
    assert fr.same_bits(mixed.want(), fr.fit_pts(mixed.pts[::7]))                              # the rows in between add nothing
    unused = np.ones(mixed.M, bool); unused[::7] = False
    rows = mixed.pts[unused]
    assert np.isinf(rows).any() and np.isnan(rows).any() and (np.abs(rows[np.isfinite(rows)]) >= 3e38).any() and len(mixed.void) == 100
    kp1, kp2, pairs = mixed.lists()
    assert ((pairs[:, 0] < 0) | (pairs[:, 0] >= len(kp1)) | (pairs[:, 1] < 0) | (pairs[:, 1] >= len(kp2))).sum() == 100
    names = [c.name.split("/")[1] for c in fc.min_n()]
    assert names == ["triangle", "three on a line", "mask leaves 3", "mask leaves 2", "mask leaves 1"]
    assert [c.dictated["n"] for c in fc.min_n()] == [3, 3, 3, 2, 1]
    assert [c.dictated["status"] for c in fc.min_n()] == [fr.OK, fr.DEGENERATE, fr.OK, fr.DEGENERATE, fr.DEGENERATE]
    assert fr.default_blocks(fc.MIN_M) == 2 and [r // fr.T for r in fc.MIN_ROWS] == [0, 1, 1]


def test_rounded_det_has_both_signs():
    found, worst = fc.rounded_search()
    assert tuple(found) == fc.ROUNDED_SETS
    print("most negative computed det / scale %.3e (recorded %.3e)" % (worst, fc.ROUNDED_MOST_NEGATIVE))
    assert 8 * fc.ROUNDED_MOST_NEGATIVE <= worst <= 0 and fc.ROUNDED_MOST_NEGATIVE > -1e-14
    signs = []
    for c in fc.rounded_det():
        e = c.exact()
        assert e["det"] == 0 and e["scale"] > 1e12 and c.dictated["status"] == fr.DEGENERATE, c.name
        det = fc.computed_det(c.want())
        assert int(np.sign(det)) == c.claims["sign"], c.name
        signs.append(c.claims["sign"])
    assert signs.count(-1) >= 1 and signs.count(1) >= 1 and signs.count(0) >= 1


# ---------------------------------------------------------------------------------------------- accuracy against exact arithmetic
def deviation(c, blocks=0):
    """largest |coefficient - exact coefficient| of the restatement over a, b, d, e and over c, f; the exact map's largest
    |a, b, d, e|; and the reach 1 + |mx| + |my| through which an error of a, b arrives in c = mu - (a*mx + b*my)"""
    e, w = c.exact(), c.want(blocks)
    err = [float(abs(Fraction(float(v)) - q)) for v, q in zip(w[fr.MODEL], e["model"])]
    return (max(err[0], err[1], err[3], err[4]), max(err[2], err[5]), max(float(abs(e["model"][k])) for k in (0, 1, 3, 4)),
            1.0 + float(abs(e["means"][0]) + abs(e["means"][1])))


def test_accuracy_of_accepted_fits_follows_the_conditioning():
    """The ladders' accepted rungs: the error of a, b, d, e is at most a small multiple of 2^-53 scale / |det| max|a, b, d, e| --
    about 1e-4 at the threshold, some pixels across a 16 384 px frame -- and the error of c, f that multiple times the reach
    1 + |mx| + |my|.  The error follows the conditioning; it does not merely stay small."""
    u = 2.0 ** -53
    worst = 0.0
    print("%-34s %9s %10s %10s %10s %9s %10s" % ("rung", "ratio", "scale/det", "dev a,b,d,e", "dev c,f", "multiple", "px @16384"))
    for c in fc.ladder_line():
        if c.dictated["status"] != fr.OK:
            continue
        e = c.exact()
        cond = float(e["scale"] / abs(e["det"]))
        for blocks in (0, 1):
            lin, off, top, reach = deviation(c, blocks)
            multiple = max(lin / (u * cond * top), off / (u * cond * top * reach))
            worst = max(worst, multiple)
            if blocks == 0:
                print("%-34s %9.5f %10.3e %10.3e %10.3e %9.3f %10.3f" % (c.name.split("/")[1], float(e["ratio"]), cond, lin, off, multiple, lin * 16384))
            assert lin <= fc.ACCURACY_LADDER_MULTIPLE_BOUND * u * cond * top, (c.name, blocks, lin, multiple)
            assert off <= fc.ACCURACY_LADDER_MULTIPLE_BOUND * u * cond * top * reach, (c.name, blocks, off, multiple)
    print("largest multiple of 2^-53 scale/|det| max|a, b, d, e| %.4f (recorded %.4f, bound %.4f)" % (
        worst, fc.ACCURACY_LADDER_MULTIPLE_MEASURED, fc.ACCURACY_LADDER_MULTIPLE_BOUND))
    assert worst <= fc.ACCURACY_LADDER_MULTIPLE_BOUND
    # the families whose solve is exact: nothing to allow
    for c in fc.tiny_cluster() + fc.exact_fit() + fc.min_n() + fc.huge():
        if c.dictated["status"] == fr.OK:
            assert deviation(c)[:2] == (0.0, 0.0), c.name


def test_accuracy_of_well_conditioned_fits():
    """fit_ref.CASES up to 5000 pairs against the exact solution (test_fit_ref_host.py holds them against lstsq, another binary64 solver)"""
    u = 2.0 ** -53
    worst = 0.0
    for M, seed, outliers, extent in fr.CASES:
        if M > 5000:
            continue
        kp1, kp2, pairs, truth = fr.make_case(M, seed, outliers, extent)
        c = fc.Case("generic", "M=%d" % M, fr.gather(kp1, kp2, pairs))
        e = c.exact()
        assert e["status"] == fr.OK == c.want()[fr.STATUS]
        lin, off, top, reach = deviation(c)
        dev = max(lin, off)
        print("M = %5d: scale/det %.3f, deviation from the exact solution %.3e in a, b, d, e and %.3e in c, f" % (
            M, float(e["scale"] / e["det"]), lin, off))
        worst = max(worst, dev)
    print("largest %.3e (recorded %.3e, bound %.3e)" % (worst, fc.ACCURACY_GENERIC_MEASURED, fc.ACCURACY_GENERIC_BOUND))
    assert worst <= fc.ACCURACY_GENERIC_BOUND


# ---------------------------------------------------------------------------------------------- mutants of the restatement
def fma(a, b, c):
    """a * b + c rounded once to binary64 (int / int is correctly rounded)"""
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def reduce_any(v, B, dtype=np.float64):
    """fit_ref.reduce_R with the accumulators in `dtype`"""
    v = np.asarray(v, dtype)
    M, G = v.shape[0], B * fr.T
    K = max(1, -(-M // G))
    rows = np.zeros((K, G), dtype)
    rows.reshape(-1)[:M] = v
    lane = np.zeros(G, dtype)
    for k in range(K):
        lane = lane + rows[k]
    w = lane.reshape(B, fr.T).copy()
    s = fr.T // 2
    while s >= 1:
        w[:, :s] = w[:, :s] + w[:, s:2 * s]
        s //= 2
    total = dtype(0.0)
    for b in range(B):
        total = total + w[b, 0]
    return np.float64(total)


def reduce_fused(p, q, used, B):
    """R(p*q) with step (i) contracted: a lane's sum = fma(p, q, sum)"""
    M, G = len(p), B * fr.T
    lane = [0.0] * G
    for j in np.flatnonzero(used):
        lane[j % G] = fma(p[j], q[j], lane[j % G])
    return reduce_any(np.asarray(lane), B)              # the G lane sums, one per lane: steps (ii) and (iii) as they are


def variant(pts, mask=None, blocks=0, m=None):
    """fit_ref.fit_pts with ONE line changed, named by m (None: the contract itself)"""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    M = pts.shape[0]
    out = np.full(20, np.nan, np.float64)
    used = np.isfinite(pts).all(axis=1)
    if mask is not None:
        used &= np.asarray(mask).reshape(-1) != 0
    n = int(used.sum())
    out[fr.STATUS], out[fr.N] = fr.EMPTY, 0.0
    if n == 0:
        return out
    B = blocks if blocks else fr.default_blocks(M)
    p = pts.astype(np.float64)
    zero = np.float64(0.0)
    acc = np.float32 if m == "float32 accumulation" else np.float64

    def R(v):
        return reduce_any(np.where(used, v, zero), B, acc)

    def RP(s, t):
        return reduce_fused(s, t, used, B) if m == "fused X*X + s" else R(s * t)
    with np.errstate(all="ignore"):
        x0, y0, x1, y1 = (np.where(used, p[:, k], zero) for k in range(4))
        nd = np.float64(n)
        if m == "means by 1/n":
            inv = np.float64(1.0) / nd
            mx, my, mu, mv = R(x0) * inv, R(y0) * inv, R(x1) * inv, R(y1) * inv
        else:
            mx, my, mu, mv = R(x0) / nd, R(y0) / nd, R(x1) / nd, R(y1) / nd
        if m == "sums not centred":
            Sxx, Sxy, Syy = R(x0 * x0) - nd * mx * mx, R(x0 * y0) - nd * mx * my, R(y0 * y0) - nd * my * my
            Sxu, Syu, Sxv, Syv = R(x0 * x1) - nd * mx * mu, R(y0 * x1) - nd * my * mu, R(x0 * y1) - nd * mx * mv, R(y0 * y1) - nd * my * mv
        else:
            X, Y, U, V = x0 - mx, y0 - my, x1 - mu, y1 - mv
            Sxx, Sxy, Syy = RP(X, X), RP(X, Y), RP(Y, Y)
            Sxu, Syu, Sxv, Syv = RP(X, U), RP(Y, U), RP(X, V), RP(Y, V)
        out[fr.N] = nd
        out[fr.MEANS] = mx, my, mu, mv
        out[fr.MOMENTS] = Sxx, Sxy, Syy, Sxu, Syu, Sxv, Syv
        scale = Sxx * Syy
        det = scale - Sxy * Sxy
        if m == "scale = Sxx + Syy":
            scale = Sxx + Syy
        thr = np.float64({"threshold 1e-11": 1e-11, "threshold 1e-13": 1e-13}.get(m, 1e-12))
        floor = scale if m == "no fmax" else max(np.float64(1.0), scale)
        size = det if m == "no fabs" else abs(det)
        if n < (4 if m == "n < 4" else 3) or not (size > thr * floor):
            out[fr.STATUS] = fr.DEGENERATE
            return out
        if m == "Sxx and Syy exchanged":
            a = (Sxu * Sxx - Syu * Sxy) / det; b = (Syu * Syy - Sxu * Sxy) / det
            d = (Sxv * Sxx - Syv * Sxy) / det; e = (Syv * Syy - Sxv * Sxy) / det
        elif m == "Sxy with the wrong sign":
            a = (Sxu * Syy + Syu * Sxy) / det; b = (Syu * Sxx + Sxu * Sxy) / det
            d = (Sxv * Syy + Syv * Sxy) / det; e = (Syv * Sxx + Sxv * Sxy) / det
        else:
            a = (Sxu * Syy - Syu * Sxy) / det; b = (Syu * Sxx - Sxu * Sxy) / det
            d = (Sxv * Syy - Syv * Sxy) / det; e = (Syv * Sxx - Sxv * Sxy) / det
        if m == "c = (mu - a*mx) - b*my":
            c = (mu - a * mx) - b * my; f = (mv - d * mx) - e * my
        else:
            c = mu - (a * mx + b * my); f = mv - (d * mx + e * my)
        if m == "fused a*x0 + b*y0":
            px = np.array([fma(a, s, b * t) for s, t in zip(x0, y0)]); py = np.array([fma(d, s, e * t) for s, t in zip(x0, y0)])
        else:
            px, py = a * x0 + b * y0, d * x0 + e * y0
        ex, ey = (px + c) - x1, (py + f) - y1
        out[fr.STATUS] = fr.OK
        out[fr.MODEL] = a, b, c, d, e, f
        out[fr.SSR] = R(ex * ex + ey * ey)
    return out


def named(family, only=None):
    cases = fc.ladder(family) if family in fc.LADDERS else fc.family(family)
    return [c for c in cases if only is None or only in c.name]


#: mutant -> (the family or ladder that must show it, blocks): each differs from the contract there in status or in bits.  The
#: contraction of the sums runs with one workgroup -- under the default grid a lane of these sets owns one pair and
#: fma(X, X, +0.0) is X*X
MUTANTS = {
    "no fmax": ("tiny_cluster", 0),
    "threshold 1e-11": ("diagonal", 0),
    "threshold 1e-13": ("diagonal", 0),
    "scale = Sxx + Syy": ("steep", 0),
    "n < 4": ("min_n", 0),
    "sums not centred": ("moved 32768", 0),
    "float32 accumulation": ("anti", 0),
    "fused X*X + s": ("rounded_det", 1),
    "fused a*x0 + b*y0": ("moved apart", 0),
    "c = (mu - a*mx) - b*my": ("moved apart", 0),
    "Sxx and Syy exchanged": ("exact_fit", 0),
    "Sxy with the wrong sign": ("exact_fit", 0),
    "means by 1/n": ("exact_fit", 0),
}


def test_the_variant_without_a_change_is_the_restatement():
    for c in fc.all_cases():
        if c.M > 1000:
            continue
        for blocks in (0, 1):
            assert fr.same_bits(variant(c.pts, c.mask, blocks), c.want(blocks)), (c.name, blocks)


@pytest.mark.parametrize("m", sorted(MUTANTS))
def test_every_mutant_is_caught_by_its_family(m):
    where, blocks = MUTANTS[m]
    caught, flipped = [], []
    for c in named(where):
        got = variant(c.pts, c.mask, blocks, m)
        if not fr.same_bits(got, c.want(blocks)):
            caught.append(c.name)
            if got[fr.STATUS] != c.dictated["status"]:
                flipped.append(c.name)
    print("%s: differs on %d of %d sets of %s, %d of them in status" % (m, len(caught), len(named(where)), where, len(flipped)))
    assert caught, (m, where)
    # the mutants of the rule itself are seen in the status, which exact arithmetic dictates
    if m in ("no fmax", "threshold 1e-11", "threshold 1e-13", "scale = Sxx + Syy", "n < 4", "sums not centred"):
        assert flipped, (m, where)
    # the mutants of the solve leave the returned moments alone: solve_from_results notices them by itself
    if m in ("Sxx and Syy exchanged", "Sxy with the wrong sign", "c = (mu - a*mx) - b*my", "no fmax", "threshold 1e-11", "threshold 1e-13",
             "scale = Sxx + Syy", "n < 4"):
        assert any(not fc.solved_like(variant(c.pts, c.mask, blocks, m)) for c in named(where)), m


def test_each_threshold_mutant_flips_one_side_of_every_ladder():
    for name in fc.LADDERS:
        for m, side in (("threshold 1e-11", fr.OK), ("threshold 1e-13", fr.DEGENERATE)):
            for c in fc.ladder(name):
                got = variant(c.pts, c.mask, 0, m)[fr.STATUS]
                assert (got != c.dictated["status"]) == (c.dictated["status"] == side), (name, m, c.name)
    for c in fc.ladder("horizontal") + fc.ladder("vertical"):           # the absolute regime is fmax's as well
        assert variant(c.pts, c.mask, 0, "no fmax")[fr.STATUS] == fr.OK
    # exchanged moments on the two axis-parallel ladders: one of Sxx, Syy is 2 k^2 there
    for name in ("horizontal", "vertical"):
        assert any(not fr.same_bits(variant(c.pts, c.mask, 0, "Sxx and Syy exchanged"), c.want()) for c in fc.ladder(name))


def test_variants_that_cannot_be_observed_are_not():
    """det without fabs: no set here has a computed det below -1e-12 max(1, scale) (fit_cases' docstring argues none can)"""
    for c in fc.all_cases():
        if c.M > 1000:
            continue
        for blocks in (0, 1):
            assert fr.same_bits(variant(c.pts, c.mask, blocks, "no fabs"), c.want(blocks)), (c.name, blocks)
    # two pairs: det is exactly 0 or rounding noise, the clause n < 3 decides nothing
    rng = np.random.default_rng(2)
    for k in range(200):
        pts = (rng.uniform(-1, 1, (2, 4)) * 10.0 ** rng.integers(-3, 5)).astype(np.float32)
        w = fr.fit_pts(pts)
        scale = w[fr.MOMENTS][0] * w[fr.MOMENTS][2]
        assert abs(fc.computed_det(w)) <= 1e-15 * max(1.0, scale), pts
