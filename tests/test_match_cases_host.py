"""CPU side of the crafted matching lists (tests/match_cases.py): the generator does what it says, and on every family the GPU
tests use, the oracle's matcher, the numpy restatement (tests/window_ref.py with an infinite window), the answer the
construction dictates and -- through tests/golden/match_crafted.npz -- the reference's own kernel agree exactly."""
import os
import time

import numpy as np
import pytest

import match_cases as mc
import window_ref as wr
from util import sort_rows

HOST_N1 = 2                      # the queries are identical: two of them say what six hundred would
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "match_crafted.npz")


def rows_of(pairs):
    return sort_rows(np.asarray(pairs, np.int32).reshape(-1, 2))


# ---------------------------------------------------------------------------------------------- the generator
def test_prescribed_distances_are_exact():
    rng = np.random.default_rng(0)
    base = mc.make_base(rng)
    assert set(np.unique(base)) == {0, 255}
    for lane in range(4):                                            # both directions of |a - b| in every byte of a dword
        assert set(np.unique(base[lane::4])) == {0, 255}
    dists = np.concatenate([np.arange(0, 300), np.arange(300, mc.DMAX - 300, 37), np.arange(mc.DMAX - 300, mc.DMAX + 1)])
    t0 = time.perf_counter()
    d = mc.descs_at(base, dists, rng)
    took = time.perf_counter() - t0
    assert d.dtype == np.uint8 and d.shape == (len(dists), 128)
    assert np.array_equal(mc.l1(base, d), dists)
    assert took < 1.0, "%d descriptors took %.2f s: the generator must stay vectorised" % (len(dists), took)
    delta = np.abs(d.astype(np.int64) - base.astype(np.int64))
    mid = (dists >= 1020) & (dists <= mc.DMAX - 1020)
    assert ((delta[mid] == 0).any(axis=1) & (delta[mid] == 255).any(axis=1)).all()          # some bytes equal, some opposite
    for lane in range(4):                                            # every byte of the dwords carries differences, irregular ones
        assert (delta[mid][:, lane::4].sum(axis=1) > 0).mean() > 0.99
    low = (dists >= 1020) & (dists <= 20000)
    assert (np.array([len(np.unique(r)) for r in delta[low][::20]]) > 8).all()
    assert (d[-1] == 255 - base).all() and (d[0] == base).all()
    one = mc.desc_at(base, 12345, rng)
    assert one.shape == (128,) and mc.l1(base, one) == 12345
    # planted(): the planted distances where asked, everything else above them
    b = mc.planted(base, 130, {5: 17380, 129: 32614}, rng)
    dist = mc.l1(base, b["desc"])
    assert dist[5] == 17380 and dist[129] == 32614 and (np.delete(dist, [5, 129]) > 32614).all()
    assert np.array_equal(mc.queries(base, 7)["desc"], np.repeat(base[None], 7, axis=0))


def test_critical_ratio_pairs():
    pairs = mc.critical_ratio_pairs(mc.RATIO)
    assert len(pairs) == 37 and len(set(pairs)) == 37
    th = mc.RATIO
    exact = [(a, b) for a, b in pairs if np.float32(a) / np.float32(b) == th]
    assert len(exact) == 32
    assert {(3361, 6307), (5329, 10000), (17380, 32614)} <= set(exact)
    assert sum(mc.passes(a, b, th) for a, b in pairs) == 5
    for a, b in set(pairs) - set(exact):                             # one of the other forms decides differently
        f1, f2 = np.float32(a), np.float32(b)
        rule = f1 / f2 < th
        assert (f1 < th * f2) != rule or (f1 * (np.float32(1) / f2) < th) != rule or (a / b < float(th)) != rule
    for th in (np.float32(0.5), np.float32(1.0)):
        p = mc.critical_ratio_pairs(th)
        assert 20 <= len(p) <= 96 and all(0 <= a <= b <= mc.DMAX for a, b in p)
        assert any(np.float32(a) / np.float32(b) == th for a, b in p)
    # what the multiplied form gets wrong is in the default set: the test it replaces must see at least one such pair
    assert any((np.float32(a) < mc.RATIO * np.float32(b)) != (np.float32(a) / np.float32(b) < mc.RATIO) for a, b in pairs)


@pytest.mark.parametrize("n2", mc.SIZES)
def test_placements(n2):
    pl = mc.placements(n2)
    if n2 == 1:
        assert pl == [(0, None)]
        return
    assert len(set(pl)) == len(pl)
    assert all(0 <= p < n2 and 0 <= q < n2 and p != q for p, q in pl)
    assert all((q, p) in pl for p, q in pl)                          # both orders
    used = {p for e in pl for p in e}
    want = {0, 1, n2 - 1} | {e for k in range(64, n2 + 1, 64) for e in (k - 1, k, k + 1) if e < n2}
    assert used == {p for p in want if 0 <= p < n2}
    if n2 > 128:
        assert any(p // 64 == q // 64 and p >= 64 for p, q in pl)                # one later tile
        assert any(abs(p // 64 - q // 64) == 1 for p, q in pl)                   # adjacent tiles
        assert any(abs(p - q) == 1 and p // 64 != q // 64 for p, q in pl)        # the two sides of an edge


# ---------------------------------------------------------------------------------------------- oracle == restatement == construction
@pytest.mark.parametrize("name", mc.PLAIN_FAMILIES)
def test_oracle_restatement_and_construction_agree(oracle, name):
    seen = 0
    for c in mc.family(name, HOST_N1):
        assert np.array_equal(c.a["desc"][0], c.a["desc"][-1])
        want, n = oracle.match(c.a, c.b, ratio_th=c.th)
        got = wr.match(c.a, c.b, np.inf, ratio_th=c.th)
        assert n == len(want) == len(got), c.name
        assert np.array_equal(rows_of(want), rows_of(got)), c.name
        assert c.best is not mc.UNKNOWN
        assert np.array_equal(rows_of(want), c.expected_rows()), c.name
        ex, n_ex = oracle.match_ex(c.a, c.b, None, 0, ratio_th=c.th)
        assert n_ex == n and np.array_equal(rows_of(ex), rows_of(want)), c.name
        seen += 1
    assert seen >= (1 if name.endswith(" 1") else 4)


def test_families_hold_what_they_promise():
    """both outcomes at every size, ties whose winner is not the first planted, the largest distance, the extra pairs of 1.0"""
    for n2 in mc.SIZES:
        cases = list(mc.family("placement %d" % n2, HOST_N1))
        assert {c.best is None for c in cases} == ({False} if n2 == 1 else {False, True})
    ties = list(mc.family("ties 320", HOST_N1))
    assert any(c.best != c.planted[0] for c in ties) and any(len(c.planted) == 3 for c in ties) and any(len(c.planted) == 5 for c in ties)
    assert any("earlier" in c.name for c in ties) and any("later" in c.name for c in ties)
    assert all(c.th == 2.0 and c.best == min(c.planted) for c in ties)
    one = {c.name: c for c in mc.family("ratio 1.0", HOST_N1)}
    assert any("d=(32639, 32640)" in k and c.best is not None for k, c in one.items())
    assert any("d=(32640, 32640)" in k and c.best is None for k, c in one.items())
    assert any(c.best is not None for c in mc.family("ratio default", HOST_N1)) and any(c.best is None for c in mc.family("ratio default", HOST_N1))
    inf = [c for c in mc.family("odd thresholds", HOST_N1) if c.th == np.inf]
    assert any(c.best is None for c in inf) and any(c.best is not None for c in inf)
    assert all(c.best is None for c in mc.family("odd thresholds", HOST_N1) if not c.th > 0)


def test_mutual_duplicates(oracle):
    for c in mc.mutual_cases():
        want, n = oracle.match_ex(c.a, c.b, None, 0, mutual=True, ratio_th=c.th)
        got = wr.match(c.a, c.b, np.inf, mutual=True, ratio_th=c.th)
        assert n == len(want) == len(got) and np.array_equal(rows_of(want), rows_of(got)), c.name
        i_a, i_b = c.planted
        back = wr.scan(c.a, c.b, np.inf, reverse=True)[0]
        assert back[70] == i_a, c.name                               # the earlier of the duplicates is the nearest of the minimum
        with_min = rows_of(want)[rows_of(want)[:, 1] == 70]
        assert with_min.tolist() == [[i_a, 70]], c.name
        fwd = rows_of(oracle.match(c.a, c.b, ratio_th=c.th)[0])
        assert [i_b, 70] in fwd.tolist(), c.name                     # without the reverse check the later duplicate pairs too


def test_flag_cases(oracle):
    """the masked cases against the restatement without flags (an excluded keypoint deleted, a forced zero made a copy of the
    queries' descriptor) and against the answer the construction dictates"""
    seen = set()
    for c in mc.flag_cases(6):
        want, n = oracle.match_ex(c.a, c.b, c.roi, c.roi_mode, mutual=c.mutual, ratio_th=c.th)
        a2, b2, ia, ib = mc.flags_restated(c)
        got = wr.match(a2, b2, np.inf, mutual=c.mutual, ratio_th=c.th)
        got = np.stack([ia[got[:, 0]], ib[got[:, 1]]], axis=1).astype(np.int32) if len(got) else got
        if len(b2) == 0 and c.th > 1:        # nothing left to scan and 1e12 / 1e12 < ratio_th: the restatement has no index to offer,
            got = c.expected_rows()          # the rule's is the 0 it starts from
        assert n == len(want) == len(got) and np.array_equal(rows_of(want), rows_of(got)), c.name
        if c.best is not mc.UNKNOWN and not c.mutual:
            assert np.array_equal(rows_of(want), c.expected_rows()), c.name
        seen.add((c.roi_mode, c.mutual, n > 0))
    assert {(m, p) for m, _, p in seen} == {(m, p) for m in (1, 2) for p in (False, True)}      # both modes, both outcomes
    assert {(m, u) for m, u, _ in seen} == {(m, u) for m in (1, 2) for u in (False, True)}


def test_positions_for_finite_windows():
    """spread_over_spots keeps the planted answer for the queries on spot 0; tied_in_different_cells keeps every element a
    candidate, the tied ones in two cells with the earliest index in the later cell"""
    for name in ("ratio default", "ties 320"):
        for c in list(mc.family(name, 12))[:20]:
            a, b = mc.spread_over_spots(c)
            got = wr.match(a, b, mc.SPOT_WINDOW, ratio_th=c.th)
            on0 = np.nonzero((a["x"] == mc.SPOTS[0, 0]) & (a["y"] == mc.SPOTS[0, 1]))[0]
            assert len(on0) == 9
            sub = got[np.isin(got[:, 0], on0)]
            want = np.zeros((0, 2), np.int32) if c.best is None else np.stack([on0, np.full(len(on0), c.best)], axis=1)
            assert np.array_equal(rows_of(sub), want), c.name
            lonely = got[np.isin(got[:, 0], np.nonzero(a["x"] == mc.SPOTS[3, 0])[0])]
            # no candidate: both distances stay 1e12, the ratio is 1 -- no pair, unless the threshold is above 1 (then best is -1)
            assert (len(lonely) == 0) if c.th <= 1 else (len(lonely) > 0 and (lonely[:, 1] == -1).all()), c.name
    for c in mc.family("ties 320", 3):
        a, b = mc.tied_in_different_cells(c)
        assert wr.candidate_matrix(a, b, mc.SPOT_WINDOW).all()
        assert np.array_equal(rows_of(wr.match(a, b, mc.SPOT_WINDOW, ratio_th=c.th)), c.expected_rows()), c.name
        if len(c.planted) > 1:
            first, second = sorted(c.planted)[:2]
            assert np.floor((b["x"][first] + 2.0) / mc.SPOT_WINDOW) > np.floor((b["x"][second] + 2.0) / mc.SPOT_WINDOW)


# ---------------------------------------------------------------------------------------------- the reference's own kernel
def test_reference_kernel_pins(oracle):
    """tests/golden/match_crafted.npz: what the reference's `matching`, built natively, answered on the critical-ratio, odd-threshold,
    extreme and tie lists (tests/golden/make_match_crafted.py).  The inputs are regenerated here and checked by digest."""
    z = np.load(GOLDEN)
    assert [str(s) for s in z["families"]] == list(mc.GOLDEN_FAMILIES)
    n1 = int(z["n1"])
    paired = 0
    for k, name in enumerate(mc.GOLDEN_FAMILIES):
        cases = list(mc.family(name, n1))
        assert mc.digest(cases) == str(z["digest_%d" % k]), "%s: the generated inputs are not the ones the fixture was made from" % name
        pairs, off, totals = z["pairs_%d" % k], z["offsets_%d" % k], z["totals_%d" % k]
        assert len(totals) == len(cases) and len(off) == len(cases) + 1
        for i, c in enumerate(cases):
            ref = pairs[off[i]:off[i + 1]]
            want, n = oracle.match(c.a, c.b, ratio_th=c.th)
            assert n == totals[i] == len(ref), c.name
            assert np.array_equal(rows_of(want), rows_of(ref)), c.name
            assert np.array_equal(rows_of(ref), c.expected_rows()), c.name
            paired += n > 0
    assert paired > 100
