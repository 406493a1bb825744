"""CPU proof that every family of tests/consensus_cases.py reaches the rule of the consensus contract it is named after, with the
restatement (tests/consensus_ref.py) alone and, for the two rounding families, against fused variants that are rounded exactly
once (fractions).  The counts asserted here are conditions on the INPUTS, not measurements of the product.  Then the chunk rule
of the vote grid: the wide cases give the h_chunk they claim, and the older cases never went above 256.  No kernel runs here."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import consensus_batch_ref as cb
import consensus_cases as cc
import consensus_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the exact arithmetic itself
def test_round_f32_rounds_once():
    q = Fraction(1) + Fraction(1, 2 ** 24) + Fraction(1, 2 ** 60)         # just above the middle of 1 and 1 + 2^-23
    assert F32(float(q)) == F32(1.0)                                      # twice: to 1 + 2^-24, then to even
    assert cc.round_f32(q) == F32(1.0) + F32(2.0 ** -23)
    assert cc.round_f32(Fraction(1) + Fraction(1, 2 ** 24)) == F32(1.0)                               # a tie goes to even
    assert cc.round_f32(Fraction(1) + Fraction(3, 2 ** 24)) == F32(1.0) + F32(2.0 ** -22)
    assert cc.round_f32(-q) == -(F32(1.0) + F32(2.0 ** -23)) and cc.round_f32(Fraction(0)) == 0
    rng = np.random.default_rng(0)
    for a, b, c in rng.uniform(-8, 8, (200, 3)).astype(F32):
        assert cc.fma32(a, b, F32(0)) == a * b and cc.fma32(a, F32(1), c) == a + c                   # one operation: the same rounding
        assert cc.fma64(float(a), float(b), 0.0) == float(a) * float(b)


def test_every_case_is_deterministic_and_small():
    names = [c.name for c in cc.all_cases()]
    assert len(names) == len(set(names)) == len(cc.case_names())
    for (family, k), c in zip(cc.case_names(), cc.all_cases()):
        assert cc.family(family)[k] is c and c.family == family
        assert c.M <= 1100 and c.n_hyp <= 2048 and np.isfinite(c.tol) and c.tol > 0
    before = cc.all_cases()
    cc._CACHE.clear()                                   # built again from nothing: the same bytes, the same seeds
    for c, d in zip(before, cc.all_cases()):
        assert d is not c and d.name == c.name and (d.n_hyp, d.tol, d.seed, d.bad) == (c.n_hyp, c.tol, c.seed, c.bad)
        assert np.array_equal(bits(d.pts), bits(c.pts)) and np.array_equal(d.pairs, c.pairs)
        assert d.kp1.tobytes() == c.kp1.tobytes() and d.kp2.tobytes() == c.kp2.tobytes()


# ---------------------------------------------------------------------------------------------- det_edge
def test_det_edge_has_every_class_on_both_sides_of_256():
    c = cc.det_edge()
    w, idx = c.want(), c.idx()
    det = cc.det_of(c.pts, idx)
    classes = c.claims["classes"]
    assert set(classes) == set(cc.DET_TRIPLES) | {"0 repeated"}
    for name, hs in classes.items():
        hs = np.asarray(hs)
        assert (hs < cc.DET_SPLIT).any() and (hs >= cc.DET_SPLIT).any(), name
        if name == "0 repeated":
            assert (~cc.distinct(idx[hs])).all() and not w["valid"][hs].any()
            assert not np.isnan(c.pts[idx[hs]]).any() and (det[hs] == 0).all()
            continue
        assert cc.distinct(idx[hs]).all(), name                         # distinct rows, also for "0 coincident"
        want = cc.DET_TRIPLES[name][2]
        assert np.isnan(det[hs]).all() if np.isnan(want) else (det[hs] == want).all(), (name, det[hs])
        assert (w["valid"][hs] == (name in cc.DET_VALID)).all(), name
        if name in cc.DET_VALID:                                        # the translation, exactly
            assert (w["models_all"][hs] == np.array([1, 0, cc.DET_SHIFT[0], 0, 1, cc.DET_SHIFT[1]], F32)).all(), name
        else:
            assert (bits(w["models_all"][hs]) == 0x7fc00000).all() and not w["votes_all"][hs].any(), name
    assert cc.BELOW64 < 1.0 and np.nextafter(cc.BELOW64, 2.0) == 1.0 and F32(cc.BELOW64) == 1.0        # binary32 cannot see it
    assert F32(cc.BELOW32) < 1 and np.nextafter(F32(cc.BELOW32), F32(2)) == 1
    # what a wrong threshold would change: > for >= loses the +-1 classes, a threshold of 0.5 admits five void classes
    assert (np.abs(det) == 1.0).sum() >= 6
    assert ((np.abs(det) >= 0.5) & (np.abs(det) < 1.0)).sum() >= 12


# ---------------------------------------------------------------------------------------------- solve_rounding
@pytest.mark.parametrize("form", [0, 1])
def test_solve_rounding_sees_a_fused_sum_of_products(form):
    c = cc.solve_rounding()
    idx = c.idx()
    models, valid = cr.solve(c.pts, idx)
    fused, valid_f = cc.solve_fused(c.pts, idx, form)
    assert np.array_equal(valid, valid_f) and valid.sum() >= 1900 and np.isfinite(models[valid]).all()
    differ = bits(models) != bits(fused)
    n_c, n_f = int(differ[valid][:, 2].sum()), int(differ[valid][:, 5].sum())
    print("%s: c of %d and f of %d of %d valid models change" % (cc.SOLVE_FORMS[form], n_c, n_f, valid.sum()))
    assert not differ[:, [0, 1, 3, 4]].any()
    assert n_c >= cc.SOLVE_MIN_CHANGED and n_f >= cc.SOLVE_MIN_CHANGED
    assert np.array_equal(bits(c.want()["models_all"]), bits(models))


# ---------------------------------------------------------------------------------------------- vote_ring
def test_vote_ring_probes_split_the_unfused_vote_from_each_fused_form():
    c = cc.vote_ring()
    w, idx = c.want(), c.idx()
    probes = c.claims["probes"]
    rows = [p[1] for p in probes]
    assert set(rows) == set(cc.RING_ROWS) and {0, 63, 64, 255, 256, 1023, 1024, c.M - 1} <= set(rows) and c.M > 1024
    targets = np.array([p[2] for p in probes])
    assert len(set(targets.tolist())) == len(probes) and (targets < 256).any() and (targets >= 256).any()
    assert not np.isin(idx[targets], rows).any() and w["valid"][targets].all()          # no probe moves a target's model
    per_place = dict((place, 0) for place in (1, 2, 3, 4))
    for place, row, h, unfused, fused in probes:
        model = w["models_all"][h]
        assert cr.vote_matrix(c.pts[row:row + 1], model, c.tol)[0, 0] == unfused == cc.vote_exact(model, c.pts[row], c.tol, 0)
        assert cc.vote_exact(model, c.pts[row], c.tol, place) == fused != unfused, (cc.PLACES[place], row, h)
        per_place[place] += 1
    assert min(per_place.values()) >= cc.RING_MIN_PER_PLACE, per_place
    # and the counts: a kernel that fuses place p is off by one at the target of each of its probes (more where probes coincide)
    for place in (1, 2, 3, 4):
        off = [h for p, row, h, u, f in probes if p == place]
        fused_votes = w["votes_all"][off] + [(-1 if u else 1) for p, row, h, u, f in probes if p == place]
        assert (fused_votes != w["votes_all"][off]).all()


# ---------------------------------------------------------------------------------------------- vote_equal, tol_range
def _errors(c):
    """float32 (ex, ey, t) of every row against the one model, operation by operation"""
    m = np.array([1, 0, cc.EQ_SHIFT[0], 0, 1, cc.EQ_SHIFT[1]], F32)
    with np.errstate(all="ignore"):
        ex = ((m[0] * c.pts[:, 0] + m[1] * c.pts[:, 1]) + m[2]) - c.pts[:, 2]
        ey = ((m[3] * c.pts[:, 0] + m[4] * c.pts[:, 1]) + m[5]) - c.pts[:, 3]
        return ex, ey, ex * ex + ey * ey


def _check_equal_rows(c, voting):
    w, at = c.want(), c.claims["rows"]
    model = np.array([1, 0, cc.EQ_SHIFT[0], 0, 1, cc.EQ_SHIFT[1]], F32)
    assert w["valid"].sum() >= 100 and (w["models_all"][w["valid"]] == model).all()      # exactly one model (b, d: 0 of either sign)
    assert not np.isin(c.idx(), list(at.values())).any()
    n_map = c.claims["first"]
    assert w["mask"][:n_map].all()
    assert sorted(n for n, r in at.items() if w["mask"][r]) == sorted(voting), c.name
    assert (w["votes_all"][w["valid"]] == n_map + len(voting)).all() and w["winner"] == int(np.flatnonzero(w["valid"])[0])


def test_vote_equal_rows_sit_exactly_on_the_tolerance():
    at5, below = cc.vote_equal()
    assert at5.tol == 5 and below.tol < 5 and np.nextafter(below.tol, F32(9)) == 5 and np.array_equal(bits(at5.pts), bits(below.pts))
    ex, ey, t = _errors(at5)
    at = at5.claims["rows"]
    for name, e in (("(3,4)", (3, 4)), ("(0,5)", (0, 5)), ("(5,0)", (5, 0)), ("(-4,3)", (-4, 3))):
        assert (ex[at[name]], ey[at[name]]) == e and t[at[name]] == at5.tol * at5.tol == 25
    r = at["(3,4)+ulp"]
    assert 3 < ex[r] < 3.001 and ey[r] == 4                                      # one ulp of x1 beyond
    assert t[r] > 25 and t[r] < 25.001
    assert below.tol * below.tol < 25
    tiny = ["1e-20", "-1e-20 y", "2e-20"]
    _check_equal_rows(at5, ["(3,4)", "(0,5)", "(5,0)", "(-4,3)"] + tiny)          # t == tol2 votes
    _check_equal_rows(below, tiny)                                                # one ulp less: they no longer do


def test_tol_range_reaches_inf_subnormal_and_zero():
    (n_inf, c_inf), (n_sub, c_sub), (n_zero, c_zero) = zip([n for n, _ in cc.TOL_RANGE], cc.tol_range())
    tiny_f32 = np.finfo(F32).tiny
    with np.errstate(all="ignore"):
        assert np.isinf(c_inf.tol * c_inf.tol) and np.isfinite(c_inf.tol)
        assert 0 < c_sub.tol * c_sub.tol < tiny_f32
        assert c_zero.tol > 0 and c_zero.tol * c_zero.tol == 0 and np.nextafter(F32(0), F32(1)) == c_zero.tol
    ex, ey, t = _errors(c_inf)
    at = c_inf.claims["rows"]
    assert np.isinf(t[[at["3e38"], at["inf"], at["-inf y"]]]).all() and np.isfinite(c_inf.pts[at["3e38"]]).all()
    assert ex[at["1e-20"]] == F32(1e-20) and ey[at["-1e-20 y"]] == F32(-1e-20) and ex[at["2e-20"]] == F32(2e-20)
    assert 0 < t[at["1e-20"]] == c_sub.tol * c_sub.tol < t[at["2e-20"]] < tiny_f32          # subnormal, equal to tol2 and above it
    assert (t[:c_inf.claims["first"]] == 0).all()
    _check_equal_rows(c_inf, list(cc.EQ_OFF))                                     # an inf error votes against tol2 = inf
    _check_equal_rows(c_sub, ["1e-20", "-1e-20 y"])
    _check_equal_rows(c_zero, [])                                                 # only an exact zero error


# ---------------------------------------------------------------------------------------------- select_order
def test_select_order_places_the_ties():
    first_pos, same_lane, later = cc.select_order()
    for c in (first_pos, same_lane, later):
        w = c.want()
        valid = np.flatnonzero(w["valid"])
        assert valid.tolist() == c.claims["valid"] and valid[0] == c.claims["first"] and len(c.bad) > 0.7 * c.M
        assert np.isnan(c.pts[list(c.bad)]).all() and not w["mask"][list(c.bad)].any()
    for c in (first_pos, same_lane):
        w = c.want()
        valid = np.flatnonzero(w["valid"])
        assert len(valid) >= 2 and len(set(w["votes_all"][valid].tolist())) == 1 and w["votes_all"][valid[0]] == c.M - len(c.bad)
        assert w["winner"] == valid[0] > 0
    valid = np.asarray(same_lane.claims["valid"])
    assert valid[0] >= 512 and ((valid[1:] - valid[0]) % cc.SELECT_LANES == 0).any()
    w = later.want()
    valid = np.flatnonzero(w["valid"])
    before = valid[valid < w["winner"]]
    assert w["winner"] == later.claims["winner"] >= 256 and len(before) >= 1 and valid[0] < w["winner"]
    assert (w["votes_all"][before] < w["winner_votes"]).all() and w["votes_all"][before].max() >= 6
    assert (w["votes_all"][valid] <= w["winner_votes"]).all()


# ---------------------------------------------------------------------------------------------- non_finite
def test_non_finite_rows_are_drawn_and_not_drawn_and_never_vote():
    planted, no_votes = cc.non_finite()
    w, idx = planted.want(), planted.idx()
    drawn, undrawn = planted.claims["drawn"], planted.claims["undrawn"]
    assert len(set(drawn + undrawn)) == 2 * len(cc.NF_KINDS)
    for k, (col, val) in enumerate(cc.NF_KINDS):
        for r in (drawn[k], undrawn[k]):
            got = planted.pts[r, col]
            assert (np.isnan(got) if np.isnan(val) else got == F32(val)) and np.isfinite(np.delete(planted.pts[r], col)).all()
    assert np.isin(drawn, idx).all() and not np.isin(undrawn, idx).any()
    assert not w["mask"][drawn + undrawn].any()
    models, valid = w["models_all"], w["valid"]
    odd = valid & ~np.isfinite(models).all(axis=1)
    print("planted: %d valid hypotheses with a coefficient that is not finite (%d with NaN, %d with inf)"
          % (odd.sum(), (valid & np.isnan(models).any(axis=1)).sum(), (valid & np.isinf(models).any(axis=1)).sum()))
    assert odd.sum() >= 4 and (valid & np.isnan(models).any(axis=1)).any() and (valid & np.isinf(models).any(axis=1)).any()
    assert not w["votes_all"][odd].any()
    assert (bits(models[~valid]) == 0x7fc00000).all()
    assert w["winner"] >= 0 and w["winner_votes"] == planted.M - 2 * len(cc.NF_KINDS)
    w = no_votes.want()
    valid = np.flatnonzero(w["valid"])
    assert len(valid) > 100 and not w["votes_all"].any() and not w["mask"].any()
    assert w["winner"] == valid[0] > 0 and w["winner_votes"] == 0
    assert np.isinf(w["models_all"][valid]).any(axis=1).all() and np.isfinite(no_votes.pts).all()


# ---------------------------------------------------------------------------------------------- the vote grid
def _define(name, text):
    return re.search(r"#define\s+%s\s+(.+?)\s*(//.*)?$" % name, text, re.M).group(1)


def test_restated_constants_and_chunk_rule_are_the_sources():
    hpp = open(os.path.join(ROOT, "sift_pyocl_amd", "csrc", "k_consensus.hpp")).read()
    threads, mpl = int(_define("SIFT_CONS_THREADS", hpp)), int(_define("SIFT_CONS_MPL", hpp))
    assert threads == cc.CONS_FOLD == cc.SELECT_LANES and threads * mpl == cc.CONS_TILE and int(_define("SIFT_CONS_HMAX", hpp)) == cc.CONS_HMAX
    assert "hh += SIFT_CONS_THREADS" in hpp
    src = open(os.path.join(ROOT, "sift_pyocl_amd", "csrc", "match.hip")).read()
    for stem in ("tiles", "n_tiles"):                   # the single call and the batch
        rule = (r"int chunks = \(2048 \+ %s - 1\) / %s;\s*"
                r"const int min_chunks = \(H \+ SIFT_CONS_HMAX - 1\) / SIFT_CONS_HMAX, max_chunks = \(H \+ 15\) / 16;\s*"
                r"if \(chunks > max_chunks\) chunks = max_chunks;\s*if \(chunks < min_chunks\) chunks = min_chunks;\s*"
                r"const int h_chunk = \(H \+ chunks - 1\) / chunks;\s*chunks = \(H \+ h_chunk - 1\) / h_chunk;") % (stem, stem)
        assert re.search(rule, src), stem


def test_wide_cases_give_the_chunks_they_claim_and_the_older_ones_never_did():
    import test_gpu_consensus_batch as tb
    W = cc.WIDE_SINGLE
    g = cc.vote_grid(cc.tiles_of(W["M"]), W["n_hyp"])
    assert cc.tiles_of(W["M"]) == 66 and g["h_chunk"] == W["h_chunk"] == 257 > cc.CONS_FOLD
    assert W["M"] // 2 * W["n_hyp"] * 1.1 <= 200000 * 2048                       # the CPU's cost: about half the rows are finite
    wide = [(name, H) for name, H, _ in cc.WIDE_BATCH_CASES]
    assert tb.CASES[-len(wide):] == wide
    for name, H, h_chunk in cc.WIDE_BATCH_CASES:
        batch = getattr(cb, name + "_batch")()
        g = cc.vote_grid(cc.tiles_of(batch.pair_counts), H)
        assert g["h_chunk"] == h_chunk > cc.CONS_FOLD and h_chunk <= cc.CONS_HMAX and g["chunks"] * h_chunk >= H
        assert (batch.pair_counts >= 3).sum() == 5 and batch.pair_counts.max() <= 64       # the CPU's cost is five small segments
    assert sorted(h for _, _, h in cc.WIDE_BATCH_CASES) == [260, 342, 512]          # one past the fold, in between, every counter
    # what the suite reached before: a single call per set of consensus_ref.SETS ...
    reached = 0
    for M, w, seed in cr.SETS:
        for H in (2048,) + ((5000, 7) if M <= 5000 else ()):
            reached = max(reached, cc.vote_grid(cc.tiles_of(M), H)["h_chunk"])
    assert reached == 187
    # ... and the crafted batches
    old = tb.CASES[:-len(wide)]
    assert len(old) == 18 and not set(old) & set(wide)
    assert max(cc.vote_grid(cc.tiles_of(getattr(cb, name + "_batch")().pair_counts), H)["h_chunk"] for name, H in old) == 18


def test_counting_over_the_finite_rows_is_the_restatement():
    kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(700, 0.6, 77)
    pairs = pairs.copy()
    out = np.random.default_rng(1).random(len(pairs)) < 0.4
    pairs[out, 1] = -1
    want = cr.consensus(kp1, kp2, pairs, 300, 3.0, 9)
    got = cc.consensus_on_finite(kp1, kp2, pairs, 300, 3.0, 9)
    assert want["winner"] >= 0 and 10 < want["valid"].sum() < 290
    for key in ("mask", "votes_all", "valid"):
        assert np.array_equal(got[key], want[key]), key
    assert np.array_equal(bits(got["models_all"]), bits(want["models_all"])) and np.array_equal(bits(got["model"]), bits(want["model"]))
    assert got["winner"] == want["winner"] and got["winner_votes"] == want["winner_votes"]
    kp1, kp2, pairs = cc.wide_single()
    assert len(pairs) == cc.WIDE_SINGLE["M"] and 0.45 < np.isnan(cr.gather(kp1, kp2, pairs)[:, 0]).mean() < 0.55
