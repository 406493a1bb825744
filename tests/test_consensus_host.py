"""CPU tests of the consensus filter: the entry point is declared, exported and bound, and the numpy
restatement the GPU test compares against (tests/consensus_ref.py) is sane on the inputs that test uses and on the edge cases
of the contract.  No kernel runs here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import consensus_ref as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_HYP, TOL = 2048, 3.0


def test_symbol_is_declared_exported_and_bound():
    from sift_pyocl_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "siftmi.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+siftmi_match_consensus\s*\(", header)
    assert "siftmi_match_consensus" in _lib.exported_symbols()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    fn = L.siftmi_match_consensus
    assert fn.restype is C.c_int and len(fn.argtypes) == 20
    # argument checks come before anything touches a device: a null matcher is refused with EINVAL on any machine
    w = C.c_int32(7)
    assert fn(None, None, 0, 0, None, 0, 0, None, 0, 0, 16, C.c_float(3.0), 0, None, None, C.byref(w), None, None, None, None) == _lib.EINVAL
    import sift_pyocl_amd as sp
    assert callable(getattr(sp.MatchPlan, "consensus"))
    if L.siftmi_device_count() < 1:
        with pytest.raises(RuntimeError):          # as before: no device, no plan, no CPU fallback
            sp.MatchPlan()


def test_mixer_and_sampler_follow_the_contract_text():
    """scalar Python integers against the vectorised form"""
    def mix1(v):
        v &= 0xFFFFFFFF
        v ^= v >> 16; v = (v * 0x7FEB352D) & 0xFFFFFFFF; v ^= v >> 15; v = (v * 0x846CA68B) & 0xFFFFFFFF; v ^= v >> 16
        return v
    for seed in (0, 1, 0xFFFFFFFF, 0xDEADBEEF):
        for M in (3, 257, 200000):
            got = cr.sample(seed, 50, M)
            want = [[mix1(seed + 0x9E3779B9 * (3 * h + k + 1)) % M for k in range(3)] for h in range(50)]
            assert got.tolist() == want
    assert mix1(0) == 0 and int(cr.mix(np.array([1]))[0]) == mix1(1)


@pytest.mark.parametrize("M,w,seed", cr.SETS)
def test_restatement_is_sane_on_the_gpu_test_inputs(M, w, seed):
    """A condition on the INPUTS of tests/test_gpu_consensus.py, not a measurement of the product: with the construction's
    labels as truth the restatement's mask has precision >= 0.99 and recall >= 0.95, and the least-squares fit on it lands on
    the ground-truth map.  All nine sets of cr.SETS met the bounds at their first seed: none was re-seeded or dropped."""
    kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(M, w, seed)
    assert not np.array_equal(pairs[:, 0], np.arange(M)) and len(set(pairs[:, 0].tolist())) == M      # an injection, not the identity
    r = cr.consensus(kp1, kp2, pairs, N_HYP, TOL, 0)
    mask = r["mask"].astype(bool)
    assert r["winner"] >= 0 and r["winner_votes"] == mask.sum() == r["votes_all"].max()
    tp = (mask & inlier).sum()
    precision, recall = tp / mask.sum(), tp / inlier.sum()
    p = r["pts"]
    fit = cr.lstsq_affine(p[mask, 0], p[mask, 1], p[mask, 2], p[mask, 3])
    fit_all = cr.lstsq_affine(p[:, 0], p[:, 1], p[:, 2], p[:, 3])
    err, err_all = cr.corner_error(fit, truth), cr.corner_error(fit_all, truth)
    # The fit's bound is 0.1 px wherever the construction supports it.  It does for N >= 1500 true inliers; it cannot for the
    # M = 200 sets (60 - 180 inliers): a least-squares affine fit on N points uniform in the frame with position noise sigma
    # predicts a frame corner with variance sigma^2 (1/N + 3/N + 3/N) per coordinate (the corner lies half a frame from the
    # mean on both axes, a uniform coordinate has variance L^2 / 12), i.e. sigma sqrt(14 / N) for the distance -- 0.08 to 0.14 px
    # here, measured 0.19 / 0.20 px at w = 0.5 / 0.3 (max over four corners).  Those sets are held to four of these sigmas.
    n_true = int(inlier.sum())
    bound = 0.1 if n_true >= 1500 else 4.0 * cr.NOISE_SIGMA * np.sqrt(14.0 / n_true)
    print("M=%d w=%.1f seed=%d: winner %d with %d votes, precision %.4f recall %.4f, fit on the mask off by %.4f px (bound %.3f), "
          "fit on all matches off by %.1f px" % (M, w, seed, r["winner"], r["winner_votes"], precision, recall, err, bound, err_all))
    assert precision >= 0.99 and recall >= 0.95
    assert err <= bound
    if w == 0.5:
        assert err_all > 10.0


def _records(xy):
    kp = np.zeros(len(xy), cr.DTYPE_KP)
    if len(xy):
        kp["x"] = np.asarray(xy, np.float32)[:, 0]; kp["y"] = np.asarray(xy, np.float32)[:, 1]
    return kp


def _identity_pairs(n):
    return np.stack([np.arange(n, dtype=np.int32)] * 2, axis=1)


@pytest.mark.parametrize("M", [0, 1, 2])
def test_fewer_than_three_matches_have_no_winner(M):
    xy = [(10.0 * i, 7.0 * i * i) for i in range(M)]
    r = cr.consensus(_records(xy), _records(xy), _identity_pairs(M), 64, TOL, 5)
    assert r["winner"] == -1 and r["model"] is None and r["mask"].shape == (M,) and not r["mask"].any()
    assert not r["votes_all"].any() and np.isnan(r["models_all"]).all()


def test_identical_or_collinear_points_void_every_triple():
    for xy in ([(5.0, 9.0)] * 40, [(3.0 * i, 2.0 * i + 1.0) for i in range(40)]):
        r = cr.consensus(_records(xy), _records(xy), _identity_pairs(40), 256, TOL, 1)
        assert not r["valid"].any() and r["winner"] == -1 and not r["mask"].any()
        assert not r["votes_all"].any() and np.isnan(r["models_all"]).all()


def test_repeated_index_voids_its_triple_and_ties_go_to_the_smaller_h():
    # three matches on an exact shift: every triple without a repeat is a permutation of (0, 1, 2), solves to the same map and
    # collects all three votes -- a tie between all of them, which the smallest such h wins; triples with a repeat are void
    a = [(0.0, 0.0), (100.0, 0.0), (0.0, 100.0)]
    b = [(x + 8.0, y - 3.0) for x, y in a]
    H = 200
    r = cr.consensus(_records(a), _records(b), _identity_pairs(3), H, TOL, 11)
    idx = cr.sample(11, H, 3)
    distinct = np.array([len(set(t)) == 3 for t in idx.tolist()])
    assert distinct.any() and (~distinct).any()
    assert np.array_equal(r["valid"], distinct)
    assert np.isnan(r["models_all"][~distinct]).all() and not r["votes_all"][~distinct].any()
    assert (r["votes_all"][distinct] == 3).all()
    assert r["winner"] == int(np.flatnonzero(distinct)[0]) and r["winner_votes"] == 3 and r["mask"].all()
    assert np.allclose(r["model"], [1, 0, 8, 0, 1, -3], atol=1e-6)


def test_pairs_outside_their_list_never_vote():
    kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(300, 0.8, 9)
    bad = pairs.copy()
    bad[5, 0] = len(kp1); bad[17, 1] = -1; bad[40, 1] = len(kp2) + 1000
    r = cr.consensus(kp1, kp2, bad, 512, TOL, 2)
    assert np.isnan(r["pts"][[5, 17, 40]]).all() and not r["mask"][[5, 17, 40]].any()
    assert r["winner"] >= 0 and r["mask"].sum() == r["winner_votes"] > 200
