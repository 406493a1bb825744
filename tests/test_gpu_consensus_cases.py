"""GPU tests of the consensus filter on the crafted families of tests/consensus_cases.py (what each reaches is proved on the CPU
by tests/test_consensus_cases_host.py): siftmi_match_consensus gives the restatement's votes, model bits, winner and mask on every
case, for equality; every case again as the middle segment of one siftmi_match_consensus_batch call, with separate and with shared
first lists, between two neighbours whose rows follow the case's own maps; and the single call whose workgroups walk 257 hypotheses.
No tolerance anywhere.  One exception, for non_finite only: a coefficient that is NaN in a VALID hypothesis is compared as "NaN on
both sides" (the sign of a generated NaN is not in the contract); void rows are 0x7fc00000 bit for bit everywhere."""
import numpy as np
import pytest

import consensus_batch_ref as cb
import consensus_cases as cc
import estimate_batch_ref as eb
from test_gpu_consensus import abi_consensus, assert_equal_to_restatement
from test_gpu_consensus_batch import Call, assert_equal

pytestmark = pytest.mark.gpu

QNAN = 0x7fc00000


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


def assert_equal_with_valid_nan(got, want, what):
    """assert_equal_to_restatement for sets whose valid hypotheses may hold NaN coefficients"""
    valid = want["valid"]
    assert np.array_equal(got["votes_all"], want["votes_all"]), what
    assert (bits(got["models_all"][~valid]) == QNAN).all(), what
    assert cb.same_bits(got["models_all"][valid], want["models_all"][valid]), what
    assert got["winner"] == want["winner"] and got["winner_votes"] == want["winner_votes"], what
    assert np.array_equal(got["mask"], want["mask"]), what
    assert want["winner"] >= 0 and cb.same_bits(got["model"], want["model"]), what


def case_of(family, k):
    return cc.family(family)[k]


@pytest.mark.parametrize("family,k", cc.case_names())
def test_family_equals_the_restatement(siftlib, mp, family, k):
    c = case_of(family, k)
    want = c.want()
    got = abi_consensus(siftlib, mp, *c.args)
    if family == "non_finite":
        assert_equal_with_valid_nan(got, want, c.name)
    else:
        assert_equal_to_restatement(got, want, c.name)
    assert (bits(got["models_all"][~want["valid"]]) == QNAN).all()
    # what the family is about, said once more on the device's own output
    if family == "det_edge":
        for name, hs in c.claims["classes"].items():
            void = np.isnan(got["models_all"][hs]).all(axis=1)
            assert (void == (name not in cc.DET_VALID)).all(), name
    if family == "vote_ring":
        for place, row, h, unfused, fused in c.claims["probes"]:
            assert got["votes_all"][h] == want["votes_all"][h], (cc.PLACES[place], row, h, unfused)
    if family in ("vote_equal", "tol_range"):
        at = c.claims["rows"]
        assert [n for n in cc.EQ_OFF if got["mask"][at[n]]] == [n for n in cc.EQ_OFF if want["mask"][at[n]]]
    if family == "select_order":
        assert got["winner"] == c.claims.get("winner", c.claims["first"])
    if c.name == "non_finite/no votes":
        assert got["winner"] == int(np.flatnonzero(want["valid"])[0]) > 0 and got["winner_votes"] == 0 and not got["mask"].any()


_BATCH = {}


def batch_of(c):
    """the case between two neighbours: the same matches in reverse order, so that a read across the segment's bounds finds rows
    that vote on the case's hypotheses.  (batch, restatement)"""
    if c.name not in _BATCH:
        batch = eb.from_segments(c.name, [c.reversed_segment(), (c.kp1, c.kp2, c.pairs), c.reversed_segment()])
        _BATCH[c.name] = batch, cb.consensus_batch(batch, c.n_hyp, float(c.tol), c.seed)
    return _BATCH[c.name]


@pytest.mark.parametrize("form", ["separate", "shared"])
@pytest.mark.parametrize("family,k", cc.case_names())
def test_family_as_a_segment_of_a_batch(siftlib, mp, family, k, form):
    c = case_of(family, k)
    batch, want = batch_of(c)
    single = c.want()
    # the middle segment's expectation is the single call's
    assert np.array_equal(want["votes_all"][1], single["votes_all"]) and np.array_equal(want["mask"][batch.rows(1)], single["mask"])
    assert want["winners"][1] == single["winner"] and cb.same_bits(want["models_all"][1], single["models_all"])
    got = Call(siftlib, mp, batch if form == "separate" else batch.shared(), c.n_hyp, float(c.tol), c.seed)
    assert_equal(got, want, batch, form)
    for s in range(batch.S):
        assert (bits(got.models_all[s][~want["valid"][s]]) == QNAN).all(), (c.name, s)
    if family != "non_finite":          # the case itself, bit for bit (a neighbour's other sample may draw the case's inf rows)
        assert np.array_equal(bits(got.models_all[1]), bits(want["models_all"][1])), c.name
    if want["winners"][1] >= 0 and family != "non_finite":
        assert np.array_equal(bits(got.models[1]), bits(single["model"]))


def test_single_call_whose_workgroups_walk_257_hypotheses(siftlib, mp):
    """66 tiles and 8224 hypotheses: 32 chunks of 257, so every workgroup folds column 256 of its counters in a second trip; about
    half the rows are NaN and the votes are counted on the CPU over the other half"""
    W = cc.WIDE_SINGLE
    kp1, kp2, pairs = cc.wide_single()
    want = cc.consensus_on_finite(kp1, kp2, pairs, W["n_hyp"], W["tol"], W["seed"])
    assert want["winner"] >= 0 and 500 < want["valid"].sum() < 2000
    got = abi_consensus(siftlib, mp, kp1, kp2, pairs, W["n_hyp"], W["tol"], W["seed"])
    assert_equal_to_restatement(got, want, "h_chunk 257")
    assert got["winner_votes"] > 0.5 * 0.6 * 0.5 * W["M"]
