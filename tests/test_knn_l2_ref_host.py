"""CPU pins of what the GPU tests of MatchPlan.knn(metric="l2") lean on: the numpy restatement
tests/knn_l2_ref.py against an independent brute force in the dot-product form, the generator of descriptors at a prescribed
squared distance (tests/knn_l2_cases.py), a pair of elements the two metrics rank in opposite orders, ratio_filter on squared
distances around the threshold, and the interface (the `metric` keyword, the C entry point in the signature table and the header).
Every comparison is for equality."""
import inspect
import os
import re

import numpy as np
import pytest

import knn_l2_cases as lc
import knn_l2_ref
import knn_ref
import match_cases as mc
from sift_pyocl_amd.match import MatchPlan, ratio_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_restatement_against_a_dot_form_brute_force():
    """d = |a|^2 + |b|^2 - 2 a.b in float64 (exact: every term is below 2^24), a lexsort on (distance, index) per row"""
    rng = np.random.default_rng(51)
    a = mc.records(rng.integers(0, 256, (40, 128), dtype=np.uint8))
    b = mc.records(rng.integers(0, 256, (300, 128), dtype=np.uint8))
    b["desc"][17] = b["desc"][3]; b["desc"][250] = a["desc"][5]          # a tie and a zero
    A, B = a["desc"].astype(np.float64), b["desc"].astype(np.float64)
    D = ((A * A).sum(axis=1)[:, None] + (B * B).sum(axis=1)[None, :] - 2.0 * (A @ B.T)).astype(np.int64)
    assert D.min() == 0 and D.max() <= knn_l2_ref.DMAX
    for k in (1, 3, 8):
        idx, dist = knn_l2_ref.knn(a, b, k, budget=1 << 16)            # several chunks of queries
        assert idx.dtype == dist.dtype == np.int32 and idx.shape == dist.shape == (40, k)
        for i in range(40):
            order = np.lexsort((np.arange(300), D[i]))[:k]
            assert np.array_equal(idx[i], order) and np.array_equal(dist[i], D[i][order]), (k, i)
    idx, dist = knn_l2_ref.knn(a, b, 2)
    assert idx[5, 0] == 250 and dist[5, 0] == 0
    idx, dist = knn_l2_ref.knn(a, b[:3], 5)
    assert (idx[:, 3:] == -1).all() and (dist[:, 3:] == -1).all() and (idx[:, :3] >= 0).all()
    assert all((v == -1).all() and v.shape == (40, 2) for v in knn_l2_ref.knn(a, b[:0], 2))
    assert [v.shape for v in knn_l2_ref.knn(a[:0], b, 3)] == [(0, 3), (0, 3)]
    for k in (0, 9):
        with pytest.raises(ValueError):
            knn_l2_ref.knn(a, b, k)


PRESCRIBED = (0, 1, 2, 3, 7, 65024, 65025, 65026, 4194304, 123 * 65025 + 7, 8323200)


def test_generator_hits_the_prescribed_distances():
    rng = np.random.default_rng(52)
    base = mc.make_base(rng)
    descs = lc.descs_at(base, PRESCRIBED * 3, rng)
    assert descs.dtype == np.uint8 and descs.shape == (33, 128)
    a64 = descs.astype(np.int64) - base.astype(np.int64)
    assert ((a64 * a64).sum(axis=1) == np.array(PRESCRIBED * 3)).all()
    assert (descs[0] == base).all() and (descs[10] == 255 - base).all()
    assert len({descs[k].tobytes() for k in (4, 15, 26)}) == 3            # the positions are drawn anew for every row
    for r in (0, 1, 2, 3, 7, 65024, 28, 31, 240 * 240 + 7):
        roots = lc.four_squares(r)
        assert len(roots) <= 4 and all(0 < v <= 254 for v in roots) and sum(v * v for v in roots) == r
    # through the restatement: the queries are the base
    idx, dist = knn_l2_ref.knn(mc.queries(base, 2), mc.records(descs[:11]), 8)
    assert dist[0].tolist() == sorted(PRESCRIBED)[:8] and idx[1].tolist() == list(range(8))
    with pytest.raises(AssertionError):
        lc.descs_at(base, [126 * 65025 + 7], rng)                          # 126 + 4 bytes do not fit
    far = lc.far_dists(500, 7803004, rng)
    assert (far >= 7803004).all() and (far <= lc.DMAX).all()
    assert (lc.l2(base, lc.descs_at(base, far, rng)) == far).all()


def test_the_two_metrics_rank_the_reversing_pair_in_opposite_orders():
    rng = np.random.default_rng(53)
    query, near_l1, near_l2 = lc.reversing_pair(rng)
    a = mc.records(query[None, :]); b = mc.records(np.stack([near_l1, near_l2]))
    i1, d1 = knn_ref.knn(a, b, 2)
    i2, d2 = knn_l2_ref.knn(a, b, 2)
    assert i1.tolist() == [[0, 1]] and d1.tolist() == [[100, 120]]
    assert i2.tolist() == [[1, 0]] and d2.tolist() == [[120, 10000]]


def test_ratio_filter_on_squared_distances():
    """ratio_filter is not changed: on squared distances d1 <= d2 it keeps a row iff d2 != 0 and float32(d1) / float32(d2) <
    float32(ratio ** 2) -- Lowe's sqrt(d1) / sqrt(d2) < ratio.  d2 = 10 000 puts the edge of 0.8 at d1 = 6 400 and of 0.73 at 5 329."""
    for ratio, edge in ((0.8, 6400), (None, 5329)):
        r = 0.73 if ratio is None else ratio
        th = np.float32(r * r)
        d1 = np.array([0, 120, edge - 2, edge - 1, edge, edge + 1, edge + 2, 9999, 10000, 8323200 // 2, 5], np.int32)
        d2 = np.array([10000] * 9 + [8323200, 0], np.int32)
        d1[-1] = 0                                                         # d1 = d2 = 0: never a pair
        want = [i for i in range(len(d1)) if d2[i] != 0 and np.float32(d1[i]) / np.float32(d2[i]) < th]
        idx = np.stack([np.arange(len(d1)) + 100, np.arange(len(d1)) + 200], axis=1).astype(np.int32)
        got = ratio_filter(idx, np.stack([d1, d2], axis=1), ratio)
        assert got.tolist() == [[i, i + 100] for i in want]
        assert 3 in want and 5 not in want and 0 in want and 8 not in want and 10 not in want
        for i in (1, 3, 5, 7, 9):                                          # away from the edge it is Lowe's test as published
            assert (i in want) == (np.sqrt(float(d1[i])) / np.sqrt(float(d2[i])) < r)
    # the conversions are exact up to the largest squared distance
    assert int(np.float32(8323200)) == 8323200 and int(np.float32(8323199)) == 8323199


def test_interface():
    from sift_pyocl_amd import _lib
    sig = inspect.signature(MatchPlan.knn)
    assert list(sig.parameters) == ["self", "kp1", "kp2", "k", "metric"]
    assert sig.parameters["metric"].default == "l1" and sig.parameters["k"].default == 2
    assert "siftmi_match_knn_metric" in _lib.exported_symbols() and "siftmi_match_knn" in _lib.exported_symbols()
    res, args = _lib._SIGNATURES["siftmi_match_knn_metric"]
    assert len(args) == len(_lib._SIGNATURES["siftmi_match_knn"][1]) + 1
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    assert re.search(r"\bint\s+siftmi_match_knn_metric\s*\(", header)
    assert re.search(r"#define\s+SIFTMI_METRIC_L1\s+0\b", header) and re.search(r"#define\s+SIFTMI_METRIC_L2SQ\s+1\b", header)
    assert (_lib.METRIC_L1, _lib.METRIC_L2SQ) == (0, 1)
    assert "Lowe" in ratio_filter.__doc__
