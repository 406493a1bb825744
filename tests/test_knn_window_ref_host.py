"""CPU pins of what the GPU tests of MatchPlan.knn_window(window=) lean on: the numpy restatement
tests/knn_window_ref.py against the restatements that exist -- windowed matching (window_ref.match, identity W1), the two
brute-force knn restatements (W2) -- against itself with the lists exchanged (W3) and against the full sorted rows (W4), a direct
row-by-row evaluation of the ratio test on squared distances, and the interface.  Every comparison is for equality."""
import inspect
import os
import re

import numpy as np
import pytest

import knn_l2_ref
import knn_ref
import knn_window_ref as kw
import window_ref as wr
from sift_pyocl_amd.match import MatchPlan, ratio_filter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
SIZES = [(700, 650), (257, 64), (5, 900)]
SHIFTS = ((0.0, 0.0), (3.25, -1.5))
WINDOWS = (0, 2.5, (7, 3), INF)
FULL = {"l1": knn_ref, "l2": knn_l2_ref}


@pytest.mark.parametrize("n1,n2", SIZES)
def test_w1_ratio_filter_of_the_rows_is_windowed_match(n1, n2):
    seen = {"lone": 0, "none": 0}
    for shift in SHIFTS:
        a, b = wr.crafted(n1, n2, seed=n1 + n2, shift=shift)
        for window in WINDOWS:
            idx, dist = kw.knn(a, b, 2, window, shift)
            assert idx.dtype == dist.dtype == np.int32 and idx.shape == dist.shape == (n1, 2)
            got = ratio_filter(idx, dist)
            assert np.array_equal(wr.sort_rows(got), wr.sort_rows(wr.match(a, b, window, shift))), (window, shift)
            lone = (idx[:, 0] >= 0) & (idx[:, 1] < 0)
            assert set(np.nonzero(lone)[0]) <= set(got[:, 0])                 # a lone candidate always pairs
            assert not (set(np.nonzero(idx[:, 0] < 0)[0]) & set(got[:, 0]))   # no candidate never pairs
            seen["lone"] += int(lone.sum()); seen["none"] += int((idx[:, 0] < 0).sum())
    assert seen["lone"] > 0 and seen["none"] > 0


@pytest.mark.parametrize("n1,n2", SIZES)
def test_w2_infinite_window_is_the_whole_list(n1, n2):
    a, b = wr.crafted(n1, n2, seed=n1 + n2)
    for metric in ("l1", "l2"):
        for k in (1, 2, 8):
            want = FULL[metric].knn(a, b, k)
            got = kw.knn(a, b, k, INF, metric=metric)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (metric, k)


@pytest.mark.parametrize("n1,n2", SIZES)
def test_w3_exchanged_lists_with_the_shift_negated(n1, n2):
    """the candidates of list-2 keypoint j among list 1, ranked: the same set as the column j of the forward candidate matrix"""
    for shift in SHIFTS:
        a, b = wr.crafted(n1, n2, seed=n1 + n2, shift=shift)
        for window in WINDOWS[:3]:
            fwd = wr.candidate_matrix(a, b, window, shift)
            back = wr.candidate_matrix(b, a, window, (-shift[0], -shift[1]))
            assert np.array_equal(back, fwd.T), (window, shift)
            for metric in ("l1", "l2"):
                counts = np.zeros(n2, np.int64)
                idx, dist = kw.knn(b, a, 8, window, (-shift[0], -shift[1]), metric, counts=counts)
                assert np.array_equal(counts, fwd.sum(axis=0))
                for j in range(0, n2, 7):
                    cand = np.nonzero(fwd[:, j])[0]
                    d = kw.distances(a["desc"], b["desc"], cand, np.full(len(cand), j), metric)
                    order = np.lexsort((cand, d))[:8]
                    m = len(order)
                    assert np.array_equal(idx[j, :m], cand[order]) and np.array_equal(dist[j, :m], d[order]) and (idx[j, m:] == -1).all()


@pytest.mark.parametrize("n1,n2", SIZES)
def test_w4_rows_are_the_full_rows_restricted_to_candidates(n1, n2):
    kinds = np.zeros(4, np.int64)
    for shift in SHIFTS:
        a, b = wr.crafted(n1, n2, seed=n1 + n2, shift=shift)
        for metric in ("l1", "l2"):
            full_idx, full_dist = kw.knn(a, b, 8, INF, metric=metric, chunk=64)       # also: the chunk size plays no part
            for window in WINDOWS[:3]:
                counts = np.zeros(n1, np.int64)
                idx8, dist8 = kw.knn(a, b, 8, window, shift, metric, counts=counts)
                ok = wr.candidate_matrix(a, b, window, shift)
                assert np.array_equal(counts, ok.sum(axis=1))
                assert ((idx8 >= 0).sum(axis=1) == np.minimum(counts, 8)).all() and ((idx8 < 0) == (dist8 < 0)).all()
                has = idx8[:, 0] >= 0
                assert (dist8[has, 0] >= full_dist[has, 0]).all()
                for i in range(n1):
                    m = int(min(counts[i], 8))
                    keys = [(int(dist8[i, r]), int(idx8[i, r])) for r in range(m)]
                    assert keys == sorted(keys) and len(set(keys)) == m and all(ok[i, j] for _, j in keys)
                    # the candidates among the full row's eight, in its order, lead the windowed row
                    lead = [(int(full_dist[i, r]), int(full_idx[i, r])) for r in range(full_idx.shape[1]) if full_idx[i, r] >= 0 and ok[i, full_idx[i, r]]]
                    assert keys[:len(lead)] == lead[:m]
                for k in (1, 2, 3, 5):
                    idx, dist = kw.knn(a, b, k, window, shift, metric)
                    assert np.array_equal(idx, idx8[:, :k]) and np.array_equal(dist, dist8[:, :k])
                if (n1, n2) == (700, 650) and window == 2.5 and metric == "l1":
                    kinds += [(counts == 0).sum(), (counts == 1).sum(), ((counts >= 2) & (counts <= 7)).sum(), (counts > 8).sum()]
    if (n1, n2) == (700, 650):
        assert (kinds > 100).all(), kinds                                       # every row kind, both shifts together


def test_ratio_filter_on_windowed_l2_rows_against_a_direct_evaluation():
    shift = (3.25, -1.5)
    a, b = wr.crafted(700, 650, seed=1350, shift=shift)
    for window in (2.5, (7, 3)):
        idx, dist = kw.knn(a, b, 2, window, shift, "l2")
        for ratio in (0.8, None, 1.0):
            r = 0.73 if ratio is None else ratio
            want = kw.ratio_pairs(idx, dist, np.float32(r * r))
            got = ratio_filter(idx, dist, ratio)
            assert got.dtype == np.int32 and np.array_equal(got, want), (window, ratio)
            assert len(want) > 100


def test_edges_of_the_restatement():
    a, b = wr.crafted(257, 64, seed=5)
    assert [v.shape for v in kw.knn(a[:0], b, 3, 2.5)] == [(0, 3), (0, 3)]
    assert all(v.shape == (257, 2) and (v == -1).all() for v in kw.knn(a, b[:0], 2, 2.5))
    for k in (0, 9):
        with pytest.raises(ValueError):
            kw.knn(a, b, k, 2.5)
    with pytest.raises(ValueError):
        kw.knn(a, b, 2, 2.5, metric="cosine")
    a = a.copy(); a["x"][3] = np.nan                                       # a NaN makes the predicate false
    assert (kw.knn(a, b, 2, INF)[0][3] == -1).all()


def test_interface():
    from sift_pyocl_amd import _lib
    from sift_pyocl_amd.alignment import LinearAlign
    assert list(inspect.signature(MatchPlan.knn).parameters) == ["self", "kp1", "kp2", "k", "metric"]         # as rows 7 and 8 pin it
    sig = inspect.signature(MatchPlan.knn_window)
    assert list(sig.parameters) == ["self", "kp1", "kp2", "k", "metric", "window", "window_shift"]
    assert sig.parameters["k"].default == 2 and sig.parameters["metric"].default == "l1"
    assert sig.parameters["window"].default is None and tuple(sig.parameters["window_shift"].default) == (0.0, 0.0)
    sig = inspect.signature(LinearAlign.align)
    assert sig.parameters["match_metric"].default == "l1" and sig.parameters["match_ratio"].default is None
    assert "siftmi_match_knn_window" in _lib.exported_symbols()
    res, args = _lib._SIGNATURES["siftmi_match_knn_window"]
    assert len(args) == len(_lib._SIGNATURES["siftmi_match_knn_metric"][1]) + 4
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    assert re.search(r"\bint\s+siftmi_match_knn_window\s*\(", header)
    assert "W1" in MatchPlan.knn_window.__doc__ and "W3" in MatchPlan.knn_window.__doc__
