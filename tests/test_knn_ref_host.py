"""CPU pins of tests/knn_ref.py, the numpy restatement the GPU tests of MatchPlan.knn compare with,
and of sift_pyocl_amd.match.ratio_filter.  Identity K1: the first index and the first two distances of a k-nearest-neighbour row
are the best / dist1 / dist2 of the matcher's rule, so ratio_filter over them must return the pairs of the oracle's matcher and
of the matcher's numpy restatement (tests/window_ref.py with an infinite window) -- on lists with prescribed distances
(tests/match_cases.py: planted minima, ties for the minimum, zero second distances, every critical pair of the threshold) and on
random lists with shared and duplicate descriptors.  Every comparison is for equality."""
import numpy as np
import pytest

import knn_ref
import match_cases as mc
import window_ref as wr
from sift_pyocl_amd.match import ratio_filter

N1 = 3
INF = float("inf")


def rows(a):
    return wr.sort_rows(np.asarray(a, np.int32).reshape(-1, 2))


def check_k1(oracle, a, b, ratio=None, what=""):
    """ratio_filter over the restatement's two nearest against both matchers; returns the rows"""
    th = mc.RATIO if ratio is None else np.float32(ratio * ratio)
    got = ratio_filter(*knn_ref.knn(a, b, 2), ratio=ratio)
    assert got.dtype == np.int32 and got.ndim == 2 and got.shape[1] == 2
    assert np.array_equal(got, rows(got)), what                      # ascending i
    want, n = oracle.match(a, b, ratio_th=th, cap=max(1, len(a)))
    assert n == len(want)
    assert np.array_equal(got, rows(want)), what
    assert np.array_equal(got, rows(wr.match(a, b, INF, ratio_th=th))), what
    return got


@pytest.mark.parametrize("name", ["ratio default", "extremes", "placement 2", "placement 65", "placement 257", "ties 65", "ties 320"])
def test_ratio_filter_is_the_matcher_on_prescribed_distances(oracle, name):
    paired = cases = 0
    for c in mc.family(name, N1):
        got = check_k1(oracle, c.a, c.b, what=c.name)
        if np.float32(c.th).tobytes() != mc.RATIO.tobytes():          # the case's own threshold (above 1: the C ABI alone) is not
            check_k1(oracle, c.a, c.b, ratio=1.0, what=c.name)        # used: its LISTS are, under the default ratio and under 1
        elif c.best is not mc.UNKNOWN:
            assert np.array_equal(got, c.expected_rows()), c.name
        paired += len(got) > 0; cases += 1
    assert cases > 0
    if not name.startswith("ties"):                                    # a tie for the minimum has ratio 1: never a pair
        assert paired > 0


@pytest.mark.parametrize("ratio", [0.5, 0.73, 0.9, 1.0])
def test_ratio_filter_with_a_ratio_of_the_callers(oracle, ratio):
    """every critical (dist1, dist2) pair of float32(ratio ** 2), planted among far elements (for a threshold with a short significand
    they all sit on the failing side), beside a pair that passes under every ratio here and a tie, which never does"""
    th = np.float32(ratio * ratio)
    outcomes = set()
    for c in mc.ratio_cases(th, N1, seed=21, extra=[(100, 4000), (4000, 4000)] + (mc.ONE_EXTRA if ratio == 1.0 else [])):
        got = check_k1(oracle, c.a, c.b, ratio=ratio, what=c.name)
        assert np.array_equal(got, c.expected_rows()), c.name
        outcomes.add(len(got) > 0)
    assert outcomes == {True, False}


@pytest.mark.parametrize("n1,n2", [(700, 650), (257, 64), (5, 900), (40, 1), (40, 2)])
def test_ratio_filter_is_the_matcher_on_random_lists(oracle, n1, n2):
    a, b, _ = wr.lists(n1, max(n2, 8), min(n1, max(n2, 8) - 2) // 2, seed=n1 + n2)
    b = b[:n2]
    for ratio in (None, 0.9):
        got = check_k1(oracle, a, b, ratio=ratio)
        if n2 >= 64 or n2 == 1:                                        # a lone element always pairs
            assert len(got) > 0


def test_ties_and_zeros_in_the_restatement():
    """equal distances come out in ascending index; planted zeros first; the padding; the errors"""
    rng = np.random.default_rng(31)
    base = mc.make_base(rng)
    a = mc.queries(base, 2)
    tied = [129, 5, 64, 63, 70]
    b = mc.planted(base, 130, {j: 1000 for j in tied}, rng)
    idx, dist = knn_ref.knn(a, b, 8)
    assert idx.dtype == dist.dtype == np.int32 and idx.shape == dist.shape == (2, 8)
    assert idx[0, :5].tolist() == sorted(tied) and (dist[:, :5] == 1000).all() and (dist[:, 5:] > 1000).all()
    assert np.array_equal(dist[0], mc.l1(base, b["desc"][idx[0]]))
    assert (np.diff(dist, axis=1) >= 0).all()
    same = mc.records(mc.descs_at(base, [777] * 20, rng))
    idx, dist = knn_ref.knn(a, same, 8)
    assert (idx == np.arange(8)).all() and (dist == 777).all()
    zeros = mc.planted(base, 130, {128: 0, 0: 0, 64: 0}, rng)
    idx, dist = knn_ref.knn(a, zeros, 4)
    assert idx[1, :3].tolist() == [0, 64, 128] and (dist[:, :3] == 0).all() and (dist[:, 3] > 0).all()
    assert len(ratio_filter(idx, dist)) == 0                           # dist2 == 0: never a pair
    idx, dist = knn_ref.knn(a, b[:3], 5)
    assert (idx[:, 3:] == -1).all() and (dist[:, 3:] == -1).all() and sorted(idx[0, :3].tolist()) == [0, 1, 2]
    idx, dist = knn_ref.knn(a, b[:0], 2)
    assert (idx == -1).all() and (dist == -1).all() and len(ratio_filter(idx, dist, 1.0)) == 0
    assert [v.shape for v in knn_ref.knn(a[:0], b, 3)] == [(0, 3), (0, 3)]
    for k in (0, 9):
        with pytest.raises(ValueError):
            knn_ref.knn(a, b, k)


def test_ratio_filter_arguments():
    idx = np.array([[3, 1], [2, 0], [-1, -1], [5, -1]], np.int32)
    dist = np.array([[10, 100], [90, 100], [-1, -1], [7, -1]], np.int32)
    assert ratio_filter(idx, dist).tolist() == [[0, 3], [3, 5]]       # 0.1 passes, 0.9 fails, no neighbour fails, a lone one passes
    assert ratio_filter(idx, dist, 1.0).tolist() == [[0, 3], [1, 2], [3, 5]]
    assert ratio_filter(idx, dist, 0.0).shape == (0, 2)
    assert ratio_filter(idx[:0], dist[:0]).shape == (0, 2) and ratio_filter(idx[:0], dist[:0]).dtype == np.int32
    with pytest.raises(ValueError):
        ratio_filter(idx[:, :1], dist[:, :1])                         # k = 1: no second distance
    with pytest.raises(ValueError):
        ratio_filter(idx, dist, 1.01)                                 # above 1 the scan's (i, 0) for an empty query has no counterpart
    with pytest.raises(ValueError):
        ratio_filter(idx, dist[:3])
