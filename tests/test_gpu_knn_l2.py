"""GPU tests of k-nearest-neighbour matching under the squared Euclidean distance:
knn_l2_partial_kernel<K> / knn_l2_merge_kernel<K> (k_knn_l2.hpp) through MatchPlan.knn(metric="l2") and siftmi_match_knn_metric,
against the numpy restatement tests/knn_l2_ref.py (pinned by tests/test_knn_l2_ref_host.py).  Every comparison is for equality of
both arrays: the order (distance, index) is total.

The shapes are the smallest that reach each mechanism: the 64-descriptor tile, the window of 256 list elements whose index shares
the 32-bit key with the distance (and 512, a multiple of it), the 512 queries of a block, the first partition split (above 256
list elements), in one test a list of 70 000 (indices past 16 bits, hundreds of partitions) and in one 32 773 queries, the fewest
with which a partition holds more than one window."""
import functools

import numpy as np
import pytest

import knn_l2_cases as lc
import knn_l2_ref
import knn_ref
import match_cases as mc
import window_ref as wr
from util import smooth_noise

pytestmark = pytest.mark.gpu

N1S = (1, 255, 513, 600)
N2S = (1, 2, 7, 8, 9, 63, 64, 65, 257, 511, 512, 513, 600, 1500)
KS = (1, 2, 3, 5, 8)
# three of the twenty (n1, k) per list length, walking through both axes, and the largest of everything
SWEEP = sorted({(N1S[(j + t) % 4], n2, KS[(2 * j + t) % 5]) for j, n2 in enumerate(N2S) for t in range(3)} |
               {(600, 1500, 8), (513, 600, 8), (600, 257, 8), (600, 513, 8), (1, 1, 8), (600, 1, 1)})
assert {s[0] for s in SWEEP} == set(N1S) and {s[1] for s in SWEEP} == set(N2S) and {s[2] for s in SWEEP} == set(KS)


@functools.lru_cache(maxsize=None)
def random_lists(n1, n2):
    """random descriptors, half of the shorter list shared within +-6, one exact duplicate (window_ref.lists)"""
    m2 = max(n2, 8)
    a, b, _ = wr.lists(n1, m2, min(n1, m2 - 2) // 2, seed=11 * n1 + n2)
    return a, b[:n2].copy()


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


def same(got, want, what):
    for g, w, name in zip(got, want, ("idx", "dist")):
        assert g.dtype == np.int32 and g.shape == w.shape, "%s: %s is %s %s, expected %s" % (what, name, g.dtype, g.shape, w.shape)
        bad = np.nonzero((g != w).any(axis=1))[0] if g.size else []
        assert len(bad) == 0, "%s: %s differs in %d rows, first row %d: %s, expected %s" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]])


def check(mp, a, b, k, what):
    want = knn_l2_ref.knn(a, b, k)
    same(mp.knn(a, b, k, metric="l2"), want, what)
    return want


# ---------------------------------------------------------------------------------------------- shapes and k
@pytest.mark.parametrize("n1,n2,k", SWEEP)
def test_shapes_and_k(mp, n1, n2, k):
    a, b = random_lists(n1, n2)
    idx, dist = check(mp, a, b, k, "n1=%d n2=%d k=%d" % (n1, n2, k))
    assert ((idx >= 0).sum(axis=1) == min(k, n2)).all()


# ---------------------------------------------------------------------------------------------- both metrics on one plan
def test_both_metrics_on_one_plan(siftlib):
    """l1, l2, l1 on one MatchPlan, every call over longer lists than the one before (the key buffer the two paths share is
    regrown in each path's unit); a pair of elements the metrics rank in opposite orders is planted among random ones"""
    import sift_pyocl_amd as sp
    rng = np.random.default_rng(61)
    query, near_l1, near_l2 = lc.reversing_pair(rng)
    plan = sp.MatchPlan()
    for metric, n1, n2, k, p1, p2 in (("l1", 255, 300, 2, 299, 64), ("l2", 600, 700, 2, 255, 256), ("l1", 600, 1500, 8, 0, 1499)):
        a, b = (v.copy() for v in random_lists(n1, n2))
        a["desc"][[0, n1 - 1]] = query
        b["desc"][p1] = near_l1; b["desc"][p2] = near_l2
        ref = knn_ref if metric == "l1" else knn_l2_ref
        want = ref.knn(a, b, k)
        got = plan.knn(a, b, k, metric=metric)
        same(got, want, "%s %d x %d" % (metric, n1, n2))
        other = (knn_l2_ref if metric == "l1" else knn_ref).knn(a, b, k)
        assert not np.array_equal(got[1], other[1]) and not np.array_equal(got[0], other[0])
        nearest = [p1, p2] if metric == "l1" else [p2, p1]
        assert got[0][0, :2].tolist() == nearest and got[0][n1 - 1, :2].tolist() == nearest
        assert got[1][0, :2].tolist() == ([100, 120] if metric == "l1" else [120, 10000])
    same(plan.knn(*random_lists(255, 65), 3), knn_ref.knn(*random_lists(255, 65), 3), "the default metric afterwards")


# ---------------------------------------------------------------------------------------------- ties
def tie_queries(base, rng):
    """600 copies of `base` (both register slots of a lane, two query blocks, a partial wave) and 50 random descriptors"""
    return np.concatenate([mc.queries(base, 600), mc.records(rng.integers(0, 256, (50, 128), dtype=np.uint8))])


def test_ties_four_distances(mp):
    """600 elements whose distances to the queries' descriptor are drawn from four values: every top-8 row is decided by the index
    rule, across every tile, window and partition boundary"""
    rng = np.random.default_rng(62)
    base = mc.make_base(rng)
    a = tie_queries(base, rng)
    b = mc.records(lc.descs_at(base, rng.choice([900, 901, 65025, 8323200], 600), rng))
    for k in (8, 5, 2):
        idx, dist = check(mp, a, b, k, "four distances, k=%d" % k)
        assert (dist[:600] == 900).all() and (np.diff(idx[:600], axis=1) > 0).all()      # 150 or so at the smallest: all ties


def test_ties_constant_list(mp):
    rng = np.random.default_rng(63)
    base = mc.make_base(rng)
    a = tie_queries(base, rng)
    for value in (1000, 0, lc.DMAX):                                   # 8 323 200: the largest distance, next to the packed "none"
        b = mc.records(lc.descs_at(base, [value] * 600, rng))
        idx, dist = check(mp, a, b, 8, "all at %d" % value)
        assert (idx[:600] == np.arange(8)).all() and (dist[:600] == value).all()


def test_wide_distances(mp):
    """distances that differ in their lowest and in their highest bits: a key that drops either end ranks them wrongly"""
    rng = np.random.default_rng(64)
    base = mc.make_base(rng)
    a = tie_queries(base, rng)
    values = [70000, 70001, 4194304, 4194305, 120 * 65025, 120 * 65025 + 1, 120 * 65025 + 2, 120 * 65025 + 3, 8323200]
    where = [599, 3, 64, 255, 256, 300, 511, 512, 100]
    order = rng.permutation(9)
    plant = {where[t]: values[order[t]] for t in range(9)}
    b = lc.planted(base, 600, plant, rng, far_lo=120 * 65025 + 4)
    idx, dist = check(mp, a, b, 8, "wide distances")
    assert (dist[:600] == values[:8]).all()
    assert (idx[:600] == [where[int(np.nonzero(order == v)[0][0])] for v in range(8)]).all()


def test_zeros_planted(mp):
    """distance 0 at several indices, on both sides of tile, window and partition edges"""
    rng = np.random.default_rng(65)
    base = mc.make_base(rng)
    a = tie_queries(base, rng)
    for zeros in ([599, 0, 63, 64, 255, 256, 257, 300], [511, 512, 513, 0, 64, 599, 256, 1]):
        extra = [j for j in (2, 258) if j not in zeros]
        b = lc.planted(base, 600, dict([(j, 0) for j in zeros] + [(j, 3) for j in extra]), rng)
        idx, dist = check(mp, a, b, 8, "eight zeros at %s" % zeros)
        assert (idx[:600] == sorted(zeros)).all() and (dist[:600] == 0).all()
    b = lc.planted(base, 600, {599: 0, 0: 0, 63: 0, 1: 3, 258: 3}, rng)
    idx, dist = check(mp, a, b, 8, "three zeros")
    assert (idx[:600, :5] == [0, 63, 599, 1, 258]).all() and (dist[:600, :5] == [0, 0, 0, 3, 3]).all()


# ---------------------------------------------------------------------------------------------- a long list
def test_long_list(mp):
    """70 000 elements: hundreds of partitions, indices beyond 16 bits.  Equal distances at 0, 511 | 512 (a window multiple),
    65 471 | 65 472 (the L1 path's largest partition) and 69 999, a second value around the same edge"""
    rng = np.random.default_rng(66)
    base = mc.make_base(rng)
    a = np.concatenate([mc.queries(base, 2), mc.records(rng.integers(0, 256, (2, 128), dtype=np.uint8))])
    b = mc.records(rng.integers(0, 256, (70000, 128), dtype=np.uint8))
    first, second = [0, 511, 512, 65471, 65472, 69999], [65470, 65473]
    b["desc"][first] = lc.descs_at(base, [5000] * 6, rng)
    b["desc"][second] = lc.descs_at(base, [7000] * 2, rng)
    idx, dist = check(mp, a, b, 8, "70 000 elements")
    assert (idx[:2] == first + second).all() and (dist[:2] == [5000] * 6 + [7000] * 2).all()


def test_partitions_of_several_windows(mp):
    """A partition is longer than one window of 256 elements only when there are so many query blocks that about 2048 workgroups
    need fewer partitions than the list has windows: 32 773 queries (65 blocks, at most 32 partitions) against 16 500 elements make
    29 partitions of 576 = 256 + 256 + 64.  Only then does a window's fold read running keys back.  The queries are copies of
    four descriptors, so the restatement runs on four rows; the ties lie on both sides of the window edges inside a partition
    (255 | 256, 511 | 512), of the partition edge (575 | 576) and of the next partition's first window edge (831 | 832)."""
    rng = np.random.default_rng(68)
    base = mc.make_base(rng)
    four = np.concatenate([mc.queries(base, 1), mc.records(rng.integers(0, 256, (3, 128), dtype=np.uint8))])
    ids = rng.integers(0, 4, 32773); ids[[0, 511, 512, 32772]] = 0
    a = four[ids]
    ties = [255, 256, 511, 512, 575, 576, 831, 832, 16499]
    for k in (8, 3):
        b = lc.planted(base, 16500, dict([(j, 4000) for j in ties] + [(300, 4001), (1000, 3999 if k == 3 else 4001)]), rng)
        rand = np.setdiff1d(np.arange(2, 16500, 3), ties + [300, 1000])                  # a third of the far ones are random instead
        b["desc"][rand] = rng.integers(0, 256, (len(rand), 128), dtype=np.uint8)
        want = knn_l2_ref.knn(four, b, k)
        same(mp.knn(a, b, k, metric="l2"), (want[0][ids], want[1][ids]), "32 773 x 16 500, k=%d" % k)
        assert want[0][0].tolist() == (ties[:8] if k == 8 else [1000, 255, 256])


# ---------------------------------------------------------------------------------------------- real keypoints
@pytest.fixture(scope="module")
def real(siftlib):
    import sift_pyocl_amd as sp
    big = smooth_noise((700, 760), seed=21, sigma=2.0)
    i1 = np.ascontiguousarray(big[10:650, 20:724]); i2 = np.ascontiguousarray(big[17:657, 9:713])
    plan = sp.SiftPlan(template=i1)
    kp1, kp2 = plan.keypoints(i1), plan.keypoints(i2)
    assert min(len(kp1), len(kp2)) > 1000
    return plan, kp1, kp2, knn_l2_ref.knn(kp1[:1500], kp2[:2000], 5)


def test_real_keypoints(mp, real):
    plan, kp1, kp2, want = real
    same(mp.knn(kp1[:1500], kp2[:2000], 5, metric="l2"), want, "real pair, k=5")
    assert (want[1][:, 0] <= want[1][:, 4]).all() and want[1].max() <= lc.DMAX
    # the second list where SiftPlan left it on the device (kp2 is the plan's last result)
    same(mp.knn(kp1[:300], plan.device_records(), 3, metric="l2"), knn_l2_ref.knn(kp1[:300], kp2, 3), "device_records")


def test_real_keypoints_as_device_tensors(mp, real):
    import torch
    _, kp1, kp2, want = real
    a, b = kp1[:1500], kp2[:2000]
    da = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda(); db = torch.from_numpy(b.view(np.uint8).reshape(-1).copy()).cuda()
    for l1, l2 in ((da, db), (a, db), (da, b), (a, b)):
        same(mp.knn(l1, l2, 5, metric="l2"), want, "device tensors")


def test_lowes_ratio_test_on_real_keypoints(mp, real):
    """ratio_filter on squared distances with ratio 0.8 is Lowe's test; the crops are 11 px apart in x and -7 in y"""
    from sift_pyocl_amd.match import ratio_filter
    _, kp1, kp2, _ = real
    a = kp1[:800]
    want = ratio_filter(*knn_l2_ref.knn(a, kp2, 2), ratio=0.8)
    dx = np.median(kp2["x"][want[:, 1]] - a["x"][want[:, 0]]); dy = np.median(kp2["y"][want[:, 1]] - a["y"][want[:, 0]])
    assert len(want) > 500 and (round(float(dx)), round(float(dy))) == (11, -7), "the test's own pairs: %d, (%g, %g)" % (len(want), dx, dy)
    got = ratio_filter(*mp.knn(a, kp2, 2, metric="l2"), ratio=0.8)
    assert got.dtype == np.int32 and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------- edges and errors
def abi_knn(siftlib, mp, a, b, k, metric, rows=None):
    """(rc, idx, dist) of siftmi_match_knn_metric on buffers prefilled with -7"""
    rows = len(a) if rows is None else rows
    idx = np.full((max(1, rows), 8), -7, np.int32); dist = np.full((max(1, rows), 8), -7, np.int32)
    rc = siftlib.siftmi_match_knn_metric(mp._handle, a.ctypes.data, len(a), 0, b.ctypes.data, len(b), 0, k, metric, idx.ctypes.data,
                                         dist.ctypes.data)
    return rc, idx, dist


def test_empty_lists_and_padding(siftlib, mp):
    a, b = random_lists(255, 7)
    for k in (1, 8):
        idx, dist = mp.knn(a[:0], b, k, metric="l2")
        assert idx.shape == dist.shape == (0, k) and idx.dtype == dist.dtype == np.int32
        idx, dist = mp.knn(a, b[:0], k, metric="l2")
        assert idx.shape == dist.shape == (255, k) and (idx == -1).all() and (dist == -1).all()
    idx, dist = check(mp, a, b, 8, "n2 = 7 < k = 8")
    assert (idx[:, 7] == -1).all() and (dist[:, 7] == -1).all() and (idx[:, :7] >= 0).all()
    idx, dist = check(mp, a, b[:1], 3, "n2 = 1 < k = 3")
    assert (idx == [0, -1, -1]).all()
    # through the C ABI: n1 == 0 writes nothing; n2 == 0 writes exactly n1 * k cells
    rc, idx, dist = abi_knn(siftlib, mp, a[:0], b, 2, 1)
    assert rc == 0 and (idx == -7).all() and (dist == -7).all()
    rc, idx, dist = abi_knn(siftlib, mp, a, b[:0], 3, 1)
    assert rc == 0
    for v in (idx, dist):
        flat = v.reshape(-1)
        assert (flat[:255 * 3] == -1).all() and (flat[255 * 3:] == -7).all()
    rc, idx, dist = abi_knn(siftlib, mp, a, b, 3, 1)
    assert rc == 0 and (idx.reshape(-1)[255 * 3:] == -7).all() and (dist.reshape(-1)[255 * 3:] == -7).all()
    want = knn_l2_ref.knn(a, b, 3)
    assert np.array_equal(idx.reshape(-1)[:255 * 3].reshape(255, 3), want[0]) and np.array_equal(dist.reshape(-1)[:255 * 3].reshape(255, 3), want[1])
    # metric 0 through the new entry is siftmi_match_knn
    rc, idx, dist = abi_knn(siftlib, mp, a, b, 3, 0)
    want = knn_ref.knn(a, b, 3)
    assert rc == 0 and np.array_equal(idx.reshape(-1)[:255 * 3].reshape(255, 3), want[0]) and np.array_equal(dist.reshape(-1)[:255 * 3].reshape(255, 3), want[1])


def test_bad_arguments(siftlib, mp):
    from sift_pyocl_amd import _lib
    a, b = random_lists(255, 65)
    for k in (0, 9, -1):
        with pytest.raises(RuntimeError):
            mp.knn(a, b, k, metric="l2")
        rc, idx, dist = abi_knn(siftlib, mp, a, b, k, 1)
        assert rc == _lib.EINVAL and (idx == -7).all() and (dist == -7).all()
    for metric in (2, -1):
        rc, idx, dist = abi_knn(siftlib, mp, a, b, 2, metric)
        assert rc == _lib.EINVAL and (idx == -7).all() and (dist == -7).all()
    for metric in ("cosine", "L2", None, 1):
        with pytest.raises(ValueError):
            mp.knn(a, b, 2, metric=metric)
    rc = siftlib.siftmi_match_knn_metric(mp._handle, a.ctypes.data, -1, 0, b.ctypes.data, len(b), 0, 2, 1, None, None)
    assert rc == _lib.EINVAL
    rc = siftlib.siftmi_match_knn_metric(mp._handle, None, 5, 0, b.ctypes.data, len(b), 0, 2, 1, None, None)
    assert rc == _lib.EINVAL
    same(mp.knn(a, b, 2, metric="l2"), knn_l2_ref.knn(a, b, 2), "after the errors")
    same(mp.knn(a, b, 2), knn_ref.knn(a, b, 2), "the default metric after the errors")


def test_l2_leaves_the_pair_capacity_alone(siftlib):
    import sift_pyocl_amd as sp
    rng = np.random.default_rng(67)
    base = mc.make_base(rng)
    a = mc.queries(base, 10)
    b = mc.planted(base, 2, {1: 100, 0: 5000}, rng)
    small = sp.MatchPlan(size=16)
    first = small.match(a, b, raw_results=True)
    assert len(first) == 10 and small.kpsize == 16
    big_a, big_b = random_lists(600, 1500)
    same(small.knn(big_a, big_b, 8, metric="l2"), knn_l2_ref.knn(big_a, big_b, 8), "l2 on a plan of 16")
    assert small.kpsize == 16
    second = small.match(a, b, raw_results=True)
    assert np.array_equal(wr.sort_rows(second), wr.sort_rows(first)) and small.kpsize == 16


# ---------------------------------------------------------------------------------------------- profile
def test_profile_events_and_kernel_time(siftlib):
    import sift_pyocl_amd as sp
    a, b = random_lists(600, 1500)
    plan = sp.MatchPlan(profile=True)
    same(plan.knn(a, b, 3, metric="l2"), knn_l2_ref.knn(a, b, 3), "profile=True")
    assert plan.kernel_ms() > 0
    assert [l for l, _ in plan.events] == list(sp.MatchPlan.KNN_STAGE_LABELS)
    for label, evt in plan.events:
        assert 0 <= evt.profile.end - evt.profile.start < 1e9, label
    plain = sp.MatchPlan()
    plain.knn(a, b, 8, metric="l2")
    assert plain.kernel_ms() > 0 and plain.events == []
