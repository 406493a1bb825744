"""GPU tests of k-nearest-neighbour matching with distances: knn_partial_kernel<K> / knn_merge_kernel<K>
(k_knn.hpp) through MatchPlan.knn and siftmi_match_knn, against the numpy restatement tests/knn_ref.py (pinned to the oracle's
matcher by tests/test_knn_ref_host.py).  Every comparison is for equality of both arrays: the order (distance, index) is total.

The shapes are the smallest that reach each mechanism: the 64-descriptor tile, the 512 queries of a block, the first partition
split (above 256 list elements) and, in one test, the 16-bit index of a partition (a list of 70 000)."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_ref
import match_cases as mc
import window_ref as wr
from util import smooth_noise, sort_rows

pytestmark = pytest.mark.gpu

N1S = (1, 255, 513, 600)
N2S = (1, 2, 7, 8, 9, 63, 64, 65, 257, 600, 1500)
KS = (1, 2, 3, 5, 8)
# three of the twenty (n1, k) per list length, walking through both axes, and the largest of everything
SWEEP = sorted({(N1S[(j + t) % 4], n2, KS[(2 * j + t) % 5]) for j, n2 in enumerate(N2S) for t in range(3)} |
               {(600, 1500, 8), (513, 600, 8), (600, 257, 8), (1, 1, 8), (600, 1, 1)})
assert {s[0] for s in SWEEP} == set(N1S) and {s[1] for s in SWEEP} == set(N2S) and {s[2] for s in SWEEP} == set(KS)


@functools.lru_cache(maxsize=None)
def random_lists(n1, n2):
    """random descriptors, half of the shorter list shared within +-6, one exact duplicate (window_ref.lists)"""
    m2 = max(n2, 8)
    a, b, _ = wr.lists(n1, m2, min(n1, m2 - 2) // 2, seed=7 * n1 + n2)
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
    want = knn_ref.knn(a, b, k)
    same(mp.knn(a, b, k), want, what)
    return want


# ---------------------------------------------------------------------------------------------- shapes and k
@pytest.mark.parametrize("n1,n2,k", SWEEP)
def test_shapes_and_k(mp, n1, n2, k):
    a, b = random_lists(n1, n2)
    idx, dist = check(mp, a, b, k, "n1=%d n2=%d k=%d" % (n1, n2, k))
    assert ((idx >= 0).sum(axis=1) == min(k, n2)).all()


# ---------------------------------------------------------------------------------------------- ties
def tie_queries(base, rng):
    """600 copies of `base` (both register slots of a lane, two query blocks, a partial wave) and 50 random descriptors"""
    return np.concatenate([mc.queries(base, 600), mc.records(rng.integers(0, 256, (50, 128), dtype=np.uint8))])


def test_ties_four_distances(mp):
    """600 elements whose distances to the queries' descriptor are drawn from four values: every top-8 row is decided by the index
    rule, across every tile and partition boundary"""
    rng = np.random.default_rng(41)
    base = mc.make_base(rng)
    a = tie_queries(base, rng)
    b = mc.records(mc.descs_at(base, rng.choice([900, 901, 1400, 32640], 600), rng))
    for k in (8, 5, 2):
        idx, dist = check(mp, a, b, k, "four distances, k=%d" % k)
        assert (dist[:600] == 900).all() and (np.diff(idx[:600], axis=1) > 0).all()      # 150 or so at the smallest: all ties


def test_ties_constant_list(mp):
    rng = np.random.default_rng(42)
    base = mc.make_base(rng)
    a = tie_queries(base, rng)
    for value in (1000, 0, mc.DMAX):                                  # 32 640 = 0x7f80: just under the packed key's sentinel
        b = mc.records(mc.descs_at(base, [value] * 600, rng))
        idx, dist = check(mp, a, b, 8, "all at %d" % value)
        assert (idx[:600] == np.arange(8)).all() and (dist[:600] == value).all()


def test_zeros_planted(mp):
    """distance 0 at several indices, on both sides of tile and partition edges: the key of (0, j) is j itself"""
    rng = np.random.default_rng(43)
    base = mc.make_base(rng)
    a = tie_queries(base, rng)
    zeros = [599, 0, 63, 64, 255, 256, 257, 300]
    b = mc.planted(base, 600, dict([(j, 0) for j in zeros] + [(1, 3), (258, 3)]), rng)
    idx, dist = check(mp, a, b, 8, "eight zeros")
    assert (idx[:600] == sorted(zeros)).all() and (dist[:600] == 0).all()
    b = mc.planted(base, 600, dict([(j, 0) for j in zeros[:3]] + [(1, 3), (258, 3)]), rng)
    idx, dist = check(mp, a, b, 8, "three zeros")
    assert (idx[:600, :5] == [0, 63, 599, 1, 258]).all() and (dist[:600, :5] == [0, 0, 0, 3, 3]).all()


# ---------------------------------------------------------------------------------------------- the 16-bit index of a partition
def test_long_list(mp):
    """70 000 elements: more than one partition by the 16-bit limit, hundreds by the occupancy rule.  Equal distances at 0, 65 471,
    65 472 (the last index of a full partition and the one after it) and 69 999, a second tie around the same edge"""
    rng = np.random.default_rng(44)
    base = mc.make_base(rng)
    a = np.concatenate([mc.queries(base, 2), mc.records(rng.integers(0, 256, (2, 128), dtype=np.uint8))])
    b = mc.records(rng.integers(0, 256, (70000, 128), dtype=np.uint8))
    first, second = [0, 65471, 65472, 69999], [65470, 65473, 64, 63]
    b["desc"][first] = mc.descs_at(base, [500] * 4, rng)
    b["desc"][second] = mc.descs_at(base, [700] * 4, rng)
    idx, dist = check(mp, a, b, 8, "70 000 elements")
    assert (idx[:2] == first + sorted(second)).all() and (dist[:2] == [500] * 4 + [700] * 4).all()


# ---------------------------------------------------------------------------------------------- identity K1
def k1(mp, a, b, what):
    """ratio_filter over knn(k = 2) is match(): idx[:, 0], dist[:, 0], dist[:, 1] are best, dist1, dist2"""
    from sift_pyocl_amd.match import ratio_filter
    got = ratio_filter(*mp.knn(a, b, 2))
    want = sort_rows(mp.match(a, b, raw_results=True))
    assert got.dtype == np.int32 and np.array_equal(got, want), what
    return len(want)


def test_k1_on_crafted_lists(mp):
    n = 0
    for n1, n2 in ((600, 1500), (513, 600), (255, 65), (600, 1), (600, 2)):
        n += k1(mp, *random_lists(n1, n2), what="random %d x %d" % (n1, n2))
    for name in ("ratio default", "extremes", "ties 257"):
        for c in mc.family(name, 600):
            n += k1(mp, c.a, c.b, c.name)
    assert n >= 3000


def test_k1_on_real_keypoints(mp):
    import sift_pyocl_amd as sp
    big = smooth_noise((700, 760), seed=21, sigma=2.0)
    i1 = np.ascontiguousarray(big[10:650, 20:724]); i2 = np.ascontiguousarray(big[17:657, 9:713])
    plan = sp.SiftPlan(template=i1)
    kp1, kp2 = plan.keypoints(i1), plan.keypoints(i2)
    assert min(len(kp1), len(kp2)) > 1000
    assert k1(mp, kp1, kp2, "real pair") > 500
    want = check(mp, kp1[:1500], kp2[:2000], 5, "real pair, k=5")
    # the second list where SiftPlan left it on the device (kp2 is the plan's last result)
    same(mp.knn(kp1[:300], plan.device_records(), 3), knn_ref.knn(kp1[:300], kp2, 3), "device_records")
    assert (want[1][:, 0] <= want[1][:, 4]).all()


# ---------------------------------------------------------------------------------------------- device inputs
def test_device_tensors(mp):
    import torch
    a, b = random_lists(600, 1500)
    want = knn_ref.knn(a, b, 5)
    da = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda(); db = torch.from_numpy(b.view(np.uint8).reshape(-1).copy()).cuda()
    for l1, l2 in ((da, db), (a, db), (da, b), (a, b)):
        same(mp.knn(l1, l2, 5), want, "device tensors")


# ---------------------------------------------------------------------------------------------- edges and errors
def abi_knn(siftlib, mp, a, b, k, rows=None):
    """(rc, idx, dist) of siftmi_match_knn on buffers prefilled with -7"""
    rows = len(a) if rows is None else rows
    idx = np.full((max(1, rows), 8), -7, np.int32); dist = np.full((max(1, rows), 8), -7, np.int32)
    rc = siftlib.siftmi_match_knn(mp._handle, a.ctypes.data, len(a), 0, b.ctypes.data, len(b), 0, k, idx.ctypes.data, dist.ctypes.data)
    return rc, idx, dist


def test_empty_lists_and_padding(siftlib, mp):
    a, b = random_lists(255, 7)
    for k in (1, 8):
        idx, dist = mp.knn(a[:0], b, k)
        assert idx.shape == dist.shape == (0, k) and idx.dtype == dist.dtype == np.int32
        idx, dist = mp.knn(a, b[:0], k)
        assert idx.shape == dist.shape == (255, k) and (idx == -1).all() and (dist == -1).all()
    idx, dist = check(mp, a, b, 8, "n2 = 7 < k = 8")
    assert (idx[:, 7] == -1).all() and (dist[:, 7] == -1).all() and (idx[:, :7] >= 0).all()
    idx, dist = check(mp, a, b[:1], 3, "n2 = 1 < k = 3")
    assert (idx == [0, -1, -1]).all()
    # through the C ABI: n1 == 0 writes nothing; n2 == 0 writes exactly n1 * k cells
    rc, idx, dist = abi_knn(siftlib, mp, a[:0], b, 2)
    assert rc == 0 and (idx == -7).all() and (dist == -7).all()
    rc, idx, dist = abi_knn(siftlib, mp, a, b[:0], 3)
    assert rc == 0
    for v in (idx, dist):
        flat = v.reshape(-1)
        assert (flat[:255 * 3] == -1).all() and (flat[255 * 3:] == -7).all()
    rc, idx, dist = abi_knn(siftlib, mp, a, b, 3)
    assert rc == 0 and (idx.reshape(-1)[255 * 3:] == -7).all() and (dist.reshape(-1)[255 * 3:] == -7).all()
    want = knn_ref.knn(a, b, 3)
    assert np.array_equal(idx.reshape(-1)[:255 * 3].reshape(255, 3), want[0]) and np.array_equal(dist.reshape(-1)[:255 * 3].reshape(255, 3), want[1])


def test_bad_arguments(siftlib, mp):
    from sift_pyocl_amd import _lib
    a, b = random_lists(255, 65)
    for k in (0, 9, -1):
        with pytest.raises(RuntimeError):
            mp.knn(a, b, k)
        rc, idx, dist = abi_knn(siftlib, mp, a, b, k)
        assert rc == _lib.EINVAL and (idx == -7).all() and (dist == -7).all()
    with pytest.raises(RuntimeError):
        mp.knn(np.zeros(10, np.dtype([("x", np.float32), ("desc", (np.uint8, 128))])), b, 2)       # 132-byte records
    with pytest.raises(RuntimeError):
        mp.knn(a, b.view(np.uint8).reshape(-1, 72), 2)
    rc = siftlib.siftmi_match_knn(mp._handle, a.ctypes.data, -1, 0, b.ctypes.data, len(b), 0, 2, None, None)
    assert rc == _lib.EINVAL
    rc = siftlib.siftmi_match_knn(mp._handle, None, 5, 0, b.ctypes.data, len(b), 0, 2, None, None)
    assert rc == _lib.EINVAL
    same(mp.knn(a, b, 2), knn_ref.knn(a, b, 2), "after the errors")


def abi_match_ex(siftlib, mp, a, b, th, capacity):
    """(rc, pairs[:n_out], n_out, n_total) of siftmi_match_ex"""
    pairs = np.full((capacity, 2), -7, np.int32)
    n, total = C.c_int64(-5), C.c_int64(-5)
    rc = siftlib.siftmi_match_ex(mp._handle, a.ctypes.data, len(a), 0, b.ctypes.data, len(b), 0, C.c_float(float(th)), 0, 0,
                                 pairs.ctypes.data, capacity, C.byref(n), C.byref(total))
    return rc, pairs[:n.value].copy(), n.value, total.value


def test_knn_leaves_the_pair_capacity_alone(siftlib):
    """a knn call over lists far beyond a plan's size between two match calls: kpsize and the handle's size stay, the second match
    result equals the first"""
    import sift_pyocl_amd as sp
    rng = np.random.default_rng(45)
    base = mc.make_base(rng)
    a = mc.queries(base, 600)
    b = mc.planted(base, 2, {1: 100, 0: 5000}, rng)
    small = sp.MatchPlan(size=16)
    first = small.match(a[:10], b, raw_results=True)
    assert np.array_equal(sort_rows(first), np.stack([np.arange(10), np.ones(10, np.int64)], axis=1))
    rc, _, n, total = abi_match_ex(siftlib, small, a, b, mc.RATIO, capacity=600)
    assert rc == 0 and n == 16 and total == 600
    big_a, big_b = random_lists(600, 1500)
    same(small.knn(big_a, big_b, 8), knn_ref.knn(big_a, big_b, 8), "knn on a plan of 16")
    assert small.kpsize == 16
    rc, _, n, total = abi_match_ex(siftlib, small, a, b, mc.RATIO, capacity=600)
    assert rc == 0 and n == 16 and total == 600                         # the device still keeps 16 pairs of a call
    second = small.match(a[:10], b, raw_results=True)
    assert np.array_equal(sort_rows(second), sort_rows(first)) and small.kpsize == 16


# ---------------------------------------------------------------------------------------------- profile
def test_profile_events_and_kernel_time(siftlib):
    import torch
    import sift_pyocl_amd as sp
    a, b = random_lists(600, 1500)
    mp = sp.MatchPlan(profile=True)
    same(mp.knn(a, b, 3), knn_ref.knn(a, b, 3), "profile=True")
    assert mp.kernel_ms() > 0
    assert [l for l, _ in mp.events] == ["copy H->D KP_1", "copy H->D KP_2", "knn", "copy D->H knn"]
    for label, evt in mp.events:
        assert 0 <= evt.profile.end - evt.profile.start < 1e9, label
    mp.reset_timer()
    db = torch.from_numpy(b.view(np.uint8).reshape(-1).copy()).cuda()
    mp.knn(a, db, 3)
    assert [l for l, _ in mp.events] == ["copy H->D KP_1", "knn", "copy D->H knn"]
    mp.reset_timer()
    mp.match(a, b, raw_results=True)                                   # match keeps its own labels
    assert [l for l, _ in mp.events][:3] == list(sp.MatchPlan.STAGE_LABELS[:3])
    plain = sp.MatchPlan()
    plain.knn(a, b, 8)
    assert plain.kernel_ms() > 0 and plain.events == []
