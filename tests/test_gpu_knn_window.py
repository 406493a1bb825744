"""GPU tests of k-nearest-neighbour matching inside a search window: mw_knn_kernel<K, L2>
(k_knn_window.hpp) through MatchPlan.knn_window(window=, window_shift=), siftmi_match_knn_window and
LinearAlign.align(match_metric=, match_ratio=), against the numpy restatement tests/knn_window_ref.py (pinned by
tests/test_knn_window_ref_host.py).  Every comparison is for equality of both int32 arrays: the order (distance, index) is total.

The restatement is evaluated once per (lists, window, shift, metric) at k = 8; the row for a smaller k is its first k columns
(pinned on the CPU), and every k in 1 .. 8 is run on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import knn_l2_cases as lc
import knn_window_ref as kw
import match_cases as mc
import window_ref as wr
from util import dtype_kp, smooth_noise, sort_kp, sort_rows

pytestmark = pytest.mark.gpu
INF = float("inf")
METRICS = ("l1", "l2")
KS = tuple(range(1, 9))
SHIFTS = ((0.0, 0.0), (3.25, -1.5))


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


@functools.lru_cache(maxsize=None)
def crafted(n1, n2, shift):
    return wr.crafted(n1, n2, seed=n1 + n2, shift=shift)


def same(got, want, what):
    for g, w, name in zip(got, want, ("idx", "dist")):
        assert g.dtype == np.int32 and g.shape == w.shape, "%s: %s is %s %s, expected %s" % (what, name, g.dtype, g.shape, w.shape)
        bad = np.nonzero((g != w).any(axis=1))[0] if g.size else []
        assert len(bad) == 0, "%s: %s differs in %d rows, first row %d: %s, expected %s" % (what, name, len(bad), bad[0], g[bad[0]], w[bad[0]])


def check(mp, a, b, window, shift=(0.0, 0.0), what="", metrics=METRICS, ks=KS, counts=None):
    """every k on both metrics against the restatement; returns the restatement's k = 8 rows per metric"""
    out = {}
    for metric in metrics:
        want = kw.knn(a, b, 8, window, shift, metric, counts=counts)
        for k in ks:
            got = mp.knn_window(a, b, k, metric=metric, window=window, window_shift=shift)
            same(got, (want[0][:, :k], want[1][:, :k]), "%s window %s shift %s %s k=%d" % (what, window, shift, metric, k))
        out[metric] = want
    return out


# ---------------------------------------------------------------------------------------------- crafted lists
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("n1,n2", [(700, 650), (257, 64), (5, 900), (3000, 5000)])
def test_crafted_lists_vs_restatement(mp, n1, n2, shift):
    a, b = crafted(n1, n2, shift)
    found = 0
    for window in (0, 2.5, (7, 3)) + ((INF,) if n1 < 3000 else ()):
        counts = np.zeros(n1, np.int64)
        want = check(mp, a, b, window, shift, "crafted %dx%d" % (n1, n2), counts=counts)
        found += int((want["l1"][0] >= 0).sum())
        if (n1, n2) == (700, 650) and window == 2.5:
            # every kind of row: no candidate, a lone one, fewer than k, more than k; the crowded cell; equal distances among the first eight
            kinds = [(counts == 0).sum(), (counts == 1).sum(), ((counts >= 2) & (counts <= 7)).sum(), (counts > 8).sum()]
            assert min(kinds) > 100, kinds
            assert 216 <= counts.max() <= 220 and (counts >= 216).sum() >= 200
            for metric in METRICS:
                d = want[metric][1]
                # L1 distances of random descriptors collide now and then; squared ones hardly: there the duplicated descriptor is the tie
                assert ((d[:, 1:] == d[:, :-1]) & (d[:, 1:] >= 0)).any(axis=1).sum() >= (10 if metric == "l1" else 1)
    assert found > 0


# ---------------------------------------------------------------------------------------------- prescribed distances
def test_prescribed_l1_distances_ties_in_different_cells(mp):
    """tie cases of match_cases (equal L1 distances at prescribed indices) with the tied elements alternately in two cells, the
    earliest index in the later cell: the smaller index comes first whatever order the cells are streamed in"""
    n = 0
    for n2 in (65, 320):
        for t, c in enumerate(mc.family("ties %d" % n2, 70)):
            if t % 6 and "every tile" not in c.name and "constant" not in c.name:
                continue
            a, b = mc.tied_in_different_cells(c)
            want = check(mp, a, b, mc.SPOT_WINDOW, what=c.name, metrics=("l1",), ks=(1, 2, 3, 8))["l1"]
            tied = sorted(c.planted)
            if "constant" in c.name:
                assert (want[0] == np.arange(8)).all() and len(set(want[1].reshape(-1))) == 1
            else:
                m = min(len(tied), 8)
                assert (want[0][:, :m] == tied[:m]).all() and (want[1][:, :m] == want[1][0, 0]).all(), c.name
            n += 1
    assert n > 20


def test_prescribed_distances_on_four_spots(mp):
    """planted distances (both metrics, the largest included) over lists whose keypoints sit on four spots 200 px apart: three
    queries of four see the planted elements, the others only far ones (their nearest neighbour by descriptor is OUTSIDE their
    window) or nothing"""
    rng = np.random.default_rng(81)
    base = mc.make_base(rng)
    q = mc.queries(base, 260)
    plant_l1 = {70: 1000, 3: 1000, 64: 1000, 63: 999, 129: 0, 5: mc.DMAX - 1, 200: 4000}
    plant_l2 = {70: 65025, 3: 65025, 64: 65025, 63: 65024, 129: 0, 5: 4194304, 200: 70001}
    lists = {"l1": mc.planted(base, 330, plant_l1, rng, far_lo=mc.DMAX), "l2": lc.planted(base, 330, plant_l2, rng, far_lo=lc.DMAX)}
    for metric, plant in (("l1", plant_l1), ("l2", plant_l2)):
        a, b = mc.spread_over_spots(mc.Case("planted " + metric, q, lists[metric], mc.RATIO, planted=tuple(plant)))
        want = check(mp, a, b, mc.SPOT_WINDOW, what="four spots", metrics=(metric,))[metric]
        order = sorted(plant.items(), key=lambda kv: (kv[1], kv[0]))
        on0 = np.nonzero(a["x"] == mc.SPOTS[0, 0])[0]; on1 = np.nonzero(a["x"] == mc.SPOTS[1, 0])[0]; on3 = np.nonzero(a["x"] == mc.SPOTS[3, 0])[0]
        assert len(on0) > 100 and len(on1) > 20 and len(on3) > 20
        assert (want[0][on0, :7] == [j for j, _ in order]).all() and (want[1][on0, :7] == [d for _, d in order]).all()
        far = mc.DMAX if metric == "l1" else lc.DMAX
        assert (want[1][on0, 7] == far).all()                                   # the largest distance there is, as the eighth
        # on spot 1 the nearest by descriptor (element 129 at distance 0) is not a candidate: the far elements there rank by index
        assert (want[1][on1] == far).all() and (np.diff(want[0][on1], axis=1) > 0).all() and not np.isin(want[0][on1], list(plant)).any()
        assert (want[0][on3] == -1).all() and (want[1][on3] == -1).all()


# ---------------------------------------------------------------------------------------------- the edge of the window
def boundary_lists():
    """The constructions of tests/test_gpu_match_window.py: row k of list 2 carries the descriptor of row k of list 1 (+-6 per
    byte) and sits on, or a few float32 steps beside, the edge of that keypoint's window.  The first 24 queries are 200 px apart,
    each with that ONE keypoint near it.  Returns the lists, (sx, sy), (wx, wy) and, for the positions that are exact in float32,
    the rows that must / must not be candidates of their own query."""
    sx, sy, wx, wy = 3.25, -1.5, 2.5, 4.0
    f = np.float32
    rows = []            # (x1, y1, x2, y2, expected: True / False / None = whatever the float32 predicate says)
    for base in (100.5, -500.25, 1000.0):
        for case in range(8):
            y = f(base / 2 + 200.0 * len(rows))                  # 200 px apart in y: every query keeps its candidate to itself
            x2, y2 = f(base + sx), f(y + sy)
            if case < 4:                                         # on the right / left edge, and one float32 step beyond
                x2 = f(base + sx + (wx if case < 2 else -wx))
                if case % 2:
                    x2 = np.nextafter(x2, f(INF if case < 2 else -INF))
            else:                                                # bottom / top edge
                y2 = f(y + sy + (wy if case < 6 else -wy))
                if case % 2:
                    y2 = np.nextafter(y2, f(INF if case < 6 else -INF))
            rows.append((f(base), y, x2, y2, case % 2 == 0))
    # around 16 000 with fractional parts the float32 spacing is 2^-10: the predicate's two roundings decide, not the real numbers
    rng = np.random.default_rng(77)
    for k in range(60):
        x1 = f(16000.0 + 3.0 * k + rng.random()); y1 = f(15900.0 + rng.random())
        for side in (1.0, -1.0):
            edge = f(f(x1 + f(sx)) + f(side * wx))
            for step in (0, 1, 2, -1, -2):
                x2 = edge
                for _ in range(abs(step)):
                    x2 = np.nextafter(x2, f(INF if step > 0 else -INF))
                rows.append((x1, y1, x2, f(y1 + f(sy)), None))
            edge = f(f(y1 + f(sy)) + f(side * wy))
            for step in (0, 1, -1):
                y2 = edge if step == 0 else np.nextafter(edge, f(INF if step > 0 else -INF))
                rows.append((x1, y1, f(x1 + f(sx)), y2, None))
    n = len(rows)
    rng = np.random.default_rng(78)
    extra = 6
    a = np.zeros(n + extra, dtype_kp); b = np.zeros(n + extra, dtype_kp)
    a["desc"] = rng.integers(0, 256, (n + extra, 128), dtype=np.uint8)
    b["desc"] = np.clip(a["desc"].astype(int) + rng.integers(-6, 7, (n + extra, 128)), 0, 255).astype(np.uint8)
    for k, (x1, y1, x2, y2, _) in enumerate(rows):
        a["x"][k] = x1; a["y"][k] = y1; b["x"][k] = x2; b["y"][k] = y2
    # keypoints that must neither be candidates nor disturb the grid's arithmetic
    a["x"][n:] = [np.nan, 1e30, -1e30, 7.0, np.inf, 1e30]; a["y"][n:] = [5.0, 1e30, 3.0, np.nan, 2.0, -1e30]
    b["x"][n:] = [1e30, np.nan, -1e30, np.inf, 7.0, 1e30]; b["y"][n:] = [1e30, 5.0, 3.0, 2.0, np.nan, -1e30]
    must = [k for k, r in enumerate(rows) if r[4] is True]
    never = [k for k, r in enumerate(rows) if r[4] is False]
    return a, b, (sx, sy), (wx, wy), must, never


def test_window_boundaries(mp):
    a, b, shift, window, must, never = boundary_lists()
    want = check(mp, a, b, window, shift, "boundaries")["l1"]
    got = mp.knn_window(a, b, 8, window=window, window_shift=shift)[0]
    ok = wr.candidate_matrix(a, b, window, shift)
    for k in must:                                # exact in float32: on the edge is a candidate, one step beyond is not
        assert ok[k, k] and got[k].tolist() == [k] + [-1] * 7, k
    for k in never:
        assert not ok[k, k] and (got[k] == -1).all(), k
    n = len(a) - 6
    assert (want[0][n:] == -1).all()              # NaN, the infinities and 1e30: no candidate, none of anything
    check(mp, a[:n], b[:n], window, shift, "boundaries, finite")      # without the huge coordinates: a fine grid over the same cases
    big = np.abs(a["x"][:n]) > 8000               # the 16 000 block alone
    w16 = check(mp, a[:n][big], b[:n][big], window, shift, "boundaries, 16 000 block")["l1"]
    assert (w16[0][:, 0] >= 0).sum() > 100
    # a window of one float32 step centred on the right edge: the rows one step to either side are in, two steps are out
    tiny = check(mp, a[:n][big], b[:n][big], 2.0 ** -10, (shift[0] + window[0], shift[1]), "boundaries, tiny window")["l1"]
    assert (tiny[0][:, 0] >= 0).sum() > 50
    # an infinite window on one axis only, and on both with the huge coordinates in the lists
    check(mp, a, b, (INF, 4.0), shift, "boundaries, wx = inf", ks=(2, 8))
    check(mp, a, b, INF, shift, "boundaries, w = inf", ks=(2, 8))


# ---------------------------------------------------------------------------------------------- degenerate grids
def test_one_cell_one_point_and_window_zero(mp):
    a, b, _ = wr.lists(900, 1100, 400, seed=9, H=1, W=1)
    for window, shift in ((5.0, (0.0, 0.0)), (0.25, (0.1, -0.1)), ((0.05, 5.0), (0.0, 0.0))):       # wider than the extent: one cell
        check(mp, a, b, window, shift, "one cell", ks=(1, 3, 8))
    a["x"] = 3.5; a["y"] = -2.25; b["x"] = 3.5; b["y"] = -2.25
    want = check(mp, a, b, 0, (0.0, 0.0), "one point, window 0", ks=(2, 8))                       # 1100 candidates for everyone
    assert (want["l1"][0] >= 0).all()
    want = check(mp, a, b, 0, (1.0, 0.0), "one point, shifted away", ks=(2, 8))
    assert (want["l2"][0] == -1).all()
    a2, b2 = crafted(700, 650, SHIFTS[0])
    want = check(mp, a2, b2, 0, what="window 0 on crafted lists", ks=(1, 8))
    assert 0 < (want["l1"][0][:, 0] >= 0).sum() < 700


# ---------------------------------------------------------------------------------------------- the identities on the device
@pytest.mark.parametrize("shift", SHIFTS)
def test_w1_ratio_filter_of_knn_is_windowed_match(mp, shift):
    from sift_pyocl_amd.match import ratio_filter
    total = 0
    for n1, n2 in ((700, 650), (257, 64), (3000, 5000)):
        a, b = crafted(n1, n2, shift)
        for window in (0, 2.5, (7, 3), INF):
            got = ratio_filter(*mp.knn_window(a, b, 2, window=window, window_shift=shift))
            want = mp.match(a, b, raw_results=True, window=window, window_shift=shift)
            assert np.array_equal(sort_rows(got), sort_rows(want)), (n1, n2, window)
            total += len(got)
    assert total > 1000


def test_w2_infinite_window_is_brute_force_knn(mp):
    a, b = crafted(3000, 5000, SHIFTS[0])
    for metric in METRICS:
        for k in KS:
            same(mp.knn_window(a, b, k, metric=metric, window=INF), mp.knn(a, b, k, metric=metric), "3000x5000 %s k=%d" % (metric, k))


def test_w3_exchanged_lists_with_the_shift_negated(mp):
    shift = SHIFTS[1]
    back_shift = (-shift[0], -shift[1])
    for n1, n2 in ((700, 650), (257, 64)):
        a, b = crafted(n1, n2, shift)
        for window in (2.5, (7, 3)):
            cb = np.zeros(n2, np.int64)
            back = {}
            for metric in METRICS:
                want = kw.knn(b, a, 8, window, back_shift, metric, counts=cb)
                for k in KS:
                    same(mp.knn_window(b, a, k, metric=metric, window=window, window_shift=back_shift), (want[0][:, :k], want[1][:, :k]),
                         "exchanged %dx%d %s %s k=%d" % (n1, n2, window, metric, k))
                back[metric] = mp.knn_window(b, a, 8, metric=metric, window=window, window_shift=back_shift)
            # candidacy is symmetric: between rows that are not truncated, (i, j) is in the forward result iff it is in the other
            fwd = mp.knn_window(a, b, 8, window=window, window_shift=shift)[0]
            ca = (wr.candidate_matrix(a, b, window, shift)).sum(axis=1)
            F = {(i, int(j)) for i in np.nonzero(ca <= 8)[0] for j in fwd[i] if j >= 0 and cb[j] <= 8}
            B = {(int(i), j) for j in np.nonzero(cb <= 8)[0] for i in back["l1"][0][j] if i >= 0 and ca[i] <= 8}
            assert F == B and len(F) > (500 if n1 == 700 else 40)       # 614 / 1399 and 43 / 87 pairs, counted on the CPU


# ---------------------------------------------------------------------------------------------- real keypoints, inputs
@pytest.fixture(scope="module")
def real(siftlib):
    import sift_pyocl_amd as sp
    big = smooth_noise((700, 760), seed=21, sigma=2.0)
    i1 = np.ascontiguousarray(big[10:650, 20:724]); i2 = np.ascontiguousarray(big[17:657, 9:713])      # real_pair() of test_gpu_match_window.py
    plan = sp.SiftPlan(template=i1)
    kp1, kp2 = plan.keypoints(i1), plan.keypoints(i2)
    assert min(len(kp1), len(kp2)) > 1000
    return plan, kp1, kp2


def test_real_keypoints(mp, real):
    from sift_pyocl_amd.match import ratio_filter
    plan, k1, k2 = real
    want = check(mp, k1, k2, 16, what="real keypoints")
    centred = check(mp, k1, k2, 6, (11.0, -7.0), "real keypoints, centred window")
    # Lowe's test inside the centred window finds the displacement of the crops
    pairs = ratio_filter(*centred["l2"], ratio=0.8)
    dx = np.median(k2["x"][pairs[:, 1]] - k1["x"][pairs[:, 0]]); dy = np.median(k2["y"][pairs[:, 1]] - k1["y"][pairs[:, 0]])
    assert len(pairs) > 500 and abs(dx - 11.0) < 0.1 and abs(dy + 7.0) < 0.1, (len(pairs), dx, dy)
    # the second list where SiftPlan left it on the device (k2 is the plan's last result)
    for metric in METRICS:
        same(mp.knn_window(k1, plan.device_records(), 5, metric=metric, window=16), (want[metric][0][:, :5], want[metric][1][:, :5]), "device_records")


def test_device_and_mixed_lists(mp):
    import torch
    shift, window = SHIFTS[1], (7, 3)
    a, b = crafted(700, 650, shift)
    da = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda(); db = torch.from_numpy(b.view(np.uint8).reshape(-1).copy()).cuda()
    for metric in METRICS:
        want = kw.knn(a, b, 8, window, shift, metric)
        for l1, l2 in ((da, db), (a, db), (da, b), (a, b)):
            same(mp.knn_window(l1, l2, 8, metric=metric, window=window, window_shift=shift), want, "device tensors " + metric)


def test_pair_capacity_par_and_roi_play_no_part(siftlib):
    import sift_pyocl_amd as sp
    a, b = crafted(700, 650, SHIFTS[0])
    small = sp.MatchPlan(size=16)
    small.set_roi(np.zeros((90, 120), np.int8))
    want = kw.knn(a, b, 8, 2.5)
    same(small.knn_window(a, b, 8, window=2.5), want, "a plan of 16 with an empty region of interest")
    assert small.kpsize == 16
    old = sp.par.MatchRatio
    try:
        sp.par.MatchRatio = 0.1
        same(small.knn_window(a, b, 8, window=2.5), want, "another MatchRatio")
    finally:
        sp.par.MatchRatio = old


# ---------------------------------------------------------------------------------------------- profile
def test_profile_events_and_kernel_time(siftlib):
    import sift_pyocl_amd as sp
    a, b = crafted(700, 650, SHIFTS[0])
    plan = sp.MatchPlan(profile=True)
    same(plan.knn_window(a, b, 3, metric="l2", window=2.5), tuple(v[:, :3] for v in kw.knn(a, b, 8, 2.5, metric="l2")), "profile=True")
    assert plan.kernel_ms() > 0
    assert [l for l, _ in plan.events] == list(sp.MatchPlan.KNN_STAGE_LABELS)
    for label, evt in plan.events:
        assert 0 <= evt.profile.end - evt.profile.start < 1e9, label
    plain = sp.MatchPlan()
    plain.knn_window(a, b, 8, window=2.5)
    assert plain.kernel_ms() > 0 and plain.events == []


# ---------------------------------------------------------------------------------------------- errors and empty lists
def abi(siftlib, mp, a, b, k, metric, window=(4.0, 4.0), shift=(0.0, 0.0), n1=None, p1=True, p2=True, out=True):
    """(rc, idx, dist) of siftmi_match_knn_window on buffers prefilled with -7"""
    n1 = len(a) if n1 is None else n1
    idx = np.full((max(1, len(a)), 8), -7, np.int32); dist = np.full((max(1, len(a)), 8), -7, np.int32)
    rc = siftlib.siftmi_match_knn_window(mp._handle, a.ctypes.data if p1 else None, n1, 0, b.ctypes.data if p2 else None, len(b), 0, k, metric,
                                         C.c_float(window[0]), C.c_float(window[1]), C.c_float(shift[0]), C.c_float(shift[1]),
                                         idx.ctypes.data if out else None, dist.ctypes.data)
    return rc, idx, dist


def test_errors_and_empty_lists(siftlib, mp):
    from sift_pyocl_amd import _lib
    a, b = crafted(257, 64, SHIFTS[0])
    for bad in (-1.0, float("nan"), (3.0, -0.5), (float("nan"), 3.0)):
        with pytest.raises(RuntimeError):
            mp.knn_window(a, b, 2, window=bad)
    for bad in ((INF, 0.0), (0.0, float("nan"))):
        with pytest.raises(RuntimeError):
            mp.knn_window(a, b, 2, window=4, window_shift=bad)
    for k in (0, 9):
        with pytest.raises(RuntimeError):
            mp.knn_window(a, b, k, window=4)
    for metric in ("cosine", "L2", None, 1):
        with pytest.raises(ValueError):
            mp.knn_window(a, b, 2, metric=metric, window=4)
    with pytest.raises(ValueError):
        mp.knn_window(a, b, 2, window_shift=(1.0, 0.0))                      # a shift without a window
    same(mp.knn_window(a, b, 2, window_shift=(0.0, 0.0)), mp.knn(a, b, 2), "without a window it is knn")
    for k in (1, 8):
        for metric in METRICS:
            idx, dist = mp.knn_window(a[:0], b, k, metric=metric, window=4)
            assert idx.shape == dist.shape == (0, k) and idx.dtype == dist.dtype == np.int32
            idx, dist = mp.knn_window(a, b[:0], k, metric=metric, window=4)
            assert idx.shape == dist.shape == (257, k) and (idx == -1).all() and (dist == -1).all()
    # the C ABI: every refusal leaves the result buffers alone
    refused = [abi(siftlib, mp, a, b, 0, 0), abi(siftlib, mp, a, b, 9, 1), abi(siftlib, mp, a, b, 2, 2), abi(siftlib, mp, a, b, 2, -1),
               abi(siftlib, mp, a, b, 2, 0, window=(-1.0, 4.0)), abi(siftlib, mp, a, b, 2, 0, window=(4.0, float("nan"))),
               abi(siftlib, mp, a, b, 2, 0, shift=(INF, 0.0)), abi(siftlib, mp, a, b, 2, 0, shift=(0.0, float("nan"))),
               abi(siftlib, mp, a, b, 2, 0, n1=-1), abi(siftlib, mp, a, b, 2, 0, n1=1 << 28), abi(siftlib, mp, a, b, 2, 0, p1=False),
               abi(siftlib, mp, a, b, 2, 0, p2=False), abi(siftlib, mp, a, b, 2, 0, out=False)]
    for t, (rc, idx, dist) in enumerate(refused):
        assert rc == _lib.EINVAL and (idx == -7).all() and (dist == -7).all(), t
    idx = np.full((257, 2), -7, np.int32)
    assert siftlib.siftmi_match_knn_window(None, a.ctypes.data, 257, 0, b.ctypes.data, 64, 0, 2, 0, C.c_float(4), C.c_float(4), C.c_float(0),
                                           C.c_float(0), idx.ctypes.data, idx.ctypes.data) == _lib.EINVAL and (idx == -7).all()
    # n1 == 0 writes nothing, n2 == 0 writes exactly n1 * k cells, a good call exactly n1 * k cells
    rc, idx, dist = abi(siftlib, mp, a[:0], b, 2, 1)
    assert rc == 0 and (idx == -7).all() and (dist == -7).all()
    rc, idx, dist = abi(siftlib, mp, a, b[:0], 3, 1)
    assert rc == 0
    for v in (idx, dist):
        assert (v.reshape(-1)[:257 * 3] == -1).all() and (v.reshape(-1)[257 * 3:] == -7).all()
    rc, idx, dist = abi(siftlib, mp, a, b, 3, 1)
    want = kw.knn(a, b, 3, 4.0, metric="l2")
    assert rc == 0 and (idx.reshape(-1)[257 * 3:] == -7).all() and (dist.reshape(-1)[257 * 3:] == -7).all()
    assert np.array_equal(idx.reshape(-1)[:257 * 3].reshape(257, 3), want[0]) and np.array_equal(dist.reshape(-1)[:257 * 3].reshape(257, 3), want[1])
    check(mp, a, b, 2.5, what="after the errors", ks=(2,))


# ---------------------------------------------------------------------------------------------- LinearAlign
def test_align_match_metric_and_ratio(siftlib, oracle):
    """the frames of test_align_max_shift_matches_cpu_pipeline (tests/test_gpu_match_window.py) with max_shift=12"""
    import sift_pyocl_amd as sp
    from sift_pyocl_amd.match import ratio_filter
    ref_img = smooth_noise((480, 512), seed=14, sigma=2.0)
    M_true = np.array([1.004, 0.018, -0.017, 0.997], np.float32); off_true = np.array([3.4, -2.2], np.float32)
    img = oracle.transform(ref_img, M_true, off_true, fill=0.0, mode=1)
    la = sp.LinearAlign(ref_img)
    before = la.align(img)
    k_ref = sort_kp(oracle.keypoints(ref_img)); kp = sort_kp(oracle.keypoints(img))

    def records(pairs):
        return {(k_ref[i].tobytes(), kp[j].tobytes()) for i, j in pairs}

    def matched(res):
        return {(p.tobytes(), q.tobytes()) for p, q in zip(res["matching"][:, 0], res["matching"][:, 1])}

    # Lowe's test on Euclidean distances inside the window: the restatement and ratio_filter on the oracle's keypoints
    res = la.align(img, return_all=True, max_shift=12, match_metric="l2", match_ratio=0.8)
    pairs = ratio_filter(*kw.knn(k_ref, kp, 2, 12, metric="l2"), ratio=0.8)
    assert len(pairs) >= 18 and res["matching"].shape[0] == len(pairs) and matched(res) == records(pairs)
    # the reference's ratio on L1 distances through knn: the set of align(max_shift=12)
    fixed = la.align(img, return_all=True, max_shift=12)
    res = la.align(img, return_all=True, max_shift=12, match_metric="l1", match_ratio=sp.par.MatchRatio)
    assert res["matching"].shape[0] == fixed["matching"].shape[0] >= 18 and matched(res) == matched(fixed)
    # without a window the same keywords go through brute-force knn
    res = la.align(img, return_all=True, match_metric="l2", match_ratio=0.8)
    pairs = ratio_filter(*kw.knn(k_ref, kp, 2, INF, metric="l2"), ratio=0.8)
    assert matched(res) == records(pairs)
    with pytest.raises(ValueError):
        la.align(img, match_metric="cosine")
    # the default call's bytes, before and after
    assert np.array_equal(before.view(np.uint8), la.align(img).view(np.uint8))
    assert np.array_equal(before.view(np.uint8), la.align(img, match_metric="l1", match_ratio=None).view(np.uint8))
