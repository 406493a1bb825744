"""GPU tests of windowed matching: MatchPlan.match(window=, window_shift=) and
LinearAlign.align(max_shift=) against the numpy restatement of the contract (tests/window_ref.py, itself pinned against the
oracle by tests/test_window_ref_host.py).  Every comparison of pairs is exact: the sorted rows are equal."""
import ctypes as C

import numpy as np
import pytest

import window_ref as wr
from util import dtype_kp, smooth_noise, sort_kp, sort_rows

pytestmark = pytest.mark.gpu
INF = float("inf")


def check(mp, a, b, window, shift=(0.0, 0.0), mutual=False, what=""):
    got = mp.match(a, b, raw_results=True, mutual=mutual, window=window, window_shift=shift)
    want = wr.match(a, b, window, shift, mutual=mutual)
    what = "%s window %s shift %s mutual %s" % (what, window, shift, mutual)
    assert got.dtype == np.int32 and got.ndim == 2 and got.shape[1] == 2, what
    assert len(got) == len(want), "%s: %d pairs, restatement %d" % (what, len(got), len(want))
    assert np.array_equal(sort_rows(got), sort_rows(want)), what
    return len(got)


@pytest.mark.parametrize("n1,n2", [(700, 650), (257, 64), (5, 900), (3000, 5000)])
def test_crafted_lists_vs_restatement(siftlib, n1, n2):
    import sift_pyocl_amd as sp
    mp = sp.MatchPlan()
    total = 0
    for shift in ((0.0, 0.0), (3.25, -1.5)):
        a, b = wr.crafted(n1, n2, seed=n1 + n2, shift=shift)
        for window in (0, 2.5, (7, 3), INF):
            for mutual in (False, True):
                total += check(mp, a, b, window, shift, mutual, "crafted %dx%d" % (n1, n2))
    if min(n1, n2) >= 64:
        assert total > 0


def boundary_lists():
    """Row k of list 2 carries the descriptor of row k of list 1 (+-6 per byte) and sits on, or a few float32 steps beside, the edge
    of that keypoint's window: the pair (k, k) comes out iff row k is a candidate.  The first 24 queries are 200 px apart, each
    with that ONE keypoint near it (a lone candidate always pairs).  Returns the lists, (sx, sy), (wx, wy) and, for the positions
    that are exact in float32, the pairs that must / must not come out."""
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


def test_window_boundaries(siftlib):
    import sift_pyocl_amd as sp
    a, b, shift, window, must, never = boundary_lists()
    mp = sp.MatchPlan()
    for mutual in (False, True):
        check(mp, a, b, window, shift, mutual, "boundaries")
    got = {tuple(r) for r in mp.match(a, b, raw_results=True, window=window, window_shift=shift)}
    # the cases whose positions are exact in float32: on the edge is a candidate, one step beyond is not
    ok = wr.candidate_matrix(a, b, window, shift)
    for k in must:
        assert ok[k, k] and (k, k) in got, k
    for k in never:
        assert not ok[k, k] and (k, k) not in got, k
    # the frame without the huge coordinates: a fine grid over the same boundary cases
    n = len(a) - 6
    for mutual in (False, True):
        check(mp, a[:n], b[:n], window, shift, mutual, "boundaries, finite")
    # the 16 000 block alone, also with a zero shift and a window of one float32 step
    big = np.abs(a["x"][:n]) > 8000
    assert check(mp, a[:n][big], b[:n][big], window, shift, False, "boundaries, 16 000 block") > 100
    # a window of one float32 step centred on the right edge: the rows one step to either side are in, two steps are out
    assert check(mp, a[:n][big], b[:n][big], 2.0 ** -10, (shift[0] + window[0], shift[1]), True, "boundaries, 16 000 block, tiny window") > 50


def test_one_cell_and_crowded(siftlib):
    """every keypoint of both lists inside one cell (a window wider than the lists' extent), and lists that are one point"""
    import sift_pyocl_amd as sp
    mp = sp.MatchPlan()
    a, b, _ = wr.lists(900, 1100, 400, seed=9, H=1, W=1)
    for window in (5.0, 0.25, (0.05, 5.0)):
        check(mp, a, b, window, (0.0, 0.0), False, "one cell")
        check(mp, a, b, window, (0.1, -0.1), True, "one cell")
    a["x"] = 3.5; a["y"] = -2.25; b["x"] = 3.5; b["y"] = -2.25
    assert check(mp, a, b, 0, (0.0, 0.0), True, "one point") > 0
    assert check(mp, a, b, 0, (1.0, 0.0), False, "one point, shifted away") == 0


@pytest.mark.parametrize("n1,n2", [(700, 650), (257, 64), (5, 900), (3000, 5000)])
def test_infinite_window_is_plain_match(siftlib, oracle, n1, n2):
    """I1: window inf, shift 0, finite coordinates -> exactly match(), also with mutual"""
    import sift_pyocl_amd as sp
    mp = sp.MatchPlan()
    a, b = wr.crafted(n1, n2, seed=n1 + n2)
    for mutual in (False, True):
        plain = mp.match(a, b, raw_results=True, mutual=mutual)
        got = mp.match(a, b, raw_results=True, mutual=mutual, window=INF)
        want, n = oracle.match_ex(a, b, None, 0, mutual=mutual, cap=max(1, len(a)))
        assert len(got) == len(plain) == n
        assert np.array_equal(sort_rows(got), sort_rows(plain)) and np.array_equal(sort_rows(got), sort_rows(want))


def real_pair():
    import sift_pyocl_amd as sp
    big = smooth_noise((700, 760), seed=21, sigma=2.0)
    i1 = np.ascontiguousarray(big[10:650, 20:724]); i2 = np.ascontiguousarray(big[17:657, 9:713])
    plan = sp.SiftPlan(template=i1)
    return plan.keypoints(i1), plan.keypoints(i2)


def test_real_keypoints_window_16(siftlib):
    """I2 on real keypoints (the crops of test_mutual_on_real_keypoints: content moved by +11 / -7), and the displacement"""
    import sift_pyocl_amd as sp
    k1, k2 = real_pair()
    mp = sp.MatchPlan()
    n = check(mp, k1, k2, 16, what="real keypoints")
    check(mp, k1, k2, 16, mutual=True, what="real keypoints")
    check(mp, k1, k2, 6, (11.0, -7.0), what="real keypoints, centred window")
    plain = mp.match(k1, k2, raw_results=True)
    got = mp.match(k1, k2, raw_results=True, window=16)
    inside = wr.subset_in_window(plain, k1, k2, 16)
    assert len(inside) > 50 and {tuple(r) for r in inside} <= {tuple(r) for r in got}
    dx = k2["x"][got[:, 1]] - k1["x"][got[:, 0]]; dy = k2["y"][got[:, 1]] - k1["y"][got[:, 0]]
    print("windowed pairs %d (plain %d, inside %d), median displacement (%.4f, %.4f)" % (n, len(plain), len(inside), np.median(dx), np.median(dy)))
    assert abs(np.median(dx) - 11.0) < 0.1 and abs(np.median(dy) + 7.0) < 0.1


def test_device_lists_and_records(siftlib):
    import torch
    import sift_pyocl_amd as sp
    mp = sp.MatchPlan()
    shift, window = (3.25, -1.5), (7, 3)
    a, b = wr.crafted(700, 650, seed=3, shift=shift)
    want = sort_rows(wr.match(a, b, window, shift))
    da = torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda(); db = torch.from_numpy(b.view(np.uint8).reshape(-1).copy()).cuda()
    for l1, l2 in ((da, db), (a, db), (da, b)):
        assert np.array_equal(sort_rows(mp.match(l1, l2, raw_results=True, window=window, window_shift=shift)), want)
    assert np.array_equal(sort_rows(mp.match(da, db, raw_results=True, window=window, window_shift=shift, mutual=True)),
                          sort_rows(wr.match(a, b, window, shift, mutual=True)))
    rec = mp.match(a, b, window=window, window_shift=shift)
    assert rec.shape == (len(want), 2) and rec.dtype == sp.MatchPlan.dtype_kp
    assert (np.abs((rec[:, 1].x - rec[:, 0].x) - np.float32(shift[0])) <= window[0]).all()
    assert (np.abs((rec[:, 1].y - rec[:, 0].y) - np.float32(shift[1])) <= window[1]).all()
    with pytest.raises(RuntimeError):
        mp.match(da, db, window=window)                     # records need host lists, as for match()


def test_profile_events_and_kernel_time(siftlib):
    import sift_pyocl_amd as sp
    a, b = wr.crafted(700, 650, seed=4)
    mp = sp.MatchPlan(profile=True)
    got = mp.match(a, b, raw_results=True, window=2.5)
    assert len(got) > 0 and mp.kernel_ms() > 0
    assert [l for l, _ in mp.events] == list(sp.MatchPlan.STAGE_LABELS)
    for label, evt in mp.events:
        assert 0 <= evt.profile.end - evt.profile.start < 1e9, label


def test_errors_and_empty(siftlib):
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    a, b = wr.crafted(300, 200, seed=5)
    mp = sp.MatchPlan()
    assert mp.match(a[:0], b, raw_results=True, window=4).shape == (0, 2)
    assert mp.match(a, b[:0], raw_results=True, window=4, mutual=True).shape == (0, 2)
    for bad in (-1.0, float("nan"), (3.0, -0.5), (float("nan"), 3.0)):
        with pytest.raises(RuntimeError):
            mp.match(a, b, raw_results=True, window=bad)
    for bad in ((INF, 0.0), (0.0, float("nan"))):
        with pytest.raises(RuntimeError):
            mp.match(a, b, raw_results=True, window=4, window_shift=bad)
    mp.set_roi(np.ones((90, 120), np.int8))
    with pytest.raises(RuntimeError):
        mp.match(a, b, raw_results=True, window=4, roi_mode=2)
    assert len(mp.match(a, b, raw_results=True, window=4)) == len(wr.match(a, b, 4))      # a region of interest alone changes nothing
    # the C ABI: null / negative list arguments, and the capacity convention of siftmi_match_ex
    n, total = C.c_int64(-5), C.c_int64(-5)
    pairs = np.empty((300, 2), np.int32)
    args = (C.c_float(wr.RATIO), C.c_float(4), C.c_float(4), C.c_float(0), C.c_float(0), 0)
    assert siftlib.siftmi_match_window(mp._handle, None, 5, 0, b.ctypes.data, len(b), 0, *args, pairs.ctypes.data, 300, C.byref(n), C.byref(total)) == _lib.EINVAL
    assert siftlib.siftmi_match_window(mp._handle, a.ctypes.data, -1, 0, b.ctypes.data, len(b), 0, *args, pairs.ctypes.data, 300, C.byref(n), C.byref(total)) == _lib.EINVAL
    want = len(wr.match(a, b, 4))
    assert want > 3
    rc = siftlib.siftmi_match_window(mp._handle, a.ctypes.data, len(a), 0, b.ctypes.data, len(b), 0, *args, pairs.ctypes.data, 3, C.byref(n), C.byref(total))
    assert rc == _lib.ECAPACITY and n.value == 3 and total.value == want


def test_align_max_shift_recovers_translation(siftlib):
    import sift_pyocl_amd as sp
    big = smooth_noise((600, 640), seed=12, sigma=2.0)
    ref_img = np.ascontiguousarray(big[20:532, 30:542])
    img = np.ascontiguousarray(big[27:539, 19:531])          # the frames of test_align_shift_only_recovers_translation
    la = sp.LinearAlign(ref_img)
    res = la.align(img, shift_only=True, return_all=True, max_shift=16)
    assert res["matching"].shape[0] > 100
    assert np.array_equal(res["matrix"], np.identity(2, dtype=np.float32))
    assert abs(res["offset"][0] - (-7.0)) < 0.05 and abs(res["offset"][1] - 11.0) < 0.05


def test_align_max_shift_matches_cpu_pipeline(siftlib, oracle):
    """the frames of test_align_affine_matches_cpu_pipeline: exactly the pair set of the restatement on the oracle's keypoints"""
    import sift_pyocl_amd as sp
    from sift_pyocl_amd.utils import matching_correction
    ref_img = smooth_noise((480, 512), seed=14, sigma=2.0)
    M_true = np.array([1.004, 0.018, -0.017, 0.997], np.float32); off_true = np.array([3.4, -2.2], np.float32)
    img = oracle.transform(ref_img, M_true, off_true, fill=0.0, mode=1)
    la = sp.LinearAlign(ref_img)
    plain = la.align(img)
    assert np.array_equal(plain.view(np.uint8), la.align(img, max_shift=None).view(np.uint8))       # the default path, untouched
    res = la.align(img, return_all=True, max_shift=12)
    k_ref = sort_kp(oracle.keypoints(ref_img)); kp = sort_kp(oracle.keypoints(img))
    pairs = wr.match(k_ref, kp, 12)
    n = len(pairs)
    assert n == res["matching"].shape[0] and n >= 18
    m = np.recarray(shape=(n, 2), dtype=dtype_kp)
    m[:, 0] = k_ref[pairs[:, 0]]; m[:, 1] = kp[pairs[:, 1]]
    got_pairs = {(a.tobytes(), b.tobytes()) for a, b in zip(res["matching"][:, 0], res["matching"][:, 1])}
    assert got_pairs == {(a.tobytes(), b.tobytes()) for a, b in zip(m[:, 0], m[:, 1])}
    t = matching_correction(m)
    assert np.allclose([t[4], t[3], t[1], t[0]], res["matrix"].reshape(4), rtol=0, atol=2e-6)
    assert np.allclose([t[5], t[2]], res["offset"], rtol=0, atol=2e-4)
    # and the default call still is the brute-force pipeline
    full = la.align(img, return_all=True)
    assert full["matching"].shape[0] == oracle.match(k_ref, kp)[1]
    assert np.array_equal(full["result"].view(np.uint8), plain.view(np.uint8))
