"""GPU tests of the device median: siftmi_match_shift / MatchPlan.shift give exactly what the numpy
restatement of the contract gives (tests/shift_ref.py) -- the six floats as bit patterns, NaN as "is NaN", the counts and the
keep mask exactly -- for every grid, wherever lists, pairs and mask lie, and LinearAlign.align(median="device") uses it end to
end with the results of the host path."""
import ctypes as C

import numpy as np
import pytest

import shift_ref as sr
from fit_ref import LSTSQ_BOUND
from util import assert_same_keypoints, smooth_noise

pytestmark = pytest.mark.gpu

FILL = np.float32(-77.0)
COUNT_FILL = -5
KEEP_FILL = 0xEE


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def abi_shift(L, mp, kp1, kp2, pairs, mask=None, blocks=0, tol=None, place=(0, 0, 0, 0), expect=0):
    """straight through the C ABI (include/siftmi.h); place = (kp1, kp2, pairs, mask) on the device?  Returns out (6,), counts
    (2,), keep (M,) uint8 or None -- all pre-filled with sentinels -- and the kernel time."""
    import torch
    from sift_pyocl_amd import _lib
    M = int(pairs.shape[0])
    hold = []

    def ptr(a, dev):
        a = np.ascontiguousarray(a)
        if dev:
            t = on_device(a); hold.append(t)
            return t.data_ptr()
        hold.append(a)
        return a.ctypes.data
    p1, p2, pp = ptr(kp1, place[0]), ptr(kp2, place[1]), ptr(pairs.astype(np.int32), place[2])
    pm = None if mask is None else ptr(np.asarray(mask).astype(np.uint8), place[3])
    if any(place):
        torch.cuda.synchronize()
    out = np.full(6, FILL, np.float32)
    counts = np.full(2, COUNT_FILL, np.int64)
    keep = None if tol is None else np.full(M, KEEP_FILL, np.uint8)
    ms = C.c_double(-1)
    rc = L.siftmi_match_shift(mp._handle, p1, len(kp1), place[0], p2, len(kp2), place[1], pp if M else None, M, place[2],
                              pm, place[3] if mask is not None else 0, blocks, C.c_float(0.0 if tol is None else tol),
                              None if tol is None else keep.ctypes.data, out.ctypes.data, counts.ctypes.data, C.byref(ms))
    assert rc == expect, _lib.last_error()
    return out, counts, keep, ms.value


def check(L, mp, kp1, kp2, pairs, what, mask=None, blocks=0, tol=None, place=(0, 0, 0, 0)):
    """one call against the restatement; returns the restatement's results"""
    want, wcounts, wkeep = sr.shift(kp1, kp2, pairs, mask, tol)
    out, counts, keep, ms = abi_shift(L, mp, kp1, kp2, pairs, mask, blocks, tol, place)
    assert sr.same_bits(out, want), "%r\n got  %r\n want %r" % (what, out, want)
    assert counts.tolist() == wcounts.tolist(), (what, counts, wcounts)
    if tol is not None:
        assert np.array_equal(keep, wkeep.astype(np.uint8)), what
    assert (ms > 0) == (len(pairs) > 0), what                                   # no pair: nothing is launched
    return want, wcounts, wkeep


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


@pytest.fixture(scope="module")
def case1000():
    return sr.make_case(1000, 4, 0.1, 16384.0)


@pytest.fixture(scope="module")
def case70001():
    return sr.make_case(70001, 7, 0.1, 16384.0)


@pytest.mark.parametrize("M", [0, 1, 2, 3, 4, 5, 18, 255, 256, 257, 1000])
def test_equal_to_restatement_with_the_default_grid(siftlib, mp, M):
    kp1, kp2, pairs, truth = sr.make_case(max(M, 4), 100 + M, 0.1, 16384.0)
    pairs = pairs[:M]
    want, counts, _ = check(siftlib, mp, kp1, kp2, pairs, M)
    assert counts[0] == M and np.isnan(want).all() == (M == 0)
    if M:       # and the restatement is the host path's value
        pts = sr.gather(kp1, kp2, pairs)
        assert want[sr.MDX] == np.median(pts[:, 2] - pts[:, 0]) and want[sr.MDY] == np.median(pts[:, 3] - pts[:, 1])


@pytest.mark.parametrize("blocks", [1, 2, 3, 7, 1024])
def test_the_grid_does_not_change_the_result(siftlib, mp, case1000, blocks):
    """1000 pairs: blocks = 1 is four pairs per lane (the last row ragged), 2 and 3 two rows, 7 and 1024 workgroups without a pair"""
    kp1, kp2, pairs, truth = case1000
    half = np.random.default_rng(3).random(1000) < 0.5
    plain = check(siftlib, mp, kp1, kp2, pairs, blocks, blocks=blocks, tol=0.5)
    check(siftlib, mp, kp1, kp2, pairs, (blocks, "half"), mask=half, blocks=blocks, tol=0.5)
    assert sr.same_bits(abi_shift(siftlib, mp, kp1, kp2, pairs)[0], plain[0])


def test_a_lane_owns_more_than_one_pair(siftlib, mp, case70001):
    """B reaches 256 at 65 536 pairs: a ragged second row at 70 001"""
    kp1, kp2, pairs, truth = case70001
    check(siftlib, mp, kp1, kp2, pairs, "plain", tol=0.5)
    half = np.random.default_rng(70001).random(70001) < 0.5
    check(siftlib, mp, kp1, kp2, pairs, "half", mask=half, tol=0.5)


def f32(bits):
    return np.asarray(bits, np.uint32).view(np.float32)


def crafted():
    """name -> (dx float32 (M,), what the restatement must find: (lo, hi) of x, or None); M <= 1024, x0 = 0 so x1 - x0 is exact"""
    rng = np.random.default_rng(17)
    sets = {}
    sets["all equal"] = (np.full(700, 2.5, np.float32), (2.5, 2.5))
    sets["lowest byte only"] = (f32(0x41200000 + rng.permutation(256)), f32([0x4120007f, 0x41200080]))
    # keys with one low part and 254 top bytes (a top byte of 0 with these low bits would be the key of a NaN)
    sets["highest byte only"] = (sr.unkey(((rng.permutation(255)[:254].astype(np.uint32) + 1) << 24) | 0x00345678), None)
    sets["around zero"] = (rng.permutation(np.arange(-300, 301).astype(np.float32) * np.float32(0.125))[:600], None)
    sets["zeros straddle"] = (rng.permutation(np.float32([-2, -1, -0.0, -0.0, 0.0, 0.0, 1, 2] * 50 + [-0.0, 0.0])), None)
    sets["minus zero below plus zero"] = (np.float32([0.0, -0.0, 3.0, -3.0]), (-0.0, 0.0))
    sets["sum rounds"] = (np.float32([1.0, 1.0000001, 0.5, 7.0]), f32([0x3f800000, 0x3f800001]))
    sets["subnormal"] = (rng.permutation((np.arange(-250, 251) * 3).astype(np.float32) * np.float32(1.4e-45))[:500], None)
    mid = np.float32(11.75)
    sets["duplicated middle"] = (rng.permutation(np.concatenate([np.full(600, mid), rng.normal(11.75, 4, 424).astype(np.float32)])), (mid, mid))
    sets["top bins differ"] = (np.float32([-3.0, -2.0, -1.5, 1e20, 2e20, 3e30]), (-1.5, 1e20))
    sets["odd, large"] = (np.float32([3e38, 3e38, -1.0]), (3e38, 3e38))
    return sets


@pytest.mark.parametrize("name", sorted(crafted()))
def test_crafted_displacements(siftlib, mp, name):
    dx, pinned = crafted()[name]
    kp1, kp2, pairs = sr.lists_from_displacements(dx, seed=len(dx))
    pts = sr.gather(kp1, kp2, pairs)
    assert np.array_equal((pts[:, 2] - pts[:, 0]).view(np.uint32), dx.view(np.uint32))      # the displacements are the crafted ones
    for blocks in (0, 3):
        want, counts, keep = check(siftlib, mp, kp1, kp2, pairs, (name, blocks), blocks=blocks, tol=0.0)
        assert counts[0] == len(dx)
        if pinned is not None:
            assert sr.same_bits(want[[sr.LO_DX, sr.HI_DX]], np.float32(pinned)), (name, want)
        assert sr.same_bits(want[[sr.LO_DY, sr.HI_DY]], want[[sr.LO_DX, sr.HI_DX]])        # dy is dx reversed: the same multiset


def test_crafted_sets_are_what_their_names_say():
    sets = crafted()
    assert all(len(v[0]) <= 1024 for v in sets.values())
    k = sr.key(sets["lowest byte only"][0]); assert len(set(k >> 8)) == 1 and len(set(k & 255)) == 256
    k = sr.key(sets["highest byte only"][0]); assert len(set(k & 0xFFFFFF)) == 1 and len(set(k >> 24)) == 254
    z = sets["zeros straddle"][0]; lo, hi = sr.middle(z)[1:]
    assert np.signbit(lo) and not np.signbit(hi) and lo == hi == 0 and len(z) % 2 == 0
    s = sets["sum rounds"][0]; med, lo, hi = sr.middle(s)
    assert np.float64(lo) + np.float64(hi) != np.float64(np.float32(lo + hi))                # the f32 sum is inexact
    k = sr.key(sets["top bins differ"][0]); k.sort(); assert k[2] >> 24 != k[3] >> 24
    sub = sets["subnormal"][0]; assert (np.abs(sub) < np.float32(1.2e-38)).all() and len(set(sub.tolist())) > 400


def test_infinite_displacements_from_finite_positions(siftlib, mp):
    """x1 - x0 overflows for positions of +-3e38: -inf, +inf take part; an even count with lo = -inf, hi = +inf has a NaN median"""
    big = np.float32(3e38)
    kp1 = np.zeros(6, sr.DTYPE_KP); kp2 = np.zeros(6, sr.DTYPE_KP)
    kp1["x"] = [-big, -big, big, big, 0, 0]; kp2["x"] = [big, big, -big, -big, 1, 2]
    kp1["y"] = [0, 0, 0, 0, 0, 0]; kp2["y"] = [1, 2, 3, 4, 5, 6]
    idx = np.arange(6, dtype=np.int32); pairs = np.stack([idx, idx], axis=1)
    want, counts, keep = check(siftlib, mp, kp1, kp2, pairs, "inf", tol=np.inf)
    assert counts.tolist() == [6, 6] and want[sr.LO_DX] == 1 and want[sr.HI_DX] == 2 and want[sr.MDX] == 1.5
    want, counts, keep = check(siftlib, mp, kp1, kp2, pairs[:4], "inf only", tol=np.inf)
    assert want[sr.LO_DX] == -np.inf and want[sr.HI_DX] == np.inf and np.isnan(want[sr.MDX]) and counts.tolist() == [4, 0]
    want, counts, keep = check(siftlib, mp, kp1, kp2, pairs[:3], "odd inf", tol=np.inf)
    assert want[sr.MDX] == np.inf and want[sr.MDY] == 2 and counts.tolist() == [3, 0] and not keep.any()


def test_pairs_that_are_not_used(siftlib, mp, case1000):
    kp1, kp2, pairs, truth = case1000
    kp1, kp2, bad = kp1.copy(), kp2.copy(), pairs.copy()
    bad[3, 0] = -1; bad[500, 0] = len(kp1); bad[999, 1] = len(kp2); bad[0, 1] = -1; bad[256, 0] = -2 ** 31
    kp1["x"][pairs[10, 0]] = np.nan; kp1["y"][pairs[11, 0]] = np.inf
    kp2["x"][pairs[12, 1]] = -np.inf; kp2["y"][pairs[700, 1]] = np.nan
    for place in ((0, 0, 0, 0), (1, 1, 1, 0)):
        want, counts, keep = check(siftlib, mp, kp1, kp2, bad, place, tol=np.inf, place=place)
        assert counts.tolist() == [991, 991] and not keep[[3, 500, 999, 0, 256, 10, 11, 12, 700]].any()
    half = np.random.default_rng(8).random(1000) < 0.5
    want, counts, keep = check(siftlib, mp, kp1, kp2, bad, "half", mask=half, tol=0.5)
    assert 400 < counts[0] < 600
    plain = check(siftlib, mp, kp1, kp2, bad, "none")[0]
    assert sr.same_bits(check(siftlib, mp, kp1, kp2, bad, "0x80", mask=np.full(1000, 0x80, np.uint8))[0], plain)
    # everything masked, every pair void: EMPTY, and keep is written (zeros) all the same
    for what, p, m in (("masked", bad, np.zeros(1000, np.uint8)), ("void", np.full((300, 2), -1, np.int32), None)):
        want, counts, keep = check(siftlib, mp, kp1, kp2, p, what, mask=m, tol=np.inf)
        assert np.isnan(want).all() and counts.tolist() == [0, 0] and not keep.any()


@pytest.mark.parametrize("place", [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1)])
def test_same_result_wherever_the_inputs_lie(siftlib, mp, case1000, place):
    kp1, kp2, pairs, truth = case1000
    half = np.random.default_rng(3).random(1000) < 0.5
    check(siftlib, mp, kp1, kp2, pairs, place, mask=half, tol=0.5, place=place)
    check(siftlib, mp, kp1, kp2, pairs, place, place=place)


def test_a_small_call_after_a_large_one(siftlib, case70001):
    """stale scratch: the counters, keys and keep bytes of 70 001 pairs lie behind the 5 pairs of the next call"""
    import sift_pyocl_amd as sp
    own = sp.MatchPlan()
    kp1, kp2, pairs, truth = case70001
    check(siftlib, own, kp1, kp2, pairs, "large", tol=np.inf)
    s1, s2, sp_ = sr.lists_from_displacements(np.float32([5, -1, 9, 2, 2]), seed=1)
    want = check(siftlib, own, s1, s2, sp_, "small", tol=0.0)[0]
    assert want[sr.MDX] == 2
    check(siftlib, own, s1, s2, sp_[:0], "none", tol=0.0)
    check(siftlib, own, kp1, kp2, pairs[:300], "again", mask=np.zeros(300, np.uint8), tol=1.0)
    check(siftlib, own, s1, s2, sp_, "small again")


@pytest.mark.parametrize("tol", [0.0, 0.5, np.inf])
def test_keep(siftlib, mp, case1000, tol):
    kp1, kp2, pairs, truth = case1000
    kp1, kp2 = kp1.copy(), kp2.copy()
    sel = pairs[np.arange(1000) % 5 != 0]                                         # a tied middle, so that tol = 0 keeps something
    kp1["x"][sel[:, 0]] = 100.0; kp1["y"][sel[:, 0]] = 200.0; kp2["x"][sel[:, 1]] = 102.0; kp2["y"][sel[:, 1]] = 199.0
    want, counts, keep = check(siftlib, mp, kp1, kp2, pairs, tol, tol=tol)
    pts = sr.gather(kp1, kp2, pairs)
    dx, dy = pts[:, 2] - pts[:, 0], pts[:, 3] - pts[:, 1]
    direct = (np.abs(dx - np.median(dx)) <= np.float32(tol)) & (np.abs(dy - np.median(dy)) <= np.float32(tol))
    assert np.array_equal(keep, direct) and 800 <= counts[1] <= 1000 and (counts[1] == 1000) == (tol == np.inf)
    # without keep the second count is 0 and tol plays no part, NaN included
    out, c, _, _ = abi_shift(siftlib, mp, kp1, kp2, pairs)
    assert sr.same_bits(out, want) and c.tolist() == [1000, 0]


def test_argument_errors_launch_nothing_and_write_nothing(siftlib, mp, case1000):
    from sift_pyocl_amd import _lib
    kp1, kp2, pairs, truth = case1000
    out = np.full(6, FILL, np.float32)
    counts = np.full(2, COUNT_FILL, np.int64)
    keep = np.full(1000, KEEP_FILL, np.uint8)
    ms = C.c_double(-1)

    def call(h=mp._handle, k1=kp1.ctypes.data, n1=len(kp1), k2=kp2.ctypes.data, n2=len(kp2), pp=pairs.ctypes.data, m=1000, blocks=0,
             tol=1.0, kp=keep.ctypes.data, o=out.ctypes.data, c=counts.ctypes.data):
        return siftlib.siftmi_match_shift(h, k1, n1, 0, k2, n2, 0, pp, m, 0, None, 0, blocks, C.c_float(tol), kp, o, c, C.byref(ms))
    for kw in (dict(h=None), dict(o=None), dict(c=None), dict(m=-1), dict(n1=-1), dict(n2=-7), dict(m=2 ** 31), dict(n1=2 ** 31),
               dict(n2=2 ** 40), dict(k1=None), dict(k2=None), dict(pp=None), dict(blocks=-1), dict(blocks=1025),
               dict(tol=-1.0), dict(tol=float("nan")), dict(tol=-0.5, m=0)):
        assert call(**kw) == _lib.EINVAL, kw
        assert _lib.last_error()
        assert (out == FILL).all() and (counts == COUNT_FILL).all() and (keep == KEEP_FILL).all() and ms.value == -1, kw
    # a valid call after the refused ones is right; a tol no keep mask reads is not looked at
    check(siftlib, mp, kp1, kp2, pairs, "after EINVAL", tol=1.0)
    assert call(tol=float("nan"), kp=None) == _lib.OK and sr.same_bits(out, sr.shift(kp1, kp2, pairs)[0]) and counts.tolist() == [1000, 0]
    assert ms.value > 0 and (keep == KEEP_FILL).all()
    # no pairs: EMPTY, nothing launched, also with null lists of length 0 and null pairs
    out[:] = FILL
    assert call(m=0) == _lib.OK and np.isnan(out).all() and counts.tolist() == [0, 0] and ms.value == 0 and (keep == KEEP_FILL).all()
    out[:] = FILL
    assert call(k1=None, n1=0, k2=None, n2=0, pp=None, m=0) == _lib.OK and np.isnan(out).all()
    with pytest.raises(RuntimeError):
        mp.shift(kp1, kp2, pairs, blocks=2000)
    with pytest.raises(RuntimeError):
        mp.shift(kp1, kp2, pairs.astype(np.int64))
    with pytest.raises(RuntimeError):
        mp.shift(kp1, kp2, pairs, mask=np.ones(999, np.uint8))
    with pytest.raises(RuntimeError):
        mp.shift(kp1, kp2, pairs, tol=-1.0)


def test_python_entry(siftlib, mp, case1000):
    import torch
    kp1, kp2, pairs, truth = case1000
    half = np.random.default_rng(8).random(1000) < 0.5
    for mask in (None, half, half.view(np.uint8)):
        want, wcounts, wkeep = sr.shift(kp1, kp2, pairs, mask, 0.5)
        res = mp.shift(kp1, kp2, pairs, mask=mask)
        assert len(res) == 2 and len(res[0]) == 2 and type(res[0][0]) is np.float32 and type(res[0][1]) is np.float32 and type(res[1]) is int
        assert sr.same_bits(np.float32(res[0]), want[:2]) and res[1] == wcounts[0]
        (dx, dy), n, keep, raw = mp.shift(kp1, kp2, pairs, mask=mask, tol=0.5, return_ranks=True)
        assert keep.dtype == np.bool_ and keep.shape == (1000,) and np.array_equal(keep, wkeep)
        assert raw.dtype == np.float32 and raw.shape == (6,) and sr.same_bits(raw, want)
        assert len(mp.shift(kp1, kp2, pairs, mask=mask, tol=0.5)) == 3 and len(mp.shift(kp1, kp2, pairs, mask=mask, return_ranks=True)) == 3
    # device tensors, a bool mask tensor among them, and a grid of the caller's
    t1, t2, tp, tm = on_device(kp1), on_device(kp2), torch.from_numpy(pairs).cuda(), torch.from_numpy(half).cuda()
    (dx, dy), n, keep, raw = mp.shift(t1, t2, tp, mask=tm, tol=0.5, blocks=3, return_ranks=True)
    want, wcounts, wkeep = sr.shift(kp1, kp2, pairs, half, 0.5)
    assert sr.same_bits(raw, want) and n == wcounts[0] and np.array_equal(keep, wkeep)
    # no usable pair: no displacement
    assert mp.shift(kp1, kp2, pairs, mask=np.zeros(1000, bool)) == (None, 0)
    assert mp.shift(kp1, kp2, pairs[:0]) == (None, 0)
    moved, n, keep, raw = mp.shift(kp1, kp2, pairs[:0], tol=1.0, return_ranks=True)
    assert moved is None and n == 0 and keep.shape == (0,) and np.isnan(raw).all()


def test_profile_appends_a_shift_event(siftlib, case1000):
    import sift_pyocl_amd as sp
    kp1, kp2, pairs, truth = case1000
    prof = sp.MatchPlan(profile=True)
    prof.shift(kp1, kp2, pairs)
    assert [label for label, _ in prof.events] == ["shift"]
    assert 0 < prof.events[0][1].profile.end - prof.events[0][1].profile.start < 1e9


# ---------------------------------------------------------------------------------------------- end to end on images
def same_arrays(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def pair_rows(matching, keep=None):
    """the matched record pairs as a sorted list of their bytes: keypoints() appends its records in no fixed order, so two calls
    on one frame return the same keypoints and the same matches in another order"""
    m = np.ascontiguousarray(matching)
    assert m.ndim == 2 and m.shape[1] == 2 and m.dtype.itemsize == 144
    rows = m.view(np.uint8).reshape(m.shape[0], 288)
    return sorted(r.tobytes() for r in (rows if keep is None else rows[keep]))


def assert_same_alignment(host, dev, what):
    assert sorted(host) == sorted(dev), what
    assert same_arrays(host["result"], dev["result"]), what
    assert same_arrays(host["matrix"], dev["matrix"]), what
    assert host["offset"].dtype == dev["offset"].dtype == np.float32 and (host["offset"] == dev["offset"]).all(), (what, host["offset"], dev["offset"])
    assert_same_keypoints(host["keypoint"], dev["keypoint"], "keypoint")
    assert pair_rows(host["matching"]) == pair_rows(dev["matching"]), what
    if "inliers" in host:
        assert pair_rows(host["matching"], host["inliers"]) == pair_rows(dev["matching"], dev["inliers"]), what
    # the host path's rms on both sides: a float32 mean over the pairs in the order of the call, equal up to that order
    assert abs(float(dev["rms"]) - float(host["rms"])) <= 1e-5 * float(host["rms"]), what


@pytest.fixture(scope="module")
def gray_pair(siftlib):
    """the 512 x 512 pair of test_gpu_align.py::test_align_shift_only_recovers_translation"""
    big = smooth_noise((600, 640), seed=12, sigma=2.0)
    return np.ascontiguousarray(big[20:532, 30:542]), np.ascontiguousarray(big[27:539, 19:531])


@pytest.fixture(scope="module")
def rgb_pair(siftlib):
    """the RGB pair of test_gpu_align.py::test_align_rgb_and_extra_and_relative"""
    base = smooth_noise((300, 330), seed=16, sigma=1.5)
    base = (255 * (base - base.min()) / (base.max() - base.min()))
    rgb_big = np.stack([base, base[::-1, ::-1], base.T[:300, :300].repeat(2, axis=1)[:, :330]], axis=-1).astype(np.uint8)
    return np.ascontiguousarray(rgb_big[10:266, 12:268]), np.ascontiguousarray(rgb_big[14:270, 9:265])


def test_shift_is_numpy_median_over_the_host_gathers_on_a_real_frame_pair(gray_pair):
    import sift_pyocl_amd as sp
    ref, img = gray_pair
    la = sp.LinearAlign(ref)
    kp = la.sift.keypoints(img)
    pairs = la.match.match(la.ref_kp, kp, raw_results=True)
    assert pairs.shape[0] > 100
    g0, g1 = la._xysa(la.ref_kp)[pairs[:, 0]], la._xysa(kp)[pairs[:, 1]]
    matrix, offset = la._median_shift(g0, g1)
    (dx, dy), n = la.match.shift(la.ref_kp, kp, pairs)
    assert n == pairs.shape[0] and dy == offset[0] and dx == offset[1]
    (dx, dy), n = la.match.shift(la._ref_dev, la.sift.device_records(), pairs)      # where align() reads them
    assert n == pairs.shape[0] and dy == offset[0] and dx == offset[1]
    assert abs(offset[0] + 7.0) < 0.05 and abs(offset[1] - 11.0) < 0.05


@pytest.mark.parametrize("kw", [dict(), dict(max_shift=16), dict(robust=True), dict(double_check=True), dict(robust=True, max_shift=16)],
                         ids=lambda kw: "+".join(sorted(kw)) or "plain")
@pytest.mark.parametrize("pair", ["gray", "rgb"])
def test_align_with_the_device_median_is_the_host_path(gray_pair, rgb_pair, pair, kw):
    import sift_pyocl_amd as sp
    ref, img = gray_pair if pair == "gray" else rgb_pair
    la = sp.LinearAlign(ref, extra=(4, 6) if pair == "rgb" else 0)
    host = la.align(img, shift_only=True, return_all=True, **kw)
    dev = la.align(img, shift_only=True, return_all=True, median="device", **kw)
    assert host["matching"].shape[0] > 18
    if "double_check" not in kw:        # (double_check re-fits an affine map on the pairs it keeps, on the host, on either side)
        assert np.array_equal(dev["matrix"], np.identity(2, dtype=np.float32))
    assert_same_alignment(host, dev, (pair, kw))
    # without return_all: the same image
    assert same_arrays(la.align(img, shift_only=True, median="device", **kw), host["result"])
    # median= leaves an affine estimate alone, on either side: the same fit on the same pairs, in the order of each call (the
    # bound on what that order can change is the one of test_gpu_fit.py: fit_ref.LSTSQ_BOUND plus a float32 spacing)
    for est in ("host", "device"):
        a, b = la.align(img, return_all=True, estimate=est, **kw), la.align(img, return_all=True, estimate=est, median="device", **kw)
        assert pair_rows(a["matching"]) == pair_rows(b["matching"]) and not np.array_equal(b["matrix"], np.identity(2, dtype=np.float32))
        for key in ("matrix", "offset"):
            tol = LSTSQ_BOUND + np.spacing(np.maximum(np.abs(a[key]), np.abs(b[key])))
            assert (np.abs(a[key].astype(np.float64) - b[key].astype(np.float64)) <= tol).all(), (pair, kw, est, key, a[key], b[key])


@pytest.mark.parametrize("pair", ["gray", "rgb"])
def test_align_relative_with_the_device_median(gray_pair, rgb_pair, pair):
    import sift_pyocl_amd as sp
    ref, img = gray_pair if pair == "gray" else rgb_pair
    la_h, la_d = sp.LinearAlign(ref), sp.LinearAlign(ref)
    for step, (frame, return_all) in enumerate(((img, True), (img, False), (ref, True))):
        host = la_h.align(frame, shift_only=True, relative=True, return_all=return_all)
        dev = la_d.align(frame, shift_only=True, relative=True, return_all=return_all, median="device")
        if return_all:
            assert_same_alignment(host, dev, (pair, step))
        else:
            assert same_arrays(host, dev)
        assert np.array_equal(la_h.relative_transfo, la_d.relative_transfo) and len(la_h.ref_kp) == len(la_d.ref_kp)


def test_align_below_18_matches_takes_the_device_median(siftlib):
    """the sparse frame of test_gpu_fit.py: a 40 x 40 patch of the reference in other noise"""
    import sift_pyocl_amd as sp
    S = 320
    big = smooth_noise((S + 64, S + 64), seed=21, sigma=2.0)
    ref = np.ascontiguousarray(big[32:32 + S, 32:32 + S])
    few = smooth_noise((S, S), seed=99, sigma=2.0)
    few[100:140, 120:160] = ref[100:140, 120:160]
    la = sp.LinearAlign(ref, profile=True)
    for kw in (dict(), dict(estimate="device"), dict(robust=True), dict(robust=True, estimate="device")):
        host = la.align(few, return_all=True, **kw)
        assert 0 < host["matching"].shape[0] < 18
        la.match.reset_timer()
        dev = la.align(few, return_all=True, median="device", **kw)
        assert "shift" in [label for label, _ in la.match.events], kw            # the estimate did come from MatchPlan.shift
        assert_same_alignment(host, dev, kw)
        assert same_arrays(la.align(few, median="device", **kw), host["result"])


def test_align_gathers_nothing_on_the_host_without_return_all(gray_pair):
    import sift_pyocl_amd as sp
    ref, img = gray_pair
    la = sp.LinearAlign(ref)
    assert la._ref_heads is None
    got = la.align(img, shift_only=True, median="device")
    assert la._ref_heads is None
    la.align(img, shift_only=True, median="device", robust=True, max_shift=16)
    assert la._ref_heads is None
    want = la.align(img, shift_only=True)
    assert la._ref_heads is not None and same_arrays(got, want)


def test_align_refuses_an_unknown_median_and_the_default_is_the_host(gray_pair):
    import sift_pyocl_amd as sp
    ref, img = gray_pair
    la = sp.LinearAlign(ref)
    with pytest.raises(ValueError):
        la.align(img, median="bogus")
    assert same_arrays(la.align(img), la.align(img, median="host"))
    assert same_arrays(la.align(img, shift_only=True), la.align(img, shift_only=True, median="host"))
