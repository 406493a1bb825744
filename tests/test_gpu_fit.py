"""GPU tests of the device fit: siftmi_match_fit / MatchPlan.fit give exactly what the numpy
restatement of the contract gives (tests/fit_ref.py) -- all 20 doubles as bit patterns, NaN as "is NaN" -- for every grid,
wherever lists, pairs and mask lie, and LinearAlign.align(estimate="device") uses it end to end."""
import ctypes as C

import numpy as np
import pytest

import fit_ref as fr
from util import assert_same_keypoints, smooth_noise

pytestmark = pytest.mark.gpu

FILL = -77.0


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def abi_fit(L, mp, kp1, kp2, pairs, mask=None, blocks=0, place=(0, 0, 0, 0), expect=0):
    """straight through the C ABI (include/siftmi.h); place = (kp1, kp2, pairs, mask) on the device?  Returns the 20 doubles
    (filled with FILL before the call) and the kernel time."""
    import torch
    from sift_pyocl_amd import _lib
    M = int(pairs.shape[0])
    keep = []

    def ptr(a, dev):
        a = np.ascontiguousarray(a)
        if dev:
            t = on_device(a); keep.append(t)
            return t.data_ptr()
        keep.append(a)
        return a.ctypes.data
    p1, p2, pp = ptr(kp1, place[0]), ptr(kp2, place[1]), ptr(pairs.astype(np.int32), place[2])
    pm = None if mask is None else ptr(np.asarray(mask).astype(np.uint8), place[3])
    if any(place):
        torch.cuda.synchronize()
    out = np.full(20, FILL, np.float64)
    ms = C.c_double(-1)
    rc = L.siftmi_match_fit(mp._handle, p1, len(kp1), place[0], p2, len(kp2), place[1], pp if M else None, M, place[2],
                            pm, place[3] if mask is not None else 0, blocks, out.ctypes.data, C.byref(ms))
    assert rc == expect, _lib.last_error()
    return out, ms.value


def assert_bits(got, want, what):
    assert fr.same_bits(got, want), "%r\n got  %r\n want %r" % (what, got, want)


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


@pytest.fixture(scope="module")
def case1000():
    return fr.make_case(1000, 4, 0.1, 16384.0)


@pytest.mark.parametrize("M", [0, 1, 2, 3, 18, 255, 256, 257, 1000])
def test_equal_to_restatement_with_the_default_grid(siftlib, mp, M):
    kp1, kp2, pairs, truth = fr.make_case(max(M, 4), 100 + M, 0.1, 16384.0)
    pairs = pairs[:M]
    want = fr.fit(kp1, kp2, pairs)
    assert want[fr.STATUS] == (fr.EMPTY if M == 0 else fr.DEGENERATE if M < 3 else fr.OK) and want[fr.N] == M
    got, ms = abi_fit(siftlib, mp, kp1, kp2, pairs)
    assert_bits(got, want, M)
    assert (ms > 0) == (M > 0)                                                  # no pair: nothing is launched


@pytest.mark.parametrize("M", [65537, 70001])
def test_equal_to_restatement_when_a_lane_owns_more_than_one_pair(siftlib, mp, M):
    """B reaches 256 at 65 536 pairs: one pair wraps round at 65 537, a ragged second row at 70 001"""
    assert fr.default_blocks(M) == 256 and M > 256 * fr.T
    kp1, kp2, pairs, truth = fr.make_case(M, 7, 0.1, 16384.0)
    want = fr.fit(kp1, kp2, pairs)
    assert want[fr.STATUS] == fr.OK
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs)[0], want, M)
    half = np.random.default_rng(M).random(M) < 0.5
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs, mask=half)[0], fr.fit(kp1, kp2, pairs, half), (M, "half"))


@pytest.mark.parametrize("blocks", [1, 2, 3, 7, 1024])
def test_equal_to_restatement_for_a_given_grid(siftlib, mp, case1000, blocks):
    """1000 pairs: blocks = 1 is four pairs per lane (the last row ragged) and a one-element workgroup sum; 2 and 3 give two
    rows, the second ragged; 7 and 1024 (the largest grid) hold every pair in the first four workgroups like the default
    rule and add workgroups without a pair"""
    kp1, kp2, pairs, truth = case1000
    want = fr.fit(kp1, kp2, pairs, blocks=blocks)
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs, blocks=blocks)[0], want, blocks)
    # the order is part of the result: a grid that places the pairs differently gives other bits, workgroups of +0.0 do not
    assert fr.same_bits(want, fr.fit(kp1, kp2, pairs)) == (blocks >= 4)


@pytest.mark.parametrize("place", [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1)])
def test_same_result_wherever_the_inputs_lie(siftlib, mp, case1000, place):
    kp1, kp2, pairs, truth = case1000
    half = np.random.default_rng(3).random(1000) < 0.5
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs, mask=half, place=place)[0], fr.fit(kp1, kp2, pairs, half), place)
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs, place=place)[0], fr.fit(kp1, kp2, pairs), place)


def test_masks(siftlib, mp, case1000):
    kp1, kp2, pairs, truth = case1000
    plain = abi_fit(siftlib, mp, kp1, kp2, pairs)[0]
    assert_bits(plain, fr.fit(kp1, kp2, pairs), "none")
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs, mask=np.ones(1000, np.uint8))[0], plain, "ones")
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs, mask=np.full(1000, 0x80, np.uint8))[0], plain, "non-zero")
    got = abi_fit(siftlib, mp, kp1, kp2, pairs, mask=np.zeros(1000, np.uint8))[0]
    assert got[0] == fr.EMPTY and got[1] == 0 and np.isnan(got[2:]).all()
    assert_bits(got, fr.fit(kp1, kp2, pairs, np.zeros(1000, np.uint8)), "zeros")
    half = np.random.default_rng(8).random(1000) < 0.5
    want = fr.fit(kp1, kp2, pairs, half)
    assert want[fr.N] == half.sum() and want[fr.STATUS] == fr.OK
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs, mask=half)[0], want, "half")
    two = np.zeros(1000, np.uint8); two[[17, 900]] = 1
    got = abi_fit(siftlib, mp, kp1, kp2, pairs, mask=two)[0]
    assert got[0] == fr.DEGENERATE and got[1] == 2 and np.isnan(got[13:]).all() and np.isfinite(got[2:13]).all()
    assert_bits(got, fr.fit(kp1, kp2, pairs, two), "two")
    # the next call on the same matcher is not affected by the status of the last one
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs)[0], plain, "after")


def test_pairs_the_gather_voids_are_skipped(siftlib, mp, case1000):
    kp1, kp2, pairs, truth = case1000
    kp1, kp2, bad = kp1.copy(), kp2.copy(), pairs.copy()
    bad[3, 0] = -1; bad[500, 0] = len(kp1); bad[999, 1] = len(kp2); bad[0, 1] = -1; bad[256, 0] = -2 ** 31
    kp1["x"][pairs[10, 0]] = np.nan; kp1["y"][pairs[11, 0]] = np.inf
    kp2["x"][pairs[12, 1]] = -np.inf; kp2["y"][pairs[700, 1]] = np.nan
    want = fr.fit(kp1, kp2, bad)
    assert want[fr.STATUS] == fr.OK and want[fr.N] == 1000 - 9
    for place in ((0, 0, 0, 0), (1, 1, 1, 0)):
        got = abi_fit(siftlib, mp, kp1, kp2, bad, place=place)[0]
        assert got[1] == 991
        assert_bits(got, want, place)
    # every pair void: EMPTY
    none = np.full((300, 2), -1, np.int32)
    got = abi_fit(siftlib, mp, kp1, kp2, none)[0]
    assert got[0] == fr.EMPTY and got[1] == 0 and np.isnan(got[2:]).all()


def test_degenerate_positions(siftlib, mp):
    kp = np.zeros(500, fr.DTYPE_KP)
    kp["x"] = 3.0 * np.arange(500); kp["y"] = 2.0 * np.arange(500) + 1.0
    idx = np.arange(500, dtype=np.int32)
    pairs = np.stack([idx, idx[::-1]], axis=1)
    want = fr.fit(kp, kp, pairs)
    assert want[fr.STATUS] == fr.DEGENERATE and want[fr.N] == 500
    assert_bits(abi_fit(siftlib, mp, kp, kp, pairs)[0], want, "collinear")
    model, rms, n = mp.fit(kp, kp, pairs)
    assert model is None and np.isnan(rms) and n == 500
    same = np.zeros(40, fr.DTYPE_KP)
    same["x"] = 7.5; same["y"] = 9.25
    pairs = np.stack([idx[:40], idx[:40]], axis=1)
    want = fr.fit(same, same, pairs)
    assert want[fr.STATUS] == fr.DEGENERATE and (want[fr.MOMENTS] == 0).all()    # det = scale = 0: no reading of the rule accepts it (fit_cases.tiny_cluster is where fmax decides)
    assert_bits(abi_fit(siftlib, mp, same, same, pairs)[0], want, "identical")


def test_argument_errors_launch_nothing_and_write_nothing(siftlib, mp, case1000):
    from sift_pyocl_amd import _lib
    kp1, kp2, pairs, truth = case1000
    out = np.full(20, FILL, np.float64)
    ms = C.c_double(-1)

    def call(h=mp._handle, k1=kp1.ctypes.data, n1=len(kp1), k2=kp2.ctypes.data, n2=len(kp2), pp=pairs.ctypes.data, m=1000, blocks=0, o=out.ctypes.data):
        return siftlib.siftmi_match_fit(h, k1, n1, 0, k2, n2, 0, pp, m, 0, None, 0, blocks, o, C.byref(ms))
    for kw in (dict(h=None), dict(o=None), dict(m=-1), dict(n1=-1), dict(n2=-7), dict(m=2 ** 31), dict(n1=2 ** 31), dict(n2=2 ** 40),
               dict(k1=None), dict(k2=None), dict(pp=None), dict(blocks=-1), dict(blocks=1025)):
        assert call(**kw) == _lib.EINVAL, kw
        assert _lib.last_error()
        assert (out == FILL).all() and ms.value == -1, kw                       # nothing was written
    # a valid call after the refused ones is right
    assert_bits(abi_fit(siftlib, mp, kp1, kp2, pairs)[0], fr.fit(kp1, kp2, pairs), "after EINVAL")
    # no pairs: EMPTY, also with null lists of length 0 and null pairs
    assert call(m=0) == _lib.OK and out[0] == fr.EMPTY and out[1] == 0 and np.isnan(out[2:]).all() and ms.value == 0
    out[:] = FILL
    assert call(k1=None, n1=0, k2=None, n2=0, pp=None, m=0) == _lib.OK and out[0] == fr.EMPTY and np.isnan(out[2:]).all()
    with pytest.raises(RuntimeError):
        mp.fit(kp1, kp2, pairs, blocks=2000)
    with pytest.raises(RuntimeError):
        mp.fit(kp1, kp2, pairs.astype(np.int64))
    with pytest.raises(RuntimeError):
        mp.fit(kp1, kp2, pairs, mask=np.ones(999, np.uint8))


def test_python_entry_returns_what_the_abi_returned(siftlib, mp, case1000):
    import torch
    kp1, kp2, pairs, truth = case1000
    half = np.random.default_rng(8).random(1000) < 0.5
    for mask in (None, half, half.view(np.uint8)):
        want = abi_fit(siftlib, mp, kp1, kp2, pairs, mask=mask)[0]
        model, rms, n, raw = mp.fit(kp1, kp2, pairs, mask=mask, return_moments=True)
        assert raw.shape == (20,) and raw.dtype == np.float64
        assert_bits(raw, want, "python")
        assert model.dtype == np.float64 and model.shape == (6,) and np.array_equal(model.view(np.uint64), want[fr.MODEL].view(np.uint64))
        assert n == int(want[fr.N]) and rms == float(np.sqrt(want[fr.SSR] / want[fr.N]))
        assert len(mp.fit(kp1, kp2, pairs, mask=mask)) == 3
    # device tensors, a bool mask tensor among them, and a grid of the caller's
    t1, t2, tp, tm = on_device(kp1), on_device(kp2), torch.from_numpy(pairs).cuda(), torch.from_numpy(half).cuda()
    model, rms, n, raw = mp.fit(t1, t2, tp, mask=tm, blocks=3, return_moments=True)
    assert_bits(raw, fr.fit(kp1, kp2, pairs, half, 3), "tensors")
    # off status 0 there is no model
    model, rms, n = mp.fit(kp1, kp2, pairs, mask=np.zeros(1000, bool))
    assert model is None and np.isnan(rms) and n == 0
    model, rms, n = mp.fit(kp1, kp2, pairs[:0])
    assert model is None and np.isnan(rms) and n == 0
    model, rms, n = mp.fit(kp1, kp2, pairs[:2])
    assert model is None and np.isnan(rms) and n == 2


def test_profile_appends_a_fit_event(siftlib, case1000):
    import sift_pyocl_amd as sp
    kp1, kp2, pairs, truth = case1000
    prof = sp.MatchPlan(profile=True)
    prof.fit(kp1, kp2, pairs)
    assert [label for label, _ in prof.events] == ["fit"]
    assert 0 < prof.events[0][1].profile.end - prof.events[0][1].profile.start < 1e9


# ---------------------------------------------------------------------------------------------- end to end on images
S = 320
MATRIX = np.array([[1.004, -0.006], [0.007, 0.997]])           # (y, x) map of scipy's affine_transform: a known sub-pixel affine map
OFFSET = np.array([2.35, -3.6])


@pytest.fixture(scope="module")
def frames(siftlib):
    """reference frame, the same scene under the affine map (about a thousand matches) and a frame that shares a 40 x 40 patch
    with the reference only (fewer than 18 matches)"""
    import scipy.ndimage as ndi
    import sift_pyocl_amd as sp
    big = smooth_noise((S + 64, S + 64), seed=21, sigma=2.0)
    ref = np.ascontiguousarray(big[32:32 + S, 32:32 + S])
    img = ndi.affine_transform(big.astype(np.float64), MATRIX, offset=OFFSET + 32, output_shape=(S, S), order=3).astype(np.float32)
    few = smooth_noise((S, S), seed=99, sigma=2.0)
    few[100:140, 120:160] = ref[100:140, 120:160]
    return sp.LinearAlign(ref), img, few


def same_arrays(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def pair_rows(matching, keep=None):
    """the matched record pairs as a sorted list of their bytes: keypoints() appends its records in no fixed order, so two calls
    on one frame return the same keypoints and the same matches in another order"""
    m = np.ascontiguousarray(matching)
    assert m.ndim == 2 and m.shape[1] == 2 and m.dtype.itemsize == 144
    rows = m.view(np.uint8).reshape(m.shape[0], 288)
    return sorted(r.tobytes() for r in (rows if keep is None else rows[keep]))


def same_lists(host, dev):
    """the keypoints and the matches of two align() calls on one frame, order aside"""
    assert_same_keypoints(host["keypoint"], dev["keypoint"], "keypoint")
    return pair_rows(host["matching"]) == pair_rows(dev["matching"])


@pytest.mark.parametrize("robust", [False, True])
def test_align_on_the_device_agrees_with_the_host_path(frames, robust):
    la, img, few = frames
    host = la.align(img, return_all=True, robust=robust)
    dev = la.align(img, return_all=True, robust=robust, estimate="device")
    n = int(host["inliers"].sum()) if robust else host["matching"].shape[0]
    assert n >= 200
    # Both paths solve the same centred normal equations in float64 on the same pairs (in whatever order each call's match()
    # appended them) and differ in the order of the sums only, like the restatement under two grids, whose coefficients test_fit_ref_host.py holds within fr.LSTSQ_BOUND of each other
    # (measured there on coordinates up to 16 384; here they stay below 320).  Each float64 coefficient is then rounded to
    # float32, which moves it by at most half a float32 spacing at its magnitude: two values no further apart than the bound
    # round to float32 numbers no further apart than the bound plus one spacing.
    for key in ("matrix", "offset"):
        h, d = host[key], dev[key]
        assert h.dtype == d.dtype == np.float32 and h.shape == d.shape
        tol = fr.LSTSQ_BOUND + np.spacing(np.maximum(np.abs(h), np.abs(d)))
        diff = np.abs(h.astype(np.float64) - d.astype(np.float64))
        print("%s: largest difference %.3e (float32 spacing there %.3e)" % (key, diff.max(), tol.max()))
        assert (diff <= tol).all(), (key, h, d)
    # the map is the one the frame was made with: scipy's (y, x) map sends a pixel of the new frame to the scene, align()
    # reports reference -> new frame, its inverse (up to the interpolation and the keypoints' own precision)
    inv = np.linalg.inv(MATRIX)
    assert np.allclose(dev["matrix"], inv, atol=1e-3) and np.allclose(dev["offset"], -inv @ OFFSET, atol=0.1)
    # the warp of the device path is the warp of its matrix, and equal to the host path's wherever the float32 maps are equal
    assert same_arrays(dev["result"], la.transform(dev["matrix"], dev["offset"], fill=la.sift.minmax()[0]))
    if same_arrays(host["matrix"], dev["matrix"]) and same_arrays(host["offset"], dev["offset"]):
        assert same_arrays(host["result"], dev["result"])
    assert same_lists(host, dev)
    if robust:          # the same matches are kept
        assert dev["inliers"].dtype == np.bool_ and dev["inliers"].shape == (dev["matching"].shape[0],)
        assert pair_rows(host["matching"], host["inliers"]) == pair_rows(dev["matching"], dev["inliers"])
    else:
        assert "inliers" not in dev
    # rms: the float64 model's residual from the device, the float32 matrix's on the host path -- close, not equal
    assert isinstance(dev["rms"], float) and abs(dev["rms"] - float(host["rms"])) < 1e-3 * float(host["rms"]) + 1e-4
    assert same_arrays(la.align(img, estimate="device"), dev["result"])


def test_align_fallbacks_are_the_host_path_bit_for_bit(frames):
    la, img, few = frames
    sparse = la.align(few, return_all=True)
    assert 0 < sparse["matching"].shape[0] < 18
    for frame, kw in ((img, dict(shift_only=True)), (few, dict()), (few, dict(robust=True)), (img, dict(double_check=True)),
                      (img, dict(double_check=True, robust=True))):
        host = la.align(frame, return_all=True, **kw)
        dev = la.align(frame, return_all=True, estimate="device", **kw)
        assert sorted(host) == sorted(dev)
        for key in ("result", "matrix", "offset"):
            assert same_arrays(host[key], dev[key]), (kw, key)
        assert same_lists(host, dev), kw
        if "inliers" in host:
            assert pair_rows(host["matching"], host["inliers"]) == pair_rows(dev["matching"], dev["inliers"]), kw
        # the host path's rms: a float32 mean over the pairs in the order of the call, equal up to that order
        assert type(dev["rms"]) is type(host["rms"]) and abs(float(dev["rms"]) - float(host["rms"])) <= 1e-5 * float(host["rms"]), kw


def test_align_refuses_an_unknown_estimate(frames):
    la, img, few = frames
    with pytest.raises(ValueError):
        la.align(img, estimate="bogus")
    assert same_arrays(la.align(img), la.align(img, estimate="host"))
