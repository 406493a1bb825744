"""GPU tests of the consensus filter: siftmi_match_consensus / MatchPlan.consensus give exactly what
the numpy restatement of the contract gives (tests/consensus_ref.py) -- every vote count, every model bit, the winner, the
mask -- wherever the lists and the pairs lie, and LinearAlign.align(robust=True) uses it end to end."""
import ctypes as C

import numpy as np
import pytest

import consensus_ref as cr
from util import smooth_noise

pytestmark = pytest.mark.gpu


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def abi_consensus(L, mp, kp1, kp2, pairs, n_hyp, tol, seed, place=(0, 0, 0)):
    """straight through the C ABI (include/siftmi.h); place = (kp1, kp2, pairs) on the device?"""
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
    if any(place):
        torch.cuda.synchronize()
    mask = np.full(M, 0xA5, np.uint8); model = np.full(6, -77.0, np.float32)
    votes_all = np.full(n_hyp, -1, np.int32); models_all = np.zeros((n_hyp, 6), np.float32)
    winner, wvotes, ms = C.c_int32(-5), C.c_int32(-5), C.c_double(-1)
    rc = L.siftmi_match_consensus(mp._handle, p1, len(kp1), place[0], p2, len(kp2), place[1], pp, M, place[2], n_hyp, C.c_float(tol),
                                  seed, mask.ctypes.data, model.ctypes.data, C.byref(winner), C.byref(wvotes),
                                  votes_all.ctypes.data, models_all.ctypes.data, C.byref(ms))
    assert rc == _lib.OK, _lib.last_error()
    return dict(mask=mask, model=model, winner=winner.value, winner_votes=wvotes.value, votes_all=votes_all, models_all=models_all,
                kernel_ms=ms.value)


def assert_equal_to_restatement(got, want, what):
    assert np.array_equal(got["votes_all"], want["votes_all"]), what
    assert np.array_equal(got["models_all"].view(np.uint32), want["models_all"].view(np.uint32)), what
    assert np.array_equal(np.isnan(got["models_all"]).all(axis=1), ~want["valid"]), what
    assert got["winner"] == want["winner"] and got["winner_votes"] == want["winner_votes"], what
    assert np.array_equal(got["mask"], want["mask"]), what
    if want["winner"] >= 0:
        assert np.array_equal(got["model"].view(np.uint32), want["model"].view(np.uint32)), what
    else:
        assert (got["model"] == -77.0).all(), what          # untouched


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


@pytest.mark.parametrize("M,w,seed", cr.SETS)
def test_equal_to_restatement_on_the_synthetic_sets(siftlib, mp, M, w, seed):
    kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(M, w, seed)
    cases = [(2048, 3.0, 0)] + ([(5000, 0.5, 12345), (7, 3.0, 0xFFFFFFF0)] if M <= 5000 else [])
    wants = []
    for n_hyp, tol, s in cases:
        wants.append(cr.consensus(kp1, kp2, pairs, n_hyp, tol, s))
        got = abi_consensus(siftlib, mp, kp1, kp2, pairs, n_hyp, tol, s)
        assert_equal_to_restatement(got, wants[-1], (M, w, seed, n_hyp, tol, s))
        assert got["kernel_ms"] > 0
    # the Python entry point hands the same results on
    mask, model, votes, (votes_all, models_all) = mp.consensus(kp1, kp2, pairs, n_hyp=2048, tol=3.0, seed=0, return_votes=True)
    want = wants[0]
    assert mask.dtype == np.bool_ and np.array_equal(mask, want["mask"].astype(bool)) and votes == want["winner_votes"]
    assert np.array_equal(model.view(np.uint32), want["model"].view(np.uint32)) and np.array_equal(votes_all, want["votes_all"])
    assert len(mp.consensus(kp1, kp2, pairs)) == 3


@pytest.mark.parametrize("M", [3, 63, 64, 65, 257])
def test_equal_to_restatement_at_wave_and_tile_edges(siftlib, mp, M):
    for seed in (0, 0x9E3779B9):
        kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(M, 0.7, 1000 + M, frame=(640, 480))
        for n_hyp in (1, 7, 2048, 5000):
            for tol in (0.5, 3.0):
                want = cr.consensus(kp1, kp2, pairs, n_hyp, tol, seed)
                got = abi_consensus(siftlib, mp, kp1, kp2, pairs, n_hyp, tol, seed)
                assert_equal_to_restatement(got, want, (M, n_hyp, tol, seed))


def test_more_matches_than_one_tile_row_and_a_partial_last_tile(siftlib, mp):
    """1024 matches are a workgroup's tile: one below, exactly, one above, and a hypothesis count that is no multiple of a chunk"""
    for M in (1023, 1024, 1025, 4099):
        kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(M, 0.6, 2000 + M)
        for n_hyp in (513, 1031):
            want = cr.consensus(kp1, kp2, pairs, n_hyp, 3.0, 4)
            assert_equal_to_restatement(abi_consensus(siftlib, mp, kp1, kp2, pairs, n_hyp, 3.0, 4), want, (M, n_hyp))


def test_same_result_wherever_the_inputs_lie_and_bad_pairs_never_vote(siftlib, mp):
    kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(5000, 0.5, 31)
    bad = pairs.copy()
    bad[5, 0] = len(kp1); bad[17, 1] = -1; bad[4040, 1] = len(kp2) + 1000; bad[4999, 0] = -2 ** 31
    for prs in (pairs, bad):
        want = cr.consensus(kp1, kp2, prs, 2048, 3.0, 3)
        outs = [abi_consensus(siftlib, mp, kp1, kp2, prs, 2048, 3.0, 3, place) for place in ((0, 0, 0), (1, 1, 0), (1, 1, 1), (0, 1, 1))]
        for got in outs:
            assert_equal_to_restatement(got, want, "placement")
    assert not outs[0]["mask"][[5, 17, 4040, 4999]].any()
    # device tensors through the Python entry point
    import torch
    t1, t2 = on_device(kp1), on_device(kp2)
    tp = torch.from_numpy(bad).cuda()
    mask, model, votes = mp.consensus(t1, t2, tp, n_hyp=2048, tol=3.0, seed=3)
    assert np.array_equal(mask, want["mask"].astype(bool)) and votes == want["winner_votes"]


def test_argument_errors_launch_nothing_and_empty_input_is_ok(siftlib, mp):
    from sift_pyocl_amd import _lib
    kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(300, 0.8, 9)
    M = len(pairs)
    mask = np.full(M, 0xA5, np.uint8); model = np.full(6, -77.0, np.float32)
    winner, wvotes = C.c_int32(-5), C.c_int32(-5)

    def call(k1=kp1.ctypes.data, n1=len(kp1), k2=kp2.ctypes.data, n2=len(kp2), pp=pairs.ctypes.data, m=M, n_hyp=64, tol=3.0, out=mask.ctypes.data):
        return siftlib.siftmi_match_consensus(mp._handle, k1, n1, 0, k2, n2, 0, pp, m, 0, n_hyp, C.c_float(tol), 1, out, model.ctypes.data,
                                              C.byref(winner), C.byref(wvotes), None, None, None)
    for kw in (dict(n_hyp=0), dict(n_hyp=-3), dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")),
               dict(m=-1), dict(n1=-1), dict(n2=-7), dict(k1=None), dict(k2=None), dict(pp=None), dict(out=None)):
        assert call(**kw) == _lib.EINVAL, kw
        assert _lib.last_error()
        assert (mask == 0xA5).all() and (model == -77.0).all(), kw            # nothing was written
    # a valid call after the refused ones is right
    assert_equal_to_restatement(abi_consensus(siftlib, mp, kp1, kp2, pairs, 64, 3.0, 1), cr.consensus(kp1, kp2, pairs, 64, 3.0, 1), "after EINVAL")
    # no pairs: OK, no winner; also with null lists of length 0
    assert call(m=0) == _lib.OK and winner.value == -1 and wvotes.value == 0
    winner.value = 9
    assert call(k1=None, n1=0, k2=None, n2=0, pp=None, m=0, out=None) == _lib.OK and winner.value == -1
    for m in (1, 2):                              # fewer than three pairs: mask cleared, no winner
        mask[:] = 0xA5
        assert call(m=m) == _lib.OK and winner.value == -1 and not mask[:m].any() and (mask[m:] == 0xA5).all()
    mk, model_none, votes = mp.consensus(kp1, kp2, pairs[:0])
    assert mk.shape == (0,) and model_none is None and votes == 0
    with pytest.raises(RuntimeError):
        mp.consensus(kp1, kp2, pairs, n_hyp=0)
    with pytest.raises(RuntimeError):
        mp.consensus(kp1, kp2, pairs.astype(np.int64))


def test_collinear_matches_have_no_winner_on_the_device(siftlib, mp):
    kp = np.zeros(500, cr.DTYPE_KP)
    kp["x"] = 3.0 * np.arange(500); kp["y"] = 2.0 * np.arange(500) + 1.0
    idx = np.arange(500, dtype=np.int32)
    pairs = np.stack([idx, idx[::-1]], axis=1)
    want = cr.consensus(kp, kp, pairs, 300, 3.0, 0)
    assert want["winner"] == -1
    assert_equal_to_restatement(abi_consensus(siftlib, mp, kp, kp, pairs, 300, 3.0, 0), want, "collinear")
    mask, model, votes = mp.consensus(kp, kp, pairs, n_hyp=300)
    assert model is None and votes == 0 and not mask.any()


def test_profile_appends_a_consensus_event(siftlib):
    import sift_pyocl_amd as sp
    kp1, kp2, pairs, inlier, truth = cr.synthetic_matches(5000, 0.5, 31)
    prof = sp.MatchPlan(profile=True)
    prof.consensus(kp1, kp2, pairs)
    assert [label for label, _ in prof.events] == ["consensus"]
    assert 0 < prof.events[0][1].profile.end - prof.events[0][1].profile.start < 1e9


# ---------------------------------------------------------------------------------------------- end to end on images
S = 768
MAJOR, MINOR = (-7, 11), (9, -14)              # (dy, dx) that align() should report for the two motions: reference corner - frame corner
BAND = (60, 360)                               # rows of frame B that carry the minority motion: 300 of 768 rows, 39 % of the area


def _frames():
    big = smooth_noise((S + 128, S + 128), seed=12, sigma=2.0)
    def cut(shift):
        return np.ascontiguousarray(big[64 - shift[0]:64 - shift[0] + S, 64 - shift[1]:64 - shift[1] + S])
    a, clean, other = cut((0, 0)), cut(MAJOR), cut(MINOR)
    mixed = clean.copy()
    mixed[BAND[0]:BAND[1]] = other[BAND[0]:BAND[1]]
    return a, clean, mixed


def _offset_error(res, shift=MAJOR):
    """distance between the map align() found and the pure shift, at the frame's centre (where the offset of an affine map
    with a matrix close to the identity is least sensitive to the matrix), pixels"""
    c = np.array([S / 2.0, S / 2.0])
    moved = res["matrix"].astype(np.float64) @ c + res["offset"].astype(np.float64)
    return float(np.hypot(*(moved - (c + np.array(shift, np.float64)))))


def test_align_robust_end_to_end(siftlib):
    import sift_pyocl_amd as sp
    a, clean, mixed = _frames()
    la = sp.LinearAlign(a)
    e_clean = _offset_error(la.align(clean, return_all=True))
    plain = la.align(mixed, return_all=True)
    e_plain = _offset_error(plain)
    res = la.align(mixed, robust=True, return_all=True)
    e_robust = _offset_error(res)
    inl = res["inliers"]
    print("offset error at the frame centre: clean pair %.4f px, contaminated pair %.4f px, contaminated pair with robust=True %.4f px "
          "(%d of %d matches kept)" % (e_clean, e_plain, e_robust, inl.sum(), inl.size))
    assert "inliers" not in plain
    assert inl.dtype == np.bool_ and inl.shape == (res["matching"].shape[0],) and 18 <= inl.sum() < inl.size
    # the same consensus by hand: the pairs align() used, recovered from the records it returned (equal records have equal positions)
    ref_index = {r.tobytes(): i for i, r in enumerate(la.ref_kp)}
    kp_index = {r.tobytes(): i for i, r in enumerate(res["keypoint"])}
    pairs = np.array([[ref_index[m0.tobytes()], kp_index[m1.tobytes()]] for m0, m1 in zip(res["matching"][:, 0], res["matching"][:, 1])], np.int32)
    mask, model, votes = sp.MatchPlan().consensus(np.ascontiguousarray(la.ref_kp), np.ascontiguousarray(res["keypoint"]), pairs,
                                                  n_hyp=2048, tol=3.0, seed=0)
    assert np.array_equal(mask, inl) and votes == inl.sum()
    want = cr.consensus(np.ascontiguousarray(la.ref_kp), np.ascontiguousarray(res["keypoint"]), pairs, 2048, 3.0, 0)
    assert np.array_equal(want["mask"].astype(bool), inl)
    # voters lie outside the band that moved differently
    y_new = res["matching"][:, 1].y
    in_band = (y_new > BAND[0] + 8) & (y_new < BAND[1] - 8)
    assert not (inl & in_band).any()
    assert e_robust <= e_clean + 0.05
    assert e_plain > 1.0


def test_align_default_keywords_are_unchanged(siftlib):
    import sift_pyocl_amd as sp
    a, clean, mixed = _frames()
    la = sp.LinearAlign(a)
    for kw in (dict(), dict(shift_only=True)):
        r0 = la.align(mixed, **kw)
        r1 = la.align(mixed, robust=False, **kw)
        assert r0.dtype == r1.dtype and np.array_equal(r0.view(np.uint8), r1.view(np.uint8))
        d = la.align(mixed, return_all=True, **kw)
        assert "inliers" not in d and np.array_equal(d["result"].view(np.uint8), r0.view(np.uint8))
    d = la.align(mixed, robust=True, robust_tol=2.0, robust_hyp=512, return_all=True)
    assert "inliers" in d and d["inliers"].sum() >= 18
