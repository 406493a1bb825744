"""GPU tests of the segmented consensus filter (k_consensus_batch.hpp): siftmi_match_consensus_batch
gives for every segment exactly what the restatement gives on that segment alone (tests/consensus_batch_ref.py slices and calls
consensus_ref.consensus) -- every mask byte, winners and votes exactly, models and the two test hooks as bit patterns with NaN as
"is NaN" -- wherever lists, pairs and mask lie, and MatchPlan.consensus_batch gives what the loop of consensus() over the slices of
a match_batch gives."""
import ctypes as C

import numpy as np
import pytest

import consensus_batch_ref as cb
import consensus_cases as cc
import consensus_ref as cr
import estimate_batch_ref as eb
import fit_ref as fr
import shift_ref as sr
from util import smooth_noise, white_noise

pytestmark = pytest.mark.gpu

MASK_FILL = 0xEE
FILL32 = np.float32(-77.0)
INT_FILL = -5
TOL, SEED = 3.0, 3

_REF = {}


def ref(batch, n_hyp, tol=TOL, seed=SEED):
    """the restatement of the batch with separate lists; the shared-list form of a batch must give the very same"""
    key = (batch.name.replace(" [shared]", ""), n_hyp, float(tol), seed)
    if key not in _REF:
        assert "[shared]" not in batch.name
        _REF[key] = cb.consensus_batch(batch, n_hyp, tol, seed)
    return _REF[key]


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Call(object):
    """one call straight through the C ABI (include/siftmi.h); place = (kp1, kp2, pairs, mask) on the device?  A device tensor is
    exactly as large as its data.  Every output is pre-filled with a sentinel."""

    def __init__(self, L, mp, batch, n_hyp, tol=TOL, seed=SEED, place=(0, 0, 0, 0), hooks=True, expect=0):
        import torch
        from sift_pyocl_amd import _lib
        b, hold = batch, []
        S, M = b.S, len(b.pairs)

        def ptr(a, dev):
            a = np.ascontiguousarray(a)
            if a.size == 0:
                return None
            if dev:
                t = on_device(a); hold.append(t)
                return t.data_ptr()
            hold.append(a)
            return a.ctypes.data
        c1 = None if b.counts1 is None else np.ascontiguousarray(b.counts1, np.int64)
        c2, pc = np.ascontiguousarray(b.counts2, np.int64), np.ascontiguousarray(b.pair_counts, np.int64)
        mask = np.full(M, MASK_FILL, np.uint8)
        dmask = on_device(mask) if place[3] and M else None
        self.models = np.full((S, 6), FILL32, np.float32)
        self.winners, self.votes = np.full(S, INT_FILL, np.int32), np.full(S, INT_FILL, np.int32)
        self.votes_all = np.full((S, n_hyp), INT_FILL, np.int32) if hooks else None
        self.models_all = np.full((S, n_hyp, 6), FILL32, np.float32) if hooks else None
        ms = C.c_double(-1)
        if any(place):
            torch.cuda.synchronize()
        rc = L.siftmi_match_consensus_batch(
            mp._handle, ptr(b.kp1, place[0]), len(b.kp1), place[0], ptr(b.kp2, place[1]), len(b.kp2), place[1], S,
            None if c1 is None else c1.ctypes.data, c2.ctypes.data if S else None, ptr(b.pairs, place[2]), M, place[2],
            pc.ctypes.data if S else None, n_hyp, C.c_float(tol), seed,
            (dmask.data_ptr() if dmask is not None else mask.ctypes.data) if M else None, int(dmask is not None),
            self.models.ctypes.data, self.winners.ctypes.data, self.votes.ctypes.data,
            self.votes_all.ctypes.data if hooks else None, self.models_all.ctypes.data if hooks else None, C.byref(ms))
        assert rc == expect, _lib.last_error()
        self.mask = dmask.cpu().numpy() if dmask is not None else mask
        self.ms = ms.value


def assert_equal(got, want, batch, what=""):
    """got: a Call; want: the restatement's dict"""
    name = "%s %s" % (batch.name, what)
    for s in range(batch.S):
        r = batch.rows(s)
        assert np.array_equal(got.mask[r], want["mask"][r]), "%s: mask of segment %d (%d pairs)" % (name, s, batch.pair_counts[s])
    assert got.winners.tolist() == want["winners"].tolist(), name
    assert got.votes.tolist() == want["winner_votes"].tolist(), name
    assert cb.same_bits(got.models, want["models"]), "%s\n got  %r\n want %r" % (name, got.models, want["models"])
    if got.votes_all is not None:
        for s in range(batch.S):
            assert np.array_equal(got.votes_all[s], want["votes_all"][s]), "%s: votes_all of segment %d" % (name, s)
            assert cb.same_bits(got.models_all[s], want["models_all"][s]), "%s: models_all of segment %d" % (name, s)


def check(L, mp, batch, n_hyp, tol=TOL, seed=SEED, place=(0, 0, 0, 0), want=None, hooks=True):
    want = ref(batch, n_hyp, tol, seed) if want is None else want
    got = Call(L, mp, batch, n_hyp, tol, seed, place, hooks)
    assert_equal(got, want, batch, "H %d place %s" % (n_hyp, place))
    assert (got.ms > 0) == bool((batch.pair_counts >= 3).any()), batch.name        # no segment of three pairs: nothing is launched
    return got


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


# ---------------------------------------------------------------------------------------------- 1. the crafted batches
# n_hyp 1; 15: less than the 16 of the smallest chunk; 17: two chunks (9 + 8) below 2048 tiles and one chunk from 2048 tiles on
# (many_batch); 520: above the 512 LDS counters, and with the 70 tiles of large_batch 29 chunks of 18 with a last one of 16; 2048.
# consensus_cases.WIDE_BATCH_CASES: many_batch with 520, 1024 and 1025 hypotheses, chunks of 260, 512 and 342 -- a workgroup's fold
# of its LDS counters takes a second trip
CASES = [(name, H) for name in ("edge", "leak", "tile") for H in (1, 15, 17, 520, 2048)] + [("large", 17), ("large", 520), ("many", 17)]
CASES += [(name, H) for name, H, _ in cc.WIDE_BATCH_CASES]


@pytest.mark.parametrize("form", ["separate", "shared"])
@pytest.mark.parametrize("name,n_hyp", CASES)
def test_crafted_batch_equals_the_restatement(siftlib, mp, name, n_hyp, form):
    batch = getattr(cb, name + "_batch")()
    want = ref(batch, n_hyp)
    got = check(siftlib, mp, batch if form == "separate" else batch.shared(), n_hyp, want=want)
    small = batch.pair_counts < 3
    assert (got.winners[small] == -1).all() and np.isnan(got.models[small]).all() and not got.votes_all[small].any()
    if n_hyp >= 520:
        assert (got.winners[~small] >= 0).all()
    if name == "tile" and n_hyp == 2048:            # the maps of the synthetic segments are found: most inliers vote
        for s, (M, w) in enumerate(cb.TILE_SEGMENTS):
            assert M < 3 or got.votes[s] > 0.9 * w * M, (s, got.votes[s])
    if name == "many":
        assert (-(-batch.pair_counts // 1024)).sum() == 2048 and (~small).sum() == 5


# ---------------------------------------------------------------------------------------------- 2. no read across a segment's bounds
@pytest.mark.parametrize("mask_on_device", [0, 1])
@pytest.mark.parametrize("form", ["separate", "shared"])
def test_leak_batch_in_device_tensors_of_exactly_their_size(siftlib, mp, form, mask_on_device):
    """read across its segment's bounds, an out-of-range row would be finite, could be sampled and could vote: the models of the
    hypotheses, the votes and the mask would all differ from the restatement"""
    batch = cb.leak_batch()
    want = ref(batch, 256, tol=0.5, seed=0)
    got = check(siftlib, mp, batch if form == "separate" else batch.shared(), 256, tol=0.5, seed=0, place=(1, 1, 1, mask_on_device), want=want)
    for s in range(batch.S):
        kp1, kp2, pairs, _ = batch.segment(s)
        inside = (pairs[:, 0] < len(kp1)) & (pairs[:, 1] >= 0)
        assert np.array_equal(got.mask[batch.rows(s)], inside.astype(np.uint8)) and got.votes[s] == eb.LEAK_IN_RANGE
        assert got.models[s].tolist() == cb.leak_model(s).tolist()
        assert 10 <= (~np.isnan(got.models_all[s][:, 0])).sum() <= 22


# ---------------------------------------------------------------------------------------------- 3. residency
@pytest.mark.parametrize("place", [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1)])
def test_same_result_wherever_the_inputs_and_the_mask_lie(siftlib, mp, place):
    for batch in (cb.tile_batch(), cb.tile_batch().shared()):
        check(siftlib, mp, batch, 15, place=place, want=ref(cb.tile_batch(), 15))
    check(siftlib, mp, cb.edge_batch(), 520, place=place, hooks=False)


# ---------------------------------------------------------------------------------------------- 4. nothing stale
def test_a_small_call_after_a_large_one_and_the_same_call_twice(siftlib):
    """the positions, models, votes and flags of 70 001 pairs x 520 hypotheses and a table of 70 tiles lie behind the next,
    smaller calls; the single call shares the buffers and works before and after"""
    import sift_pyocl_amd as sp
    own = sp.MatchPlan()
    check(siftlib, own, cb.large_batch(), 520)
    for _ in range(2):
        check(siftlib, own, cb.leak_batch(), 256, tol=0.5, seed=0)
    check(siftlib, own, cb.edge_batch(), 2048)
    kp1, kp2, pairs, _ = cb.tile_batch().segment(0)
    single = cr.consensus(kp1, kp2, pairs, 64, TOL, SEED)
    mask, model, votes = own.consensus(kp1, kp2, pairs, n_hyp=64, tol=TOL, seed=SEED)
    assert np.array_equal(mask.view(np.uint8), single["mask"]) and votes == single["winner_votes"]
    check(siftlib, own, cb.tile_batch(), 15)
    check(siftlib, own, cb.edge_batch(), 17)
    check(siftlib, own, cb.edge_batch(), 17)


# ---------------------------------------------------------------------------------------------- 5. nothing to do, nothing to win
def test_no_segment_and_no_active_segment_launch_nothing(siftlib, mp):
    none = eb.from_segments("none", [])
    got = Call(siftlib, mp, none, 16)
    assert got.ms == 0 and got.models.shape == (0, 6)
    tiny = eb.from_segments("tiny", [eb.case_segment(M, 95 + M) for M in (2, 0, 1, 2)])
    for batch in (tiny, tiny.shared()):
        for place in ((0, 0, 0, 0), (0, 0, 0, 1), (1, 1, 1, 1)):
            got = Call(siftlib, mp, batch, 16, place=place)
            assert got.ms == 0 and not got.mask.any() and len(got.mask) == 5
            assert got.winners.tolist() == [-1] * 4 and got.votes.tolist() == [0] * 4 and np.isnan(got.models).all()
            assert not got.votes_all.any() and np.isnan(got.models_all).all()
    kp = np.zeros(0, cr.DTYPE_KP)
    mask, models, votes = mp.consensus_batch(kp, None, kp, [], np.zeros((0, 2), np.int32), [])
    assert mask.shape == (0,) and models.shape == (0, 6) and votes.shape == (0,)
    mask, models, votes = mp.consensus_batch(tiny.kp1, tiny.counts1, tiny.kp2, tiny.counts2, tiny.pairs, tiny.pair_counts, out="device")
    assert mask.is_cuda and not mask.cpu().numpy().any() and np.isnan(models).all() and votes.tolist() == [0] * 4


def test_three_collinear_pairs_have_no_winner(siftlib, mp):
    """every triple of the middle segment is void (a repeated index or a zero determinant): launched, but nothing wins"""
    kp1, kp2 = np.zeros(3, cr.DTYPE_KP), np.zeros(3, cr.DTYPE_KP)
    kp1["x"] = [0, 10, 20]; kp1["y"] = [0, 10, 20]; kp2["x"] = [1, 11, 21]; kp2["y"] = [2, 12, 22]
    idx = np.arange(3, dtype=np.int32)
    batch = eb.from_segments("collinear", [eb.case_segment(40, 55), (kp1, kp2, np.stack([idx, idx], axis=1)), eb.case_segment(18, 84)])
    for place in ((0, 0, 0, 0), (1, 1, 1, 1)):
        got = check(siftlib, mp, batch, 64, place=place)
        assert got.winners[1] == -1 and got.votes[1] == 0 and np.isnan(got.models[1]).all() and not got.mask[batch.rows(1)].any()
        assert np.isnan(got.models_all[1]).all() and not got.votes_all[1].any() and got.winners[0] >= 0 and got.winners[2] >= 0
    alone = eb.from_segments("collinear alone", [(kp1, kp2, np.stack([idx, idx], axis=1))])
    got = check(siftlib, mp, alone, 64)
    assert got.ms > 0 and got.winners.tolist() == [-1] and not got.mask.any()


# ---------------------------------------------------------------------------------------------- 6. errors
def test_argument_errors_launch_nothing_and_write_nothing(siftlib, mp):
    from sift_pyocl_amd import _lib
    b = cb.leak_batch()
    S, M, H = b.S, len(b.pairs), 32
    mask = np.full(M, MASK_FILL, np.uint8)
    models = np.full((S, 6), FILL32, np.float32)
    winners, votes = np.full(S, INT_FILL, np.int32), np.full(S, INT_FILL, np.int32)
    votes_all, models_all = np.full((S, H), INT_FILL, np.int32), np.full((S, H, 6), FILL32, np.float32)
    ms = C.c_double(-1)
    c1, c2, pc = b.counts1.copy(), b.counts2.copy(), b.pair_counts.copy()
    hold = []

    def bad(a, k, v):
        a = a.copy(); a[k] = v
        return a

    def call(h=mp._handle, k1=b.kp1.ctypes.data, n1=len(b.kp1), k2=b.kp2.ctypes.data, n2=len(b.kp2), S=S, c1=c1, c2=c2,
             pp=b.pairs.ctypes.data, m=M, pc=pc, n_hyp=H, tol=1.0, mk=mask.ctypes.data, mo=models.ctypes.data, w=winners.ctypes.data,
             v=votes.ctypes.data):
        hold[:] = [None if a is None else np.ascontiguousarray(a, np.int64) for a in (c1, c2, pc)]
        p1, p2, p3 = (None if a is None else a.ctypes.data for a in hold)
        return siftlib.siftmi_match_consensus_batch(h, k1, n1, 0, k2, n2, 0, S, p1, p2, pp, m, 0, p3, n_hyp, C.c_float(tol), 1, mk, 0, mo, w, v,
                                                    votes_all.ctypes.data, models_all.ctypes.data, C.byref(ms))

    errors = [dict(h=None), dict(S=65536), dict(S=-1), dict(c2=bad(c2, 1, -1)), dict(c1=bad(c1, 0, -3)), dict(pc=bad(pc, 2, -1)),
              dict(n2=len(b.kp2) - 1), dict(n1=len(b.kp1) + 1), dict(c2=bad(c2, 0, c2[0] + 1)), dict(c1=bad(c1, 4, c1[4] - 1)),
              dict(m=M - 1), dict(pc=bad(pc, 0, pc[0] + 1)), dict(m=2 ** 31), dict(n1=-1), dict(n2=2 ** 40),
              dict(k1=None), dict(k2=None), dict(pp=None), dict(c2=None), dict(pc=None),
              dict(n_hyp=0), dict(n_hyp=-1), dict(n_hyp=2 ** 20 + 1),
              dict(tol=0.0), dict(tol=-1.0), dict(tol=float("nan")), dict(tol=float("inf")),
              dict(mk=None), dict(mo=None), dict(w=None), dict(v=None),
              dict(n_hyp=2 ** 20),                                                        # 5 segments x 2^20 hypotheses > 2^22
              # one segment of 2^30 + 1 rows is 2^20 + 1 tiles; nothing is read before the refusal
              dict(S=1, c1=None, c2=[len(b.kp2)], m=2 ** 30 + 1, pc=[2 ** 30 + 1])]
    for kw in errors:
        assert call(**kw) == _lib.EINVAL, kw
        assert _lib.last_error()
        assert (mask == MASK_FILL).all() and (models == FILL32).all() and (winners == INT_FILL).all() and (votes == INT_FILL).all(), kw
        assert (votes_all == INT_FILL).all() and (models_all == FILL32).all() and ms.value == -1, kw
    # a valid call after the refused ones is right
    assert call(tol=0.5) == _lib.OK
    want = ref(b, H, tol=0.5, seed=1)
    assert np.array_equal(mask, want["mask"]) and cb.same_bits(models, want["models"]) and np.array_equal(votes_all, want["votes_all"])


# ---------------------------------------------------------------------------------------------- 7. the method
def loop_of_consensus(mp, b, n_hyp, tol, seed):
    out = []
    for s in range(b.S):
        kp1, kp2, pairs, _ = b.segment(s)
        out.append(mp.consensus(kp1, kp2, pairs, n_hyp=n_hyp, tol=tol, seed=seed, return_votes=True))
    return out


def test_python_method_on_host_arrays_and_tensors(siftlib, mp):
    import torch
    b = cb.tile_batch()
    H = 100
    loop = loop_of_consensus(mp, b, H, 2.5, 11)
    host = (b.kp1, b.counts1, b.kp2, b.counts2, b.pairs, b.pair_counts)
    dev = (on_device(b.kp1), b.counts1, on_device(b.kp2), list(b.counts2), torch.from_numpy(b.pairs).cuda(), tuple(b.pair_counts))
    sh = b.shared()
    shared = (on_device(sh.kp1), None, sh.kp2, sh.counts2, torch.from_numpy(sh.pairs).cuda(), sh.pair_counts)
    for args in (host, dev, shared):
        for out in ("host", "device"):
            mask, models, votes, (winners, votes_all, models_all) = mp.consensus_batch(*args, n_hyp=H, tol=2.5, seed=11, return_votes=True,
                                                                                      out=out)
            if out == "device":
                assert isinstance(mask, torch.Tensor) and mask.dtype == torch.uint8 and mask.is_cuda and mask.shape == (len(b.pairs),)
                mask = mask.cpu().numpy().view(np.bool_)
            assert mask.dtype == np.bool_ and models.dtype == np.float32 and models.shape == (b.S, 6)
            assert votes.dtype == winners.dtype == votes_all.dtype == np.int32 and votes_all.shape == (b.S, H) and models_all.shape == (b.S, H, 6)
            for s in range(b.S):
                m_s, model_s, v_s, (va_s, ma_s) = loop[s]
                assert np.array_equal(mask[b.rows(s)], m_s) and votes[s] == v_s and (winners[s] >= 0) == (model_s is not None)
                assert np.isnan(models[s]).all() if model_s is None else cb.same_bits(models[s], model_s)
                assert np.array_equal(votes_all[s], va_s) and cb.same_bits(models_all[s], ma_s)
                if model_s is not None:
                    assert cb.same_bits(models_all[s, winners[s]], model_s) and votes_all[s, winners[s]] == v_s
    assert len(mp.consensus_batch(*host, n_hyp=H)) == 3
    # the defaults are consensus()'s
    mask, models, votes = mp.consensus_batch(*host)
    m0, model0, v0 = mp.consensus(*b.segment(0)[:3])
    assert np.array_equal(mask[b.rows(0)], m0) and cb.same_bits(models[0], model0) and votes[0] == v0


def test_profile_appends_the_event(siftlib):
    import sift_pyocl_amd as sp
    b = cb.leak_batch()
    prof = sp.MatchPlan(profile=True)
    prof.consensus_batch(b.kp1, b.counts1, b.kp2, b.counts2, b.pairs, b.pair_counts, n_hyp=64)
    assert [label for label, _ in prof.events] == ["consensus_batch"]
    assert 0 < prof.events[0][1].profile.end - prof.events[0][1].profile.start < 1e9


def test_python_method_refuses_what_the_entry_refuses(siftlib, mp):
    b = cb.leak_batch()
    args = (b.kp1, b.counts1, b.kp2, b.counts2, b.pairs, b.pair_counts)
    for kw in (dict(out="pinned"), dict(out=None), dict(n_hyp=0), dict(n_hyp=2 ** 20 + 1), dict(tol=0.0), dict(tol=-3.0),
               dict(tol=float("nan")), dict(tol=float("inf")), dict(tol=1e39), dict(n_hyp=2 ** 20)):
        with pytest.raises(ValueError):
            mp.consensus_batch(*args, **kw)

    def with_(k, v):
        a = list(args); a[k] = v
        return a
    for a in (with_(5, b.pair_counts[:-1]), with_(3, b.counts2 + 1), with_(1, b.counts1[:-1]), with_(4, b.pairs[:-1])):
        with pytest.raises(ValueError):
            mp.consensus_batch(*a)
    with pytest.raises(RuntimeError):
        mp.consensus_batch(*with_(4, b.pairs.astype(np.int64)))
    # one segment of 2^30 + 1 rows would be 2^20 + 1 tiles: refused from the counts alone
    with pytest.raises(ValueError):
        mp.consensus_batch(b.kp1, None, b.kp2, [len(b.kp2)], b.pairs, [2 ** 30 + 1])


# ---------------------------------------------------------------------------------------------- 8. the chain of a stack
def test_chain_on_real_keypoints_against_the_loop(mp):
    """three 256 x 256 frames through BatchPlan.keypoints_batch_device -> match_batch(out="device") -> consensus_batch(out="device")
    -> fit_batch(mask=that tensor) and shift_batch(mask=...): every segment's results are consensus() -> fit(mask=) / shift(mask=)
    on the slices, bit for bit, and the mask never visits the host.  The only comparison with package code instead of the
    restatement."""
    import torch
    import sift_pyocl_amd as sp
    shape = (256, 256)
    base = smooth_noise(shape, seed=71, sigma=1.5)
    frames = [base, np.roll(base, (3, -2), axis=(0, 1)) + 0.02 * white_noise(shape, seed=72), smooth_noise(shape, seed=73, sigma=1.5)]
    bp = sp.BatchPlan(shape=shape, dtype=np.float32, lanes=2)
    counts, records = bp.keypoints_batch_device([torch.from_numpy(f.astype(np.float32)).cuda() for f in frames])
    assert min(counts) > 20
    ref_list = records[:counts[0] * 144]
    off = np.concatenate([[0], np.cumsum(counts)])
    pairs, pair_counts = mp.match_batch(ref_list, None, records, counts, out="device")
    assert pair_counts[0] > 18 and pair_counts[1] > 18
    rows = np.concatenate([[0], np.cumsum(pair_counts)])
    head = (ref_list, None, records, counts, pairs, pair_counts)
    mask, models, votes = mp.consensus_batch(*head, n_hyp=512, tol=1.5, seed=4, out="device")
    assert isinstance(mask, torch.Tensor) and mask.is_cuda
    fits, rms, n, raw = mp.fit_batch(*head, mask=mask, return_moments=True)
    shifts, ns, ranks = mp.shift_batch(*head, mask=mask, return_ranks=True)
    host_mask = mask.cpu().numpy()
    for s in range(3):
        seg, ps = records[off[s] * 144:off[s + 1] * 144], pairs[rows[s]:rows[s + 1]]
        mask_s, model_s, votes_s = mp.consensus(ref_list, seg, ps, n_hyp=512, tol=1.5, seed=4)
        assert np.array_equal(host_mask[rows[s]:rows[s + 1]], mask_s.view(np.uint8)) and votes[s] == votes_s
        assert np.isnan(models[s]).all() if model_s is None else cb.same_bits(models[s], model_s)
        fit_s, rms_s, n_s, raw_s = mp.fit(ref_list, seg, ps, mask=mask_s, return_moments=True)
        assert fr.same_bits(raw[s], raw_s) and n[s] == n_s == mask_s.sum(), (s, raw[s], raw_s)
        moved, m_s, ranks_s = mp.shift(ref_list, seg, ps, mask=mask_s, return_ranks=True)
        assert sr.same_bits(ranks[s], ranks_s) and ns[s] == m_s
    # frame 0 against itself: the identity wins; frame 1 is frame 0 moved by (-2, 3)
    assert votes[0] >= 0.9 * pair_counts[0] and models[0].tolist() == [1, 0, 0, 0, 1, 0] and shifts[0].tolist() == [0.0, 0.0]
    assert votes[1] > 0.5 * pair_counts[1] and abs(shifts[1, 0] + 2) < 0.25 and abs(shifts[1, 1] - 3) < 0.25
