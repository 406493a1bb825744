"""GPU tests of the segmented fit and median (k_estimate_batch.hpp): siftmi_match_fit_batch /
siftmi_match_shift_batch give for every segment exactly what the restatement gives on that segment alone
(tests/estimate_batch_ref.py slices and calls fit_ref / shift_ref) -- 20 doubles and 6 floats per segment as bit patterns, NaN as
"is NaN", counts and keep bytes exactly -- wherever lists, pairs and mask lie, and MatchPlan.fit_batch / shift_batch give what the
loop of fit() / shift() over the slices of a match_batch gives."""
import ctypes as C

import numpy as np
import pytest

import estimate_batch_ref as eb
import fit_ref as fr
import shift_ref as sr
from util import smooth_noise, white_noise

pytestmark = pytest.mark.gpu

FILL64 = np.float64(-77.0)
FILL32 = np.float32(-77.0)
COUNT_FILL = -5
KEEP_FILL = 0xEE

_REF = {}


def ref_fit(batch, blocks=0):
    key = ("fit", batch.name, blocks)
    if key not in _REF:
        _REF[key] = eb.fit_batch(batch, blocks)
    return _REF[key]


def ref_shift(batch, tol=None):
    key = ("shift", batch.name, None if tol is None else float(tol))
    if key not in _REF:
        _REF[key] = eb.shift_batch(batch, tol)
    return _REF[key]


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


class Args(object):
    """the arguments both entries share, straight for the C ABI (include/siftmi.h); place = (kp1, kp2, pairs, mask) on the device?
    A device tensor is exactly as large as its data."""

    def __init__(self, mp, batch, place=(0, 0, 0, 0)):
        import torch
        self.hold = []
        b = batch

        def ptr(a, dev):
            a = np.ascontiguousarray(a)
            if a.size == 0:
                return None
            if dev:
                t = on_device(a); self.hold.append(t)
                return t.data_ptr()
            self.hold.append(a)
            return a.ctypes.data
        self.c1 = None if b.counts1 is None else np.ascontiguousarray(b.counts1, np.int64)
        self.c2 = np.ascontiguousarray(b.counts2, np.int64)
        self.pc = np.ascontiguousarray(b.pair_counts, np.int64)
        self.head = [mp._handle, ptr(b.kp1, place[0]), len(b.kp1), place[0], ptr(b.kp2, place[1]), len(b.kp2), place[1], b.S,
                     None if self.c1 is None else self.c1.ctypes.data, self.c2.ctypes.data if b.S else None,
                     ptr(b.pairs, place[2]), len(b.pairs), place[2], self.pc.ctypes.data if b.S else None,
                     None if b.mask is None else ptr(b.mask, place[3]), place[3] if b.mask is not None else 0]
        if any(place):
            torch.cuda.synchronize()


def abi_fit(L, mp, batch, blocks=0, place=(0, 0, 0, 0), expect=0):
    """returns out (S, 20), pre-filled with a sentinel, and the kernel time"""
    from sift_pyocl_amd import _lib
    a = Args(mp, batch, place)
    out = np.full((batch.S, 20), FILL64, np.float64)
    ms = C.c_double(-1)
    rc = L.siftmi_match_fit_batch(*a.head, blocks, out.ctypes.data, C.byref(ms))
    assert rc == expect, _lib.last_error()
    return out, ms.value


def abi_shift(L, mp, batch, tol=None, place=(0, 0, 0, 0), expect=0):
    """returns out (S, 6), counts (S, 2), keep (M,) uint8 or None -- all pre-filled with sentinels -- and the kernel time"""
    from sift_pyocl_amd import _lib
    a = Args(mp, batch, place)
    out = np.full((batch.S, 6), FILL32, np.float32)
    counts = np.full((batch.S, 2), COUNT_FILL, np.int64)
    keep = None if tol is None else np.full(len(batch.pairs), KEEP_FILL, np.uint8)
    ms = C.c_double(-1)
    rc = L.siftmi_match_shift_batch(*a.head, C.c_float(0.0 if tol is None else tol), None if tol is None else keep.ctypes.data,
                                    out.ctypes.data, counts.ctypes.data, C.byref(ms))
    assert rc == expect, _lib.last_error()
    return out, counts, keep, ms.value


def check_fit(L, mp, batch, blocks=0, place=(0, 0, 0, 0), want=None):
    want = ref_fit(batch, blocks) if want is None else want
    out, ms = abi_fit(L, mp, batch, blocks, place)
    for s in range(batch.S):
        assert fr.same_bits(out[s], want[s]), "%s: fit of segment %d (%d pairs), blocks %d\n got  %r\n want %r" % (
            batch.name, s, batch.pair_counts[s], blocks, out[s], want[s])
    assert (ms > 0) == (len(batch.pairs) > 0), batch.name                       # no pair: nothing is launched
    return want


def check_shift(L, mp, batch, tol=None, place=(0, 0, 0, 0), want=None):
    want, wcounts, wkeep = ref_shift(batch, tol) if want is None else want
    out, counts, keep, ms = abi_shift(L, mp, batch, tol, place)
    for s in range(batch.S):
        assert sr.same_bits(out[s], want[s]), "%s: shift of segment %d (%d pairs)\n got  %r\n want %r" % (
            batch.name, s, batch.pair_counts[s], out[s], want[s])
    if tol is None:
        wcounts = wcounts.copy(); wcounts[:, 1] = 0
    assert counts.tolist() == wcounts.tolist(), (batch.name, counts, wcounts)
    if tol is not None:
        assert np.array_equal(keep, wkeep.astype(np.uint8)), batch.name
    assert (ms > 0) == (len(batch.pairs) > 0), batch.name
    return want, wcounts, wkeep


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


# ---------------------------------------------------------------------------------------------- 1. the crafted batches
@pytest.mark.parametrize("form", ["separate", "shared"])
@pytest.mark.parametrize("name", ["edge", "large", "leak", "degenerate", "masked", "value"])
def test_crafted_batch_equals_the_restatement(siftlib, mp, name, form):
    batch = getattr(eb, name + "_batch")()
    if form == "shared":
        batch = batch.shared()
    fit = check_fit(siftlib, mp, batch)
    out, counts, _ = check_shift(siftlib, mp, batch)
    if name == "edge":
        assert fit[:, fr.N].tolist() == list(eb.EDGE_SIZES) and counts[:, 0].tolist() == list(eb.EDGE_SIZES)
        assert fit[:, fr.STATUS].tolist() == [fr.EMPTY, fr.DEGENERATE, fr.DEGENERATE] + [fr.OK] * 9
    if name == "large":
        assert fit[:, fr.N].tolist() == [0, 70001, 3]
    if name == "leak":
        for s in range(batch.S):
            assert out[s, :2].tolist() == list(eb.leak_displacement(s)) and counts[s, 0] == eb.LEAK_IN_RANGE == fit[s, fr.N]
    if name == "degenerate":
        assert fit[:, fr.STATUS].tolist() == [fr.OK, fr.DEGENERATE, fr.OK, fr.DEGENERATE, fr.OK]
    if name == "masked":
        assert fit[:, fr.STATUS].tolist() == [fr.OK, fr.EMPTY, fr.OK] and np.isnan(out[1]).all() and counts[1, 0] == 0


# ---------------------------------------------------------------------------------------------- 2. the grid of the fit
@pytest.mark.parametrize("blocks", [1, 3, 256, 1024])
def test_fit_with_a_grid_of_the_callers(siftlib, mp, blocks):
    """every segment of the edge batch on `blocks` workgroups, against fit_ref.fit(blocks=blocks): 1 is up to four pairs per lane,
    3 two rows for the largest segments, 256 and 1024 workgroups without a pair"""
    batch = eb.edge_batch()
    want = check_fit(siftlib, mp, batch, blocks=blocks)
    for s in (9, 11):               # and the restatement of the batch is fit_ref.fit on the segment
        kp1, kp2, pairs, mask = batch.segment(s)
        assert fr.same_bits(want[s], fr.fit(kp1, kp2, pairs, mask, blocks))


# ---------------------------------------------------------------------------------------------- 3. keep
@pytest.mark.parametrize("tol", [0.0, 1.5, np.inf])
def test_keep(siftlib, mp, tol):
    batch = eb.keep_batch()
    out, counts, keep = check_shift(siftlib, mp, batch, tol=tol)
    assert not keep[batch.rows(1)].any() and not keep[batch.rows(3)].any() and counts[1].tolist() == [4, 0]     # medians not finite
    assert counts[0, 1] >= 400 and (counts[0, 1] == 500) == (tol == np.inf)
    check_shift(siftlib, mp, eb.masked_batch(), tol=tol)
    check_shift(siftlib, mp, eb.value_batch().shared(), tol=tol)


# ---------------------------------------------------------------------------------------------- 4. no read across a segment's bounds
@pytest.mark.parametrize("form", ["separate", "shared"])
def test_leak_batch_in_device_tensors_of_exactly_their_size(siftlib, mp, form):
    batch = eb.leak_batch() if form == "separate" else eb.leak_batch().shared()
    check_fit(siftlib, mp, batch, place=(1, 1, 1, 0))
    out, counts, keep = check_shift(siftlib, mp, batch, tol=0.0, place=(1, 1, 1, 0))
    for s in range(batch.S):
        assert out[s, :2].tolist() == list(eb.leak_displacement(s)) and counts[s].tolist() == [eb.LEAK_IN_RANGE] * 2


# ---------------------------------------------------------------------------------------------- 5. residency
@pytest.mark.parametrize("place", [(0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1)])
def test_same_result_wherever_the_inputs_lie(siftlib, mp, place):
    for batch in (eb.masked_batch(), eb.masked_batch().shared()):
        check_fit(siftlib, mp, batch, place=place)
        check_shift(siftlib, mp, batch, tol=1.5, place=place)


# ---------------------------------------------------------------------------------------------- 6. nothing stale
def test_a_small_call_after_a_large_one_and_the_same_call_twice(siftlib):
    """the partials, positions, keys and keep bytes of 70 001 pairs lie behind the next, smaller call; a table of 12 segments
    behind one of 3"""
    import sift_pyocl_amd as sp
    own = sp.MatchPlan()
    check_fit(siftlib, own, eb.large_batch())
    check_shift(siftlib, own, eb.large_batch(), tol=np.inf)
    for _ in range(2):
        check_fit(siftlib, own, eb.leak_batch())
        check_shift(siftlib, own, eb.leak_batch(), tol=0.0)
    check_fit(siftlib, own, eb.edge_batch(), blocks=3)
    check_fit(siftlib, own, eb.masked_batch())
    check_shift(siftlib, own, eb.edge_batch(), tol=1.5)
    check_shift(siftlib, own, eb.masked_batch(), tol=1.5)
    check_shift(siftlib, own, eb.masked_batch())
    check_fit(siftlib, own, eb.edge_batch())


# ---------------------------------------------------------------------------------------------- 7. nothing to do
def test_no_segment_and_no_pair_launch_nothing(siftlib, mp):
    none = eb.from_segments("none", [])
    out, ms = abi_fit(siftlib, mp, none)
    assert out.shape == (0, 20) and ms == 0
    out, counts, keep, ms = abi_shift(siftlib, mp, none, tol=1.0)
    assert out.shape == (0, 6) and ms == 0
    blank = eb.from_segments("blank", [eb.case_segment(0, 90 + k) for k in range(3)])
    for batch in (blank, blank.shared(), blank.with_mask(np.zeros(0, np.uint8))):
        assert len(batch.kp1) > 0 and len(batch.pairs) == 0
        out, ms = abi_fit(siftlib, mp, batch)
        assert ms == 0 and out[:, 0].tolist() == [fr.EMPTY] * 3 and out[:, 1].tolist() == [0] * 3 and np.isnan(out[:, 2:]).all()
        out, counts, keep, ms = abi_shift(siftlib, mp, batch, tol=1.0)
        assert ms == 0 and np.isnan(out).all() and counts.tolist() == [[0, 0]] * 3
    fit, rms, n = mp.fit_batch(blank.kp1, blank.counts1, blank.kp2, blank.counts2, blank.pairs, blank.pair_counts)
    assert fit.shape == (3, 6) and np.isnan(fit).all() and np.isnan(rms).all() and n.tolist() == [0, 0, 0]
    kp = np.zeros(0, sr.DTYPE_KP)
    shifts, n = mp.shift_batch(kp, None, kp, [], np.zeros((0, 2), np.int32), [])
    assert shifts.shape == (0, 2) and n.shape == (0,)


# ---------------------------------------------------------------------------------------------- 8. errors
def test_argument_errors_launch_nothing_and_write_nothing(siftlib, mp):
    from sift_pyocl_amd import _lib
    b = eb.degenerate_batch()
    S, M = b.S, len(b.pairs)
    fit_out = np.full((S, 20), FILL64, np.float64)
    out = np.full((S, 6), FILL32, np.float32)
    counts = np.full((S, 2), COUNT_FILL, np.int64)
    keep = np.full(M, KEEP_FILL, np.uint8)
    ms = C.c_double(-1)
    c1, c2, pc = b.counts1.copy(), b.counts2.copy(), b.pair_counts.copy()

    def bad(a, k, v):
        a = a.copy(); a[k] = v
        return a
    # a batch of 1025 one-pair segments: blocks = 1024 makes 1025 * 1024 > 2^20 workgroups
    many = 1025
    kp_many = np.zeros(many, sr.DTYPE_KP)
    c_many = np.ones(many, np.int64)
    pairs_many = np.zeros((many, 2), np.int32)
    hold = []

    def call(which, h=mp._handle, k1=b.kp1.ctypes.data, n1=len(b.kp1), k2=b.kp2.ctypes.data, n2=len(b.kp2), S=S, c1=c1, c2=c2,
             pp=b.pairs.ctypes.data, m=M, pc=pc, blocks=0, tol=1.0, kp=keep.ctypes.data, fo=fit_out.ctypes.data, o=out.ctypes.data,
             c=counts.ctypes.data):
        hold[:] = [None if a is None else np.ascontiguousarray(a, np.int64) for a in (c1, c2, pc)]
        p1, p2, p3 = (None if a is None else a.ctypes.data for a in hold)
        head = (h, k1, n1, 0, k2, n2, 0, S, p1, p2, pp, m, 0, p3, None, 0)
        if which == "fit":
            return siftlib.siftmi_match_fit_batch(*head, blocks, fo, C.byref(ms))
        return siftlib.siftmi_match_shift_batch(*head, C.c_float(tol), kp, o, c, C.byref(ms))

    shared_errors = [dict(h=None), dict(S=65536), dict(S=-1), dict(c2=bad(c2, 1, -1)), dict(c1=bad(c1, 0, -3)), dict(pc=bad(pc, 2, -1)),
                     dict(n2=len(b.kp2) - 1), dict(n1=len(b.kp1) + 1), dict(c2=bad(c2, 0, c2[0] + 1)), dict(c1=bad(c1, 4, c1[4] - 1)),
                     dict(m=M - 1), dict(pc=bad(pc, 0, pc[0] + 1)), dict(m=2 ** 31), dict(n1=-1), dict(n2=2 ** 40),
                     dict(k1=None), dict(k2=None), dict(pp=None), dict(c2=None), dict(pc=None)]
    for which, more in (("fit", [dict(blocks=-1), dict(blocks=1025), dict(fo=None),
                                 dict(k1=kp_many.ctypes.data, n1=many, c1=None, k2=kp_many.ctypes.data, n2=many, S=many, c2=c_many,
                                      pp=pairs_many.ctypes.data, m=many, pc=c_many, blocks=1024)]),
                        ("shift", [dict(tol=-1.0), dict(tol=float("nan")), dict(o=None), dict(c=None)])):
        for kw in shared_errors + more:
            assert call(which, **kw) == _lib.EINVAL, (which, kw)
            assert _lib.last_error()
            assert (fit_out == FILL64).all() and (out == FILL32).all() and (counts == COUNT_FILL).all() and (keep == KEEP_FILL).all(), (which, kw)
            assert ms.value == -1, (which, kw)
    # valid calls after the refused ones are right; a tol no keep mask reads is not looked at
    check_fit(siftlib, mp, b)
    check_shift(siftlib, mp, b, tol=1.0)
    assert call("shift", tol=float("nan"), kp=None) == _lib.OK and eb.same_bits32(out, ref_shift(b)[0]) and (keep == KEEP_FILL).all()
    assert call("fit", blocks=1024) == _lib.OK and eb.same_bits64(fit_out, ref_fit(b, 1024))
    # through the methods: ValueError for what the counts, blocks and tol can get wrong, RuntimeError for a wrong array
    args = (b.kp1, b.counts1, b.kp2, b.counts2, b.pairs, b.pair_counts)

    def with_(k, v):
        a = list(args); a[k] = v
        return a
    zero = np.zeros(0, sr.DTYPE_KP)
    wrong = [with_(3, bad(c2, 1, -1)), with_(1, bad(c1, 0, -3)), with_(5, bad(pc, 2, -1)), with_(3, bad(c2, 0, c2[0] + 1)),
             with_(1, bad(c1, 4, c1[4] - 1)), with_(5, bad(pc, 0, pc[0] + 1)), with_(5, pc[:-1]), with_(1, c1[:-1]), with_(4, b.pairs[:-1]),
             [zero, None, zero, [0] * 65536, np.zeros((0, 2), np.int32), [0] * 65536]]
    for a in wrong:
        with pytest.raises(ValueError):
            mp.fit_batch(*a)
        with pytest.raises(ValueError):
            mp.shift_batch(*a)
    for kw in (dict(blocks=-1), dict(blocks=1025)):
        with pytest.raises(ValueError):
            mp.fit_batch(*args, **kw)
    with pytest.raises(ValueError):
        mp.fit_batch(kp_many, None, kp_many, c_many, pairs_many, c_many, blocks=1024)
    for tol in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            mp.shift_batch(*args, tol=tol)
    for method in (mp.fit_batch, mp.shift_batch):
        with pytest.raises(RuntimeError):
            method(*with_(4, b.pairs.astype(np.int64)))
        with pytest.raises(RuntimeError):
            method(*args, mask=np.ones(M - 1, np.uint8))
        with pytest.raises(RuntimeError):
            method(*args, mask=np.ones(M, np.float32))


# ---------------------------------------------------------------------------------------------- 9. the methods
def test_python_methods_on_host_arrays_and_tensors(siftlib, mp):
    import torch
    b = eb.masked_batch()
    args = (b.kp1, b.counts1, b.kp2, b.counts2, b.pairs, b.pair_counts)
    want = ref_fit(b)
    wout, wcounts, wkeep = ref_shift(b, 1.5)
    for mask in (b.mask, b.mask != 0, torch.from_numpy(b.mask != 0).cuda()):
        models, rms, n, raw = mp.fit_batch(*args, mask=mask, return_moments=True)
        assert raw.shape == (3, 20) and eb.same_bits64(raw, want) and models.shape == (3, 6) and rms.shape == (3,)
        assert n.dtype == np.int64 and n.tolist() == want[:, fr.N].tolist()
        assert eb.same_bits64(models[[0, 2]], want[[0, 2]][:, fr.MODEL]) and np.isnan(models[1]).all() and np.isnan(rms[1])
        assert rms[0] == np.sqrt(want[0, fr.SSR] / want[0, fr.N]) and rms[2] == np.sqrt(want[2, fr.SSR] / want[2, fr.N])
        assert len(mp.fit_batch(*args, mask=mask)) == 3
        shifts, n, keep, n_keep, ranks = mp.shift_batch(*args, mask=mask, tol=1.5, return_ranks=True)
        assert shifts.dtype == np.float32 and shifts.shape == (3, 2) and eb.same_bits32(shifts, wout[:, :2]) and eb.same_bits32(ranks, wout)
        assert n.dtype == n_keep.dtype == np.int64 and n.tolist() == wcounts[:, 0].tolist() and n_keep.tolist() == wcounts[:, 1].tolist()
        assert keep.dtype == np.bool_ and np.array_equal(keep, wkeep)
        assert len(mp.shift_batch(*args, mask=mask)) == 2 and len(mp.shift_batch(*args, mask=mask, return_ranks=True)) == 3
        assert len(mp.shift_batch(*args, mask=mask, tol=np.inf)) == 4
    e = eb.edge_batch().shared()
    raw = mp.fit_batch(on_device(e.kp1), None, on_device(e.kp2), e.counts2, torch.from_numpy(e.pairs).cuda(), e.pair_counts, blocks=3,
                       return_moments=True)[3]
    assert eb.same_bits64(raw, ref_fit(e, 3))


def test_profile_appends_the_events(siftlib):
    import sift_pyocl_amd as sp
    b = eb.degenerate_batch()
    prof = sp.MatchPlan(profile=True)
    args = (b.kp1, b.counts1, b.kp2, b.counts2, b.pairs, b.pair_counts)
    prof.fit_batch(*args)
    prof.shift_batch(*args)
    assert [label for label, _ in prof.events] == ["fit_batch", "shift_batch"]
    for _, ev in prof.events:
        assert 0 < ev.profile.end - ev.profile.start < 1e9


# ---------------------------------------------------------------------------------------------- 10. against the existing methods
def test_against_the_loop_of_fit_and_shift_on_real_keypoints(mp):
    """three 256 x 256 frames through BatchPlan.keypoints_batch_device -> match_batch(out="device") -> both new methods: every
    segment's result is fit() / shift() on the slices, bit for bit.  The only comparison with package code instead of the
    restatement."""
    import torch
    import sift_pyocl_amd as sp
    shape = (256, 256)
    base = smooth_noise(shape, seed=71, sigma=1.5)
    frames = [base, np.roll(base, (3, -2), axis=(0, 1)) + 0.02 * white_noise(shape, seed=72), smooth_noise(shape, seed=73, sigma=1.5)]
    bp = sp.BatchPlan(shape=shape, dtype=np.float32, lanes=2)
    counts, records = bp.keypoints_batch_device([torch.from_numpy(f.astype(np.float32)).cuda() for f in frames])
    assert min(counts) > 20
    ref = records[:counts[0] * 144]
    off = np.concatenate([[0], np.cumsum(counts)])
    pairs, pair_counts = mp.match_batch(ref, None, records, counts, out="device")
    assert pair_counts[0] > 18 and pair_counts[1] > 18
    rows = np.concatenate([[0], np.cumsum(pair_counts)])
    models, rms, n, raw = mp.fit_batch(ref, None, records, counts, pairs, pair_counts, return_moments=True)
    shifts, ns, keep, n_keep, ranks = mp.shift_batch(ref, None, records, counts, pairs, pair_counts, tol=1.5, return_ranks=True)
    for s in range(3):
        seg, ps = records[off[s] * 144:off[s + 1] * 144], pairs[rows[s]:rows[s + 1]]
        model_s, rms_s, n_s, raw_s = mp.fit(ref, seg, ps, return_moments=True)
        assert fr.same_bits(raw[s], raw_s) and n[s] == n_s, (s, raw[s], raw_s)
        if model_s is None:
            assert np.isnan(models[s]).all() and np.isnan(rms[s])
        else:
            assert fr.same_bits(models[s], model_s) and rms[s] == rms_s
        moved, m_s, keep_s, ranks_s = mp.shift(ref, seg, ps, tol=1.5, return_ranks=True)
        assert sr.same_bits(ranks[s], ranks_s) and ns[s] == m_s, (s, ranks[s], ranks_s)
        assert np.array_equal(keep[rows[s]:rows[s + 1]], keep_s) and n_keep[s] == keep_s.sum()
        if moved is not None:
            assert sr.same_bits(shifts[s], np.float32(moved))
    # frame 0 against itself does not move; frame 1 is frame 0 rolled by whole pixels (3 down, 2 left) plus faint noise, and a
    # median of sub-pixel positions stays well within a quarter pixel of that
    assert shifts[0].tolist() == [0.0, 0.0] and abs(shifts[1, 0] + 2) < 0.25 and abs(shifts[1, 1] - 3) < 0.25
