"""GPU tests of MatchPlan.match_window_batch / siftmi_match_window_batch (k_match_window_batch.hpp): the
windowed matcher over S segment pairs in one set of launches.  The expected result is the numpy restatement's
(tests/match_window_batch_ref.py: window_ref.match on every segment's slices; tests/test_match_window_batch_ref_host.py pins what
each crafted batch holds).  Every comparison is exact and of whole arrays: the rows of `pairs` in their order, `pair_counts`,
dtype and shape."""
import ctypes as C

import numpy as np
import pytest

import match_batch_ref as mb
import match_cases as mc
import match_window_batch_ref as wb
from util import sort_rows

pytestmark = pytest.mark.gpu

INF = float("inf")
_REF = {}


def reference(batch, **kw):
    """the restatement's answer, computed once a batch and variant"""
    key = (batch.name,) + tuple(sorted((k, repr(v)) for k, v in kw.items()))
    if key not in _REF:
        _REF[key] = batch.reference(**kw)
    return _REF[key]


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


def to_device(records):
    """a uint8 tensor sized exactly to the records"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(records).view(np.uint8).reshape(-1).copy()).cuda()
    assert t.numel() == len(records) * 144
    return t


def same(got, want, what):
    pairs, counts = got
    if not isinstance(pairs, np.ndarray):
        import torch
        assert pairs.dtype == torch.int32 and pairs.is_cuda, what
        pairs = pairs.cpu().numpy()
    assert isinstance(counts, np.ndarray) and counts.dtype == np.int64 and counts.shape == want[1].shape, what
    assert np.array_equal(counts, want[1]), "%s: pair_counts %s, expected %s" % (what, counts.tolist(), want[1].tolist())
    assert pairs.dtype == np.int32 and pairs.shape == want[0].shape, "%s: pairs %s %s, expected %s" % (what, pairs.dtype, pairs.shape, want[0].shape)
    assert np.array_equal(pairs, want[0]), what


def run(mp, batch, device=False, **kw):
    kp1, counts1, kp2, counts2 = batch.args()
    if device:
        kp1, kp2 = to_device(kp1), to_device(kp2)
    kw.setdefault("window", batch.window)
    kw.setdefault("mutual", batch.mutual)
    kw.setdefault("ratio", batch.ratio)
    return mp.match_window_batch(kp1, counts1, kp2, counts2, window_shift=batch.shifts, **kw)


# ---------------------------------------------------------------------------------------------- 1. loop and block edges
@pytest.mark.parametrize("window", [INF, 4.0, (7.0, 3.0)], ids=repr)
def test_loop_and_block_edges(mp, window):
    """0, 1, 2, 255 .. 513 queries against 0, 1, 63 .. 129 elements, and one segment whose 600 queries and 200 elements share one
    position; with the infinite window every segment is one cell, so the chunks of 256 queries and the tiles of 64 are all met"""
    batch = wb.edge_batch(window)
    want = reference(batch)
    same(run(mp, batch), want, batch.name)
    same(run(mp, batch, device=True, grid_max=1), want, batch.name + " [device lists, one cell]")
    same(run(mp, batch, mutual=True), reference(batch, mutual=True), batch.name + " [mutual]")


# ---------------------------------------------------------------------------------------------- 2. isolation
@pytest.mark.parametrize("shared", [False, True], ids=["own lists", "shared reference"])
def test_segments_are_isolated(mp, shared):
    """the exact descriptor of every query lies inside the window in both neighbouring segments and not in its own: no pair may
    reference it, and the neighbours' counts are the restatement's"""
    batch = wb.leak_batch(shared)
    want = reference(batch)
    for grid_max in (0, 1, 5):
        same(run(mp, batch, device=True, grid_max=grid_max), want, "%s [grid_max %d]" % (batch.name, grid_max))
    same(run(mp, batch, device=True, out="device"), want, batch.name + " [device result]")
    same(run(mp, batch, device=True, mutual=True), reference(batch, mutual=True), batch.name + " [mutual]")
    if not shared:
        segs, partner = wb.leak_parts()
        assert np.array_equal(want[0], np.concatenate([np.stack([np.arange(len(a)), p], axis=1) for (a, _), p in zip(segs, partner)]))


# ---------------------------------------------------------------------------------------------- 3. per-segment grids
def test_per_segment_grids(mp):
    """extents 0 .. 100, 1e6 .. 1e6 + 50, a single point, NaN / inf / 1e30 coordinates and an empty segment side by side: the same
    arrays for every cap on the grid"""
    batch = wb.grid_batch()
    want = reference(batch)
    want_mutual = reference(batch, mutual=True)
    for grid_max in wb.GRID_MAXES:
        same(run(mp, batch, grid_max=grid_max), want, "%s [grid_max %d]" % (batch.name, grid_max))
        same(run(mp, batch, grid_max=grid_max, mutual=True), want_mutual, "%s [grid_max %d, mutual]" % (batch.name, grid_max))
    same(run(mp, batch, window=INF), reference(batch, window=INF), batch.name + " [window inf]")
    same(run(mp, batch, window=(INF, 2.0)), reference(batch, window=(INF, 2.0)), batch.name + " [window (inf, 2)]")
    same(run(mp, batch, window=0.0), reference(batch, window=0.0), batch.name + " [window 0]")


# ---------------------------------------------------------------------------------------------- 4. the rule
@pytest.mark.parametrize("ratio", [1.0, 0.5, None])
def test_the_rule(mp, ratio):
    """prescribed distances either side of the threshold, tied minima in different cells, dist2 == 0, as segments of one call"""
    batch = wb.rule_batch(ratio)
    want = reference(batch)
    same(run(mp, batch), want, batch.name)
    same(run(mp, batch, grid_max=2, device=True), want, batch.name + " [grid_max 2, device lists]")


def test_lone_and_no_candidates(mp):
    batch = wb.lone_batch()
    want = reference(batch)
    same(run(mp, batch), want, batch.name)
    assert want[1].tolist() == [2 * n for n in batch.counts2]          # two lone-candidate queries an element, the third has none
    same(run(mp, batch, mutual=True), reference(batch, mutual=True), batch.name + " [mutual]")


# ---------------------------------------------------------------------------------------------- 5. shifts
@pytest.mark.parametrize("mutual", [False, True])
def test_per_segment_shifts(mp, mutual):
    """(S, 2) shifts, negative and fractional ones: the arrays of the restatement and of one scalar-shift call a segment"""
    batch = wb.shift_batch(mutual=mutual)
    want = reference(batch)
    got = run(mp, batch)
    same(got, want, batch.name)
    loop = [sort_rows(mp.match(a, b, raw_results=True, mutual=mutual, window=batch.window, window_shift=tuple(s)).reshape(-1, 2))
            for (a, b), s in zip(batch.segments(), wb.SHIFTS)]
    assert np.array_equal(np.concatenate(loop), got[0]) and [len(r) for r in loop] == got[1].tolist()
    one = mp.match_window_batch(*batch.args(), window=batch.window, window_shift=tuple(wb.SHIFTS[1]), mutual=mutual)
    same(one, wb.match_window_batch(*batch.args(), batch.window, tuple(wb.SHIFTS[1]), mutual=mutual), batch.name + " [one shift for all]")


# ---------------------------------------------------------------------------------------------- 6. identities
@pytest.mark.parametrize("batch", mb.edge_batches()[:1] + mb.mutual_batches() + mb.shared_batches()[:1], ids=lambda b: b.name)
def test_infinite_window_is_match_batch(mp, batch):
    """window = inf, zero shift, finite coordinates: match_batch's arrays exactly, order included, also with mutual"""
    for mutual in (False, True):
        want = mp.match_batch(*batch.args(), ratio=batch.ratio, mutual=mutual)
        got = mp.match_window_batch(*batch.args(), window=INF, ratio=batch.ratio, mutual=mutual)
        same(got, want, "%s [mutual %r]" % (batch.name, mutual))
        assert want[1].sum() > 0


def test_one_segment_twice_and_device_result(mp):
    """S = 1 is match(window=, window_shift=); two consecutive calls and out="device" give identical arrays"""
    batch = wb.shift_batch()
    (a, b), s = batch.segments()[2], tuple(wb.SHIFTS[2])
    got = mp.match_window_batch(a, [len(a)], b, [len(b)], window=batch.window, window_shift=s)
    want = sort_rows(mp.match(a, b, raw_results=True, window=batch.window, window_shift=s).reshape(-1, 2))
    assert np.array_equal(got[0], want) and got[1].tolist() == [len(want)] and len(want) > 20
    first = run(mp, batch)
    same(run(mp, batch), first, batch.name + " [second call]")
    same(run(mp, batch, device=True, out="device"), first, batch.name + " [device result]")


def test_device_result_feeds_consensus_and_fit(mp):
    batch = wb.shift_batch()
    d1, d2 = to_device(batch.kp1), to_device(batch.kp2)
    pairs_d, pc_d = mp.match_window_batch(d1, batch.counts1, d2, batch.counts2, window=batch.window, window_shift=batch.shifts, out="device")
    pairs_h, pc_h = run(mp, batch)
    same((pairs_d, pc_d), (pairs_h, pc_h), batch.name)
    mask_d, win_d = mp.consensus_batch(d1, batch.counts1, d2, batch.counts2, pairs_d, pc_d, out="device")[:2]
    mask_h, win_h = mp.consensus_batch(batch.kp1, batch.counts1, batch.kp2, batch.counts2, pairs_h, pc_h)[:2]
    assert np.array_equal(mask_d.cpu().numpy().astype(bool), np.asarray(mask_h).astype(bool)) and np.array_equal(win_d, win_h, equal_nan=True)
    fit_d = mp.fit_batch(d1, batch.counts1, d2, batch.counts2, pairs_d, pc_d, mask=mask_d)
    fit_h = mp.fit_batch(batch.kp1, batch.counts1, batch.kp2, batch.counts2, pairs_h, pc_h, mask=mask_h)
    for x, y in zip(fit_d, fit_h):
        assert np.array_equal(x, y, equal_nan=True)
    moved = mp.shift_batch(d1, batch.counts1, d2, batch.counts2, pairs_d, pc_d)[0]
    assert np.allclose(moved, wb.SHIFTS, atol=1.5)


# ---------------------------------------------------------------------------------------------- 7. many segments
def test_many_segments(mp):
    """1 100 segments of 0 .. 5 keypoints: more than 1 024 blocks through mb_scan_kernel, more segments than one scan pass"""
    batch = wb.many_batch()
    want = reference(batch)
    same(run(mp, batch), want, batch.name)
    same(run(mp, batch, mutual=True, device=True), reference(batch, mutual=True), batch.name + " [mutual, device lists]")
    shared = batch.segments()[3][0]
    got = mp.match_window_batch(shared, None, batch.kp2, batch.counts2, window=INF, mutual=True)
    same(got, wb.match_window_batch(shared, None, batch.kp2, batch.counts2, INF, mutual=True), batch.name + " [shared reference]")


def test_profile_events(siftlib):
    import sift_pyocl_amd as sp
    plan = sp.MatchPlan(profile=True)
    batch = wb.lone_batch()
    same(run(plan, batch), reference(batch), batch.name + " [profile]")
    assert [label for label, _ in plan.events] == list(sp.MatchPlan.STAGE_LABELS)
    plan.reset_timer()
    same(run(plan, batch, device=True, out="device"), reference(batch), batch.name + " [profile, device]")
    assert [label for label, _ in plan.events] == ["matching"]


# ---------------------------------------------------------------------------------------------- 8. errors
def test_argument_errors_leave_the_plan_usable(siftlib, mp):
    from sift_pyocl_amd import _lib
    batch = wb.lone_batch()
    kp1, counts1, kp2, counts2 = batch.args()
    S = len(counts2)
    for bad in (-1.0, float("nan"), (3.0, -0.5), (float("nan"), 3.0), None):
        with pytest.raises(ValueError):
            mp.match_window_batch(kp1, counts1, kp2, counts2, window=bad)
    for bad in ((INF, 0.0), (0.0, float("nan")), np.zeros((S + 1, 2)), [(0.0, 0.0)] * (S - 1) + [(0.0, -INF)]):
        with pytest.raises(ValueError):
            mp.match_window_batch(kp1, counts1, kp2, counts2, window=3.0, window_shift=bad)
    for bad in ([counts2[0] + 1] + counts2[1:], counts2[:-1], counts2 + [1]):
        with pytest.raises(ValueError):
            mp.match_window_batch(kp1, counts1, kp2, bad, window=3.0)
    for grid_max in (257, -1):
        with pytest.raises(ValueError):
            mp.match_window_batch(kp1, counts1, kp2, counts2, window=3.0, grid_max=grid_max)
    with pytest.raises(ValueError):
        mp.match_window_batch(kp1, counts1, kp2, counts2, window=3.0, ratio=1.1)
    with pytest.raises(ValueError):
        mp.match_window_batch(kp1, None, kp2[:0], [0] * 65536, window=3.0)
    with pytest.raises(ValueError):
        mp.match_window_batch(kp1, counts1, kp2, counts2, window=3.0, out="pinned")
    # the entry point refuses the same on its own, and writes nothing
    pairs = np.full((len(kp1), 2), -7, np.int32)
    pc = np.full(S, -7, np.int64)
    c1 = np.asarray(counts1, np.int64)

    def abi(c2=counts2, th=float(mc.RATIO), w=(3.0, 3.0), sh=None, grid_max=0, n_seg=S, handle=mp._handle, p2=kp2.ctypes.data):
        c2 = np.asarray(c2, np.int64)
        sh = np.zeros(2 * S, np.float32) if sh is None else np.asarray(sh, np.float32)
        return siftlib.siftmi_match_window_batch(handle, kp1.ctypes.data, len(kp1), 0, p2, len(kp2), 0, n_seg, c1.ctypes.data, c2.ctypes.data,
                                                 C.c_float(th), C.c_float(w[0]), C.c_float(w[1]), sh.ctypes.data, 0, grid_max,
                                                 pairs.ctypes.data, 0, pc.ctypes.data)

    assert abi(w=(-1.0, 3.0)) == _lib.EINVAL and abi(w=(3.0, float("nan"))) == _lib.EINVAL
    assert abi(sh=[0.0] * (2 * S - 1) + [INF]) == _lib.EINVAL and abi(sh=[float("nan")] + [0.0] * (2 * S - 1)) == _lib.EINVAL
    assert abi(c2=[counts2[0] + 1] + counts2[1:]) == _lib.EINVAL and b"add up" in siftlib.siftmi_last_error()
    assert abi(c2=[-1] + counts2[1:]) == _lib.EINVAL
    assert abi(grid_max=257) == _lib.EINVAL and abi(grid_max=-1) == _lib.EINVAL
    assert abi(n_seg=-1) == _lib.EINVAL and abi(n_seg=65536) == _lib.EINVAL
    assert abi(th=1.5) == _lib.EINVAL and abi(handle=None) == _lib.EINVAL and abi(p2=None) == _lib.EINVAL
    assert (pairs == -7).all() and (pc == -7).all()
    assert abi() == 0
    want = reference(batch)
    assert np.array_equal(pc, want[1]) and np.array_equal(pairs[:len(want[0])], want[0])
    assert abi(w=(INF, INF)) == 0
    want_inf = reference(batch, window=INF)
    assert np.array_equal(pc, want_inf[1]) and np.array_equal(pairs[:len(want_inf[0])], want_inf[0])
    same(run(mp, batch), want, batch.name + " [after the refused calls]")
    # no segment, and segments that are all empty on one side
    got = mp.match_window_batch(kp1[:0], [], kp2[:0], [], window=3.0)
    assert got[0].shape == (0, 2) and got[0].dtype == np.int32 and got[1].shape == (0,) and got[1].dtype == np.int64
    same(mp.match_window_batch(kp1[:0], None, kp2, counts2, window=3.0), (np.zeros((0, 2), np.int32), np.zeros(S, np.int64)), "empty shared list")
