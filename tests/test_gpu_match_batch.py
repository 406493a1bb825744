"""GPU tests of MatchPlan.match_batch / siftmi_match_batch (k_match_batch.hpp): S segment pairs matched
by one set of launches.  The expected result is the numpy restatement's (tests/match_batch_ref.py; the CPU test
tests/test_match_batch_ref_host.py pins it to the oracle's matcher segment by segment and to the answer each construction
dictates) and, on real keypoints, the existing matcher's.  Every comparison is exact: the rows of `pairs` in their order,
`pair_counts`, dtype and shape."""
import ctypes as C

import numpy as np
import pytest

import match_batch_ref as mb
import match_cases as mc
from util import smooth_noise, sort_rows, white_noise

pytestmark = pytest.mark.gpu

_REF = {}


def reference(batch):
    """the restatement's answer, computed once a batch"""
    if batch.name not in _REF:
        _REF[batch.name] = batch.reference()
    return _REF[batch.name]


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
    return mp.match_batch(kp1, counts1, kp2, counts2, ratio=batch.ratio, mutual=batch.mutual, **kw)


# ---------------------------------------------------------------------------------------------- 1. segment edges
@pytest.mark.parametrize("batch", mb.edge_batches(), ids=lambda b: b.name)
def test_segment_edges(mp, batch):
    """lists of 0, 1, 2, 63 .. 320 elements against 0, 1, 255 .. 513 and 600 queries, the tables exchanged, one segment alone"""
    want = reference(batch)
    same(run(mp, batch), want, batch.name)
    same(run(mp, batch, device=True), want, batch.name + " [device lists]")
    same(run(mp, batch, part_len=64), want, batch.name + " [part_len 64]")


# ---------------------------------------------------------------------------------------------- 2. no leak across a boundary
def test_no_leak_across_a_boundary(mp):
    """device tensors sized exactly to the records; right outside every segment's list lie elements at distances 0 and 1 from
    its queries, and the neighbours' queries carry other descriptors"""
    batch = mb.leak_batch()
    want = reference(batch)
    assert np.array_equal(want[0], np.concatenate(batch.dictated))
    for part_len in (0, 64):
        same(run(mp, batch, device=True, part_len=part_len), want, "%s [part_len %d]" % (batch.name, part_len))
    same(run(mp, batch, device=True, out="device"), want, batch.name + " [device result]")
    got = mp.match_batch(to_device(batch.kp1), batch.counts1, to_device(batch.kp2), batch.counts2, mutual=True)
    same(got, mb.match_batch(batch.kp1, batch.counts1, batch.kp2, batch.counts2, mutual=True), batch.name + " [mutual]")


# ---------------------------------------------------------------------------------------------- 3. partition fold
@pytest.mark.parametrize("ratio", [None, 1.0])
def test_partition_fold(mp, ratio):
    """the tie and placement families at 65, 130 and 257 elements as segments of one call: with 64 elements a partition the
    minimum, its tie and the second minimum fall into different partitions; the library's choice must give the same"""
    batch = mb.fold_batch(ratio)
    want = reference(batch)
    assert np.array_equal(want[0], np.concatenate(batch.dictated))
    for part_len in (64, 0, 128):
        same(run(mp, batch, part_len=part_len), want, "%s [part_len %d]" % (batch.name, part_len))


# ---------------------------------------------------------------------------------------------- 4. ratio
@pytest.mark.parametrize("ratio", mb.RATIOS)
def test_ratio(mp, ratio):
    """every critical (dist1, dist2) of float32(ratio ** 2), one list a segment"""
    batch = mb.ratio_batch(ratio)
    want = reference(batch)
    assert np.array_equal(want[0], np.concatenate(batch.dictated))
    same(run(mp, batch), want, batch.name)
    same(run(mp, batch, part_len=64), want, batch.name + " [part_len 64]")


def test_ratio_above_one_raises(mp):
    batch = mb.shared_batches()[1]
    with pytest.raises(ValueError):
        mp.match_batch(*batch.args(), ratio=1.1)
    same(run(mp, batch), reference(batch), batch.name + " [after the refused call]")


# ---------------------------------------------------------------------------------------------- 5. mutual
@pytest.mark.parametrize("batch", mb.mutual_batches(), ids=lambda b: b.name)
def test_mutual(mp, batch):
    """duplicates in the first list: the reverse scan's nearest must be the earliest of them; separate first lists and one
    shared first list (the reversed scan then has the one list as every segment's list)"""
    want = reference(batch)
    same(run(mp, batch), want, batch.name)
    same(run(mp, batch, part_len=64, device=True), want, batch.name + " [part_len 64, device lists]")
    plain = mp.match_batch(*batch.args())
    assert plain[1].sum() > want[1].sum()                            # the filter does drop pairs here


# ---------------------------------------------------------------------------------------------- 6. shared reference, residency
def test_shared_reference_and_residency(mp):
    import torch
    large, small = mb.shared_batches()
    want = reference(large)
    kpsize = mp.kpsize
    same(run(mp, large), want, large.name)
    # counts1 = None is the per-segment loop
    loop = [mp.match(large.kp1, b, raw_results=True) for _, b in large.segments()]
    assert np.array_equal(np.concatenate([sort_rows(r.reshape(-1, 2)) for r in loop]), want[0])
    assert [len(r) for r in loop] == want[1].tolist()
    # ... and the same list repeated S times with its counts
    S = len(large.counts2)
    same(mp.match_batch(np.concatenate([large.kp1] * S), [len(large.kp1)] * S, large.kp2, large.counts2), want, large.name + " [repeated]")
    # host records against device tensors, one side at a time and both
    d1, d2 = to_device(large.kp1), to_device(large.kp2)
    same(mp.match_batch(d1, None, large.kp2, large.counts2), want, large.name + " [kp1 on the device]")
    same(mp.match_batch(large.kp1, None, d2, large.counts2), want, large.name + " [kp2 on the device]")
    got = mp.match_batch(d1, None, d2, large.counts2, out="device")
    assert isinstance(got[0], torch.Tensor) and got[0].device.index == mp.device
    same(got, want, large.name + " [device result]")
    # a slice of the device result goes straight into the calls that consume pairs
    first = got[0][:int(want[1][0])]
    (dx, dy), n = mp.shift(d1, d2[:large.counts2[0] * 144], first)
    assert n == want[1][0]
    # a second, smaller call on the same plan: nothing of the larger one's scratch shows
    same(run(mp, small), reference(small), small.name + " [after the larger call]")
    same(run(mp, small, device=True, out="device"), reference(small), small.name + " [device]")
    same(run(mp, large, part_len=64), want, large.name + " [again, part_len 64]")
    assert mp.kpsize == kpsize
    # no segment at all: two empty arrays
    pairs, counts = mp.match_batch(large.kp1, None, large.kp2[:0], [])
    assert pairs.shape == (0, 2) and pairs.dtype == np.int32 and counts.shape == (0,) and counts.dtype == np.int64
    pairs, counts = mp.match_batch(large.kp1[:0], [], large.kp2[:0], [], out="device")
    assert tuple(pairs.shape) == (0, 2) and pairs.dtype == torch.int32 and counts.shape == (0,)
    # segments that are all empty on one side
    same(mp.match_batch(large.kp1[:0], None, large.kp2, large.counts2), (np.zeros((0, 2), np.int32), np.zeros(S, np.int64)), "empty shared list")
    same(mp.match_batch(large.kp1, None, large.kp2[:0], [0, 0, 0]), (np.zeros((0, 2), np.int32), np.zeros(3, np.int64)), "empty second lists")


def test_profile_events(siftlib):
    import sift_pyocl_amd as sp
    plan = sp.MatchPlan(profile=True)
    batch = mb.shared_batches()[1]
    same(run(plan, batch), reference(batch), batch.name + " [profile]")
    assert [label for label, _ in plan.events] == list(sp.MatchPlan.STAGE_LABELS)
    assert all(evt.profile.end >= evt.profile.start for _, evt in plan.events)
    plan.reset_timer()
    same(run(plan, batch, device=True, out="device"), reference(batch), batch.name + " [profile, device]")
    assert [label for label, _ in plan.events] == ["matching"]


# ---------------------------------------------------------------------------------------------- 7. against the existing matcher
def test_against_match_on_real_keypoints(mp):
    """the records of BatchPlan.keypoints_batch_device for four 256 x 256 frames (one all blank: a segment of 0 records), every
    frame against the first: the pairs of every segment are match(ref, frame_s, raw_results=True) as sorted rows"""
    import sift_pyocl_amd as sp
    shape = (256, 256)
    base = smooth_noise(shape, seed=71, sigma=1.5)
    frames = [base, np.roll(base, (3, -2), axis=(0, 1)) + 0.02 * white_noise(shape, seed=72), np.zeros(shape, np.float32),
              smooth_noise(shape, seed=73, sigma=1.5)]
    import torch
    bp = sp.BatchPlan(shape=shape, dtype=np.float32, lanes=2)
    counts, records = bp.keypoints_batch_device([torch.from_numpy(f.astype(np.float32)).cuda() for f in frames])
    assert counts[2] == 0 and min(counts[0], counts[1], counts[3]) > 20 and records.numel() == sum(counts) * 144
    ref = records[:counts[0] * 144]
    off = np.concatenate([[0], np.cumsum(counts)])
    pairs, pair_counts = mp.match_batch(ref, None, records, counts)
    assert pairs.dtype == np.int32 and pair_counts.dtype == np.int64 and pair_counts.shape == (4,) and pair_counts.sum() == len(pairs)
    assert pair_counts[0] > 0 and pair_counts[2] == 0
    got = mb.split(pairs, pair_counts)
    for s in range(4):
        want = sort_rows(mp.match(ref, records[off[s] * 144:off[s + 1] * 144], raw_results=True).reshape(-1, 2))
        assert np.array_equal(got[s], want), "frame %d" % s
    # each frame against the one before it: two slices of one tensor
    pairs, pair_counts = mp.match_batch(records[:off[3] * 144], counts[:-1], records[off[1] * 144:], counts[1:], mutual=True)
    got = mb.split(pairs, pair_counts)
    for s in range(3):
        want = mp.match(records[off[s] * 144:off[s + 1] * 144], records[off[s + 1] * 144:off[s + 2] * 144], raw_results=True, mutual=True)
        assert np.array_equal(got[s], sort_rows(want.reshape(-1, 2))), "frame %d against frame %d" % (s + 1, s)


# ---------------------------------------------------------------------------------------------- 8. argument errors
def test_argument_errors_leave_the_plan_usable(siftlib, mp):
    from sift_pyocl_amd import _lib
    batch = mb.shared_batches()[1]
    kp1, _, kp2, counts2 = batch.args()
    for bad in ([counts2[0] + 1, counts2[1]], [counts2[0]], [counts2[0], counts2[1], 1]):          # counts that do not add up
        with pytest.raises(ValueError):
            mp.match_batch(kp1, None, kp2, bad)
    with pytest.raises(ValueError):
        mp.match_batch(kp1, [len(kp1), 1], kp2, counts2)
    with pytest.raises(ValueError):
        mp.match_batch(kp1, [len(kp1)], kp2, counts2)                                               # S differs between the tables
    with pytest.raises(ValueError):
        mp.match_batch(kp1, None, kp2, [len(kp2) + 1, -1])                                          # a negative count
    for part_len in (65, 100, -64, 65536):
        with pytest.raises(ValueError):
            mp.match_batch(kp1, None, kp2, counts2, part_len=part_len)
    with pytest.raises(ValueError):
        mp.match_batch(kp1, None, kp2[:0], [0] * 65536)                                             # more than 65 535 segments
    with pytest.raises(ValueError):
        mp.match_batch(kp1, None, kp2, counts2, out="pinned")
    # the entry point refuses the same on its own, and writes nothing
    pairs = np.full((2 * len(kp1), 2), -7, np.int32)
    pc = np.full(2, -7, np.int64)

    def abi(c2, th=float(mc.RATIO), part_len=0, S=2, p2=kp2.ctypes.data):
        c2 = np.asarray(c2, np.int64)
        return siftlib.siftmi_match_batch(mp._handle, kp1.ctypes.data, len(kp1), 0, p2, len(kp2), 0, S, None, c2.ctypes.data, C.c_float(th), 0,
                                          part_len, pairs.ctypes.data, 0, pc.ctypes.data)

    assert abi([counts2[0] + 1, counts2[1]]) == _lib.EINVAL and b"add up" in siftlib.siftmi_last_error()
    assert abi([len(kp2) + 1, -1]) == _lib.EINVAL
    assert abi(counts2, th=1.5) == _lib.EINVAL and abi(counts2, th=float("nan")) == _lib.EINVAL
    assert abi(counts2, part_len=96) == _lib.EINVAL and abi(counts2, part_len=65536) == _lib.EINVAL
    assert abi(counts2, S=-1) == _lib.EINVAL and abi(counts2, S=65536) == _lib.EINVAL
    assert abi(counts2, p2=None) == _lib.EINVAL
    assert (pairs == -7).all() and (pc == -7).all()
    assert abi(counts2) == 0
    want = reference(batch)
    assert np.array_equal(pc, want[1]) and np.array_equal(pairs[:len(want[0])], want[0])
    same(run(mp, batch), want, batch.name + " [after the refused calls]")
