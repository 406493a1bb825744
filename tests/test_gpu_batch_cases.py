"""GPU tests of the batch keypoint path's hand-back, through the C ABI (include/siftmi.h) on the cases of tests/batch_cases.py:
which frames siftmi_batch_keypoints_into delivers and which it parks, what lies behind and in the caller's arrays afterwards,
the arena's regrowth with records already parked, every range of siftmi_batch_fetch, the state a failed or a refused call leaves
behind, the per-frame bookkeeping (counts, offsets, min / max) around `lanes` and 2 * lanes frames, and the overflow flag.
Every comparison is byte equality of sorted records with the oracle; tests/test_batch_cases_host.py proves on the CPU that the
cases can tell the paths apart."""
import ctypes as C

import numpy as np
import pytest

import batch_cases as bc
from util import assert_same_keypoints, dtype_kp

pytestmark = pytest.mark.gpu

RB = bc.RECORD_BYTES
SENTINEL = -77
EINVAL = -1


# ------------------------------------------------------------------------------------------------ the ABI, with guards
def make_plan(shape, lanes, **kw):
    import sift_pyocl_amd as sp
    return sp.BatchPlan(shape=shape, dtype=np.float32, lanes=lanes, **kw)


def stage(specs, shape, on_device):
    """the frames of a batch where the call wants them: (list of objects to keep alive, list of addresses)"""
    frames = [bc.frame_of(s, shape) for s in specs]
    if not on_device:
        return frames, [f.ctypes.data for f in frames]
    import torch
    dev = [torch.from_numpy(f.copy()).cuda() for f in frames]
    torch.cuda.synchronize()
    return dev, [t.data_ptr() for t in dev]


class Result(object):
    pass


def abi_batch(L, bp, addrs, on_device, row=None, dtype=0, expect=0, n_images=None):
    """siftmi_batch_keypoints_into (row: [(class, capacity, null)] per frame) or siftmi_batch_keypoints (row None).  Every
    host_outs[i] has room for capacity + GUARD records and is filled with 0xa5; counts and offsets are filled with a sentinel."""
    n = len(addrs) if n_images is None else n_images
    ptrs = (C.c_void_p * max(1, len(addrs)))(*addrs)
    r = Result()
    r.counts, r.offsets = np.full(max(1, n), SENTINEL, np.int64), np.full(max(1, n), SENTINEL, np.int64)
    total, ovf = C.c_int64(SENTINEL), C.c_int32(SENTINEL)
    i64p = C.POINTER(C.c_int64)
    r.arrays = None
    if row is None:
        r.rc = L.siftmi_batch_keypoints(bp._handle, ptrs if addrs else None, n, dtype, int(on_device), r.counts.ctypes.data_as(i64p),
                                        r.offsets.ctypes.data_as(i64p), C.byref(total), C.byref(ovf))
    else:
        assert len(row) == n
        r.arrays = [None if null else np.full((cap + bc.GUARD) * RB, bc.FILL, np.uint8) for _, cap, null in row]
        outs = (C.c_void_p * n)(*[None if a is None else a.ctypes.data for a in r.arrays])
        caps = (C.c_int64 * n)(*[cap for _, cap, _ in row])
        r.rc = L.siftmi_batch_keypoints_into(bp._handle, ptrs, n, dtype, int(on_device), outs, caps, r.counts.ctypes.data_as(i64p),
                                             r.offsets.ctypes.data_as(i64p), C.byref(total), C.byref(ovf))
    from sift_pyocl_amd import _lib
    assert r.rc == expect, "rc %d, expected %d: %s" % (r.rc, expect, _lib.last_error())
    r.counts, r.offsets, r.total, r.overflow = r.counts[:n], r.offsets[:n], total.value, ovf.value
    return r


def abi_fetch(L, bp, first, count, on_device=False, expect=0):
    """siftmi_batch_fetch into a destination with one guard record of 0xa5 on either side; returns the (count, 144) bytes.  A
    refused call gets room for four records and must leave all of it untouched."""
    room = count if expect == 0 else 4
    if on_device:
        import torch
        buf = torch.full(((room + 2) * RB,), bc.FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        rc = L.siftmi_batch_fetch(bp._handle, buf.data_ptr() + RB, 1, first, count)
        host = buf.cpu().numpy()
    else:
        host = np.full((room + 2) * RB, bc.FILL, np.uint8)
        rc = L.siftmi_batch_fetch(bp._handle, host.ctypes.data + RB, 0, first, count)
    assert rc == expect, "fetch(%d, %d): rc %d, expected %d" % (first, count, rc, expect)
    body = host[RB:(room + 1) * RB]
    assert (host[:RB] == bc.FILL).all() and (host[(room + 1) * RB:] == bc.FILL).all(), "fetch(%d, %d) wrote outside" % (first, count)
    if expect != 0:
        assert (body == bc.FILL).all(), "refused fetch(%d, %d) wrote" % (first, count)
        return None
    return body.reshape(count, RB)


def abi_minmax(L, bp, n, expect=0):
    mins, maxs = np.full(max(1, n), np.float32(SENTINEL)), np.full(max(1, n), np.float32(SENTINEL))
    rc = L.siftmi_batch_minmax(bp._handle, mins.ctypes.data, maxs.ctypes.data, n)
    assert rc == expect, "minmax(%d): rc %d, expected %d" % (n, rc, expect)
    if expect != 0:
        assert (mins == SENTINEL).all() and (maxs == SENTINEL).all()
    return mins[:n], maxs[:n]


def same_records(got_bytes, spec, shape, what, pix_per_kp=None):
    """(n, 144) bytes in any order against the oracle's records of a frame"""
    got = np.ascontiguousarray(got_bytes).reshape(-1).view(dtype_kp)
    assert_same_keypoints(got, bc.oracle_of(spec, shape, pix_per_kp)[0], what)


def check_minmax(L, bp, specs, shape, what):
    n = len(specs)
    mins, maxs = abi_minmax(L, bp, n)
    for i, s in enumerate(specs):
        mn, mx = bc.oracle_of(s, shape)[1]
        assert (mins[i].tobytes(), maxs[i].tobytes()) == (np.float32(mn).tobytes(), np.float32(mx).tobytes()), \
            "%s: frame %d %r has min / max %r %r, oracle %r %r" % (what, i, s, mins[i], maxs[i], mn, mx)
    abi_minmax(L, bp, n + 1, expect=EINVAL)
    if n > 1:
        abi_minmax(L, bp, n - 1, expect=EINVAL)


def check_handback(L, bp, r, specs, shape, row, what):
    """everything a finished call promises, from the oracle's counts and batch_retire's rule alone"""
    counts = bc.counts_of(specs, shape)
    if row is None:
        row = [(bc.CAP_NULL, bc.NULL_CAP, True)] * len(specs)
    offs, total = bc.expected_offsets(counts, row)
    assert list(r.counts) == counts, "%s: counts %r, oracle %r" % (what, list(r.counts), counts)
    assert list(r.offsets) == offs, "%s: offsets %r, expected %r (counts %r, row %r)" % (what, list(r.offsets), offs, counts, row)
    assert r.total == total and r.overflow == 0, what
    parked = abi_fetch(L, bp, 0, total)
    for i, (s, n, o) in enumerate(zip(specs, counts, offs)):
        w = "%s, frame %d %r" % (what, i, s)
        a = r.arrays[i] if r.arrays is not None else None
        if o < 0:
            same_records(a[:n * RB].reshape(n, RB), s, shape, w + " (delivered)")
            assert (a[n * RB:] == bc.FILL).all(), w + ": written behind its %d records" % n
        else:
            same_records(parked[o:o + n], s, shape, w + " (parked)")
            assert a is None or (a == bc.FILL).all(), w + ": parked, yet its array was written"
    check_minmax(L, bp, specs, shape, what)


# ------------------------------------------------------------------------------------------------ a, b: deliver or park, bookkeeping
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("lanes,n_images", bc.small_ids(), ids=lambda v: str(v))
def test_deliver_or_park(siftlib, lanes, n_images, on_device):
    """Every row of the capacity matrix twice on one handle, then a shorter batch that leaves lanes idle: the frames with a
    non-null array and n <= cap are delivered (offset -1), the others parked at the prefix sums of the parked counts; delivered
    and fetched records are the oracle's; nothing is written behind a delivered frame's records or into a parked frame's array;
    min / max are each frame's own."""
    _, specs, counts, matrix = bc.small_case(lanes).batch(n_images)
    short = bc.shorter_batch(lanes, n_images)
    short_matrix = bc.cap_matrix(bc.counts_of(short, bc.SMALL))
    bp = make_plan(bc.SMALL, lanes)
    keep, addrs = stage(specs, bc.SMALL, on_device)
    keep_s, addrs_s = stage(short, bc.SMALL, on_device)
    for k, row in enumerate(matrix):
        for call in range(2):
            r = abi_batch(siftlib, bp, addrs, on_device, row)
            check_handback(siftlib, bp, r, specs, bc.SMALL, row, "%d lanes, %d frames, row %d, call %d" % (lanes, n_images, k, call))
        srow = short_matrix[(k + 1) % len(short_matrix)]
        r = abi_batch(siftlib, bp, addrs_s, on_device, srow)
        check_handback(siftlib, bp, r, short, bc.SMALL, srow, "%d lanes, %d frames after %d, row %d" % (lanes, len(short), n_images, k))
    # ... and without arrays at all: everything parks
    r = abi_batch(siftlib, bp, addrs, on_device, None)
    check_handback(siftlib, bp, r, specs, bc.SMALL, None, "%d lanes, %d frames, no arrays" % (lanes, n_images))
    del keep, keep_s


@pytest.mark.parametrize("lanes", [1, 3, 5])
def test_wrong_and_empty_batches(siftlib, lanes):
    """n_images = 0 with a null table is a batch of its own: 0 records, nothing of the batch before is left to fetch."""
    n_images = 2 * lanes + 1
    _, specs, counts, _ = bc.small_case(lanes).batch(n_images)
    bp = make_plan(bc.SMALL, lanes)
    keep, addrs = stage(specs, bc.SMALL, False)
    r = abi_batch(siftlib, bp, addrs, False, None)
    check_handback(siftlib, bp, r, specs, bc.SMALL, None, "before the empty batch")
    assert r.total == sum(counts) > 0
    r = abi_batch(siftlib, bp, [], False, None, n_images=0)
    assert r.total == 0 and r.overflow == 0
    assert abi_fetch(siftlib, bp, 0, 0).shape == (0, RB)
    abi_fetch(siftlib, bp, 0, 1, expect=EINVAL)
    abi_minmax(siftlib, bp, 0)
    abi_minmax(siftlib, bp, 1, expect=EINVAL)
    abi_batch(siftlib, bp, addrs, False, None, n_images=-1, expect=EINVAL)
    r = abi_batch(siftlib, bp, addrs, False, None)
    check_handback(siftlib, bp, r, specs, bc.SMALL, None, "after the empty batch")


# ------------------------------------------------------------------------------------------------ c: the arena
def bytes_allocated(L, bp):
    n = C.c_int64(-1)
    assert L.siftmi_batch_info(bp._handle, None, C.byref(n)) == 0
    return n.value


@pytest.mark.parametrize("lanes", bc.ARENA_LANES)
def test_arena_regrows_with_records_parked(siftlib, lanes):
    """Three sparse frames, then five lattice frames: the fifth outgrows the arena's first 4 MiB with more than 20 000 records
    parked (tests/test_batch_cases_host.py replays the rule), and those must come through the copy into the larger arena."""
    warm, main = bc.arena_warmup(lanes), bc.ARENA_MAIN
    ev, cap = bc.arena_replay(bc.counts_of(main, bc.BIG), bc.arena_replay(bc.counts_of(warm, bc.BIG))[1])
    assert len(ev) == 1 and ev[0][1] > 20000
    bp = make_plan(bc.BIG, lanes)
    keep_w, addrs_w = stage(warm, bc.BIG, True)
    keep_m, addrs_m = stage(main, bc.BIG, True)
    r = abi_batch(siftlib, bp, addrs_w, True, None)
    check_handback(siftlib, bp, r, warm, bc.BIG, None, "warm-up, %d lanes" % lanes)
    after_warm = bytes_allocated(siftlib, bp)
    r = abi_batch(siftlib, bp, addrs_m, True, None)
    after_main = bytes_allocated(siftlib, bp)
    print("bytes allocated: %d after the warm-up, %d after the main batch; the rule grows the arena by %d" % (
        after_warm, after_main, cap - bc.ARENA_START))
    check_handback(siftlib, bp, r, main, bc.BIG, None, "main batch, %d lanes" % lanes)
    assert after_main - after_warm >= cap - bc.ARENA_START > 0
    r = abi_batch(siftlib, bp, addrs_m, True, None)
    check_handback(siftlib, bp, r, main, bc.BIG, None, "main batch again, %d lanes" % lanes)
    assert bytes_allocated(siftlib, bp) == after_main
    del keep_w, keep_m


# ------------------------------------------------------------------------------------------------ d: fetch
@pytest.mark.parametrize("form", ["parked", "mixed"])
def test_fetch_ranges(siftlib, form):
    lanes, n_images = 3, 7
    _, specs, counts, matrix = bc.small_case(lanes).batch(n_images)
    row = None if form == "parked" else matrix[0]
    bp = make_plan(bc.SMALL, lanes)
    keep, addrs = stage(specs, bc.SMALL, False)
    r = abi_batch(siftlib, bp, addrs, False, row)
    check_handback(siftlib, bp, r, specs, bc.SMALL, row, form)
    T = r.total
    assert T > 100
    whole = abi_fetch(siftlib, bp, 0, T)                     # (compared with the oracle frame by frame above)
    accepted, refused = bc.fetch_ranges(list(r.offsets), list(r.counts))
    assert len(accepted) >= 3 + sum(o >= 0 for o in r.offsets) + 2
    for first, count in accepted:
        got = abi_fetch(siftlib, bp, first, count)
        assert np.array_equal(got, whole[first:first + count]), "fetch(%d, %d) of %d" % (first, count, T)
    cross = [a for a in accepted if a[1] == 2]
    for first, count in [(0, T), cross[0], (T - 1, 1)]:
        got = abi_fetch(siftlib, bp, first, count, on_device=True)
        assert np.array_equal(got, whole[first:first + count]), "fetch(%d, %d) of %d to the device" % (first, count, T)
    for first, count in refused:
        assert not bc.range_accepted(first, count, T)
        abi_fetch(siftlib, bp, first, count, expect=EINVAL)
        abi_fetch(siftlib, bp, first, count, on_device=True, expect=EINVAL)
    assert siftlib.siftmi_batch_fetch(bp._handle, None, 0, 0, 1) == EINVAL
    assert siftlib.siftmi_batch_fetch(bp._handle, None, 0, T, 0) == 0
    # refusals change nothing
    assert np.array_equal(abi_fetch(siftlib, bp, 0, T), whole)


def test_plan_fetch_ranges(siftlib):
    """siftmi_plan_fetch has the same contract on the records of the plan's last call"""
    import sift_pyocl_amd as sp
    spec = ("lattice", 1)
    plan = sp.SiftPlan(shape=bc.SMALL, dtype=np.float32)
    want = bc.oracle_of(spec, bc.SMALL)[0]
    assert_same_keypoints(plan.keypoints(bc.frame_of(spec, bc.SMALL)), want, "plan")
    T = len(want)

    def fetch(first, count, expect=0):
        room = count if expect == 0 else 4
        host = np.full((room + 2) * RB, bc.FILL, np.uint8)
        rc = siftlib.siftmi_plan_fetch(plan._handle, host.ctypes.data + RB, 0, first, count)
        assert rc == expect, "plan fetch(%d, %d): rc %d" % (first, count, rc)
        assert (host[:RB] == bc.FILL).all() and (host[(room + 1) * RB:] == bc.FILL).all()
        if expect != 0:
            assert (host == bc.FILL).all()
            return None
        return host[RB:(room + 1) * RB].reshape(count, RB)

    whole = fetch(0, T)
    same_records(whole, spec, bc.SMALL, "plan fetch")
    accepted, refused = bc.fetch_ranges([0], [T])
    for first, count in accepted + [(3, 5)]:
        assert np.array_equal(fetch(first, count), whole[first:first + count])
    for first, count in refused:
        fetch(first, count, expect=EINVAL)


# ------------------------------------------------------------------------------------------------ e: recovery
@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("lanes", [1, 3, 5])
def test_failed_call_leaves_nothing_and_the_next_one_is_right(siftlib, lanes, on_device):
    """A null images[k] is found in the middle of the loop, with frames in flight: SIFTMI_EINVAL, the caller's counts and offsets
    untouched, nothing behind a delivered frame's records, no min / max and nothing to fetch afterwards; the same call with the
    frame put back is right."""
    n_images = 2 * lanes + 1
    _, specs, counts, matrix = bc.small_case(lanes).batch(n_images)
    bp = make_plan(bc.SMALL, lanes)
    keep, addrs = stage(specs, bc.SMALL, on_device)
    r = abi_batch(siftlib, bp, addrs, on_device, None)                        # something parked that must not be served later
    check_handback(siftlib, bp, r, specs, bc.SMALL, None, "first")
    for j, k in enumerate(sorted({0, 1, lanes, n_images - 1})):
        row = matrix[j % len(matrix)]
        broken = list(addrs)
        broken[k] = None
        r = abi_batch(siftlib, bp, broken, on_device, row, expect=EINVAL)
        what = "%d lanes, frame %d of %d null" % (lanes, k, n_images)
        assert (r.counts == SENTINEL).all() and (r.offsets == SENTINEL).all(), what
        for i, (a, n) in enumerate(zip(r.arrays, counts)):
            # (a frame before k may have been delivered already: its records and nothing else)
            if a is not None:
                assert (a[min(n, row[i][1]) * RB:] == bc.FILL).all(), what + ": frame %d written behind its records" % i
                assert i < k or (a == bc.FILL).all(), what + ": frame %d written" % i
        abi_minmax(siftlib, bp, n_images, expect=EINVAL)
        abi_minmax(siftlib, bp, 0, expect=EINVAL)
        for first, count in [(0, 1), (0, counts[1] if counts[1] else 1), (1, 1), (0, sum(counts))]:
            abi_fetch(siftlib, bp, first, count, expect=EINVAL)
        assert abi_fetch(siftlib, bp, 0, 0).shape == (0, RB)
        r = abi_batch(siftlib, bp, addrs, on_device, row)
        check_handback(siftlib, bp, r, specs, bc.SMALL, row, what + ", put back")
    del keep


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_refused_call_leaves_the_batch_before(siftlib, on_device):
    """A dtype code that is neither the plan's nor float32 is refused before any state is touched."""
    lanes, n_images = 3, 7
    _, specs, counts, matrix = bc.small_case(lanes).batch(n_images)
    bp = make_plan(bc.SMALL, lanes)
    keep, addrs = stage(specs, bc.SMALL, on_device)
    row = matrix[2]
    r = abi_batch(siftlib, bp, addrs, on_device, row)
    check_handback(siftlib, bp, r, specs, bc.SMALL, row, "before")
    whole, mm = abi_fetch(siftlib, bp, 0, r.total), abi_minmax(siftlib, bp, n_images)
    assert r.total > 0
    for code in (2, 8, 9, -1, 99):                       # uint16 and RGB8 on a float32 plan; no such code
        bad = abi_batch(siftlib, bp, addrs, on_device, row, dtype=code, expect=EINVAL)
        assert (bad.counts == SENTINEL).all() and (bad.offsets == SENTINEL).all()
        assert bad.total == SENTINEL and bad.overflow == SENTINEL
        assert all(a is None or (a == bc.FILL).all() for a in bad.arrays)
        assert np.array_equal(abi_fetch(siftlib, bp, 0, r.total), whole)
        again = abi_minmax(siftlib, bp, n_images)
        assert again[0].tobytes() == mm[0].tobytes() and again[1].tobytes() == mm[1].tobytes()
    check_minmax(siftlib, bp, specs, bc.SMALL, "after the refused calls")
    del keep


# ------------------------------------------------------------------------------------------------ f: Python
def test_python_host_batches_take_both_paths(siftlib):
    """BatchPlan(lanes=2) delivers into arrays of a guessed capacity: 6400 records on a fresh plan, which the smooth frames fit
    and the lattice frames do not; after a batch of blank frames the guess is 257 and everything parks."""
    mixed, blank = bc.PY_MIXED, bc.PY_BLANK
    counts = bc.counts_of(mixed, bc.BIG)
    assert min(counts) <= bc.PY_FIRST_GUESS < max(counts)
    assert [c > bc.PY_FIRST_GUESS for c in counts] == [False, True, False, True]
    bp = make_plan(bc.BIG, 2)
    assert int(1.5 * bp._records_per_frame) + 256 == bc.PY_FIRST_GUESS
    for step, specs in enumerate((mixed, blank, mixed)):
        got = bp.keypoints_batch([bc.frame_of(s, bc.BIG) for s in specs])
        assert len(got) == len(specs)
        for i, (g, s) in enumerate(zip(got, specs)):
            assert_same_keypoints(g, bc.oracle_of(s, bc.BIG)[0], "step %d frame %d %r" % (step, i, s))
        if step == 1:
            assert int(1.5 * bp._records_per_frame) + 256 == 257 < min(counts)
        mins, maxs = bp.minmax_batch()
        for i, s in enumerate(specs):
            mn, mx = bc.oracle_of(s, bc.BIG)[1]
            assert (mins[i].tobytes(), maxs[i].tobytes()) == (np.float32(mn).tobytes(), np.float32(mx).tobytes())


def test_python_device_batches(siftlib):
    import torch
    mixed, blank = bc.PY_MIXED, bc.PY_BLANK
    bp = make_plan(bc.BIG, 3)
    for step, specs in enumerate((mixed, blank, mixed)):
        dev = [torch.from_numpy(bc.frame_of(s, bc.BIG).copy()).cuda() for s in specs]
        counts, records = bp.keypoints_batch_device(dev)
        want = bc.counts_of(specs, bc.BIG)
        assert counts == want, "step %d" % step
        assert records.is_cuda and records.numel() == sum(want) * RB
        host = records.cpu().numpy()
        at = 0
        for i, (s, n) in enumerate(zip(specs, counts)):
            same_records(host[at * RB:(at + n) * RB].reshape(n, RB), s, bc.BIG, "step %d frame %d %r" % (step, i, s))
            at += n


# ------------------------------------------------------------------------------------------------ g: the overflow flag
@pytest.mark.parametrize("lanes", [2, 3])
def test_overflow_flag_wherever_the_flagged_frame_lies(siftlib, lanes):
    ppk = bc.OVERFLOW_PIX_PER_KP
    bp = make_plan(bc.MID, lanes, PIX_PER_KP=ppk)

    def run(specs, flag, what):
        keep, addrs = stage(specs, bc.MID, True)
        r = abi_batch(siftlib, bp, addrs, True, None)
        assert r.overflow == flag, "%s: overflow %d" % (what, r.overflow)
        assert r.total == sum(r.counts)
        parked = abi_fetch(siftlib, bp, 0, r.total)
        at = 0
        for i, s in enumerate(specs):
            n = int(r.counts[i])
            assert r.offsets[i] == at
            if not bc.oracle_of(s, bc.MID, ppk)[2]:
                same_records(parked[at:at + n], s, bc.MID, "%s, frame %d %r" % (what, i, s), ppk)
            else:
                assert 0 < n <= bp.octave_max * bp.kpsize
            at += n

    for name, specs in bc.overflow_batches():
        run(specs, 1, "%d lanes, flagged frame %s" % (lanes, name))
        run(bc.OVERFLOW_PLAIN, 0, "%d lanes, no flagged frame after %s" % (lanes, name))
