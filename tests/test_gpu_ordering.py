"""The ordering contract of every entry point that takes a device pointer (include/siftmi.h, conventions), on the MI355X: a device
pointer is read and written only after everything the caller had enqueued on ANY stream of the process before the call, and host
and device results are complete when the call returns.  The cases, the references' expected values and the late-producer harness
are tests/ordering_cases.py; tests/test_ordering_cases_host.py shows on the CPU that every case can tell real from decoy.

  * control   the harness sees a missing synchronisation: unsynchronised clones on four fresh streams, no library call
  * RAW       every input device pointer, one at a time and all together: the argument is produced late on a side stream
  * WAW       every output device pointer: a late producer fills it with a sentinel, the call must write after it
  * complete  the out="device" forms: the result is read on a fresh stream straight after the return.  This one is the WEAKER
              check: the window a missing final hipStreamSynchronize would leave is as short as the last kernel, so it can pass
              by luck.  RAW and WAW cannot: their window is a delay of ten call times, asserted open when the call is made.

Every racing case runs twice, with the producer on each of two side streams that were created one after the other (at most one
of them shares a hardware queue with the library's stream), prints its call time and delay, and asserts that the producer was
still running when the call was made.  Every racing read is a read of allocated, initialised memory holding a valid input.
"""
import ctypes as C

import numpy as np
import pytest

import match_batch_ref as mb
import ordering_cases as oc
import stack_cases as sc
from stack_ref import stack_ref
from util import dtype_kp

pytestmark = pytest.mark.gpu
F = np.float32
_objects = {}


def shared(key, make):
    """one plan / matcher per kind for the whole module"""
    if key not in _objects:
        _objects[key] = make()
    return _objects[key]


def plan(dtype=np.float32):
    import sift_pyocl_amd as sp
    return shared(("plan", np.dtype(dtype).name), lambda: sp.SiftPlan(shape=oc.FRAME, dtype=dtype))


def batch(lanes, shape=oc.FRAME):
    from sift_pyocl_amd.batch import BatchPlan
    return shared(("batch", lanes, shape), lambda: BatchPlan(shape=shape, dtype=np.float32, lanes=lanes))


def matcher():
    import sift_pyocl_amd as sp
    return shared("matcher", lambda: sp.MatchPlan())


def is_tensor(v):
    return hasattr(v, "data_ptr")


def address(v):
    return (v.data_ptr(), 1) if is_tensor(v) else (v.ctypes.data, 0)


def check(siftlib, rc):
    assert rc == 0, (rc, siftlib.siftmi_last_error())


# --------------------------------------------------------------------------------------------------------- raw C ABI callers
# (new ones: the helpers of the other test modules synchronise the device themselves, which is what must not happen here)
def raw_batch_keypoints(siftlib, bp, frames):
    """siftmi_batch_keypoints + siftmi_batch_fetch to the host: [records of frame i]"""
    n = len(frames)
    ptrs = (C.c_void_p * n)(*[address(f)[0] for f in frames])
    counts, offsets = (C.c_int64 * n)(), (C.c_int64 * n)()
    total, ovf = C.c_int64(0), C.c_int32(0)
    check(siftlib, siftlib.siftmi_batch_keypoints(bp._handle, ptrs, n, 0, address(frames[0])[1], counts, offsets, C.byref(total), C.byref(ovf)))
    flat = np.empty(total.value, dtype_kp)
    if total.value:
        check(siftlib, siftlib.siftmi_batch_fetch(bp._handle, flat.ctypes.data, 0, 0, total.value))
    return [flat[offsets[i]:offsets[i] + counts[i]] for i in range(n)], int(total.value)


def raw_transform(siftlib, image, out):
    M, off, ms = np.array(oc.WARP_M, F), np.array(oc.WARP_OFF, F), C.c_double(0)
    (ip, idev), (op, odev) = address(image), address(out)
    check(siftlib, siftlib.siftmi_plan_transform(plan()._handle, ip, idev, 1, op, odev, oc.FRAME[1], oc.FRAME[0], M.ctypes.data,
                                                 off.ctypes.data, C.c_float(oc.WARP_FILL), 1, C.byref(ms)))


def warp_table(n):
    return np.ascontiguousarray(np.tile(np.array(oc.WARP_M + oc.WARP_OFF, F), (n, 1))), np.full(n, oc.WARP_FILL, F)


def raw_batch_transform(siftlib, frames, out):
    n = len(frames)
    ptrs = (C.c_void_p * n)(*[address(f)[0] for f in frames])
    maps, fills = warp_table(n)
    ms = C.c_double(0)
    check(siftlib, siftlib.siftmi_batch_transform(batch(1)._handle, ptrs, n, address(frames[0])[1], 1, address(out)[0], address(out)[1],
                                                  oc.FRAME[1], oc.FRAME[0], maps.ctypes.data, fills.ctypes.data, 1, C.byref(ms)))


def raw_stack(siftlib, frames, maps, fills, out, cov, reduce):
    n = len(frames)
    ptrs = (C.c_void_p * max(n, 1))(*[address(f)[0] for f in frames])
    table = np.zeros((max(n, 1), 6), F)
    for s, (M, off) in enumerate(maps):
        table[s, :4], table[s, 4:] = M, off
    fills = np.ascontiguousarray(np.concatenate([np.asarray(fills, F).reshape(-1), np.zeros(1, F)]))
    ms = C.c_double(0)
    bp = batch(1, sc.SHAPE)
    check(siftlib, siftlib.siftmi_batch_stack(bp._handle, ptrs, n, address(frames[0])[1] if n else 0, address(out)[0], address(cov)[0],
                                              address(out)[1], oc.STACK_OUT[1], oc.STACK_OUT[0], table.ctypes.data, fills.ctypes.data, 1,
                                              bp.STACK_REDUCERS[reduce], C.c_float(oc.STACK_EMPTY), C.byref(ms)))


def counts_array(c):
    return None if c is None else np.ascontiguousarray(c, np.int64)


def raw_match_batch(siftlib, case, pairs, window):
    """siftmi_match_batch / siftmi_match_window_batch with host lists and `pairs` where it lies; returns pair_counts"""
    kp1, kp2 = case.inputs["kp1"].real, case.inputs["kp2"].real
    c1, c2 = counts_array(case.counts1), counts_array(case.counts2)
    pc = np.zeros(len(c2), np.int64)
    head = (matcher()._handle, kp1.ctypes.data, len(kp1), 0, kp2.ctypes.data, len(kp2), 0, len(c2), None if c1 is None else c1.ctypes.data,
            c2.ctypes.data, C.c_float(mb.threshold()))
    if window:
        shifts = np.ascontiguousarray(np.tile(np.array(oc.WINDOW_SHIFT, F), (len(c2), 1)))
        check(siftlib, siftlib.siftmi_match_window_batch(*head, C.c_float(oc.WINDOW), C.c_float(oc.WINDOW), shifts.ctypes.data, 0, 0,
                                                         address(pairs)[0], address(pairs)[1], pc.ctypes.data))
    else:
        check(siftlib, siftlib.siftmi_match_batch(*head, 0, 0, address(pairs)[0], address(pairs)[1], pc.ctypes.data))
    return pc


def raw_consensus_batch(siftlib, b, vals, mask):
    """siftmi_match_consensus_batch on the batch `b` with the lists and pairs of `vals` (arrays or tensors) and `mask` where it lies"""
    S = b.S
    c1, c2, pc = counts_array(b.counts1), counts_array(b.counts2), counts_array(b.pair_counts)
    models, winners, votes, ms = np.empty((S, 6), F), np.empty(S, np.int32), np.empty(S, np.int32), C.c_double(0)
    (p1, d1), (p2, d2), (pp, dp) = address(vals["kp1"]), address(vals["kp2"]), address(vals["pairs"])
    check(siftlib, siftlib.siftmi_match_consensus_batch(
        matcher()._handle, p1, len(b.kp1), d1, p2, len(b.kp2), d2, S, None if c1 is None else c1.ctypes.data, c2.ctypes.data, pp,
        len(b.pairs), dp, pc.ctypes.data, oc.N_HYP, C.c_float(oc.TOL), oc.SEED, address(mask)[0], address(mask)[1], models.ctypes.data,
        winners.ctypes.data, votes.ctypes.data, None, None, C.byref(ms)))
    return models, votes


# ------------------------------------------------------------------------------------------------- the callers of the RAW cases
def records_of(k):
    return oc.canon_records(np.asarray(k))


def frames_of(case, v):
    """the frames of a batch case: the ready ones where the late one lies (a batch is all host or all device)"""
    if not is_tensor(v["last"]):
        return list(case.ready) + [v["last"]]
    if "ready_dev" not in case.__dict__:
        case.ready_dev = [oc.to_device(f) for f in case.ready]
    return case.ready_dev + [v["last"]]


def call_batch_device(case, v):
    import torch
    counts, rec = batch(3).keypoints_batch_device(frames_of(case, v))
    torch.cuda.synchronize()
    flat = rec.cpu().numpy().view(dtype_kp)
    edges = np.concatenate([[0], np.cumsum(counts)])
    return [records_of(flat[edges[i]:edges[i + 1]]) for i in range(len(counts))]


def call_stack(case, v):
    frames = frames_of(case, v)
    plane, cov = batch(1, sc.SHAPE).stack_batch(frames, [m for m, _ in case.maps], [o for _, o in case.maps], case.fills,
                                                out_shape=oc.STACK_OUT, reduce=case.reduce, empty=oc.STACK_EMPTY, coverage=True)
    return [np.array(plane), np.array(cov)]


def call_transform(siftlib, v):
    out = np.full(oc.FRAME, -77.0, F)
    raw_transform(siftlib, v["image"], out)
    return [out]


def call_batch_transform(v):
    maps, _ = warp_table(3)
    return [np.array(batch(1).transform_batch([v["f0"], v["f1"], v["f2"]], maps[:, :4], maps[:, 4:], fills=oc.WARP_FILL))]


def call_consensus(v):
    mask, model, votes = matcher().consensus(v["kp1"], v["kp2"], v["pairs"], oc.N_HYP, oc.TOL, oc.SEED)
    return [mask.view(np.uint8), np.full(6, np.nan, F) if model is None else model, np.array([votes], np.int32)]


def call_shift(v):
    _, n, raw = matcher().shift(v["kp1"], v["kp2"], v["pairs"], mask=v["mask"], return_ranks=True)
    return [raw, np.array([n, 0], np.int64)]


def call_shift_batch(b, v):
    _, n, raw = matcher().shift_batch(v["kp1"], b.counts1, v["kp2"], b.counts2, v["pairs"], b.pair_counts, mask=v["mask"], return_ranks=True)
    return [raw, np.stack([n, np.zeros_like(n)], axis=1)]


def call_consensus_batch(b, v):
    mask, models, votes = matcher().consensus_batch(v["kp1"], b.counts1, v["kp2"], b.counts2, v["pairs"], b.pair_counts, oc.N_HYP, oc.TOL, oc.SEED)
    return [mask.view(np.uint8), models, votes]


def caller_of(siftlib, case):
    """v -> canonical result: through the Python methods where they take tensors, through the C ABI for the arguments they never
    pass as device pointers"""
    name, mp = case.name, matcher()
    W, WS = oc.WINDOW, oc.WINDOW_SHIFT
    table = {
        "plan_keypoints": lambda v: [records_of(plan().keypoints(v["image"]))],
        "plan_keypoints[uint16]": lambda v: [records_of(plan(np.uint16).keypoints(v["image"]))],
        "batch_keypoints": lambda v: [records_of(k) for k in raw_batch_keypoints(siftlib, batch(3), frames_of(case, v))[0]],
        "batch_keypoints_into[lanes=1]": lambda v: [records_of(k) for k in batch(1).keypoints_batch(frames_of(case, v))],
        "batch_keypoints_into[lanes=3]": lambda v: [records_of(k) for k in batch(3).keypoints_batch(frames_of(case, v))],
        "batch_keypoints_into[device]": lambda v: call_batch_device(case, v),
        "plan_transform": lambda v: call_transform(siftlib, v),
        "batch_transform": call_batch_transform,
        "batch_stack[mean]": lambda v: call_stack(case, v),
        "batch_stack[median]": lambda v: call_stack(case, v),
        "match": lambda v: [oc.canon_rows(mp.match(v["kp1"], v["kp2"], raw_results=True))],
        "match_window": lambda v: [oc.canon_rows(mp.match(v["kp1"], v["kp2"], raw_results=True, window=W, window_shift=WS))],
        "match_knn[l1]": lambda v: list(mp.knn(v["kp1"], v["kp2"], 3, "l1")),
        "match_knn[l2]": lambda v: list(mp.knn(v["kp1"], v["kp2"], 3, "l2")),
        "match_knn_window": lambda v: list(mp.knn_window(v["kp1"], v["kp2"], 3, "l2", W, WS)),
        "match_consensus": call_consensus,
        "match_fit": lambda v: [matcher().fit(v["kp1"], v["kp2"], v["pairs"], mask=v["mask"], return_moments=True)[3]],
        "match_shift": call_shift,
    }
    if name in table:
        return table[name]
    if name.startswith("match_batch"):
        return lambda v: list(mp.match_batch(v["kp1"], case.counts1, v["kp2"], case.counts2))
    if name.startswith("match_window_batch"):
        return lambda v: list(mp.match_window_batch(v["kp1"], case.counts1, v["kp2"], case.counts2, W, WS))
    b = case.batch
    return {"match_fit_batch": lambda v: [mp.fit_batch(v["kp1"], b.counts1, v["kp2"], b.counts2, v["pairs"], b.pair_counts, mask=v["mask"],
                                                        return_moments=True)[3]],
            "match_shift_batch": lambda v: call_shift_batch(b, v),
            "match_consensus_batch": lambda v: call_consensus_batch(b, v)}[name]


# ------------------------------------------------------------------------------------------------------------ the two races
def race_inputs(what, call, items, want):
    """RAW: `call` must return `want` although the tensors of `items` [(tensor, real, decoy)] get their real contents late"""
    assert oc.same(call(), want), "%s: wrong result on ready inputs" % what
    call_ms = oc.timed(call)
    delay = oc.delay_for(call_ms)
    print("%s: call %.3f ms, delay %.1f ms" % (what, call_ms, delay))
    for k, stream in enumerate(oc.side_streams()):
        done = oc.late_many(items, stream, delay)
        oc.window_open(done, what)
        got = call()
        assert oc.same(got, want), "%s, producer on side stream %d: the call read an input before the caller's stream had written it" % (what, k)
        assert done.query(), "%s, side stream %d: the call returned a result while its input was still being produced" % (what, k)


def race_outputs(what, call, outs, read, want):
    """WAW: outs = [(tensor, sentinel array)]; after `call` and a full synchronisation read() must be `want`, not the sentinel
    that a late producer writes into every output tensor"""
    import torch
    call()
    torch.cuda.synchronize()
    assert oc.same(read(), want), "%s: wrong result without a producer" % what
    call_ms = oc.timed(call)
    delay = oc.delay_for(call_ms)
    print("%s: call %.3f ms, delay %.1f ms" % (what, call_ms, delay))
    for k, stream in enumerate(oc.side_streams()):
        done = oc.late_many([(t, s, np.zeros_like(s)) for t, s in outs], stream, delay)
        oc.window_open(done, what)
        call()
        early = not done.query()
        torch.cuda.synchronize()
        assert oc.same(read(), want), "%s, producer on side stream %d: the call wrote its output before the caller's stream had, the late fill landed on top of the result" % (what, k)
        assert not early, "%s, side stream %d: the call returned while the caller's stream was still writing the output" % (what, k)


def sentinel(shape, dtype):
    return np.full(shape, {"f": -12345.0, "i": 0x5a5a5a5a, "u": 0x5a}[np.dtype(dtype).kind], dtype)


def host(t):
    return t.cpu().numpy()


# -------------------------------------------------------------------------------------------------------------------- control
def test_control_unsynchronised_clones_see_the_decoy(siftlib):
    """No library call: the same late() producer, and in place of the call an unsynchronised clone() on each of four freshly
    created streams.  At least one clone must hold the decoy -- otherwise the harness could not see a missing synchronisation
    on this machine and every other test of this module would prove nothing."""
    import torch
    inp = oc.cases()["plan_keypoints"].inputs["image"]
    tensor = oc.to_device(inp.decoy)
    fresh = [torch.cuda.Stream() for _ in range(4)]
    for s in fresh:                                  # the allocator's pool of each stream holds a block: clone() allocates nothing
        with torch.cuda.stream(s):
            warm = torch.empty_like(tensor)
            del warm
    done = oc.late(tensor, inp.real, inp.decoy, oc.side_streams()[0], oc.MIN_DELAY_MS)
    oc.window_open(done, "control")
    clones = []
    for s in fresh:
        with torch.cuda.stream(s):
            clones.append(tensor.clone())
    still_open = not done.query()
    torch.cuda.synchronize()
    stale = [bool(np.array_equal(host(c), inp.decoy)) for c in clones]
    print("control: clones that hold the decoy: %s, window still open after the clones were issued: %s" % (stale, still_open))
    assert np.array_equal(host(tensor), inp.real)
    assert any(stale), "no unsynchronised clone saw the decoy: the harness cannot see a missing synchronisation here"


# ------------------------------------------------------------------------------------------------------------------------ RAW
@pytest.mark.parametrize("item", oc.case_variants(), ids=oc.variant_id)
def test_raw_late_input(siftlib, item):
    import torch
    name, late = item
    case = oc.cases()[name]
    if name == "plan_keypoints[noncontiguous]":
        return noncontiguous_frame(case)
    want = oc.expected(case)
    call_with = caller_of(siftlib, case)
    vals = case.values()
    for a in late:
        vals[a] = oc.to_device(case.inputs[a].real)
    torch.cuda.synchronize()
    race_inputs(oc.variant_id(item), lambda: call_with(vals), [(vals[a], case.inputs[a].real, case.inputs[a].decoy) for a in late], want)


def noncontiguous_frame(case):
    """The late producer is the .contiguous() of plan._pointer_of itself: the caller's current stream is the side stream, which is
    still busy with the delay when keypoints() is given a transposed view.  The pointer handed over is the fresh contiguous copy;
    the block it lands in held the decoy (the stream's allocator pool hands the block that was just freed out again)."""
    import torch
    inp, what = case.inputs["image"], case.name
    want = oc.expected(case)
    base = oc.to_device(np.ascontiguousarray(inp.real.T))
    view = base.t()
    assert not view.is_contiguous() and tuple(view.shape) == oc.FRAME
    p = plan()
    torch.cuda.synchronize()
    assert oc.same([records_of(p.keypoints(view))], want), "%s: wrong result on ready inputs" % what
    call_ms = oc.timed(lambda: p.keypoints(view))
    delay = oc.delay_for(call_ms)
    print("%s: call %.3f ms, delay %.1f ms" % (what, call_ms, delay))
    for k, stream in enumerate(oc.side_streams()):
        decoy = oc.to_device(inp.decoy)
        with torch.cuda.stream(stream):
            block = torch.empty_like(decoy)
            block.copy_(decoy)
        torch.cuda.synchronize()
        del block
        gate = torch.cuda.Event()
        with torch.cuda.stream(stream):
            oc.enqueue_delay(stream, delay)
            gate.record(stream)
            oc.window_open(gate, what)
            got = p.keypoints(view)
        assert oc.same([records_of(got)], want), "%s, side stream %d: the frame was read before .contiguous() had written it" % (what, k)
        assert gate.query()


# ------------------------------------------------------------------------------------------------------------------------ WAW
def test_waw_plan_transform(siftlib):
    import torch
    img = oc.cases()["plan_transform"].inputs["image"].real
    out = torch.zeros(oc.FRAME, dtype=torch.float32, device="cuda")
    race_outputs("waw plan_transform out", lambda: raw_transform(siftlib, img, out), [(out, sentinel(oc.FRAME, F))], lambda: [host(out)],
                 oc.expected(oc.cases()["plan_transform"]))


def test_waw_batch_transform(siftlib):
    import torch
    case = oc.cases()["batch_transform"]
    frames = [case.inputs[a].real for a in case.inputs]
    out = torch.zeros((3,) + oc.FRAME, dtype=torch.float32, device="cuda")
    race_outputs("waw batch_transform out", lambda: raw_batch_transform(siftlib, frames, out), [(out, sentinel(out.shape, F))],
                 lambda: [host(out)], oc.expected(case))


@pytest.mark.parametrize("frames", [oc.STACK_S, 0], ids=["S5", "S0-fill"])
def test_waw_batch_stack(siftlib, frames):
    """`out` and `coverage`; S = 0 is the path where the reduction kernel launched over no frame is the fill"""
    import torch
    case = oc.cases()["batch_stack[mean]"]
    imgs = (list(case.ready) + [case.inputs["last"].real])[:frames]
    want = list(stack_ref(imgs, case.maps[:frames], case.fills[:frames], sc.SHAPE, oc.STACK_OUT, 1, "mean", oc.STACK_EMPTY))
    out = torch.zeros(oc.STACK_OUT, dtype=torch.float32, device="cuda")
    cov = torch.zeros(oc.STACK_OUT, dtype=torch.int32, device="cuda")
    if frames == 0:
        assert (want[0] == F(oc.STACK_EMPTY)).all() and (want[1] == 0).all()
    race_outputs("waw batch_stack out+coverage S=%d" % frames, lambda: raw_stack(siftlib, imgs, case.maps[:frames], case.fills[:frames], out, cov, "mean"),
                 [(out, sentinel(oc.STACK_OUT, F)), (cov, sentinel(oc.STACK_OUT, np.int32))], lambda: [host(out), host(cov)], want)


def test_waw_plan_keypoints_and_fetch(siftlib):
    """siftmi_plan_keypoints with out_is_device = SIFTMI_OUT_DEVICE, and siftmi_plan_fetch into a device buffer"""
    import torch
    case = oc.cases()["plan_keypoints"]
    img, want = case.inputs["image"].real, oc.expected(case)
    n_want = len(want[0])
    out = torch.zeros((n_want + 8) * 144, dtype=torch.uint8, device="cuda")
    p = plan()

    def keypoints(to_out):
        n, ovf = C.c_int64(0), C.c_int32(0)
        check(siftlib, siftlib.siftmi_plan_keypoints(p._handle, img.ctypes.data, 0, 0, out.data_ptr() if to_out else None, int(to_out),
                                                     n_want + 8 if to_out else 0, C.byref(n), C.byref(ovf)))
        assert n.value == n_want
        return n.value

    def read():
        return [records_of(host(out)[:n_want * 144].view(dtype_kp))]

    fill = sentinel((n_want + 8) * 144, np.uint8)
    race_outputs("waw plan_keypoints out", lambda: keypoints(True), [(out, fill)], read, want)
    keypoints(False)                                 # count only: the records stay on the device for the fetch
    race_outputs("waw plan_fetch out", lambda: check(siftlib, siftlib.siftmi_plan_fetch(p._handle, out.data_ptr(), 1, 0, n_want)),
                 [(out, fill)], read, want)


def test_waw_batch_fetch(siftlib):
    """the device result of siftmi_batch_keypoints[_into]: siftmi_batch_fetch into a device buffer (keypoints_batch_device)"""
    import torch
    case = oc.cases()["batch_keypoints"]
    frames = list(case.ready) + [case.inputs["last"].real]
    bp = batch(3)
    per_frame, total = raw_batch_keypoints(siftlib, bp, frames)
    assert oc.same([records_of(k) for k in per_frame], oc.expected(case))
    want = [records_of(np.concatenate(per_frame))]
    out = torch.zeros(total * 144, dtype=torch.uint8, device="cuda")
    race_outputs("waw batch_fetch out", lambda: check(siftlib, siftlib.siftmi_batch_fetch(bp._handle, out.data_ptr(), 1, 0, total)),
                 [(out, sentinel(total * 144, np.uint8))], lambda: [records_of(host(out).view(dtype_kp))], want)


@pytest.mark.parametrize("name", ["match_batch[own]", "match_batch[shared]", "match_window_batch[own]", "match_window_batch[shared]"])
def test_waw_match_batch_pairs(siftlib, name):
    import torch
    case = oc.cases()[name]
    want_pairs, want_counts = oc.expected(case)
    n1, S = len(case.inputs["kp1"].real), len(case.counts2)
    rows = n1 * S if case.counts1 is None else n1
    pairs = torch.zeros((rows, 2), dtype=torch.int32, device="cuda")
    state = {}

    def call():
        state["pc"] = raw_match_batch(siftlib, case, pairs, name.startswith("match_window"))

    race_outputs("waw %s pairs" % name, call, [(pairs, sentinel((rows, 2), np.int32))],
                 lambda: [host(pairs)[:len(want_pairs)], state["pc"]], [want_pairs, want_counts])


@pytest.mark.parametrize("form", ["mask-only", "all-device", "no-launch"])
def test_waw_consensus_batch_mask(siftlib, form):
    """the device mask: with only the mask on the device (the second place the entry point synchronises at), with every pointer
    on the device, and on the path where no segment has three pairs and the mask is cleared by a memset"""
    import torch
    import consensus_batch_ref as cbr
    if form == "no-launch":
        b = oc.sparse_batch()
        r = cbr.consensus_batch(b, oc.N_HYP, oc.TOL, oc.SEED)
        want = [r["mask"], r["models"], r["winner_votes"]]
        assert not r["mask"].any()
    else:
        b = oc.cases()["match_consensus_batch"].batch
        want = oc.expected(oc.cases()["match_consensus_batch"])
    vals = dict(kp1=b.kp1, kp2=b.kp2, pairs=b.pairs)
    if form == "all-device":
        vals = {k: oc.to_device(v) for k, v in vals.items()}
    mask = torch.zeros(len(b.pairs), dtype=torch.uint8, device="cuda")
    state = {}

    def call():
        state["models"], state["votes"] = raw_consensus_batch(siftlib, b, vals, mask)

    race_outputs("waw consensus_batch mask, %s" % form, call, [(mask, sentinel(len(b.pairs), np.uint8))],
                 lambda: [host(mask), state["models"], state["votes"]], want)


# ------------------------------------------------------------------------------------------------- complete on return (weaker)
def read_on_fresh_stream(make, shapes_dtypes):
    """make() -> device tensors; they are copied to pinned host buffers on a stream created for the purpose, straight after make()
    returns and with no other synchronisation.  The buffers and the stream exist before the call (a pinned allocation may
    synchronise the device)."""
    import torch
    bufs = [torch.empty(shape, dtype=dtype, pin_memory=True) for shape, dtype in shapes_dtypes]
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    tensors = make()
    for t, b in zip(tensors, bufs):
        assert tuple(t.shape) == tuple(b.shape) and t.dtype == b.dtype, ("the device result has shape %s, expected %s" % (tuple(t.shape), tuple(b.shape)))
    with torch.cuda.stream(stream):
        for t, b in zip(tensors, bufs):
            b.copy_(t, non_blocking=True)
    stream.synchronize()
    return [b.numpy().copy() for b in bufs]


def test_complete_on_return_warps(siftlib):
    """WEAKER check (see the module docstring): pins the final stream synchronisation of the out="device" forms; a missing one
    leaves a window as short as the last kernel, which this read can miss.  The RAW and WAW tests cannot miss theirs."""
    import torch
    case = oc.cases()["batch_transform"]
    frames = [case.inputs[a].real for a in case.inputs]
    maps, _ = warp_table(3)
    got = read_on_fresh_stream(lambda: [batch(1).transform_batch(frames, maps[:, :4], maps[:, 4:], fills=oc.WARP_FILL, out="device")],
                               [((3,) + oc.FRAME, torch.float32)])
    assert oc.same(got, oc.expected(case))
    case = oc.cases()["batch_stack[median]"]
    imgs = list(case.ready) + [case.inputs["last"].real]
    got = read_on_fresh_stream(lambda: list(batch(1, sc.SHAPE).stack_batch(imgs, [m for m, _ in case.maps], [o for _, o in case.maps], case.fills,
                                                                           out_shape=oc.STACK_OUT, reduce="median", empty=oc.STACK_EMPTY,
                                                                           coverage=True, out="device")),
                               [(oc.STACK_OUT, torch.float32), (oc.STACK_OUT, torch.int32)])
    assert oc.same(got, oc.expected(case))


def test_complete_on_return_records(siftlib):
    """WEAKER check: keypoints_batch_device (one lane: the frames retire in input order and nothing is rearranged afterwards)"""
    import torch
    case = oc.cases()["batch_keypoints_into[device]"]
    frames = list(case.ready) + [case.inputs["last"].real]
    want = oc.expected(case)
    state = {}

    def make():
        state["counts"], rec = batch(1).keypoints_batch_device(frames)
        return [rec]

    got = read_on_fresh_stream(make, [((sum(len(w) for w in want) * 144,), torch.uint8)])[0].view(dtype_kp)
    edges = np.concatenate([[0], np.cumsum(state["counts"])])
    assert oc.same([records_of(got[edges[i]:edges[i + 1]]) for i in range(len(frames))], want)


@pytest.mark.parametrize("name", ["match_batch[own]", "match_window_batch[shared]"])
def test_complete_on_return_pairs(siftlib, name):
    """WEAKER check: match_batch / match_window_batch with out="device" """
    import torch
    case = oc.cases()[name]
    want_pairs, want_counts = oc.expected(case)
    v, mp, state = case.values(), matcher(), {}

    def make():
        if name.startswith("match_window"):
            pairs, state["pc"] = mp.match_window_batch(v["kp1"], case.counts1, v["kp2"], case.counts2, oc.WINDOW, oc.WINDOW_SHIFT, out="device")
        else:
            pairs, state["pc"] = mp.match_batch(v["kp1"], case.counts1, v["kp2"], case.counts2, out="device")
        return [pairs]

    got = read_on_fresh_stream(make, [(want_pairs.shape, torch.int32)])
    assert oc.same(got + [state["pc"]], [want_pairs, want_counts])


def test_complete_on_return_mask(siftlib):
    """WEAKER check: consensus_batch with out="device" """
    import torch
    case = oc.cases()["match_consensus_batch"]
    b, v, state = case.batch, case.values(), {}
    want = oc.expected(case)

    def make():
        mask, state["models"], state["votes"] = matcher().consensus_batch(v["kp1"], b.counts1, v["kp2"], b.counts2, v["pairs"], b.pair_counts,
                                                                          oc.N_HYP, oc.TOL, oc.SEED, out="device")
        return [mask]

    got = read_on_fresh_stream(make, [(want[0].shape, torch.uint8)])
    assert oc.same(got + [state["models"], state["votes"]], want)
