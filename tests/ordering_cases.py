"""The ordering contract of the entry points that take device pointers (include/siftmi.h, conventions): the cases and the
late-producer harness that tests/test_ordering_cases_host.py (CPU) and tests/test_gpu_ordering.py (MI355X) share.  Plain helpers,
no fixtures.

The idea.  Every stream of the library is non-blocking, so the one hipDeviceSynchronize() at the head of a call is all that keeps a
kernel of ours from reading data that a stream of the caller is still producing.  A test that hands over finished data cannot see
that synchronisation disappear.  Here a device tensor holds a DECOY -- another valid input of the same shape -- and a side stream
is given a delay followed by the copy of the REAL input; the library call is made while the delay still runs (asserted through an
event).  A call that orders itself after the caller's streams returns the reference's result for the real input; one that does
not reads the decoy and returns the reference's result for that, which every case asserts up front to be different.  For an
output pointer the late producer writes a sentinel instead: a call that does not wait has its result overwritten by it.

Part 1 of this module is numpy only (the cases and what the project's references expect of them); part 2, the harness, imports
torch inside its functions.
"""
import time

import numpy as np

import consensus_batch_ref as cbr
import consensus_ref as cr
import estimate_batch_ref as eb
import fit_ref as fr
import knn_l2_ref
import knn_ref
import knn_window_ref as kwr
import match_batch_ref as mb
import match_window_batch_ref as mwb
import shift_ref as sr
import window_ref as wr
import stack_cases as sc
from stack_ref import stack_ref
from util import smooth_noise, sort_kp
from warp_ref import warp_ref

F = np.float32
FRAME = (97, 131)                      # H, W of the frames of the keypoint and warp cases
N1, N2 = 300, 260                      # records of the two lists (window_ref.crafted)
PAIRS = 500                            # pairs of the estimator cases (fit_ref.make_case)
STACK_S = 5                            # frames of a stack (stack_cases.SHAPE planes); batches of keypoint frames too
SEGMENTS = eb.MASKED_SIZES             # pairs of the three segments of the estimator batches
SEG_LISTS = ((300, 260), (130, 257), (65, 64))      # records of the three segment pairs of the matcher batches
WINDOW, WINDOW_SHIFT = 4.0, (3.5, -2.25)
N_HYP, TOL, SEED = 256, 3.0, 7
WARP_M, WARP_OFF, WARP_FILL = (0.99, 0.02, -0.03, 1.01), (1.7, 4.2), 3.0       # util.TRANSFORM_CASES: the LinearAlign regime
STACK_OUT = (41, 70)
STACK_EMPTY = -5.5


# ====================================================================================================== part 1: the cases
class Input(object):
    """One device-capable input of a case: `real` and `decoy` are numpy arrays of one shape and dtype.  kind: "frame", "records",
    "pairs" (limit: (M, 2) exclusive upper bounds of the two indices of every row) or "mask"."""

    def __init__(self, kind, real, decoy, limit=None):
        self.kind, self.real, self.decoy, self.limit = kind, np.ascontiguousarray(real), np.ascontiguousarray(decoy), limit
        assert self.real.shape == self.decoy.shape and self.real.dtype == self.decoy.dtype

    def valid(self, a):
        """a racing read of `a` is a read of a valid input: finite positions, indices inside their lists, a 0/1 mask"""
        if self.kind == "frame":
            return bool(np.isfinite(a.astype(np.float64)).all())
        if self.kind == "records":
            return all(bool(np.isfinite(a[f]).all()) for f in ("x", "y", "scale", "angle"))
        if self.kind == "pairs":
            return bool((a >= 0).all() and (a < self.limit).all())
        if self.kind == "mask":
            return bool(np.isin(a, (0, 1)).all())
        raise ValueError(self.kind)


class Case(object):
    """name: the entry point and its form.  inputs: {argument: Input}, in the order of the C signature.  expect(values) -> list
    of numpy arrays in canonical form (what `same` compares), from the project's references, for {argument: array}.
    only_all: the case has one variant, every input late (the forms of an entry point beyond its first)."""

    def __init__(self, name, inputs, expect, only_all=False, **extra):
        self.name, self.inputs, self.expect, self.only_all = name, inputs, expect, only_all
        self.__dict__.update(extra)

    def variants(self):
        """tuples of the arguments that are late: each alone, then all of them"""
        names = tuple(self.inputs)
        if self.only_all or len(names) == 1:
            return [names]
        return [(n,) for n in names] + [names]

    def values(self, decoys=()):
        return {n: (i.decoy if n in decoys else i.real) for n, i in self.inputs.items()}


_EXPECTED = {}


def expected(case, decoys=()):
    """the reference's result with the arguments `decoys` replaced by their decoys, computed once"""
    key = (case.name, tuple(sorted(decoys)))
    if key not in _EXPECTED:
        _EXPECTED[key] = [np.ascontiguousarray(a) for a in case.expect(case.values(decoys))]
    return _EXPECTED[key]


def same(got, want):
    """two canonical results are equal: shapes and dtypes, integers and bytes exactly, floats by value with NaN == NaN (the bit
    patterns are pinned by the tests of each entry point; real and decoy differ grossly)"""
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        g, w = np.asarray(g), np.asarray(w)
        if g.shape != w.shape or g.dtype != w.dtype:
            return False
        if g.dtype.kind == "f":
            nan = np.isnan(w)
            if not (np.array_equal(np.isnan(g), nan) and np.array_equal(g[~nan], w[~nan])):
                return False
        elif not np.array_equal(g, w):
            return False
    return True


def canon_records(k):
    """keypoint records in the order of util.sort_kp, as bytes (their order in a result is unspecified)"""
    k = np.asarray(k)
    return np.ascontiguousarray(sort_kp(k)).view(np.uint8).reshape(len(k), 144)


def canon_rows(pairs):
    """(m, 2) int32 rows sorted (siftmi_match appends its pairs through a counter)"""
    return wr.sort_rows(np.asarray(pairs, np.int32).reshape(-1, 2)).astype(np.int32)


# ---------------------------------------------------------------------------------------------- frames
def frame(seed, dtype=np.float32):
    f = smooth_noise(FRAME, seed=seed, sigma=1.5)
    f = (f - f.min()) / (f.max() - f.min())
    if np.dtype(dtype) == np.float32:
        return (f * 255.0).astype(np.float32)
    return (f.astype(np.float64) * np.iinfo(dtype).max * 0.99).astype(dtype)


def oracle_keypoints(img):
    from oracle import pyoracle
    pyoracle.build()
    return pyoracle.keypoints(np.ascontiguousarray(img).astype(np.float32))


def _keypoint_cases():
    out = []
    for name, dtype, seeds in (("plan_keypoints", np.float32, (41, 42)), ("plan_keypoints[uint16]", np.uint16, (43, 44)),
                               ("plan_keypoints[noncontiguous]", np.float32, (45, 46))):
        out.append(Case(name, {"image": Input("frame", frame(seeds[0], dtype), frame(seeds[1], dtype))},
                        lambda v: [canon_records(oracle_keypoints(v["image"]))], dtype=np.dtype(dtype)))
    ready = [frame(50 + s) for s in range(STACK_S - 1)]
    for name in ("batch_keypoints", "batch_keypoints_into[lanes=1]", "batch_keypoints_into[lanes=3]", "batch_keypoints_into[device]"):
        out.append(Case(name, {"last": Input("frame", frame(60), frame(61))},
                        lambda v: [canon_records(oracle_keypoints(f)) for f in ready + [v["last"]]], ready=ready))
    return out


def _warp_cases():
    def one(v):
        return [warp_ref(v["image"], F(WARP_M), F(WARP_OFF), FRAME, WARP_FILL, 1)[0]]

    def many(v):
        return [np.stack([warp_ref(f, F(WARP_M), F(WARP_OFF), FRAME, WARP_FILL, 1)[0] for f in (v["f0"], v["f1"], v["f2"])])]

    out = [Case("plan_transform", {"image": Input("frame", frame(70), frame(71))}, one),
           Case("batch_transform", {"f%d" % s: Input("frame", frame(72 + s), frame(76 + s)) for s in range(3)}, many, only_all=True)]
    real, decoy = sc.frames_of("noise", STACK_S, seed=1), sc.frames_of("noise", STACK_S, seed=2)
    maps, fills = sc.maps_of("shift", STACK_S), sc.fills_of(STACK_S)
    for reduce in ("mean", "median"):
        out.append(Case("batch_stack[%s]" % reduce, {"last": Input("frame", real[-1], decoy[-1])},
                        lambda v, reduce=reduce: list(stack_ref(real[:-1] + [v["last"]], maps, fills, sc.SHAPE, STACK_OUT, 1, reduce,
                                                                STACK_EMPTY)),
                        ready=real[:-1], maps=maps, fills=fills, reduce=reduce))
    return out


# ---------------------------------------------------------------------------------------------- matchers
def _match_cases():
    a, b = wr.crafted(N1, N2, 11, WINDOW_SHIFT)
    da, db = wr.crafted(N1, N2, 12, WINDOW_SHIFT)
    lists = lambda: {"kp1": Input("records", a, da), "kp2": Input("records", b, db)}       # noqa: E731
    return [
        Case("match", lists(), lambda v: [canon_rows(wr.match(v["kp1"], v["kp2"], np.inf))]),
        Case("match_window", lists(), lambda v: [canon_rows(wr.match(v["kp1"], v["kp2"], WINDOW, WINDOW_SHIFT))]),
        Case("match_knn[l1]", lists(), lambda v: list(knn_ref.knn(v["kp1"], v["kp2"], 3))),
        Case("match_knn[l2]", lists(), lambda v: list(knn_l2_ref.knn(v["kp1"], v["kp2"], 3))),
        Case("match_knn_window", lists(), lambda v: list(kwr.knn(v["kp1"], v["kp2"], 3, WINDOW, WINDOW_SHIFT, "l2"))),
    ]


def _segment_lists(seed, shared=None):
    rng = np.random.default_rng(seed)
    return [mwb.lists(n1, n2, rng, shift=WINDOW_SHIFT, a=shared) for n1, n2 in SEG_LISTS]


def _match_batch_cases():
    out = []
    for form in ("own", "shared"):
        first = mwb.lists(N1, N2, np.random.default_rng(20), shift=WINDOW_SHIFT)[0] if form == "shared" else None
        dfirst = mwb.lists(N1, N2, np.random.default_rng(21), shift=WINDOW_SHIFT)[0] if form == "shared" else None
        # (a shared decoy list against segments planted on the real one and the other way round: no partners, other pairs)
        real, decoy = mb.Batch(form, _segment_lists(22, first), shared=first), mb.Batch(form, _segment_lists(23, dfirst), shared=dfirst)
        assert real.counts1 == decoy.counts1 and real.counts2 == decoy.counts2
        inputs = lambda: {"kp1": Input("records", real.kp1, decoy.kp1), "kp2": Input("records", real.kp2, decoy.kp2)}       # noqa: E731
        c1, c2 = real.counts1, real.counts2
        out.append(Case("match_batch[%s]" % form, inputs(),
                        lambda v, c1=c1, c2=c2: list(mb.match_batch(v["kp1"], c1, v["kp2"], c2)), counts1=c1, counts2=c2))
        out.append(Case("match_window_batch[%s]" % form, inputs(),
                        lambda v, c1=c1, c2=c2: list(mwb.match_window_batch(v["kp1"], c1, v["kp2"], c2, WINDOW, WINDOW_SHIFT)),
                        counts1=c1, counts2=c2))
    return out


# ---------------------------------------------------------------------------------------------- estimators
def _mask(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.6).astype(np.uint8)


def _consensus_result(r):
    model = np.full(6, np.nan, F) if r["model"] is None else np.asarray(r["model"], F)
    return [np.asarray(r["mask"], np.uint8), model, np.array([r["winner_votes"]], np.int32)]


def _shift_result(r):
    return [np.asarray(r[0], F), np.asarray(r[1], np.int64)]


def _estimator_cases():
    k1, k2, p = fr.make_case(PAIRS, 31)[:3]
    d1, d2, dp = fr.make_case(PAIRS, 32)[:3]
    limit = np.array([len(k1), len(k2)])
    three = lambda: {"kp1": Input("records", k1, d1), "kp2": Input("records", k2, d2), "pairs": Input("pairs", p, dp, limit)}  # noqa: E731
    four = lambda: dict(three(), mask=Input("mask", _mask(PAIRS, 33), _mask(PAIRS, 34)))       # noqa: E731
    return [
        Case("match_consensus", three(), lambda v: _consensus_result(cr.consensus(v["kp1"], v["kp2"], v["pairs"], N_HYP, TOL, SEED))),
        Case("match_fit", four(), lambda v: [fr.fit(v["kp1"], v["kp2"], v["pairs"], v["mask"])]),
        Case("match_shift", four(), lambda v: _shift_result(sr.shift(v["kp1"], v["kp2"], v["pairs"], v["mask"]))),
    ]


def _batch_of(v, like):
    return eb.Batch(like.name, v["kp1"], like.counts1, v["kp2"], like.counts2, v["pairs"], like.pair_counts, v.get("mask"))


def _estimator_batch_cases():
    real = eb.from_segments("real", [eb.case_segment(M, 60 + k) for k, M in enumerate(SEGMENTS)])
    decoy = eb.from_segments("decoy", [eb.case_segment(M, 70 + k) for k, M in enumerate(SEGMENTS)])
    assert (real.counts1 == decoy.counts1).all() and (real.counts2 == decoy.counts2).all()
    limit = np.concatenate([np.tile([[c1, c2]], (pc, 1)) for c1, c2, pc in zip(real.counts1, real.counts2, real.pair_counts)])
    M = len(real.pairs)
    three = lambda: {"kp1": Input("records", real.kp1, decoy.kp1), "kp2": Input("records", real.kp2, decoy.kp2),       # noqa: E731
                     "pairs": Input("pairs", real.pairs, decoy.pairs, limit)}
    four = lambda: dict(three(), mask=Input("mask", _mask(M, 35), _mask(M, 36)))       # noqa: E731

    def consensus(v):
        r = cbr.consensus_batch(_batch_of(v, real), N_HYP, TOL, SEED)
        return [r["mask"], r["models"], r["winner_votes"]]

    return [
        Case("match_fit_batch", four(), lambda v: [eb.fit_batch(_batch_of(v, real))], batch=real),
        Case("match_shift_batch", four(), lambda v: _shift_result(eb.shift_batch(_batch_of(v, real))[:2]), batch=real),
        Case("match_consensus_batch", three(), consensus, batch=real),
    ]


_CASES = None


def cases():
    """every RAW case, built once: {name: Case}"""
    global _CASES
    if _CASES is None:
        all_cases = (_keypoint_cases() + _warp_cases() + _match_cases() + _match_batch_cases() + _estimator_cases() +
                     _estimator_batch_cases())
        _CASES = {c.name: c for c in all_cases}
        assert len(_CASES) == len(all_cases)
    return _CASES


def case_variants():
    """[(case name, late arguments)] of every RAW test"""
    return [(c.name, v) for c in cases().values() for v in c.variants()]


def variant_id(item):
    return "%s-%s" % (item[0], "+".join(item[1]))


def sparse_batch():
    """consensus_batch's path without a launch: no segment has three pairs, so the mask is cleared where it lies"""
    return eb.from_segments("sparse", [eb.case_segment(M, 80 + k) for k, M in enumerate((2, 0, 1))])


# ====================================================================================================== part 2: the harness
MIN_DELAY_MS = 10.0            # floor of the delay: the interpreter's own time between late() and the library's first read is ~0.1 ms
DELAY_FACTOR = 10.0            # the delay is at least this many times the call's own wall time on ready inputs
_UNIT = None                   # (kind, milliseconds per unit, scratch tensor or None), calibrated once per session
_SIDES = None
_KEEP = []                     # what the producers of the current call read: alive until the next late_many()


def side_streams():
    """Two side streams created one after the other: they land on different hardware queues, so the library's stream can share
    a queue -- and with it an accidental order -- with one of them at most.  Every case runs once with each."""
    global _SIDES
    if _SIDES is None:
        import torch
        _SIDES = [torch.cuda.Stream(), torch.cuda.Stream()]
    return _SIDES


def _elapsed_ms(stream, work):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        a.record(stream)
        work()
        b.record(stream)
    b.synchronize()
    return a.elapsed_time(b)


def delay_unit():
    """The unit of delay, calibrated once with two events on a synchronised stream: a million cycles of torch.cuda._sleep where
    this build has it and it measures sanely, else one element-wise pass over a 64 MB scratch tensor."""
    global _UNIT
    if _UNIT is None:
        import torch
        stream = side_streams()[0]
        if hasattr(torch.cuda, "_sleep"):
            _elapsed_ms(stream, lambda: torch.cuda._sleep(1000000))
            ms = min(_elapsed_ms(stream, lambda: torch.cuda._sleep(1000000)) for _ in range(3))
            if 0.02 <= ms <= 100.0:
                _UNIT = ("sleep", ms, None)
        if _UNIT is None:
            scratch = torch.zeros(16 << 20, dtype=torch.float32, device="cuda")
            _elapsed_ms(stream, lambda: scratch.add_(1.0))
            ms = min(_elapsed_ms(stream, lambda: [scratch.add_(1.0) for _ in range(8)]) for _ in range(3)) / 8.0
            _UNIT = ("passes", ms, scratch)
        print("ordering harness: delay unit %s = %.4f ms" % (_UNIT[0], _UNIT[1]))
    return _UNIT


def enqueue_delay(stream, ms):
    """at least `ms` milliseconds of ordinary torch work on `stream` (to be called with `stream` current)"""
    import torch
    kind, unit_ms, scratch = delay_unit()
    units = ms / unit_ms * 1.25                      # the calibration is a minimum over three: a margin on top
    if kind == "sleep":
        torch.cuda._sleep(int(units * 1000000) + 1)
    else:
        for _ in range(int(units) + 1):
            scratch.add_(1.0)


def to_device(a):
    """a device tensor with the bytes of `a`: records as a flat uint8 tensor (what MatchPlan takes), anything else in its own
    shape and type"""
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype.names:
        a = a.view(np.uint8).reshape(-1)
    return torch.from_numpy(a.copy()).cuda()


def late_many(items, stream, delay_ms):
    """items: [(tensor, real, decoy)].  Every tensor is given its decoy and that state is synchronised; then `stream` gets the
    delay and, behind it, tensor.copy_(real, non_blocking=True) for every item.  Returns the event recorded behind the last copy.
    The caller makes the library call with no synchronisation of any kind in between."""
    import torch
    del _KEEP[:]
    staged = []
    for tensor, real, decoy in items:
        tensor.copy_(to_device(decoy).view_as(tensor))
        staged.append(to_device(real).view_as(tensor))
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    with torch.cuda.stream(stream):
        enqueue_delay(stream, delay_ms)
        for (tensor, _, _), real_dev in zip(items, staged):
            tensor.copy_(real_dev, non_blocking=True)
        done.record(stream)
    _KEEP.extend(staged)
    return done


def late(tensor, real, decoy, stream, delay_ms=MIN_DELAY_MS):
    """`tensor` holds `decoy`, synchronised; `real` arrives on `stream` behind a delay.  Returns the event `done` behind the copy."""
    return late_many([(tensor, real, decoy)], stream, delay_ms)


def window_open(done, what):
    """The assertion made immediately before a racing call: the producer has not finished, so the call is made inside the window.
    A case where this cannot hold proves nothing."""
    assert not done.query(), ("%s: the late producer had finished before the call was made -- the window was not open and this "
                              "case proves nothing (delay too short for this machine?)" % what)


def timed(call):
    """wall time in ms of `call` on ready, synchronised inputs"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    call()
    return (time.perf_counter() - t0) * 1e3


def delay_for(call_ms):
    return max(DELAY_FACTOR * call_ms, MIN_DELAY_MS)
