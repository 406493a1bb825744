"""GPU tests of the streaming stack accumulator: stack_accum_kernel / stack_accum_result_kernel (csrc/k_stack_accum.hpp) through
siftmi_batch_stack_accum, siftmi_batch_stack_accum_result, BatchPlan.stack_accumulator and LinearAlign.stack_stream.

Every crafted stack of tests/stack_cases.py is fed at once, one frame per call and in calls of 3, 4 and 5 frames (the edges of the
depth-4 and depth-2 groups and their tails); the state after EVERY call and the result planes are compared with
tests/stack_accum_ref.py bit for bit (a NaN matches any NaN).  State and result planes lie between guard bytes in one device
buffer.  The stack of the stack_stream tests is tests/stack_accum_cases.py's, where the choice of its noise is written down.
"""
import ctypes as C

import numpy as np
import pytest

import ordering_cases as oc
import stack_accum_cases as ac
import stack_accum_ref as ar
import stack_cases as sc
import stack_ref as sr
import warp_cubic_cases as cc
from warp_ref import same

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 256                                     # bytes
INF = float("inf")
_cache = {}


def batch_plan():
    import sift_pyocl_amd as sp
    if "plan" not in _cache:
        _cache["plan"] = sp.BatchPlan(shape=sc.SHAPE, dtype=F, lanes=1)
    return _cache["plan"]


def table(maps):
    if not len(maps):
        return np.zeros((0, 6), F)
    return np.ascontiguousarray(np.array([tuple(M) + tuple(off) for M, off in maps], F))


def tables(maps):
    t = table(maps)
    return t[:, :4].copy(), t[:, 4:].copy()


def host_pointers(frames):
    return (C.c_void_p * max(1, len(frames)))(*[f.ctypes.data for f in frames])


def device_stack(frames):
    import torch
    whole = torch.from_numpy(np.stack(frames)).cuda()
    step = frames[0].nbytes
    return whole, [whole.data_ptr() + s * step for s in range(len(frames))]


class Guarded(object):
    """Planes between guard bytes in one device buffer.  fields: [(name, dtype)], every plane of `out_shape`; the planes start
    zero-filled, the guards hold 0xa5.  Planes of 8-byte elements come first, so every plane is aligned to its element."""

    def __init__(self, out_shape, fields, fill=0):
        import torch
        self.out_shape, self.fields = tuple(out_shape), [(n, np.dtype(d)) for n, d in fields]
        assert [d.itemsize for _, d in self.fields] == sorted([d.itemsize for _, d in self.fields], reverse=True)
        n = self.out_shape[0] * self.out_shape[1]
        self.at, pos = {}, GUARD
        for name, d in self.fields:
            self.at[name] = (pos, n * d.itemsize, d)
            pos += (n * d.itemsize + 7) // 8 * 8 + GUARD
        host = np.full(pos, 0xa5, np.uint8)
        for start, nbytes, _ in self.at.values():
            host[start:start + nbytes] = fill
        self.buf = torch.from_numpy(host).cuda()
        assert self.buf.data_ptr() % 8 == 0
        torch.cuda.synchronize()

    def ptr(self, name):
        return None if name is None else self.buf.data_ptr() + self.at[name][0]

    def tensor(self, name):
        import torch
        start, nbytes, d = self.at[name]
        return self.buf[start:start + nbytes].view({"float64": torch.float64, "float32": torch.float32, "int32": torch.int32}[d.name]).view(self.out_shape)

    def write(self, name, plane):
        import torch
        self.tensor(name).copy_(torch.from_numpy(np.ascontiguousarray(plane, self.at[name][2])))
        torch.cuda.synchronize()

    def read(self):
        """{name: plane} on the host, after checking that no guard byte changed"""
        host = self.buf.cpu().numpy()
        keep = np.ones(host.shape, bool)
        out = {}
        for name, (start, nbytes, d) in self.at.items():
            keep[start:start + nbytes] = False
            out[name] = host[start:start + nbytes].view(d).reshape(self.out_shape).copy()
            keep[start + nbytes:start + (nbytes + 7) // 8 * 8] = True
        assert (host[keep] == 0xa5).all(), (self.out_shape, "bytes outside the planes were written")
        return out


STATE = [("s1", np.float64), ("s2", np.float64), ("coverage", np.int32), ("kept", np.int32)]
RESULT = [("mean", F), ("var", F)]


def raw_accum(siftlib, g, ptrs, n, is_dev, out_shape, maps, fills, mode=1, interp=0, moments=True, clip=None, kappa=(3.0, 3.0), want_rc=0, over=()):
    """siftmi_batch_stack_accum into the guarded state `g`; clip: (address, address); over: arguments replaced by name; returns kernel_ms"""
    tab = table(maps)
    fills = np.ascontiguousarray(fills, F)
    ms = C.c_double(-1.0)
    a = dict(h=batch_plan()._handle, images=ptrs, n=n, s1=g.ptr("s1"), s2=g.ptr("s2") if moments else None, cov=g.ptr("coverage"), kept=g.ptr("kept"),
             ow=out_shape[1], oh=out_shape[0], maps=tab.ctypes.data, fills=fills.ctypes.data, mode=mode, interp=interp,
             center=clip[0] if clip else None, var=clip[1] if clip else None, kl=kappa[0], kh=kappa[1])
    a.update(dict(over))
    rc = siftlib.siftmi_batch_stack_accum(a["h"], a["images"], a["n"], is_dev, a["s1"], a["s2"], a["cov"], a["kept"], a["ow"], a["oh"], a["maps"], a["fills"],
                                          a["mode"], a["interp"], a["center"], a["var"], C.c_float(a["kl"]), C.c_float(a["kh"]), C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def raw_result(siftlib, g, out_shape, mean_ptr, var_ptr, out_is_dev, empty, moments=True, want_rc=0, **over):
    ms = C.c_double(-1.0)
    a = dict(h=batch_plan()._handle, s1=g.ptr("s1"), s2=g.ptr("s2") if moments else None, kept=g.ptr("kept"), ow=out_shape[1], oh=out_shape[0],
             mean=mean_ptr, var=var_ptr)
    a.update(over)
    rc = siftlib.siftmi_batch_stack_accum_result(a["h"], a["s1"], a["s2"], a["kept"], a["ow"], a["oh"], a["mean"], a["var"], out_is_dev, C.c_float(empty),
                                                 C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def state_is(got, want, moments=True):
    """the planes read from the device are the restatement's, bit for bit (a NaN sum matches any NaN sum)"""
    def same64(a, b):
        nan = np.isnan(b)
        return a.dtype == b.dtype == np.float64 and a.shape == b.shape and np.array_equal(np.isnan(a), nan) and \
            np.array_equal(a.view(np.uint64)[~nan], b.view(np.uint64)[~nan])
    ok = same64(got["s1"], want.s1) and np.array_equal(got["coverage"], want.coverage) and np.array_equal(got["kept"], want.kept)
    if moments:
        return ok and same64(got["s2"], want.s2)
    return ok and (got["s2"] == 0).all()                                 # without second moments the plane is never touched


def prefixes(vals, live, out_shape, clip=None, kappa=(3.0, 3.0)):
    """the restatement's state after every frame: [State] of S + 1 entries (any split of the stack gives these states, which
    tests/test_stack_accum_ref_host.py holds the restatement to)"""
    st = ar.State(out_shape, True)
    out = [st.copy()]
    for s in range(vals.shape[0]):
        st.add_samples(vals[s:s + 1], live[s:s + 1], clip, kappa)
        out.append(st.copy())
    return out


def check_fed_every_way(siftlib, case, vals, live, interp, clip=None, kappa=(3.0, 3.0)):
    S = len(case.frames)
    want = prefixes(vals, live, case.out_shape, clip, kappa)
    hptrs = [f.ctypes.data for f in case.frames]
    whole, dptrs = device_stack(case.frames)
    planes = Guarded(case.out_shape, RESULT, fill=0x11)
    gclip = None
    if clip is not None:
        gclip = Guarded(case.out_shape, [("center", F), ("var", F)])
        gclip.write("center", clip[0]); gclip.write("var", clip[1])
    for k, per_call in enumerate(ac.CALLS):
        moments, is_dev = k % 2 == 0, k % 2
        g = Guarded(case.out_shape, STATE)
        for a, b in ac.splits(S, per_call):
            addrs = (dptrs if is_dev else hptrs)[a:b]
            ms = raw_accum(siftlib, g, (C.c_void_p * (b - a))(*addrs), b - a, is_dev, case.out_shape, case.maps[a:b], case.fills[a:b], case.mode, interp,
                           moments, clip=(gclip.ptr("center"), gclip.ptr("var")) if clip is not None else None, kappa=kappa)
            assert ms > 0.0
            assert state_is(g.read(), want[b], moments), (case.name, per_call, b)
        # the result: device planes between guards, host planes, with and without the variance
        empty = -3.5 if k % 2 else float("nan")
        wmean, wvar = want[S].result(empty=empty, var=True)
        raw_result(siftlib, g, case.out_shape, planes.ptr("mean"), planes.ptr("var") if moments else None, 1, empty, moments)
        got = planes.read()
        assert same(got["mean"], wmean, nan_any_payload=True), (case.name, per_call, "mean")
        if moments:
            assert same(got["var"], wvar, nan_any_payload=True), (case.name, per_call, "var")
        hmean, hvar = np.full(case.out_shape, -77.0, F), np.full(case.out_shape, -78.0, F)
        raw_result(siftlib, g, case.out_shape, hmean.ctypes.data, hvar.ctypes.data if moments else None, 0, empty, moments)
        assert same(hmean, wmean, nan_any_payload=True) and (same(hvar, wvar, nan_any_payload=True) if moments else (hvar == -78.0).all())
        assert state_is(g.read(), want[S], moments)                      # the result reads the state only
    del whole


# ------------------------------------------------------------------------------------------------------ the crafted stacks
def test_the_sizes_the_issue_names_are_there():
    assert {len(c.frames) for c in sc.cases()} >= {1, 2, 3, 4, 5, 8, 64, 200}
    assert {len(c.frames) for c in cubic_cases()} >= {1, 2, 3, 4, 5, 8, 64}


@pytest.mark.parametrize("case", sc.cases(), ids=[c.name for c in sc.cases()])
def test_every_case_fed_every_way_is_the_restatement_bit_for_bit(siftlib, case):
    vals, live = sr.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, case.mode)
    check_fed_every_way(siftlib, case, vals, live, 0)


def cubic_cases():
    """the cubic stacks whose maps reach the clamped columns and rows (frames leaving across an edge, half-pixel shifts) or mix taps"""
    return [c for c in cc.stack_cases() if c.family in ("leaving", "half", "rot") and len(c.frames) <= 64]


@pytest.mark.parametrize("case", cubic_cases(), ids=lambda c: c.name)
def test_the_cubic_instances_are_the_restatement_bit_for_bit(siftlib, case):
    import warp_cubic_ref as wcr
    vals, live = wcr.samples_cubic(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape)
    check_fed_every_way(siftlib, case, vals, live, 1)


@pytest.mark.parametrize("name,interp", [("noise-leaving-S8-41x70-m1", 0), ("zinger-shift-S64-41x70-m1", 0), ("noise-rot-S5-41x70-m1", 1),
                                         ("nan-shift-S8-41x70-m1", 0), ("noise-half-S5-41x70-m0", 0)])
def test_a_clip_fed_every_way_is_the_restatement_bit_for_bit(siftlib, name, interp):
    case = {c.name: c for c in sc.cases()}[name]
    vals, live = ar.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, case.mode, "cubic" if interp else None)
    first = ar.State(case.out_shape, True).add_samples(vals, live)
    center, var = first.result(var=True)                                 # NaN where nothing is live: rejects nothing there
    kappa = (1.0, 1.5)
    clipped = ar.State(case.out_shape, True).add_samples(vals, live, (center, var), kappa)
    if case.kind != "nan":
        assert 0 < (clipped.kept < clipped.coverage).sum() and (clipped.kept > 0).sum() > 100
    check_fed_every_way(siftlib, case, vals, live, interp, clip=(center, var), kappa=kappa)


def test_the_clips_edges_on_crafted_planes(siftlib):
    """identity maps and the nearest-lower tap (a bilinear sample would mix the NaN pixel into its neighbour as 0 * NaN): the samples
    are the pixels.  Every column of the frame holds one situation, every row repeats it."""
    up = lambda v: np.nextafter(F(v), F(np.inf))                        # noqa: E731
    H, W = sc.SHAPE
    col = np.zeros(W, F); m = np.zeros(W, F); v = np.ones(W, F)
    # centre 0, var 1, kappa (2, 3): tl = 4, th = 9
    col[:8] = [-2.0, -up(2.0), 3.0, up(3.0), 2.5, -2.5, 0.0, np.nan]     # kept: 1 0 1 0 1 0 1 1
    col[8:12] = [0.0, 1.0, -1.0, 5.0]; v[8:12] = 0.0                     # var == 0: only d == 0 stays ...
    m[11] = 5.0                                                          # ... wherever the centre is
    col[12:14] = [100.0, -100.0]; m[12] = np.nan; v[13] = np.nan         # a NaN centre, a NaN variance: nothing is rejected
    col[14:16] = [7.0, -7.0]; v[14:16] = np.inf                          # an infinite variance: nothing is rejected
    col[16:20] = [4.0, -4.0, 4.0, -4.0]; m[18:20] = [1.5, -1.5]          # d = +-4 and +-2.5 against tl = 4, th = 9
    frame = np.ascontiguousarray(np.tile(col, (H, 1)))
    center, var = np.ascontiguousarray(np.tile(m, (H, 1))), np.ascontiguousarray(np.tile(v, (H, 1)))
    vals, live = sr.samples([frame], [sc.IDENT], [0.0], sc.SHAPE, sc.SHAPE, 0)
    assert same(vals[0], frame, nan_any_payload=True) and live.all()
    gclip = Guarded(sc.SHAPE, [("center", F), ("var", F)])
    gclip.write("center", center); gclip.write("var", var)
    seen = {}
    for kappa in ((2.0, 3.0), (3.0, 2.0), (INF, 2.0), (2.0, INF), (INF, INF), (0.5, 0.25)):
        want = ar.State(sc.SHAPE, True).add_samples(vals, live, (center, var), kappa)
        g = Guarded(sc.SHAPE, STATE)
        raw_accum(siftlib, g, host_pointers([frame]), 1, 0, sc.SHAPE, [sc.IDENT], [0.0], mode=0, clip=(gclip.ptr("center"), gclip.ptr("var")), kappa=kappa)
        got = g.read()
        assert state_is(got, want), kappa
        assert (got["coverage"] == 1).all()
        seen[kappa] = got["kept"][0, :20].tolist()
    assert seen[(2.0, 3.0)] == [1, 0, 1, 0, 1, 0, 1, 1] + [1, 0, 0, 1] + [1, 1, 1, 1] + [0, 0, 1, 0]
    assert seen[(3.0, 2.0)][:8] == [1, 1, 0, 0, 0, 1, 1, 1] and seen[(3.0, 2.0)][16:20] == [0, 0, 0, 1]
    assert seen[(INF, 2.0)][:8] == [1, 1, 0, 0, 0, 1, 1, 1] and seen[(2.0, INF)][:8] == [1, 0, 1, 1, 1, 0, 1, 1]
    assert seen[(INF, INF)] == [1] * 20                                  # inf * 0 is NaN at var == 0: nothing is rejected either
    assert seen[(0.5, 0.25)] == [0, 0, 0, 0, 0, 0, 1, 1] + [1, 0, 0, 1] + [1, 1, 1, 1] + [0, 0, 0, 0]


@pytest.mark.parametrize("interp", [0, 1], ids=["bilinear", "cubic"])
def test_output_shapes_around_the_tile_between_guards(siftlib, interp):
    case = {c.name: c for c in sc.cases()}["noise-rot-S5-41x70-m1"]
    whole, dptrs = device_stack(case.frames)
    for out_shape in ((1, 1), (1, 63), (4, 64), (5, 65), (3, 129), (9, 2)):
        vals, live = ar.samples(case.frames, case.maps, case.fills, sc.SHAPE, out_shape, 1, "cubic" if interp else None)
        rng = np.random.default_rng(out_shape[1])
        center, var = rng.normal(0, 50.0, out_shape).astype(F), (rng.random(out_shape) * 1e4).astype(F)
        want = ar.State(out_shape, True).add_samples(vals[:2], live[:2]).add_samples(vals[2:], live[2:], (center, var), (1.0, 1.0))
        g, gclip, planes = Guarded(out_shape, STATE), Guarded(out_shape, [("center", F), ("var", F)]), Guarded(out_shape, RESULT, fill=0x11)
        gclip.write("center", center); gclip.write("var", var)
        raw_accum(siftlib, g, (C.c_void_p * 2)(*dptrs[:2]), 2, 1, out_shape, case.maps[:2], case.fills[:2], 1, interp)
        raw_accum(siftlib, g, (C.c_void_p * 3)(*dptrs[2:]), 3, 1, out_shape, case.maps[2:], case.fills[2:], 1, interp,
                  clip=(gclip.ptr("center"), gclip.ptr("var")), kappa=(1.0, 1.0))
        assert state_is(g.read(), want), out_shape
        raw_result(siftlib, g, out_shape, planes.ptr("mean"), planes.ptr("var"), 1, -1.0)
        got, (wmean, wvar) = planes.read(), want.result(empty=-1.0, var=True)
        assert same(got["mean"], wmean, nan_any_payload=True) and same(got["var"], wvar, nan_any_payload=True), out_shape
        gclip.read()
    del whole


# --------------------------------------------------------------------------------------------- against the mean kernel itself
@pytest.mark.parametrize("S,chunk", [(200, 64), (64, 5), (5, 1)])
def test_whole_numbers_and_whole_shifts_give_stack_batchs_mean_bit_for_bit(siftlib, S, chunk):
    import torch
    plan = batch_plan()
    frames = ac.integer_stack(S)
    maps, fills = sc.maps_of("shift", S), sc.fills_of(S)
    M, off = tables(maps)
    want, want_c = plan.stack_batch(frames, M, off, fills, out_shape=sc.OUTS[1], reduce="mean", empty=-3.0, coverage=True, out="device")
    acc = plan.stack_accumulator(sc.OUTS[1])
    assert acc.frames == 0 and set(acc.state()) == {"s1", "coverage", "kept"}
    for a, b in ac.splits(S, chunk):
        assert acc.add(frames[a:b], M[a:b], off[a:b], fills[a:b]) is acc
        assert acc.last_stack_ms > 0.0
    assert acc.frames == S
    mean, cov, kept = acc.result(empty=-3.0, counts=True, out="device")
    assert isinstance(mean, torch.Tensor) and mean.is_cuda and mean.dtype == torch.float32 and cov.dtype == torch.int32
    assert same(mean.cpu().numpy(), want.cpu().numpy()) and torch.equal(cov, want_c) and torch.equal(kept, want_c)
    host = acc.result(empty=-3.0)
    assert isinstance(host, np.ndarray) and same(host, want.cpu().numpy())
    acc.reset()
    assert acc.frames == 0 and all(not bool(t.any()) for t in acc.state().values())
    assert (acc.result(empty=4.0) == 4.0).all()


def test_the_python_class(siftlib):
    import torch
    import sift_pyocl_amd as sp
    plan = batch_plan()
    case = {c.name: c for c in sc.cases()}["noise-leaving-S8-41x70-m1"]
    M, off = tables(case.maps)
    vals, live = sr.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, 1)
    first = plan.stack_accumulator(case.out_shape, moments=True)
    assert isinstance(first, sp.StackAccumulator) and set(first.state()) == {"s1", "s2", "coverage", "kept"}
    first.add(np.stack(case.frames[:3]), M[:3].reshape(-1, 2, 2), off[:3], case.fills[:3])
    first.add([torch.from_numpy(f).cuda() for f in case.frames[3:]], M[3:], off[3:], case.fills[3:])
    want = ar.State(case.out_shape, True).add_samples(vals, live)
    st = {k: t.cpu().numpy() for k, t in first.state().items()}
    assert state_is(st, want)
    mean, var, cov, kept = first.result(var=True, counts=True)
    wmean, wvar = want.result(var=True)
    assert same(mean, wmean, nan_any_payload=True) and same(var, wvar, nan_any_payload=True) and np.array_equal(cov, want.coverage) and np.array_equal(kept, want.kept)
    # the second pass: host planes are uploaded, device planes are taken as they are
    wsecond = ar.State(case.out_shape, False).add_samples(vals, live, (wmean, wvar), (1.0, 2.0))
    for clip in ((mean, var), first.result(var=True, out="device")):
        second = plan.stack_accumulator(case.out_shape).add(case.frames, M, off, case.fills, clip=clip, kappa=(1.0, 2.0))
        m2, c2, k2 = second.result(counts=True)
        assert same(m2, wsecond.result(), nan_any_payload=True) and np.array_equal(k2, wsecond.kept) and np.array_equal(c2, wsecond.coverage)
    assert 0 < (wsecond.kept < wsecond.coverage).sum()
    cub = plan.stack_accumulator(case.out_shape).add(case.frames, M, off, case.fills, interp="cubic").result()
    cvals, clive = ar.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, 1, "cubic")
    assert same(cub, ar.State(case.out_shape, False).add_samples(cvals, clive).result(), nan_any_payload=True)
    assert plan.stack_accumulator().out_shape == sc.SHAPE
    # what Python refuses, before any launch
    acc = plan.stack_accumulator(case.out_shape)
    with pytest.raises(ValueError):
        acc.result(var=True)
    with pytest.raises(ValueError):
        acc.result(out="pinned")
    for bad in (dict(clip=(mean[:-1], var)), dict(clip=(mean, var.astype(np.float64))), dict(clip=(mean,)), dict(clip=(mean, var), kappa=(0.0, 3.0)),
                dict(clip=(mean, var), kappa=(3.0, float("nan"))), dict(clip=(mean, var), kappa=(3.0,)), dict(interp="cubic", mode=0), dict(interp="nearest")):
        with pytest.raises(ValueError):
            acc.add(case.frames, M, off, case.fills, **bad)
    with pytest.raises(ValueError):
        acc.add(case.frames, M[:2], off, case.fills)
    assert acc.frames == 0 and not bool(acc.state()["coverage"].any())
    rgb = sp.BatchPlan(shape=sc.SHAPE + (3,), dtype=np.uint8, lanes=1)
    with pytest.raises(RuntimeError):
        rgb.stack_accumulator()


# ------------------------------------------------------------------------------------------------------- edges of the interface
def test_no_frame_and_an_empty_output_launch_nothing_and_change_nothing(siftlib):
    frames = sc.frames_of("noise", 2)
    maps, fills = sc.maps_of("shift", 2), sc.fills_of(2)
    g = Guarded(sc.OUTS[1], STATE)
    raw_accum(siftlib, g, host_pointers(frames), 2, 0, sc.OUTS[1], maps, fills)
    before = g.read()
    assert before["coverage"].max() == 2
    assert raw_accum(siftlib, g, None, 0, 0, sc.OUTS[1], [], np.zeros(0, F)) == 0.0
    assert raw_accum(siftlib, g, None, 0, 1, sc.OUTS[1], [], np.zeros(0, F), over=dict(images=None, maps=None, fills=None)) == 0.0
    for n, out_shape in ((2, (0, 7)), (2, (5, 0)), (0, (0, 0))):
        assert raw_accum(siftlib, g, host_pointers(frames), n, 0, out_shape, maps[:n], fills[:n]) == 0.0
        assert raw_accum(siftlib, g, host_pointers(frames), n, 0, out_shape, maps[:n], fills[:n], over=dict(s1=None, s2=None, cov=None, kept=None)) == 0.0
        planes = Guarded((2, 2), RESULT, fill=0x11)
        assert raw_result(siftlib, g, out_shape, planes.ptr("mean"), planes.ptr("var"), 1, 1.0) == 0.0
        assert raw_result(siftlib, g, out_shape, None, None, 0, 1.0, s1=None, s2=None, kept=None) == 0.0
        assert all((p.view(np.uint8) == 0x11).all() for p in planes.read().values())
    after = g.read()
    assert all(np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)) for k in before)
    # a result without any frame added: `empty` everywhere
    z, planes = Guarded(sc.OUTS[1], STATE), Guarded(sc.OUTS[1], RESULT, fill=0x11)
    raw_result(siftlib, z, sc.OUTS[1], planes.ptr("mean"), planes.ptr("var"), 1, 6.25)
    got = planes.read()
    assert (got["mean"] == F(6.25)).all() and (got["var"] == F(6.25)).all()


def test_argument_errors_write_nothing(siftlib):
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    frames = sc.frames_of("noise", 2)
    maps, fills = sc.maps_of("shift", 2), sc.fills_of(2)
    ptrs, holed = host_pointers(frames), host_pointers(frames)
    holed[1] = None
    out_shape = sc.OUTS[1]
    g, gclip, planes = Guarded(out_shape, STATE, fill=0x33), Guarded(out_shape, [("center", F), ("var", F)], fill=0x44), Guarded(out_shape, RESULT, fill=0x11)
    clip = (gclip.ptr("center"), gclip.ptr("var"))
    rgb = sp.BatchPlan(shape=sc.SHAPE + (3,), dtype=np.uint8, lanes=1)
    E = _lib.EINVAL
    for bad in (dict(h=None), dict(images=None), dict(maps=None), dict(fills=None), dict(images=holed), dict(ow=-1), dict(oh=-1), dict(n=-1), dict(n=65536),
                dict(oh=262141), dict(h=rgb._handle), dict(interp=2), dict(interp=-1), dict(interp=1, mode=0), dict(interp=1, mode=2),
                dict(s1=None), dict(cov=None), dict(kept=None), dict(center=clip[0]), dict(var=clip[1]),
                dict(center=clip[0], var=clip[1], kl=0.0), dict(center=clip[0], var=clip[1], kh=-1.0), dict(center=clip[0], var=clip[1], kl=float("nan")),
                dict(center=clip[0], var=clip[1], kh=float("nan")), dict(center=clip[0], var=clip[1], kl=-INF)):
        assert raw_accum(siftlib, g, ptrs, 2, 0, out_shape, maps, fills, want_rc=E, over=bad) == -1.0, bad
        assert siftlib.siftmi_last_error()
    # a kappa is looked at only when a clip is given
    ok = Guarded(out_shape, STATE)
    raw_accum(siftlib, ok, ptrs, 2, 0, out_shape, maps, fills, over=dict(kl=float("nan"), kh=-1.0))
    for bad in (dict(h=None), dict(ow=-1), dict(oh=-1), dict(oh=262141), dict(h=rgb._handle), dict(s1=None), dict(kept=None), dict(mean=None), dict(s2=None)):
        assert raw_result(siftlib, ok, out_shape, planes.ptr("mean"), planes.ptr("var"), 1, 0.0, want_rc=E, **bad) == -1.0, bad
        assert siftlib.siftmi_last_error()
    host = np.full(out_shape, -77.0, F)
    assert raw_result(siftlib, ok, out_shape, host.ctypes.data, host.ctypes.data, 0, 0.0, moments=False, want_rc=E) == -1.0
    assert (host == -77.0).all()
    assert all((p.view(np.uint8) == 0x33).all() for p in g.read().values())
    assert all((p.view(np.uint8) == 0x44).all() for p in gclip.read().values())
    assert all((p.view(np.uint8) == 0x11).all() for p in planes.read().values())


# -------------------------------------------------------------------------------------------------------------------- ordering
def ordering_setup():
    """a stack of 8: the first 5 frames are in the state, a call adds the last 3 under a clip.  Every device input has a decoy
    that changes the result."""
    if "ordering" not in _cache:
        real, decoy = sc.frames_of("noise", 8, seed=1), sc.frames_of("noise", 8, seed=2)
        maps, fills = sc.maps_of("shift", 8), sc.fills_of(8)
        out = oc.STACK_OUT
        vals, live = sr.samples(real, maps, fills, sc.SHAPE, out, 1)
        dvals, dlive = sr.samples(real[:7] + [decoy[7]], maps, fills, sc.SHAPE, out, 1)
        before = ar.State(out, True).add_samples(vals[:5], live[:5])
        other = ar.State(out, True).add_samples(dvals[3:8], dlive[3:8])              # a decoy for every state plane
        center, var = ar.State(out, True).add_samples(vals, live).result(var=True)
        rng = np.random.default_rng(9)
        dcenter, dvar = (center + rng.normal(0, 1e3, out)).astype(F), (var * 0.01).astype(F)
        _cache["ordering"] = dict(real=real, decoy=decoy, maps=maps, fills=fills, out=out, vals=vals, live=live, dvals=dvals, dlive=dlive, before=before,
                                  other=other, center=center, var=var, dcenter=dcenter, dvar=dvar, kappa=(1.0, 1.0))
    return _cache["ordering"]


def planes_of(state):
    return {"s1": state.s1, "s2": state.s2, "coverage": state.coverage, "kept": state.kept}


@pytest.mark.parametrize("late", ["s1", "s2", "coverage", "kept", "center", "var", "frame"])
def test_accum_waits_for_a_late_producer_of_every_device_pointer(siftlib, late):
    """RAW and WAW at once for the state planes, which the call reads and writes: a call that did not wait would add to the decoy,
    and the late copy of the real plane would land on top of what it wrote"""
    import torch
    o = ordering_setup()
    out, kappa = o["out"], o["kappa"]
    want = o["before"].copy().add_samples(o["vals"][5:], o["live"][5:], (o["center"], o["var"]), kappa)
    wrong = dict(s1=o["other"].s1, s2=o["other"].s2, coverage=o["other"].coverage, kept=o["other"].kept, center=o["dcenter"], var=o["dvar"],
                 frame=o["decoy"][7])
    real = dict(planes_of(o["before"]), center=o["center"], var=o["var"], frame=o["real"][7])
    # the decoy changes the result
    if late in ("center", "var"):
        alt = o["before"].copy().add_samples(o["vals"][5:], o["live"][5:], (wrong["center"] if late == "center" else o["center"],
                                                                              wrong["var"] if late == "var" else o["var"]), kappa)
    elif late == "frame":
        alt = o["before"].copy().add_samples(o["dvals"][5:], o["dlive"][5:], (o["center"], o["var"]), kappa)
    else:
        alt = o["other"]
    assert not alt.same(want)
    g, gclip = Guarded(out, STATE), Guarded(out, [("center", F), ("var", F)])
    gclip.write("center", o["center"]); gclip.write("var", o["var"])
    whole, dptrs = device_stack(o["real"][5:])
    tensors = dict({k: g.tensor(k) for k in ("s1", "s2", "coverage", "kept")}, center=gclip.tensor("center"), var=gclip.tensor("var"), frame=whole[2])

    def reset():
        for k, plane in planes_of(o["before"]).items():
            g.write(k, plane)

    def call():
        raw_accum(siftlib, g, (C.c_void_p * 3)(*dptrs), 3, 1, out, o["maps"][5:], o["fills"][5:], clip=(gclip.ptr("center"), gclip.ptr("var")), kappa=kappa)

    reset()
    call_ms = oc.timed(call)
    assert state_is(g.read(), want), "wrong state on ready inputs"
    delay = oc.delay_for(call_ms)
    for k, stream in enumerate(oc.side_streams()):
        reset()
        done = oc.late_many([(tensors[late], real[late], wrong[late])], stream, delay)
        oc.window_open(done, late)
        call()
        early = not done.query()
        torch.cuda.synchronize()
        assert state_is(g.read(), want), "%s late on side stream %d: the call did not wait for the caller's stream" % (late, k)
        assert not early, "%s, side stream %d: the call returned while the caller's stream was still working" % (late, k)
    del whole


@pytest.mark.parametrize("late", ["s1", "s2", "kept", "mean", "var"])
def test_result_waits_for_a_late_producer_of_every_device_pointer(siftlib, late):
    import torch
    o = ordering_setup()
    out = o["out"]
    state = o["before"]
    wmean, wvar = state.result(empty=oc.STACK_EMPTY, var=True)
    omean, ovar = o["other"].result(empty=oc.STACK_EMPTY, var=True)
    assert not same(wmean, omean, nan_any_payload=True) and not same(wvar, ovar, nan_any_payload=True)
    g, planes = Guarded(out, STATE), Guarded(out, RESULT)
    for k, plane in planes_of(state).items():
        g.write(k, plane)
    call = lambda: raw_result(siftlib, g, out, planes.ptr("mean"), planes.ptr("var"), 1, oc.STACK_EMPTY)      # noqa: E731
    call_ms = oc.timed(call)
    got = planes.read()
    assert same(got["mean"], wmean, nan_any_payload=True) and same(got["var"], wvar, nan_any_payload=True)
    delay = oc.delay_for(call_ms)
    if late in ("mean", "var"):                                          # an output: the late producer writes a sentinel
        tensor, real, decoy = planes.tensor(late), np.full(out, -12345.0, F), np.zeros(out, F)
    else:
        tensor, real, decoy = g.tensor(late), planes_of(state)[late], planes_of(o["other"])[late]
    for k, stream in enumerate(oc.side_streams()):
        done = oc.late_many([(tensor, real, decoy)], stream, delay)
        oc.window_open(done, late)
        call()
        early = not done.query()
        torch.cuda.synchronize()
        got = planes.read()
        assert same(got["mean"], wmean, nan_any_payload=True) and same(got["var"], wvar, nan_any_payload=True), (late, k)
        assert not early, (late, k)


# -------------------------------------------------------------------------------------------------- LinearAlign.stack_stream
def aligner():
    import sift_pyocl_amd as sp
    if "la" not in _cache:
        _cache["la"] = sp.LinearAlign(ac.stream_stack()[0])
    return _cache["la"]


def returned_maps(res):
    return [(res["matrix"][s].reshape(4), res["offset"][s]) for s in range(len(res["matrix"]))]


def test_stack_stream_is_the_restatement_fed_the_returned_maps_whatever_the_chunk(siftlib):
    la = aligner()
    ref, clean, dirty, where = ac.stream_stack()
    a = la.stack_stream(dirty, chunk=5, var=True, return_all=True)
    b = la.stack_stream(np.stack(dirty), chunk=12, var=True, return_all=True)
    assert set(a) == {"stack", "coverage", "kept", "var", "matrix", "offset", "mode", "n", "rms", "fill"} and la.last_stack_ms > 0.0
    for k in a:
        assert same(np.asarray(a[k]), np.asarray(b[k]), nan_any_payload=True), k
    assert a["matrix"].shape == (12, 2, 2) and a["offset"].shape == (12, 2) and (a["mode"] > 0).all() and a["fill"].shape == (12,)
    for s, (dy, dx) in enumerate(ac.STREAM_OFFSETS):
        assert abs(a["offset"][s][0] + dy) < 1.0 and abs(a["offset"][s][1] + dx) < 1.0, s
    want = ar.State(la.outshape, True).add(dirty, returned_maps(a), a["fill"], ref.shape)
    wmean, wvar = want.result(var=True)
    assert a["stack"].dtype == F and a["coverage"].dtype == np.int32
    assert same(a["stack"], wmean, nan_any_payload=True) and same(a["var"], wvar, nan_any_payload=True)
    assert np.array_equal(a["coverage"], want.coverage) and np.array_equal(a["kept"], want.coverage)
    # the plain return values, on the host and on the device, and the mean kernel's own answer to within its float32 sum
    plain = la.stack_stream(dirty, chunk=5)
    assert isinstance(plain, np.ndarray) and same(plain, a["stack"], nan_any_payload=True)
    dev, dvar = la.stack_stream(dirty, chunk=7, var=True, out="device")
    assert dev.is_cuda and same(dev.cpu().numpy(), a["stack"], nan_any_payload=True) and same(dvar.cpu().numpy(), a["var"], nan_any_payload=True)
    cub = la.stack_stream(dirty, chunk=5, interp="cubic", return_all=True)
    cwant = ar.State(la.outshape, False).add(dirty, returned_maps(cub), cub["fill"], ref.shape, interp="cubic")
    assert same(cub["stack"], cwant.result(), nan_any_payload=True) and same(cub["matrix"], a["matrix"])
    win = la.stack_stream(dirty, chunk=5, max_shift=12, return_all=True)
    wwant = ar.State(la.outshape, False).add(dirty, returned_maps(win), win["fill"], ref.shape)
    assert same(win["stack"], wwant.result(), nan_any_payload=True)


def test_stack_stream_sigma_drops_the_zingers_and_nothing_else(siftlib):
    """The frames are pure shifts and are estimated as such (shift_only): the median displacement is whole to within 1e-3 pixels.
    An affine fit of the same matches is off by 0.01 to 0.03 pixels at the frame's far edge (measured: 9e-5 in the matrix, 0.014 in
    the offset), and the bilinear sample of a frame's last column then mixes that much of the fill into it -- hundreds of counts
    on this plane, which the sigma rule rightly drops: 63 edge pixels lost a sample that way."""
    la = aligner()
    ref, clean, dirty, where = ac.stream_stack()
    res = la.stack_stream(dirty, chunk=5, reject="sigma", var=True, shift_only=True, return_all=True)
    assert (res["mode"] == 1).all()
    maps = returned_maps(res)
    first = ar.State(la.outshape, True).add(dirty, maps, res["fill"], ref.shape)
    center, spread = first.result(var=True)
    want = ar.State(la.outshape, True).add(dirty, maps, res["fill"], ref.shape, clip=(center, spread), kappa=(3.0, 3.0))
    wmean, wvar = want.result(var=True)
    assert same(res["stack"], wmean, nan_any_payload=True) and same(res["var"], wvar, nan_any_payload=True)
    assert np.array_equal(res["coverage"], want.coverage) and np.array_equal(res["kept"], want.kept)
    again = la.stack_stream(dirty, chunk=12, reject="sigma", var=True, shift_only=True, return_all=True)
    for k in res:
        assert same(np.asarray(res[k]), np.asarray(again[k]), nan_any_payload=True), k
    zing = np.zeros(la.outshape, bool)
    for yr, xr in where:
        zing[yr, xr] = True
    many = res["coverage"] >= 11
    ideal = table(ac.stream_ideal_maps())
    odd = np.argwhere(many & ~zing & (res["kept"] != res["coverage"]))
    print("stack_stream sigma: maps off the ideal ones by at most %g (matrix) and %g (offset); %d pixels of %d beside the zingers lost a sample: %s"
          % (np.abs(table(maps)[:, :4] - ideal[:, :4]).max(), np.abs(table(maps)[:, 4:] - ideal[:, 4:]).max(), len(odd), int(many.sum()), odd[:20].tolist()))
    print("zingers at %s; modes %s" % (where, res["mode"].tolist()))
    assert many.sum() > 200 * 200 and many[zing].all()
    assert np.array_equal(res["kept"][many & zing], res["coverage"][many & zing] - 1)
    assert np.array_equal(res["kept"][many & ~zing], res["coverage"][many & ~zing])
    plain = la.stack_stream(dirty, chunk=5)
    assert (plain[zing] - res["stack"][zing] > 2000.0).all()


def test_stack_stream_refuses_what_it_cannot_do(siftlib):
    import sift_pyocl_amd as sp
    la = aligner()
    ref, clean, dirty, where = ac.stream_stack()
    empty = la.stack_stream([], empty=4.0)
    assert empty.shape == la.outshape and (empty == 4.0).all()
    for bad in (dict(reject="trim"), dict(chunk=0), dict(chunk=2.5), dict(kappa=(0.0, 3.0)), dict(kappa=(3.0,)), dict(out="pinned"),
                dict(expected_shift=(1.0, 0.0)), dict(interp="nearest")):
        with pytest.raises(ValueError):
            la.stack_stream(dirty[:2], **bad)
    colour = np.random.default_rng(5).integers(0, 256, (72, 90, 3), dtype=np.uint8)
    rgb = sp.LinearAlign(colour)
    with pytest.raises(RuntimeError):
        rgb.stack_stream([colour])
