"""GPU tests of the clipped stack reduction's row: stack_clip_kernel (csrc/k_stack_clip.hpp) through siftmi_batch_stack_clip,
BatchPlan.stack_clip_batch and LinearAlign.stack_clip.

Every crafted stack of tests/stack_clip_cases.py is compared with tests/stack_clip_ref.py bit for bit -- plane, coverage and kept
counts; a NaN matches any NaN.  The existing reductions are the yardstick for the identities: with nothing rejected the plane and
the coverage are stack_batch(reduce="mean")'s, and on a NaN-free all-live stack of odd S trimming S >> 1 from either side leaves
stack_batch(reduce="median")'s plane.  The LinearAlign.stack_clip tests use the stack of tests/test_gpu_stack.py's
LinearAlign.stack tests, built here the same way: 7 crops of a smooth plane with 20 zingers each, no two in one cell of a 16-pixel
lattice, so a pixel sees a zinger in at most one of its 7 samples.
"""
import ctypes as C

import numpy as np
import pytest

import ordering_cases as oc
import stack_cases as sc
import stack_clip_cases as cc
import stack_clip_ref as cr
import stack_ref as sr
from util import smooth_noise
from warp_ref import same

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 256                                     # bytes
EMPTY = -12345.0
_cache = {}


def batch_plan():
    import sift_pyocl_amd as sp
    if "plan" not in _cache:
        _cache["plan"] = sp.BatchPlan(shape=sc.SHAPE, dtype=F, lanes=1)
    return _cache["plan"]


def by_name(name):
    return {c.name: c for c in cc.cases()}[name]


def sampled(case):
    key = ("samples", case.stack)
    if key not in _cache:
        _cache[key] = sr.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, case.mode)
    return _cache[key]


def table(maps):
    """the n x 6 table of the C ABI"""
    if not len(maps):
        return np.zeros((0, 6), F)
    return np.ascontiguousarray(np.array([tuple(M) + tuple(off) for M, off in maps], F))


def tables(maps):
    t = table(maps)
    return t[:, :4].copy(), t[:, 4:].copy()


def raw_call(siftlib, ptrs, n, is_dev, out_ptr, cov_ptr, kept_ptr, out_is_dev, out_shape, maps, fills, mode, p, empty=EMPTY, want_rc=0):
    """siftmi_batch_stack_clip with plain addresses and the parameters p (stack_clip_cases.params); returns kernel_ms"""
    tab = table(maps)
    fills = np.ascontiguousarray(fills, F)
    w = None if p["weights"] is None else np.ascontiguousarray(p["weights"], F)
    ms = C.c_double(-1.0)
    rc = siftlib.siftmi_batch_stack_clip(batch_plan()._handle, ptrs, n, is_dev, out_ptr, cov_ptr, kept_ptr, out_is_dev, out_shape[1], out_shape[0],
                                         tab.ctypes.data, fills.ctypes.data, None if w is None else w.ctypes.data, mode,
                                         {"trim": 0, "sigma": 1}[p["reject"]], p["trim"][0], p["trim"][1], C.c_float(p["kappa"][0]),
                                         C.c_float(p["kappa"][1]), p["iters"], C.c_float(empty), C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def host_pointers(frames):
    return (C.c_void_p * max(1, len(frames)))(*[f.ctypes.data for f in frames])


def device_stack(frames):
    """the frames as one device tensor (kept alive by the caller) and the pointer of every plane"""
    import torch
    whole = torch.from_numpy(np.stack(frames)).cuda()
    step = frames[0].nbytes
    return whole, (C.c_void_p * len(frames))(*[whole.data_ptr() + s * step for s in range(len(frames))])


def guarded_call(siftlib, ptrs, n, is_dev, out_shape, maps, fills, mode, p, counts=(True, True), empty=EMPTY):
    """a device plane, coverage and kept plane, each between guard bytes in one buffer: (plane, coverage or None, kept or None) on
    the host, after checking that no byte outside the planes asked for changed"""
    import torch
    nbytes = out_shape[0] * out_shape[1] * 4
    buf = torch.full((4 * GUARD + 3 * nbytes,), 0xa5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    at = [GUARD + k * (GUARD + nbytes) for k in range(3)]
    torch.cuda.synchronize()
    raw_call(siftlib, ptrs, n, is_dev, buf.data_ptr() + at[0], buf.data_ptr() + at[1] if counts[0] else None,
             buf.data_ptr() + at[2] if counts[1] else None, 1, out_shape, maps, fills, mode, p, empty)
    host = buf.cpu().numpy()
    keep = np.ones(host.shape, bool)
    res = []
    for k, (on, dtype) in enumerate(((True, F), (counts[0], np.int32), (counts[1], np.int32))):
        if on:
            keep[at[k]:at[k] + nbytes] = False
            res.append(host[at[k]:at[k] + nbytes].view(dtype).reshape(out_shape).copy())
        else:
            res.append(None)
    assert (host[keep] == 0xa5).all(), (out_shape, p["reject"], counts, "bytes outside the result were written")
    return res


def agrees(got, want, name, path):
    plane, cov, kept = got
    assert same(plane, want[0], nan_any_payload=True), (name, path, "plane", int((plane.view(np.uint32) != want[0].view(np.uint32)).sum()))
    assert cov is None or np.array_equal(cov, want[1]), (name, path, "coverage")
    assert kept is None or np.array_equal(kept, want[2]), (name, path, "kept", int((kept != want[2]).sum()))


# ------------------------------------------------------------------------------------------------------ the crafted stacks
@pytest.mark.parametrize("case", cc.cases(), ids=[c.name for c in cc.cases()])
def test_every_case_is_the_reference_bit_for_bit(siftlib, case):
    """two calls that together take every pointer path: host frames to a host result with both counts, device frames to a device
    result between guards with one of the counts or none"""
    vals, live = sampled(case)
    p = cc.params(case)
    S = len(case.frames)
    want = cr.reduce_clip(vals, live, empty=EMPTY, **p)
    out = np.full(case.out_shape, -77.0, F)
    cov = np.full(case.out_shape, -5, np.int32)
    kept = np.full(case.out_shape, -6, np.int32)
    ms = raw_call(siftlib, host_pointers(case.frames), S, 0, out.ctypes.data, cov.ctypes.data, kept.ctypes.data, 0, case.out_shape, case.maps,
                  case.fills, case.mode, p)
    assert ms > 0.0
    agrees((out, cov, kept), want, case.name, "host to host")
    whole, dptrs = device_stack(case.frames)
    counts = ((False, True), (True, False), (False, False))[len(case.name) % 3]
    agrees(guarded_call(siftlib, dptrs, S, 1, case.out_shape, case.maps, case.fills, case.mode, p, counts), want, case.name, "device to device")
    del whole


@pytest.mark.parametrize("name", ["noise-leaving-S8-41x70-sigma1.5-mixed", "ties-shift-S8-trim2_3-w", "noise-nan_some-S64-trim31_32"])
def test_the_mixed_pointer_paths_and_the_python_method(siftlib, name):
    import torch
    case = by_name(name)
    vals, live = sampled(case)
    p = cc.params(case)
    S = len(case.frames)
    want = cr.reduce_clip(vals, live, empty=EMPTY, **p)
    agrees(guarded_call(siftlib, host_pointers(case.frames), S, 0, case.out_shape, case.maps, case.fills, case.mode, p), want, name, "host to device")
    whole, dptrs = device_stack(case.frames)
    out = np.full(case.out_shape, -77.0, F)
    kept = np.full(case.out_shape, -6, np.int32)
    raw_call(siftlib, dptrs, S, 1, out.ctypes.data, None, kept.ctypes.data, 0, case.out_shape, case.maps, case.fills, case.mode, p)
    agrees((out, None, kept), want, name, "device to host, kept alone")
    cov = np.full(case.out_shape, -5, np.int32)
    raw_call(siftlib, dptrs, S, 1, out.ctypes.data, cov.ctypes.data, None, 0, case.out_shape, case.maps, case.fills, case.mode, p)
    agrees((out, cov, None), want, name, "device to host, coverage alone")
    del whole
    # BatchPlan.stack_clip_batch: counts on and off, host and device
    plan = batch_plan()
    Ms, offs = tables(case.maps)
    kw = dict(out_shape=case.out_shape, mode=case.mode, empty=EMPTY, **p)
    got = plan.stack_clip_batch(case.frames, Ms.reshape(-1, 2, 2), offs, case.fills, counts=True, **kw)
    assert all(isinstance(a, np.ndarray) for a in got) and [a.dtype for a in got] == [F, np.int32, np.int32] and plan.last_stack_ms > 0.0
    agrees(got, want, name, "method, host")
    plain = plan.stack_clip_batch(np.stack(case.frames), Ms, offs, case.fills, **kw)
    assert isinstance(plain, np.ndarray) and same(plain, want[0], nan_any_payload=True)
    tens = [torch.from_numpy(f).cuda() for f in case.frames]
    dev = plan.stack_clip_batch(tens, Ms, offs, case.fills, out="device", **kw)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32 and same(dev.cpu().numpy(), want[0], nan_any_payload=True)
    dev = plan.stack_clip_batch(tens, Ms, offs, case.fills, counts=True, out="device", **kw)
    assert all(t.is_cuda for t in dev) and [t.dtype for t in dev] == [torch.float32, torch.int32, torch.int32]
    agrees([t.cpu().numpy() for t in dev], want, name, "method, device")
    if case.weights is not None:                        # no weights: ones
        ones = plan.stack_clip_batch(case.frames, Ms, offs, case.fills, counts=True, **dict(kw, weights=np.ones(S, F)))
        none = plan.stack_clip_batch(case.frames, Ms, offs, case.fills, counts=True, **dict(kw, weights=None))
        assert all(same(a, b, nan_any_payload=True) for a, b in zip(ones, none))
        agrees(none, cr.reduce_clip(vals, live, empty=EMPTY, **dict(p, weights=None)), name, "no weights")


@pytest.mark.parametrize("reject", cr.REJECTS)
def test_output_shapes_around_the_tile_between_guards(siftlib, reject):
    """a store beyond a row or the plane shows here: widths around the 64-column tile, heights around its 4 rows"""
    case = by_name("noise-leaving-S8-41x70-sigma1.5-mixed")
    p = dict(cc.params(case), reject=reject, trim=(1, 2))
    whole, dptrs = device_stack(case.frames)
    for out_shape in ((1, 1), (1, 63), (4, 64), (5, 65), (3, 129), (9, 2)):
        want = cr.stack_clip_ref(case.frames, case.maps, case.fills, sc.SHAPE, out_shape, 1, empty=EMPTY, **p)
        agrees(guarded_call(siftlib, dptrs, 8, 1, out_shape, case.maps, case.fills, 1, p), want, reject, out_shape)
    del whole


# --------------------------------------------------------------------------------------------- against the existing reductions
def test_nothing_rejected_is_stack_batchs_mean_and_a_full_trim_its_median(siftlib):
    plan = batch_plan()
    seen = set()
    for case in cc.cases():
        if case.stack in seen:
            continue
        seen.add(case.stack)
        Ms, offs = tables(case.maps)
        kw = dict(out_shape=case.out_shape, mode=case.mode, empty=EMPTY)
        mean, cov = plan.stack_batch(case.frames, Ms, offs, case.fills, reduce="mean", coverage=True, **kw)
        mean, cov = np.array(mean), np.array(cov)
        for p in (dict(reject="trim", trim=(0, 0)), dict(reject="sigma", iters=0), dict(reject="sigma", kappa=(np.inf, np.inf), iters=4)):
            plane, c, kept = plan.stack_clip_batch(case.frames, Ms, offs, case.fills, counts=True, **dict(kw, **p))
            assert same(plane, mean, nan_any_payload=True) and np.array_equal(c, cov) and np.array_equal(kept, cov), (case.stack, p)
    assert len(seen) > 20
    checked = 0
    for stack, S in (("noisyzinger-identity-S63", 63), ("zinger-identity-S5", 5), ("const00005-identity-S5", 5), ("ties-identity-S5", 5)):
        case = [c for c in cc.cases() if c.stack == stack][0]
        vals, live = sampled(case)
        assert S & 1 and live.all() and not np.isnan(vals).any()
        Ms, offs = tables(case.maps)
        kw = dict(out_shape=case.out_shape, mode=case.mode)
        median = plan.stack_batch(case.frames, Ms, offs, case.fills, reduce="median", **kw)
        plane, c, kept = plan.stack_clip_batch(case.frames, Ms, offs, case.fills, reject="trim", trim=(S >> 1, S >> 1), counts=True, **kw)
        assert same(plane, np.array(median)) and (kept == 1).all() and (c == S).all(), stack
        checked += 1
    assert checked == 4


# ------------------------------------------------------------------------------------------------------- edges of the interface
def test_no_frame_fills_the_plane_and_an_empty_output_launches_nothing(siftlib):
    import torch
    plan = batch_plan()
    frames = sc.frames_of("noise", 2)
    hptrs = host_pointers(frames)
    maps, fills = sc.maps_of("shift", 2), sc.fills_of(2)
    for reject in cr.REJECTS:
        p = dict(reject=reject, trim=(1, 1), kappa=(3.0, 3.0), iters=3, weights=None)
        out = np.full(sc.OUTS[1], -77.0, F)
        cov = np.full(sc.OUTS[1], -5, np.int32)
        kept = np.full(sc.OUTS[1], -6, np.int32)
        raw_call(siftlib, None, 0, 0, out.ctypes.data, cov.ctypes.data, kept.ctypes.data, 0, sc.OUTS[1], [], np.zeros(0, F), 1, p, empty=6.25)
        assert (out == F(6.25)).all() and (cov == 0).all() and (kept == 0).all(), reject
        got = guarded_call(siftlib, None, 0, 1, sc.OUTS[1], [], np.zeros(0, F), 1, p, empty=float("nan"))
        assert np.isnan(got[0]).all() and (got[1] == 0).all() and (got[2] == 0).all(), reject
        got = guarded_call(siftlib, None, 0, 0, (5, 65), [], np.zeros(0, F), 1, p, counts=(False, False), empty=-1.5)
        assert (got[0] == F(-1.5)).all(), reject
        plane, c, k = plan.stack_clip_batch([], np.zeros((0, 2, 2), F), np.zeros((0, 2), F), out_shape=(3, 7), reject=reject, empty=9.0, counts=True)
        assert plane.shape == (3, 7) and (plane == 9.0).all() and c.dtype == k.dtype == np.int32 and (c == 0).all() and (k == 0).all()
        for n, out_shape in ((2, (0, 7)), (2, (5, 0)), (0, (0, 0))):
            host = np.full(96, 0x5a, np.uint8)
            ms = raw_call(siftlib, hptrs, n, 0, host.ctypes.data, host.ctypes.data + 32, host.ctypes.data + 64, 0, out_shape, maps[:n], fills[:n], 1, p)
            assert ms == 0.0 and (host == 0x5a).all()
            dev = torch.full((96,), 0xa5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ms = raw_call(siftlib, hptrs, n, 0, dev.data_ptr(), dev.data_ptr() + 32, dev.data_ptr() + 64, 1, out_shape, maps[:n], fills[:n], 1, p)
            assert ms == 0.0 and bool((dev == 0xa5).all())
    assert plan.stack_clip_batch(frames, *tables(maps), fills=0.0, out_shape=(0, 7)).shape == (0, 7)
    # the defaults: sigma (3, 3) in 3 passes, the plan's shape, NaN where nothing is live
    case = by_name("noise-leaving-S64-trim0_0")
    got = plan.stack_clip_batch(case.frames, *tables(case.maps), fills=case.fills)
    want = cr.stack_clip_ref(case.frames, case.maps, case.fills, sc.SHAPE, sc.SHAPE, 1)[0]
    assert got.shape == sc.SHAPE and same(got, want, nan_any_payload=True)
    dead = plan.stack_clip_batch(frames, *tables(sc.maps_of("nan_all", 2)), fills=fills)
    assert dead.shape == sc.SHAPE and np.isnan(dead).all()


def test_argument_errors_write_nothing(siftlib):
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    plan = batch_plan()
    frames = sc.frames_of("noise", 65)
    maps, fills = sc.maps_of("shift", 65), sc.fills_of(65)
    ptrs = host_pointers(frames)
    holed = host_pointers(frames)
    holed[1] = None
    tab = table(maps)
    out = np.full(sc.OUTS[1], -77.0, F)
    cov = np.full(sc.OUTS[1], -5, np.int32)
    kept = np.full(sc.OUTS[1], -6, np.int32)
    weights = lambda *v: np.array(v + (1.0,) * (65 - len(v)), F)       # noqa: E731
    args = dict(h=plan._handle, images=ptrs, n=3, out=out.ctypes.data, cov=cov.ctypes.data, kept=kept.ctypes.data, ow=sc.OUTS[1][1],
                oh=sc.OUTS[1][0], maps=tab.ctypes.data, fills=fills.ctypes.data, w=None, reject=1, lo=0, hi=1, kl=3.0, kh=3.0, iters=3)

    def rc_of(**kw):
        a = dict(args); a.update(kw)
        w = a["w"]
        return siftlib.siftmi_batch_stack_clip(a["h"], a["images"], a["n"], 0, a["out"], a["cov"], a["kept"], 0, a["ow"], a["oh"], a["maps"],
                                               a["fills"], None if w is None else w.ctypes.data, 1, a["reject"], a["lo"], a["hi"],
                                               C.c_float(a["kl"]), C.c_float(a["kh"]), a["iters"], C.c_float(0.0), None)
    for good in (dict(), dict(n=64, reject=0, lo=31, hi=32), dict(lo=63, hi=0), dict(lo=0, hi=63), dict(kl=np.inf, kh=np.inf), dict(iters=0),
                 dict(cov=None), dict(kept=None), dict(cov=None, kept=None), dict(w=weights(0.5, 3.0, 1e-30)), dict(w=weights(1.0, 1.0, 1.0, np.nan))):
        assert rc_of(**good) == 0, good                          # (the fourth weight is beyond the three frames: not read)
    out[...] = -77.0; cov[...] = -5; kept[...] = -6
    rgb = sp.BatchPlan(shape=sc.SHAPE + (3,), dtype=np.uint8, lanes=1)
    for bad in (dict(h=None), dict(images=None), dict(maps=None), dict(fills=None), dict(out=None), dict(images=holed), dict(ow=-1), dict(oh=-1),
                dict(n=-1), dict(n=65536), dict(oh=262141), dict(h=rgb._handle),                   # what siftmi_batch_stack refuses
                dict(n=65), dict(n=65, reject=0), dict(reject=2), dict(reject=-1), dict(lo=-1), dict(hi=-1), dict(lo=32, hi=32),
                dict(lo=0, hi=64), dict(lo=64, hi=0), dict(lo=2 ** 31 - 1, hi=2 ** 31 - 1), dict(reject=0, lo=32, hi=32), dict(kl=0.0), dict(kh=0.0),
                dict(kl=-3.0), dict(kl=np.nan), dict(kh=np.nan), dict(kh=-np.inf), dict(reject=0, kl=0.0), dict(iters=-1),
                dict(w=weights(0.0)), dict(w=weights(1.0, -1.0)), dict(w=weights(1.0, 1.0, np.nan)), dict(w=weights(np.inf)),
                dict(w=weights(-np.inf)), dict(reject=0, w=weights(0.0))):
        assert rc_of(**bad) == _lib.EINVAL, bad
        assert siftlib.siftmi_last_error()
    assert (out == -77.0).all() and (cov == -5).all() and (kept == -6).all()
    # the Python layer: ValueError before the call
    M, off = tables(maps)
    few = (frames[:3], M[:3], off[:3])
    with pytest.raises(ValueError):
        plan.stack_clip_batch(frames, M, off, fills)                                  # 65 frames
    assert plan.stack_clip_batch(frames[:64], M[:64], off[:64], fills[:64]).shape == sc.SHAPE
    for bad in (dict(reject="median"), dict(reject=None), dict(trim=(32, 32)), dict(trim=(0, 64)), dict(trim=(-1, 0)), dict(trim=(0, -1)),
                dict(kappa=(0.0, 3.0)), dict(kappa=(3.0, np.nan)), dict(kappa=(-1.0, 3.0)), dict(iters=-1), dict(weights=[1.0, 0.0, 1.0]),
                dict(weights=[1.0, -1.0, 1.0]), dict(weights=[np.nan, 1.0, 1.0]), dict(weights=[1.0, 1.0, np.inf]), dict(weights=[1.0, 1.0]),
                dict(weights=[1.0] * 4), dict(out="pinned")):
        with pytest.raises(ValueError):
            plan.stack_clip_batch(*few, **bad)
    with pytest.raises(ValueError):
        plan.stack_clip_batch(frames[:2], M[:1], off[:2])
    with pytest.raises(RuntimeError):
        plan.stack_clip_batch([frames[0], frames[1][:-1]], M[:2], off[:2])
    with pytest.raises(RuntimeError):
        rgb.stack_clip_batch([np.zeros(sc.SHAPE + (3,), np.uint8)] * 2, M[:2], off[:2])
    assert plan.stack_clip_batch(*few, kappa=(np.inf, 0.5), trim=(63, 0), weights=[0.5, 1, 3]).shape == sc.SHAPE


# ------------------------------------------------------------------------------------------------------------------- ordering
def test_a_frame_produced_late_on_a_side_stream_is_waited_for(siftlib):
    """tests/ordering_cases.py's late producer: the last frame's tensor holds a decoy while a side stream, behind a delay, copies
    the real frame into it; the call is made inside that window and must return the result for the real frame"""
    import torch
    plan = batch_plan()
    S = oc.STACK_S
    real, decoy = sc.frames_of("noise", S, seed=1), sc.frames_of("noise", S, seed=2)
    maps, fills = sc.maps_of("shift", S), sc.fills_of(S)
    Ms, offs = tables(maps)
    for p in (dict(reject="trim", trim=(1, 1)), dict(reject="sigma", kappa=(1.0, 1.0))):
        want = list(cr.stack_clip_ref(real, maps, fills, sc.SHAPE, oc.STACK_OUT, 1, empty=oc.STACK_EMPTY, **p))
        wrong = list(cr.stack_clip_ref(real[:-1] + [decoy[-1]], maps, fills, sc.SHAPE, oc.STACK_OUT, 1, empty=oc.STACK_EMPTY, **p))
        assert not oc.same(want, wrong)
        tensors = [oc.to_device(f) for f in real]
        torch.cuda.synchronize()

        def call():
            return [np.array(a) for a in plan.stack_clip_batch(tensors, Ms, offs, fills, out_shape=oc.STACK_OUT, empty=oc.STACK_EMPTY, counts=True, **p)]
        assert oc.same(call(), want)
        delay = oc.delay_for(oc.timed(call))
        for k, stream in enumerate(oc.side_streams()):
            done = oc.late(tensors[-1], real[-1], decoy[-1], stream, delay)
            oc.window_open(done, "stack_clip %s" % p["reject"])
            got = call()
            assert oc.same(got, want), (p["reject"], k, "the call read the last frame before the caller's stream had written it")
            assert done.query(), (p["reject"], k)
        # and an output produced late: the call must write after the caller's stream has
        outs = [torch.zeros(oc.STACK_OUT, dtype=torch.float32, device="cuda")] + [torch.zeros(oc.STACK_OUT, dtype=torch.int32, device="cuda") for _ in range(2)]
        sentinels = [np.full(oc.STACK_OUT, -12345.0, F), np.full(oc.STACK_OUT, 0x5a5a5a5a, np.int32), np.full(oc.STACK_OUT, 0x5a5a5a5a, np.int32)]
        whole, dptrs = device_stack(real)
        pp = dict(dict(reject="sigma", trim=(0, 1), kappa=(3.0, 3.0), iters=3, weights=None), **p)

        def write():
            raw_call(siftlib, dptrs, S, 1, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), 1, oc.STACK_OUT, maps, fills, 1, pp, empty=oc.STACK_EMPTY)
        delay = oc.delay_for(oc.timed(write))
        done = oc.late_many([(t, s, np.zeros_like(s)) for t, s in zip(outs, sentinels)], oc.side_streams()[0], delay)
        oc.window_open(done, "stack_clip outputs")
        write()
        early = not done.query()
        torch.cuda.synchronize()
        assert oc.same([t.cpu().numpy() for t in outs], want) and not early, p["reject"]
        del whole


# ------------------------------------------------------------------------------------------------------- LinearAlign.stack_clip
OFFSETS = [(0, 0), (5, -3), (-8, 8), (2, 7), (-6, -5), (8, 1), (-1, -8)]


def zinger_stack():
    """(reference crop, the 7 clean frames, the same frames with 20 zingers each): tests/test_gpu_stack.py's stack"""
    if "stack" not in _cache:
        big = smooth_noise((320, 320), seed=21, sigma=2.0)
        ref = np.ascontiguousarray(big[32:288, 32:288])
        lo, hi = float(big.min()), float(big.max())
        zinger = F(hi + (hi - lo))
        cells = [(32 + 16 * i, 32 + 16 * j) for i in range(12) for j in range(12)]       # in the reference's coordinates
        rng = np.random.default_rng(5)
        order = rng.permutation(len(cells))[:140]
        clean, dirty = [], []
        for s, (dy, dx) in enumerate(OFFSETS):
            f = np.ascontiguousarray(big[32 + dy:288 + dy, 32 + dx:288 + dx])
            clean.append(f)
            g = f.copy()
            for k in order[20 * s:20 * s + 20]:
                yr, xr = cells[k][0] + int(rng.integers(-3, 4)), cells[k][1] + int(rng.integers(-3, 4))
                g[yr - dy, xr - dx] = zinger                      # at least 10 pixels from every other zinger of the stack
            dirty.append(g)
        _cache["stack"] = (ref, clean, dirty)
    return _cache["stack"]


def aligner():
    import sift_pyocl_amd as sp
    if "la" not in _cache:
        _cache["la"] = sp.LinearAlign(zinger_stack()[0])
    return _cache["la"]


@pytest.mark.parametrize("max_shift", [None, 12])
def test_linear_align_stack_clip(siftlib, max_shift):
    la = aligner()
    ref, clean, dirty = zinger_stack()
    if max_shift is None:
        want_maps = la.align_batch(dirty, return_all=True)
    else:
        want_maps = la.align_batch_window(dirty, max_shift, return_all=True)
    kw = {} if max_shift is None else dict(max_shift=max_shift)
    del la.events[:]
    la.profile = True                                         # (the aligner's own event list only: its plans were created without)
    try:
        res = la.stack_clip(dirty, reject="trim", trim=(0, 1), return_all=True, **kw)
    finally:
        la.profile = False
    assert [name for name, _ in la.events] == ["stack_clip_batch"] and la.events[0][1].ms > 0.0 and la.last_stack_ms > 0.0
    del la.events[:]
    assert "result" not in res and set(res) == (set(want_maps) - {"result"}) | {"stack", "coverage", "kept"}
    for k in ("matrix", "offset", "mode"):
        assert same(np.asarray(res[k]), np.asarray(want_maps[k])), k
    assert (res["mode"] > 0).all()
    maps = [(res["matrix"][s].reshape(4), res["offset"][s]) for s in range(7)]
    shape = clean[0].shape
    vals, live = sr.samples(dirty, maps, res["fill"], shape, la.outshape, 1)
    want = cr.reduce_clip(vals, live, "trim", trim=(0, 1))
    agrees((res["stack"], res["coverage"], res["kept"]), want, "stack_clip", max_shift)
    assert res["stack"].dtype == F and res["coverage"].dtype == res["kept"].dtype == np.int32
    # without the zingers, on the same maps: wherever all seven frames are live the result lies within the clean samples' range
    cvals, clive = sr.samples(clean, maps, res["fill"], shape, la.outshape, 1)
    full = want[1] == 7
    assert full.sum() > 200 * 200 and clive[:, full].all() and (res["kept"][full] == 6).all()
    lo, hi = cvals[:, full].min(axis=0), cvals[:, full].max(axis=0)
    assert ((res["stack"][full] >= lo) & (res["stack"][full] <= hi)).all()
    mean = la.stack(dirty, reduce="mean", **kw)
    assert (mean[full] > hi).sum() >= 100                     # 140 zingers, each lifts at least its nearest pixel
    # the plain return value on the host and on the device, and the sigma rule with weights through the same method
    plain = la.stack_clip(dirty, reject="trim", trim=(0, 1), **kw)
    assert isinstance(plain, np.ndarray) and same(plain, res["stack"], nan_any_payload=True)
    dev = la.stack_clip(dirty, reject="trim", trim=(0, 1), out="device", **kw)
    assert dev.is_cuda and same(dev.cpu().numpy(), res["stack"], nan_any_payload=True)
    w = np.array([0.5, 1, 3, 1, 0.5, 3, 1], F)
    sig = la.stack_clip(dirty, kappa=(3.0, 1.5), iters=2, weights=w, return_all=True, **kw)
    agrees((sig["stack"], sig["coverage"], sig["kept"]), cr.reduce_clip(vals, live, "sigma", kappa=(3.0, 1.5), iters=2, weights=w), "sigma", max_shift)
    # stack and align_batch on the same aligner are not disturbed
    again = la.align_batch(dirty, return_all=True) if max_shift is None else la.align_batch_window(dirty, max_shift, return_all=True)
    assert same(again["result"], want_maps["result"]) and same(again["matrix"], want_maps["matrix"])


def test_linear_align_stack_clip_refuses_what_it_cannot_do(siftlib):
    import sift_pyocl_amd as sp
    la = aligner()
    ref, clean, dirty = zinger_stack()
    empty = la.stack_clip([], empty=4.0)
    assert empty.shape == la.outshape and (empty == 4.0).all()
    for bad in (dict(reject="mode"), dict(out="pinned"), dict(expected_shift=(1.0, 0.0)), dict(trim=(40, 40)), dict(kappa=(0.0, 1.0)), dict(iters=-2),
                dict(weights=[1.0, 0.0, 1.0]), dict(weights=[1.0, 1.0])):
        with pytest.raises(ValueError):
            la.stack_clip(clean[:3], **bad)
    colour = np.random.default_rng(5).integers(0, 256, (72, 90, 3), dtype=np.uint8)
    rgb = sp.LinearAlign(colour)
    with pytest.raises(RuntimeError):
        rgb.stack_clip([colour])
