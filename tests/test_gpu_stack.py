"""GPU tests of the stack-reduction row: stack_reduce_kernel / stack_median_kernel (csrc/k_stack.hpp) through siftmi_batch_stack,
BatchPlan.stack_batch and LinearAlign.stack.

Every crafted stack of tests/stack_cases.py is run with every reducer and compared with tests/stack_ref.py bit for bit (a NaN
matches any NaN).  The warp kernels are the yardstick for the sample itself: a stack of one frame summed is transform_batch's
plane wherever the frame is live, and the mean of five frames is the ordered mean of transform_batch's five planes.

The stack of the LinearAlign.stack tests: the reference is a 256 x 256 crop of a 320 x 320 smooth_noise plane, the 7 frames are
crops at integer offsets within +-8 pixels, each with 20 planted zingers.  A zinger sits in one cell of a 16-pixel lattice of the
reference's coordinates and no two share a cell, so after alignment a pixel sees a zinger in at most one of its 7 samples.
"""
import ctypes as C

import numpy as np
import pytest

import stack_cases as sc
import stack_ref as sr
from util import smooth_noise
from warp_ref import same

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 256                                     # bytes
EMPTY = {"sum": -12345.0, "mean": float("nan"), "median": 0.5}
CODE = {"sum": 0, "mean": 1, "median": 2}
_cache = {}


def batch_plan():
    import sift_pyocl_amd as sp
    if "plan" not in _cache:
        _cache["plan"] = sp.BatchPlan(shape=sc.SHAPE, dtype=F, lanes=1)
    return _cache["plan"]


def sampled(case):
    key = ("samples", case.name)
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


def raw_call(siftlib, plan, ptrs, n, is_dev, out_ptr, cov_ptr, out_is_dev, out_shape, maps, fills, mode, reduce, empty, want_rc=0):
    """siftmi_batch_stack with plain addresses; returns kernel_ms"""
    tab = table(maps)
    fills = np.ascontiguousarray(fills, F)
    ms = C.c_double(-1.0)
    rc = siftlib.siftmi_batch_stack(plan._handle, ptrs, n, is_dev, out_ptr, cov_ptr, out_is_dev, out_shape[1], out_shape[0], tab.ctypes.data,
                                    fills.ctypes.data, mode, CODE[reduce], C.c_float(empty), C.byref(ms))
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


def guarded_call(siftlib, ptrs, n, is_dev, out_shape, maps, fills, mode, reduce, empty, with_cov):
    """a device plane and a device coverage, each between guard bytes in one buffer: (plane, coverage or None) on the host, after
    checking that no guard byte changed"""
    import torch
    nbytes = out_shape[0] * out_shape[1] * 4
    buf = torch.full((3 * GUARD + 2 * nbytes,), 0xa5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    p_at, c_at = GUARD, 2 * GUARD + nbytes
    torch.cuda.synchronize()
    raw_call(siftlib, batch_plan(), ptrs, n, is_dev, buf.data_ptr() + p_at, buf.data_ptr() + c_at if with_cov else None, 1, out_shape, maps, fills,
             mode, reduce, empty)
    host = buf.cpu().numpy()
    plane = host[p_at:p_at + nbytes].view(F).reshape(out_shape).copy()
    cov = host[c_at:c_at + nbytes].view(np.int32).reshape(out_shape).copy()
    keep = np.ones(host.shape, bool)
    keep[p_at:p_at + nbytes] = False
    if with_cov:
        keep[c_at:c_at + nbytes] = False
    assert (host[keep] == 0xa5).all(), (out_shape, reduce, "bytes outside the plane%s were written" % (" and the coverage" if with_cov else ""))
    return plane, (cov if with_cov else None)


# ------------------------------------------------------------------------------------------------------ the crafted stacks
@pytest.mark.parametrize("case", sc.cases(), ids=[c.name for c in sc.cases()])
def test_every_case_and_reducer_is_the_reference_bit_for_bit(siftlib, case):
    """per reducer two calls that together take every pointer path: host or device frames, host or device result (the device one
    between guards), with and without the coverage"""
    plan = batch_plan()
    vals, live = sampled(case)
    S = len(case.frames)
    hptrs = host_pointers(case.frames)
    whole, dptrs = device_stack(case.frames)
    for reduce in sc.reducers_of(case):
        empty = EMPTY[reduce]
        want, want_c = sr.reduce_samples(vals, live, reduce, empty)
        # host frames to a host result
        out = np.full(case.out_shape, -77.0, F)
        cov = np.full(case.out_shape, -5, np.int32)
        with_cov = reduce != "median"
        ms = raw_call(siftlib, plan, hptrs, S, 0, out.ctypes.data, cov.ctypes.data if with_cov else None, 0, case.out_shape, case.maps, case.fills,
                      case.mode, reduce, empty)
        assert ms > 0.0
        assert same(out, want, nan_any_payload=True), (case.name, reduce, "host to host", int((out.view(np.uint32) != want.view(np.uint32)).sum()))
        assert np.array_equal(cov, want_c) if with_cov else (cov == -5).all(), (case.name, reduce)
        # device frames to a device result
        got, got_c = guarded_call(siftlib, dptrs, S, 1, case.out_shape, case.maps, case.fills, case.mode, reduce, empty, with_cov=not with_cov)
        assert same(got, want, nan_any_payload=True), (case.name, reduce, "device to device")
        assert got_c is None or np.array_equal(got_c, want_c), (case.name, reduce)
    # the mixed paths once per case: host frames to a device result, device frames to a host result
    reduce = sc.reducers_of(case)[-1]
    want, want_c = sr.reduce_samples(vals, live, reduce, EMPTY[reduce])
    got, got_c = guarded_call(siftlib, hptrs, S, 0, case.out_shape, case.maps, case.fills, case.mode, reduce, EMPTY[reduce], with_cov=True)
    assert same(got, want, nan_any_payload=True) and np.array_equal(got_c, want_c), (case.name, reduce, "host to device")
    out = np.full(case.out_shape, -77.0, F)
    cov = np.full(case.out_shape, -5, np.int32)
    raw_call(siftlib, plan, dptrs, S, 1, out.ctypes.data, cov.ctypes.data, 0, case.out_shape, case.maps, case.fills, case.mode, reduce, EMPTY[reduce])
    assert same(out, want, nan_any_payload=True) and np.array_equal(cov, want_c), (case.name, reduce, "device to host")
    del whole


@pytest.mark.parametrize("reduce", sr.REDUCERS)
def test_output_shapes_around_the_tile_between_guards(siftlib, reduce):
    """a store beyond a row or the plane shows here: widths around the 64-column tile, heights around its 4 rows"""
    case = {c.name: c for c in sc.cases()}["noise-rot-S5-41x70-m1"]
    whole, dptrs = device_stack(case.frames)
    for out_shape in ((1, 1), (1, 63), (4, 64), (5, 65), (3, 129), (9, 2)):
        want, want_c = sr.stack_ref(case.frames, case.maps, case.fills, sc.SHAPE, out_shape, 1, reduce, EMPTY[reduce])
        got, got_c = guarded_call(siftlib, dptrs, 5, 1, out_shape, case.maps, case.fills, 1, reduce, EMPTY[reduce], with_cov=True)
        assert same(got, want, nan_any_payload=True) and np.array_equal(got_c, want_c), (reduce, out_shape)
    del whole


# ------------------------------------------------------------------------------------------- against the warp kernels themselves
def test_a_stack_of_one_summed_is_the_warps_plane_where_the_frame_is_live(siftlib):
    plan = batch_plan()
    by = {c.name: c for c in sc.cases()}
    seen_dead = seen_live = 0
    for name, s in (("noise-rot-S5-41x70-m1", 1), ("noise-half-S5-41x70-m1", 3), ("noise-leaving-S8-41x70-m1", 5), ("noise-half-S5-41x70-m0", 2),
                    ("nan-identity-S5-37x53-m1", 0), ("noise-nan_mid-S4-41x70-m1", 2)):
        case = by[name]
        frame, (M, off), fill = case.frames[s], case.maps[s], case.fills[s:s + 1]
        Ms, offs = tables([(M, off)])
        warped = plan.transform_batch([frame], Ms, offs, fill, out_shape=case.out_shape, mode=case.mode)[0]
        plane, cov = plan.stack_batch([frame], Ms, offs, fill, out_shape=case.out_shape, mode=case.mode, reduce="sum", empty=-3.0, coverage=True)
        assert isinstance(plane, np.ndarray) and plane.dtype == F and cov.dtype == np.int32 and plane.shape == cov.shape == case.out_shape
        assert plan.last_stack_ms > 0.0
        live = sr.live_mask(M, off, sc.SHAPE, case.out_shape)
        assert np.array_equal(cov, live.astype(np.int32)), name
        assert same(plane[live], warped[live], nan_any_payload=True), name
        assert (plane[~live] == F(-3.0)).all() and same(warped[~live], np.full(int((~live).sum()), fill[0], F)), name
        seen_dead += int((~live).sum()); seen_live += int(live.sum())
        for reduce in ("mean", "median"):                       # one value: its own mean and median
            again = plan.stack_batch([frame], Ms, offs, fill, out_shape=case.out_shape, mode=case.mode, reduce=reduce, empty=-3.0)
            assert same(again, plane, nan_any_payload=True), (name, reduce)
    assert seen_dead > 1000 and seen_live > 1000


def test_the_mean_of_five_is_the_ordered_mean_of_the_warps_planes(siftlib):
    import torch
    plan = batch_plan()
    for name in ("noise-rot-S5-41x70-m1", "noise-half-S5-41x70-m1", "noise-leaving-S5-41x70-m1", "inf-identity-S5-37x53-m0"):
        case = {c.name: c for c in sc.cases()}[name]
        Ms, offs = tables(case.maps)
        planes = plan.transform_batch(case.frames, Ms, offs, case.fills, out_shape=case.out_shape, mode=case.mode)
        live = np.stack([sr.live_mask(M, off, sc.SHAPE, case.out_shape) for M, off in case.maps])
        for reduce in sr.REDUCERS:
            want, want_c = sr.reduce_samples(np.asarray(planes), live, reduce, empty=np.nan)
            got, cov = plan.stack_batch(np.stack(case.frames), Ms.reshape(-1, 2, 2), offs, case.fills, out_shape=case.out_shape, mode=case.mode,
                                        reduce=reduce, coverage=True)
            assert same(got, want, nan_any_payload=True) and np.array_equal(cov, want_c), (name, reduce)
            # device tensors in, device tensors out; without the coverage a single tensor comes back
            tens = [torch.from_numpy(f).cuda() for f in case.frames]
            dev = plan.stack_batch(tens, Ms, offs, case.fills, out_shape=case.out_shape, mode=case.mode, reduce=reduce, out="device")
            assert isinstance(dev, torch.Tensor) and dev.is_cuda and dev.dtype == torch.float32
            assert same(dev.cpu().numpy(), want, nan_any_payload=True), (name, reduce)
            dev, dcov = plan.stack_batch(tens, Ms, offs, case.fills, out_shape=case.out_shape, mode=case.mode, reduce=reduce, coverage=True,
                                         out="device")
            assert dcov.is_cuda and dcov.dtype == torch.int32 and np.array_equal(dcov.cpu().numpy(), want_c)
    # the default output shape is the plan's, the default reducer the mean, the default empty value NaN
    case = {c.name: c for c in sc.cases()}["noise-leaving-S5-41x70-m1"]
    Ms, offs = tables(case.maps)
    got = plan.stack_batch(case.frames, Ms, offs, case.fills)
    want, _ = sr.stack_ref(case.frames, case.maps, case.fills, sc.SHAPE, sc.SHAPE, 1, "mean", np.nan)
    assert got.shape == sc.SHAPE and same(got, want, nan_any_payload=True)


# ------------------------------------------------------------------------------------------------------- edges of the interface
def test_no_frame_fills_the_plane_and_an_empty_output_launches_nothing(siftlib):
    import torch
    plan = batch_plan()
    frames = sc.frames_of("noise", 2)
    hptrs = host_pointers(frames)
    maps, fills = sc.maps_of("shift", 2), sc.fills_of(2)
    for reduce in sr.REDUCERS:
        out = np.full(sc.OUTS[1], -77.0, F)
        cov = np.full(sc.OUTS[1], -5, np.int32)
        raw_call(siftlib, plan, None, 0, 0, out.ctypes.data, cov.ctypes.data, 0, sc.OUTS[1], [], np.zeros(0, F), 1, reduce, 6.25)
        assert (out == F(6.25)).all() and (cov == 0).all(), reduce
        got, got_c = guarded_call(siftlib, None, 0, 1, sc.OUTS[1], [], np.zeros(0, F), 1, reduce, float("nan"), with_cov=True)
        assert np.isnan(got).all() and (got_c == 0).all(), reduce
        got, _ = guarded_call(siftlib, None, 0, 0, (5, 65), [], np.zeros(0, F), 1, reduce, -1.5, with_cov=False)
        assert (got == F(-1.5)).all(), reduce
        plane, c = plan.stack_batch([], np.zeros((0, 2, 2), F), np.zeros((0, 2), F), out_shape=(3, 7), reduce=reduce, empty=9.0, coverage=True)
        assert plane.shape == (3, 7) and (plane == 9.0).all() and c.dtype == np.int32 and (c == 0).all()
        for n, out_shape in ((2, (0, 7)), (2, (5, 0)), (0, (0, 0))):
            host = np.full(64, 0x5a, np.uint8)
            ms = raw_call(siftlib, plan, hptrs, n, 0, host.ctypes.data, host.ctypes.data + 32, 0, out_shape, maps[:n], fills[:n], 1, reduce, 1.0)
            assert ms == 0.0 and (host == 0x5a).all()
            dev = torch.full((64,), 0xa5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ms = raw_call(siftlib, plan, hptrs, n, 0, dev.data_ptr(), dev.data_ptr() + 32, 1, out_shape, maps[:n], fills[:n], 1, reduce, 1.0)
            assert ms == 0.0 and bool((dev == 0xa5).all())
    assert plan.stack_batch(frames, *tables(maps), fills=0.0, out_shape=(0, 7)).shape == (0, 7)


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
    args = dict(h=plan._handle, images=ptrs, n=2, out=out.ctypes.data, cov=cov.ctypes.data, ow=sc.OUTS[1][1], oh=sc.OUTS[1][0], maps=tab.ctypes.data,
                fills=fills.ctypes.data, reduce=1)

    def rc_of(**kw):
        a = dict(args); a.update(kw)
        return siftlib.siftmi_batch_stack(a["h"], a["images"], a["n"], 0, a["out"], a["cov"], 0, a["ow"], a["oh"], a["maps"], a["fills"], 1,
                                          a["reduce"], C.c_float(0.0), None)
    assert rc_of() == 0 and rc_of(n=64, reduce=2) == 0 and rc_of(n=65, reduce=0) == 0 and rc_of(cov=None) == 0
    out[...] = -77.0; cov[...] = -5
    rgb = sp.BatchPlan(shape=sc.SHAPE + (3,), dtype=np.uint8, lanes=1)
    for bad in (dict(h=None), dict(images=None), dict(maps=None), dict(fills=None), dict(out=None), dict(images=holed), dict(reduce=3),
                dict(reduce=-1), dict(n=65, reduce=2), dict(ow=-1), dict(oh=-1), dict(n=-1), dict(n=65536), dict(oh=262141), dict(h=rgb._handle)):
        assert rc_of(**bad) == _lib.EINVAL, bad
        assert siftlib.siftmi_last_error()
    assert (out == -77.0).all() and (cov == -5).all()
    # the Python layer
    M, off = tables(maps)
    with pytest.raises(ValueError):
        plan.stack_batch(frames, M, off, fills, reduce="median")                    # 65 frames
    assert plan.stack_batch(frames[:64], M[:64], off[:64], fills[:64], reduce="median").shape == sc.SHAPE
    assert plan.stack_batch(frames, M, off, fills, reduce="mean").shape == sc.SHAPE
    for name in ("max", "Mean", None, 1):
        with pytest.raises(ValueError):
            plan.stack_batch(frames[:2], M[:2], off[:2], reduce=name)
    with pytest.raises(ValueError):
        plan.stack_batch(frames[:2], M[:2], off[:2], out="pinned")
    with pytest.raises(ValueError):
        plan.stack_batch(frames[:2], M[:1], off[:2])
    with pytest.raises(RuntimeError):
        plan.stack_batch([frames[0], frames[1][:-1]], M[:2], off[:2])
    rgb_frames = [np.zeros(sc.SHAPE + (3,), np.uint8)] * 2
    with pytest.raises(RuntimeError):
        rgb.stack_batch(rgb_frames, M[:2], off[:2])
    assert rgb.transform_batch(rgb_frames, M[:2], off[:2]).shape == (2,) + sc.SHAPE + (3,)      # the warp of an RGB plan is not touched


# ----------------------------------------------------------------------------------------------------------- LinearAlign.stack
OFFSETS = [(0, 0), (5, -3), (-8, 8), (2, 7), (-6, -5), (8, 1), (-1, -8)]


def zinger_stack():
    """(reference crop, the 7 clean frames, the same frames with 20 zingers each)"""
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


def check_stack_result(la, res, want_maps, reduce, clean, dirty):
    assert "result" not in res
    for k in ("matrix", "offset", "mode"):
        assert same(np.asarray(res[k]), np.asarray(want_maps[k])), k
    assert set(res) == (set(want_maps) - {"result"}) | {"stack", "coverage"}
    assert (res["mode"] > 0).all()
    maps = [(res["matrix"][s].reshape(4), res["offset"][s]) for s in range(7)]
    shape = clean[0].shape
    want, want_c = sr.stack_ref(dirty, maps, res["fill"], shape, la.outshape, 1, reduce, np.nan)
    assert res["stack"].dtype == F and res["coverage"].dtype == np.int32
    assert same(res["stack"], want, nan_any_payload=True), reduce
    assert np.array_equal(res["coverage"], want_c)
    # what every pixel would hold without the zingers, on the same maps
    vals, live = sr.samples(clean, maps, res["fill"], shape, la.outshape, 1)
    full = want_c == 7
    assert full.sum() > 200 * 200 and live[:, full].all()
    return res["stack"], vals[:, full].min(axis=0), vals[:, full].max(axis=0), full


@pytest.mark.parametrize("max_shift", [None, 12])
def test_linear_align_stack(siftlib, max_shift):
    la = aligner()
    ref, clean, dirty = zinger_stack()
    if max_shift is None:
        want_maps = la.align_batch(dirty, return_all=True)
    else:
        want_maps = la.align_batch_window(dirty, max_shift, return_all=True)
    for s, (dy, dx) in enumerate(OFFSETS):                      # the estimate finds the crops, to within a pixel (the windowed
        assert abs(want_maps["offset"][s][0] + dy) < 1.0 and abs(want_maps["offset"][s][1] + dx) < 1.0, s      # matcher pairs some zingers)
    kw = {} if max_shift is None else dict(max_shift=max_shift)
    med, lo, hi, full = check_stack_result(la, la.stack(dirty, reduce="median", return_all=True, **kw), want_maps, "median", clean, dirty)
    mean, lo2, hi2, full2 = check_stack_result(la, la.stack(dirty, reduce="mean", return_all=True, **kw), want_maps, "mean", clean, dirty)
    assert la.last_stack_ms > 0.0
    # a pixel sees a zinger in at most one of its seven samples: the median stays within the clean samples, the mean does not
    assert ((med[full] >= lo) & (med[full] <= hi)).all()
    assert (mean[full2] > hi2).sum() >= 100                   # 140 zingers, each lifts at least its nearest pixel
    # the plain return value, on the host and on the device
    plain = la.stack(dirty, reduce="median", **kw)
    assert isinstance(plain, np.ndarray) and same(plain, med, nan_any_payload=True)
    dev = la.stack(dirty, reduce="median", out="device", **kw)
    assert dev.is_cuda and same(dev.cpu().numpy(), med, nan_any_payload=True)
    # align_batch on the same aligner is not disturbed
    again = la.align_batch(dirty, return_all=True) if max_shift is None else la.align_batch_window(dirty, max_shift, return_all=True)
    assert same(again["result"], want_maps["result"]) and same(again["matrix"], want_maps["matrix"])


def test_linear_align_stack_leaves_out_a_frame_without_a_match_and_refuses_what_it_cannot_do(siftlib, caplog):
    import sift_pyocl_amd as sp
    la = aligner()
    ref, clean, dirty = zinger_stack()
    frames = [clean[1], np.zeros_like(ref), clean[2]]
    res = la.stack(frames, reduce="sum", empty=-1.0, return_all=True)
    assert res["mode"][1] == 0 and res["mode"][0] > 0 and res["mode"][2] > 0 and np.isnan(res["matrix"][1]).all()
    assert any("frame 1" in r.getMessage() for r in caplog.records)
    assert res["coverage"].max() == 2 and res["coverage"].min() == 0
    maps = [(res["matrix"][s].reshape(4), res["offset"][s]) for s in range(3)]
    want, want_c = sr.stack_ref(frames, maps, res["fill"], ref.shape, la.outshape, 1, "sum", -1.0)
    assert same(res["stack"], want, nan_any_payload=True) and np.array_equal(res["coverage"], want_c)
    empty = la.stack([], empty=4.0)
    assert empty.shape == la.outshape and (empty == 4.0).all()
    with pytest.raises(ValueError):
        la.stack(frames, reduce="mode")
    with pytest.raises(ValueError):
        la.stack(frames, out="pinned")
    with pytest.raises(ValueError):
        la.stack(frames, expected_shift=(1.0, 0.0))
    colour = np.random.default_rng(5).integers(0, 256, (72, 90, 3), dtype=np.uint8)
    rgb = sp.LinearAlign(colour)
    with pytest.raises(RuntimeError):
        rgb.stack([colour])
