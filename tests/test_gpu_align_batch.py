"""GPU tests of the align_batch row: the batched warp (transform_batch_kernel / transform_rgb_batch_kernel, csrc/k_align_batch.hpp)
through siftmi_batch_transform and BatchPlan.transform_batch, the per-frame minima of siftmi_batch_minmax, and
LinearAlign.align_batch end to end.

The warp is compared with tests/warp_ref.py frame by frame, bit for bit.  Keypoint order differs between a BatchPlan lane and a
SiftPlan, so lists are compared sorted and pairs as sets of records; nothing compares the batch with the loop bit for bit where
the order of a sum enters (the affine fit): there the tolerances are those tests/test_gpu_align.py gives two summation orders of
one fit (matrix 2e-6, offset 2e-4).

The stack of the align_batch tests is cut from one smooth_noise plane as tests/test_gpu_align.py cuts its frames.  Its frames
were chosen on the CPU with oracle.keypoints / oracle.match against the reference crop (750 keypoints); pairs per frame there:
    0, 1   crops moved by a few pixels                     657 and 701 pairs   affine
    2      the content kept in a 48 x 48 window             15 pairs            shift (fewer than 18)
    3      all zero                                          no keypoint         none
    4      the content kept in a 20 x 20 window              1 pair             shift; no consensus possible (fewer than three)
    5      the content kept in a 28 x 28 window              6 keypoints, 0 pairs   none
    6      the content kept in a 64 x 64 window             28 pairs            affine
The tests assert these modes, so that no branch is skipped silently.
"""
import ctypes as C

import numpy as np
import pytest

import align_batch_ref as ab
import warp_cases as wc
from util import assert_same_keypoints, smooth_noise, sort_rows
from warp_ref import same, warp_ref

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 256
S9 = 9                                      # more than one frame per XCD (8)
_cache = {}


# ------------------------------------------------------------------------------------------------------------ warp: inputs
def batch_plan(kind, lanes=1):
    """one BatchPlan per element type of warp_cases.SHAPE, shared by the warp tests"""
    import sift_pyocl_amd as sp
    key = ("plan", kind, lanes)
    if key not in _cache:
        shape = wc.SHAPE + ((3,) if kind == "rgb" else ())
        _cache[key] = sp.BatchPlan(shape=shape, dtype=np.uint8 if kind == "rgb" else np.float32, lanes=lanes)
    return _cache[key]


def frames9(kind):
    """nine different planes of warp_cases.SHAPE (the first is the crafted cases' own)"""
    key = ("frames", kind)
    if key not in _cache:
        out = [np.array(wc.image((kind, wc.SHAPE)))]
        for s in range(1, S9):
            rng = np.random.default_rng(500 + s)
            if kind == "rgb":
                out.append(rng.integers(0, 256, wc.SHAPE + (3,), dtype=np.uint8))
            else:
                out.append((rng.random(wc.SHAPE, dtype=F) * F(500) - F(100)).astype(F))
        _cache[key] = out
    return _cache[key]


def maps9():
    """[(M, off)]: identity, rot30, zoom_corner, two of the lattice, three non-finite ones of warp_cases, and all NaN"""
    by = {c.name: c for c in wc.cases()}
    names = ["f1-identity-gray-m1", "f1-rot30-gray-m1", "f1-zoom_corner-gray-m1", "f2-lo_lo-gray-m1", "f2-hi_hi-gray-m1",
             "f4-nan_coeff-gray-m1", "f4-inf_coeff-gray-m1", "f4-ninf_offset-gray-m1"]
    out = [(by[n].M, by[n].off) for n in names]
    assert all(by[n].out_shape == wc.OUT for n in names)
    out.append(((np.nan,) * 4, (np.nan,) * 2))
    assert len(out) == S9
    return out


def fills9():
    return np.array([wc.FILLS[s % len(wc.FILLS)] for s in range(S9)], F)


def expected(kind, frames, maps, fills, out_shape, mode):
    return np.stack([warp_ref(f, M, off, out_shape, fill, mode)[0] for f, (M, off), fill in zip(frames, maps, fills)])


def tables(maps):
    return np.array([M for M, _ in maps], F).reshape(-1, 4), np.array([off for _, off in maps], F).reshape(-1, 2)


def raw_call(siftlib, plan, ptrs, n, is_dev, rgb, out_ptr, out_is_dev, out_shape, maps, fills, mode, want_rc=0):
    """siftmi_batch_transform with plain addresses; returns kernel_ms"""
    M, off = tables(maps) if len(maps) else (np.zeros((0, 4), F), np.zeros((0, 2), F))
    tab = np.ascontiguousarray(np.concatenate([M, off], axis=1), F)
    fills = np.ascontiguousarray(fills, F)
    ms = C.c_double(-1.0)
    rc = siftlib.siftmi_batch_transform(plan._handle, ptrs, n, is_dev, 3 if rgb else 1, out_ptr, out_is_dev, out_shape[1], out_shape[0],
                                        tab.ctypes.data, fills.ctypes.data, mode, C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def device_frames(frames):
    """separate device tensors (one allocation each) and their pointer table"""
    import torch
    tens = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    ptrs = (C.c_void_p * max(1, len(tens)))(*[t.data_ptr() for t in tens])
    return tens, ptrs


def guarded(siftlib, kind, frames, maps, fills, out_shape, mode=1):
    """device frames to a device output between guard bytes: the payload is the expected bytes, the guards survive"""
    import torch
    rgb = kind == "rgb"
    want = expected(kind, frames, maps, fills, out_shape, mode)
    tens, ptrs = device_frames(frames)
    buf = torch.full((GUARD + want.nbytes + GUARD,), 0xa5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    torch.cuda.synchronize()
    raw_call(siftlib, batch_plan(kind), ptrs, len(frames), 1, rgb, buf.data_ptr() + GUARD, 1, out_shape, maps, fills, mode)
    host = buf.cpu().numpy()
    got = host[GUARD:GUARD + want.nbytes].view(want.dtype).reshape(want.shape)
    for s in range(len(frames)):
        assert same(got[s], want[s]), (kind, out_shape, "frame %d" % s)
    assert (host[:GUARD] == 0xa5).all() and (host[GUARD + want.nbytes:] == 0xa5).all(), (kind, out_shape, "guard bytes were written")
    del tens


# ------------------------------------------------------------------------------------------------------------- warp: tests
@pytest.mark.parametrize("mode", [1, 0])
@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_nine_host_frames_to_a_host_stack(siftlib, kind, mode):
    frames, maps, fills = frames9(kind), maps9(), fills9()
    if kind == "rgb":
        assert (wc.OUT[0] * wc.OUT[1] * 3) % 4 == 3          # 8319 bytes per frame: the frames start at every alignment mod 4
    want = expected(kind, frames, maps, fills, wc.OUT, mode)
    M, off = tables(maps)
    plan = batch_plan(kind)
    got = plan.transform_batch(frames, M.reshape(-1, 2, 2), off, fills, out_shape=wc.OUT, mode=mode)
    assert isinstance(got, np.ndarray) and got.shape == want.shape and got.dtype == want.dtype
    for s in range(S9):
        assert same(got[s], want[s]), (kind, mode, "frame %d" % s)
    assert plan.last_transform_ms > 0.0
    # the all-NaN map and the non-finite ones: planes of the frame's own fill (where the map reaches)
    assert same(got[8], np.full(want[8].shape, fills[8]).astype(want.dtype))
    # a stack passed as one array, (S, 4) matrices, and the separate pointers of the C ABI give the same bytes
    again = plan.transform_batch(np.stack(frames), M, off, fills, out_shape=wc.OUT, mode=mode)
    assert same(again, got)
    raw = np.full(want.shape, 0x5a, want.dtype) if kind == "rgb" else np.full(want.shape, -77.0, want.dtype)
    ptrs = (C.c_void_p * S9)(*[f.ctypes.data for f in frames])
    ms = raw_call(siftlib, plan, ptrs, S9, 0, kind == "rgb", raw.ctypes.data, 0, wc.OUT, maps, fills, mode)
    assert same(raw, got) and ms > 0.0


@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_device_frames_to_a_device_stack_between_guards(siftlib, kind):
    guarded(siftlib, kind, frames9(kind), maps9(), fills9(), wc.OUT)
    import torch
    tens, _ = device_frames(frames9(kind))
    M, off = tables(maps9())
    got = batch_plan(kind).transform_batch(tens, M, off, fills9(), out_shape=wc.OUT, out="device")
    assert isinstance(got, torch.Tensor) and got.is_cuda
    assert same(got.cpu().numpy(), expected(kind, frames9(kind), maps9(), fills9(), wc.OUT, 1))


@pytest.mark.parametrize("oh", [1, 4, 5])
@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_output_widths_between_guards(siftlib, kind, oh):
    """a store beyond a row, a frame or the stack shows here: one and three frames, widths around the 4-pixel and the 64 / 256
    column steps; with three RGB frames of odd sizes the second and third start off a dword boundary"""
    frames, maps, fills = frames9(kind), maps9(), fills9()
    for ow in (1, 3, 4, 5, 64, 65, 257):
        guarded(siftlib, kind, frames[:1], maps[1:2], fills[1:2], (oh, ow))
        guarded(siftlib, kind, frames[:3], maps[:3], fills[:3], (oh, ow))


@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_no_frame_or_an_empty_output_writes_nothing(siftlib, kind):
    import torch
    plan = batch_plan(kind)
    frames, maps, fills = frames9(kind)[:2], maps9()[:2], fills9()[:2]
    ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
    for n, out_shape in ((0, wc.OUT), (2, (0, 7)), (2, (5, 0)), (2, (0, 0))):
        host = np.full(64, 0x5a, np.uint8)
        ms = raw_call(siftlib, plan, ptrs, n, 0, kind == "rgb", host.ctypes.data, 0, out_shape, maps[:n], fills[:n], 1)
        assert ms == 0.0 and (host == 0x5a).all()
        dev = torch.full((64,), 0xa5, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ms = raw_call(siftlib, plan, ptrs, n, 0, kind == "rgb", dev.data_ptr() + 32, 1, out_shape, maps[:n], fills[:n], 1)
        assert ms == 0.0 and bool((dev == 0xa5).all())
    tail = (3,) if kind == "rgb" else ()
    assert plan.transform_batch([], np.zeros((0, 2, 2), F), np.zeros((0, 2), F), out_shape=wc.OUT).shape == (0,) + wc.OUT + tail
    assert plan.transform_batch(frames, *tables(maps), fills=0.0, out_shape=(0, 7)).shape == (2, 0, 7) + tail


def test_transform_argument_errors(siftlib):
    import torch
    from sift_pyocl_amd import _lib
    for kind in ("gray", "rgb"):
        plan = batch_plan(kind)
        frames, maps, fills = frames9(kind)[:2], maps9()[:2], fills9()[:2]
        ptrs = (C.c_void_p * 2)(*[f.ctypes.data for f in frames])
        sentinel = np.full((2,) + wc.OUT + ((3,) if kind == "rgb" else ()), 0x5a if kind == "rgb" else -77, np.uint8 if kind == "rgb" else F)
        before = sentinel.copy()
        tab = np.ascontiguousarray(np.concatenate(tables(maps), axis=1), F)
        args = dict(images=ptrs, n=2, ch=3 if kind == "rgb" else 1, out=sentinel.ctypes.data, ow=wc.OUT[1], oh=wc.OUT[0], maps=tab.ctypes.data,
                    fills=fills.ctypes.data)

        def rc_of(**kw):
            a = dict(args); a.update(kw)
            return siftlib.siftmi_batch_transform(plan._handle, a["images"], a["n"], 0, a["ch"], a["out"], 0, a["ow"], a["oh"], a["maps"],
                                                  a["fills"], 1, None)
        assert rc_of() == 0
        sentinel[...] = before
        for bad in (dict(images=None), dict(maps=None), dict(fills=None), dict(out=None), dict(ch=2), dict(ch=4), dict(ow=-1), dict(oh=-1),
                    dict(n=-1), dict(n=65536)):
            assert rc_of(**bad) == _lib.EINVAL, bad
            assert siftlib.siftmi_last_error()
        assert same(sentinel, before)
        # the Python layer
        M, off = tables(maps)
        with pytest.raises(RuntimeError):                          # mixed residency
            plan.transform_batch([frames[0], torch.from_numpy(frames[1]).cuda()], M, off)
        with pytest.raises(RuntimeError):                          # frame shape
            plan.transform_batch([frames[0], frames[1][:-1]], M, off)
        with pytest.raises(RuntimeError):                          # element type
            plan.transform_batch([frames[0], frames[1].astype(np.float64)], M, off)
        for bad_m, bad_off, bad_fill in ((M[:1], off, 0.0), (M.reshape(-1, 2), off, 0.0), (M, off[:, :1], 0.0), (M, off, np.zeros(3, F))):
            with pytest.raises(ValueError):
                plan.transform_batch(frames, bad_m, bad_off, bad_fill)
        with pytest.raises(ValueError):
            plan.transform_batch(frames, M, off, out="pinned")
        if kind == "rgb":
            for fill in (-0.5, 255.5, np.array([0.0, np.nan], F)):
                with pytest.raises(ValueError):
                    plan.transform_batch(frames, M, off, fill)


# ------------------------------------------------------------------------------------------------------------------ minima
def minima_frames():
    rng = np.random.default_rng(77)
    return [(smooth_noise((96, 120), seed=60 + k, sigma=1.5) * F(rng.uniform(10, 900)) - F(rng.uniform(-50, 300))).astype(F) for k in range(7)]


@pytest.mark.parametrize("lanes", [1, 3])
def test_minmax_batch_gives_every_frames_own_extremes(siftlib, lanes):
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    frames = minima_frames()
    single = sp.SiftPlan(shape=frames[0].shape, dtype=F)
    per_frame = []
    for f in frames:
        single.keypoints(f)
        per_frame.append(single.minmax())
    assert len({mn for mn, _ in per_frame}) == 7                   # seven different minima: an index mix-up cannot hide
    bp = sp.BatchPlan(shape=frames[0].shape, dtype=F, lanes=lanes)
    with pytest.raises(RuntimeError):
        bp.minmax_batch()                                          # no batch has finished
    with pytest.raises(RuntimeError):
        bp.minmax()                                                # the single-frame query keeps raising
    for order, device in (((0, 1, 2, 3, 4, 5, 6), False), ((6, 2, 5, 0, 3), False), ((4, 6, 1, 0, 5, 3, 2), True)):
        batch = [frames[i] for i in order]
        if device:                                                 # always parked
            bp.keypoints_batch_device(batch)
        else:                                                      # one lane: delivered directly; three lanes: parked
            bp.keypoints_batch(batch)
        mins, maxs = bp.minmax_batch()
        assert mins.dtype == F and maxs.dtype == F and mins.shape == (len(order),) and maxs.shape == (len(order),)
        for k, i in enumerate(order):
            assert (mins[k], maxs[k]) == (frames[i].min(), frames[i].max()), (lanes, order, k)
            assert (float(mins[k]), float(maxs[k])) == per_frame[i], (lanes, order, k)
    # the size of the last batch is part of the question
    buf = np.full(8, -5, F)
    assert siftlib.siftmi_batch_minmax(bp._handle, buf.ctypes.data, buf.ctypes.data, 6) == _lib.EINVAL
    assert (buf == -5).all()
    assert siftlib.siftmi_batch_minmax(bp._handle, None, buf.ctypes.data, 7) == 0 and tuple(buf[:7]) == tuple(frames[i].max() for i in order)
    assert bp.keypoints_batch([]) == [] and bp.minmax_batch()[0].shape == (0,)


def test_minmax_batch_of_rgb_frames(siftlib):
    import sift_pyocl_amd as sp
    rng = np.random.default_rng(5)
    frames = [rng.integers(lo, hi, (72, 90, 3), dtype=np.uint8) for lo, hi in ((0, 256), (30, 200), (100, 101), (7, 250))]
    single = sp.SiftPlan(template=frames[0])
    want = []
    for f in frames:
        single.keypoints(f)
        want.append(single.minmax())
    bp = sp.BatchPlan(template=frames[0], lanes=2)
    bp.keypoints_batch(frames)
    mins, maxs = bp.minmax_batch()
    assert [(float(a), float(b)) for a, b in zip(mins, maxs)] == want and len(set(want)) == 4


# ------------------------------------------------------------------------------------------------------------- align_batch
MODES = [2, 2, 1, 0, 1, 0, 2]
WINDOWS = {2: (100, 90, 48, 48), 4: (60, 200, 20, 20), 5: (180, 180, 28, 28), 6: (96, 96, 64, 64)}


def stack():
    """(reference crop, the seven frames of the module docstring)"""
    if "stack" not in _cache:
        big = smooth_noise((330, 340), seed=12, sigma=2.0)
        ref = np.ascontiguousarray(big[20:276, 30:286])
        frames = [np.ascontiguousarray(big[27:283, 19:275]), np.ascontiguousarray(big[16:272, 35:291])]
        for s in range(2, 7):
            if s == 3:
                frames.append(np.zeros_like(ref))
                continue
            y0, x0, h, w = WINDOWS[s]
            f = np.full_like(ref, ref.mean())
            f[y0:y0 + h, x0:x0 + w] = ref[y0:y0 + h, x0:x0 + w]
            frames.append(f)
        _cache["stack"] = (ref, frames)
    return _cache["stack"]


def aligner():
    import sift_pyocl_amd as sp
    if "la" not in _cache:
        _cache["la"] = sp.LinearAlign(stack()[0])
    return _cache["la"]


def full_result():
    """align_batch(return_all=True) of the stack with the defaults, computed once"""
    if "full" not in _cache:
        _cache["full"] = aligner().align_batch(stack()[1], return_all=True)
    return _cache["full"]


def segments(res):
    """[(keypoints, pairs)] per frame from the flat tables of a return_all dict"""
    at = np.concatenate([[0], np.cumsum(res["pair_counts"])])
    return [(res["keypoint"][s], res["pairs"][at[s]:at[s + 1]]) for s in range(len(res["keypoint"]))]


def single_estimates(la, res, mask=None, shift_only=False):
    """fit() and shift() of every segment on the batch's own lists and pairs, put into the tables of align_batch_ref"""
    segs = segments(res)
    S = len(segs)
    models, n_fit, rms = np.full((S, 6), np.nan), np.zeros(S, np.int64), np.full(S, np.nan)
    shifts, n_shift = np.full((S, 2), np.nan, F), np.zeros(S, np.int64)
    at = 0
    for s, (kp, pairs) in enumerate(segs):
        m = None if mask is None else np.ascontiguousarray(mask[at:at + len(pairs)])
        at += len(pairs)
        if len(pairs) == 0:
            continue
        if not shift_only:
            model, r, n = la.match.fit(la.ref_kp, kp, pairs, mask=m)
            n_fit[s], rms[s] = n, r
            if model is not None:
                models[s] = model
        moved, n = la.match.shift(la.ref_kp, kp, pairs, mask=m)
        n_shift[s] = n
        if moved is not None:
            shifts[s] = moved
    return models, n_fit, rms, shifts, n_shift


def check_against_single_calls(la, res, frames, shift_only=False, mask=None, out_shape=None):
    """(c) and (d) of the module: the estimates through align_batch_ref, the planes through warp_ref"""
    models, n_fit, rms, shifts, n_shift = single_estimates(la, res, mask=mask, shift_only=shift_only)
    mode, matrix, offset = ab.align_batch_ref(res["pair_counts"], None if shift_only else models, n_fit, shifts, n_shift, shift_only=shift_only)
    assert res["mode"].dtype == np.int8 and res["mode"].tolist() == mode.tolist()
    assert same(res["matrix"], matrix) and same(res["offset"], offset)
    for s in range(len(frames)):
        if mode[s] == 2:
            assert res["rms"][s] == rms[s] and res["n"][s] == n_fit[s]
        else:
            assert np.isnan(res["rms"][s]) and res["n"][s] == (n_shift[s] if mode[s] == 1 else 0)
        assert res["fill"][s] == frames[s].min()
        want = warp_ref(frames[s], res["matrix"][s].reshape(4), res["offset"][s], out_shape or la.outshape, res["fill"][s], 1)[0]
        assert same(res["result"][s], want), "plane %d" % s
        if mode[s] == 0:
            assert same(res["result"][s], np.full(want.shape, res["fill"][s]).astype(want.dtype))


def test_align_batch_stages_equal_the_single_calls(siftlib):
    import sift_pyocl_amd as sp
    la, (ref, frames), res = aligner(), stack(), full_result()
    assert res["mode"].tolist() == MODES
    pc = res["pair_counts"]
    assert pc[0] >= 18 and pc[1] >= 18 and 1 <= pc[2] <= 17 and pc[3] == 0 and 1 <= pc[4] <= 2 and pc[5] == 0 and pc[6] >= 18
    assert res["counts"][3] == 0 and res["counts"][5] > 0
    assert res["result"].shape == (7, 256, 256) and res["result"].dtype == F and "inliers" not in res
    # (a) every list is the SiftPlan's, as a set
    single = sp.SiftPlan(template=ref)
    for s, f in enumerate(frames):
        assert_same_keypoints(res["keypoint"][s], single.keypoints(f), "frame %d" % s)
        assert res["counts"][s] == len(res["keypoint"][s])
    # (b) the pairs are match()'s of each segment on those records
    for s, (kp, pairs) in enumerate(segments(res)):
        if len(kp) == 0:
            assert len(pairs) == 0
            continue
        want = la.match.match(la.ref_kp, kp, raw_results=True)
        assert np.array_equal(sort_rows(pairs), sort_rows(np.asarray(want, np.int32).reshape(-1, 2))), "frame %d" % s
    # (c), (d)
    check_against_single_calls(la, res, frames)


def test_align_batch_against_the_loop_of_align(siftlib):
    la, (ref, frames) = aligner(), stack()
    before = la.align(frames[0], estimate="device", median="device")
    plain = la.align_batch(frames)
    after = la.align(frames[0], estimate="device", median="device")
    assert same(before, after)                                    # align() on the same aligner is not disturbed
    res = full_result()
    loop = [la.align(f, estimate="device", median="device", return_all=True) for f in frames]
    assert same(before, loop[0]["result"])
    for s, ((kp, pairs), one) in enumerate(zip(segments(res), loop)):
        if one is None:
            assert res["mode"][s] == 0, s
            continue
        assert res["mode"][s] in (1, 2)
        got = {(a.tobytes(), b.tobytes()) for a, b in zip(la.ref_kp[pairs[:, 0]], kp[pairs[:, 1]])}
        assert got == {(a.tobytes(), b.tobytes()) for a, b in zip(one["matching"][:, 0], one["matching"][:, 1])}, s
        if res["mode"][s] == 1:
            assert same(res["matrix"][s], one["matrix"]) and np.array_equal(res["offset"][s], one["offset"]), s
        else:
            assert np.allclose(res["matrix"][s], one["matrix"], rtol=0, atol=2e-6), s
            assert np.allclose(res["offset"][s], one["offset"], rtol=0, atol=2e-4), s
    assert [one is None for one in loop] == [m == 0 for m in MODES]
    # the plain return value, on the host and on the device, is the dict's stack
    assert isinstance(plain, np.ndarray) and same(plain, res["result"])
    dev = la.align_batch(frames, out="device")
    assert dev.is_cuda and same(dev.cpu().numpy(), plain)
    # device tensors in, a stack in
    import torch
    assert same(la.align_batch([torch.from_numpy(f).cuda() for f in frames]), plain)
    assert same(la.align_batch(np.stack(frames)), plain)


def test_align_batch_shift_only_and_another_stack_size(siftlib):
    la, (ref, frames) = aligner(), stack()
    res = la.align_batch(frames, shift_only=True, return_all=True)
    assert res["mode"].tolist() == [1 if m else 0 for m in MODES]
    check_against_single_calls(la, res, frames, shift_only=True)
    assert abs(res["offset"][0][0] + 7.0) < 0.05 and abs(res["offset"][0][1] - 11.0) < 0.05       # the crop of frame 0, (dy, dx)
    # a second call with another S: three frames in another order, then none
    sub = [frames[4], frames[1], frames[3]]
    res3 = la.align_batch(sub, return_all=True)
    assert res3["mode"].tolist() == [1, 2, 0]
    check_against_single_calls(la, res3, sub)
    full = full_result()
    assert same(res3["result"][1], full["result"][1]) and same(res3["result"][0], full["result"][4])
    empty = la.align_batch([])
    assert isinstance(empty, np.ndarray) and empty.shape == (0, 256, 256) and empty.dtype == F
    none = la.align_batch([], return_all=True, robust=True)
    assert none["result"].shape == (0, 256, 256) and none["mode"].shape == (0,) and none["keypoint"] == [] and none["pairs"].shape == (0, 2)


def test_align_batch_robust(siftlib, caplog):
    la, (ref, frames) = aligner(), stack()
    res = la.align_batch(frames, robust=True, robust_tol=2.0, robust_hyp=512, return_all=True)
    assert res["mode"].tolist()[:6] == MODES[:6] and res["mode"][6] in (1, 2)
    assert res["inliers"].dtype == np.bool_ and res["inliers"].shape == (len(res["pairs"]),)
    segs = segments(res)
    at = np.concatenate([[0], np.cumsum(res["pair_counts"])])
    want_mask = np.zeros(len(res["pairs"]), np.uint8)
    models = np.full((len(segs), 6), np.nan)
    for s, (kp, pairs) in enumerate(segs):
        if len(pairs) == 0:
            continue
        mask, model, votes = la.match.consensus(la.ref_kp, kp, pairs, n_hyp=512, tol=2.0, seed=0)
        want_mask[at[s]:at[s + 1]] = mask
        if model is not None:
            models[s] = model
        if s == 4:
            assert model is None and len(pairs) < 3               # fewer than three pairs: no winner, all of them are used
    want_mask = ab.used_mask(want_mask, models, res["pair_counts"])
    assert want_mask[at[4]:at[5]].all()
    assert np.array_equal(res["inliers"], want_mask.astype(bool))
    assert 18 <= res["inliers"][at[0]:at[1]].sum() <= res["pair_counts"][0]
    check_against_single_calls(la, res, frames, mask=want_mask)
    assert any("frame 4" in r.getMessage() and "consensus" in r.getMessage() for r in caplog.records)
    assert any("frame 3" in r.getMessage() for r in caplog.records) and any("frame 5" in r.getMessage() for r in caplog.records)


def test_align_batch_extra_margin(siftlib):
    import sift_pyocl_amd as sp
    ref, frames = stack()
    la = sp.LinearAlign(ref, extra=(4, 6))
    sub = [frames[1], frames[2], frames[3]]
    res = la.align_batch(sub, return_all=True, lanes=2)
    assert la.outshape == (264, 268) and res["result"].shape == (3, 264, 268) and res["mode"].tolist() == [2, 1, 0]
    assert la._batch.lanes == 2
    check_against_single_calls(la, res, sub)


def test_align_batch_rgb(siftlib):
    import sift_pyocl_amd as sp
    base = smooth_noise((200, 220), seed=16, sigma=1.5)
    base = (255 * (base - base.min()) / (base.max() - base.min()))
    big = np.stack([base, base[::-1, ::-1], base.T[:200, :200].repeat(2, axis=1)[:, :220]], axis=-1).astype(np.uint8)
    ref = np.ascontiguousarray(big[10:170, 12:172])
    frames = [np.ascontiguousarray(big[14:174, 9:169]), np.zeros_like(ref), np.ascontiguousarray(big[8:168, 15:175])]
    la = sp.LinearAlign(ref, extra=(1, 2))
    res = la.align_batch(frames, shift_only=True, return_all=True)
    assert res["result"].shape == (3, 162, 164, 3) and res["result"].dtype == np.uint8 and res["mode"].tolist() == [1, 0, 1]
    for s, f in enumerate(frames):
        one = la.align(f, shift_only=True, median="device", return_all=True)
        if one is None:
            assert s == 1 and same(res["result"][s], np.full((162, 164, 3), res["fill"][s]).astype(np.uint8))
            continue
        assert res["fill"][s] == F(la.sift.minmax()[0])
        assert same(res["offset"][s], one["offset"]) and same(res["result"][s], one["result"]), s
        want = warp_ref(f, res["matrix"][s].reshape(4), res["offset"][s], la.outshape, res["fill"][s], 1)[0]
        assert same(res["result"][s], want)
    assert abs(res["offset"][0][0] + 4.0) < 0.1 and abs(res["offset"][0][1] - 3.0) < 0.1
