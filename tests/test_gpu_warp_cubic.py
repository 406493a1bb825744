"""GPU tests of the cubic sampler's row: transform_cubic_kernel / transform_cubic_batch_kernel
(csrc/k_warp_cubic.hpp) and the cubic instances of the stack kernels (k_stack.hpp, k_stack_clip.hpp) through the four _ex entries
of include/siftmi.h, the `interp` keyword of BatchPlan and LinearAlign, and the refusals.

The expected bits come from the numpy restatement tests/warp_cubic_ref.py alone (checked on the CPU by
tests/test_warp_cubic_ref_host.py); the stack expectations are its samples fed into the existing stack_ref.reduce_samples and
stack_clip_ref.reduce_clip.  Every comparison is bit equality; where a case can create a NaN (the `special` image, frames with
NaN, inf or 3e38) a NaN of the restatement is matched by any NaN.
"""
import ctypes as C

import numpy as np
import pytest

import stack_cases as sc
import stack_clip_ref as cr
import stack_ref as sr
import warp_cases as wc
import warp_cubic_cases as cc
from warp_cubic_ref import samples_cubic, warp_cubic_ref
from warp_ref import same

pytestmark = pytest.mark.gpu
F = np.float32
GUARD = 256                                     # bytes either side of every device output
EMPTY = -12345.0
MODE, CUBIC = 0, 1                              # SIFTMI_INTERP_*
_cache = {}


# ---------------------------------------------------------------------------------------------------------------- helpers
def sift_plan(shape, rgb=False):
    import sift_pyocl_amd as sp
    key = ("plan", shape, rgb)
    if key not in _cache:
        _cache[key] = sp.SiftPlan(shape=shape + (3,), dtype=np.uint8) if rgb else sp.SiftPlan(shape=shape, dtype=F)
    return _cache[key]


def batch_plan(shape, rgb=False):
    import sift_pyocl_amd as sp
    key = ("batch", shape, rgb)
    if key not in _cache:
        _cache[key] = sp.BatchPlan(shape=shape + (3,), dtype=np.uint8, lanes=1) if rgb else sp.BatchPlan(shape=shape, dtype=F, lanes=1)
    return _cache[key]


def table(maps):
    if not len(maps):
        return np.zeros((0, 6), F)
    return np.ascontiguousarray(np.array([tuple(M) + tuple(off) for M, off in maps], F))


def pointers(addresses):
    return (C.c_void_p * max(1, len(addresses)))(*addresses)


def on_device(arrays):
    """(tensor kept alive by the caller, the device address of every array): the arrays back to back in one allocation"""
    import torch
    raw = np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1) for a in arrays])
    t = torch.from_numpy(raw).cuda()
    at, addrs = 0, []
    for a in arrays:
        addrs.append(t.data_ptr() + at)
        at += a.nbytes
    return t, addrs


class Guarded:
    """device outputs of the given byte sizes between guard bytes in one buffer of 0xa5"""

    def __init__(self, sizes):
        import torch
        self.sizes = list(sizes)
        self.at = []
        pos = GUARD
        for n in self.sizes:
            self.at.append(pos)
            pos += n + GUARD
        self.buf = torch.full((pos,), 0xa5, dtype=torch.uint8, device="cuda")
        assert self.buf.data_ptr() % 4 == 0
        torch.cuda.synchronize()

    def ptr(self, k):
        return self.buf.data_ptr() + self.at[k]

    def fetch(self, dtypes, shapes, written=None):
        """the outputs on the host, after checking that nothing outside the outputs that were asked for changed"""
        host = self.buf.cpu().numpy()
        keep = np.ones(host.shape, bool)
        res = []
        for k, (dtype, shape) in enumerate(zip(dtypes, shapes)):
            if written is None or written[k]:
                keep[self.at[k]:self.at[k] + self.sizes[k]] = False
                res.append(host[self.at[k]:self.at[k] + self.sizes[k]].view(dtype).reshape(shape).copy())
            else:
                res.append(None)
        assert (host[keep] == 0xa5).all(), "bytes outside the result were written"
        return res


def transform_ex(siftlib, plan, image_ptr, image_is_device, channels, out_ptr, out_is_device, out_shape, M, off, fill, mode, interp, want_rc=0):
    M = np.ascontiguousarray(M, F).reshape(4); off = np.ascontiguousarray(off, F).reshape(2)
    ms = C.c_double(-1.0)
    rc = siftlib.siftmi_plan_transform_ex(plan._handle, image_ptr, image_is_device, channels, out_ptr, out_is_device, out_shape[1], out_shape[0],
                                          M.ctypes.data, off.ctypes.data, C.c_float(fill), mode, interp, C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def batch_transform_ex(siftlib, plan, ptrs, n, is_dev, channels, out_ptr, out_is_dev, out_shape, maps, fills, mode, interp, want_rc=0):
    tab = table(maps); fills = np.ascontiguousarray(fills, F)
    ms = C.c_double(-1.0)
    rc = siftlib.siftmi_batch_transform_ex(plan._handle, ptrs, n, is_dev, channels, out_ptr, out_is_dev, out_shape[1], out_shape[0],
                                           tab.ctypes.data, fills.ctypes.data, mode, interp, C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def stack_ex(siftlib, plan, ptrs, n, is_dev, out_ptr, cov_ptr, out_is_dev, out_shape, maps, fills, mode, interp, reduce, empty=EMPTY, want_rc=0):
    tab = table(maps); fills = np.ascontiguousarray(fills, F)
    ms = C.c_double(-1.0)
    rc = siftlib.siftmi_batch_stack_ex(plan._handle, ptrs, n, is_dev, out_ptr, cov_ptr, out_is_dev, out_shape[1], out_shape[0], tab.ctypes.data,
                                       fills.ctypes.data, mode, interp, {"sum": 0, "mean": 1, "median": 2}[reduce], C.c_float(empty), C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def clip_ex(siftlib, plan, ptrs, n, is_dev, out_ptr, cov_ptr, kept_ptr, out_is_dev, out_shape, maps, fills, mode, interp, p, empty=EMPTY, want_rc=0):
    tab = table(maps); fills = np.ascontiguousarray(fills, F)
    w = None if p.get("weights") is None else np.ascontiguousarray(p["weights"], F)
    trim, kappa = p.get("trim", (0, 1)), p.get("kappa", (3.0, 3.0))
    ms = C.c_double(-1.0)
    rc = siftlib.siftmi_batch_stack_clip_ex(plan._handle, ptrs, n, is_dev, out_ptr, cov_ptr, kept_ptr, out_is_dev, out_shape[1], out_shape[0],
                                            tab.ctypes.data, fills.ctypes.data, None if w is None else w.ctypes.data, mode, interp,
                                            {"trim": 0, "sigma": 1}[p["reject"]], trim[0], trim[1], C.c_float(kappa[0]), C.c_float(kappa[1]),
                                            p.get("iters", 3), C.c_float(empty), C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def expected(case):
    img = wc.image(case.image)
    want, counts = warp_cubic_ref(img, case.M, case.off, case.out_shape, case.fill)
    cc.check_expect(case, counts)
    return img, want


#: the second frame of every two-frame batch: another map and another fill on the same image
OTHER = ((1.0, 0.03, -0.02, 1.0), (0.5, -1.25))
OTHER_FILL = -3.5


# ------------------------------------------------------------------------------------------------------------------ paths
@pytest.mark.parametrize("case", cc.cases(), ids=lambda c: c.name)
def test_every_case_through_the_single_and_the_batch_entry(siftlib, case):
    """host image to host output through siftmi_plan_transform_ex; then the case and a second map as a batch of two through
    siftmi_batch_transform_ex, device frames to a device output between guards: frame 0 is the case, frame 1 the single call"""
    img, want = expected(case)
    shape = case.image[1]
    loose = case.family == 8
    got = np.full(want.shape, -77.0, F)
    ms = transform_ex(siftlib, sift_plan(shape), img.ctypes.data, 0, 1, got.ctypes.data, 0, case.out_shape, case.M, case.off, case.fill, 1, CUBIC)
    assert same(got, want, nan_any_payload=loose), (case.name, "single", int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert np.isfinite(ms) and ms > 0.0
    single = np.full(want.shape, -77.0, F)
    transform_ex(siftlib, sift_plan(shape), img.ctypes.data, 0, 1, single.ctypes.data, 0, case.out_shape, OTHER[0], OTHER[1], OTHER_FILL, 1, CUBIC)
    assert same(single, warp_cubic_ref(img, OTHER[0], OTHER[1], case.out_shape, OTHER_FILL)[0], nan_any_payload=loose), (case.name, "second map")
    keep, addrs = on_device([img, img])
    g = Guarded([2 * want.nbytes])
    batch_transform_ex(siftlib, batch_plan(shape), pointers(addrs), 2, 1, 1, g.ptr(0), 1, case.out_shape, [(case.M, case.off), OTHER],
                       [case.fill, OTHER_FILL], 1, CUBIC)
    both, = g.fetch([F], [(2,) + want.shape])
    del keep
    assert same(both[0], got), (case.name, "batch frame 0 is not the single call")
    assert same(both[1], single), (case.name, "batch frame 1 is not the single call")


POINTER = [cc.by_name(n) for n in cc.POINTER_CASES]


@pytest.mark.parametrize("case", POINTER, ids=lambda c: c.name)
def test_the_other_pointer_paths(siftlib, case):
    img, want = expected(case)
    shape = case.image[1]
    args = (case.out_shape, case.M, case.off, case.fill, 1, CUBIC)
    keep, (iptr,) = on_device([img])
    got = np.full(want.shape, -77.0, F)
    transform_ex(siftlib, sift_plan(shape), iptr, 1, 1, got.ctypes.data, 0, *args)                      # device image, host output
    assert same(got, want), (case.name, "device to host")
    for image_ptr, image_dev in ((img.ctypes.data, 0), (iptr, 1)):                                     # device output between guards
        g = Guarded([want.nbytes])
        transform_ex(siftlib, sift_plan(shape), image_ptr, image_dev, 1, g.ptr(0), 1, *args)
        assert same(g.fetch([F], [want.shape])[0], want), (case.name, image_dev, "to device")
    del keep
    # the batch entry: host frames (one stack, and separate arrays) to a host output, host frames to a device output
    maps, fills = [(case.M, case.off), OTHER, (case.M, case.off)], [case.fill, OTHER_FILL, 1e6]
    wants = [warp_cubic_ref(img, M, off, case.out_shape, f)[0] for (M, off), f in zip(maps, fills)]
    stack, apart = np.stack([img] * 3), img.copy()
    for ptrs in (pointers([stack[s].ctypes.data for s in range(3)]), pointers([img.ctypes.data, apart.ctypes.data, img.ctypes.data])):
        out = np.full((3,) + want.shape, -77.0, F)
        batch_transform_ex(siftlib, batch_plan(shape), ptrs, 3, 0, 1, out.ctypes.data, 0, case.out_shape, maps, fills, 1, CUBIC)
        assert all(same(out[s], wants[s]) for s in range(3)), (case.name, "batch host to host")
    g = Guarded([3 * want.nbytes])
    batch_transform_ex(siftlib, batch_plan(shape), pointers([stack[s].ctypes.data for s in range(3)]), 3, 0, 1, g.ptr(0), 1, case.out_shape, maps, fills, 1, CUBIC)
    out, = g.fetch([F], [(3,) + want.shape])
    assert all(same(out[s], wants[s]) for s in range(3)), (case.name, "batch host to device")


def test_empty_outputs_and_batches_launch_nothing(siftlib):
    img = wc.image(("gray", wc.SMALL))
    for out_shape in ((0, 7), (5, 0)):
        host = np.full(64, 0x5a, np.uint8)
        assert transform_ex(siftlib, sift_plan(wc.SMALL), img.ctypes.data, 0, 1, host.ctypes.data, 0, out_shape, [1, 0, 0, 1], [0, 0], 13.0, 1, CUBIC) == 0.0
        assert batch_transform_ex(siftlib, batch_plan(wc.SMALL), pointers([img.ctypes.data]), 1, 0, 1, host.ctypes.data, 0, out_shape,
                                  [((1, 0, 0, 1), (0, 0))], [13.0], 1, CUBIC) == 0.0
        assert (host == 0x5a).all()
    host = np.full(64, 0x5a, np.uint8)
    assert batch_transform_ex(siftlib, batch_plan(wc.SMALL), pointers([]), 0, 0, 1, host.ctypes.data, 0, (3, 3), [], [], 1, CUBIC) == 0.0
    assert (host == 0x5a).all()


# ---------------------------------------------------------------------------------------------------------- stack kernels
def sampled(case):
    key = ("samples", case.name)
    if key not in _cache:
        _cache[key] = samples_cubic(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape)
    return _cache[key]


def loose(case):
    return case.kind in cc.NAN_KINDS


@pytest.mark.parametrize("case", cc.stack_cases(), ids=lambda c: c.name)
def test_every_stack_and_reducer_is_the_restatement(siftlib, case):
    """host frames to a host plane and coverage; device frames to a device plane and coverage between guards"""
    vals, live = sampled(case)
    S = len(case.frames)
    plan = batch_plan(sc.SHAPE)
    hptrs = pointers([f.ctypes.data for f in case.frames])
    keep, addrs = on_device(case.frames)
    nbytes = case.out_shape[0] * case.out_shape[1] * 4
    for reduce in cc.reducers_of(case):
        want, want_c = sr.reduce_samples(vals, live, reduce, EMPTY)
        out = np.full(case.out_shape, -77.0, F); cov = np.full(case.out_shape, -5, np.int32)
        ms = stack_ex(siftlib, plan, hptrs, S, 0, out.ctypes.data, cov.ctypes.data, 0, case.out_shape, case.maps, case.fills, 1, CUBIC, reduce)
        assert ms > 0.0
        assert same(out, want, nan_any_payload=loose(case)), (case.name, reduce, "host", int((out.view(np.uint32) != want.view(np.uint32)).sum()))
        assert np.array_equal(cov, want_c), (case.name, reduce, "host coverage")
        with_cov = reduce != "sum"
        g = Guarded([nbytes, nbytes])
        stack_ex(siftlib, plan, pointers(addrs), S, 1, g.ptr(0), g.ptr(1) if with_cov else None, 1, case.out_shape, case.maps, case.fills, 1, CUBIC, reduce)
        got, got_c = g.fetch([F, np.int32], [case.out_shape] * 2, written=[True, with_cov])
        assert same(got, out), (case.name, reduce, "device result is not the host result")
        assert got_c is None or np.array_equal(got_c, want_c), (case.name, reduce, "device coverage")
    del keep


@pytest.mark.parametrize("case", cc.clip_stacks(), ids=lambda c: c.name)
def test_every_clip_is_the_restatement_and_nothing_rejected_is_the_cubic_mean(siftlib, case):
    vals, live = sampled(case)
    S = len(case.frames)
    plan = batch_plan(sc.SHAPE)
    hptrs = pointers([f.ctypes.data for f in case.frames])
    keep, addrs = on_device(case.frames)
    nbytes = case.out_shape[0] * case.out_shape[1] * 4
    mean = np.full(case.out_shape, -77.0, F)
    stack_ex(siftlib, plan, hptrs, S, 0, mean.ctypes.data, None, 0, case.out_shape, case.maps, case.fills, 1, CUBIC, "mean")
    for k, (label, p) in enumerate(cc.CLIPS):
        p = dict(p, weights=None if label == "trim0_0" else cc.clip_weights(case, label))
        want, want_c, want_k = cr.reduce_clip(vals, live, empty=EMPTY, **p)
        out = np.full(case.out_shape, -77.0, F); cov = np.full(case.out_shape, -5, np.int32); kept = np.full(case.out_shape, -6, np.int32)
        clip_ex(siftlib, plan, hptrs, S, 0, out.ctypes.data, cov.ctypes.data, kept.ctypes.data, 0, case.out_shape, case.maps, case.fills, 1, CUBIC, p)
        assert same(out, want, nan_any_payload=loose(case)), (case.name, label, "plane", int((out.view(np.uint32) != want.view(np.uint32)).sum()))
        assert np.array_equal(cov, want_c) and np.array_equal(kept, want_k), (case.name, label, "counts")
        if label == "trim0_0":
            assert same(out, mean), (case.name, "with nothing rejected the clip plane is not the cubic mean")
        if k == len(case.name) % len(cc.CLIPS):                    # one rejection per stack again on the device, with one of the counts
            which = (k % 2 == 0, k % 2 == 1)
            g = Guarded([nbytes] * 3)
            clip_ex(siftlib, plan, pointers(addrs), S, 1, g.ptr(0), g.ptr(1) if which[0] else None, g.ptr(2) if which[1] else None, 1,
                    case.out_shape, case.maps, case.fills, 1, CUBIC, p)
            got, got_c, got_k = g.fetch([F, np.int32, np.int32], [case.out_shape] * 3, written=[True, which[0], which[1]])
            assert same(got, out), (case.name, label, "device result is not the host result")
            assert (got_c is None or np.array_equal(got_c, want_c)) and (got_k is None or np.array_equal(got_k, want_k)), (case.name, label)
    del keep


def test_no_frame_fills_the_plane(siftlib):
    plan = batch_plan(sc.SHAPE)
    out = np.full((5, 7), -77.0, F); cov = np.full((5, 7), -5, np.int32); kept = np.full((5, 7), -6, np.int32)
    stack_ex(siftlib, plan, pointers([]), 0, 0, out.ctypes.data, cov.ctypes.data, 0, (5, 7), [], [], 1, CUBIC, "median", empty=4.0)
    assert (out == 4.0).all() and (cov == 0).all()
    out[:] = -77.0
    clip_ex(siftlib, plan, pointers([]), 0, 0, out.ctypes.data, cov.ctypes.data, kept.ctypes.data, 0, (5, 7), [], [], 1, CUBIC, dict(reject="sigma"), empty=4.0)
    assert (out == 4.0).all() and (cov == 0).all() and (kept == 0).all()


# ----------------------------------------------------------------------------------------------------------------- legacy
LEGACY_WARP = ["f1-rot30-gray-m1", "f1-rot30-gray-m0", "f1-rot30-rgb-m1", "f1-zoom_corner-rgb-m1", "f2-hi_hi-gray-m1", "f2-half_below-gray-m1",
               "f3-mode-gray-m2", "f3-mode-rgb-m-1", "f3-mode-gray-m257", "f4-nan_coeff-gray-m1", "f6-quarter_2x2-gray-m1", "f8-special_0.5_0.5-special-m1"]
LEGACY_STACK = ["noise-leaving-S5-41x70-m1", "ties-shift-S2-37x53-m1", "noise-half-S5-41x70-m0", "ties-rot-S8-37x53-m3", "noise-nan_some-S4-41x70-m1",
                "zinger-shift-S64-41x70-m1"]


@pytest.mark.parametrize("name", LEGACY_WARP)
def test_interp_mode_is_the_old_warp_bit_for_bit(siftlib, name):
    case = wc.by_name(name)
    img = wc.image(case.image)
    rgb = wc.is_rgb(case)
    shape, ch = case.image[1], 3 if rgb else 1
    oshape = case.out_shape + ((3,) if rgb else ())
    old = np.full(oshape, 0x5a, np.uint8) if rgb else np.full(oshape, -77.0, F)
    new = old.copy()
    M = np.ascontiguousarray(case.M, F); off = np.ascontiguousarray(case.off, F)
    ms = C.c_double(-1)
    assert siftlib.siftmi_plan_transform(sift_plan(shape, rgb)._handle, img.ctypes.data, 0, ch, old.ctypes.data, 0, case.out_shape[1], case.out_shape[0],
                                         M.ctypes.data, off.ctypes.data, C.c_float(case.fill), case.mode, C.byref(ms)) == 0
    transform_ex(siftlib, sift_plan(shape, rgb), img.ctypes.data, 0, ch, new.ctypes.data, 0, case.out_shape, case.M, case.off, case.fill, case.mode, MODE)
    assert same(new, old), name
    # the batch entries, two frames
    maps, fills = [(case.M, case.off), (case.M, case.off)], [case.fill, 200.0]
    tab, f = table(maps), np.ascontiguousarray(fills, F)
    ptrs = pointers([img.ctypes.data, img.ctypes.data])
    old2 = np.concatenate([old[None], old[None]]); old2[:] = 0x5a if rgb else -77.0
    new2 = old2.copy()
    assert siftlib.siftmi_batch_transform(batch_plan(shape, rgb)._handle, ptrs, 2, 0, ch, old2.ctypes.data, 0, case.out_shape[1], case.out_shape[0],
                                          tab.ctypes.data, f.ctypes.data, case.mode, C.byref(ms)) == 0
    batch_transform_ex(siftlib, batch_plan(shape, rgb), ptrs, 2, 0, ch, new2.ctypes.data, 0, case.out_shape, maps, fills, case.mode, MODE)
    assert same(new2, old2) and same(new2[0], old), name


@pytest.mark.parametrize("name", LEGACY_STACK)
def test_interp_mode_is_the_old_stack_and_clip_bit_for_bit(siftlib, name):
    case = {c.name: c for c in sc.cases()}[name]
    S = len(case.frames)
    plan = batch_plan(sc.SHAPE)
    ptrs = pointers([f.ctypes.data for f in case.frames])
    tab, f = table(case.maps), np.ascontiguousarray(case.fills, F)
    ow, oh = case.out_shape[1], case.out_shape[0]
    ms = C.c_double(-1)
    for reduce, code in (("sum", 0), ("mean", 1), ("median", 2)):
        old = np.full(case.out_shape, -77.0, F); old_c = np.full(case.out_shape, -5, np.int32)
        new, new_c = old.copy(), old_c.copy()
        assert siftlib.siftmi_batch_stack(plan._handle, ptrs, S, 0, old.ctypes.data, old_c.ctypes.data, 0, ow, oh, tab.ctypes.data, f.ctypes.data,
                                          case.mode, code, C.c_float(EMPTY), C.byref(ms)) == 0
        stack_ex(siftlib, plan, ptrs, S, 0, new.ctypes.data, new_c.ctypes.data, 0, case.out_shape, case.maps, case.fills, case.mode, MODE, reduce)
        assert same(new, old) and np.array_equal(new_c, old_c), (name, reduce)
    w = np.linspace(0.5, 2.0, S).astype(F)
    for p, code in ((dict(reject="trim", trim=(1, 2), weights=w), 0), (dict(reject="sigma", kappa=(1.5, 2.0), iters=2, weights=None), 1)):
        outs = [[np.full(case.out_shape, -77.0, F), np.full(case.out_shape, -5, np.int32), np.full(case.out_shape, -6, np.int32)] for _ in range(2)]
        trim, kappa = p.get("trim", (0, 1)), p.get("kappa", (3.0, 3.0))
        assert siftlib.siftmi_batch_stack_clip(plan._handle, ptrs, S, 0, outs[0][0].ctypes.data, outs[0][1].ctypes.data, outs[0][2].ctypes.data, 0, ow, oh,
                                               tab.ctypes.data, f.ctypes.data, None if p["weights"] is None else w.ctypes.data, case.mode, code,
                                               trim[0], trim[1], C.c_float(kappa[0]), C.c_float(kappa[1]), p.get("iters", 3), C.c_float(EMPTY),
                                               C.byref(ms)) == 0
        clip_ex(siftlib, plan, ptrs, S, 0, outs[1][0].ctypes.data, outs[1][1].ctypes.data, outs[1][2].ctypes.data, 0, case.out_shape, case.maps,
                case.fills, case.mode, MODE, p)
        assert same(outs[1][0], outs[0][0]) and np.array_equal(outs[1][1], outs[0][1]) and np.array_equal(outs[1][2], outs[0][2]), (name, p["reject"])


# -------------------------------------------------------------------------------------------------------------- refusals
#: (interp, mode, channels): an unknown sampler; the cubic one with a reserved mode; the cubic one on RGB8
REFUSED = [(2, 1, 1), (-1, 1, 1), (257, 1, 1), (CUBIC, 0, 1), (CUBIC, 2, 1), (CUBIC, -1, 1), (CUBIC, 1, 3)]


@pytest.mark.parametrize("interp,mode,channels", REFUSED)
def test_refused_combinations_return_einval_and_write_nothing(siftlib, interp, mode, channels):
    from sift_pyocl_amd import _lib
    rgb = channels == 3
    img = wc.image(("rgb" if rgb else "gray", wc.SMALL))
    oshape = (9, 11)
    nbytes = 9 * 11 * (3 if rgb else 4)
    host = np.full(nbytes, 0x5a, np.uint8)
    ident = ((1, 0, 0, 1), (0.5, 0.5))
    transform_ex(siftlib, sift_plan(wc.SMALL, rgb), img.ctypes.data, 0, channels, host.ctypes.data, 0, oshape, ident[0], ident[1], 13.0, mode, interp,
                 want_rc=_lib.EINVAL)
    g = Guarded([2 * nbytes])
    transform_ex(siftlib, sift_plan(wc.SMALL, rgb), img.ctypes.data, 0, channels, g.ptr(0), 1, oshape, ident[0], ident[1], 13.0, mode, interp,
                 want_rc=_lib.EINVAL)
    ptrs = pointers([img.ctypes.data, img.ctypes.data])
    batch_transform_ex(siftlib, batch_plan(wc.SMALL, rgb), ptrs, 2, 0, channels, g.ptr(0), 1, oshape, [ident, ident], [13.0, 13.0], mode, interp,
                       want_rc=_lib.EINVAL)
    host2 = np.full(2 * nbytes, 0x5a, np.uint8)
    batch_transform_ex(siftlib, batch_plan(wc.SMALL, rgb), ptrs, 2, 0, channels, host2.ctypes.data, 0, oshape, [ident, ident], [13.0, 13.0], mode, interp,
                       want_rc=_lib.EINVAL)
    assert (host == 0x5a).all() and (host2 == 0x5a).all()
    g.fetch([], [])                                                     # every byte still 0xa5
    # the stack entries: float32 frames on a float32 batch for the first six, an RGB8 batch for the last
    frames = [np.zeros(wc.SMALL + ((3,) if rgb else ()), np.uint8 if rgb else F)] * 2
    ptrs = pointers([fr.ctypes.data for fr in frames])
    out = np.full(oshape, -77.0, F); cov = np.full(oshape, -5, np.int32); kept = np.full(oshape, -6, np.int32)
    plan = batch_plan(wc.SMALL, rgb)
    for reduce in ("sum", "median"):
        stack_ex(siftlib, plan, ptrs, 2, 0, out.ctypes.data, cov.ctypes.data, 0, oshape, [ident, ident], [0.0, 0.0], mode, interp, reduce, want_rc=_lib.EINVAL)
    for p in (dict(reject="trim", trim=(0, 1)), dict(reject="sigma")):
        clip_ex(siftlib, plan, ptrs, 2, 0, out.ctypes.data, cov.ctypes.data, kept.ctypes.data, 0, oshape, [ident, ident], [0.0, 0.0], mode, interp, p,
                want_rc=_lib.EINVAL)
    assert (out == -77.0).all() and (cov == -5).all() and (kept == -6).all()


def test_the_python_keyword_refuses_before_any_launch(siftlib):
    import sift_pyocl_amd as sp
    plan = batch_plan(sc.SHAPE)
    frames = sc.frames_of("noise", 3)
    M = np.tile(np.eye(2, dtype=F), (3, 1, 1)); off = np.full((3, 2), 0.5, F)
    before = (plan.last_transform_ms, plan.last_stack_ms)
    for call in (plan.transform_batch, plan.stack_batch, plan.stack_clip_batch):
        for kw in (dict(interp="lanczos"), dict(interp="Cubic"), dict(interp=1), dict(interp="cubic", mode=0), dict(interp="cubic", mode=2)):
            with pytest.raises(ValueError):
                call(frames, M, off, **kw)
    assert (plan.last_transform_ms, plan.last_stack_ms) == before
    rgb = batch_plan(sc.SHAPE, rgb=True)
    rgb_frames = [np.zeros(sc.SHAPE + (3,), np.uint8)] * 3
    for call in (rgb.transform_batch, rgb.stack_batch, rgb.stack_clip_batch):
        with pytest.raises(ValueError):
            call(rgb_frames, M, off, interp="cubic")
    assert rgb.transform_batch(rgb_frames, M, off, interp="linear").shape == (3,) + sc.SHAPE + (3,)
    # None and "linear" are today's calls
    base = plan.transform_batch(frames, M, off, 7.0)
    for interp in (None, "linear"):
        assert same(plan.transform_batch(frames, M, off, 7.0, interp=interp), base)
        assert same(plan.stack_batch(frames, M, off, 7.0, interp=interp), plan.stack_batch(frames, M, off, 7.0))
        assert same(plan.stack_clip_batch(frames, M, off, 7.0, reject="trim", interp=interp), plan.stack_clip_batch(frames, M, off, 7.0, reject="trim"))
    # and "cubic" is the restatement, through the methods: host and device
    import torch
    maps = [(M[s].reshape(4), off[s]) for s in range(3)]
    vals, live = samples_cubic(frames, maps, [7.0] * 3, sc.SHAPE, sc.SHAPE)
    got = plan.transform_batch(frames, M, off, 7.0, interp="cubic")
    assert same(got, vals) and plan.last_transform_ms > 0.0
    dev = plan.transform_batch([torch.from_numpy(f).cuda() for f in frames], M, off, 7.0, out="device", interp="cubic")
    assert dev.is_cuda and same(dev.cpu().numpy(), vals)
    plane, cov = plan.stack_batch(np.stack(frames), M, off, 7.0, reduce="median", coverage=True, empty=EMPTY, interp="cubic")
    want, want_c = sr.reduce_samples(vals, live, "median", EMPTY)
    assert same(plane, want) and np.array_equal(cov, want_c)
    plane, cov, kept = plan.stack_clip_batch(frames, M, off, 7.0, reject="trim", trim=(1, 1), counts=True, empty=EMPTY, interp="cubic")
    want, want_c, want_k = cr.reduce_clip(vals, live, reject="trim", trim=(1, 1), empty=EMPTY)
    assert same(plane, want) and np.array_equal(cov, want_c) and np.array_equal(kept, want_k)


# ------------------------------------------------------------------------------------------------------------ LinearAlign
def test_linear_align_with_the_cubic_sampler(siftlib):
    from test_gpu_stack import OFFSETS, aligner, zinger_stack
    la = aligner()
    ref, clean, dirty = zinger_stack()
    shape = ref.shape
    # align: the warp of the matrix it returns
    res = la.align(clean[1], return_all=True, interp="cubic")
    lin = la.align(clean[1], return_all=True)
    assert same(np.asarray(res["matrix"], F), np.asarray(lin["matrix"], F)) and same(np.asarray(res["offset"], F), np.asarray(lin["offset"], F))
    fill = float(clean[1].min())
    want = np.full(la.outshape, -77.0, F)
    transform_ex(siftlib, sift_plan(shape), clean[1].ctypes.data, 0, 1, want.ctypes.data, 0, la.outshape, np.asarray(res["matrix"], F).reshape(4),
                 res["offset"], fill, 1, CUBIC)
    assert same(res["result"], want) and not same(res["result"], lin["result"])
    assert same(want, warp_cubic_ref(clean[1], np.asarray(res["matrix"], F).reshape(4), res["offset"], la.outshape, fill)[0])
    assert same(la.transform(res["matrix"], res["offset"], image=clean[1], fill=fill, interp="cubic"), want)
    assert same(la.transform(res["matrix"], res["offset"], image=clean[1], fill=fill, interp="linear"), lin["result"])
    for kw in (dict(interp="cubic", mode=0), dict(interp="bicubic")):
        with pytest.raises(ValueError):
            la.transform(res["matrix"], res["offset"], image=clean[1], **kw)
    with pytest.raises(ValueError):
        la.align(clean[1], interp="nearest")
    # align_batch / align_batch_window: frame s is the restatement under the map it returns
    for got in (la.align_batch(dirty, return_all=True, interp="cubic"), la.align_batch_window(dirty, 12, return_all=True, interp="cubic")):
        maps = [(got["matrix"][s].reshape(4), got["offset"][s]) for s in range(7)]
        for s, (dy, dx) in enumerate(OFFSETS):
            assert abs(got["offset"][s][0] + dy) < 1.0 and abs(got["offset"][s][1] + dx) < 1.0, s
        vals, live = samples_cubic(dirty, maps, got["fill"], shape, la.outshape)
        assert same(got["result"], vals)
    # stack and stack_clip: the restatement fed with the maps they return
    res = la.stack(dirty, reduce="median", return_all=True, interp="cubic")
    maps = [(res["matrix"][s].reshape(4), res["offset"][s]) for s in range(7)]
    vals, live = samples_cubic(dirty, maps, res["fill"], shape, la.outshape)
    want, want_c = sr.reduce_samples(vals, live, "median", np.nan)
    assert same(res["stack"], want, nan_any_payload=True) and np.array_equal(res["coverage"], want_c) and la.last_stack_ms > 0.0
    lin_stack = la.stack(dirty, reduce="median")
    assert not same(lin_stack, res["stack"], nan_any_payload=True)
    assert same(la.stack(dirty, reduce="median", interp="linear"), lin_stack, nan_any_payload=True)
    dev = la.stack(dirty, reduce="median", out="device", interp="cubic")
    assert dev.is_cuda and same(dev.cpu().numpy(), want, nan_any_payload=True)
    res = la.stack_clip(dirty, reject="trim", trim=(1, 1), max_shift=12, return_all=True, interp="cubic")
    maps = [(res["matrix"][s].reshape(4), res["offset"][s]) for s in range(7)]
    vals, live = samples_cubic(dirty, maps, res["fill"], shape, la.outshape)
    want, want_c, want_k = cr.reduce_clip(vals, live, reject="trim", trim=(1, 1), empty=np.nan)
    assert same(res["stack"], want, nan_any_payload=True) and np.array_equal(res["coverage"], want_c) and np.array_equal(res["kept"], want_k)
    for call in (la.stack, la.stack_clip, la.align_batch):
        with pytest.raises(ValueError):
            call(dirty, interp="cubic ")
