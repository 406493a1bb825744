"""Every pyramid plane a plan leaves behind, and its candidate counts, against the oracle -- bit for bit, no tolerance.

The plan runs exactly as for a user (no stage hook, no extra launch); SiftPlan.planes() / SiftPlan.last_counts() read back what
the finished call left in memory.  This reaches what the record comparisons cannot: the planes of octaves without a candidate
(most octaves of octave_tail_kernel, k_tail.hpp, which restates the blur instead of sharing k_pyramid.hpp's kernels), samples
nearer to the edge than the detection border, the protocol between the tail's workgroups, its dynamic-LDS grant.

Frames (tests/pyramid_cases.py; tests/test_pyramid_cases_host.py checks on the CPU that each reaches what it is listed for):
  (128, 128)                tail octaves 64^2, 32^2, 16^2 (64 000 bytes of LDS: no grant needed)
  (112, 112)                56^2, 28^2, 14^2: reflect_index on a side of 14 under 27 taps
  (111, 111)                the last octave is 13^2: the tail must refuse, tail_first == n_oct
  (64, 256), (256, 64)      first tail octaves 128 x 32 / 32 x 128: more than 64 KiB of LDS, the W = 128 / H = 128 limits
  (58, 280)                 octave 1 is 140 x 29 = 4060 samples but W > 128: the tail starts at octave 2, 70 x 14
  (56, 300), (300, 56)      octave 1 has 4200 samples: a single tail octave, 75 x 14 / 14 x 75
  (130, 250), (114, 118), (118, 114)   tail widths 62, 31 / 59, 29 / 57, 28: padded pitches, odd last columns, odd heights
  (512, 512)                six octaves, forked chains, tail_first = 3
  (1400, 1400) f32 and u8   the marching blur, the fused convert and the tile kernels at plan level; the only slow cases
"""
import ctypes as C

import numpy as np
import pytest

import pyramid_cases as pc
from util import assert_same_keypoints

pytestmark = pytest.mark.gpu

_RECORDS = {}


def _records(oracle, frame):
    if frame.name not in _RECORDS:
        _RECORDS[frame.name] = oracle.keypoints(np.ascontiguousarray(pc.image(frame), np.float32))
    return _RECORDS[frame.name]


def _plan(frame, opts=None):
    import sift_pyocl_amd as sp
    plan = sp.SiftPlan(shape=frame.shape, dtype=np.dtype(frame.dtype))
    for name, value in (opts or {}).items():
        plan.set_option(name, value)
    return plan


def check_call(plan, oracle, frame, opts=None, what="", tail_first=None, records=True):
    """One keypoints() call on `plan` and everything it left behind against the oracle's expectations of `frame`."""
    opts = opts or {}
    what = "%s %s %r" % (frame.name, what, opts)
    exp = pc.expectations(oracle, frame)
    got = plan.keypoints(pc.image(frame))
    if tail_first is None:
        tail_first = pc.tail_first(exp.sizes, tail=opts.get("tail", 1), tail_pixels=opts.get("tail_pixels", pc.TAIL_PIXELS))
    # (the comparisons live in pyramid_cases.check_left_behind, shared with tests/test_gpu_tail_flush.py)
    pc.check_left_behind(plan, exp, what, tail_first, opts.get("fused_refine", 1))
    if records:
        assert_same_keypoints(got, _records(oracle, frame), what)
    return got


# ---- LDS grant order: these two run first in this module, in this order (the grant is per process and device, and only grows)
def test_lds_grant_small_frame_then_large(siftlib, oracle):
    """A (128, 128) plan (64 000 bytes: inside the default limit) runs before this module's first (64, 256) plan, whose 128 x 32
    octave needs 66 560 bytes through hipFuncSetAttribute."""
    check_call(_plan(pc.BY_NAME["smooth128"]), oracle, pc.BY_NAME["smooth128"], what="before a large grant")
    check_call(_plan(pc.BY_NAME["smooth64x256"]), oracle, pc.BY_NAME["smooth64x256"], what="first large grant")


def test_lds_grant_large_frame_then_small(siftlib, oracle):
    """A (256, 64) plan (68 864 bytes: the grant grows again) is built and run, a (128, 128) plan after it must not lower it:
    both plans run once more afterwards."""
    big, small = _plan(pc.BY_NAME["multi256x64"]), _plan(pc.BY_NAME["smooth128"])
    check_call(big, oracle, pc.BY_NAME["multi256x64"], what="largest grant")
    check_call(small, oracle, pc.BY_NAME["smooth128"], what="after the largest grant")
    check_call(big, oracle, pc.BY_NAME["multi256x64"], what="again after a small plan")


@pytest.mark.parametrize("frame", pc.FRAMES, ids=lambda f: f.name)
def test_default_plan_leaves_the_oracles_pyramid(siftlib, oracle, frame):
    plan = _plan(frame)
    check_call(plan, oracle, frame, what="default plan")
    sizes = pc.octave_sizes(*frame.shape)
    assert [sizes[o] for o in range(plan.last_counts()["tail_first"], len(sizes))] == pc.TAIL_OCTAVES[frame.name]
    if frame.name == "smooth111":
        assert plan.last_counts()["tail_first"] == len(sizes) == 4


FORM_FRAMES = ("smooth128", "smooth64x256", "multi130x250", "smooth512")
FORMS = [dict(tail=0), dict(tail_pixels=1024), dict(tail=1, overlap=0), dict(fused_shrink=0), dict(fork=0, early_chain=0),
         dict(split=1, fork=0), dict(ext_rows=8),
         dict(fused_refine=0)]        # (beyond the issue's list: the two-launch detection, whose candidate list every octave then has)


@pytest.mark.parametrize("opts", FORMS, ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("name", FORM_FRAMES)
def test_forms_leave_the_same_pyramid(siftlib, oracle, name, opts):
    frame = pc.BY_NAME[name]
    plan = _plan(frame, opts)
    check_call(plan, oracle, frame, opts, what="form")
    if "tail_pixels" in opts:          # the option really moved the tail's first octave down
        moved = {"smooth128": 2, "smooth64x256": 2, "multi130x250": 3, "smooth512": 4}[name]
        assert plan.last_counts()["tail_first"] == moved == pc.tail_first(pc.octave_sizes(*frame.shape)) + 1


@pytest.mark.parametrize("name", FORM_FRAMES)
def test_tail_timeout_rerun_leaves_the_same_pyramid(siftlib, oracle, name):
    """option "tail_fault" = 1: the first call is treated as timed out and runs again octave by octave inside the same call --
    planes and counts are those of the re-run, which had no tail launch"""
    frame = pc.BY_NAME[name]
    plan = _plan(frame, dict(tail_fault=1))
    n_oct = len(pc.octave_sizes(*frame.shape))
    check_call(plan, oracle, frame, what="tail_fault=1", tail_first=n_oct)
    assert plan.tail_timeouts() == (1, False)
    check_call(plan, oracle, frame, what="after the time-out", tail_first=n_oct)
    assert plan.tail_timeouts() == (1, False)


@pytest.mark.parametrize("a, b", [("smooth128", "white128"), ("smooth64x256", "white64x256")])
def test_alternating_images_leave_their_own_pyramids(siftlib, oracle, a, b):
    """Workgroup k + 1 of the tail starts on plane 3 of octave k as soon as tail_ready[k] is up, and the flags are cleared for
    the next image by another launch: a flag left up would let it read the PREVIOUS image's plane.  Two different images in
    turn on one plan, ten calls: after every call all planes and counts are those of the image just given."""
    frames = (pc.BY_NAME[a], pc.BY_NAME[b])
    assert frames[0].shape == frames[1].shape
    assert not np.array_equal(pc.expectations(oracle, frames[0]).planes[-1], pc.expectations(oracle, frames[1]).planes[-1])
    plan = _plan(frames[0])
    for call in range(10):
        check_call(plan, oracle, frames[call % 2], what="call %d of A, B, A, B, ..." % call)


def test_accessor_errors(siftlib, oracle):
    from sift_pyocl_amd import _lib
    frame = pc.BY_NAME["smooth128"]
    exp = pc.expectations(oracle, frame)
    plan = _plan(frame)
    L, h = siftlib, plan._handle
    buf = np.full(6 * 128 * 128 + 1, -7.0, np.float32)
    w, hh = C.c_int32(-1), C.c_int32(-1)
    first, cand, cs = C.c_int32(-1), np.full(4, -1, np.int32), np.full((4, 3), -1, np.int32)

    def planes(handle, octave, ptr, cap):
        return L.siftmi_plan_planes(handle, octave, ptr, cap, C.byref(w), C.byref(hh))

    def last(handle, pf, pc_, ps, n):
        return L.siftmi_plan_last_counts(handle, pf, pc_, ps, n)

    # a plan that has run nothing
    assert planes(h, 0, buf.ctypes.data, buf.size) == _lib.EINVAL and b"not finished a call" in L.siftmi_last_error()
    assert last(h, C.byref(first), cand.ctypes.data, cs.ctypes.data, 4) == _lib.EINVAL and b"not finished a call" in L.siftmi_last_error()
    with pytest.raises(RuntimeError):
        plan.planes(0)
    with pytest.raises(RuntimeError):
        plan.last_counts()
    want = plan.keypoints(pc.image(frame)).copy()
    # bad arguments on a finished call: refused, nothing written
    assert planes(None, 0, buf.ctypes.data, buf.size) == _lib.EINVAL
    assert planes(h, 0, None, buf.size) == _lib.EINVAL and b"null" in L.siftmi_last_error()
    assert planes(h, 0, buf.ctypes.data, 6 * 128 * 128 - 1) == _lib.EINVAL and b"needs" in L.siftmi_last_error()
    assert planes(h, -1, buf.ctypes.data, buf.size) == _lib.EINVAL and b"octave" in L.siftmi_last_error()
    assert planes(h, 4, buf.ctypes.data, buf.size) == _lib.EINVAL and b"octave" in L.siftmi_last_error()
    assert last(None, C.byref(first), cand.ctypes.data, cs.ctypes.data, 4) == _lib.EINVAL
    assert last(h, None, cand.ctypes.data, cs.ctypes.data, 4) == _lib.EINVAL
    assert last(h, C.byref(first), None, cs.ctypes.data, 4) == _lib.EINVAL
    assert last(h, C.byref(first), cand.ctypes.data, None, 4) == _lib.EINVAL
    assert last(h, C.byref(first), cand.ctypes.data, cs.ctypes.data, 3) == _lib.EINVAL and b"octaves" in L.siftmi_last_error()
    assert np.all(buf == -7.0) and (w.value, hh.value, first.value) == (-1, -1, -1) and np.all(cand == -1) and np.all(cs == -1)
    for octave in (-1, 4, 99):
        with pytest.raises(RuntimeError):
            plan.planes(octave)
    # an exact buffer is enough, the guard float behind it stays
    assert planes(h, 0, buf.ctypes.data, 6 * 128 * 128) == 0 and (w.value, hh.value) == (128, 128)
    assert buf[-1] == -7.0 and pc.plane_mismatch(buf[:-1].reshape(6, 128, 128), exp.planes[0], 0) is None
    assert planes(h, 3, buf.ctypes.data, 6 * 16 * 16) == 0 and (w.value, hh.value) == (16, 16)
    assert pc.plane_mismatch(buf[:6 * 256].reshape(6, 16, 16), exp.planes[3], 3) is None
    assert last(h, C.byref(first), cand.ctypes.data, cs.ctypes.data, 4) == 0 and first.value == 1
    # reading does not disturb the plan: the next call gives the same records, and its planes are there again
    for o in range(4):
        plan.planes(o)
    assert_same_keypoints(plan.keypoints(pc.image(frame)), want, "keypoints after planes()")
    assert pc.plane_mismatch(plan.planes(2), exp.planes[2], 2) is None
