"""What tests/test_gpu_pyramid_cases.py rests on, checked without a GPU: the two accessors are part of the C ABI and refuse a
null plan, the restated tail rule sends every frame to the tail octaves it is there for, most tail octaves have no candidate
(so no record could ever show their planes) while a few do, and the tail kernel's wave walk carries parked candidates from one
strip to the next on these frames -- but never fills its buffer."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyramid_cases as pc
import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_accessors_are_declared_exported_and_bound():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "siftmi.h")).read(), flags=re.S)
    for name in ("siftmi_plan_planes", "siftmi_plan_last_counts"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in include/siftmi.h" % name
        assert hasattr(L, name) and name in _lib.exported_symbols()
    import sift_pyocl_amd as sp
    assert callable(sp.SiftPlan.planes) and callable(sp.SiftPlan.last_counts)
    # a null plan is refused before anything touches a device: the same answer on any machine
    buf = np.full(6 * 16 * 16, 7.0, np.float32)
    w, h = C.c_int32(-1), C.c_int32(-1)
    assert L.siftmi_plan_planes(None, 0, buf.ctypes.data, buf.size, C.byref(w), C.byref(h)) == _lib.EINVAL
    assert b"null plan" in L.siftmi_last_error()
    assert (w.value, h.value) == (-1, -1) and np.all(buf == 7.0)
    first, cand, cs = C.c_int32(-1), np.full(8, -1, np.int32), np.full((8, 3), -1, np.int32)
    assert L.siftmi_plan_last_counts(None, C.byref(first), cand.ctypes.data, cs.ctypes.data, 8) == _lib.EINVAL
    assert b"null plan" in L.siftmi_last_error()
    assert first.value == -1 and np.all(cand == -1) and np.all(cs == -1)


@pytest.mark.parametrize("frame", pc.FRAMES, ids=lambda f: f.name)
def test_tail_rule_reaches_the_stated_octaves(oracle, frame):
    H, W = frame.shape
    sizes = pc.octave_sizes(H, W)
    assert len(sizes) == oracle.octave_count(H, W)
    first = pc.tail_first(sizes)
    assert sizes[first:] == pc.TAIL_OCTAVES[frame.name], (frame.name, sizes, first)
    for w, h in sizes[first:]:
        assert w * h <= pc.TAIL_PIXELS and w <= 128 and h <= 128 and min(w, h) >= 14
    assert pc.tail_first(sizes, tail=0) == len(sizes)


def test_tail_rule_details():
    """the cases the frame list is built around, spelled out"""
    sz = pc.octave_sizes
    assert sz(128, 128) == [(128, 128), (64, 64), (32, 32), (16, 16)] and pc.tail_first(sz(128, 128)) == 1
    assert sz(111, 111)[-1] == (13, 13) and pc.tail_first(sz(111, 111)) == 4             # a side below 14: refused
    assert sz(58, 280)[1] == (140, 29) and 140 * 29 <= pc.TAIL_PIXELS and pc.tail_first(sz(58, 280)) == 2     # W > 128
    assert sz(56, 300)[1] == (150, 28) and 150 * 28 == 4200 and pc.tail_first(sz(56, 300)) == 2 == len(sz(56, 300)) - 1
    assert pc.tail_first(sz(300, 56)) == 2 == len(sz(300, 56)) - 1
    assert len(sz(512, 512)) == 6 and pc.tail_first(sz(512, 512)) == 3
    # option "tail_pixels" = 1024 moves the first tail octave down on the frames of the option sets
    assert [pc.tail_first(sz(*s), tail_pixels=1024) for s in ((128, 128), (64, 256), (130, 250), (512, 512))] == [2, 2, 3, 4]
    # every pitch remainder, an odd last column and an odd height among the tail octaves
    tails = [s for f in pc.FRAMES for s in pc.TAIL_OCTAVES[f.name]]
    assert {w % 4 for w, _ in tails} == {0, 1, 2, 3} and any(h % 2 for _, h in tails)
    # dynamic LDS beyond 64 KiB for exactly the W = 128 / H = 128 first octaves (tail_lds_bytes, k_tail.hpp)
    def lds(w, h):
        pt = (w + 3) & ~3
        blur = h * (pt + 32) + (h + 26) * pt
        ext = pc.TAIL_WAVES * (pc.TAIL_EXT_BUF + 192) * 4
        return 4 * (h * pt + max(blur, ext))
    assert (lds(128, 32), lds(32, 128), lds(64, 64)) == (66560, 68864, 64000)
    assert {f.name for f in pc.FRAMES if pc.TAIL_OCTAVES[f.name] and lds(*pc.TAIL_OCTAVES[f.name][0]) > 65536} == {
        "smooth64x256", "white64x256", "multi256x64"}
    assert sum(f.maker == "white_noise" for f in pc.FRAMES) >= 2 and any(f.dtype == "uint8" for f in pc.FRAMES)


def _tail_octaves(oracle, frames):
    for frame in frames:
        exp = pc.expectations(oracle, frame)
        for o in range(pc.tail_first(exp.sizes), len(exp.sizes)):
            yield frame, o, exp


def test_most_tail_octaves_have_no_candidate(oracle):
    """The hole the plane comparison closes: a tail octave without a candidate has no record.  Some do have one -- the
    candidate lists, the per-scale counts and the records of the tail are compared on them."""
    zero, nonzero = [], []
    for frame, o, exp in _tail_octaves(oracle, pc.FRAMES):
        (nonzero if exp.c_scale[o].sum() else zero).append((frame.name, exp.sizes[o], int(exp.c_scale[o].sum())))
    print("tail octaves without a candidate:", zero)
    print("tail octaves with candidates:", nonzero)
    assert len(zero) >= 6 and len(nonzero) >= 3
    # octave 1 of every frame that is not white noise has candidates
    for frame in pc.SMALL_FRAMES:
        if frame.maker == "white_noise":
            continue
        assert pc.expectations(oracle, frame).c_scale[1].sum() > 0, frame.name


def test_parking_buffer_replay(oracle):
    """The tail kernel's wave walk on the oracle's candidates.  A wave that holds candidates of two of its strips has carried
    `pending` from one strip into the next; the largest number a wave ever holds stays far below SIFT_TAIL_EXT_BUF, also
    counted before the edge test (as the entries are parked): the flush inside extrema_strip is not reached by any frame here."""
    carried, worst, worst_raw = [], (0, None), (0, None)
    for frame, o, exp in _tail_octaves(oracle, pc.FRAMES):
        W, H = exp.sizes[o]
        total, strips = pc.wave_totals(exp.cands[o], W, H)
        assert total.sum() == exp.c_scale[o].sum()
        if strips.max() >= 2:
            carried.append((frame.name, o))
        worst = max(worst, (int(total.max()), (frame.name, o)))
        raw = pc.unfiltered_candidates(oracle, oracle.dog(exp.planes[o]), 2 ** o)
        assert len(raw) >= len(exp.cands[o])
        worst_raw = max(worst_raw, (int(pc.wave_totals(raw, W, H)[0].max()), (frame.name, o)))
    print("largest per-wave total of candidates: %d of %d slots, at %r" % (worst[0], pc.TAIL_EXT_BUF, worst[1]))
    print("largest per-wave total before the edge test: %d of %d slots, at %r" % (worst_raw[0], pc.TAIL_EXT_BUF, worst_raw[1]))
    print("tail octaves where a wave carries candidates across strips:", carried)
    assert carried, "no tail octave makes a wave carry parked candidates from one strip to the next"
    assert worst_raw[0] <= pc.TAIL_EXT_BUF, "a frame reaches the in-launch flush: it is no longer untested, say so in DESIGN.md"
