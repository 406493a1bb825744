"""Every option of siftmi_plan_set_option against the oracle: "results never depend on an option" (include/siftmi.h).

SWEEP maps each option name to the cases that make it take effect: (frame, options set on a fresh plan).  The frames are
chosen for the paths they reach -- a small one (tail kernel, tiled blur, fused refinement), a marching one of at least
1400^2 (marching blur, separate refinement launch), a 2048^2 one for the tiled blur of a full plane, a keypoint-rich lattice
(gradient maps, the descriptor launch of a large group), a five-octave one (the forked chains) and typed frames (the fused
converter).  Every case runs twice on its plan (the "previous image" rules) and must equal the oracle bit for bit.

The minimum workgroup counts are safe to run: no workgroup of the orientation, descriptor, gradient-map, min/max or marching
launches waits on another workgroup of the same launch (the descriptor launch's record block is published by workgroup 0,
which waits for nobody: k_keypoint.hpp descriptor_open); the tail kernel's chain waits with a bound (k_tail.hpp).
The LDS pads are bounded by the library (SIFT_LDS_PAD_MAX); values beyond it are rejected, not run.

test_sweep_covers_every_option needs no GPU: it reads the option names of include/siftmi.h and of siftmi_plan_set_option
and fails when a name is missing from SWEEP."""
import os
import re

import numpy as np
import pytest

from util import assert_same_keypoints, smooth_noise

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BIG = (1280, 1536)          # march_plane(): W >= 1024, H >= 512, W * H >= 1400^2
HUGE = 1 << 30

# option -> [(frame, {option: value, ...})]
SWEEP = {
    "fused_convert": [("u16", {"fused_convert": 0}), ("u16_big", {"fused_convert": 0})],
    "overlap": [("big", {"overlap": 0}), ("rich", {"overlap": 0})],
    "march": [("full2048", {"march": 0}), ("big", {"march": 0})],
    "march_wgs": [("big", {"march_wgs": 1}), ("big", {"march_wgs": 3}), ("big", {"march_wgs": 77}), ("big", {"march_wgs": 5000})],
    "xcd_map": [("big", {"xcd_map": 0}), ("small", {"xcd_map": 0})],
    "march_prio": [("big", {"march_prio": 0}), ("big", {"march_prio": 2})],
    "mm_blocks": [("small", {"mm_blocks": 1}), ("u16", {"mm_blocks": 1}), ("big", {"mm_blocks": 1}), ("u16_big", {"mm_blocks": 3})],
    "mm_threads": [("small", {"mm_threads": 256}), ("small", {"mm_threads": 512}), ("big", {"mm_threads": 256, "mm_blocks": 1}),
                   ("u16", {"mm_threads": 256}), ("u16", {"mm_threads": 512}), ("u16_big", {"mm_threads": 1024})],
    "ext_rows": [("small", {"ext_rows": 1}), ("small", {"ext_rows": 7}), ("small", {"ext_rows": 400}),
                 ("big", {"ext_rows": 1}), ("big", {"ext_rows": 13}), ("big", {"ext_rows": BIG[0]})],
    "ext_strips": [("small", {"ext_strips": 1}), ("big", {"ext_strips": 1}), ("big", {"ext_strips": HUGE})],
    "ori_blocks": [("small", {"ori_blocks": 1}), ("rich", {"ori_blocks": 1})],
    "ori_small_blocks": [("small", {"ori_small_blocks": 1}), ("big", {"ori_small_blocks": 1})],
    "ori_pad": [("small", {"ori_pad": 4096}), ("big", {"ori_pad": 65536})],
    "ori_team": [("big", {"ori_team": 0}), ("big", {"ori_team": HUGE})],
    "desc_blocks": [("small", {"desc_blocks": 1}), ("rich", {"desc_blocks": 1}), ("rich", {"desc_blocks": 1, "maps": 1})],
    "desc_small_blocks": [("big", {"desc_small_blocks": 1}), ("big", {"desc_small_blocks": 1, "early_chain": 0})],
    "desc_early_blocks": [("big", {"desc_early_blocks": 1, "early_chain": 1})],
    "desc_dense_blocks": [("dense", {"desc_dense_blocks": 1})],
    "desc_pad": [("small", {"desc_pad": 65536}), ("big", {"desc_pad": 20000})],
    "desc_team": [("big", {"desc_team": 0}), ("big", {"desc_team": HUGE})],
    "desc_dynamic": [("big", {"desc_dynamic": 0}), ("big", {"desc_dynamic": 0, "desc_team": 0})],
    "desc_stream": [("big", {"desc_stream": 1})],
    "maps_blocks": [("rich", {"maps": 1, "maps_blocks": 1}), ("big", {"maps": 1, "maps_blocks": 3})],
    "fused_refine": [("small", {"fused_refine": 0}), ("big", {"fused_refine": 2})],
    "fused_shrink": [("small", {"fused_shrink": 0}), ("big", {"fused_shrink": 0})],
    "tail": [("small", {"tail": 0}), ("five", {"tail": 0})],
    "tail_pixels": [("small", {"tail_pixels": 1}), ("five", {"tail_pixels": 1})],
    "maps": [("rich", {"maps": 0}), ("rich", {"maps": 1}), ("big", {"maps": 1})],
    "maps_density": [("rich", {"maps_density": 1}), ("rich", {"maps_density": HUGE}), ("big", {"maps_density": HUGE})],
    "fork": [("five", {"fork": 0}), ("five", {"fork": 1}), ("big", {"fork": 0}), ("small", {"fork": 1})],
    "split": [("five", {"split": 1, "fork": 0}), ("big", {"split": 1, "fork": 0, "early_chain": 0})],
    "early_chain": [("big", {"early_chain": 0}), ("big", {"early_chain": 1}), ("rich", {"early_chain": 1})],
    "spin": [("small", {"spin": 0}), ("big", {"spin": 0})],
    "host_timing": [("small", {"host_timing": 1})],
    "tail_fault": [("small", {"tail_fault": 1}), ("five", {"tail_fault": 2})],
}

# values the library must refuse (never run): beyond the LDS budget, outside int32, out of range
REJECTED = [("ori_pad", 65537), ("ori_pad", -1), ("desc_pad", 65537), ("desc_pad", -1), ("desc_pad", 1 << 20),
            ("desc_team", 1 << 32), ("ori_team", 1 << 32), ("march_wgs", -(1 << 31) - 1), ("ext_rows", 1 << 31),
            ("maps", 1 << 32), ("tail_pixels", 0), ("mm_threads", 128), ("mm_blocks", 0), ("ext_strips", 0)]


def _header_names():
    text = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    start = text.index("Tuning / diagnostic option of one plan by name")
    block = text[start:text.index("int siftmi_plan_set_option", start)]
    block = re.sub(r"\([^()]*(\([^()]*\)[^()]*)*\)", "", block)        # drop the parenthesised explanations
    return set(re.findall(r'"([a-z_0-9]+)"', block))


def _library_names():
    text = open(os.path.join(ROOT, "sift_pyocl_amd", "csrc", "siftmi.hip")).read()
    start = text.index("int siftmi_plan_set_option(")
    body = text[start:text.index("\n}\n", start)]
    return set(re.findall(r'n == "([a-z_0-9]+)"', body))


def test_sweep_covers_every_option():
    """The names documented in the header, the names the library accepts and the keys of SWEEP are one set, and every
    case of an option sets that option: a new option without a sweep case fails here."""
    header, library = _header_names(), _library_names()
    assert len(library) >= 30
    assert header == library, "header only: %s, library only: %s" % (sorted(header - library), sorted(library - header))
    assert set(SWEEP) == library, "no sweep case: %s, unknown: %s" % (sorted(library - set(SWEEP)), sorted(set(SWEEP) - library))
    for name, cases in SWEEP.items():
        assert cases, name
        for frame, opts in cases:
            assert name in opts and frame in FRAMES and set(opts) <= library, (name, frame, opts)
    assert {n for n, _ in REJECTED} <= library


def _frames():
    from test_gpu_edges import lattice
    small = smooth_noise((333, 402), seed=17, sigma=2.0)
    big = smooth_noise(BIG, seed=19, sigma=3.0)          # octave 0 below 16384 keypoints: the "small group" launches

    def u16(f):
        return ((f - f.min()) / (f.max() - f.min()) * 60000 + 1000).astype(np.uint16)
    return {
        "small": lambda: small,
        "big": lambda: big,
        "full2048": lambda: smooth_noise((2048, 2048), seed=21, sigma=2.0),
        "rich": lambda: lattice((1024, 1024), seed=23),
        "dense": lambda: lattice((2048, 2048), seed=29),
        "five": lambda: smooth_noise((400, 520), seed=31, sigma=1.5),
        "u16": lambda: u16(small),
        "u16_big": lambda: u16(big),
    }


FRAMES = ("small", "big", "full2048", "rich", "dense", "five", "u16", "u16_big")


@pytest.fixture(scope="module")
def expected(oracle):
    """frame name -> (frame, oracle result of frame.astype(float32)), computed on first use"""
    makers, cache = _frames(), {}

    def get(name):
        if name not in cache:
            img = makers[name]()
            cache[name] = (img, oracle.keypoints(img.astype(np.float32)))
        return cache[name]
    return get


CASES = [(name, i) for name in sorted(SWEEP) for i in range(len(SWEEP[name]))]


@pytest.mark.gpu
@pytest.mark.parametrize("name,i", CASES, ids=["%s-%d" % c for c in CASES])
def test_option_case_equals_oracle(siftlib, oracle, expected, capfd, name, i):
    import sift_pyocl_amd as sp
    frame, opts = SWEEP[name][i]
    img, want = expected(frame)
    if frame == "five":
        assert oracle.octave_count(*img.shape) >= 5
    if frame in ("rich", "dense"):
        assert len(want) >= img.size // 200                      # keypoint-rich: the maps / early-chain density rules fire
    plan = sp.SiftPlan(template=img)
    for k, v in opts.items():
        plan.set_option(k, v)
    for call in range(2):
        got = plan.keypoints(img)
        assert not plan.overflow
        assert_same_keypoints(got, want, "%s: %r, call %d" % (frame, opts, call))
    if name == "host_timing":
        out = capfd.readouterr()
        assert (out.out + out.err).strip(), "host_timing 1 printed nothing"


@pytest.mark.gpu
def test_rejected_values_leave_the_plan_unchanged(siftlib, expected):
    """Out-of-range values fail with SIFTMI_EINVAL (RuntimeError) -- in particular 1 << 32 is no longer truncated to 0 -- and
    the option keeps its value: the plan still computes the oracle's records."""
    import sift_pyocl_amd as sp
    img, want = expected("small")
    plan = sp.SiftPlan(template=img)
    for name, value in REJECTED:
        with pytest.raises(RuntimeError):
            plan.set_option(name, value)
    for name in sorted(SWEEP):
        for value in (1 << 31, -(1 << 31) - 1, 1 << 40, -(1 << 62)):
            with pytest.raises(RuntimeError):
                plan.set_option(name, value)
    assert_same_keypoints(plan.keypoints(img), want, "after rejected options")
    bp = sp.BatchPlan(template=img, lanes=2)
    with pytest.raises(RuntimeError):
        bp.set_option("desc_team", 1 << 32)
    with pytest.raises(RuntimeError):
        bp.set_option("desc_pad", 65537)


@pytest.mark.gpu
def test_batch_set_option(siftlib, expected):
    """BatchPlan.set_option reaches every lane: odd strip heights and one-workgroup launches through a two-lane batch."""
    import sift_pyocl_amd as sp
    img, want = expected("small")
    u16, want16 = expected("u16")
    bp = sp.BatchPlan(template=img, lanes=2)
    for name, value in (("ext_rows", 7), ("desc_blocks", 1), ("ori_blocks", 1), ("mm_blocks", 1), ("tail", 0)):
        bp.set_option(name, value)
    for r in bp.keypoints_batch([img, img, img]):
        assert_same_keypoints(r, want, "BatchPlan with options")
    bp16 = sp.BatchPlan(template=u16, lanes=2)
    bp16.set_option("fused_convert", 0)
    bp16.set_option("mm_threads", 256)
    for r in bp16.keypoints_batch([u16, u16]):
        assert_same_keypoints(r, want16, "uint16 BatchPlan with options")
