"""The small-plane tile blur (k_pyramid.hpp: blur_tile2_kernel) reached as a stage and through a plan, bit for bit against
the CPU oracle.  siftmi_stage_blur_ex reports the kernel that ran (3 = blur_tile2_kernel); bits 2-3 of its xcd_map
argument pick the small-plane form (1 + Options::small_blur)."""
import ctypes as C

import numpy as np
import pytest

from util import assert_same_keypoints, smooth_noise, white_noise

pytestmark = pytest.mark.gpu

TILE, TEAM, TILE2 = 1, 2, 3
FORCE_TILE, FORCE_TILE2, BY_SIZE = 1 << 2, 2 << 2, 3 << 2

# (H, W): square, odd both ways, wide, just past 1024 both ways (32 x 64 tiles), small, partial 32 x 32 tiles both ways
SHAPES = [(1024, 1024), (1023, 1021), (513, 1300), (1025, 1030), (300, 421), (700, 650)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _blur(siftlib, frame, code, W, H, taps, norm, flags):
    out = np.empty((H, W), np.float32)
    used = C.c_int32(-1)
    frame = np.ascontiguousarray(frame)
    assert siftlib.siftmi_stage_blur_ex(0, _p(frame), code, _p(out), W, H, _p(taps), len(taps), norm, 1 | flags, 0,
                                        C.byref(used)) == 0
    return out, used.value


def _same(a, b):
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    return bad.size == 0, (len(bad), bad[:4])


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("ntaps", [11, 15, 17, 21, 27])
def test_tile2_bit_exact(siftlib, oracle, shape, ntaps):
    H, W = shape
    img = white_noise(shape, seed=200 + ntaps) * 255
    taps = oracle.gaussian_taps(ntaps / 8.0, ntaps)
    exp = oracle.blur(img, taps)
    out, used = _blur(siftlib, img, 0, W, H, taps, 0, FORCE_TILE2)
    assert used == TILE2, "the plane did not reach blur_tile2_kernel"
    ok, why = _same(out, exp)
    assert ok, (ntaps, why)
    out, used = _blur(siftlib, img, 0, W, H, taps, 0, FORCE_TILE)
    assert used == TILE
    ok, why = _same(out, exp)
    assert ok, (ntaps, why)


def test_size_rule(siftlib, oracle):
    """By default planes from 600^2 pixels up to the marching cross-over take the new form, smaller ones the 32 x 16 tile."""
    taps = oracle.gaussian_taps(17 / 8.0, 17)
    for (H, W), want in [((1024, 1024), TILE2), ((1024, 1023), TILE2), ((600, 600), TILE2), ((599, 600), TILE), ((512, 512), TILE), ((300, 421), TILE),
                         ((1408, 1536), TEAM)]:
        img = white_noise((H, W), seed=H) * 255
        exp = oracle.blur(img, taps)
        for flags in (0, BY_SIZE):
            out, used = _blur(siftlib, img, 0, W, H, taps, 0, flags)
            assert used == want, ((H, W), flags, used)
            ok, why = _same(out, exp)
            assert ok, ((H, W), why)


def test_asymmetric_and_even_taps_fall_back(siftlib, oracle):
    H, W = 700, 650
    img = white_noise((H, W), seed=3) * 255
    asym = oracle.gaussian_taps(15 / 8.0, 15).copy()
    asym[0] = np.nextafter(asym[0], np.float32(1))                   # no longer bitwise symmetric
    even = oracle.gaussian_taps(12 / 8.0, 12)
    for taps, want in [(asym, TILE), (even, 0)]:
        exp = oracle.blur(img, taps)
        out, used = _blur(siftlib, img, 0, W, H, taps, 0, FORCE_TILE2)
        assert used == want, (len(taps), used)
        ok, why = _same(out, exp)
        assert ok, (len(taps), why)


@pytest.mark.parametrize("shape", [(1023, 1021), (300, 421)])
def test_tile2_normalising_and_typed_instances(siftlib, oracle, shape):
    """blur_tile2_kernel<15, NORM = true, DT>: `normalizes` applied while staging, behind the min/max pass; DT != 0: the
    integer / RGB converters at the point of use."""
    H, W = shape
    taps = oracle.gaussian_taps(float(np.sqrt(1.6 ** 2 - 0.25)), 15)
    rng = np.random.default_rng(H)
    f32 = (white_noise(shape, seed=9) - 0.25) * 3000.0
    u8 = rng.integers(0, 256, shape, dtype=np.uint8)
    u16 = rng.integers(0, 65536, shape, dtype=np.uint16)
    u32 = rng.integers(0, 2 ** 32, shape, dtype=np.uint32)
    i32 = rng.integers(-2 ** 31, 2 ** 31, shape, dtype=np.int32)
    u64 = rng.integers(0, 2 ** 63, shape, dtype=np.uint64)
    i64 = rng.integers(-2 ** 62, 2 ** 62, shape, dtype=np.int64)
    rgb = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    r, g, b = (rgb[..., c].astype(np.float32) for c in range(3))
    rgb32 = (np.float32(0.299) * r + np.float32(0.587) * g) + np.float32(0.114) * b
    cases = [("f32", 0, f32, f32), ("u8", 1, u8, u8.astype(np.float32)), ("u16", 2, u16, u16.astype(np.float32)),
             ("u32", 3, u32, u32.astype(np.float32)), ("u64", 4, u64, u64.astype(np.float32)),
             ("i32", 5, i32, i32.astype(np.float32)), ("i64", 6, i64, i64.astype(np.float32)), ("rgb8", 8, rgb, rgb32)]
    for name, code, frame, as32 in cases:
        as32 = np.ascontiguousarray(as32, np.float32)
        exp = oracle.blur(oracle.normalize(as32, as32.min(), as32.max()), taps)
        out, used = _blur(siftlib, frame, code, W, H, taps, 1, FORCE_TILE2)
        assert used == TILE2, name
        ok, why = _same(out, exp)
        assert ok, (name, why)


@pytest.mark.parametrize("shape", [(1024, 1024), (1023, 901)])
def test_tile2_frames_and_fused_half(siftlib, oracle, shape):
    """Frames whose octave 0 takes blur_tile2_kernel under the default size rule: its plane-3 launch also writes the next
    octave's plane 0 (`half`), which every later octave's keypoints depend on.  (The hand-off as a stage, with guards around
    the half plane and every tap count: tests/test_gpu_handoff.py.)"""
    import sift_pyocl_amd as sp
    img = smooth_noise(shape, seed=41, sigma=2.0)
    taps = oracle.gaussian_taps(17 / 8.0, 17)
    _, used = _blur(siftlib, white_noise(shape, seed=1) * 255, 0, shape[1], shape[0], taps, 0, 0)
    assert used == TILE2
    want = oracle.keypoints(img)
    plan = sp.SiftPlan(template=img)
    for call in range(2):
        got = plan.keypoints(img)
        assert not plan.overflow
        assert_same_keypoints(got, want, "%r, call %d" % (shape, call))
