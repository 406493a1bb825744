"""The octave hand-off, next[y][x] = plane3[2y][2x] (preprocess.cl:267-285), as a stage, bit for bit against the CPU oracle:
every fused blur form (k_pyramid.hpp: blur_hv_kernel, blur_tile2_kernel, blur_team_kernel) at every tap count with its
`half` / `next0` pointer set, the unfused shrink_kernel on every path it has, and a plan's wiring of the two.

siftmi_stage_blur_handoff makes the launch a plan makes for plane 3 and returns the half plane between two guards of
GUARD floats the kernel is not told of, the whole buffer filled with 0xa5 bytes before the launch.  The inputs are white
noise in [0, 255): every blur output is positive, so none can equal the fill (a negative float), and an element that
still holds the fill was never written.  A whole-frame comparison cannot show that: a plan's half plane keeps the last
frame's values, which are the right ones when the same frame is run again.

Every comparison is on uint32 views; there is no tolerance."""
import ctypes as C

import numpy as np
import pytest

from util import assert_same_keypoints, multiscale_noise, sort_kp, white_noise

pytestmark = pytest.mark.gpu

GUARD = 64                       # SIFTMI_STAGE_GUARD
FILL = np.uint32(0xa5a5a5a5)
TILE, TEAM, TILE2 = 1, 2, 3      # *kernel_used (0: the generic two-pass blur, which hands nothing off)
FORCE_TILE, FORCE_TILE2 = 1 << 2, 2 << 2     # bits 2-3 of xcd_map: the small-plane form, as in siftmi_stage_blur_ex
NTAPS = [11, 15, 17, 21, 27]     # the tap counts with fused instances

# (H, W).  32 x 16 tiles: every parity of H and W; test_tile_smallest_planes adds the two smallest legal planes per tap count
TILE_SHAPES = [(97, 131), (130, 96), (33, 47), (64, 64)]
# 32 x 32 tiles, and 32 x 64 tiles from 1024^2 pixels on
TILE2_SHAPES = [(300, 421), (97, 131), (33, 47), (700, 650), (1024, 1024), (1025, 1031)]
# The marching team kernel (planes of at least 1400^2 pixels, 1024 columns, 512 rows): all four parities, an odd W takes the
# scalar stores, (1400, 1401) sits just above the size rule.  Per shape [(xcd_map, march_wgs, parity of rows_out)]: a
# segment (grid row) of launch_team outputs
#     rows_out = max(ceil(H / gy), 2 N + 1)   with   gy = wgs / gx,   gx = ceil(W / 256),   wgs = 1024 (768 for 27 taps) by default
# rows from ys = by * rows_out on.  With an odd rows_out the segment starts alternate parity and `!(y & 1)` alone decides
# which of a segment's rows are handed off.  The default workgroup count gives 2 N + 1 on all four planes (odd); the counts
# below give 88 / 57, 62, 58 and 56 rows, at least the 55 of 27 taps, hence the same at every tap count.  Both workgroup orders
# (bit 0 of xcd_map) meet both parities.
TEAM_CASES = {(1408, 1536): [(1, 0, 1), (0, 96, 0), (1, 150, 1)],
              (1537, 1301): [(1, 0, 1), (0, 150, 0)],
              (1027, 2050): [(0, 0, 1), (1, 162, 0)],
              (1400, 1401): [(0, 0, 1), (1, 150, 0)]}
FALLBACK_SHAPE = (700, 650)
# the plane shrink_kernel reads: LW even (16-byte loads) and odd, SW mod 4 = 0 (16-byte stores), 1, 2, 3 -- a last thread with
# x + 3 >= SW that moves 1, 2 and 3 samples, (11, 20) behind two threads that load 16 bytes and store scalars --, SH odd and
# above 8 (more than one workgroup in y), three and five workgroups of 256 outputs in x (test_handoff_ref_host.py pins this)
SHRINK_SHAPES = [(10, 16), (9, 14), (19, 30), (21, 1030), (40, 2056), (301, 203), (2, 2), (3, 9), (11, 20)]
# frames whose octave 0 takes the 32 x 16 tile, the 32 x 32 tile and the team form
PLAN_SHAPES = [(300, 421), (601, 700), (1400, 1401)]
PLAN_SIGMAS = [1.0, 1.3, 1.6, 2.0, 2.5]      # 11 / 15 / 17 / 21 / 27 taps on the launch that writes plane 3 (test_handoff_ref_host.py)


def smallest_planes(ntaps):
    """the two smallest planes the blur is defined on (convolution.cl:45-48), one of each parity order"""
    m = (ntaps + 1) // 2
    return [(m, m + 1), (m + 1, m)]


def all_shapes():
    """every (H, W) a hand-off is computed on in this module"""
    small = [s for n in NTAPS for s in smallest_planes(n)]
    return sorted(set(TILE_SHAPES + small + TILE2_SHAPES + list(TEAM_CASES) + [FALLBACK_SHAPE] + SHRINK_SHAPES + PLAN_SHAPES))


def team_rows_out(W, H, ntaps, wgs):
    """launch_team's segment height, restated: it must follow siftmi.hip (launch_team: gx, gy, rows_out) by hand -- if the
    formula there moves and this one does not, the cases below keep passing with other parities than they state"""
    if wgs <= 0:
        wgs = 768 if ntaps >= 27 else 1024
    gx = (W + 255) // 256
    gy = min(max(wgs // gx, 1), H)
    return max((H + gy - 1) // gy, 2 * ntaps + 1)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _handoff(siftlib, img, taps, xcd_map, wgs=0):
    """(out, half with its guards, kernel_used) of siftmi_stage_blur_handoff"""
    H, W = img.shape
    out = np.empty((H, W), np.float32)
    half = np.zeros(GUARD + (W // 2) * (H // 2) + GUARD, np.float32)
    used = C.c_int32(-1)
    assert siftlib.siftmi_stage_blur_handoff(0, _p(img), _p(out), _p(half), W, H, _p(taps), len(taps), xcd_map, wgs, C.byref(used)) == 0
    return out, half, used.value


def _check(oracle, what, got, exp, want_form, handed=True):
    """out is the oracle's blur, the guards are untouched, every sample of the half plane was written, with the oracle's value"""
    out, half, used = got
    H, W = exp.shape
    assert used == want_form, "%s: kernel_used %d, not %d" % (what, used, want_form)
    bad = np.argwhere(out.view(np.uint32) != exp.view(np.uint32))
    assert bad.size == 0, "%s: out differs at %d samples, e.g. %r" % (what, len(bad), bad[:4].tolist())
    h = half.view(np.uint32)
    assert (h[:GUARD] == FILL).all(), "%s: write before the half plane, guard slots %r" % (what, np.nonzero(h[:GUARD] != FILL)[0][:4].tolist())
    assert (h[-GUARD:] == FILL).all(), "%s: write beyond the half plane, guard slots %r" % (what, np.nonzero(h[-GUARD:] != FILL)[0][:4].tolist())
    inner = h[GUARD:-GUARD].reshape(H // 2, W // 2)
    if not handed:
        assert (inner == FILL).all(), "%s: %d samples of the half plane written without a hand-off" % (what, int((inner != FILL).sum()))
        return
    left = np.argwhere(inner == FILL)
    assert left.size == 0, "%s: %d samples of the half plane never written, e.g. %r" % (what, len(left), left[:4].tolist())
    want = oracle.shrink(exp).view(np.uint32)
    assert want.shape == inner.shape
    bad = np.argwhere(inner != want)
    assert bad.size == 0, "%s: half plane differs at %d samples, e.g. %r" % (what, len(bad), bad[:4].tolist())


def _input(oracle, shape, ntaps, seed=0):
    img = white_noise(shape, seed=300 + ntaps + seed) * 255
    taps = oracle.gaussian_taps(ntaps / 8.0, ntaps)
    return img, taps, oracle.blur(img, taps)


@pytest.mark.parametrize("shape", TILE_SHAPES)
@pytest.mark.parametrize("ntaps", NTAPS)
def test_tile_form(siftlib, oracle, shape, ntaps):
    """blur_hv_kernel<N, false, 0, 32, 16, 4> with `half`"""
    img, taps, exp = _input(oracle, shape, ntaps)
    _check(oracle, "%r, %d taps" % (shape, ntaps), _handoff(siftlib, img, taps, 1 | FORCE_TILE), exp, TILE)


@pytest.mark.parametrize("ntaps", NTAPS)
def test_tile_smallest_planes(siftlib, oracle, ntaps):
    """half planes of 3 x 3 ... 7 x 7 samples inside one partial tile, whose window is reflected on all four sides"""
    for shape in smallest_planes(ntaps):
        img, taps, exp = _input(oracle, shape, ntaps)
        _check(oracle, "%r, %d taps" % (shape, ntaps), _handoff(siftlib, img, taps, 1 | FORCE_TILE), exp, TILE)


@pytest.mark.parametrize("shape", TILE2_SHAPES)
@pytest.mark.parametrize("ntaps", NTAPS)
def test_tile2_form(siftlib, oracle, shape, ntaps):
    """blur_tile2_kernel<N, false, 0, 32, 32> and, from 1024^2 pixels on, <N, false, 0, 32, 64> with `half`"""
    img, taps, exp = _input(oracle, shape, ntaps)
    _check(oracle, "%r, %d taps" % (shape, ntaps), _handoff(siftlib, img, taps, 1 | FORCE_TILE2), exp, TILE2)


@pytest.mark.parametrize("shape", sorted(TEAM_CASES))
@pytest.mark.parametrize("ntaps", NTAPS)
def test_team_form(siftlib, oracle, shape, ntaps):
    """blur_team_kernel<N, false, S> with `next0`: odd and even segment heights, both workgroup orders"""
    H, W = shape
    img, taps, exp = _input(oracle, shape, ntaps)
    for xcd_map, wgs, odd in TEAM_CASES[shape]:
        rows_out = team_rows_out(W, H, ntaps, wgs)
        assert rows_out % 2 == odd, "march_wgs %d gives segments of %d rows on %r" % (wgs, rows_out, shape)
        _check(oracle, "%r, %d taps, xcd_map %d, march_wgs %d (segments of %d rows)" % (shape, ntaps, xcd_map, wgs, rows_out),
               _handoff(siftlib, img, taps, xcd_map, wgs), exp, TEAM)


def test_fallbacks(siftlib, oracle):
    """Taps that are not bitwise symmetric take the 32 x 16 tile kernel whatever form is asked for, and hand off; a tap count
    without a fused kernel (12, even) takes the generic two-pass blur, which does not: the half plane keeps its fill."""
    img = white_noise(FALLBACK_SHAPE, seed=3) * 255
    asym = oracle.gaussian_taps(15 / 8.0, 15).copy()
    asym[0] = np.nextafter(asym[0], np.float32(1))                   # no longer bitwise symmetric
    _check(oracle, "asymmetric taps", _handoff(siftlib, img, asym, 1 | FORCE_TILE2), oracle.blur(img, asym), TILE)
    even = oracle.gaussian_taps(12 / 8.0, 12)
    _check(oracle, "12 taps", _handoff(siftlib, img, even, 1 | FORCE_TILE2), oracle.blur(img, even), 0, handed=False)


def test_rejected_arguments(siftlib):
    """SIFTMI_EINVAL (-1) with nothing launched: a null pointer, an empty plane, a tap count outside 1..64"""
    a = np.zeros((8, 8), np.float32); half = np.zeros(2 * GUARD + 16, np.float32); taps = np.ones(65, np.float32)
    call = siftlib.siftmi_stage_blur_handoff
    assert call(0, None, _p(a), _p(half), 8, 8, _p(taps), 11, 0, 0, None) == -1
    assert call(0, _p(a), None, _p(half), 8, 8, _p(taps), 11, 0, 0, None) == -1
    assert call(0, _p(a), _p(a), None, 8, 8, _p(taps), 11, 0, 0, None) == -1
    assert call(0, _p(a), _p(a), _p(half), 8, 8, None, 11, 0, 0, None) == -1
    assert call(0, _p(a), _p(a), _p(half), 0, 8, _p(taps), 11, 0, 0, None) == -1
    assert call(0, _p(a), _p(a), _p(half), 8, 0, _p(taps), 11, 0, 0, None) == -1
    assert call(0, _p(a), _p(a), _p(half), 8, 8, _p(taps), 0, 0, 0, None) == -1
    assert call(0, _p(a), _p(a), _p(half), 8, 8, _p(taps), 65, 0, 0, None) == -1


@pytest.mark.parametrize("shape", SHRINK_SHAPES)
def test_shrink_kernel(siftlib, oracle, shape):
    """shrink_kernel, the unfused hand-off: both 16-byte loads and the 16-byte store, the scalar paths, the tail thread"""
    H, W = shape
    img = white_noise(shape, seed=H + W) + 1.0
    out = np.empty((H // 2, W // 2), np.float32)
    assert siftlib.siftmi_stage_shrink(0, _p(img), _p(out), W, H) == 0
    assert np.array_equal(out.view(np.uint32), img[:2 * (H // 2):2, :2 * (W // 2):2].view(np.uint32))
    assert np.array_equal(out.view(np.uint32), oracle.shrink(img).view(np.uint32))


@pytest.mark.parametrize("shape", PLAN_SHAPES)
@pytest.mark.parametrize("init_sigma", PLAN_SIGMAS)
def test_plan_fused_against_unfused(siftlib, oracle, shape, init_sigma):
    """A plan with the hand-off inside its plane-3 blur launch against one that runs shrink_kernel (`fused_shrink` 0), at
    every tap count of that launch: the same records byte for byte.  Another image of the same shape runs in between, so a
    sample of a half plane that a launch leaves out holds that image's value, not the right one."""
    import sift_pyocl_amd as sp
    img, other = multiscale_noise(shape, seed=5), multiscale_noise(shape, seed=6)
    fused = sp.SiftPlan(template=img, init_sigma=init_sigma)
    plain = sp.SiftPlan(template=img, init_sigma=init_sigma)
    plain.set_option("fused_shrink", 0)
    runs = []
    for frame in (img, other, img):
        got = [plan.keypoints(frame) for plan in (fused, plain)]
        assert not fused.overflow and not plain.overflow
        runs.append(got)
    for call in (0, 2):
        a, b = runs[call]
        what = "%r, init_sigma %g, call %d" % (shape, init_sigma, call)
        # Keypoints of octave 1 and below: without them the hand-off decided nothing.  An octave-0 keypoint has scale
        # init_sigma * 2^((s + offset) / 3) with s <= 3 and |offset| <= 1.5 (image.cl:354), at most 2^1.5 = 2.83 init_sigma.
        assert int((a["scale"] > 2.9 * init_sigma).sum()) > 0, what
        assert_same_keypoints(a, b, what)
        assert sort_kp(a).tobytes() == sort_kp(b).tobytes(), what
        if shape == PLAN_SHAPES[0]:
            assert_same_keypoints(a, oracle.keypoints(img, par=oracle.default_params(init_sigma=init_sigma)), what + ", oracle")
