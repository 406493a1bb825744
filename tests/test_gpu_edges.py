"""Dense, degenerate and extreme-range frames against the oracle.

* An "extrema lattice" (alternating-sign isotropic blobs on a jittered grid) packs so many DoG extrema into one extrema strip
  that the wave's parking buffer (SIFT_EXT_BUF = 128 candidates, k_extrema.hpp extrema_strip) fills and is flushed in the
  middle of the strip; test_lattice_strips_overflow_the_parking_buffer proves that on the host from the oracle's candidates.
  Isotropic blobs also give many extra orientations per keypoint, and a 2048^2 lattice puts more than 65 536 keypoints into
  one group (the desc_dense_blocks launch).
* Constant frames (normalisation 0 / 0), frames whose range is a few ulp, subnormal, or overflows 255 * (x - min), all-negative
  frames, float64 frames and 64-bit / 32-bit integer frames at the ends of their types: every one bit-exact with the oracle run
  on frame.astype(float32), at a tiled and at a marching size.
* A sequence of very different frames through one plan (the rules that look at the previous image, list growth).
* Min / max with NaN pixels: the reference's default path (max_min_global_stage1/2, plan.py:490-522) reduces with fmax / fmin
  (reductions.cl:44), which ignore NaN.  Checked at the stage level and through SiftPlan.minmax() on frames whose planes are
  NaN everywhere after the initial blur.  Out of scope: keypoint parity of a frame with some NaN pixels -- the reference's
  orientation and descriptor code then takes (int) of a NaN (the oracle restates it), which is undefined behaviour in both.
"""
import ctypes as C
import warnings

import numpy as np
import pytest

from util import assert_same_keypoints, lattice, smooth_noise, sort_kp
from test_gpu_params import CASES as PAR_CASES

BORDER = 5                      # par.BorderDist
LATTICE_ROWS = 256              # ext_rows of the lattice runs: 62 x 256 sample strips
SIFT_EXT_BUF = 128
TILED = (333, 402)
MARCH = (1280, 1536)            # march_plane(): the marching blur, refinement in its own launch


def extrema_strip_rows(W, H, border=BORDER, min_strips=2000):
    """k_extrema.hpp extrema_strip_rows restated: rows of a strip when option ext_rows is 0."""
    nx = (W - 2 * border + 61) // 62
    rows = 64
    while rows > 4 and nx * ((H - 2 * border + rows - 1) // rows) < min_strips:
        rows >>= 1
    return rows


def strip_counts(oracle, img, rows):
    """Octave-0 candidates that pass the oracle's local_maxmin (extremum, contrast and edge tests: image.cl:119-213) per
    extrema strip of the GPU kernel -- 62 columns x `rows` rows from (BORDER, BORDER) -- over the three detection scales."""
    from util import oracle_pyramid
    (_, dogs), = oracle_pyramid(oracle, img, 1)
    H, W = img.shape
    nx = (W - 2 * BORDER + 61) // 62
    counts = np.zeros(nx * ((H - 2 * BORDER + rows - 1) // rows), np.int64)
    for scale in (1, 2, 3):
        kps, n = oracle.local_maxmin(dogs, scale, 1, H * W)
        r, c = kps[:n, 1].astype(np.int64), kps[:n, 2].astype(np.int64)
        np.add.at(counts, ((r - BORDER) // rows) * nx + (c - BORDER) // 62, 1)
    return counts


def test_lattice_strips_overflow_the_parking_buffer(oracle):
    """Host-side proof that the lattice runs reach the flush branch of extrema_strip: a wave parks every extremum of its
    strip and flushes when more than SIFT_EXT_BUF are parked; the entries that survive the edge test are a subset of those,
    so a strip with more than SIFT_EXT_BUF survivors has flushed at least once."""
    for shape, seed in (((1024, 1024), 23), ((2048, 2048), 29)):
        counts = strip_counts(oracle, lattice(shape, seed=seed), LATTICE_ROWS)
        print("lattice %r: %d strips of 62 x %d, %d above %d, largest %d" % (shape, counts.size, LATTICE_ROWS,
              (counts > SIFT_EXT_BUF).sum(), SIFT_EXT_BUF, counts.max()))
        assert (counts > SIFT_EXT_BUF).sum() >= counts.size // 2 and counts.max() > SIFT_EXT_BUF
    # at the default strip heights (16 - 64 rows) even the lattice stays below the buffer: hence ext_rows in the GPU runs
    assert extrema_strip_rows(1024, 1024) <= 16 and extrema_strip_rows(2048, 2048) == 32


def test_oracle_minmax_ignores_nan(oracle):
    rng = np.random.default_rng(3)
    img = rng.normal(0, 100, (61, 67)).astype(np.float32)
    for where in ([0], [img.size - 1], [0, 5, 77, img.size - 1], list(rng.choice(img.size, 300, replace=False))):
        f = img.copy()
        f.flat[where] = np.nan
        assert oracle.minmax(f) == (np.nanmin(f), np.nanmax(f)), where
    assert all(np.isnan(oracle.minmax(np.full((5, 7), np.nan, np.float32))))


# ------------------------------------------------------------------------------------------------ dense frames (GPU)
@pytest.fixture(scope="module")
def cache(oracle):
    """name -> (frame, oracle result of frame.astype(float32)), built on first use"""
    store = {}

    def get(name, make):
        if name not in store:
            img = make()
            with np.errstate(over="ignore"):
                store[name] = (img, oracle.keypoints(img.astype(np.float32)))
        return store[name]
    return get


@pytest.mark.gpu
def test_lattice_flush_fused_and_plain(siftlib, cache):
    """1024^2 lattice with 256-row strips: the flush of the fused-refinement form (refine_parked) and of the plain form
    (atomicAdd + candidate list, then the refinement launch), and the default strips, all equal to the oracle."""
    import sift_pyocl_amd as sp
    img, want = cache("lattice1024", lambda: lattice((1024, 1024), seed=23))
    assert len(want) > 20000
    for opts in ({}, {"ext_rows": LATTICE_ROWS}, {"ext_rows": LATTICE_ROWS, "fused_refine": 0}, {"ext_rows": LATTICE_ROWS, "tail": 0, "overlap": 0}):
        plan = sp.SiftPlan(template=img)
        for k, v in opts.items():
            plan.set_option(k, v)
        for call in range(2):
            assert_same_keypoints(plan.keypoints(img), want, "lattice 1024^2 %r call %d" % (opts, call))


@pytest.mark.gpu
def test_dense_group(siftlib, oracle, cache):
    """2048^2 lattice: more than 65 536 oriented keypoints in group 0 (the dense descriptor launch), about two orientations
    per keypoint; within capacity bit-exact in every refinement form, beyond it (PIX_PER_KP 60) the overflow / subset rule
    of test_gpu_capacity.py."""
    import sift_pyocl_amd as sp
    from collections import Counter
    img, want = cache("lattice2048", lambda: lattice((2048, 2048), seed=29))
    assert len(want) >= 65536
    positions = len(np.unique(np.stack([want["x"], want["y"], want["scale"]], axis=1), axis=0))
    assert len(want) > 1.5 * positions                                # extra orientations
    for opts in ({}, {"ext_rows": LATTICE_ROWS}, {"ext_rows": LATTICE_ROWS, "fused_refine": 2}, {"maps": 1}, {"maps": 0, "desc_team": 0}):
        plan = sp.SiftPlan(template=img)
        for k, v in opts.items():
            plan.set_option(k, v)
        got = plan.keypoints(img)
        assert not plan.overflow
        assert_same_keypoints(got, want, "lattice 2048^2 %r" % (opts,))
    par = oracle.default_params()
    par.pix_per_kp = 60
    capped, ovf = oracle.keypoints(img, par, return_overflow=True)
    assert ovf
    plan = sp.SiftPlan(template=img, PIX_PER_KP=60)
    for call in range(2):
        got = plan.keypoints(img)
        assert plan.overflow
        assert len(capped) <= len(got) <= plan.octave_max * plan.kpsize
        have, full = Counter(r.tobytes() for r in got), Counter(r.tobytes() for r in sort_kp(want))
        assert not (have - full), "a record that the uncapped pipeline does not produce"


# ------------------------------------------------------------------------------------------------ degenerate frames (GPU)
CONSTANTS = [(np.float32, 0.0), (np.float32, 7.0), (np.uint8, 255), (np.uint16, 4321)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(48, 60), TILED, MARCH])
def test_constant_frames(siftlib, oracle, shape):
    """min == max: the normalisation is 0 / 0 and every plane NaN (the reference does not guard either): no keypoints, no
    overflow, min / max equal to the value -- through SiftPlan (twice, after a frame with keypoints) and a two-lane BatchPlan."""
    import sift_pyocl_amd as sp
    rich = smooth_noise(shape, seed=5, sigma=2.0)
    for dtype, value in CONSTANTS:
        frame = np.full(shape, value, dtype)
        assert len(oracle.keypoints(frame.astype(np.float32))) == 0
        plan = sp.SiftPlan(template=frame)
        assert len(plan.keypoints(rich)) > 0
        for call in range(2):
            got = plan.keypoints(frame)
            assert len(got) == 0 and not plan.overflow, (dtype, value, call)
            assert plan.minmax() == (np.float32(value), np.float32(value)), (dtype, value)
        bp = sp.BatchPlan(template=frame, lanes=2)
        out = bp.keypoints_batch([frame, frame, frame])
        assert [len(r) for r in out] == [0, 0, 0] and not bp.overflow, (dtype, value)
        assert len(bp.keypoints_batch([rich])[0]) > 0 and len(bp.keypoints_batch([frame])[0]) == 0


def _u64_near_top(s):
    """values a * 2^40 + 2^39 + d (0 < d < 2^10) just above an f32 rounding tie near 2^64: (float)x rounds up, the double
    rounding (float)(double)x lands on the tie and rounds to even -- they differ wherever a is even; plus 2^64 - 1"""
    q = np.floor(s * 999).astype(np.uint64)
    d = np.random.default_rng(1).integers(1, 1 << 10, s.shape).astype(np.uint64)
    x = ((np.uint64((1 << 24) - 1) - q) << np.uint64(40)) + np.uint64(1 << 39) + d
    x.flat[0] = np.iinfo(np.uint64).max
    return x


def _i64_near_bottom(s):
    """the same below -2^63 + ...: -(m * 2^39 + 2^38 + d), 0 < d < 2^9, m < 2^24 -- plus -2^63 itself"""
    q = np.floor(s * 999).astype(np.int64)
    d = np.random.default_rng(2).integers(1, 1 << 9, s.shape).astype(np.int64)
    x = -((((1 << 24) - 1 - q) << 39) + (1 << 38) + d)
    x.flat[0] = np.iinfo(np.int64).min
    return x


def _u32_near_top(s):
    q = np.floor(s * 999).astype(np.uint32)
    x = np.uint32(0xFFFFFFFF) - q * np.uint32(256) - np.random.default_rng(3).integers(0, 256, s.shape).astype(np.uint32)
    x.flat[0] = 0xFFFFFFFF
    return x


def _f64_ties(s):
    """float64 values exactly halfway between two neighbouring floats: the f64 -> f32 cast rounds them to even"""
    lo = (s * 1000.0 + 3.0).astype(np.float32)
    return (lo.astype(np.float64) + np.nextafter(lo, np.float32(np.inf)).astype(np.float64)) / 2.0


def _f64_beyond(s):
    x = s.astype(np.float64) * 1000.0
    x.flat[::97] = 1e39                                               # beyond FLT_MAX: inf after the cast, so the range is inf
    return x


def _unit(shape, seed):
    s = smooth_noise(shape, seed=seed, sigma=2.0).astype(np.float64)
    return (s - s.min()) / (s.max() - s.min())


EXTREME = {
    "few_ulp": lambda s: (1.0 + np.floor(s * 3.999) * 2.0 ** -23).astype(np.float32),    # four values, 3 ulp apart
    "subnormal": lambda s: (s * 1e-39).astype(np.float32),                                # range below FLT_MIN
    "overflow": lambda s: (s * 2e36).astype(np.float32),                                  # 255 * (x - min) > FLT_MAX
    "negative": lambda s: (-5000.0 - s * 1000.0).astype(np.float32),
    "f64_ties": _f64_ties,
    "f64_beyond": _f64_beyond,
    "u64_top": _u64_near_top,
    "i64_bottom": _i64_near_bottom,
    "u32_top": _u32_near_top,
}


@pytest.mark.gpu
@pytest.mark.filterwarnings("ignore:overflow encountered in cast:RuntimeWarning")
@pytest.mark.parametrize("shape", [TILED, MARCH])
@pytest.mark.parametrize("kind", sorted(EXTREME))
def test_extreme_range_frames(siftlib, oracle, cache, kind, shape):
    """Where reassociating 255 * (v - min) / range, flushing denormals or converting through another type would change bits."""
    import sift_pyocl_amd as sp
    img, want = cache("%s%r" % (kind, shape), lambda: EXTREME[kind](_unit(shape, 11 + len(kind))))
    if img.dtype in (np.uint64, np.int64):
        twice = img.astype(np.float64).astype(np.float32)
        assert (twice != img.astype(np.float32)).sum() > img.size // 4     # the double rounding would be visible
    with np.errstate(over="ignore"):
        ref32 = img.astype(np.float32)
    plan = sp.SiftPlan(template=img)
    for call in range(2):
        got = plan.keypoints(img)
        assert not plan.overflow
        assert_same_keypoints(got, want, "%s %r call %d" % (kind, shape, call))
    mn, mx = plan.minmax()
    emn, emx = oracle.minmax(ref32)
    assert np.float32(mn).tobytes() == emn.tobytes() and np.float32(mx).tobytes() == emx.tobytes(), (kind, mn, mx, emn, emx)
    if kind in ("few_ulp", "subnormal", "negative", "f64_ties", "u64_top", "i64_bottom", "u32_top"):
        assert len(want) > 0, kind                                    # the frames that must keep their keypoints do


# ------------------------------------------------------------------------------------------------ frame sequences (GPU)
def _sequence(shape):
    dense = lattice(shape, seed=29)
    rich = smooth_noise(shape, seed=41)
    sparse = smooth_noise(shape, seed=43, sigma=8.0)
    return [("rich", rich), ("sparse", sparse), ("constant", np.zeros(shape, np.float32)), ("dense", dense),
            ("sparse", sparse), ("constant_u16", np.full(shape, 4000, np.uint16)), ("rich", rich)]


@pytest.mark.gpu
def test_heterogeneous_sequence(siftlib, oracle):
    """rich, sparse, constant, dense, sparse, constant uint16, rich through one uint16 SiftPlan and one two-lane BatchPlan at
    2048^2 with PIX_PER_KP 120: the rich frame needs more records than kpsize (the list grows, no overflow), the lattice
    overflows; every frame follows the oracle (bit-exact, or the overflow / subset rule)."""
    import sift_pyocl_amd as sp
    from collections import Counter
    shape = (2048, 2048)
    seq = _sequence(shape)
    par = oracle.default_params()
    par.pix_per_kp = 120
    want = {}
    for name, img in seq:
        if name not in want:
            want[name] = oracle.keypoints(img.astype(np.float32), par, return_overflow=True)
    full_dense = oracle.keypoints(seq[3][1])
    assert len(want["rich"][0]) > shape[0] * shape[1] // 120 and not want["rich"][1] and want["dense"][1]

    def check(name, got, what):
        exp, eovf = want[name]
        if not eovf:
            assert_same_keypoints(got, exp, "%s: %s" % (what, name))
        else:
            assert len(exp) <= len(got)
            have, full = Counter(r.tobytes() for r in got), Counter(r.tobytes() for r in full_dense)
            assert not (have - full), "%s: %s: a record that the uncapped pipeline does not produce" % (what, name)

    plan = sp.SiftPlan(shape=shape, dtype=np.uint16, PIX_PER_KP=120)
    for name, img in seq:
        got = plan.keypoints(img)
        assert plan.overflow == want[name][1], name
        check(name, got, "SiftPlan")
    assert plan.capacity()[1] >= 1
    bp = sp.BatchPlan(shape=shape, dtype=np.uint16, PIX_PER_KP=120, lanes=2)
    floats = [(n, f) for n, f in seq if f.dtype == np.float32]
    for batch in (floats[:4], [seq[5]], floats[4:]):
        out = bp.keypoints_batch([f for _, f in batch])
        assert bp.overflow == any(want[n][1] for n, _ in batch)
        for (name, _), got in zip(batch, out):
            check(name, got, "BatchPlan")


@pytest.mark.gpu
@pytest.mark.parametrize("shape,ext_rows", [(MARCH, 0), (MARCH, 64), ((1536, 1536), 32), ((400, 520), 0)])
def test_par_at_size(siftlib, oracle, shape, ext_rows):
    """The `par` cases of test_gpu_params.py on a marching frame (marching blur, refinement launch, 16-row strips by default,
    64- and 32-row strips forced) and on a five-octave frame (forked chains, tail kernel)."""
    import sift_pyocl_amd as sp
    from sift_pyocl_amd.param import par
    saved = dict(par)
    img = smooth_noise(shape, seed=shape[1] + ext_rows, sigma=2.0)
    assert oracle.octave_count(*shape) >= 5
    plan = sp.SiftPlan(template=img)
    if ext_rows:
        plan.set_option("ext_rows", ext_rows)
    counts = []
    try:
        for case in PAR_CASES:
            par.update(saved)
            par.update(case)
            want = oracle.default_params()
            want.peak_thresh = np.float32(par.PeakThresh)
            want.edge_thresh0 = np.float32(par.EdgeThresh1)
            want.edge_thresh = np.float32(par.EdgeThresh)
            want.ori_sigma = np.float32(par.OriSigma)
            want.border_dist = int(par.BorderDist)
            got = plan.keypoints(img)
            assert_same_keypoints(got, oracle.keypoints(img, par=want), "%r ext_rows %d par %r" % (shape, ext_rows, case))
            counts.append(len(got))
    finally:
        par.update(saved)
    assert len(set(counts)) >= 5, counts


# ------------------------------------------------------------------------------------------------ min / max with NaN (GPU)
def _nan_frames(shape):
    rng = np.random.default_rng(7)
    base = (rng.random(shape, dtype=np.float32) - 0.25) * 1000
    n = base.size
    out = {}
    for name, where in (("pixel0", [0]), ("last", [n - 1]), ("tail", list(range(n - n % 4, n)) or [n - 1]),
                        ("scattered", list(rng.choice(n, n // 50, replace=False)) + [0])):
        f = base.copy()
        f.flat[where] = np.nan
        out[name] = f
    # the complement of "tail": NaN everywhere but the float4 tail, where the extremes then are -- a kernel that never reads
    # the tail passes "tail" and fails this one
    f = np.full(shape, np.nan, np.float32)
    f.flat[n - (n % 4 or 1):] = base.flat[n - (n % 4 or 1):]
    out["only_tail"] = f
    out["all"] = np.full(shape, np.nan, np.float32)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(131, 97), (512, 512), (37, 53)])
def test_stage_minmax_ignores_nan(siftlib, oracle, shape):
    """siftmi_stage_minmax_normalize: min / max equal np.nanmin / np.nanmax (fmin / fmax, reductions.cl:44), as the oracle's;
    the normalised plane equals the oracle's, NaN where the input is NaN."""
    for name, f in _nan_frames(shape).items():
        out = np.empty_like(f)
        mn, mx = C.c_float(), C.c_float()
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert siftlib.siftmi_stage_minmax_normalize(0, p(f), p(out), shape[1], shape[0], C.byref(mn), C.byref(mx)) == 0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore", RuntimeWarning)
            emn, emx = np.nanmin(f), np.nanmax(f)
        if name == "all":
            assert np.isnan(mn.value) and np.isnan(mx.value)
            continue
        assert (np.float32(mn.value), np.float32(mx.value)) == (emn, emx) == oracle.minmax(f), (shape, name)
        exp = oracle.normalize(f, emn, emx)
        nan = np.isnan(f) | (emn == emx)                              # a single finite pixel: min == max, 0 / 0 there as well
        assert np.array_equal(np.isnan(out), nan) and np.array_equal(out, exp, equal_nan=True), (shape, name)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [TILED, (131, 97)])
def test_plan_minmax_ignores_nan(siftlib, shape):
    """SiftPlan.minmax() of frames with NaN pixels: every fourth row NaN (pixel 0 included, so every plane is NaN after the
    initial blur and no keypoint is formed), a constant frame with NaN at pixel 0 and in the float4 tail, and a frame that is
    finite in the float4 tail alone."""
    import sift_pyocl_amd as sp
    rng = np.random.default_rng(9)
    rows = (rng.random(shape, dtype=np.float32) - 0.5) * 300
    rows[::4] = np.nan
    flat = np.full(shape, 2.5, np.float32)
    flat.flat[0] = flat.flat[-1] = np.nan
    plan = sp.SiftPlan(template=rows)
    for f in (rows, flat, _nan_frames(shape)["only_tail"]):
        plan.keypoints(f)
        assert plan.minmax() == (np.nanmin(f), np.nanmax(f))
