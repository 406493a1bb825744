"""The min / max reduction at the head of every frame (k_pyramid.hpp minmax_kernel, minmax_typed_kernel<DT>) on frames whose
two extremes are PLANTED at the edges of every loop of the kernels (tests/minmax_cases.py): a seeded band frame, the minimum on
P[k] and the maximum on P[len(P)-1-k], one frame per position, for every launch shape of the options "mm_threads" /
"mm_blocks", every frame type, through SiftPlan.keypoints + SiftPlan.minmax(), siftmi_stage_minmax_normalize and
BatchPlan.minmax_batch().  Expected: oracle.minmax of the frame converted as test_gpu_typed_input.as_f32 converts it (pinned to
the reference's converters by test_converters_identical), compared by bytes.

tests/test_minmax_cases_host.py proves on the CPU that a kernel which drops the tail, the strided loop, an unrolled slot, a
pixel of every chunk, a wave, a workgroup, the last chunk or an end pixel fails here.  Every failure message names the frame
type, the shape, the launch shape, the family and, for both planted pixels, the loop, slot, pixel in its chunk, wave and
workgroup that read it."""
import ctypes as C
from collections import Counter

import numpy as np
import pytest

import minmax_cases as mc
from test_gpu_typed_input import as_f32

pytestmark = pytest.mark.gpu

NORMALIZE_EVERY = 16            # test_stage_hook_planted compares the normalised plane of every 16th frame


def sid(shape):
    return "%dx%d" % shape


def same(got, want):
    return np.float32(got).tobytes() == np.float32(want).tobytes()


def one(pixel):
    """float32 of one planted pixel, as as_f32 converts it"""
    return as_f32(pixel.reshape((1, 1) + pixel.shape[1:])).reshape(-1)


def make_plan(dtype, shape, launch):
    """a SiftPlan of the frame type with the launch shape set; None: no option set (the defaults)"""
    import sift_pyocl_amd as sp
    plan = sp.SiftPlan(shape=shape + ((3,) if dtype == "rgb8" else ()), dtype=mc.np_dtype(dtype))
    if launch is not None:
        threads, blocks = launch
        if dtype == "float32":
            plan.set_option("mm_threads", threads)
        else:
            assert threads == mc.TYPED_THREADS
        plan.set_option("mm_blocks", blocks)

    def run(frame):
        plan.keypoints(frame)
        return plan.minmax()
    return run


def check_family(run, oracle, dtype, shape, launch, family, P, lab, each=None):
    """Every frame of the family through `run` (frame -> (min, max)); one assertion for the family, which counts the wrong
    frames, says which loops read their planted pixels and spells the first one out.  each(k, frame, min, max): more checks."""
    n = shape[0] * shape[1]
    flat = mc.band(dtype, family, n)
    frame = flat.reshape(shape + flat.shape[1:])
    lo, hi = mc.planted(dtype, family)
    conv = frame if dtype == "float32" else as_f32(frame)             # as_f32 is per pixel: kept current at the planted two
    also = None if dtype == "float32" else (conv.reshape(-1), one(lo), one(hi))
    todo = mc.pairs(P)
    wrong, loops = [], Counter()
    for k, pmin, pmax in mc.frames(flat, todo, lo, hi, also):
        got = run(frame)
        want = oracle.minmax(conv)
        if not (same(got[0], want[0]) and same(got[1], want[1])):
            wrong.append((k, pmin, pmax, got, want))
            loops.update(mc.LOOP_NAMES[lab.loop[p]] for p, g, w in ((pmin, got[0], want[0]), (pmax, got[1], want[1])) if not same(g, w))
        elif each is not None:
            each(k, frame, *want)
    if wrong:
        k, pmin, pmax, got, want = wrong[0]
        raise AssertionError("%s %s, %d threads x at most %d workgroups, family %s: %d of %d frames wrong (missed extremes by loop: %s); "
                             "first: frame %d gives %r, expected %r; minimum on pixel %d (%s), maximum on pixel %d (%s)" % (
                                 dtype, sid(shape), launch[0], launch[1], family, len(wrong), len(todo), dict(loops), k, got,
                                 (float(want[0]), float(want[1])), pmin, mc.describe(lab[pmin]), pmax, mc.describe(lab[pmax])))
    assert len(todo) >= len(P) - 1
    return len(todo)


def planting(dtype, shape, launch):
    n = shape[0] * shape[1]
    lab = mc.labels(n, dtype, *launch)
    return mc.positions(n, dtype, *launch, lab=lab), lab


@pytest.mark.parametrize("shape", mc.SHAPES, ids=sid)
@pytest.mark.parametrize("dtype", ("float32",) + mc.TYPED)
def test_planted_extremes(siftlib, oracle, dtype, shape):
    """All families of the frame type at every launch shape of the plan: (mm_threads, mm_blocks) (256, 1), (256, 3), (512, 2),
    (1024, 1) and the defaults for f32; mm_blocks 1, 3 and the default for a typed frame (always 256 threads)."""
    frames = 0
    for launch in mc.launches(dtype):
        run = make_plan(dtype, shape, launch)
        P, lab = planting(dtype, shape, launch)
        for family in mc.families(dtype):
            frames += check_family(run, oracle, dtype, shape, launch, family, P, lab)
    print("%s %s: %d frames" % (dtype, sid(shape), frames))


@pytest.mark.parametrize("shape", mc.SHAPES, ids=sid)
def test_lone_finite_pixel(siftlib, shape):
    """Every pixel NaN but one: the workgroup whose only finite value is the planted one must publish it (the all-NaN
    partials of the others are skipped), whichever lane, wave and loop reads it."""
    n = shape[0] * shape[1]
    for launch in mc.F32_LAUNCHES:
        run = make_plan("float32", shape, launch)
        P, lab = planting("float32", shape, launch)
        flat = np.full(n, np.nan, np.float32)
        wrong = []
        for k, p, v in mc.lone_frames(flat, P):
            got = run(flat.reshape(shape))
            if not (same(got[0], v) and same(got[1], v)):
                wrong.append((k, p, v, got))
        if wrong:
            k, p, v, got = wrong[0]
            raise AssertionError("float32 %s, %d threads x at most %d workgroups, family lone: %d of %d frames wrong (by loop: %s); first: "
                                 "frame %d gives %r, expected %r twice; the finite pixel is %d (%s)" % (
                                     sid(shape), launch[0], launch[1], len(wrong), len(P),
                                     dict(Counter(mc.LOOP_NAMES[lab.loop[w[1]]] for w in wrong)), k, got, float(v), p, mc.describe(lab[p])))


@pytest.mark.parametrize("dtype", mc.BIG_DTYPES)
def test_defaults_at_3_megapixels(siftlib, oracle, dtype):
    """1773 x 1777 with no option set: the default launch shape itself -- 256 workgroups, and the unrolled loop on 4 892 (f32),
    1 220 (u8, RGB8), 262 144 (u16) and 786 432 (i64) chunks (test_every_configuration_reaches_its_loops)."""
    launch = mc.launches(dtype)[-1]
    run = make_plan(dtype, mc.BIG, None)
    P, lab = planting(dtype, mc.BIG, launch)
    family = "pos" if dtype == "float32" else dtype
    print("%s: %d frames" % (dtype, check_family(run, oracle, dtype, mc.BIG, launch, family, P, lab)))


@pytest.mark.parametrize("shape", mc.SHAPES, ids=sid)
def test_stage_hook_planted(siftlib, oracle, shape):
    """siftmi_stage_minmax_normalize (256 threads, up to 2048 workgroups), family `pos`; the normalised plane of every 16th
    frame equals oracle.normalize."""
    P, lab = planting("float32", shape, mc.STAGE_LAUNCH)
    out = np.empty(shape, np.float32)
    mn, mx = C.c_float(), C.c_float()
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def run(frame):
        out.fill(-1)
        assert siftlib.siftmi_stage_minmax_normalize(0, p(frame), p(out), shape[1], shape[0], C.byref(mn), C.byref(mx)) == 0
        return mn.value, mx.value

    def normalised(k, frame, emn, emx):
        if k % NORMALIZE_EVERY == 0:
            assert np.array_equal(out, oracle.normalize(frame, emn, emx)), "float32 %s, stage hook, family pos, frame %d: normalised plane" % (sid(shape), k)
    check_family(run, oracle, "float32", shape, mc.STAGE_LAUNCH, "pos", P, lab, each=normalised)


def test_batch_lanes_keep_their_own_extremes(siftlib, oracle):
    """Seven frames per call through a BatchPlan of 1, 2 and 3 lanes, u16 and f32: frame i has its own planted pair of values
    on its own pair of positions; minmax_batch() returns them in input order, also when the same plan gets the frames again
    in reverse order."""
    import sift_pyocl_amd as sp
    shape = (97, 131)
    n = shape[0] * shape[1]
    for dtype, family in (("float32", "pos"), ("uint16", "uint16")):
        launch = mc.launches(dtype)[-1]
        P, lab = planting(dtype, shape, launch)
        todo = mc.pairs(P)
        picks = [todo[i] for i in np.linspace(0, len(todo) - 1, 7).astype(int)]
        frames, want, where = [], [], []
        for i, (k, pmin, pmax) in enumerate(picks):
            flat = mc.band(dtype, family, n, seed=mc.SEED + i)
            lo, hi = mc.planted(dtype, family)
            flat[pmin], flat[pmax] = lo[0] + i, hi[0] - i              # inside the type, outside the band, different per frame
            frames.append(flat.reshape(shape))
            want.append(oracle.minmax(as_f32(frames[-1])))
            where.append("minimum on pixel %d (%s), maximum on pixel %d (%s)" % (pmin, mc.describe(lab[pmin]), pmax, mc.describe(lab[pmax])))
            assert want[-1] == (one(lo + i)[0], one(hi - i)[0])
        assert len(set(want)) == len({w[0] for w in want}) == len({w[1] for w in want}) == 7    # an index mix-up cannot hide
        for lanes in (1, 2, 3):
            bp = sp.BatchPlan(shape=shape, dtype=mc.np_dtype(dtype), lanes=lanes)
            for order in (list(range(7)), list(range(6, -1, -1))):
                bp.keypoints_batch([frames[i] for i in order])
                mins, maxs = bp.minmax_batch()
                assert mins.shape == maxs.shape == (7,)
                for slot, i in enumerate(order):
                    assert same(mins[slot], want[i][0]) and same(maxs[slot], want[i][1]), \
                        "%s %s, %d lanes, order %r, slot %d = frame %d: got %r, expected %r; %s" % (
                            dtype, sid(shape), lanes, order, slot, i, (float(mins[slot]), float(maxs[slot])),
                            (float(want[i][0]), float(want[i][1])), where[i])
