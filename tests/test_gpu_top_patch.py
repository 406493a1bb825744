"""The lazy detection chain -- extrema without plane 5, top_patch_kernel, refinement -- as a stage on crafted planes and at plan
level, against the CPU oracle bit for bit.

siftmi_stage_detect_lazy takes planes 0..4 and the top plane's taps, fills plane 5 with a NaN pattern and launches what a plan
launches under option "lazy_top".  Expected values come only from the oracle (tests/top_patch_cases.py): its blur of plane 4
gives plane 5, oracle.local_maxmin / oracle.interp_keypoint on the six planes give the lists; the provisional scale-3
candidates are local_maxmin's under the 18-neighbour test.  Rows are sorted and compared as uint32.  Every sample of plane 5
inside a provisional candidate's 13 x 13 patch must hold the oracle's bits and every other sample the fill; a refinement read
outside a patch would meet the NaN fill, turn a peak into NaN and show as a missing refined row, so the equality of the
refined rows is the check that the patch is large enough.  (A NaN sample of plane 5 -- the blur of a NaN in plane 4 -- is
compared as NaN and as different from the fill: IEEE 754 leaves the payload of an arithmetic NaN to the platform.)"""
import ctypes as C

import numpy as np
import pytest

import top_patch_cases as tp
from util import smooth_noise, sort_rows_bits, oracle_pyramid
from test_gpu_detection_forms import GUARD, same_rows, _p
from test_gpu_detection_forms import params as _params

gpu = pytest.mark.gpu
FILL_KP = 0xa5a5a5a5

# (case, (H, W), border, strip rows): planes just above the tail kernel's 64 x 64; W - 2 * border = 62 k - 1, 62 k, 62 k + 1
CASES = [("planted", (72, 71), 5, 4), ("planted", (80, 72), 5, 64), ("planted", (72, 73), 5, 4), ("planted", (135, 133), 5, 64),
         ("planted", (67, 134), 5, 4), ("planted", (141, 135), 5, 64), ("planted", (70, 63), 1, 4), ("planted", (72, 64), 1, 64),
         ("planted", (69, 65), 1, 64), ("planted", (66, 126), 1, 4),
         ("nonfinite", (135, 141), 5, 64), ("nonfinite", (135, 127), 1, 4),
         ("none", (72, 80), 5, 4), ("rejected", (72, 80), 5, 64), ("rejected", (67, 66), 1, 4),
         ("dense", (72, 80), 5, 4), ("dense", (68, 127), 1, 64)]


def params(oracle, border):
    return _params(oracle, border=border)


def detect_lazy(siftlib, blurs5, taps, lpar, rows, xcd=1):
    blurs5 = np.ascontiguousarray(blurs5, np.float32)
    taps = np.ascontiguousarray(taps, np.float32)
    _, H, W = blurs5.shape
    cap = 3 * (H - 2 * lpar.border_dist) * (W - 2 * lpar.border_dist)
    cand = np.zeros((cap + GUARD, 4), np.float32); kp = np.zeros((cap + GUARD, 4), np.float32)
    aux = np.zeros(cap + GUARD, np.int32); counters = np.full(5, -7, np.int32); p5 = np.zeros((H, W), np.float32)
    rc = siftlib.siftmi_stage_detect_lazy(0, _p(blurs5), _p(taps), len(taps), W, H, 1, C.byref(lpar), rows, xcd, -1, -1, cap, cap,
                                          _p(cand), _p(kp), _p(aux), _p(counters), _p(p5))
    assert rc == 0, "siftmi_stage_detect_lazy returned %d" % rc
    return cand, kp, aux, [int(v) for v in counters], p5, cap


@gpu
@pytest.mark.parametrize("name,shape,border,rows", CASES)
def test_lazy_chain_on_crafted_planes(siftlib, oracle, name, shape, border, rows):
    opar, lpar = params(oracle, border)
    case = tp.build(oracle, name, shape, border)
    e = tp.expect(oracle, case, opar, key=(name, shape, border))
    tp.assert_named(case, e)
    what = "%s %dx%d border %d rows %d" % (name, shape[0], shape[1], border, rows)
    cand, kp, aux, counters, p5, cap = detect_lazy(siftlib, case.blurs5, tp.top_taps(oracle), lpar, rows, xcd=rows == 4)
    n_listed = len(e.cand) - len(e.kept3) + len(e.prov3)
    print(what, "listed", counters[0], "provisional", len(e.prov3), "kept", len(e.kept3), "refined", counters[1])
    assert counters[0] == n_listed, "%s: %d list entries, expected %d" % (what, counters[0], n_listed)
    listed = cand[:n_listed]
    holes = (listed == -1.0).all(axis=1)
    assert int(holes.sum()) == len(e.prov3) - len(e.kept3), "%s: %d holes, expected %d" % (what, holes.sum(), len(e.prov3) - len(e.kept3))
    same_rows(listed[~holes], e.cand, what + " candidates")
    assert (cand[n_listed:] == -1.0).all(), what + ": candidate slots beyond the list were written"
    assert counters[2:5] == e.counts, "%s: c_scale %r, expected %r" % (what, counters[2:5], e.counts)
    assert counters[1] == len(e.refined), "%s: g_kp %d, expected %d" % (what, counters[1], len(e.refined))
    m = counters[1]
    same_rows(np.concatenate([kp[:m], (aux[:m] & 0xff).astype(np.float32)[:, None]], axis=1), e.refined, what + " refined")
    assert (kp[m:].view(np.uint32) == FILL_KP).all() and (aux[m:].view(np.uint32) == FILL_KP).all()
    # plane 5: the oracle's bits inside the patches, the fill outside
    mask = tp.patch_mask(e.prov3, *shape)
    got, want = p5.view(np.uint32), e.blurs[5].view(np.uint32)
    assert (got[~mask] == tp.FILL).all(), "%s: %d samples outside every patch were written" % (what, (got[~mask] != tp.FILL).sum())
    nan = np.isnan(e.blurs[5])
    bad = mask & ~nan & (got != want)
    assert not bad.any(), "%s: %d patch samples differ from the oracle's plane 5, first at %r" % (what, bad.sum(), np.argwhere(bad)[0].tolist())
    assert (np.isnan(p5) & (got != tp.FILL))[mask & nan].all(), what + ": a NaN sample of plane 5 inside a patch was not written"


@gpu
def test_refused_arguments(siftlib, oracle):
    opar, lpar = params(oracle, 5)
    case = tp.build(oracle, "none", (72, 80), 5)
    b5 = np.ascontiguousarray(case.blurs5); taps = tp.top_taps(oracle)
    z = np.zeros((64, 4), np.float32); zi = np.zeros(64, np.int32); p5 = np.zeros((72, 80), np.float32)

    def call(ntaps=27, rows=0, par=lpar, band=(-1, -1)):
        return siftlib.siftmi_stage_detect_lazy(0, _p(b5), _p(taps), ntaps, 80, 72, 1, C.byref(par), rows, 0, band[0], band[1], 0, 0,
                                                _p(z), _p(z), _p(zi), _p(zi), _p(p5))
    assert call(ntaps=0) == -1 and call(ntaps=65) == -1 and call(rows=-1) == -1 and call(band=(4, 20)) == -1
    assert call(par=params(oracle, 0)[1]) == -1
    assert call() == 0


# ------------------------------------------------------------------------------------------------------------ plan level
def _records(k):
    b = np.ascontiguousarray(k).view(np.uint8).reshape(len(k), -1)
    return b[np.lexsort(b.T[::-1])]


def _frames(shape):
    sparse = np.random.default_rng(11).random(shape, dtype=np.float32)      # white noise: one scale-3 candidate per ~8 000 pixels
    return sparse, smooth_noise(shape)                                       # smoothed noise: one per ~500


@gpu
@pytest.mark.parametrize("shape", [(300, 421), (512, 512)])
def test_plan_records_and_planes_do_not_depend_on_lazy_top(oracle, shape):
    """lazy_top 0 / 1 / 2 (the two-launch detection on every octave, so that these small frames keep candidate lists): the same
    records as sorted bytes on both calls; after a lazy run planes(0) are the oracle's, plane 5 included."""
    import sift_pyocl_amd as sp
    sparse, rich = _frames(shape)
    for img in (sparse, rich):
        want = None
        for mode in (0, 1, 2):
            plan = sp.SiftPlan(template=img, devicetype="GPU")
            plan.set_option("fused_refine", 0)
            plan.set_option("lazy_top", mode)
            for call in range(2):
                got = _records(plan.keypoints(img))
                want = got if want is None else want
                assert got.shape == want.shape and np.array_equal(got, want), "lazy_top %d, call %d: records differ" % (mode, call)
            lazy = plan.lazy_octaves()
            if mode == 0:
                assert not any(lazy)
            if mode == 1:
                first = plan.last_counts()["tail_first"]
                assert lazy[0] and all(lazy[:first]) and not any(lazy[first:])
                blurs = oracle_pyramid(oracle, img, 1)[0][0]
                assert np.array_equal(plan.planes(0).view(np.uint32), blurs.view(np.uint32)), "planes(0) after a lazy run differ from the oracle's"
                assert np.array_equal(plan.planes(0).view(np.uint32), blurs.view(np.uint32))      # ... and stay whole on a second read


@gpu
def test_auto_rule_follows_the_previous_image(oracle):
    """lazy_top 2: a plan's first call is eager; after a sparse frame octave 0 runs lazy, after a rich one eager again, and back --
    with the records of each frame unchanged throughout."""
    import sift_pyocl_amd as sp
    shape = (512, 512)
    sparse, rich = _frames(shape)
    ref = sp.SiftPlan(template=sparse, devicetype="GPU")
    ref.set_option("lazy_top", 0)
    want = {"sparse": _records(ref.keypoints(sparse)), "rich": _records(ref.keypoints(rich))}
    plan = sp.SiftPlan(template=sparse, devicetype="GPU")
    plan.set_option("fused_refine", 0)
    seen = []
    for name in ("sparse", "sparse", "rich", "rich", "sparse", "sparse"):
        got = _records(plan.keypoints(sparse if name == "sparse" else rich))
        assert np.array_equal(got, want[name]), "records of the %s frame differ (call %d)" % (name, len(seen))
        seen.append(plan.lazy_octaves()[0])
        c3 = int(plan.last_counts()["c_scale"][0][2])
        assert (c3 * 6000 < 512 * 512) == (name == "sparse"), "the %s frame has %d scale-3 candidates" % (name, c3)
    assert seen == [False, True, True, False, False, True], seen


@gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_lazy_top_against_the_oracle_on_a_marching_frame(oracle, mode):
    """The lazy setting swept like a plan option (tests/test_gpu_options.py): a frame whose octave 0 takes the marching blur and
    the two-launch detection under the default options, two calls on one plan (the second is lazy under the automatic rule too:
    a threshold of one pixel per candidate), both equal to the oracle's keypoints."""
    import sift_pyocl_amd as sp
    from util import assert_same_keypoints
    img = smooth_noise((1280, 1536), seed=19, sigma=3.0)
    want = oracle.keypoints(img)
    plan = sp.SiftPlan(template=img, devicetype="GPU")
    plan.set_option("lazy_top", mode)
    plan.set_option("lazy_density", 1)
    for call in range(2):
        assert_same_keypoints(plan.keypoints(img), want, "lazy_top %d, call %d" % (mode, call))
        assert plan.lazy_octaves()[0] == (mode == 1 or call == 1)
