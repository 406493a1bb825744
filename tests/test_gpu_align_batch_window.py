"""GPU tests of LinearAlign.align_batch_window: align_batch with the match stage replaced by
MatchPlan.match_window_batch.  Frames of 256 x 256, grey and RGB: one textured frame, three copies of it moved by integer
numpy.roll's of (+3, -2), (-5, +4) and (0, 0) -- a roll of (dy, dx) moves every keypoint by (dx, dy), so the median displacement
is exactly the roll and the offset, in the kernel's (y, x) order, is the roll tuple itself -- and one constant frame.

Two conditions the stack must meet, or the tests below would compare little: every rolled frame reaches pair_counts >= 18 and
mode 2 without shift_only, and the shift_only offsets are exactly the rolls.  How the texture was chosen: on the CPU, before any
GPU run, oracle.keypoints of the reference and of every rolled frame (for RGB: of 0.299 R + 0.587 G + 0.114 B in float32, the
library's conversion) were matched with window_ref.match(ref, frame, 8.0) and with window_ref.match(ref, frame, 2.0, roll as
(dx, dy)).  smooth_noise((256, 256), seed=12, sigma=1.5) gave 398 reference keypoints and 390 / 372 / 398 pairs (385 / 372 / 398
with the window of 2 around the roll), the RGB stack built from it 416 keypoints and 399 / 396 / 416 pairs (392 / 390 / 416), and
numpy.median of the displacements was exactly (-2, 3), (4, -5) and (0, 0) in every one of those twelve cases.  The tests assert
both conditions, so no branch is skipped silently.
"""
import logging

import numpy as np
import pytest

import align_batch_ref as ab
import match_window_batch_ref as wb
from util import smooth_noise
from warp_ref import same

pytestmark = pytest.mark.gpu
F = np.float32
INF = float("inf")
ROLLS = [(3, -2), (-5, 4), (0, 0)]
MAX_SHIFT = 8.0
_cache = {}


def stack(kind):
    """(reference, [three rolled frames, one constant frame])"""
    if ("stack", kind) not in _cache:
        tex = smooth_noise((256, 256), seed=12, sigma=1.5)
        if kind == "rgb":
            q = (255 * (tex - tex.min()) / (tex.max() - tex.min())).astype(np.uint8)
            tex = np.ascontiguousarray(np.stack([q, q[::-1, ::-1], q.T], axis=-1))
            flat = np.full_like(tex, 77)
        else:
            flat = np.full_like(tex, tex.mean())
        _cache[("stack", kind)] = (tex, [np.ascontiguousarray(np.roll(tex, r, axis=(0, 1))) for r in ROLLS] + [flat])
    return _cache[("stack", kind)]


def aligner(kind):
    import sift_pyocl_amd as sp
    if ("la", kind) not in _cache:
        _cache[("la", kind)] = sp.LinearAlign(stack(kind)[0])
    return _cache[("la", kind)]


def full_result(kind):
    """align_batch_window(max_shift=8, return_all=True) of the stack, computed once"""
    if ("full", kind) not in _cache:
        _cache[("full", kind)] = aligner(kind).align_batch_window(stack(kind)[1], MAX_SHIFT, return_all=True)
    return _cache[("full", kind)]


def lists_of(la, res):
    return la.ref_kp, None, np.concatenate(res["keypoint"]), res["counts"]


def resolved(res):
    """per frame the pairs as (i, the record of j): what the pairs say whatever order a frame's list came out in"""
    at = np.concatenate([[0], np.cumsum(res["pair_counts"])])
    return [[(int(i), kp[j].tobytes()) for i, j in res["pairs"][at[s]:at[s + 1]]] for s, kp in enumerate(res["keypoint"])]


def same_dict(got, want):
    """Bit equality of two return_all dicts.  The order of a frame's keypoint list is not fixed from one detection to the next
    (the lists are compacted with atomics), and `pairs` indexes that list: the lists are compared as sorted records and the pairs
    through the records they name.  The pairs of a frame ascend in i, the index into the fixed reference list, so everything
    computed from them -- every other key -- is compared bit for bit."""
    assert sorted(got) == sorted(want)
    for key in want:
        if key == "keypoint":
            assert len(got[key]) == len(want[key])
            for a, b in zip(got[key], want[key]):
                assert sorted(r.tobytes() for r in a) == sorted(r.tobytes() for r in b)
        elif key == "pairs":
            assert got[key].dtype == want[key].dtype and resolved(got) == resolved(want)
        else:
            assert same(got[key], want[key]), key


@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_stages_equal_the_restatement_and_the_batch_calls(siftlib, kind):
    la, (ref, frames), res = aligner(kind), stack(kind), full_result(kind)
    S = len(frames)
    pc = res["pair_counts"]
    # the two conditions of the module docstring (the second is asserted in the shift_only test)
    assert (pc[:3] >= 18).all() and res["mode"].tolist() == [2, 2, 2, 0]
    assert res["counts"][3] == 0 and pc[3] == 0 and pc.sum() == len(res["pairs"])
    # the pairs are the restatement's on the returned lists
    want = wb.match_window_batch(*lists_of(la, res), MAX_SHIFT)
    assert res["pairs"].dtype == np.int32 and np.array_equal(res["pairs"], want[0]) and np.array_equal(pc, want[1])
    # the estimates are align_batch's rule on fit_batch / shift_batch of those pairs
    lists = lists_of(la, res) + (res["pairs"], pc)
    models, rms, n_fit = la.match.fit_batch(*lists)
    moved, n_moved = la.match.shift_batch(*lists)
    mode, matrix, offset = ab.align_batch_ref(pc, models, n_fit, moved, n_moved)
    assert res["mode"].dtype == np.int8 and res["mode"].tolist() == mode.tolist()
    assert same(res["matrix"], matrix) and same(res["offset"], offset)
    for s in range(3):
        assert res["n"][s] == n_fit[s] and res["rms"][s] == rms[s]
        # a sanity bound, not a measurement: a wrong pair is off by at most max_shift plus the roll, 13 px, and one of them among
        # 370 pairs spread over +-70 px moves a coefficient by 13 / (370 * 70) = 5e-4 and the offset by 13 / 370 + 128 * 5e-4 = 0.1
        # at most; fewer than 30 pairs are off the roll by more than half a pixel (counted here)
        rows = res["pairs"][pc[:s].sum():pc[:s + 1].sum()]
        kp = res["keypoint"][s]
        off = ((np.abs(kp["x"][rows[:, 1]] - la.ref_kp["x"][rows[:, 0]] - ROLLS[s][1]) > 0.5) |
               (np.abs(kp["y"][rows[:, 1]] - la.ref_kp["y"][rows[:, 0]] - ROLLS[s][0]) > 0.5))
        assert off.sum() < 30, (s, int(off.sum()))
        assert np.allclose(res["matrix"][s], np.identity(2), atol=0.015) and np.allclose(res["offset"][s], ROLLS[s], atol=3.0)
    assert res["n"][3] == 0 and np.isnan(res["rms"][3])
    # the planes are transform_batch's for those maps
    assert res["result"].shape == (S,) + la.outshape + ((3,) if kind == "rgb" else ())
    assert same(res["result"], la._batch.transform_batch(frames, res["matrix"], res["offset"], res["fill"], out_shape=la.outshape, mode=1))
    assert same(aligner(kind).align_batch_window(frames, MAX_SHIFT), res["result"])


@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_shift_only_offsets_are_the_rolls_and_those_of_align(siftlib, kind):
    la, (ref, frames) = aligner(kind), stack(kind)
    res = la.align_batch_window(frames, MAX_SHIFT, shift_only=True, return_all=True)
    assert res["mode"].tolist() == [1, 1, 1, 0]
    for s, roll in enumerate(ROLLS):
        assert res["offset"][s].tolist() == [float(roll[0]), float(roll[1])], s
        one = la.align(frames[s], shift_only=True, max_shift=MAX_SHIFT, median="device", return_all=True)
        assert same(res["offset"][s], np.asarray(one["offset"], F)), s
    want = wb.match_window_batch(*lists_of(la, res), MAX_SHIFT)
    assert np.array_equal(res["pairs"], want[0]) and np.array_equal(res["pair_counts"], want[1])
    # a window of 2 around the true displacement of every frame, in (x, y) order: the same offsets
    expected = np.array([(dx, dy) for dy, dx in ROLLS] + [(0, 0)], F)
    near = la.align_batch_window(frames, 2.0, expected_shift=expected, shift_only=True, return_all=True)
    assert same(near["offset"], res["offset"]) and near["mode"].tolist() == [1, 1, 1, 0] and (near["pair_counts"][:3] >= 18).all()
    want = wb.match_window_batch(*lists_of(la, near), 2.0, expected)
    assert np.array_equal(near["pairs"], want[0]) and np.array_equal(near["pair_counts"], want[1])
    affine = la.align_batch_window(frames, 2.0, expected_shift=expected, return_all=True)
    assert affine["mode"].tolist() == [2, 2, 2, 0] and resolved(affine) == resolved(near)
    # the window of 2 around no displacement misses the partners of the first two frames: few or wrong matches, not an error
    missed = la.align_batch_window(frames, 2.0, shift_only=True, return_all=True)
    assert (missed["pair_counts"][:2] < near["pair_counts"][:2]).all() and missed["pair_counts"][2] == near["pair_counts"][2]
    one_for_all = la.align_batch_window(frames[:1], 2.0, expected_shift=(-2.0, 3.0), shift_only=True, return_all=True)
    assert same(one_for_all["offset"][0], res["offset"][0])


@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_infinite_window_is_align_batch(siftlib, kind):
    la, (ref, frames) = aligner(kind), stack(kind)
    same_dict(la.align_batch_window(frames, INF, return_all=True), la.align_batch(frames, return_all=True))
    same_dict(la.align_batch_window(frames, INF, shift_only=True, robust=True, return_all=True),
              la.align_batch(frames, shift_only=True, robust=True, return_all=True))


@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_the_constant_frame_is_its_fill_value_with_a_warning(siftlib, kind, caplog):
    la, (ref, frames) = aligner(kind), stack(kind)
    with caplog.at_level(logging.WARNING):
        res = la.align_batch_window(frames, MAX_SHIFT, return_all=True, out="device")
    assert any("frame 3" in r.getMessage() for r in caplog.records)
    assert res["mode"][3] == 0 and np.isnan(res["matrix"][3]).all() and np.isnan(res["offset"][3]).all()
    plane = res["result"][3].cpu().numpy()
    assert res["fill"][3] == frames[3].min() and same(plane, np.full(plane.shape, res["fill"][3]).astype(plane.dtype))
    assert same(res["result"].cpu().numpy(), full_result(kind)["result"])
    with pytest.raises(ValueError):
        la.align_batch_window(frames, None)
    with pytest.raises(ValueError):
        la.align_batch_window(frames, -1.0)
    with pytest.raises(ValueError):
        la.align_batch_window(frames, MAX_SHIFT, expected_shift=np.zeros((3, 2)))
