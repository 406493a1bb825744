"""What tests/test_gpu_handoff.py rests on, checked without a GPU: the oracle's shrink is plain every-second-sample slicing on
every shape used there, the blur schedule puts the tap counts the plan test claims on the launch that writes plane 3, and the
workgroup counts of its team-form cases give the segment heights they are chosen for."""
import math

import numpy as np
import pytest

from test_gpu_handoff import NTAPS, PLAN_SIGMAS, SHRINK_SHAPES, TEAM_CASES, all_shapes, team_rows_out
from util import white_noise


@pytest.mark.parametrize("shape", all_shapes())
def test_oracle_shrink_is_every_second_sample(oracle, shape):
    H, W = shape
    x = white_noise(shape, seed=H * 3 + W) * 255
    got = oracle.shrink(x)
    assert got.shape == (H // 2, W // 2)
    assert np.array_equal(got.view(np.uint32), x[:2 * (H // 2):2, :2 * (W // 2):2].view(np.uint32))


def test_plane3_tap_counts():
    """The per-octave blur schedule (plan.py:602-618; compute_schedule in siftmi.hip restates it) by utils.kernel_size: the
    launch with s == 2 writes plane 3 and carries the hand-off.  If the rule moves, the plan test no longer reaches the
    instances it is there for, and this test says so."""
    from sift_pyocl_amd.utils import kernel_size
    want = {1.0: [9, 9, 11, 15, 17], 1.3: [9, 13, 15, 17, 23], 1.6: [11, 15, 17, 21, 27], 2.0: [15, 17, 21, 27, 33],
            2.5: [17, 21, 27, 33, 41]}
    assert sorted(want) == PLAN_SIGMAS
    ratio = 2.0 ** (1.0 / 3.0)
    for init_sigma, sizes in want.items():
        prev, got = init_sigma, []
        for _ in range(5):
            got.append(kernel_size(prev * math.sqrt(ratio ** 2 - 1.0), True))
            prev *= ratio
        assert got == sizes, init_sigma
    assert [want[s][2] for s in PLAN_SIGMAS] == NTAPS


def test_team_cases_cover_both_parities():
    """every tap count meets an odd and an even segment height under either workgroup order, as the cases state"""
    for ntaps in NTAPS:
        seen = set()
        for (H, W), cases in TEAM_CASES.items():
            assert W >= 1024 and H >= 512 and W * H >= 1400 * 1400, "not a plane of the team form"
            for xcd_map, wgs, odd in cases:
                assert team_rows_out(W, H, ntaps, wgs) % 2 == odd, ((H, W), ntaps, wgs)
                seen.add((xcd_map, odd))
        assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}, (ntaps, seen)


def test_shrink_shapes_cover_every_path():
    """shrink_kernel (k_pyramid.hpp): a thread moves four outputs from x = 4 * thread on; vec_in = LW even and x + 3 < SW,
    vec_out = SW a multiple of 4, else the scalar loop over min(4, SW - x) outputs; 256 outputs and 8 rows per workgroup"""
    paths, tails = set(), set()
    for H, W in SHRINK_SHAPES:
        SW = W // 2
        for x in range(0, SW, 4):
            vec_in = W % 2 == 0 and x + 3 < SW
            paths.add((vec_in, vec_in and SW % 4 == 0))
            if not vec_in:
                tails.add((W % 2, min(4, SW - x)))
    assert paths == {(True, True), (True, False), (False, False)}
    # the scalar loop moves 1, 2, 3 and 4 outputs: the last thread of an even pitch 1 to 3, every thread of an odd pitch up to 4
    assert tails >= {(0, 1), (0, 2), (0, 3), (1, 1), (1, 4)}, tails
    assert {(W // 2) % 4 for _, W in SHRINK_SHAPES} == {0, 1, 2, 3}
    assert {3, 5} <= {(W // 2 + 255) // 256 for _, W in SHRINK_SHAPES}                       # workgroups in x
    assert any((H // 2) % 2 == 1 and H // 2 > 8 for H, _ in SHRINK_SHAPES)                   # SH odd, more than one workgroup in y
