"""The per-keypoint kernels on crafted gradient planes (tests/keypoint_cases.py), every form as a stage, bit for bit against the
CPU oracle.

tests/test_gpu_keypoint_forms.py reaches every form of orientation_kernel and of the descriptor kernels, but on noise planes,
where no gradient orientation lies on a histogram bin edge, no two peaks tie, no histogram is empty or infinite, the
descriptor's orientation never wraps at exactly 2 pi and no byte saturates.  The planes here are made of those cases
(tests/test_keypoint_cases_host.py asserts that each is reached; tests/test_oracle_vs_ref.py pins the oracle to the
reference's kernels on the same inputs).  The keypoints are finite, their sigmas positive and their windows small: nothing
here can keep a loop of a kernel from ending.  All comparisons are exact."""
import numpy as np
import pytest

import keypoint_cases as kc
from test_gpu_keypoint_forms import (BLOCKS, DESC_FORMS, ORI_FORMS, _check_descriptor_forms, _check_orientation_forms,
                                     _oracle_descriptors, _oracle_orientation)

pytestmark = pytest.mark.gpu

SIFT_ORI_OBUF = 96          # k_keypoint.hpp: oriented keypoints a wave parks before it reserves slots in the list
# (octave size, ori_sigma): all nine on the default shape; three on the odd one, whose windows hang over every border
ORI_CASES = {kc.SHAPE: [(o, s) for o in kc.OCTSIZES for s in kc.ORI_SIGMAS], kc.ODD_SHAPE: [(1, 1.0), (2, 1.5), (4, 2.5)]}
CASES = [(f, shape) for shape in (kc.SHAPE, kc.ODD_SHAPE) for f in kc.FAMILIES]


@pytest.mark.parametrize("family,shape", CASES)
def test_orientation_on_crafted_planes(siftlib, oracle, family, shape):
    """Every form (a wave or a workgroup per keypoint, the gradient evaluated in the window or read from the plan's own maps)
    on 0, 1 and 7 workgroups, the planes given as those of octave size 1, 2 and 4, ori_sigma 1.0, 1.5 and 2.5: the oriented
    rows as a set, bit for bit, with the oracle's; rows with a NaN angle are dropped by the kernel (the reference's host
    does it), so the count must be the oracle's without them.  The list is never cut (capacity 8 n + 8)."""
    blurs = kc.blur_stack(family, shape)
    kps, ss = kc.orientation_keypoints(family, shape)
    if family == "small":
        # four copies: on one workgroup each of its four waves takes every fourth keypoint and has to flush its parking
        # buffer in mid-list
        kps, ss = np.tile(kps, (4, 1)), np.tile(ss, 4)
        for w in range(4):
            assert len(_oracle_orientation(oracle, blurs, kps[w::4], ss[w::4])) > SIFT_ORI_OBUF
    for octsize, ori_sigma in ORI_CASES[shape]:
        want = _oracle_orientation(oracle, blurs, kps, ss, octsize, ori_sigma)
        what = "%s %r, octsize %d, ori_sigma %.1f" % (family, shape, octsize, ori_sigma)
        _check_orientation_forms(siftlib, blurs, kps, ss, want, what, ORI_FORMS, BLOCKS, octsize, ori_sigma)


@pytest.mark.parametrize("family,shape", CASES)
def test_descriptor_on_crafted_planes(siftlib, oracle, family, shape):
    """Every form (a wave or a workgroup per keypoint over row intervals, with or without the maps, and the streaming form) on
    0, 1 and 7 workgroups, octave sizes 1 and 2: byte for byte the oracle's descriptors -- the all-zero ones of holes, of
    empty and of poisoned histograms included."""
    blurs = kc.blur_stack(family, shape)
    for octsize in (1, 2):
        kk, ss = kc.descriptor_keypoints(family, octsize, shape)
        want = _oracle_descriptors(oracle, blurs, octsize, kk, ss)
        _check_descriptor_forms(siftlib, blurs, octsize, kk, ss, want, "%s %r, octsize %d" % (family, shape, octsize), DESC_FORMS, BLOCKS)
