"""CPU checks of the cases of tests/ordering_cases.py (the late-producer tests of tests/test_gpu_ordering.py): a case can only
show that a call read its input too early if the project's reference gives ANOTHER result for the decoy than for the real input,
in the outputs the GPU test compares -- and a stale read must be a read of a valid input, never of an out-of-range index.  Both
are asserted here for every case and every set of late arguments, so a case that cannot tell real from decoy fails on the CPU."""
import numpy as np
import pytest

import ordering_cases as oc


@pytest.mark.parametrize("item", oc.case_variants(), ids=oc.variant_id)
def test_reference_tells_real_from_decoy(item):
    name, late = item
    case = oc.cases()[name]
    real, stale = oc.expected(case), oc.expected(case, late)
    assert oc.same(real, real) and oc.same(stale, stale)
    assert not oc.same(stale, real), "%s: with %s stale the reference gives the result of the real inputs" % (name, "+".join(late))
    differing = [k for k, (a, b) in enumerate(zip(stale, real)) if not oc.same([a], [b])]
    print("%s [%s]: outputs that differ: %s of %d" % (name, "+".join(late), differing, len(real)))


@pytest.mark.parametrize("name", sorted(oc.cases()))
def test_real_and_decoy_are_valid_inputs(name):
    case = oc.cases()[name]
    assert case.inputs
    for arg, inp in case.inputs.items():
        assert inp.valid(inp.real), (name, arg, "real")
        assert inp.valid(inp.decoy), (name, arg, "decoy")
        assert inp.real.shape == inp.decoy.shape and inp.real.dtype == inp.decoy.dtype
        assert not np.array_equal(inp.real.view(np.uint8), inp.decoy.view(np.uint8)), (name, arg, "the decoy is the real input")


def test_every_input_is_late_alone_and_all_together():
    for case in oc.cases().values():
        v = case.variants()
        assert v[-1] == tuple(case.inputs)
        if not case.only_all and len(case.inputs) > 1:
            assert v[:-1] == [(a,) for a in case.inputs]


def test_sizes_are_the_crafted_cases():
    c = oc.cases()
    assert c["plan_keypoints"].inputs["image"].real.shape == (97, 131)
    assert (len(c["match"].inputs["kp1"].real), len(c["match"].inputs["kp2"].real)) == (300, 260)
    assert len(c["match_fit"].inputs["pairs"].real) == 500
    assert c["match_fit_batch"].batch.S == 3 and len(c["match_batch[own]"].counts2) == 3
    assert len(c["batch_stack[mean]"].ready) + 1 == 5
    for name in ("plan_keypoints", "plan_keypoints[uint16]", "plan_keypoints[noncontiguous]"):
        assert len(oc.expected(c[name])[0]) >= 10, "%s: too few keypoints to tell two frames apart" % name


def test_sparse_batch_launches_nothing():
    b = oc.sparse_batch()
    assert len(b.pairs) > 0 and (b.pair_counts < 3).all()
