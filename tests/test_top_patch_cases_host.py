"""The case builder of the lazy detection chain (tests/top_patch_cases.py) produces what it claims -- checked on the CPU against
the oracle -- and the entry points the GPU tests go through exist."""
import numpy as np
import pytest

import top_patch_cases as tp
from test_gpu_top_patch import CASES, params


@pytest.mark.parametrize("name,shape,border,rows", CASES)
def test_case_contains_what_it_is_named_for(oracle, name, shape, border, rows):
    opar, _ = params(oracle, border)
    case = tp.build(oracle, name, shape, border)
    assert case.blurs5.shape == (5,) + shape and case.blurs5.dtype == np.float32
    e = tp.expect(oracle, case, opar, key=(name, shape, border))
    tp.assert_named(case, e)
    # DoG0..3 are exact: small integers wherever the planes are finite and no centre was planted
    d = e.dogs[:4]
    fin = np.isfinite(d)
    whole = fin & (d == np.rint(d))
    assert whole.sum() >= fin.sum() - 4 * len(case.sites) * 2
    # the patches of the provisional candidates lie inside the plane after clipping and cover each candidate's 3 x 3
    m = tp.patch_mask(e.prov3, *shape)
    for r in e.prov3:
        y, x = int(r[1]), int(r[2])
        assert border <= y < shape[0] - border and border <= x < shape[1] - border and m[y - 1:y + 2, x - 1:x + 2].all()


def test_case_list_covers_the_geometry():
    widths = {shape[1] - 2 * border for _, shape, border, _ in CASES}
    assert set(tp.AREA_W) <= widths
    assert {border for _, _, border, _ in CASES} == {1, 5} and {rows for _, _, _, rows in CASES} == {4, 64}
    assert {name for name, _, _, _ in CASES} == {"planted", "nonfinite", "none", "rejected", "dense"}
    assert all(shape[0] * shape[1] > 64 * 64 for _, shape, _, _ in CASES)      # more pixels than the tail kernel's 64 x 64


def test_top_taps_are_the_plans(oracle):
    t = tp.top_taps(oracle)
    assert len(t) == 27 and np.array_equal(t, t[::-1])


def test_entry_points_are_declared():
    from sift_pyocl_amd import _lib
    import sift_pyocl_amd as sp
    assert "siftmi_stage_detect_lazy" in _lib.exported_symbols() and "siftmi_plan_lazy_octaves" in _lib.exported_symbols()
    assert callable(sp.SiftPlan.lazy_octaves)
