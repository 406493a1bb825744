"""CPU tests of the align_batch row: the decision rule of tests/align_batch_ref.py on crafted tables, its coefficient layout
against LinearAlign._affine, the warp of an all-NaN map, and the host side of the two new entry points (include/siftmi.h:
siftmi_batch_transform, siftmi_batch_minmax) -- header, library and signature table agree, a null handle is refused without a
device.  No kernel runs."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import align_batch_ref as ab
from warp_ref import same, warp_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
NAN6 = [np.nan] * 6
GOOD = [1.01, 0.02, 3.5, -0.015, 0.99, -4.25]          # a, b, c, d, e, f


def test_eighteen_pairs_make_a_segment_affine_and_seventeen_do_not():
    pc = [17, 18]
    models = np.array([GOOD, GOOD])
    shifts = np.array([[2.5, -1.25], [7.0, 8.0]], F)
    mode, matrix, offset = ab.align_batch_ref(pc, models, [17, 18], shifts, [17, 18])
    assert mode.tolist() == [1, 2] and mode.dtype == np.int8
    assert same(matrix[0], np.identity(2, dtype=F)) and same(offset[0], np.array([-1.25, 2.5], F))
    assert same(matrix[1], np.array([[0.99, -0.015], [0.02, 1.01]], F)) and same(offset[1], np.array([-4.25, 3.5], F))
    # the pairs the FIT used count, not the rows of the segment: 30 rows of which 17 were usable stay a shift
    mode, _, _ = ab.align_batch_ref([30], np.array([GOOD]), [17], np.array([[1.0, 2.0]], F), [17])
    assert mode.tolist() == [1]


def test_a_degenerate_segment_takes_the_shift_and_an_empty_one_nothing():
    pc = [30, 0, 5, 4]
    models = np.array([NAN6, NAN6, NAN6, GOOD])
    shifts = np.array([[0.5, 0.75], [np.nan, np.nan], [np.nan, np.nan], [-3.0, 9.0]], F)
    mode, matrix, offset = ab.align_batch_ref(pc, models, [30, 0, 0, 4], shifts, [30, 0, 0, 4])
    assert mode.tolist() == [1, 0, 0, 1]                 # NaN model with 30 pairs: shift; pc == 0 and 5 unusable pairs: none
    assert same(offset[0], np.array([0.75, 0.5], F)) and same(offset[3], np.array([9.0, -3.0], F))
    for s in (1, 2):
        assert np.isnan(matrix[s]).all() and np.isnan(offset[s]).all()
    assert matrix.dtype == F and offset.dtype == F and matrix.shape == (4, 2, 2) and offset.shape == (4, 2)
    # one non-finite coefficient is enough
    bad = np.array([GOOD]); bad[0, 2] = np.inf
    assert ab.align_batch_ref([40], bad, [40], np.array([[1, 1]], F), [40])[0].tolist() == [1]


def test_shift_only_never_fits():
    mode, matrix, offset = ab.align_batch_ref([50, 0], None, None, np.array([[4.0, -6.0], [np.nan, np.nan]], F), [50, 0], shift_only=True)
    assert mode.tolist() == [1, 0] and same(offset[0], np.array([-6.0, 4.0], F))
    mode, _, _ = ab.align_batch_ref([50], np.array([GOOD]), [50], np.array([[4.0, -6.0]], F), [50], shift_only=True)
    assert mode.tolist() == [1]


def test_a_segment_without_a_winner_uses_all_its_pairs():
    pc = [4, 0, 2, 3]
    mask = np.array([1, 0, 1, 1, 0, 0, 0, 0, 0], np.uint8)
    models = np.array([GOOD, NAN6, NAN6, NAN6], F)
    got = ab.used_mask(mask, models, pc)
    assert got.tolist() == [1, 0, 1, 1, 1, 1, 1, 1, 1] and mask.tolist() == [1, 0, 1, 1, 0, 0, 0, 0, 0]
    assert ab.used_mask(np.zeros(0, np.uint8), np.zeros((2, 6), F) * np.nan, [0, 0]).shape == (0,)


def test_coefficient_layout_is_that_of_linear_align():
    from sift_pyocl_amd import LinearAlign
    from sift_pyocl_amd.alignment import MIN_MATCHES_AFFINE
    from sift_pyocl_amd.utils import affine_least_squares
    assert ab.MIN_MATCHES_AFFINE == MIN_MATCHES_AFFINE
    rng = np.random.default_rng(15)
    g0 = (rng.random((40, 4)) * 300).astype(F)
    g1 = g0.copy()
    g1[:, 0] = 1.01 * g0[:, 0] + 0.02 * g0[:, 1] + 3.0
    g1[:, 1] = -0.015 * g0[:, 0] + 0.99 * g0[:, 1] - 4.0
    model = np.asarray(affine_least_squares(g0[:, 0], g0[:, 1], g1[:, 0], g1[:, 1])[:6], np.float64)
    want_m, want_o = LinearAlign._affine(g0, g1)
    mode, matrix, offset = ab.align_batch_ref([40], model[None], [40])
    assert mode.tolist() == [2] and same(matrix[0], want_m) and same(offset[0], want_o)


@pytest.mark.parametrize("kind", ["gray", "rgb"])
def test_an_all_nan_map_warps_to_a_plane_of_fill(kind):
    import warp_cases as wc
    img = wc.image((kind, wc.SHAPE))
    for fill in (13.7, 0.0, 255.0):
        out, counts = warp_ref(img, [np.nan] * 4, [np.nan] * 2, wc.OUT, fill, 1)
        assert counts["inside"] == 0
        want = np.full(out.shape, F(fill)).astype(out.dtype)        # (uint8) 13.7f = 13
        assert same(out, want)


NEW = {"siftmi_batch_transform": 13, "siftmi_batch_minmax": 4}


@pytest.fixture(scope="module")
def L():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_library_and_signature_table_agree(L):
    from sift_pyocl_amd import _lib
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in NEW.items():
        assert name in _lib.exported_symbols()
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib._SIGNATURES[name][1]), name
        assert hasattr(L, name)


def test_a_null_handle_is_refused_before_any_device_is_touched(L):
    from sift_pyocl_amd import _lib
    img = np.zeros((8, 8), F)
    ptrs = (C.c_void_p * 1)(img.ctypes.data)
    out = np.full((8, 8), -77, F)
    maps = np.array([[1, 0, 0, 1, 0, 0]], F); fills = np.zeros(1, F)
    ms = C.c_double(-1)
    rc = L.siftmi_batch_transform(None, ptrs, 1, 0, 1, out.ctypes.data, 0, 8, 8, maps.ctypes.data, fills.ctypes.data, 1, C.byref(ms))
    assert rc == _lib.EINVAL and _lib.last_error()
    assert (out == -77).all() and ms.value == -1
    mins, maxs = np.full(1, -5, F), np.full(1, -5, F)
    assert L.siftmi_batch_minmax(None, mins.ctypes.data, maxs.ctypes.data, 1) == _lib.EINVAL and _lib.last_error()
    assert (mins == -5).all() and (maxs == -5).all()


def test_the_methods_exist_with_the_documented_parameters():
    from sift_pyocl_amd import BatchPlan, LinearAlign
    assert list(inspect.signature(BatchPlan.minmax_batch).parameters) == ["self"]
    assert list(inspect.signature(BatchPlan.transform_batch).parameters) == [
        "self", "images", "matrices", "offsets", "fills", "out_shape", "mode", "out"]
    sig = inspect.signature(LinearAlign.align_batch)
    assert list(sig.parameters) == ["self", "images", "shift_only", "robust", "robust_tol", "robust_hyp", "match_ratio", "return_all",
                                    "out", "lanes"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [False, False, 3.0, 2048, None, False, "host", None]
    d = inspect.signature(BatchPlan.transform_batch).parameters
    assert (d["fills"].default, d["out_shape"].default, d["mode"].default, d["out"].default) == (0.0, None, 1, "host")
    for absent in ("relative", "double_check", "orsa", "max_shift", "match_metric"):
        assert absent not in sig.parameters
