"""CPU tests of the stack-reduction row: tests/stack_ref.py against numpy.mean / numpy.median where those are comparable, the
crafted stacks of tests/stack_cases.py reaching the rules they are named for, and the host side of siftmi_batch_stack
(include/siftmi.h) -- header, library and signature table agree, a null handle is refused without a device.  No kernel runs."""
import ctypes as C
import inspect
import os
import re
import warnings

import numpy as np
import pytest

import stack_cases as sc
import stack_ref as sr
from warp_ref import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_cache = {}


def sampled(case):
    """(values, live) of a case, computed once"""
    if case.name not in _cache:
        _cache[case.name] = sr.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, case.mode)
    return _cache[case.name]


def by_name(name):
    return {c.name: c for c in sc.cases()}[name]


def test_the_case_list_covers_what_it_promises():
    cases = sc.cases()
    for S in sc.SIZES + (sc.BIG_S,):
        assert any(len(c.frames) == S for c in cases), S
    for S in sc.SIZES:
        assert any(len(c.frames) == S and c.family == "leaving" for c in cases), S
    assert {c.kind for c in cases} == set(sc.KINDS) and {c.family for c in cases} == set(sc.MAPS)
    assert {c.out_shape for c in cases} == set(sc.OUTS) and any(c.mode != 1 for c in cases)
    assert all(f.shape == sc.SHAPE and f.dtype == F for c in cases for f in c.frames)
    assert all(sc.reducers_of(c) == (("sum", "mean", "median") if len(c.frames) <= sr.MEDIAN_MAX else ("sum", "mean")) for c in cases)
    assert len({sc.zinger_pixel(s) for s in range(64)}) == 64


@pytest.mark.parametrize("kind", ["noise", "ties", "zeros", "subnormal", "zinger"])
def test_the_median_is_numpys_over_the_live_samples(kind):
    """finite values: numpy's median of the live float32 samples, equal in value (-0.0 == 0.0)"""
    for case in [c for c in sc.cases() if c.kind == kind and len(c.frames) <= sr.MEDIAN_MAX]:
        vals, live = sampled(case)
        assert np.isfinite(vals[live]).all()
        plane, c = sr.reduce_samples(vals, live, "median", empty=-1.0)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            want = np.nanmedian(np.where(live, vals, F(np.nan)), axis=0)
        assert want.dtype == F and np.array_equal(c, live.sum(axis=0))
        ok = c > 0
        finite = ok & np.isfinite(want)                       # (1e30 + 1e30 is finite; nothing here overflows)
        assert np.array_equal(finite, ok)
        assert np.array_equal(plane[ok], want[ok]), case.name
        assert (plane[~ok] == F(-1.0)).all()


def test_the_mean_is_the_exactly_rounded_ordered_sum_over_the_count():
    """every partial sum formed in float64 and rounded to float32: two float32 terms are added exactly or so far apart that
    the smaller one cannot reach the rounding, so each step is the correctly rounded float32 sum"""
    for case in sc.cases():
        vals, live = sampled(case)
        acc = np.zeros(case.out_shape, F)
        c = np.zeros(case.out_shape, np.int32)
        with np.errstate(all="ignore"):
            for s in range(len(case.frames)):
                step = (acc.astype(np.float64) + vals[s].astype(np.float64)).astype(F)
                acc = np.where(live[s], np.where(c == 0, vals[s], step), acc)
                c += live[s]
            mean = np.where(c > 0, acc / np.maximum(c, 1).astype(F), F(7.0)).astype(F)
        got_sum, got_c = sr.reduce_samples(vals, live, "sum", empty=7.0)
        got_mean, _ = sr.reduce_samples(vals, live, "mean", empty=7.0)
        assert np.array_equal(got_c, c)
        assert same(got_sum, np.where(c > 0, acc, F(7.0)).astype(F), nan_any_payload=True), case.name
        assert same(got_mean, mean, nan_any_payload=True), case.name
        if case.kind in ("ties", "zinger"):                    # well-conditioned: numpy's own mean, in float64
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                want = np.nanmean(np.where(live, vals.astype(np.float64), np.nan), axis=0)
            ok = c > 0
            assert np.allclose(got_mean[ok], want[ok], rtol=1e-5, atol=0), case.name


def test_the_sum_of_one_value_is_that_value():
    vals = np.array([[[-0.0, 5.0]], [[3.0, -0.0]]], F)
    live = np.array([[[True, False]], [[False, True]]])
    for reduce in sr.REDUCERS:
        plane, c = sr.reduce_samples(vals, live, reduce)
        assert c.tolist() == [[1, 1]] and same(plane, np.array([[-0.0, -0.0]], F)), reduce
    plane, c = sr.reduce_samples(vals[:0], live[:0], "mean", empty=-9.0)
    assert c.tolist() == [[0, 0]] and same(plane, np.full((1, 2), -9.0, F))


def test_coverage_runs_from_nothing_to_the_whole_stack():
    for case in [c for c in sc.cases() if c.family == "leaving"]:
        S = len(case.frames)
        _, live = sampled(case)
        c = live.sum(axis=0)
        hist = np.bincount(c.ravel(), minlength=S + 1)
        assert hist[0] > 0 and hist[S] > 0, case.name
        assert (hist > 0).sum() >= min(S + 1, 40), case.name        # and the counts in between (53 columns: not all 65 of them)
        if S >= 2:
            assert (c[c > 0] % 2 == 0).any() and (c % 2 == 1).any(), case.name
    rising = by_name("noise-rising-S64-1x1-m1")
    assert sampled(rising)[1].sum() == 1                            # only the frame that has not moved reaches pixel (0, 0)


def test_the_order_of_the_sum_matters_in_the_order_cases():
    chosen = [c for c in sc.cases() if c.kind == "order" and len(c.frames) % 4 == 0]
    assert {len(c.frames) for c in chosen} == {8, 64, 200}
    for case in chosen:
        vals, live = sampled(case)
        forward, c = sr.ordered_sum(vals, live)
        backward, c2 = sr.ordered_sum(vals, live, order=range(len(case.frames) - 1, -1, -1))
        assert np.array_equal(c, c2)
        assert (forward != backward).any(), case.name
        # and a pairwise tree gives a third answer: (1e8 + 1) + (-1e8 + 1) = 0 where the chain gives 1
        full = c == len(case.frames)
        if full.any():
            pair = (vals[0::2] + vals[1::2])
            tree = (pair[0::2] + pair[1::2]).sum(axis=0, dtype=F)
            assert (tree[full] != forward[full]).any(), case.name


def test_nan_maps_leave_their_frames_out():
    for family, dead in (("nan_mid", 1), ("nan_ends", 2), ("nan_all", 4)):
        case = by_name("noise-%s-S4-41x70-m1" % family)
        vals, live = sampled(case)
        assert live.sum(axis=0).max() == 4 - dead, family
        gone = [s for s in range(4) if not live[s].any()]
        assert len(gone) == dead
        for s in gone:                                              # the warp's plane of such a frame is its fill
            assert same(vals[s], np.full(case.out_shape, case.fills[s], F))
    some = by_name("noise-nan_some-S5-41x70-m1")
    assert [bool(sampled(some)[1][s].any()) for s in range(5)] == [False, False, True, True, False]
    everything = by_name("noise-nan_all-S64-37x53-m1")
    for reduce in sr.REDUCERS:
        plane, c = sr.stack_ref(everything.frames, everything.maps, everything.fills, sc.SHAPE, everything.out_shape, 1, reduce, empty=-4.0)
        assert (c == 0).all() and same(plane, np.full(everything.out_shape, -4.0, F))


def test_the_value_families_reach_their_rules():
    def planes(name):
        case = by_name(name)
        vals, live = sampled(case)
        return {r: sr.reduce_samples(vals, live, r)[0] for r in sr.REDUCERS}, vals, live
    got, vals, live = planes("inf-identity-S5-37x53-m0")
    assert np.isnan(got["sum"]).any() and np.isposinf(got["sum"]).any() and np.isneginf(got["sum"]).any()        # inf + -inf
    assert np.isfinite(got["median"][np.isnan(got["sum"])]).any()
    got, vals, live = planes("big-shift-S8-41x70-m1")
    assert np.isinf(got["sum"]).any() and np.isinf(got["median"]).any()                  # 3e38 + 3e38, in the sum and in lo + hi
    assert (got["median"] == 0).any()                                                   # 3e38 + -3e38
    got, vals, live = planes("nan-identity-S5-37x53-m1")
    with_nan = np.isnan(vals).any(axis=0)
    assert np.isnan(got["median"]).any() and np.isfinite(got["median"][with_nan]).any()  # a NaN at either end of the order
    assert np.isnan(got["sum"][with_nan]).all()
    got, vals, live = planes("zeros-identity-S5-37x53-m1")
    for r in sr.REDUCERS:                                                               # (a bilinear sample of -0.0 is +0.0 unless
        assert (got[r] == 0).all()                                                      # all four taps are -0.0: 0 * px + -0.0)
    got, vals, live = planes("zeros-identity-S3-37x53-m0")                              # the nearest-lower tap keeps the sign
    for r in sr.REDUCERS:
        assert (got[r] == 0).all() and np.signbit(got[r]).any() and not np.signbit(got[r]).all(), r
    got, vals, live = planes("subnormal-shift-S8-41x70-m1")
    tiny = np.abs(got["median"][live.any(axis=0)])
    assert ((tiny > 0) & (tiny < F(1.17549435e-38))).any()
    got, vals, live = planes("ties-identity-S5-37x53-m1")
    assert (np.sort(vals, axis=0)[1] == np.sort(vals, axis=0)[3]).any()                  # three equal values around the middle


def test_integer_shifts_predict_the_answer_and_the_median_drops_the_zingers():
    """frame s is the smooth plane with one outlier; an integer shift samples pixels exactly, so the stack of the SAME plane under
    identity maps is that plane, and a median of three or more frames holds no outlier while the mean does"""
    case = by_name("zinger-identity-S5-37x53-m1")
    base = sc.base_plane()
    med, c = sr.stack_ref(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, 1, "median")
    mean, _ = sr.stack_ref(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, 1, "mean")
    total, _ = sr.stack_ref(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, 1, "sum")
    live_all = c == 5
    assert live_all.all()                                          # the last column is at tx = W - 1 < W - 0.5
    assert np.array_equal(med[live_all], base[live_all])
    hit = np.zeros(sc.SHAPE, bool)
    for s in range(5):
        hit[sc.zinger_pixel(s)] = True
    assert (hit & live_all).sum() == 5
    assert np.array_equal(mean[live_all & ~hit], base[live_all & ~hit])
    assert np.array_equal(total[live_all & hit], 4 * base[live_all & hit] + sc.ZINGER)       # small integers: the sum is exact
    assert (mean[live_all & hit] > 10000).all() and (med < 1000).all()
    # shifted copies: frame s warped by its integer offset is the plane moved by it, wherever it is live
    case = by_name("zinger-shift-S64-41x70-m1")
    vals, live = sampled(case)
    for s in (0, 1, 17, 63):
        dy, dx = (int(v) for v in case.maps[s][1])
        ys, xs = np.nonzero(live[s])
        assert np.array_equal(vals[s][ys, xs], case.frames[s][ys + dy, xs + dx])
    med, c = sr.reduce_samples(vals, live, "median")
    assert c.max() == 64 and (med[c >= 3] < 1000).all()


# ------------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def L():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_the_symbol_is_declared_exported_and_bound_with_fifteen_arguments(L):
    from sift_pyocl_amd import _lib
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    for name, value in (("SIFTMI_STACK_SUM", 0), ("SIFTMI_STACK_MEAN", 1), ("SIFTMI_STACK_MEDIAN", 2), ("SIFTMI_STACK_MEDIAN_MAX", 64)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "siftmi_batch_stack"
    assert name in _lib.exported_symbols() and hasattr(L, name)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m and len(m.group(1).split(",")) == 15 == len(_lib._SIGNATURES[name][1])
    assert _lib._SIGNATURES[name][1][13] is C.c_float and _lib._SIGNATURES[name][0] is C.c_int


def test_a_null_handle_is_refused_before_any_device_is_touched(L):
    from sift_pyocl_amd import _lib
    img = np.zeros((8, 8), F)
    ptrs = (C.c_void_p * 1)(img.ctypes.data)
    out = np.full((8, 8), -77, F)
    cov = np.full((8, 8), -5, np.int32)
    maps = np.array([[1, 0, 0, 1, 0, 0]], F); fills = np.zeros(1, F)
    ms = C.c_double(-1)
    for reduce in (0, 1, 2):
        rc = L.siftmi_batch_stack(None, ptrs, 1, 0, out.ctypes.data, cov.ctypes.data, 0, 8, 8, maps.ctypes.data, fills.ctypes.data, 1, reduce,
                                  C.c_float(0.0), C.byref(ms))
        assert rc == _lib.EINVAL and _lib.last_error()
    assert (out == -77).all() and (cov == -5).all() and ms.value == -1


def test_the_methods_exist_with_the_documented_parameters():
    from sift_pyocl_amd import BatchPlan, LinearAlign
    sig = inspect.signature(BatchPlan.stack_batch)
    assert list(sig.parameters) == ["self", "images", "matrices", "offsets", "fills", "out_shape", "mode", "reduce", "empty", "coverage", "out"]
    d = [sig.parameters[k].default for k in list(sig.parameters)[4:]]
    assert d[:4] == [0.0, None, 1, "mean"] and np.isnan(d[4]) and d[5:] == [False, "host"]
    sig = inspect.signature(LinearAlign.stack)
    assert list(sig.parameters) == ["self", "images", "reduce", "max_shift", "expected_shift", "shift_only", "robust", "robust_tol", "robust_hyp",
                                    "match_ratio", "empty", "return_all", "out", "lanes"]
    d = [sig.parameters[k].default for k in list(sig.parameters)[2:]]
    assert d[:8] == ["mean", None, None, False, False, 3.0, 2048, None] and np.isnan(d[8]) and d[9:] == [False, "host", None]
    # the batch aligners keep their parameter lists
    assert list(inspect.signature(LinearAlign.align_batch).parameters) == [
        "self", "images", "shift_only", "robust", "robust_tol", "robust_hyp", "match_ratio", "return_all", "out", "lanes"]
    assert list(inspect.signature(BatchPlan.transform_batch).parameters) == ["self", "images", "matrices", "offsets", "fills", "out_shape", "mode", "out"]
    assert BatchPlan.STACK_MEDIAN_MAX == sr.MEDIAN_MAX and sorted(BatchPlan.STACK_REDUCERS) == sorted(sr.REDUCERS)
