"""CPU tests of the clipped stack reduction's row: the crafted stacks of tests/stack_clip_cases.py reach the rules they are named
for under tests/stack_clip_ref.py, a restatement with one fused multiply-add changes a case, and the host side of
siftmi_batch_stack_clip (include/siftmi.h) -- header, library and signature table agree, a null handle is refused without a
device, the parameter lists of the two methods.  No kernel runs."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import stack_cases as sc
import stack_clip_cases as cc
import stack_clip_ref as cr
import stack_ref as sr
from shift_ref import key
from warp_ref import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_cache = {}


def sampled(case):
    """(values, live) of a case's stack, computed once"""
    if case.stack not in _cache:
        _cache[case.stack] = sr.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, case.mode)
    return _cache[case.stack]


def by_name(name):
    return {c.name: c for c in cc.cases()}[name]


def run(case, **kw):
    vals, live = sampled(case)
    p = cc.params(case)
    p.update(kw)
    return cr.reduce_clip(vals, live, **p)


def test_the_case_list_covers_what_it_promises():
    cases = cc.cases()
    assert {len(c.frames) for c in cases} == set(sc.SIZES) and {c.out_shape for c in cases} == set(sc.OUTS)
    assert {c.family for c in cases} == {"trim", "sigma", "weights"} and {c.reject for c in cases} == set(cr.REJECTS)
    for maps in ("leaving", "nan_some"):
        assert {c.trim for c in cases if c.stack == "noise-%s-S64" % maps and c.reject == "trim"} == set(cc.PAIRS)
    for S in sc.SIZES:
        assert any(len(c.frames) == S and c.reject == r for c in cases for r in cr.REJECTS), S
    assert {c.iters for c in cases if c.stack.startswith("twostage")} == {0, 1, 2, 5}
    assert all(f.shape == sc.SHAPE and f.dtype == F for c in cases for f in c.frames)
    assert any(c.mode != 1 for c in cases) and any(c.weights is not None for c in cases)


# ---------------------------------------------------------------------------------------------------------------------- trim
def test_trim_keeps_c_minus_h_minus_l_and_never_nothing():
    for case in [c for c in cc.cases() if c.reject == "trim"]:
        plane, c, kept = run(case, empty=-9.0)
        lo, hi = case.trim
        h = np.maximum(np.minimum(hi, c - 1), 0)
        l = np.maximum(np.minimum(lo, c - 1 - h), 0)
        assert np.array_equal(kept, c - h - l), case.name
        assert (kept[c > 0] >= 1).all() and (kept[c == 0] == 0).all() and (plane[c == 0] == F(-9.0)).all(), case.name
    # one plane with coverage below, at and above n_low + n_high + 1, wherever the stack has that many live frames
    for lo, hi in cc.PAIRS:
        full = lo + hi + 1
        for stack, top in (("noise-leaving-S8-41x70" if full < 8 else "noise-leaving-S64", 8 if full < 8 else 64), ("noise-nan_some-S64", 64 - 23)):
            c = run(by_name("%s-trim%d_%d" % (stack, lo, hi)))[1]
            assert c.max() == top and ((c < full) & (c > 0)).any() == (full > 1), (stack, lo, hi)
            assert (c == full).any() == (full <= top) and (c > full).any() == (full < top), (stack, lo, hi)
    # the high side is served first: with coverage 2 and (1, 1) the larger sample goes
    case = by_name("noise-shift-S2-trim1_1")
    vals, live = sampled(case)
    plane, c, kept = run(case)
    two = c == 2
    assert two.any() and (c == 1).any() and np.array_equal(plane[two], np.minimum(vals[0], vals[1])[two])
    one = run(by_name("noise-rising-S64-1x1-trim2_3"))
    assert one[1].tolist() == [[1]] and one[2].tolist() == [[1]]


def test_trim_is_the_sorted_slice_mean_on_finite_values():
    """numpy's own reading: sort the live values, drop h from the top and l from the bottom -- equal in value to a float64 mean"""
    case = by_name("noise-leaving-S64-trim2_3")
    vals, live = sampled(case)
    plane, c, kept = run(case)
    for y, x in ((0, 0), (5, 17), (36, 30), (13, 44), (20, 51), (3, 52)):
        v = np.sort(vals[live[:, y, x], y, x].astype(np.float64))
        n = len(v)
        h = min(3, n - 1); l = min(2, n - 1 - h)
        assert n == c[y, x] and n - h - l == kept[y, x]
        assert np.isclose(plane[y, x], v[l:n - h].mean(), rtol=1e-4, atol=0), (y, x)


def reversed_ties(vals, live, lo, hi):
    """a WRONG reading of the tie rule -- among equal keys the first frame goes with the high side and the last with the low"""
    return cr.trim_keep(vals[::-1], live[::-1], lo, hi)[::-1]


def test_only_the_weights_show_which_of_equal_keys_went():
    seen = 0
    for case in [c for c in cc.cases() if c.stack.startswith("ties-")]:
        vals, live = sampled(case)
        K, wrong = cr.trim_keep(vals, live, *case.trim), reversed_ties(vals, live, *case.trim)
        assert np.array_equal(K.sum(axis=0), wrong.sum(axis=0))
        differ = (K != wrong).any(axis=0)
        assert differ.any(), case.name
        # the kept VALUES are the same multiset either way ...
        assert np.array_equal(np.sort(np.where(K, vals, F(np.inf)), axis=0), np.sort(np.where(wrong, vals, F(np.inf)), axis=0))
        # ... and the plane tells them apart through the weights
        plane = run(case)[0]
        S = len(case.frames)
        w = case.weights.reshape(S, 1, 1)
        with np.errstate(all="ignore"):
            other = sr.ordered_sum(w * vals, wrong)[0] / sr.ordered_sum(np.broadcast_to(w, vals.shape), wrong)[0]
        seen += int((plane[differ] != other[differ]).sum())
        assert len(set(case.weights.tolist())) == S
    assert seen > 100


def test_signed_zeros_and_nans_take_the_place_their_bits_give_them():
    case = by_name("zeros-identity-S3-m0-trim0_1-w")
    vals, live = sampled(case)
    plane, c, kept = run(case)
    assert (c == 3).all() and (kept == 2).all() and (plane == 0).all()
    neg = np.signbit(vals).sum(axis=0)
    assert np.array_equal(np.signbit(plane), neg >= 2)            # the one +0.0 among two -0.0 is the largest key and goes
    assert (neg == 2).any() and (neg == 1).any()
    case = by_name("nan-identity-S5-trim1_1")
    vals, live = sampled(case)
    plane, c, kept = run(case)
    k = key(vals)
    pos_nan = (np.isnan(vals) & ~np.signbit(vals)).sum(axis=0)
    neg_nan = (np.isnan(vals) & np.signbit(vals)).sum(axis=0)
    assert (k[np.isnan(vals) & ~np.signbit(vals)] > key(F([np.inf]))[0]).all()
    assert (pos_nan == 1).any() and (neg_nan == 1).any() and (pos_nan == 2).any()
    assert np.array_equal(np.isnan(plane), (pos_nan > 1) | (neg_nan > 1))       # one NaN on either side is trimmed away


# --------------------------------------------------------------------------------------------------------------------- sigma
def test_one_zinger_among_many_goes_at_kappa_3_and_among_five_only_at_1_5():
    for S in (63, 64):
        case = by_name("noisyzinger-identity-S%d-sigma3" % S)
        vals, live = sampled(case)
        log = []
        plane, c, kept = run(case, log=log)
        assert (c == S).all()
        for s in range(S):
            y, x = sc.zinger_pixel(s)
            assert log[0][s, y, x] and log[0][:, y, x].sum() == 1, (S, s)
            assert abs(plane[y, x] - sc.base_plane()[y, x]) < 1.0 and kept[y, x] <= S - 1
        assert (plane < 1000).all() and (run(case, iters=0)[0] > 900).sum() == S
    three, half = by_name("zinger-identity-S5-sigma3_3"), by_name("zinger-identity-S5-sigma3_1.5")
    hit = np.zeros(sc.SHAPE, bool)
    for s in range(5):
        hit[sc.zinger_pixel(s)] = True
    plane, c, kept = run(three)
    assert (kept == 5).all() and (plane[hit] > 10000).all()                    # 4 / sqrt(5) = 1.79 sigma: it stays
    plane, c, kept = run(half)
    assert np.array_equal(kept, np.where(hit, 4, 5)) and np.array_equal(plane, sc.base_plane())


def test_n_samples_hold_no_z_score_above_n_minus_1_over_root_n():
    for n in range(3, 14):
        vals = np.zeros((n, 1, 1), F)
        vals[n - 1] = 1e4
        live = np.ones((n, 1, 1), bool)
        kept = cr.reduce_clip(vals, live, "sigma", kappa=(3.0, 3.0))[2]
        assert kept[0, 0] == (n if (n - 1) / np.sqrt(n) <= 3.0 else n - 1), n      # 10: 2.85; 11: 3.02


def test_the_second_zinger_goes_in_the_second_pass():
    base = by_name("twostage-identity-S64-sigma3-i5")
    vals, live = sampled(base)
    (s1, v1, cols1), (s2, v2, cols2) = cc.TWO_STAGE["first"], cc.TWO_STAGE["second"]
    both = np.zeros(sc.SHAPE, bool)
    both[:, 10:30] = True
    log = []
    run(base, log=log)
    assert len(log) == 5
    assert log[0][s1][both].all() and not log[0][s2][both].any() and log[1][s2][both].all()
    assert log[0][s2][:, 30:40].all()                          # alone, the 50 goes in the first pass
    kept = {i: run(by_name("twostage-identity-S64-sigma3-i%d" % i))[2] for i in (0, 1, 2, 5)}
    assert (kept[0] == 64).all() and (kept[1][both] == 63).all() and (kept[2][both] <= 62).all() and (kept[2][both] >= 60).all()
    assert (kept[5] <= kept[2]).all() and (kept[5] < kept[2]).any()             # a third pass finds a 3-sigma noise sample somewhere
    p1, p2 = run(by_name("twostage-identity-S64-sigma3-i1"))[0], run(by_name("twostage-identity-S64-sigma3-i2"))[0]
    clean = both & (kept[2] == 62)                                              # mean of 50 and 62 noise samples; of the 62 alone
    assert clean.sum() > 500 and (np.abs(p1 - p2 - F(50.0 / 63))[clean] < 0.02).all() and (np.abs(p2[clean]) < 0.6).all()


def test_the_threshold_is_strict_and_the_guard_keeps_everything():
    plane, c, kept = run(by_name("const00005-identity-S5-sigma-kh2"))
    assert (kept == 5).all() and (plane == F(1.0)).all()                         # mean 1, var 4, threshold 16 == d * d: it stays
    plane, c, kept = run(by_name("const00005-identity-S5-sigma-kh2below"))
    assert F(cc.BELOW_TWO) < F(2.0) and (kept == 4).all() and (plane == F(0.0)).all()
    case = by_name("alternating-identity-S8-sigma-k0.5")
    log = []
    plane, c, kept = run(case, log=log)
    assert (kept == 8).all() and (plane == 0).all() and not any(g.any() for g in log)
    vals, live = sampled(case)
    assert (vals * vals > F(0.25) * F(1.0)).all()                                # m = 0, var = 1: the rule names every sample
    plane, c, kept = run(by_name("equal-shift-S8-sigma-k0.5"))
    assert np.array_equal(kept, c) and (plane[c > 0] == F(2.5)).all() and (c == 0).any()
    for S in (1, 2):
        plane, c, kept = run(by_name("noise-shift-S%d-sigma-k0.1" % S))
        assert np.array_equal(kept, c) and c.max() == S
    few = run(by_name("noise-leaving-S8-41x70-sigma"))
    assert (few[2][few[1] < 3] == few[1][few[1] < 3]).all() and (few[2] < few[1]).any()


def test_an_infinite_kappa_switches_its_side_off_and_non_finite_samples_stop_the_rule():
    vals, live = sampled(by_name("noise-shift-S8-sigma-inf_2"))
    logs = {}
    for name in ("inf_2", "2_inf", "inf_inf"):
        logs[name] = []
        plane, c, kept = run(by_name("noise-shift-S8-sigma-%s" % name), log=logs[name])
        if name == "inf_inf":
            assert np.array_equal(kept, c)
    m = np.where(live, vals, 0).sum(axis=0) / np.maximum(live.sum(axis=0), 1)
    high, low = logs["inf_2"][0], logs["2_inf"][0]
    assert high.any() and low.any() and (vals[high] > np.broadcast_to(m, vals.shape)[high]).all()
    assert (vals[low] < np.broadcast_to(m, vals.shape)[low]).all()
    for stack in ("inf-shift-S8", "big-shift-S8", "nan-shift-S8", "nan-identity-S5"):
        case = by_name("%s-sigma1" % stack)
        vals, live = sampled(case)
        plane, c, kept = run(case)
        bad = (live & ~np.isfinite(vals)).any(axis=0)
        if stack.startswith("big"):
            assert np.array_equal(kept, c) and (np.abs(vals[live]) == F(3e38)).all()       # d * d overflows: inf > inf is false
        else:
            assert bad.any() and np.array_equal(kept[bad], c[bad]) and (kept < c)[~bad].any(), stack


# ----------------------------------------------------------------------------------------------------- weights and identities
def test_weights_and_the_identities_with_the_mean():
    case = by_name("noise-leaving-S8-41x70-sigma1.5-mixed")
    assert sorted(set(case.weights.tolist())) == [0.5, 1.0, 3.0]
    vals, live = sampled(case)
    mixed, ones, none = run(case), run(by_name("noise-leaving-S8-41x70-sigma1.5-ones")), run(case, weights=None)
    assert same(ones[0], none[0], nan_any_payload=True) and np.array_equal(mixed[2], none[2])          # the statistics are unweighted
    assert (mixed[0][mixed[1] > 1] != none[0][mixed[1] > 1]).any()
    # a weighted mean of the kept samples, in float64
    K = cr.sigma_keep(vals, live, 1.5, 1.5, 3)
    w = case.weights.astype(np.float64).reshape(8, 1, 1)
    want = np.where(K, w * vals, 0).sum(axis=0) / np.maximum(np.where(K, w, 0).sum(axis=0), 1e-300)
    ok = mixed[1] > 0
    assert np.allclose(mixed[0][ok], want[ok], rtol=1e-4, atol=1e-4 * np.abs(vals).max())
    for case in cc.cases():                                                                            # nothing rejected: the mean
        vals, live = sampled(case)
        mean, c = sr.reduce_samples(vals, live, "mean", empty=-2.0)
        for kw in (dict(reject="trim", trim=(0, 0)), dict(reject="sigma", iters=0)):
            plane, cov, kept = cr.reduce_clip(vals, live, empty=-2.0, **kw)
            assert same(plane, mean, nan_any_payload=True) and np.array_equal(cov, c) and np.array_equal(kept, c), (case.name, kw)
    # odd S, all live, no NaN: trimming S >> 1 from either side leaves the median
    case = by_name("noisyzinger-identity-S63-sigma3")
    vals, live = sampled(case)
    assert live.all()
    assert same(cr.reduce_clip(vals, live, "trim", trim=(31, 31))[0], sr.reduce_samples(vals, live, "median")[0])


@pytest.mark.parametrize("fuse", ["wv", "dd"])
def test_one_fused_multiply_add_changes_a_case(fuse):
    changed = []
    for case in cc.cases():
        if (fuse == "wv" and case.weights is None) or (fuse == "dd" and case.reject != "sigma"):
            continue
        plane, c, kept = run(case)
        fused = run(case, fuse=(fuse,))
        if not (same(plane, fused[0], nan_any_payload=True) and np.array_equal(kept, fused[2])):
            changed.append(case.name)
    assert changed, fuse


# ------------------------------------------------------------------------------------------------------------------- the ABI
@pytest.fixture(scope="module")
def L():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_the_symbol_is_declared_exported_and_bound_with_twenty_two_arguments(L):
    from sift_pyocl_amd import _lib
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    for name, value in (("SIFTMI_STACK_TRIM", 0), ("SIFTMI_STACK_SIGMA", 1), ("SIFTMI_STACK_CLIP_MAX", 64)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "siftmi_batch_stack_clip"
    assert name in _lib.exported_symbols() and hasattr(L, name)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m and len(m.group(1).split(",")) == 22 == len(_lib._SIGNATURES[name][1])
    sig = _lib._SIGNATURES[name]
    assert sig[0] is C.c_int and [i for i, t in enumerate(sig[1]) if t is C.c_float] == [17, 18, 20]


def test_a_null_handle_is_refused_before_any_device_is_touched(L):
    from sift_pyocl_amd import _lib
    img = np.zeros((8, 8), F)
    ptrs = (C.c_void_p * 1)(img.ctypes.data)
    out = np.full((8, 8), -77, F)
    cov = np.full((8, 8), -5, np.int32)
    kept = np.full((8, 8), -6, np.int32)
    maps = np.array([[1, 0, 0, 1, 0, 0]], F); fills = np.zeros(1, F)
    ms = C.c_double(-1)
    for reject in (0, 1):
        rc = L.siftmi_batch_stack_clip(None, ptrs, 1, 0, out.ctypes.data, cov.ctypes.data, kept.ctypes.data, 0, 8, 8, maps.ctypes.data,
                                       fills.ctypes.data, None, 1, reject, 0, 1, C.c_float(3.0), C.c_float(3.0), 3, C.c_float(0.0), C.byref(ms))
        assert rc == _lib.EINVAL and _lib.last_error()
    assert (out == -77).all() and (cov == -5).all() and (kept == -6).all() and ms.value == -1


def test_the_methods_exist_with_the_documented_parameters():
    from sift_pyocl_amd import BatchPlan, LinearAlign
    sig = inspect.signature(BatchPlan.stack_clip_batch)
    assert list(sig.parameters) == ["self", "images", "matrices", "offsets", "fills", "out_shape", "mode", "reject", "trim", "kappa", "iters",
                                    "weights", "empty", "counts", "out"]
    d = [sig.parameters[k].default for k in list(sig.parameters)[4:]]
    assert d[:8] == [0.0, None, 1, "sigma", (0, 1), (3.0, 3.0), 3, None] and np.isnan(d[8]) and d[9:] == [False, "host"]
    sig = inspect.signature(LinearAlign.stack_clip)
    assert list(sig.parameters) == ["self", "images", "reject", "trim", "kappa", "iters", "weights", "max_shift", "expected_shift", "shift_only",
                                    "robust", "robust_tol", "robust_hyp", "match_ratio", "empty", "return_all", "out", "lanes"]
    d = [sig.parameters[k].default for k in list(sig.parameters)[2:]]
    assert d[:12] == ["sigma", (0, 1), (3.0, 3.0), 3, None, None, None, False, False, 3.0, 2048, None] and np.isnan(d[12])
    assert d[13:] == [False, "host", None]
    assert BatchPlan.STACK_CLIP_MAX == cr.CLIP_MAX == 64 and BatchPlan.STACK_REJECTS == {"trim": 0, "sigma": 1}
    assert sorted(BatchPlan.STACK_REJECTS) == sorted(cr.REJECTS)
    for doc in (BatchPlan.stack_clip_batch.__doc__, LinearAlign.stack_clip.__doc__):
        assert "(n - 1) / sqrt(n)" in doc and "11 live" in " ".join(doc.split())


def test_python_refuses_what_the_library_refuses_before_any_call():
    from sift_pyocl_amd import BatchPlan
    ok = dict(reject="sigma", trim=(0, 1), kappa=(3.0, 3.0), iters=3, weights=None)
    assert BatchPlan._clip_args(**ok)[:6] == (1, 0, 1, 3.0, 3.0, 3)
    assert BatchPlan._clip_args(**dict(ok, reject="trim", trim=(31, 32), kappa=(np.inf, 0.5), iters=0, weights=[0.5, 2]))[:6] == (0, 31, 32, np.inf, 0.5, 0)
    for bad in (dict(reject="median"), dict(reject=1), dict(trim=(-1, 0)), dict(trim=(0, -1)), dict(trim=(32, 32)), dict(trim=(0, 64)),
                dict(trim=(0.5, 1)), dict(trim=3), dict(kappa=(0.0, 3.0)), dict(kappa=(3.0, -1.0)), dict(kappa=(np.nan, 3.0)), dict(kappa=3.0),
                dict(iters=-1), dict(iters=1.5), dict(weights=[1.0, 0.0]), dict(weights=[-1.0]), dict(weights=[np.nan]), dict(weights=[np.inf]),
                dict(weights=[[1.0]])):
        with pytest.raises(ValueError):
            BatchPlan._clip_args(**dict(ok, **bad))
