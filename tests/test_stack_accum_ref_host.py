"""CPU tests of the streaming stack accumulator's row: the restatement tests/stack_accum_ref.py has the properties the contract
promises (any split of a stack gives the same state, an infinite clip is no clip, exact sums give stack_ref's mean bit for bit,
the variance of a 16-bit-like stack is numpy's), every mutant of the restatement changes a result on a crafted case, the
stack_stream test's stack does on the restatement what the GPU test asks of the device, and the host side of the two entry points
(include/siftmi.h) -- header, library and signature table agree, a null handle is refused without a device.  No kernel runs."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import stack_accum_cases as ac
import stack_accum_ref as ar
import stack_cases as sc
import stack_ref as sr
from warp_ref import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INF = float("inf")


def by_name(name):
    return {c.name: c for c in sc.cases()}[name]


def fed(case, per_call, moments=True, interp=None, clip=None, kappa=(3.0, 3.0), vals_live=None):
    """the state after feeding a case's stack in calls of `per_call` frames"""
    vals, live = vals_live if vals_live is not None else ar.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, case.mode, interp)
    st = ar.State(case.out_shape, moments)
    for a, b in ac.splits(len(case.frames), per_call):
        st.add_samples(vals[a:b], live[a:b], clip, kappa)
    return st


@pytest.mark.parametrize("name,interp", [("noise-leaving-S8-41x70-m1", None), ("order-shift-S200-37x53-m1", None), ("nan-shift-S8-41x70-m1", None),
                                         ("noise-nan_some-S5-41x70-m1", None), ("noise-rot-S5-41x70-m1", "cubic"), ("noise-half-S5-41x70-m0", None)])
def test_any_split_of_a_stack_gives_the_same_state_bit_for_bit(name, interp):
    case = by_name(name)
    vl = ar.samples(case.frames, case.maps, case.fills, sc.SHAPE, case.out_shape, case.mode, interp)
    rng = np.random.default_rng(3)
    center = rng.normal(0.0, 3.0, case.out_shape).astype(F)
    var = (rng.random(case.out_shape) * 50.0).astype(F)
    for clip in (None, (center, var)):
        whole = fed(case, None, clip=clip, kappa=(1.5, 2.0), vals_live=vl)
        assert whole.coverage.max() >= 2
        if clip is not None and name.startswith("noise"):
            assert 0 < (whole.kept < whole.coverage).sum()                              # the clip does something here
        for per_call in ac.CALLS[1:]:
            assert fed(case, per_call, clip=clip, kappa=(1.5, 2.0), vals_live=vl).same(whole), (name, per_call)
        # a call without a frame changes nothing, and without s2 the other planes are the same
        again = whole.copy().add([], [], [], sc.SHAPE)
        assert again.same(whole)
        bare = fed(case, 3, moments=False, clip=clip, kappa=(1.5, 2.0), vals_live=vl)
        assert bare.s2 is None and same(bare.s1, whole.s1, nan_any_payload=True) and np.array_equal(bare.kept, whole.kept)


def test_a_clip_with_both_kappas_infinite_is_no_clip():
    for name in ("noise-leaving-S8-41x70-m1", "inf-shift-S8-41x70-m0", "nan-shift-S8-41x70-m1"):
        case = by_name(name)
        rng = np.random.default_rng(4)
        center = rng.normal(0.0, 3.0, case.out_shape).astype(F)
        var = (rng.random(case.out_shape) * 5.0).astype(F)
        var[::3] = 0.0                                                   # inf * 0 is NaN: the comparison is false
        center[1::5] = np.nan
        plain = fed(case, None)
        assert fed(case, None, clip=(center, var), kappa=(INF, INF)).same(plain), name
        one = fed(case, None, clip=(center, var), kappa=(INF, 0.5))
        assert not one.same(plain) and np.array_equal(one.coverage, plain.coverage)


def test_the_binary64_quotient_rounded_to_binary32_is_the_binary32_quotient():
    """(float)(a / c) in binary64 == a / c in binary32 for every whole |a| < 2 ** 18 and 1 <= c <= 512: what lets the accumulator's
    mean equal stack_batch's where the sums are exact.  Exhaustive."""
    a = np.arange(-(1 << 18) + 1, 1 << 18, dtype=np.int64)
    a64, a32 = a.astype(np.float64), a.astype(F)
    for c in range(1, 513):
        assert np.array_equal((a64 / np.float64(c)).astype(F), a32 / F(c)), c


@pytest.mark.parametrize("S,family", [(200, "shift"), (64, "leaving"), (5, "nan_some")])
def test_whole_numbers_and_whole_shifts_give_the_mean_of_stack_ref_bit_for_bit(S, family):
    frames = ac.integer_stack(S)
    maps, fills = sc.maps_of(family if family != "leaving" else "shift", S), sc.fills_of(S)
    if family == "leaving":                                             # whole shifts that push the frames out of view one after another
        maps = [((1.0, 0.0, 0.0, 1.0), (0.0, float(round(s * 52.0 / (S - 1))))) for s in range(S)]
    out_shape = sc.OUTS[1]
    vals, live = sr.samples(frames, maps, fills, sc.SHAPE, out_shape, 1)
    assert (np.abs(vals[live]) < 1024).all() and (vals[live] == np.round(vals[live])).all()
    want, want_c = sr.reduce_samples(vals, live, "mean", -3.0)
    st = ar.State(out_shape, True).add_samples(vals, live)
    assert np.array_equal(st.coverage, want_c) and np.array_equal(st.kept, want_c)
    assert same(st.result(empty=-3.0), want)
    assert want_c.max() >= 2 and want_c.min() == 0


def test_the_variance_of_a_sixteen_bit_like_stack_is_numpys():
    """500 frames of 30000 + 50 N(0, 1): binary32 sums of v and v * v cannot give this variance; the binary64 state does"""
    rng = np.random.default_rng(11)
    vals = (30000.0 + 50.0 * rng.normal(0.0, 1.0, (500, 16, 16))).astype(F)
    live = np.ones(vals.shape, bool)
    st = ar.State((16, 16), True)
    for a in range(0, 500, 64):
        st.add_samples(vals[a:a + 64], live[a:a + 64])
    mean, var = st.result(var=True)
    want_v = np.var(vals.astype(np.float64), axis=0)
    want_m = np.mean(vals.astype(np.float64), axis=0)
    M = st.s1 / 500.0
    V = st.s2 / 500.0 - M * M
    assert (np.abs(V - want_v) <= 1e-9 * want_v).all(), float(np.abs(V / want_v - 1).max())
    assert np.array_equal(var, V.astype(F)) and np.array_equal(mean, M.astype(F)) and (np.abs(M - want_m) <= 1e-12 * want_m).all()
    assert 1500 < want_v.min() and want_v.max() < 3600
    # the same in binary32 is useless, which is what the float32_state mutant is
    bad = ar.State((16, 16), True, rule="float32_state").add_samples(vals, live).result(var=True)[1]
    assert (np.abs(bad - want_v) > 0.05 * want_v).any()


# --------------------------------------------------------------------------------------------------------------- the mutants
def crafted(rule):
    """(state of the contract, state of the mutant, result of each) on the case made for `rule`"""
    shape = (1, 4)
    plane = lambda *v: np.array([v], F)                                 # noqa: E731
    live = np.ones((1,) + shape, bool)
    kw = {}
    if rule == "float32_state":                                          # 1e8 + 1 - 1e8: the 1 is lost in binary32
        vals = np.stack([plane(1e8, 1e8, 1e8, 1e8), plane(1, 1, 1, 1), plane(-1e8, -1e8, -1e8, -1e8)])
        live = np.ones(vals.shape, bool)
    elif rule == "clip_ge":                                              # q == th and q == tl exactly: kept
        vals = np.stack([plane(2.0, -2.0, 3.0, -3.0)])
        kw = dict(clip=(plane(0, 0, 0, 0), plane(1, 1, 2.25, 2.25)), kappa=(2.0, 2.0))
    elif rule == "kappa_swapped":
        vals = np.stack([plane(2.0, -2.0, 2.0, -2.0)])
        kw = dict(clip=(plane(0, 0, 0, 0), plane(1, 1, 1, 1)), kappa=(1.0, 3.0))
    elif rule == "clip_coverage":                                        # a rejected live sample still counts as covered
        vals = np.stack([plane(9.0, 0.5, -9.0, 0.0)])
        kw = dict(clip=(plane(0, 0, 0, 0), plane(1, 1, 1, 1)), kappa=(3.0, 3.0))
    else:                                                                # var_unclamped: 39 equal samples and one a binary32 step above:
        rng = np.random.default_rng(12)                                  # the true variance is below the rounding of s2 / k and M * M,
        shape = (1, 512)                                                 # so V comes out negative in some pixels
        one = (rng.random(shape) * 100.0).astype(F)
        vals = np.stack([one] * 39 + [np.nextafter(one, F(np.inf))])
        live = np.ones(vals.shape, bool)
    out = []
    for r in (None, rule):
        st = ar.State(shape, True, rule=r).add_samples(vals, live, **kw)
        out.append((st, st.result(empty=-1.0, var=True)))
    return out


@pytest.mark.parametrize("rule", ar.MUTANTS)
def test_every_mutant_of_the_restatement_changes_a_result(rule):
    (st, (mean, var)), (mst, (mmean, mvar)) = crafted(rule)
    changed = (not same(mean, mmean, nan_any_payload=True) or not same(var, mvar, nan_any_payload=True) or not np.array_equal(st.kept, mst.kept)
               or not np.array_equal(st.coverage, mst.coverage))
    assert changed, rule
    if rule == "float32_state":
        assert (mean == F(1.0 / 3.0)).all() and (mmean == 0).all()
    elif rule == "clip_ge":
        assert (st.kept == 1).all() and (mst.kept == 0).all()
    elif rule == "kappa_swapped":
        assert st.kept.tolist() == [[1, 0, 1, 0]] and mst.kept.tolist() == [[0, 1, 0, 1]]
    elif rule == "clip_coverage":
        assert st.coverage.tolist() == [[1, 1, 1, 1]] and st.kept.tolist() == [[0, 1, 0, 1]] and mst.coverage.tolist() == [[0, 1, 0, 1]]
    else:
        assert (var >= 0).all() and (mvar < 0).any() and (var[mvar < 0] == 0).all()


def test_the_clips_edges_one_binary32_step_apart():
    """q == tl is kept and the next binary32 above is rejected, on each side; d == 0, var == 0, NaN centre, NaN variance, NaN sample"""
    up = lambda v: np.nextafter(F(v), F(np.inf))                        # noqa: E731
    # centre 0, var 1, kappa (2, 3): tl = 4, th = 9; 2 * 2 == 4 and 3 * 3 == 9 exactly; up(2) ** 2 > 4 and up(3) ** 2 > 9 in binary32
    assert F(up(2.0)) * F(up(2.0)) > F(4.0) and F(up(3.0)) * F(up(3.0)) > F(9.0)
    vals = np.array([[[-2.0, -up(2.0), 3.0, up(3.0), 2.5, -2.5, 0.0, np.nan]]], F)
    live = np.ones(vals.shape, bool)
    ones, zeros = np.ones((1, 8), F), np.zeros((1, 8), F)
    st = ar.State((1, 8), True).add_samples(vals, live, clip=(zeros, ones), kappa=(2.0, 3.0))
    assert st.kept.tolist() == [[1, 0, 1, 0, 1, 0, 1, 1]] and (st.coverage == 1).all()
    # var == 0 rejects all that differs from the centre; d == 0 stays; a NaN sample stays
    st = ar.State((1, 8), True).add_samples(vals, live, clip=(zeros, zeros), kappa=(2.0, 3.0))
    assert st.kept.tolist() == [[0, 0, 0, 0, 0, 0, 1, 1]]
    # a NaN centre or a NaN variance rejects nothing
    for clip in ((np.full((1, 8), np.nan, F), ones), (zeros, np.full((1, 8), np.nan, F))):
        assert (ar.State((1, 8), True).add_samples(vals, live, clip=clip, kappa=(0.001, 0.001)).kept == 1).all()
    # inf on one side
    assert ar.State((1, 8), True).add_samples(vals, live, clip=(zeros, ones), kappa=(INF, 1.0)).kept.tolist() == [[1, 1, 0, 0, 0, 1, 1, 1]]
    assert ar.State((1, 8), True).add_samples(vals, live, clip=(zeros, ones), kappa=(1.0, INF)).kept.tolist() == [[0, 0, 1, 1, 1, 0, 1, 1]]


def test_the_stream_stack_loses_its_zingers_and_nothing_else_in_two_passes():
    """the assertion tests/test_gpu_stack_accum.py makes on the device's stack_stream, here on the restatement with the maps a
    perfect estimate returns: kept == coverage - 1 at exactly the zinger pixels, kept == coverage elsewhere, wherever coverage >= 11"""
    ref, clean, dirty, where = ac.stream_stack()
    maps, fills = ac.stream_ideal_maps(), np.zeros(12, F)
    first = ar.State(ref.shape, True)
    for a, b in ac.splits(12, 5):
        first.add(dirty[a:b], maps[a:b], fills[a:b], ref.shape)
    center, var = first.result(var=True)
    second = ar.State(ref.shape, False).add(dirty, maps, fills, ref.shape, clip=(center, var), kappa=(3.0, 3.0))
    zing = np.zeros(ref.shape, bool)
    for yr, xr in where:
        zing[yr, xr] = True
    assert zing.sum() == 12
    many = second.coverage >= 11
    assert many.sum() > 200 * 200 and many[zing].all() and (second.coverage[zing] == 12).sum() >= 1
    assert np.array_equal(second.kept[many & zing], second.coverage[many & zing] - 1)
    assert np.array_equal(second.kept[many & ~zing], second.coverage[many & ~zing])
    # and the clipped mean is within the noise of the clean frames' mean there, which the plain mean is not
    cleanm = ar.State(ref.shape, False).add(clean, maps, fills, ref.shape).result()
    assert (np.abs(second.result()[many] - cleanm[many]) < ac.STREAM_NOISE).all()
    assert (np.abs(first.result()[zing] - cleanm[zing]) > 2000.0).all()


# ------------------------------------------------------------------------------------------------------------ the host side
@pytest.fixture(scope="module")
def L():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_both_symbols_are_declared_exported_and_bound_with_matching_argument_counts(L):
    from sift_pyocl_amd import _lib
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, count, floats in (("siftmi_batch_stack_accum", 19, [16, 17]), ("siftmi_batch_stack_accum_result", 11, [9])):
        assert name in _lib.exported_symbols() and hasattr(L, name)
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m and len(m.group(1).split(",")) == count == len(_lib._SIGNATURES[name][1]), name
        sig = _lib._SIGNATURES[name]
        assert sig[0] is C.c_int and [i for i, t in enumerate(sig[1]) if t is C.c_float] == floats


def test_a_null_handle_is_refused_before_any_device_is_touched(L):
    from sift_pyocl_amd import _lib
    img = np.zeros((8, 8), F)
    ptrs = (C.c_void_p * 1)(img.ctypes.data)
    s1, s2 = np.full((8, 8), -77.0), np.full((8, 8), -78.0)
    cov, kept = np.full((8, 8), -5, np.int32), np.full((8, 8), -6, np.int32)
    mean, var = np.full((8, 8), -7, F), np.full((8, 8), -8, F)
    maps = np.array([[1, 0, 0, 1, 0, 0]], F); fills = np.zeros(1, F)
    ms = C.c_double(-1)
    for interp in (0, 1):
        rc = L.siftmi_batch_stack_accum(None, ptrs, 1, 0, s1.ctypes.data, s2.ctypes.data, cov.ctypes.data, kept.ctypes.data, 8, 8, maps.ctypes.data,
                                        fills.ctypes.data, 1, interp, None, None, C.c_float(3.0), C.c_float(3.0), C.byref(ms))
        assert rc == _lib.EINVAL and _lib.last_error()
    rc = L.siftmi_batch_stack_accum_result(None, s1.ctypes.data, s2.ctypes.data, kept.ctypes.data, 8, 8, mean.ctypes.data, var.ctypes.data, 0,
                                           C.c_float(0.0), C.byref(ms))
    assert rc == _lib.EINVAL and _lib.last_error()
    assert (s1 == -77).all() and (s2 == -78).all() and (cov == -5).all() and (kept == -6).all() and (mean == -7).all() and (var == -8).all()
    assert ms.value == -1


def test_the_classes_and_methods_exist_with_the_documented_parameters():
    import sift_pyocl_amd as sp
    assert sp.StackAccumulator is sp.batch.StackAccumulator and "StackAccumulator" in sp.__all__
    assert list(inspect.signature(sp.BatchPlan.stack_accumulator).parameters) == ["self", "out_shape", "moments"]
    sig = inspect.signature(sp.StackAccumulator.add)
    assert list(sig.parameters) == ["self", "images", "matrices", "offsets", "fills", "mode", "interp", "clip", "kappa"]
    assert [p for p, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY] == ["interp", "clip", "kappa"]
    assert sig.parameters["kappa"].default == (3.0, 3.0) and sig.parameters["fills"].default == 0.0 and sig.parameters["mode"].default == 1
    sig = inspect.signature(sp.StackAccumulator.result)
    assert list(sig.parameters) == ["self", "empty", "var", "counts", "out"] and np.isnan(sig.parameters["empty"].default)
    for name in ("reset", "state"):
        assert callable(getattr(sp.StackAccumulator, name))
    sig = inspect.signature(sp.LinearAlign.stack_stream)
    assert list(sig.parameters) == ["self", "images", "chunk", "reject", "kappa", "var", "max_shift", "expected_shift", "shift_only", "robust",
                                    "robust_tol", "robust_hyp", "match_ratio", "empty", "return_all", "out", "lanes", "interp"]
    assert sig.parameters["chunk"].default == 32 and sig.parameters["reject"].default is None and sig.parameters["interp"].kind is inspect.Parameter.KEYWORD_ONLY
