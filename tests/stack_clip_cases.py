"""Crafted stacks for the clipped stack reduction (siftmi_batch_stack_clip: stack_clip_kernel in csrc/k_stack_clip.hpp), shared by
tests/test_stack_clip_ref_host.py and tests/test_gpu_stack_clip.py.  numpy only.

Frames (37 x 53), maps, fills and output shapes (37 x 53, 41 x 70, 1 x 1) are stack_cases'.  A case is a stack -- frames, maps,
fills, output shape, mode -- and the parameters of one call; stacks are shared between cases (the same `stack` name: the samples
are computed once).

Families (the `family` of a case)
  trim      the pairs of PAIRS on 64 noise frames under `leaving` (coverage from 64 down to 0 across a row) and `nan_some`; every
            stack size under `leaving`; ties (seven values, many equal, distinct weights: only the weights show which of equal keys
            went), +-0 (nearest-lower tap: the sign of the result shows whether a -0.0 or a +0.0 went), NaNs of both signs, one
            and two frames
  sigma     one zinger among 63 / 64 noise frames at kappa 3; one among 5 at (3, 3) and (3, 1.5); two-stage zingers (1e6 and 50
            among 64 frames near 0 +- 1) with iters 0, 1, 2, 5; 0, 0, 0, 0, 5 at kappa_high 2 and just below; alternating +-1 at
            kappa 0.5; all-equal values; fewer than three samples; kappa_low = inf; inf, NaN and 3e38 samples
  weights   0.5, 1 and 3 mixed, under both rules
"""
import collections

import numpy as np

import stack_cases as sc

F = np.float32
PAIRS = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 3), (0, 63), (63, 0), (31, 32))
# more small trims, up to three samples on a side, on the stacks where the order is hardest (ties, +-0, NaNs) and where the
# coverage takes every count from 0 to 8
EDGE_PAIRS = ((2, 2), (0, 2), (2, 0), (1, 2), (3, 0), (0, 3), (3, 2))
TWO_STAGE = dict(first=(7, F(1e6), slice(0, 30)), second=(20, F(50.0), slice(10, 40)))     # frame, value, columns
BELOW_TWO = float(np.nextafter(F(2.0), F(0.0)))

Case = collections.namedtuple("Case", "name stack frames maps fills out_shape mode family reject trim kappa iters weights")
_STACKS = {}


def mixed_weights(S):
    return np.array([(0.5, 1.0, 3.0)[(s * 5 + s // 3) % 3] for s in range(S)], F)


def distinct_weights(S):
    """all different and all exact in float32"""
    return np.array([1.0 + 2.0 ** -(s % 20 + 1) + (s // 20) for s in range(S)], F)


def constant_frames(values):
    return [np.full(sc.SHAPE, v, F) for v in values]


def noisy_zinger_frames(S, seed):
    """the smooth plane plus N(0, 1) noise in every frame, and frame s's zinger at stack_cases.zinger_pixel(s)"""
    rng = np.random.default_rng(2000 + seed)
    out = []
    for s in range(S):
        f = (sc.base_plane() + rng.normal(0.0, 1.0, sc.SHAPE)).astype(F)
        f[sc.zinger_pixel(s)] = sc.ZINGER
        out.append(np.ascontiguousarray(f))
    return out


def two_stage_frames(seed=3):
    """64 frames of N(0, 1); frame 7 holds 1e6 in columns 0..29, frame 20 holds 50 in columns 10..39: in columns 10..29 the first
    pass takes the 1e6 (the 50 lies below the mean then) and the second pass the 50"""
    rng = np.random.default_rng(3000 + seed)
    out = [rng.normal(0.0, 1.0, sc.SHAPE).astype(F) for _ in range(64)]
    for s, v, cols in TWO_STAGE.values():
        out[s][:, cols] = v
    return out


def stack(name, frames, family_of_maps, out_shape, mode=1):
    if name not in _STACKS:
        S = len(frames)
        _STACKS[name] = (name, frames, sc.maps_of(family_of_maps, S), sc.fills_of(S), tuple(out_shape), mode)
    return _STACKS[name]


def case(label, st, family, reject, trim=(0, 1), kappa=(3.0, 3.0), iters=3, weights=None):
    return Case("%s-%s" % (st[0], label), st[0], st[1], st[2], st[3], st[4], st[5], family, reject, tuple(trim), tuple(kappa), iters, weights)


_CASES = None


def cases():
    """every case, built once"""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    O0, O1, O2 = sc.OUTS
    # ---- trim
    leaving64 = stack("noise-leaving-S64", sc.frames_of("noise", 64, seed=70), "leaving", O1)
    some64 = stack("noise-nan_some-S64", sc.frames_of("noise", 64, seed=71), "nan_some", O1)
    for lo, hi in PAIRS:
        out.append(case("trim%d_%d" % (lo, hi), leaving64, "trim", "trim", trim=(lo, hi)))
        out.append(case("trim%d_%d" % (lo, hi), some64, "trim", "trim", trim=(lo, hi)))
    for i, S in enumerate(sc.SIZES):
        shape = O2 if S == 3 else (O0 if S in (2, 63) else O1)
        st = stack("noise-leaving-S%d-%dx%d" % ((S,) + shape), sc.frames_of("noise", S, seed=80 + i), "leaving", shape)
        out.append(case("trim1_1", st, "trim", "trim", trim=(1, 1)))
        out.append(case("sigma", st, "sigma", "sigma", kappa=(1.5, 1.5)))
    # (64 frames leave over 53 columns: coverage 3 never occurs; the eight frames of this stack take every count from 0 to 8)
    leaving8 = stack("noise-leaving-S8-41x70", None, "leaving", O1)
    for lo, hi in PAIRS:
        if lo + hi + 1 < 8 and (lo, hi) != (1, 1):
            out.append(case("trim%d_%d" % (lo, hi), leaving8, "trim", "trim", trim=(lo, hi)))
    zeros5 = stack("zeros-identity-S5-m0", sc.frames_of("zeros", 5, seed=105), "identity", O0, mode=0)
    for lo, hi in EDGE_PAIRS:
        out.append(case("trim%d_%d" % (lo, hi), leaving8, "trim", "trim", trim=(lo, hi)))
        out.append(case("trim%d_%d-w" % (lo, hi), zeros5, "trim", "trim", trim=(lo, hi), weights=distinct_weights(5)))
    rising1 = stack("noise-rising-S64-1x1", sc.frames_of("noise", 64, seed=89), "rising", O2)        # one live frame in 64
    out.append(case("trim2_3", rising1, "trim", "trim", trim=(2, 3)))
    for S, fam, shape in ((5, "identity", O0), (8, "shift", O1), (64, "shift", O0)):
        st = stack("ties-%s-S%d" % (fam, S), sc.frames_of("ties", S, seed=90 + S), fam, shape)
        for lo, hi in ((1, 1), (2, 3), (0, 1), (1, 0)) + EDGE_PAIRS:
            out.append(case("trim%d_%d-w" % (lo, hi), st, "trim", "trim", trim=(lo, hi), weights=distinct_weights(S)))
    for S in (3, 5):
        st = stack("zeros-identity-S%d-m0" % S, sc.frames_of("zeros", S, seed=100 + S), "identity", O0, mode=0)
        out.append(case("trim0_1-w", st, "trim", "trim", trim=(0, 1), weights=distinct_weights(S)))
        out.append(case("trim1_1", st, "trim", "trim", trim=(1, 1)))
    for S, fam, shape in ((5, "identity", O0), (8, "shift", O1)):
        st = stack("nan-%s-S%d" % (fam, S), sc.frames_of("nan", S, seed=110 + S), fam, shape)
        out.append(case("trim1_1", st, "trim", "trim", trim=(1, 1)))
        for lo, hi in EDGE_PAIRS:
            out.append(case("trim%d_%d" % (lo, hi), st, "trim", "trim", trim=(lo, hi)))
        out.append(case("sigma1", st, "sigma", "sigma", kappa=(1.0, 1.0)))
    for S in (1, 2):
        st = stack("noise-shift-S%d" % S, sc.frames_of("noise", S, seed=120 + S), "shift", O0)
        out.append(case("trim1_1", st, "trim", "trim", trim=(1, 1)))
        out.append(case("trim0_63", st, "trim", "trim", trim=(0, 63)))
        out.append(case("sigma-k0.1", st, "sigma", "sigma", kappa=(0.1, 0.1)))                      # n < 3: nothing leaves
    # ---- sigma
    for S in (63, 64):
        st = stack("noisyzinger-identity-S%d" % S, noisy_zinger_frames(S, S), "identity", O0)
        out.append(case("sigma3", st, "sigma", "sigma"))
        out.append(case("trim0_1", st, "trim", "trim", trim=(0, 1)))
    five = stack("zinger-identity-S5", sc.frames_of("zinger", 5, seed=20), "identity", O0)
    out.append(case("sigma3_3", five, "sigma", "sigma", kappa=(3.0, 3.0)))
    out.append(case("sigma3_1.5", five, "sigma", "sigma", kappa=(3.0, 1.5)))
    two = stack("twostage-identity-S64", two_stage_frames(), "identity", O0)
    for iters in (0, 1, 2, 5):
        out.append(case("sigma3-i%d" % iters, two, "sigma", "sigma", iters=iters))
    edge = stack("const00005-identity-S5", constant_frames([0, 0, 0, 0, 5]), "identity", O0)
    out.append(case("sigma-kh2", edge, "sigma", "sigma", kappa=(3.0, 2.0)))
    out.append(case("sigma-kh2below", edge, "sigma", "sigma", kappa=(3.0, BELOW_TWO)))
    alt = stack("alternating-identity-S8", constant_frames([1, -1] * 4), "identity", O0)
    out.append(case("sigma-k0.5", alt, "sigma", "sigma", kappa=(0.5, 0.5)))
    equal = stack("equal-shift-S8", constant_frames([2.5] * 8), "shift", O1)
    out.append(case("sigma-k0.5", equal, "sigma", "sigma", kappa=(0.5, 0.5)))
    noise8 = stack("noise-shift-S8", sc.frames_of("noise", 8, seed=130), "shift", O1)
    out.append(case("sigma-inf_2", noise8, "sigma", "sigma", kappa=(np.inf, 2.0)))
    out.append(case("sigma-2_inf", noise8, "sigma", "sigma", kappa=(2.0, np.inf)))
    out.append(case("sigma-inf_inf", noise8, "sigma", "sigma", kappa=(np.inf, np.inf)))
    for kind, mode in (("inf", 0), ("big", 1)):
        st = stack("%s-shift-S8" % kind, sc.frames_of(kind, 8, seed=140), "shift", O1, mode=mode)
        out.append(case("sigma1", st, "sigma", "sigma", kappa=(1.0, 1.0)))
        out.append(case("trim1_1", st, "trim", "trim", trim=(1, 1)))
    # ---- weights
    w8 = stack("noise-leaving-S8-41x70", None, "leaving", O1)                                     # (built above, for every size)
    out.append(case("sigma1.5-mixed", w8, "weights", "sigma", kappa=(1.5, 1.5), weights=mixed_weights(8)))
    out.append(case("trim1_1-mixed", w8, "weights", "trim", trim=(1, 1), weights=mixed_weights(8)))
    out.append(case("trim0_0-mixed", w8, "weights", "trim", trim=(0, 0), weights=mixed_weights(8)))
    out.append(case("sigma3-mixed", leaving64, "weights", "sigma", weights=mixed_weights(64)))
    out.append(case("sigma1.5-ones", w8, "weights", "sigma", kappa=(1.5, 1.5), weights=np.ones(8, F)))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    _CASES = out
    return _CASES


def params(c):
    """the keywords of stack_clip_ref.reduce_clip / BatchPlan.stack_clip_batch for a case"""
    return dict(reject=c.reject, trim=c.trim, kappa=c.kappa, iters=c.iters, weights=c.weights)
