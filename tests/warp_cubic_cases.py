"""Crafted cases for the cubic sampler (SIFTMI_INTERP_CUBIC: csrc/k_warp_cubic.hpp and the cubic instances of k_stack.hpp /
k_stack_clip.hpp), shared by tests/test_warp_cubic_ref_host.py and tests/test_gpu_warp_cubic.py.  Images, maps and helpers are
warp_cases' and stack_cases' (imported, not edited); a warp case states what it is there for as class counts of
warp_cubic_ref.CLASSES that both tests assert, so that a case cannot silently stop reaching its path.

Warp families (float32 planes, mode 1)
  1 maps      warp_cases._maps on the 40 x 53 plane -> 47 x 59
  2 lattice   quarter-pixel steps at both ends of both axes (tx from -0.25 to 1.25 and from W - 2.25 to W: every clamped column
              and row at every exact weight), -0.0 coordinates, half / half_below
  4 nonfinite every map of warp_cases._nonfinite
  5 shapes    output widths 1 .. 8, 63, 64, 65, 257 by heights 1, 3, 4, 5 on the 16 x 21 plane
  6 tiny      planes (1, 1), (1, 9), (9, 1), (2, 2), (3, 70), (13, 13): for W or H <= 3 every tap clamps
  8 special   the `special` image: -0.0, subnormals, +-inf, NaN, FLT_MAX (a created NaN may carry any payload)
  9 random    40 seeded maps: rotation <= 10 degrees, scale 0.8 .. 1.25, shift +-5

Stacks: stack_cases' kinds at S in SIZES (1, 2, 3, 5 = D - 1, D, D + 1, 2 D + 1 for the cubic kernels' depth D = 2; 4, 8, 64) and
65 for sum / mean, map families shift, half, rot, leaving, nan_some, nan_all.  A NaN that the sampler's own arithmetic creates
(-0 * inf at an integer shift already, inf - inf where 3e38 taps overflow) has the platform's sign, which moves its rank: frames
with inf are left out of the median and clip cases, `big` frames are there under integer shifts only.

numpy only, deterministic from seeds, nothing here imports the package.
"""
import collections
import functools
import math

import numpy as np

import stack_cases as sc
import stack_clip_cases as scc
import warp_cases as wc

F = np.float32
OUT_WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 257]
OUT_HEIGHTS = [1, 3, 4, 5]
DEPTH = 2                                        # SIFT_STACK_DEPTH_CUBIC
SIZES = (1, 2, 3, 4, 5, 8, 64)
BIG_S = 65
STACK_MAPS = ("shift", "half", "rot", "leaving", "nan_some", "nan_all")
NAN_KINDS = ("nan", "inf", "big")                # a sample may be a NaN: compared with nan_any_payload

#: name, family, image key for warp_cases.image(), matrix[4], offset[2], fill, (OH, OW), {class: (op, count)}
Case = collections.namedtuple("Case", "name family image M off fill out_shape expect")


def _lattice(shape):
    H, W = shape
    q = [0.25, 0, 0, 0.25]
    small = (14, 15)                              # t = start + 0.25 * index: 3.25 pixels from the start in both axes
    edge = H + W - 1
    return [
        ("lo_lo", q, [-0.25, -0.25], small, {"clamp_x_lo": (">=", 40), "clamp_y_lo": (">=", 40), "corner": ("==", 16), "integer": (">=", 9),
                                             "interior_wide": (">=", 40)}),
        ("hi_hi", q, [H - 2.25, W - 2.25], small, {"clamp_x_hi1": (">=", 8), "clamp_x_hi2": (">=", 16), "clamp_y_hi1": (">=", 8),
                                                   "clamp_y_hi2": (">=", 16), "corner": ("==", 36), "inside_not_live": (">=", 8)}),
        ("lo_hi", q, [-0.25, W - 2.25], small, {"clamp_y_lo": (">=", 20), "clamp_x_hi1": (">=", 20), "clamp_x_hi2": (">=", 40)}),
        ("hi_lo", q, [H - 2.25, -0.25], small, {"clamp_x_lo": (">=", 20), "clamp_y_hi1": (">=", 20), "clamp_y_hi2": (">=", 40)}),
        ("neg_zero_both", [-1, -0.0, -0.0, -1], [-0.0, -0.0], wc.OUT, {"live": ("==", 1), "integer": ("==", 1), "corner": ("==", 1)}),
        ("neg_zero_x", [1, -0.0, -0.0, -1], [-0.0, -0.0], wc.OUT, {"live": ("==", H), "clamp_x_lo": ("==", H)}),
        ("half", [1, 0, 0, 1], [0.5, 0.5], shape, {"inside_not_live": ("==", edge), "live": ("==", (H - 1) * (W - 1)), "integer": ("==", 0)}),
        ("half_below", [1, 0, 0, 1], [wc.HALF_BELOW, wc.HALF_BELOW], shape, {"inside_not_live": ("==", edge), "live": ("==", (H - 1) * (W - 1))}),
    ]


def random_map(i, shape=wc.SHAPE):
    """(M, off): rotation <= 10 degrees about the centre, scale 0.8 .. 1.25, shift +-5, from seed i"""
    rng = np.random.default_rng(7000 + i)
    deg, scale = rng.uniform(-10, 10), rng.uniform(0.8, 1.25)
    dy, dx = rng.uniform(-5, 5, 2)
    M, off = wc.rotation(deg, shape)
    cy, cx = (shape[0] - 1) / 2.0, (shape[1] - 1) / 2.0
    M = [scale * v for v in M]
    # scaled about the centre as well, then shifted
    off = [cy - (M[0] * cy + M[1] * cx) + dy, cx - (M[2] * cy + M[3] * cx) + dx]
    return M, off


@functools.lru_cache(maxsize=None)
def cases():
    """every warp case, in a fixed order"""
    out = []

    def add(name, family, img, M, off, out_shape, expect=None, fill=13.0):
        out.append(Case("c%d-%s" % (family, name), family, img, tuple(float(v) for v in M), tuple(float(v) for v in off), float(fill),
                        tuple(out_shape), dict(expect or {})))

    H, W = wc.SHAPE
    gray = ("gray", wc.SHAPE)
    n_out = wc.OUT[0] * wc.OUT[1]
    expect1 = {
        "identity": {"live": ("==", H * W), "integer": ("==", H * W), "interior_wide": ("==", H * (W - 3)), "corner": ("==", 9),
                     "clamp_x_lo": ("==", H), "clamp_x_hi1": ("==", H), "clamp_x_hi2": ("==", H)},
        "zero": {"live": ("==", n_out), "corner": ("==", n_out), "clamp_x_hi1": ("==", n_out), "clamp_y_hi1": ("==", n_out)},
        "zoom_corner": {"live": ("==", n_out), "clamp_x_hi2": (">=", 100), "clamp_y_hi2": (">=", 100), "clamp_y_hi1": (">=", 100), "corner": (">=", 100)},
        "rot90": {"live": ("==", H * W), "integer": ("==", H * W)},
        "rot30": {"live": (">=", 1000), "interior_wide": (">=", 1000), "integer": ("<=", 4)},
    }
    for name, M, off, oshape, _ in wc._maps(wc.SHAPE):                                      # 1
        add(name, 1, gray, M, off, oshape, expect1.get(name, {"live": (">=", 100)}))
    for name, M, off, oshape, expect in _lattice(wc.SHAPE):                               # 2
        add(name, 2, gray, M, off, oshape, expect)
    for name, M, off in wc._nonfinite():                                                  # 4
        add(name, 4, gray, M, off, wc.OUT, {"live": ("<=", wc.OUT[0] + wc.OUT[1])})
    r30s = wc.rotation(30, wc.SMALL)
    for name, M, off in (("quarter", [1, 0, 0, 1], [0.25, -0.75]), ("rot30", r30s[0], r30s[1])):      # 5
        for ow in OUT_WIDTHS:
            for oh in OUT_HEIGHTS:
                add("%s_%dx%d" % (name, oh, ow), 5, ("gray", wc.SMALL), M, off, (oh, ow))
    for shape in wc.TINY:                                                                 # 6
        h, w = shape
        img = ("gray", shape)
        wide = h * max(w - 3, 0)
        add("ident_%dx%d" % shape, 6, img, [1, 0, 0, 1], [0, 0], (h + 2, w + 3), {"live": ("==", h * w), "integer": ("==", h * w), "interior_wide": ("==", wide)})
        add("quarter_%dx%d" % shape, 6, img, [0.25, 0, 0, 0.25], [-0.25, -0.25], (4 * h + 4, 4 * w + 5),
            {"live": ("==", (4 * h - 2) * (4 * w - 2)), "interior_wide": ("==" if w <= 3 else ">=", 0 if w <= 3 else 1)})
        add("rot180_%dx%d" % shape, 6, img, [-1, 0, 0, -1], [h - 0.75, w - 0.75], (h + 1, w + 2), {"live": (">=", 1)})
    for off in ([0.5, 0.5], [-0.5, 0.5], [0.25, -0.75], [0.0, 0.0], [2.0, -3.0]):          # 8
        add("special_%g_%g" % tuple(off), 8, ("special", wc.SHAPE), [1, 0, 0, 1], off, wc.OUT, {"live": (">=", 1000)})
    for i in range(40):                                                                   # 9
        M, off = random_map(i)
        add("random%02d" % i, 9, gray, M, off, wc.OUT, {"live": (">=", 1000), "interior_wide": (">=", 1000)})
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


check_expect = wc.check_expect

#: the representative cases of the pointer-path tests
POINTER_CASES = ["c1-zoom_corner", "c1-rot30", "c2-lo_lo", "c2-hi_hi", "c9-random03"]


# ------------------------------------------------------------------------------------------------------------------ stacks
_STACKS = None


def stack_cases():
    """[stack_cases.Case], mode 1 throughout; every one is run with reducers_of(case)"""
    global _STACKS
    if _STACKS is None:
        out = []
        O0, O1, O2 = sc.OUTS
        for i, S in enumerate(SIZES):                                          # every size: coverage from 0 to S, two tile columns
            out.append(sc.make("noise", "leaving", S, O1, seed=200 + i))
            out.append(sc.make(sc.KINDS[1 + i % (len(sc.KINDS) - 1)], "half", S, O0, seed=210 + i))
        for kind in sc.KINDS:                                                  # every value family under an exact and a mixing map
            out.append(sc.make(kind, "shift", 5, O0, seed=220)._replace(mode=1))
            out.append(sc.make(kind, "rot", 4, O1, seed=221)._replace(mode=1))
        for family in STACK_MAPS:                                              # every map family
            if family != "leaving":                                            # (already there for every size)
                out.append(sc.make("noise", family, 5, O1, seed=230))
            out.append(sc.make("ties", family, 8, O0 if family != "leaving" else O2, seed=231))
        out.append(sc.make("zinger", "half", 64, O1, seed=240))
        out.append(sc.make("noise", "nan_some", 64, O0, seed=241))
        out.append(sc.make("noise", "leaving", BIG_S, O1, seed=250))           # more than a median takes
        out.append(sc.make("order", "half", BIG_S, O0, seed=251))
        out = [c._replace(mode=1, name=c.name.replace("-m0", "-m1")) for c in out]
        names = [c.name for c in out]
        assert len(set(names)) == len(names), names
        _STACKS = out
    return _STACKS


def ranks_pinned(case):
    """whether the order of the samples is the same on every platform: no NaN that the sampler creates"""
    return case.kind != "inf" and (case.kind != "big" or case.family in ("identity", "shift"))


def reducers_of(case):
    r = ["sum", "mean"]
    if len(case.frames) <= 64 and ranks_pinned(case):
        r.append("median")
    return tuple(r)


#: the rejections every clip stack is run with: (label, keywords of stack_clip_ref.reduce_clip)
CLIPS = (
    ("trim0_0", dict(reject="trim", trim=(0, 0))),                             # nothing rejected: the cubic mean bit for bit
    ("trim1_1", dict(reject="trim", trim=(1, 1))),
    ("trim2_3", dict(reject="trim", trim=(2, 3))),
    ("sigma1.5", dict(reject="sigma", kappa=(1.5, 1.5), iters=3)),
    ("sigma3", dict(reject="sigma", kappa=(3.0, 3.0), iters=2)),
)


def clip_stacks():
    """the stacks of at most 64 frames whose sample order is pinned"""
    return [c for c in stack_cases() if len(c.frames) <= 64 and ranks_pinned(c)]


def clip_weights(case, label):
    """distinct weights where equal keys have to be told apart, mixed ones on the sigma rule of the noise stacks, else none"""
    S = len(case.frames)
    if case.kind == "ties":
        return scc.distinct_weights(S)
    if case.kind == "noise" and label == "sigma1.5":
        return scc.mixed_weights(S)
    return None
