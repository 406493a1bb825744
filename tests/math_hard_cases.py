"""The hard arguments of siftmath's fast paths (tests/golden/math_hard.npz): what the fixture's labels mean.

siftmath's device fast paths (expf_fast_try, atan2f_fast_try) evaluate in binary64 with an error of at most 2^-45 relative --
at most 256 ulps of the binary64 value -- and may be used only where the value is farther than 8192 ulps from every binary32
round-to-nearest boundary; elsewhere the defining function is evaluated.  A random argument almost never comes near that rule,
so the fixture holds arguments found by search (tests/golden/make_math_hard.py), labelled by the distance d of the DEFINING
function's binary64 value (oracle.expf_f64_array / atan2f_f64_array, oracle.boundary_distance) from the boundary:

    H0    d <= 64                     the fast value may round to the other side: the guard must refuse
    H1    64 < d <= 8192 - 512        the guard must refuse (512: twice the fast paths' claimed error)
    G     8192 - 512 < d <= 8192 + 512  either answer; the returned value is the defining function's
    S     8192 + 512 < d <= 65536     the guard must accept, and the candidate is already the defining function's value

Strata.  exp: (a) window weights, x in [-12, 0]; (b) the end of the reduction interval, x within 0.0166 of (k + 1/2) ln 2 for
k = -115 .. 114, so that |r| > 0.33, where the truncated polynomial is least accurate; (c) wide, |x| <= 80 with a uniform
exponent from 2^-30 on and both signs, plus 80.0f and its two inner neighbours (no band claimed).
atan2: (a) gradient-like, differences of two values of [0, 255] with 8 .. 24 significant bits; (b) the ends of the octant
intervals, min / max within 2^-10 of (k + 1/2) / 8 for k = 0 .. 7, in all four folds; (c) range edges, one operand at 1e18f /
1e-18f or one of the two floats next to it inside the guarded range, the other comparable (ratio >= 2^-5) or far (down to 2^-119).
The exp strata are finite sets of floats, small against the rarity of the bands, so the generator walks every float of them
and the fixture holds ALL arguments of a band where fewer exist than MIN_COUNT asks for (EXP_AVAILABLE: [-12, 0] holds 50
floats within 64 ulps, not 200; the windows of stratum (b) hold 7 * 10^6 floats and so 2 / 196 / 31 / 1664 arguments in the
four bands).  atan2 operand pairs are plentiful and are drawn at random until every band is full.
Range cases are stored apart: arguments outside the guarded range, for which the fast path must say "not usable".
"""
import os

import numpy as np

H0, H1, G, S, NO_BAND = 0, 1, 2, 3, 4
BAND_NAMES = {H0: "H0", H1: "H1", G: "G", S: "S", NO_BAND: "none"}
GUARD = 8192                    # siftmath::f32_rounding_is_safe
MARGIN = 512                    # twice 2^-45 relative, in ulps of a binary64 value (2^-45 / 2^-53 = 256 at most)
D_MAX = 65536
MIN_COUNT = {H0: 200, H1: 3000, G: 1500, S: 6000}
# exp: the number of floats that exist in a stratum's band, where that is below MIN_COUNT (counted by walking every float,
# tests/golden/make_math_hard.py; test_math_hard_host.py walks stratum (b) again)
EXP_AVAILABLE = {(0, H0): 50, (0, G): 943, (1, H0): 2, (1, H1): 196, (1, G): 31, (1, S): 1664, (2, H0): 119}
LN2 = float.fromhex("0x1.62e42fefa39efp-1")
LOG2E = float.fromhex("0x1.71547652b82fep+0")
F32_MIN_NORMAL = np.float32(2.0 ** -126)

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "math_hard.npz")


def band_of(d):
    d = np.asarray(d)
    return np.select([d <= 64, d <= GUARD - MARGIN, d <= GUARD + MARGIN, d <= D_MAX], [H0, H1, G, S], NO_BAND)


def load():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def step(f, ulps):
    """float32 f (positive) moved by `ulps` floats"""
    return (np.array([f], np.float32).view(np.uint32) + np.uint32(ulps & 0xffffffff)).view(np.float32)[0]


# ----------------------------------------------------------------------------- the guarded ranges, as siftmath.hpp states them
def exp_in_range(x):
    return np.abs(x) <= np.float32(80.0)          # false for NaN


def atan2_in_range(y, x):
    ay, ax = np.abs(y), np.abs(x)
    with np.errstate(invalid="ignore"):
        return (ax <= np.float32(1e18)) & (ay <= np.float32(1e18)) & (np.fmin(ax, ay) >= np.float32(1e-18)) & ~np.isnan(ax) & ~np.isnan(ay)


# ----------------------------------------------------------------------------- labels recomputed from the arguments
def exp_reduction(x):
    """(k, r) of the argument reduction x = k ln2 + r, in binary64"""
    x = np.asarray(x, np.float64)
    k = np.rint(x * LOG2E)
    return k.astype(np.int64), x - k * LN2


def exp_window(x):
    """stratum (b): (k, x - (k + 1/2) ln 2) of the window centre nearest to x; the stratum is |offset| <= 0.0166, -115 <= k <= 114"""
    x = np.asarray(x, np.float64)
    k = np.rint(x * (1.0 / LN2) - 0.5)
    return k.astype(np.int64), x - (k + 0.5) * LN2


def exp_window_floats():
    """every float32 of stratum (b), ascending by bit pattern within each sign"""
    out = []
    for k in range(-115, 115):
        c = (k + 0.5) * LN2
        lo, hi = np.float32(c - 0.0167), np.float32(c + 0.0167)
        a, b = sorted(int(np.array([v], np.float32).view(np.uint32)[0]) for v in (lo, hi))
        out.append(np.arange(a, b + 1, dtype=np.uint32).view(np.float32))
    x = np.concatenate(out)
    kk, off = exp_window(x)
    return x[(np.abs(off) <= 0.0166) & (kk >= -115) & (kk <= 114)]


def atan2_fold(y, x):
    """fold = (|y| > |x|) + 2 (x < 0), the octant index k = int(8 min / max + 0.5) of the exactly rounded float quotient, and
    t = (min - c max) / (max + c min), c = k / 8"""
    ay, ax = np.abs(y).astype(np.float32), np.abs(x).astype(np.float32)
    swap = ay > ax
    mn, mx = np.where(swap, ax, ay), np.where(swap, ay, ax)
    k = (mn / mx * np.float32(8.0) + np.float32(0.5)).astype(np.int64)
    c = k * 0.125
    t = (mn.astype(np.float64) - c * mx) / (mx + c * mn)
    return swap.astype(np.int64) + 2 * np.signbit(x).astype(np.int64), k, t


def sign_combo(y, x):
    return np.signbit(y).astype(np.int64) + 2 * np.signbit(x).astype(np.int64)


# ----------------------------------------------------------------------------- crafted cases
def exp_edge_inside():
    """80.0f and its two neighbours inside the guarded range, both signs"""
    v = np.array([step(80.0, -2), step(80.0, -1), np.float32(80.0)], np.float32)
    return np.concatenate([v, -v])


def exp_range_cases():
    """outside |x| <= 80: the two floats past 80.0f, the defining function's own range tests (89, -104), results that are
    sub-normal in binary32 or flush to zero, huge arguments, infinities, NaN"""
    v = np.array([step(80.0, 1), step(80.0, 2), 80.5, 81.0, 87.0, 88.5, 88.72284, 89.0, step(89.0, 1), 90.0, 1e30, np.inf], np.float32)
    w = np.array([-87.0, -87.33655, -87.4, -88.0, -95.0, -103.0, -103.9, step(104.0, -1) * -1, -104.0, -step(104.0, 1), -104.5, np.nan], np.float32)
    return np.concatenate([v, -v[:4], -v[-2:], w])


def atan2_range_cases():
    """outside the guarded range of atan2f_fast_try: an operand above 1e18f, a smaller operand below 1e-18f (the floats next to
    either limit, the other operand comparable or far), zeros, sub-normal results and operands, infinities, NaN"""
    big = [step(1e18, 1), step(1e18, 2), np.float32(2e18), np.float32(3e38)]
    small = [step(1e-18, -1), step(1e-18, -2), np.float32(5e-19), np.float32(1e-30), np.float32(1e-45)]
    ys, xs = [], []
    for p in big:                                     # the other operand: comparable, far, at the other limit
        for o in (p * np.float32(0.75), np.float32(1e18), np.float32(7.0), np.float32(1e-18), np.float32(3e-20)):
            ys += [p, o]; xs += [o, p]
    for p in small:
        for o in (p * np.float32(1.5), np.float32(1e-18), np.float32(0.3), np.float32(1e18), np.float32(2e18)):
            ys += [p, o]; xs += [o, p]
    # results below the binary32 normal range (y / x < 2^-126) and at its edge
    for y, x in ((1e-21, 1e18), (1e-30, 1e10), (1e-38, 1.0), (1.1754944e-38, 2.0), (1e-45, 1.0), (3e-20, 1e18), (1e-44, 1e-6)):
        ys.append(np.float32(y)); xs.append(np.float32(x))
    y = np.array(ys, np.float32); x = np.array(xs, np.float32)
    y = np.concatenate([y, -y, y, -y]); x = np.concatenate([x, x, -x, -x])
    z, o, i, n = np.float32(0.0), np.float32(1.0), np.float32(np.inf), np.float32(np.nan)
    special = [(z, z), (-z, z), (z, -z), (-z, -z), (z, o), (-z, o), (z, -o), (-z, -o), (o, z), (-o, z), (o, -z), (-o, -z),
               (i, o), (o, i), (-i, o), (o, -i), (i, i), (i, -i), (i, z), (z, i), (n, o), (o, n), (n, n), (n, z), (n, i)]
    return (np.concatenate([y, np.array([s[0] for s in special], np.float32)]),
            np.concatenate([x, np.array([s[1] for s in special], np.float32)]))
