"""Crafted stacks for the stack reduction (siftmi_batch_stack: stack_reduce_kernel / stack_median_kernel in csrc/k_stack.hpp),
shared by tests/test_stack_ref_host.py and tests/test_gpu_stack.py.  numpy only.

Frames are 37 x 53 and the outputs 37 x 53, 41 x 70 (two tile columns of 64, eleven tile rows of 4 with a ragged last one) and
1 x 1: the smallest shapes that cross a tile edge in both directions.  A case is a stack, its maps and fills, an output shape and
a mode; every case is run with every reducer (the median up to 64 frames).

Map families                                                   Value families
  identity   every frame onto itself                             noise      random values of mixed sign and size
  shift      integer shifts: the samples are the pixels          order      1e8, 1, -1e8, 1, ...: the float32 sum depends on the order
  half       half-pixel shifts                                   ties       seven values, many equal
  rot        a small rotation about the centre                   zeros      +0.0 and -0.0
  leaving    frame s pushed s * 52 / (S - 1) pixels out of       subnormal  multiples of 1.4e-45
             view: coverage runs from S down to 0 across a row   inf        +-inf planted; +inf and -inf meet in some pixels (mode 0)
  rising     the same downwards, from the top edge               big        +-3e38: lo + hi and the sum overflow
  nan_mid / nan_ends / nan_some   NaN maps inside, at both       nan        NaN pixels, positive in even and negative in odd frames
             ends, at several places of the stack                zinger     one smooth plane in every frame, one outlier per
  nan_all    every map NaN: nothing is live                                 frame, each at a pixel of its own
"""
import collections

import numpy as np

F = np.float32
SHAPE = (37, 53)                                 # H, W of every frame
OUTS = ((37, 53), (41, 70), (1, 1))
SIZES = (1, 2, 3, 4, 5, 8, 63, 64)
BIG_S = 200                                      # sum and mean have no cap
KINDS = ("noise", "order", "ties", "zeros", "subnormal", "inf", "big", "nan", "zinger")
MAPS = ("identity", "shift", "half", "rot", "leaving", "rising", "nan_mid", "nan_ends", "nan_some", "nan_all")
ZINGER = F(60000.0)

Case = collections.namedtuple("Case", "name frames maps fills out_shape mode kind family")
IDENT = ((1.0, 0.0, 0.0, 1.0), (0.0, 0.0))
NANMAP = ((np.nan,) * 4, (np.nan,) * 2)


def base_plane():
    """a smooth plane of small integers: sums of up to 2 ** 16 of them are exact"""
    y, x = np.mgrid[0:SHAPE[0], 0:SHAPE[1]]
    return (40 + 3 * y + 2 * x + ((x * y) % 7)).astype(F)


def zinger_pixel(s):
    """(row, column) of frame s's outlier: all different for s < 64"""
    return (s % 64) // 8 * 4 + 2, (s % 8) * 6 + 3


def frames_of(kind, S, seed=0):
    rng = np.random.default_rng(1000 + seed)
    H, W = SHAPE
    out = []
    for s in range(S):
        if kind == "noise":
            f = (rng.normal(0.0, 1.0, SHAPE) * 10.0 ** rng.integers(-3, 6, SHAPE)).astype(F)
        elif kind == "order":
            f = np.full(SHAPE, (1e8, 1.0, -1e8, 1.0)[s % 4], F)
        elif kind == "ties":
            f = F([-3.5, -1.0, -0.0, 0.0, 0.25, 2.0, 1e30])[rng.integers(0, 7, SHAPE)]
        elif kind == "zeros":
            f = np.where(rng.random(SHAPE) < 0.5, F(-0.0), F(0.0)).astype(F)
        elif kind == "subnormal":
            f = rng.integers(-200, 200, SHAPE).astype(F) * F(1.4e-45)
        elif kind == "inf":                                          # (always sampled with the nearest-lower tap, see make())
            f = rng.normal(0.0, 5.0, SHAPE).astype(F)
            f[rng.random(SHAPE) < 0.08] = np.inf if s % 2 == 0 else -np.inf
            f[rng.random(SHAPE) < 0.04] = -np.inf if s % 2 == 0 else np.inf
        elif kind == "big":
            f = np.where(rng.random(SHAPE) < 0.5, F(3e38), F(-3e38)).astype(F)
            f[rng.random(SHAPE) < 0.3] = F(3e38)
        elif kind == "nan":                                          # one sign per frame: a bilinear sample mixes taps of ONE frame
            f = rng.normal(0.0, 5.0, SHAPE).astype(F)
            f.view(np.uint32)[rng.random(SHAPE) < 0.15] = (0x7fc00000, 0xffc00001)[s % 2] + s      # +NaN: above +inf; -NaN: below -inf
        elif kind == "zinger":
            f = base_plane()
            f[zinger_pixel(s)[0], zinger_pixel(s)[1]] = ZINGER
        else:
            raise ValueError(kind)
        out.append(np.ascontiguousarray(f, F))
    return out


def maps_of(family, S):
    """[(M, off)] of S frames; M acts on (y, x), off = (dy, dx), as the warp takes them"""
    H, W = SHAPE
    if family == "identity":
        return [IDENT] * S
    if family == "shift":
        return [((1.0, 0.0, 0.0, 1.0), (float((3 * s) % 7 - 3), float((5 * s) % 9 - 4))) for s in range(S)]
    if family == "half":
        return [((1.0, 0.0, 0.0, 1.0), ((s % 5) - 2 + 0.5, (s % 3) - 1 - 0.5)) for s in range(S)]
    if family == "rot":
        out = []
        for s in range(S):
            t = np.deg2rad(1.5 * ((s % 7) - 3))
            c, si = np.cos(t), np.sin(t)
            cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
            out.append(((c, -si, si, c), (cy - c * cy + si * cx, cx - si * cy - c * cx)))
        return out
    if family == "leaving":                      # tx = x + dx_s: live while tx < W - 0.5; dx_0 = 0 (all of the row), dx_last = W - 1
        return [((1.0, 0.0, 0.0, 1.0), (0.0, s * (W - 1.0) / max(S - 1, 1))) for s in range(S)]
    if family == "rising":                       # ty = y - dy_s: live from row dy_s on
        return [((1.0, 0.0, 0.0, 1.0), (-(s * (H - 1.0) / max(S - 1, 1)), 0.25)) for s in range(S)]
    base = maps_of("shift", S)
    if family == "nan_mid":
        dead = {S // 2}
    elif family == "nan_ends":
        dead = {0, S - 1}
    elif family == "nan_some":
        dead = {0, S - 1} | set(range(1, S, 3))
    elif family == "nan_all":
        dead = set(range(S))
    else:
        raise ValueError(family)
    # one NaN coefficient is enough where it reaches every pixel (an offset); the all-NaN map is align_batch's mode 0
    return [NANMAP if (s in dead and s % 2 == 0) else (((1.0, 0.0, 0.0, 1.0), (np.nan, 1.0)) if s in dead else base[s]) for s in range(S)]


def fills_of(S):
    return np.array([(-7.5, 0.0, 13.25, 1e6)[s % 4] for s in range(S)], F)


def make(kind, family, S, out_shape, mode=1, seed=0):
    """A NaN that the warp's own arithmetic creates (0 * inf, inf - inf) has the sign of the hardware's default NaN -- negative
    on x86, positive on gfx950 -- and with it another place in the median's order.  Only NaNs that come from the frames are
    pinned: frames with infinities are sampled with the nearest-lower tap (the sample is the pixel), and the NaNs of one frame
    share a sign, so whichever operand a bilinear sample propagates, the sign is that one."""
    if kind == "inf":
        mode = 0
    name = "%s-%s-S%d-%dx%d-m%d" % (kind, family, S, out_shape[0], out_shape[1], mode)
    return Case(name, frames_of(kind, S, seed), maps_of(family, S), fills_of(S), tuple(out_shape), mode, kind, family)


_CASES = None


def cases():
    """every case, built once"""
    global _CASES
    if _CASES is None:
        out = []
        # every stack size: coverage from 0 to S across the plane, on the output with two tile columns and a ragged last row
        for i, S in enumerate(SIZES):
            out.append(make("noise", "leaving", S, OUTS[1], seed=i))
            out.append(make(KINDS[1 + i % (len(KINDS) - 1)], "shift", S, OUTS[0], seed=i))
            out.append(make("noise", "rising", S, OUTS[2] if S in (3, 64) else OUTS[0], seed=10 + i))
        # every value family on an odd and an even stack, exact samples
        for kind in KINDS:
            out.append(make(kind, "identity", 5, OUTS[0], seed=20))
            out.append(make(kind, "shift", 8, OUTS[1], seed=21))
        out.append(make("zinger", "shift", 64, OUTS[1], seed=22))
        out.append(make("order", "leaving", 64, OUTS[1], seed=23))
        # every map family
        for S in (4, 5):
            for family in MAPS:
                if family != "leaving":              # (already there for every size)
                    out.append(make("noise", family, S, OUTS[1], seed=30 + S))
        out.append(make("ties", "nan_some", 63, OUTS[1], seed=40))
        out.append(make("noise", "nan_all", 64, OUTS[0], seed=41))
        # the nearest-lower tap
        out.append(make("noise", "half", 5, OUTS[1], mode=0, seed=50))
        out.append(make("ties", "rot", 8, OUTS[0], mode=3, seed=51))
        out.append(make("zeros", "identity", 3, OUTS[0], mode=0, seed=52))
        # more frames than a median takes: sum and mean only
        out.append(make("noise", "leaving", BIG_S, OUTS[1], seed=60))
        out.append(make("order", "shift", BIG_S, OUTS[0], seed=61))
        names = [c.name for c in out]
        assert len(set(names)) == len(names)
        _CASES = out
    return _CASES


def reducers_of(case):
    return ("sum", "mean", "median") if len(case.frames) <= 64 else ("sum", "mean")
