"""Crafted inputs of the streaming stack accumulator (siftmi_batch_stack_accum; csrc/k_stack_accum.hpp), shared by
tests/test_stack_accum_ref_host.py and tests/test_gpu_stack_accum.py.  numpy only.  Frames and maps are tests/stack_cases.py's.

The stack of the LinearAlign.stack_stream tests is test_gpu_stack.py's recipe with 12 frames: a 320 x 320 smooth_noise plane
scaled to [0, 30000], the reference its 256 x 256 centre crop, the frames crops at integer offsets within +-8 pixels.  Every frame
carries ONE zinger of 60000 (the plane's hi + (hi - lo), as there), each in a 16-pixel cell of its own in the reference's
coordinates, and noise of its own.

The noise, and why it is what it is.  stack_stream(reject="sigma") must drop the zinger and nothing else wherever at least 11
frames cover a pixel.  A zinger among n - 1 samples of the plane has z * z = (n - 1) ** 2 / n of its own making: 10.08 at n = 12 and
9.09 at n = 11, above kappa * kappa = 9 -- the samples' own spread must stay small beside the zinger's 30000 or more, or the 1 %
margin at n = 11 is gone.  At the other pixels no sample may reach z = 3.  z-scores do not depend on the noise's scale, and among
12 normal samples about 3 pixels in 10000 hold one above 3, and independent uniform noise still left 4 of 58790 pixels with one:
independent noise fails at every level.  So the noise is balanced instead: a pixel of the plane carries, over the 12 frames, the
12 levels -30, -24.5, ..., 30 once each, in an order of its own (a random start, frame s takes level (start + s) mod 12).  Twelve
such samples have no z above 11 / sqrt(143 / 3) = 1.6, eleven of them none above 2.  The half-width of 30 is far above what an
estimated map that is off by 1e-4 pixels leaks of a zinger into its neighbours (6) or moves a sample along the plane's slope
(below 1), so the neighbours of a zinger stay, and it is a thousandth of the plane's range, so the keypoints do not notice.
tests/test_stack_accum_ref_host.py checks all of this on the restatement alone.
"""
import numpy as np

import stack_cases as sc

F = np.float32
CALLS = (None, 1, 3, 4, 5)                        # frames per call: all at once, or the edges of the depth-4 and depth-2 groups
SIZES = (1, 2, 3, 4, 5, 8, 64, 200)
STREAM_OFFSETS = [(0, 0), (5, -3), (-8, 8), (2, 7), (-6, -5), (8, 1), (-1, -8), (4, 4), (-3, 6), (7, -7), (-5, 2), (1, -2)]
STREAM_ZINGER = F(60000.0)
STREAM_NOISE = 30.0                               # half-width of the balanced noise
_cache = {}


def splits(S, per_call):
    """[(first, last)) of every call"""
    if per_call is None:
        return [(0, S)]
    return [(a, min(a + per_call, S)) for a in range(0, S, per_call)]


def integer_stack(S, seed=0):
    """S frames of whole numbers |v| < 2 ** 10: every partial sum of up to 2 ** 14 of them is exact in binary32"""
    rng = np.random.default_rng(7000 + seed)
    return [rng.integers(-1023, 1024, sc.SHAPE).astype(F) for _ in range(S)]


def stream_stack():
    """(reference crop, the 12 clean frames -- noise included --, the same frames with one zinger each, the zingers' (row, column)
    in the reference's coordinates)"""
    if "stream" not in _cache:
        from util import smooth_noise
        big = smooth_noise((320, 320), seed=21, sigma=2.0).astype(np.float64)
        big = ((big - big.min()) / (big.max() - big.min()) * 30000.0).astype(F)
        ref = np.ascontiguousarray(big[32:288, 32:288])
        cells = [(32 + 16 * i, 32 + 16 * j) for i in range(12) for j in range(12)]       # in the reference's coordinates
        rng = np.random.default_rng(8)
        order = rng.permutation(len(cells))[:len(STREAM_OFFSETS)]
        levels = np.linspace(-STREAM_NOISE, STREAM_NOISE, len(STREAM_OFFSETS)).astype(F)
        start = rng.integers(0, len(levels), big.shape)
        clean, dirty, where = [], [], []
        for s, (dy, dx) in enumerate(STREAM_OFFSETS):
            noise = levels[(start + s) % len(levels)]                     # on the plane: the same pixel, another level in every frame
            f = big[32 + dy:288 + dy, 32 + dx:288 + dx] + noise[32 + dy:288 + dy, 32 + dx:288 + dx]
            f = np.ascontiguousarray(f, F)
            yr, xr = cells[order[s]][0] + int(rng.integers(-3, 4)), cells[order[s]][1] + int(rng.integers(-3, 4))
            g = f.copy()
            g[yr - dy, xr - dx] = STREAM_ZINGER
            clean.append(f); dirty.append(g); where.append((yr, xr))
        _cache["stream"] = (ref, clean, dirty, where)
    return _cache["stream"]


def stream_ideal_maps():
    """the maps a perfect estimate would return: frame pixel (i, j) is the reference's (i + dy, j + dx)"""
    return [((1.0, 0.0, 0.0, 1.0), (-float(dy), -float(dx))) for dy, dx in STREAM_OFFSETS]
