"""The contract of siftmi_batch_stack (include/siftmi.h) restated in numpy, written from the
contract text, for tests/test_stack_ref_host.py and tests/test_gpu_stack.py.  Nothing here imports the package: the GPU results
are compared with what this file computes, bit for bit.

Per output pixel (x, y), binary32 throughout, one rounding per operation:
    v_s     = the warp's value for frame s (warp_ref.warp_ref: taps beside the image replaced by fills[s] and all)
    live_s  = 0 <= tx && tx < (float)W + -0.5f && 0 <= ty && ty < (float)H + -0.5f       (ty, tx) = warp_ref.coords; false for NaN
    c       = number of live frames (int32)
    sum     over the live frames in ascending s: acc = v for the first, acc = acc + v for each later one
    mean    acc / (float)c
    median  lo, hi = the live values of rank (c - 1) >> 1 and c >> 1 in ascending shift_ref.key order;
            c odd: lo, c even: (lo + hi) * 0.5f                                         (shift_ref.middle's rule)
    c == 0  `empty`
"""
import numpy as np

from shift_ref import key, unkey
from warp_ref import coords, warp_ref

F = np.float32
REDUCERS = ("sum", "mean", "median")
MEDIAN_MAX = 64


def live_mask(M, off, shape, out_shape):
    """where frame (M, off) of `shape` = (H, W) is live on the output grid"""
    H, W = shape
    ty, tx = coords(M, off, out_shape)
    with np.errstate(all="ignore"):
        return (F(0) <= tx) & (tx < F(W) + F(-0.5)) & (F(0) <= ty) & (ty < F(H) + F(-0.5))


def samples(frames, maps, fills, shape, out_shape, mode=1):
    """(values float32 (S, OH, OW), live bool (S, OH, OW)): every frame warped on its own, and where it counts"""
    S = len(frames)
    vals = np.empty((S,) + tuple(out_shape), F)
    live = np.zeros((S,) + tuple(out_shape), bool)
    for s in range(S):
        M, off = maps[s]
        assert frames[s].shape == tuple(shape)
        vals[s] = warp_ref(frames[s], M, off, tuple(out_shape), fills[s], mode)[0]
        live[s] = live_mask(M, off, shape, out_shape)
    return vals, live


def ordered_sum(vals, live, order=None):
    """(acc float32, c int32): the contract's sum, frame after frame in `order` (default: ascending s)"""
    acc = np.zeros(vals.shape[1:], F)
    c = np.zeros(vals.shape[1:], np.int32)
    with np.errstate(all="ignore"):
        for s in (range(vals.shape[0]) if order is None else order):
            acc = np.where(live[s], np.where(c == 0, vals[s], acc + vals[s]), acc)
            c = c + live[s].astype(np.int32)
    assert acc.dtype == F and c.dtype == np.int32
    return acc, c


def reduce_samples(vals, live, reduce="mean", empty=np.nan):
    """(plane float32, coverage int32) from the samples of every frame"""
    assert reduce in REDUCERS
    acc, c = ordered_sum(vals, live)
    covered = c > 0
    with np.errstate(all="ignore"):
        if reduce == "sum":
            plane = acc
        elif reduce == "mean":
            plane = acc / np.where(covered, c, 1).astype(F)
        else:
            assert vals.shape[0] <= MEDIAN_MAX
            # the keys of the live samples in ascending order, the others behind them
            k = np.sort(np.where(live, key(vals).astype(np.uint64), np.uint64(1) << np.uint64(32)), axis=0, kind="stable")
            if k.shape[0] == 0:
                k = np.zeros((1,) + vals.shape[1:], np.uint64)
            pick = lambda r: unkey(np.take_along_axis(k, np.where(covered, r, 0)[None].astype(np.int64), axis=0)[0].astype(np.uint32))  # noqa: E731
            lo, hi = pick((c - 1) >> 1), pick(c >> 1)
            plane = np.where(c & 1, lo, (lo + hi) * F(0.5))
    plane = np.where(covered, plane, F(empty)).astype(F)
    return plane, c


def stack_ref(frames, maps, fills, shape, out_shape, mode=1, reduce="mean", empty=np.nan):
    """(plane, coverage) of the contract for S frames of `shape`, maps [(M, off)] and S fill values"""
    vals, live = samples(frames, maps, fills, shape, out_shape, mode)
    return reduce_samples(vals, live, reduce, empty)
