"""The contract of siftmi_batch_stack_clip (include/siftmi.h) restated in numpy, written from the
contract text, for tests/test_stack_clip_ref_host.py and tests/test_gpu_stack_clip.py.  It builds on stack_ref.samples and
stack_ref.ordered_sum; nothing here imports the package: the GPU results are compared with what this file computes, bit for bit.

Per output pixel, binary32 throughout, one rounding per operation; v_s, live_s, c and key() are stack_ref's, osum is
stack_ref.ordered_sum over the kept set K (ascending s, the first value starts the accumulator), K starts as the live frames:
    TRIM(n_low, n_high)     order the live samples by (key(v_s), s) ascending; h = min(n_high, c - 1), l = min(n_low, c - 1 - h);
                            the last h and the first l leave K
    SIGMA(kl, kh, iters)    kl2 = kl * kl, kh2 = kh * kh; at most `iters` passes, each: n = |K|; n < 3: stop; m = osum(v) / (float)n;
                            d_s = v_s - m; q = osum(d_s * d_s); var = q / (float)n; tl = kl2 * var; th = kh2 * var; s leaves when
                            (d_s < 0 && d_s * d_s > tl) || (d_s > 0 && d_s * d_s > th); a pass that would remove nothing stops, a
                            pass that would remove every kept sample removes none and stops
    result                  osum(w_s * v_s) / osum(w_s) over K; kept = |K|; coverage = c; c == 0: `empty`, kept 0; w_s = 1.0f
                            without weights
"""
import numpy as np

from shift_ref import key
from stack_ref import ordered_sum, samples

F = np.float32
REJECTS = ("trim", "sigma")
CLIP_MAX = 64


def trim_keep(vals, live, n_low, n_high):
    """the kept set of TRIM: bool (S, OH, OW)"""
    S = vals.shape[0]
    c = live.sum(axis=0).astype(np.int64)
    h = np.maximum(np.minimum(n_high, c - 1), 0)
    l = np.maximum(np.minimum(n_low, c - 1 - h), 0)
    # (key, s) as one number; the frames that are not live behind every live one
    s = np.arange(S, dtype=np.uint64).reshape((S,) + (1,) * (vals.ndim - 1))
    order = np.where(live, key(vals).astype(np.uint64) * np.uint64(CLIP_MAX) + s, np.uint64(1) << np.uint64(40))
    rank = np.argsort(np.argsort(order, axis=0, kind="stable"), axis=0, kind="stable")       # of a live sample among the live ones
    return live & (rank >= l[None]) & (rank < (c - h)[None])


def fused_sum(a, b, K):
    """the ordered sum of a * b over K with every step but the first fused: acc = fma(a, b, acc), rounded once (the product of two
    float32 values is exact in float64).  What a build without -ffp-contract=off may compute; the contract rounds the product"""
    acc = np.zeros(K.shape[1:], F)
    n = np.zeros(K.shape[1:], np.int32)
    with np.errstate(all="ignore"):
        for s in range(K.shape[0]):
            prod = a[s].astype(np.float64) * b[s].astype(np.float64)
            acc = np.where(K[s], np.where(n == 0, prod.astype(F), (prod + acc.astype(np.float64)).astype(F)), acc)
            n = n + K[s].astype(np.int32)
    return acc


def sigma_keep(vals, live, kl, kh, iters, fuse=(), log=None):
    """the kept set of SIGMA: bool (S, OH, OW).  `log`, a list, receives per pass that is started the bool (S, OH, OW) of what it
    removed.  fuse: "dd" computes q with fused steps (fused_sum): a variant, not the contract"""
    K = live.copy()
    kl2, kh2 = F(kl) * F(kl), F(kh) * F(kh)
    going = np.ones(vals.shape[1:], bool)
    with np.errstate(all="ignore"):
        for _ in range(iters):
            n = K.sum(axis=0).astype(np.int32)
            going = going & (n >= 3)
            nf = np.where(n > 0, n, 1).astype(F)
            m = ordered_sum(vals, K)[0] / nf
            d = vals - m[None]
            dd = d * d
            q = fused_sum(d, d, K) if "dd" in fuse else ordered_sum(dd, K)[0]
            var = q / nf
            tl, th = kl2 * var, kh2 * var
            assert d.dtype == F and dd.dtype == F and var.dtype == F and tl.dtype == F and th.dtype == F
            gone = K & (((d < 0) & (dd > tl[None])) | ((d > 0) & (dd > th[None])))
            k = gone.sum(axis=0)
            going = going & (k > 0) & (k < n)
            gone = gone & going[None]
            if log is not None:
                log.append(gone)
            K = K & ~gone
    return K


def reduce_clip(vals, live, reject="sigma", trim=(0, 1), kappa=(3.0, 3.0), iters=3, weights=None, empty=np.nan, fuse=(), log=None):
    """(plane float32, coverage int32, kept int32) from the samples of every frame"""
    assert reject in REJECTS and vals.shape[0] <= CLIP_MAX
    S = vals.shape[0]
    c = live.sum(axis=0).astype(np.int32)
    K = trim_keep(vals, live, *trim) if reject == "trim" else sigma_keep(vals, live, kappa[0], kappa[1], iters, fuse, log)
    w = np.ones(S, F) if weights is None else np.asarray(weights, F)
    assert w.shape == (S,)
    wide = np.broadcast_to(w.reshape((S,) + (1,) * (vals.ndim - 1)), vals.shape)
    with np.errstate(all="ignore"):
        num = fused_sum(wide, vals, K) if "wv" in fuse else ordered_sum(wide * vals, K)[0]
        den, kept = ordered_sum(wide, K)
        plane = num / np.where(c > 0, den, F(1))
    assert plane.dtype == F and kept.dtype == np.int32
    return np.where(c > 0, plane, F(empty)).astype(F), c, kept


def stack_clip_ref(frames, maps, fills, shape, out_shape, mode=1, **kw):
    """(plane, coverage, kept) of the contract for S frames of `shape`, maps [(M, off)] and S fill values"""
    vals, live = samples(frames, maps, fills, shape, out_shape, mode)
    return reduce_clip(vals, live, **kw)
