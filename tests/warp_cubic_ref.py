"""The contract of the cubic sampler (include/siftmi.h: SIFTMI_INTERP_CUBIC; csrc/k_warp_cubic.hpp)
restated in vectorised numpy, written from the contract text, for tests/test_warp_cubic_ref_host.py and
tests/test_gpu_warp_cubic.py.  Binary32 throughout; every product, sum and difference is rounded on its own, in the order written.

    (ty, tx)   warp_ref.coords: ty = (m0*y + m1*x) + off0, tx = (m2*y + m3*x) + off1
    live       0 <= tx && tx < (float)W + -0.5f && 0 <= ty && ty < (float)H + -0.5f        (false for NaN; no index unless live)
    !live      out = fill
    xp = (int)tx, yp = (int)ty;  fx = tx - (float)xp,  fy = ty - (float)yp
    columns    c_k = clamp(xp - 1 + k, 0, W - 1),  rows r_j = clamp(yp - 1 + j, 0, H - 1),  j, k = 0..3
    weights    w0 = ((-0.5f*f + 1.0f)*f - 0.5f)*f        w1 = ((1.5f*f - 2.5f)*f)*f + 1.0f
               w2 = ((-1.5f*f + 2.0f)*f + 0.5f)*f        w3 = ((0.5f*f - 0.5f)*f)*f
    rows       R_j = ((wx0*p[r_j][c_0] + wx1*p[r_j][c_1]) + wx2*p[r_j][c_2]) + wx3*p[r_j][c_3]
    value      out = ((wy0*R_0 + wy1*R_1) + wy2*R_2) + wy3*R_3

The `rule` argument of warp_cubic_ref swaps ONE of these rules for a plausible wrong one (MUTANTS): the host test shows that each
of them changes a dictated result, i.e. that the cases can tell the contract from its neighbours.

numpy only; nothing here imports the package or the oracle.
"""
import numpy as np

import stack_ref
import warp_ref
from warp_ref import coords

F = np.float32
CLASSES = ("live", "inside_not_live", "clamp_x_lo", "clamp_x_hi1", "clamp_x_hi2", "clamp_y_lo", "clamp_y_hi1", "clamp_y_hi2", "corner",
           "integer", "interior_wide")
MUTANTS = ("fma_row", "vertical_first", "fill_tap", "clamp_w", "live_inside", "expanded_weights", "floor_double", "a075")


def weights(f, rule=None):
    """(w0, w1, w2, w3) of the fraction f (float32 array), Horner form as the contract writes it"""
    f = np.asarray(f, F)
    with np.errstate(all="ignore"):
        if rule == "expanded_weights":
            f2 = f * f
            f3 = f2 * f
            return (F(-0.5) * f3 + f2 - F(0.5) * f, F(1.5) * f3 - F(2.5) * f2 + F(1.0), F(-1.5) * f3 + F(2.0) * f2 + F(0.5) * f,
                    F(0.5) * f3 - F(0.5) * f2)
        if rule == "a075":                         # a = -3/4, OpenCV's INTER_CUBIC
            a = F(-0.75)
            return (((a * f - F(2) * a) * f + a) * f, ((a + F(2)) * f - (a + F(3))) * f * f + F(1.0),
                    ((-(a + F(2)) * f + (F(2) * a + F(3))) * f - a) * f, ((-a * f + a) * f) * f)
        w0 = ((F(-0.5) * f + F(1.0)) * f - F(0.5)) * f
        w1 = ((F(1.5) * f - F(2.5)) * f) * f + F(1.0)
        w2 = ((F(-1.5) * f + F(2.0)) * f + F(0.5)) * f
        w3 = ((F(0.5) * f - F(0.5)) * f) * f
    for w in (w0, w1, w2, w3):
        assert w.dtype == F
    return w0, w1, w2, w3


def _dot4(w, p, fma=False):
    """((w0*p0 + w1*p1) + w2*p2) + w3*p3 in float32; fma: the whole sum rounded exactly once (from float64: the products of two
    float32 are exact there and the sum of four stays within its 53 bits for the magnitudes the cases use)"""
    with np.errstate(all="ignore"):
        if fma:
            return sum(w[k].astype(np.float64) * p[k].astype(np.float64) for k in range(4)).astype(F)
        return ((w[0] * p[0] + w[1] * p[1]) + w[2] * p[2]) + w[3] * p[3]


def warp_cubic_ref(image, M, off, out_shape=None, fill=0.0, rule=None):
    """(out, counts): the cubic warp of `image` (H x W float32) and the number of output pixels in each class of CLASSES (every
    class but inside_not_live counts live pixels)"""
    assert rule is None or rule in MUTANTS
    image = np.ascontiguousarray(image)
    assert image.dtype == F and image.ndim == 2
    H, W = image.shape
    OH, OW = out_shape or (H, W)
    fill = F(fill)
    ty, tx = coords(M, off, (OH, OW))
    with np.errstate(all="ignore"):
        inside = (F(0) <= tx) & (tx < F(W)) & (F(0) <= ty) & (ty < F(H))
        live = (F(0) <= tx) & (tx < F(W) + F(-0.5)) & (F(0) <= ty) & (ty < F(H) + F(-0.5))
        use = inside if rule == "live_inside" else live
        # truncation toward zero only where the point is used: 0 <= t < 2^24, so the cast is exact and defined
        xp = np.where(use, tx, F(0)).astype(np.int64)
        yp = np.where(use, ty, F(0)).astype(np.int64)
        if rule == "floor_double":                 # the fraction from coordinates formed in double, rounded once at the end
            m = [float(F(v)) for v in np.asarray(M, F).reshape(4)]
            o = [float(F(v)) for v in np.asarray(off, F).reshape(2)]
            y64, x64 = np.arange(OH, dtype=np.float64)[:, None], np.arange(OW, dtype=np.float64)[None, :]
            tx64, ty64 = (m[2] * y64 + m[3] * x64) + o[1], (m[0] * y64 + m[1] * x64) + o[0]
            fx = (tx64 - np.floor(tx64)).astype(F)
            fy = (ty64 - np.floor(ty64)).astype(F)
            fx = np.where(use, fx, F(0)); fy = np.where(use, fy, F(0))
        else:
            fx = np.where(use, tx, F(0)) - xp.astype(F)
            fy = np.where(use, ty, F(0)) - yp.astype(F)
        wx, wy = weights(fx, rule), weights(fy, rule)
        hi_x = W if rule == "clamp_w" else W - 1
        cols = [np.clip(xp - 1 + k, 0, hi_x) for k in range(4)]
        rows = [np.clip(yp - 1 + j, 0, H - 1) for j in range(4)]
        padded = np.concatenate([image, np.full((H, 1), fill, F)], axis=1)         # column W exists for the clamp_w mutant only

        def tap(j, k):
            v = padded[rows[j], cols[k]]
            if rule == "fill_tap":                 # taps beside the image replaced by fill, the bilinear warp's rule
                out_x = (xp - 1 + k < 0) | (xp - 1 + k > W - 1)
                out_y = (yp - 1 + j < 0) | (yp - 1 + j > H - 1)
                v = np.where(out_x | out_y, fill, v)
            return v

        p = [[tap(j, k) for k in range(4)] for j in range(4)]
        if rule == "vertical_first":
            Ck = [_dot4(wy, [p[j][k] for j in range(4)]) for k in range(4)]
            v = _dot4(wx, Ck)
        else:
            R = [_dot4(wx, p[j], fma=rule == "fma_row") for j in range(4)]
            v = _dot4(wy, R)
        out = np.where(use, v, fill).astype(F)
    cx_lo, cx_hi1, cx_hi2 = live & (xp == 0), live & (xp == W - 1), live & (xp == W - 2)
    cy_lo, cy_hi1, cy_hi2 = live & (yp == 0), live & (yp == H - 1), live & (yp == H - 2)
    counts = {
        "live": live, "inside_not_live": inside & ~live,
        "clamp_x_lo": cx_lo, "clamp_x_hi1": cx_hi1, "clamp_x_hi2": cx_hi2,
        "clamp_y_lo": cy_lo, "clamp_y_hi1": cy_hi1, "clamp_y_hi2": cy_hi2,
        "corner": (cx_lo | cx_hi1 | cx_hi2) & (cy_lo | cy_hi1 | cy_hi2),
        "integer": live & (fx == 0) & (fy == 0),
        "interior_wide": live & (xp >= 1) & (xp + 2 <= W - 1),
    }
    assert tuple(counts) == CLASSES
    return out, {k: int(m.sum()) for k, m in counts.items()}


def warp(image, M, off, out_shape=None, fill=0.0, mode=1, interp=None):
    """the warp under either sampler: "cubic" is warp_cubic_ref, None and "linear" delegate to warp_ref.warp_ref unchanged"""
    if interp == "cubic":
        assert mode == 1
        return warp_cubic_ref(image, M, off, out_shape, fill)
    assert interp in (None, "linear")
    return warp_ref.warp_ref(image, M, off, out_shape, fill, mode)


def samples_cubic(frames, maps, fills, shape, out_shape):
    """(values float32 (S, OH, OW), live bool (S, OH, OW)): stack_ref.samples under the cubic sampler; the live set is the same"""
    S = len(frames)
    vals = np.empty((S,) + tuple(out_shape), F)
    live = np.zeros((S,) + tuple(out_shape), bool)
    for s in range(S):
        M, off = maps[s]
        assert frames[s].shape == tuple(shape)
        vals[s] = warp_cubic_ref(frames[s], M, off, tuple(out_shape), fills[s])[0]
        live[s] = stack_ref.live_mask(M, off, shape, out_shape)
    return vals, live
