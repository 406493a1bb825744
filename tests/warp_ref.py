"""The contract of siftmi_plan_transform (include/siftmi.h; transform.cl:22-110 `transform`, 116-204 `transform_RGB` as the
header cites them) restated in vectorised numpy, for tests/test_warp_ref_host.py and tests/test_gpu_warp_cases.py.  Written from
the header's formula and the OpenCL text, not from the oracle's C loop (oracle/sift_oracle.c: so_transform), so that the two
are independent readings of the same kernel.

    ty = (m0 * y + m1 * x) + off0        tx = (m2 * y + m3 * x) + off1           every product and sum rounded to float32
    inside = 0 <= tx < W and 0 <= ty < H                                          (false for NaN; true for -0.0)
    mode == 1:  i1 = (tx_next - tx) * p  + (tx - tx_prev) * px                    tx_prev = (int) tx, tx_next = tx_prev + 1
                i2 = (tx_next - tx) * py + (tx - tx_prev) * pn                    px, pn = fill where tx_next >= W
                v  = (ty_next - ty) * i1 + (ty - ty_prev) * i2                    py, pn = fill where ty_next >= H
    otherwise:  v  = p                                                            (the nearest-lower tap)
    out = fill  unless inside;  out = fill  where tx >= W + -0.5f or ty >= H + -0.5f;  RGB: every channel, (uint8) v

No index is formed unless `inside` holds: tx may be NaN, infinite or beyond int32 everywhere else.

numpy only; nothing here imports the package or the oracle.
"""
import numpy as np

F = np.float32
CLASSES = ("inside", "cut_inside", "xedge", "yedge", "corner", "last2", "wide1off", "frac_x_at_last2")


def coords(M, off, out_shape):
    """(ty, tx): float32 source coordinates of every output pixel, each operation rounded on its own"""
    m0, m1, m2, m3 = (F(v) for v in np.asarray(M, F).reshape(4))
    o0, o1 = (F(v) for v in np.asarray(off, F).reshape(2))
    OH, OW = out_shape
    y = np.arange(OH, dtype=F)[:, None]
    x = np.arange(OW, dtype=F)[None, :]
    with np.errstate(all="ignore"):
        tx = (m2 * y + m3 * x) + o1
        ty = (m0 * y + m1 * x) + o0
    assert tx.dtype == F and ty.dtype == F and tx.shape == (OH, OW) and ty.shape == (OH, OW)
    return ty, tx


def warp_ref(image, M, off, out_shape=None, fill=0.0, mode=1):
    """(out, counts): the warp of `image` (H x W float32, or H x W x 3 uint8) and the number of output pixels in each class of
    CLASSES.  The three tap classes (last2, wide1off, frac_x_at_last2) count pixels that are inside and not cut, i.e. whose taps
    reach the output when mode == 1."""
    image = np.ascontiguousarray(image)
    rgb = image.ndim == 3
    assert image.dtype == (np.uint8 if rgb else F) and (not rgb or image.shape[2] == 3)
    H, W = image.shape[:2]
    OH, OW = out_shape or (H, W)
    fill = F(fill)
    ty, tx = coords(M, off, (OH, OW))
    with np.errstate(all="ignore"):
        inside = (F(0) <= tx) & (tx < F(W)) & (F(0) <= ty) & (ty < F(H))
        cut = (tx >= F(W) + F(-0.5)) | (ty >= F(H) + F(-0.5))
        # truncation toward zero, only where the point is inside: 0 <= t < 2^24, so the cast is exact and defined
        xp = np.where(inside, tx, F(0)).astype(np.int64)
        yp = np.where(inside, ty, F(0)).astype(np.int64)
        xin = xp + 1 < W
        yin = yp + 1 < H
        xn = np.where(xin, xp + 1, xp)              # a valid index either way; the tap is replaced by fill where not xin
        yn = np.where(yin, yp + 1, yp)
        src = image.astype(F)
        ch = (slice(None), slice(None), None) if rgb else (slice(None), slice(None))
        p = src[yp, xp]
        if mode == 1:
            px = np.where(xin[ch], src[yp, xn], fill)
            py = np.where(yin[ch], src[yn, xp], fill)
            pn = np.where((xin & yin)[ch], src[yn, xn], fill)
            fx1 = ((xp + 1).astype(F) - tx)[ch]; fx0 = (tx - xp.astype(F))[ch]
            fy1 = ((yp + 1).astype(F) - ty)[ch]; fy0 = (ty - yp.astype(F))[ch]
            i1 = fx1 * p + fx0 * px
            i2 = fx1 * py + fx0 * pn
            v = fy1 * i1 + fy0 * i2
        else:
            v = p
        v = np.where((inside & ~cut)[ch], v, fill)
    assert v.dtype == F
    if rgb:
        t = np.trunc(v)
        assert np.isfinite(t).all() and t.min(initial=0) >= 0 and t.max(initial=0) <= 255, "outside uint8: undefined in C"
        out = t.astype(np.int64).astype(np.uint8)
    else:
        out = v
    live = inside & ~cut
    pix = yp * W + xp
    last2 = live & (pix >= W * H - 2)
    counts = {
        "inside": inside, "cut_inside": inside & cut,
        "xedge": live & ~xin & yin, "yedge": live & xin & ~yin, "corner": live & ~xin & ~yin,
        "last2": last2,
        "wide1off": live & yin & (3 * pix + 3 * W + 8 > 3 * W * H),
        "frac_x_at_last2": last2 & xin & (tx != xp.astype(F)),
    }
    assert tuple(counts) == CLASSES
    return out, {k: int(m.sum()) for k, m in counts.items()}


def same(got, want, nan_any_payload=False):
    """bit equality of two arrays; with nan_any_payload a NaN of `want` is matched by any NaN"""
    got = np.ascontiguousarray(got); want = np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if nan_any_payload and want.dtype == F:
        nan = np.isnan(want)
        if not np.array_equal(np.isnan(got), nan):
            return False
        return np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    return np.array_equal(got.view(np.uint8), want.view(np.uint8))
