"""numpy restatement of the device median's contract, written from the contract text, and the match
sets the CPU and GPU tests share.  Nothing here imports the package: the GPU results are compared with what this file computes,
bit for bit.

Contract, in the order of the steps (binary32 throughout, one rounding per operation, subnormals kept):
  gather  match j -> float32 (x0, y0, x1, y1), four NaN where an index is outside its list (consensus_ref.gather)
  used    (mask is None or mask[j] != 0) and all four finite
  displ.  dx = x1 - x0, dy = y1 - y0; +-inf from an overflow takes part
  order   key(v) = bits(v) ^ (0xffffffff if bits(v) >> 31 else 0x80000000) as uint32; ascending key is the total order of float32
  ranks   n used pairs: lo, hi = the values of rank (n - 1) >> 1 and n >> 1 in ascending key order, per axis
  median  n odd: lo; n even: (lo + hi) * 0.5
  n == 0  EMPTY: six NaN, counts 0
  keep    used and both medians finite and |dx - mdx| <= tol and |dy - mdy| <= tol (tol may be inf)
"""
import numpy as np

from consensus_ref import DTYPE_KP, gather
from fit_ref import make_case  # noqa: F401  (the generated match sets of the fit's tests serve here too)

#: positions of the six results
MDX, MDY, LO_DX, HI_DX, LO_DY, HI_DY = range(6)


def key(v):
    """the contract's order key of float32 values, uint32"""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.ascontiguousarray(k, np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF)).astype(np.uint32)).view(np.float32)


def middle(d):
    """(median, lo, hi) of the float32 values d (n >= 1,) by the contract: a full sort of the keys, not a selection"""
    k = np.sort(key(d), kind="stable")
    n = k.shape[0]
    lo, hi = unkey(k[(n - 1) >> 1:((n - 1) >> 1) + 1])[0], unkey(k[n >> 1:(n >> 1) + 1])[0]
    with np.errstate(all="ignore"):
        med = lo if n & 1 else np.float32(np.float32(lo + hi) * np.float32(0.5))
    return med, lo, hi


def used_pairs(pts, mask=None):
    used = np.isfinite(pts).all(axis=1)
    if mask is not None:
        used &= np.asarray(mask).reshape(-1) != 0
    return used


def shift_pts(pts, mask=None, tol=None):
    """(out float32 (6,), counts int64 (2,), keep bool (M,) or None) from gathered float32 (M, 4) positions"""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    out = np.full(6, np.nan, np.float32)
    counts = np.zeros(2, np.int64)
    used = used_pairs(pts, mask)
    keep = None if tol is None else np.zeros(pts.shape[0], bool)
    n = int(used.sum())
    if n == 0:
        return out, counts, keep
    with np.errstate(all="ignore"):
        dx = (pts[:, 2] - pts[:, 0]).astype(np.float32)
        dy = (pts[:, 3] - pts[:, 1]).astype(np.float32)
        out[MDX], out[LO_DX], out[HI_DX] = middle(dx[used])
        out[MDY], out[LO_DY], out[HI_DY] = middle(dy[used])
        counts[0] = n
        if tol is not None and np.isfinite(out[MDX]) and np.isfinite(out[MDY]):
            t = np.float32(tol)
            keep = used & (np.abs(dx - out[MDX]) <= t) & (np.abs(dy - out[MDY]) <= t)
            counts[1] = int(keep.sum())
    return out, counts, keep


def shift(kp1, kp2, pairs, mask=None, tol=None):
    """the results of the contract for two record lists and (M, 2) pairs"""
    return shift_pts(gather(kp1, kp2, pairs), mask, tol)


def same_bits(got, want):
    """float32 values equal as bit patterns; a NaN matches any NaN"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    return bool(got.shape == want.shape and np.array_equal(np.isnan(got), nan)
                and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32)))


# ---------------------------------------------------------------------------------------------- match sets
def lists_from_displacements(dx, dy=None, seed=0, base=None):
    """Two record lists and (M, 2) pairs whose pair j has exactly the float32 displacement (dx[j], dy[j]): x0 = y0 = `base`
    (default 0.0, so that x1 - x0 is x1 itself, sign of a zero, subnormals and all) and the records shuffled within their lists.
    `base` may be an array; the caller then answers for x1 - x0 being exact."""
    dx = np.asarray(dx, np.float32)
    dy = dx[::-1].copy() if dy is None else np.asarray(dy, np.float32)
    M = dx.shape[0]
    rng = np.random.default_rng(seed)
    b = np.zeros(M, np.float32) if base is None else np.asarray(base, np.float32)
    n1, n2 = M + 3, M + 5
    pairs = np.stack([rng.permutation(n1)[:M], rng.permutation(n2)[:M]], axis=1).astype(np.int32)
    kp1, kp2 = np.zeros(n1, DTYPE_KP), np.zeros(n2, DTYPE_KP)
    kp1["x"] = 777.0; kp1["y"] = -55.0; kp2["x"] = 12345.0; kp2["y"] = 0.5          # records no pair names
    kp1["x"][pairs[:, 0]] = b; kp1["y"][pairs[:, 0]] = b
    with np.errstate(all="ignore"):
        kp2["x"][pairs[:, 1]] = dx if base is None else (b + dx).astype(np.float32)     # (+0.0) + (-0.0) would lose the sign
        kp2["y"][pairs[:, 1]] = dy if base is None else (b + dy).astype(np.float32)
    return kp1, kp2, pairs


def value_sets(n, seed):
    """name -> float32 (n,) displacement values of the kinds the host test holds against numpy.median"""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, 2 * n + 64, dtype=np.uint64).astype(np.uint32).view(np.float32)
    bits = bits[np.isfinite(bits)][:n]                                            # differences of these overflow now and then
    seven = np.float32([-3.5, -1.0, -0.0, 0.0, 0.25, 2.0, 1e30])
    return {
        "normal": rng.normal(3.0, 10.0, n).astype(np.float32),
        "tied": seven[rng.integers(0, 7, n)],
        "bits": bits,
        "zeros": np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32),
        "subnormal": (rng.integers(-200, 200, n).astype(np.int64) * 1).astype(np.float32) * np.float32(1.4e-45),
    }
