"""numpy restatement of the device fit's contract, written from the contract text, and the match sets
the CPU and GPU tests share.  Nothing here imports the package: the GPU results are compared with what this file computes,
bit for bit.

Contract, in the order of the steps (binary64 throughout, one rounding per product / sum / quotient in the order written):
  gather  match j -> float32 (x0, y0, x1, y1), four NaN where an index is outside its list (consensus_ref.gather)
  used    (mask is None or mask[j] != 0) and all four finite; an unused pair adds +0.0 to every sum and nothing to n
  R(v)    T = 256 lanes, B workgroups, G = B T; pair j sits on global lane j mod G
          (i) every lane adds its pairs in ascending j to +0.0; (ii) a workgroup folds its 256 lane sums by
          for s = 128, 64 .. 1: v[t] = v[t] + v[t + s] for t < s; (iii) the B results are added in ascending order to +0.0
  pass 1  n; sx, sy, su, sv = R(x0), R(y0), R(x1), R(y1); n == 0: EMPTY; else mx = sx / n, ...
  pass 2  X = x0 - mx, Y = y0 - my, U = x1 - mu, V = y1 - mv; Sxx, Sxy, Syy, Sxu, Syu, Sxv, Syv = R(X*X), R(X*Y), ...
  solve   scale = Sxx*Syy, det = scale - Sxy*Sxy; DEGENERATE iff n < 3 or not (|det| > 1e-12 * max(1.0, scale))
          a = (Sxu*Syy - Syu*Sxy)/det, b = (Syu*Sxx - Sxu*Sxy)/det, c = mu - (a*mx + b*my); d, e, f from Sxv, Syv, mv
  pass 3  ex = ((a*x0 + b*y0) + c) - x1, ey = ((d*x0 + e*y0) + f) - y1; ssr = R(ex*ex + ey*ey)
"""
import numpy as np

from consensus_ref import DTYPE_KP, gather

T = 256
OK, EMPTY, DEGENERATE = 0, 1, 2
#: positions of the 20 results
STATUS, N, MEANS, MOMENTS, MODEL, SSR = 0, 1, slice(2, 6), slice(6, 13), slice(13, 19), 19


def default_blocks(M):
    return min(256, max(1, -(-M // T)))


def reduce_R(v, B):
    """R(v) of the per-pair float64 values v (M,), unused pairs already +0.0, over B workgroups"""
    v = np.asarray(v, np.float64)
    M, G = v.shape[0], B * T
    K = max(1, -(-M // G))
    rows = np.zeros((K, G), np.float64)
    rows.reshape(-1)[:M] = v                           # pair j = k G + g: row k, lane g
    lane = np.zeros(G, np.float64)
    for k in range(K):                                 # (i) ascending j per lane
        lane = lane + rows[k]
    w = lane.reshape(B, T).copy()
    s = T // 2
    while s >= 1:                                      # (ii) the fixed tree, all workgroups at once
        w[:, :s] = w[:, :s] + w[:, s:2 * s]
        s //= 2
    total = np.float64(0.0)
    for b in range(B):                                 # (iii) ascending workgroup
        total = total + w[b, 0]
    return total


def fit_pts(pts, mask=None, blocks=0):
    """the 20 float64 results from gathered float32 (M, 4) positions"""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    M = pts.shape[0]
    out = np.full(20, np.nan, np.float64)
    used = np.isfinite(pts).all(axis=1)
    if mask is not None:
        used &= np.asarray(mask).reshape(-1) != 0
    n = int(used.sum())
    out[STATUS], out[N] = EMPTY, 0.0
    if n == 0:
        return out
    B = blocks if blocks else default_blocks(M)
    p = pts.astype(np.float64)
    zero = np.float64(0.0)

    def R(v):
        return reduce_R(np.where(used, v, zero), B)
    with np.errstate(all="ignore"):
        x0, y0, x1, y1 = (np.where(used, p[:, k], zero) for k in range(4))
        nd = np.float64(n)
        mx, my, mu, mv = R(x0) / nd, R(y0) / nd, R(x1) / nd, R(y1) / nd
        X, Y, U, V = x0 - mx, y0 - my, x1 - mu, y1 - mv
        Sxx, Sxy, Syy = R(X * X), R(X * Y), R(Y * Y)
        Sxu, Syu, Sxv, Syv = R(X * U), R(Y * U), R(X * V), R(Y * V)
        out[N] = nd
        out[MEANS] = mx, my, mu, mv
        out[MOMENTS] = Sxx, Sxy, Syy, Sxu, Syu, Sxv, Syv
        scale = Sxx * Syy
        det = scale - Sxy * Sxy
        if n < 3 or not (abs(det) > np.float64(1e-12) * max(np.float64(1.0), scale)):
            out[STATUS] = DEGENERATE
            return out
        a = (Sxu * Syy - Syu * Sxy) / det; b = (Syu * Sxx - Sxu * Sxy) / det
        c = mu - (a * mx + b * my)
        d = (Sxv * Syy - Syv * Sxy) / det; e = (Syv * Sxx - Sxv * Sxy) / det
        f = mv - (d * mx + e * my)
        ex = ((a * x0 + b * y0) + c) - x1
        ey = ((d * x0 + e * y0) + f) - y1
        out[STATUS] = OK
        out[MODEL] = a, b, c, d, e, f
        out[SSR] = R(ex * ex + ey * ey)
    return out


def fit(kp1, kp2, pairs, mask=None, blocks=0):
    """the 20 float64 results of the contract for two record lists and (M, 2) pairs"""
    return fit_pts(gather(kp1, kp2, pairs), mask, blocks)


def same_bits(got, want):
    """all 20 doubles equal as bit patterns; a NaN matches any NaN"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64)))


def lstsq_model(pts, mask=None):
    """independent solver: numpy.linalg.lstsq on the (2n, 6) system of the used pairs, float64 (a, b, c, d, e, f)"""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    used = np.isfinite(pts).all(axis=1)
    if mask is not None:
        used &= np.asarray(mask).reshape(-1) != 0
    p = pts[used].astype(np.float64)
    n = p.shape[0]
    A = np.zeros((2 * n, 6)); rhs = np.zeros(2 * n)
    A[::2, 0] = p[:, 0]; A[::2, 1] = p[:, 1]; A[::2, 2] = 1.0
    A[1::2, 3] = p[:, 0]; A[1::2, 4] = p[:, 1]; A[1::2, 5] = 1.0
    rhs[::2] = p[:, 2]; rhs[1::2] = p[:, 3]
    return np.linalg.lstsq(A, rhs, rcond=None)[0]


# ---------------------------------------------------------------------------------------------- match sets
def make_case(M, seed, outliers=0.1, extent=16384.0, noise=0.3):
    """M matches: positions with fractional parts in [0, extent)^2, an affine map (rotation <= 3 degrees, scale within 2 %,
    shift <= 40 px) plus Gaussian noise of `noise` px, and a share `outliers` of gross outliers with independent uniform
    partners.  The records sit at random places of two longer lists, as in consensus_ref.synthetic_matches.
    Returns kp1, kp2, pairs int32 (M, 2), truth float64 (6,)."""
    rng = np.random.default_rng(seed)
    theta = np.deg2rad(rng.uniform(-3.0, 3.0)); s = rng.uniform(0.98, 1.02)
    tx, ty = rng.uniform(-40.0, 40.0, 2)
    truth = np.array([s * np.cos(theta), -s * np.sin(theta), tx, s * np.sin(theta), s * np.cos(theta), ty])
    p0 = rng.uniform(0, extent, (M, 2))
    p1 = np.stack([truth[0] * p0[:, 0] + truth[1] * p0[:, 1] + truth[2], truth[3] * p0[:, 0] + truth[4] * p0[:, 1] + truth[5]], axis=1)
    p1 += rng.normal(0, noise, (M, 2))
    gross = rng.random(M) < outliers
    p1[gross] = rng.uniform(0, extent, (int(gross.sum()), 2))
    n1, n2 = M + M // 8 + 5, M + M // 16 + 3
    pairs = np.stack([rng.permutation(n1)[:M], rng.permutation(n2)[:M]], axis=1).astype(np.int32)
    lists = []
    for n, pos, col in ((n1, p0, 0), (n2, p1, 1)):
        kp = np.zeros(n, DTYPE_KP)
        kp["x"] = rng.uniform(0, extent, n); kp["y"] = rng.uniform(0, extent, n)
        kp["scale"] = rng.uniform(1, 8, n); kp["angle"] = rng.uniform(-3.14, 3.14, n)
        kp["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        kp["x"][pairs[:, col]] = pos[:, 0]; kp["y"][pairs[:, col]] = pos[:, 1]
        lists.append(kp)
    return lists[0], lists[1], pairs, truth


#: (M, seed, outlier share, extent): the case list of tests/test_fit_ref_host.py, where the bound below was measured
CASES = [(18, 1, 0.0, 512.0), (255, 2, 0.1, 4096.0), (257, 3, 0.3, 16384.0), (1000, 4, 0.1, 16384.0), (1000, 5, 0.5, 2048.0),
         (5000, 6, 0.2, 16384.0), (70001, 7, 0.1, 16384.0), (200000, 8, 0.3, 16384.0)]

#: largest |coefficient difference| between the restatement and numpy.linalg.lstsq over CASES as measured on the CPU
#: (test_fit_ref_host.py prints it), and the tests' bound: 8 x that.  Both sides are float64 and differ in summation order and
#: solver only, so a small multiple covers other libm / BLAS builds without hiding a wrong formula.
LSTSQ_MEASURED = 4.547473508864641e-12
LSTSQ_BOUND = 8 * LSTSQ_MEASURED
