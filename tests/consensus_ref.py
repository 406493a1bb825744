"""numpy restatement of the consensus filter's contract, written from the contract text, and the
synthetic match sets the CPU and GPU tests share.  Nothing here imports the package: the GPU results are compared with
what this file computes, for equality.

Contract, in the order of the steps:
  gather  match j -> float32 (x0, y0, x1, y1) = (kp1[pairs[j,0]].x, .y, kp2[pairs[j,1]].x, .y); four NaN where an index is
          outside its list
  sample  i_k = mix(seed + 0x9E3779B9 * (3h + k + 1)) mod M, k = 0, 1, 2, uint32 wrap-around arithmetic
  solve   binary64, one rounding per product / sum in the order written; void iff not (|det| >= 1.0); six coefficients -> float32
  vote    float32, unfused: ex = ((a*x0 + b*y0) + c) - x1, ey = ((d*x0 + e*y0) + f) - y1, vote iff ex*ex + ey*ey <= tol*tol
  select  the non-void h with most votes, ties to the smallest h; none if every h is void or M < 3
  mask    the winner's votes
"""
import numpy as np

DTYPE_KP = np.dtype([("x", np.float32), ("y", np.float32), ("scale", np.float32), ("angle", np.float32), ("desc", (np.uint8, 128))])
_M32 = np.uint64(0xFFFFFFFF)


def mix(v):
    """the contract's 32-bit mixer on an array of uint32 values held in uint64 (masked after every step that can carry)"""
    v = np.asarray(v, np.uint64) & _M32
    v = v ^ (v >> np.uint64(16))
    v = (v * np.uint64(0x7FEB352D)) & _M32
    v = v ^ (v >> np.uint64(15))
    v = (v * np.uint64(0x846CA68B)) & _M32
    v = v ^ (v >> np.uint64(16))
    return v


def sample(seed, n_hyp, M):
    """(n_hyp, 3) indices of the matches each hypothesis is solved from"""
    h = np.arange(n_hyp, dtype=np.uint64)[:, None]
    k = np.arange(3, dtype=np.uint64)[None, :]
    arg = (np.uint64(seed & 0xFFFFFFFF) + ((np.uint64(0x9E3779B9) * ((np.uint64(3) * h + k + np.uint64(1)) & _M32)) & _M32)) & _M32
    return (mix(arg) % np.uint64(M)).astype(np.int64)


def gather(kp1, kp2, pairs):
    """(M, 4) float32; rows of pairs with an index outside its list are NaN"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    n1, n2 = len(kp1), len(kp2)
    ok = (pairs[:, 0] >= 0) & (pairs[:, 0] < n1) & (pairs[:, 1] >= 0) & (pairs[:, 1] < n2)
    pts = np.full((pairs.shape[0], 4), np.nan, np.float32)
    i0, i1 = pairs[ok, 0], pairs[ok, 1]
    pts[ok, 0] = kp1["x"][i0]; pts[ok, 1] = kp1["y"][i0]
    pts[ok, 2] = kp2["x"][i1]; pts[ok, 3] = kp2["y"][i1]
    return pts


def solve(pts, idx):
    """models (H, 6) float32, void rows all NaN, and the boolean `valid` (H,)"""
    p = pts.astype(np.float64)
    i0, i1, i2 = idx[:, 0], idx[:, 1], idx[:, 2]
    x0, y0, x1, y1 = p[:, 0], p[:, 1], p[:, 2], p[:, 3]
    with np.errstate(all="ignore"):
        ux = x0[i1] - x0[i0]; uy = y0[i1] - y0[i0]; vx = x0[i2] - x0[i0]; vy = y0[i2] - y0[i0]
        det = ux * vy - vx * uy
        valid = np.abs(det) >= 1.0                      # False for NaN
        px = x1[i1] - x1[i0]; qx = x1[i2] - x1[i0]; py = y1[i1] - y1[i0]; qy = y1[i2] - y1[i0]
        a = (px * vy - qx * uy) / det; b = (qx * ux - px * vx) / det
        c = x1[i0] - (a * x0[i0] + b * y0[i0])
        d = (py * vy - qy * uy) / det; e = (qy * ux - py * vx) / det
        f = y1[i0] - (d * x0[i0] + e * y0[i0])
        models = np.stack([a, b, c, d, e, f], axis=1).astype(np.float32)
    models[~valid] = np.nan
    return models, valid


def vote_matrix(pts, models, tol):
    """boolean (len(models), M): does match j vote for the model -- float32, every operation rounded on its own"""
    tol = np.float32(tol)
    x0, y0, x1, y1 = (np.ascontiguousarray(pts[:, k]) for k in range(4))
    m = np.asarray(models, np.float32).reshape(-1, 6)
    a, b, c, d, e, f = (m[:, k:k + 1] for k in range(6))
    with np.errstate(all="ignore"):
        tol2 = tol * tol                                # float32: inf from 1.9e19 on, 0 below 2.7e-23
        t = a * x0; u = b * y0; t += u; t += c; t -= x1; t *= t
        s = d * x0; u = e * y0; s += u; s += f; s -= y1; s *= s
        t += s
        assert t.dtype == np.float32
        return t <= tol2


def count_votes(pts, models, tol):
    """votes (H,) int32; chunked over H so that a chunk's temporaries stay in cache"""
    H, M = models.shape[0], pts.shape[0]
    votes = np.zeros(H, np.int32)
    step = max(1, (1 << 20) // max(M, 1))
    for h0 in range(0, H, step):
        votes[h0:h0 + step] = vote_matrix(pts, models[h0:h0 + step], tol).sum(axis=1)
    return votes


def consensus(kp1, kp2, pairs, n_hyp=2048, tol=3.0, seed=0):
    """dict(mask uint8 (M,), model float32 (6,) or None, winner, winner_votes, votes_all int32 (H,), models_all float32 (H, 6),
    valid bool (H,))"""
    pts = gather(kp1, kp2, pairs)
    M = pts.shape[0]
    out = dict(mask=np.zeros(M, np.uint8), model=None, winner=-1, winner_votes=0, votes_all=np.zeros(n_hyp, np.int32),
               models_all=np.full((n_hyp, 6), np.nan, np.float32), valid=np.zeros(n_hyp, bool), pts=pts)
    if M < 3:
        return out
    models, valid = solve(pts, sample(seed, n_hyp, M))
    votes = count_votes(pts, models, tol)
    votes[~valid] = 0
    out.update(votes_all=votes, models_all=models, valid=valid)
    ranked = np.where(valid, votes.astype(np.int64), -1)
    w = int(np.argmax(ranked))                          # first of the maxima = smallest h
    if ranked[w] < 0:
        return out
    out.update(winner=w, winner_votes=int(votes[w]), model=models[w].copy(),
               mask=vote_matrix(pts, models[w], tol)[0].astype(np.uint8))
    return out


# ---------------------------------------------------------------------------------------------- synthetic match sets
NOISE_SIGMA = 0.3


def synthetic_matches(M, w, seed, frame=(4096, 4096)):
    """M matches in a frame of (width, height): a share `w` follows a ground-truth affine map (rotation <= 3 degrees, scale
    within 2 %, shift <= 40 px) with Gaussian position noise of NOISE_SIGMA px, the rest has independent uniform positions;
    rows shuffled; the records sit at random places of two longer lists (`pairs` is a random injection into each), descriptors
    and the other fields arbitrary.
    Returns kp1, kp2, pairs int32 (M, 2), inlier bool (M,), truth float64 (6,) = (a, b, c, d, e, f)."""
    rng = np.random.default_rng(seed)
    W, Hh = frame
    n_in = int(round(w * M))
    theta = np.deg2rad(rng.uniform(-3.0, 3.0)); s = rng.uniform(0.98, 1.02)
    tx, ty = rng.uniform(-40.0, 40.0, 2)
    truth = np.array([s * np.cos(theta), -s * np.sin(theta), tx, s * np.sin(theta), s * np.cos(theta), ty])
    p0 = np.stack([rng.uniform(0, W, M), rng.uniform(0, Hh, M)], axis=1)
    p1 = np.stack([rng.uniform(0, W, M), rng.uniform(0, Hh, M)], axis=1)
    inlier = np.zeros(M, bool); inlier[:n_in] = True
    p1[:n_in, 0] = truth[0] * p0[:n_in, 0] + truth[1] * p0[:n_in, 1] + truth[2] + rng.normal(0, NOISE_SIGMA, n_in)
    p1[:n_in, 1] = truth[3] * p0[:n_in, 0] + truth[4] * p0[:n_in, 1] + truth[5] + rng.normal(0, NOISE_SIGMA, n_in)
    order = rng.permutation(M)
    p0, p1, inlier = p0[order], p1[order], inlier[order]
    n1, n2 = M + M // 8 + 5, M + M // 16 + 3
    pairs = np.stack([rng.permutation(n1)[:M], rng.permutation(n2)[:M]], axis=1).astype(np.int32)
    lists = []
    for n, pos, col in ((n1, p0, 0), (n2, p1, 1)):
        kp = np.zeros(n, DTYPE_KP)
        kp["x"] = rng.uniform(0, W, n); kp["y"] = rng.uniform(0, Hh, n)          # the records no pair names
        kp["scale"] = rng.uniform(1, 8, n); kp["angle"] = rng.uniform(-3.14, 3.14, n)
        kp["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
        kp["x"][pairs[:, col]] = pos[:, 0]; kp["y"][pairs[:, col]] = pos[:, 1]
        lists.append(kp)
    return lists[0], lists[1], pairs, inlier, truth


def lstsq_affine(x0, y0, x1, y1):
    """float64 least-squares (a, b, c, d, e, f) of x1 = a x0 + b y0 + c, y1 = d x0 + e y0 + f"""
    A = np.stack([np.asarray(x0, np.float64), np.asarray(y0, np.float64), np.ones(len(x0))], axis=1)
    abc = np.linalg.lstsq(A, np.asarray(x1, np.float64), rcond=None)[0]
    def_ = np.linalg.lstsq(A, np.asarray(y1, np.float64), rcond=None)[0]
    return np.concatenate([abc, def_])


def corner_error(model, truth, frame=(4096, 4096)):
    """largest distance between the images of the four frame corners under two affine maps, pixels"""
    W, Hh = frame
    worst = 0.0
    for x, y in ((0, 0), (W, 0), (0, Hh), (W, Hh)):
        dx = (model[0] - truth[0]) * x + (model[1] - truth[1]) * y + (model[2] - truth[2])
        dy = (model[3] - truth[3]) * x + (model[4] - truth[4]) * y + (model[5] - truth[5])
        worst = max(worst, float(np.hypot(dx, dy)))
    return worst


#: the sets of the issue's item 2 -- (M, inlier share, seed) on a 4096 x 4096 frame, H = 2048, tol = 3
SETS = [(M, w, 100 * i + k) for i, M in enumerate((200, 5000, 200000)) for k, w in enumerate((0.9, 0.5, 0.3))]
