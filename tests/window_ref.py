"""numpy restatement of windowed matching, written from the contract text, and the crafted keypoint
lists the CPU and GPU tests share.  Nothing here imports the package: the GPU results are compared with what this file
computes, for equality of the sorted rows.

Contract:
  candidate  list-2 keypoint j is a candidate of list-1 keypoint i iff, in float32 with every operation rounded on its own,
             abs((x2[j] - x1[i]) - sx) <= wx  and  abs((y2[j] - y1[i]) - sy) <= wy      (a NaN makes it false; w may be inf)
  rule       matching_cpu.cl:57-109 over the candidates of i in ascending j: int32 L1 distance over the 128 descriptor bytes,
             dist1 / dist2 start at 1e12f, strict '<' (earliest index of the minimum; dist2 = second smallest of the multiset),
             (i, best) emitted iff dist2 != 0 and dist1 / dist2 < ratio_th in float32
  mutual     (i, j) kept iff i is also the nearest candidate of j (same predicate, same operand order), ties to the smallest i
"""
import numpy as np

DTYPE_KP = np.dtype([("x", np.float32), ("y", np.float32), ("scale", np.float32), ("angle", np.float32), ("desc", (np.uint8, 128))])
RATIO = np.float32(0.73 * 0.73)
_FAR = np.int64(1) << 40                    # "no candidate": above every distance (<= 128 * 255)
_INIT = np.float32(1e12)


def _pair(v):
    return tuple(np.float32(t) for t in (v if hasattr(v, "__len__") else (v, v)))


def candidate_matrix(kp1, kp2, window, shift=(0.0, 0.0), rows=None):
    """boolean (len(rows), n2): is kp2[j] a candidate of kp1[rows[i]]"""
    wx, wy = _pair(window)
    sx, sy = _pair(shift)
    rows = slice(None) if rows is None else rows
    x1 = kp1["x"][rows][:, None]; y1 = kp1["y"][rows][:, None]
    x2 = kp2["x"][None, :]; y2 = kp2["y"][None, :]
    with np.errstate(all="ignore"):
        dx = x2 - x1; dx -= sx
        dy = y2 - y1; dy -= sy
        assert dx.dtype == np.float32
        return (np.abs(dx) <= wx) & (np.abs(dy) <= wy)


def _l1(d1, d2, qi, lj, step=1 << 18):
    """int64 L1 distances of the descriptor pairs (d1[qi[k]], d2[lj[k]])"""
    out = np.empty(len(qi), np.int64)
    for k0 in range(0, len(qi), step):
        a = d1[qi[k0:k0 + step]].astype(np.int16); a -= d2[lj[k0:k0 + step]].astype(np.int16)
        out[k0:k0 + step] = np.abs(a, out=a).sum(axis=1, dtype=np.int64)
    return out


def scan(kp1, kp2, window, shift=(0.0, 0.0), reverse=False, chunk=256):
    """best (int64, -1: no candidate), dist1, dist2 (float32, 1e12 where missing) per query: the queries are the keypoints of
    kp1 and the elements those of kp2, or with `reverse` the other way round (the predicate keeps its operand order)"""
    nq, nl = (len(kp2), len(kp1)) if reverse else (len(kp1), len(kp2))
    dq, dl = (kp2["desc"], kp1["desc"]) if reverse else (kp1["desc"], kp2["desc"])
    best = np.full(nq, -1, np.int64); f1 = np.full(nq, _INIT, np.float32); f2 = np.full(nq, _INIT, np.float32)
    if nl == 0:
        return best, f1, f2
    for q0 in range(0, nq, chunk):
        q1 = min(nq, q0 + chunk)
        if reverse:
            ok = candidate_matrix(kp1, kp2[q0:q1], window, shift).T          # (queries j, elements i)
        else:
            ok = candidate_matrix(kp1, kp2, window, shift, rows=slice(q0, q1))
        r, c = np.nonzero(ok)
        D = np.full(ok.shape, _FAR, np.int64)
        D[r, c] = _l1(dq, dl, r + q0, c)
        rows = np.arange(q1 - q0)
        b = D.argmin(axis=1)                                # first of the minima = earliest index
        d1 = D[rows, b].copy()
        D[rows, b] = _FAR
        d2 = D.min(axis=1)                                  # second smallest of the multiset
        has1 = d1 < _FAR; has2 = d2 < _FAR
        best[q0:q1] = np.where(has1, b, -1)
        f1[q0:q1] = np.where(has1, d1, 0).astype(np.float32); f1[q0:q1][~has1] = _INIT
        f2[q0:q1] = np.where(has2, d2, 0).astype(np.float32); f2[q0:q1][~has2] = _INIT
    return best, f1, f2


def match(kp1, kp2, window, shift=(0.0, 0.0), mutual=False, ratio_th=RATIO):
    """(m, 2) int32 pairs in ascending i"""
    if len(kp1) == 0 or len(kp2) == 0:
        return np.zeros((0, 2), np.int32)
    best, f1, f2 = scan(kp1, kp2, window, shift)
    with np.errstate(all="ignore"):
        keep = (f2 != 0) & (f1 / f2 < np.float32(ratio_th))
    if mutual:
        back = scan(kp1, kp2, window, shift, reverse=True)[0]
        keep &= back[np.maximum(best, 0)] == np.arange(len(kp1))
    i = np.nonzero(keep)[0]
    return np.stack([i, best[i]], axis=1).astype(np.int32)


def sort_rows(a):
    a = np.asarray(a).reshape(-1, 2)
    return a[np.lexsort((a[:, 1], a[:, 0]))]


def subset_in_window(pairs, kp1, kp2, window, shift=(0.0, 0.0)):
    """the rows (i, j) of `pairs` that satisfy the predicate (identity I2: all of them are in the windowed result)"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    keep = np.array([candidate_matrix(kp1[i:i + 1], kp2[j:j + 1], window, shift)[0, 0] for i, j in pairs], bool)
    return pairs[keep]


# ---------------------------------------------------------------------------------------------- crafted lists
def lists(n1, n2, shared, seed, H=90, W=120):
    """two lists built like `lists()` of tests/test_gpu_match_roi.py: random descriptors, `shared` of list 2 within +-6 of a
    list-1 descriptor, one exact duplicate descriptor, independent uniform positions"""
    rng = np.random.default_rng(seed)
    a = np.zeros(n1, DTYPE_KP); b = np.zeros(n2, DTYPE_KP)
    a["desc"] = rng.integers(0, 256, (n1, 128), dtype=np.uint8)
    b["desc"] = rng.integers(0, 256, (n2, 128), dtype=np.uint8)
    idx = rng.permutation(n1)[:shared]
    b["desc"][:shared] = np.clip(a["desc"][idx].astype(int) + rng.integers(-6, 7, (shared, 128)), 0, 255).astype(np.uint8)
    b["desc"][shared + 1] = b["desc"][shared]                       # an exact duplicate: tie-breaking matters
    a["x"] = rng.random(n1) * W * 1.15; a["y"] = rng.random(n1) * H * 1.15
    b["x"] = rng.random(n2) * W * 1.15; b["y"] = rng.random(n2) * H * 1.15
    return a, b, idx


def crafted(n1, n2, seed, shift=(0.0, 0.0), H=90, W=120):
    """`lists()` with positions that make windows bite: the partners lie at their originals plus `shift` (a quarter exactly, the
    rest within +-1.5 px), the duplicate descriptor sits on the position of its twin (both are candidates: the tie rule decides),
    and a block of each list (up to 300 keypoints) shares ONE position: a crowded cell."""
    shared = min(n1, n2) // 2
    a, b, idx = lists(n1, n2, shared, seed, H, W)
    rng = np.random.default_rng(seed + 1000)
    noise = rng.uniform(-1.5, 1.5, (shared, 2)).astype(np.float32)
    noise[::4] = 0
    b["x"][:shared] = a["x"][idx] + np.float32(shift[0]) + noise[:, 0]
    b["y"][:shared] = a["y"][idx] + np.float32(shift[1]) + noise[:, 1]
    if shared + 1 < n2:
        b["x"][shared + 1] = b["x"][shared]; b["y"][shared + 1] = b["y"][shared]
    crowd = min(300, n1 // 3, n2 // 3)
    if crowd:
        a["x"][n1 - crowd:] = 40.25; a["y"][n1 - crowd:] = 33.5
        b["x"][n2 - crowd:] = np.float32(40.25) + np.float32(shift[0]); b["y"][n2 - crowd:] = np.float32(33.5) + np.float32(shift[1])
    return a, b
