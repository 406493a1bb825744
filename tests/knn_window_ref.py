"""numpy restatement of k-nearest-neighbour matching inside a search window, written from the contract
text.  Nothing here imports the package: the GPU results are compared with what this file computes, for equality of both arrays.

Contract, for lists kp1 (n1 records), kp2 (n2 records), 1 <= k <= 8, a window (wx, wy) >= 0 (inf allowed) and a finite shift:
  candidate  list-2 keypoint j is a candidate of list-1 keypoint i iff, in float32 with every operation rounded on its own,
             abs((x2[j] - x1[i]) - sx) <= wx  and  abs((y2[j] - y1[i]) - sy) <= wy      (row 6's predicate: window_ref.candidate_matrix)
  d(i, j)    metric "l1": the int32 L1 distance over the 128 descriptor bytes (row 7); metric "l2": the int32 sum of the squared
             byte differences (row 8)
  row i      the k smallest elements of {(d(i, j), j) : j a candidate of i} in ascending lexicographic order of (distance, index);
             idx[i, r] is the index, dist[i, r] the distance (both int32)
  padding    where i has fewer than k candidates (none included) the remaining slots hold idx = -1, dist = -1
The row for k is the first k columns of the row for 8.
"""
import numpy as np

import window_ref as wr

K_MAX = 8


def distances(d1, d2, qi, lj, metric, step=1 << 17):
    """int64 distances of the descriptor pairs (d1[qi[t]], d2[lj[t]])"""
    out = np.empty(len(qi), np.int64)
    for t0 in range(0, len(qi), step):
        a = d1[qi[t0:t0 + step]].astype(np.int64) - d2[lj[t0:t0 + step]].astype(np.int64)
        out[t0:t0 + step] = np.abs(a).sum(axis=1) if metric == "l1" else (a * a).sum(axis=1)
    return out


def knn(kp1, kp2, k, window, shift=(0.0, 0.0), metric="l1", chunk=256, counts=None):
    """(idx, dist), two int32 (n1, k) arrays.  The candidates of a chunk of queries come out of numpy.nonzero in ascending (i, j); a
    stable argsort by (i, distance) therefore leaves equal distances of a query in ascending j.  counts: an int64 array of n1
    that receives the number of candidates of every query."""
    k = int(k)
    if k < 1 or k > K_MAX:
        raise ValueError("k must be 1 .. %d" % K_MAX)
    if metric not in ("l1", "l2"):
        raise ValueError("metric must be 'l1' or 'l2'")
    n1, n2 = len(kp1), len(kp2)
    idx = np.full((n1, k), -1, np.int32); dist = np.full((n1, k), -1, np.int32)
    if counts is not None:
        counts[:] = 0
    if n1 == 0 or n2 == 0:
        return idx, dist
    d1, d2 = np.ascontiguousarray(kp1["desc"]), np.ascontiguousarray(kp2["desc"])
    for q0 in range(0, n1, chunk):
        q1 = min(n1, q0 + chunk)
        r, c = np.nonzero(wr.candidate_matrix(kp1, kp2, window, shift, rows=slice(q0, q1)))
        if len(r) == 0:
            continue
        d = distances(d1, d2, r + q0, c, metric)
        order = np.argsort(r.astype(np.int64) * (np.int64(1) << 32) + d, kind="stable")
        r, c, d = r[order], c[order], d[order]
        n = np.bincount(r, minlength=q1 - q0)
        rank = np.arange(len(r)) - (np.cumsum(n) - n)[r]              # position inside the query's sorted candidates
        take = rank < k
        idx[r[take] + q0, rank[take]] = c[take]
        dist[r[take] + q0, rank[take]] = d[take]
        if counts is not None:
            counts[q0:q1] = n
    return idx, dist


def ratio_pairs(idx, dist, th):
    """the ratio test of matching_cpu.cl:103-108 on the first two columns, evaluated row by row: (i, idx[i, 0]) iff
    dist2 != 0 and dist1 / dist2 < th in float32, a missing distance (-1) counting as 1e12f"""
    out = []
    for i in range(len(idx)):
        f1 = np.float32(1e12) if dist[i, 0] < 0 else np.float32(dist[i, 0])
        f2 = np.float32(1e12) if dist[i, 1] < 0 else np.float32(dist[i, 1])
        if f2 != 0 and np.float32(f1 / f2) < np.float32(th):
            out.append((i, idx[i, 0]))
    return np.array(out, np.int32).reshape(-1, 2)
