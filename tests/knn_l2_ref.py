"""numpy restatement of k-nearest-neighbour matching under the squared Euclidean distance, written from
the contract text.  Nothing here imports the package: the GPU results are compared with what this file computes, for equality of
both arrays.

Contract, for lists kp1 (n1 records), kp2 (n2 records) and 1 <= k <= 8 -- row 7's (tests/knn_ref.py) with another item 1:
  d(i, j)   the sum over the 128 descriptor bytes of (kp1[i].desc[b] - kp2[j].desc[b]) ** 2 as integers: the SQUARED Euclidean
            distance, 0 .. 8 323 200 (= 128 * 255 ** 2), int32.  No square root is taken.
  row i     the k smallest elements of {(d(i, j), j) : 0 <= j < n2} in ascending lexicographic order of (distance, index):
            among equal distances the smaller index comes first.  idx[i, r] is the index, dist[i, r] the distance (both int32)
  padding   where n2 < k the remaining slots hold idx = -1, dist = -1
  errors    k < 1 or k > 8
Positions play no part.
"""
import numpy as np

K_MAX = 8
DMAX = 128 * 255 * 255                     # 8 323 200 = 0x7F0100


def _l2sq(d1, d2, q0, q1):
    """int64 (q1 - q0, n2) squared Euclidean distances of the (int64) descriptors d1[q0:q1] to every descriptor of d2, in the difference form"""
    a = d1[q0:q1, None, :] - d2[None, :, :]
    return (a * a).sum(axis=2, dtype=np.int64)


def knn(kp1, kp2, k, budget=1 << 18):
    """(idx, dist), two int32 (n1, k) arrays.  The distances are computed in chunks of queries (about `budget` int64 differences
    at a time); a stable argsort of a row is ascending in the index among equal distances."""
    k = int(k)
    if k < 1 or k > K_MAX:
        raise ValueError("k must be 1 .. %d" % K_MAX)
    n1, n2 = len(kp1), len(kp2)
    idx = np.full((n1, k), -1, np.int32); dist = np.full((n1, k), -1, np.int32)
    if n1 == 0 or n2 == 0:
        return idx, dist
    d1, d2 = np.ascontiguousarray(kp1["desc"]).astype(np.int64), np.ascontiguousarray(kp2["desc"]).astype(np.int64)
    m = min(k, n2)
    step = max(1, budget // (128 * n2))
    for q0 in range(0, n1, step):
        D = _l2sq(d1, d2, q0, min(n1, q0 + step))
        order = np.argsort(D, axis=1, kind="stable")[:, :m]
        idx[q0:q0 + step, :m] = order
        dist[q0:q0 + step, :m] = np.take_along_axis(D, order, axis=1)
    return idx, dist
