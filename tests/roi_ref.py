"""numpy restatement of the brute-force matcher's region-of-interest rule (match_roi_flags_kernel in k_match.hpp, so_roi_inside /
so_match_ex in oracle/sift_oracle.c).  For a float32 coordinate v, a mask `roi` of rh rows by rw columns, as int8:

    v is convertible  iff  fabsf(v) < 2147483648.0f  (false for NaN and +-inf); then int(v) truncates toward zero, so every v in
                      (-1, 1) gives 0, -0.0 included -- the reference's literal (int)x;
    inside            iff  both coordinates are convertible and 0 <= r < rh and 0 <= c < rw, (c, r) = int(x), int(y);
                      a keypoint with a coordinate that is not convertible is outside and no index is formed;
    on                =    inside and roi[r, c] != 0: any non-zero int8 counts, negative values included;
    query dropped     iff  inside and not on (mode 1)  /  not on (mode 2);
    list flag         =    0 if on, else 1 (mode 1: the distance is forced to 0) or 2 (mode 2: excluded).

The guard is written out: no value is converted that the rule does not convert.  numpy only; nothing here imports the package or
the oracle.  tests/test_roi_cases_host.py pins the oracle to this on the crafted cases of tests/roi_cases.py, the GPU tests
(tests/test_gpu_roi_cases.py) compare the kernels with it."""
import numpy as np

import window_ref as wr

LIMIT = np.float32(2147483648.0)


def convertible(v):
    """bool per element of a float32 array: |v| < 2^31 (NaN and the infinities compare false)"""
    v = np.asarray(v)
    assert v.dtype == np.float32
    with np.errstate(invalid="ignore"):
        return np.abs(v) < LIMIT


def truncated(v, ok):
    """int64 per element: v truncated toward zero where `ok`, -1 elsewhere (never used: such a keypoint is outside)"""
    out = np.full(v.shape, -1, np.int64)
    out[ok] = np.trunc(v[ok].astype(np.float64)).astype(np.int64)         # |v| < 2^31: exact in binary64 and in int64
    return out


def inside_on(kp, roi):
    """(inside, on), bool per keypoint"""
    roi = np.asarray(roi)
    assert roi.dtype == np.int8 and roi.ndim == 2
    rh, rw = roi.shape
    x, y = np.ascontiguousarray(kp["x"]), np.ascontiguousarray(kp["y"])
    ok = convertible(x) & convertible(y)
    c, r = truncated(x, ok), truncated(y, ok)
    inside = ok & (r >= 0) & (r < rh) & (c >= 0) & (c < rw)
    on = np.zeros(len(x), bool)
    on[inside] = roi[r[inside], c[inside]] != 0                           # indexed only where inside
    return inside, on


def flags(kp, roi, mode):
    """(query_dropped bool[n], list_flag uint8[n]) of one keypoint list"""
    assert mode in (1, 2)
    inside, on = inside_on(kp, roi)
    dropped = (inside & ~on) if mode == 1 else ~on
    return dropped, np.where(on, 0, 1 if mode == 1 else 2).astype(np.uint8)


def restated(a, b, roi, mode):
    """(a', b', rows of a', rows of b'): the masked call without flags.  A dropped query and an excluded element are deleted; an
    element whose distance is forced to 0 gets the queries' descriptor, which all queries must then share.  The restated lists
    sit on one position: what the positions meant is in the flags."""
    dropped, _ = flags(a, roi, mode)
    _, lflag = flags(b, roi, mode)
    keep1, keep2 = ~dropped, lflag != 2
    b2 = b.copy()
    if (lflag == 1).any():
        assert len(a) and (a["desc"] == a["desc"][0]).all(), "a forced zero is restated for queries that share one descriptor"
        b2["desc"][lflag == 1] = a["desc"][0]
    a2, b2 = a[keep1].copy(), b2[keep2]
    a2["x"] = a2["y"] = b2["x"] = b2["y"] = 0
    return a2, b2, np.nonzero(keep1)[0], np.nonzero(keep2)[0]


def expected_pairs(a, b, roi, mode, mutual=False, ratio_th=wr.RATIO):
    """sorted (m, 2) int32 rows of match_ex(a, b, roi, mode, mutual) for ratio_th <= 1"""
    assert ratio_th <= 1          # above 1 a query without any element pairs with index 0, which a deleted list cannot name
    a2, b2, ia, ib = restated(a, b, roi, mode)
    got = wr.match(a2, b2, np.inf, mutual=mutual, ratio_th=ratio_th)
    if len(got):
        got = np.stack([ia[got[:, 0]], ib[got[:, 1]]], axis=1)
    return wr.sort_rows(got.astype(np.int32))
