"""Descriptors at a PRESCRIBED squared Euclidean distance from a 0 / 255 base (match_cases.make_base), for the tests of
MatchPlan.knn(metric="l2").  match_cases.py does this for the L1 distance; here

    D = q * 65025 + r,   0 <= r < 65025 = 255 ** 2

q bytes differ from the base by the full 255 and r is written as at most four squares (Lagrange; r < 255 ** 2, so every root is
at most 254), each on a byte of its own.  The bytes are at random positions and differ in the direction the base allows (up from
0, down from 255).  q + (number of squares) must fit the 128 bytes: that is asserted, and so is the distance that comes out.
(Every D up to 124 * 65025 + 65024 fits whatever r is; above, r has to be a sum of 128 - q squares: 8 323 200 itself is q = 128,
r = 0.)

numpy only, deterministic from seeds, nothing here imports the package.
"""
import functools
import math

import numpy as np

import match_cases as mc

SQ = 255 * 255                              # 65 025
DMAX = 128 * SQ                             # 8 323 200 = 0x7F0100: the largest squared distance of two descriptors


@functools.lru_cache(maxsize=None)
def four_squares(r):
    """non-zero roots (descending, at most four) whose squares sum to r"""
    assert 0 <= r < SQ
    for a in range(math.isqrt(r), -1, -1):
        ra = r - a * a
        for b in range(min(a, math.isqrt(ra)), -1, -1):
            rb = ra - b * b
            if rb > 2 * b * b:              # c <= b and d <= b cannot reach it
                break
            for c in range(min(b, math.isqrt(rb)), -1, -1):
                rc = rb - c * c
                if rc > c * c:
                    break
                d = math.isqrt(rc)
                if d * d == rc:
                    return tuple(v for v in (a, b, c, d) if v)
    raise AssertionError("no four squares for %d" % r)


def descs_at(base, dists, rng):
    """(n, 128) uint8 descriptors, row k at squared Euclidean distance dists[k] from `base` exactly"""
    d = np.atleast_1d(np.asarray(dists, np.int64))
    assert d.ndim == 1 and (d >= 0).all() and (d <= DMAX).all()
    base = np.asarray(base, np.uint8)
    assert base.shape == (128,) and np.isin(base, (0, 255)).all()
    out = np.repeat(base[None, :], len(d), axis=0)
    for k, D in enumerate(d.tolist()):
        q, r = divmod(D, SQ)
        roots = four_squares(r)
        assert q + len(roots) <= 128, "D = %d needs %d + %d bytes" % (D, q, len(roots))
        delta = np.array([255] * q + list(roots), np.int64)
        pos = rng.permutation(128)[:len(delta)]
        out[k, pos] = np.where(base[pos] == 0, delta, 255 - delta).astype(np.uint8)
    assert (l2(base, out) == d).all()
    return out


def l2(base, descs):
    """int64 squared Euclidean distances of the rows of `descs` to `base`"""
    a = np.asarray(descs).astype(np.int64) - np.asarray(base).astype(np.int64)
    return (a * a).sum(axis=-1)


def far_dists(n, lo, rng):
    """n distances in [lo, DMAX] of the form q * 65025 + s * s, which fit whatever q is"""
    lo = min(int(lo), DMAX)
    q = rng.integers(min(lo // SQ, 127), 128, n)
    s = rng.integers(0, 255, n)
    d = q * SQ + s * s
    d[d < lo] = DMAX
    return d


def planted(base, n2, plant, rng, far_lo=None):
    """a list of n2 elements: element j at squared distance plant[j] from `base`, every other one far (above the largest planted
    distance, or from `far_lo` on)"""
    lo = (max(plant.values()) + 1 if plant else DMAX // 2) if far_lo is None else far_lo
    d = far_dists(n2, lo, rng)
    for j, v in plant.items():
        d[j] = v
    return mc.records(descs_at(base, d, rng))


def reversing_pair(rng):
    """(query, near_l1, near_l2): `near_l1` differs from the query in one byte by 100 (L1 100, squared L2 10 000), `near_l2` in 120
    bytes by 1 (L1 120, squared L2 120): the two metrics rank them in opposite orders"""
    query = rng.integers(100, 156, 128).astype(np.uint8)
    near_l1 = query.copy(); near_l2 = query.copy()
    near_l1[int(rng.integers(0, 128))] += 100
    pos = rng.permutation(128)[:120]
    near_l2[pos] = (near_l2[pos].astype(np.int64) + rng.choice([-1, 1], 120)).astype(np.uint8)
    return query, near_l1, near_l2
