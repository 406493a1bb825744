"""CPU tests of the numpy restatement of the device median (tests/shift_ref.py): the restatement the
GPU results are compared with bit for bit must itself be numpy.median of the float32 displacements, the value the host path of
LinearAlign.align takes.  `==` per axis; the sign of a zero is left open, since numpy's partition does not order -0.0 and +0.0."""
import numpy as np
import pytest

import shift_ref as sr

SIZES = list(range(1, 41)) + [255, 256, 257, 1000, 70001]


def host_median(pts, used):
    """the host path: LinearAlign._median_shift on the gathers of the used pairs"""
    g0, g1 = pts[used][:, :2], pts[used][:, 2:]
    with np.errstate(all="ignore"):
        delta = g1 - g0
        return np.median(delta[:, 0]), np.median(delta[:, 1])


def pts_of(dx, dy):
    z = np.zeros_like(dx)
    return np.stack([z, z, dx, dy], axis=1).astype(np.float32)


@pytest.mark.parametrize("n", SIZES)
def test_restatement_is_numpy_median(n):
    sets = sr.value_sets(n, 1000 + n)
    cases = [(name, pts_of(v, v[::-1].copy() if name != "normal" else np.roll(v, 1) * np.float32(0.5))) for name, v in sets.items()]
    # positions of random finite bit patterns on both sides: the differences themselves overflow to +-inf now and then
    a, b = sr.value_sets(n, 2000 + n)["bits"], sr.value_sets(n, 3000 + n)["bits"]
    m = min(len(a), len(b))
    cases.append(("bits - bits", np.stack([a[:m], b[:m], b[:m], a[:m]], axis=1)))
    for name, pts in cases:
        used = sr.used_pairs(pts)
        out, counts, keep = sr.shift_pts(pts)
        assert out.dtype == np.float32 and counts[0] == used.sum() == pts.shape[0] and counts[1] == 0 and keep is None
        want = host_median(pts, used)
        for axis in (0, 1):
            assert type(want[axis]) is np.float32
            got = out[sr.MDX + axis]
            assert got == want[axis] or (np.isnan(got) and np.isnan(want[axis])), (name, n, axis, got, want[axis])
            lo, hi = out[sr.LO_DX + 2 * axis], out[sr.HI_DX + 2 * axis]
            d = pts[:, 2 + axis] - pts[:, axis] if name != "bits - bits" else None
            if d is not None:                                                 # the ranks are the sorted values' middle ones
                s = np.sort(d)
                assert lo == s[(n - 1) // 2] and hi == s[n // 2], (name, n, axis)


def test_large_values_do_not_overflow_for_an_odd_count():
    """numpy takes the mean of ONE element for odd n: 3e38 stays 3e38, where (lo + lo) * 0.5 would be inf"""
    pts = pts_of(np.float32([3e38, -3e38, 3e38]), np.float32([1.0, 3e38, 2.0]))
    out, counts, _ = sr.shift_pts(pts)
    assert out[sr.MDX] == np.float32(3e38) == np.median(pts[:, 2]) and out[sr.MDY] == np.float32(2.0)
    out, counts, _ = sr.shift_pts(pts_of(np.float32([3e38, 3e38]), np.float32([-3e38, 3e38])))
    with np.errstate(all="ignore"):
        assert np.isinf(out[sr.MDX]) and np.isinf(np.median(np.float32([3e38, 3e38])))     # even n: the sum overflows in both
        assert out[sr.MDY] == 0.0


def test_key_order_is_the_total_order_of_float32():
    v = np.float32([np.inf, 1.5, 1e-45, 0.0, -0.0, -1e-45, -1.5, -3.4e38, -np.inf])
    k = sr.key(v)
    assert (np.diff(k.astype(np.int64)) < 0).all()                               # strictly descending as listed
    assert np.array_equal(sr.unkey(k).view(np.uint32), v.view(np.uint32))
    med, lo, hi = sr.middle(np.float32([0.0, -0.0]))
    assert np.signbit(lo) and not np.signbit(hi) and med == 0.0
    med, lo, hi = sr.middle(np.float32([-0.0, 0.0, 5.0, -5.0]))
    assert np.signbit(lo) and lo == 0 and not np.signbit(hi) and hi == 0


@pytest.mark.parametrize("tol", [0.0, 0.5, np.inf])
def test_keep_against_a_direct_expression(tol):
    kp1, kp2, pairs, truth = sr.make_case(1000, 4, 0.1, 16384.0)
    pts = sr.gather(kp1, kp2, pairs)
    tied = np.arange(1000) % 5 != 0                                               # a tied middle, so that tol = 0 keeps something
    pts[tied, :2] = (100.0, 200.0); pts[tied, 2:] = (102.0, 199.0)
    mask = np.random.default_rng(5).random(1000) < 0.7
    for msk in (None, mask):
        out, counts, keep = sr.shift_pts(pts, msk, tol)
        used = np.ones(1000, bool) if msk is None else msk
        dx, dy = pts[:, 2] - pts[:, 0], pts[:, 3] - pts[:, 1]
        mdx, mdy = np.median(dx[used]), np.median(dy[used])
        want = used & (np.abs(dx - mdx) <= np.float32(tol)) & (np.abs(dy - mdy) <= np.float32(tol))
        assert keep.dtype == np.bool_ and np.array_equal(keep, want) and counts[1] == want.sum() > 500 and counts[0] == used.sum()
        if tol == np.inf:
            assert np.array_equal(keep, used)


def test_a_non_finite_median_keeps_nothing():
    out, counts, keep = sr.shift_pts(pts_of(np.float32([np.inf, np.inf, 1.0]), np.float32([0.0, 1.0, 2.0])), None, np.inf)
    assert out[sr.MDX] == 1.0 and counts[0] == 1 and keep.tolist() == [False, False, True]   # an infinite coordinate: no used pair
    big = np.float32(3e38)
    out, counts, keep = sr.shift_pts(np.float32([[-big, 0, big, 1], [-big, 0, big, 2], [-big, 0, big, 3]]), None, np.inf)
    assert np.isinf(out[sr.MDX]) and out[sr.MDY] == 2.0 and counts[0] == 3 and counts[1] == 0 and not keep.any()


def test_empty():
    kp1, kp2, pairs, truth = sr.make_case(300, 11)
    pts = sr.gather(kp1, kp2, pairs)
    for out, counts, keep in (sr.shift_pts(pts[:0], None, 1.0), sr.shift_pts(pts, np.zeros(300, np.uint8), 1.0),
                              sr.shift_pts(np.full((9, 4), np.nan, np.float32), None, 1.0)):
        assert np.isnan(out).all() and out.shape == (6,) and (counts == 0).all() and not keep.any()


def test_voided_pairs_are_dropped_and_any_non_zero_mask_byte_counts():
    kp1, kp2, pairs, truth = sr.make_case(1000, 12)
    bad = pairs.copy()
    bad[3, 0] = -1; bad[500, 0] = len(kp1); bad[999, 1] = len(kp2)
    kp1 = kp1.copy(); kp2 = kp2.copy()
    kp1["x"][pairs[10, 0]] = np.nan; kp1["y"][pairs[11, 0]] = np.inf; kp2["x"][pairs[12, 1]] = -np.inf
    out, counts, _ = sr.shift(kp1, kp2, bad)
    good = np.ones(1000, bool); good[[3, 500, 999, 10, 11, 12]] = False
    assert counts[0] == 994
    pts = sr.gather(kp1, kp2, pairs)
    assert (out[sr.MDX], out[sr.MDY]) == host_median(pts, good)
    assert sr.same_bits(sr.shift(kp1, kp2, pairs, good)[0], out)
    assert sr.same_bits(sr.shift(kp1, kp2, bad, np.full(1000, 0x80, np.uint8))[0], out)
    assert sr.same_bits(sr.shift(kp1, kp2, bad, np.ones(1000, bool))[0], out)


def test_lists_from_displacements_are_exact():
    d = np.float32([-0.0, 0.0, 1e-45, -3e-42, 7.25, -np.float32(3.4e38)])
    kp1, kp2, pairs = sr.lists_from_displacements(d, seed=3)
    pts = sr.gather(kp1, kp2, pairs)
    assert np.array_equal((pts[:, 2] - pts[:, 0]).view(np.uint32), d.view(np.uint32))
    assert np.array_equal((pts[:, 3] - pts[:, 1]).view(np.uint32), d[::-1].view(np.uint32))
