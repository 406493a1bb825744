"""CPU tests of the numpy restatement of the device fit (tests/fit_ref.py): the restatement the GPU
results are compared with bit for bit must itself be a least-squares fit.  It is held against numpy.linalg.lstsq on the
(2n, 6) system, an independent solver, on every generated case."""
import numpy as np
import pytest

import fit_ref as fr


@pytest.fixture(scope="module")
def cases():
    out = []
    for M, seed, outliers, extent in fr.CASES:
        kp1, kp2, pairs, truth = fr.make_case(M, seed, outliers, extent)
        out.append((M, fr.gather(kp1, kp2, pairs), truth))
    return out


def test_case_generator_covers_what_it_claims(cases):
    for (M, seed, outliers, extent), (_, pts, truth) in zip(fr.CASES, cases):
        assert pts.shape == (M, 4) and np.isfinite(pts).all()
        assert (pts[:, :2] != np.floor(pts[:, :2])).mean() > 0.9                 # fractional parts
        assert pts[:, :2].max() <= extent
    assert max(pts[:, :2].max() for _, pts, _ in cases) > 16000.0


def test_restatement_agrees_with_lstsq_on_every_case(cases):
    worst = 0.0
    for M, pts, truth in cases:
        r = fr.fit_pts(pts)
        assert r[fr.STATUS] == fr.OK and r[fr.N] == M
        dev = float(np.abs(r[fr.MODEL] - fr.lstsq_model(pts)).max())
        print("M = %6d: largest coefficient deviation from numpy.linalg.lstsq %.3e" % (M, dev))
        worst = max(worst, dev)
        # the sum of squared residuals is the least-squares minimum: no larger than at the true map or at lstsq's
        p = pts.astype(np.float64)
        for a, b, c, d, e, f in (truth, fr.lstsq_model(pts)):
            ssr = (((a * p[:, 0] + b * p[:, 1] + c) - p[:, 2]) ** 2 + ((d * p[:, 0] + e * p[:, 1] + f) - p[:, 3]) ** 2).sum()
            assert r[fr.SSR] <= ssr * (1 + 1e-9)
    print("largest over the cases %.3e (recorded: %.3e), bound %.3e" % (worst, fr.LSTSQ_MEASURED, fr.LSTSQ_BOUND))
    assert worst <= fr.LSTSQ_BOUND


def test_masked_fit_agrees_with_lstsq_and_recovers_the_map(cases):
    """with the gross outliers masked out the fit is the true map up to the noise"""
    M, seed, outliers, extent = fr.CASES[5]
    kp1, kp2, pairs, truth = fr.make_case(M, seed, outliers, extent)
    pts = fr.gather(kp1, kp2, pairs)
    p = pts.astype(np.float64)
    err = np.hypot(truth[0] * p[:, 0] + truth[1] * p[:, 1] + truth[2] - p[:, 2], truth[3] * p[:, 0] + truth[4] * p[:, 1] + truth[5] - p[:, 3])
    mask = err < 3.0
    assert 0.6 * M < mask.sum() < M
    r = fr.fit_pts(pts, mask)
    assert r[fr.STATUS] == fr.OK and r[fr.N] == mask.sum()
    assert np.abs(r[fr.MODEL] - fr.lstsq_model(pts, mask)).max() <= fr.LSTSQ_BOUND
    assert np.allclose(r[fr.MODEL], truth, rtol=0, atol=[1e-5, 1e-5, 0.05, 1e-5, 1e-5, 0.05])
    assert 0.3 < np.sqrt(r[fr.SSR] / r[fr.N]) < 0.6                               # noise of 0.3 px per axis
    assert fr.same_bits(fr.fit_pts(pts, mask.view(np.uint8)), r)


def test_mask_of_ones_is_no_mask_bit_for_bit(cases):
    for M, pts, truth in cases:
        want = fr.fit_pts(pts)
        assert fr.same_bits(fr.fit_pts(pts, np.ones(M, np.uint8)), want)
        assert fr.same_bits(fr.fit_pts(pts, np.ones(M, bool)), want)
        assert fr.same_bits(fr.fit_pts(pts, None, fr.default_blocks(M)), want)


def test_degenerate_and_empty():
    t = np.arange(500, dtype=np.float32)
    line = np.stack([3 * t, 2 * t + 1, t, 5 * t], axis=1)
    r = fr.fit_pts(line)
    assert r[fr.STATUS] == fr.DEGENERATE and r[fr.N] == 500 and np.isnan(r[fr.MODEL]).all() and np.isnan(r[fr.SSR])
    assert np.isfinite(r[fr.MEANS]).all() and np.isfinite(r[fr.MOMENTS]).all()
    same = np.tile(np.float32([7.5, 9.25, 1.0, 2.0]), (40, 1))
    r = fr.fit_pts(same)
    assert r[fr.STATUS] == fr.DEGENERATE and (r[fr.MOMENTS] == 0).all()          # det = scale = 0: DEGENERATE with or without fmax (fit_cases.tiny_cluster: fmax decides)
    kp1, kp2, pairs, truth = fr.make_case(300, 11)
    pts = fr.gather(kp1, kp2, pairs)
    for n in (1, 2):
        r = fr.fit_pts(pts[:n])
        assert r[fr.STATUS] == fr.DEGENERATE and r[fr.N] == n
        mask = np.zeros(300, np.uint8); mask[[5, 250][:n]] = 1
        r = fr.fit_pts(pts, mask)
        assert r[fr.STATUS] == fr.DEGENERATE and r[fr.N] == n and np.isnan(r[fr.MODEL]).all()
    assert fr.fit_pts(pts[:3])[fr.STATUS] == fr.OK
    for r in (fr.fit_pts(pts, np.zeros(300, np.uint8)), fr.fit_pts(pts[:0]), fr.fit_pts(np.full((9, 4), np.nan, np.float32))):
        assert r[fr.STATUS] == fr.EMPTY and r[fr.N] == 0 and np.isnan(r[2:]).all()


def test_voided_pairs_are_skipped():
    kp1, kp2, pairs, truth = fr.make_case(1000, 12)
    bad = pairs.copy()
    bad[3, 0] = -1; bad[500, 0] = len(kp1); bad[999, 1] = len(kp2)
    kp1 = kp1.copy()
    kp1["x"][pairs[10, 0]] = np.nan; kp1["y"][pairs[11, 0]] = np.inf; kp2 = kp2.copy(); kp2["x"][pairs[12, 1]] = -np.inf
    r = fr.fit(kp1, kp2, bad)
    assert r[fr.STATUS] == fr.OK and r[fr.N] == 994
    keep = np.ones(1000, bool); keep[[3, 500, 999, 10, 11, 12]] = False
    assert np.abs(r[fr.MODEL] - fr.lstsq_model(fr.gather(kp1, kp2, pairs)[keep])).max() <= fr.LSTSQ_BOUND


def test_different_blocks_stay_within_the_bound_of_each_other(cases):
    for M, pts, truth in cases:
        models = [fr.fit_pts(pts, blocks=b)[fr.MODEL] for b in (0, 1, 2, 3, 7, 64, 1024)]
        spread = max(float(np.abs(a - b).max()) for a in models for b in models)
        print("M = %6d: largest coefficient spread over blocks %.3e" % (M, spread))
        assert spread <= fr.LSTSQ_BOUND


def test_reduction_order_is_the_contracts():
    """R on values whose sum depends on the order: the restatement must add exactly lane-serial, tree, workgroup-serial"""
    rng = np.random.default_rng(5)
    for M, B in ((1000, 1), (1000, 3), (70001, 256), (5, 2)):
        v = rng.uniform(-1, 1, M) * 10.0 ** rng.integers(-8, 8, M)
        G = B * fr.T
        lanes = [0.0] * G
        for j in range(M):
            lanes[j % G] = lanes[j % G] + float(v[j])
        total = 0.0
        for b in range(B):
            w = lanes[b * fr.T:(b + 1) * fr.T]
            s = fr.T // 2
            while s:
                for t in range(s):
                    w[t] = w[t] + w[t + s]
                s //= 2
            total = total + w[0]
        assert np.float64(total).tobytes() == np.float64(fr.reduce_R(v, B)).tobytes()
