"""tests/golden/math_hard.npz reaches the rules it was built for (no GPU): every stored argument still lies in the band of
its label when the distance is recomputed with the live oracle, every stratum x band holds its count with both sides of the
half-way pattern and every sign / fold / k, and every range case lies outside the fast paths' guarded range.  If the oracle's
binary64 sequence changes, the labels move and this fails: regenerate with tests/golden/make_math_hard.py."""
import numpy as np
import pytest

import math_hard_cases as mh

BANDS = (mh.H0, mh.H1, mh.G, mh.S)


@pytest.fixture(scope="module")
def fx():
    return mh.load()


@pytest.fixture(scope="module")
def exp_v(fx, oracle):
    return oracle.expf_f64_array(fx["exp_x"])


@pytest.fixture(scope="module")
def atan2_v(fx, oracle):
    return oracle.atan2f_f64_array(fx["atan2_y"], fx["atan2_x"])


def _want(func, stratum, band):
    return min(mh.MIN_COUNT[band], mh.EXP_AVAILABLE.get((stratum, band), 1 << 30)) if func == "exp" else mh.MIN_COUNT[band]


def _both_sides(oracle, v, sel, what):
    """low bits below and above the half-way pattern 2^28; in G also below and above the guard's 8192"""
    up = oracle.boundary_side(v[sel])
    assert up.any() and (~up).any(), what


def test_boundary_distance_is_the_distance_on_the_bits(oracle):
    half = np.array([1.0 + 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52, 1.0 + 2.0 ** -24 - 5 * 2.0 ** -52, 1.0, 1.0 + 2.0 ** -23,
                     -(2.0 ** -100) * (1.0 + 3 * 2.0 ** -24 + 100 * 2.0 ** -52)])
    assert list(oracle.boundary_distance(half)) == [0, 1, 5, 1 << 28, 1 << 28, 100]
    assert list(oracle.boundary_side(half)) == [False, True, False, False, False, True]
    # the float conversion flips exactly at distance 0: one binary64 ulp below the half-way point rounds down, one above rounds up
    assert np.float32(half[2]) == np.float32(1.0) and np.float32(half[1]) == np.float32(1.0 + 2.0 ** -23)


def test_f64_entry_points_round_to_the_float_functions(fx, oracle, exp_v, atan2_v):
    assert np.array_equal(exp_v.astype(np.float32).view(np.uint32), oracle.expf_array(fx["exp_x"]).view(np.uint32))
    assert np.array_equal(atan2_v.astype(np.float32).view(np.uint32), oracle.atan2f_array(fx["atan2_y"], fx["atan2_x"]).view(np.uint32))
    rx = fx["exp_range_x"]
    with np.errstate(over="ignore"):
        a, b = oracle.expf_f64_array(rx).astype(np.float32), oracle.expf_array(rx)
    assert np.array_equal(a.view(np.uint32)[~np.isnan(b)], b.view(np.uint32)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))
    ry, rx = fx["atan2_range_y"], fx["atan2_range_x"]
    a, b = oracle.atan2f_f64_array(ry, rx).astype(np.float32), oracle.atan2f_array(ry, rx)
    assert np.array_equal(a.view(np.uint32)[~np.isnan(b)], b.view(np.uint32)[~np.isnan(b)]) and np.array_equal(np.isnan(a), np.isnan(b))


def test_array_entry_points_equal_the_scalar_ones(oracle):
    rng = np.random.default_rng(5)
    x = np.concatenate([(rng.standard_normal(2000) * 10.0 ** rng.integers(-3, 3, 2000)).astype(np.float32),
                        np.array([0, -0.0, 128, -150, -151, 129, np.inf, -np.inf, np.nan, 2.0 ** 30, 1.5 * 2.0 ** 30, -2.0 ** 31, 3e38], np.float32)])
    L = oracle.lib()
    import ctypes as C
    s, c = C.c_float(), C.c_float()
    e2, sn, cs = oracle.exp2f_array(x), *oracle.sincosf_array(x)
    for i, v in enumerate(x):
        L.so_sincosf(C.c_float(v), C.byref(s), C.byref(c))
        for got, ref in ((e2[i], L.so_exp2f(C.c_float(v))), (sn[i], s.value), (cs[i], c.value)):
            assert (np.isnan(got) and np.isnan(ref)) or np.float32(got).view(np.uint32) == np.float32(ref).view(np.uint32), (v, got, ref)
    # sin / cos are total: NaN for both beyond 2^30 (the quadrant number would leave the int range), finite up to it
    big = np.abs(x) > np.float32(2.0 ** 30)
    assert np.isnan(sn[big | np.isnan(x)]).all() and np.isnan(cs[big | np.isnan(x)]).all()
    assert np.isfinite(sn[~big & ~np.isnan(x)]).all() and np.isfinite(cs[~big & ~np.isnan(x)]).all()


def test_every_label_still_holds(fx, oracle, exp_v, atan2_v):
    for name, v in (("exp", exp_v), ("atan2", atan2_v)):
        band = mh.band_of(oracle.boundary_distance(v))
        stored = fx[name + "_band"]
        claimed = stored != mh.NO_BAND
        assert np.array_equal(band[claimed], stored[claimed]), name
        f = np.abs(v.astype(np.float32))
        assert (f >= mh.F32_MIN_NORMAL).all() and np.isfinite(f).all(), name           # d is meaningful: normal binary32 results
    assert mh.exp_in_range(fx["exp_x"]).all()
    assert mh.atan2_in_range(fx["atan2_y"], fx["atan2_x"]).all()
    # the unclaimed arguments are 80.0f and its inner neighbours
    edge = fx["exp_x"][fx["exp_band"] == mh.NO_BAND]
    assert np.array_equal(np.sort(edge.view(np.uint32)), np.sort(mh.exp_edge_inside().view(np.uint32)))
    assert (fx["exp_stratum"][fx["exp_band"] == mh.NO_BAND] == 2).all()


@pytest.mark.parametrize("stratum", [0, 1, 2])
def test_exp_strata_reach_their_counts(fx, oracle, exp_v, stratum):
    x, st, band = fx["exp_x"], fx["exp_stratum"], fx["exp_band"]
    mine = st == stratum
    assert np.unique(x[mine].view(np.uint32)).size == mine.sum()
    if stratum == 0:
        assert ((x[mine] >= -12) & (x[mine] <= 0)).all()
    elif stratum == 1:
        k, off = mh.exp_window(x[mine])
        assert (np.abs(off) <= 0.0166).all() and (k >= -115).all() and (k <= 114).all()
        # the end of the reduction interval: |r| >= ln2 / 2 - 0.0166 = 0.32997 (0.33 to two places)
        assert (np.abs(mh.exp_reduction(x[mine])[1]) > mh.LN2 / 2 - 0.0166 - 1e-9).all()
    for b in BANDS:
        sel = mine & (band == b)
        assert sel.sum() >= _want("exp", stratum, b), (stratum, mh.BAND_NAMES[b], int(sel.sum()))
        if sel.sum() >= 20:
            _both_sides(oracle, exp_v, sel, (stratum, b))
            if stratum == 1:
                r = mh.exp_reduction(x[sel])[1]
                assert (r > 0).any() and (r < 0).any()
            if stratum == 2:
                assert (x[sel] > 0).any() and (x[sel] < 0).any()
    d = oracle.boundary_distance(exp_v)
    g = mine & (band == mh.G)
    assert (d[g] < mh.GUARD).any() and (d[g] > mh.GUARD).any()
    if stratum == 1:
        k = mh.exp_window(x[mine])[0]
        assert k.min() <= -100 and k.max() >= 100 and np.unique(k).size >= 200       # the whole guarded range of k
    if stratum == 2:
        assert np.abs(x[mine]).max() > 64 and np.abs(x[mine]).min() < 2.0 ** -20


def test_exp_window_stratum_is_complete(fx, oracle):
    """stratum (b) is a finite set (7 * 10^6 floats): the fixture holds every argument of it that lies in a band, which is why
    its counts are below the usual ones (mh.EXP_AVAILABLE)"""
    x = mh.exp_window_floats()
    assert 7_000_000 < x.size < 8_000_000
    band = mh.band_of(oracle.boundary_distance(oracle.expf_f64_array(x)))
    for b in BANDS:
        assert (band == b).sum() == mh.EXP_AVAILABLE[(1, b)]
    have = fx["exp_x"][fx["exp_stratum"] == 1]
    assert np.array_equal(np.sort(x[band != mh.NO_BAND].view(np.uint32)), np.sort(have.view(np.uint32)))


@pytest.mark.parametrize("stratum", [0, 1, 2])
def test_atan2_strata_reach_their_counts(fx, oracle, atan2_v, stratum):
    y, x, st, band = fx["atan2_y"], fx["atan2_x"], fx["atan2_stratum"], fx["atan2_band"]
    mine = st == stratum
    key = y.view(np.uint32).astype(np.uint64) << np.uint64(32) | x.view(np.uint32).astype(np.uint64)
    assert np.unique(key[mine]).size == mine.sum()
    fold, k, t = mh.atan2_fold(y, x)
    ay, ax = np.abs(y), np.abs(x)
    mn, mx = np.minimum(ay, ax).astype(np.float64), np.maximum(ay, ax).astype(np.float64)
    if stratum == 0:
        assert (ay[mine] <= 255).all() and (ax[mine] <= 255).all()
    elif stratum == 1:
        centre = (np.floor(mn / mx * 8.0) + 0.5) / 8.0
        assert (np.abs(mn / mx - centre)[mine] <= 2.0 ** -10).all()
        # the end of an octant interval: |min / max - k / 8| >= 1/16 - 2^-10, i.e. |t| >= (1/16 - 2^-10) / (1 + c min / max),
        # which is above 0.058 for the first intervals and above 0.03 for all (c <= 1)
        assert (np.abs(mn / mx - k * 0.125)[mine] >= 1.0 / 16 - 2.0 ** -10 - 2.0 ** -24).all()
        assert (np.abs(t[mine]) > 0.03).all() and (np.abs(t[mine & (mn / mx < 0.19)]) > 0.058).all()
    else:
        big = [mh.step(1e18, -j) for j in range(3)]
        small = [mh.step(1e-18, j) for j in range(3)]
        pinned = np.isin(np.maximum(ay, ax), big) | np.isin(np.minimum(ay, ax), small)
        assert pinned[mine].all()
    d = oracle.boundary_distance(atan2_v)
    for b in BANDS:
        sel = mine & (band == b)
        assert sel.sum() >= _want("atan2", stratum, b), (stratum, mh.BAND_NAMES[b], int(sel.sum()))
        _both_sides(oracle, atan2_v, sel, (stratum, b))
        assert np.unique(mh.sign_combo(y[sel], x[sel])).size == 4
        assert np.unique(fold[sel]).size == 4
        if stratum == 0:
            assert (ay[sel] > ax[sel]).any() and (ay[sel] < ax[sel]).any()
        elif stratum == 1:
            centre_k = np.floor(mn[sel] / mx[sel] * 8.0).astype(np.int64)
            assert np.array_equal(np.unique(centre_k), np.arange(8))
            assert np.unique(k[sel]).size == 9                                            # both ends of every interval
        else:
            for p in big:
                assert (np.maximum(ay[sel], ax[sel]) == p).any()
            for p in small:
                assert (np.minimum(ay[sel], ax[sel]) == p).any()
            ratio = mn[sel] / mx[sel]
            assert (ratio >= 2.0 ** -5).any() and (ratio < 2.0 ** -20).any()
    g = mine & (band == mh.G)
    assert (d[g] < mh.GUARD).any() and (d[g] > mh.GUARD).any()
    if stratum == 1:                                                                      # every interval end in every fold
        assert np.unique(fold[mine] * 16 + k[mine]).size == 4 * 9


def test_range_cases_lie_outside_the_guarded_range(fx, oracle):
    x = fx["exp_range_x"]
    assert not mh.exp_in_range(x).any()
    out = oracle.expf_array(x)
    assert np.isnan(x).any() and np.isinf(x).any() and (x > 0).any() and (x < 0).any()
    assert ((out > 0) & (out < mh.F32_MIN_NORMAL)).any() and (out == 0).any() and np.isinf(out).any()     # sub-normal, flushed, overflowed
    for v in (mh.step(80.0, 1), mh.step(80.0, 2), -mh.step(80.0, 1), -mh.step(80.0, 2),   # just past 80.0f; both sides of 89 and -104
              np.float32(89.0), mh.step(89.0, 1), -mh.step(104.0, -1), np.float32(-104.0), -mh.step(104.0, 1)):
        assert (x == v).any(), v
    y, x = fx["atan2_range_y"], fx["atan2_range_x"]
    assert not mh.atan2_in_range(y, x).any()
    ay, ax = np.abs(y), np.abs(x)
    out = oracle.atan2f_array(y, x)
    assert ((np.abs(out) > 0) & (np.abs(out) < mh.F32_MIN_NORMAL)).any()                  # results that are sub-normal in binary32
    for p in (mh.step(1e18, 1), mh.step(1e18, 2)):
        assert (np.fmax(ay, ax) == p).any()
    for p in (mh.step(1e-18, -1), mh.step(1e-18, -2)):
        assert (np.fmin(ay, ax) == p).any()
    assert ((ay == 0) & (ax == 0)).any() and ((ay == 0) & (ax > 0)).any() and ((ax == 0) & (ay > 0)).any()
    assert np.isnan(y).any() and np.isnan(x).any() and np.isinf(y).any() and np.isinf(x).any()


def test_fixture_size():
    import os
    assert os.path.getsize(mh.PATH) < 400_000
