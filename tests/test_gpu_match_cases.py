"""GPU tests of the rule both matchers share -- nearest and second nearest L1 distance, the earliest index among equal minima,
(i, best) emitted iff dist2 != 0 and dist1 / dist2 < ratio_th in float32 -- on lists with PRESCRIBED distances
(tests/match_cases.py): match_partial_kernel / match_merge_kernel (k_match.hpp) and the tail of mw_match_kernel
(k_match_window.hpp), through MatchPlan.match and, for a ratio_th of the test's choice, through siftmi_match_ex and
siftmi_match_window directly.

The expected pairs are the oracle's (oracle.match_ex; tests/test_match_cases_host.py pins it to the numpy restatement, to the
answer each construction dictates and to the reference's own kernel on the same lists).  Every comparison is exact: the sorted
pair rows, n_out and n_total.  The queries of most cases are 600 copies of one descriptor (both register slots of a lane, two
query blocks, a partial last wave): the oracle is then asked about one of them and the answer repeated."""
import ctypes as C

import numpy as np
import pytest

import match_cases as mc
import window_ref as wr
from util import sort_rows

pytestmark = pytest.mark.gpu
N1 = 600
INF = float("inf")


def rows_of(pairs):
    return sort_rows(np.asarray(pairs, np.int32).reshape(-1, 2))


# ---------------------------------------------------------------------------------------------- the C ABI with a free ratio_th
def abi_match_ex(siftlib, mp, a, b, th, roi_mode=0, mutual=False, capacity=None):
    """(rc, pairs[:n_out], n_out, n_total) of siftmi_match_ex"""
    cap = max(1, len(a)) if capacity is None else capacity
    pairs = np.full((max(1, cap), 2), -7, np.int32)
    n, total = C.c_int64(-5), C.c_int64(-5)
    rc = siftlib.siftmi_match_ex(mp._handle, a.ctypes.data, len(a), 0, b.ctypes.data, len(b), 0, C.c_float(float(th)), roi_mode,
                                 int(mutual), pairs.ctypes.data, cap, C.byref(n), C.byref(total))
    assert (pairs[n.value:] == -7).all()                             # nothing written beyond n_out
    return rc, pairs[:n.value].copy(), n.value, total.value


def abi_match_window(siftlib, mp, a, b, th, window, shift=(0.0, 0.0), mutual=False, capacity=None):
    cap = max(1, len(a)) if capacity is None else capacity
    pairs = np.full((max(1, cap), 2), -7, np.int32)
    n, total = C.c_int64(-5), C.c_int64(-5)
    wx, wy = window if hasattr(window, "__len__") else (window, window)
    rc = siftlib.siftmi_match_window(mp._handle, a.ctypes.data, len(a), 0, b.ctypes.data, len(b), 0, C.c_float(float(th)), C.c_float(wx),
                                     C.c_float(wy), C.c_float(shift[0]), C.c_float(shift[1]), int(mutual), pairs.ctypes.data, cap,
                                     C.byref(n), C.byref(total))
    assert (pairs[n.value:] == -7).all()
    return rc, pairs[:n.value].copy(), n.value, total.value


def same(result, want, what):
    """an entry point's (rc, pairs, n_out, n_total) against the expected rows, exactly"""
    rc, pairs, n, total = result
    assert rc == 0, what
    assert n == total == len(want), "%s: n_out %d, n_total %d, expected %d pairs" % (what, n, total, len(want))
    assert np.array_equal(rows_of(pairs), want), what


def same_plan(got, want, what):
    assert got.dtype == np.int32 and got.shape == (len(want), 2), "%s: %s pairs, expected %d" % (what, got.shape, len(want))
    assert np.array_equal(rows_of(got), want), what


def expect(oracle, c):
    """the oracle's sorted rows for a case (asked about ONE query where they are all the same record), checked against the
    answer the construction dictates where it dictates one"""
    short = c.identical and not c.mutual
    a = c.a[:1] if short else c.a
    want, n = oracle.match_ex(a, c.b, c.roi, c.roi_mode, mutual=c.mutual, ratio_th=c.th, cap=max(1, len(a)))
    assert n == len(want)
    want = rows_of(want)
    if short and n:
        want = np.stack([np.arange(len(c.a)), np.full(len(c.a), want[0, 1])], axis=1).astype(np.int32)
    if c.best is not mc.UNKNOWN and not c.mutual:
        assert np.array_equal(want, c.expected_rows()), c.name
    return want


def is_default(th):
    return np.float32(th).tobytes() == mc.RATIO.tobytes()


def run_plain(siftlib, oracle, mp, c, finite=True):
    """one case through every entry point that can take it; returns the expected rows"""
    want = expect(oracle, c)
    if is_default(c.th):
        same_plan(mp.match(c.a, c.b, raw_results=True), want, c.name + " [MatchPlan.match]")
        same_plan(mp.match(c.a, c.b, raw_results=True, window=INF), want, c.name + " [MatchPlan.match window=inf]")
    same(abi_match_ex(siftlib, mp, c.a, c.b, c.th), want, c.name + " [siftmi_match_ex]")
    same(abi_match_window(siftlib, mp, c.a, c.b, c.th, INF), want, c.name + " [siftmi_match_window inf]")
    if finite:      # every keypoint of these lists sits on one position: a finite window admits them all
        same(abi_match_window(siftlib, mp, c.a, c.b, c.th, (2.0, 0.0)), want, c.name + " [siftmi_match_window (2, 0)]")
    return want


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


# ---------------------------------------------------------------------------------------------- the threshold edge
@pytest.mark.parametrize("name", ["ratio default", "ratio 0.5", "ratio 1.0", "odd thresholds"])
def test_ratio_edge(siftlib, oracle, mp, name):
    """every critical (dist1, dist2) of the threshold planted among far elements: brute force, windowed with an infinite window,
    and a finite window over lists whose keypoints sit on four spots (the restatement says what each query sees there)"""
    paired = 0
    for k, c in enumerate(mc.family(name, N1)):
        paired += len(run_plain(siftlib, oracle, mp, c)) > 0
        if name == "ratio default" or k % 4 == 0:
            a, b = mc.spread_over_spots(c)
            want = rows_of(wr.match(a, b, mc.SPOT_WINDOW, ratio_th=c.th))
            same(abi_match_window(siftlib, mp, a, b, c.th, mc.SPOT_WINDOW), want, c.name + " [four spots, window 3]")
            if is_default(c.th):
                same_plan(mp.match(a, b, raw_results=True, window=mc.SPOT_WINDOW), want, c.name + " [four spots, MatchPlan.match]")
    assert paired >= (0 if name == "ratio 0.5" else 5)


# ---------------------------------------------------------------------------------------------- ties
@pytest.mark.parametrize("n2", [n for n in mc.SIZES if n > 1])
def test_ties_made_visible(siftlib, oracle, mp, n2):
    """ratio_th = 2: a tie for the minimum emits a pair and its second index is the tie-break -- two and three equal minima on
    both sides of every tile and partition edge, one in every tile, a constant list.  Brute force, windowed (infinite window, a
    finite one with the tied elements on one position, and with them in different cells, the earliest in the later cell)."""
    for c in mc.family("ties %d" % n2, N1):
        want = run_plain(siftlib, oracle, mp, c)
        assert len(want) == N1 and (want[:, 1] == min(c.planted)).all(), c.name
        a, b = mc.tied_in_different_cells(c)
        same(abi_match_window(siftlib, mp, a, b, c.th, mc.SPOT_WINDOW), want, c.name + " [tied elements in different cells]")


def test_ties_in_the_reverse_scan(siftlib, oracle, mp):
    """mutual=True with duplicates in list 1: nearest[j] of the reverse scan must be the earlier of the two, so of the copies that
    pair with the planted minimum exactly the first survives"""
    for c in mc.mutual_cases():
        want = expect(oracle, c)
        i_a, i_b = c.planted
        assert [i_a, 70] in want.tolist() and [i_b, 70] not in want.tolist()
        same_plan(mp.match(c.a, c.b, raw_results=True, mutual=True), want, c.name + " [MatchPlan.match]")
        same_plan(mp.match(c.a, c.b, raw_results=True, mutual=True, window=INF), want, c.name + " [MatchPlan.match window=inf]")
        same(abi_match_ex(siftlib, mp, c.a, c.b, c.th, mutual=True), want, c.name + " [siftmi_match_ex]")
        same(abi_match_ex(siftlib, mp, c.a, c.b, 2.0, mutual=True), rows_of(oracle.match_ex(c.a, c.b, None, 0, mutual=True, ratio_th=2.0)[0]),
             c.name + " [siftmi_match_ex, ratio 2]")
        # the duplicates in different cells of the reverse scan's grid, the earlier one in the later cell
        a = c.a.copy()
        a["x"][i_a] = 2.0; a["x"][i_b] = -2.0
        want_w = rows_of(wr.match(a, c.b, mc.SPOT_WINDOW, mutual=True, ratio_th=c.th))
        assert [i_a, 70] in want_w.tolist() and [i_b, 70] not in want_w.tolist()
        same(abi_match_window(siftlib, mp, a, c.b, c.th, mc.SPOT_WINDOW, mutual=True), want_w, c.name + " [windowed, two cells]")


# ---------------------------------------------------------------------------------------------- placement
@pytest.mark.parametrize("n2", mc.SIZES)
def test_placement(siftlib, oracle, mp, n2):
    """a passing and a failing (minimum, second) pair at every placement: both orders, both sides of every tile / partition edge,
    one tile, adjacent tiles, a later tile behind far elements only"""
    outcomes = set()
    for c in mc.family("placement %d" % n2, N1):
        outcomes.add(len(run_plain(siftlib, oracle, mp, c, finite=n2 <= 320)) > 0)
    assert outcomes == ({True} if n2 == 1 else {True, False})


def test_extremes(siftlib, oracle, mp):
    """distance 0 against a positive second (pairs) and against another 0 (never); one element (always, also at 32 640);
    everything at 32 640 = 0x7F80, just under the packed key's sentinel; 32 639 against 32 640 at ratio 1 and 2"""
    n = 0
    for c in mc.family("extremes", N1):
        run_plain(siftlib, oracle, mp, c)
        n += 1
    assert n > 60


# ---------------------------------------------------------------------------------------------- flags
def test_flags(siftlib, oracle):
    """the FLAGS template of match_partial_kernel (roi_mode 1 and 2; the positions choose the flags): the planted minimum
    excluded, whole aligned runs of 256 and 64 elements excluded, every element excluded (every partial empty), a forced zero
    before and after a true zero, dropped queries between kept ones"""
    import sift_pyocl_amd as sp
    mp = sp.MatchPlan()
    mp.set_roi(mc.ROI)
    seen = set()
    for c in mc.flag_cases(N1):
        want = expect(oracle, c)
        same(abi_match_ex(siftlib, mp, c.a, c.b, c.th, c.roi_mode, c.mutual), want, c.name + " [siftmi_match_ex]")
        if is_default(c.th):
            same_plan(mp.match(c.a, c.b, raw_results=True, roi_mode=c.roi_mode, mutual=c.mutual), want, c.name + " [MatchPlan.match]")
        seen.add((c.roi_mode, len(want) > 0))
    assert seen == {(1, False), (1, True), (2, False), (2, True)}


# ---------------------------------------------------------------------------------------------- capacity
def test_capacity_of_the_brute_force_matcher(siftlib):
    """600 identical queries that all pair, a plan of 16: n_total is 600, 16 rows come back, each (a distinct i, best); a caller
    capacity of 3 is SIFTMI_ECAPACITY with 3 rows; a call with min(n1, n2) = 40 raises the plan's size to 40 for good.  Which rows
    survive a truncation is the atomics' business and not asserted."""
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    rng = np.random.default_rng(8)
    base = mc.make_base(rng)
    a = mc.queries(base, N1)
    b = mc.planted(base, 2, {1: 100, 0: 5000}, rng)

    def check_rows(pairs, count):
        assert pairs.shape == (count, 2) and (pairs[:, 1] == 1).all()
        assert len(set(pairs[:, 0].tolist())) == count and pairs[:, 0].min() >= 0 and pairs[:, 0].max() < N1

    small = sp.MatchPlan(size=16)
    check_rows(small.match(a, b, raw_results=True), 16)
    assert small.kpsize == 16
    rc, pairs, n, total = abi_match_ex(siftlib, small, a, b, mc.RATIO, capacity=16)
    assert rc == 0 and n == 16 and total == N1
    check_rows(pairs, 16)
    rc, pairs, n, total = abi_match_ex(siftlib, small, a, b, mc.RATIO, capacity=3)
    assert rc == _lib.ECAPACITY and n == 3 and total == N1
    check_rows(pairs, 3)
    rc, pairs, n, total = abi_match_ex(siftlib, small, a, b, mc.RATIO, capacity=N1)       # the plan's 16 still bound it
    assert rc == 0 and n == 16 and total == N1
    check_rows(pairs, 16)
    # a failing pair: nothing, whatever the capacity
    rc, pairs, n, total = abi_match_ex(siftlib, small, a, mc.planted(base, 2, {1: 4900, 0: 5000}, rng), mc.RATIO, capacity=3)
    assert rc == 0 and n == 0 and total == 0
    # min(n1, n2) beyond the plan's size: kpsize grows to it and every pair comes back (match.py: kpsize = min(n1, n2))
    b40 = mc.planted(base, 50, {7: 100, 8: 5000}, rng)
    got = small.match(a[:40], b40, raw_results=True)
    assert small.kpsize == 40
    assert np.array_equal(rows_of(got), np.stack([np.arange(40), np.full(40, 7)], axis=1))
    # ... and stays grown, as the reference's kpsize does: the next call keeps up to 40 pairs, also in the windowed matcher
    check_rows(small.match(a, b, raw_results=True), 40)
    rc, pairs, n, total = abi_match_ex(siftlib, small, a, b, mc.RATIO, capacity=N1)
    assert rc == 0 and n == 40 and total == N1
    check_rows(pairs, 40)
    rc, pairs, n, total = abi_match_window(siftlib, small, a, b, mc.RATIO, INF, capacity=N1)
    assert rc == 0 and n == 40 and total == N1
    check_rows(pairs, 40)
    big = sp.MatchPlan()                                             # the default plan holds them all
    got = big.match(a, b, raw_results=True)
    assert np.array_equal(rows_of(got), np.stack([np.arange(N1), np.full(N1, 1)], axis=1))
