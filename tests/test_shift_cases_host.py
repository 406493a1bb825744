"""CPU tests of the crafted match sets of the two median selects (tests/shift_cases.py): the
restatement gives every dictated result bit for bit, numpy.median agrees, and a plain Python model of the radix select -- written
from the comments of k_shift.hpp and of eb_shift_kernel, with the serial 256-bin scan of the one and the wave scan of the other
(four bins per lane, an inclusive scan over 64 lanes, the claim excl <= r < incl, the chain inside the lane) -- gives them too and
says, per selector and level, which digit it took, the rank it carried into the bin, the bin's count and the occupied bins before
it.  On that trace the reach of the families is asserted, and each listed one-line fault of the model changes a dictated result
of a named family: the GPU tests on the same sets (tests/test_gpu_shift_cases.py) would notice it in either kernel.

Faults that were asked for and that no set can show, so they are not in FAULTS (test_faults_that_cannot_be_observed_are_not holds
the model equal to the contract under them on every case):
    the sentinel counted in the first histogram      the key of an unused row, 0xffffffff, is the largest key: it falls into bin 255,
    the sentinel not skipped in later passes         the last bin of every level.  A scan compares the rank with the running count
                                                     BEFORE the end of a bin and the rank is below the count of the used keys, so
                                                     what the last bin holds beyond them is never looked at.  Counting the unused
                                                     rows shows once n counts them as well: that fault is listed in their place
"""
import numpy as np
import pytest

import shift_cases as sc
import shift_ref as sr
from consensus_ref import gather

SENTINEL = 0xFFFFFFFF
M32 = 0xFFFFFFFF
SCANS = ("serial", "wave")

#: fault -> (the scans it can be made in, the family that must show it)
FAULTS = {
    "r <= c": (SCANS, "every_digit"),
    "hi rank (n + 1) >> 1": (SCANS, "ranks"),
    "lo rank n >> 1": (SCANS, "ranks"),
    "ranks from M": (SCANS, "ranks"),
    "unused rows counted, in n and in the first histogram": (SCANS, "top_bins"),
    "key without the sign branch": (SCANS, "divergence"),
    "unkey with the branches swapped": (SCANS, "every_digit"),
    "prefix compared at low": (SCANS, "every_digit"),
    "selector 1 with selector 0's prefix": (SCANS, "divergence"),
    "y selectors read x keys": (SCANS, "every_digit"),
    "lane scan exclusive": (("wave",), "every_digit"),
    "lane scan drops lane 0's sum": (("wave",), "lane_edges"),
    "in-lane chain stops one bin early": (("wave",), "every_digit"),
    "odd median (lo + lo) * 0.5": (SCANS, "median_arithmetic"),
    "subnormals flushed in the halving": (SCANS, "median_arithmetic"),
    "< for <= in keep": (SCANS, "keep"),
    "keep with a non-finite median": (SCANS, "keep"),
    "keep from all M rows": (SCANS, "keep"),
}
UNOBSERVABLE = ("sentinel counted in the first histogram", "sentinel not skipped in later passes")


# ---------------------------------------------------------------------------------------------- the model
def m_key(v, fault):
    b = int(np.float32(v).view(np.uint32))
    if fault == "key without the sign branch":
        return b ^ 0x80000000
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def m_unkey(k, fault):
    if fault == "unkey with the branches swapped":
        b = k ^ (0xFFFFFFFF if k >> 31 else 0x80000000)
    else:
        b = k ^ (0x80000000 if k >> 31 else 0xFFFFFFFF)
    return np.uint32(b & M32).view(np.float32)


def serial_scan(bins, r, fault):
    """shift_advance: the digit is the first bin whose running count exceeds the rank"""
    r0, digit = r, 255
    for d in range(256):
        c = bins[d]
        if (r <= c) if fault == "r <= c" else (r < c):
            digit = d
            break
        r -= c
    return digit, r, dict(rank_in=r0)


LANE = np.arange(64)


def wave_scan(bins, r, fault):
    """eb_shift_kernel: lane l owns bins 4 l .. 4 l + 3; an inclusive scan of the lanes' sums by __shfl_up; the one lane whose range
    of running counts holds the rank records the digit.  Returns digit None where no lane claims (the state stays as it is)"""
    c = np.asarray(bins, np.int64).reshape(64, 4)
    sums = c.sum(axis=1)
    incl = sums.copy()
    d = 1
    while d < 64:
        up = np.roll(incl, d)
        adds = LANE > d if fault == "lane scan drops lane 0's sum" else LANE >= d
        incl = np.where(adds, incl + up, incl)
        d <<= 1
    if fault == "lane scan exclusive":
        incl = incl - sums
    excl = (incl - sums) & M32                           # unsigned arithmetic
    incl = incl & M32
    claim = (r >= excl) & ((r <= incl) if fault == "r <= c" else (r < incl))
    digit, rr, info = None, r, dict(rank_in=r)
    for l in np.flatnonzero(claim):                      # one lane, unless a fault lets several in: the last store stays
        c0, c1, c2 = (int(v) for v in c[l, :3])
        rr, digit, pos = (r - int(excl[l])) & M32, 4 * int(l), 0
        ge = (lambda a, b: a > b) if fault == "r <= c" else (lambda a, b: a >= b)
        if ge(rr, c0):
            rr -= c0; pos = 1
            if ge(rr, c1):
                rr -= c1; pos = 2
                if fault != "in-lane chain stops one bin early" and ge(rr, c2):
                    rr -= c2; pos = 3
        digit += pos
        info = dict(rank_in=r, lane=int(l), pos=pos, at_excl=r == int(excl[l]), at_last=r == int(incl[l]) - 1)
    return digit, rr, info


def ftz(v):
    v = np.float32(v)
    return np.float32(np.copysign(0.0, v)) if v != 0 and abs(v) < np.float32(2.0 ** -126) else v


def select(pts, mask=None, tol=None, scan="serial", fault=None):
    """(out float32 (6,), counts [n, n_keep], keep bool (M,) or None, trace): the radix select of the two kernels on gathered
    positions.  trace[s] has one entry per level for selector s = 2 * axis + (0: lo, 1: hi): digit, rank_in (the rank brought to
    the level), rank_in_bin, count (of the bin taken), before (occupied bins before it); the wave scan adds lane, pos, at_excl and
    at_last (the rank is the lane's first / last running count)."""
    pts = np.asarray(pts, np.float32).reshape(-1, 4)
    M = len(pts)
    used = np.isfinite(pts).all(axis=1)
    if mask is not None:
        used &= np.asarray(mask).reshape(-1) != 0
    with np.errstate(all="ignore"):
        dx, dy = pts[:, 2] - pts[:, 0], pts[:, 3] - pts[:, 1]
    kx = np.array([m_key(dx[j], fault) if used[j] else SENTINEL for j in range(M)], np.int64)
    ky = np.array([m_key(dy[j], fault) if used[j] else SENTINEL for j in range(M)], np.int64)
    n = int(used.sum())
    first = used
    if fault == "unused rows counted, in n and in the first histogram":
        n, first = M, np.ones(M, bool)
    elif fault == "sentinel counted in the first histogram":
        first = np.ones(M, bool)
    out = np.full(6, np.nan, np.float32)
    keep = None if tol is None else np.zeros(M, bool)
    if n == 0:
        return out, [0, 0], keep, None
    nr = M if fault == "ranks from M" else n
    lo_rank = nr >> 1 if fault == "lo rank n >> 1" else (nr - 1) >> 1
    hi_rank = (nr + 1) >> 1 if fault == "hi rank (n + 1) >> 1" else nr >> 1
    rank = [lo_rank, hi_rank, lo_rank, hi_rank]
    prefix = [0, 0, 0, 0]
    keys = [kx, kx, kx, kx] if fault == "y selectors read x keys" else [kx, kx, ky, ky]
    later = np.ones(M, bool) if fault == "sentinel not skipped in later passes" else used
    trace = [[], [], [], []]
    for level in range(4):
        low = 24 - 8 * level
        high = low if fault == "prefix compared at low" else low + 8
        for s in range(4):
            k = keys[s]
            if level == 0:
                sel = first
            else:
                pre = prefix[0] if (s == 1 and fault == "selector 1 with selector 0's prefix") else prefix[s]
                sel = later & ((k >> high) == pre)
            bins = np.bincount((k[sel] >> low) & 255, minlength=256).tolist()
            digit, r, info = (serial_scan if scan == "serial" else wave_scan)(bins, rank[s], fault)
            if digit is not None:
                prefix[s], rank[s] = ((prefix[s] << 8) | digit) & M32, r
                info.update(digit=digit, rank_in_bin=r, count=bins[digit], before=sum(1 for c in bins[:digit] if c))
            trace[s].append(info)
    v = [m_unkey(prefix[s], fault) for s in range(4)]
    with np.errstate(all="ignore"):
        for axis in range(2):
            lo, hi = v[2 * axis], v[2 * axis + 1]
            if n & 1 and fault != "odd median (lo + lo) * 0.5":
                med = lo
            else:
                if n & 1:
                    hi = lo
                med = np.float32(np.float32(lo + hi) * np.float32(0.5))
                if fault == "subnormals flushed in the halving":
                    med = ftz(np.float32(ftz(np.float32(ftz(lo) + ftz(hi))) * np.float32(0.5)))
            out[axis] = med
        out[2:] = v
        n_keep = 0
        if tol is not None:
            mdx, mdy, t = out[0], out[1], np.float32(tol)
            ok_median = (np.isfinite(mdx) and np.isfinite(mdy)) or fault == "keep with a non-finite median"
            le = (lambda a, b: a < b) if fault == "< for <= in keep" else (lambda a, b: a <= b)
            for j in range(M):
                if fault == "keep from all M rows":
                    ex, ey = dx[j], dy[j]                                   # the row's displacement whether it is used or not
                elif kx[j] == SENTINEL:
                    continue
                else:
                    ex, ey = m_unkey(int(kx[j]), fault), m_unkey(int(ky[j]), fault)
                keep[j] = bool(ok_median and le(np.abs(np.float32(ex - mdx)), t) and le(np.abs(np.float32(ey - mdy)), t))
            n_keep = int(keep.sum())
    return out, [n, n_keep], keep, trace


_PTS, _TRACE = {}, {}


def pts_of(c):
    if c.name not in _PTS:
        _PTS[c.name] = gather(*c.lists())
    return _PTS[c.name]


def differs(c, got):
    """does a result differ from what the case dictates: the six floats, n, and keep / n_keep where the family dictates them"""
    out, counts, keep, _ = got
    if not sr.same_bits(out, c.want) or counts[0] != c.n:
        return True
    return c.keep is not None and (not np.array_equal(keep, c.keep) or counts[1] != c.n_keep)


def traces():
    """name -> scan -> trace, of the model without a fault; filled once (and held to the dictated results while at it)"""
    if not _TRACE:
        for c in sc.all_cases():
            _TRACE[c.name] = {}
            for scan in SCANS:
                got = select(pts_of(c), c.mask, c.tol, scan)
                assert not differs(c, got), (c.name, scan, got[0], c.want)
                if c.tol is not None and c.keep is None:    # a keep mask no family dictates: the restatement's
                    want = sr.shift_pts(pts_of(c), c.mask, c.tol)
                    assert np.array_equal(got[2], want[2]) and got[1][1] == want[1][1], (c.name, scan)
                _TRACE[c.name][scan] = got[3]
    return _TRACE


def entries(scan="wave"):
    """(case, selector, level, trace entry) of every case"""
    t = traces()
    for c in sc.all_cases():
        for s in range(4):
            for level, e in enumerate(t[c.name][scan][s]):
                yield c, s, level, e


# ---------------------------------------------------------------------------------------------- the dictated results
def test_the_restatement_gives_every_dictated_result():
    cases = sc.all_cases()
    assert len(cases) == 2197 and set(c.family for c in cases) == set(sc.FAMILIES) and len(set(c.name for c in cases)) == len(cases)
    for c in cases:
        kp1, kp2, pairs = c.lists()
        out, counts, keep = sr.shift(kp1, kp2, pairs, c.mask, c.tol)
        assert sr.same_bits(out, c.want), (c.name, out, c.want)
        assert counts[0] == c.n and c.n >= 1, c.name
        assert c.M <= 1024 or (c.family == "runs" and c.M == 1203) or (c.family == "ranks" and c.M in (1031, 1032)), (c.name, c.M)
        assert c.x.multiset() != c.y.multiset() and c.x.n == c.y.n == c.n, c.name
        assert (c.M != c.n) == any(k is not None for k in c.kind), c.name
        if c.family == "keep":
            assert c.keep is not None and np.array_equal(keep, c.keep) and counts[1] == c.n_keep, c.name
            assert not c.keep[~c.used].any()
        if c.family == "ranks" and "unused" in c.name:
            assert set(c.kind) - {None} == set(sc.KINDS) and c.M >= c.n + 8, c.name
        if c.family == "top_bins":
            assert c.M - c.n >= c.n, c.name
    assert max(c.M for c in cases) == 1203
    # the hand-written medians are what one float32 sum and halving give
    for c in sc.family("median_arithmetic"):
        assert sr.same_bits(sc.halve(c.x.lo, c.x.hi, c.n), c.x.med), c.name


def test_numpy_median_agrees_up_to_the_sign_of_a_zero():
    seen_nan = 0
    for c in sc.all_cases():
        pts = pts_of(c)
        used = sr.used_pairs(pts, c.mask)
        with np.errstate(all="ignore"):
            for axis in range(2):
                d = (pts[:, 2 + axis] - pts[:, axis])[used]
                if np.isnan(c.want[axis]):
                    seen_nan += 1
                    continue
                med = np.median(d)
                assert med.dtype == np.float32 and med == c.want[axis], (c.name, axis, med, c.want[axis])
    assert seen_nan == 2                                    # keep's lo -inf, hi +inf, once per axis


def test_dictated_keep_masks():
    by = dict((c.name.split("/")[1], c) for c in sc.family("keep"))
    for axis in "xy":
        def kept(name):
            c = by["%s on %s" % (name, axis)]
            d = c.dx if axis == "x" else c.dy
            return sorted(float(v) for v in d[c.keep]), c
        assert kept("tol 0.5 about 10")[0] == [9.5, float(np.nextafter(np.float32(9.5), np.float32(10))), 10.0,
                                               float(np.nextafter(np.float32(10.5), np.float32(10))), 10.5]
        vals, c = kept("tol 0 about +0.0")
        assert vals == [0.0, 0.0] and c.n_keep == 2 and c.want[0 if axis == "x" else 1].view(np.uint32) == 0
        assert any(np.signbit(v) for v in (c.dx if axis == "x" else c.dy)[c.keep])              # -0.0 is kept
        assert kept("difference rounds onto tol")[0] == [-16777216.0, -16777214.0, 1.0, 16777214.0, 16777218.0]
        assert kept("tol 2^-149")[0] == [2 * sc.UNIT, 3 * sc.UNIT, 4 * sc.UNIT]
        vals, c = kept("tol inf, infinite displacements")
        assert vals == [-np.inf, -5.0, 2.0, 7.0, np.inf] and c.n_keep == c.n == 5 and c.M == 11
        for name in ("tol inf, NaN median", "tol inf, +inf median", "tol inf, -inf median", "tol 0.5, +inf median"):
            c = by["%s on %s" % (name, axis)]
            assert c.n_keep == 0 and not np.isfinite(c.want[0 if axis == "x" else 1]), c.name
        # a masked row sits exactly at both medians and is not kept
        c = by["tol 0.5 about 10 on %s" % axis]
        rows = [r for r in range(c.M) if c.kind[r] == "mask 0"]
        assert len(rows) == 2 and all(c.dx[r] == c.want[0] and c.dy[r] == c.want[1] and not c.keep[r] for r in rows)


# ---------------------------------------------------------------------------------------------- the model and its reach
def test_the_model_gives_every_dictated_result_with_both_scans():
    t = traces()
    assert len(t) == 2197
    for c in sc.all_cases():                                # and both scans walk the same way
        for s in range(4):
            a, b = t[c.name]["serial"][s], t[c.name]["wave"][s]
            assert [(e["digit"], e["rank_in_bin"], e["count"], e["before"]) for e in a] == \
                   [(e["digit"], e["rank_in_bin"], e["count"], e["before"]) for e in b], c.name


def test_every_level_and_digit_is_reached_by_a_lo_and_by_a_hi_selector():
    reached = {0: set(), 1: set()}
    for c, s, level, e in entries():
        reached[s & 1].add((level, e["digit"]))
    full = set((p, d) for p in range(4) for d in range(256))
    assert reached[0] == full and reached[1] == full
    # and the every_digit family alone does it, on the x axis, with the digit it names
    t = traces()
    for c in sc.family("every_digit"):
        k = c.x.claims
        sel = 0 if k["sel"] == "lo" else 1
        assert t[c.name]["wave"][sel][k["level"]]["digit"] == k["digit"], c.name
        assert 5 <= c.n <= 6 and len(set(sc.bits(c.dx).tolist())) == c.n, c.name
    # a serial scan with `r <= c` changes every one of them
    for c in sc.family("every_digit"):
        assert differs(c, select(pts_of(c), c.mask, c.tol, "serial", "r <= c")), c.name


def test_rank_in_bin_edges_at_every_level():
    first, last = set(), set()
    for c, s, level, e in entries():
        if e["count"] > 1 and e["rank_in_bin"] == 0:
            first.add(level)
        if e["count"] > 1 and e["rank_in_bin"] == e["count"] - 1:
            last.add(level)
    assert first == last == {0, 1, 2, 3}
    # the runs: the rank is carried through the run's bin at every level, with empty and with occupied bins before it
    t = traces()
    seen = set()
    for c in sc.family("runs"):
        k = c.x.claims
        if k["where"] in ("first", "last"):
            e = t[c.name]["wave"][0][3]
            assert e["count"] == k["run"] and e["rank_in_bin"] == (0 if k["where"] == "first" else k["run"] - 1), c.name
            assert (e["before"] > 0) == k["occupied"], c.name
            seen.add((k["run"], k["where"], k["occupied"], bool(np.signbit(c.x.lo))))
    assert len(seen) == 20 and set(v[0] for v in seen) == set(sc.RUNS) and set(v[3] for v in seen) == {False, True}


def test_lane_edges_of_the_wave_scan():
    at_excl, at_last, pos = set(), set(), set()
    for c, s, level, e in entries("wave"):
        if e["at_excl"]:
            at_excl.add((level, e["lane"]))
        if e["at_last"]:
            at_last.add((level, e["lane"]))
        pos.add((level, e["pos"]))
    want = set((p, lane) for p in range(4) for lane in sc.EDGE_LANES)
    assert want <= at_excl and want <= at_last, (sorted(want - at_excl), sorted(want - at_last))
    assert pos == set((p, k) for p in range(4) for k in range(4))
    # the lane_edges family alone does it, on the x axis, where it says
    t = traces()
    for c in sc.family("lane_edges"):
        k = c.x.claims
        hits = [t[c.name]["wave"][s][k["level"]] for s in (0, 1)]
        assert any(e["lane"] == k["lane"] and e["at_excl" if k["edge"] == "excl" else "at_last"] for e in hits), c.name


def test_every_divergence_level_occurs():
    t = traces()
    seen = set()
    for c in sc.family("divergence"):
        lo, hi = t[c.name]["serial"][0], t[c.name]["serial"][1]
        first = next((p for p in range(4) if lo[p]["digit"] != hi[p]["digit"]), 4)
        assert first == c.x.claims["diverge"], c.name
        seen.add(first)
        if "carry" in c.name:                               # lo finishes on digits 255, hi on digits 0
            assert all(lo[p]["digit"] == 255 and hi[p]["digit"] == 0 for p in range(first + 1, 4)), c.name
    assert seen == {0, 1, 2, 3, 4}
    z = dict((c.name.split("/")[1], c) for c in sc.family("divergence"))
    assert z["-0.0 | +0.0"].want[2:4].view(np.uint32).tolist() == [0x80000000, 0]
    assert z["subnormals either side of zero"].want[2:4].view(np.uint32).tolist() == [0x80000001, 1]


# ---------------------------------------------------------------------------------------------- faults
def fault_cases():
    """every case but for every_digit, of which every level keeps the digits 0, 7, 8, 15, ... (d % 8 in (0, 7): the carries) and 100"""
    return [c for c in sc.all_cases() if c.family != "every_digit" or c.x.claims["digit"] % 8 in (0, 7) or c.x.claims["digit"] == 100]


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_every_fault_changes_a_dictated_result_of_its_family(fault):
    scans, where = FAULTS[fault]
    for scan in scans:
        caught = {}
        for c in fault_cases():
            if differs(c, select(pts_of(c), c.mask, c.tol, scan, fault)):
                caught[c.family] = caught.get(c.family, 0) + 1
        print("%-52s %-6s caught by %s" % (fault, scan, ", ".join("%s (%d)" % kv for kv in sorted(caught.items())) or "nothing"))
        assert caught.get(where), (fault, scan, caught)


def test_faults_that_cannot_be_observed_are_not():
    for fault in UNOBSERVABLE:
        assert fault not in FAULTS
        for c in fault_cases():
            for scan in SCANS:
                got = select(pts_of(c), c.mask, c.tol, scan, fault)
                assert not differs(c, got), (fault, c.name, scan)
                if c.tol is not None:                       # the keep mask of the families that do not dictate one
                    want = sr.shift_pts(pts_of(c), c.mask, c.tol)
                    assert np.array_equal(got[2], want[2]) and got[1][1] == want[1][1], (fault, c.name, scan)
