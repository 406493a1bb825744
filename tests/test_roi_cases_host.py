"""CPU side of the region-of-interest cases (tests/roi_cases.py): on every case the oracle's pairs are the pairs the numpy
restatement (tests/roi_ref.py) expects, every probe's flag can be read back from those pairs, and the cases are decisive -- both
outcomes occur, and a restatement with one of the usual mistakes in it gives some probe of the mask another flag.

Which case catches which wrong rule (CAUGHT below is asserted exactly, per mask):

  floor           floor(v) instead of truncation: a coordinate in (-1, 0) leaves the mask.  Every mask with a non-zero pixel in
                  row 0 or column 0, through the probes nextafter(-1, 0), -0.5.
  nearest         round to nearest: nextafter(k, 0) lands on pixel k.  Every mask (on 1 x 1, nextafter(1, 0) leaves it).
  c <= rw         and r <= rh: the probes rw and rw + 0.5 (rh, rh + 0.5) are inside and read the next row's first byte or past
                  the mask.  Every mask; where the read is past the mask the flag differs whatever byte is found there (the
                  wrong rule is tried with a 0 and with a 1 behind the mask).
  r * rh + c      the row stride taken from the wrong dimension: 7 x 1, 3 x 5, 5 x 3 and both 64 x 257 masks (the planted pixel
                  (63, 256) is byte 16 447, the wrong rule reads byte 4 288).  Not 1 x 1 and 1 x 7, where r is always 0, and not
                  the square 16 x 16.
  c * rw + r      the axes swapped in the index: 3 x 5 and 5 x 3 (the same 15 bytes), 1 x 7 (the index runs past the mask),
                  both 64 x 257 masks and 16 x 16.  Not 1 x 1 and 7 x 1, where c is always 0.
  valid > 0       every mask that holds a negative byte: all but "64 x 257 ones".
  NaN as 0        the guard removed and NaN converted to 0, as the device's conversion does: every mask, each has a non-zero
                  byte in row 0 or column 0 under a NaN probe.
  mode 1 ~inside  mode 1's query rule without `inside &&`: a query beyond the array is dropped.  Every mask.

The wrong rules are tried on the numpy restatement only."""
import os

import numpy as np
import pytest

import match_cases as mc
import roi_cases as rc
import roi_ref
from util import sort_rows

MASK_NAMES = list(rc.MASKS)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "roi_edges_ref.npz")
RULES = ("floor", "nearest", "c <= rw", "r * rh + c", "c * rw + r", "valid > 0", "NaN as 0", "mode 1 ~inside")
ALL = set(RULES)
CAUGHT = {
    "1x1": ALL - {"r * rh + c", "c * rw + r"},
    "1x7": ALL - {"r * rh + c"},
    "7x1": ALL - {"c * rw + r"},
    "3x5": ALL,
    "5x3": ALL,
    "64x257 ones": ALL - {"valid > 0"},
    "64x257 zeros": ALL,
    "16x16 values": ALL - {"r * rh + c"},                 # square: both strides are 16
}


def rows_of(pairs):
    return sort_rows(np.asarray(pairs, np.int32).reshape(-1, 2))


@pytest.fixture(scope="module")
def all_cases():
    return {m: rc.cases(m) for m in MASK_NAMES}


# ---------------------------------------------------------------------------------------------- the restatement with mistakes
def wrong_flags(kp, roi, mode, rule=None, behind=0):
    """roi_ref.flags with ONE mistake (`rule`; None: no mistake).  The mask is read as the flat bytes a kernel sees; a read past
    them finds `behind`."""
    rh, rw = roi.shape
    flat = roi.ravel()

    def convert(v32):
        """(converted at all, the integer) per coordinate"""
        with np.errstate(invalid="ignore"):
            v = v32.astype(np.float64)
            ok = np.abs(v32) < roi_ref.LIMIT
        out = np.full(len(v), -1, np.int64)
        w = v[ok]
        out[ok] = np.floor(w) if rule == "floor" else (np.rint(w) if rule == "nearest" else np.trunc(w))
        if rule == "NaN as 0":                            # the guard removed, the conversion the device's: NaN gives 0
            out[np.isnan(v)] = 0
            ok = ok | np.isnan(v)
        return ok, out

    (okx, c), (oky, r) = convert(kp["x"]), convert(kp["y"])
    good = okx & oky
    hi_c, hi_r = (c <= rw, r <= rh) if rule == "c <= rw" else (c < rw, r < rh)
    inside = good & (r >= 0) & hi_r & (c >= 0) & hi_c
    idx = r * rh + c if rule == "r * rh + c" else (c * rw + r if rule == "c * rw + r" else r * rw + c)
    byte = np.full(len(c), behind, np.int64)
    within = inside & (idx >= 0) & (idx < flat.size)
    byte[within] = flat[idx[within]]
    on = inside & ((byte > 0) if rule == "valid > 0" else (byte != 0))
    if mode == 1:
        dropped = ~on if rule == "mode 1 ~inside" else (inside & ~on)
    else:
        dropped = ~on
    return dropped, np.where(on, 0, 1 if mode == 1 else 2).astype(np.uint8)


def probe_lists(mask):
    """the probe keypoints of a mask, once each: those of the query cases and of the one-probe calls"""
    cs = rc.cases(mask)
    lists = [c.probes() for c in cs if c.kind == "query" and c.mode == 1]
    lists.append(np.concatenate([c.probes() for c in cs if c.kind == "forced" and not c.mutual]))
    return np.concatenate(lists)


# ---------------------------------------------------------------------------------------------- the generator
def test_probe_values():
    v = rc.axis_values(5)
    bits = v.view(np.uint32).tolist()
    assert len(set(bits)) == len(bits)
    for b in rc.NAN_BITS:                                            # both signs, two payloads each, kept bit for bit
        assert b in bits
    f, zero = np.float32, np.float32(0)
    want = [-1.0, np.nextafter(f(-1), zero), -0.5, 0.0, np.nextafter(f(1), zero), 1.0, 5.0, 5.5, 2147483520.0, 2147483648.0, -2147483648.0,
            -2147483904.0, 3e38, np.inf, -np.inf] + [w for k in range(1, 6) for w in (f(k), np.nextafter(f(k), zero))]
    assert set(np.array(want, np.float32).view(np.uint32).tolist()) <= set(bits)
    assert np.array(-0.0, np.float32).view(np.uint32) in bits and np.array(0.0, np.float32).view(np.uint32) in bits
    assert np.nextafter(f(2147483648.0), zero) == rc.LAST_BELOW_2_31
    assert f(-2147483648.0 - 256.0) == np.nextafter(f(-2147483648.0), f(-np.inf))


def test_masks():
    m = rc.MASKS
    assert [m[k].shape for k in MASK_NAMES] == [(1, 1), (1, 7), (7, 1), (3, 5), (5, 3), (64, 257), (64, 257), (16, 16)]
    assert all(v.dtype == np.int8 and v.flags["C_CONTIGUOUS"] for v in m.values())
    assert m["3x5"].tobytes() == m["5x3"].tobytes()
    assert sorted(m["16x16 values"].ravel().tolist()) == list(range(-128, 128))
    for name, planted in (("64x257 ones", True), ("64x257 zeros", False)):
        z = m[name] == 0
        assert int(z.sum() if planted else (~z).sum()) == 4
        assert all(z[r, c] == planted for r, c in rc.CORNERS) and (63, 256) in rc.CORNERS
    # a mask differs from its neighbour along the lines the sweeps address
    for name in ("1x7", "7x1"):
        line = m[name].ravel() != 0
        assert (line[1:] != line[:-1]).all()


@pytest.mark.parametrize("mask", MASK_NAMES)
def test_lists_are_short_and_one_is_long(mask, all_cases):
    sizes = [max(len(c.a), len(c.b)) for c in all_cases[mask]]
    assert max(sizes) <= 600
    if mask.startswith("64x257"):                                    # the flag kernel's second and third workgroup, a partial last one
        assert max(sizes) > 512 and max(sizes) % 256 != 0
    for c in all_cases[mask]:
        if c.kind == "forced":
            assert len(c.a) == 4 and len(c.b) == 3


# ---------------------------------------------------------------------------------------------- oracle == restatement
@pytest.mark.parametrize("mask", MASK_NAMES)
def test_oracle_equals_the_restatement(oracle, mask, all_cases):
    """sorted pair rows and totals; the flag of every probe is what the pairs say; in the list cases no pair but the dedicated
    ones appears (asserted on the oracle's pairs)"""
    for c in all_cases[mask]:
        want = roi_ref.expected_pairs(c.a, c.b, c.roi, c.mode, c.mutual, c.th)
        got, n = oracle.match_ex(c.a, c.b, c.roi, c.mode, mutual=c.mutual, ratio_th=c.th)
        assert n == len(got) == len(want), c.name
        assert np.array_equal(rows_of(got), want), c.name
        probes = c.a if c.probe == "a" else c.b
        dropped, lflag = roi_ref.flags(probes, c.roi, c.mode)
        assert np.array_equal(c.read(got), c.flag(dropped, lflag)), c.name
        if c.kind == "list":
            assert (got[:, 0] == got[:, 1] + rc.LEAD).all(), c.name
        elif c.kind == "query":
            assert (got[:, 1] == 0).all(), c.name
        elif c.kind == "query+":
            assert (got[:, 0] == got[:, 1]).all(), c.name


@pytest.mark.parametrize("mask", MASK_NAMES)
def test_both_outcomes_occur(mask, all_cases):
    """per mask and observable (query flag in mode 1 and 2, list flag in mode 2, forced zero in mode 1), both outcomes -- except
    that on 1 x 1 no query is dropped in mode 1 (inside means on)"""
    seen = {}
    for c in all_cases[mask]:
        probes = c.a if c.probe == "a" else c.b
        seen.setdefault((c.kind, c.mode, c.mutual), set()).update(c.flag(*roi_ref.flags(probes, c.roi, c.mode)).tolist())
    assert len(seen) == 8
    for key, outcomes in seen.items():
        if mask == "1x1" and key[0] in ("query", "query+") and key[1] == 1:
            assert outcomes == {True}
        else:
            assert outcomes == {True, False}, (mask, key)


def test_both_outcomes_in_every_probe_family():
    """along each sweep -- the edge of the conversion at 0, the integers, the bounds, the huge values, the NaNs -- a probe is on the mask
    and a probe is not, over the small masks"""
    fam = {"around 0": lambda v: np.abs(v) <= 1, "integers": lambda v: (v >= 1) & (v <= 7), "huge": lambda v: np.abs(v) >= 2.0 ** 30,
           "nan": np.isnan}
    for label, pick in fam.items():
        on_seen = set()
        for mask in ("1x1", "1x7", "7x1", "3x5", "5x3"):
            p = probe_lists(mask)
            with np.errstate(invalid="ignore"):
                sel = pick(p["x"].astype(np.float64)) | pick(p["y"].astype(np.float64))
            on_seen.update(roi_ref.inside_on(p[sel], rc.MASKS[mask])[1].tolist())
        assert on_seen == ({False} if label in ("huge", "nan") else {True, False}), label       # never on: that is the contract


# ---------------------------------------------------------------------------------------------- decisive
@pytest.mark.parametrize("mask", MASK_NAMES)
def test_wrong_rules_change_a_flag(mask):
    roi = rc.MASKS[mask]
    p = probe_lists(mask)
    caught = set()
    for mode in (1, 2):
        right = roi_ref.flags(p, roi, mode)
        for k, got in enumerate(wrong_flags(p, roi, mode)):          # without a mistake it is roi_ref
            assert np.array_equal(got, right[k])
    for rule in RULES:
        hit = []
        for behind in (0, 1):
            differs = False
            for mode in (1, 2):
                right, wrong = roi_ref.flags(p, roi, mode), wrong_flags(p, roi, mode, rule, behind)
                differs |= bool((right[0] != wrong[0]).any() or (right[1] != wrong[1]).any())
            hit.append(differs)
        if all(hit):
            caught.add(rule)
    assert caught == CAUGHT[mask], "%s: caught %s" % (mask, sorted(caught))
    assert set().union(*CAUGHT.values()) == ALL


def test_the_nan_case_of_the_issue(oracle):
    """mask [[1, 0, 1], [0, 1, 1]], a query at x = NaN, y = 0.5: outside.  Mode 2 drops it, mode 1 keeps it; as a list-2 element it
    is a forced zero in mode 1 and excluded in mode 2.  Taken as column 0 it would sit on a non-zero pixel."""
    roi = np.array([[1, 0, 1], [0, 1, 1]], np.int8)
    k = mc.records(np.zeros((1, 128), np.uint8), x=np.nan, y=0.5)
    assert [f.tolist() for f in roi_ref.flags(k, roi, 1)] == [[False], [1]]
    assert [f.tolist() for f in roi_ref.flags(k, roi, 2)] == [[True], [2]]
    assert [f.tolist() for f in wrong_flags(k, roi, 2, "NaN as 0")] == [[False], [0]]
    rng = np.random.default_rng(3)
    base = mc.make_base(rng)
    a = mc.queries(base, 1); a["x"] = np.nan; a["y"] = 0.5
    b = mc.records(mc.descs_at(base, [100, 5000], rng), x=0.5, y=0.5)
    assert oracle.match_ex(a, b, roi, 2)[1] == 0 and oracle.match_ex(a, b, roi, 1)[1] == 1


# ---------------------------------------------------------------------------------------------- flags_restated moved here
def _flags_restated_before(case):
    """match_cases.flags_restated as it stood before it moved onto roi_ref (its inputs are finite, so the cast was defined)"""
    a, b, mode = case.a, case.b, case.roi_mode
    H, W = case.roi.shape

    def on(k):
        c, r = k["x"].astype(np.int64), k["y"].astype(np.int64)
        inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
        return inside, inside & (case.roi[np.clip(r, 0, H - 1), np.clip(c, 0, W - 1)] != 0)

    in1, on1 = on(a); _, on2 = on(b)
    keep1 = ~(in1 & ~on1) if mode == 1 else on1
    b2 = b.copy()
    if mode == 1:
        b2["desc"][~on2] = a["desc"][0]
        keep2 = np.ones(len(b), bool)
    else:
        keep2 = on2
    return a[keep1], b2[keep2], np.nonzero(keep1)[0], np.nonzero(keep2)[0]


def test_flags_restated_is_unchanged_on_flag_cases():
    n = 0
    for c in mc.flag_cases(6):
        a0, b0, ia0, ib0 = _flags_restated_before(c)
        a1, b1, ia1, ib1 = mc.flags_restated(c)
        assert np.array_equal(ia0, ia1) and np.array_equal(ib0, ib1), c.name
        assert np.array_equal(a0["desc"], a1["desc"]) and np.array_equal(b0["desc"], b1["desc"]), c.name
        n += 1
    assert n > 60


# ---------------------------------------------------------------------------------------------- the reference's own kernel
def test_oracle_equals_the_reference_kernel(oracle):
    """tests/golden/roi_edges_ref.npz: what the reference's `matching_valid`, built natively, answered on the mode-1 cases restricted
    to probes in (-1, 2^31) (tests/golden/make_roi_edges_ref.py; a NaN, |v| >= 2^31 and a negative index are undefined there).  The inputs are
    regenerated here and checked by digest; the oracle (roi_mode 1) and the restatement must give the reference's pairs."""
    z = np.load(GOLDEN)
    assert [str(s) for s in z["masks"]] == MASK_NAMES
    kinds = set()
    for k, mask in enumerate(MASK_NAMES):
        cases = rc.reference_cases(mask)
        assert rc.digest(cases) == str(z["digest_%d" % k]), "%s: the generated inputs are not the ones the fixture was made from" % mask
        pairs, off, totals = z["pairs_%d" % k], z["offsets_%d" % k], z["totals_%d" % k]
        assert len(totals) == len(cases) and len(off) == len(cases) + 1
        for i, c in enumerate(cases):
            p = c.probes()
            assert roi_ref.convertible(p["x"]).all() and roi_ref.convertible(p["y"]).all() and c.mode == 1 and not c.mutual
            ref = pairs[off[i]:off[i + 1]]
            want, n = oracle.match_ex(c.a, c.b, c.roi, 1, ratio_th=c.th)
            assert n == totals[i] == len(ref), c.name
            assert np.array_equal(rows_of(want), rows_of(ref)), c.name
            assert np.array_equal(roi_ref.expected_pairs(c.a, c.b, c.roi, 1, False, c.th), rows_of(ref)), c.name
            kinds.add((c.kind, bool(c.read(ref).all()), bool(c.read(ref).any())))
    assert {k for k, _, _ in kinds} == {"query", "forced"}
    assert ("query", False, True) in kinds and ("forced", True, True) in kinds and ("forced", False, False) in kinds
