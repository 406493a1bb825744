"""CPU tests of the restatement of the segmented fit and median (tests/estimate_batch_ref.py): the
answers the crafted batches dictate hold for it, its models are numpy.linalg.lstsq's within the bound measured on the same cases,
its medians are numpy.median's, and the header, the library and the signature table agree on the two entries."""
import os
import re

import numpy as np
import pytest

import estimate_batch_ref as eb
import fit_ref as fr
import shift_ref as sr
from consensus_ref import gather

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_crafted_batches_are_what_their_names_say():
    e = eb.edge_batch()
    assert e.pair_counts.tolist() == list(eb.EDGE_SIZES) and e.S == 12
    big = eb.large_batch()
    assert big.pair_counts.tolist() == [0, 70001, 3] and fr.default_blocks(70001) == 256 and 70001 - 256 * 256 < 256 * 256
    v = eb.value_batch()
    assert v.S == 10 and sorted(set(k for k, n in v.kinds)) == ["bits", "normal", "subnormal", "tied", "zeros"]
    assert v.pair_counts.tolist() == [257] * 5 + [1000] * 5
    for b in eb.crafted_batches() + [eb.keep_batch(), eb.cases_batch()]:
        assert b.counts1.sum() == len(b.kp1) and b.pairs.dtype == np.int32


def test_leak_batch_dictates_its_medians_and_counts():
    b = eb.leak_batch()
    out, counts, keep = eb.shift_batch(b, tol=0.0)
    n_rows = eb.LEAK_IN_RANGE + eb.LEAK_OUT
    assert b.pair_counts.tolist() == [n_rows] * eb.LEAK_SEGMENTS and eb.LEAK_OUT > eb.LEAK_IN_RANGE
    for s in range(b.S):
        dx, dy = eb.leak_displacement(s)
        assert out[s].tolist() == [dx, dy, dx, dx, dy, dy], s
        assert counts[s].tolist() == [eb.LEAK_IN_RANGE, eb.LEAK_IN_RANGE]
        kp1, kp2, pairs, mask = b.segment(s)
        outside = (pairs[:, 0] == len(kp1)) | (pairs[:, 1] == -1)
        assert outside.sum() == eb.LEAK_OUT and not keep[b.rows(s)][outside].any() and keep[b.rows(s)][~outside].all()
    # read across the bounds of its segment, a row of the inner segments would give a displacement of about 1e6
    off1, off2 = np.cumsum(b.counts1), np.cumsum(b.counts2)
    for s in range(1, b.S - 1):
        kp1, kp2, pairs, mask = b.segment(s)
        for i, j in pairs:
            if i == len(kp1):
                assert b.kp2["x"][off2[s - 1] + j] - b.kp1["x"][off1[s - 1] + i] > 9e5
            if j == -1:
                assert b.kp2["x"][off2[s - 1] + j] - b.kp1["x"][off1[s - 1] + i] > 9e5
    # the fit of the in-range rows is the translation
    fit = eb.fit_batch(b)
    for s in range(b.S):
        dx, dy = eb.leak_displacement(s)
        assert fit[s, fr.STATUS] == fr.OK and fit[s, fr.N] == eb.LEAK_IN_RANGE
        assert np.abs(fit[s, fr.MODEL] - [1, 0, dx, 0, 1, dy]).max() < 1e-9 and fit[s, fr.SSR] < 1e-18


def test_degenerate_batch_dictates_its_statuses():
    fit = eb.fit_batch(eb.degenerate_batch())
    assert fit[:, fr.STATUS].tolist() == [fr.OK, fr.DEGENERATE, fr.OK, fr.DEGENERATE, fr.OK]
    assert fit[:, fr.N].tolist() == [50, 20, 300, 2, 40]
    for s in (1, 3):
        assert np.isnan(fit[s, fr.MODEL]).all() and np.isnan(fit[s, fr.SSR]) and np.isfinite(fit[s, fr.MOMENTS]).all()
    out, counts, _ = eb.shift_batch(eb.degenerate_batch())
    assert counts[:, 0].tolist() == [50, 20, 300, 2, 40] and out[1, sr.MDX] == 3.5 and out[1, sr.MDY] == 5.25


def test_masked_batch_dictates_an_empty_segment_between_ok_ones():
    b = eb.masked_batch()
    fit = eb.fit_batch(b)
    assert fit[:, fr.STATUS].tolist() == [fr.OK, fr.EMPTY, fr.OK] and fit[1, fr.N] == 0 and np.isnan(fit[1, 2:]).all()
    want_n = [int((b.mask[b.rows(s)] != 0).sum()) for s in range(3)]
    assert fit[:, fr.N].tolist() == want_n and want_n[1] == 0 and 0 < want_n[0] < eb.MASKED_SIZES[0]
    out, counts, keep = eb.shift_batch(b, tol=np.inf)
    assert np.isnan(out[1]).all() and counts.tolist() == [[n, n] for n in want_n] and np.array_equal(keep, b.mask != 0)
    assert set(np.unique(b.mask)) - {0, 1}                    # bytes other than 1 count as set


def test_keep_batch_has_a_segment_whose_median_is_not_finite():
    b = eb.keep_batch()
    out, counts, keep = eb.shift_batch(b, tol=np.inf)
    assert np.isnan(out[1, sr.MDX]) and out[1, sr.LO_DX] == -np.inf and out[1, sr.HI_DX] == np.inf and counts[1].tolist() == [4, 0]
    assert out[3, sr.MDX] == np.inf and counts[3].tolist() == [3, 0] and counts[4].tolist() == [0, 0]
    assert not keep[b.rows(1)].any() and not keep[b.rows(3)].any() and keep[b.rows(0)].all() and keep[b.rows(2)].all()
    assert eb.shift_batch(b, tol=0.0)[1][0, 1] >= 400         # the tied middle of segment 0


def test_shared_list_form_gathers_the_same_rows():
    for b in eb.crafted_batches() + [eb.keep_batch()]:
        sh = b.shared()
        assert sh.counts1 is None and len(sh.kp1) == len(b.kp1)
        for s in range(b.S):
            a, c = b.segment(s), sh.segment(s)
            ga, gc = gather(a[0], a[1], a[2]), gather(c[0], c[1], c[2])
            assert np.array_equal(np.isnan(ga), np.isnan(gc)) and np.array_equal(ga[~np.isnan(ga)], gc[~np.isnan(gc)]), (b.name, s)


def test_models_are_lstsq_within_the_measured_bound():
    """the entries of fit_ref.CASES up to 5 000 pairs: the very cases on which LSTSQ_BOUND was measured"""
    b = eb.cases_batch()
    assert b.pair_counts.tolist() == [18, 255, 257, 1000, 1000, 5000]
    fit = eb.fit_batch(b)
    worst = 0.0
    for s in range(b.S):
        kp1, kp2, pairs, mask = b.segment(s)
        assert fit[s, fr.STATUS] == fr.OK
        worst = max(worst, float(np.abs(fit[s, fr.MODEL] - fr.lstsq_model(gather(kp1, kp2, pairs))).max()))
    print("largest |coefficient difference| against lstsq: %.3e (bound %.3e)" % (worst, fr.LSTSQ_BOUND))
    assert worst <= fr.LSTSQ_BOUND


def test_every_median_is_numpy_median():
    for b in eb.crafted_batches() + [eb.keep_batch(), eb.cases_batch()]:
        out, counts, _ = eb.shift_batch(b)
        for s in range(b.S):
            kp1, kp2, pairs, mask = b.segment(s)
            pts = gather(kp1, kp2, pairs)
            used = sr.used_pairs(pts, mask)
            assert counts[s, 0] == used.sum()
            if not used.any():
                assert np.isnan(out[s]).all()
                continue
            with np.errstate(all="ignore"):
                dx, dy = (pts[:, 2] - pts[:, 0])[used], (pts[:, 3] - pts[:, 1])[used]
                mx, my = np.median(dx), np.median(dy)
            for got, want in ((out[s, sr.MDX], mx), (out[s, sr.MDY], my)):
                assert got == want or (np.isnan(got) and np.isnan(want)), (b.name, s, got, want)


def test_header_library_and_signature_table_agree():
    from sift_pyocl_amd import _lib
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("siftmi_match_fit_batch", 19), ("siftmi_match_shift_batch", 21)):
        assert name in _lib.exported_symbols()
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
        assert m and len(m.group(1).split(",")) == n_args == len(_lib._SIGNATURES[name][1])
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    assert hasattr(L, "siftmi_match_fit_batch") and hasattr(L, "siftmi_match_shift_batch")


def test_the_methods_exist_with_the_documented_parameters():
    import inspect
    from sift_pyocl_amd import MatchPlan
    assert list(inspect.signature(MatchPlan.fit_batch).parameters) == [
        "self", "kp1", "counts1", "kp2", "counts2", "pairs", "pair_counts", "mask", "blocks", "return_moments"]
    assert list(inspect.signature(MatchPlan.shift_batch).parameters) == [
        "self", "kp1", "counts1", "kp2", "counts2", "pairs", "pair_counts", "mask", "tol", "return_ranks"]
