"""CPU side of MatchPlan.match_window_batch / LinearAlign.align_batch_window: the numpy restatement
(tests/match_window_batch_ref.py) against match_batch's restatement where the window is infinite, every crafted batch of the GPU
test (tests/test_gpu_match_window_batch.py) against the rule it is named after, and the host side of the new entry point --
header, library and signature table agree, a null handle is refused without a device, the new methods have the documented
parameters and the old ones keep theirs.  No kernel runs."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

import match_batch_ref as mb
import match_cases as mc
import match_window_batch_ref as wb
import window_ref as wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = mb.all_batches()


@pytest.mark.parametrize("batch", BATCHES, ids=[b.name for b in BATCHES])
def test_infinite_window_is_match_batch(batch):
    """window = inf and zero shifts: match_batch's arrays, with and without mutual"""
    for mutual in (False, True):
        want = mb.match_batch(batch.kp1, batch.counts1, batch.kp2, batch.counts2, batch.ratio, mutual)
        got = wb.match_window_batch(batch.kp1, batch.counts1, batch.kp2, batch.counts2, wb.INF, (0.0, 0.0), batch.ratio, mutual)
        assert got[0].dtype == np.int32 and got[1].dtype == np.int64
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), "%s, mutual %r" % (batch.name, mutual)


def candidates(a, b, window, shift=(0.0, 0.0)):
    return wr.candidate_matrix(a, b, window, shift)


def test_edge_batch_holds_its_edges():
    batch = wb.edge_batch()
    assert tuple(batch.counts1) == wb.EDGE_QUERIES + (wb.ONE_SPOT[0],) and tuple(batch.counts2) == wb.EDGE_LISTS + (wb.ONE_SPOT[1],)
    assert {0, 1, 2, 255, 256, 257, 511, 512, 513} <= set(batch.counts1) and {0, 1, 63, 64, 65, 128, 129} <= set(batch.counts2)
    a, b = batch.segments()[-1]
    assert len(set(zip(a["x"].tolist(), a["y"].tolist())) | set(zip(b["x"].tolist(), b["y"].tolist()))) == 1
    for window in (wb.INF, 4.0):
        pairs, counts = wb.edge_batch(window).reference()
        rows = mb.split(pairs, counts)
        for s, (a, b) in enumerate(batch.segments()):
            if len(a) == 0 or len(b) == 0:
                assert counts[s] == 0
        assert counts[-1] > 0 and (counts[3:8] > 0).all()
        # a list of one element pairs every query that has it as a candidate (segments 2 and 8)
        for s in (2, 8):
            a, b = batch.segments()[s]
            ok = candidates(a, b, window)[:, 0]
            assert np.array_equal(rows[s], np.stack([np.nonzero(ok)[0], np.zeros(ok.sum(), np.int64)], axis=1))


@pytest.mark.parametrize("shared", [False, True])
def test_leak_batch_would_answer_differently_if_segments_leaked(shared):
    segs, partner = wb.leak_parts()
    batch = wb.leak_batch(shared)
    S = len(segs)
    pairs, counts = batch.reference()
    rows = mb.split(pairs, counts)
    off1 = np.concatenate([[0], np.cumsum([len(a) for a, _ in segs])])
    for s, (a, b) in enumerate(segs):
        for t in (s - 1, (s + 1) % S):                               # the exact copy lies in both neighbours, inside the window ...
            nb = segs[t][1]
            ok = candidates(a, nb, wb.LEAK_WINDOW)
            for i in (0, len(a) // 2, len(a) - 1):
                d = mc.l1(a["desc"][i], nb["desc"])
                j = int(np.argmin(d))
                assert d[j] == 0 and ok[i, j] and nb["x"][j] == a["x"][i] and nb["y"][j] == a["y"][i]
        own = np.array([mc.l1(a["desc"][i], b["desc"]).min() for i in range(len(a))])
        assert own.min() > 0                                         # ... and not in the segment's own list
        # the dictated answer: every query pairs with its partner
        mine = rows[s]
        if shared:
            mine = mine[(mine[:, 0] >= off1[s]) & (mine[:, 0] < off1[s + 1])] - [off1[s], 0]
        assert np.array_equal(mine, np.stack([np.arange(len(a)), partner[s]], axis=1)), s
    # what a matcher that sees one neighbour's records as well answers: the copy wins; with both neighbours the two copies tie
    # at distance 0 and dist2 == 0 refuses every pair
    a0, b0 = segs[0]
    off = len(b0)
    one = wr.match(a0, np.concatenate([b0, segs[1][1]]), wb.LEAK_WINDOW)
    assert len(one) == len(a0) and (one[:, 1] >= off).all()
    assert len(wr.match(a0, np.concatenate([b for _, b in segs]), wb.LEAK_WINDOW)) == 0


def test_grid_batch_has_the_extents():
    batch = wb.grid_batch()
    near, far, point, wild, empty, again = batch.segments()
    assert near[1]["x"].min() >= -2 and near[1]["x"].max() <= 102
    assert far[1]["x"].min() >= 1e6 - 2 and far[1]["x"].max() <= 1e6 + 52
    assert len(set(point[1]["x"].tolist())) == 1 and len(set(point[0]["y"].tolist())) == 1
    assert np.isnan(wild[1]["x"]).any() and np.isinf(wild[1]["x"]).any() and (np.abs(wild[1]["y"]) == np.float32(1e30)).any()
    assert len(empty[0]) == 0 and len(empty[1]) == 0
    pairs, counts = batch.reference()
    assert counts[4] == 0 and (counts[[0, 1, 2, 3, 5]] > 0).all()
    rows = mb.split(pairs, counts)
    # a keypoint with a NaN or an infinite coordinate is never a candidate and never has one (inf - inf is NaN); +-1e30 against
    # the same +-1e30 is a difference of 0: those do pair
    for k, l in enumerate(wild):
        bad = np.nonzero(~(np.isfinite(l["x"]) & np.isfinite(l["y"])))[0]
        assert len(bad) == 3 and not np.isin(rows[3][:, k], bad).any()
    assert (rows[3][:, 0] >= len(wild[0]) - 6).any()


@pytest.mark.parametrize("ratio", mb.RATIOS)
def test_rule_batch_reaches_the_rule(ratio):
    batch = wb.rule_batch(ratio)
    th = mb.threshold(ratio)
    pairs, counts = batch.reference()
    rows = mb.split(pairs, counts)
    emitted, refused, zero2, tied = 0, 0, 0, 0
    for (a, b), r in zip(batch.segments(), rows):
        best, f1, f2 = wr.scan(a, b, mc.SPOT_WINDOW)
        has2 = f2 < np.float32(1e11)
        with np.errstate(all="ignore"):
            emitted += int((has2 & (f2 != 0) & (f1 / f2 < th)).sum()); refused += int((has2 & (f2 != 0) & ~(f1 / f2 < th)).sum())
        zero2 += int((f2 == 0).sum()); tied += int((has2 & (f1 == f2) & (f1 > 0)).sum())
        assert (best[3::8] >= 0).all() or len(b) == 1                # the queries on spot 1 see a few far candidates ...
        assert (best[7::8] == -1).all() or (a["x"] == a["x"][0]).all()   # ... those on spot 3 none (the tie lists keep x = 0)
    assert emitted > 0 and refused > 0 and zero2 > 0 and tied > 0 and len(pairs) > 0


def test_lone_batch_has_lone_and_no_candidates():
    batch = wb.lone_batch()
    pairs, counts = batch.reference()
    for (a, b), r in zip(batch.segments(), mb.split(pairs, counts)):
        n = candidates(a, b, batch.window).sum(axis=1)
        assert (n[0::3] == 1).all() and (n[1::3] == 1).all() and (n[2::3] == 0).all()
        k = np.arange(len(a)) // 3
        keep = np.arange(len(a)) % 3 != 2
        assert np.array_equal(r, np.stack([np.arange(len(a))[keep], k[keep]], axis=1))


def test_shift_and_many_batches():
    batch = wb.shift_batch()
    assert (wb.SHIFTS < 0).any() and (wb.SHIFTS != np.round(wb.SHIFTS)).any()
    with_shift = batch.reference()[1]
    without = wb.match_window_batch(batch.kp1, batch.counts1, batch.kp2, batch.counts2, batch.window)[1]
    assert (with_shift[[1, 2, 4]] > 2 * without[[1, 2, 4]]).all() and with_shift[3] > without[3] and with_shift[0] == without[0]
    mutual = wb.shift_batch(mutual=True).reference()[1]
    assert (mutual <= with_shift).all() and mutual.sum() > 0
    many = wb.many_batch()
    assert len(many.counts2) == wb.MANY > 1024 and max(many.counts1) == 5 and min(many.counts1) == 0 and min(many.counts2) == 0
    assert sum(-(-c // 512) for c in many.counts1) > 0 and many.reference()[1].sum() > 100


# ---------------------------------------------------------------------------------------------- the host side of the entry point
NAME = "siftmi_match_window_batch"


@pytest.fixture(scope="module")
def L():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


def test_header_library_and_signature_table_agree(L):
    from sift_pyocl_amd import _lib
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, header)
    assert m, "not declared"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 19
    res, args = _lib._SIGNATURES[NAME]
    assert res is C.c_int and len(args) == 19
    floats = [k for k, p in enumerate(params) if re.match(r"float\s+\w+$", p)]
    assert floats == [10, 11, 12] and [params[k].split()[-1] for k in floats] == ["ratio_th", "wx", "wy"]
    assert [k for k, t in enumerate(args) if t is C.c_float] == floats
    assert params[13].replace(" ", "") == "constfloat*shifts" and params[14].endswith("mutual") and params[15].endswith("grid_max")
    assert NAME in _lib.exported_symbols()
    assert hasattr(L, NAME)


def test_null_handle_is_refused_without_a_device(L):
    from sift_pyocl_amd import _lib
    kp = np.zeros(4, mc.DTYPE_KP)
    counts = np.array([4], np.int64)
    shifts = np.zeros(2, np.float32)
    pairs = np.full((4, 2), -7, np.int32)
    pc = np.full(1, -7, np.int64)
    rc = getattr(L, NAME)(None, kp.ctypes.data, 4, 0, kp.ctypes.data, 4, 0, 1, None, counts.ctypes.data, C.c_float(0.5), C.c_float(1.0),
                          C.c_float(1.0), shifts.ctypes.data, 0, 0, pairs.ctypes.data, 0, pc.ctypes.data)
    assert rc == _lib.EINVAL and L.siftmi_last_error()
    assert (pairs == -7).all() and (pc == -7).all()


def test_the_new_methods_have_the_documented_parameters():
    from sift_pyocl_amd import LinearAlign, MatchPlan
    sig = inspect.signature(MatchPlan.match_window_batch)
    assert list(sig.parameters) == ["self", "kp1", "counts1", "kp2", "counts2", "window", "window_shift", "ratio", "mutual", "grid_max", "out"]
    assert sig.parameters["window"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in list(sig.parameters)[6:]] == [(0.0, 0.0), None, False, 0, "host"]
    sig = inspect.signature(LinearAlign.align_batch_window)
    assert list(sig.parameters) == ["self", "images", "max_shift", "expected_shift", "shift_only", "robust", "robust_tol", "robust_hyp",
                                    "match_ratio", "return_all", "out", "lanes"]
    assert sig.parameters["max_shift"].default is inspect.Parameter.empty
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [None, False, False, 3.0, 2048, None, False, "host", None]
    doc = LinearAlign.align_batch_window.__doc__
    assert "not an error" in doc and "robust=True" in doc


def test_the_old_methods_keep_their_parameters():
    from sift_pyocl_amd import LinearAlign, MatchPlan
    sig = inspect.signature(MatchPlan.match_batch)
    assert list(sig.parameters) == ["self", "kp1", "counts1", "kp2", "counts2", "ratio", "mutual", "part_len", "out"]
    assert [sig.parameters[k].default for k in ("ratio", "mutual", "part_len", "out")] == [None, False, 0, "host"]
    sig = inspect.signature(LinearAlign.align_batch)
    assert list(sig.parameters) == ["self", "images", "shift_only", "robust", "robust_tol", "robust_hyp", "match_ratio", "return_all",
                                    "out", "lanes"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [False, False, 3.0, 2048, None, False, "host", None]
    sig = inspect.signature(MatchPlan.match)
    assert list(sig.parameters) == ["self", "nkp1", "nkp2", "raw_results", "roi_mode", "mutual", "window", "window_shift"]
