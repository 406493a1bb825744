"""CPU side of MatchPlan.match_batch: the numpy restatement (tests/match_batch_ref.py) against the
oracle's matcher, segment by segment, on every crafted batch the GPU test runs (tests/test_gpu_match_batch.py), and against the
answer each construction dictates; the new entry point is declared, bound and exported."""
import os
import re

import numpy as np
import pytest

import match_batch_ref as mb
import match_cases as mc
from util import sort_rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCHES = mb.all_batches()


@pytest.mark.parametrize("batch", BATCHES, ids=[b.name for b in BATCHES])
def test_restatement_oracle_and_construction_agree(oracle, batch):
    pairs, counts = batch.reference()
    assert pairs.dtype == np.int32 and pairs.ndim == 2 and pairs.shape[1] == 2
    assert counts.dtype == np.int64 and counts.shape == (len(batch.counts2),) and counts.sum() == len(pairs)
    th = mb.threshold(batch.ratio)
    for s, ((a, b), rows) in enumerate(zip(batch.segments(), mb.split(pairs, counts))):
        what = "%s, segment %d" % (batch.name, s)
        assert (np.diff(rows[:, 0]) > 0).all(), what                 # ascending i: the order is the contract's
        if len(a) == 0 or len(b) == 0:
            assert len(rows) == 0, what                              # an empty list on either side: no pair
        else:
            want, n = oracle.match_ex(a, b, None, 0, mutual=batch.mutual, ratio_th=th)
            assert n == len(want) == len(rows), what
            assert np.array_equal(sort_rows(want.reshape(-1, 2)), rows), what
            assert rows[:, 0].max(initial=0) < len(a) and rows[:, 1].max(initial=0) < len(b), what     # local indices
        if len(b) == 1 and not batch.mutual:
            assert np.array_equal(rows, np.stack([np.arange(len(a)), np.zeros(len(a), np.int64)], axis=1)), what   # dist2 stays 1e12
        if batch.dictated is not None and batch.dictated[s] is not None:
            assert np.array_equal(rows, batch.dictated[s]), what


def test_batches_hold_what_they_promise():
    by_name = {b.name: b for b in BATCHES}
    edges = by_name["segment edges"]
    assert tuple(edges.counts1) == mb.EDGE_COUNTS1 and tuple(edges.counts2) == mb.EDGE_COUNTS2
    assert tuple(by_name["segment edges, tables exchanged"].counts1) == mb.EDGE_COUNTS2
    assert len(by_name["one segment"].counts2) == 1
    counts = edges.reference()[1]
    assert (counts[[0, 1]] == 0).all() and (counts[3:] > 0).all()
    swapped = by_name["segment edges, tables exchanged"].reference()[1]
    assert (swapped[[0, 1]] == 0).all() and swapped[2] == 2 and (swapped[3:] > 0).all()      # segment 2: a list of one element pairs both queries
    # the leak batch: what a scan over the neighbours' elements would answer differs from the dictated answer in every segment
    leak = by_name["no leak across a boundary"]
    assert np.array_equal(leak.reference()[0], np.concatenate(leak.dictated))
    whole = mb.match_batch(leak.kp1, leak.counts1, leak.kp2, [len(leak.kp2)] + [0] * (len(leak.counts2) - 1))
    assert len(whole[0]) == 0 or not np.array_equal(whole[0][:257], leak.dictated[0])
    off = np.concatenate([[0], np.cumsum(leak.counts2)])
    for s, (a, b) in enumerate(leak.segments()):
        lo, hi = off[s], off[s + 1]
        d = mc.l1(a["desc"][0], leak.kp2["desc"])
        assert d[lo - 1] == 0 and d[hi % len(d)] == 1                # the decoys sit right outside the segment
        assert d[lo:hi].min() == 100 and sorted(d[lo:hi])[1] == 200
        assert not np.array_equal(a["desc"][0], leak.segments()[s - 1][0]["desc"][0])
    assert sorted(set(leak.counts1)) == [257, 513]
    # the fold batches: ties that must not pair, placements that do and do not; more than one partition of 64 in every list
    for ratio, some_fail in ((None, True), (1.0, False)):
        fold = by_name["partition fold, ratio %r" % (ratio,)]
        assert min(fold.counts2) == 65 and max(fold.counts2) == 257 and len(fold.counts2) > 300
        got = [len(d) for d in fold.dictated]
        assert 0 in got and 3 in got
        fails = sum(1 for (a, b), d in zip(fold.segments(), fold.dictated) if len(d) == 0 and mc.l1(a["desc"][0], b["desc"]).min() == 3000)
        assert (fails > 0) == some_fail
    for r in mb.RATIOS:
        rb = by_name["ratio %r" % (r,)]
        got = [len(d) for d in rb.dictated]
        assert len(got) >= 20 and 0 in got and (260 in got or r == 0.5)
    shared = by_name["mutual, one shared first list"]
    assert shared.counts1 is None and 0 in shared.counts2 and 1 in shared.counts2
    pairs, counts = shared.reference()
    first = mb.split(pairs, counts)[0]
    assert first[first[:, 1] == 70].tolist() == [[257, 70]]          # of the duplicates from 257 on, the earliest survives
    plain = mb.match_batch(shared.kp1, None, shared.kp2, shared.counts2)
    assert plain[1][0] > counts[0]                                   # without the reverse check the later duplicates pair too
    large, small = by_name["shared reference"], by_name["shared reference, smaller"]
    assert len(large.kp2) > len(small.kp2) and len(large.kp1) > len(small.kp1) and large.reference()[1].sum() > small.reference()[1].sum() > 0


def test_ratio_above_one_is_refused():
    with pytest.raises(ValueError):
        mb.threshold(1.1)
    assert mb.threshold(1.0) == 1 and mb.threshold(None) == mc.RATIO


def test_entry_point_is_declared_and_bound():
    """include/siftmi.h declares siftmi_match_batch, _lib.py binds it with sixteen arguments"""
    import ctypes as C
    from sift_pyocl_amd import _lib
    assert "siftmi_match_batch" in _lib.exported_symbols()
    res, args = _lib._SIGNATURES["siftmi_match_batch"]
    assert res is C.c_int and len(args) == 16 and args[10] is C.c_float
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    m = re.search(r"\bint\s+siftmi_match_batch\s*\(([^;]*)\)\s*;", header)
    assert m and len(m.group(1).split(",")) == 16
    import inspect
    import sift_pyocl_amd as sp
    sig = inspect.signature(sp.MatchPlan.match_batch)
    assert list(sig.parameters) == ["self", "kp1", "counts1", "kp2", "counts2", "ratio", "mutual", "part_len", "out"]
    assert [sig.parameters[k].default for k in ("ratio", "mutual", "part_len", "out")] == [None, False, 0, "host"]
