"""CPU tests of the restatement of the segmented consensus filter (tests/consensus_batch_ref.py): the
answers the leak batch dictates hold for it, the shared-list form and a reordering of the segments give the same results, and the
header, the library and the signature table agree on the entry, which refuses a null matcher without a device."""
import ctypes as C
import os
import re

import numpy as np

import consensus_batch_ref as cb
import estimate_batch_ref as eb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LEAK_H, LEAK_TOL = 256, 0.5


def same_results(a, b):
    return (np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["winners"], b["winners"]) and
            np.array_equal(a["winner_votes"], b["winner_votes"]) and np.array_equal(a["votes_all"], b["votes_all"]) and
            cb.same_bits(a["models"], b["models"]) and cb.same_bits(a["models_all"], b["models_all"]))


def test_crafted_batches_are_what_their_names_say():
    t = cb.tile_batch()
    assert t.pair_counts.tolist() == [1500, 1024, 1025, 300, 2, 0, 4097] == [M for M, w in cb.TILE_SEGMENTS]
    assert (-(-t.pair_counts // 1024)).tolist() == [2, 1, 2, 1, 1, 0, 5]                # tiles per segment
    assert cb.edge_batch().pair_counts.tolist() == [0, 1, 2, 3, 4, 5, 18, 255, 256, 257, 513, 1000]
    assert cb.large_batch().pair_counts.tolist() == [0, 70001, 3]
    assert [b.name for b in cb.crafted_batches()] == ["edge", "leak", "large", "tile"]


def test_leak_batch_dictates_mask_votes_and_model():
    b = cb.leak_batch()
    r = cb.consensus_batch(b, LEAK_H, LEAK_TOL, 0)
    for s in range(b.S):
        kp1, kp2, pairs, _ = b.segment(s)
        inside = (pairs[:, 0] < len(kp1)) & (pairs[:, 1] >= 0)
        assert inside.sum() == eb.LEAK_IN_RANGE and len(pairs) == eb.LEAK_IN_RANGE + eb.LEAK_OUT
        assert np.array_equal(r["mask"][b.rows(s)], inside.astype(np.uint8)), s
        assert r["winner_votes"][s] == eb.LEAK_IN_RANGE and r["winners"][s] >= 0
        assert r["models"][s].tolist() == cb.leak_model(s).tolist(), (s, r["models"][s])
        # most triples hold a row that is out of range and are void: 22 rows, 10 in range, not all of those in general position
        assert 10 <= r["valid"][s].sum() <= 22, (s, r["valid"][s].sum())
        assert np.isnan(r["models_all"][s][~r["valid"][s]]).all() and not r["votes_all"][s][~r["valid"][s]].any()


def test_shared_list_form_gives_the_same_results():
    for b, H in ((cb.leak_batch(), LEAK_H), (cb.edge_batch(), 64), (cb.tile_batch(), 32)):
        assert same_results(cb.consensus_batch(b, H, 3.0, 5), cb.consensus_batch(b.shared(), H, 3.0, 5)), b.name


def test_reordering_the_segments_permutes_the_results():
    b = cb.edge_batch()
    order = [11, 3, 0, 7, 5, 1, 10, 2, 9, 4, 8, 6]
    p = cb.permuted(b, order)
    r, q = cb.consensus_batch(b, 64, 3.0, 9), cb.consensus_batch(p, 64, 3.0, 9)
    assert r["winners"].max() >= 0
    for k, s in enumerate(order):
        assert np.array_equal(q["mask"][p.rows(k)], r["mask"][b.rows(s)])
        assert q["winners"][k] == r["winners"][s] and q["winner_votes"][k] == r["winner_votes"][s]
        assert np.array_equal(q["votes_all"][k], r["votes_all"][s])
        assert cb.same_bits(q["models"][k], r["models"][s]) and cb.same_bits(q["models_all"][k], r["models_all"][s])


def test_segments_without_three_pairs_have_no_winner():
    b = cb.edge_batch()
    r = cb.consensus_batch(b, 16, 3.0, 0)
    assert r["winners"][:3].tolist() == [-1, -1, -1] and r["winner_votes"][:3].tolist() == [0, 0, 0]
    assert np.isnan(r["models"][:3]).all() and np.isnan(r["models_all"][:3]).all() and not r["votes_all"][:3].any()
    assert not r["mask"][:3].any()


def test_header_library_and_signature_table_agree():
    from sift_pyocl_amd import _lib
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    name = "siftmi_match_consensus_batch"
    assert name in _lib.exported_symbols()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert m and len(m.group(1).split(",")) == 25 == len(_lib._SIGNATURES[name][1])
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(_lib.lib(), name)


def test_a_null_matcher_is_refused_before_any_device_is_touched():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    b = cb.leak_batch()
    M, S = len(b.pairs), b.S
    mask = np.full(M, 0xEE, np.uint8)
    models = np.full((S, 6), -77, np.float32)
    winners, votes = np.full(S, -5, np.int32), np.full(S, -5, np.int32)
    ms = C.c_double(-1)
    rc = L.siftmi_match_consensus_batch(None, b.kp1.ctypes.data, len(b.kp1), 0, b.kp2.ctypes.data, len(b.kp2), 0, S,
                                        b.counts1.ctypes.data, b.counts2.ctypes.data, b.pairs.ctypes.data, M, 0, b.pair_counts.ctypes.data,
                                        LEAK_H, C.c_float(LEAK_TOL), 0, mask.ctypes.data, 0, models.ctypes.data, winners.ctypes.data,
                                        votes.ctypes.data, None, None, C.byref(ms))
    assert rc == _lib.EINVAL and _lib.last_error()
    assert (mask == 0xEE).all() and (models == -77).all() and (winners == -5).all() and (votes == -5).all() and ms.value == -1


def test_the_method_exists_with_the_documented_parameters():
    import inspect
    from sift_pyocl_amd import MatchPlan
    assert list(inspect.signature(MatchPlan.consensus_batch).parameters) == [
        "self", "kp1", "counts1", "kp2", "counts2", "pairs", "pair_counts", "n_hyp", "tol", "seed", "return_votes", "out"]
