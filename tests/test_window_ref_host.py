"""CPU pins of tests/window_ref.py, the numpy restatement the GPU tests of windowed matching compare with (DESIGN.md section 7
row 6): with an infinite window it must be the oracle's matcher (identity I1), and every pair of the plain matcher that satisfies
the window predicate must be in the windowed result (identity I2)."""
import numpy as np
import pytest

import window_ref as wr

SIZES = [(700, 650), (257, 64), (5, 900)]


@pytest.mark.parametrize("n1,n2", SIZES)
@pytest.mark.parametrize("mutual", [False, True])
def test_infinite_window_is_the_oracle_matcher(oracle, n1, n2, mutual):
    a, b, _ = wr.lists(n1, n2, min(n1, n2) // 2, seed=n1 + n2)
    want, n = oracle.match_ex(a, b, None, 0, mutual=mutual, cap=max(1, len(a)))
    got = wr.match(a, b, np.inf, mutual=mutual)
    assert len(got) == n
    assert np.array_equal(wr.sort_rows(got), wr.sort_rows(want))
    if min(n1, n2) >= 64:
        assert n > 0


@pytest.mark.parametrize("n1,n2", SIZES)
@pytest.mark.parametrize("w", [0, 2, 6, 30])
def test_plain_pairs_inside_the_window_survive(oracle, n1, n2, w):
    for shift in ((0.0, 0.0), (3.25, -1.5)):
        a, b = wr.crafted(n1, n2, seed=n1 + n2, shift=shift)
        plain, n = oracle.match_ex(a, b, None, 0, cap=max(1, len(a)))
        inside = wr.subset_in_window(plain[:n], a, b, w, shift)
        got = {tuple(r) for r in wr.match(a, b, w, shift)}
        assert {tuple(r) for r in inside} <= got, (w, shift)
        if w >= 2 and min(n1, n2) >= 64:
            assert len(inside) > 0


def test_contract_corners():
    """no candidate -> no pair; a lone candidate always pairs; ties go to the earliest index; NaN is never a candidate"""
    a = np.zeros(3, wr.DTYPE_KP); b = np.zeros(4, wr.DTYPE_KP)
    rng = np.random.default_rng(5)
    a["desc"] = rng.integers(0, 256, (3, 128), dtype=np.uint8); b["desc"] = rng.integers(0, 256, (4, 128), dtype=np.uint8)
    a["x"] = [10, 50, 90]; a["y"] = 5
    b["x"] = [10.5, 90, 90, np.nan]; b["y"] = 5
    b["desc"][1] = b["desc"][2]                                    # two equal candidates of query 2: dist1 == dist2 -> ratio 1
    got = wr.match(a, b, 1.0)
    assert got.tolist() == [[0, 0]]                                # query 0: a lone candidate; query 1: none; query 2: a tie
    best = wr.scan(a, b, 1.0)[0]
    assert best.tolist() == [0, -1, 1]
    assert wr.scan(a, b, 1.0, reverse=True)[0].tolist() == [0, 2, 2, -1]
    assert len(wr.match(a, b, np.inf)) == len(wr.match(a, b[:3], np.inf))     # the NaN keypoint takes no part
