"""siftmath's fast paths on the arguments that are hard to round and on the edges of their guarded range
(tests/golden/math_hard.npz, described in tests/math_hard_cases.py), bit for bit against the CPU oracle.

siftmi_stage_math exposes what the device computes: fn 5 / 6 are expf_fast / atan2f_fast (what the kernels use), fn 8 / 10 the
candidate of expf_fast_try / atan2f_fast_try as returned, fn 9 / 11 its `ok`.  Expected bits: oracle.expf_array / atan2f_array;
everything is compared as uint32, NaN as "is NaN".  The bands are those of the DEFINING function's binary64 value; the fast
value may differ from it by 2^-45 relative (256 binary64 ulps at most), hence the 512-ulp margin around the guard's 8192:
inside it the guard must refuse, outside it must accept, and what it accepts must already be the oracle's float."""
import ctypes as C

import numpy as np
import pytest

import math_hard_cases as mh

pytestmark = pytest.mark.gpu

FUNCS = ("exp", "atan2")
FN = {"exp": (5, 8, 9), "atan2": (6, 10, 11)}           # wrapper, candidate, ok


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _same(got, want):
    return (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))


class Run:
    """one function on one argument list: the oracle's float and the three device answers"""

    def __init__(self, siftlib, oracle, func, a, b):
        assert a.size <= 40000
        self.a, self.b = a, b
        self.want = oracle.expf_array(a) if func == "exp" else oracle.atan2f_array(a, b)
        res = []
        for fn in FN[func]:
            out = np.full(a.size, 7.0, np.float32)
            assert siftlib.siftmi_stage_math(0, fn, _p(a), _p(b), _p(out), a.size) == 0
            res.append(out)
        self.value, self.cand = res[0], res[1]
        assert np.isin(res[2], (0.0, 1.0)).all()
        self.ok = res[2] == 1.0
        self.value_same, self.cand_same = _same(self.value, self.want), _same(self.cand, self.want)

    def show(self, sel, n=4):
        i = np.nonzero(sel)[0][:n]
        return [(self.a[j], self.b[j], self.value[j], self.cand[j], bool(self.ok[j]), self.want[j]) for j in i]


@pytest.fixture(scope="module")
def hard(siftlib, oracle):
    fx = mh.load()
    runs = {"exp": Run(siftlib, oracle, "exp", fx["exp_x"], fx["exp_x"]),
            "atan2": Run(siftlib, oracle, "atan2", fx["atan2_y"], fx["atan2_x"]),
            "exp_range": Run(siftlib, oracle, "exp", fx["exp_range_x"], fx["exp_range_x"]),
            "atan2_range": Run(siftlib, oracle, "atan2", fx["atan2_range_y"], fx["atan2_range_x"])}
    return fx, runs


@pytest.mark.parametrize("func", FUNCS)
def test_fast_functions_equal_the_oracle_on_every_hard_argument(hard, func):
    """fn 5 / 6, what the kernels call: every stratum, every band"""
    fx, runs = hard
    r = runs[func]
    assert r.value_same.all(), r.show(~r.value_same)


@pytest.mark.parametrize("func", FUNCS)
def test_guard_refuses_inside_the_margin(hard, func):
    """H0 and H1 (d <= 8192 - 512): the fast value is within 256 ulps of the defining one, so within the guard's 8192"""
    fx, runs = hard
    r, band = runs[func], fx[func + "_band"]
    bad = r.ok & ((band == mh.H0) | (band == mh.H1))
    assert not bad.any(), r.show(bad)


@pytest.mark.parametrize("func", FUNCS)
def test_guard_accepts_outside_the_margin_and_the_candidate_is_the_oracle(hard, func):
    """S (8192 + 512 < d <= 65536): usable, and already the oracle's float"""
    fx, runs = hard
    r, band = runs[func], fx[func + "_band"]
    s = band == mh.S
    assert r.ok[s].all(), r.show(s & ~r.ok)
    assert r.cand_same[s].all(), r.show(s & ~r.cand_same)


@pytest.mark.parametrize("func", FUNCS)
def test_guard_band_may_answer_either_way(hard, func):
    """G (within 512 ulps of the guard's 8192): either answer, the returned value is the oracle's.  Both answers occur, so the
    device's threshold does lie in this band."""
    fx, runs = hard
    r, band = runs[func], fx[func + "_band"]
    g = band == mh.G
    assert r.value_same[g].all(), r.show(g & ~r.value_same)
    assert r.ok[g].any() and (~r.ok[g]).any()


@pytest.mark.parametrize("func", FUNCS)
def test_a_usable_candidate_is_the_oracle_value(hard, func):
    """whenever `ok` is true the candidate equals the oracle: every band and stratum, the range cases included"""
    fx, runs = hard
    for r in (runs[func], runs[func + "_range"]):
        bad = r.ok & ~r.cand_same
        assert not bad.any(), r.show(bad)


@pytest.mark.parametrize("func", FUNCS)
def test_outside_the_guarded_range_the_candidate_is_never_usable(hard, func):
    """|x| > 80; an atan2 operand above 1e18f or a smaller one below 1e-18f; zeros, NaN, infinities; sub-normal results:
    `ok` is false and fn 5 / 6 still equal the oracle"""
    fx, runs = hard
    r = runs[func + "_range"]
    assert not r.ok.any(), r.show(r.ok)
    assert r.value_same.all(), r.show(~r.value_same)


@pytest.mark.parametrize("func", FUNCS)
def test_report_how_much_the_guard_is_needed(hard, func):
    """Prints, per stratum and band, the number of arguments, how many candidates were called usable and how many candidates
    differ from the oracle (run with -s).  In H0 / H1 a differing candidate is one that the guard had to catch."""
    fx, runs = hard
    r, band, stratum = runs[func], fx[func + "_band"], fx[func + "_stratum"]
    caught = 0
    for st in range(3):
        for b in (mh.H0, mh.H1, mh.G, mh.S, mh.NO_BAND):
            sel = (stratum == st) & (band == b)
            if sel.any():
                differ = int((~r.cand_same[sel]).sum())
                print("%-5s stratum %s band %-4s: %5d arguments, %5d usable, %3d candidates differ from the oracle"
                      % (func, "abc"[st], mh.BAND_NAMES[b], int(sel.sum()), int(r.ok[sel].sum()), differ))
                if b in (mh.H0, mh.H1):
                    caught += differ
    print("%-5s: %d candidates in H0 / H1 differ from the oracle" % (func, caught))
    hard_bands = (band == mh.H0) | (band == mh.H1)
    assert caught == int((~r.cand_same[hard_bands]).sum())
