"""GPU tests of both median selects on crafted match sets (tests/shift_cases.py): every case goes
through siftmi_match_shift on several grids and, as a segment among all the others, through siftmi_match_shift_batch -- in the
order of the families, in reverse order (every row0 and list offset another) and against one shared first list -- and gives the
dictated six floats as bit patterns (a NaN matches any NaN), the dictated n, and the keep mask and n_keep that the keep family
dictates (for the other families: the restatement's).  The batch's segments are, bit for bit, the single calls' results.
MatchPlan.shift and MatchPlan.shift_batch hand the same values back.  No tolerance anywhere: tests/test_shift_cases_host.py shows
on the CPU what these sets reach in either scan and which faults they catch."""
import numpy as np
import pytest

import estimate_batch_ref as eb
import shift_cases as sc
import shift_ref as sr
from test_gpu_estimate_batch import abi_shift as abi_shift_batch
from test_gpu_shift import abi_shift, on_device

pytestmark = pytest.mark.gpu

#: every level of every_digit on its own (512 sets: the lo and the hi instance), the other families whole
GROUPS = tuple("every_digit p=%d" % p for p in range(4)) + sc.FAMILIES[1:]
_SINGLE, _REF, _BATCH = {}, {}, {}


def group(name):
    if name.startswith("every_digit"):
        return [c for c in sc.family("every_digit") if c.x.claims["level"] == int(name[-1])]
    return sc.family(name)


def expected_keep(c):
    """(keep bool (M,), n_keep): dictated for the keep family, the restatement's elsewhere"""
    if c.keep is not None:
        return c.keep, c.n_keep
    if c.name not in _REF:
        out, counts, keep = sr.shift(*c.lists(), mask=c.mask, tol=c.tol)
        _REF[c.name] = (keep, int(counts[1]))
    return _REF[c.name]


def check_single(L, mp, c, blocks):
    kp1, kp2, pairs = c.lists()
    out, counts, keep, ms = abi_shift(L, mp, kp1, kp2, pairs, c.mask, blocks, c.tol)
    assert sr.same_bits(out, c.want), "%s, blocks %d\n got  %r\n want %r" % (c.name, blocks, out, c.want)
    assert counts[0] == c.n, (c.name, blocks, counts)
    if c.tol is None:
        assert keep is None and counts[1] == 0, (c.name, blocks, counts)
    else:
        wkeep, n_keep = expected_keep(c)
        assert np.array_equal(keep, wkeep.astype(np.uint8)) and counts[1] == n_keep, (c.name, blocks, counts, n_keep)
    return out, counts, keep


def single(L, mp, c):
    """the single call's results under the default grid, made once"""
    if c.name not in _SINGLE:
        _SINGLE[c.name] = check_single(L, mp, c, 0)
    return _SINGLE[c.name]


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


# ---------------------------------------------------------------------------------------------- siftmi_match_shift
@pytest.mark.parametrize("name", GROUPS)
def test_single_form_gives_the_dictated_results(siftlib, mp, name):
    """the default grid and three workgroups; one workgroup (up to five rows per lane) for the sets above 256 rows"""
    cases = group(name)
    assert cases
    for c in cases:
        single(siftlib, mp, c)
        check_single(siftlib, mp, c, 3)
        if c.M > 256:
            check_single(siftlib, mp, c, 1)


# ---------------------------------------------------------------------------------------------- siftmi_match_shift_batch
def batch(cases, order, tag):
    key = (tag, order)
    if key not in _BATCH:
        cases = list(cases)[::-1] if order == "reverse" else list(cases)
        b = eb.from_segments("shift cases %s %s" % key, [c.segment() for c in cases])
        _BATCH[key] = (cases, b.shared() if order == "shared" else b)
    return _BATCH[key]


def check_batch(L, mp, cases, b, tol):
    out, counts, keep, ms = abi_shift_batch(L, mp, b, tol)
    row0 = np.concatenate([[0], np.cumsum(b.pair_counts)])
    for s, c in enumerate(cases):
        what = (b.name, s, c.name, tol)
        assert sr.same_bits(out[s], c.want), "%r\n got  %r\n want %r" % (what, out[s], c.want)
        one, one_counts, one_keep = single(L, mp, c)
        assert sr.same_bits(out[s], one) and sr.same_bits(one, out[s]), "%r\n got  %r\n single %r" % (what, out[s], one)
        assert counts[s, 0] == c.n == one_counts[0], (what, counts[s])
        if tol is None:
            assert counts[s, 1] == 0, (what, counts[s])
        else:
            assert c.tol == tol
            wkeep, n_keep = expected_keep(c)
            rows = slice(int(row0[s]), int(row0[s + 1]))
            assert np.array_equal(keep[rows], wkeep.astype(np.uint8)) and np.array_equal(keep[rows], one_keep), what
            assert counts[s, 1] == n_keep == one_counts[1], (what, counts[s], n_keep)


@pytest.mark.parametrize("order", ["forward", "reverse", "shared"])
def test_batch_segments_are_the_dictated_results_and_the_single_calls(siftlib, mp, order):
    """all cases as the segments of ONE call (no keep mask: a call has one tol), then the cases of each tol as one call with it"""
    cases, b = batch(sc.all_cases(), order, "all")
    assert 2000 < b.S == len(sc.all_cases()) < 65535 and (b.counts1 is None) == (order == "shared") and b.mask is not None
    check_batch(siftlib, mp, cases, b, None)
    tols = sorted(set(c.tol for c in sc.all_cases() if c.tol is not None))
    assert tols == [0.0, sc.UNIT, 0.5, 2.0 ** 24, np.inf]
    for tol in tols:
        cases, b = batch([c for c in sc.all_cases() if c.tol == tol], order, "tol %r" % tol)
        check_batch(siftlib, mp, cases, b, tol)


# ---------------------------------------------------------------------------------------------- the methods
def chosen():
    """one case per family: the one with the most rows that has a tol"""
    return [max((c for c in sc.family(name) if c.tol is not None), key=lambda c: c.M) for name in sc.FAMILIES]


def test_python_entries(siftlib, mp):
    import torch
    cases = chosen()
    assert [c.family for c in cases] == list(sc.FAMILIES)
    for k, c in enumerate(cases):
        kp1, kp2, pairs = c.lists()
        mask = c.mask if c.mask is None or k % 2 else c.mask != 0
        if k % 3 == 2:
            kp1, kp2, pairs = on_device(kp1), on_device(kp2), torch.from_numpy(pairs).cuda()
        (dx, dy), n, keep, raw = mp.shift(kp1, kp2, pairs, mask=mask, tol=c.tol, return_ranks=True)
        wkeep, n_keep = expected_keep(c)
        assert sr.same_bits(raw, c.want) and sr.same_bits(np.float32([dx, dy]), c.want[:2]) and n == c.n, c.name
        assert keep.dtype == np.bool_ and np.array_equal(keep, wkeep), c.name
        (dx, dy), n = mp.shift(kp1, kp2, pairs, mask=mask)
        assert sr.same_bits(np.float32([dx, dy]), c.want[:2]) and n == c.n, c.name
    b = eb.from_segments("chosen", [c.segment() for c in cases])
    want = np.stack([c.want for c in cases])
    for form in (b, b.shared()):
        args = (form.kp1, form.counts1, form.kp2, form.counts2, form.pairs, form.pair_counts)
        shifts, n, raw = mp.shift_batch(*args, mask=form.mask, return_ranks=True)
        assert eb.same_bits32(raw, want) and eb.same_bits32(shifts, want[:, :2]) and n.tolist() == [c.n for c in cases]
        # one tol for the whole call: against the restatement on every segment, and the dictated medians all the same
        wout, wcounts, wkeep = eb.shift_batch(form, np.inf)
        shifts, n, keep, n_keep, raw = mp.shift_batch(*args, mask=torch.from_numpy(form.mask != 0).cuda(), tol=np.inf, return_ranks=True)
        assert eb.same_bits32(raw, want) and eb.same_bits32(wout, want) and np.array_equal(keep, wkeep)
        assert n_keep.tolist() == wcounts[:, 1].tolist() and n.tolist() == wcounts[:, 0].tolist()
