"""GPU tests of the device fit on crafted match sets (tests/fit_cases.py): on sets that stand on
both sides of `n < 3 || !(fabs(det) > 1e-12 * fmax(1.0, scale))`, in both of its regimes, siftmi_match_fit gives the 20 doubles of
the restatement bit for bit on every grid, the status and the values exact arithmetic dictates, and a model that
fit_cases.solve_from_results rebuilds from the returned moments alone; MatchPlan.fit hands it back; and
siftmi_match_fit_batch / MatchPlan.fit_batch -- the second copy of the rule, k_estimate_batch.hpp -- give for every segment the
single call's result bit for bit.  No tolerance anywhere: tests/test_fit_cases_host.py shows on the CPU what these sets reach."""
import ctypes as C

import numpy as np
import pytest

import estimate_batch_ref as eb
import fit_cases as fc
import fit_ref as fr

pytestmark = pytest.mark.gpu

FILL = -77.0
GRIDS = (0, 1, 3, 1024)
PLACES = ((0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 1, 0), (0, 1, 0, 1))
#: every ladder on its own, the other families whole
GROUPS = tuple(fc.LADDERS) + ("big",) + fc.FAMILIES[1:]


def group(name):
    if name in fc.LADDERS:
        return fc.ladder(name)
    return fc.big_ladder() if name == "big" else fc.family(name)


def on_device(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def abi_fit(L, mp, kp1, kp2, pairs, mask=None, blocks=0, place=(0, 0, 0, 0)):
    """straight through the C ABI (include/siftmi.h); place = (kp1, kp2, pairs, mask) on the device?  Returns the 20 doubles,
    filled with FILL before the call."""
    import torch
    from sift_pyocl_amd import _lib
    M = int(pairs.shape[0])
    keep = []

    def ptr(a, dev):
        a = np.ascontiguousarray(a)
        if dev:
            t = on_device(a); keep.append(t)
            return t.data_ptr()
        keep.append(a)
        return a.ctypes.data
    p1, p2, pp = ptr(kp1, place[0]), ptr(kp2, place[1]), ptr(pairs.astype(np.int32), place[2])
    pm = None if mask is None else ptr(np.asarray(mask).astype(np.uint8), place[3])
    if any(place):
        torch.cuda.synchronize()
    out = np.full(20, FILL, np.float64)
    ms = C.c_double(-1)
    rc = L.siftmi_match_fit(mp._handle, p1, len(kp1), place[0], p2, len(kp2), place[1], pp, M, place[2],
                            pm, place[3] if mask is not None else 0, blocks, out.ctypes.data, C.byref(ms))
    assert rc == 0, _lib.last_error()
    return out


def abi_fit_batch(L, mp, b, blocks=0, place=(0, 0, 0, 0)):
    """siftmi_match_fit_batch on an estimate_batch_ref.Batch: (S, 20), filled with FILL before the call"""
    import torch
    from sift_pyocl_amd import _lib
    keep = []

    def ptr(a, dev):
        a = np.ascontiguousarray(a)
        if dev:
            t = on_device(a); keep.append(t)
            return t.data_ptr()
        keep.append(a)
        return a.ctypes.data
    c1 = None if b.counts1 is None else np.ascontiguousarray(b.counts1, np.int64)
    c2, pc = np.ascontiguousarray(b.counts2, np.int64), np.ascontiguousarray(b.pair_counts, np.int64)
    head = [mp._handle, ptr(b.kp1, place[0]), len(b.kp1), place[0], ptr(b.kp2, place[1]), len(b.kp2), place[1], b.S,
            None if c1 is None else c1.ctypes.data, c2.ctypes.data, ptr(b.pairs, place[2]), len(b.pairs), place[2], pc.ctypes.data,
            None if b.mask is None else ptr(b.mask, place[3]), place[3] if b.mask is not None else 0]
    if any(place):
        torch.cuda.synchronize()
    out = np.full((b.S, 20), FILL, np.float64)
    ms = C.c_double(-1)
    rc = L.siftmi_match_fit_batch(*head, blocks, out.ctypes.data, C.byref(ms))
    assert rc == 0, _lib.last_error()
    return out


def check_dictated(c, got, what):
    """status, n and whatever else exact arithmetic prescribes for the case, and the solve rebuilt from the returned moments"""
    d = c.dictated
    assert got[fr.STATUS] == c.status() and got[fr.N] == d["n"], (what, got)
    if "means" in d:
        assert got[fr.MEANS].tolist() == list(d["means"]), (what, got)
    if "model" in d:
        assert got[fr.MODEL].tolist() == list(d["model"]), (what, got)
    if "ssr" in d:
        assert got[fr.SSR] == 0.0 and not np.signbit(got[fr.SSR]), (what, got)
    if c.exact_sums:
        assert [float(v) for v in c.exact()["moments"]] == got[fr.MOMENTS].tolist(), (what, got)
    assert fc.solved_like(got), (what, got, fc.solve_from_results(got))


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


# ---------------------------------------------------------------------------------------------- siftmi_match_fit
@pytest.mark.parametrize("name", GROUPS)
def test_fit_on_every_grid(siftlib, mp, name):
    """every set of the group under the default grid and blocks = 1, 3, 1024; lists, pairs and mask in turn on host and device"""
    turn = 0
    for c in group(name):
        kp1, kp2, pairs = c.lists()
        for blocks in GRIDS:
            place = PLACES[turn % len(PLACES)]
            turn += 1
            got = abi_fit(siftlib, mp, kp1, kp2, pairs, c.mask, blocks, place)
            want = c.want(blocks)
            assert fr.same_bits(got, want), "%s, blocks %d, place %r\n got  %r\n want %r" % (c.name, blocks, place, got, want)
            check_dictated(c, got, (c.name, blocks))


def test_statuses_on_both_sides_of_the_threshold(siftlib, mp):
    """the rule in one place: along every ladder the device's status flips where exact arithmetic says, once"""
    for name in fc.LADDERS:
        rungs = fc.ladder(name)
        got = [abi_fit(siftlib, mp, *c.lists())[fr.STATUS] for c in rungs]
        assert got == [c.status() for c in rungs], (name, got)
        assert got.count(fr.OK) == got.count(fr.DEGENERATE) == fc.RUNGS_PER_SIDE
    got = dict((c.name.split("/")[1], abi_fit(siftlib, mp, *c.lists())[fr.STATUS]) for c in fc.tiny_cluster())
    assert got["j=9 m=1"] == fr.OK and got["j=10 m=1"] == fr.DEGENERATE and got["j=11 m=4"] == fr.DEGENERATE and got["j=11 m=5"] == fr.OK


# ---------------------------------------------------------------------------------------------- MatchPlan.fit
@pytest.mark.parametrize("name", fc.FAMILIES)
def test_python_entry(siftlib, mp, name):
    import torch
    cases = group(name) if name != "ladder_line" else fc.ladder("steep") + fc.ladder("vertical") + fc.big_ladder()[1:3]
    for k, c in enumerate(cases):
        kp1, kp2, pairs = c.lists()
        mask = c.mask if c.mask is None or k % 2 else c.mask != 0
        if k % 3 == 2:
            kp1, kp2, pairs = on_device(kp1), on_device(kp2), torch.from_numpy(pairs).cuda()
        model, rms, n, raw = mp.fit(kp1, kp2, pairs, mask=mask, return_moments=True)
        assert fr.same_bits(raw, c.want()), c.name
        assert (model is None) == (c.status() != fr.OK) and n == c.dictated["n"] and type(n) is int, c.name
        if model is None:
            assert np.isnan(rms), c.name
        else:
            assert fr.same_bits(model, c.want()[fr.MODEL]) and rms == float(np.sqrt(raw[fr.SSR] / raw[fr.N])), c.name
        if name == "exact_fit":
            assert model.tolist() == list(fc.MAP) and rms == 0.0, c.name


# ---------------------------------------------------------------------------------------------- the batch entries
def crafted_batch():
    """the segments the second copy of the rule has to get right side by side: an OK rung, the DEGENERATE rung after it, a segment
    without a pair, huge, a tiny_cluster pair either side of fmax, exact_fit, the 28 803-pair ladder, three pairs"""
    diagonal = fc.ladder("diagonal")
    by = dict((c.name.split("/")[1], c) for c in fc.tiny_cluster() + fc.min_n())
    empty = fc.Case("min_n", "no pair", np.zeros((0, 4), np.float32))
    cases = [diagonal[fc.RUNGS_PER_SIDE - 1], diagonal[fc.RUNGS_PER_SIDE], empty, fc.huge()[1], by["j=9 m=1"], by["j=10 m=1"],
             fc.exact_fit()[-1], fc.big_ladder()[1], by["triangle"]]
    return cases, eb.from_segments("fit cases", [c.segment() for c in cases])


@pytest.mark.parametrize("form", ["separate", "shared"])
def test_batch_rows_are_the_single_calls(siftlib, mp, form):
    import torch
    cases, batch = crafted_batch()
    assert [c.status() for c in cases] == [fr.OK, fr.DEGENERATE, fr.EMPTY, fr.OK, fr.OK, fr.DEGENERATE, fr.OK, fr.OK, fr.OK]
    assert cases[7].M == fc.BIG_PAIRS and batch.mask is not None
    if form == "shared":
        batch = batch.shared()
    for blocks, place in zip(GRIDS, PLACES):
        out = abi_fit_batch(siftlib, mp, batch, blocks, place)
        for s, c in enumerate(cases):
            single = abi_fit(siftlib, mp, *c.lists(), mask=c.mask, blocks=blocks) if c.M else c.want(blocks)
            assert fr.same_bits(out[s], single), "%s: segment %d (%s), blocks %d\n got  %r\n want %r" % (form, s, c.name, blocks, out[s], single)
            assert fr.same_bits(out[s], c.want(blocks)), (form, s, c.name, blocks)
            check_dictated(c, out[s], (form, s, c.name, blocks))
    # the method: NaN models exactly on the rows off status 0
    args = (batch.kp1, batch.counts1, batch.kp2, batch.counts2, batch.pairs, batch.pair_counts)
    for mask in (batch.mask, torch.from_numpy(batch.mask != 0).cuda()):
        models, rms, n, raw = mp.fit_batch(*args, mask=mask, return_moments=True)
        assert eb.same_bits64(raw, np.stack([c.want() for c in cases]))
        off = np.array([c.status() != fr.OK for c in cases])
        assert np.array_equal(np.isnan(models).all(axis=1), off) and np.array_equal(np.isnan(models).any(axis=1), off)
        assert np.array_equal(np.isnan(rms), off) and n.tolist() == [c.dictated["n"] for c in cases]
        assert eb.same_bits64(models[~off], raw[~off][:, fr.MODEL])
        assert models[6].tolist() == list(fc.MAP) and rms[6] == 0.0 and rms[3] == 0.0


def test_batch_of_every_rung(siftlib, mp):
    """every rung of every ladder and every tiny_cluster set as the segments of one batch: the second copy of the rule along the
    threshold, each row against its own single call"""
    cases = [c for name in fc.LADDERS for c in fc.ladder(name)] + fc.tiny_cluster() + fc.rounded_det()
    batch = eb.from_segments("rungs", [c.segment() for c in cases])
    for blocks in (0, 1):
        out = abi_fit_batch(siftlib, mp, batch, blocks, (1, 1, 1, 0))
        for s, c in enumerate(cases):
            assert fr.same_bits(out[s], c.want(blocks)), (s, c.name, blocks, out[s], c.want(blocks))
            check_dictated(c, out[s], (s, c.name, blocks))
    single = np.stack([abi_fit(siftlib, mp, *c.lists()) for c in cases])
    assert eb.same_bits64(abi_fit_batch(siftlib, mp, batch), single)
