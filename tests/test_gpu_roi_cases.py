"""GPU tests of the brute-force matcher's region-of-interest rule -- which flag a POSITION gets -- on the crafted cases of
tests/roi_cases.py: match_roi_flags_kernel (k_match.hpp) read through the pairs of siftmi_match_ex and, the cases' ratio being
the default one, of MatchPlan.match, with host lists and with device lists, in modes 1 and 2, plain and mutual.

The expected pairs are those of the numpy restatement (tests/roi_ref.py; tests/test_roi_cases_host.py pins the oracle and, where
the reference is defined, its own kernel to it, and shows that each probe decides something).  Every comparison is exact: the
sorted pair rows, n_out and n_total.  Also here: the mask's lifetime on one plan, and set_roi's conversion to int8."""
import ctypes as C

import numpy as np
import pytest

import match_cases as mc
import roi_cases as rc
import roi_ref
from util import sort_rows

pytestmark = pytest.mark.gpu
MASK_NAMES = list(rc.MASKS)


def rows_of(pairs):
    return sort_rows(np.asarray(pairs, np.int32).reshape(-1, 2))


def on_device(k):
    import torch
    return torch.from_numpy(k.view(np.uint8).reshape(-1).copy()).cuda()


def abi_match_ex(siftlib, mp, a, b, th, roi_mode, mutual, device=False):
    """(rc, pairs[:n_out], n_out, n_total) of siftmi_match_ex, the lists on the host or (device) in device memory"""
    cap = max(1, len(a))
    pairs = np.full((cap, 2), -7, np.int32)
    n, total = C.c_int64(-5), C.c_int64(-5)
    keep = (on_device(a), on_device(b)) if device else (a, b)
    pa, pb = (keep[0].data_ptr(), keep[1].data_ptr()) if device else (a.ctypes.data, b.ctypes.data)
    rc_ = siftlib.siftmi_match_ex(mp._handle, C.c_void_p(pa), len(a), int(device), C.c_void_p(pb), len(b), int(device), C.c_float(float(th)),
                                  roi_mode, int(mutual), pairs.ctypes.data, cap, C.byref(n), C.byref(total))
    assert (pairs[n.value:] == -7).all()                             # nothing written beyond n_out
    return rc_, pairs[:n.value].copy(), n.value, total.value


def check(siftlib, mp, c, want=None):
    """one case through both entry points, with host and with device lists"""
    assert np.float32(c.th).tobytes() == mc.RATIO.tobytes()
    want = roi_ref.expected_pairs(c.a, c.b, c.roi, c.mode, c.mutual, c.th) if want is None else want
    for device in (False, True):
        where = " [device lists]" if device else " [host lists]"
        rc_, pairs, n, total = abi_match_ex(siftlib, mp, c.a, c.b, c.th, c.mode, c.mutual, device)
        assert rc_ == 0, c.name + where
        assert n == total == len(want), "%s%s: n_out %d, n_total %d, expected %d pairs" % (c.name, where, n, total, len(want))
        assert np.array_equal(rows_of(pairs), want), c.name + " [siftmi_match_ex]" + where
        a, b = (on_device(c.a), on_device(c.b)) if device else (c.a, c.b)
        got = mp.match(a, b, raw_results=True, roi_mode=c.mode, mutual=c.mutual)
        assert got.dtype == np.int32 and got.shape == (len(want), 2), "%s%s: %s pairs, expected %d" % (c.name, where, got.shape, len(want))
        assert np.array_equal(rows_of(got), want), c.name + " [MatchPlan.match]" + where
    return want


@pytest.fixture(scope="module")
def expected():
    """the restatement's pairs of every case, computed once"""
    cache = {}

    def get(mask):
        if mask not in cache:
            cache[mask] = [(c, roi_ref.expected_pairs(c.a, c.b, c.roi, c.mode, c.mutual, c.th)) for c in rc.cases(mask)]
        return cache[mask]
    return get


@pytest.fixture(scope="module")
def mp(siftlib):
    import sift_pyocl_amd as sp
    return sp.MatchPlan()


def probe_calls(mask, expected):
    """a short list of a mask's cases that between them read every probe: the query flags of both modes, the list flags, and
    three one-probe calls"""
    forced = [cw for cw in expected(mask) if cw[0].kind == "forced" and not cw[0].mutual]
    return [cw for cw in expected(mask) if cw[0].kind in ("query", "list") and not cw[0].mutual] + forced[:1] + forced[9:12]


# ---------------------------------------------------------------------------------------------- every case
@pytest.mark.parametrize("mask", MASK_NAMES)
def test_flags_of_every_probe(siftlib, mp, expected, mask):
    """every case of the mask: the probes' query flags (modes 1 and 2), list flags (mode 2) and forced zeros (mode 1, one probe per
    call), plain and mutual.  The NaN probes are among them: a kernel that converts a NaN to 0 puts them on row or column 0."""
    mp.set_roi(rc.MASKS[mask])
    seen = set()
    for c, want in expected(mask):
        check(siftlib, mp, c, want)
        seen.add((c.kind, c.mode, c.mutual))
    assert len(seen) == 8


# ---------------------------------------------------------------------------------------------- the mask's lifetime
def test_mask_lifetime_on_one_plan(siftlib, expected):
    """64 x 257, then 3 x 5, then 5 x 3 of the same bytes, unset (a non-zero roi_mode raises), then 1 x 1, on ONE plan: the right
    pairs at every step.  A smaller mask after a larger one must be read with its own shape and bytes."""
    import sift_pyocl_amd as sp
    plan = sp.MatchPlan()
    last = None
    for mask in ("64x257 ones", "3x5", "5x3", None, "1x1", "64x257 zeros", "7x1"):
        if mask is None:
            plan.unset_roi()
            c = last[0]
            for mode in (1, 2, "strict", "reference"):
                with pytest.raises(RuntimeError):
                    plan.match(c.a, c.b, raw_results=True, roi_mode=mode)
            rc_, _, n, total = abi_match_ex(siftlib, plan, c.a, c.b, c.th, 2, False)
            assert rc_ != 0                                          # the C ABI refuses it too
            plain = plan.match(c.a, c.b, raw_results=True)           # roi_mode 0 still works, and ignores the positions
            a0, b0 = c.a.copy(), c.b.copy()
            a0["x"] = a0["y"] = b0["x"] = b0["y"] = 0
            assert np.array_equal(rows_of(plain), rows_of(roi_ref.wr.match(a0, b0, np.inf)))
            continue
        plan.set_roi(rc.MASKS[mask])
        for c, want in probe_calls(mask, expected):
            check(siftlib, plan, c, want)
            last = (c, want)


# ---------------------------------------------------------------------------------------------- set_roi's conversion
def test_set_roi_converts_as_ascontiguousarray_int8(siftlib, expected):
    """numpy.ascontiguousarray(roi, numpy.int8) is the conversion: a bool mask; a uint8 200 becomes -56 and stays on; an int16 256
    becomes 0 and is off; a float 0.5 becomes 0 and is off; a mask that is not 2-D is refused"""
    import sift_pyocl_amd as sp
    plan = sp.MatchPlan()
    base = rc.MASKS["3x5"]
    cases = [cw[0] for cw in probe_calls("3x5", expected)]
    given = [
        ("bool", base != 0, base != 0),
        ("uint8 of 200", np.where(base != 0, 200, 0).astype(np.uint8), base != 0),
        ("int16 of 256 and 1", np.where(base != 0, 256, 1).astype(np.int16), base == 0),
        ("float of 0.5 and -1.5", np.where(base != 0, 0.5, -1.5), base == 0),
        ("Fortran-ordered int8", np.asfortranarray(base), base != 0),
        ("a strided view", np.repeat(base, 2, axis=1)[:, ::2], base != 0),
    ]
    for label, roi, on in given:
        plan.set_roi(roi)
        as_int8 = np.ascontiguousarray(roi, np.int8)
        assert np.array_equal(as_int8 != 0, on), label
        assert np.array_equal(plan.roi, as_int8) and plan.roi.dtype == np.int8
        for c in cases:
            want = roi_ref.expected_pairs(c.a, c.b, as_int8, c.mode, c.mutual, c.th)
            for device in (False, True):
                a, b = (on_device(c.a), on_device(c.b)) if device else (c.a, c.b)
                got = plan.match(a, b, raw_results=True, roi_mode=c.mode, mutual=c.mutual)
                assert got.shape == (len(want), 2) and np.array_equal(rows_of(got), want), "%s: %s" % (label, c.name)
    assert np.ascontiguousarray(np.uint8(200), np.int8) == -56
    kept = plan.roi
    for bad in (base.ravel(), base.reshape(3, 5, 1), np.int8(1)):
        with pytest.raises(RuntimeError):
            plan.set_roi(bad)
        assert plan.roi is kept
    # the refused masks changed nothing on the device: the last good one still answers
    c = cases[0]
    want = roi_ref.expected_pairs(c.a, c.b, np.ascontiguousarray(given[-1][1], np.int8), c.mode, c.mutual, c.th)
    rc_, pairs, n, total = abi_match_ex(siftlib, plan, c.a, c.b, c.th, c.mode, c.mutual)
    assert rc_ == 0 and n == total == len(want) and np.array_equal(rows_of(pairs), want)
