"""octave_tail_kernel's in-launch candidate flush against the oracle -- bit for bit, no tolerance.

No frame of tests/pyramid_cases.py makes a wave of the tail kernel park more than five candidates; the `pending > 32` block of
extrema_strip inside that launch, the carry that follows it, the refinement loop over a list of hundreds and the contents of the
tail's own candidate lists were never run by a test.  The striped frames of tests/tail_flush_cases.py reach all of it
(tests/test_tail_flush_cases_host.py proves on the CPU which case reaches what); here they run on a plan exactly as for a user,
and SiftPlan.planes() / last_counts() / tail_candidates() read back what the finished call left in memory.

Every comparison is uint32 / integer equality: all six planes of every octave, tail_first, candidates, c_scale, the tail's
candidate list of every tail octave against the oracle's local_maxmin lists (as sorted sets: the order of a list is that of
the atomics), the records, the overflow flag.  `par` is changed AFTER the plan is made (the plan's octave list comes from the
default border, as the oracle's) and put back whatever happens."""
import contextlib
import ctypes as C

import numpy as np
import pytest

import pyramid_cases as pc
import tail_flush_cases as tf
from util import assert_same_keypoints, sort_rows_bits

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def _par(name):
    from sift_pyocl_amd.param import par
    saved = dict(par)
    try:
        par.update(tf.PARAMS[name])
        yield
    finally:
        par.update(saved)


def _plan(shape, opts=None, **kwargs):
    import sift_pyocl_amd as sp
    plan = sp.SiftPlan(shape=shape, dtype=np.float32, **kwargs)
    for name, value in (opts or {}).items():
        plan.set_option(name, value)
    return plan


def check_tail_lists(plan, exp, what, tail_first):
    """plan.tail_candidates(o) of every tail octave == the oracle's candidates of the three scales, as sorted rows of bits; the
    octaves above the tail have no such list"""
    n_oct = len(exp.sizes)
    for o in range(n_oct):
        if o < tail_first:
            with pytest.raises(RuntimeError):
                plan.tail_candidates(o)
            continue
        got, want = plan.tail_candidates(o), exp.cands[o]
        assert got.shape == want.shape, "%s: octave %d: the tail kept %d candidates, oracle %d" % (what, o, len(got), len(want))
        g, w = sort_rows_bits(got), sort_rows_bits(want)
        bad = np.nonzero((g != w).any(axis=1))[0]
        assert bad.size == 0, "%s: octave %d: %d of %d candidates of the tail's list differ, first %r, oracle %r" % (
            what, o, bad.size, len(w), g[bad[:1]].view(np.float32), w[bad[:1]].view(np.float32))


def check_left(plan, exp, got, want_records, want_overflow, opts, what, tail_first=None):
    opts = opts or {}
    if tail_first is None:
        tail_first = pc.tail_first(exp.sizes, tail=opts.get("tail", 1), tail_pixels=opts.get("tail_pixels", pc.TAIL_PIXELS))
    pc.check_left_behind(plan, exp, what, tail_first, opts.get("fused_refine", 1))
    check_tail_lists(plan, exp, what, tail_first)
    assert_same_keypoints(got, want_records, what)
    assert plan.overflow is bool(want_overflow), "%s: overflow %r, oracle %r" % (what, plan.overflow, want_overflow)
    return tail_first


def check_case(plan, oracle, case, opts=None, what="", tail_first=None):
    """One keypoints() call on `plan` under the case's `par`, and everything it left behind against the oracle"""
    what = "%s %s %r" % (case.name, what, opts or {})
    exp = tf.expectations(oracle, case)
    with _par(case.par):
        got = plan.keypoints(tf.image(case))
        return check_left(plan, exp, got, exp.records, exp.overflow, opts, what, tail_first)


@pytest.mark.parametrize("case", tf.CASES, ids=lambda c: c.name)
def test_flush_frames_leave_the_oracles_lists(siftlib, oracle, case):
    plan = _plan(case.shape, PIX_PER_KP=case.pix_per_kp)
    first = check_case(plan, oracle, case, what="default plan")
    assert [pc.octave_sizes(*case.shape)[o] for o in range(first, plan.octave_max)] == case.octaves
    check_case(plan, oracle, case, what="second call")


FORM_CASES = ("h128_l24", "v64x256_l20", "compo_v128_l24", "h512_l104")
FORMS = [dict(tail=0), dict(fused_refine=0), dict(tail_pixels=1024), dict(overlap=0)]


@pytest.mark.parametrize("opts", FORMS, ids=lambda o: ",".join("%s=%d" % kv for kv in o.items()))
@pytest.mark.parametrize("name", FORM_CASES)
def test_forms_leave_the_same(siftlib, oracle, name, opts):
    """the same frames through the per-octave launches (tail = 0: the 128-slot buffer of extrema_kernel), the two-launch
    detection, a tail that starts one octave later, a single stream: the same records, planes and counts"""
    case = tf.BY_NAME[name]
    plan = _plan(case.shape, opts)
    first = check_case(plan, oracle, case, opts, what="form")
    n_oct = len(pc.octave_sizes(*case.shape))
    if "tail" in opts:
        assert first == n_oct
    if "tail_pixels" in opts:
        assert first == pc.tail_first(pc.octave_sizes(*case.shape)) + 1


@pytest.mark.parametrize("name", FORM_CASES)
def test_tail_timeout_rerun_has_no_tail_list(siftlib, oracle, name):
    """option "tail_fault" = 1: the call is treated as timed out and runs again octave by octave.  The tail launch DID write its
    lists, but the result comes from the re-run: tail_first == n_oct and the accessor refuses every octave."""
    from sift_pyocl_amd import _lib
    case = tf.BY_NAME[name]
    plan = _plan(case.shape, dict(tail_fault=1))
    n_oct = len(pc.octave_sizes(*case.shape))
    check_case(plan, oracle, case, what="tail_fault=1", tail_first=n_oct)
    assert plan.tail_timeouts() == (1, False)
    buf, n = np.full(4 * 3 * 4096, -7.0, np.float32), C.c_int64(-1)
    for o in range(-1, n_oct + 1):
        assert siftlib.siftmi_plan_tail_candidates(plan._handle, o, buf.ctypes.data, buf.size, C.byref(n)) == _lib.EINVAL
        assert b"octave" in siftlib.siftmi_last_error()
    assert n.value == -1 and np.all(buf == -7.0)


def test_alternating_images_leave_their_own_lists(siftlib, oracle):
    """The 594-candidate frame and smooth128 (18 candidates in the same octave, under the default parameters) in turn on one plan,
    ten calls: after every call the lists and counts are those of the image just given -- a counter, a list prefix or parked
    entries left over from the striped image would show in the other's list."""
    case, frame = tf.BY_NAME["v128_l20"], pc.BY_NAME["smooth128"]
    assert case.shape == frame.shape
    fexp = pc.expectations(oracle, frame)
    frecords = oracle.keypoints(np.ascontiguousarray(pc.image(frame), np.float32))
    assert 0 < fexp.c_scale[1].sum() < tf.expectations(oracle, case).c_scale[1].sum()
    plan = _plan(case.shape)
    for call in range(10):
        what = "call %d of A, B, A, B, ..." % call
        if call % 2 == 0:
            check_case(plan, oracle, case, what=what)
        else:
            got = plan.keypoints(pc.image(frame))
            check_left(plan, fexp, got, frecords, False, None, "%s %s" % (frame.name, what))


def test_pix_per_kp_60_overflow_and_growth(siftlib, oracle):
    """kpsize = 128 * 128 // 60 = 273 < the 594 candidates of the tail octave: the oracle flags the overflow because of the tail
    alone (test_tail_flush_cases_host.py), and so must the plan; its lists start at kpsize, grow inside the first call (which
    runs the image again) and no result changes."""
    case = tf.BY_NAME["v128_l20_ppk60"]
    exp = tf.expectations(oracle, case)
    assert exp.overflow is True
    plan = _plan(case.shape, PIX_PER_KP=60)
    assert plan.kpsize == 273 and plan.capacity()[1] == 0
    check_case(plan, oracle, case, what="first call")
    grows = plan.capacity()[1]
    assert grows >= 1, "the candidate lists did not grow"
    check_case(plan, oracle, case, what="second call")
    assert plan.capacity()[1] == grows and plan.tail_timeouts() == (0, True)
    # the same frame on a plan of the default PIX_PER_KP: no overflow, nothing grows
    other = _plan(case.shape)
    check_case(other, oracle, tf.BY_NAME["v128_l20"], what="PIX_PER_KP 10")
    assert other.capacity()[1] == 0 and other.overflow is False


def test_batch_plan_of_two_lanes(siftlib, oracle):
    import sift_pyocl_amd as sp
    cases = [tf.BY_NAME[n] for n in ("h128_l24", "v128_l20", "compo_v128_l24")]
    assert len({c.shape for c in cases}) == 1 and {c.par for c in cases} == {"LOW"}
    bp = sp.BatchPlan(shape=cases[0].shape, dtype=np.float32, lanes=2)
    with _par("LOW"):
        for round_ in range(2):
            res = bp.keypoints_batch([tf.image(c) for c in cases])
            assert len(res) == len(cases)
            for c, r in zip(cases, res):
                assert_same_keypoints(r, tf.expectations(oracle, c).records, "%s BatchPlan round %d" % (c.name, round_))
    assert len(tf.expectations(oracle, cases[2]).records) >= 20


def test_accessor_errors(siftlib, oracle):
    from sift_pyocl_amd import _lib
    case = tf.BY_NAME["v128_l20"]
    exp = tf.expectations(oracle, case)
    n1 = int(exp.c_scale[1].sum())
    assert n1 == len(exp.cands[1]) > 500 and exp.c_scale[2].sum() == 0
    plan = _plan(case.shape)
    L, h = siftlib, plan._handle
    buf, n = np.full(4 * n1 + 1, -7.0, np.float32), C.c_int64(-1)

    def tail(handle, octave, ptr, cap, pn=None):
        return L.siftmi_plan_tail_candidates(handle, octave, ptr, cap, C.byref(n) if pn is None else pn)

    # a plan that has run nothing
    assert tail(h, 1, buf.ctypes.data, buf.size) == _lib.EINVAL and b"not finished a call" in L.siftmi_last_error()
    with pytest.raises(RuntimeError):
        plan.tail_candidates(1)
    with _par(case.par):
        want = plan.keypoints(tf.image(case)).copy()
    # bad arguments on a finished call: refused, nothing written
    null = C.POINTER(C.c_int64)()
    assert tail(None, 1, buf.ctypes.data, buf.size) == _lib.EINVAL and b"null plan" in L.siftmi_last_error()
    assert tail(h, 1, None, buf.size) == _lib.EINVAL and b"null" in L.siftmi_last_error()
    assert tail(h, 1, buf.ctypes.data, buf.size, null) == _lib.EINVAL and b"null" in L.siftmi_last_error()
    assert tail(h, 1, buf.ctypes.data, 4 * n1 - 1) == _lib.EINVAL and b"needs" in L.siftmi_last_error()
    assert tail(h, 1, buf.ctypes.data, 0) == _lib.EINVAL and b"needs" in L.siftmi_last_error()
    for octave in (0, -1, 4, 99):                       # octave 0 is above the tail (tail_first = 1), the others do not exist
        assert tail(h, octave, buf.ctypes.data, buf.size) == _lib.EINVAL and b"octave" in L.siftmi_last_error()
        with pytest.raises(RuntimeError):
            plan.tail_candidates(octave)
    assert np.all(buf == -7.0) and n.value == -1
    # an exact buffer is enough, the guard float behind it stays
    assert tail(h, 1, buf.ctypes.data, 4 * n1) == 0 and n.value == n1
    assert buf[-1] == -7.0 and np.array_equal(sort_rows_bits(buf[:-1].reshape(-1, 4)), sort_rows_bits(exp.cands[1]))
    # an octave of the tail without a candidate: zero floats are enough, nothing is written
    buf[:] = -7.0
    assert tail(h, 2, buf.ctypes.data, 0) == 0 and n.value == 0 and np.all(buf == -7.0)
    assert plan.tail_candidates(2).shape == (0, 4) and plan.tail_candidates(1).shape == (n1, 4)
    # reading does not disturb the plan: the next call gives the same records and lists
    with _par(case.par):
        assert_same_keypoints(plan.keypoints(tf.image(case)), want, "keypoints after tail_candidates()")
    check_tail_lists(plan, exp, "after reading", 1)
