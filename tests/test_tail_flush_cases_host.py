"""What tests/test_gpu_tail_flush.py rests on, checked without a GPU: the new accessor is part of the C ABI and refuses a null
plan, the generators' planes really tie, every case of tail_flush_cases.CASES keeps the tail octaves it is meant for, and the
replay of the tail kernel's wave walk on the oracle's extrema reaches, across the list, every path of the in-launch flush.
These are conditions on the oracle's output, re-derived here on every run, not recorded figures."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pyramid_cases as pc
import tail_flush_cases as tf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_accessor_is_declared_exported_and_bound():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    L = _lib.lib()
    name = "siftmi_plan_tail_candidates"
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "siftmi.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, header), "%s is not declared in include/siftmi.h" % name
    assert hasattr(L, name) and name in _lib.exported_symbols()
    import sift_pyocl_amd as sp
    assert callable(sp.SiftPlan.tail_candidates)
    # a null plan is refused before anything touches a device: the same answer on any machine
    buf, n = np.full(64, 7.0, np.float32), C.c_int64(-1)
    assert L.siftmi_plan_tail_candidates(None, 1, buf.ctypes.data, buf.size, C.byref(n)) == _lib.EINVAL
    assert b"null plan" in L.siftmi_last_error()
    assert n.value == -1 and np.all(buf == 7.0)


def test_module_imports_nothing_from_the_package():
    src = open(os.path.join(ROOT, "tests", "tail_flush_cases.py")).read()
    assert not re.search(r"^\s*(import|from)\s+(sift_pyocl_amd|oracle)\b", src, flags=re.M)


def test_generators():
    h, v = tf.hstripes((7, 5), 24), tf.vstripes((5, 7), 24)
    assert h.dtype == v.dtype == np.float32 and h.shape == (7, 5) and np.array_equal(h, v.T)
    want = np.cos(2.0 * np.pi * np.arange(7, dtype=np.float64) / 24).astype(np.float32)
    assert np.array_equal(h[:, 0], want) and np.all(h == h[:, :1])
    for axis, stripes in ((0, tf.hstripes((128, 128), 24)), (1, tf.vstripes((128, 128), 24))):
        img = tf.compo((128, 128), stripes, 84, axis)
        a, b = (img[:84], img[84:]) if axis == 0 else (img[:, :84], img[:, 84:])
        assert img.dtype == np.float32 and np.array_equal(a, stripes[:84] if axis == 0 else stripes[:, :84])
        assert -1.0 <= b.min() and b.max() <= 1.0 and len(np.unique(b)) > b.size // 2         # the rest is the noise, in [-1, 1]
    # the parameter sets: LOW's negative edge thresholds, the two border variants
    assert tf.PARAMS["DEFAULT"] == {} and tf.PARAMS["LOW"] == dict(PeakThresh=255.0 * 0.0004 / 3.0, EdgeThresh=-1.0, EdgeThresh1=-1.0)
    assert [tf.border_of(n) for n in ("DEFAULT", "LOW", "LOW_B2", "LOW_B9")] == [5, 5, 2, 9]
    # W = 128 at border 2: 124 columns are exactly two full strips (lane 62 of strip 1 tests the last column, x = 125)
    assert (128 - 2 * 2) == 2 * 62 and (128 - 2 * 2 + 61) // 62 == 2 == (128 - 2 * 5 + 61) // 62


def test_stripe_planes_tie_bitwise(oracle):
    """every row of every plane of an hstripes frame is bitwise constant (every column of a vstripes frame): the blur of a
    frame constant along x sums the same products in the same order for every x, also through the reflected margins"""
    for name in ("h128_l24", "h118x114_l20", "h64x256_l20", "h512_l104"):
        for o, planes in enumerate(tf.expectations(oracle, tf.BY_NAME[name]).planes):
            u = planes.view(np.uint32)
            assert np.all(u == u[:, :, :1]), "%s octave %d: a row is not constant" % (name, o)
    for name in ("v128_l20", "v256x64_l20"):
        for o, planes in enumerate(tf.expectations(oracle, tf.BY_NAME[name]).planes):
            u = planes.view(np.uint32)
            assert np.all(u == u[:, :1, :]), "%s octave %d: a column is not constant" % (name, o)


def test_oracle_params(oracle):
    for name in tf.PARAMS:
        par, dflt = tf.oracle_params(oracle, name, 60), oracle.default_params()
        p = tf.PARAMS[name]
        assert par.pix_per_kp == 60 and par.border_dist == p.get("BorderDist", 5)
        assert par.peak_thresh == np.float32(p.get("PeakThresh", dflt.peak_thresh))
        assert par.edge_thresh0 == np.float32(p.get("EdgeThresh1", dflt.edge_thresh0))
        assert par.edge_thresh == np.float32(p.get("EdgeThresh", dflt.edge_thresh))
        assert (par.ori_sigma, par.init_sigma, par.octave_max) == (dflt.ori_sigma, dflt.init_sigma, dflt.octave_max)


@pytest.mark.parametrize("case", tf.CASES, ids=lambda c: c.name)
def test_cases_keep_their_tail_octaves(oracle, case):
    """the plan's octave list comes from the default border (the plan is made before `par` is changed, as a caller's would be),
    and so does the oracle's"""
    H, W = case.shape
    sizes = pc.octave_sizes(H, W)
    assert len(sizes) == oracle.octave_count(H, W) and sizes == tf.expectations(oracle, case).sizes
    first = pc.tail_first(sizes)
    assert sizes[first:] == case.octaves and 0 <= case.watch < len(case.octaves), (case.name, sizes, first)
    for form in (dict(tail_pixels=1024), dict(tail=0)):                    # the forms of the GPU module move or drop the tail
        assert pc.tail_first(sizes, **form) > first


def _replays(oracle, case):
    exp = tf.expectations(oracle, case)
    first = pc.tail_first(exp.sizes)
    for o in range(first, len(exp.sizes)):
        W, H = exp.sizes[o]
        assert len(exp.raw[o]) >= len(exp.cands[o]) == exp.c_scale[o].sum()
        yield o - first, o, tf.replay(exp.raw[o], exp.cands[o], W, H, tf.border_of(case.par))


def test_replay_restates_the_walk():
    """the replay on hand-made lists: a row of 40 ties flushes at once, three rows of 12 flush on the third with nothing carried,
    entries of an earlier strip are `carried` into the flush of a later one, an entry absent from `kept` is not stored"""
    def rows(r, cols, scale=1):
        return np.array([(1.0, r, c, scale) for c in cols], np.float32).reshape(-1, 4)
    one = rows(5, range(5, 45))
    r = tf.replay(one, one, 64, 64, 5)
    assert [(f.wave, f.sx, f.sy, f.row, f.parked, f.carried, f.row_parked, f.stored) for f in r.flushes] == [(0, 0, 0, 5, 40, 0, 40, 40)]
    assert r.final.sum() == 0 and r.max_row == 40 and r.stored_after_flush == 0
    three = np.concatenate([rows(9 + i, range(5, 17)) for i in range(3)])                 # strip sy = 1: rows 9..12, wave 1
    r = tf.replay(three, three[:-1], 64, 64, 5)
    assert [(f.wave, f.sy, f.row, f.parked, f.carried, f.stored) for f in r.flushes] == [(1, 1, 11, 36, 0, 35)]
    # wave 0 owns strips sy = 0 (rows 5..8) and sy = 8 (rows 37..40) of a 64 x 64 octave (nx = 1): 20 + 20
    two = np.concatenate([rows(6, range(5, 25)), rows(38, range(5, 25)), rows(40, range(5, 8))])
    r = tf.replay(two, two, 64, 64, 5)
    assert [(f.wave, f.sy, f.row, f.parked, f.carried, f.stored) for f in r.flushes] == [(0, 8, 38, 40, 20, 40)]
    assert r.final.tolist() == [3, 0, 0, 0, 0, 0, 0, 0] and r.stored_after_flush == 1
    r = tf.replay(two, two, 16, 64, 9)                                                    # W <= 2 * border: nothing is scanned
    assert r.flushes == [] and r.final.sum() == 0


def test_replay_reaches_the_flush(oracle):
    flush_cases, carried_cases, zero_default, after, later_wg, sx1, big_row = [], [], [], [], [], [], []
    for case in tf.CASES:
        for k, o, r in _replays(oracle, case):
            fl = r.flushes
            print("%-24s octave %d (workgroup %d): %4d extrema, %2d flushes, most parked %2d, %2d with entries carried in, %2d storing nothing, "
                  "longest row %2d, held at the end %r" % (case.name, o, k, len(tf.expectations(oracle, case).raw[o]), len(fl),
                                                            max([f.parked for f in fl], default=0), sum(f.carried > 0 for f in fl),
                                                            sum(f.stored == 0 for f in fl), r.max_row, r.final.tolist()))
            for f in fl:
                assert pc.TAIL_EXT_BUF < f.parked <= pc.TAIL_EXT_BUF + 3 * 62 and f.carried <= pc.TAIL_EXT_BUF       # 218 of the 224 slots
            assert r.final.max() <= pc.TAIL_EXT_BUF
            if k == case.watch:
                if case.flush:
                    assert fl, "%s: octave %d does not flush" % (case.name, o)
                    flush_cases.append(case.name)
                else:                                  # listed for the carry (or the edge test) alone
                    assert not fl and (r.final > 0).any()
            if any(f.carried > 0 for f in fl):
                carried_cases.append(case.name)
            if case.par == "DEFAULT" and any(f.stored == 0 for f in fl):
                zero_default.append(case.name)
            if r.stored_after_flush:
                after.append(case.name)
            if k >= 1 and fl:
                later_wg.append(case.name)
            if any(f.sx == 1 for f in fl):
                sx1.append(case.name)
            if r.max_row > 60:
                big_row.append(case.name)
    assert len(flush_cases) == sum(c.flush for c in tf.CASES) >= 12
    assert len(set(carried_cases)) >= 3, carried_cases
    assert zero_default and "h128_l24_default" in zero_default
    assert after and later_wg and sx1 and big_row, (after, later_wg, sx1, big_row)
    # the case that only carries does so across strips: a wave ends with the ties of more than one strip row
    assert not tf.BY_NAME["h128_l40"].flush


def test_every_stripe_frame_has_no_record_and_compo_frames_have(oracle):
    """refining a ridge is singular and is rejected, in the oracle too; the compo frames give records of tail octaves"""
    ok = []
    for case in tf.CASES:
        exp = tf.expectations(oracle, case)
        if case.split is None:
            assert len(exp.records) == 0, case.name
            continue
        # records carry no octave: the tail's are those that a run limited to the octaves above the tail does not return
        par = tf.oracle_params(oracle, case.par, case.pix_per_kp)
        par.octave_max = pc.tail_first(exp.sizes)
        n_tail = len(exp.records) - len(oracle.keypoints(tf.image(case), par=par))
        print("%s: %d records, %d of tail octaves" % (case.name, len(exp.records), n_tail))
        if n_tail >= 20:
            ok.append(case.name)
    assert ok, "no compo case with at least 20 records of tail octaves"


def test_pix_per_kp_case_overflows_because_of_the_tail(oracle):
    case = tf.BY_NAME["v128_l20_ppk60"]
    exp = tf.expectations(oracle, case)
    kpsize = case.shape[0] * case.shape[1] // case.pix_per_kp
    first = pc.tail_first(exp.sizes)
    assert case.pix_per_kp == 60 and exp.overflow is True
    assert max(int(exp.c_scale[o].sum()) for o in range(first, len(exp.sizes))) > kpsize
    # no other octave can break the rule `oriented so far + candidates of the scale > kpsize`: all of its candidates and every
    # record of the frame together stay below kpsize
    for o in range(first):
        assert int(exp.c_scale[o].sum()) + len(exp.records) <= kpsize
    # the same frame at the default PIX_PER_KP: no overflow
    assert tf.expectations(oracle, tf.BY_NAME["v128_l20"]).overflow is False
