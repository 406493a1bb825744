"""Both forms of the extrema kernel, reached as a stage on crafted planes and compared with the CPU oracle bit for bit.

Detection (k_extrema.hpp) restates the reference where float images never go: `val >= max27` for "no neighbour strictly
greater", `|v| >= nextafter(contrast)` for `(double)|v| > contrast`, fmaxf's NaN rule for comparisons, an edge test kept on
plateaus (det == tr == 0), a refinement whose singular Hessians give inf / NaN steps.  The planes of util.detection_dogs are
made of ties, plateaus, threshold values and non-finite samples, and dense enough that a wave's parking buffer
(SIFT_EXT_BUF) overflows inside a 62 x 4 strip.  siftmi_stage_detect_ex launches what a plan launches -- form 0:
extrema_kernel<false>, then refine_kernel on the device-side list; form 1: extrema_kernel<true> -- with the strip height,
the workgroup order, a band of rows and both list capacities chosen here, and returns the raw counters and the lists with
their unwritten slots visible.

Every expected value comes from the oracle (oracle.local_maxmin per scale, oracle.interp_keypoint), which
tests/test_oracle_vs_ref.py::test_detection_on_crafted_planes_identical ties to the reference's own kernels on these very
families.  There is no tolerance in this module: rows are sorted and compared as uint32.

octave_tail_kernel's use of extrema_strip (its own buffer size, `pending` carried across strips) is not reached from here:
its planes are produced inside the launch.  tests/test_gpu_pyramid_cases.py compares the planes and the candidate counts of the
tail per octave at plan level, on frames where waves carry `pending` from strip to strip; the flush at a full buffer
(pending > SIFT_TAIL_EXT_BUF) stays unreached: no frame parks more than 5 of its 32 slots (tests/test_pyramid_cases_host.py)."""
import ctypes as C

import numpy as np
import pytest

from util import (DETECT_DENSE, DETECT_FAMILIES, SIFT_EXT_BUF, detection_dogs, detection_expected, detection_planes,
                  blurs_from_dogs, refined_expected, sort_rows_bits, strip_candidate_counts)
from test_gpu_edges import extrema_strip_rows

pytestmark = pytest.mark.gpu

EINVAL = -1
GUARD = 64                      # SIFTMI_STAGE_GUARD: slots after each list's capacity that the kernels are not told of
FILL = 0xa5a5a5a5               # fill of the refined lists; the candidate list is filled with -1.0f (holes)
ROWS = (4, 7, 8, 16, 32, 64)
AREA_W = (61, 62, 63, 123, 124, 125)     # W - 2 * border: 62 k - 1, 62 k, 62 k + 1 (a last strip one column wide)
F = np.float32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def params(oracle, border=5, peak=None):
    """(the oracle's parameter block, the library's): the defaults of param.py with another border / peak threshold"""
    from sift_pyocl_amd import _lib
    peak = F(255.0 * 0.04 / 3.0) if peak is None else F(peak)
    opar = oracle.default_params()
    opar.border_dist = border; opar.peak_thresh = peak
    lpar = _lib.Params(init_sigma=1.6, peak_thresh=peak, edge_thresh0=F(0.08), edge_thresh=F(0.06), ori_sigma=F(1.5),
                       border_dist=border, octave_max=0, pix_per_kp=10, double_im_size=0)
    return opar, lpar


class Detected(object):
    """what siftmi_stage_detect_ex returned: the lists whole (capacity + GUARD slots), the five raw counters"""

    def __init__(self, cand, kp, aux, counters, ccap, kcap):
        self.cand, self.kp, self.aux, self.ccap, self.kcap = cand, kp, aux, ccap, kcap
        self.n_cand, self.g_kp = int(counters[0]), int(counters[1])
        self.c_scale = [int(v) for v in counters[2:5]]

    def cand_rows(self):
        """the candidates stored"""
        return self.cand[:min(self.n_cand, self.ccap)]

    def refined_rows(self):
        """the refined rows stored, as (peak, row, col, sigma, scale)"""
        m = min(self.g_kp, self.kcap)
        return np.concatenate([self.kp[:m], (self.aux[:m] & 0xff).astype(np.float32)[:, None]], axis=1)

    def assert_fill_beyond(self, octave):
        """slots no kernel may have written keep their fill; the stored refined rows carry the octave"""
        nc, nk = min(self.n_cand, self.ccap), min(self.g_kp, self.kcap)
        assert (self.cand[nc:] == -1.0).all(), "candidate slots beyond the list were written"
        assert (self.kp[nk:].view(np.uint32) == FILL).all() and (self.aux[nk:].view(np.uint32) == FILL).all(), \
            "refined slots beyond the list were written"
        assert not (self.cand[:nc] == -1.0).all(axis=1).any(), "a reserved candidate slot was not written"
        assert not (self.kp[:nk].view(np.uint32) == FILL).all(axis=1).any(), "a reserved refined slot was not written"
        assert ((self.aux[:nk] >> 8) == octave).all()


def detect(siftlib, blurs, octsize, lpar, form, rows=0, xcd=0, band=(-1, -1), ccap=None, kcap=None, expect=0):
    blurs = np.ascontiguousarray(blurs, np.float32)
    _, H, W = blurs.shape
    most = 3 * max(0, H - 2 * lpar.border_dist) * max(0, W - 2 * lpar.border_dist)       # every sample of the area a candidate
    ccap = most if ccap is None else ccap
    kcap = most if kcap is None else kcap
    cand = np.zeros((ccap + GUARD, 4), np.float32); kp = np.zeros((kcap + GUARD, 4), np.float32)
    aux = np.zeros(kcap + GUARD, np.int32); counters = np.full(5, -7, np.int32)
    rc = siftlib.siftmi_stage_detect_ex(0, _p(blurs), W, H, octsize, C.byref(lpar), form, rows, xcd, band[0], band[1], ccap, kcap,
                                        _p(cand), _p(kp), _p(aux), _p(counters))
    assert rc == expect, "siftmi_stage_detect_ex returned %d" % rc
    return Detected(cand, kp, aux, counters, ccap, kcap) if rc == 0 else None


class Expected(object):
    def __init__(self, oracle, blurs, octsize, opar, band=None):
        self.dogs = oracle.dog(blurs)
        self.cand, self.counts, self.refined = detection_expected(oracle.local_maxmin, oracle.interp_keypoint, self.dogs, octsize,
                                                                  opar, band)


def same_rows(got, want, what):
    got, want = sort_rows_bits(got), sort_rows_bits(want)
    assert len(got) == len(want), "%s: %d rows, expected %d" % (what, len(got), len(want))
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: %d rows differ, first %r vs %r" % (what, bad.size, got[bad[:2]].view(np.float32), want[bad[:2]].view(np.float32))


def check(got, exp, form, what, octave=0):
    """a whole, uncut result against the oracle's"""
    if form == 0:
        assert got.n_cand == len(exp.cand), "%s: n_cand %d, expected %d" % (what, got.n_cand, len(exp.cand))
        same_rows(got.cand_rows(), exp.cand, what + " candidates")
    else:
        assert got.n_cand == 0, what + ": the fused form keeps no candidate list"
    assert got.c_scale == exp.counts, "%s: c_scale %r, expected %r" % (what, got.c_scale, exp.counts)
    assert got.g_kp == len(exp.refined), "%s: g_kp %d, expected %d" % (what, got.g_kp, len(exp.refined))
    same_rows(got.refined_rows(), exp.refined, what + " refined")
    got.assert_fill_beyond(octave)


def assert_dense(family, exp, W, H, border, rows):
    """What a dense case must reach, counted on the host from the oracle's candidates: the fullest strip holds more
    candidates that passed the edge test than a wave parks before it flushes (a lower bound of what it parked), and in an
    all-equal plane every row of a full-width strip adds 3 x 62 entries at once."""
    counts = strip_candidate_counts(exp.cand, W, H, border, rows)
    if family in DETECT_DENSE or (family == "blocks" and rows >= 8):
        assert counts.max() > SIFT_EXT_BUF, "%s, %d-row strips: fullest strip holds %d" % (family, rows, counts.max())
    if family.startswith("equal"):
        nx = (W - 2 * border + 61) // 62
        per_row = np.zeros((H, nx), np.int64)
        np.add.at(per_row, (exp.cand[:, 1].astype(np.int64), (exp.cand[:, 2].astype(np.int64) - border) // 62), 1)
        width = np.minimum(62, W - 2 * border - 62 * np.arange(nx))
        assert (per_row[border:H - border] == 3 * width).all() and (W - 2 * border < 62 or 3 * width[0] == 186)


def geometry_cases():
    """(family, form, rows, xcd_map, H, W): every family x both forms, paired with the other axes so that every strip
    height, workgroup order, width class (W - 2 * border = 62 k - 1, 62 k, 62 k + 1) and strip-count residue
    (nx * ny % 4 = 1, 2, 3: inactive waves in the last workgroup) occurs with each form; H - 2 * border = rows * k + 1."""
    cases = []
    for i, family in enumerate(DETECT_FAMILIES):
        for form in (0, 1):
            rows = ROWS[(i + 3 * form) % 6]
            aw = AREA_W[(i + 2 * form + i // 6) % 6]
            nx = (aw + 61) // 62
            residue = 2 if nx == 2 else (1, 3)[(i // 2 + form) % 2]      # (two strips across: the count is even)
            k = next(k for k in range(max(1, 24 // rows), 200) if (nx * (k + 1)) % 4 == residue)
            cases.append((family, form, rows, (i + form + i // 2) % 2, rows * k + 1 + 10, aw + 10))
    return cases


def test_case_list_pairs_every_axis_with_each_form():
    """(no GPU needed, but kept with the module: it guards the list the GPU cases are drawn from)"""
    cases = geometry_cases()
    for form in (0, 1):
        mine = [c for c in cases if c[1] == form]
        assert {c[0] for c in mine} == set(DETECT_FAMILIES)
        assert {c[2] for c in mine} == set(ROWS) and {c[3] for c in mine} == {0, 1}
        assert {c[5] - 10 for c in mine} == set(AREA_W)
        residues = {(((c[5] - 10 + 61) // 62) * ((c[4] - 10 + c[2] - 1) // c[2])) % 4 for c in mine}
        assert {1, 2, 3} <= residues
        assert all((c[4] - 10) % c[2] == 1 for c in mine)            # a last strip one row high


@pytest.mark.parametrize("family,form,rows,xcd,H,W", geometry_cases())
def test_family_form_geometry(siftlib, oracle, family, form, rows, xcd, H, W):
    opar, lpar = params(oracle)
    blurs = detection_planes(family, (H, W), seed=7)
    exp = Expected(oracle, blurs, 1, opar)
    assert len(exp.cand) > 0, "the oracle finds no candidate in family %s" % family
    assert_dense(family, exp, W, H, 5, rows)
    check(detect(siftlib, blurs, 1, lpar, form, rows, xcd), exp, form, "%s form %d rows %d xcd %d %dx%d" % (family, form, rows, xcd, H, W))


@pytest.mark.parametrize("family", DETECT_DENSE + ("blocks",))
def test_dense_families_at_every_strip_height(siftlib, oracle, family):
    """The families that overflow the parking buffer, at every strip height in both forms: one oracle result, 12 launches."""
    H, W = 139, 135                          # 125 x 129: three strips across (the last one column wide), a last row of its own
    opar, lpar = params(oracle)
    blurs = detection_planes(family, (H, W), seed=11)
    exp = Expected(oracle, blurs, 1, opar)
    for rows in ROWS:
        assert_dense(family, exp, W, H, 5, rows)
        for form in (0, 1):
            check(detect(siftlib, blurs, 1, lpar, form, rows, (rows // 4 + form) % 2), exp, form, "%s form %d rows %d" % (family, form, rows))


@pytest.mark.parametrize("family,form", [("iid", 1), ("spikes", 0)])
def test_default_rule_on_a_large_plane(siftlib, oracle, family, form):
    """1400 x 1100: the size rule picks 8-row strips (rows = 0), 3151 strips, both workgroup orders."""
    H, W = 1100, 1400
    assert extrema_strip_rows(W, H) == 8
    opar, lpar = params(oracle)
    blurs = detection_planes(family, (H, W), seed=13)
    exp = Expected(oracle, blurs, 1, opar)
    assert len(exp.cand) > 50000
    for xcd in (1, 0):
        check(detect(siftlib, blurs, 1, lpar, form, 0, xcd, ccap=len(exp.cand) + 1000, kcap=len(exp.cand) + 1000), exp, form, "%s 1400x1100 form %d xcd %d" % (family, form, xcd))


@pytest.mark.parametrize("form", [0, 1])
def test_tiny_and_empty_detection_areas(siftlib, oracle, form):
    """A detection area of one pixel (11 x 11), of 2 x 3 pixels (12 x 13), and none (W or H <= 2 * border: no launch, zero
    counters, nothing written)."""
    opar, lpar = params(oracle)
    found = 0
    for family, (H, W), seed in [("equal+", (11, 11), 0), ("equal-", (11, 11), 0), ("equal-", (12, 13), 0), ("iid", (12, 13), 1),
                                 ("iid", (12, 13), 2), ("iid", (11, 11), 3), ("iid", (11, 11), 4), ("spikes", (12, 13), 5)]:
        blurs = detection_planes(family, (H, W), seed=seed)
        exp = Expected(oracle, blurs, 1, opar)
        if family.startswith("equal"):
            assert len(exp.cand) == 3 * (H - 10) * (W - 10)
        found += len(exp.cand)
        for rows in (0, 4, 64):
            check(detect(siftlib, blurs, 1, lpar, form, rows, rows == 4), exp, form, "%s %dx%d rows %d" % (family, H, W, rows))
    assert found > 24
    for (H, W) in [(10, 40), (40, 10), (9, 9), (5, 200), (10, 10)]:
        got = detect(siftlib, detection_planes("equal+", (H, W)), 1, lpar, form, 0, 1)
        assert (got.n_cand, got.g_kp, got.c_scale) == (0, 0, [0, 0, 0])
        got.assert_fill_beyond(0)


@pytest.mark.parametrize("octsize", [1, 2])
def test_both_edge_thresholds(siftlib, oracle, octsize):
    """octsize 1 uses edge_thresh0, larger octaves edge_thresh (image.cl:193): ridges that one keeps and the other drops."""
    opar, lpar = params(oracle)
    H, W = 143, 197
    kept = {}
    for family in ("waves", "iid", "blocks"):
        blurs = detection_planes(family, (H, W), seed=17)
        exp = Expected(oracle, blurs, octsize, opar)
        kept[family] = len(exp.cand)
        for form in (0, 1):
            check(detect(siftlib, blurs, octsize, lpar, form, 16 if form else 4, form), exp, form, "%s octsize %d form %d" % (family, octsize, form),
                  octave=octsize - 1)
    other = Expected(oracle, detection_planes("waves", (H, W), seed=17), 3 - octsize, opar)
    assert kept["waves"] != len(other.cand), "the two edge thresholds keep the same ridges: the waves test nothing"


@pytest.mark.parametrize("border", [1, 2, 5, 9])
def test_border_dist(siftlib, oracle, border):
    """border_dist 1: candidates in row / column 1, whose 3 x 3 x 3 neighbourhood and refinement touch the plane's edge."""
    opar, lpar = params(oracle, border=border)
    for family, (H, W) in (("iid", (70 + 2 * border, 63 + 2 * border)), ("levels", (33 + 2 * border, 124 + 2 * border)),
                           ("mixed", (57, 90))):
        blurs = detection_planes(family, (H, W), seed=19)
        exp = Expected(oracle, blurs, 1, opar)
        assert exp.cand[:, 1].min() == border and exp.cand[:, 2].min() == border
        assert exp.cand[:, 1].max() == H - border - 1 and exp.cand[:, 2].max() == W - border - 1
        for form in (0, 1):
            check(detect(siftlib, blurs, 1, lpar, form, (7, 32)[form], form), exp, form, "%s border %d form %d" % (family, border, form))


def test_contrast_threshold_on_a_level(siftlib, oracle):
    """The kernel tests |v| >= cf, cf the smallest float above 0.8 * (double)peak_thresh, for the reference's
    (double)|v| > 0.8 * peak_thresh (image.cl:152).  peak_thresh is chosen so that the contrast in double lies just below,
    exactly on and just above the level 2.75 of the `levels` planes; the oracle says what is kept."""
    level = 2.75
    on = F(level / 0.8)
    assert 0.8 * float(on) == level
    below, above = np.nextafter(on, F(0)), np.nextafter(on, F(10))
    assert 0.8 * float(below) < level < 0.8 * float(above)
    blurs = detection_planes("levels", (81, 135), seed=23)
    n = {}
    for name, peak in (("below", below), ("on", on), ("above", above)):
        opar, lpar = params(oracle, peak=peak)
        exp = Expected(oracle, blurs, 1, opar)
        n[name] = len(exp.cand)
        for form in (0, 1):
            check(detect(siftlib, blurs, 1, lpar, form, 8, form), exp, form, "contrast %s the level, form %d" % (name, form))
    assert n["below"] > n["on"] == n["above"] > 0, n       # (double)2.75 > 2.75 is false: on the level means rejected


def distinct_members(rows, want, what):
    """every stored row is one of `want`, none more often than there (two candidates may refine to the same row)"""
    from collections import Counter
    have = Counter(r.tobytes() for r in sort_rows_bits(want))
    for row, n in Counter(r.tobytes() for r in sort_rows_bits(rows)).items():
        assert row in have, "%s: stored row %r is not one of the oracle's" % (what, np.frombuffer(row, np.float32))
        assert n <= have[row], "%s: row %r stored %d times, expected %d" % (what, np.frombuffer(row, np.float32), n, have[row])


def test_candidate_list_cut_at_its_capacity(siftlib, oracle):
    """Form 0 with a candidate capacity of 0, 1, 127 and n - 1: n_cand still reports n, the rows stored are distinct
    candidates of the oracle's set, nothing is written beyond the capacity, and the refinement launch works on exactly the
    rows that were stored: g_kp, c_scale and the refined rows are the oracle's for those rows."""
    opar, lpar = params(oracle)
    H, W = 75, 135
    blurs = detection_planes("iid", (H, W), seed=29)
    exp = Expected(oracle, blurs, 1, opar)
    n = len(exp.cand)
    assert n > 1000
    for ccap in (0, 1, 127, n - 1, n):
        got = detect(siftlib, blurs, 1, lpar, 0, 4, ccap & 1, ccap=ccap)
        what = "candidate capacity %d of %d" % (ccap, n)
        assert got.n_cand == n, what
        stored = got.cand_rows()
        assert len(stored) == min(ccap, n)
        distinct_members(stored, exp.cand, what)
        want = refined_expected(oracle.interp_keypoint, exp.dogs, stored, opar)
        assert got.c_scale == [int((stored[:, 3] == s).sum()) for s in (1, 2, 3)], what
        assert got.g_kp == len(want), what
        same_rows(got.refined_rows(), want, what)
        got.assert_fill_beyond(0)


@pytest.mark.parametrize("form", [0, 1])
def test_keypoint_list_cut_at_its_capacity(siftlib, oracle, form):
    """A refined-list capacity of 0, 1, 127 and m - 1: g_kp still reports m and c_scale every candidate, the rows stored are
    distinct members of the oracle's set, nothing is written beyond the capacity."""
    opar, lpar = params(oracle)
    H, W = 75, 135
    blurs = detection_planes("iid", (H, W), seed=31)
    exp = Expected(oracle, blurs, 1, opar)
    m = len(exp.refined)
    assert m > 1000
    for kcap in (0, 1, 127, m - 1, m):
        got = detect(siftlib, blurs, 1, lpar, form, 8, kcap & 1, kcap=kcap)
        what = "keypoint capacity %d of %d, form %d" % (kcap, m, form)
        assert got.g_kp == m and got.c_scale == exp.counts, what
        assert got.n_cand == (len(exp.cand) if form == 0 else 0), what
        stored = got.refined_rows()
        assert len(stored) == min(kcap, m)
        distinct_members(stored, exp.refined, what)
        got.assert_fill_beyond(0)


@pytest.mark.parametrize("form", [0, 1])
def test_bands_add_up_to_the_whole_area(siftlib, oracle, form):
    """The band arguments (rows [y_lo, y_hi) of the detection area): each band returns exactly the oracle's candidates of its
    rows -- an extremum on a band's first or last row looks at the rows outside it -- and two or three bands together the
    whole result."""
    opar, lpar = params(oracle)
    H, W = 111, 140
    for family in ("iid", "blocks"):
        blurs = detection_planes(family, (H, W), seed=37)
        whole = Expected(oracle, blurs, 1, opar)
        for cuts in ((5, 52, 106), (5, 6, 70, 106), (5, 37, 105, 106)):
            cand, refined = [], []
            for y_lo, y_hi in zip(cuts[:-1], cuts[1:]):
                exp = Expected(oracle, blurs, 1, opar, band=(y_lo, y_hi))
                got = detect(siftlib, blurs, 1, lpar, form, (16, 7)[form], y_lo & 1, band=(y_lo, y_hi))
                check(got, exp, form, "%s band [%d, %d) form %d" % (family, y_lo, y_hi, form))
                cand.append(got.cand_rows()); refined.append(got.refined_rows())
            if form == 0:
                same_rows(np.concatenate(cand), whole.cand, "bands %r together" % (cuts,))
            same_rows(np.concatenate(refined), whole.refined, "bands %r together" % (cuts,))
    # a band outside the detection area, an empty band, an unknown form, a border without a neighbourhood: refused, nothing launched
    blurs = detection_planes("iid", (40, 40))
    for kw in (dict(band=(4, 20)), dict(band=(5, 36)), dict(band=(20, 20)), dict(band=(30, 20)), dict(rows=-1)):
        detect(siftlib, blurs, 1, lpar, form, expect=EINVAL, **kw)
    detect(siftlib, blurs, 1, lpar, 2, expect=EINVAL)
    detect(siftlib, blurs, 3, lpar, form, expect=EINVAL)
    detect(siftlib, blurs, 1, params(oracle, border=0)[1], form, expect=EINVAL)


# ------------------------------------------------------------------------------------------ refine_kernel on crafted lists
def interp(siftlib, blurs, cand, lpar):
    _, H, W = blurs.shape
    cand = np.ascontiguousarray(cand, np.float32)
    n = len(cand)
    out = np.empty((max(n, 1), 4), np.float32); sc = np.empty(max(n, 1), np.int32)
    m = C.c_int64(-1)
    assert siftlib.siftmi_stage_interp(0, _p(blurs), W, H, _p(cand), n, C.byref(lpar), _p(out), _p(sc), C.byref(m)) == 0
    return np.concatenate([out[:m.value], sc[:m.value, None].astype(np.float32)], axis=1)


def ramp_planes(H, W, seed):
    """DoG planes whose gradient pushes a refinement outward from the centre for as long as it may move: a steep ramp away
    from the middle row and column in the candidate's plane plus small integer noise (so that the Hessians are regular)."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    ramp = 3 * np.abs(y - H // 2) + 3 * np.abs(x - W // 2)
    d = rng.integers(-2, 3, (5, H, W)) + ramp[None] - np.array([0, 1, 0, 1, 0])[:, None, None] * (rng.integers(0, 2, (H, W)))[None]
    return blurs_from_dogs(np.ascontiguousarray(d, np.float32))


def test_refinement_on_crafted_candidate_lists(siftlib, oracle):
    """refine_kernel alone: candidates on and next to the rows / columns where a move is refused (3 and H - 3), on planes
    that push them outward, lists with `r == -1` holes, and list lengths around a wave (1, 63, 64, 65) and far beyond the
    grid (100 000: the grid stride)."""
    opar, lpar = params(oracle)
    H, W = 41, 53
    edge_r, edge_c = (1, 2, 3, H - 4, H - 3, H - 2), (1, 2, 3, W - 4, W - 3, W - 2)
    moved = limit = 0
    for seed, maker in ((41, ramp_planes), (42, lambda h, w, s: detection_planes("iid", (h, w), s)),
                        (43, lambda h, w, s: detection_planes("blocks", (h, w), s))):
        blurs = maker(H, W, seed)
        dogs = oracle.dog(blurs)
        rows = [(dogs[s, r, c], r, c, s) for s in (1, 2, 3) for r in edge_r for c in list(edge_c) + [W // 2, 20]]
        rows += [(dogs[s, r, c], r, c, s) for s in (1, 2, 3) for c in edge_c for r in (H // 2, 17)]
        cand = np.array(rows, np.float32)
        cand[5::11, 1] = -1.0                                    # holes, as compaction leaves them in the reference's list
        want = refined_expected(oracle.interp_keypoint, dogs, cand, opar)
        same_rows(interp(siftlib, blurs, cand, lpar), want, "edge candidates, planes %d" % seed)
        full = oracle.interp_keypoint(dogs, cand, 0, len(cand), opar)
        ok = (cand[:, 1] != -1) & (full[:, 1] != -1)
        moved += int((np.abs(full[ok, 1] - cand[ok, 1]) > 1.5).sum() + (np.abs(full[ok, 2] - cand[ok, 2]) > 1.5).sum())
        limit += int((np.rint(full[ok, 1]) <= 3).sum() + (np.rint(full[ok, 1]) >= H - 4).sum())
    assert moved > 0 and limit > 0, "no candidate moved to a limit: the planes test nothing"
    # list lengths: every candidate of a dense plane, repeated up to the length asked for, holes sprinkled in
    blurs = detection_planes("iid", (H, W), seed=44)
    dogs = oracle.dog(blurs)
    base = detection_expected(oracle.local_maxmin, oracle.interp_keypoint, dogs, 1, opar)[0]
    assert len(base) > 500
    for n in (1, 63, 64, 65, 100000):
        cand = np.ascontiguousarray(np.resize(base, (n, 4)))
        if n > 2:
            cand[2::7, 1] = -1.0
        want = refined_expected(oracle.interp_keypoint, dogs, cand, opar)
        assert n < 100 or len(want) > n // 2
        same_rows(interp(siftlib, blurs, cand, lpar), want, "list of %d" % n)
