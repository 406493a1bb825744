"""Crafted plane sets for the lazy detection chain (siftmi_stage_detect_lazy: extrema without plane 5 -> top_patch_kernel ->
refinement), and what the oracle makes of them.

A case is five blur planes 0..4; plane 5 is never given: it is the oracle's blur of plane 4 with the top plane's taps, so
DoG4 = p4 - blur(p4) consists of arbitrary float32 values.  Planes 0..3 are built downwards from plane 4 by adding DoG planes
of small integers (p[s] = p[s + 1] + dog[s]: every sum and every subtraction p[s] - p[s + 1] is exact), so detection sees
DoG0..3 as generated.  A planted DoG3 centre that has to equal a DoG4 value (or lie one ulp beside it) sits on a pixel where
plane 4 is 0, so that p3 - p4 returns it exactly.

Expected values come from the oracle alone: Expect.cand are oracle.local_maxmin's candidates of the six planes, Expect.prov3
the provisional scale-3 candidates -- local_maxmin on DoG planes whose DoG4 is a copy of DoG3, under which the 27-neighbour
test is the 18-neighbour test of DoG2 / DoG3 -- and Expect.refined oracle.interp_keypoint's rows."""
import collections
import math

import numpy as np

from util import detection_expected, strip_candidate_counts, SIFT_EXT_BUF

F = np.float32
R = 6                            # k_top_patch.hpp: SIFT_TOP_R, the patch is (2 R + 1)^2
FILL = 0x7fc5a5a5                # SIFTMI_STAGE_TOP_FILL: plane 5 before the launches
AREA_W = (61, 62, 63, 123, 124, 125)   # W - 2 * border: 62 k - 1, 62 k, 62 k + 1

Case = collections.namedtuple("Case", "name blurs5 border sites")
Expect = collections.namedtuple("Expect", "blurs dogs cand counts prov3 kept3 refined")


def top_taps(oracle):
    """taps of the blur from plane 4 to plane 5 under the default parameters (27 of them)"""
    ratio = 2.0 ** (1.0 / 3.0)
    inc = 1.6 * ratio ** 4 * math.sqrt(ratio ** 2 - 1.0)
    size = int(math.ceil(8 * inc + 1)); size += (size % 2 == 0)
    return oracle.gaussian_taps(inc, size)


def planes_down(p4, d):
    """planes 0..4 from plane 4 and DoG0..3"""
    out = [p4]
    with np.errstate(invalid="ignore"):
        for s in range(3, -1, -1):
            out.insert(0, (out[0] + d[s]).astype(F))
    return out


def ulp_sites(H, W, border):
    """six pixels on the middle row, 7 apart: (y, x, sign, kind); kind 0 the centre equals DoG4's 3 x 3 extreme, 1 it lies one ulp
    inside it (rejected), 2 one ulp beyond it (kept)"""
    return [(H // 2, border + 8 + 7 * i, 1 if i < 3 else -1, i % 3) for i in range(6)]


def rim_sites(H, W, border):
    """the four corners of the detection area and a pixel on each of its edges"""
    lo, yh, xh = border, H - 1 - border, W - 1 - border
    return [(lo, lo), (lo, xh), (yh, lo), (yh, xh), (lo, W // 2), (yh, W // 2), (H // 2 + 9, lo), (H // 2 + 9, xh)]


def build(oracle, name, shape, border, seed=0):
    """Case `name` on a plane of `shape`:
    planted     iid integers; six centres on DoG4's 3 x 3 extreme and one ulp to either side of it (maxima and minima), a large
                DoG3 value on every corner and edge of the detection area
    nonfinite   iid integers with +inf, -inf and NaN in plane 4, whose blur spreads them over 27 x 27 samples of DoG4 (as
                -inf, +inf, NaN) while DoG3 sees them at the one pixel only
    none        DoG3 = 0: no scale-3 candidate
    rejected    DoG3 in {0, 4} over a +-32 checkerboard in plane 4: DoG4 holds about +16 in every 3 x 3
    dense       DoG0..3 = 4 everywhere: every sample a candidate of scales 1 and 2 and a provisional one of scale 3"""
    rng = np.random.default_rng(7000 + seed)
    H, W = shape
    d = rng.integers(-4, 5, (4, H, W)).astype(F)
    p4 = rng.integers(-4, 5, (H, W)).astype(F)
    sites = []
    taps = top_taps(oracle)
    if name == "planted":
        sites = ulp_sites(H, W, border)
        for (y, x, sign, kind) in sites:
            p4[y - 1:y + 2, x - 1:x + 2] = 0
            p4[y, x + 1] = 8 * sign
        for (y, x) in rim_sites(H, W, border):
            d[3][y, x] = 32
    elif name == "nonfinite":
        sites = [(H // 4, W // 4, np.inf), (H // 4, 3 * W // 4, -np.inf), (3 * H // 4, W // 2, np.nan)]
        for (y, x, v) in sites:
            p4[y, x] = v
    elif name == "none":
        d[3][:] = 0
    elif name == "rejected":
        yy, xx = np.mgrid[0:H, 0:W]
        p4 = (32 * ((yy + xx) & 1)).astype(F)
        d[3] = 4 * rng.integers(0, 2, (H, W)).astype(F)
    elif name == "dense":
        d[:] = 4
    else:
        raise ValueError(name)
    planes = planes_down(p4, d)
    if name == "planted":
        p5 = oracle.blur(p4, taps)
        d4 = p4 - p5                                       # one IEEE subtraction, as combine() and the kernels take it
        for (y, x, sign, kind) in sites:
            box = d4[y - 1:y + 2, x - 1:x + 2]
            ext = box.max() if sign > 0 else box.min()
            v = ext if kind == 0 else np.nextafter(ext, F(-sign * np.inf) if kind == 1 else F(sign * np.inf))
            planes[3][y, x] = v                            # p4 is 0 here: p3 - p4 == v
            planes[2][y, x] = 0                            # DoG2 = -v; planes 1 and 0 follow from it exactly
            planes[1][y, x] = planes[2][y, x] + d[1][y, x]
            planes[0][y, x] = planes[1][y, x] + d[0][y, x]
    if name == "nonfinite":
        for (y, x, v) in sites:                            # DoG3 = 0 - p4 at the pixel; DoG0..2 stay as generated
            planes[3][y, x] = 0
            planes[2][y, x] = d[2][y, x]
            planes[1][y, x] = planes[2][y, x] + d[1][y, x]
            planes[0][y, x] = planes[1][y, x] + d[0][y, x]
    return Case(name, np.ascontiguousarray(np.stack(planes), F), border, sites)


_CACHE = {}


def expect(oracle, case, opar, key=None):
    """What the oracle makes of a case (computed once per `key`; read-only)."""
    if key is not None and key in _CACHE:
        return _CACHE[key]
    p5 = oracle.blur(case.blurs5[4], top_taps(oracle))
    blurs = np.ascontiguousarray(np.concatenate([case.blurs5, p5[None]]), F)
    dogs = oracle.dog(blurs)
    cand, counts, refined = detection_expected(oracle.local_maxmin, oracle.interp_keypoint, dogs, 1, opar)
    _, H, W = dogs.shape
    d18 = dogs.copy(); d18[4] = d18[3]
    k, n = oracle.local_maxmin(d18, 3, 1, H * W, opar)
    prov3 = k[:n]
    kept3 = cand[cand[:, 3] == 3]
    for a in (blurs, dogs, cand, prov3, kept3, refined):
        a.setflags(write=False)
    e = Expect(blurs, dogs, cand, counts, prov3, kept3, refined)
    if key is not None:
        _CACHE[key] = e
    return e


def at(rows, y, x):
    """is there a row (value, y, x, scale) at pixel (y, x)"""
    return bool(((rows[:, 1] == y) & (rows[:, 2] == x)).any())


def box4(e, row):
    """DoG4's 3 x 3 around a candidate row"""
    y, x = int(row[1]), int(row[2])
    return e.dogs[4][y - 1:y + 2, x - 1:x + 2]


def patch_mask(prov3, H, W):
    """samples of plane 5 that top_patch_kernel writes: the 13 x 13 patches of the provisional candidates, clipped"""
    m = np.zeros((H, W), bool)
    for row in prov3:
        y, x = int(row[1]), int(row[2])
        m[max(0, y - R):y + R + 1, max(0, x - R):x + R + 1] = True
    return m


def assert_named(case, e):
    """A case contains what it is named for, counted from the oracle's results."""
    _, H, W = e.dogs.shape
    b = case.border
    rejected = [r for r in e.prov3 if not at(e.kept3, r[1], r[2])]
    assert len(e.kept3) + len(rejected) == len(e.prov3), "a kept scale-3 candidate is not provisional"
    if case.name == "planted":
        for (y, x, sign, kind) in case.sites:
            assert at(e.prov3, y, x), "site (%d, %d) is no provisional candidate" % (y, x)
            v = e.dogs[3][y, x]
            box = e.dogs[4][y - 1:y + 2, x - 1:x + 2]
            ext = box.max() if sign > 0 else box.min()
            assert (v > 0) == (sign > 0)
            if kind == 0:
                assert v == ext and at(e.kept3, y, x)
            elif kind == 1:
                assert np.nextafter(v, F(sign * np.inf)) == ext and not at(e.kept3, y, x)
            else:
                assert np.nextafter(v, F(-sign * np.inf)) == ext and at(e.kept3, y, x)
        for (y, x) in rim_sites(H, W, b):
            assert at(e.prov3, y, x), "rim site (%d, %d) is no provisional candidate" % (y, x)
        for sign in (1, -1):
            assert any(np.sign(r[0]) == sign for r in rejected) and any(np.sign(r[0]) == sign for r in e.kept3)
        yx = e.prov3[:, 1:3]
        near = np.abs(yx[:, None, :] - yx[None, :, :]).max(axis=2)
        near[np.arange(len(yx)), np.arange(len(yx))] = 99
        assert near.min() < 2 * R + 1, "no two patches overlap"
    elif case.name == "nonfinite":
        seen = {"nan": 0, "+inf": 0, "-inf": 0}
        for r in e.prov3:
            y, x = int(r[1]), int(r[2])
            if not (np.isfinite(e.dogs[2][y - 1:y + 2, x - 1:x + 2]).all() and np.isfinite(e.dogs[3][y - 1:y + 2, x - 1:x + 2]).all()):
                continue
            box = box4(e, r)
            seen["nan"] += bool(np.isnan(box).any() and np.isfinite(box).any())       # a 3 x 3 on the rim of a NaN footprint
            seen["+inf"] += bool((box == np.inf).any())
            seen["-inf"] += bool((box == -np.inf).any())
        assert min(seen.values()) > 0, seen
    elif case.name == "none":
        assert len(e.prov3) == 0 and len(e.cand) > 0
    elif case.name == "rejected":
        assert len(e.prov3) > 100 and len(e.kept3) == 0
    elif case.name == "dense":
        assert len(e.prov3) == (H - 2 * b) * (W - 2 * b)
        listed = np.concatenate([e.cand[e.cand[:, 3] != 3], e.prov3])
        assert strip_candidate_counts(listed, W, H, b, 4).max() > SIFT_EXT_BUF
