"""CPU test: every family of tests/keypoint_cases.py reaches the rule it was made for.

Conditions on the INPUTS of tests/test_gpu_keypoint_cases.py, checked with the oracle and the numpy predicates of
keypoint_cases alone: without them a later edit of a family could leave the GPU test green and vacuous.  Every condition
is "at least one", with a small floor where the construction gives many; the figures are printed."""
import ctypes as C

import numpy as np
import pytest

import keypoint_cases as kc
from keypoint_cases import F, PI_F, TWO_PI_F


@pytest.fixture(scope="module")
def maps(oracle):
    """family -> (blur stack, [(magnitude, orientation) of the oracle for planes 0..5])"""
    cache = {}

    def get(family, shape=kc.SHAPE):
        if (family, shape) not in cache:
            blurs = kc.blur_stack(family, shape)
            cache[family, shape] = (blurs, [oracle.gradient(p) for p in blurs])
        return cache[family, shape]
    return get


def _sincos(oracle):
    def f(a):
        s, c = C.c_float(), C.c_float()
        oracle.lib().so_sincosf(C.c_float(a), C.byref(s), C.byref(c))
        return s.value, c.value
    return f


def _orient_one(oracle, k, g, o, octsize=1, ori_sigma=1.5):
    """(main angle, [further angles]) of one refined keypoint"""
    buf = np.full((40, 4), -1, F); buf[0] = k
    par = oracle.default_params(); par.ori_sigma = F(ori_sigma)
    rows, cnt = oracle.orientation(buf, g, o, octsize, 0, 1, capacity=40, par=par)
    return rows[0, 3], [a for a in rows[1:cnt, 3]]


def _orient_all(oracle, family, maps, ori_sigma=1.5):
    blurs, gm = maps(family)
    kps, ss = kc.orientation_keypoints(family)
    return [(k, s) + _orient_one(oracle, k, gm[s][0], gm[s][1], 1, ori_sigma) for k, s in zip(kps, ss) if k[1] >= 0]


def test_lists_are_deterministic_and_within_the_limits():
    for shape in (kc.SHAPE, kc.ODD_SHAPE):
        for family in kc.FAMILIES:
            a, b = kc.blur_stack(family, shape), kc.blur_stack(family, shape)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
            k1, s1 = kc.orientation_keypoints(family, shape)          # (the limits are asserted inside)
            k2, s2 = kc.orientation_keypoints(family, shape)
            assert np.array_equal(k1.view(np.uint32), k2.view(np.uint32)) and np.array_equal(s1, s2)
            assert 100 <= len(k1) <= 500 and (k1[:, 1] == -1).sum() >= 5
            H, W = shape
            assert ((k1[:, 1] == H - 2) & (k1[:, 2] == W - 2)).any() and (k1[:, 1] == kc.HALF_BELOW).any() and (k1[:, 2] == kc.HALF_BELOW).any()
            for octsize in (1, 2):
                kk, ks = kc.descriptor_keypoints(family, octsize, shape)
                assert 100 <= len(kk) <= 2500 and (kk[:, 1] < 0).sum() >= 5
                R = np.array([kc.desc_radius(k[2], octsize)[0] for k in kk])
                assert R.min() == 0 and R.max() <= 40


def test_numpy_gradient_is_the_oracles_on_the_exact_families(oracle, maps):
    """gradient_np picks the keypoint angles that wrap a plane's own orientations: on these families its arctan2 values are
    exact cases, equal to the oracle's bit for bit"""
    for family in ("ramps", "ramps_neg", "step", "bump", "bumps", "constant", "checker", "ori_plus_pi"):
        blurs, gm = maps(family)
        for s in (1, 2, 3):
            _, _, mag, ori = kc.gradient_np(blurs[s])
            assert np.array_equal(mag.view(np.uint32), gm[s][0].view(np.uint32)), (family, s)
            assert np.array_equal(ori.view(np.uint32), gm[s][1].view(np.uint32)), (family, s)


def test_orientations_on_the_bin_edges(oracle, maps):
    """-pi lands in bin 0, +pi_f in bin 36 (clamped to 35); -0, +-pi/2, +-pi/4, +-3pi/4 occur exactly"""
    pi = PI_F
    seen = {}
    for family, s, value in [("ramps", 1, F(-0.0)), ("ramps", 2, pi / F(2)), ("ramps", 3, pi / F(4)), ("ramps_neg", 1, -pi),
                             ("ramps_neg", 2, -pi / F(4)), ("ramps_neg", 3, F(-3) * pi / F(4)), ("ori_plus_pi", 1, pi)]:
        g, o = maps(family)[1][s]
        n = int(((o.view(np.uint32) == value.view(np.uint32)) & (g > 0)).sum())
        seen[family, s] = n
        assert n >= kc.SHAPE[0], (family, s, value, n)
    votes = {}
    for family, s, edge_bin in [("ramps_neg", 1, 0), ("ori_plus_pi", 1, 36), ("ori_plus_pi", 3, 36), ("small", 1, 0)]:
        g, o = maps(family)[1][s]
        kps, ss = kc.orientation_keypoints(family)
        n = sum(int((kc.ori_votes(k, g, o, 1.5) == edge_bin).sum()) for k in kps[(ss == s) & (kps[:, 1] >= 0)])
        votes[family, s, edge_bin] = n
        assert n >= 50, (family, s, edge_bin, n)
    g, o = maps("small")[1][1]
    assert ((o == 0) & np.signbit(o) & (g > 0)).any() and ((o == 0) & ~np.signbit(o) & (g > 0)).any() and (o == pi).any() and (o == -pi).any()
    print("pixels on an edge value:", seen, "votes in the edge bins:", votes)


def test_exact_peak_ties(oracle, maps):
    """a single-pixel bump: four equidistant gradient pixels, four equal votes a quarter turn apart -- a main angle (the
    first index wins argmax) and further peaks that pass `h >= 0.8f * maxval` with equality, all at exact bin centres"""
    main_c, extra_c = kc.bin_centre_angles()
    tied = 0
    for k, s, main, extras in _orient_all(oracle, "bump", maps):
        if len(extras) >= 2 and (main_c.view(np.uint32) == main.view(np.uint32)).any() and all((extra_c.view(np.uint32) == e.view(np.uint32)).any() for e in extras):
            tied += 1
    print("keypoints with a main angle and >= 2 further ones at exact bin centres:", tied)
    assert tied >= 3


def test_peaks_either_side_of_the_threshold(oracle, maps):
    """`bumps`: the second peak is 0.8 * the first give or take the rounding of the six smoothing passes; over the sweep of
    the second bump's height, ulp by ulp, the further orientation appears"""
    blurs, gm = maps("bumps")
    has = {}
    for r, c, step in kc.bumps_sites(kc.SHAPE):
        k = np.array([12.0, r, c, kc.BUMPS_SIGMA], F)
        assert kc.ori_window(k, 1.5) == (r, c, 1)
        main, extras = _orient_one(oracle, k, gm[1][0], gm[1][1])
        assert np.isfinite(main) and len(extras) <= 1
        has[step] = len(extras)
    steps = sorted(has)
    flips = [(a, b) for a, b in zip(steps, steps[1:]) if has[a] != has[b]]
    print("further orientation per step of the second bump:", [has[s] for s in steps], "flips at", flips)
    assert len(flips) >= 1 and has[steps[0]] == 0 and has[steps[-1]] == 1


def test_empty_and_infinite_histograms(oracle, maps):
    """constant planes, planes whose gradient squares underflow: maxval == 0, interp is 0 / 0, the main angle NaN, no further
    peak; +-3e38 planes and the inf pixel: infinite votes, inf - inf in the interpolation"""
    figures = {}
    for family, floor in (("constant", None), ("huge", 20), ("nanpix", 5), ("tiny", 5)):
        res = _orient_all(oracle, family, maps)
        nan_main = [r for r in res if np.isnan(r[2])]
        figures[family] = (len(nan_main), len(res))
        if family == "constant":
            assert len(nan_main) == len(res) and all(len(r[3]) == 0 for r in res)
        else:
            assert len(nan_main) >= floor, (family, figures[family])
        if family in ("nanpix", "tiny"):
            assert len(nan_main) < len(res)
    g, o = maps("huge")[1][1]
    # infinite gradients with an ordinary angle (finite differences whose squares overflow: they vote) and with a NaN one
    # (infinite differences: the oracle's atan2 of an infinite argument is NaN, (int)NaN fails `bin >= 0`, no vote)
    assert (np.isinf(g) & np.isfinite(o)).sum() >= 1000 and (np.isinf(g) & np.isnan(o)).sum() >= 1000
    print("keypoints with a NaN main angle (of):", figures)


def test_double_against_float_rounding():
    """keypoints whose window the float-only rules (k.s1 + 0.5f, sigma * 3.0f) would place or size differently"""
    kps, ss = kc.orientation_keypoints("ramps")
    kps = kps[kps[:, 1] >= 0]
    assert int(F(kc.HALF_BELOW) + F(0.5)) == 1 and int(float(kc.HALF_BELOW) + 0.5) == 0
    assert any(np.nextafter(F(s), F(0)) == F(1.6666666) or F(s) == F(1.6666666) for s in kc.rounding_sigmas(1.0))
    for osg in kc.ORI_SIGMAS:
        d = [kc.ori_window(k, osg, True) for k in kps]
        f = [kc.ori_window(k, osg, False) for k in kps]
        rows = sum(a[0] != b[0] for a, b in zip(d, f)); cols = sum(a[1] != b[1] for a, b in zip(d, f))
        radii = sum(a[2] != b[2] for a, b in zip(d, f))
        print("ori_sigma %.1f: the float rule moves the row of %d keypoints, the column of %d, changes the radius of %d" % (osg, rows, cols, radii))
        assert rows >= 4 and cols >= 4 and radii >= 2


@pytest.mark.parametrize("octsize", [1, 2])
def test_descriptor_orientation_wrap(oracle, maps, octsize):
    """samples with o == 2 pi_f (oval == 8, oi == 8: both taps wrap to bin 0), samples that need the loops twice or more,
    samples exactly on an orientation bin, a row or a column of the cell grid"""
    sincos = _sincos(oracle)
    tot = dict(oi8=0, o2pi=0, loops2=0, of0=0, rf0=0, cf0=0, neg0=0)
    per = {}
    for family in ("ramps", "ramps_neg", "small", "bump"):
        blurs, gm = maps(family)
        kk, ks = kc.descriptor_keypoints(family, octsize)
        fam = dict.fromkeys(tot, 0)
        for k, s in zip(kk, ks):
            if k[1] < 0:
                continue
            q = kc.desc_samples(k, octsize, gm[s][0], gm[s][1], sincos)
            live = q["mag"] > 0
            fam["oi8"] += int(((q["oi"] == 8) & live).sum()); fam["o2pi"] += int(((q["o"] == TWO_PI_F) & (q["oval"] == 8) & live).sum())
            fam["loops2"] += int(((q["loops"] >= 2) & live).sum())
            fam["of0"] += int(((q["of"] == 0) & live).sum()); fam["rf0"] += int(((q["rf"] == 0) & live).sum()); fam["cf0"] += int(((q["cf"] == 0) & live).sum())
            fam["neg0"] += int(((q["oval"] == 0) & np.signbit(q["oval"]) & live).sum())
        per[family] = fam
        for key in tot:
            tot[key] += fam[key]
    # oi == 8 with an infinite magnitude: the reference adds inf * 1 and then inf * 0 = NaN to bin 0 (desc_eval4 adds +0)
    blurs, gm = maps("huge")
    kk, ks = kc.descriptor_keypoints("huge", octsize)
    inf8 = sum(int(((q["oi"] == 8) & np.isinf(q["mag"])).sum()) for q in
               (kc.desc_samples(k, octsize, gm[s][0], gm[s][1], sincos) for k, s in zip(kk, ks) if k[1] >= 0))
    per["huge"] = dict(oi8_with_infinite_magnitude=inf8)
    assert inf8 >= 100
    print("octsize %d, window samples with a gradient:" % octsize, per)
    assert per["ramps"]["oi8"] >= 100 and per["small"]["oi8"] >= 20 and tot["o2pi"] >= 100
    assert per["ramps"]["loops2"] >= 100 and per["small"]["loops2"] >= 100
    assert tot["of0"] >= 100 and tot["rf0"] >= 100 and tot["cf0"] >= 100 and tot["neg0"] >= 10


@pytest.mark.parametrize("octsize", [1, 2])
def test_descriptor_tail(oracle, maps, octsize):
    """saturated bytes, the 0.2 clamp, all-zero histograms, norms that overflow, inf / NaN magnitudes"""
    sincos = _sincos(oracle)

    def describe(family):
        blurs, gm = maps(family)
        kk, ks = kc.descriptor_keypoints(family, octsize)
        desc = np.zeros((len(kk), 128), np.uint8)
        for s in (1, 2, 3):
            sel = np.nonzero(ks == s)[0]
            desc[sel] = oracle.descriptor(np.ascontiguousarray(kk[sel]), gm[s][0], gm[s][1], octsize, 0, len(sel))
        return kk, ks, desc, gm

    fig = {}
    for family in ("ramps", "step", "bump", "checker"):
        kk, ks, desc, gm = describe(family)
        fig[family] = (int((desc == 255).any(axis=1).sum()), int(desc.any(axis=1).sum()))
        assert fig[family][0] >= 10, (family, fig[family])
    # the clamp: after the second normalisation a clamped value is the largest of the descriptor and several share it, or
    # a single cell holds everything (one bin at 0.2 / 0.2 -> 512 -> 255)
    kk, ks, desc, gm = describe("ramps")
    clamped = 0
    for k, s, d in zip(kk, ks, desc):
        if k[1] < 0 or not d.any():
            continue
        q = kc.desc_samples(k, octsize, gm[s][0], gm[s][1], sincos)
        hist = kc_histogram(oracle, q)
        with np.errstate(all="ignore"):
            n1 = hist * (F(1) / np.sqrt(np.add.reduce(hist * hist, dtype=F)))
        clamped += bool((n1 > F(0.2)).any())
    fig["ramps: clamp acted"] = clamped
    assert clamped >= 50
    for family in ("constant", "tiny", "huge", "subnormal"):
        kk, ks, desc, gm = describe(family)
        zero = int((~desc.any(axis=1) & (kk[:, 1] >= 0)).sum())
        fig[family + ": all zero"] = (zero, int((kk[:, 1] >= 0).sum()))
        if family in ("constant", "huge"):
            assert zero == (kk[:, 1] >= 0).sum()
        elif family == "tiny":
            assert zero >= 20 and desc.any(axis=1).sum() >= 20       # scale 1 (1e-18) still describes, the squares of scale 3 underflow
    # tiny: histograms that are not empty, whose 128 squares all underflow -- the first norm is 1 / sqrt(0) = inf, a non-zero
    # bin becomes inf and is clamped, a zero bin becomes 0 * inf = NaN, and the second norm makes every byte 0
    kk, ks, desc, gm = describe("tiny")
    overflow = 0
    for k, s, d in zip(kk, ks, desc):
        if k[1] < 0 or s == 1:
            continue
        hist = kc_histogram(oracle, kc.desc_samples(k, octsize, gm[s][0], gm[s][1], sincos))
        if hist.any() and not (hist * hist).any():
            assert not d.any()
            overflow += 1
    fig["tiny: first norm inf"] = overflow
    assert overflow >= 10
    # nanpix: a sample with an infinite magnitude and an ordinary orientation (next to the 2e38 pixel) makes every sum it
    # reaches inf or NaN and the descriptor all zero; a sample with a NaN orientation (next to the NaN and the inf pixel)
    # fails `oi >= 0` -- (int)NaN is INT_MIN in the reference's native build -- and is skipped: the keypoint is described
    # by its other samples, or left all zero where the window is that one sample
    kk, ks, desc, gm = describe("nanpix")
    poisoned = skipped = skipped_only = clean = 0
    for k, s, d in zip(kk, ks, desc):
        if k[1] < 0:
            continue
        q = kc.desc_samples(k, octsize, gm[s][0], gm[s][1], sincos)
        poison = bool((np.isinf(q["mag"]) & np.isfinite(q["ori"])).any())
        nan_ori = np.isnan(q["ori"])
        if poison:
            assert not d.any()
            poisoned += 1
        elif nan_ori.any():
            if d.any():
                skipped += 1
            elif nan_ori.all():
                skipped_only += 1
        elif d.any():
            clean += 1
    fig["nanpix"] = dict(all_zero_for_an_inf_sample=poisoned, described_despite_nan_orientations=skipped,
                         all_zero_windows_of_nan_orientations_only=skipped_only, described_away_from_the_pixels=clean)
    print("octsize %d:" % octsize, fig)
    assert poisoned >= 10 and skipped >= 10 and skipped_only >= 1 and clean >= 50


def kc_histogram(oracle, q):
    """the 128 sums of keypoints_cpu.cl:90-113 from the samples of desc_samples in float32 (tap by tap, not sample by sample:
    the last bits of a sum may differ from the reference's, which does not move a value across the 0.2 clamp here)"""
    er, ec = q["rx"] - F(1.5), q["cx"] - F(1.5)
    mag = q["mag"] * oracle.expf_array(F(-0.125) * (er * er + ec * ec))
    hist = np.zeros(128, F)
    ok = (q["ri"] >= -1) & (q["ri"] < 4) & (q["oi"] >= 0) & (q["oi"] <= 8) & (q["rf"] >= 0) & (q["rf"] <= 1)
    for a in (0, 1):
        rb = q["ri"] + a
        rw = mag * (q["rf"] if a else F(1) - q["rf"])
        for b in (0, 1):
            cb = q["ci"] + b
            cw = rw * (q["cf"] if b else F(1) - q["cf"])
            for e in (0, 1):
                ob = q["oi"] + e
                ob = np.where(ob >= 8, 0, ob)
                m = ok & (rb >= 0) & (rb < 4) & (cb >= 0) & (cb < 4)
                idx = ((rb * 4 + cb) * 8 + ob)[m].astype(np.int64)
                np.add.at(hist, idx, (cw * (q["of"] if e else F(1) - q["of"]))[m])
    return hist
