"""Every form of the per-keypoint kernels, reached as a stage and compared with the CPU oracle bit for bit.

A plan picks the form of its orientation and descriptor launches from counts only the device knows: a wave or a workgroup
per keypoint, the gradient evaluated in the window or read from full maps (MAPS), the row-interval or the streaming
descriptor; and on a dense frame one wave or workgroup takes many keypoints in turn.  siftmi_stage_orientation_ex /
siftmi_stage_descriptor_ex launch the form asked for on the number of workgroups asked for and report the form the launch
selects (for forms 1 and 2 the kernel's count rule applied to its arguments: the kernel does not report its form back);
siftmi_stage_gradient_maps runs the map kernel over a whole pyramid.  Every oracle result is computed once per case and each
form is compared with it."""
import ctypes as C

import numpy as np
import pytest

from util import (descriptor_edge_rows, descriptor_random_rows, multiscale_noise, oracle_pyramid, orientation_border_rows,
                  smooth_noise, sort_rows, white_noise)

pytestmark = pytest.mark.gpu

EINVAL = -1
WAVE, TEAM, STREAM, MAPS = 1, 2, 3, 4
DESC_FORMS = (WAVE, TEAM, WAVE | MAPS, TEAM | MAPS, STREAM)
ORI_FORMS = (WAVE, TEAM, WAVE | MAPS, TEAM | MAPS)
BLOCKS = (0, 1, 7)          # the stage's grid; one workgroup for the whole list; seven: neighbours in the list go to different ones
F = np.float32


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _params(ori_sigma=1.5):
    from sift_pyocl_amd import _lib
    return _lib.Params(init_sigma=1.6, peak_thresh=F(255.0 * 0.04 / 3.0), edge_thresh0=F(0.08), edge_thresh=F(0.06),
                       ori_sigma=F(ori_sigma), border_dist=5, octave_max=0, pix_per_kp=10, double_im_size=0)


def desc_radius(sigma, octsize):
    """(R, spacing) of a descriptor window, in float32 as desc_window computes them (keypoints_cpu.cl:57-62)"""
    spacing = F(F(sigma) / F(octsize)) * F(3.0)
    return int(F(F(F(1.414) * spacing) * F(2.5)) + F(0.5)), float(spacing)


def sigma_for_radius(R):
    """the largest sigma of radius R (octave size 1): 1.414 * 2.5 * spacing = R + 0.49, so that the rotated window reaches
    well into rows and columns R pixels from its centre (at exactly R they get a weight of ~1e-4)"""
    sigma = F((R + 0.49) / (1.414 * 3.0 * 2.5))
    assert desc_radius(sigma, 1)[0] == R
    return float(sigma)


def _unclipped_maps(oracle, blurs, s):
    """gradient maps of plane s as a fetch without the border rule would see them (desc_fetch<INTERIOR = true> on a border
    pixel): central differences of the neighbours in memory, no doubling -- the row above a plane is the previous plane's
    last row, the pixel left of a row the previous row's last one"""
    H, W = blurs.shape[1:]
    flat = blurs.ravel()
    p = s * H * W + np.arange(H * W)
    gx = flat[p + 1] - flat[p - 1]
    gy = flat[p - W] - flat[p + W]
    g = np.sqrt(gx * gx + gy * gy).reshape(H, W)
    o = oracle.atan2f_array(np.ascontiguousarray(-gy), np.ascontiguousarray(gx)).reshape(H, W)
    return g, o


def _blurs(oracle, maker, shape):
    return oracle_pyramid(oracle, maker(shape))[0][0]


def _oracle_descriptors(oracle, blurs, octsize, kk, ss):
    want = np.zeros((len(kk), 128), np.uint8)
    for s in np.unique(ss):
        sel = np.nonzero(ss == s)[0]
        eg, eo = oracle.gradient(blurs[s])
        want[sel] = oracle.descriptor(np.ascontiguousarray(kk[sel]), eg, eo, octsize, 0, len(sel))
    return want


def _oracle_orientation(oracle, blurs, kps, ss, octsize=1, ori_sigma=1.5):
    """the oracle's oriented keypoints of a refined list, NaN rows dropped, as sorted rows (x, y, sigma, angle, scale)"""
    out = []
    par = oracle.default_params()
    par.ori_sigma = F(ori_sigma)
    for s in np.unique(ss):
        sel = kps[ss == s]
        eg, eo = oracle.gradient(blurs[s])
        buf = np.full((len(sel) * 8 + 8, 4), -1, np.float32); buf[:len(sel)] = sel
        okp, cnt = oracle.orientation(buf, eg, eo, octsize, 0, len(sel), capacity=len(buf), par=par)
        assert cnt <= len(buf)
        okp = okp[:cnt][okp[:cnt, 1] >= 0]                          # (holes of the list stay where they were: row -1)
        okp = okp[~np.isnan(okp.sum(axis=1))]
        out.append(np.concatenate([okp, np.full((len(okp), 1), s, np.float32)], axis=1))
    return sort_rows(np.concatenate(out))


def _descriptor_ex(siftlib, blurs, octsize, kk, ss, form, blocks, fill=0):
    H, W = blurs.shape[1:]
    kk = np.ascontiguousarray(kk, np.float32); ss = np.ascontiguousarray(ss, np.int32)
    got = np.full((len(kk), 128), fill, np.uint8)
    used = C.c_int32(-1)
    rc = siftlib.siftmi_stage_descriptor_ex(0, _p(blurs), W, H, octsize, _p(kk), _p(ss), len(kk), _p(got), form, blocks, C.byref(used))
    return rc, got, used.value


def _check_descriptor_forms(siftlib, blurs, octsize, kk, ss, want, what, forms=DESC_FORMS, blocks_list=BLOCKS):
    for form in forms:
        for blocks in blocks_list:
            rc, got, used = _descriptor_ex(siftlib, blurs, octsize, kk, ss, form, blocks)
            assert rc == 0 and used == form, (what, form, blocks, rc, used)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert len(bad) == 0, "%s, form %d, %d workgroups: descriptors differ for %d keypoints, first %s" % (
                what, form, blocks, len(bad), kk[bad[:4]])


def _check_orientation_forms(siftlib, blurs, kps, ss, want, what, forms=ORI_FORMS, blocks_list=BLOCKS, octsize=1, ori_sigma=1.5):
    H, W = blurs.shape[1:]
    kps = np.ascontiguousarray(kps, np.float32); ss = np.ascontiguousarray(ss, np.int32)
    par = _params(ori_sigma)
    cap = len(kps) * 8 + 8
    for form in forms:
        for blocks in blocks_list:
            out = np.zeros((cap, 4), np.float32); osc = np.zeros(cap, np.int32)
            no, used = C.c_int64(-1), C.c_int32(-1)
            rc = siftlib.siftmi_stage_orientation_ex(0, _p(blurs), W, H, octsize, _p(kps), _p(ss), len(kps), C.byref(par), _p(out), _p(osc),
                                                     cap, C.byref(no), form, blocks, C.byref(used))
            assert rc == 0 and used.value == form, (what, form, blocks, rc, used.value)
            assert no.value == len(want), "%s, form %d, %d workgroups: %d oriented keypoints, oracle %d" % (what, form, blocks, no.value, len(want))
            got = sort_rows(np.concatenate([out[:no.value], osc[:no.value, None].astype(np.float32)], axis=1))
            bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]
            assert len(bad) == 0, "%s, form %d, %d workgroups: %d rows differ, first %s vs %s" % (what, form, blocks, len(bad), got[bad[:2]], want[bad[:2]])


# ----------------------------------------------------------------------------- descriptor
@pytest.mark.parametrize("octsize", [1, 2])
def test_descriptor_edge_set_in_every_form(siftlib, oracle, octsize):
    """The windows of test_descriptor_windows_at_their_edges (axes on and a hair off the pixel axes and diagonals, radius
    4 ... 126, centres on and beyond the borders, half-pixel offsets) in every form, on 0, 1 and 7 workgroups."""
    H, W = 300, 421
    blurs = _blurs(oracle, smooth_noise, (H, W))
    kk = descriptor_edge_rows(W, H, octsize)
    ss = np.full(len(kk), 2, np.int32)
    want = _oracle_descriptors(oracle, blurs, octsize, kk, ss)
    _check_descriptor_forms(siftlib, blurs, octsize, kk, ss, want, "edge set, octsize %d" % octsize)


@pytest.mark.parametrize("seed,octsize,shape", [(1, 1, (300, 421)), (2, 4, (257, 330)), (3, 1, (97, 131))])
def test_descriptor_random_keypoints_in_every_form(siftlib, oracle, seed, octsize, shape):
    """The 3000 random windows per case of test_descriptor_random_keypoints in every form, on 0, 1 and 7 workgroups."""
    H, W = shape
    blurs = _blurs(oracle, white_noise if seed == 2 else multiscale_noise, shape)
    kk = descriptor_random_rows(seed, W, H, octsize)
    ss = np.full(len(kk), 1 + seed % 3, np.int32)
    want = _oracle_descriptors(oracle, blurs, octsize, kk, ss)
    _check_descriptor_forms(siftlib, blurs, octsize, kk, ss, want, "random set %d" % seed)


def test_descriptor_interior_rule_at_its_edge(siftlib, oracle):
    """Windows whose first or last row or column lies 0, 1 or 2 pixels inside the plane, at R = 4, 17, 60, 127: desc_window's
    `interior` (a margin of one pixel) picks the unclipped fetch, without the one-sided differences of the border
    (image.cl:58-77).  R and the centre pixel are computed in float32 as the kernel does; three sub-pixel offsets, three
    angles.  The windows at margin 0 do sample their border row or column with weight: the oracle, fed the maps an unclipped
    fetch would see there (a rule with margin 0), gives other descriptors for some of them."""
    H, W = 300, 421
    blurs = _blurs(oracle, multiscale_noise, (H, W))
    rows, margin, interior = [], [], []
    for R in (4, 17, 60, 127):
        sg = sigma_for_radius(R)
        for d in (0, 1, 2):
            # (centre row, centre column): first row, last row, first column, last column of the window d pixels inside
            for cy, cx in [(R + d, W // 2), (H - 1 - d - R, W // 2), (H // 2, R + d), (H // 2, W - 1 - d - R)]:
                for frac in (0.0, 0.3, -0.45):
                    for ang in (0.0, float(F(np.pi / 4)), 2.3):
                        y, x = F(cy + frac if cy != H // 2 else cy), F(cx + frac if cx != W // 2 else cx)
                        irow, icol = int(F(y + F(0.5))), int(F(x + F(0.5)))
                        assert (irow, icol) == (cy, cx)
                        interior.append(irow - R >= 1 and irow + R <= H - 2 and icol - R >= 1 and icol + R <= W - 2)
                        margin.append(d)
                        rows.append((x, y, sg, ang))
    margin = np.array(margin)
    assert np.array_equal(~np.array(interior), margin == 0)
    kk = np.array(rows, np.float32)
    s = 3
    ss = np.full(len(kk), s, np.int32)
    want = _oracle_descriptors(oracle, blurs, 1, kk, ss)
    eg, eo = oracle.gradient(blurs[s])
    ug, uo = _unclipped_maps(oracle, blurs, s)
    assert np.array_equal(ug[1:-1, 1:-1].view(np.uint32), eg[1:-1, 1:-1].view(np.uint32))
    assert np.array_equal(uo[1:-1, 1:-1].view(np.uint32), eo[1:-1, 1:-1].view(np.uint32))
    at0 = np.nonzero(margin == 0)[0]
    unclipped = oracle.descriptor(np.ascontiguousarray(kk[at0]), ug, uo, 1, 0, len(at0))
    assert (unclipped != want[at0]).any(axis=1).sum() >= 5, "the margin-0 windows do not see their border"
    _check_descriptor_forms(siftlib, blurs, 1, kk, ss, want, "interior rule", blocks_list=(0, 7))


@pytest.mark.parametrize("octsize", [1, 2])
def test_descriptor_tiny_windows(siftlib, oracle, octsize):
    """sigma / octsize 0.02, 0.1, 0.2, 0.3: R = 0 ... 3; a spacing of 0.06 (< 0.1) takes the true division instead of the
    corrected reciprocal (k_descriptor.hpp: fast_div).  Centres inside, on the borders and corners, beyond the plane."""
    H, W = 97, 131
    blurs = _blurs(oracle, white_noise, (H, W))
    rows = []
    for f in (0.02, 0.1, 0.2, 0.3):
        for (cx, cy) in [(60.0, 40.0), (60.5, 40.5), (0.0, 0.0), (W - 1.0, H - 1.0), (0.25, H - 1.25), (W - 1.0, 10.75), (-1.0, 20.0)]:
            for ang in (0.0, 0.7, -2.0, float(F(np.pi)), float(F(-np.pi / 2)) + 1e-6):
                rows.append((cx * octsize, cy * octsize, f * octsize, ang))
    kk = np.array(rows, np.float32)
    radii = [desc_radius(k[2], octsize) for k in kk]
    assert sorted({R for R, _ in radii}) == [0, 1, 2, 3] and min(sp for _, sp in radii) < 0.1
    ss = np.full(len(kk), 1, np.int32)
    want = _oracle_descriptors(oracle, blurs, octsize, kk, ss)
    _check_descriptor_forms(siftlib, blurs, octsize, kk, ss, want, "tiny windows, octsize %d" % octsize)


def test_descriptor_workgroup_form_at_volume(siftlib, oracle):
    """The workgroup form adds its four waves' pools bin by bin in batch order -- the additions of the wave form, in the same
    order.  Another order changes a sum in its last bits only, and a descriptor byte only where such a sum lies at a
    quantisation step: 20 000 windows (R 10 ... 63) on a smooth plane, so that an order slip shows."""
    H, W = 300, 421
    blurs = _blurs(oracle, lambda shape: smooth_noise(shape, seed=9, sigma=2.0), (H, W))
    rng = np.random.default_rng(31)
    n = 20000
    kk = np.empty((n, 4), np.float32)
    kk[:, 0] = rng.uniform(0, W, n); kk[:, 1] = rng.uniform(0, H, n)
    kk[:, 2] = np.exp(rng.uniform(np.log(1.0), np.log(6.0), n)); kk[:, 3] = rng.uniform(-np.pi, np.pi, n)
    ss = np.full(n, 2, np.int32)
    want = _oracle_descriptors(oracle, blurs, 1, kk, ss)
    _check_descriptor_forms(siftlib, blurs, 1, kk, ss, want, "volume", forms=(TEAM, TEAM | MAPS), blocks_list=(0,))


def test_descriptor_state_left_by_the_previous_keypoint(siftlib, oracle):
    """On 1 or 7 workgroups every wave (workgroup form: every workgroup) describes a sequence of keypoints, laid out so that
    each one follows a keypoint that left the most LDS state: the largest windows (R = 127, inside and clipped) alternate with
    the smallest (R = 0, 1), with windows entirely beyond the plane, and with holes of the list (y < 0: an empty record; the
    workgroup form first waits for the previous keypoint's record), a hole right behind a largest window."""
    H, W = 300, 421
    blurs = _blurs(oracle, multiscale_noise, (H, W))
    big = sigma_for_radius(127)
    kinds = {
        "large": [(210.0, 150.0, big, 0.3), (210.5, 149.5, big, float(F(np.pi / 4))), (100.0, 40.0, big, -2.2), (400.0, 290.0, big, 1.9)],
        "small": [(50.0, 60.0, 0.02, 0.1), (300.25, 200.5, 0.1, -1.0), (0.0, 0.0, 0.1, 2.0)],
        "outside": [(W + 300.0, 100.0, 2.0, 0.5), (-250.0, H + 200.0, 3.0, -0.5)],
        "hole": [(100.0, -1.0, 2.0, 0.0), (50.0, -1.0, big, 1.0)],
    }
    pool = np.array([r for k in kinds for r in kinds[k]], np.float32)
    first = np.cumsum([0] + [len(kinds[k]) for k in kinds])
    index = {k: list(range(first[i], first[i + 1])) for i, k in enumerate(kinds)}
    ss = np.full(len(pool), 2, np.int32)
    want = _oracle_descriptors(oracle, blurs, 1, pool, ss)
    assert want[index["large"]].any(axis=1).all() and not want[index["hole"] + index["outside"]].any()
    pattern = ["large", "small", "large", "hole", "large", "outside", "large", "hole", "small", "large", "outside"]
    for form in DESC_FORMS:
        for blocks in (1, 7):
            workers = blocks if (form & 3) == TEAM else 4 * blocks       # keypoint i goes to worker i % workers
            idx = np.array([index[k][(r * workers + j) % len(index[k])] for r, k in enumerate(pattern) for j in range(workers)])
            _check_descriptor_forms(siftlib, blurs, 1, pool[idx], ss[idx], want[idx], "sequence", forms=(form,), blocks_list=(blocks,))


def test_descriptor_streaming_form_beyond_the_row_tables(siftlib, oracle):
    """Windows the row tables cannot hold (sigma 12.05 ... 45: R = 128 up to windows larger than the 300 x 421 plane,
    spacing above 128): the stage's rule takes the streaming form, equal to the oracle; the row-interval forms refuse the
    list (SIFTMI_EINVAL) before any launch -- their kernels trap on such a window -- and leave the output alone."""
    H, W = 300, 421
    blurs = _blurs(oracle, smooth_noise, (H, W))
    rng = np.random.default_rng(12)
    n = 72
    kk = np.empty((n, 4), np.float32)
    kk[:, 0] = rng.uniform(-20, W + 20, n)
    kk[:, 1] = rng.uniform(0, H + 20, n)
    kk[:, 2] = np.exp(rng.uniform(np.log(12.05), np.log(45.0), n))
    kk[:4, 2] = [12.05, 45.0, 43.0, 30.0]
    kk[:, 3] = rng.uniform(-np.pi, np.pi, n)
    kk[4, 3] = F(np.pi / 4); kk[5, 3] = 0.0
    radii = [desc_radius(k[2], 1) for k in kk]
    assert min(R for R, _ in radii) == 128 and max(sp for _, sp in radii) > 128 and max(2 * R + 1 for R, _ in radii) > W
    ss = np.full(n, 3, np.int32)
    want = _oracle_descriptors(oracle, blurs, 1, kk, ss)
    assert want.any(axis=1).sum() > n // 2
    rc, got, used = _descriptor_ex(siftlib, blurs, 1, kk, ss, 0, 0)
    assert rc == 0 and used == STREAM
    assert np.array_equal(got, want)
    _check_descriptor_forms(siftlib, blurs, 1, kk, ss, want, "beyond the row tables", forms=(STREAM,), blocks_list=(1, 7))
    for form in (WAVE, TEAM, WAVE | MAPS, TEAM | MAPS):
        rc, got, used = _descriptor_ex(siftlib, blurs, 1, kk, ss, form, 0, fill=0xA5)
        assert rc == EINVAL and used == -1 and (got == 0xA5).all(), form


# ----------------------------------------------------------------------------- orientation
def test_orientation_border_set_in_every_form(siftlib, oracle):
    """The windows of test_orientation_windows_at_the_borders (radius 2 ... 36, every border and corner, half-pixel centres),
    with discarded rows (row -1) among them, in every form on 0, 1 and 7 workgroups: as a set, bit for bit, the discarded
    rows skipped.  On one workgroup its waves park and flush every result of the list."""
    H, W = 300, 421
    blurs = _blurs(oracle, multiscale_noise, (H, W))
    sel = orientation_border_rows(W, H)
    want = _oracle_orientation(oracle, blurs, sel, np.full(len(sel), 1, np.int32))
    assert len(want) >= len(sel) // 2
    kps = np.insert(sel, np.arange(0, len(sel), 5), np.array([12.0, -1.0, 100.0, 2.0], np.float32), axis=0)
    _check_orientation_forms(siftlib, blurs, kps, np.full(len(kps), 1, np.int32), want, "border set")


# ----------------------------------------------------------------------------- natural lists
@pytest.mark.parametrize("maker,shape", [(smooth_noise, (131, 97)), (white_noise, (256, 300)), (multiscale_noise, (300, 421))])
def test_natural_lists_in_every_form(siftlib, oracle, maker, shape):
    """The refined and oriented keypoints of test_detection_stages' three frames, all three detection scales in one list,
    through every orientation and every descriptor form."""
    H, W = shape
    blurs, dogs = oracle_pyramid(oracle, maker(shape))[0]
    opar = oracle.default_params()
    cand = []
    for s in (1, 2, 3):
        k, n = oracle.local_maxmin(dogs, s, 1, H * W // 10, opar)
        cand.append(k[:n])
    cand = np.ascontiguousarray(np.concatenate(cand))
    interp = oracle.interp_keypoint(dogs, cand, 0, len(cand), opar)
    keep = interp[:, 1] != -1
    kps, ss = np.ascontiguousarray(interp[keep]), cand[keep][:, 3].astype(np.int32)
    want = _oracle_orientation(oracle, blurs, kps, ss)
    assert len(want) > 20
    _check_orientation_forms(siftlib, blurs, kps, ss, want, "natural list %r" % (shape,))
    kk, ks = np.ascontiguousarray(want[:, :4]), want[:, 4].astype(np.int32)
    _check_descriptor_forms(siftlib, blurs, 1, kk, ks, _oracle_descriptors(oracle, blurs, 1, kk, ks), "natural list %r" % (shape,))


# ----------------------------------------------------------------------------- gradient maps
def _stress_plane(kind, shape, rng):
    if kind == "noise":
        return (rng.random(shape) * 255).astype(np.float32)
    if kind == "small":                          # gx = +-gy, zeros, -0.0
        a = rng.integers(-2, 3, shape).astype(np.float32)
        a[(a == 0) & (rng.random(shape) < 0.5)] = F(-0.0)
        return a
    if kind == "constant":
        return np.full(shape, 7.25, np.float32)
    if kind == "subnormal":                      # differences below the fast path's range, magnitudes that underflow
        return (rng.integers(-2 ** 20, 2 ** 20, shape) * 2.0 ** -149).astype(np.float32)
    if kind == "large":                          # around the fast path's 1e18 bound
        return (rng.random(shape) * 4e18).astype(np.float32)
    return rng.choice(np.array([-3e38, 3e38, 1e38, 0.0], np.float32), shape)     # "huge": differences overflow to +-inf


def test_gradient_maps_over_a_pyramid(siftlib, oracle):
    """gradient_maps_kernel (compute_gradient_orientation, image.cl:47-80, on planes 1..3 of every octave: its own copy of
    the gradient arithmetic and of the Ziv atan2 with its fall-back) against oracle.gradient on every pixel, over a pyramid
    down to the smallest octave a plan makes: widths no multiple of 256, heights no multiple of 32, octaves narrower than 256
    and shorter than 32; the octave ranges a plan launches and the full range, on 1, 3 and the default number of workgroups;
    maps outside the range keep what was there.  Planes of small integers, -0.0, constants, sub-normals, values near 1e18
    and values whose differences overflow."""
    H0, W0 = 333, 601
    n_oct = oracle.octave_count(H0, W0)
    shapes = [(H0 >> o, W0 >> o) for o in range(n_oct)]
    assert n_oct >= 5 and shapes[-1][0] < 32 and shapes[-1][1] < 256
    kinds = ["noise", "small", "huge", "subnormal", "constant", "large"]
    rng = np.random.default_rng(21)
    planes, want_g, want_o = [], [], []
    for o, (h, w) in enumerate(shapes):
        six = [rng.random((h, w), dtype=np.float32) for _ in range(6)]      # (planes 0, 4 and 5 are not read)
        for p in (1, 2, 3):
            six[p] = _stress_plane(kinds[(3 * o + p - 1) % len(kinds)], (h, w), rng)
        planes.append(np.stack(six).ravel())
        grads = [oracle.gradient(six[p]) for p in (1, 2, 3)]
        want_g.append(np.stack([g for g, _ in grads]).ravel()); want_o.append(np.stack([a for _, a in grads]).ravel())
    planes = np.ascontiguousarray(np.concatenate(planes))
    Wa = np.array([w for _, w in shapes], np.int32); Ha = np.array([h for h, _ in shapes], np.int32)
    moff = np.cumsum([0] + [3 * h * w for h, w in shapes])
    sentinel = np.uint32(0xa5a5a5a5)             # (not a NaN: the in-range comparison lets NaN equal NaN)
    for lo, hi in [(0, 1), (1, 2), (2, n_oct), (1, n_oct), (0, n_oct)]:
        for blocks in (1, 3, 0):
            gmap = np.full(moff[-1], sentinel, np.uint32); omap = np.full(moff[-1], sentinel, np.uint32)
            assert siftlib.siftmi_stage_gradient_maps(0, _p(planes), n_oct, _p(Wa), _p(Ha), lo, hi, blocks, _p(gmap), _p(omap)) == 0
            for o, (h, w) in enumerate(shapes):
                seg = slice(moff[o], moff[o + 1])
                for got, want, name in ((gmap[seg], want_g[o], "magnitude"), (omap[seg], want_o[o], "orientation")):
                    if not lo <= o < hi:
                        assert (got == sentinel).all(), (lo, hi, blocks, o, name)
                        continue
                    gf = got.view(np.float32)
                    bad = np.nonzero((got != want.view(np.uint32)) & ~(np.isnan(gf) & np.isnan(want)))[0]
                    assert len(bad) == 0, "[%d, %d), %d workgroups, octave %d %s: %d pixels differ, first (plane, y, x) %s: %r vs %r" % (
                        lo, hi, blocks, o, name, len(bad), np.unravel_index(bad[0], (3, h, w)), gf[bad[:3]], want[bad[:3]])


# ----------------------------------------------------------------------------- refusals
def test_stage_hooks_refuse_what_they_cannot_launch(siftlib):
    """SIFTMI_EINVAL, nothing written: an unknown form, a negative workgroup count, MAPS with a detection scale outside 1..3,
    MAPS with the streaming or the size-picked descriptor form; an octave range outside the pyramid."""
    H, W = 40, 50
    blurs = np.random.default_rng(0).random((6, H, W), dtype=np.float32)
    kk = np.array([[20.0, 20.0, 2.0, 0.5]], np.float32)
    for form, blocks, scale in [(WAVE | MAPS, 0, 0), (TEAM | MAPS, 0, 4), (STREAM | MAPS, 0, 2), (MAPS, 0, 2), (8, 0, 2), (-1, 0, 2),
                                (WAVE, -1, 2), (TEAM, -1, 2)]:
        rc, got, used = _descriptor_ex(siftlib, blurs, 1, kk, np.array([scale], np.int32), form, blocks, fill=0xA5)
        assert rc == EINVAL and used == -1 and (got == 0xA5).all(), (form, blocks, scale)
    par = _params()
    for form, blocks, scale in [(WAVE | MAPS, 0, 0), (TEAM | MAPS, 0, 5), (3, 0, 1), (7, 0, 1), (8, 0, 1), (WAVE, -1, 1)]:
        out = np.full((16, 4), 5.0, np.float32); osc = np.full(16, 9, np.int32); ks = np.array([scale], np.int32)
        no, used = C.c_int64(-1), C.c_int32(-1)
        rc = siftlib.siftmi_stage_orientation_ex(0, _p(blurs), W, H, 1, _p(kk), _p(ks), 1, C.byref(par), _p(out), _p(osc), 16,
                                                 C.byref(no), form, blocks, C.byref(used))
        assert rc == EINVAL and used.value == -1 and no.value == -1 and (out == 5).all() and (osc == 9).all(), (form, blocks, scale)
    Wa, Ha = np.array([W], np.int32), np.array([H], np.int32)
    gm = np.full(3 * H * W, 3.0, np.float32); om = gm.copy()
    for n_oct, lo, hi, blocks in [(1, 0, 2, 0), (1, 1, 0, 0), (1, -1, 1, 0), (1, 0, 1, -1), (0, 0, 0, 0)]:
        rc = siftlib.siftmi_stage_gradient_maps(0, _p(blurs), n_oct, _p(Wa), _p(Ha), lo, hi, blocks, _p(gm), _p(om))
        assert rc == EINVAL and (gm == 3).all() and (om == 3).all(), (n_oct, lo, hi, blocks)
