"""Crafted gradient planes and keypoint lists for the per-keypoint stages (orientation_cpu.cl:41-174,
keypoints_cpu.cl:36-161), plus numpy restatements of the predicates that say a family reaches its rule.

Noise planes never put a gradient orientation on a histogram bin edge, never tie two peaks, never leave a histogram empty
or infinite and never saturate a descriptor; the planes here do, by construction.  Every family is a `blur` stack of six
planes as the stage hooks take it: the crafted planes at detection scales 1..3, noise at 0, 4 and 5.  Plain numpy: no GPU,
no oracle, no reference -- tests/test_keypoint_cases_host.py checks with the oracle that every rule is reached,
tests/test_oracle_vs_ref.py pins the oracle to the reference's kernels on these inputs, tests/test_gpu_keypoint_cases.py
runs the HIP kernels on them.

The planes may hold anything; the keypoints may not (check_orientation_list / check_descriptor_list): every field finite,
sigmas positive, no descriptor window beyond the row tables, orientation windows far below the kernel's index limits.  A
non-finite angle would make the reference's `while (o < 0) o += 2 pi` endless, a non-finite sigma its (int) undefined."""
import numpy as np

F = np.float32
PI_F = F(np.pi)                      # M_PI_F
TWO_PI_F = F(2.0) * PI_F             # 2.0f * M_PI_F (exact)
ONE_PI_F = F(1.0 / np.pi)            # M_1_PI_F
HALF_BELOW = np.nextafter(F(0.5), F(0))          # 0.5 - 2^-25: + 0.5 is 1.0 in float, below 1 in double

SHAPE = (64, 80)
ODD_SHAPE = (37, 53)
FAMILIES = ("ramps", "ramps_neg", "step", "bump", "bumps", "small", "checker", "constant", "tiny", "subnormal", "huge", "nanpix",
            "ori_plus_pi")
OCTSIZES = (1, 2, 4)
ORI_SIGMAS = (1.0, 1.5, 2.5)
DESC_MAXRAD = 127                    # k_descriptor.hpp: SIFT_DESC_MAXRAD

BUMPS_SIGMA = F(0.3)                 # ori_sigma 1.5: radius 1, the window is the centre and its four neighbours
BUMPS_ULPS = 16                      # the second bump's height sweeps this many ulps either side of 0.8 / exp(-1 / (2 sigma^2))
BIG = F(2.0 ** 20)


def bump_sites(shape):
    """(row, col) of the single-pixel bumps of `bump`, one plane per detection scale: mid-plane, near a corner, on the last
    usable row and column"""
    H, W = shape
    return [[(H // 2, W // 2), (H // 4, W // 4)], [(3, 3), (H // 2 + 1, W // 2 - 7)], [(H - 2, W - 2), (H // 2, 5)]]


def bumps_sites(shape):
    """(row, col, step) of the keypoints of `bumps`: a bump of height 1 right of the keypoint pixel (its gradient lands on
    the keypoint pixel, bin 18), one of height b(step) two rows below (its gradient lands on the pixel below, bin 27).
    The steps 0, 1, -1, 2, -2, ... as far as the plane has room, +-BUMPS_ULPS at the most."""
    H, W = shape
    steps = [0] + [sgn * n for n in range(1, BUMPS_ULPS + 1) for sgn in (1, -1)]
    places = [(r, c) for r in range(3, H - 6, 7) for c in range(3, W - 6, 7)]
    assert len(places) >= 9, "the plane is too small for a sweep of +-4 ulps"
    return [(r, c, step) for (r, c), step in zip(places, steps)]


def bumps_height(step, ori_sigma=1.5):
    sigma = float(F(ori_sigma) * BUMPS_SIGMA)
    b = F(0.8 / np.exp(-1.0 / (2.0 * sigma * sigma)))
    for _ in range(abs(step)):
        b = np.nextafter(b, F(np.inf) if step > 0 else F(0))
    return b


def _noise(shape, seed):
    return (np.random.default_rng(seed).random(shape) * 255).astype(F)


def crafted_planes(family, shape=SHAPE, seed=0):
    """the three crafted planes (detection scales 1, 2, 3) of a family"""
    H, W = shape
    rng = np.random.default_rng(1000 + seed)
    y, x = np.meshgrid(np.arange(H, dtype=F), np.arange(W, dtype=F), indexing="ij")
    z = np.zeros(shape, F)
    if family == "ramps":            # orientations -0 (gx > 0, -gy == -0), +pi/2, +pi/4
        return [F(3) * x, F(2) * y, x + y]
    if family == "ramps_neg":        # -pi (gx < 0, -gy == -0), -pi/4, -3pi/4
        return [-x, x - y, -x - y]
    if family == "step":
        out = []
        for col, h in ((W // 2, 5.0), (7, 255.0), (W - 3, 0.5)):
            p = z.copy(); p[:, col:] = h
            out.append(p)
        return out
    if family == "bump":
        out = []
        for sites in bump_sites(shape):
            p = z.copy()
            for r, c in sites:
                p[r, c] = 8.0
            out.append(p)
        return out
    if family == "bumps":
        p = z.copy()
        for r, c, step in bumps_sites(shape):
            p[r, c + 1] = 1.0
            p[r + 2, c] = bumps_height(step)
        return [p, p.copy(), p.copy()]
    if family == "small":            # gx == +-gy, zeros, -0.0
        out = []
        for _ in range(3):
            a = rng.integers(-2, 3, shape).astype(F)
            a[(a == 0) & (rng.random(shape) < 0.5)] = F(-0.0)
            out.append(a)
        return out
    if family == "checker":          # squares of 1 (no interior gradient at all: only the doubled border differences), 2 and 3 pixels
        return [(((x // n + y // n) % 2) * a).astype(F) for n, a in ((1, 4.0), (2, 4.0), (3, 255.0))]
    if family == "constant":
        return [np.full(shape, v, F) for v in (7.25, 0.0, -3.0)]
    if family == "tiny":             # squares of the gradient sub-normal; squares of the histogram underflow
        return [(rng.random(shape) * a).astype(F) for a in (1e-18, 1e-22, 4e-23)]
    if family == "subnormal":
        return [(rng.integers(-2 ** 20, 2 ** 20, shape) * 2.0 ** -149).astype(F) for _ in range(3)]
    if family == "huge":             # differences overflow to +-inf, inf - inf
        return [rng.choice(np.array([-3e38, 3e38, 1e38, 0.0], F), shape) for _ in range(3)]
    if family == "nanpix":
        out = []
        for s, (nan, inf, big) in enumerate(nanpix_sites(shape)):
            p = _noise(shape, 50 + s + seed)
            p[nan] = np.nan; p[inf] = np.inf; p[big] = 2e38
            out.append(p)
        return out
    if family == "ori_plus_pi":      # columns 1 mod 4: gx = -2^21, -gy = +2^-9: atan2 rounds to +pi_f; columns 3 mod 4: +0 side
        p = np.where(x % 4 == 0, BIG, np.where(x % 4 == 2, -BIG, y * F(2.0 ** -10))).astype(F)
        return [p, (p * F(0.5)).astype(F), (p * F(4.0)).astype(F)]
    raise ValueError(family)


def nanpix_sites(shape):
    """((row, col) of the NaN pixel, of the inf pixel, of the 2e38 pixel) per detection scale, well apart: a keypoint sees one
    of them or none.  Next to the NaN and the inf pixel the gradient and its orientation are NaN (inf and NaN); next to the
    2e38 pixel the gradient is finite, its square overflows and the orientation is an ordinary angle."""
    H, W = shape
    a, b, c, d = (H // 4, W // 4), (3 * H // 4, 3 * W // 4), (H // 4, 3 * W // 4), (3 * H // 4, W // 4)
    return [(a, b, c), (c, d, a), (b, a, d)]


def blur_stack(family, shape=SHAPE, seed=0):
    """(6, H, W): the crafted planes at scales 1..3, noise at 0, 4 and 5 (no per-keypoint kernel reads those)"""
    c = crafted_planes(family, shape, seed)
    stack = np.stack([_noise(shape, 90), c[0], c[1], c[2], _noise(shape, 94), _noise(shape, 95)]).astype(F)
    assert stack.shape == (6,) + tuple(shape)
    return np.ascontiguousarray(stack)


# ----------------------------------------------------------------------------- numpy restatements
def gradient_np(plane):
    """(gx, gy, magnitude, orientation) of compute_gradient_orientation (image.cl:47-80) in float32; the orientation through
    numpy's binary64 arctan2, rounded (its float32 one is an ulp off at pi/4): the oracle's on finite gradients but for rare
    double roundings; the oracle's atan2 of an infinite argument is NaN, numpy's is not"""
    I = np.ascontiguousarray(plane, F)
    with np.errstate(all="ignore"):
        gx = np.empty_like(I); gy = np.empty_like(I)
        gx[:, 1:-1] = I[:, 2:] - I[:, :-2]
        gx[:, 0] = F(2) * (I[:, 1] - I[:, 0]); gx[:, -1] = F(2) * (I[:, -1] - I[:, -2])
        gy[1:-1] = I[:-2] - I[2:]
        gy[0] = F(2) * (I[0] - I[1]); gy[-1] = F(2) * (I[-2] - I[-1])
        mag = np.sqrt(gx * gx + gy * gy)
        ori = np.arctan2((-gy).astype(np.float64), gx.astype(np.float64)).astype(F)
    return gx, gy, mag, ori


def frequent_orientations(plane, top=3):
    """the most frequent finite orientations among the pixels with a gradient"""
    _, _, mag, ori = gradient_np(plane)
    with np.errstate(all="ignore"):
        sel = ori[(mag > 0) & np.isfinite(ori)]
    if len(sel) == 0:
        return []
    u, n = np.unique(sel.view(np.uint32), return_counts=True)
    return [F(v) for v in u[np.argsort(-n, kind="stable")][:top].view(F)]


def ori_bin(a):
    """(int)(36.0f * (a + M_PI_F + 0.001f) / (2.0f * M_PI_F)), orientation_cpu.cl:88, before the clamp of 36 to 35"""
    a = np.asarray(a, F)
    return np.floor((F(36) * ((a + PI_F) + F(0.001))) / TWO_PI_F).astype(np.int64)


def ori_window(k, ori_sigma, in_double=True):
    """(row, col, radius) of a refined keypoint (peak, row, col, sigma), orientation_cpu.cl:67-71: the literals 0.5 and 3.0
    are doubles (in_double), where a float-only restatement would round k.s1 + 0.5f and sigma * 3.0f"""
    sigma = F(ori_sigma) * F(k[3])
    if in_double:
        return int(float(k[1]) + 0.5), int(float(k[2]) + 0.5), int(float(sigma) * 3.0)
    return int(F(k[1]) + F(0.5)), int(F(k[2]) + F(0.5)), int(sigma * F(3))


def ori_votes(k, mag, ori, ori_sigma):
    """bins (0..36, unclamped) of the samples that vote in a keypoint's histogram, in raster order"""
    H, W = mag.shape
    row, col, radius = ori_window(k, ori_sigma)
    rmin, cmin = max(0, row - radius), max(0, col - radius)
    rmax, cmax = min(row + radius, H - 2), min(col + radius, W - 2)
    if rmax < rmin or cmax < cmin:
        return np.zeros(0, np.int64)
    r, c = np.meshgrid(np.arange(rmin, rmax + 1), np.arange(cmin, cmax + 1), indexing="ij")
    d = r.astype(F) - F(k[1]); distsq = d * d
    d = c.astype(F) - F(k[2]); distsq = distsq + d * d
    with np.errstate(all="ignore"):
        vote = (mag[r, c] > 0) & (distsq < F(radius * radius) + F(0.5))
        b = ori_bin(ori[r, c][vote])
    return b[(b >= 0) & (b <= 36)]


def bin_centre_angles():
    """the angles a peak with equal neighbours gets (interp == 0): the main one, float throughout (orientation_cpu.cl:138),
    and the further ones, whose `/ 36.0` is a double division (:166)"""
    b = np.arange(36, dtype=F)
    main = (TWO_PI_F * (b + F(0.5))) / F(36) - PI_F
    extra = ((TWO_PI_F * (b + F(0.5))).astype(np.float64) / 36.0 - float(PI_F)).astype(F)
    return main.astype(F), extra


def desc_radius(sigma_oct, octsize):
    """(R, spacing) of a descriptor window in float32 (keypoints_cpu.cl:57-62)"""
    spacing = F(F(sigma_oct) / F(octsize)) * F(3.0)
    return int(F(F(F(1.414) * spacing) * F(2.5)) + F(0.5)), spacing


def desc_samples(k, octsize, mag, ori, sincos=None):
    """Every sample of an oriented keypoint's (x, y, sigma*oct, angle) window that passes the `inside` test
    (keypoints_cpu.cl:64-89), in float32: a dict of arrays rx, cx, o (after the loops), loops (iterations of the two
    `while` together), oval, oi, ri, ci, rf, cf, of, mag, ori.  `sincos`: the oracle's (angle -> (sin, cos)); numpy's differ in
    the last bit for a generic angle, not for 0."""
    H, W = mag.shape
    row, col, angle = F(k[1]) / F(octsize), F(k[0]) / F(octsize), F(k[3])
    irow, icol = int(row + F(0.5)), int(col + F(0.5))
    sine, cosine = sincos(angle) if sincos else (np.sin(angle), np.cos(angle))
    sine, cosine = F(sine), F(cosine)
    R, spacing = desc_radius(k[2], octsize)
    drow, dcol = row - F(irow), col - F(icol)
    i, j = np.meshgrid(np.arange(-R, R + 1), np.arange(-R, R + 1), indexing="ij")
    fi, fj = i.astype(F), j.astype(F)
    with np.errstate(all="ignore"):
        rx = ((cosine * fi - sine * fj) - drow) / spacing + F(1.5)
        cx = ((sine * fi + cosine * fj) - dcol) / spacing + F(1.5)
        yy, xx = irow + i, icol + j
        ins = (rx > -1) & (rx < 4) & (cx > -1) & (cx < 4) & (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        rx, cx, yy, xx = rx[ins], cx[ins], yy[ins], xx[ins]
        o = ori[yy, xx] - angle
        loops = np.zeros(o.shape, np.int64)
        for _ in range(8):
            m = o > TWO_PI_F
            o = np.where(m, o - TWO_PI_F, o); loops += m
        for _ in range(8):
            m = o < 0
            o = np.where(m, o + TWO_PI_F, o); loops += m
        oval = (F(4) * o) * ONE_PI_F
        fl = lambda v: np.trunc(np.where(v >= 0, v, v - F(1)))
        ri, ci, oi = fl(rx), fl(cx), fl(oval)
    return dict(rx=rx, cx=cx, o=o, loops=loops, oval=oval, oi=oi, ri=ri, ci=ci, rf=rx - ri, cf=cx - ci, of=oval - oi,
                mag=mag[yy, xx], ori=ori[yy, xx], yy=yy, xx=xx)


# ----------------------------------------------------------------------------- keypoint lists
def rounding_sigmas(ori_sigma, radii=(1, 2, 4, 5, 7, 10)):
    """keypoint sigmas s for which (int)(float)(sigma * 3.0f) and (int)((double)sigma * 3.0) differ, sigma = ori_sigma * s in
    float: found by search around radius / (3 ori_sigma)"""
    out = []
    for radius in radii:
        s = F(radius / (3.0 * ori_sigma))
        for _ in range(8):
            s = np.nextafter(s, F(np.inf))
        for _ in range(17):
            sigma = F(ori_sigma) * s
            if int(sigma * F(3)) != int(float(sigma) * 3.0):
                out.append(s)
                break
            s = np.nextafter(s, F(0))
    return out


def feature_centres(family, shape):
    """(row, col) of the family's crafted features per detection scale (where it has any)"""
    H, W = shape
    if family == "bump":
        return bump_sites(shape)
    if family == "bumps":
        return [[(r, c) for r, c, _ in bumps_sites(shape)[:2]]] * 3
    if family == "step":
        return [[(H // 2, W // 2)], [(H // 3, 7)], [(H // 2, W - 3)]]
    if family == "nanpix":
        return [[nan, inf, big, (nan[0] + 1, nan[1] + 2), (H // 2, W // 2)] for nan, inf, big in nanpix_sites(shape)]
    return [[(H // 2, W // 2)]] * 3


def _centres(family, shape):
    """[(row, col, detection scale)]: on and half a pixel off the features, nextafter(0.5, 0), the last usable row and
    column, the corners"""
    H, W = shape
    out = []
    for s, sites in enumerate(feature_centres(family, shape)):
        for r, c in sites:
            out += [(r, c, s + 1), (r + 0.5, c, s + 1), (r, c + 0.5, s + 1), (r + 0.5, c + 0.5, s + 1), (r - 0.5, c - 1.0, s + 1)]
    hb = float(HALF_BELOW)
    out += [(hb, 10.0, 1), (10.0, hb, 2), (hb, hb, 3), (9.0 + hb, 20.0 + hb, 1),
            (H - 2.0, W - 2.0, 1), (H - 2.0, 6.25, 2), (7.75, W - 2.0, 3), (0.0, 0.0, 1), (H - 1.0, W - 1.0, 2), (0.0, W - 1.0, 3)]
    return out


def orientation_keypoints(family, shape=SHAPE):
    """(kps (n, 4) float32 rows (peak, row, col, sigma), detection scales (n,) int32), the same list for every ori_sigma"""
    H, W = shape
    rows, ss = [], []
    for r, c, s in _centres(family, shape):
        for sg in (0.05, 0.3, 0.7, 1.6):                   # ori_sigma 1.5: radius 0, 1, 3, 7
            rows.append((12.0, r, c, sg)); ss.append(s)
    if family == "bumps":                                  # the sweep: exactly the five-pixel window on every pair
        for r, c, _ in bumps_sites(shape):
            for s in (1, 2, 3):
                rows.append((12.0, r, c, float(BUMPS_SIGMA))); ss.append(s)
    for n, sg in enumerate((0.01, 0.2223, 2.5, 6.0, 12.0, 30.0)):       # ... up to a radius beyond the plane
        for r, c in [(H / 2.0, W / 2.0), (H - 2.0, 2.5), (1.25, W - 3.0)]:
            rows.append((12.0, r, c, sg)); ss.append(1 + n % 3)
    n = 0
    for osg in ORI_SIGMAS:
        for sg in rounding_sigmas(osg):
            for r, c in [(H / 2.0, W / 2.0), (H / 2.0 + 0.5, W / 4.0)]:
                rows.append((12.0, r, c, float(sg))); ss.append(1 + n % 3); n += 1
    kps = np.array(rows, F)
    ss = np.array(ss, np.int32)
    holes = np.arange(3, len(kps), 11)                     # discarded rows among them (row -1: both kernels skip them)
    kps = np.insert(kps, holes, np.array([12.0, -1.0, 20.0, 2.0], F), axis=0)
    ss = np.insert(ss, holes, 2)
    check_orientation_list(kps, ss, shape)
    return np.ascontiguousarray(kps), np.ascontiguousarray(ss)


def power_of_two_sigmas():
    """sigma / octsize whose spacing (sigma / octsize * 3.0f) is 0.5, 1, 2, 4: rx, cx then land exactly on -1, 0, ..., 4"""
    out = []
    for sp in (0.5, 1.0, 2.0, 4.0):
        s = F(sp / 3.0)
        assert s * F(3) == F(sp)
        out.append(s)
    return out


def descriptor_keypoints(family, octsize, shape=SHAPE, seed=0):
    """(kk (n, 4) float32 rows (x, y, sigma * oct, angle), detection scales (n,) int32) for an octave of size `octsize`"""
    planes = crafted_planes(family, shape, seed)
    pi = PI_F
    fixed = [F(0), F(-0.0), pi, -pi, pi / F(2), -pi / F(2), pi / F(4), -pi / F(4), F(3) * pi / F(4), F(0.3)]
    special = []                                           # per detection scale: angles that wrap the plane's own orientations
    for p in planes:
        ang = []
        for a0 in frequent_orientations(p, top=2):
            a = a0 - TWO_PI_F
            if a0 - a == TWO_PI_F:                         # o == 2 pi_f for every sample of orientation a0, o > 2 pi_f for others
                ang.append(a)
            ang.append((a0 + TWO_PI_F) + F(1))             # o < -2 pi: two additions
        special.append(ang)
    sig = [float(s) for s in power_of_two_sigmas()] + [0.01, 0.05, 1.6, 3.1]       # (0.01, 0.05: R = 0, the window is one sample)
    rows, ss = [], []
    n = 0
    for m, (r, c, s) in enumerate(_centres(family, shape)):
        for sg in sig[m % 2::2]:
            angles = [fixed[n % len(fixed)], fixed[(n + 3) % len(fixed)]] + special[s - 1]
            n += 1
            for a in angles:
                rows.append((c * octsize, r * octsize, sg * octsize, float(a))); ss.append(s)
    kk = np.array(rows, F)
    ss = np.array(ss, np.int32)
    holes = np.arange(5, len(kk), 13)                      # holes of an oriented list (y < 0): an all-zero record
    kk = np.insert(kk, holes, np.array([10.0, -1.0, 2.0, 0.5], F), axis=0)
    ss = np.insert(ss, holes, 1)
    check_descriptor_list(kk, ss, octsize)
    return np.ascontiguousarray(kk), np.ascontiguousarray(ss)


# ----------------------------------------------------------------------------- the limits on the lists
def check_orientation_list(kps, ss, shape):
    H, W = shape
    kps = np.asarray(kps)
    assert kps.dtype == F and kps.ndim == 2 and kps.shape[1] == 4 and len(ss) == len(kps)
    assert np.isfinite(kps).all(), "a non-finite keypoint field"
    assert (kps[:, 3] > 0).all(), "sigma must be positive"
    assert ((ss >= 1) & (ss <= 3)).all(), "detection scales 1..3 (the MAPS forms hold no other map)"
    assert (np.abs(kps[:, 1:3]) < 4096).all() and (kps[:, 3] < 1000).all()
    for osg in ORI_SIGMAS:
        for k in kps:
            row, col, radius = ori_window(k, osg)
            wc = min(col + radius, W - 2) - max(0, col - radius) + 1
            hr = min(row + radius, H - 2) - max(0, row - radius) + 1
            assert wc < 4096 and max(wc, 0) * max(hr, 0) < 2 ** 22          # orientation_kernel: div_exact, the batch index


def check_descriptor_list(kk, ss, octsize):
    kk = np.asarray(kk)
    assert kk.dtype == F and kk.ndim == 2 and kk.shape[1] == 4 and len(ss) == len(kk)
    assert np.isfinite(kk).all(), "a non-finite keypoint field (a non-finite angle never leaves the reference's while loops)"
    assert (kk[:, 2] > 0).all(), "sigma must be positive"
    assert ((ss >= 1) & (ss <= 3)).all()
    assert (np.abs(kk[:, 3]) < 16).all() and (np.abs(kk[:, :2]) < 4096 * octsize).all()
    assert max(desc_radius(k[2], octsize)[0] for k in kk) <= DESC_MAXRAD, "a window beyond the row tables (desc_rows_fit)"
