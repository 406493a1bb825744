"""Shared helpers for the test-suite: synthetic inputs and order-insensitive comparison."""
import numpy as np

dtype_kp = np.dtype([("x", np.float32), ("y", np.float32), ("scale", np.float32), ("angle", np.float32),
                     ("desc", (np.uint8, 128))])


def white_noise(shape, seed=0):
    return np.random.default_rng(seed).random(shape, dtype=np.float32)


def smooth_noise(shape, seed=3, sigma=3.0):
    import scipy.ndimage as ndi
    return ndi.gaussian_filter(np.random.default_rng(seed).random(shape), sigma).astype(np.float32)


def lattice(shape, period=7, sigma=2.0, seed=11, jitter=1):
    """Alternating-sign Gaussian blobs on a jittered square grid: about one DoG extremum per 36 samples."""
    import scipy.ndimage as ndi
    rng = np.random.default_rng(seed)
    H, W = shape
    ys, xs = np.arange(period // 2, H, period), np.arange(period // 2, W, period)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    sign = np.where((np.arange(len(ys))[:, None] + np.arange(len(xs))[None, :]) % 2 == 0, 1.0, -1.0)
    yy = np.clip(yy + rng.integers(-jitter, jitter + 1, yy.shape), 0, H - 1)
    xx = np.clip(xx + rng.integers(-jitter, jitter + 1, xx.shape), 0, W - 1)
    img = np.zeros(shape, np.float64)
    img[yy, xx] = sign * (0.6 + 0.4 * rng.random(yy.shape))
    return ndi.gaussian_filter(img, sigma).astype(np.float32)


def multiscale_noise(shape, seed=5):
    import scipy.ndimage as ndi
    rng = np.random.default_rng(seed)
    base = rng.random(shape)
    return sum(ndi.gaussian_filter(base, s) * s for s in (1, 2, 4, 8)).astype(np.float32)


def rectangles(shape, seed=7, n=60):
    rng = np.random.default_rng(seed)
    img = np.zeros(shape, np.float32)
    H, W = shape
    for _ in range(n):
        y0, x0 = rng.integers(0, H - 4), rng.integers(0, W - 4)
        h, w = rng.integers(3, max(4, H // 3)), rng.integers(3, max(4, W // 3))
        img[y0:y0 + h, x0:x0 + w] += rng.random()
    return img


# ---- synthetic keypoint lists of the per-keypoint stages (tests/test_gpu_parity.py, tests/test_gpu_keypoint_forms.py)
def descriptor_edge_rows(W, H, octsize):
    """Oriented keypoints (x, y, sigma, angle) of an octave of size `octsize` chosen to stress the row-interval descriptor
    form (k_descriptor.hpp): window axes on and a hair off the pixel axes and diagonals (rows that start / end exactly on a
    cell boundary, the short rows at the corners of a 45-degree window), window radius 4 ... 126, centres on, next to and
    beyond the borders of a W x H plane (clipped rows, empty rows, empty windows), sub-pixel offsets of exactly one half."""
    pi = float(np.float32(np.pi))
    angles = []
    for a in (0.0, pi / 4, pi / 2, 3 * pi / 4, pi, -pi / 4, -pi / 2, -3 * pi / 4, -pi):
        for eps in (0.0, 1e-6, -1e-6, 1e-3):
            angles.append(np.float32(a + eps))
    angles += [np.float32(0.3), np.float32(-2.9), np.float32(1.1), np.float32(2.5)]
    sigmas = [0.8, 1.6, 2.2, 3.17, 4.5, 7.0, 11.9]          # window radius 4 ... 126 pixels of the octave
    centres = [(210.0, 150.0), (210.5, 150.5), (3.0, 4.0), (0.0, 0.0), (W - 1.0, H - 1.0), (W - 2.5, 40.25), (60.75, H - 1.5),
               (-6.0, 100.0), (W + 9.0, H + 9.0), (200.0, -3.0)]
    rows = []
    k = 0
    for sg in sigmas:
        for (cx, cy) in centres:
            for j in range(4):
                ang = angles[k % len(angles)]; k += 1
                rows.append((cx * octsize, cy * octsize, sg * octsize, ang))
    for ang in angles:                                      # every angle once on the mid-size window in the middle of the plane
        rows.append((123.25 * octsize, 77.75 * octsize, 2.9 * octsize, ang))
    return np.ascontiguousarray(np.array(rows, np.float32))


def descriptor_random_rows(seed, W, H, octsize, n=3000):
    """n random oriented keypoints of an octave of size `octsize`: uniform centres up to 8 pixels beyond a W x H plane,
    log-uniform sigma from the smallest window to R = 126, uniform angle in [-pi, pi] (and exactly pi, -pi, 0 every 97th)."""
    rng = np.random.default_rng(seed)
    kk = np.empty((n, 4), np.float32)
    kk[:, 0] = rng.uniform(-8, W + 8, n) * octsize
    kk[:, 1] = rng.uniform(-8, H + 8, n) * octsize
    kk[:, 2] = np.exp(rng.uniform(np.log(0.4), np.log(11.9), n)) * octsize
    kk[:, 3] = rng.uniform(-np.pi, np.pi, n)
    kk[::97, 3] = np.float32(np.pi); kk[1::97, 3] = -np.float32(np.pi); kk[2::97, 3] = 0.0
    return kk


def orientation_border_rows(W, H):
    """Refined keypoints (peak, row, col, sigma) whose orientation windows are clipped by every border and corner of a
    W x H plane: sigma 0.5 ... 8 (radius 2 ... 36), centres on half-pixel positions."""
    rows = []
    for sg in (0.5, 1.0, 1.6, 2.5, 4.5, 8.0):
        for (r, c) in [(150.0, 210.0), (150.5, 210.5), (0.0, 0.0), (1.0, 2.0), (H - 1.0, W - 1.0), (H - 2.0, 3.0), (5.25, W - 1.75),
                       (H / 2.0, 0.0), (0.0, W / 2.0), (H - 1.0, W / 2.0), (77.75, 123.25)]:
            rows.append((12.0, r, c, sg))
    return np.ascontiguousarray(np.array(rows, np.float32))


def sort_kp(k):
    """Keypoint order is unspecified (atomic append in the reference, plan.py:3.2): compare sorted."""
    k = np.asarray(k)
    key = np.lexsort((k["desc"][:, 1], k["desc"][:, 0], k["angle"], k["scale"], k["y"], k["x"]))
    return k[key]


def assert_same_keypoints(a, b, what=""):
    """Bit-exact equality of two keypoint sets after sorting."""
    assert len(a) == len(b), "%s: %d vs %d keypoints" % (what, len(a), len(b))
    a, b = sort_kp(a), sort_kp(b)
    for f in ("x", "y", "scale", "angle"):
        fa, fb = a[f].view(np.uint32), b[f].view(np.uint32)
        bad = np.nonzero(fa != fb)[0]
        assert bad.size == 0, "%s: field %s differs at %d rows, e.g. %r vs %r" % (
            what, f, bad.size, a[f][bad[:3]], b[f][bad[:3]])
    bad = np.nonzero((a["desc"] != b["desc"]).any(axis=1))[0]
    assert bad.size == 0, "%s: descriptors differ in %d rows" % (what, bad.size)


def sort_rows(a):
    a = np.asarray(a)
    return a[np.lexsort(a.T[::-1])]


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, np.int64(-2 ** 31) - a, a)
    b = np.where(b < 0, np.int64(-2 ** 31) - b, b)
    return np.abs(a - b)


def compare_keypoints_libm(a, b, what="", max_bad_rows=0.002, angle_abs=0.02, desc_lsb=6, scale_ulp=2):
    """Comparison against the glibc-backed native build of the reference kernels (oracle/_ref/libsiftclref.so).

    OpenCL leaves the last bits of exp / atan2 / pow to the implementation; the oracle's siftmath is correctly rounded
    (within 2^-48 of a rounding boundary), glibc 2.35's atan2f / powf are not.  Measured at 2048 x 2048 / 1031 x 1537
    (tests/test_oracle_vs_ref.py::test_glibc_build_tolerance, 60 k keypoints): count, x and y identical; scale within
    2 ulp; angle and descriptor identical in > 99.9 % of the rows.  In the remaining rows a 1-ulp atan2 difference
    moved one window sample across an orientation-bin edge (orientation_cpu.cl:88), which shifts the interpolated
    angle by up to 1.3e-2 rad and, through it, a few descriptor bins by up to 5 LSB (the measured worst cases; the bounds
    asserted here, 2e-2 rad and 6 LSB, leave a small margin and no more).  That is far inside what the reference's own
    test accepts (test/test_keypoints.py: angle < 1e-1).  With the math builtins bound to siftmath
    instead of glibc the reference kernels reproduce the oracle byte for byte (assert_same_keypoints).
    Returns a dict of the measured differences."""
    assert len(a) == len(b), "%s: %d vs %d keypoints" % (what, len(a), len(b))
    a, b = sort_kp(a), sort_kp(b)
    assert np.array_equal(a["x"].view(np.uint32), b["x"].view(np.uint32)), what + ": x differs"
    assert np.array_equal(a["y"].view(np.uint32), b["y"].view(np.uint32)), what + ": y differs"
    ds, da = ulp_diff(a["scale"], b["scale"]), ulp_diff(a["angle"], b["angle"])
    assert ds.max(initial=0) <= scale_ulp, "%s: scale differs by %d ulp" % (what, ds.max())
    dabs = np.abs(a["angle"].astype(np.float64) - b["angle"].astype(np.float64))
    dabs = np.minimum(dabs, 2 * np.pi - dabs)
    assert dabs.max(initial=0) <= angle_abs, "%s: angle differs by %g rad" % (what, dabs.max())
    dd = np.abs(a["desc"].astype(np.int16) - b["desc"].astype(np.int16))
    assert dd.max(initial=0) <= desc_lsb, "%s: descriptor bins differ by %d" % (what, dd.max())
    bad = int(((ds > 0) | (da > 2) | (dd.max(axis=1) > 0)).sum()) if len(a) else 0     # scale differences count as well
    assert bad <= max(2, max_bad_rows * len(a)), "%s: %d of %d rows differ" % (what, bad, len(a))
    return dict(rows=len(a), rows_differing=bad, scale_ulp=int(ds.max(initial=0)), angle_ulp=int(da.max(initial=0)),
                angle_rad=float(dabs.max(initial=0)), desc_bins_differing=int((dd > 0).sum()), desc_lsb=int(dd.max(initial=0)))


def kp_digest(k):
    """Per-field SHA-256 of a sorted keypoint set: lets a 2048^2 result (5.6 MB of records) be pinned by ~400 bytes."""
    import hashlib
    k = sort_kp(k)
    out = {"n": int(len(k))}
    for f in ("x", "y", "scale", "angle", "desc"):
        out[f] = hashlib.sha256(np.ascontiguousarray(k[f]).tobytes()).hexdigest()
    return out


def oracle_pyramid(oracle, img, n_oct=1):
    """[(blurs (6, H, W), dogs (5, H, W))] of the first `n_oct` octaves of `img`, computed by the oracle's stage functions in the
    order of plan.py:525-539, 602-623, 740-745: normalise, initial blur, five blurs per octave, DoG, next octave = every second
    sample of blur[3]."""
    import math
    mn, mx = oracle.minmax(img)
    base = oracle.normalize(np.ascontiguousarray(img, np.float32), mn, mx)
    base = oracle.blur(base, oracle.gaussian_taps(math.sqrt(1.6 ** 2 - 0.25), 15))
    ratio = 2.0 ** (1.0 / 3.0)
    out = []
    for o in range(n_oct):
        blurs, prev = [base], 1.6
        for s in range(5):
            inc = prev * math.sqrt(ratio ** 2 - 1.0)
            size = int(math.ceil(8 * inc + 1)); size += (size % 2 == 0)
            blurs.append(oracle.blur(blurs[-1], oracle.gaussian_taps(inc, size)))
            prev *= ratio
        blurs = np.ascontiguousarray(np.stack(blurs))
        out.append((blurs, oracle.dog(blurs)))
        base = oracle.shrink(blurs[3])
    return out


_MULT = None


def kp_multiset_digest(k):
    """Order-independent 128-bit digest of a keypoint set (the sum over its records of two 64-bit multilinear hashes of the
    record's 18 quadwords): cheap enough to take thousands of times (the soak test), a changed, lost or doubled record changes it."""
    global _MULT
    if _MULT is None:
        rng = np.random.default_rng(12345)
        _MULT = (rng.integers(1, 2 ** 63, (2, 18), dtype=np.uint64) * np.uint64(2) + np.uint64(1))
    q = np.ascontiguousarray(np.asarray(k)).view(np.uint64).reshape(-1, 18)
    with np.errstate(over="ignore"):
        h = [int((q * _MULT[i]).sum(axis=1, dtype=np.uint64).sum(dtype=np.uint64)) for i in range(2)]
    return (len(q), h[0], h[1])


# name -> (maker, shape, kwargs): the large cases pinned by digest (tests/golden/kp_digests.json)
def digest_cases():
    return {"smooth2048": (smooth_noise, (2048, 2048), {}),
            "white2048": (white_noise, (2048, 2048), {}),
            "smooth1031x1537": (smooth_noise, (1031, 1537), dict(seed=9, sigma=2.0))}


# (matrix[4], offset[2], fill, mode, extra (dy, dx) added to the output shape or None) -- transform.cl cases
TRANSFORM_CASES = [
    ([1, 0, 0, 1], [0, 0], 0.0, 1, None),                       # identity: last row / column cut to fill
    ([1, 0, 0, 1], [3.25, -2.5], 7.0, 1, None),                 # pure shift, fractional
    ([1, 0, 0, 1], [-4.0, 6.0], 1.5, 1, None),                  # integer shift
    ([0.99, 0.02, -0.03, 1.01], [1.7, 4.2], 3.0, 1, None),      # small affine (the LinearAlign regime)
    ([0.5, 0, 0, 0.5], [10, 10], 2.0, 1, None),                 # zoom in
    ([1.3, 0.2, -0.1, 1.2], [-5.5, -7.25], 9.0, 1, None),       # zoom out: large fill area
    ([0.0, 1.0, 1.0, 0.0], [0.0, 0.0], 4.0, 1, None),           # transpose
    ([0.99, 0.02, -0.03, 1.01], [1.7, 4.2], 3.0, 0, None),      # nearest-lower mode
    ([1, 0, 0, 1], [-8.5, -6.25], 5.0, 1, (17, 13)),            # output larger than the input (extra margin)
]


def transform_inputs():
    gray = (smooth_noise((97, 131), seed=41, sigma=1.5) * 255.0).astype(np.float32)
    rgb = np.random.default_rng(42).integers(0, 256, (40, 53, 3), dtype=np.uint8)
    return gray, rgb


# ---- inputs of tests/test_oracle_vs_ref.py, shared with the generator of its fixture (tests/golden/make_ref_xcheck.py)
PIPELINE_CASES = [(21, (200, 333), True), (22, (160, 160), False), (23, (97, 211), True)]
XCHECK_SIGMAS = (0.8, 1.0, 2.2, 3.3, 5.0)


def pipeline_input(seed, shape, smooth):
    return smooth_noise(shape, seed=seed, sigma=2.5) if smooth else white_noise(shape, seed=seed)


def converter_inputs():
    """{dtype name: raw frame} of integer frames whose extremes and (float)x roundings the converters must reproduce,
    plus "rgb": an RGB uint8 frame."""
    rng = np.random.default_rng(12)
    H, W = 37, 53
    out = {}
    for name in ("uint8", "uint16", "uint32", "uint64", "int32", "int64"):
        info = np.iinfo(name)
        raw = rng.integers(info.min, info.max, (H, W), dtype=name, endpoint=True)
        raw.flat[:4] = [info.min, info.max, 0, min(info.max, 2 ** 24 + 1)]      # extremes, and the first odd integer f32 cannot hold
        out[name] = raw
    out["rgb"] = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return out


def transform_xcheck_cases():
    """[(name, image, matrix, offset, out_shape, fill, mode)]: twelve random affine warps of a float and an RGB image,
    both interpolation modes, plus a larger output shape."""
    rng = np.random.default_rng(77)
    img = (smooth_noise((150, 203), seed=78) * 1000.0 - 300.0).astype(np.float32)
    rgb = rng.integers(0, 256, (64, 81, 3), dtype=np.uint8)
    cases = []
    for k in range(12):
        M = (np.eye(2) + rng.normal(0, 0.08, (2, 2))).astype(np.float32).reshape(4)
        off = rng.normal(0, 12, 2).astype(np.float32)
        fill = float(rng.integers(0, 200))
        for mode in (1, 0):
            cases.append(("gray%d_mode%d" % (k, mode), img, M, off, None, fill, mode))
            cases.append(("rgb%d_mode%d" % (k, mode), rgb, M, off, None, fill, mode))
        cases.append(("gray%d_out180x230" % k, img, M, off, (180, 230), fill, 1))
    return cases


def matching_valid_inputs():
    """(a, b, roi): list 2 entirely on valid pixels of a random mask, list 1 anywhere, also beyond the array; 300 of
    list 2 are perturbed copies of list 1."""
    rng = np.random.default_rng(5)
    n1, n2, H, W = 600, 550, 90, 120
    a = np.zeros(n1, dtype_kp); b = np.zeros(n2, dtype_kp)
    a["desc"] = rng.integers(0, 256, (n1, 128), dtype=np.uint8); b["desc"] = rng.integers(0, 256, (n2, 128), dtype=np.uint8)
    idx = rng.permutation(n1)[:300]
    b["desc"][:300] = np.clip(a["desc"][idx].astype(int) + rng.integers(-6, 7, (300, 128)), 0, 255).astype(np.uint8)
    roi = (rng.random((H, W)) > 0.3).astype(np.int8)
    ys, xs = np.nonzero(roi)
    pick = rng.integers(0, len(ys), n2)
    b["x"] = xs[pick] + 0.4; b["y"] = ys[pick] + 0.6
    a["x"] = rng.random(n1) * W * 1.2; a["y"] = rng.random(n1) * H * 1.2
    return a, b, roi


def matching_valid_steps(b, roi):
    """The list-2 variants matched in turn, as (label, b): as generated; one masked-out list-2 keypoint; two of them;
    the second one moved beyond the array instead."""
    W = roi.shape[1]
    zy, zx = np.argwhere(roi == 0)[0]
    steps = [("plain", b.copy())]
    b = b.copy()
    b["x"][7] = zx + 0.5; b["y"][7] = zy + 0.5
    steps.append(("one_masked", b.copy()))
    b["x"][8] = zx + 0.5; b["y"][8] = zy + 0.5
    steps.append(("two_masked", b.copy()))
    b["x"][8] = W + 3.0
    steps.append(("one_beyond", b.copy()))
    return steps


def array_digest(a):
    """SHA-256 of an array's dtype, shape and bytes."""
    import hashlib
    a = np.ascontiguousarray(a)
    return hashlib.sha256(("%s %s|" % (a.dtype.str, a.shape)).encode() + a.tobytes()).hexdigest()


# ---- crafted planes of the detection stage (tests/test_gpu_detection_forms.py, tests/test_oracle_vs_ref.py)
# Every family is a set of five DoG planes of small integers (or quarters), turned into six blur planes by
# blur[5] = 64, blur[s] = blur[s + 1] + dog[s]: every sum and every subtraction blur[s] - blur[s + 1] is exact, so the
# kernels see the DoG planes as generated -- with equal samples everywhere, singular Hessians and values on the contrast
# threshold, which no blurred float image has.
DETECT_FAMILIES = ("iid", "blocks", "repeat", "equal+", "equal-", "spikes", "levels", "waves", "nan", "+inf", "-inf", "mixed")
DETECT_DENSE = ("iid", "repeat", "equal+", "equal-")     # families whose 62 x 4 strips overflow the parking buffer
SIFT_EXT_BUF = 128                                       # k_extrema.hpp: candidates a wave parks before it flushes


def detection_dogs(family, shape, seed=0):
    """(5, H, W) float32 DoG planes of one family."""
    rng = np.random.default_rng(1000 + seed)
    H, W = shape
    if family == "iid":                                   # ties everywhere, refinement moves up to the 3 / H - 3 limits
        d = rng.integers(-4, 5, (5, H, W))
    elif family == "blocks":                              # 3 x 3 plateaus: singular 3-D Hessians, inf / NaN steps
        d = np.repeat(np.repeat(rng.integers(-5, 6, (5, (H + 2) // 3, (W + 2) // 3)), 3, axis=1), 3, axis=2)[:, :H, :W]
    elif family == "repeat":                              # ties across scales, H00 = 0
        d = np.repeat(rng.integers(-4, 5, (1, H, W)), 5, axis=0)
    elif family in ("equal+", "equal-"):                  # every sample a candidate at the three scales: 186 per row and wave
        d = np.full((5, H, W), 4 if family == "equal+" else -4)
    elif family == "spikes":                              # isolated extrema on zero: val != 0
        d = np.where(rng.random((5, H, W)) < 0.02, rng.integers(3, 9, (5, H, W)) * rng.choice([-1, 1], (5, H, W)), 0)
    elif family == "levels":                              # the contrast threshold 0.8 * 3.4 = 2.72 from both sides
        d = rng.choice(np.array([0.0, 2.5, -2.5, 2.75, -2.75, 3.0, -3.0]), (5, H, W))
    elif family == "waves":                               # slanted ridges: the edge test drops a third, the two thresholds differ
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        d = np.stack([np.rint(6.0 * np.sin(0.9 * y + 0.9 * s + 0.3 * x) * np.cos(0.12 * x - 0.7 * s)) for s in range(5)])
    elif family in ("nan", "+inf", "-inf", "mixed"):      # 60 non-finite samples in iid planes
        d = rng.integers(-4, 5, (5, H, W)).astype(np.float32)
        bad = {"nan": [np.nan], "+inf": [np.inf], "-inf": [-np.inf], "mixed": [np.nan, np.inf, -np.inf]}[family]
        at = rng.choice(d.size, 60, replace=False)
        d.ravel()[at] = np.array(bad, np.float32)[np.arange(60) % len(bad)]
    else:
        raise ValueError(family)
    return np.ascontiguousarray(d, np.float32)


def blurs_from_dogs(dogs):
    """Six blur planes whose differences are `dogs` exactly (where finite): blur[5] = 64, blur[s] = blur[s + 1] + dog[s]."""
    blurs = np.empty((6,) + dogs.shape[1:], np.float32)
    blurs[5] = 64.0
    with np.errstate(invalid="ignore"):
        for s in range(4, -1, -1):
            blurs[s] = blurs[s + 1] + dogs[s]
    return blurs


def detection_planes(family, shape, seed=0):
    return blurs_from_dogs(detection_dogs(family, shape, seed))


def sort_rows_bits(a):
    """Rows sorted by their bit patterns (total order also with NaN / inf / -0 in them), returned as uint32."""
    a = np.ascontiguousarray(a, np.float32)
    u = a.view(np.uint32).reshape(len(a), a.shape[1] if a.ndim > 1 else 1)
    return u[np.lexsort(u.T[::-1])]


def detection_expected(local_maxmin, interp_keypoint, dogs, octsize, par, band=None):
    """What the detection stage must return, from the stage functions of a judge (the oracle's, or the reference's own
    kernels): (candidates (n, 4) of the three scales, their count per scale, refined rows (m, 5) = (peak, row, col, sigma,
    scale)).  band = (y_lo, y_hi): only the candidates of those rows."""
    _, H, W = dogs.shape
    cands = []
    for s in (1, 2, 3):
        k, n = local_maxmin(dogs, s, octsize, H * W, par)
        assert n <= H * W
        k = k[:n]
        if band is not None:
            k = k[(k[:, 1] >= band[0]) & (k[:, 1] < band[1])]
        cands.append(k)
    cand = np.ascontiguousarray(np.concatenate(cands))
    return cand, [len(k) for k in cands], refined_expected(interp_keypoint, dogs, cand, par)


def refined_expected(interp_keypoint, dogs, cand, par):
    """Refined rows (peak, row, col, sigma, scale) of the candidates that survive interp_keypoint (holes stay holes)."""
    cand = np.ascontiguousarray(cand, np.float32).reshape(-1, 4)
    if len(cand) == 0:
        return np.empty((0, 5), np.float32)
    interp = interp_keypoint(dogs, cand, 0, len(cand), par)
    with np.errstate(invalid="ignore"):
        keep = (cand[:, 1] != -1) & ~((interp[:, 0] == -1) & (interp[:, 1] == -1) & (interp[:, 2] == -1) & (interp[:, 3] == -1))
    return np.ascontiguousarray(np.concatenate([interp[keep], cand[keep][:, 3:4]], axis=1))


def strip_candidate_counts(cand, W, H, border, rows):
    """(ny, nx) candidates per extrema strip -- 62 columns x `rows` rows from (border, border), the three scales together."""
    nx, ny = (W - 2 * border + 61) // 62, (H - 2 * border + rows - 1) // rows
    counts = np.zeros((ny, nx), np.int64)
    np.add.at(counts, ((cand[:, 1].astype(np.int64) - border) // rows, (cand[:, 2].astype(np.int64) - border) // 62), 1)
    return counts
