"""Crafted cases for the affine warp (siftmi_plan_transform: transform_kernel / transform_rgb_kernel in csrc/k_align.hpp), shared
by tests/test_warp_ref_host.py (numpy restatement against the oracle and the golden vectors) and tests/test_gpu_warp_cases.py
(the kernels against the restatement).  A case names its image, its map and its output shape, and states what it is there for
as class counts of warp_ref (tests/warp_ref.py: CLASSES) that both tests assert, so that a case cannot silently stop reaching
its path.

The matrix acts on (y, x):  ty = m0 * y + m1 * x + off0,  tx = m2 * y + m3 * x + off1.

numpy only, deterministic from seeds, nothing here imports the package.
"""
import collections
import functools
import math

import numpy as np

F = np.float32
SHAPE = (40, 53)                 # H, W of the main plane: odd width, not square, a zero remainder in no tile size
OUT = (47, 59)                   # its usual output: 177 bytes per RGB row, so the rows take every alignment mod 4
SMALL = (16, 21)                 # plane of the output-shape family
BIG = (300, 403)                 # the one large RGB plane
TINY = [(1, 1), (1, 9), (9, 1), (2, 2), (3, 70), (13, 13)]                      # (3, 70) and below: plans without an octave
OUT_WIDTHS = [1, 2, 3, 4, 5, 6, 7, 8, 63, 64, 65, 255, 256, 257, 259, 1030]     # 4 pixels per RGB thread, 64 / 256 per workgroup
OUT_HEIGHTS = [1, 3, 4, 5]                                                      # 4 rows per workgroup
MODES = [1, 0, 2, -1, 256 + 1]                                                  # only exactly 1 is bilinear
FILLS = [0.0, 13.7, 254.999, 255.0]
HALF_BELOW = float(np.nextafter(F(0.5), F(0)))                                  # 0.49999997

#: name, family (1..8), image key for image(), matrix[4], offset[2], fill, mode, (OH, OW), {class: (">=" | "<=" | "==", count)}
Case = collections.namedtuple("Case", "name family image M off fill mode out_shape expect")


@functools.lru_cache(maxsize=None)
def image(key):
    """the input plane of a case, read-only.  key = (kind, (H, W)): "gray" float32 noise in [-100, 400), "rgb" uint8 noise,
    "sat" RGB runs of 0 and 255 with a few 1 / 254 (interpolants just under an integer), "special" gray with -0.0, denormals,
    infinities, NaN and FLT_MAX planted"""
    kind, (H, W) = key
    rng = np.random.default_rng(1000 * H + W + len(kind))
    if kind == "gray":
        a = (rng.random((H, W), dtype=F) * F(500) - F(100)).astype(F)
    elif kind == "rgb":
        a = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    elif kind == "sat":
        a = np.repeat(rng.choice(np.array([0, 255, 255, 0, 1, 254], np.uint8), (H, (W + 2) // 3, 3)), 3, axis=1)[:, :W]
        a = np.ascontiguousarray(a)
    elif kind == "special":
        a = (rng.random((H, W), dtype=F) * F(2) - F(1)).astype(F)
        tiny = np.finfo(F).tiny
        vals = [-0.0, tiny / 4, -tiny / 8, float(np.nextafter(F(0), F(1))), np.inf, -np.inf, np.nan, np.finfo(F).max, -np.finfo(F).max]
        spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H - 2, W - 2)]
        spots += [(int(y), int(x)) for y, x in zip(rng.integers(1, H - 1, 40), rng.integers(1, W - 1, 40))]
        for k, (y, x) in enumerate(spots):
            a[y, x] = F(vals[k % len(vals)])
        a[5, 5:8] = [np.inf, -np.inf, np.nan]                    # neighbours: inf - inf and inf * 0 inside one interpolant
        a[9, 9:11] = [np.finfo(F).max, np.finfo(F).max]          # the mix of two FLT_MAX overflows nowhere: the weights sum to 1
        a[12:14, 12:15] = np.array([[3, 5, -7], [11, -13, 17]], F) * F(tiny / 64)            # a block whose interpolants stay denormal
    else:
        raise KeyError(kind)
    a.setflags(write=False)
    return a


def rotation(deg, shape):
    """(M, off) of the rotation by `deg` degrees about the centre of a plane of `shape`"""
    H, W = shape
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    return [c, -s, s, c], [cy - c * cy + s * cx, cx - s * cy - c * cx]


def _maps(shape):
    """family 1: [(name, M, off, out_shape, expect)]"""
    H, W = shape
    T = (OUT[1], OUT[0])                                                    # transposed output for the quarter turns
    r30, r45 = rotation(30, shape), rotation(45, shape)
    return [
        ("identity", [1, 0, 0, 1], [0, 0], OUT, {"inside": ("==", H * W), "cut_inside": ("==", 0), "xedge": ("==", H - 1), "yedge": ("==", W - 1), "corner": ("==", 1)}),
        ("rot90", [0, 1, -1, 0], [0, W - 1], T, {"inside": ("==", H * W)}),
        ("rot180", [-1, 0, 0, -1], [H - 1, W - 1], OUT, {"inside": ("==", H * W)}),
        ("rot270", [0, -1, 1, 0], [H - 1, 0], T, {"inside": ("==", H * W)}),
        ("rot30", r30[0], r30[1], OUT, {"inside": (">=", 1000)}),
        ("rot45", r45[0], r45[1], OUT, {"inside": (">=", 1000)}),
        ("flipx", [1, 0, 0, -1], [0, W - 1], OUT, {"inside": ("==", H * W)}),
        ("flipy", [-1, 0, 0, 1], [H - 1, 0], OUT, {"inside": ("==", H * W)}),
        # every output pixel lands in the last 2 x 3 pixels of the image: the byte-wise tap loads of the RGB kernel
        ("zoom_corner", [1 / 64, 0, 0, 1 / 64], [H - 1.4, W - 2.3], OUT,
         {"last2": (">=", 100), "frac_x_at_last2": (">=", 50), "wide1off": (">=", 100), "inside": ("==", OUT[0] * OUT[1])}),
        ("zoom_out", [3.75, 0, 0, 2.5], [-20.5, -30.25], OUT, {"inside": (">=", 100)}),
        ("shear", [1, 0.3, 0.4, 1], [-8.0, -10.0], OUT, {"inside": (">=", 1000)}),
        ("zero", [0, 0, 0, 0], [H - 1, W - 1], OUT, {"corner": ("==", OUT[0] * OUT[1])}),
        ("rank1", [0.5, 0.25, 1.0, 0.5], [1.5, 2.25], OUT, {"inside": (">=", 500)}),
    ]


def _lattice(shape):
    """family 2: coefficients and offsets in quarters, so tx and ty are exact.  [(name, M, off, out_shape, expect)]"""
    H, W = shape
    q = [0.25, 0, 0, 0.25]
    out = (H + 7, W + 6)
    edge = H + W - 1                                                        # output pixels of the last row or column of an H x W output
    return [
        # t = -0.25, 0, 0.25, ... from the first pixel on
        ("lo_lo", q, [-0.25, -0.25], OUT, {}),
        # t = size - 1.25, size - 1, size - 0.75, size - 0.5, size - 0.25, size, ...
        ("hi_hi", q, [H - 1.25, W - 1.25], OUT, {"corner": ("==", 4), "xedge": ("==", 2), "yedge": ("==", 2), "cut_inside": ("==", 16)}),
        ("lo_hi", q, [-0.25, W - 1.25], OUT, {"xedge": (">=", 80)}),
        ("hi_lo", q, [H - 1.25, -0.25], OUT, {"yedge": (">=", 80)}),
        # -0.0: a negative unit coefficient times index 0, plus a -0.0 product, plus a -0.0 offset
        ("neg_zero_both", [-1, -0.0, -0.0, -1], [-0.0, -0.0], OUT, {"inside": ("==", 1)}),
        ("neg_zero_x", [1, -0.0, -0.0, -1], [-0.0, -0.0], OUT, {"inside": ("==", H)}),
        # x + 0.49999997 rounds to x + 0.5 from x = 1 on (half an ulp of [1, 2) is 2^-24, the offset lacks 2^-25), so the last
        # row and column are cut exactly as with 0.5; computed in one rounding or in double, nothing would be cut
        ("half", [1, 0, 0, 1], [0.5, 0.5], shape, {"cut_inside": ("==", edge), "inside": ("==", H * W)}),
        ("half_below", [1, 0, 0, 1], [HALF_BELOW, HALF_BELOW], shape, {"cut_inside": ("==", edge), "inside": ("==", H * W)}),
        ("half_wide", [1, 0, 0, 1], [0.5, HALF_BELOW], out, {"cut_inside": ("==", edge), "inside": ("==", H * W)}),
    ]


#: values the lattice family must produce in tx (of width W) and ty (of height H), as offsets from the size or None
LATTICE_VALUES = [("abs", -0.25), ("abs", -0.0), ("abs", 0.0), ("rel", -1.0), ("rel", -0.75), ("rel", -0.5), ("rel", -0.25), ("rel", 0.0)]


def _nonfinite():
    """family 4: [(name, M, off)]; the output is `fill` except where the map happens to be finite and inside"""
    nan, inf = float("nan"), float("inf")
    return [
        ("nan_coeff", [1, 0, nan, 1], [0, 0]),
        ("inf_coeff", [1, inf, 0, 1], [0, 0]),
        ("ninf_offset", [1, 0, 0, 1], [0, -inf]),
        ("huge_cancel", [1, 0, 0, 3e9], [0, -3e9]),              # tx = 0 in column 1, +-3e9 beside it: no int32 holds that
        ("all_1e30", [1e30, -1e30, -1e30, 1e30], [1e30, -1e30]),
        ("nan_offset", [1, 0, 0, 1], [nan, 0]),
    ]


@functools.lru_cache(maxsize=None)
def cases():
    """every case, in a fixed order"""
    out = []

    def add(name, family, img, M, off, fill, mode, out_shape, expect=None):
        out.append(Case("f%d-%s-%s-m%d" % (family, name, img[0], mode), family, img, tuple(float(v) for v in M), tuple(float(v) for v in off),
                        float(fill), int(mode), tuple(out_shape), dict(expect or {})))

    gray, rgb = ("gray", SHAPE), ("rgb", SHAPE)
    for name, M, off, oshape, expect in _maps(SHAPE):                                     # 1: map families
        for img in (gray, rgb):
            for mode in (1, 0):
                add(name, 1, img, M, off, 13.0, mode, oshape, expect)
    r30big = rotation(30, BIG)
    add("rot30_big", 1, ("rgb", BIG), r30big[0], r30big[1], 7.0, 1, (303, 1030), {"inside": (">=", 100000)})
    for name, M, off, oshape, expect in _lattice(SHAPE):                                  # 2: boundary lattice
        for img in (gray, rgb):
            for mode in (1, 0):
                add(name, 2, img, M, off, 13.0, mode, oshape, expect)
    r30 = rotation(30, SHAPE)
    for img in (gray, rgb):                                                               # 3: modes
        for mode in MODES:
            add("mode", 3, img, r30[0], r30[1], 13.0, mode, OUT)
    for name, M, off in _nonfinite():                                                     # 4: non-finite and huge maps
        for img in (gray, rgb):
            for mode in (1, 0):
                add(name, 4, img, M, off, 13.0, mode, OUT, {"inside": ("<=", OUT[0] + OUT[1])})
    r30s = rotation(30, SMALL)
    shapes5 = [(oh, ow) for ow in OUT_WIDTHS for oh in OUT_HEIGHTS] + [(19, 30), (33, 22), (7, 5)]
    for name, M, off in (("ident", [1, 0, 0, 1], [0, 0]), ("rot30", r30s[0], r30s[1])):   # 5: output shapes
        for img in (("gray", SMALL), ("rgb", SMALL)):
            for oshape in shapes5:
                add("%s_%dx%d" % (name, oshape[0], oshape[1]), 5, img, M, off, 13.0, 1, oshape)
    for shape in TINY:                                                                    # 6: smallest planes
        H, W = shape
        for img in (("gray", shape), ("rgb", shape)):
            add("ident_%dx%d" % shape, 6, img, [1, 0, 0, 1], [0, 0], 13.0, 1, (H + 2, W + 3), {"inside": ("==", H * W)})
            add("ident_%dx%d" % shape, 6, img, [1, 0, 0, 1], [0, 0], 13.0, 0, (H + 2, W + 3), {"inside": ("==", H * W)})
            add("quarter_%dx%d" % shape, 6, img, [0.25, 0, 0, 0.25], [-0.25, -0.25], 13.0, 1, (4 * H + 4, 4 * W + 5), {"inside": ("==", 16 * H * W)})
            add("rot180_%dx%d" % shape, 6, img, [-1, 0, 0, -1], [H - 0.75, W - 0.75], 13.0, 1, (H + 1, W + 2), {"inside": ("==", H * W)})
    shift = ([1, 0, 0, 1], [0.999, 0.001])
    for fill in FILLS:                                                                    # 7: RGB value domain
        tag = ("%g" % fill).replace(".", "p")
        add("shift_fill%s" % tag, 7, ("sat", SHAPE), shift[0], shift[1], fill, 1, OUT)
        add("rot30_fill%s" % tag, 7, ("sat", SHAPE), r30[0], r30[1], fill, 1, OUT)
        add("rot30_fill%s" % tag, 7, ("rgb", SHAPE), r30[0], r30[1], fill, 1, OUT)
    for off in ([0.5, 0.5], [-0.5, 0.5], [0.25, -0.75]):                                  # 8: special values in a gray image
        tag = "%g_%g" % tuple(off)
        add("special_%s" % tag, 8, ("special", SHAPE), [1, 0, 0, 1], off, 13.0, 1, OUT)
    add("special_copy", 8, ("special", SHAPE), [1, 0, 0, 1], [0, 0], 13.0, 0, OUT)
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def by_name(name):
    return next(c for c in cases() if c.name == name)


def is_rgb(case):
    return case.image[0] in ("rgb", "sat")


def check_expect(case, counts):
    for cls, (op, n) in case.expect.items():
        got = counts[cls]
        ok = got >= n if op == ">=" else (got <= n if op == "<=" else got == n)
        assert ok, "%s: %s = %d, the case promises %s %d" % (case.name, cls, got, op, n)


#: the representative cases of the pointer-path tests: last-corner zoom, 30-degree rotation, identity
POINTER_CASES = ["f1-zoom_corner-%s-m1", "f1-rot30-%s-m1", "f1-identity-%s-m1"]
