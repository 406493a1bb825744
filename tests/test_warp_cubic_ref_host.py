"""CPU tests of the cubic sampler's row: the numpy restatement tests/warp_cubic_ref.py against what the
contract says must follow from it, the cases of tests/warp_cubic_cases.py against the class counts they promise, and the interface
(header, library and signature table agree on the four _ex entries, which refuse a null handle without a device; the keyword
`interp` is checked before anything is launched).  No kernel runs."""
import ctypes as C
import inspect
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import stack_ref
import warp_cases as wc
import warp_cubic_cases as cc
import warp_ref
from warp_cubic_ref import CLASSES, MUTANTS, samples_cubic, warp, warp_cubic_ref, weights

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ cases
@pytest.mark.parametrize("case", cc.cases(), ids=lambda c: c.name)
def test_every_case_reaches_what_it_promises(case):
    out, counts = warp_cubic_ref(wc.image(case.image), case.M, case.off, case.out_shape, case.fill)
    assert out.shape == case.out_shape and out.dtype == F and tuple(counts) == CLASSES
    cc.check_expect(case, counts)


def test_the_families_together_reach_every_class_and_every_lattice_value():
    total = dict.fromkeys(CLASSES, 0)
    for case in cc.cases():
        counts = warp_cubic_ref(wc.image(case.image), case.M, case.off, case.out_shape, case.fill)[1]
        for k, v in counts.items():
            total[k] += v
    assert all(total[k] > 0 for k in CLASSES), total
    H, W = wc.SHAPE
    seen_x, seen_y = set(), set()
    for name in ("c2-lo_lo", "c2-hi_hi"):
        case = cc.by_name(name)
        ty, tx = warp_ref.coords(case.M, case.off, case.out_shape)
        seen_x |= set(tx.ravel().tolist()); seen_y |= set(ty.ravel().tolist())
    for k in range(-1, 6):                       # -0.25 .. 1.25 and size - 2.25 .. size, in quarters
        assert k * 0.25 in seen_x and k * 0.25 in seen_y
    for k in range(0, 10):
        assert W - 2.25 + k * 0.25 in seen_x and H - 2.25 + k * 0.25 in seen_y
    assert len(cc.cases()) == len({c.name for c in cc.cases()}) and sum(c.family == 9 for c in cc.cases()) == 40


def test_stack_cases_cover_the_sizes_the_kernels_branch_on():
    sizes = {len(c.frames) for c in cc.stack_cases()}
    assert {cc.DEPTH - 1, cc.DEPTH, cc.DEPTH + 1, 2 * cc.DEPTH + 1, 1, 3, 4, 5, 8, 64, 65} <= sizes
    assert {c.family for c in cc.stack_cases()} >= set(cc.STACK_MAPS)
    assert all(c.mode == 1 for c in cc.stack_cases())
    for c in cc.stack_cases():
        if c.kind == "inf" or len(c.frames) > 64:
            assert "median" not in cc.reducers_of(c)
    assert all(c.kind != "inf" for c in cc.clip_stacks()) and len(cc.clip_stacks()) >= 20


# ---------------------------------------------------------------------------------------------------------------- weights
def test_weights_at_zero_and_at_the_quarters_are_exact():
    w = [v[()] for v in weights(F(0.0))]
    assert [float(v) for v in w] == [0.0, 1.0, 0.0, 0.0]
    assert [bool(np.signbit(v)) for v in w] == [True, False, False, True]                   # (-0, 1, 0, -0)
    exact = {0.25: (-9, 111, 29, -3), 0.5: (-8, 72, 72, -8), 0.75: (-3, 29, 111, -9)}       # / 128; at one half (-1, 9, 9, -1) / 16
    for f, want in exact.items():
        got = [float(v) for v in weights(F(f))]
        assert got == [k / 128.0 for k in want], (f, got)
        # and they are the Catmull-Rom polynomials in exact arithmetic
        t = Fraction(f)
        a = Fraction(-1, 2)
        poly = (a * t ** 3 - 2 * a * t ** 2 + a * t, (a + 2) * t ** 3 - (a + 3) * t ** 2 + 1, -(a + 2) * t ** 3 + (2 * a + 3) * t ** 2 - a * t,
                -a * t ** 3 + a * t ** 2)
        assert tuple(Fraction(k, 128) for k in want) == poly


def test_weights_sum_to_one_within_the_documented_bound():
    rng = np.random.default_rng(5)
    f = np.concatenate([np.arange(0, 1 << 20, dtype=np.float64) / (1 << 20), rng.random(1 << 20), [np.nextafter(F(1), F(0))]]).astype(F)
    f = f[f < 1]
    w = weights(f)
    total = sum(v.astype(np.float64) for v in w)
    assert np.abs(total - 1.0).max() <= 2.4e-7
    # against the polynomials in double: each weight is within a few ulp of 1
    t = f.astype(np.float64)
    ref = (-0.5 * t ** 3 + t ** 2 - 0.5 * t, 1.5 * t ** 3 - 2.5 * t ** 2 + 1, -1.5 * t ** 3 + 2 * t ** 2 + 0.5 * t, 0.5 * t ** 3 - 0.5 * t ** 2)
    for got, want in zip(w, ref):
        assert np.abs(got.astype(np.float64) - want).max() <= 4 * 2.0 ** -24


# ------------------------------------------------------------------------------------------------- what the contract implies
@pytest.mark.parametrize("shift", [(0, 0), (3, -2), (-5, 7), (39, 52)])
def test_an_integer_shift_returns_the_pixels(shift):
    """bit for bit on a finite image, except that -0.0 becomes +0.0 (the -0 and +0 weights meet in the sum)"""
    H, W = wc.SHAPE
    img = wc.image(("gray", wc.SHAPE)).copy()
    img[3, 4] = -0.0; img[20, 30] = -0.0; img[7, 7] = np.finfo(F).tiny / 4; img[8, 8] = np.finfo(F).max
    dy, dx = shift
    out, counts = warp_cubic_ref(img, [1, 0, 0, 1], [dy, dx], (H, W), fill=-1.0)
    assert counts["integer"] == counts["live"] > 0
    ys, xs = np.mgrid[0:H, 0:W]
    sy, sx = ys + dy, xs + dx
    live = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
    assert counts["live"] == live.sum()
    want = np.full((H, W), F(-1.0))
    want[live] = img[sy[live], sx[live]]
    want[want == 0] = F(0.0)
    assert np.array_equal(bits(out), bits(want))


def _poly(x, y):
    """integer-valued, degree 2 in each of x and y"""
    return (3 + 2 * x + x * x) + (5 * y + y * y) + x * y * 2 + x * x * y


def _representable(v):
    return Fraction(float(F(v.numerator / v.denominator))) == v


@pytest.mark.parametrize("off", [(0.5, 0.5), (0.25, 0.75), (0.75, 0.25), (0.5, 0.0), (1.25, 2.5)])
def test_a_quadratic_image_is_reproduced_exactly_at_half_and_quarter_pixels(off):
    """Catmull-Rom reproduces polynomials of degree <= 2.  With these coefficients every intermediate of the contract -- weight,
    product, partial sum -- is exact in binary32, which is PROVED here with fractions, pixel by pixel, not assumed; the
    restatement must then return the polynomial at the source point, bit for bit, wherever no tap clamps."""
    H, W = 12, 13
    ys, xs = np.mgrid[0:H, 0:W]
    img = _poly(xs, ys).astype(F)
    assert np.array_equal(img.astype(np.int64), _poly(xs, ys))
    out, counts = warp_cubic_ref(img, [1, 0, 0, 1], off, (H, W), fill=-1.0)
    a = Fraction(-1, 2)
    checked = 0
    for y in range(H):
        for x in range(W):
            ty, tx = Fraction(y) + Fraction(off[0]), Fraction(x) + Fraction(off[1])
            xp, yp = int(tx), int(ty)
            if not (1 <= xp and xp + 2 <= W - 1 and 1 <= yp and yp + 2 <= H - 1):
                continue

            def w_exact(t):
                return (a * t ** 3 - 2 * a * t ** 2 + a * t, (a + 2) * t ** 3 - (a + 3) * t ** 2 + 1,
                        -(a + 2) * t ** 3 + (2 * a + 3) * t ** 2 - a * t, -a * t ** 3 + a * t ** 2)

            def w_chain(f):                       # the contract's Horner steps, each checked
                steps = []
                h = Fraction(-1, 2) * f; steps.append(h); h = h + 1; steps.append(h); h = h * f; steps.append(h)
                h = h - Fraction(1, 2); steps.append(h); w0 = h * f
                h = Fraction(3, 2) * f; steps.append(h); h = h - Fraction(5, 2); steps.append(h); h = h * f; steps.append(h)
                h = h * f; steps.append(h); w1 = h + 1
                h = Fraction(-3, 2) * f; steps.append(h); h = h + 2; steps.append(h); h = h * f; steps.append(h)
                h = h + Fraction(1, 2); steps.append(h); w2 = h * f
                h = Fraction(1, 2) * f; steps.append(h); h = h - Fraction(1, 2); steps.append(h); h = h * f; steps.append(h); w3 = h * f
                assert all(_representable(s) for s in steps + [w0, w1, w2, w3])
                return w0, w1, w2, w3

            wx, wy = w_chain(tx - xp), w_chain(ty - yp)
            assert wx == w_exact(tx - xp) and wy == w_exact(ty - yp)
            R = []
            for j in range(4):
                p = [Fraction(int(img[yp - 1 + j, xp - 1 + k])) for k in range(4)]
                prod = [wx[k] * p[k] for k in range(4)]
                s1 = prod[0] + prod[1]; s2 = s1 + prod[2]; s3 = s2 + prod[3]
                assert all(_representable(v) for v in prod + [s1, s2, s3])
                R.append(s3)
            prod = [wy[j] * R[j] for j in range(4)]
            s1 = prod[0] + prod[1]; s2 = s1 + prod[2]; s3 = s2 + prod[3]
            assert all(_representable(v) for v in prod + [s1, s2, s3])
            want = _poly(tx, ty)
            assert s3 == want, (x, y)
            assert Fraction(float(out[y, x])) == want, (x, y, float(out[y, x]), want)
            checked += 1
    assert checked >= 40


def test_non_finite_taps_make_the_sample_nan_and_fill_is_never_mixed_in():
    img = wc.image(("gray", wc.SMALL)).copy()
    img[8, 10] = np.inf
    out, _ = warp_cubic_ref(img, [1, 0, 0, 1], [0, 0], wc.SMALL, fill=1e30)
    # every sample whose 4 x 4 footprint holds the pixel: zero weights still multiply (0 * inf); only the sample ON the pixel, where
    # the inf meets the weight 1 in both axes, stays inf
    assert not np.isfinite(out[6:10, 8:12]).any() and np.isfinite(out).sum() == out.size - 16
    assert np.isnan(out).sum() == 15 and out[8, 10] == np.inf
    # a huge fill leaves every live sample alone: edge pixels repeat
    a, ca = warp_cubic_ref(wc.image(("gray", wc.SMALL)), [1, 0, 0, 1], [0.5, 0.25], wc.SMALL, fill=1e30)
    b, cb = warp_cubic_ref(wc.image(("gray", wc.SMALL)), [1, 0, 0, 1], [0.5, 0.25], wc.SMALL, fill=-5.0)
    ty, tx = warp_ref.coords([1, 0, 0, 1], [0.5, 0.25], wc.SMALL)
    live = stack_ref.live_mask([1, 0, 0, 1], [0.5, 0.25], wc.SMALL, wc.SMALL)
    assert ca == cb and np.array_equal(bits(a)[live], bits(b)[live]) and (a[~live] == F(1e30)).all() and (b[~live] == F(-5.0)).all()


def test_the_live_set_is_the_bilinear_warps_non_fill_set():
    for case in [cc.by_name(n) for n in ("c1-rot30", "c2-half", "c2-hi_hi", "c4-huge_cancel", "c9-random07")]:
        img = wc.image(case.image)
        fill = F(-12345.0)
        cub = warp_cubic_ref(img, case.M, case.off, case.out_shape, fill)[0]
        lin = warp_ref.warp_ref(img, case.M, case.off, case.out_shape, fill, 1)[0]
        live = stack_ref.live_mask(case.M, case.off, img.shape, case.out_shape)
        assert np.array_equal(cub != fill, live) and np.array_equal(lin != fill, live), case.name


# ---------------------------------------------------------------------------------------------------------------- mutants
#: wrong rule -> the case whose dictated result it changes
MUTANT_CASES = {"fma_row": "c9-random00", "vertical_first": "c9-random01", "fill_tap": "c2-lo_lo", "clamp_w": "c2-hi_hi",
                "live_inside": "c2-half", "expanded_weights": "c9-random02", "floor_double": "c2-half_below", "a075": "c1-rot30"}


@pytest.mark.parametrize("rule", MUTANTS)
def test_each_wrong_rule_changes_a_dictated_result(rule):
    assert set(MUTANT_CASES) == set(MUTANTS) and len(MUTANTS) >= 8
    case = cc.by_name(MUTANT_CASES[rule])
    img = wc.image(case.image)
    want = warp_cubic_ref(img, case.M, case.off, case.out_shape, case.fill)[0]
    got = warp_cubic_ref(img, case.M, case.off, case.out_shape, case.fill, rule=rule)[0]
    assert not warp_ref.same(got, want), rule


def test_linear_delegates_to_the_bilinear_restatement_unchanged():
    for name in ("f1-rot30-gray-m1", "f1-rot30-gray-m0", "f3-mode-gray-m2", "f1-rot30-rgb-m1", "f2-half-gray-m1"):
        c = wc.by_name(name)
        want, counts = warp_ref.warp_ref(wc.image(c.image), c.M, c.off, c.out_shape, c.fill, c.mode)
        for interp in (None, "linear"):
            got, got_counts = warp(wc.image(c.image), c.M, c.off, c.out_shape, c.fill, c.mode, interp=interp)
            assert warp_ref.same(got, want) and got_counts == counts
    c = cc.by_name("c1-rot30")
    assert warp_ref.same(warp(wc.image(c.image), c.M, c.off, c.out_shape, c.fill, 1, interp="cubic")[0],
                         warp_cubic_ref(wc.image(c.image), c.M, c.off, c.out_shape, c.fill)[0])


def test_stack_samples_share_the_live_set_and_integer_shifts_share_the_values():
    case = next(c for c in cc.stack_cases() if c.kind == "noise" and c.family == "shift")
    vals, live = samples_cubic(case.frames, case.maps, case.fills, case.frames[0].shape, case.out_shape)
    lin, live_lin = stack_ref.samples(case.frames, case.maps, case.fills, case.frames[0].shape, case.out_shape, 1)
    assert np.array_equal(live, live_lin) and live.any() and not live.all()
    assert np.array_equal(vals[live], lin[live])                                            # (noise holds no -0.0)
    assert all((vals[s][~live[s]] == case.fills[s]).all() for s in range(len(case.frames)))


# -------------------------------------------------------------------------------------------------------------- interface
@pytest.fixture(scope="module")
def L():
    from sift_pyocl_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    return _lib.lib()


EX = {"siftmi_plan_transform_ex": "siftmi_plan_transform", "siftmi_batch_transform_ex": "siftmi_batch_transform",
      "siftmi_batch_stack_ex": "siftmi_batch_stack", "siftmi_batch_stack_clip_ex": "siftmi_batch_stack_clip"}


def test_header_library_and_signature_table_agree(L):
    from sift_pyocl_amd import _lib
    header = open(os.path.join(ROOT, "include", "siftmi.h")).read()
    assert re.search(r"#define SIFTMI_INTERP_MODE 0\b", header) and re.search(r"#define SIFTMI_INTERP_CUBIC 1\b", header)
    assert (_lib.INTERP_MODE, _lib.INTERP_CUBIC) == (0, 1)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for ex, parent in EX.items():
        assert hasattr(L, ex) and ex in _lib.exported_symbols()
        decl = {n: re.search(r"\bint %s\s*\(([^;]*)\);" % n, code).group(1) for n in (ex, parent)}
        names = {n: [re.sub(r".*[\s*]", "", a.strip()) for a in d.split(",")] for n, d in decl.items()}
        at = names[parent].index("mode") + 1
        assert names[ex] == names[parent][:at] + ["interp"] + names[parent][at:], ex      # the parent's arguments, interp after mode
        res_p, args_p = _lib._SIGNATURES[parent]
        res_e, args_e = _lib._SIGNATURES[ex]
        assert res_e is res_p and list(args_e) == list(args_p[:at]) + [C.c_int32] + list(args_p[at:]), ex
    # a null handle is refused before a device is looked for
    assert L.siftmi_plan_transform_ex(None, None, 0, 1, None, 0, 4, 4, None, None, C.c_float(0), 1, 1, None) == _lib.EINVAL
    assert L.siftmi_batch_transform_ex(None, None, 0, 0, 1, None, 0, 4, 4, None, None, 1, 1, None) == _lib.EINVAL
    assert L.siftmi_batch_stack_ex(None, None, 0, 0, None, None, 0, 4, 4, None, None, 1, 1, 1, C.c_float(0), None) == _lib.EINVAL
    assert L.siftmi_batch_stack_clip_ex(None, None, 0, 0, None, None, None, 0, 4, 4, None, None, None, 1, 1, 0, 0, 1, C.c_float(3), C.c_float(3),
                                        3, C.c_float(0), None) == _lib.EINVAL


def test_the_keyword_is_checked_before_anything_else():
    from sift_pyocl_amd import _lib
    assert [_lib.interp_code(v) for v in (None, "linear", "cubic")] == [0, 0, 1]
    assert _lib.interp_code(None, mode=0) == 0 and _lib.interp_code("linear", mode=7, rgb=True) == 0
    for bad in ("Cubic", "lanczos", "", 1, 0, True, b"cubic"):
        with pytest.raises(ValueError):
            _lib.interp_code(bad)
    for mode in (0, 2, -1, 257):
        with pytest.raises(ValueError):
            _lib.interp_code("cubic", mode=mode)
    with pytest.raises(ValueError):
        _lib.interp_code("cubic", rgb=True)


def test_every_warp_method_takes_the_keyword():
    from sift_pyocl_amd import BatchPlan, LinearAlign
    for f in (LinearAlign.transform, LinearAlign.align):
        p = inspect.signature(f).parameters["interp"]
        assert p.default is None
    for f in (BatchPlan.transform_batch, BatchPlan.stack_batch, BatchPlan.stack_clip_batch, LinearAlign.align_batch,
              LinearAlign.align_batch_window, LinearAlign.stack, LinearAlign.stack_clip):
        # (their parameter lists are pinned by the rows that introduced them: the keyword is taken by the wrapper)
        kw = inspect.signature(f, follow_wrapped=False).parameters["interp"]
        assert kw.kind is inspect.Parameter.KEYWORD_ONLY and kw.default is None, f.__name__
        assert "interp" in f.__doc__, f.__name__

    class Probe:
        RGB = False

        @__import__("sift_pyocl_amd")._lib.interp_keyword("_impl")
        def method(self, a, b=2, c="x"):
            return ("plain", a, b, c)

        def _impl(self, a, b, c, interp=None):
            return ("impl", a, b, c, interp)

    p = Probe()
    assert p.method(1) == ("plain", 1, 2, "x") and p.method(1, c="y", interp=None) == ("plain", 1, 2, "y")
    assert p.method(1, 5, interp="cubic") == ("impl", 1, 5, "x", "cubic") and p.method(b=3, a=0, interp="linear") == ("impl", 0, 3, "x", "linear")
    with pytest.raises(TypeError):
        p.method(1, nope=3, interp="cubic")
