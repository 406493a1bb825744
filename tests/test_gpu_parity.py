"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle, bit for bit.

Tolerances: none.  Integer/byte outputs (descriptors, match pairs) and every float field
(x, y, scale, angle, intermediate planes) must be bit-identical to oracle/sift_oracle.c, which is
itself pinned to the reference's natively compiled kernels (tests/test_oracle_vs_ref.py,
tests/golden/).
"""
import ctypes as C

import numpy as np
import pytest

from util import (assert_same_keypoints, descriptor_edge_rows, descriptor_random_rows, multiscale_noise, orientation_border_rows,
                  rectangles, smooth_noise, sort_rows, white_noise)

pytestmark = pytest.mark.gpu


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _params(**kw):
    from sift_pyocl_amd import _lib
    d = dict(init_sigma=1.6, peak_thresh=np.float32(255.0 * 0.04 / 3.0), edge_thresh0=np.float32(0.08),
             edge_thresh=np.float32(0.06), ori_sigma=np.float32(1.5), border_dist=5, octave_max=0, pix_per_kp=10,
             double_im_size=0)
    d.update(kw)
    return _lib.Params(**d)


# ----------------------------------------------------------------------------- siftmath
def _around(v, ulps):
    """the float32 v and the `ulps` floats on either side of it"""
    return (np.array([v], np.float32).view(np.int32) + np.arange(-ulps, ulps + 1, dtype=np.int32)).view(np.float32)


def _log_uniform(rng, n, lo_exp, hi_exp):
    """both signs, uniform exponent in [lo_exp, hi_exp), uniform mantissa"""
    return (np.ldexp(1.0 + rng.random(n), rng.integers(lo_exp, hi_exp, n)) * rng.choice([-1.0, 1.0], n)).astype(np.float32)


def _unary_sweep(fn, rng, n=1 << 22):
    """2^22 arguments of exp (0), exp2 (1), sin / cos (2, 3) over the whole argument type: any bit pattern; both sides and the
    exact values of every range test of the four functions (-104, 89, -150, 128, and 2^30 of sin / cos); results in the binary32
    sub-normal range; +-0, the smallest sub-normals, +-inf, NaN; for sin / cos also 2^k pi/2 +- a few ulps up to k = 29,
    multiples of pi/2, uniform exponents up to 2^30 and, separately, from 2^30 to FLT_MAX (NaN for both)."""
    parts = [rng.integers(0, 2 ** 32, n // 2, dtype=np.uint64).astype(np.uint32).view(np.float32)]
    for edge in (-104.0, 89.0, -150.0, 128.0, 104.0, -89.0, 150.0, -128.0, 2.0 ** 30, -2.0 ** 30):
        parts.append(_around(edge, 512))
    tiny = np.array([0, 1, 2, 3, 0x007fffff, 0x00800000, 0x00800001], np.uint32)
    parts.append(np.concatenate([tiny, tiny | np.uint32(0x80000000)]).view(np.float32))
    parts.append(np.array([np.inf, -np.inf, np.nan, -np.nan, 3.4028235e38, -3.4028235e38], np.float32))
    m = n // 16
    if fn == 0:
        parts += [rng.uniform(-104.0, -87.3, 2 * m), rng.uniform(88.0, 89.0, m), rng.uniform(-110.0, 95.0, 2 * m), _log_uniform(rng, m, -149, 7)]
    elif fn == 1:
        parts += [rng.uniform(-150.0, -126.0, 2 * m), rng.uniform(127.0, 128.0, m), rng.uniform(-155.0, 133.0, 2 * m), _log_uniform(rng, m, -149, 8),
                  np.arange(-152, 131, dtype=np.float32), np.arange(-152, 131, dtype=np.float32) + np.float32(0.5)]      # exact powers, ties of rint
    else:
        half_pi = np.float32(np.pi / 2)
        parts += [np.concatenate([_around(np.float32(np.ldexp(np.pi / 2, k)), 8) for k in range(-2, 30)])]
        parts[-1] = np.concatenate([parts[-1], -parts[-1]])
        q = rng.integers(-(1 << 29), 1 << 29, m)                                          # multiples of pi/2, |x| < 2^30
        parts += [(q * (np.pi / 2)).astype(np.float32), (rng.integers(-4096, 4096, m) * half_pi).astype(np.float32),
                  _log_uniform(rng, 3 * m, -30, 30), _log_uniform(rng, m, 30, 128), _log_uniform(rng, m // 2, -149, -100)]
    a = np.concatenate([np.asarray(p, np.float32) for p in parts])
    lo, hi = (-110.0, 95.0) if fn == 0 else (-155.0, 133.0) if fn == 1 else (-8.0, 8.0)
    assert a.size <= n
    return np.concatenate([a, rng.uniform(lo, hi, n - a.size).astype(np.float32)])


@pytest.mark.parametrize("fn", [0, 1, 2, 3, 4])
def test_device_math_bit_exact(siftlib, oracle, fn):
    """The defining functions on the device against the oracle's (array entry points): 200 000 arguments of the working ranges
    and, for the unary ones, 2^22 more over the whole argument type (_unary_sweep).  NaN results are compared as "is NaN"."""
    rng = np.random.default_rng(fn)
    n = 200000
    if fn == 0:
        a = (-rng.random(n) * 110).astype(np.float32); a[:8] = [0, -0.0, -1e-30, -88.5, -103.9, -104.5, 1.0, np.nan]
    elif fn == 1:
        a = (rng.random(n) * 12 - 6).astype(np.float32)
    elif fn in (2, 3):
        a = (rng.random(n) * 8 - 4).astype(np.float32); a[:4] = [0, np.pi, -np.pi, 3.1415927]
    else:
        a = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
    b = (rng.standard_normal(n) * 10.0 ** rng.integers(-3, 3, n)).astype(np.float32)
    if fn == 4:
        a[:6] = [0, -0.0, 0, 1, -1, 0]; b[:6] = [0, 0, -0.0, 0, 0, -1]
    else:
        a = np.concatenate([a, _unary_sweep(fn, np.random.default_rng(1000 + fn))]); b = a
        n = a.size
    out = np.empty(n, np.float32)
    assert siftlib.siftmi_stage_math(0, fn, _p(a), _p(b), _p(out), n) == 0
    if fn == 0: exp = oracle.expf_array(a)
    elif fn == 1: exp = oracle.exp2f_array(a)
    elif fn in (2, 3): exp = oracle.sincosf_array(a)[fn - 2]
    else: exp = oracle.atan2f_array(a, b)
    if fn in (2, 3):                                                                    # sin / cos are total: NaN beyond 2^30
        beyond = ~(np.abs(a) <= np.float32(2.0 ** 30))
        assert beyond.sum() > 1 << 20 and np.isnan(out[beyond]).all() and np.isfinite(out[~beyond]).all()
    if fn in (0, 1):                                                                    # the sweep reaches sub-normal results
        assert ((exp > 0) & (exp < np.float32(2.0 ** -126))).sum() > 1 << 17
    bad = np.nonzero((out.view(np.uint32) != exp.view(np.uint32)) & ~(np.isnan(out) & np.isnan(exp)))[0]
    assert bad.size == 0, (fn, bad.size, a[bad[:4]], b[bad[:4]], out[bad[:4]], exp[bad[:4]])


@pytest.mark.parametrize("fn", [5, 6])
def test_device_fast_paths_equal_the_defining_functions(siftlib, oracle, fn):
    """siftmath's Ziv fast paths (expf_fast, atan2f_fast: fused binary64 evaluation + rounding-safety test, fallback to
    the defining function) against the oracle's expf / atan2f on 10^7 arguments each: pipeline-like ranges, wide
    ranges, exact ties of the octant selection, zeros / infinities / NaN / sub-normal results.  (Random arguments hardly
    ever come near a rounding boundary: tests/test_gpu_math_hard.py holds the ones that do.)"""
    rng = np.random.default_rng(100 + fn)
    n = 1 << 20
    for rnd in range(10):
        if fn == 5:
            kind = rnd % 5
            if kind == 0: a = -(rng.random(n) * 12).astype(np.float32)                       # window weights
            elif kind == 1: a = (rng.random(n) * 240 - 120).astype(np.float32)              # incl. under / overflow
            elif kind == 2: a = (rng.standard_normal(n) * 10.0 ** rng.integers(-8, 2, n)).astype(np.float32)
            elif kind == 3: a = (np.round(rng.random(n) * 160 - 80) * np.float32(0.6931472)).astype(np.float32)   # near k ln2
            else: a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)            # any bit pattern
            a[:10] = [0, -0.0, -1e-30, -88.5, -103.9, -104.5, 1.0, np.nan, np.inf, -np.inf]
            b = a
            want = oracle.expf_array(a)
        else:
            kind = rnd % 5
            if kind == 0:                                                                     # gradients of a 0..255 image
                a = (rng.standard_normal(n) * 20).astype(np.float32); b = (rng.standard_normal(n) * 20).astype(np.float32)
            elif kind == 1:
                a = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
                b = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 6, n)).astype(np.float32)
            elif kind == 2:                                                                   # ratios at the octant-table ties
                b = (rng.random(n) * 100 + 0.01).astype(np.float32)
                a = (b * ((rng.integers(0, 8, n) + 0.5) / 8.0) * (1 + rng.integers(-3, 4, n) * 2.0 ** -23)).astype(np.float32)
                a *= rng.choice([-1, 1], n).astype(np.float32); b *= rng.choice([-1, 1], n).astype(np.float32)
            elif kind == 3:                                                                   # |y| == |x|, tiny and huge ratios
                b = (rng.standard_normal(n) * 50).astype(np.float32)
                a = (b * rng.choice([1.0, -1.0, 1e-20, 1e20, 1e-30, 1e-37], n)).astype(np.float32)
            else:
                a = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
                b = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)
            a[:8] = [0, -0.0, 0, 1, -1, 0, np.inf, np.nan]; b[:8] = [0, 0, -0.0, 0, 0, -1, 1, 1]
            want = oracle.atan2f_array(a, b)
        out = np.empty(n, np.float32)
        assert siftlib.siftmi_stage_math(0, fn, _p(a), _p(b), _p(out), n) == 0
        bad = np.nonzero(out.view(np.uint32) != want.view(np.uint32))[0]
        bad = bad[~(np.isnan(out[bad]) & np.isnan(want[bad]))]          # NaN payloads are not part of the contract
        assert bad.size == 0, (fn, rnd, a[bad[:4]], b[bad[:4]], out[bad[:4]], want[bad[:4]])


def test_division_by_reciprocal_is_the_ieee_quotient(siftlib):
    """siftmath::div_by_reciprocal (Markstein's two residual steps on a correctly rounded reciprocal) replaces the
    two divisions per descriptor sample (keypoints_cpu.cl:64-65): it must return the correctly rounded quotient for the
    operands that occur there -- |a| < 2^8 (window coordinates, incl. exact zeros and values that cancel to a few ulp),
    b = spacing in [0.1, 128] -- and for the two divisions per orientation sample (orientation_cpu.cl:88-90:
    x / (2 pi_f), -d2 / (2 sigma^2) with |a| up to 10^4, b in [1e-3, 1e6]).  numpy's float32 division is the IEEE quotient."""
    rng = np.random.default_rng(77)
    n = 1 << 22
    for rnd in range(24):
        b = np.exp(rng.uniform(np.log(0.1), np.log(128.0), n)).astype(np.float32)
        kind = rnd % 4
        if kind == 0: a = (rng.standard_normal(n) * 40).astype(np.float32)
        elif kind == 1: a = (rng.uniform(-250, 250, n)).astype(np.float32)
        elif kind == 2: a = (b * rng.integers(-30, 31, n) * np.float32(0.25) * (1 + rng.integers(-4, 5, n) * 2.0 ** -23)).astype(np.float32)  # near ties
        else: a = (rng.standard_normal(n) * 10.0 ** rng.integers(-7, 2, n)).astype(np.float32)
        a[:3] = [0.0, -0.0, 1.0]
        if rnd == 5: b = rng.integers(0x3dcccccd, 0x43000000, n).astype(np.uint32).view(np.float32)       # every spacing pattern class
        if rnd >= 12:                                                                                      # the orientation kernel's operands
            b = np.exp(rng.uniform(np.log(1e-3), np.log(1e6), n)).astype(np.float32) if rnd % 2 else np.full(n, 2.0 * np.float32(3.14159274101257), np.float32)
            a = (a * np.float32(40.0)).astype(np.float32)
        out = np.empty(n, np.float32)
        assert siftlib.siftmi_stage_math(0, 7, _p(a), _p(b), _p(out), n) == 0
        want = a / b
        bad = np.nonzero((out.view(np.uint32) != want.view(np.uint32)) & ~((out == 0) & (want == 0)))[0]   # the sign of a zero
        assert bad.size == 0, (rnd, a[bad[:4]], b[bad[:4]], out[bad[:4]], want[bad[:4]])                 # quotient is lost (1.5f is added next)


# ----------------------------------------------------------------------------- stages
def test_compact_stage(siftlib, oracle):
    """stand-alone `compact` (algebra.cl:57-84): the head [0, start) stays, the survivors of [start, end) follow in any order"""
    rng = np.random.default_rng(4)
    n, start, end = 5000, 700, 4600
    kps = rng.random((n, 4), dtype=np.float32) * 100
    kps[rng.random(n) < 0.6] = -1.0
    out = np.empty_like(kps)
    m = C.c_int64(0)
    assert siftlib.siftmi_stage_compact(0, _p(kps), n, start, end, _p(out), C.byref(m)) == 0
    want, count = oracle.compact(kps, start, end)
    assert m.value == count
    assert np.array_equal(out[:start], kps[:start])
    assert np.array_equal(sort_rows(out[start:count]), sort_rows(want[start:count]))


def test_gaussian_taps(siftlib, oracle):
    for sigma, size in [(1.5198684, 15), (1.2262735, 11), (1.5450078, 15), (1.9465878, 17), (2.452547, 21), (3.0900156, 27),
                        (3.0, 28), (0.7, 7)]:
        out = np.empty(size, np.float32)
        assert siftlib.siftmi_stage_gaussian_taps(C.c_float(sigma), size, _p(out)) == 0
        assert np.array_equal(out, oracle.gaussian_taps(sigma, size))


@pytest.mark.parametrize("shape", [(64, 64), (131, 97), (300, 421), (16, 16), (13, 700), (1025, 1030)])
@pytest.mark.parametrize("ntaps", [11, 15, 17, 21, 27, 9, 28])
def test_blur_bit_exact(siftlib, oracle, shape, ntaps):
    if min(shape) < ntaps - ((ntaps - 1) // 2):
        pytest.skip("image smaller than the filter half-width: undefined in the reference too (convolution.cl:45-48)")
    img = white_noise(shape, seed=ntaps) * 255
    taps = oracle.gaussian_taps(ntaps / 8.0, ntaps)
    out = np.empty_like(img)
    assert siftlib.siftmi_stage_blur(0, _p(img), _p(out), shape[1], shape[0], _p(taps), ntaps) == 0
    exp = oracle.blur(img, taps)
    assert np.array_equal(out.view(np.uint32), exp.view(np.uint32))


# The marching team kernel (blur_team_kernel: planes of at least 1400^2 pixels, i.e. every full-resolution launch of the headline
# frame) reached AS A STAGE: shapes with a partial last strip, an odd width (scalar stores), a height that is no multiple of
# the segment height; both workgroup orders; workgroup counts that give other segment heights / last sub-block counts.
TEAM_SHAPES = [(1408, 1536), (1026, 2050), (1537, 1301)]


@pytest.mark.parametrize("shape", TEAM_SHAPES)
@pytest.mark.parametrize("ntaps", [11, 15, 17, 21, 27])
def test_blur_team_kernel_bit_exact(siftlib, oracle, shape, ntaps):
    H, W = shape
    img = white_noise(shape, seed=100 + ntaps) * 255
    taps = oracle.gaussian_taps(ntaps / 8.0, ntaps)
    exp = oracle.blur(img, taps)
    for xcd_map, wgs in [(1, 0), (0, 0), (1, 300), (1, 1500), (3, 0), (2, 500)]:       # (bit 1 of xcd_map: priority feedback off)
        out = np.empty_like(img)
        used = C.c_int32(-1)
        assert siftlib.siftmi_stage_blur_ex(0, _p(img), 0, _p(out), W, H, _p(taps), ntaps, 0, xcd_map, wgs, C.byref(used)) == 0
        assert used.value == 2, "the plane did not reach blur_team_kernel"
        bad = np.argwhere(out.view(np.uint32) != exp.view(np.uint32))
        assert bad.size == 0, (ntaps, xcd_map, wgs, len(bad), bad[:4])


@pytest.mark.parametrize("shape", TEAM_SHAPES)
def test_blur_team_kernel_normalising_and_typed_instances(siftlib, oracle, shape):
    """blur_team_kernel<15, NORM = true, S, DT>: `normalizes` (preprocess.cl:239-252) applied while staging, behind the min/max
    pass; DT != 0: the integer / RGB converters (preprocess.cl:53-223) at the point of use."""
    H, W = shape
    taps = oracle.gaussian_taps(float(np.sqrt(1.6 ** 2 - 0.25)), 15)
    rng = np.random.default_rng(H)
    f32 = (white_noise(shape, seed=7) - 0.25) * 3000.0
    u8 = rng.integers(0, 256, shape, dtype=np.uint8)
    u16 = rng.integers(0, 65536, shape, dtype=np.uint16)
    i64 = rng.integers(-2 ** 62, 2 ** 62, shape, dtype=np.int64)
    rgb = rng.integers(0, 256, shape + (3,), dtype=np.uint8)
    r, g, b = (rgb[..., c].astype(np.float32) for c in range(3))
    rgb32 = (np.float32(0.299) * r + np.float32(0.587) * g) + np.float32(0.114) * b
    cases = [("f32", 0, f32, f32), ("u8", 1, u8, u8.astype(np.float32)), ("u16", 2, u16, u16.astype(np.float32)),
             ("i64", 6, i64, i64.astype(np.float32)), ("rgb8", 8, rgb, rgb32)]
    for name, code, frame, as32 in cases:
        as32 = np.ascontiguousarray(as32, np.float32)
        exp = oracle.blur(oracle.normalize(as32, as32.min(), as32.max()), taps)
        for xcd_map in (1, 0):
            out = np.empty(shape, np.float32)
            used = C.c_int32(-1)
            frame = np.ascontiguousarray(frame)
            assert siftlib.siftmi_stage_blur_ex(0, _p(frame), code, _p(out), W, H, _p(taps), 15, 1, xcd_map, 0, C.byref(used)) == 0, name
            assert used.value == 2, name
            bad = np.argwhere(out.view(np.uint32) != exp.view(np.uint32))
            assert bad.size == 0, (name, xcd_map, len(bad), bad[:4])


def test_minmax_normalize(siftlib, oracle):
    for shape in [(512, 512), (131, 97), (1980, 2560)]:
        img = (white_noise(shape, 1) - 0.3) * 1000
        out = np.empty_like(img)
        mn, mx = C.c_float(), C.c_float()
        assert siftlib.siftmi_stage_minmax_normalize(0, _p(img), _p(out), shape[1], shape[0], C.byref(mn), C.byref(mx)) == 0
        assert mn.value == img.min() and mx.value == img.max()
        assert np.array_equal(out, oracle.normalize(img, img.min(), img.max()))


def _octave_blurs(oracle, img):
    """blur[0..5] of the first octave of `img` computed by the oracle (normalise, init blur, 5 blurs)."""
    import math
    mn, mx = oracle.minmax(img)
    base = oracle.normalize(img, mn, mx)
    s0 = math.sqrt(1.6 ** 2 - 0.25)
    base = oracle.blur(base, oracle.gaussian_taps(s0, 15))
    blurs = [base]
    ratio = 2.0 ** (1.0 / 3.0)
    prev = 1.6
    for s in range(5):
        inc = prev * math.sqrt(ratio ** 2 - 1.0)
        size = int(math.ceil(8 * inc + 1)); size += (size % 2 == 0)
        blurs.append(oracle.blur(blurs[-1], oracle.gaussian_taps(inc, size)))
        prev *= ratio
    return np.ascontiguousarray(np.stack(blurs))


@pytest.mark.parametrize("maker,shape", [(smooth_noise, (131, 97)), (white_noise, (256, 300)), (multiscale_noise, (300, 421))])
def test_detection_stages(siftlib, oracle, maker, shape):
    img = maker(shape)
    H, W = shape
    blurs = _octave_blurs(oracle, img)
    par = _params()
    opar = oracle.default_params()
    dogs = oracle.dog(blurs)
    # DoG stage
    d = np.empty_like(dogs[0])
    assert siftlib.siftmi_stage_dog(0, _p(blurs[2]), _p(blurs[3]), _p(d), d.size) == 0
    assert np.array_equal(d, dogs[2])
    # extrema of the three scales
    cap = H * W // 10
    exp_all = []
    for s in (1, 2, 3):
        k, n = oracle.local_maxmin(dogs, s, 1, cap, opar)
        exp_all.append(k[:n])
    exp = np.concatenate(exp_all)
    got = np.empty((cap, 4), np.float32)
    n = C.c_int64()
    assert siftlib.siftmi_stage_local_maxmin(0, _p(blurs), W, H, 1, C.byref(par), _p(got), cap, C.byref(n)) == 0
    assert n.value == len(exp)
    assert np.array_equal(sort_rows(got[:n.value]), sort_rows(exp))
    # refinement + compaction
    cand = np.ascontiguousarray(exp)
    interp = oracle.interp_keypoint(dogs, cand, 0, len(cand), opar)
    keep = interp[:, 1] != -1
    exp_ref = np.concatenate([interp[keep], cand[keep][:, 3:4]], axis=1)
    ref = np.empty((len(cand), 4), np.float32); sc = np.empty(len(cand), np.int32)
    m = C.c_int64()
    assert siftlib.siftmi_stage_interp(0, _p(blurs), W, H, _p(cand), len(cand), C.byref(par), _p(ref), _p(sc), C.byref(m)) == 0
    assert m.value == keep.sum()
    got_ref = np.concatenate([ref[:m.value], sc[:m.value, None].astype(np.float32)], axis=1)
    assert np.array_equal(sort_rows(got_ref).view(np.uint32), sort_rows(exp_ref).view(np.uint32))
    # gradient maps
    g = np.empty((H, W), np.float32); o = np.empty((H, W), np.float32)
    assert siftlib.siftmi_stage_gradient(0, _p(blurs[2]), _p(g), _p(o), W, H) == 0
    eg, eo = oracle.gradient(blurs[2])
    assert np.array_equal(g.view(np.uint32), eg.view(np.uint32))
    assert np.array_equal(o.view(np.uint32), eo.view(np.uint32))
    # orientation + descriptor per detection scale
    for s in (1, 2, 3):
        sel = exp_ref[exp_ref[:, 4] == s][:, :4].copy()
        if len(sel) == 0:
            continue
        eg, eo = oracle.gradient(blurs[s])
        buf = np.full((len(sel) * 4 + 8, 4), -1, np.float32); buf[:len(sel)] = sel
        okp, cnt = oracle.orientation(buf, eg, eo, 1, 0, len(sel), capacity=len(buf), par=opar)
        okp = okp[:cnt]
        edesc = oracle.descriptor(okp, eg, eo, 1, 0, cnt)[:cnt]
        valid = ~np.isnan(okp.sum(axis=1))
        scl = np.full(len(sel), s, np.int32)
        out = np.empty((len(buf), 4), np.float32); osc = np.empty(len(buf), np.int32); no = C.c_int64()
        assert siftlib.siftmi_stage_orientation(0, _p(blurs), W, H, 1, _p(sel), _p(scl), len(sel), C.byref(par), _p(out),
                                                _p(osc), len(buf), C.byref(no)) == 0
        assert no.value == valid.sum()
        assert np.array_equal(sort_rows(out[:no.value]).view(np.uint32), sort_rows(okp[valid]).view(np.uint32))
        # descriptors for the oracle's oriented list (same order -> direct comparison)
        kk = np.ascontiguousarray(okp[valid]); ss = np.full(len(kk), s, np.int32)
        dd = np.zeros((len(kk), 128), np.uint8)
        assert siftlib.siftmi_stage_descriptor(0, _p(blurs), W, H, 1, _p(kk), _p(ss), len(kk), _p(dd)) == 0
        assert np.array_equal(dd, edesc[valid]), "descriptor bins differ at scale %d" % s


@pytest.mark.parametrize("octsize", [1, 2])
def test_descriptor_windows_at_their_edges(siftlib, oracle, octsize):
    """Descriptor stage on SYNTHETIC oriented keypoints chosen to stress the row-interval form of the kernel (k_descriptor.hpp):
    window axes on and a hair off the pixel axes and diagonals (rows that start / end exactly on a cell boundary, the short rows
    at the corners of a 45-degree window: the row look-up moves on by more than four rows per batch there), the smallest and the
    largest window the row tables hold (R = 127), centres on, next to and beyond the plane's borders (clipped rows, empty rows,
    empty windows), sub-pixel offsets of exactly one half.  Bit-identical bins against the oracle."""
    H, W = 300, 421
    img = smooth_noise((H, W))
    blurs = _octave_blurs(oracle, img)
    s = 2
    eg, eo = oracle.gradient(blurs[s])
    kk = descriptor_edge_rows(W, H, octsize)
    want = oracle.descriptor(kk, eg, eo, octsize, 0, len(kk))
    ss = np.full(len(kk), s, np.int32)
    got = np.zeros((len(kk), 128), np.uint8)
    assert siftlib.siftmi_stage_descriptor(0, _p(blurs), W, H, octsize, _p(kk), _p(ss), len(kk), _p(got)) == 0
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "descriptor bins differ for keypoints %s: %s" % (bad[:8], kk[bad[:8]])
    assert want.any(axis=1).sum() > len(kk) // 2            # (most of these windows do hold samples)


@pytest.mark.parametrize("seed,octsize,shape", [(1, 1, (300, 421)), (2, 4, (257, 330)), (3, 1, (97, 131))])
def test_descriptor_random_keypoints(siftlib, oracle, seed, octsize, shape):
    """3000 random oriented keypoints per case (uniform centres up to 8 pixels beyond the plane, log-uniform sigma from the
    smallest window to R = 126, uniform angle in [-pi, pi]): the descriptor stage against the oracle, every bin."""
    H, W = shape
    img = multiscale_noise((H, W)) if seed != 2 else white_noise((H, W))
    blurs = _octave_blurs(oracle, img)
    s = 1 + seed % 3
    eg, eo = oracle.gradient(blurs[s])
    n = 3000
    kk = descriptor_random_rows(seed, W, H, octsize, n)
    want = oracle.descriptor(kk, eg, eo, octsize, 0, n)
    ss = np.full(n, s, np.int32)
    got = np.zeros((n, 128), np.uint8)
    assert siftlib.siftmi_stage_descriptor(0, _p(blurs), W, H, octsize, _p(kk), _p(ss), n, _p(got)) == 0
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "descriptor bins differ for %d keypoints, first %s" % (len(bad), kk[bad[:4]])


def test_orientation_windows_at_the_borders(siftlib, oracle):
    """Orientation stage on SYNTHETIC refined keypoints: windows clipped by every border and corner, the smallest and the
    largest radii a plan can produce and beyond (sigma 0.5 ... 8: radius 2 ... 36), centres on half-pixel positions.  Same
    oriented list (as a set: slots are handed out by an atomic counter) as the oracle, bit for bit."""
    H, W = 300, 421
    img = multiscale_noise((H, W))
    blurs = _octave_blurs(oracle, img)
    par = _params()
    opar = oracle.default_params()
    s = 1
    eg, eo = oracle.gradient(blurs[s])
    sel = orientation_border_rows(W, H)
    buf = np.full((len(sel) * 8 + 8, 4), -1, np.float32); buf[:len(sel)] = sel
    okp, cnt = oracle.orientation(buf, eg, eo, 1, 0, len(sel), capacity=len(buf), par=opar)
    okp = okp[:cnt]
    valid = ~np.isnan(okp.sum(axis=1))
    scl = np.full(len(sel), s, np.int32)
    out = np.empty((len(buf), 4), np.float32); osc = np.empty(len(buf), np.int32); no = C.c_int64()
    assert siftlib.siftmi_stage_orientation(0, _p(blurs), W, H, 1, _p(sel), _p(scl), len(sel), C.byref(par), _p(out), _p(osc),
                                            len(buf), C.byref(no)) == 0
    assert no.value == valid.sum() and no.value >= len(sel) // 2
    assert np.array_equal(sort_rows(out[:no.value]).view(np.uint32), sort_rows(okp[valid]).view(np.uint32))


def test_shrink_and_convert(siftlib):
    img = white_noise((301, 203), 2)
    out = np.empty((150, 101), np.float32)
    assert siftlib.siftmi_stage_shrink(0, _p(img), _p(out), 203, 301) == 0
    assert np.array_equal(out, img[:300:2, :202:2])
    rng = np.random.default_rng(0)
    from sift_pyocl_amd._lib import DTYPE_CODES
    for name in ("uint8", "uint16", "uint32", "uint64", "int32", "int64", "float64"):
        dt = np.dtype(name)
        if dt.kind == "f":
            a = rng.standard_normal((50, 70)).astype(dt)
        else:
            info = np.iinfo(dt)
            a = rng.integers(info.min, info.max, (50, 70), dtype=dt, endpoint=True)
        o = np.empty((50, 70), np.float32)
        assert siftlib.siftmi_stage_convert(0, _p(a), DTYPE_CODES[name], _p(o), 70, 50) == 0
        assert np.array_equal(o, a.astype(np.float32)), name
    rgb = rng.integers(0, 256, (40, 60, 3), dtype=np.uint8)
    o = np.empty((40, 60), np.float32)
    assert siftlib.siftmi_stage_convert(0, _p(rgb), DTYPE_CODES["rgb8"], _p(o), 60, 40) == 0
    f = rgb.astype(np.float32)
    exp = (np.float32(0.299) * f[..., 0] + np.float32(0.587) * f[..., 1]) + np.float32(0.114) * f[..., 2]
    assert np.array_equal(o, exp)


# ----------------------------------------------------------------------------- whole pipeline
CASES = [("white512", white_noise, (512, 512)), ("smooth512", smooth_noise, (512, 512)),
         ("multi300x421", multiscale_noise, (300, 421)), ("rect257x511", rectangles, (257, 511)),
         ("smooth131x97", smooth_noise, (131, 97)), ("tiny16", white_noise, (16, 16)),
         ("white1024x768", white_noise, (1024, 768))]


@pytest.mark.parametrize("name,maker,shape", CASES)
def test_keypoints_bit_exact_vs_oracle(siftlib, oracle, name, maker, shape):
    import sift_pyocl_amd as sp
    img = maker(shape)
    plan = sp.SiftPlan(template=img, devicetype="CPU")
    got = plan.keypoints(img)
    exp = oracle.keypoints(img)
    assert_same_keypoints(got, exp, name)
    # a plan is reusable and deterministic as a set
    again = plan.keypoints(img)
    assert_same_keypoints(got, again, name + " (second call)")


def test_keypoints_octave_limit_and_profile(siftlib, oracle):
    import sift_pyocl_amd as sp
    img = smooth_noise((512, 512))
    plan = sp.SiftPlan(template=img, octave_max=3, profile=True)
    got = plan.keypoints(img)
    exp = oracle.keypoints(img, oracle.default_params(octave_max=3))
    assert_same_keypoints(got, exp, "octave_max=3")
    # (the stage times of a process's FIRST call hold the lazy load of every kernel's code object -- 80 ms on a fresh box --:
    # the bound below is about the second call)
    assert_same_keypoints(plan.keypoints(img), exp, "octave_max=3, second call")
    kt = plan.kernel_times()
    assert kt["total_ms"] > 0 and kt["blur_launches"] == 16 and kt["blur_ms"] <= kt["total_ms"]
    assert plan.minmax() == (float(img.min()), float(img.max()))
    # plan.events as the reference fills it under profile=True (plan.py:331, 455, 522, 594): (label, event) per stage of the
    # last call, event.profile.end - event.profile.start in nanoseconds (plan.py:838-839)
    labels = [l for l, _ in plan.events]
    assert len(plan.events) >= 16 + 6 and any("Blur" in l for l in labels) and any("descriptors" in l for l in labels)
    total_ns = sum(e.profile.end - e.profile.start for _, e in plan.events)
    # (a sanity bound on the unit, not a performance claim: code objects load lazily per kernel, and a box with noisy neighbours
    # has shown 85 ms on a second call -- the best of three further calls is what is bounded)
    best_ns = total_ns
    for _ in range(3):
        plan.keypoints(img)
        best_ns = min(best_ns, sum(e.profile.end - e.profile.start for _, e in plan.events))
    assert total_ns > 0 and 0 < best_ns * 1e-6 < 50.0
    plan.log_profile()
    plan.reset_timer()
    assert plan.events == []
    assert sp.SiftPlan(template=img).keypoints(img) is not None and sp.SiftPlan(template=img).events == []


def test_keypoints_integer_and_device_inputs(siftlib, oracle):
    import sift_pyocl_amd as sp
    import torch
    img = (smooth_noise((200, 300)) * 60000).astype(np.uint16)
    exp = oracle.keypoints(img.astype(np.float32))
    plan = sp.SiftPlan(template=img)
    assert_same_keypoints(plan.keypoints(img), exp, "uint16 input")
    assert_same_keypoints(plan.keypoints(img.astype(np.float32)), exp, "float32 image on a uint16 plan")
    t = torch.from_numpy(img.astype(np.float32)).cuda()
    fplan = sp.SiftPlan(shape=img.shape, dtype=np.float32)
    assert_same_keypoints(fplan.keypoints(t), exp, "device-resident torch input")


def test_keypoints_errors(siftlib):
    import sift_pyocl_amd as sp
    with pytest.raises(RuntimeError):
        sp.SiftPlan(shape=(4,), dtype=np.float32)
    with pytest.raises(RuntimeError):
        sp.SiftPlan(shape=(64, 64), dtype=np.complex64)
    plan = sp.SiftPlan(shape=(64, 64), dtype=np.float32)
    with pytest.raises(AssertionError):
        plan.keypoints(np.zeros((32, 64), np.float32))
    with pytest.raises(AssertionError):
        plan.keypoints(np.zeros((64, 64), np.uint8))


# ----------------------------------------------------------------------------- matching
def _random_kp(n, seed):
    rng = np.random.default_rng(seed)
    from util import dtype_kp
    k = np.zeros(n, dtype_kp)
    k["desc"] = rng.integers(0, 256, (n, 128), dtype=np.uint8)
    k["x"] = rng.random(n); k["y"] = rng.random(n)
    return k


@pytest.mark.parametrize("n1,n2", [(1000, 1500), (1, 1), (3, 1), (513, 64), (2000, 2000)])
def test_match_bit_exact(siftlib, oracle, n1, n2):
    import sift_pyocl_amd as sp
    a = _random_kp(n1, 1)
    rng = np.random.default_rng(2)
    b = _random_kp(n2, 3)
    m = min(n1, n2) // 2
    idx = rng.permutation(n1)[:m]
    noisy = np.clip(a["desc"][idx].astype(int) + rng.integers(-8, 9, (m, 128)), 0, 255).astype(np.uint8)
    b["desc"][:m] = noisy
    if n2 > 4:
        b["desc"][3] = b["desc"][2]          # exact duplicates: tie-break and dist2 == 0 paths
    mp = sp.MatchPlan()
    got = mp.match(a, b, raw_results=True)
    exp, total = oracle.match(a, b)
    assert len(got) == total
    assert np.array_equal(sort_rows(got), sort_rows(exp))
    rec = mp.match(a, b)
    assert rec.shape == (len(got), 2) and rec.dtype == mp.dtype_kp


def test_match_events_under_profile(siftlib, oracle, capsys):
    """MatchPlan.events as the reference fills it under profile=True (match.py:226, 237, 261, 263; reset at :305-310):
    (label, event) pairs whose ``profile.end - profile.start`` is the stage's device time in ns."""
    import sift_pyocl_amd as sp
    a, b = _random_kp(3000, 11), _random_kp(2500, 12)
    b["desc"][:500] = a["desc"][:500]
    mp = sp.MatchPlan(profile=True)
    got = mp.match(a, b, raw_results=True)
    exp, total = oracle.match(a, b)
    assert total == len(got) >= 500 and np.array_equal(sort_rows(got), sort_rows(exp))      # profiling does not change the result
    assert [l for l, _ in mp.events] == ["copy H->D KP_1", "copy H->D KP_2", "matching", "copy D->H match"]
    for label, evt in mp.events:
        ns = evt.profile.end - evt.profile.start
        assert 0 < ns < 1e9, (label, ns)
    assert abs(dict(mp.events)["matching"].ms - mp.kernel_ms()) < 1e-6
    mp.match(a, b)
    assert len(mp.events) == 8                     # the reference appends call after call
    mp.log_profile()
    printed = capsys.readouterr().out
    assert "matching" in printed and "copy D->H match" in printed and "Total execution time" in printed
    mp.reset_timer()
    assert mp.events == []
    # a device-resident list has no H->D copy; nothing to copy back when nothing matches
    plan = sp.SiftPlan(template=smooth_noise((256, 256)))
    kp = plan.keypoints(smooth_noise((256, 256)))
    mp.match(kp, plan.device_records(), raw_results=True)
    assert [l for l, _ in mp.events] == ["copy H->D KP_1", "matching", "copy D->H match"]
    mp.reset_timer()
    far = _random_kp(50, 13)
    far["desc"][:] = 255 - _random_kp(50, 14)["desc"] // 8
    none = mp.match(_random_kp(40, 15), far[:1], raw_results=True)          # a single list element: dist2 stays at its initial value
    assert [l for l, _ in mp.events][:3] == ["copy H->D KP_1", "copy H->D KP_2", "matching"] and len(mp.events) == 3 + (len(none) > 0)
    plain = sp.MatchPlan()
    plain.match(a, b)
    assert plain.events == []


def test_match_real_keypoints(siftlib, oracle):
    import sift_pyocl_amd as sp
    img = smooth_noise((400, 400))
    shifted = np.roll(img, (5, 8), axis=(0, 1))
    plan = sp.SiftPlan(template=img)
    k1, k2 = plan.keypoints(img), plan.keypoints(shifted)
    mp = sp.MatchPlan()
    got = mp.match(k1, k2, raw_results=True)
    exp, total = oracle.match(k1, k2)
    assert total == len(got) and np.array_equal(sort_rows(got), sort_rows(exp))
    pairs = mp.match(k1, k2)
    assert np.median(pairs[:, 1].x - pairs[:, 0].x) == 8 and np.median(pairs[:, 1].y - pairs[:, 0].y) == 5
