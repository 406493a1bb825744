"""What tests/test_gpu_warp_cases.py rests on, checked without a GPU: the numpy restatement of the warp (tests/warp_ref.py) equals
the oracle bit for bit on every crafted case (tests/warp_cases.py) and the reference's own kernels on the golden vectors
(tests/golden/transform.npz), and every case reaches the path it is there for."""
import os

import numpy as np
import pytest

import warp_cases as wc
from util import TRANSFORM_CASES, transform_inputs
from warp_ref import CLASSES, coords, same, warp_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transform.npz")
F = np.float32


@pytest.mark.parametrize("family", range(1, 9))
def test_restatement_equals_oracle(oracle, family):
    n = 0
    for c in wc.cases():
        if c.family != family:
            continue
        img = wc.image(c.image)
        want, counts = warp_ref(img, c.M, c.off, c.out_shape, c.fill, c.mode)
        got = oracle.transform(img, c.M, c.off, out_shape=c.out_shape, fill=c.fill, mode=c.mode)
        assert same(got, want, nan_any_payload=family == 8), c.name
        wc.check_expect(c, counts)
        n += 1
    assert n >= 4


def test_restatement_equals_golden():
    g = np.load(GOLDEN)
    gray, rgb = transform_inputs()
    for i, (M, off, fill, mode, extra) in enumerate(TRANSFORM_CASES):
        for key, img in (("gray%d" % i, gray), ("rgb%d" % i, rgb)):
            oshape = tuple(s + e for s, e in zip(img.shape[:2], extra or (0, 0)))
            assert same(warp_ref(img, M, off, oshape, fill, mode)[0], g[key]), key


def test_every_class_is_reached_in_gray_and_rgb():
    total = {False: dict.fromkeys(CLASSES, 0), True: dict.fromkeys(CLASSES, 0)}
    for c in wc.cases():
        if c.mode != 1:
            continue                                             # the taps beside the top-left one only matter to the bilinear mode
        counts = warp_ref(wc.image(c.image), c.M, c.off, c.out_shape, c.fill, c.mode)[1]
        for k, v in counts.items():
            total[wc.is_rgb(c)][k] += v
    for rgb in (False, True):
        for k in CLASSES:
            assert total[rgb][k] > 0, (rgb, k)


def test_lattice_reaches_every_boundary_value():
    """tx in {-0.25, -0.0, 0, W-1, W-0.75, W-0.5, W-0.25, W} and the same in ty, each exactly, each with the other coordinate
    inside the image (so the value decides the pixel), over the lattice family"""
    H, W = wc.SHAPE
    seen_x, seen_y = set(), set()
    for c in wc.cases():
        if c.family != 2 or c.image[0] != "gray" or c.mode != 1:
            continue
        ty, tx = coords(c.M, c.off, c.out_shape)
        y_in = (0 <= ty) & (ty < H - 0.5); x_in = (0 <= tx) & (tx < W - 0.5)
        for kind, v in wc.LATTICE_VALUES:
            for t, size, other_in, seen in ((tx, W, y_in, seen_x), (ty, H, x_in, seen_y)):
                target = F(v if kind == "abs" else size + v)
                hit = (t == target) & (np.signbit(t) == np.signbit(target)) & other_in
                if hit.any():
                    seen.add((kind, v, bool(np.signbit(target))))
    want = {(kind, v, bool(np.signbit(F(v))) if kind == "abs" else False) for kind, v in wc.LATTICE_VALUES}
    assert len(want) == 8
    assert seen_x == want and seen_y == want


def test_half_below_rounds_up_per_operation():
    """x + nextafter(0.5f, 0) is x + 0.5 in float32 from x = 1 on: the per-operation rounding the contract promises puts the
    last column at W - 0.5 exactly, where the cut takes it"""
    H, W = wc.SHAPE
    c = wc.by_name("f2-half_below-gray-m1")
    ty, tx = coords(c.M, c.off, c.out_shape)
    assert tx[0, 0] == F(wc.HALF_BELOW) and tx[0, 0] < F(0.5)
    assert np.array_equal(tx[0, 1:], np.arange(1, W, dtype=F) + F(0.5))
    assert float(np.float64(W - 1) + np.float64(wc.HALF_BELOW)) < W - 0.5


def test_case_list_is_what_the_gpu_test_expects():
    cs = wc.cases()
    assert {c.family for c in cs} == set(range(1, 9))
    for c in cs:
        H, W = c.image[1]
        assert (H <= 97 and W <= 131) or c.image[1] == wc.BIG, c.name
        assert c.out_shape[1] <= 1030 and c.out_shape[0] <= 303
        if wc.is_rgb(c):
            assert 0.0 <= c.fill <= 255.0, "an RGB fill outside [0, 255] is undefined"
    assert sum(c.image[1] == wc.BIG for c in cs) == 1
    f5 = {c.out_shape for c in cs if c.family == 5 and c.image[0] == "rgb"}
    assert {ow for _, ow in f5} >= set(wc.OUT_WIDTHS) and {oh for oh, _ in f5} >= set(wc.OUT_HEIGHTS)
    # both RGB store paths in every row alignment: a full group of 4 pixels whose row segment starts at byte 0..3 mod 4
    aligns = {(3 * y * ow) % 4 for oh, ow in f5 if ow >= 4 for y in range(oh)}
    assert aligns == {0, 1, 2, 3}
    assert {c.mode for c in cs if c.family == 3} == set(wc.MODES)
    assert {c.image[1] for c in cs if c.family == 6} == set(wc.TINY)
    assert {c.fill for c in cs if c.family == 7} == set(wc.FILLS)
    for pat in wc.POINTER_CASES:
        for kind in ("gray", "rgb"):
            wc.by_name(pat % kind)
