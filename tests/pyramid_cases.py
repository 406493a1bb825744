"""Frames whose whole pyramid is compared with the oracle at plan level (tests/test_gpu_pyramid_cases.py), with what the
oracle expects of them, and the rules those tests rest on restated in plain Python (tests/test_pyramid_cases_host.py checks the
restatements without a GPU).  Imports nothing from the package.

Why planes and not records: a small octave seldom has a candidate (octaves of 32 x 32 samples and below: none on any frame
here), and without a candidate there is no record -- every float octave_tail_kernel writes for such an octave could be wrong
and a comparison of records would pass.  The reflected margins are hidden twice, the detection border (5) excludes the samples
they reach first."""
import collections

import numpy as np

import util

BORDER = 5                       # par.BorderDist
TAIL_PIXELS = 4096               # SIFT_TAIL_MAX_PIXELS (k_tail.hpp), the default of option "tail_pixels"
TAIL_MAX_OCT = 6                 # SIFT_TAIL_MAX_OCT
TAIL_EXT_BUF = 32                # SIFT_TAIL_EXT_BUF: candidates a wave of the tail kernel parks before it flushes
TAIL_WAVES = 8                   # SIFT_TAIL_THREADS / 64
TAIL_STRIP_ROWS = 4              # rows of an extrema strip in the tail kernel (62 columns wide)

Frame = collections.namedtuple("Frame", "name shape maker seed dtype")

# (H, W); see the table in the module docstring of tests/test_gpu_pyramid_cases.py for what each shape is there for
FRAMES = [
    Frame("smooth128", (128, 128), "smooth_noise", 11, "float32"),
    Frame("white128", (128, 128), "white_noise", 12, "float32"),
    Frame("multi112", (112, 112), "multiscale_noise", 13, "float32"),
    Frame("smooth111", (111, 111), "smooth_noise", 14, "float32"),
    Frame("smooth64x256", (64, 256), "smooth_noise", 15, "float32"),
    Frame("white64x256", (64, 256), "white_noise", 16, "float32"),
    Frame("multi256x64", (256, 64), "multiscale_noise", 17, "float32"),
    Frame("smooth58x280", (58, 280), "smooth_noise", 18, "float32"),
    Frame("multi56x300", (56, 300), "multiscale_noise", 19, "float32"),
    Frame("smooth300x56", (300, 56), "smooth_noise", 20, "float32"),
    Frame("multi130x250", (130, 250), "multiscale_noise", 21, "float32"),
    Frame("smooth114x118", (114, 118), "smooth_noise", 22, "float32"),
    Frame("white118x114", (118, 114), "white_noise", 23, "float32"),
    Frame("smooth512", (512, 512), "smooth_noise", 24, "float32"),
    Frame("multi1400", (1400, 1400), "multiscale_noise", 25, "float32"),
    Frame("multi1400u8", (1400, 1400), "multiscale_noise", 25, "uint8"),
]
BY_NAME = {f.name: f for f in FRAMES}
MARCHING = ("multi1400", "multi1400u8")          # the frames whose octave 0 takes the marching blur: seconds, not milliseconds
SMALL_FRAMES = [f for f in FRAMES if f.name not in MARCHING]

# tail octaves (W, H) every frame is MEANT to use under the default options, first one first ([]: the tail must refuse)
TAIL_OCTAVES = {
    "smooth128": [(64, 64), (32, 32), (16, 16)], "white128": [(64, 64), (32, 32), (16, 16)],
    "multi112": [(56, 56), (28, 28), (14, 14)],          # side 14 under 27 taps
    "smooth111": [],                                     # the last octave is 13 x 13
    "smooth64x256": [(128, 32), (64, 16)], "white64x256": [(128, 32), (64, 16)],      # 66 560 bytes of LDS, W = 128
    "multi256x64": [(32, 128), (16, 64)],                # 68 864 bytes, H = 128
    "smooth58x280": [(70, 14)],                          # octave 1 is 140 x 29 = 4060 samples, but W > 128
    "multi56x300": [(75, 14)], "smooth300x56": [(14, 75)],      # octave 1 has 4200 samples: a single tail octave
    "multi130x250": [(62, 32), (31, 16)], "smooth114x118": [(59, 57), (29, 28), (14, 14)],
    "white118x114": [(57, 59), (28, 29), (14, 14)],      # W % 4 = 1, 2, 3 pitches, odd last columns, odd heights
    "smooth512": [(64, 64), (32, 32), (16, 16)],         # six octaves, forked chains, tail_first = 3
    "multi1400": [(43, 43), (21, 21)], "multi1400u8": [(43, 43), (21, 21)],
}


def image(frame):
    """The frame as the plan is given it (float32, or uint8 stretched over 0..255)."""
    img = getattr(util, frame.maker)(frame.shape, seed=frame.seed)
    if frame.dtype == "uint8":
        img = np.rint(255.0 * (img - img.min()) / (img.max() - img.min())).astype(np.uint8)
    return img


def octave_sizes(H, W, border=BORDER):
    """[(W, H)] of every octave (plan.py:213-224: halve while the smaller side exceeds 2 * BorderDist + 2, drop the last)."""
    sizes, w, h = [(W, H)], W, H
    while min(w, h) > 2 * border + 2:
        w, h = w // 2, h // 2
        sizes.append((w, h))
    sizes.pop()
    return sizes


def tail_first(sizes, tail=1, tail_pixels=TAIL_PIXELS):
    """tail_first_octave (siftmi.hip) restated: the first octave the one-launch form takes, len(sizes) when it takes none.  An
    octave >= 1 joins if W * H <= tail_pixels, W <= 128 and H <= 128, from the last octave upwards (at most TAIL_MAX_OCT of
    them); the last octave's sides must be >= 14 (the reflection of a 27-tap blur stays inside the plane)."""
    n = len(sizes)
    if not tail or n < 2 or min(sizes[-1]) < 14:
        return n
    first = n
    for o in range(n - 1, 0, -1):
        w, h = sizes[o]
        if w * h > tail_pixels or w > 128 or h > 128 or n - o > TAIL_MAX_OCT:
            break
        first = o
    return first


def march_plane(W, H):
    """planes of the marching blur (siftmi.hip: march_plane); their detection keeps a candidate list under the default options"""
    return W >= 1024 and H >= 512 and W * H >= 1400 * 1400


def listed_octaves(sizes, first, fused_refine=1):
    """Octaves whose detection appends to a candidate list, so that `candidates` of SiftPlan.last_counts() counts them: the
    tail's octaves, and those of the two-launch detection (option "fused_refine": 0 every octave, 1 the marching planes, 2
    none).  The fused detect-and-refine launch refines what a wave parked and keeps no list: its counter stays 0."""
    return [o >= first or fused_refine == 0 or (fused_refine == 1 and march_plane(*sizes[o])) for o in range(len(sizes))]


Expect = collections.namedtuple("Expect", "sizes planes cands c_scale")
_CACHE = {}


def expectations(oracle, frame):
    """What the oracle makes of a frame, computed once: Expect(sizes [(W, H)], planes [(6, H, W)] per octave, cands [(n, 4)
    candidates (value, row, col, scale) of the three scales together] per octave, c_scale (octaves, 3) their count per scale).
    Shared between tests: treat as read-only."""
    if frame.name not in _CACHE:
        img = np.ascontiguousarray(image(frame), np.float32)
        H, W = frame.shape
        n_oct = oracle.octave_count(H, W)
        planes, cands, counts = [], [], []
        par = oracle.default_params()
        for o, (blurs, dogs) in enumerate(util.oracle_pyramid(oracle, img, n_oct)):
            _, h, w = blurs.shape
            per = []
            for s in (1, 2, 3):
                k, n = oracle.local_maxmin(dogs, s, 2 ** o, 3 * w * h, par)
                per.append(k[:n])
            blurs.setflags(write=False)
            planes.append(blurs)
            cands.append(np.concatenate(per))
            counts.append([len(k) for k in per])
        _CACHE[frame.name] = Expect([(p.shape[2], p.shape[1]) for p in planes], planes, cands, np.array(counts, np.int32).reshape(-1, 3))
    return _CACHE[frame.name]


def unfiltered_candidates(oracle, dogs, octsize):
    """The 27-neighbour extrema above the contrast threshold BEFORE the edge test -- what a wave parks while it marches a strip
    (the edge test runs on the parked entries at the end of the strip, or when the buffer is full): local_maxmin with edge
    thresholds of -inf, under which `det < thresh * tr * tr` is never true."""
    par = oracle.default_params()
    par.edge_thresh0 = par.edge_thresh = -np.inf
    _, h, w = dogs.shape
    per = []
    for s in (1, 2, 3):
        k, n = oracle.local_maxmin(dogs, s, octsize, 3 * w * h, par)
        per.append(k[:n])
    return np.concatenate(per)


def wave_totals(cand, W, H):
    """The tail kernel's wave walk replayed on a candidate list: strips of 62 columns x 4 rows inside the border, wave w takes
    strips w, w + 8, ... and carries what it parked from strip to strip (`pending`).  Returns (candidates per wave (8,), strips
    with a candidate per wave (8,))."""
    counts = util.strip_candidate_counts(cand, W, H, BORDER, TAIL_STRIP_ROWS)
    ny, nx = counts.shape
    flat = counts.reshape(-1)                      # strip id = sy * nx + sx, as the kernel's wid
    total, strips = np.zeros(TAIL_WAVES, np.int64), np.zeros(TAIL_WAVES, np.int64)
    for w in range(TAIL_WAVES):
        mine = flat[w::TAIL_WAVES]
        total[w], strips[w] = mine.sum(), (mine > 0).sum()
    return total, strips


def check_left_behind(plan, exp, what, tail_first, fused_refine=1):
    """Everything a finished keypoints() call left behind on `plan` against an Expect-like `exp` (sizes, planes, c_scale): the
    first tail octave, all six planes of every octave, the candidates per octave and scale, the candidates per octave wherever
    detection keeps a list -- uint32 / integer equality.  Returns plan.last_counts()."""
    counts = plan.last_counts()
    n_oct = len(exp.sizes)
    assert counts["tail_first"] == tail_first, "%s: the tail launch took octaves from %d on, not from %d (of %d)" % (
        what, counts["tail_first"], tail_first, n_oct)
    for o in range(n_oct):
        bad = plane_mismatch(plan.planes(o), exp.planes[o], o)
        assert bad is None, "%s: %s" % (what, bad)
    assert counts["c_scale"].shape == (n_oct, 3)
    assert np.array_equal(counts["c_scale"], exp.c_scale), "%s: candidates per octave and scale %r, oracle %r" % (
        what, counts["c_scale"].tolist(), np.asarray(exp.c_scale).tolist())
    # candidates per octave == the per-scale sum wherever detection keeps a candidate list (every tail octave does); the fused
    # detect-and-refine launch keeps none and must leave its counter at 0 (listed_octaves)
    listed = listed_octaves(exp.sizes, tail_first, fused_refine)
    want = [int(exp.c_scale[o].sum()) if listed[o] else 0 for o in range(n_oct)]
    assert counts["candidates"] == want, "%s: candidates per octave %r, expected %r (octaves with a list: %r)" % (
        what, counts["candidates"], want, listed)
    return counts


def plane_mismatch(got, want, octave):
    """None, or the message of the first plane of an octave that differs bit for bit: octave, plane, the first differing (y, x),
    the number of differing samples."""
    if got.shape != want.shape:
        return "octave %d: planes of shape %r, expected %r" % (octave, got.shape, want.shape)
    g, w = got.view(np.uint32), want.view(np.uint32)
    for s in range(want.shape[0]):
        bad = np.argwhere(g[s] != w[s])
        if len(bad):
            y, x = (int(v) for v in bad[0])
            return "octave %d (%d x %d) plane %d: %d of %d samples differ, first at (y, x) = (%d, %d): %r, expected %r" % (
                octave, want.shape[2], want.shape[1], s, len(bad), g[s].size, y, x, got[s, y, x], want[s, y, x])
    return None
