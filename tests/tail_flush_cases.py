"""Striped frames that make octave_tail_kernel (k_tail.hpp) flush its parking buffer inside the launch, with what the oracle
expects of them and the kernel's wave walk restated in plain Python (tests/test_tail_flush_cases_host.py proves on the CPU that
every case reaches what it is listed for; tests/test_gpu_tail_flush.py runs them).  Imports nothing from the package.

Why stripes: a frame that is constant along one axis has blurred planes that are bitwise constant along that axis, and the
extremum rule is `v >= max27` -- every sample of an extremal row (column) ties with its neighbours and is parked.  A wave of the
tail kernel parks at most SIFT_TAIL_EXT_BUF = 32 entries before it must edge-test and store them; no frame of
pyramid_cases.FRAMES ever parks more than a handful (test_parking_buffer_replay), these park up to 62 in one row.

This list stands beside pyramid_cases.FRAMES, which stays as it is."""
import collections

import numpy as np

import pyramid_cases as pc
import util

# ---- parameter sets (names of sift_pyocl_amd.param.par -> value; what is not named keeps its default)
LOW_PEAK = 255.0 * 0.0004 / 3.0
PARAMS = {
    "DEFAULT": {},
    # a ridge has det = 0 and `det < edth * tr * tr` is never true for a negative threshold: every tied sample is a candidate
    "LOW": dict(PeakThresh=LOW_PEAK, EdgeThresh=-1.0, EdgeThresh1=-1.0),
    "LOW_B2": dict(PeakThresh=LOW_PEAK, EdgeThresh=-1.0, EdgeThresh1=-1.0, BorderDist=2),     # W = 128: two full strips, 62 + 62
    "LOW_B9": dict(PeakThresh=LOW_PEAK, EdgeThresh=-1.0, EdgeThresh1=-1.0, BorderDist=9),
}


def oracle_params(oracle, name, pix_per_kp=10):
    """PARAMS[name] as the oracle's parameter block"""
    want = oracle.default_params(pix_per_kp=pix_per_kp)
    p = PARAMS[name]
    if "PeakThresh" in p:
        want.peak_thresh = np.float32(p["PeakThresh"])
    if "EdgeThresh1" in p:
        want.edge_thresh0 = np.float32(p["EdgeThresh1"])
    if "EdgeThresh" in p:
        want.edge_thresh = np.float32(p["EdgeThresh"])
    if "BorderDist" in p:
        want.border_dist = int(p["BorderDist"])
    return want


def border_of(name):
    return int(PARAMS[name].get("BorderDist", pc.BORDER))


# ---- generators: float64, cast to float32 at the end
def hstripes(shape, lam):
    H, W = shape
    col = np.cos(2.0 * np.pi * np.arange(H, dtype=np.float64) / lam)
    return np.ascontiguousarray(np.broadcast_to(col[:, None], (H, W))).astype(np.float32)


def vstripes(shape, lam):
    H, W = shape
    row = np.cos(2.0 * np.pi * np.arange(W, dtype=np.float64) / lam)
    return np.ascontiguousarray(np.broadcast_to(row[None, :], (H, W))).astype(np.float32)


def compo(shape, stripes, split, axis):
    """smooth noise in [-1, 1] with rows [:split] (axis 0) or columns [:split] (axis 1) replaced by `stripes`"""
    n = util.smooth_noise(shape, seed=3).astype(np.float64)
    img = 2.0 * (n - n.min()) / (n.max() - n.min()) - 1.0
    if axis == 0:
        img[:split] = stripes.astype(np.float64)[:split]
    else:
        img[:, :split] = stripes.astype(np.float64)[:, :split]
    return img.astype(np.float32)


# kind: "h" / "v" stripes of wavelength lam; split: None, or the rows (kind h) / columns (kind v) of a compo frame that are stripes
# flush: the first tail octave listed in `octaves` must flush (False: it must only carry); octaves: the tail octaves (W, H) the
# case is meant to use, first one first; watch: index into `octaves` of the octave the case is there for
Case = collections.namedtuple("Case", "name shape kind lam split par pix_per_kp flush octaves watch")

_T128 = [(64, 64), (32, 32), (16, 16)]
_T118 = [(57, 59), (28, 29), (14, 14)]
CASES = [
    Case("h128_l24", (128, 128), "h", 24, None, "LOW", 10, True, _T128, 0),
    Case("v128_l20", (128, 128), "v", 20, None, "LOW", 10, True, _T128, 0),
    Case("v128_l28", (128, 128), "v", 28, None, "LOW", 10, True, _T128, 0),
    Case("h118x114_l20", (118, 114), "h", 20, None, "LOW", 10, True, _T118, 0),
    Case("v118x114_l24", (118, 114), "v", 24, None, "LOW", 10, True, _T118, 0),
    Case("h64x256_l20", (64, 256), "h", 20, None, "LOW", 10, True, [(128, 32), (64, 16)], 0),        # two strip columns
    Case("v64x256_l20", (64, 256), "v", 20, None, "LOW", 10, True, [(128, 32), (64, 16)], 0),
    Case("v256x64_l20", (256, 64), "v", 20, None, "LOW", 10, True, [(32, 128), (16, 64)], 0),        # four strips per wave
    Case("h64x256_l40", (64, 256), "h", 40, None, "LOW", 10, True, [(128, 32), (64, 16)], 1),        # second tail octave, 64 x 16
    Case("h128_l40", (128, 128), "h", 40, None, "LOW", 10, False, _T128, 1),                         # 32 x 32: carry only
    Case("compo_h128_l24", (128, 128), "h", 24, 84, "LOW", 10, True, _T128, 0),
    Case("compo_v128_l24", (128, 128), "v", 24, 84, "LOW", 10, True, _T128, 0),
    # (the two above leave 11 and 8 records of tail octaves; these two flush AND refine more than 20 tail candidates into records)
    Case("compo_h64x256_l20", (64, 256), "h", 20, 42, "LOW", 10, True, [(128, 32), (64, 16)], 0),
    Case("compo_v64x256_l20", (64, 256), "v", 20, 85, "LOW", 10, True, [(128, 32), (64, 16)], 0),
    Case("compo_h128_l24_default", (128, 128), "h", 24, 84, "DEFAULT", 10, True, _T128, 0),
    # (under DEFAULT the edge test at the end of every strip empties what a column of ties parked: 224 parked, never 33 at once)
    Case("compo_v128_l24_default", (128, 128), "v", 24, 84, "DEFAULT", 10, False, _T128, 0),
    Case("h128_l24_default", (128, 128), "h", 24, None, "DEFAULT", 10, True, _T128, 0),              # every flush stores nothing
    Case("h64x256_l20_b2", (64, 256), "h", 20, None, "LOW_B2", 10, True, [(128, 32), (64, 16)], 0),  # both strips full, rows from y = 2
    Case("v128_l20_b9", (128, 128), "v", 20, None, "LOW_B9", 10, True, _T128, 0),
    Case("v128_l20_ppk60", (128, 128), "v", 20, None, "LOW", 60, True, _T128, 0),                    # kpsize = 273 < the tail's candidates
    Case("h512_l104", (512, 512), "h", 104, None, "LOW", 10, True, _T128, 0),                        # tail_first = 3 behind forked chains
]
BY_NAME = {c.name: c for c in CASES}


def image(case):
    maker = hstripes if case.kind == "h" else vstripes
    stripes = maker(case.shape, case.lam)
    if case.split is None:
        return stripes
    return compo(case.shape, stripes, case.split, 0 if case.kind == "h" else 1)


Expect = collections.namedtuple("Expect", "sizes planes cands c_scale raw records overflow")
_CACHE = {}


def candidates(oracle, dogs, octsize, par):
    """[(n, 4)] candidates (value, row, col, scale) of the three detection scales under `par`"""
    _, h, w = dogs.shape
    per = []
    for s in (1, 2, 3):
        k, n = oracle.local_maxmin(dogs, s, octsize, 3 * w * h, par)
        per.append(k[:n])
    return per


def unfiltered_candidates(oracle, dogs, octsize, par):
    """pyramid_cases.unfiltered_candidates for any `par`: the 27-neighbour extrema above its contrast threshold inside its
    border BEFORE the edge test -- what a wave parks while it marches (edge thresholds of -inf: `det < thresh * tr * tr` is
    never true)."""
    raw = oracle_copy(par)
    raw.edge_thresh0 = raw.edge_thresh = -np.inf
    return np.concatenate(candidates(oracle, dogs, octsize, raw))


def oracle_copy(par):
    return type(par).from_buffer_copy(par)


def expectations(oracle, case):
    """What the oracle makes of a case, computed once: Expect(sizes [(W, H)], planes [(6, H, W)] per octave, cands [(n, 4)] per
    octave, c_scale (octaves, 3), raw [(n, 4) extrema before the edge test] per octave, records, overflow).  Shared between
    tests: treat as read-only."""
    if case.name not in _CACHE:
        img = image(case)
        H, W = case.shape
        par = oracle_params(oracle, case.par, case.pix_per_kp)
        planes, cands, counts, raws = [], [], [], []
        for o, (blurs, dogs) in enumerate(util.oracle_pyramid(oracle, img, oracle.octave_count(H, W))):
            per = candidates(oracle, dogs, 2 ** o, par)
            blurs.setflags(write=False)
            planes.append(blurs)
            cands.append(np.concatenate(per))
            counts.append([len(k) for k in per])
            raws.append(unfiltered_candidates(oracle, dogs, 2 ** o, par))
        records, overflow = oracle.keypoints(img, par=par, return_overflow=True)
        _CACHE[case.name] = Expect([(p.shape[2], p.shape[1]) for p in planes], planes, cands,
                                   np.array(counts, np.int32).reshape(-1, 3), raws, records, overflow)
    return _CACHE[case.name]


# ---- the tail kernel's wave walk (k_tail.hpp, extrema_strip of k_extrema.hpp with BUF = SIFT_TAIL_EXT_BUF)
Flush = collections.namedtuple("Flush", "wave sx sy row parked carried row_parked stored")
Replay = collections.namedtuple("Replay", "flushes final max_row stored_after_flush")


def _keys(rows):
    return [tuple(int(v) for v in r) for r in np.ascontiguousarray(rows[:, 1:4]).astype(np.int64)]


def replay(raw, kept, W, H, border):
    """The walk of the eight waves over an octave W x H whose extrema before the edge test are `raw` and whose candidates are
    `kept` (an entry of `raw` survives the edge test iff it is in `kept`).  Wave w takes strips w, w + 8, ... of 62 columns x
    4 rows (strip id = sy * nx + sx) and goes through a strip row by row.  After each row: more than 32 entries parked -> the
    entries from `tested` on are edge-tested, everything left is stored, the wave starts again from pending = tested = 0.  At
    the end of a strip the untested entries are edge-tested and the survivors stay parked into the next strip (tested = pending
    at its start).  What a wave still holds after its last strip is stored then.
    Returns Replay(flushes [Flush(wave, sx, sy, row, parked = entries at the flush, carried = those that came from earlier strips,
    row_parked = entries the row added, stored = survivors)], final (8,) entries per wave at its end, max_row = the most
    entries a row of a strip parks, stored_after_flush = waves that flushed and hold survivors at their end)."""
    if not (W > 2 * border and H > 2 * border):
        return Replay([], np.zeros(pc.TAIL_WAVES, np.int64), 0, 0)
    keep = set(_keys(kept))
    by_row = collections.defaultdict(list)             # (row, strip column) -> [survives?]
    for key in _keys(raw):
        by_row[(key[0], (key[1] - border) // 62)].append(key in keep)
    nx = (W - 2 * border + 61) // 62
    ny = (H - 2 * border + pc.TAIL_STRIP_ROWS - 1) // pc.TAIL_STRIP_ROWS
    flushes, final, max_row, after = [], np.zeros(pc.TAIL_WAVES, np.int64), 0, 0
    for wave in range(pc.TAIL_WAVES):
        pending, flushed = 0, False
        for wid in range(wave, nx * ny, pc.TAIL_WAVES):
            sx, sy = wid % nx, wid // nx
            tested, untested = pending, []             # what is parked at the start of a strip has had its edge test
            ya = border + sy * pc.TAIL_STRIP_ROWS
            for yc in range(ya, min(ya + pc.TAIL_STRIP_ROWS, H - border)):
                row = by_row.get((yc, sx), [])
                max_row = max(max_row, len(row))
                untested += row
                pending = tested + len(untested)
                if pending > pc.TAIL_EXT_BUF:
                    stored = tested + sum(untested)
                    flushes.append(Flush(wave, sx, sy, yc, pending, tested, len(row), stored))
                    pending, tested, untested, flushed = 0, 0, [], True
            pending = tested + sum(untested)
        final[wave] = pending
        after += int(flushed and pending > 0)
    assert sum(f.stored for f in flushes) + final.sum() == len(kept), "the replay lost or invented candidates"
    return Replay(flushes, final, max_row, after)
