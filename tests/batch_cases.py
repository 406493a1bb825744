"""Cases of the batch keypoint path's hand-back (siftmi_batch_keypoints[_into], siftmi_batch_fetch, siftmi_batch_minmax): the
frames, capacities and record ranges that tests/test_batch_cases_host.py (CPU, on the oracle alone) and
tests/test_gpu_batch_cases.py (MI355X) share.  Plain helpers, numpy only, no fixtures.

What the round-trip tests of tests/test_gpu_batch.py cannot see is WHICH path carried a frame's records: batch_retire
(csrc/siftmi.hip) copies frame i into the caller's array when `host_outs[i] && n <= host_caps[i]` and parks it in the device
arena otherwise, the arena is regrown with records already in it, and siftmi_batch_fetch serves any range of it.  The cases
here prescribe the path of every frame from the oracle's counts, so the GPU tests can assert it.

A frame is a hashable spec, ("smooth", seed), ("white", seed), ("lattice", seed) or ("const", value), of a given shape;
frame() builds it and oracle_of() gives its records, (min, max) and overflow flag, computed once per process.  Frames with
records have pairwise different record sets and every frame has its own (min, max) -- constant frames have no record and are
told apart by (min, max) alone -- so a swapped, repeated or dropped frame shows in one of the two.
"""
import numpy as np

from util import lattice, smooth_noise, sort_kp, white_noise

RECORD_BYTES = 144
SMALL = (131, 97)                      # H, W of the small cases: several blocks, no multiple of any tile
MID = (256, 256)                       # the overflow-flag cases
BIG = (512, 512)                       # the arena cases and the Python tests
SMALL_LANES = (1, 2, 3, 5)             # 5: the single-stream lane mode (lanes >= 4, siftmi_batch_create)
ARENA_LANES = (1, 3)                   # at 5 lanes the warm-up alone would outgrow the arena's first 4 MiB
ARENA_START = 1 << 22                  # batch_retire: the arena's first size, 29 127 records
GUARD = 8                              # records behind host_outs[i][cap] that must stay untouched
FILL = 0xa5
NULL_CAP = 1 << 20                     # the capacity given with a null host_outs[i]
OVERFLOW_PIX_PER_KP = 60               # kpsize 1092 at 256 x 256: the oracle flags the lattice frame (1627 records) only

# capacity classes of one frame with n records (what batch_retire must do with it)
CAP_BELOW, CAP_EXACT, CAP_ABOVE, CAP_ZERO_EMPTY, CAP_ZERO_FULL, CAP_NULL = "n-1", "n", "n+1", "0,n=0", "0,n>0", "null"
CAP_CLASSES = (CAP_BELOW, CAP_EXACT, CAP_ABOVE, CAP_ZERO_EMPTY, CAP_ZERO_FULL, CAP_NULL)
# the order in which a row of a capacity matrix deals them out: parked and delivered frames alternate
_DEAL = (CAP_BELOW, CAP_EXACT, CAP_NULL, CAP_ABOVE, CAP_ZERO_FULL, CAP_ZERO_EMPTY)


# ------------------------------------------------------------------------------------------------ frames and the oracle
def frame(spec, shape):
    kind, arg = spec
    if kind == "smooth":
        return smooth_noise(shape, seed=arg)
    if kind == "flat":                                  # few records on a large frame
        return smooth_noise(shape, seed=arg, sigma=24.0)
    if kind == "white":
        return white_noise(shape, seed=arg)
    if kind == "lattice":
        return lattice(shape, seed=arg)
    if kind == "const":
        return np.full(shape, arg, np.float32)
    raise ValueError(spec)


_FRAMES, _ORACLE = {}, {}


def frame_of(spec, shape):
    """frame(), built once and never written to"""
    key = (spec, tuple(shape))
    if key not in _FRAMES:
        f = np.ascontiguousarray(frame(spec, shape), np.float32)
        f.setflags(write=False)
        _FRAMES[key] = f
    return _FRAMES[key]


def oracle_of(spec, shape, pix_per_kp=None):
    """(records sorted as util.sort_kp, (min, max), overflow flag) of a frame from the oracle, computed once"""
    key = (spec, tuple(shape), pix_per_kp)
    if key not in _ORACLE:
        from oracle import pyoracle
        pyoracle.build()
        par = pyoracle.default_params()
        if pix_per_kp is not None:
            par.pix_per_kp = int(pix_per_kp)
        f = frame_of(spec, shape)
        k, ovf = pyoracle.keypoints(f, par, return_overflow=True)
        k = np.ascontiguousarray(sort_kp(k)) if len(k) else np.asarray(k)
        k.setflags(write=False)
        _ORACLE[key] = (k, pyoracle.minmax(f), bool(ovf))
    return _ORACLE[key]


def counts_of(specs, shape, pix_per_kp=None):
    return [len(oracle_of(s, shape, pix_per_kp)[0]) for s in specs]


def record_bytes(k):
    """records in the order of util.sort_kp, as (n, 144) bytes"""
    k = np.asarray(k)
    if len(k) == 0:
        return np.empty((0, RECORD_BYTES), np.uint8)
    return np.ascontiguousarray(sort_kp(k)).view(np.uint8).reshape(len(k), RECORD_BYTES)


# ------------------------------------------------------------------------------------------------ small cases
# blank, rich and sparse frames in turn, so that any three neighbours hold one of each; eleven frames is the longest batch
# (2 * 5 + 1)
_POOL = (("const", 0.0), ("smooth", 201), ("white", 101), ("const", 3.5), ("lattice", 1), ("white", 102),
         ("const", -2.25), ("smooth", 202), ("white", 103), ("const", 100.0), ("smooth", 203), ("white", 105))


def batch_sizes(lanes):
    """n_images around `lanes` and 2 * lanes: a lane retires in the main loop when it is reused, in the closing loop otherwise"""
    L = lanes
    return sorted({n for n in (1, L - 1, L, L + 1, 2 * L, 2 * L + 1) if n > 0})


def small_batch(lanes, n_images):
    """the frame specs of the batch of `n_images` frames on `lanes` lanes: a run of the pool that starts somewhere else for
    every batch, so that blank, sparse and rich frames meet every lane and every position"""
    start = (3 * lanes + n_images) % len(_POOL)
    return [_POOL[(start + i) % len(_POOL)] for i in range(n_images)]


def cap_class_for(n, wanted):
    """the class a frame with n records gets when the deal says `wanted`: a class that needs records falls to its sibling
    without, and the other way round"""
    if n == 0 and wanted in (CAP_BELOW, CAP_ZERO_FULL):
        return CAP_ZERO_EMPTY
    if n > 0 and wanted == CAP_ZERO_EMPTY:
        return CAP_ZERO_FULL
    return wanted


def cap_of(n, cls):
    """(capacity, host_outs[i] is null) of a frame with n records in class `cls`"""
    return {CAP_BELOW: (n - 1, False), CAP_EXACT: (n, False), CAP_ABOVE: (n + 1, False), CAP_ZERO_EMPTY: (0, False),
            CAP_ZERO_FULL: (0, False), CAP_NULL: (NULL_CAP, True)}[cls]


def cap_matrix(counts):
    """six rows, one per call: row r gives frame i the class _DEAL[(i + r) % 6] (cap_class_for), so every frame meets every
    class it can have and neighbours differ.  Each entry is (class, capacity, null)."""
    rows = []
    for r in range(len(_DEAL)):
        row = []
        for i, n in enumerate(counts):
            cls = cap_class_for(n, _DEAL[(i + r) % len(_DEAL)])
            row.append((cls,) + cap_of(n, cls))
        rows.append(row)
    return rows


def delivered(counts, row):
    """batch_retire's rule: frame i goes to the caller's array iff the array is there and the count fits"""
    return [(not null) and n <= cap for n, (_, cap, null) in zip(counts, row)]


def expected_offsets(counts, row):
    """(offsets, total_parked): -1 for a delivered frame, else the sum of the parked counts before it, in input order"""
    offs, at = [], 0
    for n, d in zip(counts, delivered(counts, row)):
        offs.append(-1 if d else at)
        at += 0 if d else n
    return offs, at


def has_between(flags, inner):
    """a frame with delivered == inner between two frames with delivered != inner"""
    return any(flags[i] == inner and flags[i - 1] != inner and flags[i + 1] != inner for i in range(1, len(flags) - 1))


class SmallCase(object):
    """every batch of one lane count: batches = [(n_images, specs, oracle counts, capacity matrix)]"""

    def __init__(self, lanes):
        self.lanes = lanes
        self.batches = []
        for n in batch_sizes(lanes):
            specs = small_batch(lanes, n)
            counts = counts_of(specs, SMALL)
            self.batches.append((n, specs, counts, cap_matrix(counts)))

    def batch(self, n_images):
        return [b for b in self.batches if b[0] == n_images][0]

    def specs(self):
        """the distinct frames of the case"""
        seen = []
        for _, specs, _, _ in self.batches:
            seen += [s for s in specs if s not in seen]
        return seen


_SMALL = {}


def small_case(lanes):
    if lanes not in _SMALL:
        _SMALL[lanes] = SmallCase(lanes)
    return _SMALL[lanes]


def small_ids():
    """[(lanes, n_images)] of every small batch"""
    return [(L, n) for L in SMALL_LANES for n in batch_sizes(L)]


def shorter_batch(lanes, n_images):
    """the batch run after (lanes, n_images) on the same handle: fewer frames than lanes where that is possible, so that lanes
    stay idle and the arrays are sized for a smaller batch; other frames than the batch before, in another order"""
    n = max(1, min(n_images, lanes) - 1)
    specs = small_batch(lanes, n_images)[::-1]
    rest = [s for s in _POOL[::-1] if s not in specs]
    return (rest + specs)[:n]


# ------------------------------------------------------------------------------------------------ arena cases
ARENA_MAIN = [("flat", 301), ("flat", 302), ("flat", 303)] + [("lattice", s) for s in (1, 2, 3, 4, 5)]


def arena_warmup(lanes):
    """L lattice frames, none of them in the main batch: every lane's lists finish growing, the arena stays at its first size"""
    return [("lattice", 11 + l) for l in range(lanes)]


def arena_replay(counts, cap=0):
    """batch_retire's growth rule restated on the counts of a batch whose frames all park (they retire in input order):
    returns (events, cap) with events = [(frame, records parked before it, new size in bytes)], one per allocation.  The arena
    starts at 1 << 22 and doubles while it is below `need` or below need / (retired + 1) * batch_size * 1.25."""
    used, events = 0, []
    for r, n in enumerate(counts):
        need = used + n * RECORD_BYTES
        if need > cap:
            c = cap if cap else ARENA_START
            projected = int(float(need) / float(r + 1) * float(len(counts)) * 1.25)
            while c < need or c < projected:
                c *= 2
            events.append((r, used // RECORD_BYTES, c))
            cap = c
        used = need
    return events, cap


# ------------------------------------------------------------------------------------------------ fetch ranges
def fetch_ranges(offsets, counts):
    """(accepted, refused) ranges (first, count) of T parked records, frame i at [offsets[i], offsets[i] + counts[i]);
    delivered frames (offset -1) have no range"""
    parked = [(o, c) for o, c in zip(offsets, counts) if o >= 0]
    T = sum(c for _, c in parked)
    accepted = [(0, 0), (T, 0), (0, T)] + parked
    accepted += [(o + c - 1, 2) for o, c in parked if c > 0 and o + c + 1 <= T]        # across a frame boundary
    accepted += [(T - 1, 1)] if T > 0 else []
    refused = [(T, 1), (0, T + 1), (-1, 1), (0, -1), (1 << 62, 1 << 62), ((1 << 63) - 1, 1), (1, (1 << 63) - 1)]
    return accepted, refused


def range_accepted(first, count, T):
    """the contract of siftmi_batch_fetch on integers of any size"""
    return first >= 0 and count >= 0 and first + count <= T


def old_range_check_accepts(first, count, arena_used):
    """the check siftmi_batch_fetch used to make, `(size_t)(first + count) * 144 > arena_used` refused, in the 64-bit
    arithmetic of the C expression (the signed sum wraps, the product is taken modulo 2^64)"""
    if first < 0 or count < 0:
        return False
    s = (first + count) & ((1 << 64) - 1)
    return (s * RECORD_BYTES) & ((1 << 64) - 1) <= arena_used


# ------------------------------------------------------------------------------------------------ overflow-flag cases
OVERFLOW_FLAGGED = ("lattice", 5)
OVERFLOW_PLAIN = [("smooth", 401), ("smooth", 402), ("smooth", 403), ("smooth", 404)]


def overflow_batches():
    """[(name, specs)]: the flagged frame first, in the middle and last among four unflagged ones"""
    p = OVERFLOW_PLAIN
    return [("first", [OVERFLOW_FLAGGED] + p), ("middle", p[:2] + [OVERFLOW_FLAGGED] + p[2:]), ("last", p + [OVERFLOW_FLAGGED])]


# ------------------------------------------------------------------------------------------------ the Python sequence
PY_MIXED = [("smooth", 3), ("lattice", 11), ("smooth", 4), ("lattice", 12)]
PY_BLANK = [("const", 0.0), ("const", 1.0), ("const", -7.0), ("const", 255.0)]
PY_FIRST_GUESS = int(1.5 * 4096) + 256           # BatchPlan's capacity per frame on a fresh plan
