"""Frames with the minimum and the maximum PLANTED on chosen pixels, for the one reduction at the head of every frame
(k_pyramid.hpp: minmax_kernel for f32, minmax_typed_kernel<DT> for u8 / u16 / u32 / u64 / i32 / i64 / RGB8; one launch site,
siftmi.hip launch_minmax).

On noise the extremes sit on one pixel somewhere, and on saturated integer noise on thousands: a kernel that skips the scalar
tail, one of its four unrolled loads, a byte lane of a chunk or one wave's partial is then wrong with negligible probability.
Here a seeded "band" frame carries realistic data and exactly two pixels lie outside the band, so the answer is wrong as
soon as either pixel is not read, and the pixels are the ones at the edges of every loop of the kernels:

    labels()     restates, per pixel, who reads it: loop (unrolled / strided / scalar tail), slot 0..3 of the unrolled step,
                 pixel index inside its chunk, global lane, wave and workgroup
    positions()  the pixels to plant on for one launch shape (at most MAX_POSITIONS)
    band(), planted(), frames()  the frames: frame k has its minimum on P[k] and its maximum on P[len(P) - 1 - k]

numpy only, deterministic from seeds, nothing here imports the package or the oracle.  tests/test_minmax_cases_host.py proves
on the CPU that labels() is the kernels' own walk, that positions() meets every way of dropping a class of pixels, and that
the constants restated here are the sources'; tests/test_gpu_minmax_cases.py runs the frames.
"""
import numpy as np

# ---------------------------------------------------------------------------------------------- restated constants
MM_BLOCKS = 256             # siftmi.hip: PlanOptions mm_blocks (workgroups at most)
MM_THREADS = 1024           # siftmi.hip: PlanOptions mm_threads (f32 frames; 256 / 512 / 1024)
TYPED_THREADS = 256         # siftmi.hip enqueue: a typed frame is always reduced by workgroups of 256
STAGE_LAUNCH = (256, 2048)  # siftmi_stage_minmax_normalize: threads, workgroups at most
WAVE = 64

# pixels per chunk (k_pyramid.hpp TypedChunk<DT>::PX; f32: one float4) and the library's dtype codes
PX = {"float32": 4, "uint8": 16, "uint16": 8, "uint32": 4, "uint64": 4, "int32": 4, "int64": 4, "rgb8": 16}
DT_CODE = {"float32": 0, "uint8": 1, "uint16": 2, "uint32": 3, "uint64": 4, "int32": 5, "int64": 6, "rgb8": 8}
TYPED = ("uint8", "uint16", "uint32", "int32", "uint64", "int64", "rgb8")

UNROLLED, STRIDED, TAIL = 0, 1, 2
LOOP_NAMES = ("unrolled", "strided", "tail")

# ---------------------------------------------------------------------------------------------- what the GPU file runs
SHAPES = [(22, 41), (37, 53), (97, 131), (199, 301)]
BIG = (1773, 1777)                                                    # the defaults themselves: 256 workgroups, unrolled loop
BIG_DTYPES = ("float32", "uint8", "uint16", "int64", "rgb8")
F32_LAUNCHES = [(256, 1), (256, 3), (512, 2), (1024, 1), (MM_THREADS, MM_BLOCKS)]
TYPED_LAUNCHES = [(TYPED_THREADS, 1), (TYPED_THREADS, 3), (TYPED_THREADS, MM_BLOCKS)]
MAX_POSITIONS = 600
SEED = 20240229


def launches(dtype):
    return F32_LAUNCHES if dtype == "float32" else TYPED_LAUNCHES


def configurations():
    """every (dtype, shape, threads, max_blocks) the GPU file runs: the plans' launch shapes on the small shapes, the stage
    hook's on the same, the defaults on BIG"""
    out = []
    for dtype in ("float32",) + TYPED:
        for shape in SHAPES:
            out += [(dtype, shape, t, b) for t, b in launches(dtype)]
    out += [("float32", shape) + STAGE_LAUNCH for shape in SHAPES]
    out += [(dtype, BIG) + launches(dtype)[-1] for dtype in BIG_DTYPES]
    return out


# ---------------------------------------------------------------------------------------------- who reads which pixel
def grid_for(n, block, max_blocks):
    """siftmi.hip grid_for"""
    return int(min(max((n + block - 1) // block, 1), max_blocks))


def geometry(n, dtype, threads, max_blocks):
    """dict(px, nchunks, grid, stride, tail) of the launch: chunks of px pixels, `grid` workgroups, stride = grid x threads
    lanes, `tail` pixels behind the last whole chunk"""
    px = PX[dtype]
    nchunks = n // px
    grid = grid_for(nchunks, threads, max_blocks)
    return dict(px=px, nchunks=nchunks, grid=grid, stride=grid * threads, tail=n - nchunks * px)


LABELS = np.dtype([("loop", np.int8), ("slot", np.int8), ("px", np.int8), ("lane", np.int32), ("wave", np.int8), ("wg", np.int32)])


def labels(n, dtype, threads, max_blocks):
    """recarray of n records (loop, slot, px, lane, wave, wg), in closed form.  Lane i takes chunks i, i + stride, ...: four
    per step while the fourth lies inside the frame (the unrolled loop, slot = chunk row % 4), then one per step (the strided
    loop); pixel nchunks * px + t of the scalar tail is read by lane t.  slot is -1 outside the unrolled loop, px -1 in the
    tail; wave = lane % threads // 64, wg = lane // threads."""
    g = geometry(n, dtype, threads, max_blocks)
    px, nchunks, stride = g["px"], g["nchunks"], g["stride"]
    pix = np.arange(n, dtype=np.int64)
    chunk = pix // px
    body = chunk < nchunks
    lane = np.where(body, chunk % stride, (pix - nchunks * px) % stride)
    row = chunk // stride
    steps = np.maximum(0, -(-(nchunks - 3 * stride - lane) // (4 * stride)))      # unrolled steps of the pixel's lane
    unrolled = body & (row < 4 * steps)
    out = np.recarray(n, LABELS)
    out.loop = np.where(body, np.where(unrolled, UNROLLED, STRIDED), TAIL)
    out.slot = np.where(unrolled, row % 4, -1)
    out.px = np.where(body, pix % px, -1)
    out.lane = lane
    out.wave = lane % threads // WAVE
    out.wg = lane // threads
    return out


def describe(lab):
    """one record of labels() in words, for assertion messages"""
    return "%s loop, slot %d, pixel %d of its chunk, lane %d = wave %d of workgroup %d" % (
        LOOP_NAMES[lab.loop], lab.slot, lab.px, lab.lane, lab.wave, lab.wg)


def positions(n, dtype, threads, max_blocks, seed=SEED, n_random=32, lab=None):
    """Sorted pixel indices to plant on:
    pixels 0, 1, n-2, n-1 and every pixel of the scalar tail; the first and the last pixel of each loop's region; every pixel
    of a first, a middle and a last chunk of the strided loop and of each unrolled slot; both sides of every 64-lane edge of
    the first and of the last workgroup; both sides of the first two and the last two stride edges; one seeded random pixel
    owned by each workgroup; n_random seeded random pixels."""
    g = geometry(n, dtype, threads, max_blocks)
    px, nchunks, stride, grid = g["px"], g["nchunks"], g["stride"], g["grid"]
    L = labels(n, dtype, threads, max_blocks) if lab is None else lab
    body = nchunks * px
    P = set()

    def add(pixels, below=n):
        P.update(int(p) for p in pixels if 0 <= p < below)

    add([0, 1, n - 2, n - 1])
    add(range(body, n))
    for loop in (UNROLLED, STRIDED, TAIL):
        idx = np.flatnonzero(L.loop == loop)
        if idx.size:
            add([idx[0], idx[-1]])
    chunk_loop, chunk_slot = L.loop[:body:px], L.slot[:body:px]
    for loop, slot in [(STRIDED, -1)] + [(UNROLLED, s) for s in range(4)]:
        ids = np.flatnonzero((chunk_loop == loop) & (chunk_slot == slot))
        if ids.size:
            for c in (ids[0], ids[ids.size // 2], ids[-1]):
                add(range(c * px, (c + 1) * px))
    for wg in {0, grid - 1}:                                           # the chunks the lanes beside an edge take first
        for w in range(threads // WAVE + 1):
            edge = (wg * threads + w * WAVE) * px
            add([edge - 1, edge], below=body)
    rows = (nchunks - 1) // stride if nchunks else 0
    for m in {1, 2, rows - 1, rows}:
        if 1 <= m <= rows:
            add([m * stride * px - 1, m * stride * px])
    rng = np.random.default_rng(seed)
    order = np.argsort(L.wg, kind="stable")
    counts = np.bincount(L.wg, minlength=grid)
    starts = np.cumsum(counts) - counts
    for wg in range(grid):
        if counts[wg]:
            add([order[starts[wg] + rng.integers(counts[wg])]])
    add(rng.integers(0, n, n_random))
    return np.array(sorted(P), np.int64)


def pairs(P, step=1):
    """[(k, pixel of the minimum, pixel of the maximum)]: frame k has its minimum on P[k] and its maximum on P[len(P)-1-k], so
    every position serves once as each; k is skipped where the two coincide.  step > 1 thins the list."""
    m = len(P)
    return [(k, int(P[k]), int(P[m - 1 - k])) for k in range(0, m, step) if P[k] != P[m - 1 - k]]


# ---------------------------------------------------------------------------------------------- frames
F32_FAMILIES = ("pos", "neg", "mixed", "inf", "tiny")
_SUB = lambda bits: np.array(bits, np.uint32).view(np.float32)       # a subnormal by its bit pattern (x 2^-149)


def families(dtype):
    """the families of a frame type: five for f32 (`lone` is separate: lone_frames), the type's own for a typed frame"""
    return F32_FAMILIES if dtype == "float32" else (dtype,)


def np_dtype(dtype):
    return np.dtype(np.uint8 if dtype == "rgb8" else dtype)


def band(dtype, family, n, seed=SEED):
    """n pixels ((n, 3) for RGB8) of seeded noise inside the family's band; no +-0 in an f32 band"""
    rng = np.random.default_rng([seed, n, DT_CODE[dtype], len(family)])
    if dtype == "float32":
        if family in ("pos", "inf"):
            return rng.uniform(100, 200, n).astype(np.float32)
        if family == "neg":
            return rng.uniform(-200, -100, n).astype(np.float32)
        if family == "mixed":
            f = rng.uniform(-100, 100, n).astype(np.float32)
            f[f == 0] = 1.0
            return f
        if family == "tiny":                                          # subnormals 1000 .. 100 000 x 2^-149
            return rng.integers(1000, 100001, n).astype(np.uint32).view(np.float32)
        raise KeyError(family)
    lo, hi = {"uint8": (64, 191), "uint16": (1000, 60000), "uint32": (1 << 20, 1 << 31), "int32": (-(1 << 30), 1 << 30),
              "uint64": (1 << 40, 1 << 62), "int64": (-(1 << 61), 1 << 61), "rgb8": (40, 215)}[dtype]
    size = (n, 3) if dtype == "rgb8" else n
    return rng.integers(lo, hi, size, dtype=np_dtype(dtype), endpoint=True)


def planted(dtype, family):
    """(min, max) to plant, each an array of one pixel in the frame's type: the type's own extremes for a typed frame"""
    if dtype == "float32":
        lo, hi = {"pos": (50.0, 250.0), "neg": (-250.0, -50.0), "mixed": (-250.0, 250.0), "inf": (-np.inf, np.inf),
                  "tiny": (_SUB(1), np.float32(2e-40))}[family]      # 1e-45 is the smallest subnormal
        return np.array([lo], np.float32).reshape(1), np.array([hi], np.float32).reshape(1)
    if dtype == "rgb8":
        return np.zeros((1, 3), np.uint8), np.full((1, 3), 255, np.uint8)
    info = np.iinfo(np_dtype(dtype))
    return np.array([info.min], info.dtype), np.array([info.max], info.dtype)


def frames(flat, todo, lo, hi, also=None):
    """Plants lo on the minimum's pixel and hi on the maximum's of `flat` (band(): modified in place, restored after every
    frame) for every (k, pmin, pmax) of `todo` and yields it.  also = (array, lo, hi): a second array planted alongside (the
    frame as float32)."""
    for k, pmin, pmax in todo:
        arrays = [(flat, lo, hi)] + ([also] if also is not None else [])
        saved = [(a[pmin].copy(), a[pmax].copy()) for a, _, _ in arrays]
        for a, l, h in arrays:
            a[pmin] = l[0]
            a[pmax] = h[0]
        yield k, pmin, pmax
        for (a, _, _), (smin, smax) in zip(arrays, saved):
            a[pmin] = smin
            a[pmax] = smax


def lone_value(k):
    """the one finite value of `lone` frame k: both signs, never zero"""
    return np.float32((3.5 + k) * (-1.0 if k % 2 else 1.0))


def lone_frames(flat, P, step=1):
    """`flat` (n float32, all NaN) with one finite pixel: lone_value(k) on P[k]; yields (k, pixel, value), restores NaN"""
    for k in range(0, len(P), step):
        flat[P[k]] = lone_value(k)
        yield k, int(P[k]), lone_value(k)
        flat[P[k]] = np.nan
