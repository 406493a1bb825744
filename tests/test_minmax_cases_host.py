"""CPU-only proof that tests/minmax_cases.py says what tests/test_gpu_minmax_cases.py needs it to say:

* labels() is the kernels' own walk: a literal restatement of the three loops of minmax_kernel / minmax_typed_kernel visits
  every pixel exactly once and gives every pixel the label labels() computes in closed form;
* every configuration reaches the loops it was chosen for (the counts of the tables below were computed with labels());
* MUTANTS: for each way to drop a class of pixels -- the tail, the strided loop, one unrolled slot, one pixel of every chunk,
  one wave, one workgroup, the last chunk, pixel 0, pixel n-1 -- positions() holds a pixel of the dropped set, for every
  configuration: a kernel wrong in that way fails the GPU file;
* the constants restated in minmax_cases.py are the sources' (regexes on siftmi.hip and k_pyramid.hpp);
* every family's planted values lie strictly outside its band after the conversion to float32, and the oracle's min / max of
  the frames is the planted pair.
"""
import os
import re

import numpy as np
import pytest

import minmax_cases as mc
from test_gpu_typed_input import as_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sift_pyocl_amd", "csrc")
CONFIGS = mc.configurations()


def cid(c):
    return "%s-%dx%d-%dx%d" % (c[0], c[1][0], c[1][1], c[2], c[3])


@pytest.fixture(scope="module")
def cases():
    """configuration -> (geometry, labels, positions), computed on first use"""
    store = {}

    def get(c):
        if c not in store:
            dtype, shape, threads, blocks = c
            n = shape[0] * shape[1]
            lab = mc.labels(n, dtype, threads, blocks)
            store[c] = (mc.geometry(n, dtype, threads, blocks), lab, mc.positions(n, dtype, threads, blocks, lab=lab))
        return store[c]
    return get


def walk(n, dtype, threads, max_blocks):
    """The loops of minmax_kernel / minmax_typed_kernel as written (k_pyramid.hpp), every lane of the launch at once:
    (visits per pixel, labels as the walk assigns them)."""
    g = mc.geometry(n, dtype, threads, max_blocks)
    px, nchunks, stride = g["px"], g["nchunks"], g["stride"]
    visits = np.zeros(n, np.int32)
    lab = np.recarray(n, mc.LABELS)
    lab[:] = (-9, -9, -9, -9, -9, -9)
    i = np.arange(stride, dtype=np.int64)                             # blockIdx.x * blockDim.x + threadIdx.x

    def read(pixels, lanes, loop, slot, j):
        np.add.at(visits, pixels, 1)
        lab.loop[pixels], lab.slot[pixels], lab.px[pixels], lab.lane[pixels] = loop, slot, j, lanes
        lab.wave[pixels], lab.wg[pixels] = lanes % threads >> 6, lanes // threads          # threadIdx.x >> 6, blockIdx.x

    k = i.copy()
    while True:                                                       # for (; k + 3 * stride < nchunks; k += 4 * stride)
        on = k + 3 * stride < nchunks
        if not on.any():
            break
        for u in range(4):
            for j in range(px):
                read((k[on] + u * stride) * px + j, i[on], mc.UNROLLED, u, j)
        k[on] += 4 * stride
    while True:                                                       # for (; k < nchunks; k += stride)
        on = k < nchunks
        if not on.any():
            break
        for j in range(px):
            read(k[on] * px + j, i[on], mc.STRIDED, -1, j)
        k[on] += stride
    k2 = nchunks * px + i
    while True:                                                       # for (k2 = nchunks * PX + i; k2 < n; k2 += stride)
        on = k2 < n
        if not on.any():
            break
        read(k2[on], i[on], mc.TAIL, -1, -1)
        k2[on] += stride
    return visits, lab


@pytest.mark.parametrize("c", CONFIGS, ids=cid)
def test_labels_partition_every_pixel(cases, c):
    dtype, shape, threads, blocks = c
    g, lab, P = cases(c)
    visits, walked = walk(shape[0] * shape[1], dtype, threads, blocks)
    assert (visits == 1).all(), "pixels read %d..%d times" % (visits.min(), visits.max())
    for field in mc.LABELS.names:
        assert np.array_equal(lab[field], walked[field]), field
    assert g["tail"] < g["px"] <= g["stride"] and g["grid"] <= blocks
    assert len(P) <= mc.MAX_POSITIONS and len(set(P)) == len(P) and (np.diff(P) > 0).all() and 0 <= P[0] and P[-1] < len(lab)


# ------------------------------------------------------------------------------------------------ what each shape reaches
TAILS = {(22, 41): {4: 2, 8: 6, 16: 6}, (37, 53): {4: 1, 8: 1, 16: 9}, (97, 131): {4: 3, 8: 3, 16: 3},
         (199, 301): {4: 3, 8: 3, 16: 11}, mc.BIG: {4: 1, 8: 5, 16: 13}}
# chunks the unrolled loop takes: (97, 131) in one workgroup of 256; BIG at the defaults
UNROLLED_97 = {"uint8": 104, "rgb8": 104, "uint16": 1024, "uint32": 3072, "int32": 3072, "uint64": 3072, "int64": 3072, "float32": 3072}
UNROLLED_BIG = {"float32": 4892, "uint8": 1220, "uint16": 262144, "int64": 786432, "rgb8": 1220}


def unrolled_chunks(g, lab):
    return int((lab.loop[:g["nchunks"] * g["px"]:g["px"]] == mc.UNROLLED).sum())


def test_every_configuration_reaches_its_loops(cases):
    """If one of these fails after a default moved (test_constants_follow_the_sources says which), revisit SHAPES and the
    launch tables of minmax_cases.py: the shapes are chosen for the loops they reach at these launch shapes."""
    reached = {}
    for c in CONFIGS:
        dtype, shape, threads, blocks = c
        g, lab, P = cases(c)
        assert g["tail"] == TAILS[shape][g["px"]] > 0, c
        reached.setdefault(dtype, set()).update(zip(lab.loop[P].tolist(), lab.slot[P].tolist()))
        un = unrolled_chunks(g, lab)
        if shape == (22, 41):                                          # fewer chunks than lanes: idle lanes, and idle waves
            assert g["grid"] == 1 and g["nchunks"] < threads and un == 0, c
            if g["px"] == 16:
                assert g["nchunks"] <= mc.WAVE and set(lab.wave.tolist()) == {0}, c
        if shape == (37, 53) and g["px"] == 4 and dtype != "float32" and blocks == mc.MM_BLOCKS:
            assert g["grid"] == 2, c
        if shape == (97, 131) and (threads, blocks) == (256, 1):
            assert un == UNROLLED_97[dtype], (c, un)
        if shape == (97, 131) and (threads, blocks) in ((1024, 1), (512, 2)):
            assert un == 416, (c, un)
        if shape == (199, 301) and blocks in (1, 3):
            assert un > 0 and (lab.loop == mc.STRIDED).any(), c
            assert {(mc.UNROLLED, s) for s in range(4)} | {(mc.STRIDED, -1), (mc.TAIL, -1)} <= set(zip(lab.loop[P].tolist(), lab.slot[P].tolist())), c
        if shape == mc.BIG:
            assert g["grid"] == mc.MM_BLOCKS == 256 and un == UNROLLED_BIG[dtype], (c, un)
    every = {(mc.UNROLLED, s) for s in range(4)} | {(mc.STRIDED, -1), (mc.TAIL, -1)}
    for dtype in ("float32",) + mc.TYPED:
        assert reached[dtype] == every, (dtype, sorted(every - reached[dtype]))
    # the stage hook's launch shape differs from every plan's on the larger shapes (more than three workgroups)
    assert cases(("float32", (199, 301)) + mc.STAGE_LAUNCH)[0]["grid"] == 59


# ------------------------------------------------------------------------------------------------ mutants
def dropped_classes(g, lab, pix):
    """names of the ways to drop a class of pixels whose dropped set holds one of the pixels `pix`"""
    px, body = g["px"], g["nchunks"] * g["px"]
    sub = lab[pix]
    names = {"no tail"} if (sub.loop == mc.TAIL).any() else set()
    names |= {"no strided loop"} if (sub.loop == mc.STRIDED).any() else set()
    names |= {"unrolled slot %d" % s for s in np.unique(sub.slot[sub.loop == mc.UNROLLED])}
    names |= {"pixel %d of every chunk" % j for j in np.unique(sub.px[sub.loop != mc.TAIL])}
    names |= {"wave %d" % w for w in np.unique(sub.wave)}
    names |= {"workgroup %d" % b for b in np.unique(sub.wg)}
    names |= {"the last chunk"} if ((pix >= body - px) & (pix < body)).any() else set()
    names |= {"pixel 0"} if (pix == 0).any() else set()
    names |= {"pixel n-1"} if (pix == len(lab) - 1).any() else set()
    return names


@pytest.mark.parametrize("c", CONFIGS, ids=cid)
def test_positions_meet_every_mutant(cases, c):
    g, lab, P = cases(c)
    mutants = dropped_classes(g, lab, np.arange(len(lab)))             # every way that drops at least one pixel of this frame
    assert {"no tail", "the last chunk", "pixel 0", "pixel n-1", "pixel %d of every chunk" % (g["px"] - 1), "wave 0",
            "workgroup %d" % (g["grid"] - 1)} <= mutants
    missed = mutants - dropped_classes(g, lab, P)
    assert not missed, sorted(missed)
    # and every planted pixel serves once as the minimum and once as the maximum
    todo = mc.pairs(P)
    assert {p for _, p, _ in todo} == {p for _, _, p in todo} and len(todo) >= len(P) - 1
    assert {p for _, p, _ in todo} >= set(P.tolist()) - {int(P[len(P) // 2])}


# ------------------------------------------------------------------------------------------------ constants
def test_constants_follow_the_sources():
    """The numbers minmax_cases.py restates, where the sources set them.  A failure names the table to revisit."""
    hip = open(os.path.join(CSRC, "siftmi.hip")).read()
    hpp = open(os.path.join(CSRC, "k_pyramid.hpp")).read()
    m = re.search(r"int mm_blocks = (\d+);", hip)
    assert m and int(m.group(1)) == mc.MM_BLOCKS, "default mm_blocks moved: revisit MM_BLOCKS, UNROLLED_BIG and the launch tables"
    m = re.search(r"int mm_threads = (\d+);", hip)
    assert m and int(m.group(1)) == mc.MM_THREADS, "default mm_threads moved: revisit MM_THREADS, F32_LAUNCHES and UNROLLED_BIG"
    m = re.search(r"fused_in \? (\d+) : p->opt\.mm_threads, p->opt\.mm_blocks", hip)
    assert m and int(m.group(1)) == mc.TYPED_THREADS, "the plan's typed launch moved: revisit TYPED_THREADS and TYPED_LAUNCHES"
    m = re.search(r"launch_minmax\(nullptr, 0, SIFTMI_F32, a\.p, \(int64_t\)N, (\d+), (\d+),", hip)
    assert m and (int(m.group(1)), int(m.group(2))) == mc.STAGE_LAUNCH, "siftmi_stage_minmax_normalize's launch moved: revisit STAGE_LAUNCH"
    assert "grid_for(n / 4, threads, max_blocks)" in hip and "grid_for(n / TypedChunk<DT>::PX, threads, max_blocks)" in hip, \
        "launch_minmax sizes its grid differently: revisit geometry()"
    m = re.search(r"int64_t g = \(n \+ block - 1\) / block;\s*if \(g < 1\) g = 1;\s*if \(g > max_blocks\) g = max_blocks;", hip)
    assert m, "grid_for changed: revisit minmax_cases.grid_for"
    m = re.search(r"static constexpr int PX = \(DT == 1 \|\| DT == 8\) \? (\d+) : \(DT == 2 \? (\d+) : (\d+)\);", hpp)
    assert m, "the TypedChunk rule changed: revisit PX"
    wide, mid, narrow = (int(v) for v in m.groups())
    for dtype in mc.TYPED:
        code = mc.DT_CODE[dtype]
        assert mc.PX[dtype] == (wide if code in (1, 8) else (mid if code == 2 else narrow)), "revisit PX[%r]" % dtype
    assert mc.PX["float32"] == 4 and "const int64_t n4 = n >> 2;" in hpp, "minmax_kernel no longer reads float4 chunks: revisit PX"
    from sift_pyocl_amd import _lib
    assert {k: v for k, v in _lib.DTYPE_CODES.items() if k in mc.DT_CODE} == mc.DT_CODE


# ------------------------------------------------------------------------------------------------ frames
def one(pixel):
    """float32 of one planted pixel, as as_f32 converts it"""
    return as_f32(pixel.reshape((1, 1) + pixel.shape[1:])).reshape(-1)[0]


@pytest.mark.parametrize("dtype", ("float32",) + mc.TYPED)
def test_planted_values_lie_outside_the_band(oracle, dtype):
    shape = (37, 53)
    n = shape[0] * shape[1]
    P = mc.positions(n, dtype, *mc.launches(dtype)[-1])
    for family in mc.families(dtype):
        flat = mc.band(dtype, family, n)
        frame = flat.reshape(shape + flat.shape[1:])
        conv = as_f32(frame)
        lo, hi = mc.planted(dtype, family)
        flo, fhi = one(lo), one(hi)
        assert flo < conv.min() <= conv.max() < fhi, (dtype, family, flo, conv.min(), conv.max(), fhi)
        assert oracle.minmax(conv) == (conv.min(), conv.max())
        if dtype == "float32":
            assert not (flat == 0).any() and np.isfinite(flat).all() and flo != 0 and fhi != 0, family
            if family == "tiny":
                tiny = np.finfo(np.float32).tiny
                assert (np.abs(flat) < tiny).all() and 0 < flo < fhi < tiny and lo.view(np.uint32)[0] == 1
            if family in ("neg", "mixed"):
                assert (flat < 0).any() and flo < 0
        else:
            info = np.iinfo(flat.dtype)
            assert (lo == info.min).all() and (hi == info.max).all()
        before = flat.copy()
        todo = mc.pairs(P, step=3)
        for k, pmin, pmax in mc.frames(flat, todo, lo, hi):
            got = oracle.minmax(as_f32(frame))
            assert got[0].tobytes() == flo.tobytes() and got[1].tobytes() == fhi.tobytes(), (dtype, family, k, got)
            assert (flat != before).reshape(n, -1).any(axis=1).nonzero()[0].tolist() == sorted((pmin, pmax))
        assert np.array_equal(flat, before) and len(todo) > 10                    # restored


def test_lone_frames(oracle):
    n = 37 * 53
    P = mc.positions(n, "float32", mc.MM_THREADS, mc.MM_BLOCKS)
    flat = np.full(n, np.nan, np.float32)
    seen = set()
    for k, p, v in mc.lone_frames(flat, P, step=5):
        assert np.isfinite(flat).sum() == 1 and flat[p] == v and v != 0 and oracle.minmax(flat) == (v, v)
        seen.add(bool(v < 0))
    assert np.isnan(flat).all() and seen == {False, True}
