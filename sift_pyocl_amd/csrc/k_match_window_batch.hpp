// k_match_window_batch.hpp -- the windowed matcher of k_match_window.hpp over S segment pairs in one set of launches (DESIGN.md
// section 7 row 16; restated in numpy by tests/match_window_batch_ref.py).  The records of S lists lie back to back on either
// side, or ONE list on the first side that every segment is matched against; segment s gets the rule of k_match_window.hpp on its
// own two lists with its own shift, indices local to the segment, and the pairs come out in (segment, ascending i) order as
// k_match_batch.hpp's do: the scan writes `best` or -1 per query into that header's dense slot layout, and its mb_scan_kernel and
// mb_scatter_kernel do the ordered compaction unchanged.  Atomics are confined to the extents, the histograms and the counting-sort
// cursors; the 64-bit (distance << 32 | original index) keys make a query's result independent of the order inside a cell.
//
// The counts are host values, so the host builds the tables and every kernel is driven by them; an entry is indexed by
// blockIdx.x (or by a value read through it), the same in every lane of a workgroup, so reading it costs scalar loads:
//   MwbSeg   one row per segment and direction (plus one for a shared list): where its queries and its list lie, where its cells,
//            its order entries, its part of the dense copy and its result slots begin, the cap on its grid, its shift
//   int2     (row, chunk of 256 records): the grids of the extent, count and scatter kernels, one table per side
// Per-segment grid: a list has its own extent words and its own grid (mw_axis's, coarsened to at most g_cap cells an axis, which
// the host derives from the list's length: cells <= max(1, records)), so the cell scratch is O(records + S) words.  mw_cell and
// mw_range are proved for any (x0, side > 0, g >= 1): the result does not depend on the grid.
//
// Launches of one direction: extent, count (lists), count (queries), scan (a workgroup per row), mb_scan_kernel over the rows'
// work counts, work list, scatter (lists), scatter (queries), match.  The work list is compacted: item k of row s lies at
// w_off[s] + k, the match grid is the host's bound on the items and a workgroup past w_off[S] exits on one scalar compare.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_match_window.hpp"
#include "k_match_batch.hpp"

namespace siftk {

#define SIFT_MWB_SCAN_THREADS 1024

// one row: a segment in one direction (or a shared list).  Records are counted from the start of their buffer.
struct MwbSeg {
    int q_first, q_count;       // the queries; q_count == 0: the row has none (an empty side: no work, no cell is touched)
    int l_first, l_count;       // the list
    int q_cells, l_cells;       // first word of the row's cells in the query-side and in the list-side arrays (cells + 1 words)
    int ext;                    // the row whose extent words give the grid (its own, or the shared list's)
    int g_cap;                  // cells per axis at most, 1 .. 256
    int order;                  // first entry of the queries' order
    int dense;                  // first record of the list's dense copy
    int out;                    // forward: the dense slot of the segment's query 0
    int own_list;               // the row bins its list itself (0: a shared list's row does)
    float sx, sy;               // the segment's shift as the predicate uses it
    int pad0, pad1;
};

// mw_axis's grid with at most `cap` cells: k = ceil(g / cap) cells become one.  Any (x0, side > 0, g >= 1) is a valid grid.
__device__ __forceinline__ void mwb_axis(uint32_t umin, uint32_t umax, float w, int cap, float &x0, float &side, int &g) {
    mw_axis(umin, umax, w, x0, side, g);
    if (g > cap) {
        const int k = (g + cap - 1) / cap;
        side *= (float)k;
        g = (side < INFINITY) ? (g + k - 1) / k : 1;
    }
}
__device__ __forceinline__ MwGrid mwb_grid(const uint32_t *__restrict__ ext_min, const uint32_t *__restrict__ ext_max, int row, int cap,
                                           float wx, float wy) {
    MwGrid g;
    mwb_axis(ext_min[2 * row], ext_max[2 * row], wx, cap, g.x0, g.side_x, g.gx);
    mwb_axis(ext_min[2 * row + 1], ext_max[2 * row + 1], wy, cap, g.y0, g.side_y, g.gy);
    return g;
}

// exclusive scan of K values per thread over the SIFT_MWB_SCAN_THREADS threads of a workgroup, and the totals
template <int K>
__device__ __forceinline__ void mwb_block_scan(const int (&v)[K], int (&excl)[K], int (&total)[K], int (*wave_tot)[SIFT_MWB_SCAN_THREADS / 64]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int incl[K];
#pragma unroll
    for (int k = 0; k < K; k++) {
        incl[k] = v[k];
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl[k], d, 64);
            if (lane >= d) incl[k] += up;
        }
        if (lane == 63) wave_tot[k][wave] = incl[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        int before = 0, all = 0;
        for (int w = 0; w < SIFT_MWB_SCAN_THREADS / 64; w++) { const int t = wave_tot[k][w]; all += t; if (w < wave) before += t; }
        excl[k] = before + incl[k] - v[k];
        total[k] = all;
    }
}

// extent of the finite coordinates of every list: mw_extent_kernel's, into the row's own words
__global__ __launch_bounds__(256) void mwb_extent_kernel(const uint8_t *__restrict__ kp, const MwbSeg *__restrict__ segs,
                                                         const int2 *__restrict__ blocks, uint32_t *__restrict__ ext_min,
                                                         uint32_t *__restrict__ ext_max) {
    __shared__ uint32_t s[4];
    const int tid = threadIdx.x;
    const int2 b = blocks[blockIdx.x];
    const MwbSeg sg = segs[b.x];
    if (tid < 4) s[tid] = tid < 2 ? 0xffffffffu : 0u;
    __syncthreads();
    const int j = b.y * 256 + tid;
    if (j < sg.l_count) {
        const float *k = reinterpret_cast<const float *>(kp + (size_t)(sg.l_first + j) * 144);
        const float x = k[0], y = k[1];
        if (fabsf(x) < INFINITY) { atomicMin(&s[0], mw_enc(x)); atomicMax(&s[2], mw_enc(x)); }
        if (fabsf(y) < INFINITY) { atomicMin(&s[1], mw_enc(y)); atomicMax(&s[3], mw_enc(y)); }
    }
    __syncthreads();
    if (tid < 2) atomicMin(&ext_min[2 * sg.ext + tid], s[tid]);
    else if (tid < 4) atomicMax(&ext_max[2 * sg.ext + tid - 2], s[tid]);
}

// histogram over the row's cells: as_list: the list with a zero shift; otherwise the queries by their window centre
__global__ __launch_bounds__(256) void mwb_count_kernel(const uint8_t *__restrict__ kp, const MwbSeg *__restrict__ segs,
                                                        const int2 *__restrict__ blocks, int as_list, int reverse,
                                                        const uint32_t *__restrict__ ext_min, const uint32_t *__restrict__ ext_max,
                                                        float wx, float wy, int *__restrict__ cnt) {
    const int2 b = blocks[blockIdx.x];
    const MwbSeg sg = segs[b.x];
    const int n = as_list ? sg.l_count : sg.q_count, first = as_list ? sg.l_first : sg.q_first;
    const int i = b.y * 256 + threadIdx.x;
    if (i >= n) return;
    const MwGrid g = mwb_grid(ext_min, ext_max, sg.ext, sg.g_cap, wx, wy);
    const float shx = as_list ? 0.f : reverse ? -sg.sx : sg.sx, shy = as_list ? 0.f : reverse ? -sg.sy : sg.sy;
    const float *k = reinterpret_cast<const float *>(kp + (size_t)(first + i) * 144);
    atomicAdd(&cnt[(as_list ? sg.l_cells : sg.q_cells) + mw_cell_of(g, k[0], k[1], shx, shy)], 1);
}

// one workgroup per row: mw_scan_kernel's exclusive scans over the row's cells (start[c], start[cells] = n), the counters turned
// into scatter cursors, and the number of the row's work items (one per SIFT_MW_QB queries of a cell)
__global__ __launch_bounds__(SIFT_MWB_SCAN_THREADS) void mwb_scan_kernel(const MwbSeg *__restrict__ segs, const uint32_t *__restrict__ ext_min,
                                                                         const uint32_t *__restrict__ ext_max, float wx, float wy,
                                                                         int *__restrict__ cnt_l, int *__restrict__ cnt_q,
                                                                         int *__restrict__ start_l, int *__restrict__ start_q,
                                                                         int *__restrict__ n_work) {
    __shared__ int wave_tot[3][SIFT_MWB_SCAN_THREADS / 64];
    const int tid = threadIdx.x;
    const MwbSeg sg = segs[blockIdx.x];
    const bool do_l = sg.own_list != 0, do_q = sg.q_count > 0;
    if (!do_l && !do_q) { if (tid == 0) n_work[blockIdx.x] = 0; return; }       // the same in every lane
    const MwGrid g = mwb_grid(ext_min, ext_max, sg.ext, sg.g_cap, wx, wy);
    const int cells = g.gx * g.gy;
    const int per = (cells + SIFT_MWB_SCAN_THREADS - 1) / SIFT_MWB_SCAN_THREADS;
    const int c0 = min(tid * per, cells), c1 = min(c0 + per, cells);
    int *cl = cnt_l + sg.l_cells, *cq = cnt_q + sg.q_cells, *sl = start_l + sg.l_cells, *sq = start_q + sg.q_cells;
    int v[3] = {0, 0, 0}, e[3], tot[3];
    for (int c = c0; c < c1; c++) {
        if (do_l) v[0] += cl[c];
        if (do_q) { const int q = cq[c]; v[1] += q; v[2] += (q + SIFT_MW_QB - 1) / SIFT_MW_QB; }
    }
    mwb_block_scan<3>(v, e, tot, wave_tot);
    int a = e[0], b = e[1];
    for (int c = c0; c < c1; c++) {
        if (do_l) { const int nl = cl[c]; sl[c] = a; cl[c] = a; a += nl; }
        if (do_q) { const int nq = cq[c]; sq[c] = b; cq[c] = b; b += nq; }
    }
    if (tid == 0) {
        if (do_l) sl[cells] = tot[0];
        if (do_q) sq[cells] = tot[1];
        n_work[blockIdx.x] = tot[2];
    }
}

// one workgroup per segment: its work items (row << 16 | cell, chunk) behind those of the segments before it
__global__ __launch_bounds__(SIFT_MWB_SCAN_THREADS) void mwb_work_kernel(const MwbSeg *__restrict__ segs, const uint32_t *__restrict__ ext_min,
                                                                         const uint32_t *__restrict__ ext_max, float wx, float wy,
                                                                         const int *__restrict__ start_q, const int *__restrict__ w_off,
                                                                         int2 *__restrict__ work, int work_cap) {
    __shared__ int wave_tot[1][SIFT_MWB_SCAN_THREADS / 64];
    const int tid = threadIdx.x;
    const MwbSeg sg = segs[blockIdx.x];
    if (sg.q_count <= 0) return;                                                 // the same in every lane
    const MwGrid g = mwb_grid(ext_min, ext_max, sg.ext, sg.g_cap, wx, wy);
    const int cells = g.gx * g.gy;
    const int per = (cells + SIFT_MWB_SCAN_THREADS - 1) / SIFT_MWB_SCAN_THREADS;
    const int c0 = min(tid * per, cells), c1 = min(c0 + per, cells);
    const int *sq = start_q + sg.q_cells;
    int v[1] = {0}, e[1], tot[1];
    for (int c = c0; c < c1; c++) v[0] += (sq[c + 1] - sq[c] + SIFT_MW_QB - 1) / SIFT_MW_QB;
    mwb_block_scan<1>(v, e, tot, wave_tot);
    int w = w_off[blockIdx.x] + e[0];
    for (int c = c0; c < c1; c++) {
        const int chunks = (sq[c + 1] - sq[c] + SIFT_MW_QB - 1) / SIFT_MW_QB;
        for (int k = 0; k < chunks; k++, w++)
            if (w >= 0 && w < work_cap) work[w] = make_int2((int)(((uint32_t)blockIdx.x << 16) | (uint32_t)c), k);
    }
}

// counting-sort scatter of every list into its part of the dense copy (mw_scatter_list_kernel's: eight threads per element);
// the stored index is local to the list
__global__ __launch_bounds__(256) void mwb_scatter_list_kernel(const uint8_t *__restrict__ kp, const MwbSeg *__restrict__ segs,
                                                               const int2 *__restrict__ blocks, const uint32_t *__restrict__ ext_min,
                                                               const uint32_t *__restrict__ ext_max, float wx, float wy,
                                                               int *__restrict__ cursor, uint4 *__restrict__ desc, float4 *__restrict__ meta) {
    const int2 b = blocks[blockIdx.x];
    const MwbSeg sg = segs[b.x];
    const MwGrid g = mwb_grid(ext_min, ext_max, sg.ext, sg.g_cap, wx, wy);
    const int piece = threadIdx.x & 7;
    for (int it = 0; it < 8; it++) {
        const int j = b.y * 256 + it * 32 + (threadIdx.x >> 3);
        const bool live = j < sg.l_count;
        float x = 0.f, y = 0.f;
        int pos = 0;
        if (live && piece == 0) {
            const float *k = reinterpret_cast<const float *>(kp + (size_t)(sg.l_first + j) * 144);
            x = k[0]; y = k[1];
            pos = atomicAdd(&cursor[sg.l_cells + mw_cell_of(g, x, y, 0.f, 0.f)], 1);
        }
        pos = __shfl(pos, (int)(threadIdx.x & 63 & ~7));
        if (!live || pos < 0 || pos >= sg.l_count) continue;
        desc[((size_t)sg.dense + pos) * 8 + piece] = reinterpret_cast<const uint4 *>(kp + (size_t)(sg.l_first + j) * 144 + 16)[piece];
        if (piece == 0) meta[(size_t)sg.dense + pos] = make_float4(x, y, __int_as_float(j), 0.f);
    }
}

// the queries of every row in cell order (indices local to the row's queries)
__global__ __launch_bounds__(256) void mwb_scatter_query_kernel(const uint8_t *__restrict__ kp, const MwbSeg *__restrict__ segs,
                                                                const int2 *__restrict__ blocks, int reverse,
                                                                const uint32_t *__restrict__ ext_min, const uint32_t *__restrict__ ext_max,
                                                                float wx, float wy, int *__restrict__ cursor, int *__restrict__ order) {
    const int2 b = blocks[blockIdx.x];
    const MwbSeg sg = segs[b.x];
    const int i = b.y * 256 + threadIdx.x;
    if (i >= sg.q_count) return;
    const MwGrid g = mwb_grid(ext_min, ext_max, sg.ext, sg.g_cap, wx, wy);
    const float *k = reinterpret_cast<const float *>(kp + (size_t)(sg.q_first + i) * 144);
    const int pos = atomicAdd(&cursor[sg.q_cells + mw_cell_of(g, k[0], k[1], reverse ? -sg.sx : sg.sx, reverse ? -sg.sy : sg.sy)], 1);
    if (pos >= 0 && pos < sg.q_count) order[(size_t)sg.order + pos] = i;
}

// mw_match_kernel's body on one work item of one segment: up to SIFT_MW_QB queries of one cell against the rectangle of the
// segment's cells that holds their candidates.  Every index is clamped to the row's own queries (order, records) and to the row's
// own part of the dense copy (positions, the tile prefetch's min(p, nl - 1)): no record of another segment is read.
// nearest == null: writes `best` or -1 (the ratio test) into dense[out + i]; otherwise the index of the minimum (-1: no
// candidate) into nearest[q_first + i].  Every query of a row with work lies in exactly one item: every such slot is written.
// The grid is the host's bound on the items; a workgroup past the device-side total exits on one scalar load and compare.  (A
// grid capped at a few thousand workgroups that stride over the items was tried: the loop costs 116 VGPRs and a wave of occupancy,
// or 13 spilled registers when held to five waves, so the empty workgroups stay; DESIGN.md row 16 counts them.)
__global__ __launch_bounds__(256) void mwb_match_kernel(const uint8_t *__restrict__ kq, const MwbSeg *__restrict__ segs,
                                                        const uint32_t *__restrict__ ext_min, const uint32_t *__restrict__ ext_max,
                                                        float wx, float wy, int reverse, const int *__restrict__ start_l_all,
                                                        const int *__restrict__ start_q_all, const int *__restrict__ order_all,
                                                        const int2 *__restrict__ work, const int *__restrict__ n_items,
                                                        const uint4 *__restrict__ desc_all, const float4 *__restrict__ meta_all,
                                                        float ratio_th, int *__restrict__ dense, int *__restrict__ nearest) {
    __shared__ uint4 tile[2][SIFT_MW_TILE * 8];
    __shared__ float4 tmeta[2][SIFT_MW_TILE];
    __shared__ int box[4];
    if ((int)blockIdx.x >= *n_items) return;
    const int tid = threadIdx.x;
    const int2 wk = work[blockIdx.x];
    const MwbSeg sg = segs[(uint32_t)wk.x >> 16];
    const int cell = wk.x & 0xffff;
    const MwGrid g = mwb_grid(ext_min, ext_max, sg.ext, sg.g_cap, wx, wy);
    const int nq = sg.q_count, nl = sg.l_count;
    const float sx = sg.sx, sy = sg.sy;
    const int *start_l = start_l_all + sg.l_cells, *start_q = start_q_all + sg.q_cells;
    const uint4 *desc = desc_all + (size_t)sg.dense * 8;
    const float4 *meta = meta_all + sg.dense;
    const int q_begin = max(start_q[cell], 0) + wk.y * SIFT_MW_QB, q_end = min(min(start_q[cell + 1], q_begin + SIFT_MW_QB), nq);
    const bool active = q_begin + tid < q_end;
    const int i = active ? min(max(order_all[(size_t)sg.order + q_begin + tid], 0), nq - 1) : 0;
    const uint8_t *rec = kq + (size_t)(sg.q_first + i) * 144;
    const float xq = reinterpret_cast<const float *>(rec)[0], yq = reinterpret_cast<const float *>(rec)[1];
    uint32_t q[32];
    {
        const uint4 *p = reinterpret_cast<const uint4 *>(rec + 16);
#pragma unroll
        for (int w = 0; w < 8; w++) {
            const uint4 v = p[w];
            q[4 * w] = v.x; q[4 * w + 1] = v.y; q[4 * w + 2] = v.z; q[4 * w + 3] = v.w;
        }
    }
    if (tid < 4) box[tid] = tid < 2 ? 0x7fffffff : -1;
    __syncthreads();
    if (active) {
        int xlo, xhi, ylo, yhi;
        mw_range(xq, reverse ? -sx : sx, wx, g.x0, g.side_x, g.gx, xlo, xhi);
        mw_range(yq, reverse ? -sy : sy, wy, g.y0, g.side_y, g.gy, ylo, yhi);
        atomicMin(&box[0], xlo); atomicMin(&box[1], ylo); atomicMax(&box[2], xhi); atomicMax(&box[3], yhi);
    }
    __syncthreads();
    const int cx_lo = box[0], cy_lo = box[1], cx_hi = box[2], cy_hi = box[3];     // inside the grid: mw_cell clamps

    uint64_t key1 = SIFT_MW_NONE, key2 = SIFT_MW_NONE;
    uint4 fa, fb;
    float4 fm = make_float4(0.f, 0.f, 0.f, 0.f);
    auto fetch = [&](int p0) {
        const int pa = min(p0 + (tid >> 3), nl - 1), pb = min(p0 + 32 + (tid >> 3), nl - 1);
        fa = desc[(size_t)pa * 8 + (tid & 7)];
        fb = desc[(size_t)pb * 8 + (tid & 7)];
        if (tid < SIFT_MW_TILE) fm = meta[min(p0 + tid, nl - 1)];
    };
    int buf = 0;
    for (int cy = cy_lo; cy <= cy_hi; cy++) {
        const int p_begin = max(start_l[cy * g.gx + cx_lo], 0), p_end = min(start_l[cy * g.gx + cx_hi + 1], nl);
        if (p_begin >= p_end) continue;                                          // uniform over the workgroup
        fetch(p_begin);
        for (int p0 = p_begin; p0 < p_end; p0 += SIFT_MW_TILE, buf ^= 1) {
            tile[buf][tid] = fa;
            tile[buf][256 + tid] = fb;
            if (tid < SIFT_MW_TILE) tmeta[buf][tid] = fm;
            __syncthreads();                  // one barrier per tile: the readers of this buffer passed the previous tile's barrier
            if (p0 + SIFT_MW_TILE < p_end) fetch(p0 + SIFT_MW_TILE);
            const int jn = min(SIFT_MW_TILE, p_end - p0);
            const uint4 *tb = tile[buf];
            for (int j = 0; j < jn; j++) {
                const float4 e = tmeta[buf][j];
                const float ax = reverse ? xq - e.x : e.x - xq, ay = reverse ? yq - e.y : e.y - yq;
                const bool ok = active && fabsf(ax - sx) <= wx && fabsf(ay - sy) <= wy;
                if (__ballot(ok) == 0) continue;                                 // wave-uniform
                uint32_t d = 0;
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    const uint4 v = tb[j * 8 + w];
                    d = __builtin_amdgcn_sad_u8(q[4 * w], v.x, d);
                    d = __builtin_amdgcn_sad_u8(q[4 * w + 1], v.y, d);
                    d = __builtin_amdgcn_sad_u8(q[4 * w + 2], v.z, d);
                    d = __builtin_amdgcn_sad_u8(q[4 * w + 3], v.w, d);
                }
                const uint64_t key = ((uint64_t)d << 32) | (uint32_t)__float_as_int(e.z);
                if (ok) {
                    if (key < key1) { key2 = key1; key1 = key; }
                    else if (key < key2) key2 = key;
                }
            }
        }
    }
    if (!active) return;
    const int best = (int)(uint32_t)key1;
    if (nearest) { nearest[sg.q_first + i] = key1 == SIFT_MW_NONE ? -1 : best; return; }
    // distances are stored as float in the reference, initialised to 1e12f (matching_cpu.cl:103-108)
    const float f1 = key1 == SIFT_MW_NONE ? 1000000000000.0f : (float)(uint32_t)(key1 >> 32);
    const float f2 = key2 == SIFT_MW_NONE ? 1000000000000.0f : (float)(uint32_t)(key2 >> 32);
    // ratio_th <= 1: a query without a candidate (1e12 / 1e12) never passes, so `best` is an element of the list
    dense[(size_t)sg.out + i] = (key1 != SIFT_MW_NONE && f2 != 0.0f && f1 / f2 < ratio_th) ? best : -1;
}

// one workgroup per block of 512 queries, before the compaction: the slots past the block's queries and those of a segment
// without work (MbBlock.nparts == 0) become -1, with nearest_in the pair (i, j) is kept only if nearest_in[l_base + j] == i (the
// mutual filter, as mb_merge_kernel applies it), and sums[e] is the number of the block's pairs.  MbBlock.stride: the list's length.
__global__ __launch_bounds__(256) void mwb_finish_kernel(const MbBlock *__restrict__ blocks, int *__restrict__ dense, int *__restrict__ sums,
                                                         const int *__restrict__ nearest_in) {
    __shared__ int wave_sum[4];
    const int tid = threadIdx.x;
    const MbBlock b = blocks[blockIdx.x];
    int mine = 0;
#pragma unroll
    for (int u = 0; u < SIFT_MATCH_QPT; u++) {
        const int t = u * 256 + tid;
        const size_t slot = (size_t)blockIdx.x * SIFT_MB_QBLOCK + t;
        int out = -1;
        if (t < b.q_count && b.nparts) {
            out = dense[slot];
            if (out >= b.stride) out = -1;
            if (out >= 0 && nearest_in && nearest_in[b.l_base + out] != b.i_first + t) out = -1;
        }
        dense[slot] = out;
        mine += out >= 0;
    }
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

}  // namespace siftk
