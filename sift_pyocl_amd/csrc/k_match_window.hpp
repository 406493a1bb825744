// k_match_window.hpp -- windowed matching: the rule of matching_cpu.cl:57-109 applied only to the
// CANDIDATES of a query, the list elements whose position lies within a window of the query's (shifted) position:
//
//     forward  (query i of list 1, element j of list 2):   fabsf((x2[j] - x1[i]) - sx) <= wx  &&  fabsf((y2[j] - y1[i]) - sy) <= wy
//     reverse  (query j of list 2, element i of list 1):   the same expression, same operand order (mutual check)
//
// in f32, unfused, exactly as written (a NaN makes it false).  Fewer descriptor pairs is the whole point: the list is binned on a
// uniform grid of at most 256 x 256 cells with a cell side of about the window, counting-sorted by cell into a dense copy
// (descriptors in one array, (x, y, original index) in another), the queries are sorted by the cell of their window centre,
// and a workgroup takes up to 256 queries of one cell and streams the small rectangle of cells that holds all their candidates
// through LDS tiles, as match_partial_kernel streams a partition.
//
// Order-free result: the scatter inside a cell is not stable, so the two smallest are kept as 64-bit keys (distance << 32 |
// original index).  The smallest key is the reference's "earliest index of the minimum" and the distance of the second smallest
// key is its dist2 (the second smallest of the multiset), whatever order the candidates arrive in.
//
// Launches of one direction: extent, count (list), count (queries), scan, scatter (list), scatter (queries), match.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace siftk {

#define SIFT_MW_MAXG 256                  // cells per axis at most
#define SIFT_MW_MAXCELLS 65536
#define SIFT_MW_QB 256                    // queries per workgroup
#define SIFT_MW_TILE 64                   // list elements per LDS tile
#define SIFT_MW_NONE 0xffffffffffffffffull
// header words of the cell scratch: min x, min y (ordered encoding, start at 0xffffffff), max x, max y (start at 0), work items
#define SIFT_MW_HDR 8

struct MwGrid { float x0, y0, side_x, side_y; int gx, gy; };

// f32 -> u32 whose unsigned order is the order of the (non-NaN) floats, and back
__device__ __forceinline__ uint32_t mw_enc(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
__device__ __forceinline__ float mw_dec(uint32_t u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u); }

// one axis of the grid from the extent of the list's finite coordinates: the cell side is the window, but at least extent / 256
// so that the axis has at most 256 cells; an infinite window, an extent that overflows or a list without a finite coordinate
// give one cell.  Every kernel of a call derives the same grid from the same header words.
__device__ __forceinline__ void mw_axis(uint32_t umin, uint32_t umax, float w, float &x0, float &side, int &g) {
    float lo = 0.f, ext = 0.f;
    if (umin <= umax) { lo = mw_dec(umin); ext = mw_dec(umax) - lo; }
    side = fmaxf(w, ext / (float)SIFT_MW_MAXG);
    if (!(side > 0.f)) side = 1.f;
    g = 1;
    if (ext < INFINITY && side < INFINITY) g = (int)fminf(ext / side, (float)(SIFT_MW_MAXG - 1)) + 1;
    x0 = lo;
}
__device__ __forceinline__ MwGrid mw_grid(const uint32_t *__restrict__ hdr, float wx, float wy) {
    MwGrid g;
    mw_axis(hdr[0], hdr[2], wx, g.x0, g.side_x, g.gx);
    mw_axis(hdr[1], hdr[3], wy, g.y0, g.side_y, g.gy);
    return g;
}
// The cell of a coordinate.  MONOTONE in v: the f32 subtraction of a constant, the correctly rounded division by a positive
// constant, floorf and the clamp are each non-decreasing, so v <= v' implies cell(v) <= cell(v') and clamping at the edges never
// separates a candidate from the interval that holds it.  The clamp acts on the float, before the conversion (1e30 and the
// infinities land in the edge cells); a NaN goes to cell 0.
__device__ __forceinline__ int mw_cell(float v, float x0, float side, int g) {
    float t = floorf((v - x0) / side);
    if (!(t >= 0.f)) t = 0.f;
    if (t > (float)(g - 1)) t = (float)(g - 1);
    return (int)t;
}
// cell index of the point (x + shx, y + shy); the list is binned with a zero shift (the sum is then x itself)
__device__ __forceinline__ int mw_cell_of(const MwGrid &g, float x, float y, float shx, float shy) {
    const float cx = (float)((double)x + (double)shx), cy = (float)((double)y + (double)shy);
    return mw_cell(cy, g.y0, g.side_y, g.gy) * g.gx + mw_cell(cx, g.x0, g.side_x, g.gx);
}
// The cells [clo, chi] of one axis that hold every candidate of a query at q, for a window w around q + shift.
// Why the margin is enough.  The predicate rounds twice: with a = v - q (or q - v) and b = fl(a) - s it asks |fl(b)| <= w, u = 2^-24
// bounding each relative error (sums of floats have no underflow error).  |fl(b)| <= w gives |b| <= w (1 + 2u), so
// |fl(a)| <= |s| + w (1 + 2u) and |a - fl(a)| <= 2u |fl(a)|: every candidate has |a - s| <= w + 2u w + 2u (|s| + w (1 + 2u))
// < w + 2^-21 (|s| + w) in real numbers.  The interval ends are formed in binary64 (three operations, relative error 2^-53 each
// on magnitudes <= |q| + |s| + w + E) and rounded to f32 once (2^-24 of the same magnitude at most); E = 2^-20 (|q| + |s| + w)
// is more than the sum of the three.  So lo <= v <= hi for every candidate v, and by monotonicity cell(lo) <= cell(v) <= cell(hi).
// An end that overflows becomes an infinity (an edge cell, where such a v is too); a NaN end (NaN or infinite q with an infinite
// window) opens that side completely.  The predicate itself decides about every element of the cells: the range only has to be
// a superset.
__device__ __forceinline__ void mw_range(float q, float shift, float w, float x0, float side, int g, int &clo, int &chi) {
    const double c = (double)q + (double)shift, W = (double)w;
    const double E = (fabs((double)q) + fabs((double)shift) + W) * (1.0 / 1048576.0);
    const float lo = (float)(c - W - E), hi = (float)(c + W + E);
    clo = mw_cell(lo, x0, side, g);                       // NaN -> 0
    chi = (hi != hi) ? g - 1 : mw_cell(hi, x0, side, g);
}

// extent of the finite coordinates of a list: LDS atomics on the ordered encoding, four global atomics per workgroup
__global__ __launch_bounds__(256) void mw_extent_kernel(const uint8_t *__restrict__ kp, int n, uint32_t *__restrict__ hdr) {
    __shared__ uint32_t s[4];
    const int tid = threadIdx.x;
    if (tid < 4) s[tid] = tid < 2 ? 0xffffffffu : 0u;
    __syncthreads();
    const int i = blockIdx.x * 256 + tid;
    if (i < n) {
        const float *k = reinterpret_cast<const float *>(kp + (size_t)i * 144);
        const float x = k[0], y = k[1];
        if (fabsf(x) < INFINITY) { atomicMin(&s[0], mw_enc(x)); atomicMax(&s[2], mw_enc(x)); }
        if (fabsf(y) < INFINITY) { atomicMin(&s[1], mw_enc(y)); atomicMax(&s[3], mw_enc(y)); }
    }
    __syncthreads();
    if (tid < 2) atomicMin(&hdr[tid], s[tid]);
    else if (tid < 4) atomicMax(&hdr[tid], s[tid]);
}

// histogram of a list over the cells (the list itself with a zero shift, the queries by their window centre)
__global__ __launch_bounds__(256) void mw_count_kernel(const uint8_t *__restrict__ kp, int n, const uint32_t *__restrict__ hdr,
                                                       float wx, float wy, float shx, float shy, int *__restrict__ cnt) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const MwGrid g = mw_grid(hdr, wx, wy);
    const float *k = reinterpret_cast<const float *>(kp + (size_t)i * 144);
    atomicAdd(&cnt[mw_cell_of(g, k[0], k[1], shx, shy)], 1);
}

// one workgroup: exclusive scans of both histograms over the cells (start[c], start[cells] = n), the counters turned into
// scatter cursors, and the work list: one item (cell, chunk) per SIFT_MW_QB queries of a cell
__global__ __launch_bounds__(1024) void mw_scan_kernel(uint32_t *__restrict__ hdr, float wx, float wy, int *__restrict__ cnt_l,
                                                       int *__restrict__ cnt_q, int *__restrict__ start_l, int *__restrict__ start_q,
                                                       int2 *__restrict__ work, int work_cap) {
    __shared__ int s[3][1024];
    const int tid = threadIdx.x;
    const MwGrid g = mw_grid(hdr, wx, wy);
    const int cells = g.gx * g.gy;
    const int per = (cells + 1023) / 1024;
    const int c0 = min(tid * per, cells), c1 = min(c0 + per, cells);
    int v[3] = {0, 0, 0};
    for (int c = c0; c < c1; c++) { const int q = cnt_q[c]; v[0] += cnt_l[c]; v[1] += q; v[2] += (q + SIFT_MW_QB - 1) / SIFT_MW_QB; }
    for (int k = 0; k < 3; k++) s[k][tid] = v[k];
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        int t[3];
        for (int k = 0; k < 3; k++) t[k] = tid >= off ? s[k][tid - off] : 0;
        __syncthreads();
        for (int k = 0; k < 3; k++) s[k][tid] += t[k];
        __syncthreads();
    }
    int a = s[0][tid] - v[0], b = s[1][tid] - v[1], w = s[2][tid] - v[2];
    for (int c = c0; c < c1; c++) {
        const int nl = cnt_l[c], nq = cnt_q[c], chunks = (nq + SIFT_MW_QB - 1) / SIFT_MW_QB;
        start_l[c] = a; cnt_l[c] = a;
        start_q[c] = b; cnt_q[c] = b;
        for (int k = 0; k < chunks; k++) if (w + k < work_cap) work[w + k] = make_int2(c, k);
        a += nl; b += nq; w += chunks;
    }
    if (tid == 1023) { start_l[cells] = a; start_q[cells] = b; hdr[4] = (uint32_t)min(w, work_cap); }
}

// counting-sort scatter of the list into the dense copy: eight threads per element, 16 descriptor bytes each
__global__ __launch_bounds__(256) void mw_scatter_list_kernel(const uint8_t *__restrict__ kp, int n, const uint32_t *__restrict__ hdr,
                                                              float wx, float wy, int *__restrict__ cursor,
                                                              uint4 *__restrict__ desc, float4 *__restrict__ meta) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t j = t >> 3;
    const int piece = (int)(t & 7);
    const bool live = j < n;
    float x = 0.f, y = 0.f;
    int pos = 0;
    if (live && piece == 0) {
        const MwGrid g = mw_grid(hdr, wx, wy);
        const float *k = reinterpret_cast<const float *>(kp + (size_t)j * 144);
        x = k[0]; y = k[1];
        pos = atomicAdd(&cursor[mw_cell_of(g, x, y, 0.f, 0.f)], 1);
    }
    pos = __shfl(pos, (int)(threadIdx.x & 63 & ~7));
    if (!live || pos < 0 || pos >= n) return;
    desc[(size_t)pos * 8 + piece] = reinterpret_cast<const uint4 *>(kp + (size_t)j * 144 + 16)[piece];
    if (piece == 0) meta[pos] = make_float4(x, y, __int_as_float((int)j), 0.f);
}

// the queries in cell order (indices only: a workgroup reads its queries' records where they lie)
__global__ __launch_bounds__(256) void mw_scatter_query_kernel(const uint8_t *__restrict__ kp, int n, const uint32_t *__restrict__ hdr,
                                                               float wx, float wy, float shx, float shy, int *__restrict__ cursor,
                                                               int *__restrict__ order) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const MwGrid g = mw_grid(hdr, wx, wy);
    const float *k = reinterpret_cast<const float *>(kp + (size_t)i * 144);
    const int pos = atomicAdd(&cursor[mw_cell_of(g, k[0], k[1], shx, shy)], 1);
    if (pos >= 0 && pos < n) order[pos] = i;
}

// One work item: up to SIFT_MW_QB queries of one cell (a query per lane, its descriptor in 32 VGPRs) against the rectangle of
// cells that holds the candidates of all of them, a row of cells (contiguous in the dense copy) at a time through double-buffered
// LDS tiles.  Every lane evaluates the exact predicate on the tile element's position; an element no lane of the wave accepts
// costs no SAD.  reverse: the lanes are list-2 keypoints and the elements list-1 keypoints (the predicate keeps its operand
// order).  nearest != null: writes the index of the minimum (-1: no candidate) instead of applying the ratio test.
__global__ __launch_bounds__(256) void mw_match_kernel(const uint8_t *__restrict__ kq, int nq, int nl, const uint32_t *__restrict__ hdr,
                                                       float wx, float wy, float sx, float sy, int reverse,
                                                       const int *__restrict__ start_l, const int *__restrict__ start_q,
                                                       const int *__restrict__ order, const int2 *__restrict__ work,
                                                       const uint4 *__restrict__ desc, const float4 *__restrict__ meta,
                                                       float ratio_th, int2 *__restrict__ pairs, int *__restrict__ counter,
                                                       int capacity, int *__restrict__ nearest) {
    __shared__ uint4 tile[2][SIFT_MW_TILE * 8];
    __shared__ float4 tmeta[2][SIFT_MW_TILE];
    __shared__ int box[4];
    if (blockIdx.x >= hdr[4]) return;
    const int tid = threadIdx.x;
    const int2 wk = work[blockIdx.x];
    const MwGrid g = mw_grid(hdr, wx, wy);
    const int q_begin = start_q[wk.x] + wk.y * SIFT_MW_QB, q_end = min(min(start_q[wk.x + 1], q_begin + SIFT_MW_QB), nq);
    const bool active = q_begin + tid < q_end;
    const int i = active ? min(max(order[q_begin + tid], 0), nq - 1) : 0;
    const float *kh = reinterpret_cast<const float *>(kq + (size_t)i * 144);
    const float xq = kh[0], yq = kh[1];
    uint32_t q[32];
    {
        const uint4 *p = reinterpret_cast<const uint4 *>(kq + (size_t)i * 144 + 16);
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
    if (nearest) { nearest[i] = key1 == SIFT_MW_NONE ? -1 : best; return; }
    // distances are stored as float in the reference, initialised to 1e12f (matching_cpu.cl:103-108)
    const float f1 = key1 == SIFT_MW_NONE ? 1000000000000.0f : (float)(uint32_t)(key1 >> 32);
    const float f2 = key2 == SIFT_MW_NONE ? 1000000000000.0f : (float)(uint32_t)(key2 >> 32);
    if (f2 != 0.0f && f1 / f2 < ratio_th) {
        const int old = atomicAdd(counter, 1);
        if (old < capacity) pairs[old] = make_int2(i, best);
    }
}

// mutual check on the forward pairs, their count read on the device: keep (i, j) iff nearest1_of_2[j] == i
__global__ __launch_bounds__(256) void mw_mutual_filter_kernel(const int2 *__restrict__ pairs, const int *__restrict__ n_fwd, int capacity,
                                                               const int *__restrict__ nearest, int n2, int2 *__restrict__ out,
                                                               int *__restrict__ counter) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= min(*n_fwd, capacity)) return;
    const int2 pr = pairs[t];
    if (pr.y < 0 || pr.y >= n2 || nearest[pr.y] != pr.x) return;
    const int o = atomicAdd(counter, 1);
    if (o < capacity) out[o] = pr;
}

}  // namespace siftk
