// k_knn_window.hpp -- k nearest neighbours INSIDE A SEARCH WINDOW (extension; the contract is DESIGN.md section 7 row 10, restated in
// numpy by tests/knn_window_ref.py): row i of the result holds the k smallest (d(i, j), j) over the CANDIDATES j of query i --
// k_match_window.hpp's predicate, forward form -- in ascending lexicographic order, -1 / -1 where i has fewer than k candidates.
// d is k_knn.hpp's int32 L1 distance or k_knn_l2.hpp's int32 squared Euclidean distance over the 128 descriptor bytes.
//
// The grid, the counting sort and the proof that a query's cell range holds its candidates are k_match_window.hpp's, launched
// unchanged; mw_knn_kernel<K, L2> has mw_match_kernel's decomposition: up to 256 queries of one cell per workgroup, a query per
// lane with its descriptor in 32 VGPRs, the bounding rectangle of the queries' cell ranges streamed a row of cells at a time
// through double-buffered 64-descriptor LDS tiles, the exact predicate per lane and element, no distance for an element that no
// lane of the wave accepts.  It differs in two things.
//   The keys.  A lane keeps K sorted 64-bit keys (distance << 32 | original index), SIFT_MW_NONE where there is none yet.  An
//   accepted key that is below the K-th runs through K compare / exchange steps.  The index is part of the key, so every key is
//   distinct and the chain's result is the contract's order whatever order the scatter left the cell in.
//   The squared Euclidean distance.  d = |a|^2 + |b|^2 - 2 a.b with 32 v_dot4_u32_u8 for the product (every term is an exact
//   unsigned integer and |a|^2 + |b|^2 >= 2 a.b, so the 32-bit result is exact).  |a|^2 is formed once per lane; |b|^2 once per tile
//   element by the eight lanes that stage it (4 dots each, knn_l2_sum8's three DPP adds) and lies beside the tile in LDS.
//
// Resources (tools/resource_usage.py, gfx950):       VGPR     SGPR     LDS              scratch  waves/SIMD
//   mw_knn_kernel<1, false> / <1, true>             78 / 80  48 / 52  18 448 / 18 960     0       6 / 6
//   mw_knn_kernel<2, false> / <2, true>             80 / 82  48 / 52  18 448 / 18 960     0       6 / 5
//   mw_knn_kernel<4, false> / <4, true>             84 / 86  48 / 52  18 448 / 18 960     0       5 / 5
//   mw_knn_kernel<8, false> / <8, true>             94 / 96  48 / 52  18 448 / 18 960     0       5 / 5
//   (mw_match_kernel beside them: 81 VGPRs, 52 SGPRs, 18 448 B LDS, 5 waves per SIMD)
// No instance spills.  The LDS would let 8 workgroups share a CU (8 waves per SIMD); the registers decide.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_knn_l2.hpp"
#include "k_match_window.hpp"

namespace siftk {

template <int K, bool L2>
__global__ __launch_bounds__(256) void mw_knn_kernel(const uint8_t *__restrict__ kq, int nq, int nl, const uint32_t *__restrict__ hdr,
                                                     float wx, float wy, float sx, float sy,
                                                     const int *__restrict__ start_l, const int *__restrict__ start_q,
                                                     const int *__restrict__ order, const int2 *__restrict__ work,
                                                     const uint4 *__restrict__ desc, const float4 *__restrict__ meta,
                                                     int k, int32_t *__restrict__ idx, int32_t *__restrict__ dist) {
    __shared__ uint4 tile[2][SIFT_MW_TILE * 8];
    __shared__ float4 tmeta[2][SIFT_MW_TILE];
    __shared__ uint32_t tsq[L2 ? 2 : 1][L2 ? SIFT_MW_TILE : 1];      // |b|^2 of the tile's elements
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
    uint32_t aa = 0;                                                 // |a|^2
    {
        const uint4 *p = reinterpret_cast<const uint4 *>(kq + (size_t)i * 144 + 16);
#pragma unroll
        for (int w = 0; w < 8; w++) {
            const uint4 v = p[w];
            q[4 * w] = v.x; q[4 * w + 1] = v.y; q[4 * w + 2] = v.z; q[4 * w + 3] = v.w;
            if (L2) aa += knn_l2_sq16(v);
        }
    }
    if (tid < 4) box[tid] = tid < 2 ? 0x7fffffff : -1;
    __syncthreads();
    if (active) {
        int xlo, xhi, ylo, yhi;
        mw_range(xq, sx, wx, g.x0, g.side_x, g.gx, xlo, xhi);
        mw_range(yq, sy, wy, g.y0, g.side_y, g.gy, ylo, yhi);
        atomicMin(&box[0], xlo); atomicMin(&box[1], ylo); atomicMax(&box[2], xhi); atomicMax(&box[3], yhi);
    }
    __syncthreads();
    const int cx_lo = box[0], cy_lo = box[1], cx_hi = box[2], cy_hi = box[3];     // inside the grid: mw_cell clamps

    uint64_t keys[K];                                                // ascending; SIFT_MW_NONE where there is none yet
#pragma unroll
    for (int r = 0; r < K; r++) keys[r] = SIFT_MW_NONE;
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
            if (L2) {                         // every lane of the wave takes part in the DPP adds: the loop is uniform over the workgroup
                const uint32_t sa = knn_l2_sum8(knn_l2_sq16(fa)), sb = knn_l2_sum8(knn_l2_sq16(fb));
                if ((tid & 7) == 0) { tsq[buf][tid >> 3] = sa; tsq[buf][32 + (tid >> 3)] = sb; }
            }
            __syncthreads();                  // one barrier per tile: the readers of this buffer passed the previous tile's barrier
            if (p0 + SIFT_MW_TILE < p_end) fetch(p0 + SIFT_MW_TILE);
            const int jn = min(SIFT_MW_TILE, p_end - p0);
            const uint4 *tb = tile[buf];
            for (int j = 0; j < jn; j++) {
                const float4 e = tmeta[buf][j];
                const float ax = e.x - xq, ay = e.y - yq;
                const bool ok = active && fabsf(ax - sx) <= wx && fabsf(ay - sy) <= wy;
                if (__ballot(ok) == 0) continue;                                 // wave-uniform
                uint32_t d = 0;
#pragma unroll
                for (int w = 0; w < 8; w++) {
                    const uint4 v = tb[j * 8 + w];
                    if (L2) {
                        d = __builtin_amdgcn_udot4(q[4 * w], v.x, d, false);
                        d = __builtin_amdgcn_udot4(q[4 * w + 1], v.y, d, false);
                        d = __builtin_amdgcn_udot4(q[4 * w + 2], v.z, d, false);
                        d = __builtin_amdgcn_udot4(q[4 * w + 3], v.w, d, false);
                    } else {
                        d = __builtin_amdgcn_sad_u8(q[4 * w], v.x, d);
                        d = __builtin_amdgcn_sad_u8(q[4 * w + 1], v.y, d);
                        d = __builtin_amdgcn_sad_u8(q[4 * w + 2], v.z, d);
                        d = __builtin_amdgcn_sad_u8(q[4 * w + 3], v.w, d);
                    }
                }
                if (L2) d = aa + tsq[buf][j] - 2u * d;
                uint64_t c = ((uint64_t)d << 32) | (uint32_t)__float_as_int(e.z);
                if (ok && c < keys[K - 1]) {
#pragma unroll
                    for (int r = 0; r < K; r++) {                                // slot r keeps the smaller, the larger moves on
                        const bool below = c < keys[r];
                        const uint64_t lo = below ? c : keys[r];
                        c = below ? keys[r] : c;
                        keys[r] = lo;
                    }
                }
            }
        }
    }
    if (!active) return;
#pragma unroll
    for (int r = 0; r < K; r++)
        if (r < k) {
            const bool none = keys[r] == SIFT_MW_NONE;
            idx[(size_t)i * k + r] = none ? -1 : (int32_t)(uint32_t)keys[r];
            dist[(size_t)i * k + r] = none ? -1 : (int32_t)(uint32_t)(keys[r] >> 32);
        }
}

}  // namespace siftk
