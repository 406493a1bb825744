// k_knn.hpp -- k nearest neighbours of every list-1 descriptor among list 2, WITH their L1 distances (extension; the contract is
// DESIGN.md section 7 row 7, restated in numpy by tests/knn_ref.py).  Row i of the result holds the k smallest elements of
// {(d(i, j), j)} in ascending lexicographic order: among equal distances the smaller index comes first.  The order is total, so
// the result does not depend on partitioning, tile order or scheduling.
//
// knn_partial_kernel<K> is match_partial_kernel's decomposition (k_match.hpp) -- query blocks x partitions of the list, QPT query
// descriptors in registers, double-buffered 64-descriptor LDS tiles read by broadcast, 32 v_sad_hi_u8 per pair accumulating into the
// key (distance << 16 | index in the partition), started from the index -- with K sorted keys per query in place of two.  A new key
// goes through a min / max chain: slot r keeps min(slot, key) and hands max(slot, key) on, and the last two slots take it as
// match_partial_kernel's pair does (v_med3_u32, v_min_u32): 2K - 2 instructions per pair beside the 32 SADs, for K = 2 the
// matcher's own two.  Keys of one query are distinct (the index is part of them), so the chain is a plain insertion into a sorted
// list; the 0x7fffffff "none" sentinel is above every key (the largest is 0x7f80 << 16 | 65 471).  It writes K keys per
// (partition, query).
// knn_merge_kernel<K>, one lane per query, folds the partitions' keys into the K smallest 64-bit keys (distance << 32 | j), as
// mw_match_kernel does for two, and writes the first k of them as idx / dist with -1 where the list has fewer than k elements.
// K is a template parameter (1, 2, 4, 8: every slot has a compile-time index and lives in a register); a requested k is rounded
// up to the next instance and the merge writes k columns.
//
// Resources (tools/resource_usage.py, gfx950):       VGPR  SGPR  LDS     scratch  waves/SIMD
//   knn_partial_kernel<1>                             114    26  16 384     0        4
//   knn_partial_kernel<2>                             116    26  16 384     0        4
//   knn_partial_kernel<4>                             122    25  16 384     0        4
//   knn_partial_kernel<8>                             127    25  16 384     0        4
//   knn_merge_kernel<1> / <2> / <4> / <8>     11 / 22 / 38 / 70   20 - 50     0     0     8 / 8 / 8 / 7
//   (match_partial_kernel<false> beside them:         116    27  16 384     0        4)
// The unrolled pair loop holds, per instance, 64 v_sad_hi_u8 per step and 2 (2K - 2) min / max / med3 (K = 1: 2 min).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_match.hpp"

namespace siftk {

#define SIFT_KNN_MAX 8
#define SIFT_KNN_NONE64 0xffffffffffffffffull

template <int K>
__global__ __launch_bounds__(256) void knn_partial_kernel(const uint8_t *__restrict__ kp1, int n1, const uint8_t *__restrict__ kp2,
                                                          int n2, int part_len, uint32_t *__restrict__ partial) {
    __shared__ uint4 tile[2][SIFT_MATCH_TILE * 8];
    const int tid = threadIdx.x;
    const int j_begin = blockIdx.y * part_len, j_end = min(j_begin + part_len, n2);
    uint32_t q[SIFT_MATCH_QPT][32];
    int qi[SIFT_MATCH_QPT];
    uint32_t keys[SIFT_MATCH_QPT][K];          // ascending (distance << 16 | index - j_begin), SIFT_MATCH_NONE where there is none yet
#pragma unroll
    for (int u = 0; u < SIFT_MATCH_QPT; u++) {
        qi[u] = (blockIdx.x * SIFT_MATCH_QPT + u) * 256 + tid;
#pragma unroll
        for (int r = 0; r < K; r++) keys[u][r] = SIFT_MATCH_NONE;
        const int src = min(qi[u], n1 - 1);
        const uint4 *p = reinterpret_cast<const uint4 *>(kp1 + (size_t)src * 144 + 16);
#pragma unroll
        for (int w = 0; w < 8; w++) {
            const uint4 v = p[w];
            q[u][4 * w] = v.x; q[u][4 * w + 1] = v.y; q[u][4 * w + 2] = v.z; q[u][4 * w + 3] = v.w;
        }
    }
    // each thread stages two 16-byte pieces of a 64-descriptor tile
    auto fetch = [&](int j0, uint4 &a, uint4 &b) {
        const int ja = min(j0 + (tid >> 3), n2 - 1), jb = min(j0 + 32 + (tid >> 3), n2 - 1);
        a = reinterpret_cast<const uint4 *>(kp2 + (size_t)ja * 144 + 16)[tid & 7];
        b = reinterpret_cast<const uint4 *>(kp2 + (size_t)jb * 144 + 16)[tid & 7];
    };
    uint4 fa, fb;
    if (j_begin < j_end) fetch(j_begin, fa, fb);
    int buf = 0;
    for (int j0 = j_begin; j0 < j_end; j0 += SIFT_MATCH_TILE, buf ^= 1) {
        tile[buf][tid] = fa;
        tile[buf][256 + tid] = fb;
        __syncthreads();                      // one barrier per tile: the other buffer is free by construction
        if (j0 + SIFT_MATCH_TILE < j_end) fetch(j0 + SIFT_MATCH_TILE, fa, fb);
        const int jn = min(SIFT_MATCH_TILE, j_end - j0);
        const uint4 *tb = tile[buf];
        const uint32_t jl0 = (uint32_t)(j0 - j_begin);
#pragma unroll 4
        for (int j = 0; j < jn; j++) {
            uint32_t key[SIFT_MATCH_QPT];
#pragma unroll
            for (int u = 0; u < SIFT_MATCH_QPT; u++) key[u] = jl0 + (uint32_t)j;
#pragma unroll
            for (int w = 0; w < 8; w++) {
                const uint4 v = tb[j * 8 + w];
#pragma unroll
                for (int u = 0; u < SIFT_MATCH_QPT; u++) {
                    key[u] = __builtin_amdgcn_sad_hi_u8(q[u][4 * w], v.x, key[u]);
                    key[u] = __builtin_amdgcn_sad_hi_u8(q[u][4 * w + 1], v.y, key[u]);
                    key[u] = __builtin_amdgcn_sad_hi_u8(q[u][4 * w + 2], v.z, key[u]);
                    key[u] = __builtin_amdgcn_sad_hi_u8(q[u][4 * w + 3], v.w, key[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < SIFT_MATCH_QPT; u++) {
                uint32_t c = key[u];            // slot r keeps the smaller, the larger moves on
#pragma unroll
                for (int r = 0; r + 2 < K; r++) {
                    const uint32_t lo = min(keys[u][r], c);
                    c = max(keys[u][r], c);
                    keys[u][r] = lo;
                }
                // the last two slots as match_partial_kernel's pair: the second smallest of the three, then the smallest
                if (K >= 2) keys[u][K - 1] = match_umed3(keys[u][K - 2], keys[u][K - 1], c);
                keys[u][K >= 2 ? K - 2 : 0] = min(keys[u][K >= 2 ? K - 2 : 0], c);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < SIFT_MATCH_QPT; u++)
        if (qi[u] < n1) {
            uint32_t *dst = partial + ((size_t)blockIdx.y * n1 + qi[u]) * K;
#pragma unroll
            for (int r = 0; r < K; r++) dst[r] = keys[u][r];
        }
}

// fold the partitions' keys: global key = distance << 32 | (partition start + index in the partition).  A partition's keys ascend and
// its "none" slots come last, so the first sentinel, or the first key that is not below the K-th smallest so far, ends a partition.
template <int K>
__global__ __launch_bounds__(256) void knn_merge_kernel(const uint32_t *__restrict__ partial, int n1, int nparts, int part_len, int k,
                                                        int32_t *__restrict__ idx, int32_t *__restrict__ dist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    uint64_t keys[K];
#pragma unroll
    for (int r = 0; r < K; r++) keys[r] = SIFT_KNN_NONE64;
    for (int p = 0; p < nparts; p++) {
        const uint32_t *src = partial + ((size_t)p * n1 + i) * K;
        uint32_t pk[K];
#pragma unroll
        for (int r = 0; r < K; r++) pk[r] = src[r];
        const uint64_t j0 = (uint64_t)p * (uint64_t)part_len;
#pragma unroll
        for (int s = 0; s < K; s++) {
            if ((pk[s] >> 16) == 0x7fffu) break;
            uint64_t c = ((uint64_t)(pk[s] >> 16) << 32) | (j0 + (pk[s] & 0xffffu));
            if (c >= keys[K - 1]) break;
#pragma unroll
            for (int r = 0; r < K; r++) {
                const uint64_t lo = min(keys[r], c);
                c = max(keys[r], c);
                keys[r] = lo;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < K; r++)
        if (r < k) {
            const bool none = keys[r] == SIFT_KNN_NONE64;
            idx[(size_t)i * k + r] = none ? -1 : (int32_t)(keys[r] & 0xffffffffull);
            dist[(size_t)i * k + r] = none ? -1 : (int32_t)(keys[r] >> 32);
        }
}

}  // namespace siftk
