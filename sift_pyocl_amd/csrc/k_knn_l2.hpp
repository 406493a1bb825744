// k_knn_l2.hpp -- k nearest neighbours under the SQUARED EUCLIDEAN descriptor distance (extension; the contract is DESIGN.md
// section 7 row 8, restated in numpy by tests/knn_l2_ref.py): d(i, j) = sum over the 128 bytes of (a - b)^2, 0 .. 8 323 200
// (= 128 * 255^2 = 0x7F0100), as int32; everything else is k_knn.hpp's contract: row i holds the k smallest (d(i, j), j) in ascending
// lexicographic order.  No square root is taken on the device.  k_knn.hpp's kernels are not touched: these are kernels of their own.
//
// knn_l2_partial_kernel<K> keeps knn_partial_kernel's decomposition -- query blocks x partitions of the list, QPT query descriptors
// in registers, double-buffered 64-descriptor LDS tiles read by broadcast -- and differs in three things.
//   The distance.  (a - b)^2 has no packed-byte instruction; d = |a|^2 + |b|^2 - 2 a.b, with v_dot4_u32_u8 for the product: 32 per
//   pair, as many as the 32 v_sad_hi_u8 of the L1 kernel.  A dot product can only be ADDED to an accumulator, so the registers hold
//   the queries' COMPLEMENT, 255 - a: (255 - a).b = 255 sum(b) - a.b, and d - |a|^2 = (|b|^2 - 510 sum(b)) + 2 (255 - a).b.  |a|^2 is
//   the same for every element of a query's row, so it takes no part in the order: the partial kernel ranks by the BIASED distance
//   v = d - |a|^2 + 8 323 200 (the bias is the largest |a|^2, so 0 <= v <= 16 646 400 < 2^24), and the merge kernel, one lane per
//   query, forms |a|^2 and takes the bias off.  (|b|^2 - 510 sum(b) + bias) is formed once per tile element by the eight lanes that
//   stage it: each takes its 16 bytes (8 dots), three DPP adds sum the eight, one lane writes the word -- 16 dots and 6 adds per
//   lane and tile against 64 * 64 dots, under 1 %.
//   The key.  24 bits of biased distance leave 8 for an index: the key is (v << 8 | index in a WINDOW of 256 elements, 4 tiles), at
//   most 0xFE0100FF, below the all-ones "none".  The element's word w = ((|b|^2 - 510 sum(b) + bias) << 8) + index lies beside the
//   tile, and the key is w + ((255 - a).b << 9) modulo 2^32: ONE v_lshl_add_u32 beside the same 2K - 2 min / max / med3 chain as
//   knn_partial_kernel's.  A step of the pair loop is 32 + 1 + 2K - 2 instructions per query where the L1 kernel has 32 + 2K - 2.
//   The fold.  After every window (and at the end of the partition) the K window keys are merged into the partition's K running
//   64-bit keys (v << 32 | index in the WHOLE list) and reset.  The running keys live in the result buffer itself, not in registers
//   (K = 8 would need 32 more): a lane reads its own keys back one slot at a time, passes the window's K keys through the slot
//   (compare / exchange: the slot keeps the smallest) and writes it -- the steps of inserting the keys one by one, in slot-major
//   order.  16 K bytes each way and K^2 exchanges of five instructions per query and 256 pairs: 640 for both queries at K = 8
//   against 256 * (64 + 2 + 28), 2.7 %; 0.2 % at K = 2.  A partition's first window starts from "none" without reading.
// A window's keys ascend in (distance, index), and every 64-bit key is distinct (the index is part of it), so the result is the
// contract's order whatever the partitioning is.  The kernel writes K 64-bit keys per (partition, query): nparts * n1 * K * 8
// bytes, 70 MB at 100k x 100k and K = 8; the index is the list's own, so a partition is not limited to 65 472 elements by it (the
// host keeps knn_partial_kernel's partitions all the same).
// knn_l2_merge_kernel<K>, one lane per query, folds the partitions' keys into the K smallest and writes the first k of them as idx /
// dist (with |a|^2 - bias added), -1 where the list has fewer than k elements.
//
// Resources (tools/resource_usage.py, gfx950):       VGPR  SGPR  LDS     scratch  waves/SIMD
//   knn_l2_partial_kernel<1>                           120    33  16 896     0        4
//   knn_l2_partial_kernel<2>                           121    33  16 896     0        4
//   knn_l2_partial_kernel<4>                           125    33  16 896     0        4
//   knn_l2_partial_kernel<8>                           128    33  16 896     0        4
//   knn_l2_merge_kernel<1> / <2> / <4> / <8>     40 / 46 / 56 / 80   16 - 30     0     0     8 / 8 / 8 / 6
//   (knn_partial_kernel<1> / <2> / <4> / <8> beside them: 114 / 116 / 122 / 127 VGPRs, 16 384 B LDS, 4 waves per SIMD)
// K = 8 needs the amdgpu_waves_per_eu(4) below: left alone the compiler takes 132 registers and three waves; held to 128 it
// neither spills nor uses scratch.  The pair loop, unrolled four times, holds per instance 256 v_dot4_u32_u8, 8 v_lshl_add_u32 and
// 8 (2K - 2) min / max / med3 (K = 1: 4 v_min3_u32), and 12 / 9 / 22 / 19 s_nop (K = 1 / 2 / 4 / 8) that the compiler puts between a
// dot product and an LDS read that reuses its register; with them, the fold and the words the measured L2 / L1 kernel time, 1.08 -
// 1.13 at 100k x 100k, is what the instruction counts give.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_knn.hpp"

namespace siftk {

#define SIFT_KNN_L2_WINDOW 256           // list elements per window: the index shares a key with the distance (8 bits)
#define SIFT_KNN_L2_NONE 0xffffffffu
#define SIFT_KNN_L2_BIAS 8323200u        // 128 * 255^2, the largest |a|^2: |b|^2 - 2 a.b + BIAS is never negative

// |v|^2 and the sum of 16 bytes
__device__ __forceinline__ uint32_t knn_l2_sq16(const uint4 v) {
    uint32_t s = __builtin_amdgcn_udot4(v.x, v.x, 0u, false);
    s = __builtin_amdgcn_udot4(v.y, v.y, s, false);
    s = __builtin_amdgcn_udot4(v.z, v.z, s, false);
    return __builtin_amdgcn_udot4(v.w, v.w, s, false);
}
__device__ __forceinline__ uint32_t knn_l2_sum16(const uint4 v) {
    uint32_t s = __builtin_amdgcn_udot4(v.x, 0x01010101u, 0u, false);
    s = __builtin_amdgcn_udot4(v.y, 0x01010101u, s, false);
    s = __builtin_amdgcn_udot4(v.z, 0x01010101u, s, false);
    return __builtin_amdgcn_udot4(v.w, 0x01010101u, s, false);
}
// the sum over the eight lanes that stage one tile element (lanes 8e .. 8e + 7 of a wave), in every one of them: three DPP adds
// (lane ^ 1 and lane ^ 2 inside a quad, then the mirror image inside the eight, which lies in the other quad)
__device__ __forceinline__ uint32_t knn_l2_sum8(uint32_t s) {
    s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0xB1, 0xF, 0xF, false);       // quad_perm [1, 0, 3, 2]
    s += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x4E, 0xF, 0xF, false);       // quad_perm [2, 3, 0, 1]
    return s + (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s, 0x141, 0xF, 0xF, false); // row_half_mirror
}
// the word of a tile element from its lanes' 16 bytes: ((|b|^2 - 510 sum(b) + BIAS) << 8) + index in the window, modulo 2^32
__device__ __forceinline__ uint32_t knn_l2_word(const uint4 v, uint32_t index) {
    return ((knn_l2_sum8(knn_l2_sq16(v) - __umul24(knn_l2_sum16(v), 510u)) + SIFT_KNN_L2_BIAS) << 8) + index;
}

template <int K>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void knn_l2_partial_kernel(const uint8_t *__restrict__ kp1, int n1, const uint8_t *__restrict__ kp2,
                                                             int n2, int part_len, uint64_t *__restrict__ partial) {
    __shared__ uint4 tile[2][SIFT_MATCH_TILE * 8];
    __shared__ uint32_t tword[2][SIFT_MATCH_TILE];      // knn_l2_word of the tile's elements
    const int tid = threadIdx.x;
    const int j_begin = blockIdx.y * part_len, j_end = min(j_begin + part_len, n2);
    uint32_t q[SIFT_MATCH_QPT][32];            // the COMPLEMENT of the query's bytes, 255 - a
    int qi[SIFT_MATCH_QPT];
    uint32_t keys[SIFT_MATCH_QPT][K];          // ascending (biased distance << 8 | index in the window), SIFT_KNN_L2_NONE where there is none yet
#pragma unroll
    for (int u = 0; u < SIFT_MATCH_QPT; u++) {
        qi[u] = (blockIdx.x * SIFT_MATCH_QPT + u) * 256 + tid;
#pragma unroll
        for (int r = 0; r < K; r++) keys[u][r] = SIFT_KNN_L2_NONE;
        const int src = min(qi[u], n1 - 1);
        const uint4 *p = reinterpret_cast<const uint4 *>(kp1 + (size_t)src * 144 + 16);
#pragma unroll
        for (int w = 0; w < 8; w++) {
            const uint4 v = p[w];
            q[u][4 * w] = ~v.x; q[u][4 * w + 1] = ~v.y; q[u][4 * w + 2] = ~v.z; q[u][4 * w + 3] = ~v.w;
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
        const uint32_t jl0 = (uint32_t)(j0 - j_begin);                       // a multiple of the tile
        const uint32_t w0 = jl0 & (SIFT_KNN_L2_WINDOW - 1);                  // the tile's first index in its window
        tile[buf][tid] = fa;
        tile[buf][256 + tid] = fb;
        {
            const uint32_t wa = knn_l2_word(fa, w0 + (uint32_t)(tid >> 3)), wb = knn_l2_word(fb, w0 + 32u + (uint32_t)(tid >> 3));
            if ((tid & 7) == 0) { tword[buf][tid >> 3] = wa; tword[buf][32 + (tid >> 3)] = wb; }
        }
        __syncthreads();                      // one barrier per tile: the other buffer is free by construction
        if (j0 + SIFT_MATCH_TILE < j_end) fetch(j0 + SIFT_MATCH_TILE, fa, fb);
        const int jn = min(SIFT_MATCH_TILE, j_end - j0);
        const uint4 *tb = tile[buf];
        const uint32_t *tw = tword[buf];
#pragma unroll 4
        for (int j = 0; j < jn; j++) {
            uint32_t dot[SIFT_MATCH_QPT];      // (255 - a).b
#pragma unroll
            for (int u = 0; u < SIFT_MATCH_QPT; u++) dot[u] = 0;
#pragma unroll
            for (int w = 0; w < 8; w++) {
                const uint4 v = tb[j * 8 + w];
#pragma unroll
                for (int u = 0; u < SIFT_MATCH_QPT; u++) {
                    dot[u] = __builtin_amdgcn_udot4(q[u][4 * w], v.x, dot[u], false);
                    dot[u] = __builtin_amdgcn_udot4(q[u][4 * w + 1], v.y, dot[u], false);
                    dot[u] = __builtin_amdgcn_udot4(q[u][4 * w + 2], v.z, dot[u], false);
                    dot[u] = __builtin_amdgcn_udot4(q[u][4 * w + 3], v.w, dot[u], false);
                }
            }
            const uint32_t wj = tw[j];
#pragma unroll
            for (int u = 0; u < SIFT_MATCH_QPT; u++) {
                uint32_t c = (dot[u] << 9) + wj;    // (|b|^2 - 510 sum(b) + 2 (255 - a).b + BIAS) << 8 | index: one v_lshl_add_u32
#pragma unroll
                for (int r = 0; r + 2 < K; r++) {   // slot r keeps the smaller, the larger moves on
                    const uint32_t lo = min(keys[u][r], c);
                    c = max(keys[u][r], c);
                    keys[u][r] = lo;
                }
                if (K >= 2) keys[u][K - 1] = match_umed3(keys[u][K - 2], keys[u][K - 1], c);
                keys[u][K >= 2 ? K - 2 : 0] = min(keys[u][K >= 2 ? K - 2 : 0], c);
            }
        }
        // the end of a window or of the partition: fold the window's keys into the running keys (in `partial`) and reset them
        if (w0 == SIFT_KNN_L2_WINDOW - SIFT_MATCH_TILE || j0 + SIFT_MATCH_TILE >= j_end) {
            const uint32_t g0 = (uint32_t)j0 - w0;                           // the window's first index in the list
            const bool first = jl0 < SIFT_KNN_L2_WINDOW;                     // the partition's first window: no running key yet
#pragma unroll
            for (int u = 0; u < SIFT_MATCH_QPT; u++) {
                if (qi[u] < n1) {
                    uint64_t *dst = partial + ((size_t)blockIdx.y * n1 + qi[u]) * K;
                    uint64_t c[K];             // the window's keys as running keys; a "none" is above every running key
#pragma unroll
                    for (int s = 0; s < K; s++)
                        c[s] = keys[u][s] == SIFT_KNN_L2_NONE ? SIFT_KNN_NONE64
                                                              : ((uint64_t)(keys[u][s] >> 8) << 32) | (uint64_t)(g0 + (keys[u][s] & (SIFT_KNN_L2_WINDOW - 1)));
                    // slot by slot (one running key in registers at a time): slot r keeps the smallest of itself and what the
                    // slots before it handed on -- the compare / exchange steps of inserting the keys one by one, in an order
                    // that respects what each step depends on
#pragma unroll
                    for (int r = 0; r < K; r++) {
                        uint64_t run = first ? SIFT_KNN_NONE64 : dst[r];
#pragma unroll
                        for (int s = 0; s < K; s++) {
                            const bool below = c[s] < run;
                            const uint64_t lo = below ? c[s] : run;
                            c[s] = below ? run : c[s];
                            run = lo;
                        }
                        dst[r] = run;
                    }
                }
#pragma unroll
                for (int r = 0; r < K; r++) keys[u][r] = SIFT_KNN_L2_NONE;
            }
        }
    }
    if (j_begin >= j_end) {                   // a partition without elements (the host makes none): no key
#pragma unroll
        for (int u = 0; u < SIFT_MATCH_QPT; u++)
            if (qi[u] < n1)
#pragma unroll
                for (int r = 0; r < K; r++) partial[((size_t)blockIdx.y * n1 + qi[u]) * K + r] = SIFT_KNN_NONE64;
    }
}

// fold the partitions' keys (distance << 32 | j).  A partition's keys ascend and its "none" slots come last, so the first key that
// is not below the K-th smallest so far ends a partition.
template <int K>
__global__ __launch_bounds__(256) void knn_l2_merge_kernel(const uint64_t *__restrict__ partial, const uint8_t *__restrict__ kp1, int n1,
                                                           int nparts, int k, int32_t *__restrict__ idx, int32_t *__restrict__ dist) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n1) return;
    uint32_t aa = 0;                          // |a|^2: the partial kernel's distances are d - |a|^2 + BIAS
    const uint4 *p = reinterpret_cast<const uint4 *>(kp1 + (size_t)i * 144 + 16);
#pragma unroll
    for (int w = 0; w < 8; w++) aa += knn_l2_sq16(p[w]);
    uint64_t keys[K];
#pragma unroll
    for (int r = 0; r < K; r++) keys[r] = SIFT_KNN_NONE64;
    for (int p = 0; p < nparts; p++) {
        const uint64_t *src = partial + ((size_t)p * n1 + i) * K;
        uint64_t pk[K];
#pragma unroll
        for (int r = 0; r < K; r++) pk[r] = src[r];
#pragma unroll
        for (int s = 0; s < K; s++) {
            uint64_t c = pk[s];
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
            dist[(size_t)i * k + r] = none ? -1 : (int32_t)((uint32_t)(keys[r] >> 32) + aa - SIFT_KNN_L2_BIAS);
        }
}

}  // namespace siftk
