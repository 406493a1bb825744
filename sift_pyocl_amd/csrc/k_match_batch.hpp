// k_match_batch.hpp -- the brute-force matcher of k_match.hpp over S segment pairs in one set of launches (DESIGN.md section 7
// row 12; restated in numpy by tests/match_batch_ref.py).  The records of S lists lie back to back on either side (or ONE list
// on the first side, which every segment is matched against); segment s gets the rule of `matching` (matching_cpu.cl:57-109)
// on its own two lists, indices local to the segment, and the pairs come out in (segment, i) order.
//
// The counts are host values, so the host builds two tables and the kernels are driven by them; an entry is the same in every
// lane of a workgroup (it is indexed by blockIdx.x), so reading it costs scalar loads:
//   MbWork   one (segment, block of 512 queries, partition of the segment's list): the scan's grid
//   MbBlock  one (segment, block of 512 queries): the grid of the merge and of the scatter
// A block of queries never straddles two segments: a workgroup shares one streamed tile among all its lanes.
//
//   mb_partial_kernel  match_partial_kernel's body: QPT = 2 queries per lane in registers, a double-buffered 64-descriptor LDS
//                      tile, v_sad_hi_u8 into a packed (distance << 16 | index) key, med3 / min.  Its two clamps are to the
//                      entry's own last query and to the partition's own last element, its scan bounds the partition's: no
//                      record of another segment is ever read.
//   mb_merge_kernel    match_merge_kernel's fold over the partitions of a query in ascending order and the f32 ratio test.  It
//                      writes `best` or -1 into slot e * 512 + t of a dense int32 array (every slot of a block is written, the
//                      ones past the block's queries with -1) and the number of its pairs into sums[e]; in "nearest only" form
//                      (the reverse scan of `mutual`) it writes the index of the minimum per query instead.  With nearest_in
//                      the pair (i, j) is kept only if nearest_in[l_base + j] == i: the mutual filter, before the compaction.
//   mb_scan_kernel     one workgroup: the exclusive scan of the blocks' sums (integers), and its values at the segments' first
//                      blocks, which the host turns into pair_counts
//   mb_scatter_kernel  the scan inside a block and the scatter: pairs[offset] = (i, best)
// No kernel waits for another workgroup, and there is no atomic: the result does not depend on scheduling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_match.hpp"

namespace siftk {

#define SIFT_MB_QBLOCK (256 * SIFT_MATCH_QPT)       // queries of one block
#define SIFT_MB_MAX_SEGMENTS 65535
#define SIFT_MB_SCAN_THREADS 1024

// one workgroup of the scan.  Records are counted from the start of their buffer.
struct MbWork {
    int q_first, q_count;       // the block's first query record and its queries, 1 .. 512
    int l_first, l_end;         // the partition's first record and one past its last; l_first < l_end
    int l_local;                // index of l_first inside its segment
    int slot;                   // partial of the block's first query for this partition
    int pad0, pad1;
};

// one block of queries for the merge and the scatter
struct MbBlock {
    int q_count;                // 1 .. 512
    int slot, stride, nparts;   // partial of query t and partition p: slot + p * stride + t; nparts may be 0 (an empty list)
    int i_first;                // index of the block's first query inside its segment
    int l_base;                 // first record of the segment's list (the mutual filter reads nearest_in[l_base + j])
    int q_first;                // the block's first query record (the "nearest only" form writes nearest_out[q_first + t])
    int pad0;
};

__global__ __launch_bounds__(256) void mb_partial_kernel(const uint8_t *__restrict__ kpq, const uint8_t *__restrict__ kpl,
                                                         const MbWork *__restrict__ work, MatchPartial *__restrict__ partial) {
    __shared__ uint4 tile[2][SIFT_MATCH_TILE * 8];
    const int tid = threadIdx.x;
    const MbWork w = work[blockIdx.x];
    const int j_begin = w.l_first, j_end = w.l_end;
    uint32_t q[SIFT_MATCH_QPT][32];
    uint32_t key1[SIFT_MATCH_QPT], key2[SIFT_MATCH_QPT];      // (distance << 16 | index - j_begin) of the smallest / second smallest
#pragma unroll
    for (int u = 0; u < SIFT_MATCH_QPT; u++) {
        key1[u] = SIFT_MATCH_NONE; key2[u] = SIFT_MATCH_NONE;
        const int src = w.q_first + min(u * 256 + tid, w.q_count - 1);        // never past the block's, so the segment's, last query
        const uint4 *p = reinterpret_cast<const uint4 *>(kpq + (size_t)src * 144 + 16);
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const uint4 v = p[k];
            q[u][4 * k] = v.x; q[u][4 * k + 1] = v.y; q[u][4 * k + 2] = v.z; q[u][4 * k + 3] = v.w;
        }
    }
    // each thread stages two 16-byte pieces of a 64-descriptor tile; never past the partition's last element
    auto fetch = [&](int j0, uint4 &a, uint4 &b) {
        const int ja = min(j0 + (tid >> 3), j_end - 1), jb = min(j0 + 32 + (tid >> 3), j_end - 1);
        a = reinterpret_cast<const uint4 *>(kpl + (size_t)ja * 144 + 16)[tid & 7];
        b = reinterpret_cast<const uint4 *>(kpl + (size_t)jb * 144 + 16)[tid & 7];
    };
    uint4 fa, fb;
    fetch(j_begin, fa, fb);
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
            for (int k = 0; k < 8; k++) {
                const uint4 v = tb[j * 8 + k];
#pragma unroll
                for (int u = 0; u < SIFT_MATCH_QPT; u++) {
                    key[u] = __builtin_amdgcn_sad_hi_u8(q[u][4 * k], v.x, key[u]);
                    key[u] = __builtin_amdgcn_sad_hi_u8(q[u][4 * k + 1], v.y, key[u]);
                    key[u] = __builtin_amdgcn_sad_hi_u8(q[u][4 * k + 2], v.z, key[u]);
                    key[u] = __builtin_amdgcn_sad_hi_u8(q[u][4 * k + 3], v.w, key[u]);
                }
            }
#pragma unroll
            for (int u = 0; u < SIFT_MATCH_QPT; u++) {
                // ascending index inside equal distances: the earliest index wins ties (matching_cpu.cl:92-100)
                key2[u] = match_umed3(key1[u], key2[u], key[u]);
                key1[u] = min(key1[u], key[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < SIFT_MATCH_QPT; u++) {
        const int t = u * 256 + tid;
        if (t < w.q_count) {
            MatchPartial r;
            r.d1 = (key1[u] >> 16) == 0x7fffu ? SIFT_MATCH_NONE : (int)(key1[u] >> 16);
            r.best = (key1[u] >> 16) == 0x7fffu ? 0 : w.l_local + (int)(key1[u] & 0xffffu);
            r.d2 = (key2[u] >> 16) == 0x7fffu ? SIFT_MATCH_NONE : (int)(key2[u] >> 16);
            r.pad = 0;
            partial[(size_t)w.slot + t] = r;
        }
    }
}

// nearest_out != null: "nearest only" form, dense / sums / nearest_in are not used
__global__ __launch_bounds__(256) void mb_merge_kernel(const MatchPartial *__restrict__ partial, const MbBlock *__restrict__ blocks,
                                                       float ratio_th, int *__restrict__ dense, int *__restrict__ sums,
                                                       const int *__restrict__ nearest_in, int *__restrict__ nearest_out) {
    __shared__ int wave_sum[4];
    const int tid = threadIdx.x;
    const MbBlock b = blocks[blockIdx.x];
    int mine = 0;
#pragma unroll
    for (int u = 0; u < SIFT_MATCH_QPT; u++) {
        const int t = u * 256 + tid;
        int out = -1;
        if (t < b.q_count) {
            int d1 = SIFT_MATCH_NONE, d2 = SIFT_MATCH_NONE, best = 0;
            for (int p = 0; p < b.nparts; p++) {
                const MatchPartial r = partial[(size_t)b.slot + (size_t)p * b.stride + t];
                // feed the partition's two smallest distances through the reference's update rule, in order
                if (r.d1 < d1) { d2 = d1; d1 = r.d1; best = r.best; }
                else if (r.d1 < d2) d2 = r.d1;
                if (r.d2 < d2) d2 = r.d2;
            }
            if (nearest_out) {
                nearest_out[b.q_first + t] = d1 == SIFT_MATCH_NONE ? -1 : best;
            } else {
                // distances are stored as float in the reference, initialised to 1e12f
                const float f1 = (d1 == SIFT_MATCH_NONE) ? 1000000000000.0f : (float)d1;
                const float f2 = (d2 == SIFT_MATCH_NONE) ? 1000000000000.0f : (float)d2;
                // ratio_th <= 1: a query without a candidate (1e12 / 1e12) never passes, so `best` is an element of the list
                if (f2 != 0.0f && f1 / f2 < ratio_th && d1 != SIFT_MATCH_NONE && (!nearest_in || nearest_in[b.l_base + best] == b.i_first + t))
                    out = best;
            }
        }
        if (!nearest_out) { dense[(size_t)blockIdx.x * SIFT_MB_QBLOCK + t] = out; mine += out >= 0; }
    }
    if (nearest_out) return;                                  // the same in every lane
    for (int d = 32; d > 0; d >>= 1) mine += __shfl_down(mine, d, 64);
    if ((tid & 63) == 0) wave_sum[tid >> 6] = mine;
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

// one workgroup: offs[e] = sums[0] + .. + sums[e - 1] for e = 0 .. n_blocks, then seg_off[s] = offs[seg_block[s]] for
// s = 0 .. n_segments (seg_block[n_segments] == n_blocks: the total)
__global__ __launch_bounds__(SIFT_MB_SCAN_THREADS) void mb_scan_kernel(const int *__restrict__ sums, int n_blocks, int *__restrict__ offs,
                                                                       const int *__restrict__ seg_block, int n_segments,
                                                                       int *__restrict__ seg_off) {
    __shared__ int wave_tot[SIFT_MB_SCAN_THREADS / 64];
    __shared__ int carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) { carry = 0; offs[0] = 0; }
    __syncthreads();
    for (int e0 = 0; e0 < n_blocks; e0 += SIFT_MB_SCAN_THREADS) {
        const int e = e0 + tid;
        const int v = e < n_blocks ? sums[e] : 0;
        int incl = v;                                         // inclusive scan inside the wave
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        int before = carry;
        for (int k = 0; k < wave; k++) before += wave_tot[k];
        if (e < n_blocks) offs[e + 1] = before + incl;
        __syncthreads();                                      // every read of carry and wave_tot is over
        if (tid == SIFT_MB_SCAN_THREADS - 1) carry = before + incl;
        __syncthreads();
    }
    // the workgroup's own global writes are visible to it after the barrier
    for (int s = tid; s <= n_segments; s += SIFT_MB_SCAN_THREADS) seg_off[s] = offs[seg_block[s]];
}

// lane `tid` owns slots 2 * tid and 2 * tid + 1 of its block: ascending slot is ascending i
__global__ __launch_bounds__(256) void mb_scatter_kernel(const int *__restrict__ dense, const int *__restrict__ offs,
                                                         const MbBlock *__restrict__ blocks, int2 *__restrict__ pairs) {
    __shared__ int wave_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const MbBlock b = blocks[blockIdx.x];
    const int2 v = reinterpret_cast<const int2 *>(dense + (size_t)blockIdx.x * SIFT_MB_QBLOCK)[tid];
    const int c = (v.x >= 0) + (v.y >= 0);
    int incl = c;
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
    }
    if (lane == 63) wave_tot[wave] = incl;
    __syncthreads();
    int pos = offs[blockIdx.x] + incl - c;
    for (int k = 0; k < wave; k++) pos += wave_tot[k];
    if (v.x >= 0) pairs[pos++] = make_int2(b.i_first + 2 * tid, v.x);
    if (v.y >= 0) pairs[pos] = make_int2(b.i_first + 2 * tid + 1, v.y);
}

}  // namespace siftk
