// k_consensus_batch.hpp -- the consensus filter (k_consensus.hpp) over the S segments of a batch in one set of launches (DESIGN.md
// section 7 row 14): what siftmi_match_batch leaves behind -- record lists back to back, pairs with indices local to their segment,
// pair_counts -- goes in unchanged, and segment s gets, bit for bit, what siftmi_match_consensus gives on that segment alone with the
// same n_hyp, tol and seed; tests/consensus_batch_ref.py restates it by slicing.
//
//   gather   k_estimate_batch.hpp's rule: row r of segment s with local (i, j) reads kp1[off1 + i] iff 0 <= i < n1_s and
//            kp2[off2 + j] iff 0 <= j < n2_s, else it is four NaN: a record of a neighbouring segment is never read
//   sample   mod the segment's own number of pairs, the row's position inside the segment as the pair index
//   solve, vote, select, mask: k_consensus.hpp's, through the very functions its kernels call
//
// The host builds one table (CbWork): an entry per tile -- up to SIFT_CONS_TILE rows of ONE segment, tiles never straddle
// segments -- and an entry per active segment (at least three pairs; `act` is its dense index, -1 for the tiles of the others).
// Models, flags and votes of active segment a lie at [a * H, (a + 1) * H).  cb_vote_kernel is the hot path and has
// consensus_vote_kernel's body: the small segments of a stack, each a launch of a few hundred short workgroups on its own, fill
// the machine together.  Its counts are integers, so the result does not depend on the grid.  No kernel waits for another
// workgroup, no floating-point atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_consensus.hpp"
#include "k_estimate_batch.hpp"

namespace siftk {

#define SIFT_CB_MAX_TILES (1 << 20)
#define SIFT_CB_MAX_HYP (1 << 22)       // active segments x n_hyp: 24 + 4 + 1 bytes each in the matcher's buffers

// a tile of a segment (row0, rows: the tile's), or an active segment itself (row0, rows: the segment's)
struct CbWork {
    int seg;            // segment
    int act;            // its index among the active segments, -1: fewer than three pairs
    int row0, rows;     // first row of `pairs` / `mask` / `pts` and number of rows
    int off1, n1;       // first record and number of records of the segment's first list (shared list: 0, n1)
    int off2, n2;       // the same for the second list
};

// grid: tiles.  Row -> (x0, y0, x1, y1) with the segment's own bounds
__global__ __launch_bounds__(SIFT_CONS_THREADS) void cb_gather_kernel(const uint8_t *__restrict__ kp1, const uint8_t *__restrict__ kp2,
                                                                      const int2 *__restrict__ pairs, const CbWork *__restrict__ tiles,
                                                                      float4 *__restrict__ pts) {
    const CbWork w = tiles[blockIdx.x];
    const EbWork g = {w.seg, 0, 0, w.row0, w.rows, w.off1, w.n1, w.off2, w.n2, 0};      // eb_gather reads row0, the offsets and the counts
    for (int j = threadIdx.x; j < w.rows; j += SIFT_CONS_THREADS) pts[(size_t)w.row0 + j] = eb_gather(kp1, kp2, pairs, g, j);
}

// grid: (ceil(H / 256), active segments).  One lane per (segment, hypothesis); also clears its votes
__global__ __launch_bounds__(256) void cb_solve_kernel(const float4 *__restrict__ pts, const CbWork *__restrict__ segs, int H, uint32_t seed,
                                                       float *__restrict__ models, uint8_t *__restrict__ valid, int *__restrict__ votes) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    const CbWork w = segs[blockIdx.y];
    float out[6];
    const bool ok = consensus_solve(pts + (size_t)w.row0, (uint32_t)w.rows, h, seed, out);
    const size_t at = (size_t)w.act * H + h;
#pragma unroll
    for (int k = 0; k < 6; k++) models[at * 6 + k] = out[k];
    valid[at] = ok ? 1 : 0;
    votes[at] = 0;
}

// grid: (all tiles of all segments) x (chunks of h_chunk <= SIFT_CONS_HMAX hypotheses); consensus_vote_kernel on one tile of one
// segment, the segment's coefficients and counters through the tile's entry (the same for every lane: scalar loads).  A tile of a
// segment that is not active has nothing to vote on.
__global__ __launch_bounds__(SIFT_CONS_THREADS) void cb_vote_kernel(const float4 *__restrict__ pts, const CbWork *__restrict__ tiles,
                                                                    const float *__restrict__ models, int H, int h_chunk, float tol2,
                                                                    int *__restrict__ votes) {
    __shared__ int wave_count[SIFT_CONS_THREADS / 64][SIFT_CONS_HMAX];
    const int act = tiles[blockIdx.x].act;
    if (act < 0) return;
    const int row0 = tiles[blockIdx.x].row0, rows = tiles[blockIdx.x].rows;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int h0 = blockIdx.y * h_chunk, hn = min(h_chunk, H - h0);
    const float nan = __int_as_float(0x7fc00000);
    float4 p[SIFT_CONS_MPL];
#pragma unroll
    for (int k = 0; k < SIFT_CONS_MPL; k++) {
        const int j = k * SIFT_CONS_THREADS + tid;
        p[k] = j < rows ? pts[(size_t)row0 + j] : make_float4(nan, nan, nan, nan);
    }
    const size_t at = (size_t)act * H + h0;
    const float *__restrict__ coef = models + at * 6;
    for (int hh = 0; hh < hn; hh++) {
        const float a = coef[6 * hh], b = coef[6 * hh + 1], c = coef[6 * hh + 2];
        const float d = coef[6 * hh + 3], e = coef[6 * hh + 4], f = coef[6 * hh + 5];
        int n = 0;
#pragma unroll
        for (int k = 0; k < SIFT_CONS_MPL; k++) n += __popcll(__ballot(consensus_votes_for(a, b, c, d, e, f, p[k], tol2)));
        if (lane == 0) wave_count[wave][hh] = n;
    }
    __syncthreads();
    for (int hh = tid; hh < hn; hh += SIFT_CONS_THREADS) {
        int n = 0;
#pragma unroll
        for (int w = 0; w < SIFT_CONS_THREADS / 64; w++) n += wave_count[w][hh];
        if (n) atomicAdd(&votes[at + hh], n);
    }
}

// grid: active segments, one workgroup each
__global__ __launch_bounds__(256) void cb_select_kernel(const int *__restrict__ votes, const uint8_t *__restrict__ valid,
                                                        const float *__restrict__ models, int H, ConsensusResult *__restrict__ results) {
    const size_t at = (size_t)blockIdx.x * H;
    consensus_select(votes + at, valid + at, models + at * 6, H, results + blockIdx.x);
}

// grid: tiles, those of the segments that are not active included: every byte of the mask is written
__global__ __launch_bounds__(SIFT_CONS_THREADS) void cb_mask_kernel(const float4 *__restrict__ pts, const CbWork *__restrict__ tiles,
                                                                    const ConsensusResult *__restrict__ results, float tol2,
                                                                    uint8_t *__restrict__ mask) {
    const CbWork w = tiles[blockIdx.x];
    const ConsensusResult *r = w.act >= 0 ? results + w.act : nullptr;
    const bool any = r && r->winner >= 0;
    for (int j = threadIdx.x; j < w.rows; j += SIFT_CONS_THREADS) {
        bool in = false;
        if (any) {
            const float *m = r->model;
            in = consensus_votes_for(m[0], m[1], m[2], m[3], m[4], m[5], pts[(size_t)w.row0 + j], tol2);
        }
        mask[(size_t)w.row0 + j] = in ? 1 : 0;
    }
}

}  // namespace siftk
