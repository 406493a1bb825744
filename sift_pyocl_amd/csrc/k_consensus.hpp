// k_consensus.hpp -- consensus filter for matched keypoints: H affine hypotheses from random triples of matches, every
// match votes on every hypothesis, the hypothesis with most votes wins and its voters are the mask.
// No reference counterpart: the reference delegates this to the third-party feature.sift_orsa (sift-src/alignment.py:54-57).
//
// The arithmetic is a contract that tests/consensus_ref.py restates in numpy, so every result is compared for equality:
//   sample   i_k = mix(seed + 0x9E3779B9 * (3h + k + 1)) mod M, uint32 wrap-around, no rejection of repeats
//   solve    binary64, every product and sum rounded on its own in the order written (-ffp-contract=off), void iff
//            !(fabs(det) >= 1.0); the six coefficients are then rounded to f32
//   vote     f32, unfused: ex = ((a*x0 + b*y0) + c) - x1, ey likewise, vote iff ex*ex + ey*ey <= tol*tol
//   select   largest votes among the non-void hypotheses, ties to the smallest h
//
// consensus_vote_kernel is the hot path, f32 VALU bound: 14 lane-operations per (hypothesis, match).  A lane keeps
// SIFT_CONS_MPL matches in registers, the workgroup walks its share of the hypotheses, whose coefficients are the same for
// every lane (read through a uniform index: scalar loads); __ballot + popcount give a wave's count, the four waves leave
// theirs in LDS and the workgroup adds each non-zero sum to votes[h] once, at the end of its walk.  The counts are
// integers: the order of the additions is free.  The other kernels are plumbing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace siftk {

#define SIFT_CONS_THREADS 256
#define SIFT_CONS_MPL 4                                          // matches a lane keeps in registers
#define SIFT_CONS_TILE (SIFT_CONS_THREADS * SIFT_CONS_MPL)       // matches of a workgroup
#define SIFT_CONS_HMAX 512                                       // most hypotheses a workgroup walks (its LDS counters)

struct ConsensusResult { int winner, votes; float model[6]; };

__device__ __forceinline__ uint32_t consensus_mix(uint32_t v) {
    v ^= v >> 16; v *= 0x7FEB352Du; v ^= v >> 15; v *= 0x846CA68Bu; v ^= v >> 16;
    return v;
}

__device__ __forceinline__ bool consensus_votes_for(float a, float b, float c, float d, float e, float f, const float4 p, float tol2) {
    const float ex = ((a * p.x + b * p.y) + c) - p.z;
    const float ey = ((d * p.x + e * p.y) + f) - p.w;
    return ex * ex + ey * ey <= tol2;
}

// match j -> (x0, y0, x1, y1); a pair with an index outside its list becomes four NaN
__global__ __launch_bounds__(256) void consensus_gather_kernel(const uint8_t *__restrict__ kp1, int n1, const uint8_t *__restrict__ kp2, int n2,
                                                               const int2 *__restrict__ pairs, int M, float4 *__restrict__ pts) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    const int2 p = pairs[j];
    const float nan = __int_as_float(0x7fc00000);
    float4 v = make_float4(nan, nan, nan, nan);
    if (p.x >= 0 && p.x < n1 && p.y >= 0 && p.y < n2) {
        const float2 a = *reinterpret_cast<const float2 *>(kp1 + (size_t)p.x * 144);
        const float2 b = *reinterpret_cast<const float2 *>(kp2 + (size_t)p.y * 144);
        v = make_float4(a.x, a.y, b.x, b.y);
    }
    pts[j] = v;
}

// hypothesis h of the M matches at pts: the sample and the binary64 solve of the contract, in the order written.  out: the six
// coefficients as f32, all NaN when the triple is void; returns "not void".  Shared with k_consensus_batch.hpp
__device__ __forceinline__ bool consensus_solve(const float4 *__restrict__ pts, uint32_t M, int h, uint32_t seed, float out[6]) {
    const uint32_t base = 3u * (uint32_t)h;
    const float4 m0 = pts[consensus_mix(seed + 0x9E3779B9u * (base + 1u)) % M];
    const float4 m1 = pts[consensus_mix(seed + 0x9E3779B9u * (base + 2u)) % M];
    const float4 m2 = pts[consensus_mix(seed + 0x9E3779B9u * (base + 3u)) % M];
    const double x0 = m0.x, y0 = m0.y, x1 = m0.z, y1 = m0.w;
    const double ux = (double)m1.x - x0, uy = (double)m1.y - y0, vx = (double)m2.x - x0, vy = (double)m2.y - y0;
    const double det = ux * vy - vx * uy;
    const float nan = __int_as_float(0x7fc00000);
#pragma unroll
    for (int k = 0; k < 6; k++) out[k] = nan;
    const bool ok = fabs(det) >= 1.0;
    if (ok) {
        const double px = (double)m1.z - x1, qx = (double)m2.z - x1, py = (double)m1.w - y1, qy = (double)m2.w - y1;
        const double a = (px * vy - qx * uy) / det, b = (qx * ux - px * vx) / det;
        const double c = x1 - (a * x0 + b * y0);
        const double d = (py * vy - qy * uy) / det, e = (qy * ux - py * vx) / det;
        const double f = y1 - (d * x0 + e * y0);
        out[0] = (float)a; out[1] = (float)b; out[2] = (float)c; out[3] = (float)d; out[4] = (float)e; out[5] = (float)f;
    }
    return ok;
}

// one lane per hypothesis; also clears votes[h]
__global__ __launch_bounds__(256) void consensus_solve_kernel(const float4 *__restrict__ pts, uint32_t M, int H, uint32_t seed,
                                                              float *__restrict__ models, uint8_t *__restrict__ valid, int *__restrict__ votes) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= H) return;
    float out[6];
    const bool ok = consensus_solve(pts, M, h, seed, out);
#pragma unroll
    for (int k = 0; k < 6; k++) models[(size_t)h * 6 + k] = out[k];
    valid[h] = ok ? 1 : 0;
    votes[h] = 0;
}

// grid: (tiles of SIFT_CONS_TILE matches) x (chunks of h_chunk <= SIFT_CONS_HMAX hypotheses).  A void hypothesis is six NaN:
// every comparison is false, it collects nothing.  Lanes beyond M hold NaN as well.
__global__ __launch_bounds__(SIFT_CONS_THREADS) void consensus_vote_kernel(const float4 *__restrict__ pts, int M, const float *__restrict__ models,
                                                                           int H, int h_chunk, float tol2, int *__restrict__ votes) {
    __shared__ int wave_count[SIFT_CONS_THREADS / 64][SIFT_CONS_HMAX];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int h0 = blockIdx.y * h_chunk, hn = min(h_chunk, H - h0);
    const float nan = __int_as_float(0x7fc00000);
    float4 p[SIFT_CONS_MPL];
#pragma unroll
    for (int k = 0; k < SIFT_CONS_MPL; k++) {
        const int j = blockIdx.x * SIFT_CONS_TILE + k * SIFT_CONS_THREADS + tid;
        p[k] = j < M ? pts[j] : make_float4(nan, nan, nan, nan);
    }
    const float *__restrict__ coef = models + (size_t)h0 * 6;
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
        if (n) atomicAdd(&votes[h0 + hh], n);
    }
}

// one workgroup of 256 lanes: maximum of (votes << 32 | ~h) over the non-void hypotheses = most votes, smallest h among equals.
// Shared with k_consensus_batch.hpp
__device__ __forceinline__ void consensus_select(const int *__restrict__ votes, const uint8_t *__restrict__ valid,
                                                 const float *__restrict__ models, int H, ConsensusResult *__restrict__ result) {
    __shared__ unsigned long long best[256];
    unsigned long long key = 0;                                   // 0: nothing (a real key has ~h != 0 in its lower half)
    for (int h = threadIdx.x; h < H; h += 256)
        if (valid[h]) {
            const unsigned long long k = ((unsigned long long)(uint32_t)votes[h] << 32) | (uint32_t)~(uint32_t)h;
            key = k > key ? k : key;
        }
    best[threadIdx.x] = key;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { const unsigned long long o = best[threadIdx.x + s]; if (o > best[threadIdx.x]) best[threadIdx.x] = o; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        ConsensusResult r;
        r.winner = -1; r.votes = 0;
        for (int k = 0; k < 6; k++) r.model[k] = 0.f;
        if (best[0]) {
            r.winner = (int)~(uint32_t)(best[0] & 0xffffffffull);
            r.votes = (int)(best[0] >> 32);
            for (int k = 0; k < 6; k++) r.model[k] = models[(size_t)r.winner * 6 + k];
        }
        *result = r;
    }
}

__global__ __launch_bounds__(256) void consensus_select_kernel(const int *__restrict__ votes, const uint8_t *__restrict__ valid,
                                                               const float *__restrict__ models, int H, ConsensusResult *__restrict__ result) {
    consensus_select(votes, valid, models, H, result);
}

__global__ __launch_bounds__(256) void consensus_mask_kernel(const float4 *__restrict__ pts, int M, const ConsensusResult *__restrict__ result,
                                                             float tol2, uint8_t *__restrict__ mask) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= M) return;
    bool in = false;
    if (result->winner >= 0) {
        const float *m = result->model;
        in = consensus_votes_for(m[0], m[1], m[2], m[3], m[4], m[5], pts[j], tol2);
    }
    mask[j] = in ? 1 : 0;
}

}  // namespace siftk
