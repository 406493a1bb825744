// k_top_patch.hpp -- the top blur plane (plane 5) computed only where detection reads it.
//
// Plane 5 has two readers: the extrema pass, as the outer layer DoG4 = p4 - p5 of scale 3's 27-neighbour test, and the
// refinement of a scale-3 candidate (its N layer).  With the lazy extrema instance (k_extrema.hpp: LAZY) the full-plane
// blur that writes plane 5 is not run: scale 3 is tested against 18 neighbours, and this kernel finishes the test for the
// provisional scale-3 entries of the candidate list -- one wave per entry evaluates plane 5 on the 13 x 13 patch centred on
// the candidate, writes it into the real plane at its true position, and turns the entry into a hole when DoG4's 3 x 3
// around it holds a sample beyond the centre.
//
// Why 13 x 13: refine_candidates makes at most 5 moves of +-1 per axis from the candidate and reads the N layer at the
// current centre +-1, i.e. within Chebyshev distance 6 of the candidate.  Its reads of plane 5 never leave the patch.
//
// Arithmetic is that of the blur kernels (k_pyramid.hpp), so a patch sample holds the bits the full-plane launch would
// have written there (overlapping patches write identical bits): H pass first, h = sum_q p4[y'][reflect(x - C + q)] *
// taps[N - 1 - q], then the V pass over h; every sum starts from 0.0f, q ascending, unfused multiply then add.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_pyramid.hpp"

namespace siftk {

#define SIFT_TOP_R 6                       // patch radius (see above)
#define SIFT_TOP_P (2 * SIFT_TOP_R + 1)    // patch side: 13
struct TopTaps { float t[64]; };

// floats of dynamic LDS: input window, H results, reversed taps, the patch
inline size_t top_patch_lds_bytes(int n_taps) {
    const size_t win = (size_t)(SIFT_TOP_P - 1 + n_taps);
    return (win * win + win * SIFT_TOP_P + 64 + SIFT_TOP_P * SIFT_TOP_P) * sizeof(float);
}

// One wave per workgroup; workgroup b takes list entries b, b + gridDim.x, ... of the first min(*n_cand, capacity).
// An entry that is not a scale-3 candidate (or is a hole) is skipped: the wave's branch on it is uniform.
__global__ __launch_bounds__(64) void top_patch_kernel(const float *__restrict__ p4, float *__restrict__ p5, int W, int H, TopTaps taps, int n_taps,
                                                       float4 *__restrict__ cand, const int *__restrict__ n_cand, int cand_capacity) {
    extern __shared__ float top_lds[];
    const int lane = threadIdx.x;
    const int C = (n_taps & 1) ? n_taps / 2 : n_taps / 2 - 1;      // BlurGeom::C
    const int WIN = SIFT_TOP_P - 1 + n_taps;                        // rows and columns of p4 the patch depends on (39 for 27 taps)
    float *win = top_lds;                                           // [WIN][WIN]   p4, border rule applied
    float *hb = win + WIN * WIN;                                    // [WIN][13]    H pass
    float *tr = hb + WIN * SIFT_TOP_P;                              // [64]         tr[q] = taps[N - 1 - q]
    float *pt = tr + 64;                                            // [13][13]     the patch of plane 5
    if (lane < n_taps) tr[lane] = taps.t[n_taps - 1 - lane];
    const int n = min(*n_cand, cand_capacity);
    for (int i = blockIdx.x; i < n; i += gridDim.x) {
        const float4 k = cand[i];
        const int r = __builtin_amdgcn_readfirstlane((int)k.y), c = __builtin_amdgcn_readfirstlane((int)k.z);
        if (__builtin_amdgcn_readfirstlane((int)k.w) != 3 || r == -1) continue;
        __syncthreads();                                            // the previous entry's outer test has read `win` and `pt`
        const int y0 = r - SIFT_TOP_R, x0 = c - SIFT_TOP_R;         // patch origin; window origin is (y0 - C, x0 - C)
        // window: a lane per column (no division), the rows' loads independent of one another
        for (int wc = lane; wc < WIN; wc += 64) {
            const float *col = p4 + reflect_index(x0 - C + wc, W);
#pragma unroll 8
            for (int wr = 0; wr < WIN; wr++) win[wr * WIN + wc] = col[(size_t)reflect_index(y0 - C + wr, H) * W];
        }
        __syncthreads();
        // H pass: output (window row wr, patch column cx) = idx; a lane owns idx = lane + 64 j and advances its outputs
        // together, tap by tap (each output still receives its products in q-ascending order from 0.0f)
        for (int base = 0; base < WIN * SIFT_TOP_P; base += 64 * 4) {
            const float *src[4];
            float a[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int idx = min(base + 64 * j + lane, WIN * SIFT_TOP_P - 1);
                const int wr = idx / SIFT_TOP_P;
                src[j] = win + wr * WIN + (idx - wr * SIFT_TOP_P);
                a[j] = 0.0f;
            }
            for (int q = 0; q < n_taps; q++) {
                const float t = tr[q];
#pragma unroll
                for (int j = 0; j < 4; j++) a[j] = a[j] + src[j][q] * t;
            }
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int idx = base + 64 * j + lane;
                if (idx < WIN * SIFT_TOP_P) hb[idx] = a[j];
            }
        }
        __syncthreads();
        // V pass: patch sample (py, px) = idx reads window rows py .. py + N - 1 of column px
        {
            const float *src[3];
            float a[3];
#pragma unroll
            for (int j = 0; j < 3; j++) { src[j] = hb + min(64 * j + lane, SIFT_TOP_P * SIFT_TOP_P - 1); a[j] = 0.0f; }
            for (int q = 0; q < n_taps; q++) {
                const float t = tr[q];
#pragma unroll
                for (int j = 0; j < 3; j++) a[j] = a[j] + src[j][q * SIFT_TOP_P] * t;
            }
#pragma unroll
            for (int j = 0; j < 3; j++) {
                const int idx = 64 * j + lane;
                if (idx < SIFT_TOP_P * SIFT_TOP_P) {
                    pt[idx] = a[j];
                    const int py = idx / SIFT_TOP_P, y = y0 + py, x = x0 + idx - py * SIFT_TOP_P;
                    if (y >= 0 && y < H && x >= 0 && x < W) p5[(size_t)y * W + x] = a[j];     // the patch clipped to the plane
                }
            }
        }
        __syncthreads();
        // Outer layer of the 27-neighbour test on the centre 3 x 3 (the candidate lies at least one pixel inside the plane):
        // a positive centre is rejected iff a DoG4 sample is strictly greater, a negative one iff a sample is strictly smaller --
        // val >= M27 / val <= m27 of extrema_strip under fmaxf's NaN rule (a NaN sample never rejects).
        bool beyond = false;
        if (lane < 9) {
            const int dy = lane / 3 - 1, dx = lane - (lane / 3) * 3 - 1;
            const float d4 = win[(SIFT_TOP_R + C + dy) * WIN + SIFT_TOP_R + C + dx] - pt[(SIFT_TOP_R + dy) * SIFT_TOP_P + SIFT_TOP_R + dx];
            beyond = (k.x > 0.0f) ? (d4 > k.x) : (d4 < k.x);
        }
        if (__ballot(beyond) && lane == 0) cand[i] = make_float4(-1.0f, -1.0f, -1.0f, -1.0f);   // a hole: refine_candidates skips it before it counts
    }
}

}  // namespace siftk
