// k_shift.hpp -- exact median displacement of matched keypoints on the device: what
// LinearAlign._median_shift computes on the host with numpy.median, from the matches consensus_gather_kernel leaves in
// (x0, y0, x1, y1) form.  The reference's form is the host one (sift-src/alignment.py:268-271).
//
// A median has no rounding or ordering freedom, so the contract that tests/shift_ref.py restates in numpy pins all six results
// as bit patterns.  Everything is binary32, every operation rounded once (-ffp-contract=off), subnormals kept; the only atomics
// are integer adds, and no result depends on the grid, on scheduling or on what an earlier call left in the scratch:
//   used     pair j is used iff (mask == NULL || mask[j] != 0) and its four f32 coordinates are finite (fit_used of k_fit.hpp)
//   displ.   dx = x1 - x0, dy = y1 - y0; a difference that overflows to +-inf takes part like any other (a used pair never
//            gives a NaN: inf - inf needs a non-finite coordinate)
//   order    key(v) = bits(v) ^ (bits(v) >> 31 ? 0xffffffff : 0x80000000) as u32: ascending key is the total order of f32,
//            -inf first, -0.0 < +0.0
//   ranks    n used pairs: lo and hi are the values of rank (n - 1) >> 1 and n >> 1 in ascending key order, per axis
//   median   n odd (lo and hi are one element): lo; n even: (lo + hi) * 0.5f -- numpy.median's mean of the middle element(s).
//            (The odd case is not written (lo + lo) * 0.5f: that overflows for |lo| > FLT_MAX / 2, numpy's mean of one does not.)
//   n == 0   EMPTY: the six results are NaN, the counts 0; every kernel after the count returns at once
//   keep     keep[j] = used(j) && isfinite(mdx) && isfinite(mdy) && fabsf(dx - mdx) <= tol && fabsf(dy - mdy) <= tol; tol may
//            be +inf; n_keep counts the kept pairs
//
// Launch structure: a radix select, four digits of 8 bits from the top, for four selectors s = 2 * axis + (0: lo, 1: hi) at
// once.  A selector's state is the key prefix fixed so far and its rank among the keys with that prefix.
//   shift_key_kernel     the keys of every pair ((~0, ~0) for an unused one: no used displacement has the key ~0, a NaN's), n,
//                        and the histogram of the first digit
//   shift_pass_kernel    p = 1, 2, 3: every workgroup redoes the 256-bin scan that fixes digit p - 1 from the histogram of the
//                        launch before (as fit_pass2/3 redo their step (iii)); workgroup 0 records the state; then the
//                        histogram of digit p over the keys that carry a selector's prefix, 4 x 256 LDS counters per workgroup
//                        flushed by integer atomicAdd
//   shift_finish_kernel  the last scan, keys back to floats, the six results
//   shift_keep_kernel    only when a keep mask is asked for
// ShiftScratch is cleared on the stream by every call.  The work is M x 8 bytes read four times: launch latency, not a hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_fit.hpp"

namespace siftk {

#define SIFT_SHIFT_THREADS 256
#define SIFT_SHIFT_UNUSED 0xffffffffu
// the six results, in the order of siftmi_match_shift's `out`
#define SIFT_SHIFT_MDX 0
#define SIFT_SHIFT_MDY 1
#define SIFT_SHIFT_RANKS 2      // lo_dx, hi_dx, lo_dy, hi_dy: selector s at SIFT_SHIFT_RANKS + s
#define SIFT_SHIFT_OUT 6

// scratch of one call; all zero when the first kernel starts
struct ShiftScratch {
    unsigned int hist[4][4][256];       // [digit, most significant first][selector][value of the digit]
    unsigned int prefix[4][4];          // [p][selector]: the p digits fixed before pass p (row 0 is unused)
    unsigned int rank[4][4];            //                and the selector's rank among the keys that carry them
    unsigned int n, n_keep;
    float out[SIFT_SHIFT_OUT];
};

__device__ __forceinline__ uint32_t shift_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float shift_unkey(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// The state before pass p (1..4; 4: all digits fixed) in st_prefix / st_rank[0..3], valid after the barrier: the state before
// pass p - 1 (from n for p == 1, recorded by workgroup 0 of the launch before otherwise) advanced by a scan of digit p - 1's
// histogram.  Lane s < 4 walks selector s's 256 bins: the digit is the first bin whose running count exceeds the rank.
__device__ __forceinline__ void shift_advance(const ShiftScratch *sc, int p, unsigned int n, unsigned int (*bins)[256],
                                              unsigned int *st_prefix, unsigned int *st_rank, int t) {
    for (int s = 0; s < 4; s++) bins[s][t] = sc->hist[p - 1][s][t];
    __syncthreads();
    if (t < 4) {
        unsigned int prefix = 0, r = (t & 1) ? n >> 1 : (n - 1) >> 1;
        if (p > 1) { prefix = sc->prefix[p - 1][t]; r = sc->rank[p - 1][t]; }
        unsigned int digit = 255;
        for (unsigned int d = 0; d < 256; d++) {
            const unsigned int c = bins[t][d];
            if (r < c) { digit = d; break; }
            r -= c;
        }
        st_prefix[t] = (prefix << 8) | digit;
        st_rank[t] = r;
    }
    __syncthreads();
}

// adds the workgroup's 4 x 256 counters to digit p's histogram; bins must be complete (barrier before)
__device__ __forceinline__ void shift_flush(ShiftScratch *sc, int p, unsigned int (*bins)[256], int t) {
    for (int s = 0; s < 4; s++) {
        const unsigned int c = bins[s][t];
        if (c) atomicAdd(&sc->hist[p][s][t], c);
    }
}

__global__ __launch_bounds__(SIFT_SHIFT_THREADS) void shift_key_kernel(const float4 *__restrict__ pts, const uint8_t *__restrict__ mask, int M,
                                                                       uint2 *__restrict__ keys, ShiftScratch *__restrict__ sc) {
    __shared__ unsigned int bins[4][256];
    __shared__ unsigned int used;
    const int t = threadIdx.x;
    for (int s = 0; s < 4; s++) bins[s][t] = 0;
    if (t == 0) used = 0;
    __syncthreads();
    const long long G = (long long)gridDim.x * SIFT_SHIFT_THREADS;
    unsigned int mine = 0;
    for (long long j = (long long)blockIdx.x * SIFT_SHIFT_THREADS + t; j < M; j += G) {
        const float4 p = pts[j];
        uint2 k = make_uint2(SIFT_SHIFT_UNUSED, SIFT_SHIFT_UNUSED);
        if (fit_used(p, mask, j)) {
            k = make_uint2(shift_key(p.z - p.x), shift_key(p.w - p.y));
            mine++;
            atomicAdd(&bins[0][k.x >> 24], 1u); atomicAdd(&bins[1][k.x >> 24], 1u);      // lo and hi share the first digit's counts
            atomicAdd(&bins[2][k.y >> 24], 1u); atomicAdd(&bins[3][k.y >> 24], 1u);
        }
        keys[j] = k;
    }
    if (mine) atomicAdd(&used, mine);
    __syncthreads();
    shift_flush(sc, 0, bins, t);
    if (t == 0 && used) atomicAdd(&sc->n, used);
}

// p = 1, 2, 3: fixes digit p - 1 and counts digit p
__global__ __launch_bounds__(SIFT_SHIFT_THREADS) void shift_pass_kernel(const uint2 *__restrict__ keys, int M, int p, ShiftScratch *__restrict__ sc) {
    __shared__ unsigned int bins[4][256];
    __shared__ unsigned int st_prefix[4], st_rank[4];
    const int t = threadIdx.x;
    const unsigned int n = sc->n;
    if (n == 0) return;                                      // EMPTY
    shift_advance(sc, p, n, bins, st_prefix, st_rank, t);
    const unsigned int pre0 = st_prefix[0], pre1 = st_prefix[1], pre2 = st_prefix[2], pre3 = st_prefix[3];
    if (blockIdx.x == 0 && t < 4) { sc->prefix[p][t] = st_prefix[t]; sc->rank[p][t] = st_rank[t]; }
    __syncthreads();                                         // the scan's reads of bins are over
    for (int s = 0; s < 4; s++) bins[s][t] = 0;
    __syncthreads();
    const int low = 24 - 8 * p, high = low + 8;              // the digit's bits and the prefix above them
    const long long G = (long long)gridDim.x * SIFT_SHIFT_THREADS;
    for (long long j = (long long)blockIdx.x * SIFT_SHIFT_THREADS + t; j < M; j += G) {
        const uint2 k = keys[j];
        if (k.x == SIFT_SHIFT_UNUSED) continue;             // no used pair has this key on either axis
        const unsigned int dx = (k.x >> low) & 255u, dy = (k.y >> low) & 255u;
        if ((k.x >> high) == pre0) atomicAdd(&bins[0][dx], 1u);
        if ((k.x >> high) == pre1) atomicAdd(&bins[1][dx], 1u);
        if ((k.y >> high) == pre2) atomicAdd(&bins[2][dy], 1u);
        if ((k.y >> high) == pre3) atomicAdd(&bins[3][dy], 1u);
    }
    __syncthreads();
    shift_flush(sc, p, bins, t);
}

// one workgroup: the last digit, the keys back to floats, the medians
__global__ __launch_bounds__(SIFT_SHIFT_THREADS) void shift_finish_kernel(ShiftScratch *__restrict__ sc) {
    __shared__ unsigned int bins[4][256];
    __shared__ unsigned int st_prefix[4], st_rank[4];
    const int t = threadIdx.x;
    const unsigned int n = sc->n;
    if (n == 0) {                                            // EMPTY
        if (t < SIFT_SHIFT_OUT) sc->out[t] = __uint_as_float(0x7fc00000u);
        return;
    }
    shift_advance(sc, 4, n, bins, st_prefix, st_rank, t);
    if (t < 4) sc->out[SIFT_SHIFT_RANKS + t] = shift_unkey(st_prefix[t]);
    if (t < 2) {                                             // lane 0: x, lane 1: y
        const float lo = shift_unkey(st_prefix[2 * t]), hi = shift_unkey(st_prefix[2 * t + 1]);
        sc->out[SIFT_SHIFT_MDX + t] = (n & 1u) ? lo : (lo + hi) * 0.5f;
    }
}

__global__ __launch_bounds__(SIFT_SHIFT_THREADS) void shift_keep_kernel(const uint2 *__restrict__ keys, int M, float tol,
                                                                        uint8_t *__restrict__ keep, ShiftScratch *__restrict__ sc) {
    __shared__ unsigned int kept;
    const int t = threadIdx.x;
    if (t == 0) kept = 0;
    __syncthreads();
    const float mdx = sc->out[SIFT_SHIFT_MDX], mdy = sc->out[SIFT_SHIFT_MDY];
    const bool any = isfinite(mdx) && isfinite(mdy);         // a non-finite median keeps nothing (EMPTY included)
    const long long G = (long long)gridDim.x * SIFT_SHIFT_THREADS;
    unsigned int mine = 0;
    for (long long j = (long long)blockIdx.x * SIFT_SHIFT_THREADS + t; j < M; j += G) {
        const uint2 k = keys[j];
        bool ok = false;
        if (any && k.x != SIFT_SHIFT_UNUSED) {
            const float dx = shift_unkey(k.x), dy = shift_unkey(k.y);
            ok = fabsf(dx - mdx) <= tol && fabsf(dy - mdy) <= tol;
        }
        keep[j] = ok ? 1 : 0;
        mine += ok;
    }
    if (mine) atomicAdd(&kept, mine);
    __syncthreads();
    if (t == 0 && kept) atomicAdd(&sc->n_keep, kept);
}

}  // namespace siftk
