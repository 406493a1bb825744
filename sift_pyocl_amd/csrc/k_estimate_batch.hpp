// k_estimate_batch.hpp -- the least-squares fit (k_fit.hpp) and the median displacement (k_shift.hpp) of S segments of pairs in one
// set of launches: what siftmi_match_batch leaves behind -- record lists back to back, pairs with
// indices local to their segment, pair_counts -- goes in unchanged.  The result of segment s is, bit for bit, what
// siftmi_match_fit / siftmi_match_shift give on that segment alone; tests/estimate_batch_ref.py restates it by slicing.
//
//   gather   row r of segment s with local (i, j) reads kp1[off1 + i] iff 0 <= i < n1_s and kp2[off2 + j] iff 0 <= j < n2_s, else it
//            is four NaN: an index that leaves the segment's list names a neighbour's record and is never read
//   fit      the four kernels of k_fit.hpp on a 1-D grid over a host-built table (EbWork, one entry per workgroup): segment s has
//            B_s workgroups, G_s = 256 B_s, pair j (its position inside the segment) on lane j mod G_s; steps (i), (ii), (iii) as
//            there, the partials of workgroup b of a segment at slot0 + b, step (iii) redone by every workgroup of the segment at
//            the head of the next launch.  The gather is fused into pass 1, which leaves the positions in `pts` for passes 2 and 3.
//            The finish kernel takes one lane per segment.  No kernel waits for another workgroup, no floating-point atomic.
//   shift    one kernel, one 256-lane workgroup per non-empty segment, the four selectors' state and counters in LDS: gather, keys
//            ((~0, ~0) for an unused row) + n + the first digit's histogram, then per digit the scan that fixes it and the
//            histogram of the next over the keys that carry a selector's prefix, the six results, and with `keep` one more pass.
//            Only barriers separate the steps; integer LDS atomics only, so the result cannot depend on scheduling.  A median is
//            exact, so it cannot depend on the launch shape either.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "k_fit.hpp"
#include "k_shift.hpp"

namespace siftk {

#define SIFT_EB_MAX_SEGMENTS 65535
#define SIFT_EB_MAX_WORK (1 << 20)

// one workgroup's share of a segment (fit), or the segment itself (b = 0: the shift's table and the finish kernel's)
struct EbWork {
    int seg;            // segment
    int b, B;           // workgroup of the segment, workgroups of the segment (0: a segment without a pair, finish table only)
    int row0, rows;     // the segment's first row of `pairs` / `mask` / `pts` and its number of rows
    int off1, n1;       // first record and number of records of the segment's first list (shared list: 0, n1)
    int off2, n2;       // the same for the second list
    int slot0;          // first partial slot of the segment
};

// the partials of all workgroups and the results of all segments (fit): one allocation, the pointers into it
struct EbFitScratch {
    double *p1;                     // [slots][4]
    double *p2;                     // [slots][7]
    double *p3;                     // [slots]
    unsigned long long *count;      // [slots]
    double *out;                    // [S][SIFT_FIT_OUT]
};

__device__ __forceinline__ float4 eb_gather(const uint8_t *__restrict__ kp1, const uint8_t *__restrict__ kp2, const int2 *__restrict__ pairs,
                                            const EbWork &w, int j) {
    const int2 p = pairs[(size_t)w.row0 + j];
    const float nan = __int_as_float(0x7fc00000);
    float4 v = make_float4(nan, nan, nan, nan);
    if (p.x >= 0 && p.x < w.n1 && p.y >= 0 && p.y < w.n2) {
        const float2 a = *reinterpret_cast<const float2 *>(kp1 + ((size_t)w.off1 + p.x) * 144);
        const float2 b = *reinterpret_cast<const float2 *>(kp2 + ((size_t)w.off2 + p.y) * 144);
        v = make_float4(a.x, a.y, b.x, b.y);
    }
    return v;
}

// ---------------------------------------------------------------------------------------------------------------- fit
// fit_pass1_kernel on workgroup w.b of segment w.seg, with the gather in front
__global__ __launch_bounds__(SIFT_FIT_THREADS) void eb_fit_pass1_kernel(const uint8_t *__restrict__ kp1, const uint8_t *__restrict__ kp2,
                                                                        const int2 *__restrict__ pairs, const uint8_t *__restrict__ mask,
                                                                        const EbWork *__restrict__ work, float4 *__restrict__ pts, EbFitScratch fs) {
    __shared__ double v[4][SIFT_FIT_THREADS];
    __shared__ unsigned int cnt[SIFT_FIT_THREADS];
    const EbWork w = work[blockIdx.x];
    const int t = threadIdx.x;
    const long long G = (long long)w.B * SIFT_FIT_THREADS;
    double sx = 0.0, sy = 0.0, su = 0.0, sv = 0.0;
    unsigned int n = 0;
    for (long long j = (long long)w.b * SIFT_FIT_THREADS + t; j < w.rows; j += G) {
        const float4 p = eb_gather(kp1, kp2, pairs, w, (int)j);
        pts[(size_t)w.row0 + j] = p;
        if (fit_used(p, mask, w.row0 + j)) {
            sx = sx + (double)p.x; sy = sy + (double)p.y; su = su + (double)p.z; sv = sv + (double)p.w;
            n++;
        }
    }
    v[0][t] = sx; v[1][t] = sy; v[2][t] = su; v[3][t] = sv;
    cnt[t] = n;
    fit_tree<4>(v, t);
    if (t == 0) {
        unsigned long long total = 0;                       // integers: the order is free
        for (int k = 0; k < SIFT_FIT_THREADS; k++) total += cnt[k];
        const size_t slot = (size_t)w.slot0 + w.b;
        fs.count[slot] = total;
#pragma unroll
        for (int k = 0; k < 4; k++) fs.p1[slot * 4 + k] = v[k][0];
    }
}

// fit_pass2_kernel: n and the means of the segment from its B partials (every workgroup of the segment), the centred moments
__global__ __launch_bounds__(SIFT_FIT_THREADS) void eb_fit_pass2_kernel(const float4 *__restrict__ pts, const uint8_t *__restrict__ mask,
                                                                        const EbWork *__restrict__ work, EbFitScratch fs) {
    __shared__ double v[7][SIFT_FIT_THREADS];
    __shared__ double sums[4];
    __shared__ unsigned long long n_all;
    const EbWork w = work[blockIdx.x];
    const int t = threadIdx.x, B = w.B;
    double *out = fs.out + (size_t)w.seg * SIFT_FIT_OUT;
    if (t == 4) {
        unsigned long long total = 0;
        for (int b = 0; b < B; b++) total += fs.count[(size_t)w.slot0 + b];
        n_all = total;
    }
    fit_serial<4>(fs.p1 + (size_t)w.slot0 * 4, B, sums, t);
    const unsigned long long n = n_all;
    if (n == 0) {                                           // EMPTY: status and n, everything else NaN; nothing further runs
        if (w.b == 0 && t < SIFT_FIT_OUT) out[t] = t == SIFT_FIT_STATUS ? 1.0 : t == SIFT_FIT_N ? 0.0 : fit_nan();
        return;
    }
    const double nd = (double)n;
    const double mx = sums[0] / nd, my = sums[1] / nd, mu = sums[2] / nd, mv = sums[3] / nd;
    if (w.b == 0 && t == 0) {
        out[SIFT_FIT_N] = nd;
        out[SIFT_FIT_MEANS] = mx; out[SIFT_FIT_MEANS + 1] = my; out[SIFT_FIT_MEANS + 2] = mu; out[SIFT_FIT_MEANS + 3] = mv;
    }
    const long long G = (long long)B * SIFT_FIT_THREADS;
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long j = (long long)w.b * SIFT_FIT_THREADS + t; j < w.rows; j += G) {
        const float4 p = pts[(size_t)w.row0 + j];
        if (fit_used(p, mask, w.row0 + j)) {
            const double X = (double)p.x - mx, Y = (double)p.y - my, U = (double)p.z - mu, V = (double)p.w - mv;
            s[0] = s[0] + X * X; s[1] = s[1] + X * Y; s[2] = s[2] + Y * Y;
            s[3] = s[3] + X * U; s[4] = s[4] + Y * U; s[5] = s[5] + X * V; s[6] = s[6] + Y * V;
        }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) v[k][t] = s[k];
    fit_tree<7>(v, t);
    if (t < 7) fs.p2[((size_t)w.slot0 + w.b) * 7 + t] = v[t][0];
}

// fit_pass3_kernel: the moments of the segment and the solve (every workgroup of the segment), the squared residuals
__global__ __launch_bounds__(SIFT_FIT_THREADS) void eb_fit_pass3_kernel(const float4 *__restrict__ pts, const uint8_t *__restrict__ mask,
                                                                        const EbWork *__restrict__ work, EbFitScratch fs) {
    __shared__ double v[1][SIFT_FIT_THREADS];
    __shared__ double S[7];
    const EbWork w = work[blockIdx.x];
    const int t = threadIdx.x, B = w.B;
    double *out = fs.out + (size_t)w.seg * SIFT_FIT_OUT;
    const double nd = out[SIFT_FIT_N];                      // written by workgroup 0 of the segment in the launch before this one
    if (!(nd > 0.0)) return;                                // EMPTY
    fit_serial<7>(fs.p2 + (size_t)w.slot0 * 7, B, S, t);
    const double mx = out[SIFT_FIT_MEANS], my = out[SIFT_FIT_MEANS + 1], mu = out[SIFT_FIT_MEANS + 2], mv = out[SIFT_FIT_MEANS + 3];
    const double Sxx = S[0], Sxy = S[1], Syy = S[2], Sxu = S[3], Syu = S[4], Sxv = S[5], Syv = S[6];
    const double scale = Sxx * Syy;
    const double det = scale - Sxy * Sxy;
    const bool degenerate = nd < 3.0 || !(fabs(det) > 1e-12 * fmax(1.0, scale));
    double a = fit_nan(), b = fit_nan(), c = fit_nan(), d = fit_nan(), e = fit_nan(), f = fit_nan();
    if (!degenerate) {
        a = (Sxu * Syy - Syu * Sxy) / det; b = (Syu * Sxx - Sxu * Sxy) / det;
        c = mu - (a * mx + b * my);
        d = (Sxv * Syy - Syv * Sxy) / det; e = (Syv * Sxx - Sxv * Sxy) / det;
        f = mv - (d * mx + e * my);
    }
    if (w.b == 0 && t == 0) {
        out[SIFT_FIT_STATUS] = degenerate ? 2.0 : 0.0;
        for (int k = 0; k < 7; k++) out[SIFT_FIT_MOMENTS + k] = S[k];
        out[SIFT_FIT_MODEL] = a; out[SIFT_FIT_MODEL + 1] = b; out[SIFT_FIT_MODEL + 2] = c;
        out[SIFT_FIT_MODEL + 3] = d; out[SIFT_FIT_MODEL + 4] = e; out[SIFT_FIT_MODEL + 5] = f;
        out[SIFT_FIT_SSR] = fit_nan();                      // eb_fit_finish_kernel replaces it when the status is OK
    }
    if (degenerate) return;
    const long long G = (long long)B * SIFT_FIT_THREADS;
    double r = 0.0;
    for (long long j = (long long)w.b * SIFT_FIT_THREADS + t; j < w.rows; j += G) {
        const float4 p = pts[(size_t)w.row0 + j];
        if (fit_used(p, mask, w.row0 + j)) {
            const double x0 = p.x, y0 = p.y, x1 = p.z, y1 = p.w;
            const double ex = ((a * x0 + b * y0) + c) - x1, ey = ((d * x0 + e * y0) + f) - y1;
            r = r + (ex * ex + ey * ey);
        }
    }
    v[0][t] = r;
    fit_tree<1>(v, t);
    if (t == 0) fs.p3[(size_t)w.slot0 + w.b] = v[0][0];
}

// one lane per segment: step (iii) of pass 3.  `segs` has one entry per segment (B == 0: no pair, the host writes its row)
__global__ __launch_bounds__(256) void eb_fit_finish_kernel(const EbWork *__restrict__ segs, int S, EbFitScratch fs) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= S) return;
    const EbWork w = segs[s];
    if (w.B == 0) return;
    double *out = fs.out + (size_t)s * SIFT_FIT_OUT;
    if (out[SIFT_FIT_STATUS] != 0.0) return;                // EMPTY or DEGENERATE: ssr stays NaN
    double acc = 0.0;
    for (int b = 0; b < w.B; b++) acc = acc + fs.p3[(size_t)w.slot0 + b];
    out[SIFT_FIT_SSR] = acc;
}

// ---------------------------------------------------------------------------------------------------------------- shift
// The whole select of segment segs[blockIdx.x] (a segment with at least one row).  out: [S][6] floats, counts: [S][2] (n, n_keep),
// keys / keep: one entry per row of `pairs`; keep may be null.  The scan of a digit takes the workgroup as four waves of 64 lanes.
static_assert(SIFT_SHIFT_THREADS == 256, "eb_shift_kernel: one wave of 64 lanes per selector, four bins per lane");
__global__ __launch_bounds__(SIFT_SHIFT_THREADS) void eb_shift_kernel(const uint8_t *__restrict__ kp1, const uint8_t *__restrict__ kp2,
                                                                      const int2 *__restrict__ pairs, const uint8_t *__restrict__ mask,
                                                                      const EbWork *__restrict__ segs, uint2 *__restrict__ keys, float tol,
                                                                      uint8_t *__restrict__ keep, float *__restrict__ out_all,
                                                                      long long *__restrict__ counts_all) {
    __shared__ unsigned int bins[4][256];
    __shared__ unsigned int st_prefix[4], st_rank[4];
    __shared__ unsigned int used, kept;
    const EbWork w = segs[blockIdx.x];
    const int t = threadIdx.x;
    float *out = out_all + (size_t)w.seg * SIFT_SHIFT_OUT;
    long long *counts = counts_all + (size_t)w.seg * 2;
    uint2 *seg_keys = keys + (size_t)w.row0;
    for (int s = 0; s < 4; s++) bins[s][t] = 0;
    if (t == 0) { used = 0; kept = 0; }
    __syncthreads();
    // the keys, n and the first digit's histogram (shift_key_kernel)
    unsigned int mine = 0;
    for (int j = t; j < w.rows; j += SIFT_SHIFT_THREADS) {
        const float4 p = eb_gather(kp1, kp2, pairs, w, j);
        uint2 k = make_uint2(SIFT_SHIFT_UNUSED, SIFT_SHIFT_UNUSED);
        if (fit_used(p, mask, (long long)w.row0 + j)) {
            k = make_uint2(shift_key(p.z - p.x), shift_key(p.w - p.y));
            mine++;
            atomicAdd(&bins[0][k.x >> 24], 1u); atomicAdd(&bins[1][k.x >> 24], 1u);      // lo and hi share the first digit's counts
            atomicAdd(&bins[2][k.y >> 24], 1u); atomicAdd(&bins[3][k.y >> 24], 1u);
        }
        seg_keys[j] = k;
    }
    if (mine) atomicAdd(&used, mine);
    __syncthreads();
    const unsigned int n = used;
    if (n == 0) {                                            // EMPTY
        if (t < SIFT_SHIFT_OUT) out[t] = __uint_as_float(0x7fc00000u);
        if (t < 2) counts[t] = 0;
        if (keep) for (int j = t; j < w.rows; j += SIFT_SHIFT_THREADS) keep[(size_t)w.row0 + j] = 0;
        return;
    }
    if (t < 4) { st_prefix[t] = 0; st_rank[t] = (t & 1) ? n >> 1 : (n - 1) >> 1; }
    __syncthreads();
    for (int p = 1; p <= 4; p++) {
        // fixes digit p - 1 (shift_advance's answer): the digit is the first bin whose running count exceeds the rank.  Wave s scans
        // selector s: lane l owns bins 4 l .. 4 l + 3, an inclusive scan of the lanes' sums over the wave, and the one lane whose
        // range of running counts holds the rank (the ranges tile [0, the selector's keys), and the rank is below that) records it
        {
            const int s = t >> 6, l = t & 63;
            const unsigned int c0 = bins[s][4 * l], c1 = bins[s][4 * l + 1], c2 = bins[s][4 * l + 2], c3 = bins[s][4 * l + 3];
            const unsigned int sum = c0 + c1 + c2 + c3;
            unsigned int incl = sum;
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned int up = __shfl_up(incl, d, 64);
                if (l >= d) incl += up;
            }
            const unsigned int r = st_rank[s], prefix = st_prefix[s], excl = incl - sum;
            __syncthreads();                                 // every lane has the state before one of them replaces it
            if (r >= excl && r < incl) {
                unsigned int rr = r - excl, digit = 4u * l;
                if (rr >= c0) { rr -= c0; digit++; if (rr >= c1) { rr -= c1; digit++; if (rr >= c2) { rr -= c2; digit++; } } }
                st_prefix[s] = (prefix << 8) | digit;
                st_rank[s] = rr;
            }
        }
        __syncthreads();
        if (p == 4) break;
        const unsigned int pre0 = st_prefix[0], pre1 = st_prefix[1], pre2 = st_prefix[2], pre3 = st_prefix[3];
        for (int s = 0; s < 4; s++) bins[s][t] = 0;
        __syncthreads();
        // the histogram of digit p over the keys that carry a selector's prefix (shift_pass_kernel)
        const int low = 24 - 8 * p, high = low + 8;
        for (int j = t; j < w.rows; j += SIFT_SHIFT_THREADS) {
            const uint2 k = seg_keys[j];                     // this lane's own store
            if (k.x == SIFT_SHIFT_UNUSED) continue;          // no used pair has this key on either axis
            const unsigned int dx = (k.x >> low) & 255u, dy = (k.y >> low) & 255u;
            if ((k.x >> high) == pre0) atomicAdd(&bins[0][dx], 1u);
            if ((k.x >> high) == pre1) atomicAdd(&bins[1][dx], 1u);
            if ((k.y >> high) == pre2) atomicAdd(&bins[2][dy], 1u);
            if ((k.y >> high) == pre3) atomicAdd(&bins[3][dy], 1u);
        }
        __syncthreads();
    }
    // the keys back to floats, the medians (shift_finish_kernel)
    const float lo_x = shift_unkey(st_prefix[0]), hi_x = shift_unkey(st_prefix[1]);
    const float lo_y = shift_unkey(st_prefix[2]), hi_y = shift_unkey(st_prefix[3]);
    const float mdx = (n & 1u) ? lo_x : (lo_x + hi_x) * 0.5f, mdy = (n & 1u) ? lo_y : (lo_y + hi_y) * 0.5f;
    if (t == 0) {
        out[SIFT_SHIFT_MDX] = mdx; out[SIFT_SHIFT_MDY] = mdy;
        out[SIFT_SHIFT_RANKS] = lo_x; out[SIFT_SHIFT_RANKS + 1] = hi_x; out[SIFT_SHIFT_RANKS + 2] = lo_y; out[SIFT_SHIFT_RANKS + 3] = hi_y;
        counts[0] = n;
        if (!keep) counts[1] = 0;
    }
    if (!keep) return;
    // shift_keep_kernel
    const bool any = isfinite(mdx) && isfinite(mdy);         // a non-finite median keeps nothing
    unsigned int ok_mine = 0;
    for (int j = t; j < w.rows; j += SIFT_SHIFT_THREADS) {
        const uint2 k = seg_keys[j];
        bool ok = false;
        if (any && k.x != SIFT_SHIFT_UNUSED) {
            const float dx = shift_unkey(k.x), dy = shift_unkey(k.y);
            ok = fabsf(dx - mdx) <= tol && fabsf(dy - mdy) <= tol;
        }
        keep[(size_t)w.row0 + j] = ok ? 1 : 0;
        ok_mine += ok;
    }
    if (ok_mine) atomicAdd(&kept, ok_mine);
    __syncthreads();
    if (t == 0) counts[1] = kept;
}

}  // namespace siftk
