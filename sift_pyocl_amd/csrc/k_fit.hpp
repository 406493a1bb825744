// k_fit.hpp -- least-squares affine map of matched keypoints on the device: what
// utils.affine_least_squares computes on the host, from the matches consensus_gather_kernel leaves in (x0, y0, x1, y1) form.
// No reference counterpart: the reference's utils.matching_correction stops before the solve (sift-src/utils.py:156-189).
//
// The arithmetic is a contract that tests/fit_ref.py restates in numpy, so all 20 results are compared as bit patterns.
// Everything is binary64, every product, sum and quotient rounded on its own in the order written (-ffp-contract=off); there
// is no floating-point atomic, and no result depends on scheduling:
//   used     pair j is used iff (mask == NULL || mask[j] != 0) and its four f32 coordinates are finite; an unused pair adds
//            +0.0 to every sum and nothing to n
//   R(v)     B workgroups of 256 lanes, G = 256 B; pair j belongs to lane (j mod G) % 256 of workgroup (j mod G) / 256
//            (i)   a lane adds its pairs in ascending j to +0.0
//            (ii)  the workgroup folds its 256 lane sums: for s = 128, 64, .. 1: lane t < s: v[t] = v[t] + v[t + s]
//            (iii) the workgroups' results are added in ascending workgroup index to +0.0
//   pass 1   n, sx = R(x0), sy = R(y0), su = R(x1), sv = R(y1); n == 0: EMPTY; else the means mx = sx / n, ...
//   pass 2   X = x0 - mx, Y = y0 - my, U = x1 - mu, V = y1 - mv: Sxx = R(X*X), Sxy = R(X*Y), Syy = R(Y*Y), Sxu = R(X*U),
//            Syu = R(Y*U), Sxv = R(X*V), Syv = R(Y*V)
//   solve    scale = Sxx*Syy, det = scale - Sxy*Sxy; DEGENERATE iff n < 3 || !(fabs(det) > 1e-12 * fmax(1.0, scale));
//            a = (Sxu*Syy - Syu*Sxy)/det, b = (Syu*Sxx - Sxu*Sxy)/det, c = mu - (a*mx + b*my); d, e, f from Sxv, Syv, mv
//   pass 3   ex = ((a*x0 + b*y0) + c) - x1, ey = ((d*x0 + e*y0) + f) - y1, ssr = R(ex*ex + ey*ey)
//
// Launch structure: step (iii) of a pass is done by every workgroup of the next launch, redundantly and in the same order
// (lane k adds column k of the partials), so each workgroup holds the same means / model without a launch in between:
// fit_pass1_kernel -> fit_pass2_kernel (means) -> fit_pass3_kernel (solve) -> fit_finish_kernel (ssr).  Workgroup 0 writes the
// results.  The work is three reads of M x 16 bytes: launch latency, not a hot path.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace siftk {

#define SIFT_FIT_THREADS 256
#define SIFT_FIT_MAX_BLOCKS 1024
// the 20 results, in the order of siftmi_match_fit's `out`
#define SIFT_FIT_STATUS 0
#define SIFT_FIT_N 1
#define SIFT_FIT_MEANS 2       // mx, my, mu, mv
#define SIFT_FIT_MOMENTS 6     // Sxx, Sxy, Syy, Sxu, Syu, Sxv, Syv
#define SIFT_FIT_MODEL 13      // a, b, c, d, e, f
#define SIFT_FIT_SSR 19
#define SIFT_FIT_OUT 20

// scratch of one call: the workgroups' results of the three passes and their counts of used pairs
struct FitPartials {
    double p1[SIFT_FIT_MAX_BLOCKS][4];
    double p2[SIFT_FIT_MAX_BLOCKS][7];
    double p3[SIFT_FIT_MAX_BLOCKS];
    unsigned long long count[SIFT_FIT_MAX_BLOCKS];
    double out[SIFT_FIT_OUT];
};

__device__ __forceinline__ double fit_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__device__ __forceinline__ bool fit_used(const float4 p, const uint8_t *__restrict__ mask, long long j) {
    return (mask == nullptr || mask[j] != 0) && isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && isfinite(p.w);
}

// step (ii) on N values per lane at once: v[k][t] holds lane t's sum of value k; the result is v[k][0]
template <int N>
__device__ __forceinline__ void fit_tree(double (*v)[SIFT_FIT_THREADS], int t) {
    __syncthreads();
    for (int s = SIFT_FIT_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < N; k++) v[k][t] = v[k][t] + v[k][t + s];
        }
        __syncthreads();
    }
}

// step (iii) for N columns of `B` rows: lane k < N adds column k in ascending row order; total[k] is valid after the barrier
template <int N>
__device__ __forceinline__ void fit_serial(const double *__restrict__ part, int B, double *total, int t) {
    if (t < N) {
        double acc = 0.0;
        for (int b = 0; b < B; b++) acc = acc + part[(size_t)b * N + t];
        total[t] = acc;
    }
    __syncthreads();
}

__global__ __launch_bounds__(SIFT_FIT_THREADS) void fit_pass1_kernel(const float4 *__restrict__ pts, const uint8_t *__restrict__ mask, int M,
                                                                     FitPartials *__restrict__ fp) {
    __shared__ double v[4][SIFT_FIT_THREADS];
    __shared__ unsigned int cnt[SIFT_FIT_THREADS];
    const int t = threadIdx.x;
    const long long G = (long long)gridDim.x * SIFT_FIT_THREADS;
    double sx = 0.0, sy = 0.0, su = 0.0, sv = 0.0;
    unsigned int n = 0;
    for (long long j = (long long)blockIdx.x * SIFT_FIT_THREADS + t; j < M; j += G) {
        const float4 p = pts[j];
        if (fit_used(p, mask, j)) {
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
        fp->count[blockIdx.x] = total;
#pragma unroll
        for (int k = 0; k < 4; k++) fp->p1[blockIdx.x][k] = v[k][0];
    }
}

// n and the means from pass 1's partials (every workgroup, the same arithmetic), then the seven centred moments
__global__ __launch_bounds__(SIFT_FIT_THREADS) void fit_pass2_kernel(const float4 *__restrict__ pts, const uint8_t *__restrict__ mask, int M,
                                                                     FitPartials *__restrict__ fp) {
    __shared__ double v[7][SIFT_FIT_THREADS];
    __shared__ double sums[4];
    __shared__ unsigned long long n_all;
    const int t = threadIdx.x, B = gridDim.x;
    if (t == 4) {
        unsigned long long total = 0;
        for (int b = 0; b < B; b++) total += fp->count[b];
        n_all = total;
    }
    fit_serial<4>(&fp->p1[0][0], B, sums, t);
    const unsigned long long n = n_all;
    if (n == 0) {                                           // EMPTY: status and n, everything else NaN; nothing further runs
        if (blockIdx.x == 0 && t < SIFT_FIT_OUT) fp->out[t] = t == SIFT_FIT_STATUS ? 1.0 : t == SIFT_FIT_N ? 0.0 : fit_nan();
        return;
    }
    const double nd = (double)n;
    const double mx = sums[0] / nd, my = sums[1] / nd, mu = sums[2] / nd, mv = sums[3] / nd;
    if (blockIdx.x == 0 && t == 0) {
        fp->out[SIFT_FIT_N] = nd;
        fp->out[SIFT_FIT_MEANS] = mx; fp->out[SIFT_FIT_MEANS + 1] = my; fp->out[SIFT_FIT_MEANS + 2] = mu; fp->out[SIFT_FIT_MEANS + 3] = mv;
    }
    const long long G = (long long)B * SIFT_FIT_THREADS;
    double s[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long j = (long long)blockIdx.x * SIFT_FIT_THREADS + t; j < M; j += G) {
        const float4 p = pts[j];
        if (fit_used(p, mask, j)) {
            const double X = (double)p.x - mx, Y = (double)p.y - my, U = (double)p.z - mu, V = (double)p.w - mv;
            s[0] = s[0] + X * X; s[1] = s[1] + X * Y; s[2] = s[2] + Y * Y;
            s[3] = s[3] + X * U; s[4] = s[4] + Y * U; s[5] = s[5] + X * V; s[6] = s[6] + Y * V;
        }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) v[k][t] = s[k];
    fit_tree<7>(v, t);
    if (t < 7) fp->p2[blockIdx.x][t] = v[t][0];
}

// the moments from pass 2's partials and the solve (every workgroup, the same arithmetic), then the squared residuals
__global__ __launch_bounds__(SIFT_FIT_THREADS) void fit_pass3_kernel(const float4 *__restrict__ pts, const uint8_t *__restrict__ mask, int M,
                                                                     FitPartials *__restrict__ fp) {
    __shared__ double v[1][SIFT_FIT_THREADS];
    __shared__ double S[7];
    const int t = threadIdx.x, B = gridDim.x;
    const double nd = fp->out[SIFT_FIT_N];                  // written by workgroup 0 of the launch before this one
    if (!(nd > 0.0)) return;                                // EMPTY
    fit_serial<7>(&fp->p2[0][0], B, S, t);
    const double mx = fp->out[SIFT_FIT_MEANS], my = fp->out[SIFT_FIT_MEANS + 1], mu = fp->out[SIFT_FIT_MEANS + 2], mv = fp->out[SIFT_FIT_MEANS + 3];
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
    if (blockIdx.x == 0 && t == 0) {
        fp->out[SIFT_FIT_STATUS] = degenerate ? 2.0 : 0.0;
        for (int k = 0; k < 7; k++) fp->out[SIFT_FIT_MOMENTS + k] = S[k];
        fp->out[SIFT_FIT_MODEL] = a; fp->out[SIFT_FIT_MODEL + 1] = b; fp->out[SIFT_FIT_MODEL + 2] = c;
        fp->out[SIFT_FIT_MODEL + 3] = d; fp->out[SIFT_FIT_MODEL + 4] = e; fp->out[SIFT_FIT_MODEL + 5] = f;
        fp->out[SIFT_FIT_SSR] = fit_nan();                  // fit_finish_kernel replaces it when the status is OK
    }
    if (degenerate) return;
    const long long G = (long long)B * SIFT_FIT_THREADS;
    double r = 0.0;
    for (long long j = (long long)blockIdx.x * SIFT_FIT_THREADS + t; j < M; j += G) {
        const float4 p = pts[j];
        if (fit_used(p, mask, j)) {
            const double x0 = p.x, y0 = p.y, x1 = p.z, y1 = p.w;
            const double ex = ((a * x0 + b * y0) + c) - x1, ey = ((d * x0 + e * y0) + f) - y1;
            r = r + (ex * ex + ey * ey);
        }
    }
    v[0][t] = r;
    fit_tree<1>(v, t);
    if (t == 0) fp->p3[blockIdx.x] = v[0][0];
}

// one lane: step (iii) of pass 3
__global__ __launch_bounds__(64) void fit_finish_kernel(FitPartials *__restrict__ fp, int B) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (fp->out[SIFT_FIT_STATUS] != 0.0) return;            // EMPTY or DEGENERATE: ssr stays NaN
    double acc = 0.0;
    for (int b = 0; b < B; b++) acc = acc + fp->p3[b];
    fp->out[SIFT_FIT_SSR] = acc;
}

}  // namespace siftk
