// k_stack_clip.hpp -- warp S <= 64 frames onto one grid and reduce them per output pixel to the weighted mean of the samples that
// survive an outlier rejection, in the same launch (siftmi_batch_stack_clip).  No reference
// counterpart.  k_stack.hpp's kernels are not touched; this header only uses its helpers (stack_key, stack_add, SIFT_STACK_DEPTH).
//
// The launch is k_stack.hpp's: 64 x 4 threads, one thread per OUTPUT pixel, grid (ceil(OW / 64), ceil(OH / 4)); every thread
// walks the device table of WarpFrame rows with SIFT_STACK_DEPTH gathers in flight.
//
// Contract per output pixel; binary32, one rounding per operation (-ffp-contract=off), restated in numpy by
// tests/stack_clip_ref.py:
//   v_s, live_s, c   k_stack.hpp's, from the same device functions (transform_taps, transform_value, transform_live); key() is
//             stack_key.  The kept set K starts as the live frames.  osum is k_stack.hpp's ordered sum over K in ascending s: the
//             first value starts the accumulator.
//   TRIM(n_low, n_high)   order the live samples by (key(v_s), s) ascending; h = min(n_high, c - 1), l = min(n_low, c - 1 - h);
//             the last h and the first l leave K.  At least one sample stays; the high side is served first; a positive NaN sorts
//             above +inf and goes with the high side.
//   SIGMA(kl, kh, iters)   kl2 = kl * kl, kh2 = kh * kh.  At most `iters` passes; a pass: n = |K|; n < 3: stop;
//             m = osum(v) / (float)n; d_s = v_s - m; q = osum(d_s * d_s); var = q / (float)n; tl = kl2 * var; th = kh2 * var;
//             s leaves when (d_s < 0 && d_s * d_s > tl) || (d_s > 0 && d_s * d_s > th).  A pass that would remove nothing stops; a
//             pass that would remove every kept sample removes none and stops.  The statistics are unweighted.  A NaN or an inf
//             among the kept values makes m, and with it every d_s * d_s or the thresholds, NaN or inf: every comparison is false
//             and nothing leaves -- the rule itself, no special case.
//   result    osum(w_s * v_s) / osum(w_s) over K in ascending s; kept = |K|; coverage = c; c == 0: `empty`, kept 0.  With
//             w_s = 1.0f (no weights given) w * v is v and the denominator is exactly (float)|K|: with nothing rejected the plane is
//             stack_reduce_kernel<true>'s bit for bit.
//
// Where the samples live.  They have to outlive the gather loop, and a dynamically indexed private array would go to scratch.
// They go to an LDS column laid out [frame][thread], stack_median_kernel's layout: the sample of frame s of thread t is word
// s * 256 + t, so the 64 lanes of a wave hit 64 consecutive words whichever frame each of them reads (no bank conflict).  Every
// frame's value is stored, live or not (a frame that is not live stores its fill), so no word below S * 256 is read before it is
// written.  K is a 64-bit mask in registers, bit s = frame s is kept; that is what caps S at SIFT_STACK_CLIP_MAX = 64.  Dynamic
// LDS is S * 1 KiB per block -- 64 KiB, the most a plain launch may ask for, at S = 64: two blocks of the 160 KiB of a CU.
// Nothing is shared between threads: no barrier.  The weights are a kernel argument (64 floats in the kernarg segment, read at a
// uniform index: scalar loads), so the launch needs no buffer beside the WarpFrame table.
//
// Cost per pixel beside the S gathers: a scan is S LDS reads (the loops run over every s < S, uniform across the wave, and test the
// thread's bit).  TRIM: h + l selection scans, then the result's scan.  SIGMA: the first pass's osum(v) is formed while gathering
// (K is the live set then); each pass is two scans -- q, then the removals together with the next pass's osum(v) over what stays
// -- and the result's scan follows: at most 2 * iters + 1 scans, and a wave runs as many passes as its slowest lane.
//
// Measured on one MI355X (tools/bench_stack_clip.py, kernel ms at 64 x 512^2 / 64 x 2048^2 / 16 x 4096^2; stack_reduce_kernel<true>
// on the same frames 0.043 / 0.43 / 0.44, stack_median_kernel 0.24 / 3.43 / 0.91): trim (0, 1) 0.078 / 1.13 / 0.57, trim (2, 2)
// 0.092 / 1.40 / 0.81, sigma (3, 3) on noise (one pass) 0.090 / 1.38 / 0.70 and with an outlier in every pixel (two passes)
// 0.111 / 1.68 / 0.85.  At S = 64 the scans are the smaller part of what the launch takes beyond the mean's (three more selection
// scans cost 0.27 ms at 64 x 2048^2); the larger is the stores and the two waves per SIMD that 64 KiB per block leave the gathers.
// The other home -- no LDS, the frames sampled again -- was built for trims of at most two samples per side (the two largest and
// two smallest (key, s) in registers on a first walk, a second walk summing what lies between the thresholds; 62 VGPRs, 8 waves)
// and measured in the same way: 0.096 / 1.06 / 1.06 for trim (0, 1) and 0.095 / 1.05 / 1.05 for trim (2, 2).  It wins only at
// 64 x 2048^2 and loses by half at S = 16, where 16 KiB per block cost this form no occupancy: it was taken out again.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; tools/resource_usage.py): stack_clip_kernel<TRIM> 58 VGPRs,
// <SIGMA> 60 (73 SGPRs each); 0 bytes of scratch, no spill and 8 waves per SIMD by registers for both; no static LDS.  What
// limits the waves is the dynamic LDS: S * 256 bytes per wave, all 8 per SIMD up to S = 20, 2 at S = 64.
//
// Cubic instances: stack_clip_cubic_kernel<REJECT> is the same body (k_stack_clip_body.hpp, included
// by both kernels) sampling with k_warp_cubic.hpp's cubic_taps / cubic_value, SIFT_STACK_DEPTH_CUBIC frames at a time; the same launch
// and the same dynamic LDS.  <TRIM> 72 VGPRs (7 waves per SIMD by registers), <SIGMA> 76 (6 waves); no scratch, no static LDS.
//
// Bounds: x < OW and y < OH by the launch shape and the first test; image reads stay inside image_s by transform_taps; rows s < S
// of the table only; an LDS word is s * 256 + t with s < S and t < 256, below the S * 256 words the launch asks for; weights w[s]
// with s < S <= 64 = the array's length (the library refuses S > 64 before the launch); a selection scan runs only while
// |K| >= 2, so it always finds a set bit and the shift 1 << best has best in [0, S); output offsets y * OW + x are formed in size_t.
#pragma once
#include "k_stack.hpp"

namespace siftk {

#define SIFT_STACK_CLIP_MAX 64
#define SIFT_STACK_TRIM 0
#define SIFT_STACK_SIGMA 1

struct StackClipArgs {
    float w[SIFT_STACK_CLIP_MAX];              // the weight of every frame (1.0f where the caller gave none)
    int n_low, n_high;                         // TRIM
    float kappa_low, kappa_high;               // SIGMA
    int iters;
};

template <int REJECT>
__global__ __launch_bounds__(256) void stack_clip_kernel(const WarpFrame *__restrict__ frames, int S, const StackClipArgs p,
                                                         float *__restrict__ out, int32_t *__restrict__ coverage,
                                                         int32_t *__restrict__ kept, int W, int H, int OW, int OH, float empty) {
#define STACK_BODY_TAPS_T WarpTaps
#define STACK_BODY_TAPS transform_taps
#define STACK_BODY_DEPTH SIFT_STACK_DEPTH
#include "k_stack_clip_body.hpp"
#undef STACK_BODY_TAPS_T
#undef STACK_BODY_TAPS
#undef STACK_BODY_DEPTH
}

template <int REJECT>
__global__ __launch_bounds__(256) void stack_clip_cubic_kernel(const WarpFrame *__restrict__ frames, int S, const StackClipArgs p,
                                                               float *__restrict__ out, int32_t *__restrict__ coverage,
                                                               int32_t *__restrict__ kept, int W, int H, int OW, int OH, float empty) {
#define STACK_BODY_TAPS_T CubicTaps
#define STACK_BODY_TAPS cubic_taps
#define STACK_BODY_DEPTH SIFT_STACK_DEPTH_CUBIC
#include "k_stack_clip_body.hpp"
#undef STACK_BODY_TAPS_T
#undef STACK_BODY_TAPS
#undef STACK_BODY_DEPTH
}

}  // namespace siftk
