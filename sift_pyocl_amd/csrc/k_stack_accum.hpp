// k_stack_accum.hpp -- the streaming form of the stack reduction (siftmi_batch_stack_accum / siftmi_batch_stack_accum_result;
// DESIGN.md section 7 row 20).  No reference counterpart.  A stack of any length is fed chunk after chunk: a launch warps the S
// frames of ONE chunk as k_stack.hpp does and adds them into per-pixel running sums that live in device memory across calls; a
// second, tiny kernel turns the sums into mean and variance.  k_stack.hpp, k_stack_clip.hpp, k_align*.hpp and k_warp_cubic.hpp
// are not touched: this header calls their device functions (transform_taps / cubic_taps, transform_value, transform_live).
//
// stack_accum_kernel<CUBIC, MOMENTS, CLIP>: the launch is stack_reduce_kernel's -- 64 x 4 threads, one thread per OUTPUT pixel,
// grid (ceil(OW / 64), ceil(OH / 4)) -- and so is the walk over the device table of WarpFrame rows, SIFT_STACK_DEPTH frames at a
// time (SIFT_STACK_DEPTH_CUBIC for the cubic instances): the rows of a group, then the taps of the group (its gathers are in flight
// together), then the values and the additions in ascending s.  The state of the thread's pixel is loaded before the loop and
// stored once after it; a thread touches only its own pixel: no atomics, no LDS, no barrier.
//
// State planes, OH x OW each, contiguous, owned and zero-filled by the caller before the first call:
//   s1        binary64   sum of the kept samples
//   s2        binary64   sum of their squares (MOMENTS instances only; the others never form its address)
//   coverage  int32      live samples
//   kept      int32      live samples that were not rejected
//
// Contract per output pixel o (-ffp-contract=off, one rounding per operation; restated in numpy by tests/stack_accum_ref.py):
//   v_s, live_s   k_stack.hpp's sample and live flag of frame s, from the same device functions
//   CLIP          m = center[o], tl = kl2 * var[o], th = kh2 * var[o] in binary32, with kl2 = kappa_low * kappa_low and
//                 kh2 = kappa_high * kappa_high formed in binary32 by the library
//   for s ascending, live frames only:
//       coverage += 1
//       CLIP      d = v_s - m; q = d * d; rejected = (d < 0 && q > tl) || (d > 0 && q > th)       (binary32)
//       not rejected:  s1 = s1 + (double)v_s;  s2 = s2 + (double)v_s * (double)v_s;  kept += 1
//   The product of two binary32 values is exact in binary64, so s2 takes one rounding per sample, as s1 does.  A NaN anywhere --
//   sample, centre, variance, or the inf * 0 of an infinite kappa on a zero variance -- makes the comparisons false: not rejected.
//   var[o] == 0 with finite kappas rejects every sample that differs from the centre.  This is stack_clip_kernel<SIGMA>'s rule
//   with the statistics supplied from outside (k_stack_clip.hpp).
//
// stack_accum_result_kernel<VAR>: one thread per pixel, 256 a block, a one-dimensional grid.
//   k = kept; k == 0: mean = var = empty
//   else M = s1 / (double)k; mean = (float)M; V = s2 / (double)k - M * M; var = (float)(V < 0 ? 0 : V)
//   The population variance, as the sigma rule's q / n is.  No square root: the clip takes the variance plane as it is.
//
// Second moments and the clip are compile-time instances, not uniform run-time branches: the plain instance then carries neither
// the second accumulator's two registers nor the three clip values through the gather loop, and is the mean kernel plus one
// conversion and one binary64 addition per live sample.
//
// Traffic per output pixel beside the S gathers (4 S bytes when every tap is a cache hit but one): 16 bytes of s1, 8 of coverage
// and kept, each read and written: 4 S + 32 against the mean's 4 S + 4; MOMENTS 4 S + 48; CLIP 8 more (centre and variance).
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; tools/resource_usage.py); 0 bytes of scratch, no spill and no
// LDS for every instance.  VGPRs / SGPRs / waves per SIMD by registers, <CUBIC, MOMENTS, CLIP>:
//   bilinear   plain 60 / 61 / 8    clip 62 / 61 / 8    moments 64 / 61 / 8    moments + clip 66 / 61 / 7
//   cubic      plain 76 / 42 / 6    clip 80 / 38 / 6    moments 80 / 36 / 6    moments + clip 86 / 38 / 5
//   stack_accum_result_kernel<false> 14 / 13 / 8, <true> 26 / 18 / 8
// (stack_reduce_kernel<true>: 54 VGPRs, 8 waves; stack_reduce_cubic_kernel<true>: 70, 7 waves.)
//
// Bounds: x < OW and y < OH by the launch shape and the first test; reads stay inside image_s (W x H, the batch's shape) by
// transform_taps / cubic_taps, which form no index unless the point is inside (cubic: clamped into the frame); rows s < S of the
// table only; every plane is indexed by o = y * OW + x < OH * OW, formed in size_t; the result kernel's index is
// blockIdx.x * 256 + threadIdx.x in size_t, tested against n = OH * OW before any access.
#pragma once
#include "k_stack.hpp"

namespace siftk {

// the sampler of an instance: taps type, depth of a group and the function that loads the taps
template <bool CUBIC> struct StackAccumSampler;
template <> struct StackAccumSampler<false> {
    typedef WarpTaps Taps;
    static constexpr int DEPTH = SIFT_STACK_DEPTH;
    static __device__ __forceinline__ Taps taps(const float *__restrict__ image, const AffineArgs &a, int W, int H, int x, int y) {
        return transform_taps(image, a, W, H, x, y);
    }
};
template <> struct StackAccumSampler<true> {
    typedef CubicTaps Taps;
    static constexpr int DEPTH = SIFT_STACK_DEPTH_CUBIC;
    static __device__ __forceinline__ Taps taps(const float *__restrict__ image, const AffineArgs &a, int W, int H, int x, int y) {
        return cubic_taps(image, a, W, H, x, y);
    }
};

struct StackAccumClip { const float *center, *var; float kl2, kh2; };      // CLIP instances only; kl2, kh2: the squared kappas

// one more sample into the state of this thread's pixel
template <bool MOMENTS, bool CLIP>
__device__ __forceinline__ void stack_accum_add(double &a1, double &a2, int &c, int &k, float v, bool live, float m, float tl, float th) {
    if (!live) return;
    c++;
    if (CLIP) {
        const float d = v - m, q = d * d;
        if ((d < 0.0f && q > tl) || (d > 0.0f && q > th)) return;
    }
    a1 = a1 + (double)v;
    if (MOMENTS) a2 = a2 + (double)v * (double)v;
    k++;
}

template <bool CUBIC, bool MOMENTS, bool CLIP>
__global__ __launch_bounds__(256) void stack_accum_kernel(const WarpFrame *__restrict__ frames, int S, double *__restrict__ s1,
                                                          double *__restrict__ s2, int32_t *__restrict__ coverage,
                                                          int32_t *__restrict__ kept, const StackAccumClip clip, int W, int H, int OW, int OH) {
    typedef StackAccumSampler<CUBIC> Sampler;
    typedef typename Sampler::Taps Taps;
    constexpr int DEPTH = Sampler::DEPTH;
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= OW || y >= OH) return;
    const size_t o = (size_t)y * OW + x;
    double a1 = s1[o], a2 = MOMENTS ? s2[o] : 0.0;
    int c = coverage[o], k = kept[o];
    float m = 0.0f, tl = 0.0f, th = 0.0f;
    if (CLIP) {
        const float var = clip.var[o];
        m = clip.center[o];
        tl = clip.kl2 * var;
        th = clip.kh2 * var;
    }
    int s = 0;
    for (; s + DEPTH <= S; s += DEPTH) {
        WarpFrame f[DEPTH];
        Taps t[DEPTH];
#pragma unroll
        for (int j = 0; j < DEPTH; j++) f[j] = frames[s + j];
#pragma unroll
        for (int j = 0; j < DEPTH; j++) t[j] = Sampler::taps(static_cast<const float *>(f[j].image), f[j].a, W, H, x, y);
#pragma unroll
        for (int j = 0; j < DEPTH; j++)
            stack_accum_add<MOMENTS, CLIP>(a1, a2, c, k, transform_value(t[j], f[j].a, W, H), transform_live(t[j], W, H), m, tl, th);
    }
    for (; s < S; s++) {
        const WarpFrame f = frames[s];
        const Taps t = Sampler::taps(static_cast<const float *>(f.image), f.a, W, H, x, y);
        stack_accum_add<MOMENTS, CLIP>(a1, a2, c, k, transform_value(t, f.a, W, H), transform_live(t, W, H), m, tl, th);
    }
    s1[o] = a1;
    if (MOMENTS) s2[o] = a2;
    coverage[o] = c;
    kept[o] = k;
}

template <bool VAR>
__global__ __launch_bounds__(256) void stack_accum_result_kernel(const double *__restrict__ s1, const double *__restrict__ s2,
                                                                 const int32_t *__restrict__ kept, size_t n, float *__restrict__ mean,
                                                                 float *__restrict__ var, float empty) {
    const size_t o = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (o >= n) return;
    const int k = kept[o];
    if (k == 0) {
        mean[o] = empty;
        if (VAR) var[o] = empty;
        return;
    }
    const double M = s1[o] / (double)k;
    mean[o] = (float)M;
    if (VAR) {
        const double V = s2[o] / (double)k - M * M;
        var[o] = (float)(V < 0.0 ? 0.0 : V);
    }
}

}  // namespace siftk
