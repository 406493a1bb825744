// k_stack.hpp -- warp S frames onto one grid and reduce them to ONE plane in the same launch (siftmi_batch_stack; DESIGN.md
// section 7 row 17).  No reference counterpart: the reference aligns frame by frame and leaves the combination to the caller.
//
// The launch is transform_batch_kernel's without the z axis: 64 x 4 threads, one thread per OUTPUT pixel, grid
// (ceil(OW / 64), ceil(OH / 4)).  Every thread walks the device table of WarpFrame rows (k_align_batch.hpp) for s = 0 .. S-1;
// the row address is uniform across the block, plain loads that stay in scalar registers.  The S warped planes are never
// written: HBM sees the S gathered reads of the batch warp and one plane (plus the coverage plane) of writes.
//
// Contract per output pixel (x, y); binary32, one rounding per operation (-ffp-contract=off), restated in numpy by
// tests/stack_ref.py:
//   sample    v_s = transform_pixel(image_s, a_s, W, H, x, y), computed as its two steps transform_value(transform_taps(...))
//             (k_align.hpp: the same operations in the same order, bilinear_mix itself), edge taps replaced by fills[s] included
//   live      live_s = 0 <= tx && tx < (float)W + -0.5f && 0 <= ty && ty < (float)H + -0.5f (transform_live, on the tx, ty of
//             the taps): where the warp's value is not the fill for a geometric reason.  A non-finite tx or ty is never live: a
//             frame whose map holds a NaN is left out wherever the NaN reaches, an all-NaN map leaves it out everywhere
//   coverage  c = number of live frames (int32)
//   sum       over the live frames in ascending s: acc = v for the first, acc = acc + v for each later one (the sum of one
//             value is that value, sign of a zero included)
//   mean      acc / (float)c, IEEE division
//   median    key(v) = bits(v) ^ (bits(v) >> 31 ? 0xffffffff : 0x80000000), the order key of k_shift.hpp; lo, hi = the live
//             values of rank (c - 1) >> 1 and c >> 1 in ascending key order; c odd: lo, c even: (lo + hi) * 0.5f.
//             S <= SIFT_STACK_MEDIAN_MAX only.  A NaN sample takes the place its bits give it: a NaN pixel keeps its sign through
//             the sample (every NaN tap of one sign), a NaN that the sample's own arithmetic creates (0 * inf, inf - inf) is the
//             hardware's default NaN, positive on gfx950
//   c == 0    the caller's `empty`
//
// Gathers in flight: a thread's frames form a chain of dependent gathers, and a small output (512 x 512: 4096 waves, half the
// wave slots of the chip) has few other waves to hide them behind.  The loops therefore take SIFT_STACK_DEPTH = 4 frames at a
// time: the four table rows into registers (one wide scalar load each, one wait), the taps of the four (16 loads), then the four
// values and the four reductions, in ascending s.  Measured on one MI355X (tools/bench_stack.py, mean, kernel ms at 64 x 512^2 /
// 64 x 2048^2 / 16 x 4096^2; transform_batch_kernel on the same frames 0.042 / 0.70 / 0.69): 0.044 / 0.42 / 0.43.  With the
// rows read where they are used (the compiler then loads some fields again between the gathers and the values) the depths
// compared as: 1: 0.051 / 0.51 / 0.52, 4: 0.047 / 0.47 / 0.48, 8 (86 VGPRs, 5 waves): 0.047 / 0.52 / 0.54, 16 (150 VGPRs, 3
// waves): 0.062 / 0.66 / 0.71.
//
// stack_reduce_kernel<MEAN>: sum (false) and mean (true) are two compile-time instances; no LDS, one pass over the frames.
// S == 0 is allowed and is the library's fill path: every pixel gets `empty`, coverage 0; the table is not read.
//
// stack_median_kernel: the thread keeps the keys of its live samples sorted in an LDS column laid out [slot][thread]: slot j of
// thread t is word j * 256 + t, so the 64 lanes of a wave hit 64 consecutive words whatever their slots are (no bank conflict,
// no dynamically indexed per-thread array).  A new key is inserted by shifting the larger keys up one slot.  Only the
// K = (S >> 1) + 1 smallest keys are kept: both ranks are <= c >> 1 <= S >> 1 for every coverage c <= S, so a key that is not
// among the K smallest can never be selected and is dropped (a non-live frame takes no slot at all).  Dynamic LDS is therefore
// K * 256 * 4 bytes -- 2 KiB for S <= 3, 33 KiB for S = 64, always below the 64 KiB a plain launch may ask for -- and the block
// stays 64 x 4 for every S.  Nothing is shared between threads: no barrier.  Cost: at most K shifts per frame, S * K / 2 LDS
// read + write pairs per pixel for descending values (1056 at S = 64).  A wave pays for its slowest lane, so values in random
// order cost what descending ones cost: 64 x 2048^2 takes 3.43 ms on noise, 3.45 ms when every frame is darker than the one
// before and 0.65 ms when every frame is brighter (a key that goes behind the kept ones moves nothing): at S = 64 the selection is
// four fifths of the launch.
//
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; tools/resource_usage.py): 54 VGPRs for each of
// stack_reduce_kernel<false>, <true> and stack_median_kernel (67 SGPRs each); 0 bytes of scratch, no spill and 8 waves per
// SIMD by registers for all three; no static LDS.
//
// Cubic instances: stack_reduce_cubic_kernel<MEAN> and stack_median_cubic_kernel sample with
// k_warp_cubic.hpp's cubic_taps / cubic_value instead of transform_taps / transform_value, SIFT_STACK_DEPTH_CUBIC = 2 frames at a time
// (16 taps a frame); live frames, the order of every sum, the LDS column and the launch (shape and dynamic LDS) are the same.  The
// body of each kernel is ONE text that the legacy kernel and its cubic twin include (k_stack_reduce_body.hpp,
// k_stack_median_body.hpp; why an include and not a template is said there): the legacy kernels compile to the code they had.
// Resources of the cubic instances: reduce 70 VGPRs (7 waves per SIMD), median 74 (6 waves); no scratch, no static LDS.
//
// Bounds: x < OW and y < OH by the launch shape and the first test; reads stay inside image_s (W x H, the batch's shape) by
// transform_taps, which forms no index unless the point is inside; rows s < S of the table only; an LDS slot is an insertion
// point j <= min(c, K - 1) or a rank <= c >> 1 <= K - 1 read only when c >= 1, so the word index 256 * j + t is < K * 256, which
// is what the launch asks for, and K <= S for every S >= 1: the index is < S * 256; output offsets y * OW + x are formed in size_t.
#pragma once
#include "k_warp_cubic.hpp"

namespace siftk {

#define SIFT_STACK_MEDIAN_MAX 64
#ifndef SIFT_STACK_DEPTH
#define SIFT_STACK_DEPTH 4                 // frames whose taps are loaded before their values are formed
#endif
#ifndef SIFT_STACK_DEPTH_CUBIC
#define SIFT_STACK_DEPTH_CUBIC 2           // the same for the cubic instances: 16 taps a frame instead of 4 (1 and 4 measured slower)
#endif

__device__ __forceinline__ uint32_t stack_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}

__device__ __forceinline__ float stack_unkey(uint32_t k) {
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

// slots the median keeps per thread, and the dynamic LDS of its launch
__host__ __device__ __forceinline__ int stack_median_slots(int S) { return (S >> 1) + 1; }

// the ordered sum: one more live value
__device__ __forceinline__ void stack_add(float &acc, int &c, float v, bool live) {
    if (live) { acc = c ? acc + v : v; c++; }
}

template <bool MEAN>
__global__ __launch_bounds__(256) void stack_reduce_kernel(const WarpFrame *__restrict__ frames, int S, float *__restrict__ out,
                                                           int32_t *__restrict__ coverage, int W, int H, int OW, int OH, float empty) {
#define STACK_BODY_TAPS_T WarpTaps
#define STACK_BODY_TAPS transform_taps
#define STACK_BODY_DEPTH SIFT_STACK_DEPTH
#include "k_stack_reduce_body.hpp"
#undef STACK_BODY_TAPS_T
#undef STACK_BODY_TAPS
#undef STACK_BODY_DEPTH
}

template <bool MEAN>
__global__ __launch_bounds__(256) void stack_reduce_cubic_kernel(const WarpFrame *__restrict__ frames, int S, float *__restrict__ out,
                                                                 int32_t *__restrict__ coverage, int W, int H, int OW, int OH, float empty) {
#define STACK_BODY_TAPS_T CubicTaps
#define STACK_BODY_TAPS cubic_taps
#define STACK_BODY_DEPTH SIFT_STACK_DEPTH_CUBIC
#include "k_stack_reduce_body.hpp"
#undef STACK_BODY_TAPS_T
#undef STACK_BODY_TAPS
#undef STACK_BODY_DEPTH
}

// one more live key into the sorted column of this thread (col points at its slot 0; slots are 256 words apart)
__device__ __forceinline__ void stack_insert(uint32_t *col, int K, int &c, uint32_t key, bool live) {
    if (!live) return;
    const bool full = c >= K;
    int j = full ? K - 1 : c;                      // the last slot, whose key leaves when the new one is smaller, or the first free one
    c++;
    if (full && col[256 * j] <= key) return;
    while (j > 0) {
        const uint32_t below = col[256 * (j - 1)];
        if (below <= key) break;
        col[256 * j] = below;
        j--;
    }
    col[256 * j] = key;
}

__global__ __launch_bounds__(256) void stack_median_kernel(const WarpFrame *__restrict__ frames, int S, float *__restrict__ out,
                                                           int32_t *__restrict__ coverage, int W, int H, int OW, int OH, float empty) {
#define STACK_BODY_TAPS_T WarpTaps
#define STACK_BODY_TAPS transform_taps
#define STACK_BODY_DEPTH SIFT_STACK_DEPTH
#include "k_stack_median_body.hpp"
#undef STACK_BODY_TAPS_T
#undef STACK_BODY_TAPS
#undef STACK_BODY_DEPTH
}

__global__ __launch_bounds__(256) void stack_median_cubic_kernel(const WarpFrame *__restrict__ frames, int S, float *__restrict__ out,
                                                                 int32_t *__restrict__ coverage, int W, int H, int OW, int OH, float empty) {
#define STACK_BODY_TAPS_T CubicTaps
#define STACK_BODY_TAPS cubic_taps
#define STACK_BODY_DEPTH SIFT_STACK_DEPTH_CUBIC
#include "k_stack_median_body.hpp"
#undef STACK_BODY_TAPS_T
#undef STACK_BODY_TAPS
#undef STACK_BODY_DEPTH
}

}  // namespace siftk
