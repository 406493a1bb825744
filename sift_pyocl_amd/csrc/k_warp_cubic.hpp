// k_warp_cubic.hpp -- the affine warp of k_align.hpp with a Catmull-Rom bicubic sampler (4 x 4 taps, a = -1/2) for float32 frames
// (siftmi_plan_transform_ex / siftmi_batch_transform_ex with SIFTMI_INTERP_CUBIC).  No reference
// counterpart: the reference resamples with its 2 x 2 bilinear kernel only.  The stack reductions' cubic instances are in
// k_stack.hpp and k_stack_clip.hpp; they sample with the device functions of this header.
//
// Contract per output pixel (x, y); binary32, every product, sum and difference rounded on its own in the order written
// (-ffp-contract=off is part of it); restated in numpy by tests/warp_cubic_ref.py:
//   (ty, tx)   as siftmi_plan_transform: ty = (m0*y + m1*x) + off0, tx = (m2*y + m3*x) + off1
//   live       0 <= tx && tx < (float)W + -0.5f && 0 <= ty && ty < (float)H + -0.5f      (transform_live, unchanged;
//              false for a non-finite tx or ty; no index is formed unless live)
//   !live      out = fill
//   xp = (int)tx, yp = (int)ty;  fx = tx - (float)xp,  fy = ty - (float)yp
//   columns    c_k = clamp(xp - 1 + k, 0, W - 1),  rows r_j = clamp(yp - 1 + j, 0, H - 1),  j, k = 0..3   (edge pixels repeat;
//              `fill` is never mixed into a live sample)
//   weights    w0 = ((-0.5f*f + 1.0f)*f - 0.5f)*f        w1 = ((1.5f*f - 2.5f)*f)*f + 1.0f
//              w2 = ((-1.5f*f + 2.0f)*f + 0.5f)*f        w3 = ((0.5f*f - 0.5f)*f)*f            (f = fx for wx, fy for wy)
//   rows       R_j = ((wx0*p[r_j][c_0] + wx1*p[r_j][c_1]) + wx2*p[r_j][c_2]) + wx3*p[r_j][c_3]
//   value      out = ((wy0*R_0 + wy1*R_1) + wy2*R_2) + wy3*R_3
//
// What follows from it:
//   * at f = 0 the weights are exactly (-0, 1, 0, -0): an integer shift of a finite frame returns its pixels bit for bit, except
//     that -0.0 becomes +0.0
//   * at f = 1/4, 1/2, 3/4 the weights are exact: k / 128 at the quarters, (-1, 9, 9, -1) / 16 at one half
//   * the four weights sum to 1 within 2.4e-7
//   * zero weights still multiply: a NaN anywhere in the 4 x 4 footprint makes the sample NaN, and so does an inf (0 * inf,
//     inf - inf) unless every weight it meets is non-zero and no opposite inf joins it -- at an integer shift only the sample ON
//     an inf pixel stays inf.  A NaN that the arithmetic creates is the hardware's default NaN, positive on gfx950 (negative on x86)
//   * the live set is the bilinear warp's non-fill set: coverage, `empty` and `kept` of a stack mean the same under both kernels
//   * a cubic sample can overshoot the range of its taps
//
// Loads.  Where 1 <= xp && xp + 2 <= W - 1 no column clamps and the four taps of a row are 16 contiguous bytes: one unaligned
// 16-byte load per row (gfx950 global loads need no alignment; transform_rgb_pixel relies on the same), 4 loads per pixel instead
// of 16.  Elsewhere -- the two columns at either edge, every pixel of a frame with W <= 3 -- the taps are 16 scalar loads at the
// clamped columns.  Both paths fill the same p[j][k] with the same pixels, and cubic_value is one text for both: the same bits.
// Rows always clamp by address (a row index costs no load).
//
// The two-step form (cubic_taps: every load of the pixel; cubic_value: the arithmetic) is transform_taps / transform_value's, so a
// stack kernel can have the taps of several frames in flight before it forms their values.  transform_cubic_pixel is the two
// steps one after the other.
//
// Bounds: x < OW, y < OH (and blockIdx.z < S) by the launch shape and the first test; no index is formed unless live, which gives
// 0 <= xp <= W - 1 and 0 <= yp <= H - 1; rows r_j and columns c_k are clamped into the frame; the 16-byte load reads columns
// xp - 1 .. xp + 2 of one row with xp - 1 >= 0 and xp + 2 <= W - 1; offsets r * W + c and the output offset are formed in size_t.
#pragma once
#include "k_align_batch.hpp"

namespace siftk {

#define SIFT_INTERP_MODE 0                 // what `mode` says: transform_pixel
#define SIFT_INTERP_CUBIC 1
#ifndef SIFT_CUBIC_WIDE
#define SIFT_CUBIC_WIDE 1                  // 0: every tap a scalar load, the form the 16-byte loads are measured against
#endif

typedef float CubicRow __attribute__((ext_vector_type(4), aligned(4)));    // four taps of a row: 16 bytes at any 4-byte boundary
struct CubicTaps { float tx, ty; float p[4][4]; bool live; };

__device__ __forceinline__ void cubic_weights(float f, float w[4]) {
    w[0] = ((-0.5f * f + 1.0f) * f - 0.5f) * f;
    w[1] = ((1.5f * f - 2.5f) * f) * f + 1.0f;
    w[2] = ((-1.5f * f + 2.0f) * f + 0.5f) * f;
    w[3] = ((0.5f * f - 0.5f) * f) * f;
}

__device__ __forceinline__ CubicTaps cubic_taps(const float *__restrict__ image, const AffineArgs &a, int W, int H, int x, int y) {
    float tx = a.m2 * (float)y + a.m3 * (float)x;
    float ty = a.m0 * (float)y + a.m1 * (float)x;
    tx += a.off1; ty += a.off0;
    CubicTaps t;
    t.tx = tx; t.ty = ty;
    t.live = 0.0f <= tx && tx < (float)W + -0.5f && 0.0f <= ty && ty < (float)H + -0.5f;
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int k = 0; k < 4; k++) t.p[j][k] = a.fill;        // (never read unless live; a defined value all the same)
    if (t.live) {
        const int xp = (int)tx, yp = (int)ty;
        const bool wide = SIFT_CUBIC_WIDE && 1 <= xp && xp + 2 <= W - 1;
        if (wide) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int r = min(max(yp - 1 + j, 0), H - 1);
                const CubicRow q = *reinterpret_cast<const CubicRow *>(image + (size_t)r * W + (xp - 1));
                t.p[j][0] = q.x; t.p[j][1] = q.y; t.p[j][2] = q.z; t.p[j][3] = q.w;
            }
        } else {
            int c[4];
#pragma unroll
            for (int k = 0; k < 4; k++) c[k] = min(max(xp - 1 + k, 0), W - 1);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float *row = image + (size_t)min(max(yp - 1 + j, 0), H - 1) * W;
#pragma unroll
                for (int k = 0; k < 4; k++) t.p[j][k] = row[c[k]];
            }
        }
    }
    return t;
}

__device__ __forceinline__ float cubic_value(const CubicTaps &t, const AffineArgs &a) {
    if (!t.live) return a.fill;
    const float fx = t.tx - (float)(int)t.tx, fy = t.ty - (float)(int)t.ty;
    float wx[4], wy[4], R[4];
    cubic_weights(fx, wx);
    cubic_weights(fy, wy);
#pragma unroll
    for (int j = 0; j < 4; j++) R[j] = ((wx[0] * t.p[j][0] + wx[1] * t.p[j][1]) + wx[2] * t.p[j][2]) + wx[3] * t.p[j][3];
    return ((wy[0] * R[0] + wy[1] * R[1]) + wy[2] * R[2]) + wy[3] * R[3];
}

// the names a stack kernel body calls for either kind of taps (k_stack.hpp)
__device__ __forceinline__ float transform_value(const CubicTaps &t, const AffineArgs &a, int, int) { return cubic_value(t, a); }
__device__ __forceinline__ bool transform_live(const CubicTaps &t, int, int) { return t.live; }

__device__ __forceinline__ float transform_cubic_pixel(const float *__restrict__ image, const AffineArgs &a, int W, int H, int x, int y) {
    return cubic_value(cubic_taps(image, a, W, H, x, y), a);
}

__global__ __launch_bounds__(256) void transform_cubic_kernel(const float *__restrict__ image, float *__restrict__ out, AffineArgs a,
                                                              int W, int H, int OW, int OH) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= OW || y >= OH) return;
    out[(size_t)y * OW + x] = transform_cubic_pixel(image, a, W, H, x, y);
}

// frame = blockIdx.z: transform_batch_kernel's table, tile and output layout
__global__ __launch_bounds__(256) void transform_cubic_batch_kernel(const WarpFrame *__restrict__ frames, float *__restrict__ out,
                                                                    int W, int H, int OW, int OH) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= OW || y >= OH) return;
    const WarpFrame &f = frames[blockIdx.z];
    const AffineArgs a = f.a;
    float *o = out + (size_t)blockIdx.z * OH * OW;
    o[(size_t)y * OW + x] = transform_cubic_pixel(static_cast<const float *>(f.image), a, W, H, x, y);
}

}  // namespace siftk
