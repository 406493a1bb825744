// k_align_batch.hpp -- the affine warp of k_align.hpp for a whole stack of frames in ONE launch (siftmi_batch_transform).
//
// Frame s is blockIdx.z.  Every block reads its frame's row of a device table -- the image address and the map, 40 bytes at an
// address that is uniform across the block, i.e. plain loads that the compiler may keep in scalar registers -- and writes
// frame s of one contiguous output: out + s * OH * OW elements (x 3 bytes for RGB8).  The tile shape is the single kernels':
// 64 x 4 threads, one pixel per thread for float32 and 4 pixels per thread for RGB8.  Still HBM bound (8 B / pixel float32,
// 6 B / pixel RGB8); what the batch form removes is the launch, the synchronisation and the copy per frame, which is all a
// stack of small frames pays for.
//
// Per-frame contract: frame s is bit for bit what transform_kernel / transform_rgb_kernel write for (image_s, map_s, fill_s,
// mode) -- the per-pixel bodies are the SAME device functions (transform_pixel, transform_rgb_quad), and the build has
// -ffp-contract=off, so a call site changes no value.  A map with a non-finite entry makes tx or ty non-finite in every pixel
// it reaches; such a pixel fails the `inside` test, forms no index and is fill_s: an all-NaN map gives a plane of fill_s.
//
// RGB8: frame s starts s * OH * OW * 3 bytes into the output, so its rows take every alignment mod 4 even when the output
// itself is aligned; transform_rgb_quad tests the address it stores to, not the column.
//
// Bounds: x < OW, y < OH and blockIdx.z < S by the launch shape; reads stay inside image_s (W x H, the batch's shape) by
// transform_pixel / transform_rgb_pixel; the largest offset written is S * OH * OW elements, formed in size_t.
#pragma once
#include "k_align.hpp"

namespace siftk {

struct WarpFrame { const void *image; AffineArgs a; };

__global__ __launch_bounds__(256) void transform_batch_kernel(const WarpFrame *__restrict__ frames, float *__restrict__ out,
                                                              int W, int H, int OW, int OH) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= OW || y >= OH) return;
    const WarpFrame &f = frames[blockIdx.z];
    const AffineArgs a = f.a;
    float *o = out + (size_t)blockIdx.z * OH * OW;
    o[(size_t)y * OW + x] = transform_pixel(static_cast<const float *>(f.image), a, W, H, x, y);
}

__global__ __launch_bounds__(256) void transform_rgb_batch_kernel(const WarpFrame *__restrict__ frames, uint8_t *__restrict__ out,
                                                                  int W, int H, int OW, int OH) {
    const int x0 = (blockIdx.x * 64 + threadIdx.x) * 4, y = blockIdx.y * 4 + threadIdx.y;
    if (x0 >= OW || y >= OH) return;
    const WarpFrame &f = frames[blockIdx.z];
    const AffineArgs a = f.a;
    uint8_t *o = out + 3 * ((size_t)blockIdx.z * OH * OW + (size_t)y * OW + x0);
    transform_rgb_quad(static_cast<const uint8_t *>(f.image), a, W, H, OW, x0, y, o);
}

}  // namespace siftk
