// k_stack_reduce_body.hpp -- the body of stack_reduce_kernel<MEAN> / stack_reduce_cubic_kernel<MEAN>, included INSIDE the kernel definitions of k_stack.hpp (no include guard on
// purpose: it is text, not declarations).  The legacy kernel and its cubic twin are this one text; the includer defines
//   STACK_BODY_TAPS_T   the taps of one frame (WarpTaps / CubicTaps)
//   STACK_BODY_TAPS     the function that loads them (transform_taps / cubic_taps)
//   STACK_BODY_DEPTH    frames whose taps are in flight together (SIFT_STACK_DEPTH / SIFT_STACK_DEPTH_CUBIC)
// and transform_value / transform_live are overloaded on the taps type (k_align.hpp, k_warp_cubic.hpp).  Why an include and not
// a `template <int INTERP> __device__ __forceinline__` body that both kernels call: that form was built first, and the extra
// inlining layer alone changed the legacy kernels' code (commuted s_and_b64 operands, one moved s_add in each unrolled group) --
// harmless, but no longer the parent's code instruction for instruction, which is what lets the legacy paths go unmeasured.
// After preprocessing, the legacy kernels' token stream is exactly what it was.
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= OW || y >= OH) return;
    float acc = 0.0f;
    int c = 0, s = 0;
    for (; s + STACK_BODY_DEPTH <= S; s += STACK_BODY_DEPTH) {
        WarpFrame f[STACK_BODY_DEPTH];
        STACK_BODY_TAPS_T t[STACK_BODY_DEPTH];
#pragma unroll
        for (int k = 0; k < STACK_BODY_DEPTH; k++) f[k] = frames[s + k];
#pragma unroll
        for (int k = 0; k < STACK_BODY_DEPTH; k++) t[k] = STACK_BODY_TAPS(static_cast<const float *>(f[k].image), f[k].a, W, H, x, y);
#pragma unroll
        for (int k = 0; k < STACK_BODY_DEPTH; k++) stack_add(acc, c, transform_value(t[k], f[k].a, W, H), transform_live(t[k], W, H));
    }
    for (; s < S; s++) {
        const WarpFrame f = frames[s];
        const STACK_BODY_TAPS_T t = STACK_BODY_TAPS(static_cast<const float *>(f.image), f.a, W, H, x, y);
        stack_add(acc, c, transform_value(t, f.a, W, H), transform_live(t, W, H));
    }
    const size_t o = (size_t)y * OW + x;
    out[o] = c ? (MEAN ? acc / (float)c : acc) : empty;
    if (coverage) coverage[o] = c;
