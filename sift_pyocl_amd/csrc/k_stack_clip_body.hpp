// k_stack_clip_body.hpp -- the body of stack_clip_kernel<REJECT> / stack_clip_cubic_kernel<REJECT>, included INSIDE the kernel definitions of k_stack_clip.hpp (no include guard on
// purpose: it is text, not declarations).  The legacy kernel and its cubic twin are this one text; the includer defines
//   STACK_BODY_TAPS_T   the taps of one frame (WarpTaps / CubicTaps)
//   STACK_BODY_TAPS     the function that loads them (transform_taps / cubic_taps)
//   STACK_BODY_DEPTH    frames whose taps are in flight together (SIFT_STACK_DEPTH / SIFT_STACK_DEPTH_CUBIC)
// and transform_value / transform_live are overloaded on the taps type (k_align.hpp, k_warp_cubic.hpp).  Why an include and not
// a `template <int INTERP> __device__ __forceinline__` body that both kernels call: that form was built first, and the extra
// inlining layer alone changed the legacy kernels' code (commuted s_and_b64 operands, one moved s_add in each unrolled group) --
// harmless, but no longer the parent's code instruction for instruction, which is what lets the legacy paths go unmeasured.
// After preprocessing, the legacy kernels' token stream is exactly what it was.
    extern __shared__ float stack_vals[];          // [S][256]
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
    if (x >= OW || y >= OH) return;
    float *col = stack_vals + threadIdx.y * 64 + threadIdx.x;
    uint64_t K = 0;
    float acc = 0.0f;                              // osum(v) over the live frames: the first SIGMA pass's
    int c = 0, s = 0;
    for (; s + STACK_BODY_DEPTH <= S; s += STACK_BODY_DEPTH) {
        WarpFrame f[STACK_BODY_DEPTH];
        STACK_BODY_TAPS_T t[STACK_BODY_DEPTH];
#pragma unroll
        for (int k = 0; k < STACK_BODY_DEPTH; k++) f[k] = frames[s + k];
#pragma unroll
        for (int k = 0; k < STACK_BODY_DEPTH; k++) t[k] = STACK_BODY_TAPS(static_cast<const float *>(f[k].image), f[k].a, W, H, x, y);
#pragma unroll
        for (int k = 0; k < STACK_BODY_DEPTH; k++) {
            const float v = transform_value(t[k], f[k].a, W, H);
            const bool live = transform_live(t[k], W, H);
            col[256 * (s + k)] = v;
            K |= (uint64_t)live << (s + k);
            stack_add(acc, c, v, live);
        }
    }
    for (; s < S; s++) {
        const WarpFrame f = frames[s];
        const STACK_BODY_TAPS_T t = STACK_BODY_TAPS(static_cast<const float *>(f.image), f.a, W, H, x, y);
        const float v = transform_value(t, f.a, W, H);
        const bool live = transform_live(t, W, H);
        col[256 * s] = v;
        K |= (uint64_t)live << s;
        stack_add(acc, c, v, live);
    }
    int n = c;
    if (REJECT == SIFT_STACK_TRIM) {
        if (c > 1) {
            const int h = min(p.n_high, c - 1), l = min(p.n_low, c - 1 - h);
            for (int i = 0; i < h; i++) {          // the largest (key, s) of K: among equal keys the last frame
                uint32_t best_key = 0;
                int best = 0;
                for (int j = 0; j < S; j++) {
                    const uint32_t k = stack_key(col[256 * j]);
                    if (((K >> j) & 1) && k >= best_key) { best_key = k; best = j; }
                }
                K &= ~((uint64_t)1 << best);
            }
            for (int i = 0; i < l; i++) {          // the smallest (key, s) of K: among equal keys the first frame
                uint32_t best_key = 0xffffffffu;
                int best = -1;
                for (int j = 0; j < S; j++) {
                    const uint32_t k = stack_key(col[256 * j]);
                    if (((K >> j) & 1) && (best < 0 || k < best_key)) { best_key = k; best = j; }
                }
                K &= ~((uint64_t)1 << best);
            }
            n = c - h - l;
        }
    } else {
        const float kl2 = p.kappa_low * p.kappa_low, kh2 = p.kappa_high * p.kappa_high;
        float sum = acc;
        for (int it = 0; it < p.iters && n >= 3; it++) {
            const float m = sum / (float)n;
            float q = 0.0f;
            bool first = true;
            for (int j = 0; j < S; j++) {
                const float d = col[256 * j] - m;
                const float dd = d * d;
                if ((K >> j) & 1) { q = first ? dd : q + dd; first = false; }
            }
            const float var = q / (float)n;
            const float tl = kl2 * var, th = kh2 * var;
            uint64_t gone = 0;
            float rest = 0.0f;                     // osum(v) over what stays: the next pass's
            int stay = 0;
            for (int j = 0; j < S; j++) {
                const float v = col[256 * j];
                const float d = v - m;
                const float dd = d * d;
                const bool in = (K >> j) & 1;
                const bool off = in && ((d < 0.0f && dd > tl) || (d > 0.0f && dd > th));
                gone |= (uint64_t)off << j;
                stack_add(rest, stay, v, in && !off);
            }
            if (gone == 0 || stay == 0) break;     // nothing to remove; or everything, which removes none
            K &= ~gone;
            n = stay;
            sum = rest;
        }
    }
    float r = empty;
    if (c) {
        float num = 0.0f, den = 0.0f;
        bool first = true;
        for (int j = 0; j < S; j++) {
            const float w = p.w[j];
            const float wv = w * col[256 * j];
            if ((K >> j) & 1) { num = first ? wv : num + wv; den = first ? w : den + w; first = false; }
        }
        r = num / den;
    }
    const size_t o = (size_t)y * OW + x;
    out[o] = r;
    if (coverage) coverage[o] = c;
    if (kept) kept[o] = c ? n : 0;
