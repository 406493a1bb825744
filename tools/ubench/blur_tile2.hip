// dev tool: tile shapes of the small-plane blur (k_pyramid.hpp: blur_tile2_kernel) against the 32 x 16 tile kernel
// (blur_hv_kernel) on one plane: bitwise equality of the outputs + time per launch, per tap count of a pyramid.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math -fhip-fp32-correctly-rounded-divide-sqrt \
//         -I sift_pyocl_amd/csrc tools/ubench/blur_tile2.hip -o tools/ubench/blur_tile2_bench
//   ./tools/ubench/blur_tile2_bench [W H]
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "k_pyramid.hpp"
using namespace siftk;

static std::vector<float> gauss(int n, float sigma) {
    std::vector<float> t(n);
    float s = 0;
    for (int i = 0; i < n; i++) { float x = (i - (n - 1) / 2.0f) / sigma; t[i] = expf(-x * x / 2); s += t[i]; }
    for (int i = 0; i < n; i++) t[i] /= s;
    for (int i = 0; i < n / 2; i++) t[n - 1 - i] = t[i];
    return t;
}
// time of one launch inside a train of `reps` back-to-back launches (as in a pyramid), best of 5 trains
template <class F> float timeit(F f, int reps = 20) {
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    f(); hipDeviceSynchronize();
    float best = 1e9;
    for (int rep = 0; rep < 5; rep++) {
        hipEventRecord(e0);
        for (int i = 0; i < reps; i++) f();
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        if (ms / reps < best) best = ms / reps;
    }
    hipEventDestroy(e0); hipEventDestroy(e1);
    return best * 1e3f;
}

static int W = 1024, H = 1024;
static float *d_in, *d_ref, *d_out;
static std::vector<float> h_ref, h_out;
static int failures = 0;

template <int N, int TX, int TY> void shape(const TapsArg<N> &ta) {
    using G = Tile2Geom<N, TX, TY>;
    dim3 grid((W + TX - 1) / TX, (H + TY - 1) / TY);
    auto run = [&] { hipLaunchKernelGGL((blur_tile2_kernel<N, false, 0, TX, TY>), grid, dim3(256), G::LDS_BYTES, 0, d_in, d_out, W, H, ta, nullptr, nullptr); };
    hipMemset(d_out, 0xff, (size_t)W * H * 4);
    run();
    hipMemcpy(h_out.data(), d_out, (size_t)W * H * 4, hipMemcpyDeviceToHost);
    const bool same = memcmp(h_out.data(), h_ref.data(), (size_t)W * H * 4) == 0;
    if (!same) failures++;
    printf("  tile2 %3dx%-3d  wgs %5u  LDS %5d B  %7.2f us  %s\n", TX, TY, grid.x * grid.y, G::LDS_BYTES, timeit(run), same ? "bit-exact" : "DIFFERS");
}

template <int N> void taps_case() {
    const std::vector<float> t = gauss(N, N / 8.0f);
    TapsArg<N> ta;
    for (int i = 0; i < N; i++) ta.t[i] = t[i];
    using G = BlurGeom<N, 32, 16>;
    dim3 grid((W + 31) / 32, (H + 15) / 16);
    auto ref = [&] { hipLaunchKernelGGL((blur_hv_kernel<N, false, 0, 32, 16, 4>), grid, dim3(256), G::LDS_BYTES, 0, d_in, d_ref, W, H, ta, nullptr, nullptr); };
    ref();
    hipMemcpy(h_ref.data(), d_ref, (size_t)W * H * 4, hipMemcpyDeviceToHost);
    printf("%d taps, %d x %d\n  hv    32x16   wgs %5u             %7.2f us\n", N, W, H, grid.x * grid.y, timeit(ref));
    shape<N, 32, 32>(ta); shape<N, 32, 64>(ta); shape<N, 32, 128>(ta);
    shape<N, 64, 32>(ta); shape<N, 64, 64>(ta); shape<N, 64, 128>(ta);
}

int main(int argc, char **argv) {
    if (argc >= 3) { W = atoi(argv[1]); H = atoi(argv[2]); }
    const size_t n = (size_t)W * H;
    std::vector<float> img(n);
    uint32_t x = 12345u;
    for (auto &v : img) { x = x * 1664525u + 1013904223u; v = (float)(x >> 8) * (255.0f / 16777216.0f); }
    h_ref.resize(n); h_out.resize(n);
    hipMalloc(&d_in, n * 4); hipMalloc(&d_ref, n * 4); hipMalloc(&d_out, n * 4);
    hipMemcpy(d_in, img.data(), n * 4, hipMemcpyHostToDevice);
    taps_case<11>(); taps_case<15>(); taps_case<17>(); taps_case<21>(); taps_case<27>();
    hipFree(d_in); hipFree(d_ref); hipFree(d_out);
    printf("%s\n", failures ? "FAILED" : "all shapes bit-exact");
    return failures ? 1 : 0;
}
