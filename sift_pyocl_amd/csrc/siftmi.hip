// siftmi.hip -- host side of libsiftmi.so: the C ABI of include/siftmi.h over the gfx950 kernels.
//
// One plan = one HIP device + one stream + every buffer pre-allocated (as SiftPlan.__init__ does,
// sift-src/plan.py:117-201,268-306).  keypoints() enqueues the whole pyramid / detection /
// description chain without reading anything back and synchronises once at the end; the
// reference's host loop (plan.py:596-756) reads a 4-byte counter back >= 18 times per octave.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <chrono>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "host_common.hpp"
#include "k_extrema.hpp"
#include "k_keypoint.hpp"
#include "k_descriptor.hpp"
#include "k_align.hpp"
#include "k_align_batch.hpp"
#include "k_warp_cubic.hpp"
#include "k_stack.hpp"
#include "k_stack_clip.hpp"
#include "k_stack_accum.hpp"
#include "k_pyramid.hpp"
#include "k_tail.hpp"
#include "k_top_patch.hpp"
#include "siftmath.hpp"

using namespace siftk;

static_assert(sizeof(siftmi_keypoint) == 144, "siftmi_keypoint must be 144 bytes");

namespace {

// Events that order one stream of a plan behind another ON THE SAME DEVICE, kernel to kernel: no timing, and no system-scope fence when they are
// recorded.  INVARIANT: producer and consumer of such an event are kernels on this device (ev_pyr, ev_p3, ev_maps0).  Anything whose
// consumer is a DMA copy, the host or another device -- the upload ring's events, the events bracketing a profile -- uses plain events.
// (The kernels' own agent-scope release / acquire at their boundaries is what the consumers need; nothing the host or another
// device reads is ordered by these events -- results are waited for through the streams themselves.)
#ifndef SIFT_SYNC_EVENT
#define SIFT_SYNC_EVENT (hipEventDisableTiming | hipEventDisableSystemFence)
#endif
#define SIFTMI_ETAILRETRY (-100)   // internal: plan_wait -> siftmi_plan_keypoints, never returned through the C ABI
#define SIFTMI_EGROW (-101)        // internal, likewise: a list was grown, the image has to run again

// ---- Gaussian taps on the host: gaussian.cl:56-140 run as one work-group of nextpower(size)
// items (plan.py:321-330); LDS tree sum restated serially in the same association order.
int nextpower(int n) { int p = 1; while (p < n) p <<= 1; return p; }

int gaussian_taps(float sigma, int size, float *out) {
    if (size < 1 || size > 1024) return fail(SIFTMI_EINVAL, "gaussian size %d out of range", size);
    int P = nextpower(size);
    if (P < 2) P = 2;
    std::vector<float> g((size_t)P, 0.0f), sum((size_t)P, 0.0f);
    const float norm = sqrtf(2.0f * SM_PI_F);
    for (int i = 0; i < size; i++) {
        const float x = ((float)i - ((float)size - 1.0f) / 2.0f) / sigma;
        const float y = siftmath::expf_(-x * x / 2.0f);
        g[(size_t)i] = y / sigma / norm;
        sum[(size_t)i] = g[(size_t)i];
    }
    for (int stride = 512; stride >= 2; stride >>= 1)
        if (size > stride)
            for (int i = 0; i < stride && i + stride < P; i++) sum[(size_t)i] += sum[(size_t)(i + stride)];
    sum[0] += sum[1];
    for (int i = 0; i < size; i++) out[i] = g[(size_t)i] / sum[0];
    return SIFTMI_OK;
}

int kernel_size(double sigma) {   // utils.py:54-64 with odd=True, cutoff=4
    int size = (int)std::ceil(2.0 * 4.0 * sigma + 1.0);
    if (size % 2 == 0) size += 1;
    return size;
}

struct Taps { int n = 0; float t[64] = {0}; float *dev = nullptr; };

// Largest "ori_pad" / "desc_pad" (bytes of dynamic LDS added to each workgroup of the orientation / descriptor launch): with
// the kernels' static LDS (12.5 KiB / 34 KiB) a workgroup still fits the 160 KiB of a CU; a larger pad would fail the launch.
#define SIFT_LDS_PAD_MAX 65536

// Per-plan tuning / diagnostic options (siftmi_plan_set_option).  Defaults are the measured best; nothing on the launch
// path reads the environment.
struct Options {
    int fused_convert = 1;   // typed frames converted at the point of use (0: separate convert pass)
    int overlap = 1;         // detection / description streams beside the pyramid stream (0: one stream)
    int march = 1;           // marching blur for large planes (0: tiled blur everywhere)
    int small_blur = 2;      // planes below the marching cross-over with symmetric odd taps: 0 the 32 x 16 tile kernel (blur_hv_kernel),
                             // 1 the 32 x 32 / 32 x 64 tile kernel (blur_tile2_kernel), 2 by plane size (tile2_plane).  No option name:
                             // siftmi_plan_set_option does not know it, only siftmi_stage_blur_ex sets it (bits 2-3 of its xcd_map)
    int march_wgs = 0;       // workgroups wanted by the marching blur (0: 1024, 768 for 27 taps)
    int xcd_map = 1;         // marching blur: whole segment rows per XCD (k_pyramid.hpp: the strips' halo columns become L2 hits)
    int march_prio = 1;      // marching blur: wave priority falls by one level per quarter of a workgroup's march, so that the workgroups of a CU
                             // advance together instead of oldest first (k_pyramid.hpp: set_prio): 0 never, 1 by launch_team's rule, 2 every launch
    int ori_blocks = 4096, ori_pad = 0;      // orientation launch: workgroups (upper bound; the kernel cuts it down by the group's count)
    // descriptor launch: workgroups (keypoints are handed out dynamically, so a workgroup stays until the group is done:
    // 1024 = every wave slot of the chip, which starves the other stream's kernels for the whole launch -- 1024^2 smooth
    // frame 0.760 ms, with 896-960 workgroups 0.671; 2048^2 smooth 1.85 -> 1.73), bytes of dynamic LDS (residency throttle)
    int desc_blocks = 960, desc_pad = 0;
    int desc_small_blocks = 576;   // ... and for groups of fewer than 16384 (the later octaves' chain needs the room)
    int desc_dense_blocks = 960;   // ... and for groups of >= 65536 keypoints (lazy-gradient form; the MAPS form always takes desc_blocks).  Round 3: 832
                                   // (704: 5.47 ms per 154 k-keypoint call, 768-896: 5.27, 960: 5.31); round 4, with 2 KB less LDS per workgroup and the
                                   // row look-ahead: 832 / 896 / 960 -> 154 k keypoints without maps 4.56 / 4.49 / 4.42 ms, 16384^2 10.64 / 10.55 / 10.50
    int desc_stream = 0;     // 1: force the streaming form of the descriptor kernel (any window size)
    // Full gradient maps (gradient_maps_kernel) for the per-keypoint kernels: 0 never, 1 always, 2 when the previous image
    // of this plan had at least one oriented keypoint per `maps_density` pixels in the group (octave 0 / the later octaves).
    // Same records either way (tests/test_gpu_params.py); the maps pay from about one keypoint per 250 pixels (4096^2: 0.18 ms for octave 0 against 2.6 ns saved per keypoint).
    int maps = 2, maps_density = 200;
    int maps_blocks = 8192;  // workgroups of gradient_maps_kernel (grid stride over 256 x 32 pixel items)
    int mm_blocks = 256;     // few, fat workgroups: every block ends with two atomics on the same cache line
    int mm_threads = 1024;   // threads per workgroup of the f32 min/max pass: sixteen waves per workgroup = four per SIMD at the same 256 atomic pairs
                             // (256 threads: one wave per SIMD; three interleaved A/B runs 0.7924-0.7934 -> 0.7863-0.7876 ms, 512^2 0.2561 -> 0.2531)
    int desc_team = 2048;    // groups with fewer oriented keypoints than this are described by the workgroup-per-keypoint form (0: never); measured cross-over
                             // 1000-1800 alone (one workgroup slot per keypoint: 4 per CU); in a frame, round 4 (interleaved A/B, 1024 / 2048 / 3072 / 4096):
                             // 1024^2 smoothed 0.588 / 0.568 / 0.568 / 0.570 ms, 2048^2 white 0.500 / 0.499 / 0.520 / 0.521, headline and the other frames equal
    int fork = 2;            // the later octaves in two chains: octave 1 (detection to description, group 1) on `stream3`, the octaves below it
                             // (pyramids from octave 1's plane 3 on, the tail launch, group 2) on `stream2`.  0: one chain, one group; 1: always;
                             // 2: frames of at least five octaves.  Interleaved A/B, forked against one chain (white noise unless noted): 512^2
                             // 0.205 / 0.249 ms, 1024^2 0.281 / 0.328, 2048^2 0.450 / 0.508, 4096^2 with 9 / 5 / 4 / 3 octaves 0.943 / 0.956,
                             // 0.852 / 0.868, 0.830 / 0.833, 0.821 / 0.789 (three octaves: two sparse groups each pay a launch chain beside
                             // octave 0's descriptors), 16384^2 10.46 / 10.48; smoothed noise 4096^2 4.45 / 4.38, 2048^2 1.45 / 1.49
    int split = 0;           // (when the chain does not fork) the pyramids and detection of the octaves below octave 1 on `stream2` from octave 1's plane 3
                             // on, beside octave 1's last blurs and detection, into the SAME group: one orientation / descriptor launch for all later octaves
    int early_chain = 2;     // the later octaves' chain starts when plane 3 of octave 0 exists (behind its third blur: octave 1's plane 0 rides on
                             // that launch), not behind its fifth: 0 never, 1 always, 2 unless the previous image of the plan was keypoint-rich
                             // (one keypoint per `maps_density` pixels of octave 0).  Round 3 measured this slower (0.854 -> 0.894 ms): the later
                             // octaves' detection then still had to wait for octave 0's orientation pass (one shared list).  With a list per
                             // group the chain runs through: its pyramids share the chip with octave 0's last two blurs instead of with its
                             // descriptor launch, whose workgroups starve them of registers (blur_hv 21 / 27 taps on a 1024^2 plane: 83 / 115 us
                             // beside 768 descriptor workgroups, 10 / 11 alone).  Interleaved A/B, early against late: 512^2 0.194 / 0.205 ms,
                             // 1024^2 0.259 / 0.281, 2048^2 0.425 / 0.453 (3 octaves: 0.367 / 0.388), 4096^2 with 9 / 4 octaves 0.891-0.900 /
                             // 0.926, 0.817 / 0.841, with 3 (the headline) 0.785-0.799 / 0.789-0.794 (hence: not on >= 8 Mpixel frames of three
                             // octaves); smoothed noise 4096^2 4.42 / 4.26 (hence the density rule), 2048^2 1.39 / 1.38, 1024^2 0.576 / 0.596
    int desc_early_blocks = 704;   // descriptor workgroups of a small octave 0 when the later octaves started early (they are nearly done by
                                   // then: 576 leaves room nobody needs, 960 starves what is left; 640 / 704 / 768 / 832: 0.797 / 0.785 / 0.788-0.799 / 0.801)
    int fused_refine = 1;    // detection and refinement in one launch: 0 never, 1 planes below 1400^2, 2 every plane
    // The top plane (plane 5) only around scale-3 candidates: octaves whose detection keeps a candidate list skip the blur launch
    // that writes plane 5, run the lazy extrema instance and top_patch_kernel (k_top_patch.hpp).  0 never, 1 always, 2 when the
    // previous image of this plan left fewer than one scale-3 candidate per `lazy_density` pixels in that octave (a plan's first
    // image is eager).  Same records either way.  lazy_density: DESIGN_APPENDIX, "Lazy top plane: the density sweep".  Set
    // through siftmi_plan_set_lazy_top.
    int lazy_top = 2, lazy_density = 6000;
    int top_blocks = 8192;   // workgroups (waves) of top_patch_kernel: one list entry each, grid stride
    int fused_shrink = 1;    // octave hand-off inside the blur launch that writes plane 3 (512^2 frame -4 %, 2048^2 -4 %, 4096^2 +-0)
    int ori_team = 1024;     // groups with fewer refined keypoints than this: a workgroup per keypoint in the orientation launch (0: never)
    int desc_dynamic = 1;    // wave-per-keypoint form: keypoints beyond each wave's first are handed out through a device counter
    int tail_pixels = SIFT_TAIL_MAX_PIXELS;   // largest plane (W * H) the tail kernel takes
    int tail = 1;            // small octaves (<= 64 x 64) in one launch (octave_tail_kernel)
    int ext_rows = 0;        // rows per extrema strip: 0 by plane size (extrema_strip_rows)
    int ext_strips = 2000;   // ... which halves the 64-row strips until at least this many of them cover the plane.  Round 2 used 12288 (16-row
                             // strips on a 4096^2 plane): the march of a strip re-reads two halo rows, and many short strips are many
                             // ramp-ups; interleaved A/B, whole call: 4096^2 0.835 (12288) / 0.823 (4000) / 0.809 (2000) / 0.817 ms (1000),
                             // 2048^2 0.521 -> 0.511, 2048^2 smoothed 1.544 -> 1.517, small frames unchanged; the launch alone 94 -> 81-86 us
    int ori_small_blocks = 608;   // orientation launch: workgroups used for a group of fewer than 16384 keypoints (512 until the descriptor launch was ordered: 0.809 ms; 576-640: 0.799-0.801; 704: 0.813)
    int spin = 1;            // poll the ending streams instead of a blocking wait
    int host_timing = 0;     // print the host time of plan_enqueue
    int tail_fault = 0;      // diagnostic: the next `tail_fault` images that go through octave_tail_kernel are treated as if a
                             // workgroup of it had timed out (exercises the host's re-run path; results do not change)
};
const Options g_default_options{};

struct Event { std::string label; hipEvent_t a = nullptr, b = nullptr; bool is_blur = false; double pixels = 0; int octave = -1; int launches = 1; };

size_t dtype_size(int dt) {
    switch (dt) {
        case SIFTMI_F32: return 4; case SIFTMI_U8: return 1; case SIFTMI_U16: return 2; case SIFTMI_U32: return 4;
        case SIFTMI_U64: return 8; case SIFTMI_I32: return 4; case SIFTMI_I64: return 8; case SIFTMI_F64: return 8;
        case SIFTMI_RGB8: return 3;
    }
    return 0;
}

}  // namespace

// The lists of one group of octaves (k_keypoint.hpp: Counters): candidates, refined keypoints, oriented keypoints.  Capacities start at kpsize (plan.py:243) and grow on demand (grow_lists).
struct GroupLists {
    float4 *kp = nullptr;  int *kp_aux = nullptr;  int64_t cap_kp = 0;     // (peak, row, col, sigma), detection scale | octave << 8
    float4 *okp = nullptr; int *oaux = nullptr;    int64_t cap_out = 0;    // (x, y, scale, angle), same tag
    float4 *cand = nullptr; int64_t cap_cand = 0;                           // candidate list of the group's detection passes (one octave at a time)
};

struct siftmi_plan {
    void *chain = nullptr;        // open light-profile bracket (a Scope, profile == 1)
    int device = 0;
    hipStream_t stream = nullptr;
    int H = 0, W = 0, dtype = 0;
    siftmi_params par{};
    Options opt;
    int profile = 0;
    int n_oct = 0;
    std::vector<int> ow, oh;
    int64_t kpsize = 0;
    int64_t bytes = 0;
    float *planes = nullptr;      // all octaves' blur planes: octave o, scale s at plane(o, s)
    std::vector<size_t> oct_off;  // float offset of octave o's first plane
    float *tmp = nullptr;         // generic two-pass blur only (tap counts without a fused kernel): intermediate plane
    float *tmp_later = nullptr;   // ... of octave 1's chain, which may run beside octave 0's last two blurs (early_chain),
    float *tmp_below = nullptr;   // ... of the chain of the octaves below octave 1, which runs beside octave 1's last blurs
    hipStream_t stream2 = nullptr;            // octave 0's gradient maps; the octaves below octave 1 (pyramids, detection, the tail launch, description)
    hipStream_t stream3 = nullptr;            // octave 1 (pyramid, detection, description) -- or every later octave when they form one chain
    int64_t acc_calls = 0, acc_b0_launches = 0;   // running totals of the light profile (siftmi_plan_profile_totals)
    double acc_total_ms = 0, acc_b0_ms = 0, acc_b0_pixels = 0;
    hipEvent_t ev_early = nullptr;
    hipEvent_t ev_p3 = nullptr;               // plane 3 of octave 1 (and octave 2's plane 0) exist: the chain of the octaves below starts there
    std::vector<hipEvent_t> ev_pyr;           // pyramid of octave o complete (recorded on `stream`)
    bool overlap = true;
    float *plane(int o, int s) const { return planes + oct_off[(size_t)o] + (size_t)s * (size_t)ow[(size_t)o] * (size_t)oh[(size_t)o]; }
    void *raw = nullptr;          // host-input staging (any dtype)
    int raw_dtype = -1;           // dtype of the image currently staged in `raw` (-1: none)
    Counters *cnt_pair = nullptr;  // the two counter blocks (`cnt` points at the one of the image in flight)
    int cnt_parity = 0;
    hipStream_t fin = nullptr;    // stream on which the last enqueued image ends
    int last_group0 = 0;          // oriented keypoints of octave 0 in the previous image (occupancy heuristic)
    int last_group1 = 0;          // ... of the later octaves
    float *gmap = nullptr, *omap = nullptr;   // gradient maps (allocated on first use: half the size of `planes` each)
    size_t planes_floats = 0;
    bool maps_g0 = false, maps_g1 = false;    // the image being enqueued: MAPS forms for octave 0 / the later octaves (groups 1 and 2)
    // the image being enqueued / waited for
    bool early_cur = false;                   // the later octaves' chain started at plane 3 of octave 0
    bool split_cur = false;                   // the octaves below octave 1 are built and searched on stream2, octave 1's candidates sit in group 1's buffer (option "split")
    hipEvent_t ev_det2 = nullptr;             // ... and this is the end of their detection
    bool fork_cur = false;                    // octave 1 is a group of its own (1), the octaves below it group 2; else all later octaves in group 2
    unsigned groups_cur = 0;                  // bit g: group g has launches in this image
    int tail_first_cur = 0;                   // first octave of the tail launch (n_oct: none)
    hipEvent_t ev_maps0 = nullptr;
    bool maps_unavailable = false;   // the lazy allocation of the gradient maps failed once: dense frames keep the lazy forms
    hipEvent_t ev_join = nullptr;
    struct HostBack { Counters c[3]; } *hb = nullptr;    // pinned read-back blocks (one asynchronous D->H per ending stream)
    hipStream_t wait_s[3] = {nullptr, nullptr, nullptr}; // the streams the image enqueued last ends on (hb->c[k] was copied on wait_s[k])
    void *warp_in = nullptr, *warp_out = nullptr;   // siftmi_plan_transform staging, grown on demand
    size_t warp_in_bytes = 0, warp_out_bytes = 0;
    hipEvent_t ev_wa = nullptr, ev_wb = nullptr;
    float *conv = nullptr;        // converted f32 input when dtype != f32
    uint32_t *mm = nullptr;
    Counters *cnt = nullptr;
    float4 *tail_cand = nullptr;   // candidate lists of octave_tail_kernel: SIFT_TAIL_MAX_OCT x tail_cand_cap
    int tail_cand_cap = 0;
    GroupLists grp[SIFT_GROUPS];
    KpRecord *records = nullptr;  // the image's records: one block per group (descriptor_reserve)
    int64_t cap_rec = 0;
    bool in_flight = false;       // an image has been enqueued and not yet waited for (plan_wait) or drained
    bool records_cut = false;     // the last image hit the reference's per-octave capacity and was cut to it (cap_octaves): a pinned result array is stale
    int64_t grows = 0;            // list growths since creation (each one ran its image again)
    int64_t tail_timeouts = 0;    // images whose tail launch gave up waiting for the octave above and ran again (0 or 1: the plan then drops the tail launch)
    KpRecord *host_out = nullptr; // pinned result array of the call being enqueued (zero-copy delivery), or null
    int host_cap = 0;
    bool desc_rows = true;        // descriptor windows fit the row tables of descriptor_kernel (R <= SIFT_DESC_MAXRAD for this init_sigma)
    Taps taps[6];                 // [0..4] per-octave schedule, [5] initial blur
    bool have_init = false;
    std::vector<Event> events;
    size_t n_events = 0;
    hipEvent_t ev_first = nullptr, ev_last[3] = {nullptr, nullptr, nullptr};
    float last_min = 0, last_max = 0;
    int64_t last_count = 0;
    int last_overflow = 0;
    // host integers of the last finished call (siftmi_plan_last_counts), copied from the complete read-back of its counters
    bool last_valid = false;                  // a call has finished and none has been enqueued or failed since
    int last_tail_first = 0;                  // tail_first_cur of the run that produced the result
    int last_n_cand[SIFT_MAX_OCTAVES] = {0};
    int last_c_scale[SIFT_MAX_OCTAVES][3] = {{0}};
    // lazy top plane (option "lazy_top"): the octaves of the image being enqueued / of the last finished call whose plane 5 holds
    // patches only (siftmi_plan_planes completes it); a call has finished on this plan (the auto rule has counts to go by);
    // the image in flight outran a candidate list with provisional entries in it and runs again eagerly
    bool lazy_cur[SIFT_MAX_OCTAVES] = {false}, lazy_last[SIFT_MAX_OCTAVES] = {false}, lazy_ran[SIFT_MAX_OCTAVES] = {false};
    bool lazy_seen = false, lazy_block = false;
    std::vector<void *> allocs;

    template <class T> int alloc(T **p, size_t nbytes) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, nbytes ? nbytes : 16);
        if (e != hipSuccess) return fail(SIFTMI_ENOMEM, "hipMalloc(%zu bytes): %s", nbytes, hipGetErrorString(e));
        allocs.push_back(q);
        bytes += (int64_t)nbytes;
        *p = (T *)q;
        return SIFTMI_OK;
    }
    // a buffer that may be replaced by a larger one later (not in `allocs`: freed by its owner)
    template <class T> int regrow(T **p, size_t old_bytes, size_t new_bytes) {
        void *q = nullptr;
        hipError_t e = hipMalloc(&q, new_bytes ? new_bytes : 16);
        if (e != hipSuccess) return fail(SIFTMI_ENOMEM, "hipMalloc(%zu bytes): %s", new_bytes, hipGetErrorString(e));
        if (*p) { (void)hipFree(*p); bytes -= (int64_t)old_bytes; }
        bytes += (int64_t)new_bytes;
        *p = (T *)q;
        return SIFTMI_OK;
    }
};

namespace {

int compute_schedule(siftmi_plan *p) {
    // plan.py:534-539 (initial blur) and plan.py:602-618 (per-octave increments)
    const double init_sigma = p->par.init_sigma;
    p->have_init = false;
    // largest descriptor window: sigma <= init_sigma * 2^((3 + 1.5) / 3) (image.cl:354, |offset| <= 1.5), spacing = 3 sigma,
    // R = (int)(1.414 * spacing * 2.5 + 0.5) (keypoints_cpu.cl:57-62); two rows of slack for float rounding
    p->desc_rows = (int)(1.414 * 3.0 * init_sigma * std::pow(2.0, 1.5) * 2.5 + 0.5) + 2 <= SIFT_DESC_MAXRAD;
    const double cur_sigma = p->par.double_im_size ? 1.0 : 0.5;   // par.DoubleImSize (plan.py:534)
    if (init_sigma > cur_sigma) {
        const double s = std::sqrt(init_sigma * init_sigma - cur_sigma * cur_sigma);
        p->taps[5].n = kernel_size(s);
        if (p->taps[5].n > 64) return fail(SIFTMI_EINVAL, "init_sigma %g needs %d taps (> 64)", init_sigma, p->taps[5].n);
        int rc = gaussian_taps((float)s, p->taps[5].n, p->taps[5].t);
        if (rc) return rc;
        p->have_init = true;
    }
    const double ratio = std::pow(2.0, 1.0 / 3.0);   // SiftPlan.sigmaRatio, par.Scales == 3
    double prev = init_sigma;
    for (int s = 0; s < 5; s++) {
        const double inc = prev * std::sqrt(ratio * ratio - 1.0);
        p->taps[s].n = kernel_size(inc);
        if (p->taps[s].n > 64) return fail(SIFTMI_EINVAL, "sigma %g needs %d taps (> 64)", inc, p->taps[s].n);
        int rc = gaussian_taps((float)inc, p->taps[s].n, p->taps[s].t);
        if (rc) return rc;
        prev *= ratio;
    }
    for (int s = 0; s < 6; s++) {
        if (!p->taps[s].dev) { int rc = p->alloc(&p->taps[s].dev, 64 * sizeof(float)); if (rc) return rc; }
        HIPCHK(hipMemcpy(p->taps[s].dev, p->taps[s].t, 64 * sizeof(float), hipMemcpyHostToDevice));
    }
    return SIFTMI_OK;
}

// A launch whose completion IS an event (`stop` not null: hipExtLaunchKernelGGL binds the event to the dispatch's own
// completion signal) instead of a launch followed by hipEventRecord, which puts a barrier packet of its own into the queue:
// between two 20 us kernels of one stream 2.3 us instead of 3.9 (fence-free event) / 5.3-6.6 (timing event), against 1.3 us
// with no event at all; a stream waiting for the event starts 7.8 us after the producer's end instead of 9.6 / 11.7
// (tools/ubench/ext_event.hip).  hipEventElapsedTime between two bound events is end of the first launch -> end of the
// second (tools/ubench/ext_event2.hip): the light profile's bracket.
template <typename K, typename... A>
inline void launch_ev(hipEvent_t stop, K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t st, A... args) {
    if (stop) hipExtLaunchKernelGGL(kernel, grid, block, (uint32_t)lds, st, nullptr, stop, 0u, args...);
    else hipLaunchKernelGGL(kernel, grid, block, lds, st, args...);
}

// Which kernel ran a blur (the stage entry point reports it): none (no fused instance for the tap count), the 32 x 16 tile
// kernel, the marching team kernel, the small-plane tile kernel (blur_tile2_kernel).
enum BlurForm { BLUR_NONE = 0, BLUR_TILE = 1, BLUR_TEAM = 2, BLUR_TILE2 = 3 };

// blur_tile2_kernel takes a plane (below the marching cross-over) when its taps are bitwise symmetric and
// Options::small_blur asks for it: 1 always, 2 from TILE2_MIN_PIXELS on.  32 x 64 tiles from TILE2_TALL_PIXELS on, 32 x 32 below.
// Alone (tools/ubench/blur_tile2.hip, 11 / 15 / 17 / 21 / 27 taps) against the 32 x 16 tile kernel: 1024^2 32 x 64 6.1 / 6.5 / 6.8 /
// 7.5 / 8.2 us against 7.1 / 8.4 / 8.8 / 11.1 / 15.6 (64 x 64: 256 workgroups, 7.4 - 10.0); 600^2 32 x 32 4.8 / 5.1 / 5.4 / 5.9 / 6.7
// against 4.7 / 5.4 / 5.7 / 6.8 / 8.4; 512^2 a tie up to 17 taps, and whole 512^2 frames measured no faster: they keep the old kernel.
constexpr int64_t TILE2_MIN_PIXELS = 600 * 600;
constexpr int64_t TILE2_TALL_PIXELS = 1024 * 1024;
inline bool tile2_plane(const Options &opt, int W, int H, bool symmetric) {
    return symmetric && (opt.small_blur == 1 || (opt.small_blur == 2 && (int64_t)W * H >= TILE2_MIN_PIXELS));
}

// Tile shape: planes that reach this kernel are narrower than 1024 columns or shorter than 512 rows (larger ones take the
// marching kernel); on all of them the 32 x 16 tile measured fastest (whole call, MI355X, round 2: 512^2 0.75 / 0.52 / 0.44 ms
// and 1020^2 0.90 / 0.63 / 0.53 ms for 128x64 / 64x32 / 32x16 tiles).
template <int N, bool NORM, int DT = 0>
BlurForm launch_blur_t(const Options &opt, hipStream_t st, const void *in, float *out, int W, int H, const float *taps, bool symmetric,
                       const uint32_t *mm, float *half = nullptr, hipEvent_t stop = nullptr) {
    TapsArg<N> ta;
    for (int i = 0; i < N; i++) ta.t[i] = taps[i];
    auto tiles = [&](auto kernel, int TX, int TY, size_t lds) {      // one workgroup per TX x TY tile
        launch_ev(stop, kernel, dim3((unsigned)((W + TX - 1) / TX), (unsigned)((H + TY - 1) / TY)), dim3(256), lds, st, in, out, W, H, ta, mm, half);
    };
    if (tile2_plane(opt, W, H, symmetric)) {
        if ((int64_t)W * H >= TILE2_TALL_PIXELS) tiles(blur_tile2_kernel<N, NORM, DT, 32, 64>, 32, 64, Tile2Geom<N, 32, 64>::LDS_BYTES);
        else tiles(blur_tile2_kernel<N, NORM, DT, 32, 32>, 32, 32, Tile2Geom<N, 32, 32>::LDS_BYTES);
        return BLUR_TILE2;
    }
    tiles(blur_hv_kernel<N, NORM, DT, 32, 16, 4>, 32, 16, BlurGeom<N, 32, 16>::LDS_BYTES);
    return BLUR_TILE;
}

// team form of the marching blur (blur_team_kernel): S sub-blocks per accumulator period, `wgs` workgroups wanted.
// A segment (grid row) outputs rows_out = ceil(H / segments) rows and marches rows_out + N - 1 rows rounded up to whole
// sub-blocks (nblocks - 1 full periods + last_subs sub-blocks), so the workgroup count is the one asked for -- 768 for
// 27 taps on a 4096^2 plane, 3 per CU -- instead of one quantised by segment heights in multiples of N rows (608: 2.4 per CU).
template <int N, bool NORM, int S, int DT = 0>
void launch_team(const Options &opt, hipStream_t st, const void *in, float *out, int W, int H, const float *taps, const uint32_t *mm, int wgs, float *half, hipEvent_t stop) {
    using G = March2Geom<N, 128, S>;
    using SS = SubSplit<N, S>;
    TapsArg<N> ta;
    for (int i = 0; i < N; i++) ta.t[i] = taps[i];
    if (opt.march_wgs > 0) wgs = opt.march_wgs;
    const int gx = (W + G::TX - 1) / G::TX;
    int gy = wgs / gx;
    if (gy < 1) gy = 1;
    if (gy > H) gy = H;
    int rows_out = (H + gy - 1) / gy;
    if (rows_out < 2 * N + 1) rows_out = 2 * N + 1;     // small planes: at most one third of the marched rows is warm-up
    gy = (H + rows_out - 1) / rows_out;
    // rows marched by b full periods + m sub-blocks of the next one
    auto covered = [](int b, int m) { int r = b * N; for (int q = 0; q < m; q++) r += SS::rows(q); return r; };
    const int need = rows_out + N - 1;
    const int b = need / N;
    int m = 0;
    while (covered(b, m) < need) m++;                // m <= S
    const int nblocks = b + (m > 0 ? 1 : 0), last_subs = m > 0 ? m : S;
    dim3 grid((unsigned)gx, (unsigned)gy);
    // priority feedback (k_pyramid.hpp: set_prio), option march_prio: 1 = where a CU holds about three or more workgroups of the
    // launch (704 of them: the workgroups of a CU then advance together instead of oldest first), 2 = every launch (launch_blur
    // asks for it on the later octaves' chains, whose launches run beside octave 0's per-keypoint kernels and end the frame:
    // their waves outrank those), 0 = never.  Interleaved A/B, whole calls, off -> on: 4096^2 with 3 / 9 octaves 0.800 -> 0.766 /
    // 0.903 -> 0.865 ms, 3000^2 0.624 -> 0.610, 16384^2 10.47 -> 10.2 (its full-resolution launches 597 -> 530 us), smoothed
    // 4096^2 4.28 -> 4.22.  Octave 0 of a 2048^2 frame (536 workgroups) loses 3 % with it and keeps the arbiter's order.
    const int prio = (opt.march_prio == 2 || (opt.march_prio == 1 && gx * gy >= 704)) ? 1 : 0;
    launch_ev(stop, blur_team_kernel<N, NORM, S, DT>, grid, dim3(256), (size_t)3 * G::LDS_BYTES, st, in, out, W, H, nblocks, last_subs,
              rows_out, ta, mm, half, opt.xcd_map, prio);
}

// Large planes: the team form, with the sub-block count and workgroup count that measured best per tap count on a 4096^2
// plane (tools/ubench/blur_team.hip: 31 / 38 / 41 / 47 / 65 us against 33 / 43 / 45 / 53 / 73 us for the one-block form of round 1).
// returns whether `half` (the fused octave hand-off) was written
template <int N, bool NORM, int DT = 0>
bool launch_march_t(const Options &opt, hipStream_t st, const void *in, float *out, int W, int H, const float *taps, const uint32_t *mm, float *half = nullptr, hipEvent_t stop = nullptr) {
    constexpr int S = (N <= 15) ? 2 : (N <= 21 ? 3 : 4);
    launch_team<N, NORM, S, DT>(opt, st, in, out, W, H, taps, mm, N >= 27 ? 768 : 1024, half, stop);
    return half != nullptr;
}

// The marching kernels amortise their prologue over long strips; measured cross-over with the 32 x 16 tile kernel
// is near 1400^2 (whole call 0.607 vs 0.609 ms; 1024^2 0.555 vs 0.529, 2048^2 0.732 vs 0.779).
inline bool march_plane(int W, int H) { return W >= 1024 && H >= 512 && (int64_t)W * H >= 1400 * 1400; }

bool taps_symmetric(const Taps &t) {
    bool symmetric = true;
    for (int i = 0; i < t.n / 2; i++) symmetric = symmetric && (memcmp(&t.t[i], &t.t[t.n - 1 - i], 4) == 0);
    return symmetric;
}

// One fused blur of N taps: the marching team kernel for the large planes (symmetric taps, option "march"), else a tile kernel.
template <int N, bool NORM, int DT = 0>
BlurForm launch_blur_n(const Options &opt, hipStream_t st, const void *in, float *out, int W, int H, const Taps &t, const uint32_t *mm, float *half = nullptr, hipEvent_t stop = nullptr) {
    const bool symmetric = taps_symmetric(t);
    if (march_plane(W, H) && symmetric && opt.march) { launch_march_t<N, NORM, DT>(opt, st, in, out, W, H, t.t, mm, half, stop); return BLUR_TEAM; }
    return launch_blur_t<N, NORM, DT>(opt, st, in, out, W, H, t.t, symmetric, mm, half, stop);
}

// returns the kernel launched (BlurForm; BLUR_NONE when no fused instantiation exists for this tap count).  Every fused form
// writes `half` when it is not null.
template <bool NORM>
BlurForm launch_blur_tiled(const Options &opt, hipStream_t st, const float *in, float *out, int W, int H, const Taps &t, const uint32_t *mm, float *half = nullptr, hipEvent_t stop = nullptr) {
    if constexpr (NORM) {
        // The normalising form exists for the default initial kernel only (15 taps, init_sigma = 1.6); any other
        // InitSigma sends its ONE initial blur through the generic two-pass path (BLUR_NONE).
        return t.n == 15 ? launch_blur_n<15, NORM>(opt, st, in, out, W, H, t, mm, half, stop) : BLUR_NONE;
    } else {
    switch (t.n) {
        case 11: return launch_blur_n<11, NORM>(opt, st, in, out, W, H, t, mm, half, stop);
        case 15: return launch_blur_n<15, NORM>(opt, st, in, out, W, H, t, mm, half, stop);
        case 17: return launch_blur_n<17, NORM>(opt, st, in, out, W, H, t, mm, half, stop);
        case 21: return launch_blur_n<21, NORM>(opt, st, in, out, W, H, t, mm, half, stop);
        case 27: return launch_blur_n<27, NORM>(opt, st, in, out, W, H, t, mm, half, stop);
        default: return BLUR_NONE;
    }
    }
}

void launch_blur_generic(hipStream_t st, const float *in, float *out, float *tmp, int W, int H, const Taps &t,
                         const uint32_t *mm, bool norm) {
    dim3 grid((unsigned)((W + 255) / 256), (unsigned)H);
    hipLaunchKernelGGL(blur_generic_pass, grid, dim3(256), 0, st, in, tmp, W, H, t.dev, t.n, 0, mm, norm ? 1 : 0);
    hipLaunchKernelGGL(blur_generic_pass, grid, dim3(256), 0, st, (const float *)tmp, out, W, H, t.dev, t.n, 1, mm, 0);
}

// `half` not null: the launch may also write out[2y][2x] there (the next octave's plane 0); returns whether it did
// `stop` not null: the event is complete when the blur is (bound to the launch, launch_ev; recorded behind the two-pass form)
bool launch_blur(siftmi_plan *p, const float *in, float *out, int W, int H, const Taps &t, bool norm, hipStream_t st = nullptr, float *half = nullptr,
                 hipEvent_t stop = nullptr) {
    if (!st) st = p->stream;
    Options opt = p->opt;
    if (opt.march_prio == 1 && st != p->stream) opt.march_prio = 2;      // a later octave's chain (launch_team)
    const BlurForm r = norm ? launch_blur_tiled<true>(opt, st, in, out, W, H, t, p->mm, half, stop)
                            : launch_blur_tiled<false>(opt, st, in, out, W, H, t, p->mm, half, stop);
    if (r == BLUR_NONE) {       // one intermediate plane per stream that builds pyramids: the chains run beside one another
        float *tmp = (st == p->stream2 && p->tmp_below) ? p->tmp_below : ((st == p->stream3 && p->tmp_later) ? p->tmp_later : p->tmp);
        launch_blur_generic(st, in, out, tmp, W, H, t, p->mm, norm);
        if (stop) (void)hipEventRecord(stop, st);
    }
    return r != BLUR_NONE && half;
}

// Initial blur reading a typed (integer / RGB) frame directly: instantiated for the default 15-tap initial
// kernel (init_sigma = 1.6); any other tap count goes through the convert pass.
template <int DT>
BlurForm launch_init_blur_dt(const Options &opt, hipStream_t st, const void *in, float *out, int W, int H, const Taps &t, const uint32_t *mm) {
    return t.n == 15 ? launch_blur_n<15, true, DT>(opt, st, in, out, W, H, t, mm) : BLUR_NONE;
}

// dispatch F(DT) over the typed-frame codes that have a fused path
#define SIFTMI_TYPED_DISPATCH(dt, CALL)                       \
    switch (dt) {                                             \
        case SIFTMI_U8: { constexpr int DT = 1; CALL; } break;   \
        case SIFTMI_U16: { constexpr int DT = 2; CALL; } break;  \
        case SIFTMI_U32: { constexpr int DT = 3; CALL; } break;  \
        case SIFTMI_U64: { constexpr int DT = 4; CALL; } break;  \
        case SIFTMI_I32: { constexpr int DT = 5; CALL; } break;  \
        case SIFTMI_I64: { constexpr int DT = 6; CALL; } break;  \
        case SIFTMI_RGB8: { constexpr int DT = 8; CALL; } break; \
        default: break;                                       \
    }

struct Scope {   // optional hipEvent bracket around one launch (profile=1: blur launches only; 2: every stage)
    siftmi_plan *p; size_t idx = (size_t)-1; hipStream_t st;
    bool stop_bound = false;      // the closing event rides on the bracket's last launch (launch_ev): nothing to record at the end
    // record_start false: the caller binds the opening event to the launch in FRONT of the bracket (its end opens it)
    Scope(siftmi_plan *pl, const char *label, bool is_blur = false, double pixels = 0, hipStream_t s = nullptr, int octave = -1, bool record_start = true) : p(pl) {
        st = s ? s : p->stream;
        if (!p->profile || (p->profile == 1 && !(is_blur && octave == 0))) return;
        if (p->n_events == p->events.size()) {
            Event e;
            hipEventCreate(&e.a); hipEventCreate(&e.b);
            p->events.push_back(e);
        }
        idx = p->n_events++;
        Event &e = p->events[idx];
        e.label = label; e.is_blur = is_blur; e.pixels = pixels; e.octave = octave; e.launches = 1;
        if (record_start) hipEventRecord(e.a, st);
    }
    ~Scope() { if (idx != (size_t)-1 && !stop_bound) hipEventRecord(p->events[idx].b, st); }
};

double tnow() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }   // host clock, us (option "host_timing")
// the ordered words of the min / max slots (k_pyramid.hpp) back to floats
float minmax_decode(uint32_t u) { uint32_t v = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u; float f; memcpy(&f, &v, 4); return f; }

int grid_for(int64_t n, int block, int max_blocks) {
    int64_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > max_blocks) g = max_blocks;
    return (int)g;
}

double contrast_threshold(const siftmi_params &par) { return 0.8 * (double)par.peak_thresh; }   // image.cl:152
float octave_edge_thresh(const siftmi_params &par, int octsize) { return (octsize <= 1) ? par.edge_thresh0 : par.edge_thresh; }   // image.cl:193, plan.py:633-634

// ---- one launch site per kernel ------------------------------------------------------------------------------------
// Each function below is the only place that launches its kernel: it picks the template instance from a run-time argument
// and holds the positional argument list once.  None knows a siftmi_plan: the plan's launch functions and the siftmi_stage_*
// hooks both call them, and where the two differ (grid, capacities, cuts) the difference is an argument at the call site.
// (The blur and gradient-map launches have the same shape: launch_blur_tiled, launch_init_blur_dt, launch_maps_kernel.)

// Strip height and workgroup count of a detection launch over a W x H plane; blocks == 0: no detection area, no launch.
// rows_opt > 0 fixes the strip height (option "ext_rows"), else extrema_strip_rows halves it until `min_strips` strips cover
// the plane (<= 0: that function's own default).  y_lo >= 0: the band [y_lo, y_hi) is marched as a detection area of its
// own.  Four strips (waves) per workgroup; behind the guard nx, ny >= 1, so there is at least one workgroup.
struct DetectGeom { int rows = 0, blocks = 0; };
DetectGeom detect_geometry(int W, int H, int border, int rows_opt, int min_strips, int y_lo, int y_hi) {
    DetectGeom g;
    if (!(W > 2 * border && H > 2 * border)) return g;
    g.rows = rows_opt > 0 ? rows_opt : (min_strips > 0 ? extrema_strip_rows(W, H, border, min_strips) : extrema_strip_rows(W, H, border));
    const int nx = (W - 2 * border + 61) / 62, ny = ((y_lo >= 0 ? y_hi - y_lo : H - 2 * border) + g.rows - 1) / g.rows;
    g.blocks = (nx * ny + 3) / 4;
    return g;
}

// extrema_kernel: `refine` picks the instance that also refines the survivors of the edge test (ra: where they go); `lazy` the
// one that does not read bp.p[5] and leaves provisional scale-3 candidates (list form only; launch_top_patch follows it)
void launch_extrema(hipStream_t st, bool refine, const DetectGeom &geo, const BlurPlanes &bp, int W, int H, int border, double contrast, float edth,
                    float4 *cand, int *n_cand, int cand_cap, const RefineArgs &ra, int y_lo, int y_hi, int xcd_map, bool lazy = false) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)geo.blocks), dim3(256), 0, st, bp, W, H, border, geo.rows, contrast, edth, cand, n_cand, cand_cap, ra, y_lo, y_hi, xcd_map);
    };
    if (refine) go(extrema_kernel<true>); else if (lazy) go(extrema_kernel<false, true>); else go(extrema_kernel<false>);
}

// top_patch_kernel over the candidate list of one octave: plane 5 (`p5`, written) from plane 4 with the top plane's taps around
// every scale-3 entry, `blocks` one-wave workgroups striding over the device-side count
int launch_top_patch(hipStream_t st, int blocks, const float *p4, float *p5, int W, int H, const Taps &t, float4 *cand, const int *n_cand, int cand_cap) {
    if (t.n < 1 || t.n > 64) return fail(SIFTMI_EINVAL, "top_patch_kernel takes 1..64 taps, not %d", t.n);
    TopTaps ta;
    for (int i = 0; i < 64; i++) ta.t[i] = i < t.n ? t.t[i] : 0.0f;
    hipLaunchKernelGGL(top_patch_kernel, dim3((unsigned)blocks), dim3(64), top_patch_lds_bytes(t.n), st, p4, p5, W, H, ta, t.n, cand, n_cand, cand_cap);
    return SIFTMI_OK;
}

// refine_kernel over the candidate list of one octave, `blocks` workgroups
void launch_refine(hipStream_t st, int blocks, const BlurPlanes &bp, int W, int H, const float4 *cand, const int *n_cand, int cand_cap, const RefineArgs &ra) {
    hipLaunchKernelGGL(refine_kernel, dim3((unsigned)blocks), dim3(256), 0, st, bp, W, H, cand, n_cand, cand_cap, ra.peak_thresh, ra.init_sigma, ra.kp, ra.kp_aux,
                       ra.n_kp, ra.kp_capacity, ra.oct, ra.c_scale);
}

// orientation_kernel: `maps` picks the instance that reads tab.gmap / tab.omap; team_below: a workgroup per keypoint for groups
// of fewer refined keypoints; small_blocks: the workgroups a group of fewer than 16384 keypoints uses
void launch_orientation(hipStream_t st, bool maps, int grid, int lds_pad, const OctaveTable &tab, float ori_sigma, const float4 *kp, const int *kp_aux,
                        Counters *cnt, int group, int kp_cap, float4 *okp, int *oaux, int out_cap, int team_below, int small_blocks) {
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), (size_t)lds_pad, st, tab, ori_sigma, kp, kp_aux, cnt, group, kp_cap, okp, oaux, out_cap, team_below, small_blocks);
    };
    if (maps) go(orientation_kernel<true>); else go(orientation_kernel<false>);
}

// The descriptor kernels: the row-interval forms (descriptor_kernel, lazy gradients or MAPS) or the streaming form (any window
// size).  cnt == null: the keypoints [range_start, range_end), else the group's count.  The last four arguments are the
// row-interval forms' alone: workgroup per keypoint below `team_below`, dynamic hand-out, the workgroups used by a group of
// >= 65536 / < 16384 keypoints.
enum DescForm { DESC_ROWS = 0, DESC_ROWS_MAPS = 1, DESC_STREAM = 2 };
void launch_descriptors(hipStream_t st, DescForm form, int grid, int lds_pad, const OctaveTable &tab, const float4 *okp, const int *oaux, Counters *cnt, int group,
                        int range_start, int range_end, int out_cap, KpRecord *records, int rec_cap, KpRecord *host_records, int host_cap,
                        int team_below, int dynamic, int dense_blocks, int small_blocks) {
    auto rows = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), (size_t)lds_pad, st, tab, okp, oaux, cnt, group, range_start, range_end, out_cap, records, rec_cap,
                           host_records, host_cap, team_below, dynamic, dense_blocks, small_blocks);
    };
    if (form == DESC_ROWS_MAPS) rows(descriptor_kernel<true>);
    else if (form == DESC_ROWS) rows(descriptor_kernel<false>);
    else hipLaunchKernelGGL(descriptor_stream_kernel, dim3((unsigned)grid), dim3(256), (size_t)lds_pad, st, tab, okp, oaux, cnt, group, range_start, range_end, out_cap,
                            records, rec_cap, host_records, host_cap);
}

// convert_kernel<T> / convert_rgb_kernel by frame format: n pixels of `src` -> f32.  false: `dt` has no convert kernel (f32 frames are not converted).
bool launch_convert(hipStream_t st, int dt, const void *src, float *dst, int64_t n) {
    const dim3 g(grid_for(n, 256, 4096));
    switch (dt) {
        case SIFTMI_U8: hipLaunchKernelGGL(convert_kernel<uint8_t>, g, dim3(256), 0, st, (const uint8_t *)src, dst, n); return true;
        case SIFTMI_U16: hipLaunchKernelGGL(convert_kernel<uint16_t>, g, dim3(256), 0, st, (const uint16_t *)src, dst, n); return true;
        case SIFTMI_U32: hipLaunchKernelGGL(convert_kernel<uint32_t>, g, dim3(256), 0, st, (const uint32_t *)src, dst, n); return true;
        case SIFTMI_U64: hipLaunchKernelGGL(convert_kernel<uint64_t>, g, dim3(256), 0, st, (const uint64_t *)src, dst, n); return true;
        case SIFTMI_I32: hipLaunchKernelGGL(convert_kernel<int32_t>, g, dim3(256), 0, st, (const int32_t *)src, dst, n); return true;
        case SIFTMI_I64: hipLaunchKernelGGL(convert_kernel<int64_t>, g, dim3(256), 0, st, (const int64_t *)src, dst, n); return true;
        case SIFTMI_F64: hipLaunchKernelGGL(convert_kernel<double>, g, dim3(256), 0, st, (const double *)src, dst, n); return true;
        case SIFTMI_RGB8: hipLaunchKernelGGL(convert_rgb_kernel, g, dim3(256), 0, st, (const uint8_t *)src, dst, n); return true;
        default: return false;
    }
}

// normalize_kernel<DT>: n pixels of a frame of format `dt` (f32 or a typed format with a fused path) scaled by the min / max in mm
void launch_normalize(hipStream_t st, int dt, const void *src, float *dst, int64_t n, const uint32_t *mm) {
    const dim3 g(grid_for(n, 256, 4096));
    if (dt == SIFTMI_F32) hipLaunchKernelGGL(normalize_kernel<0>, g, dim3(256), 0, st, src, dst, n, mm);
    SIFTMI_TYPED_DISPATCH(dt, hipLaunchKernelGGL(normalize_kernel<DT>, g, dim3(256), 0, st, src, dst, n, mm));
}

// Global min / max of a frame of n pixels into mm: minmax_kernel for f32, minmax_typed_kernel<DT> for the typed formats with a fused
// path (the callers pass no other).  At most `max_blocks` workgroups of `threads` threads (the typed kernel is built for 256).
// reset / reset_words / reset_ones: the counter block this launch clears for the next image (k_pyramid.hpp: minmax_reset_next), or
// null, 0, -1.  `stop` not null: bound to the launch (launch_ev).
void launch_minmax(hipEvent_t stop, hipStream_t st, int dt, const void *img, int64_t n, int threads, int max_blocks, uint32_t *mm, uint32_t *reset,
                   int reset_words, int reset_ones) {
    if (dt == SIFTMI_F32) launch_ev(stop, minmax_kernel, dim3(grid_for(n / 4, threads, max_blocks)), dim3(threads), 0, st, (const float *)img, n, mm, reset, reset_words, reset_ones);
    SIFTMI_TYPED_DISPATCH(dt, launch_ev(stop, minmax_typed_kernel<DT>, dim3(grid_for(n / TypedChunk<DT>::PX, threads, max_blocks)), dim3(threads), 0, st, img, n, mm,
                                        reset, reset_words, reset_ones));
}

OctaveTable octave_table(const siftmi_plan *p) {
    OctaveTable tab;
    memset(&tab, 0, sizeof tab);
    tab.base = p->planes;
    tab.gmap = p->gmap; tab.omap = p->omap;
    for (int o = 0; o < p->n_oct && o < SIFT_MAX_OCTAVES; o++) {
        tab.off[o] = (long long)p->oct_off[(size_t)o];
        tab.W[o] = p->ow[(size_t)o];
        tab.H[o] = p->oh[(size_t)o];
    }
    return tab;
}

// ---- list capacities -----------------------------------------------------------------------------------------------
// The reference gives EVERY OCTAVE a keypoint buffer of kpsize = H*W / PIX_PER_KP entries and one counter, reset per octave
// (plan.py:243, 797-804): the candidates of a detection scale are appended behind the octave's oriented keypoints so far,
// and the oriented keypoints of the scale behind those.  An image may therefore return up to kpsize records per octave.
// Here the lists of a group start at kpsize entries and grow when an image needs more (the image is then run again), up
// to what that rule can ever admit; `reference_overflow` evaluates the rule itself from the per-scale counts.
int group_of(const siftmi_plan *p, int oct);
int cand_group_of(const siftmi_plan *p, int oct);
int64_t list_limit(const siftmi_plan *p, int what, int g) {      // what: 0 candidates, 1 refined, 2 oriented, 3 records
    const int64_t K = p->kpsize, O = std::max(1, p->n_oct);
    int64_t lim = what == 0 ? 3 * K : (what == 1 ? 3 * K * (g == 2 ? O : 1) : (what == 2 ? K * (g == 2 ? O : 1) : K * O));
    return std::min<int64_t>(lim, 0x7fffff00);
}

// c == null: the initial allocation.  Else: grow every list the image behind `c` (its counters) has outrun.  *grown says
// whether anything changed (the image has to run again: what lies behind a cut list was never produced).
void drain_streams(siftmi_plan *p);
int grow_lists(siftmi_plan *p, const Counters *c, bool *grown = nullptr) {
    if (grown) *grown = false;
    bool drained = c == nullptr;
    // nothing of the plan may be in flight while a buffer is replaced (another ending stream may still be copying its counters)
    auto quiesce = [&]() { if (!drained) { drain_streams(p); drained = true; } };
    const bool forks = p->n_oct > 2;                    // (group 1 exists only beside a group 2)
    auto want = [&](int64_t cap, int64_t need, int64_t limit) {
        if (need <= cap) return cap;
        if (!c) return std::min<int64_t>(limit, need);                        // creation: exactly the reference's kpsize
        return std::min<int64_t>(limit, std::max<int64_t>(need + need / 4 + 64, cap));
    };
    for (int g = 0; g < SIFT_GROUPS; g++) {
        if (g == 1 && !forks) continue;
        GroupLists &G = p->grp[g];
        int64_t need_cand = p->kpsize, need_kp = p->kpsize, need_out = p->kpsize;
        if (c) {
            need_cand = 0;
            for (int o = 0; o < p->n_oct && o < SIFT_MAX_OCTAVES; o++) if (cand_group_of(p, o) == g) need_cand = std::max<int64_t>(need_cand, c->n_cand[o]);
            need_kp = c->g_kp[g]; need_out = c->g_out[g];
        }
        const int64_t cc = want(G.cap_cand, need_cand, list_limit(p, 0, g)), ck = want(G.cap_kp, need_kp, list_limit(p, 1, g)),
                      co = want(G.cap_out, need_out, list_limit(p, 2, g));
        int rc = SIFTMI_OK;
        if (cc != G.cap_cand || ck != G.cap_kp || co != G.cap_out) quiesce();
        if (cc != G.cap_cand) { if ((rc = p->regrow(&G.cand, (size_t)G.cap_cand * 16, (size_t)cc * 16))) return rc; G.cap_cand = cc; if (grown) *grown = true; }
        if (ck != G.cap_kp) {
            if ((rc = p->regrow(&G.kp, (size_t)G.cap_kp * 16, (size_t)ck * 16)) || (rc = p->regrow(&G.kp_aux, (size_t)G.cap_kp * 4, (size_t)ck * 4))) return rc;
            G.cap_kp = ck; if (grown) *grown = true;
        }
        if (co != G.cap_out) {
            if ((rc = p->regrow(&G.okp, (size_t)G.cap_out * 16, (size_t)co * 16)) || (rc = p->regrow(&G.oaux, (size_t)G.cap_out * 4, (size_t)co * 4))) return rc;
            G.cap_out = co; if (grown) *grown = true;
        }
    }
    const int64_t cr = want(p->cap_rec, c ? (int64_t)c->n_rec : p->kpsize, list_limit(p, 3, 0));
    if (cr != p->cap_rec) {
        quiesce();
        int rc = p->regrow(&p->records, (size_t)p->cap_rec * sizeof(KpRecord), (size_t)cr * sizeof(KpRecord));
        if (rc) return rc;
        p->cap_rec = cr; if (grown) *grown = true;
    }
    if (grown && *grown) p->grows++;
    return SIFTMI_OK;
}

// The reference's capacity rule on the counts of an image (see Counters::c_scale): per octave, with `last` the oriented
// keypoints of the scales before, local_maxmin of scale s leaves the counter at last + candidates(s) and the orientation
// pass at last + oriented(s); either beyond kpsize means the reference dropped entries (image.cl:203-205,
// orientation_cpu.cl:150-172, plan.py:771 only warns).  oracle/sift_oracle.c: so_keypoints applies the same rule.
bool reference_overflow(const siftmi_plan *p, const Counters &c) {
    for (int o = 0; o < p->n_oct && o < SIFT_MAX_OCTAVES; o++) {
        int64_t last = 0;
        for (int s = 0; s < 3; s++) {
            if (last + c.c_scale[o][s] > p->kpsize) return true;
            last += c.o_scale[o][s];
            if (last > p->kpsize) return true;
        }
    }
    return false;
}

// Group of an octave in the image being enqueued: octave 0, octave 1, everything below -- or, when the later octaves form
// one chain (single stream, option "fork" = 0, octave 1 inside the tail launch), octave 0 and everything below it.
int group_of(const siftmi_plan *p, int oct) { return oct == 0 ? 0 : ((oct == 1 && p->fork_cur) ? 1 : 2); }
// ... and the group whose CANDIDATE buffer the octave's detection uses (a buffer holds one octave at a time): with option
// "split" octave 1 is searched beside the octaves below it, so its candidates take group 1's otherwise unused buffer.
int cand_group_of(const siftmi_plan *p, int oct) { return (oct == 1 && p->split_cur) ? 1 : group_of(p, oct); }

// One launch detects and refines an octave (launch_detect_octave) or two do
bool detect_fused(const siftmi_plan *p, int oct) {
    return p->profile <= 1 && (p->opt.fused_refine == 2 || (p->opt.fused_refine == 1 && !march_plane(p->ow[(size_t)oct], p->oh[(size_t)oct])));
}

// Does octave `oct` of the image being enqueued go without its full plane 5 (option "lazy_top")?  Only an octave with a
// per-octave pyramid and a candidate list (the fused detect-and-refine form reads plane 5 as it parks; the tail kernel builds
// its own planes), not under the full profile (every stage keeps its launch and label), not in the run that repeats an image
// whose provisional entries outran the candidate list.  Auto: by the scale-3 candidates this octave had in the previous image.
bool lazy_octave(const siftmi_plan *p, int oct, int tail_first) {
    const int mode = p->opt.lazy_top;
    if (!mode || p->lazy_block || p->profile > 1 || oct >= tail_first || oct >= SIFT_MAX_OCTAVES || detect_fused(p, oct)) return false;
    const int W = p->ow[(size_t)oct], H = p->oh[(size_t)oct], border = p->par.border_dist;
    if (!(W > 2 * border && H > 2 * border)) return false;
    if (mode == 1) return true;
    return p->lazy_seen && (long long)p->last_c_scale[oct][2] * p->opt.lazy_density < (long long)W * H;
}

// Extrema of the three detection scales + sub-pixel refinement of one octave; survivors are appended to the refined list
// of the octave's group (tagged with the octave).
void launch_detect_octave(siftmi_plan *p, int oct, hipStream_t st) {
    const int W = p->ow[(size_t)oct], H = p->oh[(size_t)oct];
    const int g = group_of(p, oct);
    GroupLists &G = p->grp[g];
    p->groups_cur |= 1u << g;
    char lab[96];
    BlurPlanes bp;
    for (int s = 0; s < 6; s++) bp.p[s] = p->plane(oct, s);
    const int border = p->par.border_dist;
    GroupLists &GC = p->grp[cand_group_of(p, oct)];
    const int ccap = (int)GC.cap_cand, kcap = (int)G.cap_kp;
    int *n_cand = &p->cnt->n_cand[oct];
    const DetectGeom geo = detect_geometry(W, H, border, p->opt.ext_rows, p->opt.ext_strips, -1, -1);
    if (!geo.blocks) return;
    const RefineArgs ra = {p->par.peak_thresh, (float)p->par.init_sigma, G.kp, G.kp_aux, &p->cnt->g_kp[g], kcap, oct, &p->cnt->c_scale[oct][0]};
    // One launch detects and refines (the survivors of the edge test are refined by the wave that parked them: no
    // candidate list, no second launch) unless every stage is bracketed on its own (full profile) or option
    // "fused_refine" says otherwise (0: never, 1: planes below 1400^2, 2: every plane).
    const bool fused = detect_fused(p, oct);
    const bool lazy = oct < SIFT_MAX_OCTAVES && p->lazy_cur[oct];        // (never with `fused`: lazy_octave)
    {
        snprintf(lab, sizeof lab, fused ? "local_maxmin+interp_keypoint %d" : "local_maxmin %d", oct);
        Scope sc(p, lab, false, 0, st);
        launch_extrema(st, fused, geo, bp, W, H, border, contrast_threshold(p->par), octave_edge_thresh(p->par, 1 << oct), GC.cand, n_cand, ccap, ra, -1, -1, p->opt.xcd_map, lazy);
    }
    if (fused) return;
    if (lazy) {     // plane 5 around the provisional scale-3 candidates, and the outer layer of their test (k_top_patch.hpp)
        snprintf(lab, sizeof lab, "top_patch %d", oct);
        Scope sc(p, lab, false, 0, st);
        (void)launch_top_patch(st, p->opt.top_blocks, p->plane(oct, 4), p->plane(oct, 5), W, H, p->taps[4], GC.cand, n_cand, ccap);
    }
    snprintf(lab, sizeof lab, "interp_keypoint+compact %d", oct);
    Scope sc(p, lab, false, 0, st);
    launch_refine(st, 512, bp, W, H, GC.cand, n_cand, ccap, ra);
}

// First octave of the run that octave_tail_kernel takes (k_tail.hpp), or n_oct when it takes none: octaves >= 1 whose
// planes are small enough to sit in LDS, all the way down to the last one.
int tail_first_octave(const siftmi_plan *p) {
    if (!p->opt.tail || p->profile > 1 || p->n_oct < 2) return p->n_oct;   // full profile: every stage keeps its own launch and label
    for (int s = 0; s < 5; s++) {
        const int n = p->taps[s].n;
        if (n != 11 && n != 15 && n != 17 && n != 21 && n != 27) return p->n_oct;
    }
    const int last = p->n_oct - 1;
    if (p->ow[(size_t)last] < 14 || p->oh[(size_t)last] < 14) return p->n_oct;
    int first = p->n_oct;
    for (int o = last; o >= 1; o--) {
        const int W = p->ow[(size_t)o], H = p->oh[(size_t)o];
        if ((int64_t)W * H > p->opt.tail_pixels || W > 128 || H > 128 || last - o + 1 > SIFT_TAIL_MAX_OCT) break;
        first = o;
    }
    return first;
}

// octaves [first, n_oct): pyramid + detection in one launch
int launch_tail(siftmi_plan *p, int first, hipStream_t st) {
    TailArgs a;
    memset(&a, 0, sizeof a);
    a.src = p->plane(first - 1, 3);
    a.src_w = p->ow[(size_t)first - 1];
    a.n = p->n_oct - first;
    if (a.n < 1 || a.n > SIFT_TAIL_MAX_OCT) return fail(SIFTMI_EINVAL, "octave_tail_kernel walks 1..%d octaves, not %d", SIFT_TAIL_MAX_OCT, a.n);
    for (int k = 0; k < a.n; k++) {
        const int oct = first + k;
        TailOctave &o = a.o[k];
        for (int s = 0; s < 6; s++) o.plane[s] = p->plane(oct, s);
        o.W = p->ow[(size_t)oct]; o.H = p->oh[(size_t)oct]; o.oct = oct;
        o.edth = octave_edge_thresh(p->par, 1 << oct);
    }
    for (int s = 0; s < 5; s++) { a.taps[s] = p->taps[s].dev; a.ntaps[s] = p->taps[s].n; }
    const size_t lds = tail_lds_bytes(a.o[0].W, a.o[0].H);
    {
        // The dynamic-LDS limit of a kernel is a property of the function on a device, not of a plan: keep the largest
        // value any plan has asked for (a plan of smaller frames must not lower it under a plan of larger ones).
        static std::mutex mu;
        static size_t granted[64] = {0};
        std::lock_guard<std::mutex> g(mu);
        size_t &have = granted[p->device & 63];
        if (have < 64 * 1024) have = 64 * 1024;
        if (lds > have) {
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void *>(&octave_tail_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            have = lds;
        }
    }
    GroupLists &G = p->grp[2];                 // the tail's octaves are the last ones: group 2
    p->groups_cur |= 1u << 2;
    hipLaunchKernelGGL(octave_tail_kernel, dim3((unsigned)a.n), dim3(SIFT_TAIL_THREADS), lds, st, a, p->par.border_dist,
                       contrast_threshold(p->par), p->par.peak_thresh, (float)p->par.init_sigma, p->tail_cand, p->tail_cand_cap,
                       p->cnt->n_cand, p->cnt->tail_ready, G.kp, G.kp_aux, &p->cnt->g_kp[2], (int)G.cap_kp, &p->cnt->c_scale[0][0], &p->cnt->tail_timeout);
    return SIFTMI_OK;
}

// orientation of every refined keypoint of one group (its refinement launches precede this one on `st`)
void launch_orient_group(siftmi_plan *p, int group, hipStream_t st) {
    const OctaveTable tab = octave_table(p);
    GroupLists &G = p->grp[group];
    char lab[96];
    snprintf(lab, sizeof lab, "orientation_assignment group %d", group);
    Scope sc(p, lab, false, 0, st);
    launch_orientation(st, group == 0 ? p->maps_g0 : p->maps_g1, p->opt.ori_blocks, p->opt.ori_pad, tab, p->par.ori_sigma, G.kp, G.kp_aux, p->cnt, group, (int)G.cap_kp,
                       G.okp, G.oaux, (int)G.cap_out, p->opt.ori_team, p->opt.ori_small_blocks);
}

// descriptors of one group's oriented keypoints
void launch_descriptor_group(siftmi_plan *p, int group, hipStream_t st) {
    const OctaveTable tab = octave_table(p);
    GroupLists &G = p->grp[group];
    char lab[96];
    snprintf(lab, sizeof lab, "descriptors group %d", group);
    Scope sc(p, lab, false, 0, st);
    const int desc_blocks = p->opt.desc_blocks;
    // Optional residency throttle (option "desc_pad": bytes of unused dynamic LDS per workgroup).  Round 1 capped the
    // octave-0 launch at 3 workgroups per CU so that the later octaves' kernels found registers; with the round-2
    // kernels (shorter detection chain, 4 workgroups per CU by registers) the unthrottled launch is faster
    // (0.96 against 1.01 ms per 4096^2 frame), so the default is 0.
    const int desc_pad = p->opt.desc_pad > 0 ? p->opt.desc_pad : 0;
    // a small group of octave 0 of a LARGE frame leaves room for the later octaves' chain, which ends such an image (4096^2
    // headline -2.2 %, 4096^2 with every octave -2.5 %); on a 1024^2 frame that chain is short and the same cut costs 2 %
    const int small_blocks = (group == 0 && p->n_oct > 1 && march_plane(p->ow[0], p->oh[0])) ? (p->early_cur ? p->opt.desc_early_blocks : p->opt.desc_small_blocks) : desc_blocks;
    const int ocap = (int)G.cap_out, rcap = (int)std::min<int64_t>(p->cap_rec, 0x7fffffff);
    // one launch, two forms: the count of the group (known on the device only) picks the wave-per-keypoint form
    // (throughput) or the workgroup-per-keypoint form (latency of a sparse group) -- unless the windows need the streaming form
    const bool maps = group == 0 ? p->maps_g0 : p->maps_g1;
    const DescForm form = (p->desc_rows && !p->opt.desc_stream) ? (maps ? DESC_ROWS_MAPS : DESC_ROWS) : DESC_STREAM;
    // (the MAPS form of a dense group wants every workgroup of the launch: 154 k keypoints 4.68 ms at 832, 4.48 at 960)
    const int dense_blocks = maps ? desc_blocks : p->opt.desc_dense_blocks;
    launch_descriptors(st, form, desc_blocks, desc_pad, tab, G.okp, G.oaux, p->cnt, group, 0, 0, ocap, p->records, rcap, p->host_out,
                       p->host_cap, p->opt.desc_team, p->opt.desc_dynamic, dense_blocks, small_blocks);
}

// gradient_maps_kernel over the octaves [oct_lo, oct_hi) of `tab` into tab.gmap / tab.omap, at most `blocks` workgroups
// walking the items with a grid stride (the plan's launch below and the stage hooks, on the null stream)
void launch_maps_kernel(const OctaveTable &tab, int oct_lo, int oct_hi, int blocks, hipStream_t st) {
    long long total = 0;
    for (int o = oct_lo; o < oct_hi; o++) total += gradient_map_items_of(tab.W[o], tab.H[o]);
    if (total <= 0) return;
    const unsigned g = (unsigned)std::min<long long>(total, blocks);
    hipLaunchKernelGGL(gradient_maps_kernel, dim3(g), dim3(256), 0, st, tab, oct_lo, oct_hi, total, (float *)tab.gmap, (float *)tab.omap);
}

// gradient maps of the octaves [oct_lo, oct_hi) (their pyramids exist on `st`)
void launch_gradient_maps(siftmi_plan *p, int oct_lo, int oct_hi, hipStream_t st) {
    if (oct_lo >= oct_hi) return;
    char lab[96];
    snprintf(lab, sizeof lab, "gradient maps octaves %d-%d", oct_lo, oct_hi - 1);
    Scope sc(p, lab, false, 0, st);
    launch_maps_kernel(octave_table(p), oct_lo, oct_hi, p->opt.maps_blocks, st);
}

// orientation + descriptors of one group, on one stream, ending with the read-back of the counters into pinned block `slot`
int launch_describe_group(siftmi_plan *p, int group, hipStream_t st, int slot) {
    p->groups_cur |= 1u << group;
    launch_orient_group(p, group, st);
    launch_descriptor_group(p, group, st);
    if (p->profile > 1) hipEventRecord(p->ev_last[slot], st);
    HIPCHK(hipMemcpyAsync(&p->hb->c[slot], p->cnt, sizeof(Counters), hipMemcpyDeviceToHost, st));
    p->wait_s[slot] = st;
    return SIFTMI_OK;
}

}  // namespace

// ============================================================================================
thread_local std::string g_err;   // the calling thread's last error (declared in host_common.hpp)
extern "C" {

const char *siftmi_last_error(void) { return g_err.c_str(); }
#ifdef SIFT_PHASE_CLOCK
// development instrument (k_keypoint.hpp: PhaseClock): the 32 accumulators of the per-keypoint kernels; reset != 0 clears them
int siftmi_dev_phase(uint64_t *out32, int32_t reset) {
    unsigned long long h[32];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(siftk::g_phase), sizeof h) != hipSuccess) return fail(SIFTMI_EDEVICE, "phase clock read failed");
    if (out32) for (int i = 0; i < 32; i++) out32[i] = h[i];
    if (reset) { memset(h, 0, sizeof h); if (hipMemcpyToSymbol(HIP_SYMBOL(siftk::g_phase), h, sizeof h) != hipSuccess) return fail(SIFTMI_EDEVICE, "phase clock reset failed"); }
    return SIFTMI_OK;
}
#endif
const char *siftmi_version(void) { return "sift_pyocl_amd 0.1 (gfx950)"; }


int siftmi_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int siftmi_device_name(int device_id, char *buf, int64_t buflen) {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    snprintf(buf, (size_t)buflen, "%s (%s)", prop.name, prop.gcnArchName);
    return SIFTMI_OK;
}

static thread_local int g_lane_mode = 0;   // set by siftmi_batch_create around its plan constructions: 1 single-stream lane, 2 multi-stream lane

int siftmi_plan_create(int32_t height, int32_t width, int32_t in_dtype, int32_t device_id,
                       const siftmi_params *params, int32_t profile, siftmi_plan **out) {
    if (!out || !params) return fail(SIFTMI_EINVAL, "null argument");
    *out = nullptr;
    if (height < 1 || width < 1) return fail(SIFTMI_EINVAL, "bad shape %dx%d", height, width);
    // planes are addressed with 32-bit byte offsets in the extrema kernel and 32-bit sample indices in the window kernels
    if ((int64_t)height * width > (int64_t)1 << 30) return fail(SIFTMI_EINVAL, "image too large: at most 2^30 pixels (32768 x 32768)");
    if (dtype_size(in_dtype) == 0) return fail(SIFTMI_EINVAL, "invalid input format (%d)", in_dtype);
    if (params->pix_per_kp < 1) return fail(SIFTMI_EINVAL, "pix_per_kp must be >= 1");
    if (params->border_dist < 1) return fail(SIFTMI_EINVAL, "border_dist must be >= 1");
    int ndev = siftmi_device_count();
    if (ndev < 1) return fail(SIFTMI_EDEVICE, "no HIP device available");
    if (device_id < 0 || device_id >= ndev) return fail(SIFTMI_EINVAL, "device %d out of range (%d devices)", device_id, ndev);
    HIPCHK(hipSetDevice(device_id));
    siftmi_plan *p = new (std::nothrow) siftmi_plan();
    if (!p) return fail(SIFTMI_ENOMEM, "host allocation failed");
    p->device = device_id; p->H = height; p->W = width; p->dtype = in_dtype; p->par = *params; p->profile = profile;
    // octave shapes, plan.py:213-224
    {
        int h = height, w = width;
        std::vector<int> hh{h}, ww{w};
        while ((h < w ? h : w) > 2 * params->border_dist + 2) { h /= 2; w /= 2; hh.push_back(h); ww.push_back(w); }
        hh.pop_back(); ww.pop_back();
        p->oh = hh; p->ow = ww;
        p->n_oct = (int)hh.size();
        if (params->octave_max > 0 && params->octave_max < p->n_oct) p->n_oct = params->octave_max;
        if (p->n_oct > SIFT_MAX_OCTAVES) p->n_oct = SIFT_MAX_OCTAVES;
    }
    const size_t N = (size_t)height * width;
    p->kpsize = (int64_t)(N / (size_t)params->pix_per_kp);   // plan.py:243
    if (p->kpsize < 1) p->kpsize = 1;
    int rc = SIFTMI_OK;
    // Stream priorities (pyramid and later-octave streams above the octave-0 detection stream, whose long orientation /
    // descriptor kernels would otherwise win every dispatch slot) pay off where two multi-stream plans share the GPU
    // (BatchPlan with 2 lanes of large frames: 1.13 instead of 1.33 ms per 4096^2 frame); for a single plan they are
    // within noise (round 2, later-octave chain above the octave-0 chain: 0.962 against 0.972 ms), and once a process has created prioritised streams its normal-priority streams get fewer hardware
    // queues (8 single-stream lanes of 512^2 frames: 0.72 instead of 0.41 ms per frame).  Hence: only for the
    // multi-stream lanes of a batch.
    const bool prio = g_lane_mode == 2;
    int prio_lo = 0, prio_hi = 0;
    if (prio) hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);
    hipError_t e = prio ? hipStreamCreateWithPriority(&p->stream, hipStreamNonBlocking, prio_hi) : hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete p; return fail(SIFTMI_EDEVICE, "hipStreamCreate: %s", hipGetErrorString(e)); }
    {
        size_t off = 0;
        for (int o = 0; o < p->n_oct; o++) { p->oct_off.push_back(off); off += 6 * (size_t)p->ow[(size_t)o] * p->oh[(size_t)o]; }
        if (p->n_oct == 0) { p->oct_off.push_back(0); off = 6 * N; p->ow.assign(1, width); p->oh.assign(1, height); }
        p->planes_floats = off;
        rc = p->alloc(&p->planes, off * sizeof(float));
    }
    if (!rc && (prio ? hipStreamCreateWithPriority(&p->stream2, hipStreamNonBlocking, prio_lo) : hipStreamCreateWithFlags(&p->stream2, hipStreamNonBlocking)) != hipSuccess) rc = fail(SIFTMI_EDEVICE, "hipStreamCreate failed");
    if (!rc && (prio ? hipStreamCreateWithPriority(&p->stream3, hipStreamNonBlocking, prio_hi) : hipStreamCreateWithFlags(&p->stream3, hipStreamNonBlocking)) != hipSuccess) rc = fail(SIFTMI_EDEVICE, "hipStreamCreate failed");
    if (!rc && hipEventCreateWithFlags(&p->ev_p3, SIFT_SYNC_EVENT) != hipSuccess) rc = fail(SIFTMI_EDEVICE, "hipEventCreate failed");
    p->overlap = true;
    for (int o = 0; o < p->n_oct && !rc; o++) {
        hipEvent_t e;
        if (hipEventCreateWithFlags(&e, SIFT_SYNC_EVENT) != hipSuccess) rc = fail(SIFTMI_EDEVICE, "hipEventCreate failed");
        else p->ev_pyr.push_back(e);
    }
    if (!rc) rc = p->alloc(&p->tmp, N * sizeof(float));
    if (!rc && p->n_oct > 1) rc = p->alloc(&p->tmp_later, (size_t)p->ow[1] * p->oh[1] * sizeof(float));
    if (!rc && p->n_oct > 2) rc = p->alloc(&p->tmp_below, (size_t)p->ow[2] * p->oh[2] * sizeof(float));
    if (!rc) rc = p->alloc(&p->raw, N * (dtype_size(in_dtype) > 4 ? dtype_size(in_dtype) : 4));
    if (!rc && in_dtype != SIFTMI_F32) rc = p->alloc(&p->conv, N * sizeof(float));

    // two counter blocks, used by alternate images: the min/max pass of an image resets the other one for its successor
    if (!rc) rc = p->alloc(&p->cnt_pair, 2 * sizeof(Counters));
    if (!rc) { p->cnt = p->cnt_pair; p->mm = p->cnt->mm; }   // (mm: device address of the min/max slots inside the counter block)
    // a tail octave (<= SIFT_TAIL_MAX_PIXELS samples, 3 scales) cannot hold more candidates than this
    p->tail_cand_cap = 3 * SIFT_TAIL_MAX_PIXELS;
    if (!rc) rc = p->alloc(&p->tail_cand, (size_t)SIFT_TAIL_MAX_OCT * p->tail_cand_cap * sizeof(float4));
    // The lists start at the reference's kpsize (plan.py:243: its capacity PER OCTAVE) and grow when an image needs more
    // (grow_lists): a frame of the default PIX_PER_KP never does.  Octave 0 in two groups needs group 1's lists too:
    // large planes only (the planes the marching blur takes).
    if (!rc) rc = grow_lists(p, nullptr);
    if (!rc) rc = compute_schedule(p);
    if (!rc) {
        // both blocks all zero, min / max slots at their identities (minmax_reset_next does the same for every later image)
        Counters zero;
        memset(&zero, 0, sizeof zero);
        zero.mm[0] = 0xffffffffu;
        if (hipMemcpy(p->cnt_pair, &zero, sizeof zero, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(p->cnt_pair + 1, &zero, sizeof zero, hipMemcpyHostToDevice) != hipSuccess) rc = fail(SIFTMI_EDEVICE, "counter initialisation failed");
    }
    if (!rc) { hipEventCreate(&p->ev_first); for (hipEvent_t &e : p->ev_last) hipEventCreate(&e); }
    if (rc) { std::string keep = g_err; siftmi_plan_destroy(p); g_err = keep; return rc; }
    *out = p;
    return SIFTMI_OK;
}

int siftmi_plan_destroy(siftmi_plan *p) {
    if (!p) return SIFTMI_OK;
    hipSetDevice(p->device);
    if (p->stream) hipStreamSynchronize(p->stream);
    if (p->stream2) { hipStreamSynchronize(p->stream2); hipStreamDestroy(p->stream2); }
    if (p->stream3) { hipStreamSynchronize(p->stream3); hipStreamDestroy(p->stream3); }
    if (p->ev_p3) hipEventDestroy(p->ev_p3);
    if (p->ev_det2) hipEventDestroy(p->ev_det2);
    if (p->ev_early) hipEventDestroy(p->ev_early);
    if (p->ev_maps0) hipEventDestroy(p->ev_maps0);
    for (hipEvent_t e : p->ev_pyr) hipEventDestroy(e);
    for (void *q : p->allocs) hipFree(q);
    for (GroupLists &G : p->grp)
        for (void *q : {(void *)G.kp, (void *)G.kp_aux, (void *)G.okp, (void *)G.oaux, (void *)G.cand}) if (q) hipFree(q);
    if (p->records) hipFree(p->records);
    if (p->hb) hipHostFree(p->hb);
    if (p->ev_join) hipEventDestroy(p->ev_join);
    if (p->warp_in) hipFree(p->warp_in);
    if (p->warp_out) hipFree(p->warp_out);
    if (p->ev_wa) hipEventDestroy(p->ev_wa);
    if (p->ev_wb) hipEventDestroy(p->ev_wb);
    for (Event &e : p->events) { hipEventDestroy(e.a); hipEventDestroy(e.b); }
    if (p->ev_first) hipEventDestroy(p->ev_first);
    for (hipEvent_t e : p->ev_last) if (e) hipEventDestroy(e);
    if (p->stream) hipStreamDestroy(p->stream);
    delete p;
    return SIFTMI_OK;
}

int siftmi_plan_info(const siftmi_plan *p, int32_t *n_octaves, int64_t *kpsize, int64_t *bytes_allocated) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (n_octaves) *n_octaves = p->n_oct;
    if (kpsize) *kpsize = p->kpsize;
    if (bytes_allocated) *bytes_allocated = p->bytes;
    return SIFTMI_OK;
}

int siftmi_plan_capacity(const siftmi_plan *p, int64_t *records, int64_t *growths) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (records) *records = p->cap_rec;
    if (growths) *growths = p->grows;
    return SIFTMI_OK;
}

int siftmi_plan_tail_timeouts(const siftmi_plan *p, int64_t *timeouts, int32_t *tail_enabled) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (timeouts) *timeouts = p->tail_timeouts;
    if (tail_enabled) *tail_enabled = p->opt.tail ? 1 : 0;
    return SIFTMI_OK;
}

int siftmi_plan_set_params(siftmi_plan *p, const siftmi_params *params) {
    if (!p || !params) return fail(SIFTMI_EINVAL, "null argument");
    if (params->pix_per_kp != p->par.pix_per_kp || params->octave_max != p->par.octave_max)
        return fail(SIFTMI_EINVAL, "pix_per_kp / octave_max are fixed at plan creation");
    // border_dist may change between calls: like the reference, which sizes its octave list from par.BorderDist in the
    // constructor (plan.py:213-224) but hands the CURRENT par.BorderDist to local_maxmin (plan.py:631-641), the octave
    // shapes stay those of creation and only the detection border follows.
    if (params->border_dist < 1) return fail(SIFTMI_EINVAL, "border_dist must be >= 1");
    HIPCHK(hipSetDevice(p->device));
    const bool resched = params->init_sigma != p->par.init_sigma || (params->double_im_size != 0) != (p->par.double_im_size != 0);
    p->par = *params;
    return resched ? compute_schedule(p) : SIFTMI_OK;
}

// Tuning / diagnostic options of one plan, by name.  Results never depend on them (every path is bit-identical);
// tests use "fused_convert" = 0 to compare the fused typed-frame path with the separate convert pass.
int siftmi_plan_set_option(siftmi_plan *p, const char *name, int64_t value) {
    if (!p || !name) return fail(SIFTMI_EINVAL, "null argument");
    const std::string n(name);
    if (value < INT32_MIN || value > INT32_MAX) return fail(SIFTMI_EINVAL, "option '%s': value %lld is outside int32", name, (long long)value);
    const int v = (int)value;
    Options &o = p->opt;
    if (n == "fused_convert") o.fused_convert = v != 0;
    else if (n == "overlap") { o.overlap = v != 0; p->overlap = o.overlap; }
    else if (n == "march") o.march = v != 0;
    else if (n == "march_wgs") o.march_wgs = v > 0 ? v : 0;
    else if (n == "xcd_map") o.xcd_map = v != 0;
    else if (n == "march_prio") { if (v < 0 || v > 2) return fail(SIFTMI_EINVAL, "march_prio must be 0, 1 or 2"); o.march_prio = (int)v; }
    else if (n == "ori_blocks") { if (v < 1) return fail(SIFTMI_EINVAL, "ori_blocks must be >= 1"); o.ori_blocks = v; }
    else if (n == "ori_pad") { if (v < 0 || v > SIFT_LDS_PAD_MAX) return fail(SIFTMI_EINVAL, "ori_pad must be in 0..%d", SIFT_LDS_PAD_MAX); o.ori_pad = v; }
    else if (n == "desc_blocks") { if (v < 1) return fail(SIFTMI_EINVAL, "desc_blocks must be >= 1"); o.desc_blocks = v; }
    else if (n == "desc_pad") { if (v < 0 || v > SIFT_LDS_PAD_MAX) return fail(SIFTMI_EINVAL, "desc_pad must be in 0..%d", SIFT_LDS_PAD_MAX); o.desc_pad = v; }
    else if (n == "desc_stream") o.desc_stream = v != 0;
    else if (n == "mm_threads") { if (v != 256 && v != 512 && v != 1024) return fail(SIFTMI_EINVAL, "mm_threads must be 256, 512 or 1024"); o.mm_threads = v; }
    else if (n == "mm_blocks") { if (v < 1) return fail(SIFTMI_EINVAL, "mm_blocks must be >= 1"); o.mm_blocks = v; }
    else if (n == "ori_small_blocks") { if (v < 1) return fail(SIFTMI_EINVAL, "ori_small_blocks must be >= 1"); o.ori_small_blocks = v; }
    else if (n == "ext_rows") o.ext_rows = (int)v;
    else if (n == "ext_strips") { if (v < 1) return fail(SIFTMI_EINVAL, "ext_strips must be >= 1"); o.ext_strips = (int)v; }
    else if (n == "tail") o.tail = v != 0;
    else if (n == "tail_pixels") { if (v < 1 || v > SIFT_TAIL_MAX_PIXELS) return fail(SIFTMI_EINVAL, "tail_pixels must be in 1..%d", SIFT_TAIL_MAX_PIXELS); o.tail_pixels = (int)v; }
    else if (n == "desc_team") o.desc_team = v > 0 ? v : 0;
    else if (n == "desc_dynamic") o.desc_dynamic = v != 0;
    else if (n == "ori_team") o.ori_team = v > 0 ? v : 0;
    else if (n == "fused_shrink") o.fused_shrink = v != 0;
    else if (n == "fused_refine") { if (v < 0 || v > 2) return fail(SIFTMI_EINVAL, "fused_refine must be 0, 1 or 2"); o.fused_refine = (int)v; }
    else if (n == "maps") { if (v < 0 || v > 2) return fail(SIFTMI_EINVAL, "maps must be 0 (never), 1 (always) or 2 (by the previous image)"); o.maps = v; }
    else if (n == "maps_blocks") { if (v < 1) return fail(SIFTMI_EINVAL, "maps_blocks must be >= 1"); o.maps_blocks = v; }
    else if (n == "maps_density") { if (v < 1) return fail(SIFTMI_EINVAL, "maps_density must be >= 1"); o.maps_density = v; }
    else if (n == "early_chain") { if (v < 0 || v > 2) return fail(SIFTMI_EINVAL, "early_chain must be 0 (never), 1 (always) or 2 (unless the previous image was keypoint-rich)"); o.early_chain = v; }
    else if (n == "desc_early_blocks") { if (v < 1) return fail(SIFTMI_EINVAL, "desc_early_blocks must be >= 1"); o.desc_early_blocks = v; }
    else if (n == "split") o.split = v != 0;
    else if (n == "fork") { if (v < 0 || v > 2) return fail(SIFTMI_EINVAL, "fork must be 0 (never), 1 (always) or 2 (frames of five octaves and more)"); o.fork = v; }
    else if (n == "desc_small_blocks") { if (v < 1) return fail(SIFTMI_EINVAL, "desc_small_blocks must be >= 1"); o.desc_small_blocks = v; }
    else if (n == "desc_dense_blocks") { if (v < 1) return fail(SIFTMI_EINVAL, "desc_dense_blocks must be >= 1"); o.desc_dense_blocks = v; }
    else if (n == "spin") o.spin = v != 0;
    else if (n == "host_timing") o.host_timing = v != 0;
    else if (n == "tail_fault") o.tail_fault = v > 0 ? v : 0;
    else return fail(SIFTMI_EINVAL, "unknown option '%s'", name);
    return SIFTMI_OK;
}

// The lazy top plane of a plan (Options::lazy_top and its two tuning values; see include/siftmi.h).  An entry point of its own:
// mode, threshold and grid are set together, and a value <= 0 of the latter two keeps what the plan has.
int siftmi_plan_set_lazy_top(siftmi_plan *p, int32_t mode, int32_t density, int32_t blocks) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (mode < 0 || mode > 2) return fail(SIFTMI_EINVAL, "lazy_top must be 0 (never), 1 (always) or 2 (by the previous image)");
    if (blocks > 65535) return fail(SIFTMI_EINVAL, "top_patch_kernel takes at most 65535 workgroups");
    p->opt.lazy_top = mode;
    if (density > 0) p->opt.lazy_density = density;
    if (blocks > 0) p->opt.top_blocks = blocks;
    return SIFTMI_OK;
}

}  // extern "C"

namespace {
int enqueue_body(siftmi_plan *p);

// Enqueue the whole pipeline of one image on the plan's streams, ending with the asynchronous read-back of the
// counters into the plan's pinned block.  No host wait.  `sync_device`: order after the caller's other streams.
int plan_enqueue(siftmi_plan *p, const void *image, int32_t image_dtype, int32_t image_is_device, bool sync_device) {
    if (image_dtype != p->dtype && image_dtype != SIFTMI_F32)
        return fail(SIFTMI_EINVAL, "image dtype %d is neither the plan's (%d) nor float32", image_dtype, p->dtype);
    HIPCHK(hipSetDevice(p->device));
    if (!p->hb) HIPCHK(hipHostMalloc((void **)&p->hb, sizeof(*p->hb), hipHostMallocDefault));
    if (!p->ev_join) HIPCHK(hipEventCreate(&p->ev_join));
    const size_t N = (size_t)p->H * p->W;
    const void *src = image;
    if (image_is_device) {
        if (sync_device) HIPCHK(hipDeviceSynchronize());   // order after the caller's work on other streams
    } else {
        HIPCHK(hipMemcpyAsync(p->raw, image, N * dtype_size(image_dtype), hipMemcpyHostToDevice, p->stream));
        src = p->raw;
        p->raw_dtype = image_dtype;
    }
    const bool htime = p->opt.host_timing != 0;
    const double t_enter = tnow();
    p->n_events = 0;
    if (p->profile > 1) hipEventRecord(p->ev_first, p->stream);     // (light profile: only the blur bracket -- every event record between kernels is a bubble)
    // this image's counter block was reset by the min/max pass of the previous image (or at plan creation); the other block
    // is reset by this image's min/max pass (k_pyramid.hpp: minmax_reset_next)
    // (the two blocks alternate only if an image never overlaps its predecessor on the same plan: plan_wait -- or a drain
    // on an error path -- always comes between two enqueues; `in_flight` enforces it)
    if (p->in_flight) return fail(SIFTMI_EINVAL, "the plan still has an image in flight");
    p->last_valid = false;       // the planes and counts of the previous call are about to be overwritten
    p->cnt = p->cnt_pair + p->cnt_parity;
    p->mm = p->cnt->mm;
    Counters *next_cnt = p->cnt_pair + (p->cnt_parity ^ 1);
    constexpr int kCntWords = (int)(sizeof(Counters) / 4), kCntOnes = (int)(offsetof(Counters, mm) / 4);
    static_assert(sizeof(Counters) % 4 == 0, "Counters is a block of 32-bit words");
    const float *f32src = (const float *)src;
    // Typed frames (u8 / u16 / ... / RGB8) are converted at the point of use by the min/max and the initial blur
    // (or the plain normalise) -- no f32 copy of the frame in HBM.  Fallback to the convert pass: float64 frames,
    // a non-default initial tap count, a frame that is not 16-byte aligned.
    const bool fused_in = image_dtype != SIFTMI_F32 && image_dtype != SIFTMI_F64 && (((uintptr_t)src) & 15) == 0 &&
                          (!p->have_init || p->taps[5].n == 15) && p->opt.fused_convert;
    if (image_dtype != SIFTMI_F32 && !fused_in) {
        Scope sc(p, "convert -> float");
        if (!launch_convert(p->stream, image_dtype, src, p->conv, (int64_t)N)) return fail(SIFTMI_EINVAL, "invalid input format");
        f32src = p->conv;
    }
    // light profiling: ONE event pair around the six full-resolution blur launches (initial + five scales of octave 0),
    // opened by the END of the min/max launch and closed by the end of octave 0's last blur (enqueue_body) -- both events
    // ride on those launches (launch_ev), no packet of their own sits between two kernels
    hipEvent_t open_ev = nullptr;
    if (p->profile == 1 && p->have_init) {
        Scope *ch = new Scope(p, "Blur octave 0: initial + scales 0-4 (one bracket)", true, 6.0 * (double)N, nullptr, 0, false);
        if (ch->idx != (size_t)-1) { p->events[ch->idx].launches = 6; open_ev = p->events[ch->idx].a; }
        p->chain = ch;
    }
    {
        Scope sc(p, "max_min");
        // a typed frame is reduced where it lies (workgroups of 256), anything else as f32 (option "mm_threads")
        launch_minmax(open_ev, p->stream, fused_in ? image_dtype : SIFTMI_F32, fused_in ? src : f32src, (int64_t)N, fused_in ? 256 : p->opt.mm_threads, p->opt.mm_blocks,
                      p->mm, (uint32_t *)next_cnt, kCntWords, kCntOnes);
    }
    p->cnt_parity ^= 1;          // the pass that resets the other block is in the queue: the next image takes that block
    p->in_flight = true;
    float *base0 = p->plane(0, 0);
    if (p->have_init) {
        Scope *sc = nullptr;
        if (p->profile != 1) sc = new Scope(p, "normalize + initial blur", true, (double)N, nullptr, 0);
        if (fused_in) {
            SIFTMI_TYPED_DISPATCH(image_dtype, launch_init_blur_dt<DT>(p->opt, p->stream, src, base0, p->W, p->H, p->taps[5], p->mm));
        } else {
            launch_blur(p, f32src, base0, p->W, p->H, p->taps[5], true);
        }
        delete sc;
    } else {
        Scope sc(p, "normalize");
        launch_normalize(p->stream, fused_in ? image_dtype : SIFTMI_F32, fused_in ? src : f32src, base0, (int64_t)N, p->mm);
    }
    // ---- everything below depends on plan-owned buffers only
    const int rc = enqueue_body(p);
    if (htime) fprintf(stderr, "[siftmi] enqueue %.0f us\n", tnow() - t_enter);
    return rc;
}

// Pyramid of every octave, detection, orientation, description, read-back of the counters: the part of one image's
// work that touches plan-owned buffers only.  Sets p->fin and p->wait_s.
int enqueue_body(siftmi_plan *p) {
    char lab[96];
    // Streams (option "overlap"; a single-stream plan runs the same launches in this order on `stream`):
    //   stream  : octave 0 end to end -- pyramid, detection, orientation, descriptors (group 0), read-back of the counters;
    //   stream3 : octave 1 from octave 0's pyramid on -- its pyramid, detection, orientation and descriptors (group 1);
    //   stream2 : the octaves below (option "fork"), from the moment octave 1's plane 3 exists -- pyramids, detection, the tail
    //             launch, orientation and descriptors (group 2); before that, octave 0's gradient maps on keypoint-rich frames.
    // The groups have their own lists and counters and meet only in the record list (descriptor_open): nothing orders them
    // but the two pyramid events.  Octave planes are never rewritten.  (Round 4 had one chain for all later octaves, whose
    // detection also waited for the end of octave 0's orientation pass -- the lists were shared; that chain ended the frame,
    // ~75 us after octave 0's descriptors, on a nearly idle chip.  Round 5 also tried octave 0 in two groups -- scale 1 from
    // plane 3 on, under the last two blurs: 0.86 against 0.80 ms, the blurs beside it slow down by more than the chain gains.)
    const bool two = p->overlap && p->n_oct > 0;
    const int tail_first = tail_first_octave(p);
    p->tail_first_cur = tail_first;
    p->groups_cur = 0;
    for (int o = 0; o < SIFT_MAX_OCTAVES; o++) p->lazy_cur[o] = o < p->n_oct && lazy_octave(p, o, tail_first);
    for (hipStream_t &w : p->wait_s) w = nullptr;
    // Gradient maps for the per-keypoint kernels of this image (option "maps"): large frames, by the previous image's counts
    {
        const int mode = p->opt.maps;
        long long px0 = 0, px1 = 0;
        for (int o = 0; o < p->n_oct; o++) {
            const long long px = (long long)p->ow[(size_t)o] * p->oh[(size_t)o];
            if (o == 0) px0 = px; else px1 += px;
        }
        auto dense = [&](int count, long long pixels) { return mode == 1 || (mode == 2 && (long long)count * p->opt.maps_density >= pixels); };
        const bool layout_ok = mode != 0 && p->n_oct > 0 && (mode == 1 || march_plane(p->ow[0], p->oh[0]));
        bool want0 = layout_ok && dense(p->last_group0, px0);
        bool want1 = layout_ok && p->n_oct > 1 && dense(p->last_group1, px1);
        if ((want0 || want1) && !p->gmap) {
            // first keypoint-rich image of this plan: two maps of half the pyramid's size each (three planes per octave)
            float *g = nullptr, *o = nullptr;
            const size_t bytes = (p->planes_floats / 2 + 16) * sizeof(float);
            if (!p->maps_unavailable && p->alloc(&g, bytes) == SIFTMI_OK) {          // (alloc() keeps the books: allocs, bytes)
                if (p->alloc(&o, bytes) == SIFTMI_OK) { p->gmap = g; p->omap = o; }
                else {                       // half a pair is of no use: give it back instead of holding it until the plan dies
                    (void)hipFree(g);
                    p->allocs.pop_back();
                    p->bytes -= (int64_t)bytes;
                }
            }
            if (!p->gmap) {                  // no room: the lazy forms, and no further attempt (a hipMalloc synchronises the device)
                p->maps_unavailable = true;
                want0 = want1 = false;
                (void)hipGetLastError();
            }
        }
        p->maps_g0 = want0; p->maps_g1 = want1;
        if (want0 && two && !p->ev_maps0) HIPCHK(hipEventCreateWithFlags(&p->ev_maps0, SIFT_SYNC_EVENT));
    }
    // the later octaves in two chains: two streams, an octave 1 outside the tail launch, at least one octave below it
    const bool fork = two && (p->opt.fork == 1 || (p->opt.fork == 2 && p->n_oct >= 5)) && p->n_oct > 2 && tail_first != 1 && p->grp[1].okp;
    p->fork_cur = fork;
    // ... or ONE group whose octaves are built and searched on two streams (option "split"; not beside octave 0's gradient maps,
    // which use stream2)
    const bool split = two && !fork && p->opt.split && p->n_oct > 2 && tail_first != 1 && p->grp[1].cand && !p->maps_g0;
    p->split_cur = split;
    if (split && !p->ev_det2) HIPCHK(hipEventCreateWithFlags(&p->ev_det2, SIFT_SYNC_EVENT));
    hipStream_t later = two ? p->stream3 : p->stream;       // octave 1's chain (every later octave's without the fork)
    hipStream_t below = (fork || split) ? p->stream2 : later;   // the chain of the octaves below octave 1
    // ... starts at plane 3 of octave 0 (option "early_chain"): needs the fused hand-off (octave 1's plane 0 written by octave 0's third blur)
    bool early = two && p->opt.early_chain && p->n_oct > 1 && p->profile <= 1 && p->opt.fused_shrink && tail_first != 1;
    if (early && p->opt.early_chain == 2) {
        const long long px0 = (long long)p->ow[0] * p->oh[0];
        // not on keypoint-rich frames (+4 % at 4096^2), and not where it brings nothing: a frame of at least 8 Mpixel with three
        // octaves (the later octaves' chain is short there: +-1 %, and octave 0's last two blurs would share the chip for nothing)
        early = (long long)p->last_group0 * p->opt.maps_density < px0 && (p->n_oct >= 4 || px0 < (8ll << 20));
    }
    p->early_cur = early;
    bool handed[SIFT_MAX_OCTAVES + 1] = {false};   // plane 0 of the octave was written by the blur launch of the octave above
    hipEvent_t pyr0_done = nullptr;            // light profile: the blur bracket's closing event stands in for ev_pyr[0]
    int slot = 0;                              // read-back blocks used so far (one per ending stream)
    // shrink + five blurs of one octave on stream `pyr`
    auto build_pyramid = [&](int oct, hipStream_t pyr) -> int {
        const int W = p->ow[(size_t)oct], H = p->oh[(size_t)oct];
        if (oct > 0 && !handed[oct]) {
            const int LW = p->ow[(size_t)oct - 1];
            snprintf(lab, sizeof lab, "shrink %d", oct - 1);
            Scope sc(p, lab, false, 0, pyr);
            hipLaunchKernelGGL(shrink_kernel, shrink_grid(W, H), dim3(256), 0, pyr,
                               (const float *)p->plane(oct - 1, 3), p->plane(oct, 0), LW, W, H);
        }
        // The octave hand-off (next[y][x] = plane 3 [2y][2x]) rides on the launch that writes plane 3, unless the next octave
        // is built by the tail kernel (which shrinks for itself) or every stage is bracketed on its own (full profile).
        float *half = nullptr;
        if (p->opt.fused_shrink && p->profile <= 1 && oct + 1 < p->n_oct && oct + 1 != tail_first)
            half = p->plane(oct + 1, 0);
        if (p->profile == 1 && oct == 0 && !p->chain) {          // no initial blur: the bracket opens here, five launches
            Scope *ch = new Scope(p, "Blur octave 0, scales 0-4 (one bracket)", true, 5.0 * W * H, nullptr, 0);
            if (ch->idx != (size_t)-1) p->events[ch->idx].launches = 5;
            p->chain = ch;
        }
        bool pyr0_bound = false;
        // lazy top plane: the launch that writes plane 5 is not run; what rode on it rides on the one that writes plane 4
        const bool lazy = oct < SIFT_MAX_OCTAVES && p->lazy_cur[oct];
        const int s_last = lazy ? 3 : 4;
        if (lazy && oct == 0 && p->profile == 1 && p->chain) {
            Scope *ch = static_cast<Scope *>(p->chain);
            if (ch->idx != (size_t)-1) { p->events[ch->idx].launches -= 1; p->events[ch->idx].pixels -= (double)W * H; }
        }
        for (int s = 0; s <= s_last; s++) {
            if (p->profile > 1) snprintf(lab, sizeof lab, "Blur octave %d scale %d (%d taps)", oct, s, p->taps[s].n);
            // the events other streams (or the light profile) wait for are the END of a blur launch: they ride on it (launch_ev)
            hipEvent_t done = nullptr;
            if (s == 2 && oct == 0 && early) {
                if (!p->ev_early) HIPCHK(hipEventCreateWithFlags(&p->ev_early, SIFT_SYNC_EVENT));
                done = p->ev_early;
            } else if (s == 2 && oct == 1 && (fork || split)) {
                done = p->ev_p3;       // plane 3 of octave 1 and plane 0 of octave 2 exist (or will be shrunk from it): the chain below starts here
            } else if (s == s_last && oct == 0 && p->profile == 1 && p->chain) {
                Scope *ch = static_cast<Scope *>(p->chain);
                if (ch->idx != (size_t)-1) { done = p->events[ch->idx].b; ch->stop_bound = true; }     // closes the light profile's bracket
            } else if (s == s_last && oct == 0 && p->profile == 0 && two) {
                done = p->ev_pyr[0]; pyr0_bound = true;
            }
            {
                Scope sc(p, lab, true, (double)W * H, pyr, p->profile > 1 ? oct : -2);      // (light profile: octave 0 is inside the open bracket, the others are not timed)
                if (launch_blur(p, p->plane(oct, s), p->plane(oct, s + 1), W, H, p->taps[s], false, pyr, s == 2 ? half : nullptr, done)) handed[oct + 1] = true;
            }
            if (s == 2 && oct == 1 && (fork || split)) HIPCHK(hipStreamWaitEvent(below, p->ev_p3, 0));
        }
        if (oct == 0 && p->profile == 1) {
            Scope *ch = static_cast<Scope *>(p->chain);
            const size_t idx = ch ? ch->idx : (size_t)-1;
            delete ch; p->chain = nullptr;                  // (the closing event rode on the last blur launch)
            if (idx != (size_t)-1 && two) pyr0_done = p->events[idx].b;   // ... which is also "octave 0's pyramid exists"
        }
        if (two && oct == 0 && !pyr0_done && !pyr0_bound) HIPCHK(hipEventRecord(p->ev_pyr[0], pyr));
        return SIFTMI_OK;
    };
    auto wait_pyr0 = [&](hipStream_t st) { return hipStreamWaitEvent(st, pyr0_done ? pyr0_done : p->ev_pyr[0], 0); };
    auto wait_later = [&](hipStream_t st) { return early ? hipStreamWaitEvent(st, p->ev_early, 0) : wait_pyr0(st); };
    int rc = SIFTMI_OK;
    if (p->n_oct > 0) {
        // ---- octave 0 (tail_first_octave never takes it: the tail launch starts from plane 3 of an octave above)
        if ((rc = build_pyramid(0, p->stream))) return rc;
        if (p->maps_g0) {
            // octave 0's maps: on the idle stream beside detection and refinement (two streams), else in line
            if (two) {
                HIPCHK(wait_pyr0(p->stream2));
                launch_gradient_maps(p, 0, 1, p->stream2);
                HIPCHK(hipEventRecord(p->ev_maps0, p->stream2));
            } else launch_gradient_maps(p, 0, 1, p->stream);
        }
        launch_detect_octave(p, 0, p->stream);
        // octave 0's gradient maps ran beside detection and refinement: only orientation and description read them
        if (p->maps_g0 && two) HIPCHK(hipStreamWaitEvent(p->stream, p->ev_maps0, 0));
        if ((rc = launch_describe_group(p, 0, p->stream, slot++))) return rc;
    }
    if (p->n_oct > 1) {
        // ---- the later octaves: octave 1 (group 1 when the chain forks, else part of group 2), then the octaves below (group 2)
        if (two) HIPCHK(wait_later(later));
        for (int oct = 1; oct < p->n_oct; oct++) {
            hipStream_t st = (oct == 1) ? later : below;
            if (oct == tail_first) {   // this octave and every later one: one launch (k_tail.hpp)
                if ((rc = launch_tail(p, oct, st))) return rc;
                break;
            }
            if ((rc = build_pyramid(oct, st))) return rc;
            launch_detect_octave(p, oct, st);
            if (oct == 1 && fork) {
                if (p->maps_g1) launch_gradient_maps(p, 1, 2, later);
                if ((rc = launch_describe_group(p, 1, later, slot++))) return rc;
            }
        }
        hipStream_t desc2 = below;
        if (split) {              // the two detection chains meet: orientation and description of the group follow octave 1's chain
            HIPCHK(hipEventRecord(p->ev_det2, below));
            HIPCHK(hipStreamWaitEvent(later, p->ev_det2, 0));
            desc2 = later;
        }
        if (p->maps_g1) launch_gradient_maps(p, fork ? 2 : 1, p->n_oct, desc2);
        if ((rc = launch_describe_group(p, 2, desc2, slot++))) return rc;
    }
    if (p->chain) { delete static_cast<Scope *>(p->chain); p->chain = nullptr; }   // no octave closed the light-profile bracket (n_oct == 0)
    if (slot == 0) {                           // no octave at all: the counters (min / max) still come back
        HIPCHK(hipMemcpyAsync(&p->hb->c[0], p->cnt, sizeof(Counters), hipMemcpyDeviceToHost, p->stream));
        p->wait_s[0] = p->stream;
    }
    // (Capturing this fork / join into a hipGraph was tried in round 2: it replays correctly, but a graph launch is no faster
    // than the plain launches: small images are bound by the GPU-side latency of dependent kernels, not by host launch cost.)
    p->fin = p->stream;       // copies of the records are issued here after the wait: ordered before the next image's kernels
    return SIFTMI_OK;
}

// wait for everything in flight on the plan's streams, ignoring errors (error paths only)
void drain_streams(siftmi_plan *p) {
    for (hipStream_t s : {p->stream, p->stream2, p->stream3})
        if (s) (void)hipStreamSynchronize(s);
    p->in_flight = false;
}

// The reference's capacity per octave, enforced after the fact on an image that broke it (rare: reference_overflow): at
// most kpsize records of each octave stay -- which ones is as arbitrary as in the reference, whose atomic counter decides.
// Device list compacted in place through a gather into a temporary; a pinned result array of the call is stale afterwards
// (records_cut: siftmi_plan_keypoints copies the list out again).
int cap_octaves(siftmi_plan *p, const Counters &c, int64_t *n_io) {
    std::vector<int32_t> keep;
    std::vector<int64_t> kept((size_t)SIFT_MAX_OCTAVES, 0);
    std::vector<int32_t> aux;
    bool cut = false;
    // the record blocks in list order
    std::vector<std::pair<int64_t, int>> blocks;            // (base, group)
    for (int g = 0; g < SIFT_GROUPS; g++)
        if ((p->groups_cur >> g) & 1u) blocks.push_back({(int64_t)(c.rec_word[g] & 0x7fffffffu), g});
    std::sort(blocks.begin(), blocks.end());
    for (auto &bg : blocks) {
        const int g = bg.second;
        const int64_t n = std::min<int64_t>(std::min<int64_t>(c.g_out[g], p->grp[g].cap_out), std::max<int64_t>(0, *n_io - bg.first));
        if (n <= 0) continue;
        aux.resize((size_t)n);
        HIPCHK(hipMemcpy(aux.data(), p->grp[g].oaux, (size_t)n * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < n; i++) {
            const int oct = std::min(std::max(aux[(size_t)i] >> 8, 0), SIFT_MAX_OCTAVES - 1);
            if (kept[(size_t)oct] < p->kpsize) { kept[(size_t)oct]++; keep.push_back((int32_t)(bg.first + i)); }
            else cut = true;
        }
    }
    if (!cut) return SIFTMI_OK;
    const size_t m = keep.size();
    int32_t *didx = nullptr; KpRecord *tmp = nullptr;
    if (hipMalloc((void **)&didx, std::max<size_t>(m, 1) * 4) != hipSuccess || hipMalloc((void **)&tmp, std::max<size_t>(m, 1) * sizeof(KpRecord)) != hipSuccess) {
        if (didx) (void)hipFree(didx);
        return fail(SIFTMI_ENOMEM, "hipMalloc failed while cutting the record list to the per-octave capacity");
    }
    hipError_t e = hipMemcpy(didx, keep.data(), m * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && m) {
        hipLaunchKernelGGL(gather_records_kernel, dim3((unsigned)std::min<size_t>((m * 36 + 255) / 256, 65535)), dim3(256), 0, p->stream,
                           (const KpRecord *)p->records, (const int *)didx, tmp, (int)m);
        e = hipMemcpyAsync(p->records, tmp, m * sizeof(KpRecord), hipMemcpyDeviceToDevice, p->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(p->stream);
    }
    (void)hipFree(didx); (void)hipFree(tmp);
    if (e != hipSuccess) return fail(SIFTMI_EDEVICE, "cutting the record list: %s", hipGetErrorString(e));
    *n_io = (int64_t)m;
    p->records_cut = true;
    return SIFTMI_OK;
}

// Wait for the image enqueued last on this plan; returns its record count (records stay on the device).
// SIFTMI_ETAILRETRY / SIFTMI_EGROW (internal): the image has to be enqueued again (the plan has been adjusted).
int plan_wait(siftmi_plan *p, int64_t *n_out, int32_t *overflow) {
    HIPCHK(hipSetDevice(p->device));
    // wait by polling: a blocking hipStreamSynchronize can add wake-up latency to a ~1 ms call
    const bool spin = p->opt.spin != 0;
    for (hipStream_t w : p->wait_s) {
        if (!w) continue;
        if (spin) {
            hipError_t q;
            while ((q = hipStreamQuery(w)) == hipErrorNotReady) __builtin_ia32_pause();
            if (q != hipSuccess) HIPCHK(q);
        }
        HIPCHK(hipStreamSynchronize(w));
    }
    HIPCHK(hipStreamSynchronize(p->stream));
    p->in_flight = false;
    HIPCHK(hipGetLastError());
    // The complete copy of the counters: the one taken after every group of the image had reserved its record block
    // (a group reserves when its descriptor launch starts, i.e. after its orientation launch; the stream that ends last
    // copied after all of them).
    const Counters *hcp = nullptr;
    bool tail_timed_out = false;
    for (int k = 0; k < 3; k++) {
        if (!p->wait_s[k]) continue;
        const Counters &c = p->hb->c[k];
        tail_timed_out = tail_timed_out || c.tail_timeout;
        bool complete = true;
        for (int g = 0; g < SIFT_GROUPS; g++) if (((p->groups_cur >> g) & 1u) && !(c.rec_word[g] & 0x80000000u)) complete = false;
        if (complete && (!hcp || c.n_rec >= hcp->n_rec)) hcp = &c;
    }
    if (!hcp) { drain_streams(p); return fail(SIFTMI_EDEVICE, "no complete copy of the image's counters came back"); }
    const Counters &hc = *hcp;
    p->last_min = minmax_decode(hc.mm[0]); p->last_max = minmax_decode(hc.mm[1]);
    if (!tail_timed_out && p->opt.tail_fault > 0 && p->opt.tail) { p->opt.tail_fault--; tail_timed_out = true; }   // injected (option "tail_fault")
    if (tail_timed_out) {
        // a workgroup of octave_tail_kernel stopped waiting for the octave above (k_tail.hpp): this image is incomplete.
        // From now on the plan walks the small octaves with the per-octave launches; the caller runs the image again.
        p->opt.tail = 0;
        p->tail_timeouts++;
        drain_streams(p);
        return fail(SIFTMI_ETAILRETRY, "octave_tail_kernel timed out waiting for the previous octave; tail launches disabled for this plan");
    }
    // A candidate list with provisional scale-3 entries in it (lazy top plane) holds more than the eager form's: where it was
    // cut, the image runs again eagerly, so that growth, the capacity rule and the cut act on the counts they are defined on.
    for (int o = 0; o < p->n_oct && o < SIFT_MAX_OCTAVES; o++)
        if (p->lazy_cur[o] && hc.n_cand[o] > p->grp[cand_group_of(p, o)].cap_cand) {
            p->lazy_block = true;
            return fail(SIFTMI_EGROW, "provisional candidates outran the list; the image runs again with the full top plane");
        }
    {
        // a list that was cut at its buffer's size: grow it and run the image again (what lies behind the cut was never made)
        bool grown = false;
        int rc = grow_lists(p, &hc, &grown);
        if (rc) return rc;
        if (grown) return fail(SIFTMI_EGROW, "a keypoint list was grown; the image runs again");
    }
    int64_t n = 0;
    for (int g = 0; g < SIFT_GROUPS; g++) if ((p->groups_cur >> g) & 1u) n += std::min<int64_t>(hc.g_out[g], p->grp[g].cap_out);
    n = std::min<int64_t>(std::min<int64_t>(n, hc.n_rec), p->cap_rec);
    // the reference's rule: kpsize entries per octave (see reference_overflow); an image that breaks it is flagged and cut to it
    int ovf = reference_overflow(p, hc) ? 1 : 0;
    // (a list that cannot grow any further has been cut: only an image beyond that rule gets there)
    for (int g = 0; g < SIFT_GROUPS; g++)
        if (((p->groups_cur >> g) & 1u) && (hc.g_kp[g] > p->grp[g].cap_kp || hc.g_out[g] > p->grp[g].cap_out)) ovf = 1;
    if (hc.n_rec > p->cap_rec) ovf = 1;
    // ... and so has a candidate list that stayed cut (grow_lists stops at what the reference's rule can admit): the per-scale
    // counts reference_overflow sees were taken from the cut list, so the cut itself is the evidence
    for (int g = 0; g < SIFT_GROUPS; g++) {
        if (!((p->groups_cur >> g) & 1u) || p->grp[g].cap_cand <= 0) continue;
        for (int o = 0; o < p->n_oct; o++)
            if (o < SIFT_MAX_OCTAVES && cand_group_of(p, o) == g && hc.n_cand[o] > p->grp[g].cap_cand) ovf = 1;
    }
    p->records_cut = false;
    if (ovf) { int rc = cap_octaves(p, hc, &n); if (rc) return rc; }
    if (p->profile == 1) {                   // light profile: running totals, read once by the caller's benchmark loop
        float tot = 0, bms = 0; int32_t bl = 0; double px = 0;
        if (siftmi_plan_last_kernel_ms(p, &tot, nullptr, nullptr, nullptr) == SIFTMI_OK && siftmi_plan_blur_ms(p, 0, &bms, &bl, &px) == SIFTMI_OK) {
            p->acc_calls++; p->acc_total_ms += tot; p->acc_b0_ms += bms; p->acc_b0_launches += bl; p->acc_b0_pixels += px;
        }
    }
    p->last_count = n;
    p->last_overflow = ovf;
    p->last_tail_first = p->tail_first_cur;
    for (int o = 0; o < SIFT_MAX_OCTAVES; o++) {
        p->last_n_cand[o] = hc.n_cand[o] + (o == 0 ? hc.n_cand[SIFT_MAX_OCTAVES] : 0);   // (the slot of a split octave 0 belongs to octave 0)
        for (int s = 0; s < 3; s++) p->last_c_scale[o][s] = hc.c_scale[o][s];
        // lazy top plane: the list also held the provisional entries top_patch_kernel turned into holes; the candidates are what
        // the refinement read (the list was not cut: see above)
        if (p->lazy_cur[o]) p->last_n_cand[o] = hc.c_scale[o][0] + hc.c_scale[o][1] + hc.c_scale[o][2];
        p->lazy_last[o] = p->lazy_ran[o] = p->lazy_cur[o];      // (lazy_last is cleared when siftmi_plan_planes completes the plane)
    }
    p->lazy_seen = true;
    p->lazy_block = false;
    p->last_valid = true;
    p->last_group0 = (int)std::min<int64_t>(hc.g_out[0], n);
    p->last_group1 = (int)n - p->last_group0;
    *n_out = n;
    if (overflow) *overflow = ovf;
    return SIFTMI_OK;
}

// One image, start to finish: enqueue + wait, run again when the plan had to be adjusted under it -- once after a tail
// time-out (plan_wait has switched to the per-octave launches), and after every growth of a list (at most one per list
// stage: candidates, refined, oriented, records; what lies behind a cut list only shows once the list is whole).
int plan_run(siftmi_plan *p, const void *image, int32_t image_dtype, int32_t image_is_device, bool sync_device, int64_t *n, int32_t *ovf) {
    int rc = SIFTMI_OK, tail_retries = 0;
    for (int attempt = 0; attempt < 12; attempt++) {
        rc = plan_enqueue(p, image, image_dtype, image_is_device, sync_device);
        if (!rc) rc = plan_wait(p, n, ovf);
        if (rc == SIFTMI_ETAILRETRY && tail_retries++ == 0) continue;
        if (rc == SIFTMI_EGROW) continue;
        break;
    }
    if (rc == SIFTMI_ETAILRETRY || rc == SIFTMI_EGROW) rc = SIFTMI_EDEVICE;
    // A failed enqueue or wait must not leave the plan marked busy: the next call would then report "still has an image in
    // flight" instead of this error.  Whatever was launched is drained here (the message of `rc` stays the last error).
    if (rc && p->in_flight) { const std::string keep = g_err; drain_streams(p); g_err = keep; }
    return rc;
}
}  // namespace

extern "C" {

int siftmi_plan_keypoints(siftmi_plan *p, const void *image, int32_t image_dtype, int32_t image_is_device, siftmi_keypoint *out,
                          int32_t out_is_device, int64_t capacity, int64_t *n_out, int32_t *overflow) {
    if (!p || !image || !n_out) return fail(SIFTMI_EINVAL, "null argument");
    if (capacity > 0 && !out) return fail(SIFTMI_EINVAL, "null output with capacity > 0");
    if (out_is_device < 0 || out_is_device > SIFTMI_OUT_PINNED) return fail(SIFTMI_EINVAL, "out_is_device must be 0 (host), 1 (device) or 2 (pinned host)");
    *n_out = 0;
    if (overflow) *overflow = 0;
    // Pinned host result array (siftmi_host_alloc): the descriptor kernels write every record to it as well (zero-copy over
    // PCIe while they run), so nothing is left to copy once the last kernel has ended.
    const bool pinned = out_is_device == SIFTMI_OUT_PINNED && out && capacity > 0;
    p->host_out = pinned ? reinterpret_cast<KpRecord *>(out) : nullptr;
    p->host_cap = pinned ? (int)(capacity < 0x7fffffff ? capacity : 0x7fffffff) : 0;
    int64_t n = 0;
    int32_t ovf = 0;
    // a device result array: ordered after what the caller's streams were given for it (siftmi.h, conventions); a device frame
    // is synchronised for by plan_enqueue
    if (out_is_device == SIFTMI_OUT_DEVICE && out && capacity > 0 && !image_is_device) {
        HIPCHK(hipSetDevice(p->device));
        HIPCHK(hipDeviceSynchronize());
    }
    int rc = plan_run(p, image, image_dtype, image_is_device, true, &n, &ovf);
    p->host_out = nullptr; p->host_cap = 0;
    if (rc) {
        // descriptor kernels that were already launched may still be writing to the caller's pinned block: nothing
        // returns before every stream of the plan has drained (the caller recycles the block on an error)
        if (pinned) drain_streams(p);
        return rc;
    }
    hipStream_t fin = p->fin;
    if (out == nullptr && capacity == 0) {
        // count-only call: the records stay on the device until siftmi_plan_fetch()
    } else {
        if (n > capacity) { n = capacity; rc = SIFTMI_ECAPACITY; g_err = "output capacity too small; result truncated"; }
        // (pinned: the kernels have written the records already -- unless the list was cut to the per-octave capacity afterwards)
        if (n > 0 && (!pinned || p->records_cut)) {
            HIPCHK(hipMemcpyAsync(out, p->records, (size_t)n * sizeof(KpRecord),
                                  out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, fin));
            HIPCHK(hipStreamSynchronize(fin));
        }
    }
    *n_out = n;
    if (overflow) *overflow = ovf;
    return rc;
}


int siftmi_plan_fetch(siftmi_plan *p, siftmi_keypoint *out, int32_t out_is_device, int64_t first, int64_t count) {
    if (!p || (count > 0 && !out)) return fail(SIFTMI_EINVAL, "null argument");
    // (no sum of the two: first + count can overflow)
    if (first < 0 || count < 0 || first > p->last_count || count > p->last_count - first) return fail(SIFTMI_EINVAL, "record range out of bounds");
    if (count == 0) return SIFTMI_OK;
    HIPCHK(hipSetDevice(p->device));
    if (out_is_device) HIPCHK(hipDeviceSynchronize());   // a device destination: ordered after the caller's streams (siftmi.h, conventions)
    HIPCHK(hipMemcpyAsync(out, p->records + first, (size_t)count * sizeof(KpRecord),
                          out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    return SIFTMI_OK;
}

// The six blur planes of one octave as the last finished call left them (see include/siftmi.h).  The plan's streams are waited
// for (they are idle after plan_wait) and the planes are copied out; nothing is launched but the top plane's blur of an
// octave that went without it (option "lazy_top").
int siftmi_plan_planes(siftmi_plan *p, int32_t octave, float *out, int64_t capacity, int32_t *width, int32_t *height) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (!out) return fail(SIFTMI_EINVAL, "null output buffer");
    if (octave < 0 || octave >= p->n_oct) return fail(SIFTMI_EINVAL, "octave %d outside 0..%d", octave, p->n_oct - 1);
    if (!p->last_valid || p->in_flight) return fail(SIFTMI_EINVAL, "the plan has not finished a call: there are no planes to read");
    const int W = p->ow[(size_t)octave], H = p->oh[(size_t)octave];
    const int64_t need = 6 * (int64_t)W * H;
    if (capacity < need) return fail(SIFTMI_EINVAL, "buffer of %lld floats, octave %d needs 6 * %d * %d", (long long)capacity, octave, W, H);
    HIPCHK(hipSetDevice(p->device));
    for (hipStream_t s : {p->stream2, p->stream3})
        if (s) HIPCHK(hipStreamSynchronize(s));
    if (octave < SIFT_MAX_OCTAVES && p->lazy_last[octave]) {
        // the last call wrote plane 5 of this octave only around its scale-3 candidates (option "lazy_top"): the launch it
        // went without runs now (the patches hold the same bits)
        launch_blur(p, p->plane(octave, 4), p->plane(octave, 5), W, H, p->taps[4], false, p->stream);
        p->lazy_last[octave] = false;
    }
    HIPCHK(hipMemcpyAsync(out, p->plane(octave, 0), (size_t)need * sizeof(float), hipMemcpyDeviceToHost, p->stream));
    HIPCHK(hipStreamSynchronize(p->stream));
    if (width) *width = W;
    if (height) *height = H;
    return SIFTMI_OK;
}

// Which octaves of the last finished call went without their full plane 5 (option "lazy_top"); see include/siftmi.h
int siftmi_plan_lazy_octaves(const siftmi_plan *p, int32_t *lazy, int32_t n_octaves) {
    if (!p || !lazy) return fail(SIFTMI_EINVAL, "null argument");
    if (n_octaves < p->n_oct) return fail(SIFTMI_EINVAL, "room for %d octaves, the plan has %d", n_octaves, p->n_oct);
    if (!p->last_valid || p->in_flight) return fail(SIFTMI_EINVAL, "the plan has not finished a call");
    for (int o = 0; o < p->n_oct; o++) lazy[o] = (o < SIFT_MAX_OCTAVES && p->lazy_ran[o]) ? 1 : 0;
    return SIFTMI_OK;
}

int siftmi_plan_last_counts(const siftmi_plan *p, int32_t *tail_first, int32_t *candidates, int32_t *c_scale, int32_t n_octaves) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (!tail_first || !candidates || !c_scale) return fail(SIFTMI_EINVAL, "null output");
    if (n_octaves < p->n_oct) return fail(SIFTMI_EINVAL, "room for %d octaves, the plan has %d", n_octaves, p->n_oct);
    if (!p->last_valid || p->in_flight) return fail(SIFTMI_EINVAL, "the plan has not finished a call: there are no counts to read");
    *tail_first = p->last_tail_first;
    for (int o = 0; o < p->n_oct; o++) {
        const bool held = o < SIFT_MAX_OCTAVES;       // (Counters holds SIFT_MAX_OCTAVES octaves; a frame never has more)
        candidates[o] = held ? p->last_n_cand[o] : 0;
        for (int s = 0; s < 3; s++) c_scale[3 * o + s] = held ? p->last_c_scale[o][s] : 0;
    }
    return SIFTMI_OK;
}

// The candidate list octave_tail_kernel kept for one of its octaves in the last finished call (see include/siftmi.h).  Nothing
// is launched; p->tail_cand is written by that launch alone (launch_tail), workgroup k = octave - tail_first at k * tail_cand_cap.
int siftmi_plan_tail_candidates(const siftmi_plan *p, int32_t octave, float *out, int64_t capacity, int64_t *count) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (!out || !count) return fail(SIFTMI_EINVAL, "null output");
    if (!p->last_valid || p->in_flight) return fail(SIFTMI_EINVAL, "the plan has not finished a call: there are no candidates to read");
    if (octave < p->last_tail_first || octave >= p->n_oct || octave >= SIFT_MAX_OCTAVES || octave - p->last_tail_first >= SIFT_TAIL_MAX_OCT)
        return fail(SIFTMI_EINVAL, "octave %d is not one of the tail launch's (%d..%d) in the run that produced the result", octave,
                    p->last_tail_first, p->n_oct - 1);
    const int64_t n = std::max(0, std::min(p->last_n_cand[octave], p->tail_cand_cap));
    if (capacity < 4 * n) return fail(SIFTMI_EINVAL, "buffer of %lld floats, octave %d needs 4 * %lld", (long long)capacity, octave, (long long)n);
    if (n > 0) {
        HIPCHK(hipSetDevice(p->device));
        for (hipStream_t s : {p->stream2, p->stream3})
            if (s) HIPCHK(hipStreamSynchronize(s));
        HIPCHK(hipMemcpyAsync(out, p->tail_cand + (size_t)(octave - p->last_tail_first) * p->tail_cand_cap, (size_t)n * sizeof(float4),
                              hipMemcpyDeviceToHost, p->stream));
        HIPCHK(hipStreamSynchronize(p->stream));
    }
    *count = n;
    return SIFTMI_OK;
}

// ---- batched, pipelined keypoints --------------------------------------------------------
// `lanes` independent plans (own planes, lists and streams) take the images round-robin.  Everything is enqueued
// without waiting; a lane is only waited for when it is about to be reused, and its records are then parked in a
// device arena by a device-to-device copy on the lane's own stream.  One device-to-host copy hands the whole batch back.
}  // extern "C"
struct siftmi_batch {
    int device = 0;
    std::vector<siftmi_plan *> lanes;
    std::vector<int> lane_image;          // image index in flight on each lane (-1: idle)
    uint8_t *arena = nullptr;             // parked records of the current batch, image after image
    size_t arena_cap = 0, arena_used = 0;
    std::vector<int64_t> counts, offsets;
    int64_t retired = 0, batch_size = 0;  // frames retired so far / frames in the current batch
    double blur0_ms = 0, blur0_pixels = 0;         // light profiling: octave-0 blur brackets summed over the frames of the batch
    int64_t blur0_launches = 0;
    siftmi_keypoint *const *host_outs = nullptr;   // optional: one caller-owned host array per frame, filled while the batch runs
    const int64_t *host_caps = nullptr;            // their capacities in records (a frame that does not fit stays parked in the arena)
    // host frames: uploads run on ONE copy stream, in frame order, one frame ahead of the kernel enqueue, into a ring of
    // lanes + 1 staging buffers (a lane's own staging buffer would hold its next upload back until its frame has retired:
    // with two lanes both uploads then share the link, both pyramids start together and the link idles while they run --
    // 4096^2 frames: 1.53 ms per frame against 1.16 ms of PCIe time)
    std::vector<void *> ring;
    std::vector<hipEvent_t> ring_ev;
    size_t ring_bytes = 0;
    hipStream_t copy_stream = nullptr;             // (the two halves of a frame on two copy streams -- two SDMA engines -- measured
                                                   // no better: 1.27-1.45 against 1.30-1.31 ms per 4096^2 frame on one box)
    const void *const *cur_images = nullptr;       // the frames of the call in progress (a lane re-runs its frame after a tail time-out)
    int32_t cur_dtype = 0, cur_is_device = 0;
    int64_t tail_retries = 0;                      // frames re-run since the batch was created
    // min / max of every frame of the batch, recorded under the frame's index as its lane retires (siftmi_batch_minmax);
    // mm_frames: frames of the last FINISHED batch, -1 while none has finished (none yet, one in progress, the last one failed)
    std::vector<float> mins, maxs;
    int64_t mm_frames = -1;
    // siftmi_batch_transform: staging of host frames and of a host output, the table of frames (pinned block and its device
    // copy), all grown on demand and counted by siftmi_batch_info
    void *warp_in = nullptr, *warp_out = nullptr, *warp_tab = nullptr, *warp_tab_host = nullptr;
    size_t warp_in_bytes = 0, warp_out_bytes = 0, warp_tab_bytes = 0, warp_tab_host_bytes = 0;
    hipEvent_t ev_wa = nullptr, ev_wb = nullptr;
};
extern "C" {

int siftmi_batch_destroy(siftmi_batch *b) {
    if (!b) return SIFTMI_OK;
    for (siftmi_plan *p : b->lanes) siftmi_plan_destroy(p);
    hipSetDevice(b->device);
    if (b->arena) hipFree(b->arena);
    for (void *q : b->ring) hipFree(q);
    for (hipEvent_t e : b->ring_ev) hipEventDestroy(e);
    if (b->copy_stream) hipStreamDestroy(b->copy_stream);
    for (void *q : {b->warp_in, b->warp_out, b->warp_tab}) if (q) hipFree(q);
    if (b->warp_tab_host) hipHostFree(b->warp_tab_host);
    if (b->ev_wa) hipEventDestroy(b->ev_wa);
    if (b->ev_wb) hipEventDestroy(b->ev_wb);
    delete b;
    return SIFTMI_OK;
}

int siftmi_batch_create(int32_t height, int32_t width, int32_t in_dtype, int32_t device_id, const siftmi_params *params,
                        int32_t lanes, siftmi_batch **out) {
    if (!out) return fail(SIFTMI_EINVAL, "null argument");
    *out = nullptr;
    if (lanes < 1 || lanes > 64) return fail(SIFTMI_EINVAL, "lanes must be in 1..64, got %d", lanes);
    siftmi_batch *b = new (std::nothrow) siftmi_batch();
    if (!b) return fail(SIFTMI_ENOMEM, "host allocation failed");
    b->device = device_id;
    for (int l = 0; l < lanes; l++) {
        siftmi_plan *p = nullptr;
        // Small frames with many lanes: one stream per lane, all at the same priority.  Lanes already overlap each other,
        // and three streams per lane oversubscribe the hardware queues (512^2, 8 lanes: 0.70 ms per frame with three
        // streams, 0.43 ms with one; priorities between peer lanes cost another 20 %).  Few lanes of large frames keep the
        // three prioritised streams of a plain plan (4096^2, 2 lanes: 1.05 ms per frame with, 1.40 ms without priorities).
        const bool single_stream = lanes >= 4 && (int64_t)height * width <= (int64_t)2048 * 2048;
        g_lane_mode = single_stream ? 1 : 2;
        int rc = siftmi_plan_create(height, width, in_dtype, device_id, params, 0, &p);
        g_lane_mode = 0;
        if (rc) { std::string keep = g_err; siftmi_batch_destroy(b); g_err = keep; return rc; }
        if (single_stream) p->overlap = false;
        b->lanes.push_back(p);
        b->lane_image.push_back(-1);
    }
    *out = b;
    return SIFTMI_OK;
}

int siftmi_batch_set_params(siftmi_batch *b, const siftmi_params *params) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    for (siftmi_plan *p : b->lanes) { int rc = siftmi_plan_set_params(p, params); if (rc) return rc; }
    return SIFTMI_OK;
}

int siftmi_batch_set_option(siftmi_batch *b, const char *name, int64_t value) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    for (siftmi_plan *p : b->lanes) { int rc = siftmi_plan_set_option(p, name, value); if (rc) return rc; }
    return SIFTMI_OK;
}

int siftmi_batch_set_profile(siftmi_batch *b, int32_t level) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (level < 0 || level > 1) return fail(SIFTMI_EINVAL, "batch lanes support profile 0 or 1 (light)");
    for (siftmi_plan *p : b->lanes) p->profile = level;
    return SIFTMI_OK;
}

int siftmi_batch_blur_ms(const siftmi_batch *b, double *blur_ms, int64_t *blur_launches, double *blur_pixels) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (blur_ms) *blur_ms = b->blur0_ms;
    if (blur_launches) *blur_launches = b->blur0_launches;
    if (blur_pixels) *blur_pixels = b->blur0_pixels;
    return SIFTMI_OK;
}

int siftmi_batch_info(const siftmi_batch *b, int32_t *lanes, int64_t *bytes_allocated) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (lanes) *lanes = (int32_t)b->lanes.size();
    if (bytes_allocated) {
        int64_t t = (int64_t)b->arena_cap + (int64_t)(b->ring.size() * b->ring_bytes) +
                    (int64_t)(b->warp_in_bytes + b->warp_out_bytes + b->warp_tab_bytes);
        for (const siftmi_plan *p : b->lanes) t += p->bytes;
        *bytes_allocated = t;
    }
    return SIFTMI_OK;
}

int siftmi_batch_tail_timeouts(const siftmi_batch *b, int64_t *timeouts, int32_t *lanes_with_tail) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    int64_t t = 0; int32_t on = 0;
    for (const siftmi_plan *p : b->lanes) { t += p->tail_timeouts; on += p->opt.tail ? 1 : 0; }
    if (timeouts) *timeouts = t;
    if (lanes_with_tail) *lanes_with_tail = on;
    return SIFTMI_OK;
}

}  // extern "C"
namespace {
// lane `l` has finished its image: learn the count and park the records in the arena (async D->D on the lane's stream)
int batch_retire(siftmi_batch *b, size_t l, int32_t *overflow) {
    siftmi_plan *p = b->lanes[l];
    const int img = b->lane_image[l];
    if (img < 0) return SIFTMI_OK;
    if (img >= b->batch_size) { b->lane_image[l] = -1; return fail(SIFTMI_EINVAL, "stale frame index %d on lane %zu", img, l); }
    int64_t n = 0; int32_t ovf = 0;
    int rc = plan_wait(p, &n, &ovf);
    if ((rc == SIFTMI_ETAILRETRY || rc == SIFTMI_EGROW) && b->cur_images) {
        // A workgroup of octave_tail_kernel gave up waiting (k_tail.hpp: most likely queued behind another lane's persistent
        // descriptor workgroups -- a batch-only condition) and plan_wait has switched the lane to the per-octave launches, or
        // the frame outran a list of the lane and plan_wait has grown it: the frame runs again on the same lane, as
        // siftmi_plan_keypoints does for a single plan (plan_run).
        if (rc == SIFTMI_ETAILRETRY) b->tail_retries++;
        // (a host frame is still in its ring slot: the slot is not reused before its frame has retired)
        const bool staged = !b->cur_is_device && !b->ring.empty();
        rc = plan_run(p, staged ? b->ring[(size_t)img % b->ring.size()] : b->cur_images[img], b->cur_dtype, staged ? 1 : b->cur_is_device, false, &n, &ovf);
    }
    if (rc == SIFTMI_ETAILRETRY || rc == SIFTMI_EGROW) rc = fail(SIFTMI_EDEVICE, "frame %d could not be completed after its plan was adjusted", img);
    if (rc) return rc;
    if (ovf && overflow) *overflow = 1;
    if (p->profile) {
        float ms = 0; int32_t nl = 0; double px = 0;
        if (siftmi_plan_blur_ms(p, 0, &ms, &nl, &px) == SIFTMI_OK) { b->blur0_ms += ms; b->blur0_launches += nl; b->blur0_pixels += px; }
    }
    const size_t bytes = (size_t)n * sizeof(KpRecord);
    if (b->host_outs && b->host_outs[img] && n <= b->host_caps[img]) {
        // straight into the caller's array for this frame: a blocking copy of one frame's records (~1.5 MB) costs the
        // host ~0.1 ms while the other lanes keep the GPU busy -- cheaper than parking everything and copying it at the end
        if (n > 0) {
            HIPCHK(hipMemcpyAsync(b->host_outs[img], p->records, bytes, hipMemcpyDeviceToHost, p->fin));
            HIPCHK(hipStreamSynchronize(p->fin));
        }
        b->counts[(size_t)img] = n;
        b->mins[(size_t)img] = p->last_min; b->maxs[(size_t)img] = p->last_max;
        b->offsets[(size_t)img] = -1;                 // delivered
        b->retired++;
        b->lane_image[l] = -1;
        return SIFTMI_OK;
    }
    const size_t need = b->arena_used + bytes;
    if (need > b->arena_cap) {
        // grow to the projected size of the whole batch (records so far / frames retired x frames of the batch,
        // +25 %), so that a batch regrows the arena at most a couple of times: each regrow drains the device
        size_t cap = b->arena_cap ? b->arena_cap : ((size_t)1 << 22);
        const size_t projected = (size_t)((double)need / (double)(b->retired + 1) * (double)b->batch_size * 1.25);
        while (cap < need || cap < projected) cap *= 2;
        uint8_t *bigger = nullptr;
        hipError_t e = hipMalloc((void **)&bigger, cap);
        if (e != hipSuccess) return fail(SIFTMI_ENOMEM, "hipMalloc(%zu): %s", cap, hipGetErrorString(e));
        if (b->arena_used) {
            HIPCHK(hipDeviceSynchronize());               // earlier parking copies may still be in flight
            HIPCHK(hipMemcpy(bigger, b->arena, b->arena_used, hipMemcpyDeviceToDevice));
        }
        if (b->arena) { HIPCHK(hipDeviceSynchronize()); hipFree(b->arena); }
        b->arena = bigger; b->arena_cap = cap;
    }
    if (n > 0)
        HIPCHK(hipMemcpyAsync(b->arena + b->arena_used, p->records, bytes, hipMemcpyDeviceToDevice, p->fin));
    b->counts[(size_t)img] = n;
    b->mins[(size_t)img] = p->last_min; b->maxs[(size_t)img] = p->last_max;
    b->offsets[(size_t)img] = (int64_t)(b->arena_used / sizeof(KpRecord));
    b->arena_used = need;
    b->retired++;
    b->lane_image[l] = -1;
    return SIFTMI_OK;
}

// Forget whatever is still in flight on the lanes (an earlier call that ended with an error): wait for each lane's
// streams, ignore the results, mark every lane idle.  Without this the next call would retire stale image indices
// into arrays sized for ITS batch.
void batch_drain(siftmi_batch *b) {
    for (size_t l = 0; l < b->lanes.size(); l++) {
        if (b->lane_image[l] < 0) continue;
        siftmi_plan *p = b->lanes[l];
        if (hipSetDevice(p->device) == hipSuccess) {
            drain_streams(p);
        }
        b->lane_image[l] = -1;
    }
}
}  // namespace
extern "C" {

int siftmi_batch_keypoints_into(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t image_dtype,
                                int32_t images_are_device, siftmi_keypoint *const *host_outs, const int64_t *host_caps,
                                int64_t *counts, int64_t *offsets, int64_t *total_parked, int32_t *overflow) {
    if (!b || (n_images > 0 && !images) || !counts || !offsets || !total_parked) return fail(SIFTMI_EINVAL, "null argument");
    if (n_images < 0) return fail(SIFTMI_EINVAL, "negative image count");
    if ((host_outs == nullptr) != (host_caps == nullptr)) return fail(SIFTMI_EINVAL, "host_outs and host_caps go together");
    if (dtype_size(image_dtype) == 0) return fail(SIFTMI_EINVAL, "invalid input format (%d)", image_dtype);
    if (!b->lanes.empty() && image_dtype != b->lanes[0]->dtype && image_dtype != SIFTMI_F32)
        return fail(SIFTMI_EINVAL, "image dtype %d is neither the plan's (%d) nor float32", image_dtype, b->lanes[0]->dtype);
    HIPCHK(hipSetDevice(b->device));
    batch_drain(b);                      // no-op unless the previous call failed half way
    if (overflow) *overflow = 0;
    *total_parked = 0;
    b->arena_used = 0;
    b->retired = 0; b->batch_size = n_images;
    b->blur0_ms = 0; b->blur0_pixels = 0; b->blur0_launches = 0;
    b->host_outs = host_outs; b->host_caps = host_caps;
    b->cur_images = images; b->cur_dtype = image_dtype; b->cur_is_device = images_are_device;
    b->counts.assign((size_t)n_images, 0);
    b->offsets.assign((size_t)n_images, 0);
    b->mm_frames = -1;
    b->mins.assign((size_t)n_images, 0.0f);
    b->maxs.assign((size_t)n_images, 0.0f);
    const size_t L = b->lanes.size();
    int rc = SIFTMI_OK;
    // (from here on an error must not return at once: the lanes and the copy stream may be reading the caller's frames or
    // writing its arrays -- every failure goes through the drain at the end)
#define BATCHCHK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess && !rc) rc = fail(e_ == hipErrorOutOfMemory ? SIFTMI_ENOMEM : SIFTMI_EDEVICE, "%s: %s", #expr, hipGetErrorString(e_)); } while (0)
    if (images_are_device) BATCHCHK(hipDeviceSynchronize());   // once per batch: order after the caller's streams
    const bool htime = L > 0 && b->lanes[0]->opt.host_timing;   // diagnostic: where the host thread spends the batch
    double t_retire = 0, t_enqueue = 0;
    // host frames go through the upload ring (see siftmi_batch)
    const bool staged = !images_are_device && n_images > 0 && L > 0;
    const size_t frame_bytes = staged ? (size_t)b->lanes[0]->H * b->lanes[0]->W * dtype_size(image_dtype) : 0;
    if (staged && !rc) {
        if (b->ring_bytes < frame_bytes || b->ring.size() != L + 1) {
            BATCHCHK(hipDeviceSynchronize());
            for (void *q : b->ring) hipFree(q);
            b->ring.clear(); b->ring_bytes = 0;
            for (size_t k = 0; k < L + 1 && !rc; k++) {
                void *q = nullptr;
                BATCHCHK(hipMalloc(&q, frame_bytes));
                if (!rc) b->ring.push_back(q);
            }
            if (!rc) b->ring_bytes = frame_bytes;          // (counted by siftmi_batch_info: L + 1 staged frames in HBM)
            else { for (void *q : b->ring) hipFree(q); b->ring.clear(); }
        }
        // (the ring's events order a DMA copy before kernels of another stream: plain events, WITH their system-scope fence --
        // unlike the plan's kernel-to-kernel events, SIFT_SYNC_EVENT)
        while (b->ring_ev.size() < L + 1 && !rc) { hipEvent_t e = nullptr; BATCHCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming)); if (!rc) b->ring_ev.push_back(e); }
        if (!b->copy_stream && !rc) BATCHCHK(hipStreamCreateWithFlags(&b->copy_stream, hipStreamNonBlocking));
    }
    auto upload = [&](int i) -> int {             // frame i -> ring slot i % (L + 1); the slot's previous frame (i - L - 1) has retired
        if (!images[i]) return fail(SIFTMI_EINVAL, "null image %d", i);
        const size_t k = (size_t)i % (L + 1);
        HIPCHK(hipMemcpyAsync(b->ring[k], images[i], frame_bytes, hipMemcpyHostToDevice, b->copy_stream));
        HIPCHK(hipEventRecord(b->ring_ev[k], b->copy_stream));
        return SIFTMI_OK;
    };
    if (staged && !rc) rc = upload(0);
    for (int i = 0; i < n_images && !rc; i++) {
        if (!images[i]) { rc = fail(SIFTMI_EINVAL, "null image %d", i); break; }
        const size_t l = (size_t)i % L;
        const double ta = htime ? tnow() : 0;
        if ((rc = batch_retire(b, l, overflow))) break;
        const double tb = htime ? tnow() : 0;
        if (htime) b->lanes[l]->opt.host_timing = 0;             // the per-call line would flood
        if (staged) {
            // frame i - L has just retired, so has every earlier one: slot (i + 1) % (L + 1), last used by frame i - L, is free
            if (i + 1 < n_images && (rc = upload(i + 1))) break;
            const size_t k = (size_t)i % (L + 1);
            BATCHCHK(hipStreamWaitEvent(b->lanes[l]->stream, b->ring_ev[k], 0));
            if (!rc) rc = plan_enqueue(b->lanes[l], b->ring[k], image_dtype, 1, false);
        } else
        rc = plan_enqueue(b->lanes[l], images[i], image_dtype, images_are_device, false);
        if (htime) { b->lanes[l]->opt.host_timing = 1; t_retire += tb - ta; t_enqueue += tnow() - tb; }
        if (rc) break;
        b->lane_image[l] = i;
    }
    if (htime) fprintf(stderr, "[siftmi] batch of %d: waiting for lanes %.0f us, enqueueing %.0f us\n", n_images, t_retire, t_enqueue);
    for (int i = n_images > (int)L ? n_images - (int)L : 0; i < n_images && !rc; i++) rc = batch_retire(b, (size_t)i % L, overflow);
    b->host_outs = nullptr; b->host_caps = nullptr; b->cur_images = nullptr;
    if (!rc) BATCHCHK(hipDeviceSynchronize());                 // the parking copies
    if (rc) {                                // nothing of this call may still read the caller's frames or write its arrays
        std::string keep = g_err;
        if (b->copy_stream) (void)hipStreamSynchronize(b->copy_stream);
        batch_drain(b);
        b->arena_used = 0;                   // a failed call leaves nothing to fetch (and no min / max: mm_frames is -1)
        g_err = keep;
        return rc;
    }
#undef BATCHCHK
    for (int i = 0; i < n_images; i++) { counts[i] = b->counts[(size_t)i]; offsets[i] = b->offsets[(size_t)i]; }
    *total_parked = (int64_t)(b->arena_used / sizeof(KpRecord));
    b->mm_frames = n_images;
    return SIFTMI_OK;
}

int siftmi_batch_keypoints(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t image_dtype,
                           int32_t images_are_device, int64_t *counts, int64_t *offsets, int64_t *total, int32_t *overflow) {
    return siftmi_batch_keypoints_into(b, images, n_images, image_dtype, images_are_device, nullptr, nullptr, counts, offsets, total,
                                       overflow);
}

int siftmi_batch_fetch(siftmi_batch *b, siftmi_keypoint *out, int32_t out_is_device, int64_t first, int64_t count) {
    if (!b || (count > 0 && !out)) return fail(SIFTMI_EINVAL, "null argument");
    // in records, and without a sum of the two: first + count can overflow, and so can its product with the record size
    const int64_t total = (int64_t)(b->arena_used / sizeof(KpRecord));
    if (first < 0 || count < 0 || first > total || count > total - first) return fail(SIFTMI_EINVAL, "record range out of bounds");
    if (count == 0) return SIFTMI_OK;
    HIPCHK(hipSetDevice(b->device));
    // a device destination: ordered after the caller's streams (siftmi.h, conventions) -- the copy below runs on the NULL stream,
    // which does not wait for the non-blocking streams a caller such as PyTorch works on
    if (out_is_device) HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, b->arena + (size_t)first * sizeof(KpRecord), (size_t)count * sizeof(KpRecord),
                     out_is_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost));
    // a device-to-device hipMemcpy need not wait on the host; the result is complete on return for readers on any stream
    if (out_is_device) HIPCHK(hipStreamSynchronize(nullptr));
    return SIFTMI_OK;
}

int siftmi_batch_minmax(const siftmi_batch *b, float *mins, float *maxs, int32_t n_images) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (b->mm_frames < 0) return fail(SIFTMI_EINVAL, "no batch has finished on this handle");
    if ((int64_t)n_images != b->mm_frames) return fail(SIFTMI_EINVAL, "the last batch had %lld frames, not %d", (long long)b->mm_frames, n_images);
    for (int32_t i = 0; i < n_images; i++) {
        if (mins) mins[i] = b->mins[(size_t)i];
        if (maxs) maxs[i] = b->maxs[(size_t)i];
    }
    return SIFTMI_OK;
}

namespace {
// a device buffer of the batch handle, replaced by a larger one when `need` outgrows it (nothing of its contents is kept)
int grow_device(void **ptr, size_t *cap, size_t need) {
    if (*ptr && need <= *cap) return SIFTMI_OK;
    if (*ptr) { HIPCHK(hipDeviceSynchronize()); hipFree(*ptr); }
    *ptr = nullptr; *cap = 0;
    hipError_t e = hipMalloc(ptr, need ? need : 16);
    if (e != hipSuccess) { *ptr = nullptr; return fail(SIFTMI_ENOMEM, "hipMalloc(%zu): %s", need, hipGetErrorString(e)); }
    *cap = need ? need : 16;
    return SIFTMI_OK;
}
}  // namespace

namespace {
// What siftmi_batch_transform and siftmi_batch_stack share around their launch.
struct WarpIo {
    hipStream_t stream = nullptr;
    int W = 0, H = 0;
    void *dst = nullptr;                           // where the kernel writes: the caller's device output, or the batch's staging
};

// Before the launch: the ordering after the caller's streams for device pointers, the batch-owned buffers (staging of host frames
// and of a host result of `out_bytes`, the table of `n_images` frames as a pinned block and its device copy), the upload of
// host frames -- one copy per run of frames that lie back to back in host memory (a stack is ONE copy) -- and of the table.
int warp_begin(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t images_are_device, size_t px, void *out,
               int32_t out_is_device, size_t out_bytes, const float *maps, const float *fills, int32_t mode, WarpIo *io,
               bool state_is_device = false) {
    HIPCHK(hipSetDevice(b->device));
    siftmi_plan *p0 = b->lanes[0];
    hipStream_t stream = p0->stream;               // every lane is idle between two calls on the handle
    const int W = p0->W, H = p0->H;
    const size_t in_bytes = (size_t)W * H * px;
    // a device pointer on either side: ordered after what the caller's streams were given for it (siftmi.h, conventions)
    // (`state_is_device`: the call takes further device pointers, the planes of siftmi_batch_stack_accum[_result])
    if ((images_are_device && n_images > 0) || out_is_device || state_is_device) HIPCHK(hipDeviceSynchronize());
    int rc;
    if (!images_are_device && (rc = grow_device(&b->warp_in, &b->warp_in_bytes, in_bytes * (size_t)n_images))) return rc;
    if (!out_is_device && (rc = grow_device(&b->warp_out, &b->warp_out_bytes, out_bytes))) return rc;
    const size_t tab_bytes = sizeof(WarpFrame) * (size_t)n_images;
    if ((rc = grow_device(&b->warp_tab, &b->warp_tab_bytes, tab_bytes))) return rc;
    if (b->warp_tab_host_bytes < tab_bytes) {
        if (b->warp_tab_host) hipHostFree(b->warp_tab_host);
        b->warp_tab_host = nullptr; b->warp_tab_host_bytes = 0;
        size_t cap = 4096;
        while (cap < tab_bytes) cap *= 2;
        hipError_t e = hipHostMalloc(&b->warp_tab_host, cap, hipHostMallocDefault);
        if (e != hipSuccess) { b->warp_tab_host = nullptr; return fail(SIFTMI_ENOMEM, "hipHostMalloc(%zu): %s", cap, hipGetErrorString(e)); }
        b->warp_tab_host_bytes = cap;
    }
    if (!b->ev_wa) { HIPCHK(hipEventCreate(&b->ev_wa)); HIPCHK(hipEventCreate(&b->ev_wb)); }
    if (!images_are_device) {
        for (int32_t i = 0; i < n_images;) {
            int32_t j = i + 1;
            while (j < n_images && (const uint8_t *)images[j] == (const uint8_t *)images[j - 1] + in_bytes) j++;
            hipError_t e = hipMemcpyAsync((uint8_t *)b->warp_in + (size_t)i * in_bytes, images[i], in_bytes * (size_t)(j - i), hipMemcpyHostToDevice, stream);
            if (e != hipSuccess) { (void)hipStreamSynchronize(stream); return fail(SIFTMI_EDEVICE, "hipMemcpyAsync: %s", hipGetErrorString(e)); }
            i = j;
        }
    }
    if (n_images > 0) {
        WarpFrame *tab = static_cast<WarpFrame *>(b->warp_tab_host);
        for (int32_t i = 0; i < n_images; i++) {
            const float *m = maps + 6 * (size_t)i;
            tab[i].image = images_are_device ? images[i] : (const void *)((const uint8_t *)b->warp_in + (size_t)i * in_bytes);
            tab[i].a = AffineArgs{m[0], m[1], m[2], m[3], m[4], m[5], fills[i], mode};
        }
        HIPCHK(hipMemcpyAsync(b->warp_tab, tab, tab_bytes, hipMemcpyHostToDevice, stream));
    }
    io->stream = stream; io->W = W; io->H = H;
    io->dst = out_is_device ? out : b->warp_out;
    return SIFTMI_OK;
}

// After the launch (bracketed by ev_wa / ev_wb): a host result copied back from the staging -- `bytes0` to `host0`, then the
// `bytes1` behind them to `host1` when there is a second piece and the `bytes2` behind those to `host2` when there is a third
// (a piece whose pointer is null is skipped, the ones behind it stay where they are) --, the one synchronisation, and kernel_ms
// from the event pair.
int warp_end(siftmi_batch *b, const WarpIo &io, void *host0, size_t bytes0, void *host1, size_t bytes1, double *kernel_ms,
             void *host2 = nullptr, size_t bytes2 = 0) {
    if (host0 && bytes0) {
        hipError_t e = hipMemcpyAsync(host0, io.dst, bytes0, hipMemcpyDeviceToHost, io.stream);
        if (e == hipSuccess && host1 && bytes1) e = hipMemcpyAsync(host1, (const uint8_t *)io.dst + bytes0, bytes1, hipMemcpyDeviceToHost, io.stream);
        if (e == hipSuccess && host2 && bytes2)
            e = hipMemcpyAsync(host2, (const uint8_t *)io.dst + bytes0 + bytes1, bytes2, hipMemcpyDeviceToHost, io.stream);
        if (e != hipSuccess) { (void)hipStreamSynchronize(io.stream); return fail(SIFTMI_EDEVICE, "hipMemcpyAsync: %s", hipGetErrorString(e)); }
    }
    HIPCHK(hipStreamSynchronize(io.stream));       // (the pinned table and the caller's frames are free again from here on)
    HIPCHK(hipGetLastError());
    if (kernel_ms) {
        float ms = 0;
        hipEventElapsedTime(&ms, b->ev_wa, b->ev_wb);
        *kernel_ms = ms;
    }
    return SIFTMI_OK;
}

// The one launch site of the stack reduction (k_stack.hpp): S frames of W x H from the device table to one OH x OW plane and,
// unless null, its coverage.  S == 0 (sum or mean) fills the plane with `empty` and the coverage with 0.
void launch_stack(hipStream_t st, int reduce, int interp, const WarpFrame *frames, int S, float *out, int32_t *coverage, int W, int H, int OW,
                  int OH, float empty) {
    const dim3 grid((unsigned)((OW + 63) / 64), (unsigned)((OH + 3) / 4)), block(64, 4);
    if (interp == SIFTMI_INTERP_CUBIC) {           // the cubic instances: the same launch shapes and the same dynamic LDS
        if (reduce == SIFTMI_STACK_MEDIAN)
            hipLaunchKernelGGL(stack_median_cubic_kernel, grid, block, (size_t)stack_median_slots(S) * 256 * sizeof(uint32_t), st, frames, S, out,
                               coverage, W, H, OW, OH, empty);
        else if (reduce == SIFTMI_STACK_MEAN)
            hipLaunchKernelGGL(stack_reduce_cubic_kernel<true>, grid, block, 0, st, frames, S, out, coverage, W, H, OW, OH, empty);
        else
            hipLaunchKernelGGL(stack_reduce_cubic_kernel<false>, grid, block, 0, st, frames, S, out, coverage, W, H, OW, OH, empty);
    } else if (reduce == SIFTMI_STACK_MEDIAN)
        hipLaunchKernelGGL(stack_median_kernel, grid, block, (size_t)stack_median_slots(S) * 256 * sizeof(uint32_t), st, frames, S, out, coverage, W, H,
                           OW, OH, empty);
    else if (reduce == SIFTMI_STACK_MEAN)
        hipLaunchKernelGGL(stack_reduce_kernel<true>, grid, block, 0, st, frames, S, out, coverage, W, H, OW, OH, empty);
    else
        hipLaunchKernelGGL(stack_reduce_kernel<false>, grid, block, 0, st, frames, S, out, coverage, W, H, OW, OH, empty);
}

// The one launch site of the clipped stack reduction (k_stack_clip.hpp): S <= 64 frames to one OH x OW plane and, unless null, its
// coverage and kept counts.  Dynamic LDS is the S x 256 samples of a block.  S == 0 fills the plane with `empty` and both counts with 0.
void launch_stack_clip(hipStream_t st, int reject, int interp, const WarpFrame *frames, int S, const StackClipArgs &p, float *out,
                       int32_t *coverage, int32_t *kept, int W, int H, int OW, int OH, float empty) {
    const dim3 grid((unsigned)((OW + 63) / 64), (unsigned)((OH + 3) / 4)), block(64, 4);
    const size_t lds = (size_t)S * 256 * sizeof(float);
    if (interp == SIFTMI_INTERP_CUBIC) {
        if (reject == SIFTMI_STACK_TRIM)
            hipLaunchKernelGGL(stack_clip_cubic_kernel<SIFT_STACK_TRIM>, grid, block, lds, st, frames, S, p, out, coverage, kept, W, H, OW, OH, empty);
        else
            hipLaunchKernelGGL(stack_clip_cubic_kernel<SIFT_STACK_SIGMA>, grid, block, lds, st, frames, S, p, out, coverage, kept, W, H, OW, OH, empty);
    } else if (reject == SIFTMI_STACK_TRIM)
        hipLaunchKernelGGL(stack_clip_kernel<SIFT_STACK_TRIM>, grid, block, lds, st, frames, S, p, out, coverage, kept, W, H, OW, OH, empty);
    else
        hipLaunchKernelGGL(stack_clip_kernel<SIFT_STACK_SIGMA>, grid, block, lds, st, frames, S, p, out, coverage, kept, W, H, OW, OH, empty);
}

// The one launch site of the streaming accumulator (k_stack_accum.hpp): S >= 1 frames added into the caller's OH x OW state
// planes.  s2 null: the instances without second moments; clip.center null: the instances without a clip.
void launch_stack_accum(hipStream_t st, int interp, const WarpFrame *frames, int S, double *s1, double *s2, int32_t *coverage, int32_t *kept,
                        const StackAccumClip &clip, int W, int H, int OW, int OH) {
    const dim3 grid((unsigned)((OW + 63) / 64), (unsigned)((OH + 3) / 4)), block(64, 4);
#define STACK_ACCUM_LAUNCH(CUBIC, MOMENTS, CLIP) \
    hipLaunchKernelGGL((stack_accum_kernel<CUBIC, MOMENTS, CLIP>), grid, block, 0, st, frames, S, s1, s2, coverage, kept, clip, W, H, OW, OH)
    const bool clipped = clip.center != nullptr;
    if (interp == SIFTMI_INTERP_CUBIC) {
        if (s2) { if (clipped) STACK_ACCUM_LAUNCH(true, true, true); else STACK_ACCUM_LAUNCH(true, true, false); }
        else { if (clipped) STACK_ACCUM_LAUNCH(true, false, true); else STACK_ACCUM_LAUNCH(true, false, false); }
    } else {
        if (s2) { if (clipped) STACK_ACCUM_LAUNCH(false, true, true); else STACK_ACCUM_LAUNCH(false, true, false); }
        else { if (clipped) STACK_ACCUM_LAUNCH(false, false, true); else STACK_ACCUM_LAUNCH(false, false, false); }
    }
#undef STACK_ACCUM_LAUNCH
}

// The one launch site of the accumulator's result (k_stack_accum.hpp): n >= 1 pixels of state to the mean and, unless null, the variance.
void launch_stack_accum_result(hipStream_t st, const double *s1, const double *s2, const int32_t *kept, size_t n, float *mean, float *var,
                               float empty) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (var)
        hipLaunchKernelGGL(stack_accum_result_kernel<true>, grid, block, 0, st, s1, s2, kept, n, mean, var, empty);
    else
        hipLaunchKernelGGL(stack_accum_result_kernel<false>, grid, block, 0, st, s1, s2, kept, n, mean, var, empty);
}

// What every _ex entry refuses about its sampler before anything else is looked at: an unknown `interp`, and the cubic sampler with
// a `mode` other than 1 (reserved) or for RGB8 frames.  SIFTMI_OK otherwise.
int check_interp(int32_t interp, int32_t mode, bool rgb) {
    static_assert(SIFTMI_INTERP_MODE == SIFT_INTERP_MODE && SIFTMI_INTERP_CUBIC == SIFT_INTERP_CUBIC, "siftmi.h and k_warp_cubic.hpp disagree");
    if (interp != SIFTMI_INTERP_MODE && interp != SIFTMI_INTERP_CUBIC) return fail(SIFTMI_EINVAL, "interp must be 0 (what mode says) or 1 (cubic), got %d", interp);
    if (interp == SIFTMI_INTERP_CUBIC && mode != 1) return fail(SIFTMI_EINVAL, "the cubic sampler takes mode 1 only (other values are reserved), got %d", mode);
    if (interp == SIFTMI_INTERP_CUBIC && rgb) return fail(SIFTMI_EINVAL, "the cubic sampler takes float32 frames only");
    return SIFTMI_OK;
}
}  // namespace

// The warp of siftmi_plan_transform for n frames in one launch (k_align_batch.hpp; cubic: k_warp_cubic.hpp).
int siftmi_batch_transform(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t images_are_device,
                           int32_t channels, void *out, int32_t out_is_device, int32_t OW, int32_t OH, const float *maps,
                           const float *fills, int32_t mode, double *kernel_ms) {
    return siftmi_batch_transform_ex(b, images, n_images, images_are_device, channels, out, out_is_device, OW, OH, maps, fills, mode,
                                     SIFTMI_INTERP_MODE, kernel_ms);
}

int siftmi_batch_transform_ex(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t images_are_device,
                              int32_t channels, void *out, int32_t out_is_device, int32_t OW, int32_t OH, const float *maps,
                              const float *fills, int32_t mode, int32_t interp, double *kernel_ms) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (int rc = check_interp(interp, mode, channels == 3 || (!b->lanes.empty() && b->lanes[0]->dtype == SIFTMI_RGB8))) return rc;
    if (n_images < 0) return fail(SIFTMI_EINVAL, "negative image count");
    if (n_images > 65535) return fail(SIFTMI_EINVAL, "%d frames: more than 65535 (one grid plane per frame)", n_images);
    if (channels != 1 && channels != 3) return fail(SIFTMI_EINVAL, "channels must be 1 (float32) or 3 (RGB8), got %d", channels);
    if (OW < 0 || OH < 0) return fail(SIFTMI_EINVAL, "negative output shape");
    if (OH > 4 * 65535) return fail(SIFTMI_EINVAL, "output height %d: more than %d rows (4 per grid row)", OH, 4 * 65535);
    const bool empty = n_images == 0 || OW == 0 || OH == 0;
    if (n_images > 0 && (!images || !maps || !fills)) return fail(SIFTMI_EINVAL, "null argument");
    if (!empty && !out) return fail(SIFTMI_EINVAL, "null output");
    for (int32_t i = 0; i < n_images; i++) if (!images[i]) return fail(SIFTMI_EINVAL, "null image %d", i);
    if (kernel_ms) *kernel_ms = 0;
    if (empty || b->lanes.empty()) return SIFTMI_OK;
    const size_t px = channels == 1 ? 4 : 3;
    const size_t out_bytes = (size_t)OW * OH * px * (size_t)n_images;
    WarpIo io;
    int rc = warp_begin(b, images, n_images, images_are_device, px, out, out_is_device, out_bytes, maps, fills, mode, &io);
    if (rc) return rc;
    const int xcols = channels == 1 ? 64 : 256;   // RGB: 4 pixels per thread
    const dim3 grid((unsigned)((OW + xcols - 1) / xcols), (unsigned)((OH + 3) / 4), (unsigned)n_images), block(64, 4);
    hipEventRecord(b->ev_wa, io.stream);
    if (interp == SIFTMI_INTERP_CUBIC)
        hipLaunchKernelGGL(transform_cubic_batch_kernel, grid, block, 0, io.stream, (const WarpFrame *)b->warp_tab, (float *)io.dst, io.W, io.H, OW, OH);
    else if (channels == 1)
        hipLaunchKernelGGL(transform_batch_kernel, grid, block, 0, io.stream, (const WarpFrame *)b->warp_tab, (float *)io.dst, io.W, io.H, OW, OH);
    else
        hipLaunchKernelGGL(transform_rgb_batch_kernel, grid, block, 0, io.stream, (const WarpFrame *)b->warp_tab, (uint8_t *)io.dst, io.W, io.H, OW, OH);
    hipEventRecord(b->ev_wb, io.stream);
    return warp_end(b, io, out_is_device ? nullptr : out, out_bytes, nullptr, 0, kernel_ms);
}

// S frames warped and reduced to one plane in one launch (k_stack.hpp).  Without a frame the reduction kernel itself is the fill
// path: launched with S == 0 it writes `empty` and coverage 0 to every pixel.
int siftmi_batch_stack(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t images_are_device, float *out,
                       int32_t *coverage, int32_t out_is_device, int32_t OW, int32_t OH, const float *maps, const float *fills,
                       int32_t mode, int32_t reduce, float empty, double *kernel_ms) {
    return siftmi_batch_stack_ex(b, images, n_images, images_are_device, out, coverage, out_is_device, OW, OH, maps, fills, mode,
                                 SIFTMI_INTERP_MODE, reduce, empty, kernel_ms);
}

int siftmi_batch_stack_ex(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t images_are_device, float *out,
                          int32_t *coverage, int32_t out_is_device, int32_t OW, int32_t OH, const float *maps, const float *fills,
                          int32_t mode, int32_t interp, int32_t reduce, float empty, double *kernel_ms) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (int rc = check_interp(interp, mode, !b->lanes.empty() && b->lanes[0]->dtype == SIFTMI_RGB8)) return rc;
    if (n_images < 0) return fail(SIFTMI_EINVAL, "negative image count");
    if (n_images > 65535) return fail(SIFTMI_EINVAL, "%d frames: more than 65535", n_images);
    if (reduce != SIFTMI_STACK_SUM && reduce != SIFTMI_STACK_MEAN && reduce != SIFTMI_STACK_MEDIAN)
        return fail(SIFTMI_EINVAL, "reduce must be 0 (sum), 1 (mean) or 2 (median), got %d", reduce);
    if (reduce == SIFTMI_STACK_MEDIAN && n_images > SIFTMI_STACK_MEDIAN_MAX)
        return fail(SIFTMI_EINVAL, "median of %d frames: more than %d", n_images, SIFTMI_STACK_MEDIAN_MAX);
    if (OW < 0 || OH < 0) return fail(SIFTMI_EINVAL, "negative output shape");
    if (OH > 4 * 65535) return fail(SIFTMI_EINVAL, "output height %d: more than %d rows (4 per grid row)", OH, 4 * 65535);
    if (!b->lanes.empty() && b->lanes[0]->dtype == SIFTMI_RGB8) return fail(SIFTMI_EINVAL, "a batch created for RGB8 frames has no stack reduction");
    const bool nothing = OW == 0 || OH == 0;
    if (n_images > 0 && (!images || !maps || !fills)) return fail(SIFTMI_EINVAL, "null argument");
    if (!nothing && !out) return fail(SIFTMI_EINVAL, "null output");
    for (int32_t i = 0; i < n_images; i++) if (!images[i]) return fail(SIFTMI_EINVAL, "null image %d", i);
    if (kernel_ms) *kernel_ms = 0;
    if (nothing || b->lanes.empty()) return SIFTMI_OK;
    static_assert(SIFTMI_STACK_MEDIAN_MAX == SIFT_STACK_MEDIAN_MAX, "siftmi.h and k_stack.hpp disagree on the median's cap");
    const size_t plane = (size_t)OW * OH * sizeof(float);
    WarpIo io;
    int rc = warp_begin(b, images, n_images, images_are_device, sizeof(float), out, out_is_device, plane * (coverage ? 2 : 1), maps, fills, mode, &io);
    if (rc) return rc;
    // a host result: the plane, then the coverage, in the batch's staging
    int32_t *cov = out_is_device ? coverage : (coverage ? reinterpret_cast<int32_t *>((uint8_t *)io.dst + plane) : nullptr);
    hipEventRecord(b->ev_wa, io.stream);
    launch_stack(io.stream, n_images ? reduce : SIFTMI_STACK_SUM, interp, (const WarpFrame *)b->warp_tab, n_images, (float *)io.dst, cov, io.W, io.H, OW, OH, empty);
    hipEventRecord(b->ev_wb, io.stream);
    return warp_end(b, io, out_is_device ? nullptr : out, plane, coverage, plane, kernel_ms);
}

// S <= 64 frames warped, outliers rejected per pixel and the survivors averaged in one launch (k_stack_clip.hpp).  Without a frame
// the kernel itself is the fill path, as for siftmi_batch_stack.
int siftmi_batch_stack_clip(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t images_are_device, float *out,
                            int32_t *coverage, int32_t *kept, int32_t out_is_device, int32_t OW, int32_t OH, const float *maps,
                            const float *fills, const float *weights, int32_t mode, int32_t reject, int32_t n_low, int32_t n_high,
                            float kappa_low, float kappa_high, int32_t iters, float empty, double *kernel_ms) {
    return siftmi_batch_stack_clip_ex(b, images, n_images, images_are_device, out, coverage, kept, out_is_device, OW, OH, maps, fills, weights,
                                      mode, SIFTMI_INTERP_MODE, reject, n_low, n_high, kappa_low, kappa_high, iters, empty, kernel_ms);
}

int siftmi_batch_stack_clip_ex(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t images_are_device, float *out,
                               int32_t *coverage, int32_t *kept, int32_t out_is_device, int32_t OW, int32_t OH, const float *maps,
                               const float *fills, const float *weights, int32_t mode, int32_t interp, int32_t reject, int32_t n_low,
                               int32_t n_high, float kappa_low, float kappa_high, int32_t iters, float empty, double *kernel_ms) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (int rc = check_interp(interp, mode, !b->lanes.empty() && b->lanes[0]->dtype == SIFTMI_RGB8)) return rc;
    if (n_images < 0) return fail(SIFTMI_EINVAL, "negative image count");
    static_assert(SIFTMI_STACK_CLIP_MAX == SIFT_STACK_CLIP_MAX && SIFTMI_STACK_TRIM == SIFT_STACK_TRIM && SIFTMI_STACK_SIGMA == SIFT_STACK_SIGMA,
                  "siftmi.h and k_stack_clip.hpp disagree");
    if (n_images > SIFTMI_STACK_CLIP_MAX) return fail(SIFTMI_EINVAL, "a clipped mean of %d frames: more than %d", n_images, SIFTMI_STACK_CLIP_MAX);
    if (reject != SIFTMI_STACK_TRIM && reject != SIFTMI_STACK_SIGMA) return fail(SIFTMI_EINVAL, "reject must be 0 (trim) or 1 (sigma), got %d", reject);
    if (n_low < 0 || n_high < 0 || (int64_t)n_low + n_high > SIFTMI_STACK_CLIP_MAX - 1)
        return fail(SIFTMI_EINVAL, "n_low %d, n_high %d: each must be >= 0 and their sum at most %d", n_low, n_high, SIFTMI_STACK_CLIP_MAX - 1);
    if (!(kappa_low > 0.0f) || !(kappa_high > 0.0f)) return fail(SIFTMI_EINVAL, "kappa_low %g, kappa_high %g: each must be > 0 (inf allowed)", kappa_low, kappa_high);
    if (iters < 0) return fail(SIFTMI_EINVAL, "negative iteration count");
    if (OW < 0 || OH < 0) return fail(SIFTMI_EINVAL, "negative output shape");
    if (OH > 4 * 65535) return fail(SIFTMI_EINVAL, "output height %d: more than %d rows (4 per grid row)", OH, 4 * 65535);
    if (!b->lanes.empty() && b->lanes[0]->dtype == SIFTMI_RGB8) return fail(SIFTMI_EINVAL, "a batch created for RGB8 frames has no stack reduction");
    const bool nothing = OW == 0 || OH == 0;
    if (n_images > 0 && (!images || !maps || !fills)) return fail(SIFTMI_EINVAL, "null argument");
    if (!nothing && !out) return fail(SIFTMI_EINVAL, "null output");
    for (int32_t i = 0; i < n_images; i++) if (!images[i]) return fail(SIFTMI_EINVAL, "null image %d", i);
    StackClipArgs p;
    for (int i = 0; i < SIFT_STACK_CLIP_MAX; i++) p.w[i] = 1.0f;
    for (int32_t i = 0; weights && i < n_images; i++) {
        if (!(weights[i] > 0.0f) || std::isinf(weights[i])) return fail(SIFTMI_EINVAL, "weight %d is %g: must be finite and > 0", i, weights[i]);
        p.w[i] = weights[i];
    }
    p.n_low = n_low; p.n_high = n_high; p.kappa_low = kappa_low; p.kappa_high = kappa_high; p.iters = iters;
    if (kernel_ms) *kernel_ms = 0;
    if (nothing || b->lanes.empty()) return SIFTMI_OK;
    const size_t plane = (size_t)OW * OH * sizeof(float);
    const bool counts = coverage || kept;
    WarpIo io;
    int rc = warp_begin(b, images, n_images, images_are_device, sizeof(float), out, out_is_device, plane * (counts ? 3 : 1), maps, fills, mode, &io);
    if (rc) return rc;
    // a host result: the plane, then the coverage, then the kept counts, in the batch's staging
    int32_t *cov = coverage, *kep = kept;
    if (!out_is_device) {
        cov = coverage ? reinterpret_cast<int32_t *>((uint8_t *)io.dst + plane) : nullptr;
        kep = kept ? reinterpret_cast<int32_t *>((uint8_t *)io.dst + 2 * plane) : nullptr;
    }
    hipEventRecord(b->ev_wa, io.stream);
    launch_stack_clip(io.stream, reject, interp, (const WarpFrame *)b->warp_tab, n_images, p, (float *)io.dst, cov, kep, io.W, io.H, OW, OH, empty);
    hipEventRecord(b->ev_wb, io.stream);
    return warp_end(b, io, out_is_device ? nullptr : out, plane, coverage, plane, kernel_ms, kept, plane);
}

// One chunk of a stack of any length warped and added into the caller's running sums (k_stack_accum.hpp).  Frames, maps, fills,
// host staging and limits are siftmi_batch_stack_ex's: the same warp_begin / warp_end around the launch.  The state planes, the
// centre and the variance are device pointers, so the call always synchronises the device once on entry.
int siftmi_batch_stack_accum(siftmi_batch *b, const void *const *images, int32_t n_images, int32_t images_are_device, double *s1,
                             double *s2, int32_t *coverage, int32_t *kept, int32_t OW, int32_t OH, const float *maps, const float *fills,
                             int32_t mode, int32_t interp, const float *center, const float *var, float kappa_low, float kappa_high,
                             double *kernel_ms) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (int rc = check_interp(interp, mode, !b->lanes.empty() && b->lanes[0]->dtype == SIFTMI_RGB8)) return rc;
    if (n_images < 0) return fail(SIFTMI_EINVAL, "negative image count");
    if (n_images > 65535) return fail(SIFTMI_EINVAL, "%d frames: more than 65535", n_images);
    if (OW < 0 || OH < 0) return fail(SIFTMI_EINVAL, "negative output shape");
    if (OH > 4 * 65535) return fail(SIFTMI_EINVAL, "output height %d: more than %d rows (4 per grid row)", OH, 4 * 65535);
    if (!b->lanes.empty() && b->lanes[0]->dtype == SIFTMI_RGB8) return fail(SIFTMI_EINVAL, "a batch created for RGB8 frames has no stack reduction");
    if (!center != !var) return fail(SIFTMI_EINVAL, "a clip takes both the centre and the variance plane, or neither");
    if (center && (!(kappa_low > 0.0f) || !(kappa_high > 0.0f)))
        return fail(SIFTMI_EINVAL, "kappa_low %g, kappa_high %g: each must be > 0 (inf allowed)", kappa_low, kappa_high);
    const bool nothing = n_images == 0 || OW == 0 || OH == 0;
    if (n_images > 0 && (!images || !maps || !fills)) return fail(SIFTMI_EINVAL, "null argument");
    if (!nothing && (!s1 || !coverage || !kept)) return fail(SIFTMI_EINVAL, "null state plane");
    for (int32_t i = 0; i < n_images; i++) if (!images[i]) return fail(SIFTMI_EINVAL, "null image %d", i);
    if (kernel_ms) *kernel_ms = 0;
    if (nothing || b->lanes.empty()) return SIFTMI_OK;
    WarpIo io;
    int rc = warp_begin(b, images, n_images, images_are_device, sizeof(float), nullptr, 1, 0, maps, fills, mode, &io, true);
    if (rc) return rc;
    StackAccumClip clip{center, var, 0.0f, 0.0f};
    if (center) { clip.kl2 = kappa_low * kappa_low; clip.kh2 = kappa_high * kappa_high; }
    hipEventRecord(b->ev_wa, io.stream);
    launch_stack_accum(io.stream, interp, (const WarpFrame *)b->warp_tab, n_images, s1, s2, coverage, kept, clip, io.W, io.H, OW, OH);
    hipEventRecord(b->ev_wb, io.stream);
    return warp_end(b, io, nullptr, 0, nullptr, 0, kernel_ms);
}

// The accumulator's sums turned into the mean and, unless null, the population variance (k_stack_accum.hpp).  A host result is
// staged as siftmi_batch_stack's is: the mean, then the variance, in the batch's staging.
int siftmi_batch_stack_accum_result(siftmi_batch *b, const double *s1, const double *s2, const int32_t *kept, int32_t OW, int32_t OH,
                                    float *mean, float *var, int32_t out_is_device, float empty, double *kernel_ms) {
    if (!b) return fail(SIFTMI_EINVAL, "null batch");
    if (OW < 0 || OH < 0) return fail(SIFTMI_EINVAL, "negative output shape");
    if (OH > 4 * 65535) return fail(SIFTMI_EINVAL, "output height %d: more than %d rows", OH, 4 * 65535);
    if (!b->lanes.empty() && b->lanes[0]->dtype == SIFTMI_RGB8) return fail(SIFTMI_EINVAL, "a batch created for RGB8 frames has no stack reduction");
    if (var && !s2) return fail(SIFTMI_EINVAL, "the variance needs the second moments (s2)");
    const size_t n = (size_t)OW * OH;
    if ((n + 255) / 256 > 2147483647u) return fail(SIFTMI_EINVAL, "%d x %d output pixels: more than one grid holds", OW, OH);
    if (n && (!s1 || !kept)) return fail(SIFTMI_EINVAL, "null state plane");
    if (n && !mean) return fail(SIFTMI_EINVAL, "null output");
    if (kernel_ms) *kernel_ms = 0;
    if (!n || b->lanes.empty()) return SIFTMI_OK;
    const size_t plane = n * sizeof(float);
    WarpIo io;
    int rc = warp_begin(b, nullptr, 0, 0, sizeof(float), mean, out_is_device, plane * (var ? 2 : 1), nullptr, nullptr, 1, &io, true);
    if (rc) return rc;
    float *v = out_is_device ? var : (var ? reinterpret_cast<float *>((uint8_t *)io.dst + plane) : nullptr);
    hipEventRecord(b->ev_wa, io.stream);
    launch_stack_accum_result(io.stream, s1, s2, kept, n, (float *)io.dst, v, empty);
    hipEventRecord(b->ev_wb, io.stream);
    return warp_end(b, io, out_is_device ? nullptr : mean, plane, var, plane, kernel_ms);
}

int siftmi_plan_records_device(const siftmi_plan *p, const siftmi_keypoint **records, int64_t *count) {
    if (!p || !records) return fail(SIFTMI_EINVAL, "null argument");
    *records = reinterpret_cast<const siftmi_keypoint *>(p->records);
    if (count) *count = p->last_count;
    return SIFTMI_OK;
}

// Affine warp of an image of the plan's shape (transform.cl:22,116; host side alignment.py:325-348).
int siftmi_plan_transform(siftmi_plan *p, const void *image, int32_t image_is_device, int32_t channels, void *out,
                          int32_t out_is_device, int32_t OW, int32_t OH, const float *matrix, const float *offset, float fill,
                          int32_t mode, double *kernel_ms) {
    return siftmi_plan_transform_ex(p, image, image_is_device, channels, out, out_is_device, OW, OH, matrix, offset, fill, mode,
                                    SIFTMI_INTERP_MODE, kernel_ms);
}

int siftmi_plan_transform_ex(siftmi_plan *p, const void *image, int32_t image_is_device, int32_t channels, void *out,
                             int32_t out_is_device, int32_t OW, int32_t OH, const float *matrix, const float *offset, float fill,
                             int32_t mode, int32_t interp, double *kernel_ms) {
    if (!p || !out || !matrix || !offset) return fail(SIFTMI_EINVAL, "null argument");
    if (int rc = check_interp(interp, mode, channels == 3)) return rc;
    if (channels != 1 && channels != 3) return fail(SIFTMI_EINVAL, "channels must be 1 (float32) or 3 (RGB8), got %d", channels);
    if (OW < 0 || OH < 0) return fail(SIFTMI_EINVAL, "negative output shape");
    HIPCHK(hipSetDevice(p->device));
    const size_t px = channels == 1 ? 4 : 3;
    const size_t in_bytes = (size_t)p->W * p->H * px, out_bytes = (size_t)OW * OH * px;
    const void *src = image;
    // a device pointer on either side: ordered after what the caller's streams were given for it (siftmi.h, conventions)
    if ((image && image_is_device) || out_is_device) HIPCHK(hipDeviceSynchronize());
    if (!image) {
        const int want = channels == 1 ? SIFTMI_F32 : SIFTMI_RGB8;
        if (p->raw_dtype != want)
            return fail(SIFTMI_EINVAL, "no staged input of the requested format (staged dtype %d, wanted %d)", p->raw_dtype, want);
        src = p->raw;
    } else if (!image_is_device) {
        if (p->warp_in_bytes < in_bytes) {
            if (p->warp_in) hipFree(p->warp_in);
            p->warp_in = nullptr; p->warp_in_bytes = 0;
            hipError_t e = hipMalloc(&p->warp_in, in_bytes ? in_bytes : 16);
            if (e != hipSuccess) return fail(SIFTMI_ENOMEM, "hipMalloc(%zu): %s", in_bytes, hipGetErrorString(e));
            p->warp_in_bytes = in_bytes;
        }
        HIPCHK(hipMemcpyAsync(p->warp_in, image, in_bytes, hipMemcpyHostToDevice, p->stream));
        src = p->warp_in;
    }
    void *dst = out;
    if (!out_is_device) {
        if (p->warp_out_bytes < out_bytes) {
            if (p->warp_out) hipFree(p->warp_out);
            p->warp_out = nullptr; p->warp_out_bytes = 0;
            hipError_t e = hipMalloc(&p->warp_out, out_bytes ? out_bytes : 16);
            if (e != hipSuccess) return fail(SIFTMI_ENOMEM, "hipMalloc(%zu): %s", out_bytes, hipGetErrorString(e));
            p->warp_out_bytes = out_bytes;
        }
        dst = p->warp_out;
    }
    if (!p->ev_wa) { HIPCHK(hipEventCreate(&p->ev_wa)); HIPCHK(hipEventCreate(&p->ev_wb)); }
    AffineArgs a{matrix[0], matrix[1], matrix[2], matrix[3], offset[0], offset[1], fill, mode};
    if (OW > 0 && OH > 0) {
        const int xcols = channels == 1 ? 64 : 256;   // RGB: 4 pixels per thread
        const dim3 grid((unsigned)((OW + xcols - 1) / xcols), (unsigned)((OH + 3) / 4)), block(64, 4);
        hipEventRecord(p->ev_wa, p->stream);
        if (interp == SIFTMI_INTERP_CUBIC)
            hipLaunchKernelGGL(transform_cubic_kernel, grid, block, 0, p->stream, (const float *)src, (float *)dst, a, p->W, p->H, OW, OH);
        else if (channels == 1)
            hipLaunchKernelGGL(transform_kernel, grid, block, 0, p->stream, (const float *)src, (float *)dst, a, p->W, p->H, OW, OH);
        else
            hipLaunchKernelGGL(transform_rgb_kernel, grid, block, 0, p->stream, (const uint8_t *)src, (uint8_t *)dst, a, p->W, p->H, OW, OH);
        hipEventRecord(p->ev_wb, p->stream);
        if (!out_is_device) HIPCHK(hipMemcpyAsync(out, dst, out_bytes, hipMemcpyDeviceToHost, p->stream));
    }
    HIPCHK(hipStreamSynchronize(p->stream));
    HIPCHK(hipGetLastError());
    if (kernel_ms) {
        float ms = 0;
        if (OW > 0 && OH > 0) hipEventElapsedTime(&ms, p->ev_wa, p->ev_wb);
        *kernel_ms = ms;
    }
    return SIFTMI_OK;
}

int siftmi_plan_get_minmax(const siftmi_plan *p, float *mn, float *mx) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (mn) *mn = p->last_min;
    if (mx) *mx = p->last_max;
    return SIFTMI_OK;
}

int siftmi_plan_profile(const siftmi_plan *p, char *buf, int64_t buflen) {
    if (!p || !buf || buflen < 1) return fail(SIFTMI_EINVAL, "bad argument");
    std::string s;
    char line[160];
    for (size_t i = 0; i < p->n_events; i++) {
        float ms = 0;
        hipEventElapsedTime(&ms, p->events[i].a, p->events[i].b);
        snprintf(line, sizeof line, "%s\t%.6f\n", p->events[i].label.c_str(), ms);
        s += line;
    }
    snprintf(buf, (size_t)buflen, "%s", s.c_str());
    return SIFTMI_OK;
}

int siftmi_plan_last_kernel_ms(const siftmi_plan *p, float *total_ms, float *blur_ms, int32_t *blur_launches,
                               double *blur_pixels) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (!p->profile) return fail(SIFTMI_EINVAL, "plan was created with profile=0");
    float tot = 0;                            // light profile: not measured (0)
    if (p->profile > 1) {
        for (int k = 0; k < 3; k++) {
            float tb = 0;
            if (p->wait_s[k] && hipEventElapsedTime(&tb, p->ev_first, p->ev_last[k]) == hipSuccess && tb > tot) tot = tb;
        }
    }
    if (total_ms) *total_ms = tot;
    return siftmi_plan_blur_ms(p, -1, blur_ms, blur_launches, blur_pixels);
}

int siftmi_plan_profile_totals(siftmi_plan *p, int32_t reset, int64_t *calls, double *total_ms, double *blur0_ms,
                               int64_t *blur0_launches, double *blur0_pixels) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (calls) *calls = p->acc_calls;
    if (total_ms) *total_ms = p->acc_total_ms;
    if (blur0_ms) *blur0_ms = p->acc_b0_ms;
    if (blur0_launches) *blur0_launches = p->acc_b0_launches;
    if (blur0_pixels) *blur0_pixels = p->acc_b0_pixels;
    if (reset) { p->acc_calls = 0; p->acc_b0_launches = 0; p->acc_total_ms = p->acc_b0_ms = p->acc_b0_pixels = 0; }
    return SIFTMI_OK;
}

int siftmi_plan_blur_ms(const siftmi_plan *p, int32_t octave, float *blur_ms, int32_t *blur_launches, double *blur_pixels) {
    if (!p) return fail(SIFTMI_EINVAL, "null plan");
    if (!p->profile) return fail(SIFTMI_EINVAL, "plan was created with profile=0");
    float bms = 0; int bl = 0; double px = 0;
    for (size_t i = 0; i < p->n_events; i++)
        if (p->events[i].is_blur && (octave < 0 || p->events[i].octave == octave)) {
            float ms = 0;
            hipEventElapsedTime(&ms, p->events[i].a, p->events[i].b);
            bms += ms; bl += p->events[i].launches; px += p->events[i].pixels;
        }
    if (blur_ms) *blur_ms = bms;
    if (blur_launches) *blur_launches = bl;
    if (blur_pixels) *blur_pixels = px;
    return SIFTMI_OK;
}

}  // extern "C"

// ============================================================================================
// Per-stage entry points: host arrays in, one kernel, host arrays out.
namespace {

struct DevBuf {
    void *p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    int alloc(size_t n) {
        hipError_t e = hipMalloc(&p, n ? n : 16);
        return e == hipSuccess ? SIFTMI_OK : fail(SIFTMI_ENOMEM, "hipMalloc(%zu): %s", n, hipGetErrorString(e));
    }
    int upload(const void *h, size_t n) {
        int rc = alloc(n);
        if (rc) return rc;
        HIPCHK(hipMemcpy(p, h, n, hipMemcpyHostToDevice));
        return SIFTMI_OK;
    }
    template <class T> T *as() { return (T *)p; }
};

int stage_begin(int device_id) {
    int ndev = siftmi_device_count();
    if (ndev < 1) return fail(SIFTMI_EDEVICE, "no HIP device available");
    if (device_id < 0 || device_id >= ndev) return fail(SIFTMI_EINVAL, "device %d out of range", device_id);
    HIPCHK(hipSetDevice(device_id));
    return SIFTMI_OK;
}

int stage_end() {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipGetLastError());
    return SIFTMI_OK;
}

// octave of a power-of-two octsize
int stage_octave(int32_t octsize, int &oct) {
    oct = 0;
    while ((1 << oct) < octsize && oct < SIFT_MAX_OCTAVES - 1) oct++;
    return (1 << oct) == octsize ? SIFTMI_OK : fail(SIFTMI_EINVAL, "octsize must be a power of two");
}

// host taps -> Taps with its device copy (kept alive by `store`)
int stage_taps(const float *taps, int ntaps, DevBuf &store, Taps &tp) {
    tp.n = ntaps;
    for (int i = 0; i < ntaps; i++) tp.t[i] = taps[i];
    int rc = store.upload(tp.t, sizeof tp.t);
    if (rc) return rc;
    tp.dev = store.as<float>();
    return SIFTMI_OK;
}

// What the per-keypoint hooks put on the device: the six planes of ONE octave and the table that holds nothing else, the
// keypoints with their aux tags (detection scale | octave << 8) and, for the MAPS forms, room for the octave's gradient maps.
struct StageOctave {
    DevBuf b, k, ks, gm, om;
    OctaveTable tab;
    int upload(const float *blurs, int W, int H, int oct, const float *kps, const int32_t *kp_scale, int64_t n, bool maps) {
        const size_t N = (size_t)W * H;
        std::vector<int32_t> aux((size_t)n);
        for (int64_t i = 0; i < n; i++) aux[(size_t)i] = kp_scale[i] | (oct << 8);
        int rc;
        if ((rc = b.upload(blurs, 6 * N * 4)) || (rc = k.upload(kps, (size_t)n * 16)) || (rc = ks.upload(aux.data(), (size_t)n * 4))) return rc;
        if (maps && ((rc = gm.alloc(3 * N * 4)) || (rc = om.alloc(3 * N * 4)))) return rc;
        memset(&tab, 0, sizeof tab);
        tab.base = b.as<float>(); tab.off[oct] = 0; tab.W[oct] = W; tab.H[oct] = H;
        tab.gmap = gm.as<float>(); tab.omap = om.as<float>();
        return SIFTMI_OK;
    }
};

// the MAPS forms read the maps of detection scales 1..3 only
int stage_maps_scales(const int32_t *kp_scale, int64_t n) {
    for (int64_t i = 0; i < n; i++)
        if (kp_scale[i] < 1 || kp_scale[i] > 3)
            return fail(SIFTMI_EINVAL, "gradient maps hold detection scales 1..3 only (keypoint %lld: %d)", (long long)i, kp_scale[i]);
    return SIFTMI_OK;
}

// Does the window of an oriented keypoint fit the row tables of the row-interval forms (R <= SIFT_DESC_MAXRAD)?  The
// kernels' expressions (desc_window, keypoints_cpu.cl:57-62); the float is compared instead of its (int) conversion, which
// is undefined on the host beyond the int range (an infinite spacing would pass as INT_MIN and reach the kernel's trap).
bool desc_rows_fit(float sigma_oct, int32_t octsize) {
    const float spacing = sigma_oct / (float)octsize * 3.0f;
    return !((1.414f * spacing * 2.5f) + 0.5f >= (float)(SIFT_DESC_MAXRAD + 1));
}

// the launch choices the blur hooks expose (siftmi.h: siftmi_stage_blur_ex) on top of the defaults
Options stage_blur_options(int32_t xcd_map, int32_t march_wgs) {
    Options opt = g_default_options;
    opt.xcd_map = (xcd_map & 1) ? 1 : 0;
    opt.march_prio = (xcd_map & 2) ? 0 : 2;       // (forced where not off: the stage planes are smaller than the rule's)
    opt.march_wgs = march_wgs > 0 ? march_wgs : 0;
    if ((xcd_map >> 2) & 3) opt.small_blur = ((xcd_map >> 2) & 3) - 1;
    return opt;
}

}  // namespace

extern "C" {

int siftmi_stage_gaussian_taps(float sigma, int32_t size, float *out) {
    if (!out) return fail(SIFTMI_EINVAL, "null argument");
    return gaussian_taps(sigma, size, out);
}

int32_t siftmi_stage_xcd_order(int32_t id, int32_t n) { return (n > 0 && id >= 0 && id < n) ? siftk::xcd_contiguous(id, n) : -1; }

int siftmi_stage_minmax_normalize(int32_t dev, const float *in, float *out, int32_t W, int32_t H, float *mn, float *mx) {
    int rc = stage_begin(dev); if (rc) return rc;
    const size_t N = (size_t)W * H;
    DevBuf a, b, mm;
    if ((rc = a.upload(in, N * 4)) || (rc = b.alloc(N * 4)) || (rc = mm.alloc(8))) return rc;
    hipLaunchKernelGGL(minmax_init, dim3(1), dim3(1), 0, 0, mm.as<uint32_t>());
    launch_minmax(nullptr, 0, SIFTMI_F32, a.p, (int64_t)N, 256, 2048, mm.as<uint32_t>(), nullptr, 0, -1);     // (no counter block to reset)
    launch_normalize(0, SIFTMI_F32, a.p, b.as<float>(), (int64_t)N, mm.as<uint32_t>());
    if ((rc = stage_end())) return rc;
    uint32_t h[2];
    HIPCHK(hipMemcpy(h, mm.p, 8, hipMemcpyDeviceToHost));
    if (mn) *mn = minmax_decode(h[0]);
    if (mx) *mx = minmax_decode(h[1]);
    if (out) HIPCHK(hipMemcpy(out, b.p, N * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

int siftmi_stage_blur(int32_t dev, const float *in, float *out, int32_t W, int32_t H, const float *taps, int32_t ntaps) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (ntaps < 1 || ntaps > 64) return fail(SIFTMI_EINVAL, "ntaps must be in 1..64");
    const size_t N = (size_t)W * H;
    DevBuf a, b, t, dt;
    if ((rc = a.upload(in, N * 4)) || (rc = b.alloc(N * 4)) || (rc = t.alloc(N * 4))) return rc;
    Taps tp;
    if ((rc = stage_taps(taps, ntaps, dt, tp))) return rc;
    if (!launch_blur_tiled<false>(g_default_options, 0, a.as<float>(), b.as<float>(), W, H, tp, nullptr))
        launch_blur_generic(0, a.as<float>(), b.as<float>(), t.as<float>(), W, H, tp, nullptr, false);
    if ((rc = stage_end())) return rc;
    HIPCHK(hipMemcpy(out, b.p, N * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

// The blur stage with a plan's launch choices exposed, so that a stage test reaches every instance of the marching team
// kernel (the plain entry point above takes planes below 1400^2 pixels only through the tiled kernel): the normalising
// instance behind a min/max pass, the typed-frame instances, both workgroup orders, any workgroup count.
int siftmi_stage_blur_ex(int32_t dev, const void *in, int32_t in_dtype, float *out, int32_t W, int32_t H, const float *taps, int32_t ntaps,
                         int32_t norm, int32_t xcd_map, int32_t march_wgs, int32_t *kernel_used) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!in || !out || !taps || W < 1 || H < 1) return fail(SIFTMI_EINVAL, "null argument or empty plane");
    if (ntaps < 1 || ntaps > 64) return fail(SIFTMI_EINVAL, "ntaps must be in 1..64");
    const size_t esz = dtype_size(in_dtype);
    if (!esz || in_dtype == SIFTMI_F64) return fail(SIFTMI_EINVAL, "input format %d has no fused blur", in_dtype);
    if (in_dtype != SIFTMI_F32 && !(norm && ntaps == 15)) return fail(SIFTMI_EINVAL, "typed frames enter through the normalising 15-tap blur only");
    const size_t N = (size_t)W * H;
    DevBuf a, b, t, dt, mm;
    if ((rc = a.upload(in, N * esz)) || (rc = b.alloc(N * 4)) || (rc = t.alloc(N * 4)) || (rc = mm.alloc(8))) return rc;
    Taps tp;
    if ((rc = stage_taps(taps, ntaps, dt, tp))) return rc;
    const Options opt = stage_blur_options(xcd_map, march_wgs);
    uint32_t *mmp = mm.as<uint32_t>();
    if (norm) {
        hipLaunchKernelGGL(minmax_init, dim3(1), dim3(1), 0, 0, mmp);
        // up to 2048 workgroups for f32, 256 for a typed frame; no counter block to reset
        launch_minmax(nullptr, 0, in_dtype, a.p, (int64_t)N, 256, in_dtype == SIFTMI_F32 ? 2048 : 256, mmp, nullptr, 0, -1);
    }
    BlurForm used = BLUR_NONE;
    if (in_dtype != SIFTMI_F32) {
        SIFTMI_TYPED_DISPATCH(in_dtype, used = launch_init_blur_dt<DT>(opt, 0, (const void *)a.p, b.as<float>(), W, H, tp, mmp));
        if (used == BLUR_NONE) return fail(SIFTMI_EINVAL, "no fused blur for input format %d", in_dtype);
    } else {
        used = norm ? launch_blur_tiled<true>(opt, 0, a.as<float>(), b.as<float>(), W, H, tp, mmp)
                    : launch_blur_tiled<false>(opt, 0, a.as<float>(), b.as<float>(), W, H, tp, mmp);
        if (used == BLUR_NONE) launch_blur_generic(0, a.as<float>(), b.as<float>(), t.as<float>(), W, H, tp, mmp, norm != 0);
    }
    if ((rc = stage_end())) return rc;
    if (kernel_used) *kernel_used = used;
    HIPCHK(hipMemcpy(out, b.p, N * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

// The f32 blur stage with the fused octave hand-off: the launch a plan makes for plane 3 (launch_blur with `half` set), so that
// a stage test reaches the hand-off line of every fused form at every tap count.  The half plane sits between two guards of
// SIFTMI_STAGE_GUARD floats the kernel is not told of; the whole buffer is filled with 0xa5 bytes first and returned whole,
// so a sample no workgroup wrote and a write before or beyond the half plane both show.
int siftmi_stage_blur_handoff(int32_t dev, const float *in, float *out, float *half, int32_t W, int32_t H, const float *taps, int32_t ntaps,
                              int32_t xcd_map, int32_t march_wgs, int32_t *kernel_used) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!in || !out || !half || !taps || W < 1 || H < 1) return fail(SIFTMI_EINVAL, "null argument or empty plane");
    if (ntaps < 1 || ntaps > 64) return fail(SIFTMI_EINVAL, "ntaps must be in 1..64");
    const size_t N = (size_t)W * H;
    const size_t hslots = (size_t)SIFTMI_STAGE_GUARD + (size_t)(W / 2) * (H / 2) + SIFTMI_STAGE_GUARD;
    DevBuf a, b, t, dt, h;
    if ((rc = a.upload(in, N * 4)) || (rc = b.alloc(N * 4)) || (rc = t.alloc(N * 4)) || (rc = h.alloc(hslots * 4))) return rc;
    HIPCHK(hipMemset(h.p, 0xa5, hslots * 4));
    Taps tp;
    if ((rc = stage_taps(taps, ntaps, dt, tp))) return rc;
    const Options opt = stage_blur_options(xcd_map, march_wgs);
    const BlurForm used = launch_blur_tiled<false>(opt, 0, a.as<float>(), b.as<float>(), W, H, tp, nullptr, h.as<float>() + SIFTMI_STAGE_GUARD);
    if (used == BLUR_NONE) launch_blur_generic(0, a.as<float>(), b.as<float>(), t.as<float>(), W, H, tp, nullptr, false);     // (no hand-off: `half` stays as filled)
    if ((rc = stage_end())) return rc;
    if (kernel_used) *kernel_used = used;
    HIPCHK(hipMemcpy(out, b.p, N * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(half, h.p, hslots * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

int siftmi_stage_dog(int32_t dev, const float *blur_a, const float *blur_b, float *out, int64_t n) {
    int rc = stage_begin(dev); if (rc) return rc;
    DevBuf a, b, o;
    if ((rc = a.upload(blur_a, (size_t)n * 4)) || (rc = b.upload(blur_b, (size_t)n * 4)) || (rc = o.alloc((size_t)n * 4))) return rc;
    hipLaunchKernelGGL(dog_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, 0, a.as<float>(), b.as<float>(), o.as<float>(), n);
    if ((rc = stage_end())) return rc;
    HIPCHK(hipMemcpy(out, o.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

int siftmi_stage_local_maxmin(int32_t dev, const float *blurs, int32_t W, int32_t H, int32_t octsize,
                              const siftmi_params *par, float *out, int64_t capacity, int64_t *n_out) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!par || !n_out) return fail(SIFTMI_EINVAL, "null argument");
    const size_t N = (size_t)W * H;
    DevBuf b, c, cnt;
    if ((rc = b.upload(blurs, 6 * N * 4)) || (rc = c.alloc((size_t)capacity * 16)) || (rc = cnt.alloc(sizeof(Counters)))) return rc;
    HIPCHK(hipMemset(cnt.p, 0, sizeof(Counters)));
    BlurPlanes bp;
    for (int s = 0; s < 6; s++) bp.p[s] = b.as<float>() + (size_t)s * N;
    const int border = par->border_dist;
    // strips by extrema_strip_rows' own default target, nothing to refine into, XCD order on
    const DetectGeom geo = detect_geometry(W, H, border, 0, 0, -1, -1);
    if (geo.blocks)
        launch_extrema(0, false, geo, bp, W, H, border, contrast_threshold(*par), octave_edge_thresh(*par, octsize), c.as<float4>(),
                       &cnt.as<Counters>()->n_cand[0], (int)capacity, RefineArgs{}, -1, -1, 1);
    if ((rc = stage_end())) return rc;
    Counters hc;
    HIPCHK(hipMemcpy(&hc, cnt.p, sizeof hc, hipMemcpyDeviceToHost));
    int64_t n = hc.n_cand[0] < capacity ? hc.n_cand[0] : capacity;
    if (n > 0) HIPCHK(hipMemcpy(out, c.p, (size_t)n * 16, hipMemcpyDeviceToHost));
    *n_out = n;
    return SIFTMI_OK;
}

int siftmi_stage_interp(int32_t dev, const float *blurs, int32_t W, int32_t H, const float *cand, int64_t n,
                        const siftmi_params *par, float *out, int32_t *out_scale, int64_t *n_out) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!par || !n_out) return fail(SIFTMI_EINVAL, "null argument");
    const size_t N = (size_t)W * H;
    DevBuf b, c, k, ks, cnt;
    if ((rc = b.upload(blurs, 6 * N * 4)) || (rc = c.upload(cand, (size_t)n * 16)) || (rc = k.alloc((size_t)n * 16)) ||
        (rc = ks.alloc((size_t)n * 4)) || (rc = cnt.alloc(sizeof(Counters)))) return rc;
    Counters hc{};
    hc.n_cand[0] = (int)n;
    HIPCHK(hipMemcpy(cnt.p, &hc, sizeof hc, hipMemcpyHostToDevice));
    BlurPlanes bp;
    for (int s = 0; s < 6; s++) bp.p[s] = b.as<float>() + (size_t)s * N;
    Counters *dc = cnt.as<Counters>();
    const RefineArgs ra = {par->peak_thresh, (float)par->init_sigma, k.as<float4>(), ks.as<int>(), &dc->g_kp[0], (int)n, 0, &dc->c_scale[0][0]};
    launch_refine(0, grid_for(n, 256, 512), bp, W, H, c.as<float4>(), &dc->n_cand[0], (int)n, ra);     // (a workgroup per 256 candidates, at most the plan's 512)
    if ((rc = stage_end())) return rc;
    HIPCHK(hipMemcpy(&hc, cnt.p, sizeof hc, hipMemcpyDeviceToHost));
    const int64_t m = hc.g_kp[0];
    if (m > 0) {
        HIPCHK(hipMemcpy(out, k.p, (size_t)m * 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out_scale, ks.p, (size_t)m * 4, hipMemcpyDeviceToHost));
    }
    *n_out = m;
    return SIFTMI_OK;
}

// The detection stage with a plan's launch choices exposed (launch_detect_octave), so that a stage test reaches both forms
// of the extrema kernel at every strip height, both workgroup orders, the band arguments and lists cut at their capacity.
// Counters come back raw (what the kernels counted, not what fits); the output lists are filled before the launch (the
// candidates with -1.0f, the refined lists with 0xa5 bytes) and copied back whole, guard slots included, so a slot no
// kernel wrote shows.
int siftmi_stage_detect_ex(int32_t dev, const float *blurs, int32_t W, int32_t H, int32_t octsize, const siftmi_params *par,
                           int32_t form, int32_t rows, int32_t xcd_map, int32_t y_lo, int32_t y_hi,
                           int64_t cand_capacity, int64_t kp_capacity, float *cand, float *kp, int32_t *kp_aux, int32_t *counters) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!blurs || !par || !counters || !cand || !kp || !kp_aux) return fail(SIFTMI_EINVAL, "null argument");
    if (W < 1 || H < 1) return fail(SIFTMI_EINVAL, "empty plane");
    if (form != 0 && form != 1) return fail(SIFTMI_EINVAL, "detection form %d: 0 extrema then refinement launch, 1 fused refinement", form);
    if (rows < 0 || rows > 4096) return fail(SIFTMI_EINVAL, "strip rows must be in 0..4096 (0: by the size rule)");
    if (cand_capacity < 0 || kp_capacity < 0 || cand_capacity > (1 << 30) || kp_capacity > (1 << 30)) return fail(SIFTMI_EINVAL, "capacity out of range");
    const int border = par->border_dist;
    if (border < 1) return fail(SIFTMI_EINVAL, "border_dist must be at least 1 (the 3 x 3 neighbourhood)");
    const bool band = y_lo >= 0;
    if (band && !(y_lo >= border && y_lo < y_hi && y_hi <= H - border))
        return fail(SIFTMI_EINVAL, "band [%d, %d) outside the detection rows [%d, %d)", y_lo, y_hi, border, H - border);
    int oct;
    if ((rc = stage_octave(octsize, oct))) return rc;
    const size_t N = (size_t)W * H;
    // every list is followed by guard slots the kernels are not told about: a write beyond the capacity shows in them
    const size_t cslots = (size_t)cand_capacity + SIFTMI_STAGE_GUARD, kslots = (size_t)kp_capacity + SIFTMI_STAGE_GUARD;
    DevBuf b, c, k, ka, cnt;
    if ((rc = b.upload(blurs, 6 * N * 4)) || (rc = c.alloc(cslots * 16)) || (rc = k.alloc(kslots * 16)) ||
        (rc = ka.alloc(kslots * 4)) || (rc = cnt.alloc(sizeof(Counters)))) return rc;
    HIPCHK(hipMemset(cnt.p, 0, sizeof(Counters)));
    {   // (the candidate list is filled with holes, the reference's own fill: the refinement launch skips a slot the extrema
        // kernel reserved and did not write, where a 0xa5 pattern would send it to row 0 of the plane and above it)
        std::vector<float> holes(cslots * 4, -1.0f);
        HIPCHK(hipMemcpy(c.p, holes.data(), cslots * 16, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(k.p, 0xa5, kslots * 16));
    HIPCHK(hipMemset(ka.p, 0xa5, kslots * 4));
    BlurPlanes bp;
    for (int s = 0; s < 6; s++) bp.p[s] = b.as<float>() + (size_t)s * N;
    Counters *dc = cnt.as<Counters>();
    const int yl = band ? y_lo : -1, yh = band ? y_hi : -1;
    const DetectGeom geo = detect_geometry(W, H, border, rows, g_default_options.ext_strips, yl, yh);
    if (geo.blocks) {
        const RefineArgs ra = {par->peak_thresh, (float)par->init_sigma, k.as<float4>(), ka.as<int>(), &dc->g_kp[0], (int)kp_capacity, oct, &dc->c_scale[0][0]};
        launch_extrema(0, form == 1, geo, bp, W, H, border, contrast_threshold(*par), octave_edge_thresh(*par, octsize), c.as<float4>(),
                       &dc->n_cand[0], (int)cand_capacity, ra, yl, yh, xcd_map ? 1 : 0);
        if (form == 0) launch_refine(0, 512, bp, W, H, c.as<float4>(), &dc->n_cand[0], (int)cand_capacity, ra);
    }
    if ((rc = stage_end())) return rc;
    Counters hc;
    HIPCHK(hipMemcpy(&hc, cnt.p, sizeof hc, hipMemcpyDeviceToHost));
    counters[0] = hc.n_cand[0]; counters[1] = hc.g_kp[0];
    for (int s = 0; s < 3; s++) counters[2 + s] = hc.c_scale[0][s];
    HIPCHK(hipMemcpy(cand, c.p, cslots * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(kp, k.p, kslots * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(kp_aux, ka.p, kslots * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

// The lazy detection chain of launch_detect_octave on five planes: extrema(LAZY) -> top_patch_kernel -> refinement.  Plane 5
// is allocated here and filled with a NaN pattern, so that a read outside the patches turns what it feeds into NaN.
int siftmi_stage_detect_lazy(int32_t dev, const float *blurs5, const float *top_taps, int32_t n_taps, int32_t W, int32_t H, int32_t octsize,
                             const siftmi_params *par, int32_t rows, int32_t xcd_map, int32_t y_lo, int32_t y_hi,
                             int64_t cand_capacity, int64_t kp_capacity, float *cand, float *kp, int32_t *kp_aux, int32_t *counters, float *plane5) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!blurs5 || !top_taps || !par || !counters || !cand || !kp || !kp_aux || !plane5) return fail(SIFTMI_EINVAL, "null argument");
    if (W < 1 || H < 1) return fail(SIFTMI_EINVAL, "empty plane");
    if (n_taps < 1 || n_taps > 64) return fail(SIFTMI_EINVAL, "1..64 taps, not %d", n_taps);
    if (rows < 0 || rows > 4096) return fail(SIFTMI_EINVAL, "strip rows must be in 0..4096 (0: by the size rule)");
    if (cand_capacity < 0 || kp_capacity < 0 || cand_capacity > (1 << 30) || kp_capacity > (1 << 30)) return fail(SIFTMI_EINVAL, "capacity out of range");
    const int border = par->border_dist;
    if (border < 1) return fail(SIFTMI_EINVAL, "border_dist must be at least 1 (the 3 x 3 neighbourhood)");
    const bool band = y_lo >= 0;
    if (band && !(y_lo >= border && y_lo < y_hi && y_hi <= H - border))
        return fail(SIFTMI_EINVAL, "band [%d, %d) outside the detection rows [%d, %d)", y_lo, y_hi, border, H - border);
    int oct;
    if ((rc = stage_octave(octsize, oct))) return rc;
    const size_t N = (size_t)W * H;
    const size_t cslots = (size_t)cand_capacity + SIFTMI_STAGE_GUARD, kslots = (size_t)kp_capacity + SIFTMI_STAGE_GUARD;
    DevBuf b, c, k, ka, cnt;
    if ((rc = b.alloc(6 * N * 4)) || (rc = c.alloc(cslots * 16)) || (rc = k.alloc(kslots * 16)) ||
        (rc = ka.alloc(kslots * 4)) || (rc = cnt.alloc(sizeof(Counters)))) return rc;
    HIPCHK(hipMemcpy(b.p, blurs5, 5 * N * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemset(cnt.p, 0, sizeof(Counters)));
    {
        std::vector<uint32_t> fill(N, SIFTMI_STAGE_TOP_FILL);
        HIPCHK(hipMemcpy(b.as<float>() + 5 * N, fill.data(), N * 4, hipMemcpyHostToDevice));
        std::vector<float> holes(cslots * 4, -1.0f);
        HIPCHK(hipMemcpy(c.p, holes.data(), cslots * 16, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemset(k.p, 0xa5, kslots * 16));
    HIPCHK(hipMemset(ka.p, 0xa5, kslots * 4));
    BlurPlanes bp;
    for (int s = 0; s < 6; s++) bp.p[s] = b.as<float>() + (size_t)s * N;
    Counters *dc = cnt.as<Counters>();
    const int yl = band ? y_lo : -1, yh = band ? y_hi : -1;
    const DetectGeom geo = detect_geometry(W, H, border, rows, g_default_options.ext_strips, yl, yh);
    if (geo.blocks) {
        Taps tp;
        tp.n = n_taps;
        for (int i = 0; i < n_taps; i++) tp.t[i] = top_taps[i];
        const RefineArgs ra = {par->peak_thresh, (float)par->init_sigma, k.as<float4>(), ka.as<int>(), &dc->g_kp[0], (int)kp_capacity, oct, &dc->c_scale[0][0]};
        launch_extrema(0, false, geo, bp, W, H, border, contrast_threshold(*par), octave_edge_thresh(*par, octsize), c.as<float4>(),
                       &dc->n_cand[0], (int)cand_capacity, ra, yl, yh, xcd_map ? 1 : 0, true);
        if ((rc = launch_top_patch(0, g_default_options.top_blocks, bp.p[4], b.as<float>() + 5 * N, W, H, tp, c.as<float4>(), &dc->n_cand[0], (int)cand_capacity))) return rc;
        launch_refine(0, 512, bp, W, H, c.as<float4>(), &dc->n_cand[0], (int)cand_capacity, ra);
    }
    if ((rc = stage_end())) return rc;
    Counters hc;
    HIPCHK(hipMemcpy(&hc, cnt.p, sizeof hc, hipMemcpyDeviceToHost));
    counters[0] = hc.n_cand[0]; counters[1] = hc.g_kp[0];
    for (int s = 0; s < 3; s++) counters[2 + s] = hc.c_scale[0][s];
    HIPCHK(hipMemcpy(cand, c.p, cslots * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(kp, k.p, kslots * 16, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(kp_aux, ka.p, kslots * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(plane5, b.as<float>() + 5 * N, N * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

int siftmi_stage_compact(int32_t dev, const float *kps, int64_t n, int64_t start, int64_t end, float *out, int64_t *n_out) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!n_out || start < 0 || end < start || end > n) return fail(SIFTMI_EINVAL, "bad range");
    DevBuf a, o, cnt;
    if ((rc = a.upload(kps, (size_t)n * 16)) || (rc = o.alloc((size_t)n * 16)) || (rc = cnt.alloc(16))) return rc;
    // the reference compacts in place of a second buffer that starts as a copy of the head: entries below `start` stay
    HIPCHK(hipMemcpy(o.p, a.p, (size_t)start * 16, hipMemcpyDeviceToDevice));
    const int first = (int)start;
    HIPCHK(hipMemcpy(cnt.p, &first, 4, hipMemcpyHostToDevice));
    if (end > start)
        hipLaunchKernelGGL(compact_kernel, dim3(grid_for(end - start, 256, 1024)), dim3(256), 0, 0, (const float4 *)a.as<float4>(),
                           o.as<float4>(), cnt.as<int>(), (int)start, (int)end, (int)n);
    if ((rc = stage_end())) return rc;
    int count = 0;
    HIPCHK(hipMemcpy(&count, cnt.p, 4, hipMemcpyDeviceToHost));
    if (count > 0) HIPCHK(hipMemcpy(out, o.p, (size_t)count * 16, hipMemcpyDeviceToHost));
    *n_out = count;
    return SIFTMI_OK;
}

int siftmi_stage_gradient(int32_t dev, const float *img, float *grad, float *ori, int32_t W, int32_t H) {
    int rc = stage_begin(dev); if (rc) return rc;
    const size_t N = (size_t)W * H;
    DevBuf a, g, o;
    if ((rc = a.upload(img, N * 4)) || (rc = g.alloc(N * 4)) || (rc = o.alloc(N * 4))) return rc;
    hipLaunchKernelGGL(gradient_kernel, dim3((unsigned)((W + 255) / 256), (unsigned)H), dim3(256), 0, 0, a.as<float>(),
                       g.as<float>(), o.as<float>(), W, H);
    if ((rc = stage_end())) return rc;
    HIPCHK(hipMemcpy(grad, g.p, N * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ori, o.p, N * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

int siftmi_stage_orientation(int32_t dev, const float *blurs, int32_t W, int32_t H, int32_t octsize, const float *kps,
                             const int32_t *kp_scale, int64_t n, const siftmi_params *par, float *out,
                             int32_t *out_scale, int64_t capacity, int64_t *n_out) {
    return siftmi_stage_orientation_ex(dev, blurs, W, H, octsize, kps, kp_scale, n, par, out, out_scale, capacity, n_out, 0, 0, nullptr);
}

int siftmi_stage_orientation_ex(int32_t dev, const float *blurs, int32_t W, int32_t H, int32_t octsize, const float *kps,
                                const int32_t *kp_scale, int64_t n, const siftmi_params *par, float *out,
                                int32_t *out_scale, int64_t capacity, int64_t *n_out, int32_t form, int32_t blocks, int32_t *form_used) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!par || !n_out) return fail(SIFTMI_EINVAL, "null argument");
    if (form < 0 || form > 7 || (form & 3) == 3) return fail(SIFTMI_EINVAL, "orientation form %d: 0 / 1 wave, 2 workgroup per keypoint, + 4 maps", form);
    if (blocks < 0) return fail(SIFTMI_EINVAL, "blocks must not be negative");
    const bool maps = (form & 4) != 0;
    if (maps && (rc = stage_maps_scales(kp_scale, n))) return rc;
    int oct;
    if ((rc = stage_octave(octsize, oct))) return rc;
    StageOctave so;
    DevBuf o, oa, cnt;
    if ((rc = so.upload(blurs, W, H, oct, kps, kp_scale, n, maps)) || (rc = o.alloc((size_t)capacity * 16)) || (rc = oa.alloc((size_t)capacity * 4)) ||
        (rc = cnt.alloc(sizeof(Counters)))) return rc;
    Counters hc{};
    hc.g_kp[0] = (int)n;
    HIPCHK(hipMemcpy(cnt.p, &hc, sizeof hc, hipMemcpyHostToDevice));
    if (maps) launch_maps_kernel(so.tab, oct, oct + 1, g_default_options.maps_blocks, 0);
    // a workgroup per keypoint below `team_below` keypoints; `blocks` is also the small-group cut, which would override the grid
    const int team_below = (form & 3) == 2 ? (1 << 30) : 0;
    const int grid = blocks > 0 ? blocks : grid_for(n * 64, 256, 1024), small_blocks = blocks > 0 ? blocks : 512;
    launch_orientation(0, maps, grid, 0, so.tab, par->ori_sigma, so.k.as<float4>(), so.ks.as<int>(), cnt.as<Counters>(), 0, (int)n, o.as<float4>(),
                       oa.as<int>(), (int)capacity, team_below, small_blocks);
    // What the launch arguments select: the kernel takes the workgroup form when its count (here n) is below team_below.
    // The kernel reports nothing back, so this is the kernel's rule applied on the host, not an observation of the launch.
    const int used = ((int)n < team_below ? 2 : 1) | (maps ? 4 : 0);
    if ((rc = stage_end())) return rc;
    if (form_used) *form_used = used;
    HIPCHK(hipMemcpy(&hc, cnt.p, sizeof hc, hipMemcpyDeviceToHost));
    int64_t m = hc.g_out[0] < capacity ? hc.g_out[0] : capacity;
    if (m > 0) {
        HIPCHK(hipMemcpy(out, o.p, (size_t)m * 16, hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(out_scale, oa.p, (size_t)m * 4, hipMemcpyDeviceToHost));
        for (int64_t i = 0; i < m; i++) out_scale[i] &= 0xff;
    }
    *n_out = m;
    return SIFTMI_OK;
}

int siftmi_stage_descriptor(int32_t dev, const float *blurs, int32_t W, int32_t H, int32_t octsize, const float *kps,
                            const int32_t *kp_scale, int64_t n, uint8_t *desc) {
    return siftmi_stage_descriptor_ex(dev, blurs, W, H, octsize, kps, kp_scale, n, desc, 0, 0, nullptr);
}

int siftmi_stage_descriptor_ex(int32_t dev, const float *blurs, int32_t W, int32_t H, int32_t octsize, const float *kps,
                               const int32_t *kp_scale, int64_t n, uint8_t *desc, int32_t form, int32_t blocks, int32_t *form_used) {
    int rc = stage_begin(dev); if (rc) return rc;
    const int kind = form & 3;
    const bool maps = (form & 4) != 0;
    if (form < 0 || form > 7 || (maps && (kind == 0 || kind == 3)))
        return fail(SIFTMI_EINVAL, "descriptor form %d: 0 by window size, 1 wave, 2 workgroup per keypoint, 3 streaming, + 4 maps (1, 2)", form);
    if (blocks < 0) return fail(SIFTMI_EINVAL, "blocks must not be negative");
    if (maps && (rc = stage_maps_scales(kp_scale, n))) return rc;
    int oct;
    if ((rc = stage_octave(octsize, oct))) return rc;
    bool rows_fit = true;
    for (int64_t i = 0; i < n; i++) rows_fit = rows_fit && desc_rows_fit(kps[4 * i + 2], octsize);
    if ((kind == 1 || kind == 2) && !rows_fit) return fail(SIFTMI_EINVAL, "a window of the list has R > %d: streaming form only", SIFT_DESC_MAXRAD);
    const int use = kind ? kind : (rows_fit ? 1 : 3);
    StageOctave so;
    DevBuf r;
    if ((rc = so.upload(blurs, W, H, oct, kps, kp_scale, n, maps)) || (rc = r.alloc((size_t)n * sizeof(KpRecord)))) return rc;
    // every form writes every record, that of a hole or of a window without samples included: a record it drops shows as 0xa5 bytes
    if (n > 0) HIPCHK(hipMemset(r.p, 0xa5, (size_t)n * sizeof(KpRecord)));
    int used = 0;
    if (n > 0) {
        if (maps) launch_maps_kernel(so.tab, oct, oct + 1, g_default_options.maps_blocks, 0);
        // `blocks` is the grid and both of the kernel's count-based cuts; a workgroup per keypoint below `team_below` keypoints
        const int grid = blocks > 0 ? blocks : grid_for(n, 4, 2048), cut = blocks > 0 ? blocks : (1 << 30);
        const int team_below = use == 2 ? (1 << 30) : 0;
        // no counters: the keypoints [0, n) into records [0, n), no pinned copy, no dynamic hand-out
        launch_descriptors(0, use == 3 ? DESC_STREAM : (maps ? DESC_ROWS_MAPS : DESC_ROWS), grid, 0, so.tab, so.k.as<float4>(), so.ks.as<int>(), nullptr, 0,
                           0, (int)n, (int)n, r.as<KpRecord>(), (int)n, nullptr, 0, team_below, 0, cut, cut);
        // what the launch selects (the kernel's own rule, count < team_below, applied here: the kernel reports nothing back)
        used = (use == 3 ? 3 : ((int)n < team_below ? 2 : 1)) | (maps ? 4 : 0);
    }
    if ((rc = stage_end())) return rc;
    if (form_used) *form_used = used;
    std::vector<KpRecord> h((size_t)n);
    if (n > 0) HIPCHK(hipMemcpy(h.data(), r.p, (size_t)n * sizeof(KpRecord), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < n; i++) memcpy(desc + (size_t)i * 128, h[(size_t)i].desc, 128);
    return SIFTMI_OK;
}

int siftmi_stage_gradient_maps(int32_t dev, const float *planes, int32_t n_oct, const int32_t *W, const int32_t *H,
                               int32_t oct_lo, int32_t oct_hi, int32_t blocks, float *gmap, float *omap) {
    int rc = stage_begin(dev); if (rc) return rc;
    if (!planes || !W || !H || !gmap || !omap) return fail(SIFTMI_EINVAL, "null argument");
    if (n_oct < 1 || n_oct > SIFT_MAX_OCTAVES) return fail(SIFTMI_EINVAL, "n_oct must be in 1..%d", SIFT_MAX_OCTAVES);
    if (oct_lo < 0 || oct_hi < oct_lo || oct_hi > n_oct) return fail(SIFTMI_EINVAL, "octave range [%d, %d) outside [0, %d)", oct_lo, oct_hi, n_oct);
    if (blocks < 0) return fail(SIFTMI_EINVAL, "blocks must not be negative");
    OctaveTable tab;
    memset(&tab, 0, sizeof tab);
    size_t total = 0;                    // floats of the plane buffer (the maps: half of it)
    for (int o = 0; o < n_oct; o++) {
        if (W[o] < 1 || H[o] < 1 || (int64_t)W[o] * H[o] > (1 << 30)) return fail(SIFTMI_EINVAL, "octave %d: bad size %d x %d", o, W[o], H[o]);
        tab.off[o] = (long long)total; tab.W[o] = W[o]; tab.H[o] = H[o];
        total += 6 * (size_t)W[o] * H[o];
    }
    DevBuf b, gm, om;
    if ((rc = b.upload(planes, total * 4)) || (rc = gm.upload(gmap, total / 2 * 4)) || (rc = om.upload(omap, total / 2 * 4))) return rc;
    tab.base = b.as<float>(); tab.gmap = gm.as<float>(); tab.omap = om.as<float>();
    launch_maps_kernel(tab, oct_lo, oct_hi, blocks > 0 ? blocks : g_default_options.maps_blocks, 0);      // blocks: width of the grid stride (0: the plan's default)
    if ((rc = stage_end())) return rc;
    HIPCHK(hipMemcpy(gmap, gm.p, total / 2 * 4, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(omap, om.p, total / 2 * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

int siftmi_stage_shrink(int32_t dev, const float *in, float *out, int32_t W, int32_t H) {
    int rc = stage_begin(dev); if (rc) return rc;
    const int SW = W / 2, SH = H / 2;
    DevBuf a, o;
    if ((rc = a.upload(in, (size_t)W * H * 4)) || (rc = o.alloc((size_t)SW * SH * 4))) return rc;
    if (SW > 0 && SH > 0)
        hipLaunchKernelGGL(shrink_kernel, shrink_grid(SW, SH), dim3(256), 0, 0, a.as<float>(), o.as<float>(), W, SW, SH);
    if ((rc = stage_end())) return rc;
    HIPCHK(hipMemcpy(out, o.p, (size_t)SW * SH * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

int siftmi_stage_convert(int32_t dev, const void *in, int32_t dt, float *out, int32_t W, int32_t H) {
    int rc = stage_begin(dev); if (rc) return rc;
    const size_t N = (size_t)W * H;
    if (dtype_size(dt) == 0) return fail(SIFTMI_EINVAL, "invalid input format (%d)", dt);
    DevBuf a, o;
    if ((rc = a.upload(in, N * dtype_size(dt))) || (rc = o.alloc(N * 4))) return rc;
    // (an f32 frame is copied: the plan never converts one)
    if (dt == SIFTMI_F32) HIPCHK(hipMemcpy(o.p, a.p, N * 4, hipMemcpyDeviceToDevice));
    else launch_convert(0, dt, a.p, o.as<float>(), (int64_t)N);
    if ((rc = stage_end())) return rc;
    HIPCHK(hipMemcpy(out, o.p, N * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

int siftmi_stage_math(int32_t dev, int32_t fn, const float *a, const float *b, float *out, int64_t n) {
    int rc = stage_begin(dev); if (rc) return rc;
    DevBuf da, db, o;
    if ((rc = da.upload(a, (size_t)n * 4)) || (rc = db.upload(b ? b : a, (size_t)n * 4)) || (rc = o.alloc((size_t)n * 4))) return rc;
    hipLaunchKernelGGL(math_kernel, dim3(grid_for(n, 256, 4096)), dim3(256), 0, 0, fn, da.as<float>(), db.as<float>(), o.as<float>(), n);
    if ((rc = stage_end())) return rc;
    HIPCHK(hipMemcpy(out, o.p, (size_t)n * 4, hipMemcpyDeviceToHost));
    return SIFTMI_OK;
}

}  // extern "C"
