// match.hip -- MatchPlan's side of libsiftmi.so: the brute-force matcher (k_match.hpp), its windowed form
// (k_match_window.hpp), the k-nearest-neighbour scans that return distances (k_knn.hpp: L1, k_knn_l2.hpp: squared Euclidean, k_knn_window.hpp: either one inside a search window), the consensus filter over the pairs (k_consensus.hpp) the least-squares affine map of the pairs (k_fit.hpp), their exact median displacement (k_shift.hpp), the matcher over a batch of segment pairs (k_match_batch.hpp) the fit and the median of every segment of such a batch at once (k_estimate_batch.hpp) and the consensus filter over every segment at once (k_consensus_batch.hpp) and the windowed matcher over a batch of segment pairs (k_match_window_batch.hpp).  Shares nothing with the SIFT pipeline of siftmi.hip but the error path (host_common.hpp).
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <new>

#include "host_common.hpp"
#include "k_match.hpp"
#include "k_match_window.hpp"
#include "k_knn.hpp"
#include "k_knn_l2.hpp"
#include "k_knn_window.hpp"
#include "k_consensus.hpp"
#include "k_fit.hpp"
#include "k_shift.hpp"
#include "k_match_batch.hpp"
#include "k_estimate_batch.hpp"
#include "k_consensus_batch.hpp"
#include "k_match_window_batch.hpp"

using namespace siftk;

struct siftmi_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t size = 0;
    int profile = 0;
    uint8_t *kp1 = nullptr, *kp2 = nullptr;
    int64_t cap1 = 0, cap2 = 0;
    int2 *pairs = nullptr;
    int64_t cap_pairs = 0;
    MatchPartial *partial = nullptr;
    int64_t cap_partial = 0;
    int *counter = nullptr;
    hipEvent_t ea = nullptr, eb = nullptr;
    float last_ms = 0;
    // profile != 0: the events of match.py:226-263 -- "copy H->D KP_1", "copy H->D KP_2", "matching", "copy D->H match" -- as
    // device times of the last call in ms (-1: the stage did not run: a device-resident list, no pair to copy)
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    float stage_ms[4] = {-1.f, -1.f, -1.f, -1.f};
    // ROI mask (MatchPlan.set_roi, match.py:312-320) and the scratch of the masked / mutual variants
    int8_t *roi = nullptr;
    int64_t cap_roi = 0;
    int roi_w = 0, roi_h = 0;
    uint8_t *q1 = nullptr, *l1 = nullptr, *q2 = nullptr, *l2 = nullptr;   // per-keypoint flags (as query / as list element)
    int64_t cap_q1 = 0, cap_l1 = 0, cap_q2 = 0, cap_l2 = 0;
    int *nearest = nullptr;
    int64_t cap_nearest = 0;
    int2 *pairs2 = nullptr;
    int64_t cap_pairs2 = 0;
    // consensus filter (siftmi_match_consensus): the gathered matches, the hypotheses and their votes; grown on demand
    float4 *c_pts = nullptr;
    uint8_t *c_mask = nullptr, *c_valid = nullptr;
    float *c_models = nullptr;
    int *c_votes = nullptr;
    int64_t cap_c_pts = 0, cap_c_mask = 0, cap_c_valid = 0, cap_c_models = 0, cap_c_votes = 0;
    ConsensusResult *c_result = nullptr;
    hipEvent_t ec_a = nullptr, ec_b = nullptr;
    // windowed matching (siftmi_match_window): header + two histograms + two scans over the cells, the work list, the dense
    // cell-sorted copy of the list (descriptors; x, y, original index) and the queries' order; grown on demand
    int *w_cells = nullptr;
    int2 *w_work = nullptr;
    uint4 *w_desc = nullptr;
    float4 *w_meta = nullptr;
    int *w_order = nullptr;
    int64_t cap_w_cells = 0, cap_w_work = 0, cap_w_desc = 0, cap_w_meta = 0, cap_w_order = 0;
    // k nearest neighbours (siftmi_match_knn_metric): the partitions' keys (32-bit words: one per L1 key, two per squared-Euclidean key)
    // and the result (n1 * k indices, then n1 * k distances); grown on demand
    uint32_t *knn_keys = nullptr;
    int32_t *knn_out = nullptr;
    int64_t cap_knn_keys = 0, cap_knn_out = 0;
    // least-squares fit (siftmi_match_fit): the staged copy of a host mask and the workgroups' partial sums; on demand
    uint8_t *f_mask = nullptr;
    int64_t cap_f_mask = 0;
    FitPartials *f_part = nullptr;
    // median displacement (siftmi_match_shift): the pairs' keys and the select's counters; on demand.  A host mask is staged in
    // f_mask, the positions in c_pts and a keep mask in c_mask, as the calls above do
    uint2 *s_keys = nullptr;
    int64_t cap_s_keys = 0;
    ShiftScratch *s_scratch = nullptr;
    // batch matching (siftmi_match_batch): the tables in pinned host memory (followed by the segments' scan values, which come
    // back there) and on the device, and the integer scratch of the compaction (dense results, the blocks' sums and offsets, the
    // segments' scan values); on demand.  The partials, `nearest` and, for a host result, `pairs` are the ones above
    uint8_t *mb_host = nullptr, *mb_tab = nullptr;
    int64_t cap_mb_host = 0, cap_mb_tab = 0;
    int *mb_ints = nullptr;
    int64_t cap_mb_ints = 0;
    // windowed batch matching (siftmi_match_window_batch) has no buffer of its own: its integer scratch (extents, histograms, scans,
    // work counts) lies in w_cells, its work list, dense copy and order in w_work, w_desc, w_meta and w_order, its tables in mb_host
    // and mb_tab, the dense results, sums and offsets in mb_ints; `nearest` and, for a host result, `pairs` are the ones above
    // segmented fit and median (siftmi_match_fit_batch / siftmi_match_shift_batch): the tables in pinned host memory (followed by the
    // per-segment results, which come back there) and on the device, the fit's partials and results, the median's results; on
    // demand.  Lists, pairs, mask, positions, keys and keep bytes are staged in the buffers of the single calls above
    uint8_t *eb_host = nullptr, *eb_tab = nullptr, *eb_res = nullptr;
    int64_t cap_eb_host = 0, cap_eb_tab = 0, cap_eb_res = 0;
    double *eb_f64 = nullptr;
    int64_t cap_eb_f64 = 0;
    // segmented consensus (siftmi_match_consensus_batch): its table and the segments' results use eb_host, eb_tab and eb_res, the
    // hypotheses of all active segments c_models, c_valid and c_votes, a host mask comes back through c_mask
};

namespace {
int ensure(void **ptr, int64_t *cap, int64_t need, size_t elem) {
    if (need <= *cap && *ptr) return SIFTMI_OK;
    if (*ptr) hipFree(*ptr);
    *ptr = nullptr; *cap = 0;
    hipError_t e = hipMalloc(ptr, (size_t)(need > 0 ? need : 1) * elem);
    if (e != hipSuccess) return fail(SIFTMI_ENOMEM, "hipMalloc(%lld x %zu): %s", (long long)need, elem, hipGetErrorString(e));
    *cap = need;
    return SIFTMI_OK;
}
// a host list of n records is staged in the matcher's own buffer (*d then points there); a device list is used where it lies
int stage_list(siftmi_matcher *m, uint8_t **buf, int64_t *cap, const siftmi_keypoint *kp, int64_t n, const uint8_t **d) {
    int rc = ensure((void **)buf, cap, n, 144);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(*buf, kp, (size_t)n * 144, hipMemcpyHostToDevice, m->stream));
    *d = *buf;
    return SIFTMI_OK;
}
}  // namespace

extern "C" {

int siftmi_match_create(int64_t size, int32_t device_id, int32_t profile, siftmi_matcher **out) {
    if (!out) return fail(SIFTMI_EINVAL, "null argument");
    *out = nullptr;
    if (size < 1) return fail(SIFTMI_EINVAL, "size must be >= 1");
    int ndev = siftmi_device_count();
    if (ndev < 1) return fail(SIFTMI_EDEVICE, "no HIP device available");
    if (device_id < 0 || device_id >= ndev) return fail(SIFTMI_EINVAL, "device %d out of range", device_id);
    HIPCHK(hipSetDevice(device_id));
    siftmi_matcher *m = new (std::nothrow) siftmi_matcher();
    if (!m) return fail(SIFTMI_ENOMEM, "host allocation failed");
    m->device = device_id; m->size = size; m->profile = profile;
    int rc = SIFTMI_OK;
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) rc = fail(SIFTMI_EDEVICE, "hipStreamCreate failed");
    if (!rc) rc = ensure((void **)&m->kp1, &m->cap1, size, 144);
    if (!rc) rc = ensure((void **)&m->kp2, &m->cap2, size, 144);
    if (!rc) rc = ensure((void **)&m->pairs, &m->cap_pairs, size, sizeof(int2));
    if (!rc && hipMalloc((void **)&m->counter, 16) != hipSuccess) rc = fail(SIFTMI_ENOMEM, "hipMalloc failed");
    if (!rc) { hipEventCreate(&m->ea); hipEventCreate(&m->eb); hipEventCreate(&m->ec_a); hipEventCreate(&m->ec_b); }
    if (!rc && profile) for (hipEvent_t &e : m->ev) if (hipEventCreate(&e) != hipSuccess) rc = fail(SIFTMI_EDEVICE, "hipEventCreate failed");
    if (rc) { std::string keep = g_err; siftmi_match_destroy(m); g_err = keep; return rc; }
    *out = m;
    return SIFTMI_OK;
}

int siftmi_match_destroy(siftmi_matcher *m) {
    if (!m) return SIFTMI_OK;
    hipSetDevice(m->device);
    if (m->stream) hipStreamSynchronize(m->stream);
    if (m->kp1) hipFree(m->kp1);
    if (m->kp2) hipFree(m->kp2);
    if (m->pairs) hipFree(m->pairs);
    if (m->partial) hipFree(m->partial);
    for (void *q : {(void *)m->roi, (void *)m->q1, (void *)m->l1, (void *)m->q2, (void *)m->l2, (void *)m->nearest, (void *)m->pairs2,
                    (void *)m->c_pts, (void *)m->c_mask, (void *)m->c_valid, (void *)m->c_models, (void *)m->c_votes, (void *)m->c_result,
                    (void *)m->w_cells, (void *)m->w_work, (void *)m->w_desc, (void *)m->w_meta, (void *)m->w_order,
                    (void *)m->knn_keys, (void *)m->knn_out, (void *)m->f_mask, (void *)m->f_part, (void *)m->s_keys, (void *)m->s_scratch,
                    (void *)m->mb_tab, (void *)m->mb_ints, (void *)m->eb_tab, (void *)m->eb_res, (void *)m->eb_f64})
        if (q) hipFree(q);
    if (m->mb_host) hipHostFree(m->mb_host);
    if (m->eb_host) hipHostFree(m->eb_host);
    if (m->ec_a) hipEventDestroy(m->ec_a);
    if (m->ec_b) hipEventDestroy(m->ec_b);
    if (m->counter) hipFree(m->counter);
    if (m->ea) hipEventDestroy(m->ea);
    if (m->eb) hipEventDestroy(m->eb);
    for (hipEvent_t e : m->ev) if (e) hipEventDestroy(e);
    if (m->stream) hipStreamDestroy(m->stream);
    delete m;
    return SIFTMI_OK;
}

int siftmi_match_set_roi(siftmi_matcher *m, const int8_t *roi, int32_t roi_width, int32_t roi_height) {
    if (!m) return fail(SIFTMI_EINVAL, "null matcher");
    HIPCHK(hipSetDevice(m->device));
    if (!roi) { m->roi_w = m->roi_h = 0; return SIFTMI_OK; }       // unset_roi
    if (roi_width < 1 || roi_height < 1) return fail(SIFTMI_EINVAL, "bad ROI shape %d x %d", roi_width, roi_height);
    int rc = ensure((void **)&m->roi, &m->cap_roi, (int64_t)roi_width * roi_height, 1);
    if (rc) return rc;
    HIPCHK(hipMemcpy(m->roi, roi, (size_t)roi_width * roi_height, hipMemcpyHostToDevice));
    m->roi_w = roi_width; m->roi_h = roi_height;
    return SIFTMI_OK;
}

namespace {
// one direction of the brute-force scan: partials of `nq` queries against `nl` list elements, folded by the merge kernel
int match_direction(siftmi_matcher *m, const uint8_t *dq, int64_t nq, const uint8_t *dl, int64_t nl, const uint8_t *qflag,
                    const uint8_t *lflag, float ratio_th, int2 *pairs, int cap, int *nearest) {
    // 2-D decomposition: query blocks x partitions of the list, enough workgroups to fill 256 CUs
    const int qblocks = (int)((nq + 256 * SIFT_MATCH_QPT - 1) / (256 * SIFT_MATCH_QPT));
    int nparts = (2048 + qblocks - 1) / qblocks;
    const int max_parts = (int)((nl + 4 * SIFT_MATCH_TILE - 1) / (4 * SIFT_MATCH_TILE));
    if (nparts > max_parts) nparts = max_parts;
    const int min_parts = (int)((nl + SIFT_MATCH_MAX_PART - 1) / SIFT_MATCH_MAX_PART);     // 16-bit index inside a partition
    if (nparts < min_parts) nparts = min_parts;
    if (nparts < 1) nparts = 1;
    int part_len = (int)((nl + nparts - 1) / nparts);
    part_len = (part_len + SIFT_MATCH_TILE - 1) / SIFT_MATCH_TILE * SIFT_MATCH_TILE;
    nparts = (int)((nl + part_len - 1) / part_len);
    int rc;
    if ((rc = ensure((void **)&m->partial, &m->cap_partial, (int64_t)nparts * nq, sizeof(MatchPartial)))) return rc;
    const dim3 grid((unsigned)qblocks, (unsigned)nparts);
    if (lflag)
        hipLaunchKernelGGL(match_partial_kernel<true>, grid, dim3(256), 0, m->stream, dq, (int)nq, dl, (int)nl, part_len, m->partial, qflag, lflag);
    else
        hipLaunchKernelGGL(match_partial_kernel<false>, grid, dim3(256), 0, m->stream, dq, (int)nq, dl, (int)nl, part_len, m->partial,
                           (const uint8_t *)nullptr, (const uint8_t *)nullptr);
    hipLaunchKernelGGL(match_merge_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, m->stream,
                       (const MatchPartial *)m->partial, (int)nq, nparts, ratio_th, pairs, m->counter, cap, qflag, nearest);
    return SIFTMI_OK;
}
}  // namespace

int siftmi_match_ex(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                    const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, float ratio_th, int32_t roi_mode,
                    int32_t mutual, int32_t *pairs, int64_t capacity, int64_t *n_out, int64_t *n_total) {
    if (!m || !n_out) return fail(SIFTMI_EINVAL, "null argument");
    if (n1 < 0 || n2 < 0 || n1 > 0x7fffffff || n2 > 0x7fffffff) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (roi_mode < 0 || roi_mode > 2) return fail(SIFTMI_EINVAL, "roi_mode must be 0 (off), 1 (matching_valid) or 2 (strict)");
    if (roi_mode && !(m->roi && m->roi_w > 0)) return fail(SIFTMI_EINVAL, "roi_mode %d without a region of interest (siftmi_match_set_roi)", roi_mode);
    HIPCHK(hipSetDevice(m->device));
    *n_out = 0;
    if (n_total) *n_total = 0;
    for (float &v : m->stage_ms) v = -1.f;
    if (n1 == 0 || n2 == 0) return SIFTMI_OK;   // dist1 == dist2 == 1e12 -> ratio 1, never < ratio_th
    if (kp1_is_device || kp2_is_device) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2;
    int rc;
    const bool prof = m->profile && m->ev[0];
    if (prof) hipEventRecord(m->ev[0], m->stream);
    if (!kp1_is_device && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (prof) hipEventRecord(m->ev[1], m->stream);
    if (!kp2_is_device && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (prof) hipEventRecord(m->ev[2], m->stream);
    // match.py:241-243,252: kpsize grows to min(n1, n2) and stays grown; the output capacity is kpsize
    if ((n1 < n2 ? n1 : n2) > m->size) m->size = (n1 < n2 ? n1 : n2);
    const int64_t cap = m->size;
    if ((rc = ensure((void **)&m->pairs, &m->cap_pairs, cap, sizeof(int2)))) return rc;
    HIPCHK(hipMemsetAsync(m->counter, 0, 8, m->stream));
    hipEventRecord(m->ea, m->stream);
    const uint8_t *qf1 = nullptr, *lf2 = nullptr;
    if (roi_mode) {
        if ((rc = ensure((void **)&m->q1, &m->cap_q1, n1, 1)) || (rc = ensure((void **)&m->l1, &m->cap_l1, n1, 1)) ||
            (rc = ensure((void **)&m->q2, &m->cap_q2, n2, 1)) || (rc = ensure((void **)&m->l2, &m->cap_l2, n2, 1))) return rc;
        hipLaunchKernelGGL(match_roi_flags_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, m->stream, d1, (int)n1,
                           (const int8_t *)m->roi, m->roi_w, m->roi_h, roi_mode, m->q1, m->l1);
        hipLaunchKernelGGL(match_roi_flags_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, m->stream, d2, (int)n2,
                           (const int8_t *)m->roi, m->roi_w, m->roi_h, roi_mode, m->q2, m->l2);
        qf1 = m->q1; lf2 = m->l2;
    }
    if ((rc = match_direction(m, d1, n1, d2, n2, qf1, lf2, ratio_th, m->pairs, (int)cap, nullptr))) return rc;
    int2 *result = m->pairs;
    int *result_counter = m->counter;
    int count = 0;
    if (mutual) {
        // reverse scan: nearest list-1 keypoint of every list-2 keypoint over the same masked distances
        if ((rc = ensure((void **)&m->nearest, &m->cap_nearest, n2, sizeof(int))) ||
            (rc = ensure((void **)&m->pairs2, &m->cap_pairs2, cap, sizeof(int2)))) return rc;
        const uint8_t *qf2 = nullptr, *lf1 = nullptr;
        if (roi_mode) {
            hipLaunchKernelGGL(match_reverse_flags_kernel, dim3((unsigned)((n2 + 255) / 256)), dim3(256), 0, m->stream, (const uint8_t *)m->l2, (int)n2, m->q2);
            hipLaunchKernelGGL(match_reverse_list_flags_kernel, dim3((unsigned)((n1 + 255) / 256)), dim3(256), 0, m->stream, (const uint8_t *)m->q1, (int)n1, m->l1);
            qf2 = m->q2; lf1 = m->l1;
        }
        HIPCHK(hipMemcpyAsync(&count, m->counter, 4, hipMemcpyDeviceToHost, m->stream));   // forward count (the partial buffer is reused below)
        if ((rc = match_direction(m, d2, n2, d1, n1, qf2, lf1, ratio_th, nullptr, 0, m->nearest))) return rc;
        HIPCHK(hipStreamSynchronize(m->stream));
        const int nfwd = count < cap ? count : (int)cap;
        if (nfwd > 0)
            hipLaunchKernelGGL(match_mutual_filter_kernel, dim3((unsigned)((nfwd + 255) / 256)), dim3(256), 0, m->stream,
                               (const int2 *)m->pairs, nfwd, (const int *)m->nearest, m->pairs2, m->counter + 1);
        result = m->pairs2; result_counter = m->counter + 1;
    }
    hipEventRecord(m->eb, m->stream);
    HIPCHK(hipMemcpyAsync(&count, result_counter, 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    hipEventElapsedTime(&m->last_ms, m->ea, m->eb);
    if (n_total) *n_total = count;
    int64_t n = count < cap ? count : cap;
    rc = SIFTMI_OK;
    if (n > capacity) { n = capacity; rc = SIFTMI_ECAPACITY; g_err = "pair capacity too small; result truncated"; }
    if (prof) {
        m->stage_ms[2] = m->last_ms;
        if (!kp1_is_device) hipEventElapsedTime(&m->stage_ms[0], m->ev[0], m->ev[1]);
        if (!kp2_is_device) hipEventElapsedTime(&m->stage_ms[1], m->ev[1], m->ev[2]);
    }
    if (n > 0) {
        if (!pairs) return fail(SIFTMI_EINVAL, "null pairs buffer");
        if (prof) {
            hipEventRecord(m->ev[3], m->stream);
            HIPCHK(hipMemcpyAsync(pairs, result, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost, m->stream));
            hipEventRecord(m->ev[4], m->stream);
            HIPCHK(hipStreamSynchronize(m->stream));
            hipEventElapsedTime(&m->stage_ms[3], m->ev[3], m->ev[4]);
        } else {
            HIPCHK(hipMemcpy(pairs, result, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost));
        }
    }
    *n_out = n;
    return rc;
}

int siftmi_match(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                 const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, float ratio_th, int32_t *pairs,
                 int64_t capacity, int64_t *n_out, int64_t *n_total) {
    return siftmi_match_ex(m, kp1, n1, kp1_is_device, kp2, n2, kp2_is_device, ratio_th, 0, 0, pairs, capacity, n_out, n_total);
}

// Windowed matching (k_match_window.hpp; the contract is DESIGN.md section 7 row 6).  Both lists are used where they lie.
namespace {
constexpr int64_t MW_CELL_WORDS = SIFT_MW_HDR + 4 * (int64_t)(SIFT_MW_MAXCELLS + 1);
// work items of `nq` queries at most: a cell's last chunk may be partial, and only a cell with a query has one
int64_t mw_work_cap(int64_t nq) { return nq / SIFT_MW_QB + (nq < SIFT_MW_MAXCELLS ? nq : SIFT_MW_MAXCELLS) + 1; }

int mw_ensure(siftmi_matcher *m, int64_t n1, int64_t n2, bool both) {
    const int64_t nl = both ? (n1 > n2 ? n1 : n2) : n2, nq = both ? nl : n1;
    int rc;
    if ((rc = ensure((void **)&m->w_cells, &m->cap_w_cells, MW_CELL_WORDS, sizeof(int))) ||
        (rc = ensure((void **)&m->w_work, &m->cap_w_work, mw_work_cap(nq), sizeof(int2))) ||
        (rc = ensure((void **)&m->w_desc, &m->cap_w_desc, nl * 8, sizeof(uint4))) ||
        (rc = ensure((void **)&m->w_meta, &m->cap_w_meta, nl, sizeof(float4))) ||
        (rc = ensure((void **)&m->w_order, &m->cap_w_order, nq, sizeof(int)))) return rc;
    return SIFTMI_OK;
}

// the grid of one scan: the extent of the list, both histograms, their scans with the work list, the dense cell-sorted copy of
// the list and the queries' order (the scratch is sized by mw_ensure).  (cx, cy) is the shift of the queries' window centre.
struct MwScratch { uint32_t *hdr; int *start_l, *start_q; int work_cap; };
int mw_build_grid(siftmi_matcher *m, const uint8_t *dq, int64_t nq, const uint8_t *dl, int64_t nl, float wx, float wy, float cx, float cy,
                  MwScratch *out) {
    uint32_t *hdr = (uint32_t *)m->w_cells;
    int *cnt_l = m->w_cells + SIFT_MW_HDR, *cnt_q = cnt_l + SIFT_MW_MAXCELLS + 1;
    int *start_l = cnt_q + SIFT_MW_MAXCELLS + 1, *start_q = start_l + SIFT_MW_MAXCELLS + 1;
    const int work_cap = (int)mw_work_cap(nq);
    const dim3 bl((unsigned)((nl + 255) / 256)), bq((unsigned)((nq + 255) / 256));
    // minima start at 0xffffffff, maxima, the work count and both histograms at 0
    HIPCHK(hipMemsetAsync(hdr, 0xff, 2 * sizeof(uint32_t), m->stream));
    HIPCHK(hipMemsetAsync(hdr + 2, 0, (size_t)(SIFT_MW_HDR - 2 + 2 * (SIFT_MW_MAXCELLS + 1)) * sizeof(int), m->stream));
    hipLaunchKernelGGL(mw_extent_kernel, bl, dim3(256), 0, m->stream, dl, (int)nl, hdr);
    hipLaunchKernelGGL(mw_count_kernel, bl, dim3(256), 0, m->stream, dl, (int)nl, (const uint32_t *)hdr, wx, wy, 0.f, 0.f, cnt_l);
    hipLaunchKernelGGL(mw_count_kernel, bq, dim3(256), 0, m->stream, dq, (int)nq, (const uint32_t *)hdr, wx, wy, cx, cy, cnt_q);
    hipLaunchKernelGGL(mw_scan_kernel, dim3(1), dim3(1024), 0, m->stream, hdr, wx, wy, cnt_l, cnt_q, start_l, start_q, m->w_work, work_cap);
    hipLaunchKernelGGL(mw_scatter_list_kernel, dim3((unsigned)((nl * 8 + 255) / 256)), dim3(256), 0, m->stream, dl, (int)nl,
                       (const uint32_t *)hdr, wx, wy, cnt_l, m->w_desc, m->w_meta);
    hipLaunchKernelGGL(mw_scatter_query_kernel, bq, dim3(256), 0, m->stream, dq, (int)nq, (const uint32_t *)hdr, wx, wy, cx, cy, cnt_q, m->w_order);
    *out = {hdr, start_l, start_q, work_cap};
    return SIFTMI_OK;
}

// one direction of the windowed scan: `nq` queries against the candidates among `nl` list elements (the scratch is sized by
// mw_ensure).  reverse: the queries are list-2 keypoints; the predicate keeps (x2 - x1) - sx, so their window centre is x2 - sx.
int match_window_direction(siftmi_matcher *m, const uint8_t *dq, int64_t nq, const uint8_t *dl, int64_t nl, int reverse, float wx, float wy,
                           float sx, float sy, float ratio_th, int2 *pairs, int cap, int *nearest) {
    MwScratch s;
    int rc;
    if ((rc = mw_build_grid(m, dq, nq, dl, nl, wx, wy, reverse ? -sx : sx, reverse ? -sy : sy, &s))) return rc;
    hipLaunchKernelGGL(mw_match_kernel, dim3((unsigned)s.work_cap), dim3(256), 0, m->stream, dq, (int)nq, (int)nl, (const uint32_t *)s.hdr,
                       wx, wy, sx, sy, reverse, (const int *)s.start_l, (const int *)s.start_q, (const int *)m->w_order, (const int2 *)m->w_work,
                       (const uint4 *)m->w_desc, (const float4 *)m->w_meta, ratio_th, pairs, m->counter, cap, nearest);
    return SIFTMI_OK;
}
}  // namespace

int siftmi_match_window(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                        const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, float ratio_th, float wx, float wy,
                        float sx, float sy, int32_t mutual, int32_t *pairs, int64_t capacity, int64_t *n_out, int64_t *n_total) {
    if (!m || !n_out) return fail(SIFTMI_EINVAL, "null argument");
    if (n1 < 0 || n2 < 0 || n1 > 0x7fffffff / 8 || n2 > 0x7fffffff / 8) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (!(wx >= 0.f) || !(wy >= 0.f)) return fail(SIFTMI_EINVAL, "the window must be >= 0 (it may be infinite), not (%g, %g)", wx, wy);
    if (!std::isfinite(sx) || !std::isfinite(sy)) return fail(SIFTMI_EINVAL, "the window shift must be finite, not (%g, %g)", sx, sy);
    HIPCHK(hipSetDevice(m->device));
    *n_out = 0;
    if (n_total) *n_total = 0;
    for (float &v : m->stage_ms) v = -1.f;
    if (n1 == 0 || n2 == 0) return SIFTMI_OK;   // no candidate: dist1 == dist2 == 1e12 -> ratio 1, never < ratio_th
    if (kp1_is_device || kp2_is_device) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2;
    int rc;
    const bool prof = m->profile && m->ev[0];
    if (prof) hipEventRecord(m->ev[0], m->stream);
    if (!kp1_is_device && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (prof) hipEventRecord(m->ev[1], m->stream);
    if (!kp2_is_device && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (prof) hipEventRecord(m->ev[2], m->stream);
    if ((n1 < n2 ? n1 : n2) > m->size) m->size = (n1 < n2 ? n1 : n2);      // as siftmi_match_ex: the size grows to min(n1, n2)
    const int64_t cap = m->size;
    if ((rc = ensure((void **)&m->pairs, &m->cap_pairs, cap, sizeof(int2))) || (rc = mw_ensure(m, n1, n2, mutual != 0))) return rc;
    if (mutual && ((rc = ensure((void **)&m->nearest, &m->cap_nearest, n2, sizeof(int))) ||
                   (rc = ensure((void **)&m->pairs2, &m->cap_pairs2, cap, sizeof(int2))))) return rc;
    HIPCHK(hipMemsetAsync(m->counter, 0, 8, m->stream));
    hipEventRecord(m->ea, m->stream);
    if ((rc = match_window_direction(m, d1, n1, d2, n2, 0, wx, wy, sx, sy, ratio_th, m->pairs, (int)cap, nullptr))) return rc;
    int2 *result = m->pairs;
    int *result_counter = m->counter;
    if (mutual) {
        // reverse scan: the nearest candidate among list 1 of every list-2 keypoint, then the filter over the forward pairs
        if ((rc = match_window_direction(m, d2, n2, d1, n1, 1, wx, wy, sx, sy, ratio_th, nullptr, 0, m->nearest))) return rc;
        hipLaunchKernelGGL(mw_mutual_filter_kernel, dim3((unsigned)((cap + 255) / 256)), dim3(256), 0, m->stream, (const int2 *)m->pairs,
                           (const int *)m->counter, (int)cap, (const int *)m->nearest, (int)n2, m->pairs2, m->counter + 1);
        result = m->pairs2; result_counter = m->counter + 1;
    }
    hipEventRecord(m->eb, m->stream);
    int count = 0;
    HIPCHK(hipMemcpyAsync(&count, result_counter, 4, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    hipEventElapsedTime(&m->last_ms, m->ea, m->eb);
    if (n_total) *n_total = count;
    int64_t n = count < cap ? count : cap;
    rc = SIFTMI_OK;
    if (n > capacity) { n = capacity; rc = SIFTMI_ECAPACITY; g_err = "pair capacity too small; result truncated"; }
    if (prof) {
        m->stage_ms[2] = m->last_ms;
        if (!kp1_is_device) hipEventElapsedTime(&m->stage_ms[0], m->ev[0], m->ev[1]);
        if (!kp2_is_device) hipEventElapsedTime(&m->stage_ms[1], m->ev[1], m->ev[2]);
    }
    if (n > 0) {
        if (!pairs) return fail(SIFTMI_EINVAL, "null pairs buffer");
        if (prof) {
            hipEventRecord(m->ev[3], m->stream);
            HIPCHK(hipMemcpyAsync(pairs, result, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost, m->stream));
            hipEventRecord(m->ev[4], m->stream);
            HIPCHK(hipStreamSynchronize(m->stream));
            hipEventElapsedTime(&m->stage_ms[3], m->ev[3], m->ev[4]);
        } else {
            HIPCHK(hipMemcpy(pairs, result, (size_t)n * sizeof(int2), hipMemcpyDeviceToHost));
        }
    }
    *n_out = n;
    return rc;
}

// k nearest neighbours with their distances (k_knn.hpp, k_knn_l2.hpp; the contract is DESIGN.md section 7 rows 7 and 8).
namespace {
// the decomposition of match_direction: query blocks x partitions of the list, about 2048 workgroups, a partition a whole number
// of tiles and at most SIFT_MATCH_MAX_PART elements
void knn_partitions(int64_t nq, int64_t nl, int *qblocks, int *nparts, int *part_len) {
    *qblocks = (int)((nq + 256 * SIFT_MATCH_QPT - 1) / (256 * SIFT_MATCH_QPT));
    int np = (2048 + *qblocks - 1) / *qblocks;
    const int max_parts = (int)((nl + 4 * SIFT_MATCH_TILE - 1) / (4 * SIFT_MATCH_TILE));
    if (np > max_parts) np = max_parts;
    const int min_parts = (int)((nl + SIFT_MATCH_MAX_PART - 1) / SIFT_MATCH_MAX_PART);     // 16-bit index inside a partition
    if (np < min_parts) np = min_parts;
    if (np < 1) np = 1;
    int len = (int)((nl + np - 1) / np);
    len = (len + SIFT_MATCH_TILE - 1) / SIFT_MATCH_TILE * SIFT_MATCH_TILE;
    *part_len = len;
    *nparts = (int)((nl + len - 1) / len);
}
// the instance a requested k (1 .. SIFT_KNN_MAX) runs on: the next of 1, 2, 4, 8
int knn_instance(int k) { return k <= 1 ? 1 : k <= 2 ? 2 : k <= 4 ? 4 : 8; }

void launch_knn_partial(hipStream_t st, int K, dim3 grid, const uint8_t *dq, int nq, const uint8_t *dl, int nl, int part_len, uint32_t *keys) {
    switch (K) {
    case 1: hipLaunchKernelGGL(knn_partial_kernel<1>, grid, dim3(256), 0, st, dq, nq, dl, nl, part_len, keys); break;
    case 2: hipLaunchKernelGGL(knn_partial_kernel<2>, grid, dim3(256), 0, st, dq, nq, dl, nl, part_len, keys); break;
    case 4: hipLaunchKernelGGL(knn_partial_kernel<4>, grid, dim3(256), 0, st, dq, nq, dl, nl, part_len, keys); break;
    default: hipLaunchKernelGGL(knn_partial_kernel<8>, grid, dim3(256), 0, st, dq, nq, dl, nl, part_len, keys); break;
    }
}
void launch_knn_merge(hipStream_t st, int K, const uint32_t *keys, int nq, int nparts, int part_len, int k, int32_t *idx, int32_t *dist) {
    const dim3 grid((unsigned)((nq + 255) / 256));
    switch (K) {
    case 1: hipLaunchKernelGGL(knn_merge_kernel<1>, grid, dim3(256), 0, st, keys, nq, nparts, part_len, k, idx, dist); break;
    case 2: hipLaunchKernelGGL(knn_merge_kernel<2>, grid, dim3(256), 0, st, keys, nq, nparts, part_len, k, idx, dist); break;
    case 4: hipLaunchKernelGGL(knn_merge_kernel<4>, grid, dim3(256), 0, st, keys, nq, nparts, part_len, k, idx, dist); break;
    default: hipLaunchKernelGGL(knn_merge_kernel<8>, grid, dim3(256), 0, st, keys, nq, nparts, part_len, k, idx, dist); break;
    }
}
void launch_knn_l2_partial(hipStream_t st, int K, dim3 grid, const uint8_t *dq, int nq, const uint8_t *dl, int nl, int part_len, uint64_t *keys) {
    switch (K) {
    case 1: hipLaunchKernelGGL(knn_l2_partial_kernel<1>, grid, dim3(256), 0, st, dq, nq, dl, nl, part_len, keys); break;
    case 2: hipLaunchKernelGGL(knn_l2_partial_kernel<2>, grid, dim3(256), 0, st, dq, nq, dl, nl, part_len, keys); break;
    case 4: hipLaunchKernelGGL(knn_l2_partial_kernel<4>, grid, dim3(256), 0, st, dq, nq, dl, nl, part_len, keys); break;
    default: hipLaunchKernelGGL(knn_l2_partial_kernel<8>, grid, dim3(256), 0, st, dq, nq, dl, nl, part_len, keys); break;
    }
}
void launch_knn_l2_merge(hipStream_t st, int K, const uint64_t *keys, const uint8_t *dq, int nq, int nparts, int k, int32_t *idx, int32_t *dist) {
    const dim3 grid((unsigned)((nq + 255) / 256));
    switch (K) {
    case 1: hipLaunchKernelGGL(knn_l2_merge_kernel<1>, grid, dim3(256), 0, st, keys, dq, nq, nparts, k, idx, dist); break;
    case 2: hipLaunchKernelGGL(knn_l2_merge_kernel<2>, grid, dim3(256), 0, st, keys, dq, nq, nparts, k, idx, dist); break;
    case 4: hipLaunchKernelGGL(knn_l2_merge_kernel<4>, grid, dim3(256), 0, st, keys, dq, nq, nparts, k, idx, dist); break;
    default: hipLaunchKernelGGL(knn_l2_merge_kernel<8>, grid, dim3(256), 0, st, keys, dq, nq, nparts, k, idx, dist); break;
    }
}
}  // namespace

int siftmi_match_knn_metric(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                            const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t k, int32_t metric,
                            int32_t *idx_out, int32_t *dist_out) {
    if (!m) return fail(SIFTMI_EINVAL, "null argument");
    if (k < 1 || k > SIFT_KNN_MAX) return fail(SIFTMI_EINVAL, "k must be 1 .. %d, not %d", SIFT_KNN_MAX, k);
    if (metric != SIFTMI_METRIC_L1 && metric != SIFTMI_METRIC_L2SQ)
        return fail(SIFTMI_EINVAL, "metric must be SIFTMI_METRIC_L1 (0) or SIFTMI_METRIC_L2SQ (1), not %d", metric);
    if (n1 < 0 || n2 < 0 || n1 > 0x7fffffff || n2 > 0x7fffffff) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (n1 > 0 && (!idx_out || !dist_out)) return fail(SIFTMI_EINVAL, "null result buffer");
    HIPCHK(hipSetDevice(m->device));
    for (float &v : m->stage_ms) v = -1.f;
    m->last_ms = 0;
    if (n1 == 0) return SIFTMI_OK;
    const size_t cells = (size_t)n1 * (size_t)k;
    if (n2 == 0) {                              // no neighbour at all: nothing is launched
        for (size_t t = 0; t < cells; t++) { idx_out[t] = -1; dist_out[t] = -1; }
        return SIFTMI_OK;
    }
    if (kp1_is_device || kp2_is_device) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2;
    int rc;
    const bool prof = m->profile && m->ev[0];
    if (prof) hipEventRecord(m->ev[0], m->stream);
    if (!kp1_is_device && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (prof) hipEventRecord(m->ev[1], m->stream);
    if (!kp2_is_device && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (prof) hipEventRecord(m->ev[2], m->stream);
    const int K = knn_instance(k);
    int qblocks, nparts, part_len;
    knn_partitions(n1, n2, &qblocks, &nparts, &part_len);
    const bool l2 = metric == SIFTMI_METRIC_L2SQ;
    if ((rc = ensure((void **)&m->knn_keys, &m->cap_knn_keys, (int64_t)nparts * n1 * K * (l2 ? 2 : 1), sizeof(uint32_t))) ||
        (rc = ensure((void **)&m->knn_out, &m->cap_knn_out, 2 * (int64_t)cells, sizeof(int32_t)))) return rc;
    int32_t *d_idx = m->knn_out, *d_dist = m->knn_out + cells;
    hipEventRecord(m->ea, m->stream);
    if (l2) {
        launch_knn_l2_partial(m->stream, K, dim3((unsigned)qblocks, (unsigned)nparts), d1, (int)n1, d2, (int)n2, part_len, (uint64_t *)m->knn_keys);
        launch_knn_l2_merge(m->stream, K, (const uint64_t *)m->knn_keys, d1, (int)n1, nparts, k, d_idx, d_dist);
    } else {
        launch_knn_partial(m->stream, K, dim3((unsigned)qblocks, (unsigned)nparts), d1, (int)n1, d2, (int)n2, part_len, m->knn_keys);
        launch_knn_merge(m->stream, K, m->knn_keys, (int)n1, nparts, part_len, k, d_idx, d_dist);
    }
    hipEventRecord(m->eb, m->stream);
    if (prof) hipEventRecord(m->ev[3], m->stream);
    HIPCHK(hipMemcpyAsync(idx_out, d_idx, cells * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(dist_out, d_dist, cells * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    if (prof) hipEventRecord(m->ev[4], m->stream);
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    hipEventElapsedTime(&m->last_ms, m->ea, m->eb);
    if (prof) {
        m->stage_ms[2] = m->last_ms;
        if (!kp1_is_device) hipEventElapsedTime(&m->stage_ms[0], m->ev[0], m->ev[1]);
        if (!kp2_is_device) hipEventElapsedTime(&m->stage_ms[1], m->ev[1], m->ev[2]);
        hipEventElapsedTime(&m->stage_ms[3], m->ev[3], m->ev[4]);
    }
    return SIFTMI_OK;
}

int siftmi_match_knn(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                     const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t k,
                     int32_t *idx_out, int32_t *dist_out) {
    return siftmi_match_knn_metric(m, kp1, n1, kp1_is_device, kp2, n2, kp2_is_device, k, SIFTMI_METRIC_L1, idx_out, dist_out);
}

// k nearest neighbours inside a search window (k_knn_window.hpp; the contract is DESIGN.md section 7 row 10)
extern "C++" {
namespace {
template <bool L2>
void launch_mw_knn(siftmi_matcher *m, int K, const MwScratch &s, const uint8_t *dq, int nq, int nl, float wx, float wy, float sx, float sy,
                   int k, int32_t *idx, int32_t *dist) {
    const dim3 grid((unsigned)s.work_cap);
#define SIFT_MW_KNN_ARGS dq, nq, nl, (const uint32_t *)s.hdr, wx, wy, sx, sy, (const int *)s.start_l, (const int *)s.start_q, \
                         (const int *)m->w_order, (const int2 *)m->w_work, (const uint4 *)m->w_desc, (const float4 *)m->w_meta, k, idx, dist
    switch (K) {
    case 1: hipLaunchKernelGGL((mw_knn_kernel<1, L2>), grid, dim3(256), 0, m->stream, SIFT_MW_KNN_ARGS); break;
    case 2: hipLaunchKernelGGL((mw_knn_kernel<2, L2>), grid, dim3(256), 0, m->stream, SIFT_MW_KNN_ARGS); break;
    case 4: hipLaunchKernelGGL((mw_knn_kernel<4, L2>), grid, dim3(256), 0, m->stream, SIFT_MW_KNN_ARGS); break;
    default: hipLaunchKernelGGL((mw_knn_kernel<8, L2>), grid, dim3(256), 0, m->stream, SIFT_MW_KNN_ARGS); break;
    }
#undef SIFT_MW_KNN_ARGS
}
}  // namespace
}  // extern "C++"

int siftmi_match_knn_window(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                            const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t k, int32_t metric,
                            float wx, float wy, float sx, float sy, int32_t *idx_out, int32_t *dist_out) {
    if (!m) return fail(SIFTMI_EINVAL, "null argument");
    if (k < 1 || k > SIFT_KNN_MAX) return fail(SIFTMI_EINVAL, "k must be 1 .. %d, not %d", SIFT_KNN_MAX, k);
    if (metric != SIFTMI_METRIC_L1 && metric != SIFTMI_METRIC_L2SQ)
        return fail(SIFTMI_EINVAL, "metric must be SIFTMI_METRIC_L1 (0) or SIFTMI_METRIC_L2SQ (1), not %d", metric);
    if (n1 < 0 || n2 < 0 || n1 > 0x7fffffff / 8 || n2 > 0x7fffffff / 8) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (n1 > 0 && (!idx_out || !dist_out)) return fail(SIFTMI_EINVAL, "null result buffer");
    if (!(wx >= 0.f) || !(wy >= 0.f)) return fail(SIFTMI_EINVAL, "the window must be >= 0 (it may be infinite), not (%g, %g)", wx, wy);
    if (!std::isfinite(sx) || !std::isfinite(sy)) return fail(SIFTMI_EINVAL, "the window shift must be finite, not (%g, %g)", sx, sy);
    HIPCHK(hipSetDevice(m->device));
    for (float &v : m->stage_ms) v = -1.f;
    m->last_ms = 0;
    if (n1 == 0) return SIFTMI_OK;
    const size_t cells = (size_t)n1 * (size_t)k;
    if (n2 == 0) {                              // no candidate at all: nothing is launched
        for (size_t t = 0; t < cells; t++) { idx_out[t] = -1; dist_out[t] = -1; }
        return SIFTMI_OK;
    }
    if (kp1_is_device || kp2_is_device) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2;
    int rc;
    const bool prof = m->profile && m->ev[0];
    if (prof) hipEventRecord(m->ev[0], m->stream);
    if (!kp1_is_device && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (prof) hipEventRecord(m->ev[1], m->stream);
    if (!kp2_is_device && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (prof) hipEventRecord(m->ev[2], m->stream);
    if ((rc = mw_ensure(m, n1, n2, false)) ||
        (rc = ensure((void **)&m->knn_out, &m->cap_knn_out, 2 * (int64_t)cells, sizeof(int32_t)))) return rc;
    int32_t *d_idx = m->knn_out, *d_dist = m->knn_out + cells;
    hipEventRecord(m->ea, m->stream);
    MwScratch s;
    if ((rc = mw_build_grid(m, d1, n1, d2, n2, wx, wy, sx, sy, &s))) return rc;
    if (metric == SIFTMI_METRIC_L2SQ) launch_mw_knn<true>(m, knn_instance(k), s, d1, (int)n1, (int)n2, wx, wy, sx, sy, k, d_idx, d_dist);
    else launch_mw_knn<false>(m, knn_instance(k), s, d1, (int)n1, (int)n2, wx, wy, sx, sy, k, d_idx, d_dist);
    hipEventRecord(m->eb, m->stream);
    if (prof) hipEventRecord(m->ev[3], m->stream);
    HIPCHK(hipMemcpyAsync(idx_out, d_idx, cells * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(dist_out, d_dist, cells * sizeof(int32_t), hipMemcpyDeviceToHost, m->stream));
    if (prof) hipEventRecord(m->ev[4], m->stream);
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    hipEventElapsedTime(&m->last_ms, m->ea, m->eb);
    if (prof) {
        m->stage_ms[2] = m->last_ms;
        if (!kp1_is_device) hipEventElapsedTime(&m->stage_ms[0], m->ev[0], m->ev[1]);
        if (!kp2_is_device) hipEventElapsedTime(&m->stage_ms[1], m->ev[1], m->ev[2]);
        hipEventElapsedTime(&m->stage_ms[3], m->ev[3], m->ev[4]);
    }
    return SIFTMI_OK;
}

// Consensus filter over the pairs of a match (k_consensus.hpp; the contract is DESIGN.md section 7 row 5).  The lists and the
// pairs are used where they lie; host ones are staged in the matcher's own buffers.
int siftmi_match_consensus(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                           const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device,
                           const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device,
                           int32_t n_hyp, float tol, uint32_t seed, uint8_t *mask, float *model, int32_t *winner,
                           int32_t *winner_votes, int32_t *votes_all, float *models_all, double *kernel_ms) {
    if (!m || !winner) return fail(SIFTMI_EINVAL, "null argument");
    if (n1 < 0 || n2 < 0 || n_pairs < 0 || n1 > 0x7fffffff || n2 > 0x7fffffff || n_pairs > 0x7fffffff) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (n_pairs > 0 && (!pairs || !mask)) return fail(SIFTMI_EINVAL, "null pairs or mask with %lld pairs", (long long)n_pairs);
    if (n_hyp < 1 || n_hyp > (1 << 20)) return fail(SIFTMI_EINVAL, "n_hyp %d outside 1..2^20", n_hyp);
    if (!std::isfinite(tol) || !(tol > 0.f)) return fail(SIFTMI_EINVAL, "tol must be finite and > 0");
    HIPCHK(hipSetDevice(m->device));
    *winner = -1;
    if (winner_votes) *winner_votes = 0;
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_pairs < 3) {      // every triple repeats an index: nothing can win, nothing is launched
        if (n_pairs > 0) memset(mask, 0, (size_t)n_pairs);
        if (votes_all) memset(votes_all, 0, sizeof(int32_t) * (size_t)n_hyp);
        if (models_all) for (int64_t i = 0; i < (int64_t)n_hyp * 6; i++) models_all[i] = std::nanf("");
        return SIFTMI_OK;
    }
    if (kp1_is_device || kp2_is_device || pairs_is_device) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2;
    const int2 *dp = (const int2 *)pairs;
    int rc;
    if (!kp1_is_device && n1 > 0 && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (!kp2_is_device && n2 > 0 && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (!pairs_is_device) {
        if ((rc = ensure((void **)&m->pairs, &m->cap_pairs, n_pairs, sizeof(int2)))) return rc;
        HIPCHK(hipMemcpyAsync(m->pairs, pairs, (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, m->stream));
        dp = m->pairs;
    }
    if ((rc = ensure((void **)&m->c_pts, &m->cap_c_pts, n_pairs, sizeof(float4))) ||
        (rc = ensure((void **)&m->c_mask, &m->cap_c_mask, n_pairs, 1)) ||
        (rc = ensure((void **)&m->c_valid, &m->cap_c_valid, n_hyp, 1)) ||
        (rc = ensure((void **)&m->c_models, &m->cap_c_models, (int64_t)n_hyp * 6, sizeof(float))) ||
        (rc = ensure((void **)&m->c_votes, &m->cap_c_votes, n_hyp, sizeof(int)))) return rc;
    if (!m->c_result) HIPCHK(hipMalloc((void **)&m->c_result, sizeof(ConsensusResult)));
    const int M = (int)n_pairs, H = n_hyp;
    const float tol2 = tol * tol;
    const unsigned mblocks = (unsigned)((M + 255) / 256);
    hipLaunchKernelGGL(consensus_gather_kernel, dim3(mblocks), dim3(256), 0, m->stream, d1, (int)n1, d2, (int)n2, dp, M, m->c_pts);
    hipLaunchKernelGGL(consensus_solve_kernel, dim3((unsigned)((H + 255) / 256)), dim3(256), 0, m->stream, (const float4 *)m->c_pts,
                       (uint32_t)M, H, seed, m->c_models, m->c_valid, m->c_votes);
    // vote grid: tiles of matches x chunks of hypotheses, about eight workgroups per CU; a chunk is at most the kernel's LDS counters
    // and at least 16 hypotheses (a workgroup's loads of its matches must be worth its walk)
    const int tiles = (M + SIFT_CONS_TILE - 1) / SIFT_CONS_TILE;
    int chunks = (2048 + tiles - 1) / tiles;
    const int min_chunks = (H + SIFT_CONS_HMAX - 1) / SIFT_CONS_HMAX, max_chunks = (H + 15) / 16;
    if (chunks > max_chunks) chunks = max_chunks;
    if (chunks < min_chunks) chunks = min_chunks;
    const int h_chunk = (H + chunks - 1) / chunks;
    chunks = (H + h_chunk - 1) / h_chunk;
    hipEventRecord(m->ec_a, m->stream);
    hipLaunchKernelGGL(consensus_vote_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(SIFT_CONS_THREADS), 0, m->stream,
                       (const float4 *)m->c_pts, M, (const float *)m->c_models, H, h_chunk, tol2, m->c_votes);
    hipEventRecord(m->ec_b, m->stream);
    hipLaunchKernelGGL(consensus_select_kernel, dim3(1), dim3(256), 0, m->stream, (const int *)m->c_votes, (const uint8_t *)m->c_valid,
                       (const float *)m->c_models, H, m->c_result);
    hipLaunchKernelGGL(consensus_mask_kernel, dim3(mblocks), dim3(256), 0, m->stream, (const float4 *)m->c_pts, M,
                       (const ConsensusResult *)m->c_result, tol2, m->c_mask);
    ConsensusResult res;
    HIPCHK(hipMemcpyAsync(&res, m->c_result, sizeof res, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipMemcpyAsync(mask, m->c_mask, (size_t)M, hipMemcpyDeviceToHost, m->stream));
    if (votes_all) HIPCHK(hipMemcpyAsync(votes_all, m->c_votes, sizeof(int) * (size_t)H, hipMemcpyDeviceToHost, m->stream));
    if (models_all) HIPCHK(hipMemcpyAsync(models_all, m->c_models, sizeof(float) * 6 * (size_t)H, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    if (kernel_ms) { float ms = 0; hipEventElapsedTime(&ms, m->ec_a, m->ec_b); *kernel_ms = ms; }
    *winner = res.winner;
    if (winner_votes) *winner_votes = res.votes;
    if (res.winner >= 0 && model) memcpy(model, res.model, sizeof res.model);
    return SIFTMI_OK;
}

// Least-squares affine map of the pairs of a match (k_fit.hpp; the contract is DESIGN.md section 7 row 9).  The lists, the pairs
// and the mask are used where they lie; host ones are staged in the matcher's own buffers.
int siftmi_match_fit(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                     const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device,
                     const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device,
                     const uint8_t *mask, int32_t mask_is_device, int32_t blocks, double *out, double *kernel_ms) {
    if (!m || !out) return fail(SIFTMI_EINVAL, "null argument");
    if (n1 < 0 || n2 < 0 || n_pairs < 0 || n1 > 0x7fffffff || n2 > 0x7fffffff || n_pairs > 0x7fffffff) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (n_pairs > 0 && !pairs) return fail(SIFTMI_EINVAL, "null pairs with %lld pairs", (long long)n_pairs);
    if (blocks < 0 || blocks > SIFT_FIT_MAX_BLOCKS) return fail(SIFTMI_EINVAL, "blocks %d outside 0..%d", blocks, SIFT_FIT_MAX_BLOCKS);
    HIPCHK(hipSetDevice(m->device));
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_pairs == 0) {     // EMPTY, nothing is launched
        for (int k = 0; k < SIFT_FIT_OUT; k++) out[k] = std::nan("");
        out[SIFT_FIT_STATUS] = 1.0; out[SIFT_FIT_N] = 0.0;
        return SIFTMI_OK;
    }
    if (kp1_is_device || kp2_is_device || pairs_is_device || (mask && mask_is_device)) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2, *dm = mask;
    const int2 *dp = (const int2 *)pairs;
    int rc;
    if (!kp1_is_device && n1 > 0 && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (!kp2_is_device && n2 > 0 && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (!pairs_is_device) {
        if ((rc = ensure((void **)&m->pairs, &m->cap_pairs, n_pairs, sizeof(int2)))) return rc;
        HIPCHK(hipMemcpyAsync(m->pairs, pairs, (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, m->stream));
        dp = m->pairs;
    }
    if (mask && !mask_is_device) {
        if ((rc = ensure((void **)&m->f_mask, &m->cap_f_mask, n_pairs, 1))) return rc;
        HIPCHK(hipMemcpyAsync(m->f_mask, mask, (size_t)n_pairs, hipMemcpyHostToDevice, m->stream));
        dm = m->f_mask;
    }
    if ((rc = ensure((void **)&m->c_pts, &m->cap_c_pts, n_pairs, sizeof(float4)))) return rc;
    if (!m->f_part) HIPCHK(hipMalloc((void **)&m->f_part, sizeof(FitPartials)));
    const int M = (int)n_pairs;
    // the rule: a workgroup per 256 pairs up to 256 workgroups, one per CU; beyond that a lane owns several pairs
    int B = blocks;
    if (B == 0) { B = (M + SIFT_FIT_THREADS - 1) / SIFT_FIT_THREADS; if (B > 256) B = 256; if (B < 1) B = 1; }
    const dim3 grid((unsigned)B), wg(SIFT_FIT_THREADS);
    hipEventRecord(m->ec_a, m->stream);
    hipLaunchKernelGGL(consensus_gather_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, m->stream, d1, (int)n1, d2, (int)n2, dp, M, m->c_pts);
    hipLaunchKernelGGL(fit_pass1_kernel, grid, wg, 0, m->stream, (const float4 *)m->c_pts, dm, M, m->f_part);
    hipLaunchKernelGGL(fit_pass2_kernel, grid, wg, 0, m->stream, (const float4 *)m->c_pts, dm, M, m->f_part);
    hipLaunchKernelGGL(fit_pass3_kernel, grid, wg, 0, m->stream, (const float4 *)m->c_pts, dm, M, m->f_part);
    hipLaunchKernelGGL(fit_finish_kernel, dim3(1), dim3(64), 0, m->stream, m->f_part, B);
    hipEventRecord(m->ec_b, m->stream);
    double res[SIFT_FIT_OUT];
    HIPCHK(hipMemcpyAsync(res, m->f_part->out, sizeof res, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    if (kernel_ms) { float ms = 0; hipEventElapsedTime(&ms, m->ec_a, m->ec_b); *kernel_ms = ms; }
    memcpy(out, res, sizeof res);
    return SIFTMI_OK;
}

namespace {
// every launch of the median select (k_shift.hpp), in stream order: gather, keys + count + first digit, three passes, finish and,
// with `keep`, the mask.  B workgroups for the kernels that walk the pairs; `sc` is cleared first.
void launch_shift(hipStream_t st, int B, const uint8_t *d1, int n1, const uint8_t *d2, int n2, const int2 *dp, int M, const uint8_t *dm,
                  float4 *pts, uint2 *keys, ShiftScratch *sc, float tol, uint8_t *keep) {
    const dim3 grid((unsigned)B), wg(SIFT_SHIFT_THREADS);
    hipMemsetAsync(sc, 0, sizeof(ShiftScratch), st);
    hipLaunchKernelGGL(consensus_gather_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, st, d1, n1, d2, n2, dp, M, pts);
    hipLaunchKernelGGL(shift_key_kernel, grid, wg, 0, st, (const float4 *)pts, dm, M, keys, sc);
    for (int p = 1; p <= 3; p++) hipLaunchKernelGGL(shift_pass_kernel, grid, wg, 0, st, (const uint2 *)keys, M, p, sc);
    hipLaunchKernelGGL(shift_finish_kernel, dim3(1), wg, 0, st, sc);
    if (keep) hipLaunchKernelGGL(shift_keep_kernel, grid, wg, 0, st, (const uint2 *)keys, M, tol, keep, sc);
}
}  // namespace

// Exact median displacement of the pairs of a match (k_shift.hpp; the contract is DESIGN.md section 7 row 11).  The lists, the
// pairs and the mask are used where they lie; host ones are staged in the matcher's own buffers.
int siftmi_match_shift(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                       const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device,
                       const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device,
                       const uint8_t *mask, int32_t mask_is_device, int32_t blocks,
                       float tol, uint8_t *keep, float *out, int64_t *counts, double *kernel_ms) {
    if (!m || !out || !counts) return fail(SIFTMI_EINVAL, "null argument");
    if (n1 < 0 || n2 < 0 || n_pairs < 0 || n1 > 0x7fffffff || n2 > 0x7fffffff || n_pairs > 0x7fffffff) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (n_pairs > 0 && !pairs) return fail(SIFTMI_EINVAL, "null pairs with %lld pairs", (long long)n_pairs);
    if (blocks < 0 || blocks > SIFT_FIT_MAX_BLOCKS) return fail(SIFTMI_EINVAL, "blocks %d outside 0..%d", blocks, SIFT_FIT_MAX_BLOCKS);
    if (keep && !(tol >= 0.f)) return fail(SIFTMI_EINVAL, "tol must be >= 0 (+inf is allowed) with a keep mask");
    HIPCHK(hipSetDevice(m->device));
    if (kernel_ms) *kernel_ms = 0.0;
    if (n_pairs == 0) {     // EMPTY, nothing is launched
        for (int k = 0; k < SIFT_SHIFT_OUT; k++) out[k] = std::nanf("");
        counts[0] = counts[1] = 0;
        return SIFTMI_OK;
    }
    if (kp1_is_device || kp2_is_device || pairs_is_device || (mask && mask_is_device)) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2, *dm = mask;
    const int2 *dp = (const int2 *)pairs;
    int rc;
    if (!kp1_is_device && n1 > 0 && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (!kp2_is_device && n2 > 0 && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (!pairs_is_device) {
        if ((rc = ensure((void **)&m->pairs, &m->cap_pairs, n_pairs, sizeof(int2)))) return rc;
        HIPCHK(hipMemcpyAsync(m->pairs, pairs, (size_t)n_pairs * sizeof(int2), hipMemcpyHostToDevice, m->stream));
        dp = m->pairs;
    }
    if (mask && !mask_is_device) {
        if ((rc = ensure((void **)&m->f_mask, &m->cap_f_mask, n_pairs, 1))) return rc;
        HIPCHK(hipMemcpyAsync(m->f_mask, mask, (size_t)n_pairs, hipMemcpyHostToDevice, m->stream));
        dm = m->f_mask;
    }
    if ((rc = ensure((void **)&m->c_pts, &m->cap_c_pts, n_pairs, sizeof(float4))) ||
        (rc = ensure((void **)&m->s_keys, &m->cap_s_keys, n_pairs, sizeof(uint2)))) return rc;
    if (keep && (rc = ensure((void **)&m->c_mask, &m->cap_c_mask, n_pairs, 1))) return rc;
    if (!m->s_scratch) HIPCHK(hipMalloc((void **)&m->s_scratch, sizeof(ShiftScratch)));
    const int M = (int)n_pairs;
    // fit's rule: a workgroup per 256 pairs up to 256 workgroups, one per CU; beyond that a lane owns several pairs
    int B = blocks;
    if (B == 0) { B = (M + SIFT_SHIFT_THREADS - 1) / SIFT_SHIFT_THREADS; if (B > 256) B = 256; if (B < 1) B = 1; }
    hipEventRecord(m->ec_a, m->stream);
    launch_shift(m->stream, B, d1, (int)n1, d2, (int)n2, dp, M, dm, m->c_pts, m->s_keys, m->s_scratch, tol, keep ? m->c_mask : nullptr);
    hipEventRecord(m->ec_b, m->stream);
    struct { unsigned int n, n_keep; float out[SIFT_SHIFT_OUT]; } res;      // the tail of ShiftScratch
    static_assert(sizeof res == sizeof(ShiftScratch) - offsetof(ShiftScratch, n), "the results are the last members of ShiftScratch");
    HIPCHK(hipMemcpyAsync(&res, &m->s_scratch->n, sizeof res, hipMemcpyDeviceToHost, m->stream));
    if (keep) HIPCHK(hipMemcpyAsync(keep, m->c_mask, (size_t)M, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    if (kernel_ms) { float ms = 0; hipEventElapsedTime(&ms, m->ec_a, m->ec_b); *kernel_ms = ms; }
    memcpy(out, res.out, sizeof res.out);
    counts[0] = res.n; counts[1] = keep ? res.n_keep : 0;
    return SIFTMI_OK;
}

// The matcher over a batch of segment pairs (k_match_batch.hpp; the contract is DESIGN.md section 7 row 12)
namespace {
// one side of the batch: S lists back to back with their counts, or (counts == NULL) ONE list of `shared` records for every segment
struct MbSide { const int64_t *counts; int64_t shared; };
inline int64_t mb_count(const MbSide &s, int k) { return s.counts ? s.counts[k] : s.shared; }
inline int64_t mb_qblocks(int64_t nq) { return (nq + SIFT_MB_QBLOCK - 1) / SIFT_MB_QBLOCK; }

// elements per partition, one length for the whole batch: about 2048 workgroups over all segments together, a whole number of
// tiles, at least four of them (match_direction's rule) and at most SIFT_MATCH_MAX_PART (the 16-bit index)
int mb_part_len(const MbSide &q, const MbSide &l, int S) {
    int64_t work = 0;
    for (int s = 0; s < S; s++) work += mb_qblocks(mb_count(q, s)) * mb_count(l, s);
    int64_t len = (work + 2047) / 2048;
    len = (len + SIFT_MATCH_TILE - 1) / SIFT_MATCH_TILE * SIFT_MATCH_TILE;
    if (len < 4 * SIFT_MATCH_TILE) len = 4 * SIFT_MATCH_TILE;
    if (len > SIFT_MATCH_MAX_PART) len = SIFT_MATCH_MAX_PART;
    return (int)len;
}
// entries of the two tables and partials of one direction
struct MbSizes { int64_t work, blocks, partials; };
MbSizes mb_sizes(const MbSide &q, const MbSide &l, int S, int len) {
    MbSizes z = {0, 0, 0};
    for (int s = 0; s < S; s++) {
        const int64_t nq = mb_count(q, s), np = (mb_count(l, s) + len - 1) / len;
        z.blocks += mb_qblocks(nq); z.work += mb_qblocks(nq) * np; z.partials += np * nq;
    }
    return z;
}
// the tables of one direction, segments in order, a segment's blocks in order; seg_block (may be null): S + 1 first blocks
void mb_fill(const MbSide &q, const MbSide &l, int S, int len, MbWork *work, MbBlock *blocks, int *seg_block) {
    int64_t qoff = 0, loff = 0, pbase = 0, e = 0, w = 0;
    for (int s = 0; s < S; s++) {
        const int64_t nq = mb_count(q, s), nl = mb_count(l, s), np = (nl + len - 1) / len;
        if (seg_block) seg_block[s] = (int)e;
        for (int64_t b0 = 0; b0 < nq; b0 += SIFT_MB_QBLOCK) {
            const int qc = (int)(nq - b0 < SIFT_MB_QBLOCK ? nq - b0 : SIFT_MB_QBLOCK);
            blocks[e++] = {qc, (int)(pbase + b0), (int)nq, (int)np, (int)b0, (int)loff, (int)(qoff + b0), 0};
            for (int64_t p = 0; p < np; p++) {
                const int64_t lf = loff + p * len, le = (p + 1) * len < nl ? lf + len : loff + nl;
                work[w++] = {(int)(qoff + b0), qc, (int)lf, (int)le, (int)(p * len), (int)(pbase + p * nq + b0), 0, 0};
            }
        }
        pbase += np * nq;
        if (q.counts) qoff += nq;
        if (l.counts) loff += nl;
    }
    if (seg_block) seg_block[S] = (int)e;
}
int ensure_pinned(uint8_t **ptr, int64_t *cap, int64_t need) {
    if (need <= *cap && *ptr) return SIFTMI_OK;
    if (*ptr) hipHostFree(*ptr);
    *ptr = nullptr; *cap = 0;
    hipError_t e = hipHostMalloc((void **)ptr, (size_t)(need > 0 ? need : 1), hipHostMallocDefault);
    if (e != hipSuccess) return fail(SIFTMI_ENOMEM, "hipHostMalloc(%lld): %s", (long long)need, hipGetErrorString(e));
    *cap = need;
    return SIFTMI_OK;
}

void launch_mb_partial(hipStream_t st, int n_work, const uint8_t *dq, const uint8_t *dl, const MbWork *work, MatchPartial *partial) {
    hipLaunchKernelGGL(mb_partial_kernel, dim3((unsigned)n_work), dim3(256), 0, st, dq, dl, work, partial);
}
void launch_mb_merge(hipStream_t st, int n_blocks, const MatchPartial *partial, const MbBlock *blocks, float ratio_th, int *dense, int *sums,
                     const int *nearest_in, int *nearest_out) {
    hipLaunchKernelGGL(mb_merge_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, partial, blocks, ratio_th, dense, sums, nearest_in, nearest_out);
}
void launch_mb_scan(hipStream_t st, const int *sums, int n_blocks, int *offs, const int *seg_block, int S, int *seg_off) {
    hipLaunchKernelGGL(mb_scan_kernel, dim3(1), dim3(SIFT_MB_SCAN_THREADS), 0, st, sums, n_blocks, offs, seg_block, S, seg_off);
}
void launch_mb_scatter(hipStream_t st, int n_blocks, const int *dense, const int *offs, const MbBlock *blocks, int2 *pairs) {
    hipLaunchKernelGGL(mb_scatter_kernel, dim3((unsigned)n_blocks), dim3(256), 0, st, dense, offs, blocks, pairs);
}
}  // namespace

int siftmi_match_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                       const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                       const int64_t *counts1, const int64_t *counts2, float ratio_th, int32_t mutual, int32_t part_len,
                       int32_t *pairs, int32_t pairs_is_device, int64_t *pair_counts) {
    if (!m) return fail(SIFTMI_EINVAL, "null argument");
    if (n_segments < 0 || n_segments > SIFT_MB_MAX_SEGMENTS) return fail(SIFTMI_EINVAL, "n_segments %d outside 0..%d", n_segments, SIFT_MB_MAX_SEGMENTS);
    if (n1 < 0 || n2 < 0 || n1 > 0x7fffffff || n2 > 0x7fffffff) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (n_segments > 0 && (!counts2 || !pair_counts)) return fail(SIFTMI_EINVAL, "null counts2 or pair_counts with %d segments", n_segments);
    if (!(ratio_th <= 1.0f)) return fail(SIFTMI_EINVAL, "ratio_th must be <= 1, not %g", ratio_th);
    if (part_len < 0 || part_len > SIFT_MATCH_MAX_PART || part_len % SIFT_MATCH_TILE)
        return fail(SIFTMI_EINVAL, "part_len must be 0 or a multiple of %d up to %d, not %d", SIFT_MATCH_TILE, SIFT_MATCH_MAX_PART, part_len);
    const int S = n_segments;
    int64_t sum1 = 0, sum2 = 0;
    for (int s = 0; s < S; s++) {
        if (counts2[s] < 0 || (counts1 && counts1[s] < 0)) return fail(SIFTMI_EINVAL, "negative count in segment %d", s);
        if (counts2[s] > n2 || (counts1 && counts1[s] > n1)) return fail(SIFTMI_EINVAL, "the count of segment %d exceeds its list", s);
        sum2 += counts2[s]; sum1 += counts1 ? counts1[s] : 0;
    }
    if (sum2 != n2) return fail(SIFTMI_EINVAL, "counts2 add up to %lld, the second list has %lld records", (long long)sum2, (long long)n2);
    if (counts1 && sum1 != n1) return fail(SIFTMI_EINVAL, "counts1 add up to %lld, the first list has %lld records", (long long)sum1, (long long)n1);
    const int64_t NQ = counts1 ? n1 : (int64_t)S * n1;         // queries of the concatenated first side: the capacity of `pairs`
    if (NQ > 0x7fffffff) return fail(SIFTMI_EINVAL, "%lld queries in all: more than 2^31 - 1", (long long)NQ);
    HIPCHK(hipSetDevice(m->device));
    for (float &v : m->stage_ms) v = -1.f;
    m->last_ms = 0;
    for (int s = 0; s < S; s++) pair_counts[s] = 0;
    const MbSide side1 = {counts1, n1}, side2 = {counts2, n2};
    const int len_f = part_len ? part_len : mb_part_len(side1, side2, S);
    const MbSizes zf = mb_sizes(side1, side2, S, len_f);
    if (zf.work == 0) return SIFTMI_OK;                        // no segment with an element on both sides: no pair, nothing is launched
    if (!pairs) return fail(SIFTMI_EINVAL, "null pairs buffer");
    const int len_r = !mutual ? 0 : part_len ? part_len : mb_part_len(side2, side1, S);
    const MbSizes zr = mutual ? mb_sizes(side2, side1, S, len_r) : MbSizes{0, 0, 0};
    const int64_t max_work = (int64_t)1 << 22;
    if (zf.work > max_work || zr.work > max_work || zf.blocks * SIFT_MB_QBLOCK > 0x7fffffff || zf.partials > 0x7fffffff || zr.partials > 0x7fffffff)
        return fail(SIFTMI_EINVAL, "the batch is too large: %lld + %lld workgroups, %lld + %lld partial results",
                    (long long)zf.work, (long long)zr.work, (long long)zf.partials, (long long)zr.partials);
    // the tables, one upload: scan entries forward / reverse, blocks forward / reverse, the segments' first blocks
    const int64_t o_wf = 0, o_wr = o_wf + zf.work * (int64_t)sizeof(MbWork), o_bf = o_wr + zr.work * (int64_t)sizeof(MbWork),
                  o_br = o_bf + zf.blocks * (int64_t)sizeof(MbBlock), o_sb = o_br + zr.blocks * (int64_t)sizeof(MbBlock),
                  tab_bytes = o_sb + (S + 1) * (int64_t)sizeof(int);
    const int Ef = (int)zf.blocks;
    const int64_t i_sums = 0, i_offs = i_sums + Ef, i_seg = i_offs + Ef + 1, i_dense = (i_seg + S + 1 + 1) / 2 * 2, n_ints = i_dense + (int64_t)Ef * SIFT_MB_QBLOCK;
    int rc;
    if ((rc = ensure_pinned(&m->mb_host, &m->cap_mb_host, tab_bytes + (S + 1) * (int64_t)sizeof(int))) ||
        (rc = ensure((void **)&m->mb_tab, &m->cap_mb_tab, tab_bytes, 1)) ||
        (rc = ensure((void **)&m->mb_ints, &m->cap_mb_ints, n_ints, sizeof(int))) ||
        (rc = ensure((void **)&m->partial, &m->cap_partial, zf.partials > zr.partials ? zf.partials : zr.partials, sizeof(MatchPartial)))) return rc;
    if (mutual && (rc = ensure((void **)&m->nearest, &m->cap_nearest, n2, sizeof(int)))) return rc;
    if (!pairs_is_device && (rc = ensure((void **)&m->pairs, &m->cap_pairs, NQ, sizeof(int2)))) return rc;
    mb_fill(side1, side2, S, len_f, (MbWork *)(m->mb_host + o_wf), (MbBlock *)(m->mb_host + o_bf), (int *)(m->mb_host + o_sb));
    if (mutual) mb_fill(side2, side1, S, len_r, (MbWork *)(m->mb_host + o_wr), (MbBlock *)(m->mb_host + o_br), nullptr);
    int *seg_off_host = (int *)(m->mb_host + tab_bytes);
    if (kp1_is_device || kp2_is_device || pairs_is_device) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2;
    const bool prof = m->profile && m->ev[0];
    if (prof) hipEventRecord(m->ev[0], m->stream);
    if (!kp1_is_device && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (prof) hipEventRecord(m->ev[1], m->stream);
    if (!kp2_is_device && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (prof) hipEventRecord(m->ev[2], m->stream);
    HIPCHK(hipMemcpyAsync(m->mb_tab, m->mb_host, (size_t)tab_bytes, hipMemcpyHostToDevice, m->stream));
    int *sums = m->mb_ints + i_sums, *offs = m->mb_ints + i_offs, *seg_off = m->mb_ints + i_seg, *dense = m->mb_ints + i_dense;
    const MbBlock *blocks_f = (const MbBlock *)(m->mb_tab + o_bf);
    int2 *result = pairs_is_device ? (int2 *)pairs : m->pairs;
    hipEventRecord(m->ea, m->stream);
    if (mutual) {
        // reverse scan: the nearest element of its segment's first list for every record of the second side
        launch_mb_partial(m->stream, (int)zr.work, d2, d1, (const MbWork *)(m->mb_tab + o_wr), m->partial);
        launch_mb_merge(m->stream, (int)zr.blocks, m->partial, (const MbBlock *)(m->mb_tab + o_br), ratio_th, nullptr, nullptr, nullptr, m->nearest);
    }
    launch_mb_partial(m->stream, (int)zf.work, d1, d2, (const MbWork *)(m->mb_tab + o_wf), m->partial);
    launch_mb_merge(m->stream, Ef, m->partial, blocks_f, ratio_th, dense, sums, mutual ? m->nearest : nullptr, nullptr);
    launch_mb_scan(m->stream, sums, Ef, offs, (const int *)(m->mb_tab + o_sb), S, seg_off);
    launch_mb_scatter(m->stream, Ef, dense, offs, blocks_f, result);
    hipEventRecord(m->eb, m->stream);
    HIPCHK(hipMemcpyAsync(seg_off_host, seg_off, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    if (!pairs_is_device) {
        // the number of pairs is not known before the one wait: every row a query could have filled comes back
        if (prof) hipEventRecord(m->ev[3], m->stream);
        HIPCHK(hipMemcpyAsync(pairs, m->pairs, (size_t)NQ * sizeof(int2), hipMemcpyDeviceToHost, m->stream));
        if (prof) hipEventRecord(m->ev[4], m->stream);
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    hipEventElapsedTime(&m->last_ms, m->ea, m->eb);
    if (prof) {
        m->stage_ms[2] = m->last_ms;
        if (!kp1_is_device) hipEventElapsedTime(&m->stage_ms[0], m->ev[0], m->ev[1]);
        if (!kp2_is_device) hipEventElapsedTime(&m->stage_ms[1], m->ev[1], m->ev[2]);
        if (!pairs_is_device) hipEventElapsedTime(&m->stage_ms[3], m->ev[3], m->ev[4]);
    }
    for (int s = 0; s < S; s++) pair_counts[s] = seg_off_host[s + 1] - seg_off_host[s];
    return SIFTMI_OK;
}

// The windowed matcher over a batch of segment pairs (k_match_window_batch.hpp; the contract is DESIGN.md section 7 row 16)
namespace {
// cells per axis of a list of n records at most: the largest g <= grid_max with g * g <= max(1, n)
int mwb_gcap(int64_t n, int grid_max) {
    int g = (int)std::sqrt((double)(n > 1 ? n : 1));
    while ((int64_t)g * g > n && g > 1) g--;
    while ((int64_t)(g + 1) * (g + 1) <= n) g++;
    return g < 1 ? 1 : g > grid_max ? grid_max : g;
}
// what one direction needs: rows are S + 1; cells: words of each of the four cell arrays; order / dense: entries of the queries'
// order and records of the dense copy; work: the bound on the work items; lblocks / qblocks: entries of the two block tables
struct MwbSizes { int64_t cells, order, dense, work, lblocks, qblocks; int live; };
// The tables of one direction (null pointers: the sizes only).  A segment with an empty side is dead: no block, no cell, no work.
// With a shared list (l.counts == NULL) row S bins it once; its grid is capped by the mean number of queries of a live segment as
// well, so that the S query-side copies of its cells stay within the records of the batch.
MwbSizes mwb_fill(const MbSide &q, const MbSide &l, int S, int grid_max, const float *shifts, const int *seg_block, MwbSeg *rows,
                  int2 *lblocks, int2 *qblocks) {
    MwbSizes z = {0, 0, 0, 0, 0, 0, 0};
    int64_t nq_live = 0;
    for (int s = 0; s < S; s++) if (mb_count(q, s) > 0 && mb_count(l, s) > 0) { z.live++; nq_live += mb_count(q, s); }
    const bool shared = !l.counts;
    int g_shared = 1;
    if (rows) std::memset(rows, 0, (size_t)(S + 1) * sizeof(MwbSeg));
    if (shared && z.live) {
        const int64_t mean = nq_live / z.live > 1 ? nq_live / z.live : 1;
        g_shared = mwb_gcap(l.shared < mean ? l.shared : mean, grid_max);
        if (rows) { MwbSeg &r = rows[S]; r.l_count = (int)l.shared; r.ext = S; r.g_cap = g_shared; r.own_list = 1; }
        for (int64_t c = 0; c * 256 < l.shared; c++, z.lblocks++) if (lblocks) lblocks[z.lblocks] = make_int2(S, (int)c);
        z.cells += (int64_t)g_shared * g_shared + 1;
        z.dense = l.shared;
    }
    int64_t qoff = 0, loff = 0;
    for (int s = 0; s < S; s++) {
        const int64_t nq = mb_count(q, s), nl = mb_count(l, s);
        if (rows) { rows[s].ext = s; rows[s].g_cap = 1; }
        if (nq > 0 && nl > 0) {
            const int g = shared ? g_shared : mwb_gcap(nl, grid_max);
            const int64_t cells = (int64_t)g * g;
            if (rows) {
                MwbSeg &r = rows[s];
                r.q_first = (int)qoff; r.q_count = (int)nq; r.l_first = shared ? 0 : (int)loff; r.l_count = (int)nl;
                r.q_cells = (int)z.cells; r.l_cells = shared ? 0 : (int)z.cells;
                r.ext = shared ? S : s; r.g_cap = g; r.order = (int)z.order; r.dense = shared ? 0 : (int)z.dense;
                r.out = seg_block ? seg_block[s] * SIFT_MB_QBLOCK : 0; r.own_list = !shared;
                r.sx = shifts[2 * s]; r.sy = shifts[2 * s + 1];
            }
            for (int64_t c = 0; c * 256 < nq; c++, z.qblocks++) if (qblocks) qblocks[z.qblocks] = make_int2(s, (int)c);
            if (!shared) {
                for (int64_t c = 0; c * 256 < nl; c++, z.lblocks++) if (lblocks) lblocks[z.lblocks] = make_int2(s, (int)c);
                z.dense += nl;
            }
            z.cells += cells + 1;
            z.order += nq;
            z.work += nq / SIFT_MW_QB + (nq < cells ? nq : cells) + 1;     // mw_work_cap's bound with the segment's cells
        }
        if (q.counts) qoff += nq;
        if (l.counts) loff += nl;
    }
    return z;
}
// the blocks of the compaction: mb_fill's for the first side, `stride` the length of the segment's second list and `nparts` whether
// the segment has work
void mwb_fill_blocks(const MbSide &q, const MbSide &l, int S, MbBlock *blocks, int *seg_block) {
    int64_t qoff = 0, loff = 0, e = 0;
    for (int s = 0; s < S; s++) {
        const int64_t nq = mb_count(q, s), nl = mb_count(l, s);
        seg_block[s] = (int)e;
        for (int64_t b0 = 0; b0 < nq; b0 += SIFT_MB_QBLOCK) {
            const int qc = (int)(nq - b0 < SIFT_MB_QBLOCK ? nq - b0 : SIFT_MB_QBLOCK);
            blocks[e++] = {qc, 0, (int)nl, nl > 0 ? 1 : 0, (int)b0, (int)loff, (int)(qoff + b0), 0};
        }
        if (q.counts) qoff += nq;
        if (l.counts) loff += nl;
    }
    seg_block[S] = (int)e;
}
// the integer scratch of one direction inside w_cells: [ext_max | cnt_l | cnt_q] are zeroed together, ext_min starts at 0xff..
struct MwbInts { int64_t ext_max, cnt_l, cnt_q, ext_min, start_l, start_q, n_work, w_off, spare, total; };
MwbInts mwb_ints(int S, int64_t cells) {
    MwbInts o;
    const int64_t R = S + 1;
    o.ext_max = 0; o.cnt_l = 2 * R; o.cnt_q = o.cnt_l + cells; o.ext_min = o.cnt_q + cells; o.start_l = o.ext_min + 2 * R;
    o.start_q = o.start_l + cells; o.n_work = o.start_q + cells; o.w_off = o.n_work + R; o.spare = o.w_off + R + 1; o.total = o.spare + 1;
    return o;
}
// one direction: the grids of all rows, the compacted work list and the scan.  nearest == null: dense gets `best` or -1 per query
int mwb_direction(siftmi_matcher *m, int S, const MwbSizes &z, const MwbSeg *rows, const int2 *lblocks, const int2 *qblocks, const int *zero,
                  const uint8_t *dq, const uint8_t *dl, int reverse, float wx, float wy, float ratio_th, int *dense, int *nearest) {
    const MwbInts o = mwb_ints(S, z.cells);
    int *w = m->w_cells;
    uint32_t *ext_min = (uint32_t *)(w + o.ext_min), *ext_max = (uint32_t *)(w + o.ext_max);
    hipStream_t st = m->stream;
    HIPCHK(hipMemsetAsync(w + o.ext_max, 0, (size_t)(o.ext_min - o.ext_max) * sizeof(int), st));
    HIPCHK(hipMemsetAsync(w + o.ext_min, 0xff, (size_t)(2 * (S + 1)) * sizeof(int), st));
    const dim3 bl((unsigned)z.lblocks), bq((unsigned)z.qblocks), th(256);
    hipLaunchKernelGGL(mwb_extent_kernel, bl, th, 0, st, dl, rows, lblocks, ext_min, ext_max);
    hipLaunchKernelGGL(mwb_count_kernel, bl, th, 0, st, dl, rows, lblocks, 1, reverse, (const uint32_t *)ext_min, (const uint32_t *)ext_max, wx, wy, w + o.cnt_l);
    hipLaunchKernelGGL(mwb_count_kernel, bq, th, 0, st, dq, rows, qblocks, 0, reverse, (const uint32_t *)ext_min, (const uint32_t *)ext_max, wx, wy, w + o.cnt_q);
    hipLaunchKernelGGL(mwb_scan_kernel, dim3((unsigned)(S + 1)), dim3(SIFT_MWB_SCAN_THREADS), 0, st, rows, (const uint32_t *)ext_min,
                       (const uint32_t *)ext_max, wx, wy, w + o.cnt_l, w + o.cnt_q, w + o.start_l, w + o.start_q, w + o.n_work);
    // w_off[s] = work items of the rows before s; w_off[S]: all of them (`zero` is a table word that holds 0: no segment values)
    launch_mb_scan(st, w + o.n_work, S, w + o.w_off, zero, 0, w + o.spare);
    hipLaunchKernelGGL(mwb_work_kernel, dim3((unsigned)S), dim3(SIFT_MWB_SCAN_THREADS), 0, st, rows, (const uint32_t *)ext_min,
                       (const uint32_t *)ext_max, wx, wy, (const int *)(w + o.start_q), (const int *)(w + o.w_off), m->w_work, (int)z.work);
    hipLaunchKernelGGL(mwb_scatter_list_kernel, bl, th, 0, st, dl, rows, lblocks, (const uint32_t *)ext_min, (const uint32_t *)ext_max, wx, wy,
                       w + o.cnt_l, m->w_desc, m->w_meta);
    hipLaunchKernelGGL(mwb_scatter_query_kernel, bq, th, 0, st, dq, rows, qblocks, reverse, (const uint32_t *)ext_min, (const uint32_t *)ext_max,
                       wx, wy, w + o.cnt_q, m->w_order);
    hipLaunchKernelGGL(mwb_match_kernel, dim3((unsigned)z.work), th, 0, st, dq, rows, (const uint32_t *)ext_min, (const uint32_t *)ext_max, wx, wy,
                       reverse, (const int *)(w + o.start_l), (const int *)(w + o.start_q), (const int *)m->w_order, (const int2 *)m->w_work,
                       (const int *)(w + o.w_off + S), (const uint4 *)m->w_desc, (const float4 *)m->w_meta, ratio_th, dense, nearest);
    return SIFTMI_OK;
}
}  // namespace

int siftmi_match_window_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                              const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                              const int64_t *counts1, const int64_t *counts2, float ratio_th, float wx, float wy, const float *shifts,
                              int32_t mutual, int32_t grid_max, int32_t *pairs, int32_t pairs_is_device, int64_t *pair_counts) {
    if (!m) return fail(SIFTMI_EINVAL, "null argument");
    if (n_segments < 0 || n_segments > SIFT_MB_MAX_SEGMENTS) return fail(SIFTMI_EINVAL, "n_segments %d outside 0..%d", n_segments, SIFT_MB_MAX_SEGMENTS);
    if (n1 < 0 || n2 < 0 || n1 > 0x7fffffff / 8 || n2 > 0x7fffffff / 8) return fail(SIFTMI_EINVAL, "bad list size");
    if ((n1 > 0 && !kp1) || (n2 > 0 && !kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (n_segments > 0 && (!counts2 || !pair_counts || !shifts)) return fail(SIFTMI_EINVAL, "null counts2, shifts or pair_counts with %d segments", n_segments);
    if (!(ratio_th <= 1.0f)) return fail(SIFTMI_EINVAL, "ratio_th must be <= 1, not %g", ratio_th);
    if (!(wx >= 0.f) || !(wy >= 0.f)) return fail(SIFTMI_EINVAL, "the window must be >= 0 (it may be infinite), not (%g, %g)", wx, wy);
    if (grid_max < 0 || grid_max > SIFT_MW_MAXG) return fail(SIFTMI_EINVAL, "grid_max must be 0 .. %d, not %d", SIFT_MW_MAXG, grid_max);
    const int S = n_segments;
    int64_t sum1 = 0, sum2 = 0;
    for (int s = 0; s < S; s++) {
        if (counts2[s] < 0 || (counts1 && counts1[s] < 0)) return fail(SIFTMI_EINVAL, "negative count in segment %d", s);
        if (counts2[s] > n2 || (counts1 && counts1[s] > n1)) return fail(SIFTMI_EINVAL, "the count of segment %d exceeds its list", s);
        if (!std::isfinite(shifts[2 * s]) || !std::isfinite(shifts[2 * s + 1]))
            return fail(SIFTMI_EINVAL, "the window shift of segment %d must be finite, not (%g, %g)", s, shifts[2 * s], shifts[2 * s + 1]);
        sum2 += counts2[s]; sum1 += counts1 ? counts1[s] : 0;
    }
    if (sum2 != n2) return fail(SIFTMI_EINVAL, "counts2 add up to %lld, the second list has %lld records", (long long)sum2, (long long)n2);
    if (counts1 && sum1 != n1) return fail(SIFTMI_EINVAL, "counts1 add up to %lld, the first list has %lld records", (long long)sum1, (long long)n1);
    const int64_t NQ = counts1 ? n1 : (int64_t)S * n1;         // queries of the concatenated first side: the capacity of `pairs`
    if (NQ > 0x7fffffff / 8) return fail(SIFTMI_EINVAL, "%lld queries in all: more than 2^28 - 1", (long long)NQ);
    HIPCHK(hipSetDevice(m->device));
    for (float &v : m->stage_ms) v = -1.f;
    m->last_ms = 0;
    for (int s = 0; s < S; s++) pair_counts[s] = 0;
    const MbSide side1 = {counts1, n1}, side2 = {counts2, n2};
    const int G = grid_max ? grid_max : SIFT_MW_MAXG;
    const MwbSizes zf = mwb_fill(side1, side2, S, G, shifts, nullptr, nullptr, nullptr, nullptr);
    if (zf.live == 0) return SIFTMI_OK;                        // no segment with an element on both sides: no pair, nothing is launched
    if (!pairs) return fail(SIFTMI_EINVAL, "null pairs buffer");
    const MwbSizes zr = mutual ? mwb_fill(side2, side1, S, G, shifts, nullptr, nullptr, nullptr, nullptr) : MwbSizes{0, 0, 0, 0, 0, 0, 0};
    int64_t Ef64 = 0;
    for (int s = 0; s < S; s++) Ef64 += mb_qblocks(mb_count(side1, s));
    const int64_t lim = (int64_t)1 << 30;
    if (zf.work > lim || zr.work > lim || zf.cells > lim / 4 || zr.cells > lim / 4 || Ef64 * SIFT_MB_QBLOCK > 0x7fffffff)
        return fail(SIFTMI_EINVAL, "the batch is too large: %lld + %lld work items, %lld + %lld cells", (long long)zf.work, (long long)zr.work,
                    (long long)zf.cells, (long long)zr.cells);
    const int Ef = (int)Ef64;
    // the tables, one upload: rows forward / reverse, the blocks of the compaction, the block tables, the segments' first blocks
    const int64_t R = S + 1;
    const int64_t o_rf = 0, o_rr = o_rf + R * (int64_t)sizeof(MwbSeg), o_bf = o_rr + (mutual ? R : 0) * (int64_t)sizeof(MwbSeg),
                  o_lf = o_bf + Ef * (int64_t)sizeof(MbBlock), o_qf = o_lf + zf.lblocks * (int64_t)sizeof(int2),
                  o_lr = o_qf + zf.qblocks * (int64_t)sizeof(int2), o_qr = o_lr + zr.lblocks * (int64_t)sizeof(int2),
                  o_sb = o_qr + zr.qblocks * (int64_t)sizeof(int2), o_zero = o_sb + R * (int64_t)sizeof(int),
                  tab_bytes = o_zero + (int64_t)sizeof(int);
    const int64_t i_sums = 0, i_offs = i_sums + Ef, i_seg = i_offs + Ef + 1, i_dense = (i_seg + S + 1 + 1) / 2 * 2, n_ints = i_dense + (int64_t)Ef * SIFT_MB_QBLOCK;
    const int64_t w_ints = std::max(mwb_ints(S, zf.cells).total, mwb_ints(S, zr.cells).total);
    const int64_t n_work = std::max(zf.work, zr.work), n_dense = std::max(zf.dense, zr.dense), n_order = std::max(zf.order, zr.order);
    int rc;
    if ((rc = ensure_pinned(&m->mb_host, &m->cap_mb_host, tab_bytes + R * (int64_t)sizeof(int))) ||
        (rc = ensure((void **)&m->mb_tab, &m->cap_mb_tab, tab_bytes, 1)) ||
        (rc = ensure((void **)&m->mb_ints, &m->cap_mb_ints, n_ints, sizeof(int))) ||
        (rc = ensure((void **)&m->w_cells, &m->cap_w_cells, w_ints, sizeof(int))) ||
        (rc = ensure((void **)&m->w_work, &m->cap_w_work, n_work, sizeof(int2))) ||
        (rc = ensure((void **)&m->w_desc, &m->cap_w_desc, n_dense * 8, sizeof(uint4))) ||
        (rc = ensure((void **)&m->w_meta, &m->cap_w_meta, n_dense, sizeof(float4))) ||
        (rc = ensure((void **)&m->w_order, &m->cap_w_order, n_order, sizeof(int)))) return rc;
    if (mutual && (rc = ensure((void **)&m->nearest, &m->cap_nearest, n2, sizeof(int)))) return rc;
    if (!pairs_is_device && (rc = ensure((void **)&m->pairs, &m->cap_pairs, NQ, sizeof(int2)))) return rc;
    int *seg_block = (int *)(m->mb_host + o_sb);
    mwb_fill_blocks(side1, side2, S, (MbBlock *)(m->mb_host + o_bf), seg_block);
    *(int *)(m->mb_host + o_zero) = 0;
    mwb_fill(side1, side2, S, G, shifts, seg_block, (MwbSeg *)(m->mb_host + o_rf), (int2 *)(m->mb_host + o_lf), (int2 *)(m->mb_host + o_qf));
    if (mutual) mwb_fill(side2, side1, S, G, shifts, nullptr, (MwbSeg *)(m->mb_host + o_rr), (int2 *)(m->mb_host + o_lr), (int2 *)(m->mb_host + o_qr));
    int *seg_off_host = (int *)(m->mb_host + tab_bytes);
    if (kp1_is_device || kp2_is_device || pairs_is_device) HIPCHK(hipDeviceSynchronize());
    const uint8_t *d1 = (const uint8_t *)kp1, *d2 = (const uint8_t *)kp2;
    const bool prof = m->profile && m->ev[0];
    if (prof) hipEventRecord(m->ev[0], m->stream);
    if (!kp1_is_device && (rc = stage_list(m, &m->kp1, &m->cap1, kp1, n1, &d1))) return rc;
    if (prof) hipEventRecord(m->ev[1], m->stream);
    if (!kp2_is_device && (rc = stage_list(m, &m->kp2, &m->cap2, kp2, n2, &d2))) return rc;
    if (prof) hipEventRecord(m->ev[2], m->stream);
    HIPCHK(hipMemcpyAsync(m->mb_tab, m->mb_host, (size_t)tab_bytes, hipMemcpyHostToDevice, m->stream));
    int *sums = m->mb_ints + i_sums, *offs = m->mb_ints + i_offs, *seg_off = m->mb_ints + i_seg, *dense = m->mb_ints + i_dense;
    const MbBlock *blocks_f = (const MbBlock *)(m->mb_tab + o_bf);
    const int *zero = (const int *)(m->mb_tab + o_zero);
    int2 *result = pairs_is_device ? (int2 *)pairs : m->pairs;
    hipEventRecord(m->ea, m->stream);
    // reverse scan: the nearest candidate among its segment's first list for every record of the second side (the shifts negated)
    if (mutual && (rc = mwb_direction(m, S, zr, (const MwbSeg *)(m->mb_tab + o_rr), (const int2 *)(m->mb_tab + o_lr), (const int2 *)(m->mb_tab + o_qr),
                                      zero, d2, d1, 1, wx, wy, ratio_th, nullptr, m->nearest))) return rc;
    if ((rc = mwb_direction(m, S, zf, (const MwbSeg *)(m->mb_tab + o_rf), (const int2 *)(m->mb_tab + o_lf), (const int2 *)(m->mb_tab + o_qf),
                            zero, d1, d2, 0, wx, wy, ratio_th, dense, nullptr))) return rc;
    hipLaunchKernelGGL(mwb_finish_kernel, dim3((unsigned)Ef), dim3(256), 0, m->stream, blocks_f, dense, sums, mutual ? (const int *)m->nearest : (const int *)nullptr);
    launch_mb_scan(m->stream, sums, Ef, offs, (const int *)(m->mb_tab + o_sb), S, seg_off);
    launch_mb_scatter(m->stream, Ef, dense, offs, blocks_f, result);
    hipEventRecord(m->eb, m->stream);
    HIPCHK(hipMemcpyAsync(seg_off_host, seg_off, (size_t)(S + 1) * sizeof(int), hipMemcpyDeviceToHost, m->stream));
    if (!pairs_is_device) {
        // the number of pairs is not known before the one wait: every row a query could have filled comes back
        if (prof) hipEventRecord(m->ev[3], m->stream);
        HIPCHK(hipMemcpyAsync(pairs, m->pairs, (size_t)NQ * sizeof(int2), hipMemcpyDeviceToHost, m->stream));
        if (prof) hipEventRecord(m->ev[4], m->stream);
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    hipEventElapsedTime(&m->last_ms, m->ea, m->eb);
    if (prof) {
        m->stage_ms[2] = m->last_ms;
        if (!kp1_is_device) hipEventElapsedTime(&m->stage_ms[0], m->ev[0], m->ev[1]);
        if (!kp2_is_device) hipEventElapsedTime(&m->stage_ms[1], m->ev[1], m->ev[2]);
        if (!pairs_is_device) hipEventElapsedTime(&m->stage_ms[3], m->ev[3], m->ev[4]);
    }
    for (int s = 0; s < S; s++) pair_counts[s] = seg_off_host[s + 1] - seg_off_host[s];
    return SIFTMI_OK;
}

// The fit and the median of every segment of a batch at once (k_estimate_batch.hpp; the contract is DESIGN.md section 7 row 13)
namespace {
struct EbBatch {
    const siftmi_keypoint *kp1; int64_t n1; int32_t dev1;
    const siftmi_keypoint *kp2; int64_t n2; int32_t dev2;
    int S;
    const int64_t *counts1, *counts2;
    const int32_t *pairs; int64_t n_pairs; int32_t devp;
    const int64_t *pair_counts;
    const uint8_t *mask; int32_t devm;
};
// everything that is wrong with the arguments both entries share; nothing touches the device
int eb_validate(const siftmi_matcher *m, const EbBatch &a) {
    if (!m) return fail(SIFTMI_EINVAL, "null argument");
    if (a.S < 0 || a.S > SIFT_EB_MAX_SEGMENTS) return fail(SIFTMI_EINVAL, "n_segments %d outside 0..%d", a.S, SIFT_EB_MAX_SEGMENTS);
    if (a.n1 < 0 || a.n2 < 0 || a.n_pairs < 0 || a.n1 > 0x7fffffff || a.n2 > 0x7fffffff || a.n_pairs > 0x7fffffff) return fail(SIFTMI_EINVAL, "bad list size");
    if ((a.n1 > 0 && !a.kp1) || (a.n2 > 0 && !a.kp2)) return fail(SIFTMI_EINVAL, "null keypoint list");
    if (a.n_pairs > 0 && !a.pairs) return fail(SIFTMI_EINVAL, "null pairs with %lld pairs", (long long)a.n_pairs);
    if (a.S > 0 && (!a.counts2 || !a.pair_counts)) return fail(SIFTMI_EINVAL, "null counts2 or pair_counts with %d segments", a.S);
    int64_t sum1 = 0, sum2 = 0, sump = 0;
    for (int s = 0; s < a.S; s++) {
        if (a.counts2[s] < 0 || (a.counts1 && a.counts1[s] < 0) || a.pair_counts[s] < 0) return fail(SIFTMI_EINVAL, "negative count in segment %d", s);
        if (a.counts2[s] > a.n2 || (a.counts1 && a.counts1[s] > a.n1) || a.pair_counts[s] > a.n_pairs)
            return fail(SIFTMI_EINVAL, "a count of segment %d exceeds its list", s);
        sum2 += a.counts2[s]; sum1 += a.counts1 ? a.counts1[s] : 0; sump += a.pair_counts[s];
    }
    if (sum2 != a.n2) return fail(SIFTMI_EINVAL, "counts2 add up to %lld, the second list has %lld records", (long long)sum2, (long long)a.n2);
    if (a.counts1 && sum1 != a.n1) return fail(SIFTMI_EINVAL, "counts1 add up to %lld, the first list has %lld records", (long long)sum1, (long long)a.n1);
    if (sump != a.n_pairs) return fail(SIFTMI_EINVAL, "pair_counts add up to %lld, there are %lld pairs", (long long)sump, (long long)a.n_pairs);
    return SIFTMI_OK;
}
// fit's rule for one segment's workgroups; 0 for a segment without a pair
inline int eb_blocks(int64_t rows, int blocks) {
    if (rows == 0) return 0;
    if (blocks) return blocks;
    const int64_t B = (rows + SIFT_FIT_THREADS - 1) / SIFT_FIT_THREADS;
    return (int)(B > 256 ? 256 : B);
}
// The tables, segments in order: `segs` gets entry b = 0 of every segment (all of them, or with `nonempty` only those with a pair),
// `work` (may be null) the B_s entries of every segment.  Returns the entries written to `segs`.
int eb_fill(const EbBatch &a, int blocks, bool nonempty, EbWork *segs, EbWork *work) {
    int64_t off1 = 0, off2 = 0, row0 = 0, slot0 = 0, e = 0, w = 0;
    for (int s = 0; s < a.S; s++) {
        const int64_t rows = a.pair_counts[s], n1 = a.counts1 ? a.counts1[s] : a.n1, n2 = a.counts2[s];
        const int B = eb_blocks(rows, blocks);
        const EbWork head = {s, 0, B, (int)row0, (int)rows, (int)off1, (int)n1, (int)off2, (int)n2, (int)slot0};
        if (B || !nonempty) segs[e++] = head;
        if (work) for (int b = 0; b < B; b++) { work[w] = head; work[w++].b = b; }
        row0 += rows; slot0 += B; off2 += n2;
        if (a.counts1) off1 += n1;
    }
    return (int)e;
}
// the device synchronisation of the header's convention and the staging of host inputs, as in siftmi_match_fit
int eb_stage(siftmi_matcher *m, const EbBatch &a, const uint8_t **d1, const uint8_t **d2, const int2 **dp, const uint8_t **dm) {
    if (a.dev1 || a.dev2 || a.devp || (a.mask && a.devm)) HIPCHK(hipDeviceSynchronize());
    *d1 = (const uint8_t *)a.kp1; *d2 = (const uint8_t *)a.kp2; *dp = (const int2 *)a.pairs; *dm = a.mask;
    int rc;
    if (!a.dev1 && a.n1 > 0 && (rc = stage_list(m, &m->kp1, &m->cap1, a.kp1, a.n1, d1))) return rc;
    if (!a.dev2 && a.n2 > 0 && (rc = stage_list(m, &m->kp2, &m->cap2, a.kp2, a.n2, d2))) return rc;
    if (!a.devp) {
        if ((rc = ensure((void **)&m->pairs, &m->cap_pairs, a.n_pairs, sizeof(int2)))) return rc;
        HIPCHK(hipMemcpyAsync(m->pairs, a.pairs, (size_t)a.n_pairs * sizeof(int2), hipMemcpyHostToDevice, m->stream));
        *dp = m->pairs;
    }
    if (a.mask && !a.devm) {
        if ((rc = ensure((void **)&m->f_mask, &m->cap_f_mask, a.n_pairs, 1))) return rc;
        HIPCHK(hipMemcpyAsync(m->f_mask, a.mask, (size_t)a.n_pairs, hipMemcpyHostToDevice, m->stream));
        *dm = m->f_mask;
    }
    return SIFTMI_OK;
}

void launch_eb_fit_pass1(hipStream_t st, int n_work, const uint8_t *d1, const uint8_t *d2, const int2 *dp, const uint8_t *dm, const EbWork *work,
                         float4 *pts, const EbFitScratch &fs) {
    hipLaunchKernelGGL(eb_fit_pass1_kernel, dim3((unsigned)n_work), dim3(SIFT_FIT_THREADS), 0, st, d1, d2, dp, dm, work, pts, fs);
}
void launch_eb_fit_pass2(hipStream_t st, int n_work, const float4 *pts, const uint8_t *dm, const EbWork *work, const EbFitScratch &fs) {
    hipLaunchKernelGGL(eb_fit_pass2_kernel, dim3((unsigned)n_work), dim3(SIFT_FIT_THREADS), 0, st, pts, dm, work, fs);
}
void launch_eb_fit_pass3(hipStream_t st, int n_work, const float4 *pts, const uint8_t *dm, const EbWork *work, const EbFitScratch &fs) {
    hipLaunchKernelGGL(eb_fit_pass3_kernel, dim3((unsigned)n_work), dim3(SIFT_FIT_THREADS), 0, st, pts, dm, work, fs);
}
void launch_eb_fit_finish(hipStream_t st, const EbWork *segs, int S, const EbFitScratch &fs) {
    hipLaunchKernelGGL(eb_fit_finish_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, st, segs, S, fs);
}
void launch_eb_shift(hipStream_t st, int n_segs, const uint8_t *d1, const uint8_t *d2, const int2 *dp, const uint8_t *dm, const EbWork *segs,
                     uint2 *keys, float tol, uint8_t *keep, float *out, long long *counts) {
    hipLaunchKernelGGL(eb_shift_kernel, dim3((unsigned)n_segs), dim3(SIFT_SHIFT_THREADS), 0, st, d1, d2, dp, dm, segs, keys, tol, keep, out, counts);
}
}  // namespace

int siftmi_match_fit_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                           const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                           const int64_t *counts1, const int64_t *counts2,
                           const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device, const int64_t *pair_counts,
                           const uint8_t *mask, int32_t mask_is_device, int32_t blocks, double *out, double *kernel_ms) {
    const EbBatch a = {kp1, n1, kp1_is_device, kp2, n2, kp2_is_device, n_segments, counts1, counts2, pairs, n_pairs, pairs_is_device,
                       pair_counts, mask, mask_is_device};
    int rc;
    if ((rc = eb_validate(m, a))) return rc;
    const int S = n_segments;
    if (S > 0 && !out) return fail(SIFTMI_EINVAL, "null argument");
    if (blocks < 0 || blocks > SIFT_FIT_MAX_BLOCKS) return fail(SIFTMI_EINVAL, "blocks %d outside 0..%d", blocks, SIFT_FIT_MAX_BLOCKS);
    int64_t W = 0;
    for (int s = 0; s < S; s++) W += eb_blocks(pair_counts[s], blocks);
    if (W > SIFT_EB_MAX_WORK) return fail(SIFTMI_EINVAL, "%lld workgroups in all: more than %d", (long long)W, SIFT_EB_MAX_WORK);
    HIPCHK(hipSetDevice(m->device));
    if (kernel_ms) *kernel_ms = 0.0;
    const auto empty_row = [](double *row) {
        for (int k = 0; k < SIFT_FIT_OUT; k++) row[k] = std::nan("");
        row[SIFT_FIT_STATUS] = 1.0; row[SIFT_FIT_N] = 0.0;
    };
    if (n_pairs == 0) {     // every segment EMPTY, nothing is launched
        for (int s = 0; s < S; s++) empty_row(out + (size_t)s * SIFT_FIT_OUT);
        return SIFTMI_OK;
    }
    // the tables, one upload: the workgroups' entries, then one entry per segment; behind them, on the host, the results
    const int64_t o_work = 0, o_segs = o_work + W * (int64_t)sizeof(EbWork), tab_bytes = o_segs + S * (int64_t)sizeof(EbWork),
                  res_bytes = (int64_t)S * SIFT_FIT_OUT * (int64_t)sizeof(double);
    // the partials and the results: p1 [W][4], p2 [W][7], p3 [W], count [W], out [S][20], eight bytes each
    const int64_t n_f64 = W * 13 + (int64_t)S * SIFT_FIT_OUT;
    if ((rc = ensure_pinned(&m->eb_host, &m->cap_eb_host, tab_bytes + res_bytes)) ||
        (rc = ensure((void **)&m->eb_tab, &m->cap_eb_tab, tab_bytes, 1)) ||
        (rc = ensure((void **)&m->eb_f64, &m->cap_eb_f64, n_f64, sizeof(double))) ||
        (rc = ensure((void **)&m->c_pts, &m->cap_c_pts, n_pairs, sizeof(float4)))) return rc;
    eb_fill(a, blocks, false, (EbWork *)(m->eb_host + o_segs), (EbWork *)(m->eb_host + o_work));
    const uint8_t *d1, *d2, *dm;
    const int2 *dp;
    if ((rc = eb_stage(m, a, &d1, &d2, &dp, &dm))) return rc;
    HIPCHK(hipMemcpyAsync(m->eb_tab, m->eb_host, (size_t)tab_bytes, hipMemcpyHostToDevice, m->stream));
    EbFitScratch fs;
    fs.p1 = m->eb_f64; fs.p2 = fs.p1 + W * 4; fs.p3 = fs.p2 + W * 7;
    fs.count = (unsigned long long *)(fs.p3 + W); fs.out = fs.p3 + 2 * W;
    const EbWork *work = (const EbWork *)(m->eb_tab + o_work), *segs = (const EbWork *)(m->eb_tab + o_segs);
    double *res = (double *)(m->eb_host + tab_bytes);
    hipEventRecord(m->ec_a, m->stream);
    launch_eb_fit_pass1(m->stream, (int)W, d1, d2, dp, dm, work, m->c_pts, fs);
    launch_eb_fit_pass2(m->stream, (int)W, (const float4 *)m->c_pts, dm, work, fs);
    launch_eb_fit_pass3(m->stream, (int)W, (const float4 *)m->c_pts, dm, work, fs);
    launch_eb_fit_finish(m->stream, segs, S, fs);
    hipEventRecord(m->ec_b, m->stream);
    HIPCHK(hipMemcpyAsync(res, fs.out, (size_t)res_bytes, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    if (kernel_ms) { float ms = 0; hipEventElapsedTime(&ms, m->ec_a, m->ec_b); *kernel_ms = ms; }
    memcpy(out, res, (size_t)res_bytes);
    for (int s = 0; s < S; s++) if (pair_counts[s] == 0) empty_row(out + (size_t)s * SIFT_FIT_OUT);     // no workgroup wrote these
    return SIFTMI_OK;
}

int siftmi_match_shift_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                             const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                             const int64_t *counts1, const int64_t *counts2,
                             const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device, const int64_t *pair_counts,
                             const uint8_t *mask, int32_t mask_is_device, float tol, uint8_t *keep, float *out, int64_t *counts,
                             double *kernel_ms) {
    const EbBatch a = {kp1, n1, kp1_is_device, kp2, n2, kp2_is_device, n_segments, counts1, counts2, pairs, n_pairs, pairs_is_device,
                       pair_counts, mask, mask_is_device};
    int rc;
    if ((rc = eb_validate(m, a))) return rc;
    const int S = n_segments;
    if (S > 0 && (!out || !counts)) return fail(SIFTMI_EINVAL, "null argument");
    if (keep && !(tol >= 0.f)) return fail(SIFTMI_EINVAL, "tol must be >= 0 (+inf is allowed) with a keep mask");
    HIPCHK(hipSetDevice(m->device));
    if (kernel_ms) *kernel_ms = 0.0;
    const auto empty_row = [&](int s) {
        for (int k = 0; k < SIFT_SHIFT_OUT; k++) out[(size_t)s * SIFT_SHIFT_OUT + k] = std::nanf("");
        counts[2 * (size_t)s] = counts[2 * (size_t)s + 1] = 0;
    };
    if (n_pairs == 0) {     // every segment EMPTY, nothing is launched
        for (int s = 0; s < S; s++) empty_row(s);
        return SIFTMI_OK;
    }
    // the table, one upload: one entry per segment with a pair; behind it, on the host, the results: counts [S][2], out [S][6]
    const int64_t tab_bytes = S * (int64_t)sizeof(EbWork), cnt_bytes = (int64_t)S * 2 * (int64_t)sizeof(long long),
                  res_bytes = cnt_bytes + (int64_t)S * SIFT_SHIFT_OUT * (int64_t)sizeof(float);
    if ((rc = ensure_pinned(&m->eb_host, &m->cap_eb_host, tab_bytes + res_bytes)) ||
        (rc = ensure((void **)&m->eb_tab, &m->cap_eb_tab, tab_bytes, 1)) ||
        (rc = ensure((void **)&m->eb_res, &m->cap_eb_res, res_bytes, 1)) ||
        (rc = ensure((void **)&m->s_keys, &m->cap_s_keys, n_pairs, sizeof(uint2)))) return rc;
    if (keep && (rc = ensure((void **)&m->c_mask, &m->cap_c_mask, n_pairs, 1))) return rc;
    const int E = eb_fill(a, 1, true, (EbWork *)m->eb_host, nullptr);
    const uint8_t *d1, *d2, *dm;
    const int2 *dp;
    if ((rc = eb_stage(m, a, &d1, &d2, &dp, &dm))) return rc;
    HIPCHK(hipMemcpyAsync(m->eb_tab, m->eb_host, (size_t)E * sizeof(EbWork), hipMemcpyHostToDevice, m->stream));
    uint8_t *res = m->eb_host + tab_bytes;
    hipEventRecord(m->ec_a, m->stream);
    launch_eb_shift(m->stream, E, d1, d2, dp, dm, (const EbWork *)m->eb_tab, m->s_keys, tol, keep ? m->c_mask : nullptr,
                    (float *)(m->eb_res + cnt_bytes), (long long *)m->eb_res);
    hipEventRecord(m->ec_b, m->stream);
    HIPCHK(hipMemcpyAsync(res, m->eb_res, (size_t)res_bytes, hipMemcpyDeviceToHost, m->stream));
    if (keep) HIPCHK(hipMemcpyAsync(keep, m->c_mask, (size_t)n_pairs, hipMemcpyDeviceToHost, m->stream));
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    if (kernel_ms) { float ms = 0; hipEventElapsedTime(&ms, m->ec_a, m->ec_b); *kernel_ms = ms; }
    static_assert(sizeof(long long) == sizeof(int64_t), "the counts come back as they are");
    memcpy(counts, res, (size_t)cnt_bytes);
    memcpy(out, res + cnt_bytes, (size_t)(res_bytes - cnt_bytes));
    for (int s = 0; s < S; s++) if (pair_counts[s] == 0) empty_row(s);      // no workgroup wrote these
    return SIFTMI_OK;
}

// The consensus filter over every segment of a batch at once (k_consensus_batch.hpp; the contract is DESIGN.md section 7 row 14)
namespace {
inline int64_t cb_tiles(int64_t rows) { return (rows + SIFT_CONS_TILE - 1) / SIFT_CONS_TILE; }
// The table, segments in order: `tiles` gets the tiles of every segment, `segs` one entry per active segment (three pairs or more)
void cb_fill(const EbBatch &a, CbWork *tiles, CbWork *segs) {
    int64_t off1 = 0, off2 = 0, row0 = 0, t = 0;
    int act = 0;
    for (int s = 0; s < a.S; s++) {
        const int64_t rows = a.pair_counts[s], n1 = a.counts1 ? a.counts1[s] : a.n1, n2 = a.counts2[s];
        CbWork w = {s, rows >= 3 ? act : -1, (int)row0, (int)rows, (int)off1, (int)n1, (int)off2, (int)n2};
        if (rows >= 3) segs[act++] = w;
        for (int64_t r = 0; r < rows; r += SIFT_CONS_TILE) {
            w.row0 = (int)(row0 + r); w.rows = (int)(rows - r < SIFT_CONS_TILE ? rows - r : SIFT_CONS_TILE);
            tiles[t++] = w;
        }
        row0 += rows; off2 += n2;
        if (a.counts1) off1 += n1;
    }
}

void launch_cb_gather(hipStream_t st, int n_tiles, const uint8_t *d1, const uint8_t *d2, const int2 *dp, const CbWork *tiles, float4 *pts) {
    hipLaunchKernelGGL(cb_gather_kernel, dim3((unsigned)n_tiles), dim3(SIFT_CONS_THREADS), 0, st, d1, d2, dp, tiles, pts);
}
void launch_cb_solve(hipStream_t st, int n_active, const float4 *pts, const CbWork *segs, int H, uint32_t seed, float *models, uint8_t *valid,
                     int *votes) {
    hipLaunchKernelGGL(cb_solve_kernel, dim3((unsigned)((H + 255) / 256), (unsigned)n_active), dim3(256), 0, st, pts, segs, H, seed, models,
                       valid, votes);
}
// siftmi_match_consensus's vote grid with all tiles of the batch in place of one list's: about eight workgroups per CU, a chunk at
// most the kernel's LDS counters and at least 16 hypotheses.  x: up to 2^20 tiles; y: at most max(2048, H / 512) = 2048 chunks
void launch_cb_vote(hipStream_t st, int n_tiles, const float4 *pts, const CbWork *tiles, const float *models, int H, float tol2, int *votes) {
    int chunks = (2048 + n_tiles - 1) / n_tiles;
    const int min_chunks = (H + SIFT_CONS_HMAX - 1) / SIFT_CONS_HMAX, max_chunks = (H + 15) / 16;
    if (chunks > max_chunks) chunks = max_chunks;
    if (chunks < min_chunks) chunks = min_chunks;
    const int h_chunk = (H + chunks - 1) / chunks;
    chunks = (H + h_chunk - 1) / h_chunk;
    hipLaunchKernelGGL(cb_vote_kernel, dim3((unsigned)n_tiles, (unsigned)chunks), dim3(SIFT_CONS_THREADS), 0, st, pts, tiles, models, H, h_chunk,
                       tol2, votes);
}
void launch_cb_select(hipStream_t st, int n_active, const int *votes, const uint8_t *valid, const float *models, int H, ConsensusResult *results) {
    hipLaunchKernelGGL(cb_select_kernel, dim3((unsigned)n_active), dim3(256), 0, st, votes, valid, models, H, results);
}
void launch_cb_mask(hipStream_t st, int n_tiles, const float4 *pts, const CbWork *tiles, const ConsensusResult *results, float tol2, uint8_t *mask) {
    hipLaunchKernelGGL(cb_mask_kernel, dim3((unsigned)n_tiles), dim3(SIFT_CONS_THREADS), 0, st, pts, tiles, results, tol2, mask);
}
}  // namespace

int siftmi_match_consensus_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                                 const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                                 const int64_t *counts1, const int64_t *counts2,
                                 const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device, const int64_t *pair_counts,
                                 int32_t n_hyp, float tol, uint32_t seed, uint8_t *mask, int32_t mask_is_device,
                                 float *models, int32_t *winners, int32_t *winner_votes, int32_t *votes_all, float *models_all,
                                 double *kernel_ms) {
    const EbBatch a = {kp1, n1, kp1_is_device, kp2, n2, kp2_is_device, n_segments, counts1, counts2, pairs, n_pairs, pairs_is_device,
                       pair_counts, nullptr, 0};
    int rc;
    if ((rc = eb_validate(m, a))) return rc;
    const int S = n_segments, H = n_hyp;
    if (n_hyp < 1 || n_hyp > (1 << 20)) return fail(SIFTMI_EINVAL, "n_hyp %d outside 1..2^20", n_hyp);
    if (!std::isfinite(tol) || !(tol > 0.f)) return fail(SIFTMI_EINVAL, "tol must be finite and > 0");
    if (n_pairs > 0 && !mask) return fail(SIFTMI_EINVAL, "null mask with %lld pairs", (long long)n_pairs);
    if (S > 0 && (!models || !winners || !winner_votes)) return fail(SIFTMI_EINVAL, "null argument");
    int64_t T = 0, A = 0;
    for (int s = 0; s < S; s++) { T += cb_tiles(pair_counts[s]); A += pair_counts[s] >= 3; }
    if (A * H > SIFT_CB_MAX_HYP) return fail(SIFTMI_EINVAL, "%lld segments of three pairs or more x %d hypotheses: more than %d", (long long)A, H, SIFT_CB_MAX_HYP);
    if (T > SIFT_CB_MAX_TILES) return fail(SIFTMI_EINVAL, "%lld tiles in all: more than %d", (long long)T, SIFT_CB_MAX_TILES);
    HIPCHK(hipSetDevice(m->device));
    if (kernel_ms) *kernel_ms = 0.0;
    // what a segment without a winner gets; the active segments' rows are replaced below
    for (int s = 0; s < S; s++) { winners[s] = -1; winner_votes[s] = 0; }
    for (int64_t i = 0; i < (int64_t)S * 6; i++) models[i] = std::nanf("");
    if (votes_all) memset(votes_all, 0, sizeof(int32_t) * (size_t)S * (size_t)H);
    if (models_all) for (int64_t i = 0; i < (int64_t)S * H * 6; i++) models_all[i] = std::nanf("");
    if (A == 0) {           // every triple of every segment repeats an index: nothing is launched, the mask is all zero
        if (n_pairs > 0 && mask_is_device) {
            HIPCHK(hipDeviceSynchronize());
            HIPCHK(hipMemsetAsync(mask, 0, (size_t)n_pairs, m->stream));
            HIPCHK(hipStreamSynchronize(m->stream));
        } else if (n_pairs > 0) {
            memset(mask, 0, (size_t)n_pairs);
        }
        return SIFTMI_OK;
    }
    // the table, one upload: the tiles' entries, then one entry per active segment; behind them, on the host, the segments' results
    const int64_t o_segs = T * (int64_t)sizeof(CbWork), tab_bytes = o_segs + A * (int64_t)sizeof(CbWork),
                  res_bytes = A * (int64_t)sizeof(ConsensusResult);
    if ((rc = ensure_pinned(&m->eb_host, &m->cap_eb_host, tab_bytes + res_bytes)) ||
        (rc = ensure((void **)&m->eb_tab, &m->cap_eb_tab, tab_bytes, 1)) ||
        (rc = ensure((void **)&m->eb_res, &m->cap_eb_res, res_bytes, 1)) ||
        (rc = ensure((void **)&m->c_pts, &m->cap_c_pts, n_pairs, sizeof(float4))) ||
        (rc = ensure((void **)&m->c_valid, &m->cap_c_valid, A * H, 1)) ||
        (rc = ensure((void **)&m->c_models, &m->cap_c_models, A * H * 6, sizeof(float))) ||
        (rc = ensure((void **)&m->c_votes, &m->cap_c_votes, A * H, sizeof(int)))) return rc;
    if (!mask_is_device && (rc = ensure((void **)&m->c_mask, &m->cap_c_mask, n_pairs, 1))) return rc;
    cb_fill(a, (CbWork *)m->eb_host, (CbWork *)(m->eb_host + o_segs));
    if (mask_is_device && !(kp1_is_device || kp2_is_device || pairs_is_device)) HIPCHK(hipDeviceSynchronize());   // eb_stage: the inputs
    const uint8_t *d1, *d2, *dm;
    const int2 *dp;
    if ((rc = eb_stage(m, a, &d1, &d2, &dp, &dm))) return rc;
    HIPCHK(hipMemcpyAsync(m->eb_tab, m->eb_host, (size_t)tab_bytes, hipMemcpyHostToDevice, m->stream));
    const CbWork *tiles = (const CbWork *)m->eb_tab, *segs = (const CbWork *)(m->eb_tab + o_segs);
    ConsensusResult *results = (ConsensusResult *)m->eb_res, *res = (ConsensusResult *)(m->eb_host + tab_bytes);
    uint8_t *dmask = mask_is_device ? mask : m->c_mask;
    const float tol2 = tol * tol;
    launch_cb_gather(m->stream, (int)T, d1, d2, dp, tiles, m->c_pts);
    launch_cb_solve(m->stream, (int)A, (const float4 *)m->c_pts, segs, H, seed, m->c_models, m->c_valid, m->c_votes);
    hipEventRecord(m->ec_a, m->stream);
    launch_cb_vote(m->stream, (int)T, (const float4 *)m->c_pts, tiles, (const float *)m->c_models, H, tol2, m->c_votes);
    hipEventRecord(m->ec_b, m->stream);
    launch_cb_select(m->stream, (int)A, (const int *)m->c_votes, (const uint8_t *)m->c_valid, (const float *)m->c_models, H, results);
    launch_cb_mask(m->stream, (int)T, (const float4 *)m->c_pts, tiles, (const ConsensusResult *)results, tol2, dmask);
    HIPCHK(hipMemcpyAsync(res, results, (size_t)res_bytes, hipMemcpyDeviceToHost, m->stream));
    if (!mask_is_device) HIPCHK(hipMemcpyAsync(mask, m->c_mask, (size_t)n_pairs, hipMemcpyDeviceToHost, m->stream));
    if (votes_all || models_all) {      // test hooks: the rows of active segment `act` go to segment s
        int64_t act = 0;
        for (int s = 0; s < S; s++) {
            if (pair_counts[s] < 3) continue;
            if (votes_all) HIPCHK(hipMemcpyAsync(votes_all + (size_t)s * H, m->c_votes + act * H, sizeof(int) * (size_t)H, hipMemcpyDeviceToHost, m->stream));
            if (models_all) HIPCHK(hipMemcpyAsync(models_all + (size_t)s * H * 6, m->c_models + act * H * 6, sizeof(float) * 6 * (size_t)H,
                                                  hipMemcpyDeviceToHost, m->stream));
            act++;
        }
    }
    HIPCHK(hipStreamSynchronize(m->stream));
    HIPCHK(hipGetLastError());
    if (kernel_ms) { float ms = 0; hipEventElapsedTime(&ms, m->ec_a, m->ec_b); *kernel_ms = ms; }
    int64_t act = 0;
    for (int s = 0; s < S; s++) {
        if (pair_counts[s] < 3) continue;
        const ConsensusResult &r = res[act++];
        winners[s] = r.winner; winner_votes[s] = r.votes;
        if (r.winner >= 0) memcpy(models + (size_t)s * 6, r.model, sizeof r.model);
    }
    return SIFTMI_OK;
}

int siftmi_match_last_kernel_ms(const siftmi_matcher *m, float *ms) {
    if (!m || !ms) return fail(SIFTMI_EINVAL, "null argument");
    *ms = m->last_ms;
    return SIFTMI_OK;
}

int siftmi_match_last_stage_ms(const siftmi_matcher *m, float *ms4) {
    if (!m || !ms4) return fail(SIFTMI_EINVAL, "null argument");
    if (!m->profile) return fail(SIFTMI_EINVAL, "the matcher was created without profiling");
    for (int i = 0; i < 4; i++) ms4[i] = m->stage_ms[i];
    return SIFTMI_OK;
}

}  // extern "C"
