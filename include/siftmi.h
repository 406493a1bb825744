/*
 * siftmi.h -- C ABI of libsiftmi.so, the MI355X (gfx950) SIFT hot path.
 *
 * This is the drop-in boundary for the reference's SiftPlan.keypoints() / MatchPlan.match()
 * path.  The reference (pierrepaleo/sift_pyocl) has no FFI of its own: its boundary is
 * PyOpenCL -- pyopencl.Program(...).build() (sift-src/plan.py:364), kernel launches
 * program.kernel(queue, global, local, *args) (e.g. plan.py:586-591, match.py:246-255),
 * pyopencl.array allocation (plan.py:276-293) and blocking enqueue_copy read-backs
 * (plan.py:452-468, 642, 751; match.py:258-261).  Each entry point below names the reference
 * interface it replaces.  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions: every function returns 0 on success, a negative SIFTMI_E* code otherwise, with a
 * message retrievable from siftmi_last_error() (thread-local).  Handles are opaque, bound to one
 * HIP device and one HIP stream, and must be used by one host thread at a time (the Python
 * wrapper holds the reference's per-plan semaphore, plan.py:156,439 / match.py:117,215).
 * "is_device" pointers are HIP device pointers on the plan's device, inputs and outputs alike
 * (out_is_device, pairs_is_device, mask_is_device ...).  What is guaranteed for them, and tested
 * entry point by entry point and pointer by pointer (tests/test_gpu_ordering.py):
 *   - a device pointer is read and written only after everything the caller had enqueued, on ANY
 *     stream of the process (blocking or not, the NULL stream included), before the call: the call
 *     synchronises the device once on entry when a device pointer is passed -- the library's own
 *     streams are non-blocking, so nothing else orders them after a caller's stream.  No event or
 *     synchronisation is needed between producing the data and the call, and none between
 *     enqueueing a write to an output buffer and the call that overwrites it;
 *   - host and device results are complete when the call returns: they may be read at once, on
 *     the host or on any stream.
 */
#ifndef SIFTMI_H
#define SIFTMI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SIFTMI_OK 0
#define SIFTMI_EINVAL (-1)   /* bad argument                       -> RuntimeError / AssertionError in Python */
#define SIFTMI_ENOMEM (-2)   /* device or host allocation failed   -> MemoryError  (plan.py:365-366)           */
#define SIFTMI_EDEVICE (-3)  /* HIP runtime error / no gfx950 GPU  -> RuntimeError                             */
#define SIFTMI_ECAPACITY (-4)/* output buffer too small (results truncated, *n_out = number written)           */

/* input pixel types accepted by SiftPlan (plan.py:99-106, 450-488) */
enum siftmi_dtype {
    SIFTMI_F32 = 0, SIFTMI_U8 = 1, SIFTMI_U16 = 2, SIFTMI_U32 = 3, SIFTMI_U64 = 4,
    SIFTMI_I32 = 5, SIFTMI_I64 = 6, SIFTMI_F64 = 7, SIFTMI_RGB8 = 8
};

/* 144-byte keypoint record == SiftPlan.dtype_kp / MatchPlan.dtype_kp (plan.py:110-115, match.py:70-75),
 * == t_keypoint of openCL/matching_cpu.cl:22-25 */
typedef struct siftmi_keypoint {
    float x, y, scale, angle;
    uint8_t desc[128];
} siftmi_keypoint;

/* SIFT parameters read from sift_pyocl.param.par at call time (param.py:52-79) */
typedef struct siftmi_params {
    double init_sigma;    /* SiftPlan(init_sigma=) or par.InitSigma; Python double (plan.py:129-131) */
    float peak_thresh;    /* par.PeakThresh  -> local_maxmin / interp_keypoint (plan.py:631, 648)    */
    float edge_thresh0;   /* par.EdgeThresh1 -> kernel slot EdgeThresh0, octsize<=1 (plan.py:633)    */
    float edge_thresh;    /* par.EdgeThresh  -> kernel slot EdgeThresh (plan.py:634)                 */
    float ori_sigma;      /* par.OriSigma    (plan.py:681)                                           */
    int32_t border_dist;  /* par.BorderDist  (plan.py:630)                                           */
    int32_t octave_max;   /* 0 = every octave (reference behaviour, plan.py:213-224); >0 = extension */
    int32_t pix_per_kp;   /* SiftPlan.PIX_PER_KP: kpsize = H*W / pix_per_kp (plan.py:109, 243)       */
    int32_t double_im_size; /* par.DoubleImSize != 0: the frame counts as blurred by sigma 1.0 instead of 0.5, i.e. the
                             * initial blur is sqrt(init_sigma^2 - 1) wide (plan.py:254, 297, 534) -- all the reference does
                             * with that parameter; the image is not resampled                                           */
} siftmi_params;

typedef struct siftmi_plan siftmi_plan;
typedef struct siftmi_matcher siftmi_matcher;

/* ---- runtime ------------------------------------------------------------------------------
 * replaces sift-src/clinit.py device enumeration (ocl.select_device, clinit.py:360-400) */
int siftmi_device_count(void);
int siftmi_device_name(int device_id, char *buf, int64_t buflen);
const char *siftmi_last_error(void);
const char *siftmi_version(void);

/* ---- SiftPlan ------------------------------------------------------------------------------
 * siftmi_plan_create    <- SiftPlan.__init__ (plan.py:117-201): sizes the pyramid (_calc_scales
 *                          :213), allocates every device buffer (_allocate_buffers :268) and the six
 *                          Gaussian tap vectors (_init_gaussian :308).
 * siftmi_plan_keypoints <- SiftPlan.keypoints (plan.py:432-567) including _one_octave (:596-756) and
 *                          _compact (:758-795); one host<->device synchronisation per image instead of
 *                          >= 18 per octave.  Output order within the result is unspecified (as in the
 *                          reference, whose kernels append through atomic_inc).
 *                          image_dtype must be the plan's dtype or SIFTMI_F32 (plan.py:444 accepts both).
 * siftmi_plan_get_minmax<- buffers["min"] / buffers["max"] (plan.py:286-287; read by alignment.py:345).
 * siftmi_plan_profile   <- SiftPlan.log_profile (plan.py:826-847): "label\tms\n" lines of the last call.
 */
int siftmi_plan_create(int32_t height, int32_t width, int32_t in_dtype, int32_t device_id,
                       const siftmi_params *params, int32_t profile, siftmi_plan **out);
int siftmi_plan_info(const siftmi_plan *plan, int32_t *n_octaves, int64_t *kpsize, int64_t *bytes_allocated);
/* Capacity as the reference (plan.py:243, 797-804): kpsize = H*W / PIX_PER_KP entries PER OCTAVE -- for the candidates of a
 * detection scale appended behind the octave's oriented keypoints so far, and for those oriented keypoints.  An image within
 * that rule returns every record (up to n_octaves * kpsize of them); one beyond it raises `overflow` and keeps at most kpsize
 * records of each octave (the reference silently drops whatever its atomic counter places beyond the buffer, image.cl:203-205).
 * The device lists start at kpsize entries and grow when an image needs more (it is then run again inside the same call):
 * siftmi_plan_capacity reports the record list's current size and how often a list has grown. */
int siftmi_plan_capacity(const siftmi_plan *plan, int64_t *records, int64_t *growths);
/* How often the one-launch form of the small octaves (a workgroup per octave, chained through a flag with a bounded wait) gave up
 * waiting and the image ran again octave by octave -- the result is the same either way, the plan keeps the per-octave launches
 * from then on (*tail_enabled 0).  No reference counterpart: the reference launches every octave's kernels one by one. */
int siftmi_plan_tail_timeouts(const siftmi_plan *plan, int64_t *timeouts, int32_t *tail_enabled);
int siftmi_plan_set_params(siftmi_plan *plan, const siftmi_params *params);
/* Tuning / diagnostic option of one plan by name (the reference's counterparts are constructor keywords such as
 * max_workgroup_size, plan.py:117-131).  Results never depend on an option.  Unknown name, a value outside int32, or "ori_pad" /
 * "desc_pad" outside 0..65536 (bytes of dynamic LDS per workgroup) -> SIFTMI_EINVAL.  Names:
 *   launch shapes      "march", "march_wgs", "xcd_map" (marching blur, extrema: every XCD takes a contiguous range of tiles; default 1), "march_prio" (marching blur: wave priority falls with a workgroup's progress -- 0 never, 1 = default: launches of about three workgroups per CU and the later octaves' chains, 2 every launch), "mm_blocks", "mm_threads", "ext_rows", "ext_strips",
 *                      "ori_blocks", "ori_small_blocks", "ori_pad", "ori_team", "desc_blocks", "desc_small_blocks", "desc_early_blocks",
 *                      "desc_dense_blocks", "desc_pad", "desc_team", "desc_dynamic", "desc_stream", "maps_blocks"
 *   kernel forms       "fused_convert", "fused_shrink", "fused_refine", "tail", "tail_pixels",
 *                      "maps" (0 never / 1 always / 2 by the previous image's count), "maps_density"
 *   stream schedule    "overlap" (0: one stream), "fork" (the octaves below octave 0 as two chains and groups -- octave 1 | the rest: 0 never, 1 always, 2 from five octaves),
 *                      "early_chain" (that chain starts at plane 3 of octave 0: 0 never, 1 always, 2 unless the previous image was keypoint-rich),
 *                      "split" (frames whose later octaves form ONE chain: the octaves below octave 1 built and searched on a stream of their own, one
 *                      orientation / descriptor launch for the group; default 0), "spin"
 *   diagnostics        "host_timing", "tail_fault" (treat the next n tail launches as timed out: exercises the re-run path) */
int siftmi_plan_set_option(siftmi_plan *plan, const char *name, int64_t value);
/* out_is_device of siftmi_plan_keypoints: where the result array lives.  SIFTMI_OUT_PINNED = pinned host memory from
 * siftmi_host_alloc: the descriptor kernels write every record straight into it while they run (zero-copy over PCIe),
 * so no device-to-host copy follows the last kernel (the reference copies keypoints and descriptors of every octave
 * back with blocking reads, plan.py:541-567). */
#define SIFTMI_OUT_HOST 0
#define SIFTMI_OUT_DEVICE 1
#define SIFTMI_OUT_PINNED 2
/* Pinned, device-writable host blocks from a size-bucketed pool (a power of two from 64 KiB to 1 MiB, a multiple of 2 MiB
 * above).  The reference returns ordinary numpy arrays (plan.py:553-565); page-locked result arrays are this build's way to
 * have no copy after the last kernel, and they cannot be swapped out: the pool holds at most `limit` bytes (default 2 GiB,
 * live + spare) and siftmi_host_alloc returns SIFTMI_ENOMEM beyond it -- the Python layer then hands out an ordinary array.
 * siftmi_host_free never calls the driver (it runs from destructors; hipHostFree synchronises the device): surplus blocks
 * are released by the next siftmi_host_alloc or by siftmi_host_pool_trim(keep_bytes). */
int siftmi_host_alloc(int64_t bytes, void **out);
int siftmi_host_free(void *ptr);
int siftmi_host_pool_limit(int64_t limit_bytes /* < 0: query only */, int64_t *live_bytes, int64_t *spare_bytes);
int siftmi_host_pool_trim(int64_t keep_bytes);
int siftmi_plan_keypoints(siftmi_plan *plan, const void *image, int32_t image_dtype, int32_t image_is_device,
                          siftmi_keypoint *out, int32_t out_is_device, int64_t capacity, int64_t *n_out,
                          int32_t *overflow);
/* two-step variant: siftmi_plan_keypoints(..., out = NULL, capacity = 0, ...) only returns the count and
 * leaves the records on the device; siftmi_plan_fetch copies records [first, first+count) of the last call
 * (to a host buffer, or to a device buffer with out_is_device) -- saves one host-side copy of the result */
int siftmi_plan_fetch(siftmi_plan *plan, siftmi_keypoint *out, int32_t out_is_device, int64_t first, int64_t count);
/* device address and count of the records of the last call; valid until the next siftmi_plan_keypoints on this plan
 * (lets MatchPlan consume them in place, as the reference matches pyopencl arrays: alignment.py:155-157,250) */
int siftmi_plan_records_device(const siftmi_plan *plan, const siftmi_keypoint **records, int64_t *count);
/* What the last finished siftmi_plan_keypoints left behind besides its records (read-only test hooks: the pyramid of every
 * producer -- marching, tile and generic blurs, the fused hand-off, octave_tail_kernel -- compared plane by plane at plan level).
 * The reference keeps the same planes in buffers["scale_<octave>_<scale>"] (plan.py:276-285) and reads its keypoint counter back
 * after every local_maxmin (plan.py:642).  Neither call launches anything (but see below); both are valid until the next call on the plan.
 * siftmi_plan_planes       copies the six blur planes of `octave` (scale 0 first, row pitch W) to the host buffer `out` of
 *                          `capacity` floats, 6 * W * H of them, and returns the octave's W and H (either may be null).  It waits
 *                          for the plan's streams only.  Octave planes are never rewritten within a call.  An octave whose last
 *                          run wrote plane 5 only around its scale-3 candidates (siftmi_plan_set_lazy_top) gets the blur launch it
 *                          went without first: the planes returned are whole either way.
 * siftmi_plan_last_counts  host integers of the complete read-back of the counters that the wait selected:
 *   tail_first     first octave that octave_tail_kernel took in the run that produced the result, n_octaves of the plan when
 *                  there was no tail launch (also after a tail time-out: the result then comes from the re-run)
 *   candidates     [n_octaves] entries the octave's detection appended to its candidate list (a split octave 0's second slot
 *                  folded in).  The fused detect-and-refine launch keeps no candidate list: its octaves read 0 here.
 *                  (Under siftmi_plan_set_lazy_top the provisional scale-3 entries that were rejected do not count.)
 *   c_scale        [n_octaves][3] candidates of the octave per detection scale 1, 2, 3, as the refinement read them
 *   n_octaves      octaves the two arrays have room for (>= the plan's)
 * siftmi_plan_tail_candidates  copies the candidate list octave_tail_kernel kept for `octave` -- min(candidates[octave], 3 * 4096)
 *                          entries (value, row, col, scale) of four floats, in no particular order -- to the host buffer `out` of
 *                          `capacity` floats and returns their number in *count.  Only that launch writes the list; an octave
 *                          below `tail_first` of the run that produced the result has none (also after a tail time-out).
 * SIFTMI_EINVAL, nothing written: a null plan or buffer, a buffer that is too small, an octave outside 0..n_octaves-1 (tail
 * candidates: outside tail_first..n_octaves-1), a plan that has not finished a call (none yet, or the last one failed). */
int siftmi_plan_planes(siftmi_plan *plan, int32_t octave, float *out, int64_t capacity, int32_t *width, int32_t *height);
int siftmi_plan_last_counts(const siftmi_plan *plan, int32_t *tail_first, int32_t *candidates, int32_t *c_scale,
                            int32_t n_octaves);
int siftmi_plan_tail_candidates(const siftmi_plan *plan, int32_t octave, float *out, int64_t capacity, int64_t *count);
/* The top blur plane (plane 5 of an octave) only around scale-3 candidates.  Plane 5 is read at few places: by the extrema pass as
 * the outer layer of scale 3's 27-neighbour test, by the refinement of a scale-3 candidate.  An octave that runs lazily skips
 * the blur launch that writes plane 5, tests scale 3 against 18 neighbours, evaluates plane 5 on a 13 x 13 patch around every
 * provisional candidate (top_patch_kernel) and finishes the test there.  Only octaves whose detection keeps a candidate
 * list run lazily (not the fused detect-and-refine form, not the tail launch, not under the full profile).  Records never
 * depend on it.
 *   mode     0 never, 1 always, 2 (the default) per octave when the previous image of the plan left fewer than one scale-3
 *            candidate per `density` pixels in that octave; a plan's first image is eager
 *   density  pixels per scale-3 candidate of the automatic rule (default 6000); <= 0 keeps the plan's value
 *   blocks   one-wave workgroups of top_patch_kernel (default 8192, at most 65535); <= 0 keeps the plan's value */
int siftmi_plan_set_lazy_top(siftmi_plan *plan, int32_t mode, int32_t density, int32_t blocks);
/* lazy[o] = 1 for every octave o of the last finished call that ran the lazy detection chain (siftmi_plan_set_lazy_top: no full plane 5,
 * provisional scale-3 candidates, top_patch_kernel), else 0; n_octaves: room in `lazy` (>= the plan's).  Read-only test hook
 * for the automatic rule; SIFTMI_EINVAL as siftmi_plan_last_counts. */
int siftmi_plan_lazy_octaves(const siftmi_plan *plan, int32_t *lazy, int32_t n_octaves);
/* Affine warp with bilinear interpolation of an image of the plan's shape -- the `transform` / `transform_RGB`
 * kernels (openCL/transform.cl:22, :116) as LinearAlign.align launches them (sift-src/alignment.py:325-348).
 *   out[y][x] = bilinear(image, (ty, tx)),  ty = matrix[0]*y + matrix[1]*x + offset[0],
 *                                           tx = matrix[2]*y + matrix[3]*x + offset[1]
 * with `fill` outside the image, for taps right of / below it, and where tx >= W-0.5 or ty >= H-0.5.  For RGB8 every
 * channel is converted with (uint8_t): `fill` must lie in [0, 255], a value outside converts a float that uint8_t cannot hold,
 * which C leaves undefined.
 *   image        H x W float32 (channels 1) or H x W x 3 uint8 (channels 3); NULL = the host image most recently
 *                handed to siftmi_plan_keypoints, still staged on the device (the reference's buffers["input"])
 *   out          OH x OW (x3) of the same element type; the whole output is written (the reference only
 *                launches W x H work-items and leaves the `extra` margin of its output buffer undefined)
 *   mode         1 = bilinear (the only value the reference passes), else nearest-lower tap
 *   kernel_ms    optional, hipEvent duration of the kernel */
int siftmi_plan_transform(siftmi_plan *plan, const void *image, int32_t image_is_device, int32_t channels, void *out,
                          int32_t out_is_device, int32_t out_width, int32_t out_height, const float *matrix /*[4]*/,
                          const float *offset /*[2]*/, float fill, int32_t mode, double *kernel_ms);
int siftmi_plan_get_minmax(const siftmi_plan *plan, float *min_out, float *max_out);
int siftmi_plan_profile(const siftmi_plan *plan, char *buf, int64_t buflen);
/* device time (ms, hipEvent on the plan's stream) of the kernels of the last keypoints() call,
 * excluding host<->device copies; requires a profile level at creation.  Under the LIGHT level (profile = 1: one event
 * pair around the octave-0 blur launches and nothing else -- every further event record is a bubble between kernels)
 * the first and last kernels are not bracketed and *total_ms is 0: only the blur figures are measured. */
int siftmi_plan_last_kernel_ms(const siftmi_plan *plan, float *total_ms, float *blur_ms, int32_t *blur_launches,
                               double *blur_pixels);
/* the same restricted to the blur launches of one octave (octave < 0: all).  Octave-0 launches never run
 * concurrently with another kernel of the plan, later octaves overlap the detection stream. */
int siftmi_plan_blur_ms(const siftmi_plan *plan, int32_t octave, float *blur_ms, int32_t *blur_launches,
                        double *blur_pixels);
/* running totals of the two figures above over every keypoints() call since the last reset (light profile): what a
 * benchmark loop reads ONCE after its timed region instead of querying events after every call.
 *   calls, total_ms (first -> last kernel of each call, summed; 0 under the light level, see above), blur0_ms /
 *   blur0_launches / blur0_pixels (octave 0) */
int siftmi_plan_profile_totals(siftmi_plan *plan, int32_t reset, int64_t *calls, double *total_ms, double *blur0_ms,
                               int64_t *blur0_launches, double *blur0_pixels);
int siftmi_plan_destroy(siftmi_plan *plan);

/* ---- batched, pipelined keypoints -----------------------------------------------------------
 * The reference processes one image per SiftPlan.keypoints call and blocks on >= 18 counter read-backs per octave
 * (plan.py:642,689,731,767,777); a stack of frames is a Python loop (scripts/sift_pyocl.py, LinearAlign).  The batch
 * handle is the throughput form of that loop: `lanes` independent plans take the images round-robin,
 * nothing waits until a lane is reused, the records of the whole batch are parked on the device and handed back by one copy.
 *   siftmi_batch_keypoints  images[n]: all host or all device pointers of the batch's shape / dtype (or float32);
 *                           counts[n], offsets[n] (in records, into the parked result) and *total are returned
 *   siftmi_batch_fetch      copies records [first, first+count) of the parked result (host or device destination) */
typedef struct siftmi_batch siftmi_batch;
int siftmi_batch_create(int32_t height, int32_t width, int32_t in_dtype, int32_t device_id, const siftmi_params *params,
                        int32_t lanes, siftmi_batch **out);
int siftmi_batch_destroy(siftmi_batch *batch);
int siftmi_batch_set_params(siftmi_batch *batch, const siftmi_params *params);
int siftmi_batch_info(const siftmi_batch *batch, int32_t *lanes, int64_t *bytes_allocated);
/* siftmi_plan_tail_timeouts summed over the lanes; *lanes_with_tail: lanes that still use the one-launch form */
int siftmi_batch_tail_timeouts(const siftmi_batch *batch, int64_t *timeouts, int32_t *lanes_with_tail);
/* light profiling of the lanes (level 1: one hipEvent pair around the full-resolution blur launches of every frame, as
 * siftmi_plan_create's profile = 1); siftmi_batch_blur_ms returns their sum over the frames of the last batch */
int siftmi_batch_set_profile(siftmi_batch *batch, int32_t level);
/* siftmi_plan_set_option on every lane of the batch */
int siftmi_batch_set_option(siftmi_batch *batch, const char *name, int64_t value);
int siftmi_batch_blur_ms(const siftmi_batch *batch, double *blur_ms, int64_t *blur_launches, double *blur_pixels);
int siftmi_batch_keypoints(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t image_dtype,
                           int32_t images_are_device, int64_t *counts, int64_t *offsets, int64_t *total, int32_t *overflow);
/* same, delivering records into caller-owned host arrays while the batch runs: frame i goes to host_outs[i] if its
 * count fits host_caps[i] (offsets[i] = -1), otherwise it stays parked on the device at offsets[i] for siftmi_batch_fetch;
 * *total_parked = records parked.  The blocking per-frame copy overlaps the other lanes' kernels. */
int siftmi_batch_keypoints_into(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t image_dtype,
                                int32_t images_are_device, siftmi_keypoint *const *host_outs, const int64_t *host_caps,
                                int64_t *counts, int64_t *offsets, int64_t *total_parked, int32_t *overflow);
/* siftmi_batch_fetch: records [first, first + count) of what the last siftmi_batch_keypoints[_into] parked, 0 <= first,
 * 0 <= count, first + count <= *total_parked (checked without forming the sum); anything else is SIFTMI_EINVAL and writes
 * nothing.  count == 0 copies nothing and needs no `out`.  A call of siftmi_batch_keypoints[_into] that FAILED leaves nothing
 * to fetch (every range but a count of 0 is refused until the next call succeeds), as it leaves no min / max; a call
 * refused for its arguments before it started (a null table, a wrong dtype code, ...) leaves the previous batch as it was. */
int siftmi_batch_fetch(siftmi_batch *batch, siftmi_keypoint *out, int32_t out_is_device, int64_t first, int64_t count);
/* The two ends of aligning a stack (the reference aligns frame by frame: LinearAlign.align, alignment.py:225-360).
 * siftmi_batch_minmax     min and max of every frame of the last FINISHED siftmi_batch_keypoints[_into], in input order: each
 *                         lane's values recorded under the frame's index as the lane retires, i.e. what
 *                         siftmi_plan_get_minmax returns for the same frame, from the same kernel (RGB8 and typed frames
 *                         included).  Either array may be null.  Launches nothing.  SIFTMI_EINVAL: a null handle, n_images not
 *                         that batch's size, no batch finished yet (none run, or the last one failed).
 * siftmi_batch_transform  siftmi_plan_transform for n frames of the batch's H x W in ONE launch (transform_batch_kernel /
 *                         transform_rgb_batch_kernel, csrc/k_align_batch.hpp), one synchronisation and at most one copy each
 *                         way besides the 40-byte-per-frame table: frame s of `out` is bit for bit what siftmi_plan_transform
 *                         writes for (images[s], maps[s], fills[s], mode).  A map with a non-finite entry gives a plane of
 *                         fills[s] wherever the entry reaches (an all-NaN map: the whole plane).
 *   images       n pointers, all host or all device (images_are_device); host frames are staged in a buffer the batch owns
 *                and grows, one copy per run of frames that lie back to back in host memory (a contiguous stack: one copy)
 *   out          n x OH x OW (x 3) contiguous, host (staged in a buffer the batch owns and grows, one copy back) or device
 *   maps         n x 6 floats: matrix[4] then offset[2] of each frame, as siftmi_plan_transform takes them
 *   fills        n floats; RGB8: each in [0, 255], as for siftmi_plan_transform
 *   kernel_ms    optional, hipEvent duration of the launch (0 when nothing is launched)
 * Device pointers are ordered after the caller's streams as everywhere (conventions, above).  n_images == 0 or an empty output
 * launches nothing and returns 0.  SIFTMI_EINVAL, nothing launched: a null handle, a null table or output with work to do, a
 * null frame, channels other than 1 or 3, a negative shape or count, n_images > 65535, out_height > 262140. */
int siftmi_batch_transform(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t images_are_device,
                           int32_t channels, void *out, int32_t out_is_device, int32_t out_width, int32_t out_height,
                           const float *maps /* n x 6: matrix[4], offset[2] */, const float *fills /* n */,
                           int32_t mode, double *kernel_ms);
int siftmi_batch_minmax(const siftmi_batch *batch, float *mins, float *maxs, int32_t n_images);
/* What a stack is aligned for (extension; DESIGN.md section 7 row 17, restated in numpy by tests/stack_ref.py; the reference
 * leaves combining the aligned frames to its caller):
 * siftmi_batch_stack      warps n float32 frames of the batch's H x W as siftmi_batch_transform does and reduces them to ONE
 *                         OH x OW plane in the same launch (stack_reduce_kernel / stack_median_kernel, csrc/k_stack.hpp); the n
 *                         warped planes are never written.  Per output pixel, binary32 with one rounding per operation:
 *                           v_s     the value siftmi_batch_transform writes for frame s at this pixel
 *                           live_s  0 <= tx && tx < W + -0.5f && 0 <= ty && ty < H + -0.5f for the source point (ty, tx) of
 *                                   siftmi_plan_transform: where v_s is not fills[s] for a geometric reason.  A non-finite tx or
 *                                   ty is never live: a map with a NaN leaves its frame out wherever the NaN reaches (an all-NaN
 *                                   map: everywhere, which is what LinearAlign.align_batch gives a frame without a usable pair)
 *                           c       the number of live frames, written to `coverage`
 *                           SUM     over the live frames in ascending s: acc = v for the first, acc = acc + v for each later one
 *                           MEAN    acc / (float)c
 *                           MEDIAN  with key(v) = bits(v) ^ (bits(v) >> 31 ? 0xffffffff : 0x80000000) (ascending key = the total
 *                                   order of float32, NaNs by their bits, as for siftmi_match_shift) and lo, hi the live values of
 *                                   rank (c - 1) >> 1 and c >> 1: lo when c is odd, (lo + hi) * 0.5f when even; n <= 64 only.  (A
 *                                   NaN the warp's own arithmetic creates -- 0 * inf, inf - inf -- is the device's default NaN,
 *                                   a positive one: it sorts above +inf)
 *                           c == 0  `empty`
 *   images, maps, fills, mode   as for siftmi_batch_transform (float32 frames only; host frames staged the same way)
 *   out          OH x OW float32, host (staged in a buffer the batch owns and grows, with the coverage behind it) or device
 *   coverage     OH x OW int32 where `out` lives, or NULL
 *   kernel_ms    optional, hipEvent duration of the launch (0 when nothing is launched)
 * One launch, one synchronisation; device pointers are ordered after the caller's streams as everywhere.  An empty output launches
 * nothing and returns 0.  n_images == 0 with a non-empty output fills `out` with `empty` and `coverage` with 0: the reduction
 * kernel launched over no frame is the fill.  SIFTMI_EINVAL, nothing launched: a null handle, a null table or output with work
 * to do, a null frame, a batch created for RGB8, an unknown `reduce`, SIFTMI_STACK_MEDIAN with n_images > 64, a negative shape
 * or count, n_images > 65535, out_height > 262140. */
#define SIFTMI_STACK_SUM 0
#define SIFTMI_STACK_MEAN 1
#define SIFTMI_STACK_MEDIAN 2
#define SIFTMI_STACK_MEDIAN_MAX 64
int siftmi_batch_stack(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t images_are_device,
                       float *out /* OH x OW */, int32_t *coverage /* OH x OW, may be null */, int32_t out_is_device,
                       int32_t out_width, int32_t out_height, const float *maps /* n x 6 */, const float *fills /* n */,
                       int32_t mode, int32_t reduce, float empty, double *kernel_ms);
/* The mean of the samples that survive an outlier rejection (extension; DESIGN.md section 7 row 18, restated in numpy by
 * tests/stack_clip_ref.py):
 * siftmi_batch_stack_clip  warps n <= 64 float32 frames as siftmi_batch_stack does and reduces them per output pixel to a weighted
 *                         mean over a kept set K of the live frames, in one launch (stack_clip_kernel, csrc/k_stack_clip.hpp).
 *                         v_s, live_s, c and key() are siftmi_batch_stack's; osum is its ordered sum over K in ascending s (the
 *                         first value starts the accumulator); binary32, one rounding per operation.  K starts as the live frames.
 *                           TRIM    order the live samples by (key(v_s), s) ascending; h = min(n_high, c - 1),
 *                                   l = min(n_low, c - 1 - h); the last h and the first l leave K.  At least one sample stays, the
 *                                   high side is served first, a positive NaN sorts above +inf and goes with the high side
 *                           SIGMA   kl2 = kappa_low * kappa_low, kh2 = kappa_high * kappa_high; at most `iters` passes, each:
 *                                   n = |K|; n < 3: stop; m = osum(v) / (float)n; d_s = v_s - m; q = osum(d_s * d_s);
 *                                   var = q / (float)n; tl = kl2 * var; th = kh2 * var; s leaves when
 *                                   (d_s < 0 && d_s * d_s > tl) || (d_s > 0 && d_s * d_s > th).  A pass that would remove nothing
 *                                   stops; one that would remove every kept sample removes none and stops.  The statistics are
 *                                   unweighted.  A NaN or inf among the kept values makes every comparison false: nothing leaves
 *                           result  osum(w_s * v_s) / osum(w_s) over K; `kept` = |K|, `coverage` = c; c == 0: `empty`, kept 0.
 *                                   Without weights w_s = 1.0f: with nothing rejected (TRIM 0, 0; SIGMA with iters 0) the plane is
 *                                   SIFTMI_STACK_MEAN's bit for bit
 *                         n samples cannot hold a z-score above (n - 1) / sqrt(n): kappa 3 rejects nothing below 11 live frames.
 *                         TRIM is the rule for short stacks.
 *   images, maps, fills, mode, out, coverage, kernel_ms   as for siftmi_batch_stack
 *   kept         OH x OW int32 where `out` lives, or NULL.  A host result is staged as the plane, the coverage and the kept counts
 *   weights      n floats, each finite and > 0, or NULL for 1.0f
 *   reject       SIFTMI_STACK_TRIM (n_low, n_high are used) or SIFTMI_STACK_SIGMA (kappa_low, kappa_high, iters are used); the
 *                parameters of the other rule are still checked
 * One launch, one synchronisation; device pointers are ordered after the caller's streams as everywhere.  An empty output launches
 * nothing and returns 0.  n_images == 0 with a non-empty output gives `empty` and zeros in both counts.  SIFTMI_EINVAL, nothing
 * launched: everything siftmi_batch_stack refuses, n_images > 64, an unknown `reject`, n_low < 0, n_high < 0 or n_low + n_high > 63, a
 * kappa that is NaN or <= 0 (+inf is allowed and switches its side off), iters < 0, a weight that is not finite and > 0. */
#define SIFTMI_STACK_TRIM 0
#define SIFTMI_STACK_SIGMA 1
#define SIFTMI_STACK_CLIP_MAX 64
int siftmi_batch_stack_clip(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t images_are_device,
                            float *out, int32_t *coverage /* may be null */, int32_t *kept /* may be null */,
                            int32_t out_is_device, int32_t out_width, int32_t out_height,
                            const float *maps /* n x 6 */, const float *fills /* n */, const float *weights /* n, or null = 1.0f */,
                            int32_t mode, int32_t reject, int32_t n_low, int32_t n_high, float kappa_low, float kappa_high,
                            int32_t iters, float empty, double *kernel_ms);
/* A second sampler for the whole warp family (extension; DESIGN.md section 7 row 19, restated in numpy by
 * tests/warp_cubic_ref.py; kernels in csrc/k_warp_cubic.hpp, k_stack.hpp and k_stack_clip.hpp).  Each _ex entry takes its
 * parent's arguments plus `interp` behind `mode`; the parent IS the _ex call with SIFTMI_INTERP_MODE -- one body: staging,
 * ordering after the caller's streams, limits and error states are the parent's.
 *   SIFTMI_INTERP_MODE   what `mode` says: the parent's result, bit for bit
 *   SIFTMI_INTERP_CUBIC  Catmull-Rom bicubic (4 x 4 taps, a = -1/2) on float32 frames.  Binary32; every product, sum and
 *                        difference rounded on its own in the order written (the build's -ffp-contract=off is part of this):
 *     (ty, tx)   as siftmi_plan_transform: ty = (m0*y + m1*x) + off0, tx = (m2*y + m3*x) + off1
 *     live       0 <= tx && tx < (float)W + -0.5f && 0 <= ty && ty < (float)H + -0.5f      (siftmi_batch_stack's live_s, unchanged;
 *                false for a non-finite tx or ty; no index is formed unless live)
 *     !live      out = fill
 *     xp = (int)tx, yp = (int)ty;  fx = tx - (float)xp,  fy = ty - (float)yp
 *     columns    c_k = clamp(xp - 1 + k, 0, W - 1),  rows r_j = clamp(yp - 1 + j, 0, H - 1),  j, k = 0..3   (edge pixels repeat;
 *                `fill` is never mixed into a live sample)
 *     weights    w0 = ((-0.5f*f + 1.0f)*f - 0.5f)*f        w1 = ((1.5f*f - 2.5f)*f)*f + 1.0f
 *                w2 = ((-1.5f*f + 2.0f)*f + 0.5f)*f        w3 = ((0.5f*f - 0.5f)*f)*f            (f = fx for wx, fy for wy)
 *     rows       R_j = ((wx0*p[r_j][c_0] + wx1*p[r_j][c_1]) + wx2*p[r_j][c_2]) + wx3*p[r_j][c_3]
 *     value      out = ((wy0*R_0 + wy1*R_1) + wy2*R_2) + wy3*R_3
 *   At f = 0 the weights are exactly (-0, 1, 0, -0): an integer shift of a finite frame returns its pixels bit for bit, except
 *   that -0.0 becomes +0.0.  At f = 1/4, 1/2, 3/4 they are exact (k / 128; (-1, 9, 9, -1) / 16); their sum is 1 within 2.4e-7.
 *   Zero weights still multiply: a NaN anywhere in the 4 x 4 footprint makes the sample NaN, and so does an inf (0 * inf, inf - inf)
 *   unless every weight it meets is non-zero -- at an integer shift only the sample ON an inf pixel stays inf; a NaN the
 *   arithmetic creates is the device's default NaN, a positive one.  The live set is the bilinear warp's non-fill set: coverage, `empty` and `kept`
 *   of a stack mean the same under both samplers; v_s of the two stack entries is the cubic sample, every rule behind it is
 *   unchanged.  A cubic sample can overshoot the range of its taps.
 * SIFTMI_EINVAL, nothing launched: everything the parent refuses, an unknown `interp`, SIFTMI_INTERP_CUBIC with mode != 1
 * (reserved) or with RGB8 frames (channels == 3, or a batch created for RGB8). */
#define SIFTMI_INTERP_MODE 0
#define SIFTMI_INTERP_CUBIC 1
int siftmi_plan_transform_ex(siftmi_plan *plan, const void *image, int32_t image_is_device, int32_t channels, void *out,
                             int32_t out_is_device, int32_t out_width, int32_t out_height, const float *matrix /*[4]*/,
                             const float *offset /*[2]*/, float fill, int32_t mode, int32_t interp, double *kernel_ms);
int siftmi_batch_transform_ex(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t images_are_device,
                              int32_t channels, void *out, int32_t out_is_device, int32_t out_width, int32_t out_height,
                              const float *maps /* n x 6 */, const float *fills /* n */, int32_t mode, int32_t interp,
                              double *kernel_ms);
int siftmi_batch_stack_ex(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t images_are_device,
                          float *out /* OH x OW */, int32_t *coverage /* may be null */, int32_t out_is_device,
                          int32_t out_width, int32_t out_height, const float *maps /* n x 6 */, const float *fills /* n */,
                          int32_t mode, int32_t interp, int32_t reduce, float empty, double *kernel_ms);
int siftmi_batch_stack_clip_ex(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t images_are_device,
                               float *out, int32_t *coverage /* may be null */, int32_t *kept /* may be null */,
                               int32_t out_is_device, int32_t out_width, int32_t out_height,
                               const float *maps /* n x 6 */, const float *fills /* n */, const float *weights /* n, or null */,
                               int32_t mode, int32_t interp, int32_t reject, int32_t n_low, int32_t n_high, float kappa_low,
                               float kappa_high, int32_t iters, float empty, double *kernel_ms);
/* A stack of any length, chunk after chunk (extension; DESIGN.md section 7 row 20, restated in numpy by
 * tests/stack_accum_ref.py; kernels in csrc/k_stack_accum.hpp).  The caller owns per-pixel running sums on the device; every call
 * adds one chunk of frames to them, a last call turns them into mean and variance.  Device memory is one chunk of frames plus 16
 * to 24 bytes per output pixel, whatever the length of the stack.
 * siftmi_batch_stack_accum  warps n float32 frames as siftmi_batch_stack_ex does (v_s, live_s; `interp` as there) and adds them
 *                         into the state planes in one launch (stack_accum_kernel).  Per output pixel o, one rounding per
 *                         operation:
 *                           clip    given when `center` and `var` are not null: m = center[o], tl = (kappa_low * kappa_low) * var[o],
 *                                   th = (kappa_high * kappa_high) * var[o], all binary32
 *                           for s ascending, live frames only:
 *                             coverage[o] += 1
 *                             clip:  d = v_s - m; q = d * d; rejected = (d < 0 && q > tl) || (d > 0 && q > th)      (binary32)
 *                             not rejected:  s1[o] = s1[o] + (double)v_s;  s2[o] = s2[o] + (double)v_s * (double)v_s (the product
 *                                   is exact in binary64);  kept[o] += 1
 *                         A NaN in the sample, the centre, the variance or a threshold (inf * 0) makes the comparisons false:
 *                         nothing is rejected -- a pixel that a first pass left `empty` = NaN rejects nothing.  var[o] == 0 with
 *                         finite kappas rejects every sample that differs from the centre; kappa = +inf switches its side off.
 *                         This is siftmi_batch_stack_clip's SIGMA rule with the statistics supplied from outside: a second pass
 *                         over the frames with the first pass's mean and variance is a sigma clip of a stack of any length.
 *                         Any split of a stack into calls gives the same state bit for bit.
 *   images, maps, fills, mode, interp   as for siftmi_batch_stack_ex (host frames staged the same way)
 *   s1, s2       OH x OW binary64, device; s2 may be NULL (no second moments: no variance later)
 *   coverage, kept   OH x OW int32, device.  All state planes are contiguous, owned by the caller and zero-filled by the caller
 *                before the first call
 *   center, var  OH x OW float32, device, both or neither
 *   kernel_ms    optional, hipEvent duration of the launch (0 when nothing is launched)
 * siftmi_batch_stack_accum_result   one launch (stack_accum_result_kernel), per pixel: k = kept[o]; k == 0: mean = var = `empty`;
 *                         else M = s1[o] / (double)k; mean = (float)M; V = s2[o] / (double)k - M * M; var = (float)(V < 0 ? 0 : V).
 *                         The population variance, as the SIGMA rule's q / n; no square root is taken, the clip takes the variance.
 *   s1, s2, kept  the state, device; s2 may be NULL when `var` is
 *   mean, var    OH x OW float32, host (staged in the batch's buffer, the variance behind the mean) or device (out_is_device);
 *                var may be NULL
 * Each call is one launch and one synchronisation.  The state, `center` and `var` are device pointers, ordered after the caller's
 * streams as everywhere: both calls synchronise the device once on entry.  n_images == 0 or an empty output launches nothing,
 * leaves the state untouched and returns 0.  SIFTMI_EINVAL, nothing launched and nothing written: everything
 * siftmi_batch_stack_ex refuses about the handle, frames, tables, shape and sampler (a batch created for RGB8 and
 * SIFTMI_INTERP_CUBIC with mode != 1 included); a null s1, coverage, kept or mean with work to do; exactly one of `center` and `var`
 * null; with a clip, a kappa that is NaN or <= 0; `var` asked of the result with s2 null. */
int siftmi_batch_stack_accum(siftmi_batch *batch, const void *const *images, int32_t n_images, int32_t images_are_device,
                             double *s1, double *s2 /* may be null */, int32_t *coverage, int32_t *kept,
                             int32_t out_width, int32_t out_height, const float *maps /* n x 6 */, const float *fills /* n */,
                             int32_t mode, int32_t interp, const float *center /* device, or null */,
                             const float *var /* device; null iff center is */, float kappa_low, float kappa_high, double *kernel_ms);
int siftmi_batch_stack_accum_result(siftmi_batch *batch, const double *s1, const double *s2 /* may be null */, const int32_t *kept,
                                    int32_t out_width, int32_t out_height, float *mean, float *var /* may be null; needs s2 */,
                                    int32_t out_is_device, float empty, double *kernel_ms);

/* ---- MatchPlan -----------------------------------------------------------------------------
 * siftmi_match_create <- MatchPlan.__init__ (match.py:77-139)
 * siftmi_match        <- MatchPlan.match (match.py:200-271) with the `matching` kernel
 *                        (matching_cpu.cl:57-109): L1 distance, best/second-best, ratio test
 *                        dist1/dist2 < ratio_th.  *n_out = pairs written (<= capacity); *n_total = pairs
 *                        that passed (the reference silently drops the excess, match.py:252).  The device keeps
 *                        at most `size` pairs of a call; a call with min(n1, n2) > size raises the matcher's
 *                        size to it for good, as the reference's kpsize grows (match.py:241-243).
 */
int siftmi_match_create(int64_t size, int32_t device_id, int32_t profile, siftmi_matcher **out);
int siftmi_match(siftmi_matcher *plan, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                 const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, float ratio_th,
                 int32_t *pairs, int64_t capacity, int64_t *n_out, int64_t *n_total);
/* ROI-masked and mutual-best variants.
 * siftmi_match_set_roi <- MatchPlan.set_roi / unset_roi (match.py:312-327): uploads the int8 mask (roi = NULL unsets).
 * siftmi_match_ex      <- the `matching_valid` kernel (matching_cpu.cl:136-199), which the reference compiles but its
 *                         host code never launches (match.py:246 always calls `matching`).
 *   roi_mode 0  no mask (== siftmi_match)
 *   roi_mode 1  `matching_valid` literally: a list-1 keypoint is dropped iff it lies inside the mask array on a zero
 *               pixel; a list-2 keypoint that is not inside the array on a non-zero pixel keeps competing with
 *               distance 0 (the kernel guards the accumulation, not the candidate); (c, r) = (int)x, (int)y
 *   roi_mode 2  strict (extension): keypoints of either list that are not on a non-zero mask pixel do not take part
 *   mutual      (extension) keep (i, j) only if i is also the nearest list-1 keypoint of j over the same masked
 *               distances, ties to the smallest index */
int siftmi_match_set_roi(siftmi_matcher *m, const int8_t *roi, int32_t roi_width, int32_t roi_height);
int siftmi_match_ex(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                    const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, float ratio_th, int32_t roi_mode,
                    int32_t mutual, int32_t *pairs, int64_t capacity, int64_t *n_out, int64_t *n_total);
/* Windowed matching (extension; DESIGN.md section 7 row 6, restated in numpy by tests/window_ref.py): the rule of `matching`
 * (matching_cpu.cl:57-109) applied only to the CANDIDATES of a list-1 keypoint i, the list-2 keypoints j with
 *     fabsf((x2[j] - x1[i]) - sx) <= wx  &&  fabsf((y2[j] - y1[i]) - sy) <= wy          (f32, unfused; a NaN makes it false)
 * taken in ascending j: strict '<' (the earliest index of the minimum wins, dist2 is the second smallest of the multiset),
 * pair kept iff dist2 != 0 && dist1 / dist2 < ratio_th with both distances starting at 1e12f.  A keypoint without a candidate
 * pairs with nothing; a keypoint with exactly one candidate always pairs with it.  wx / wy may be +inf (every finite
 * difference is admitted: with a zero shift and finite coordinates the result is siftmi_match's).
 *   mutual       keep (i, j) only if i is also the nearest candidate of j (same predicate, same operand order), ties to the
 *                smallest i
 * Capacity, SIFTMI_ECAPACITY, *n_out / *n_total, siftmi_match_last_kernel_ms (all kernels of the call, the binning of the
 * lists included) and the four siftmi_match_last_stage_ms slots (binning counts as "matching") as for siftmi_match_ex; both
 * lists are used where they lie.  The region of interest is not consulted.  n1 == 0 or n2 == 0: no pair, SIFTMI_OK.
 * SIFTMI_EINVAL, nothing launched: a negative or NaN window, a shift that is not finite, a null list with a non-zero count,
 * a negative count. */
int siftmi_match_window(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                        const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, float ratio_th, float wx, float wy,
                        float sx, float sy, int32_t mutual, int32_t *pairs, int64_t capacity, int64_t *n_out, int64_t *n_total);
/* k nearest neighbours WITH their descriptor distances (extension; DESIGN.md section 7 row 7, restated in numpy by tests/knn_ref.py).
 * d(i, j) is the int32 L1 distance over the 128 descriptor bytes (0 .. 32 640).  Row i of the result holds the k smallest elements
 * of {(d(i, j), j) : 0 <= j < n2} in ascending lexicographic order of (distance, index): among equal distances the smaller index
 * comes first.  idx_out[i * k + r] is the index and dist_out[i * k + r] the distance; where n2 < k the remaining slots hold -1 / -1.
 * The order is total: the result does not depend on partitioning or scheduling.  Positions, the region of interest and the ratio
 * play no part.  idx[, 0], dist[, 0], dist[, 1] are the best / dist1 / dist2 of `matching` (matching_cpu.cl:57-109).
 *   k            1 .. 8
 *   idx_out, dist_out   host, n1 * k int32 each
 * Both lists are used where they lie (host lists are staged).  n1 == 0 writes nothing, n2 == 0 writes -1 everywhere; neither
 * launches anything.  The call leaves the matcher's pair capacity (`size`) alone.  siftmi_match_last_kernel_ms then reports the two
 * knn kernels and siftmi_match_last_stage_ms the call's stages: [0], [1] the list copies, [2] the kernels, [3] the copy of the result.
 * SIFTMI_EINVAL, nothing written, nothing launched: k outside 1 .. 8, a negative count, a null list or result buffer with a
 * non-zero count. */
int siftmi_match_knn(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                     const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t k,
                     int32_t *idx_out, int32_t *dist_out);
/* siftmi_match_knn with the descriptor distance of the caller's choice (tests/knn_l2_ref.py).
 *   metric       SIFTMI_METRIC_L1: siftmi_match_knn, bit for bit (it is this entry with metric 0).
 *                SIFTMI_METRIC_L2SQ: d(i, j) is the SQUARED Euclidean distance, the sum over the 128 descriptor bytes of
 *                (a - b)^2 as integers, 0 .. 8 323 200 (= 128 * 255^2), as int32; no square root is taken.  Everything else --
 *                the order of a row, the padding, the empty lists, the stage times, the errors -- is siftmi_match_knn's.  The ratio
 *                test on these distances with ratio^2 is Lowe's test on Euclidean distances with the ratio itself.
 * SIFTMI_EINVAL, nothing written, nothing launched: a metric other than the two constants, and siftmi_match_knn's. */
#define SIFTMI_METRIC_L1 0
#define SIFTMI_METRIC_L2SQ 1
int siftmi_match_knn_metric(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                            const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t k, int32_t metric,
                            int32_t *idx_out, int32_t *dist_out);
/* siftmi_match_knn_metric over the CANDIDATES of a query only (extension; DESIGN.md section 7 row 10, restated in numpy by
 * tests/knn_window_ref.py).  List-2 keypoint j is a candidate of list-1 keypoint i iff siftmi_match_window's predicate holds,
 * fabsf((x2[j] - x1[i]) - sx) <= wx && fabsf((y2[j] - y1[i]) - sy) <= wy in f32, every operation rounded on its own (a NaN makes
 * it false; wx / wy may be +inf).  Row i of the result holds the k smallest elements of {(d(i, j), j) : j a candidate of i} in
 * ascending lexicographic order of (distance, index), d being the distance of `metric`; where i has fewer than k candidates (none
 * included) the remaining slots hold -1 / -1.  The order is total: the result does not depend on the binning of the lists, on
 * the order inside a cell or on scheduling.  The ratio, the region of interest and the matcher's pair capacity (`size`) play no
 * part and are left alone.  With an infinite window, a zero shift and finite coordinates the result is siftmi_match_knn_metric's;
 * exchanging the lists and negating the shift ranks the candidates of every list-2 keypoint among list 1.
 * Both lists are used where they lie (host lists are staged).  n1 == 0 writes nothing, n2 == 0 writes -1 everywhere; neither
 * launches anything.  siftmi_match_last_kernel_ms reports all kernels of the call, the binning of the lists included, and
 * siftmi_match_last_stage_ms the call's stages as for siftmi_match_knn.
 * SIFTMI_EINVAL, nothing written, nothing launched: siftmi_match_knn_metric's (k, metric, counts, null pointers), a count above
 * 2^28 - 1, a negative or NaN window, a shift that is not finite. */
int siftmi_match_knn_window(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                            const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t k, int32_t metric,
                            float wx, float wy, float sx, float sy, int32_t *idx_out, int32_t *dist_out);
/* Consensus filter over the pairs of a match (no reference counterpart: the reference hands this to the third-party
 * feature.sift_orsa, sift-src/alignment.py:54-57, 260-264).  n_hyp affine maps are solved from pseudo-random triples of matches,
 * every match votes for every map that brings its list-1 position within `tol` pixels of its list-2 position, the map with most
 * votes wins (ties: the smallest index) and mask[j] = 1 for its voters.  Deterministic for (inputs, n_hyp, tol, seed) and restated
 * exactly in numpy (tests/consensus_ref.py).  A pair with an index outside its list never votes.
 * Fewer than three pairs, or no triple with |det| >= 1: *winner = -1, the mask all zero, SIFTMI_OK.
 * SIFTMI_EINVAL, nothing launched: n_hyp outside 1..2^20, tol not finite or not > 0, a negative count, a null list, pairs or
 * mask with a non-zero count.
 *   mask         host, n_pairs bytes              model      host, 6 floats (a, b, c, d, e, f): x' = a x + b y + c,
 *   winner       index of the winning map, -1: none          y' = d x + e y + f; untouched without a winner
 *   votes_all    optional, host, n_hyp (test hook)           models_all  optional, host, n_hyp * 6, void rows all NaN (test hook)
 *   kernel_ms    optional: hipEvent time of the vote kernel alone */
int siftmi_match_consensus(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                           const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device,
                           const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device,
                           int32_t n_hyp, float tol, uint32_t seed, uint8_t *mask, float *model, int32_t *winner,
                           int32_t *winner_votes, int32_t *votes_all, float *models_all, double *kernel_ms);
/* Least-squares affine map of the pairs of a match, entirely on the device (no reference counterpart: the reference's
 * utils.matching_correction stops before the solve, sift-src/utils.py:156-189; the host form is utils.affine_least_squares).
 * Pair j is gathered to f32 (x0, y0, x1, y1) as for the consensus filter and is *used* iff (mask == NULL || mask[j] != 0) and all
 * four are finite (an index outside its list gives NaN); the used pairs are fitted in binary64 by centred normal equations: means,
 * seven centred moments, a 2 x 2 solve, the sum of squared residuals of the f64 model.  Every sum is formed in one fixed order
 * (256 lanes per workgroup, `blocks` workgroups, pair j on lane j mod 256 * blocks; lane sums in ascending j, a fixed tree over
 * the lanes, the workgroups in ascending order), every operation rounded once: deterministic for (inputs, blocks) and restated
 * exactly in numpy (tests/fit_ref.py).  Lists, pairs and mask are used where they lie; host ones
 * are staged in the matcher's buffers.  One stream synchronisation and one 160-byte copy back per call.
 * n_pairs == 0: EMPTY, nothing launched.  SIFTMI_EINVAL, nothing launched, nothing written: a null matcher or out, a negative
 * count or one above 2^31 - 1, a null list or null pairs with a non-zero count, blocks outside 0..1024.
 *   mask       optional, n_pairs bytes, non-zero = use the pair (a consensus mask)
 *   blocks     workgroups of the three passes, 1..1024; 0: min(256, max(1, ceil(n_pairs / 256)))
 *   out        host, 20 doubles, all written by every call that returns SIFTMI_OK:
 *              [0] status: 0 OK, 1 EMPTY (no used pair: [1] is 0, the rest NaN), 2 DEGENERATE (n < 3 or
 *                  !(fabs(det) > 1e-12 * fmax(1, Sxx*Syy)), the rule of utils.affine_least_squares: [13..19] NaN)
 *              [1] n, the used pairs      [2..5] the means mx, my, mu, mv of x0, y0, x1, y1
 *              [6..12] Sxx, Sxy, Syy, Sxu, Syu, Sxv, Syv, sums over the used pairs of products of the centred coordinates
 *              [13..18] a, b, c, d, e, f: x' = a x + b y + c, y' = d x + e y + f (the order of siftmi_match_consensus)
 *              [19] ssr, the sum of squared residuals; rms = sqrt(ssr / n)
 *   kernel_ms  optional: hipEvent time from the gather to the last kernel */
int siftmi_match_fit(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                     const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device,
                     const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device,
                     const uint8_t *mask, int32_t mask_is_device, int32_t blocks, double *out, double *kernel_ms);
/* Exact median displacement of the pairs of a match, entirely on the device: the translation-only estimate the reference takes with
 * numpy.median on the host (sift-src/alignment.py:268-271).  Pair j is gathered and *used* as for siftmi_match_fit; its
 * displacement is dx = x1 - x0, dy = y1 - y0 in f32 (+-inf from an overflow takes part).  Per axis, with n used pairs, lo and hi are
 * the values of rank (n - 1) >> 1 and n >> 1 in the total order of f32 (-inf first, -0.0 < +0.0), found by a radix select with
 * integer counters only, and the median is lo for odd n and (lo + hi) * 0.5f for even n: numpy.median's value, bit for bit up to
 * the sign of a zero, for every grid (tests/shift_ref.py restates it in numpy).  Lists, pairs and mask
 * are used where they lie; host ones are staged in the matcher's buffers.  One stream synchronisation per call.
 * n_pairs == 0: EMPTY, nothing launched.  SIFTMI_EINVAL, nothing launched, nothing written: a null matcher, out or counts, a
 * negative count or one above 2^31 - 1, a null list or null pairs with a non-zero count, blocks outside 0..1024, and with a
 * keep mask a tol that is NaN or negative.
 *   mask       optional, n_pairs bytes, non-zero = use the pair (a consensus mask)
 *   blocks     workgroups of the kernels that walk the pairs, 1..1024; 0: siftmi_match_fit's rule.  The result does not depend on it
 *   tol, keep  keep: optional, host, n_pairs bytes: keep[j] = 1 iff pair j is used, both medians are finite and
 *              fabsf(dx - mdx) <= tol && fabsf(dy - mdy) <= tol in f32 (tol may be +inf), else 0; tol is ignored without keep
 *   out        host, 6 floats: mdx, mdy, lo_dx, hi_dx, lo_dy, hi_dy; all NaN when no pair is used (EMPTY)
 *   counts     host, 2: n, the used pairs, and n_keep, the kept pairs (0 without keep)
 *   kernel_ms  optional: hipEvent time from the gather to the last kernel */
int siftmi_match_shift(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                       const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device,
                       const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device,
                       const uint8_t *mask, int32_t mask_is_device, int32_t blocks,
                       float tol, uint8_t *keep, float *out, int64_t *counts, double *kernel_ms);
/* siftmi_match over a batch of S segment pairs in one set of launches and one stream synchronisation (extension; DESIGN.md section 7
 * row 12, restated in numpy by tests/match_batch_ref.py).  kp2 holds the records of S lists back to back, counts2[s] of them in
 * segment s; kp1 likewise with counts1, or, with counts1 == NULL, ONE list of n1 records that every segment is matched against.
 * Segment s gets the rule of `matching` (matching_cpu.cl:57-109) on its own two lists: ascending j, strict '<' (the earliest index of
 * the minimum wins, dist2 is the second smallest of the multiset), pair kept iff dist2 != 0 && dist1 / dist2 < ratio_th in f32 with
 * both distances starting at 1e12f -- siftmi_match_ex with roi_mode 0 on the two segments.  Indices are local to the segment.
 * The pairs of segment s are the rows [sum(pair_counts[0..s)), + pair_counts[s]) of `pairs`, in ascending i: the order is fixed
 * (a query gives at most one pair), and the result does not depend on part_len or on scheduling.  A segment with an empty list on
 * either side gives no pair; one whose second list has one element pairs every query with it.
 *   mutual       keep (i, j) only if i is also the nearest element of segment s's first list to j, ties to the smallest i
 *                (siftmi_match_ex's rule); with a shared first list, the nearest of the whole list
 *   part_len     elements of a second-list segment per partition of the scan: 0 (chosen so that the whole batch gives about 2048
 *                workgroups) or a multiple of 64 up to 65 472 (test hook)
 *   pairs        room for one row of 2 int32 per query of the first side: n1 rows, or n_segments * n1 with a shared list; host, or
 *                device (pairs_is_device: the rows are written where they lie and nothing but pair_counts comes back)
 *   pair_counts  host, n_segments int64, written by every call that returns SIFTMI_OK
 * Both lists are used where they lie (host lists are staged).  The region of interest plays no part and the matcher's pair
 * capacity (`size`) is left alone.  When no segment has an element on both sides nothing is launched.
 * siftmi_match_last_kernel_ms reports all kernels of the call, siftmi_match_last_stage_ms its stages as for siftmi_match.
 * SIFTMI_EINVAL, nothing launched: n_segments outside 0 .. 65 535, a negative count, counts that do not add up to n1 / n2, a
 * ratio_th that is not <= 1 (above 1 the rule pairs a query without a candidate with index 0), a part_len that is not as above,
 * a null list, counts2, pair_counts or pairs where it is needed, more than 2^31 - 1 queries, or more work than the tables hold
 * (2^22 workgroups a direction, 2^31 - 1 partial results). */
int siftmi_match_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                       const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                       const int64_t *counts1, const int64_t *counts2, float ratio_th, int32_t mutual, int32_t part_len,
                       int32_t *pairs, int32_t pairs_is_device, int64_t *pair_counts);
/* siftmi_match_window for S segment pairs in one set of launches and one stream synchronisation (extension; DESIGN.md section 7
 * row 16, restated in numpy by tests/match_window_batch_ref.py).  The lists, n_segments, counts1 (NULL: one shared first list),
 * counts2, pairs, pairs_is_device and pair_counts are siftmi_match_batch's, and so is the result's layout: the pairs of segment s
 * are the rows [sum(pair_counts[0..s)), + pair_counts[s]) of `pairs`, indices local to the segment, in ascending i.  Segment s gets
 * siftmi_match_window's rule on its own two lists with its own shift: exactly the set of pairs of that call on the segment's
 * slices.  The result does not depend on grid_max, on scheduling or on the records of other segments.  A segment with an empty
 * list on either side gives no pair; a query with exactly one candidate always pairs with it.
 *   wx, wy       half widths of the window, >= 0; +inf is allowed
 *   shifts       host, 2 * n_segments floats: (sx, sy) of every segment, finite
 *   mutual       keep (i, j) only if i is also the nearest candidate of j inside segment s (the same predicate, same operand
 *                order), ties to the smallest i
 *   grid_max     0 (the library chooses: 256) or 1 .. 256, the most cells per axis of any segment's grid (test hook)
 * Both lists are used where they lie (host lists are staged).  The region of interest plays no part and the matcher's pair
 * capacity (`size`) is left alone.  When no segment has an element on both sides nothing is launched.
 * siftmi_match_last_kernel_ms reports all kernels of the call, siftmi_match_last_stage_ms its stages as for siftmi_match_batch.
 * SIFTMI_EINVAL, nothing launched, nothing written: a null matcher, n_segments outside 0 .. 65 535, a negative count, counts that do
 * not add up to n1 / n2, a ratio_th that is not <= 1, a negative or NaN window, a shift that is not finite, grid_max outside
 * 0 .. 256, a null list, counts2, shifts, pair_counts or pairs where it is needed, more than 2^28 - 1 records on a side or
 * queries in all, or more work than the tables hold (2^30 work items a direction). */
int siftmi_match_window_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                              const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                              const int64_t *counts1, const int64_t *counts2, float ratio_th, float wx, float wy, const float *shifts,
                              int32_t mutual, int32_t grid_max, int32_t *pairs, int32_t pairs_is_device, int64_t *pair_counts);
/* siftmi_match_fit for every segment of a batch in one set of launches and one stream synchronisation (extension; DESIGN.md
 * section 7 row 13, restated by tests/estimate_batch_ref.py).  The lists, n_segments, counts1 (NULL: one shared first list) and
 * counts2 are siftmi_match_batch's arguments and `pairs` / `pair_counts` its results, unchanged: the pairs of segment s are the rows
 * [sum(pair_counts[0..s)), + pair_counts[s]) with indices local to the segment.  Row r of segment s with (i, j) reads record
 * off1_s + i of kp1 iff 0 <= i < counts1[s] (shared list: off1_s = 0, the count is n1) and record off2_s + j of kp2 iff
 * 0 <= j < counts2[s]; otherwise it is four NaN and unused, so a record of a neighbouring segment is never read.  Segment s then gets
 * siftmi_match_fit's arithmetic with pair index = the row's position inside the segment, B_s = blocks, or with blocks == 0
 * min(256, max(1, ceil(pair_counts[s] / 256))), workgroups: the 20 doubles are bit for bit those of siftmi_match_fit on the
 * segment's own lists, pairs, mask slice and `blocks`.  A segment without a pair is EMPTY and gets no workgroup.
 * sum(pair_counts) == 0 (n_segments == 0 included): nothing launched, *kernel_ms = 0.  Lists, pairs and mask are used where they lie;
 * host ones are staged.  SIFTMI_EINVAL, nothing launched, nothing written: a null matcher, n_segments outside 0 .. 65 535, a negative
 * count, a count above 2^31 - 1, counts that do not add up to n1 / n2, pair_counts that do not add up to n_pairs, blocks outside
 * 0..1024, more than 2^20 workgroups in all, a null list, pairs, counts2, pair_counts or out where it is needed.
 *   mask       optional, n_pairs bytes aligned with the rows of `pairs`, non-zero = use the pair
 *   out        host, n_segments * 20 doubles in siftmi_match_fit's order, all written by every call that returns SIFTMI_OK
 *   kernel_ms  optional: hipEvent time from the first kernel to the last */
int siftmi_match_fit_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                           const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                           const int64_t *counts1, const int64_t *counts2,
                           const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device, const int64_t *pair_counts,
                           const uint8_t *mask, int32_t mask_is_device, int32_t blocks, double *out, double *kernel_ms);
/* siftmi_match_shift for every segment of a batch in one launch and one stream synchronisation.
 * Arguments, gather rule, empty batches and errors as for siftmi_match_fit_batch; there is no `blocks`: one workgroup selects the
 * medians of one segment, and a median does not depend on the launch shape.  The results of segment s are bit for bit those of
 * siftmi_match_shift on the segment's own lists, pairs and mask slice.  Also SIFTMI_EINVAL: a null out or counts with a segment,
 * and with a keep mask a tol that is NaN or negative.
 *   tol, keep  keep: optional, host, n_pairs bytes: siftmi_match_shift's rule with every row tested against the medians of its own
 *              segment (a segment whose median is not finite keeps nothing); tol is ignored without keep
 *   out        host, n_segments * 6 floats: mdx, mdy, lo_dx, hi_dx, lo_dy, hi_dy per segment; NaN where no pair is used
 *   counts     host, n_segments * 2 int64: n and n_keep (0 without keep) per segment
 *   kernel_ms  optional: hipEvent time of the kernel */
int siftmi_match_shift_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                             const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                             const int64_t *counts1, const int64_t *counts2,
                             const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device, const int64_t *pair_counts,
                             const uint8_t *mask, int32_t mask_is_device, float tol, uint8_t *keep, float *out, int64_t *counts,
                             double *kernel_ms);
/* siftmi_match_consensus for every segment of a batch in one set of launches and one stream synchronisation (extension; DESIGN.md
 * section 7 row 14, restated by tests/consensus_batch_ref.py).  The lists, n_segments, counts1 (NULL: one shared first list), counts2,
 * pairs and pair_counts, and the gather rule -- an index outside its own segment's list gives four NaN, a record of a neighbouring
 * segment is never read -- are siftmi_match_fit_batch's; n_hyp, tol and seed are siftmi_match_consensus's and hold for every segment.
 * Segment s samples its triples mod pair_counts[s] with the row's position inside the segment as the pair index, and its mask rows,
 * model, winner, votes and the rows of the two test hooks are bit for bit those of siftmi_match_consensus on the segment's own lists
 * and pairs.  A segment with fewer than three pairs, or with no triple with |det| >= 1, has no winner: winner -1, 0 votes, a NaN
 * model, its mask rows zero.  When no segment has three pairs (n_segments == 0 included) nothing is launched, *kernel_ms = 0, the
 * mask is zeroed where it lies and every per-segment result is filled on the host.  Lists and pairs are used where they lie; host
 * ones are staged.  One stream synchronisation per call, one copy back for the per-segment results and one for the mask only when
 * it is a host mask.
 * SIFTMI_EINVAL, nothing launched, nothing written: siftmi_match_fit_batch's (a null matcher, n_segments outside 0 .. 65 535, a
 * negative count, a count above 2^31 - 1, counts that do not add up to n1 / n2, pair_counts that do not add up to n_pairs, a null
 * list, pairs, counts2 or pair_counts where it is needed), n_hyp outside 1..2^20, tol not finite or not > 0, a null mask with a
 * pair, null models, winners or winner_votes with a segment, (segments of three pairs or more) * n_hyp above 2^22 (their models,
 * votes and flags live in the matcher's buffers, about 120 MB at the limit), more than 2^20 tiles in all (a tile: up to 1024 rows
 * of one segment).
 *   mask          n_pairs bytes aligned with the rows of `pairs`, every byte written: host, or device (mask_is_device: written where
 *                 it lies, it goes into siftmi_match_fit_batch / siftmi_match_shift_batch as it is and no mask comes back)
 *   models        host, n_segments * 6 floats (a, b, c, d, e, f); NaN where the segment has no winner
 *   winners       host, n_segments: index of the winning map, -1: none      winner_votes  host, n_segments: its votes, 0 without
 *   votes_all     optional, host, n_segments * n_hyp (test hook)            models_all    optional, host, n_segments * n_hyp * 6,
 *                 void rows all NaN; a segment with fewer than three pairs: 0 / NaN, as the single call fills them (test hook)
 *   kernel_ms     optional: hipEvent time of the vote kernel alone */
int siftmi_match_consensus_batch(siftmi_matcher *m, const siftmi_keypoint *kp1, int64_t n1, int32_t kp1_is_device,
                                 const siftmi_keypoint *kp2, int64_t n2, int32_t kp2_is_device, int32_t n_segments,
                                 const int64_t *counts1, const int64_t *counts2,
                                 const int32_t *pairs, int64_t n_pairs, int32_t pairs_is_device, const int64_t *pair_counts,
                                 int32_t n_hyp, float tol, uint32_t seed,
                                 uint8_t *mask, int32_t mask_is_device,
                                 float *models, int32_t *winners, int32_t *winner_votes,
                                 int32_t *votes_all, float *models_all,
                                 double *kernel_ms);
int siftmi_match_last_kernel_ms(const siftmi_matcher *plan, float *ms);
/* profile != 0 at creation: device time in ms of the last call's stages, in the order of the events the reference
 * appends under profile=True (sift-src/match.py:226-263): ms4[0] "copy H->D KP_1", [1] "copy H->D KP_2", [2] "matching",
 * [3] "copy D->H match"; -1 where the stage did not run (device-resident list, no pair to copy). */
int siftmi_match_last_stage_ms(const siftmi_matcher *plan, float *ms4);
int siftmi_match_destroy(siftmi_matcher *plan);

/* ---- per-stage entry points (host pointers in/out; golden-vector replay, one reference kernel each; the *_ex ones
 * launch a plan's own forms of a stage with its launch choices exposed: blur_ex, detect_ex, orientation_ex, descriptor_ex)
 * gaussian.cl:56 | reductions.cl:62-241 + preprocess.cl:239 | convolution.cl:16,62 | algebra.cl:18 |
 * image.cl:119 | image.cl:235 + algebra.cl:57 | image.cl:47 | orientation_cpu.cl:41 |
 * keypoints_cpu.cl:36 | preprocess.cl:267 | preprocess.cl:53-223 */
int siftmi_stage_gaussian_taps(float sigma, int32_t size, float *out);
/* (host only, no reference counterpart) position of workgroup `id` of a grid of `n` in the XCD-contiguous order the marching
 * blur and the extrema pass use (csrc/k_xcd.hpp): the tile it works on.  A bijection of [0, n) for every n. */
int32_t siftmi_stage_xcd_order(int32_t id, int32_t n);
int siftmi_stage_minmax_normalize(int32_t device_id, const float *in, float *out, int32_t W, int32_t H,
                                  float *min_out, float *max_out);
int siftmi_stage_blur(int32_t device_id, const float *in, float *out, int32_t W, int32_t H,
                      const float *taps, int32_t ntaps);
/* the same stage with a plan's launch choices exposed (test hook for the large-plane kernels): `in` holds a frame of
 * `in_dtype` (SIFTMI_F32, or an integer / RGB8 code: those enter through the normalising 15-tap blur only, as in a plan);
 * norm != 0: min/max of the frame first (reductions.cl:62-241), then the blur with `normalizes` (preprocess.cl:239-252)
 * applied to its inputs; xcd_map: bit 0 = workgroup order of the marching kernel (option "xcd_map"), bit 1 set = its priority
 * feedback off (option "march_prio" 0), bits 2-3 = the small-plane blur form plus one (0: the default rule, 1: 32 x 16 tile kernel,
 * 2: 32 x 32 / 32 x 64 tile kernel, 3: by plane size); march_wgs: its workgroup count (0: default);
 * *kernel_used (may be null): 0 generic two-pass, 1 tiled kernel, 2 marching team kernel, 3 32 x 32 / 32 x 64 tile kernel -- the kernel
 * that was launched. */
int siftmi_stage_blur_ex(int32_t device_id, const void *in, int32_t in_dtype, float *out, int32_t W, int32_t H,
                         const float *taps, int32_t ntaps, int32_t norm, int32_t xcd_map, int32_t march_wgs,
                         int32_t *kernel_used);
/* the f32, non-normalising blur with the fused octave hand-off (test hook: the launch a plan makes for plane 3 of an octave,
 * which also writes out[2y][2x] to plane 0 of the next one, preprocess.cl:267-285).  xcd_map, march_wgs and *kernel_used as
 * in siftmi_stage_blur_ex (bits 2-3 of xcd_map pick the small-plane form).  half: SIFTMI_STAGE_GUARD + (W/2)*(H/2) +
 * SIFTMI_STAGE_GUARD floats; the device buffer is filled with 0xa5 bytes before the launch and returned whole, and the kernel
 * is given the address behind the first guard: a sample no workgroup wrote, or a write outside the half plane, shows.  A tap
 * count without a fused kernel runs the generic two-pass blur, which hands nothing off: `half` comes back as filled and
 * *kernel_used is 0.  SIFTMI_EINVAL, nothing launched, for a null pointer, an empty plane or ntaps outside 1..64. */
int siftmi_stage_blur_handoff(int32_t device_id, const float *in, float *out, float *half, int32_t W, int32_t H,
                              const float *taps, int32_t ntaps, int32_t xcd_map, int32_t march_wgs, int32_t *kernel_used);
int siftmi_stage_dog(int32_t device_id, const float *blur_a, const float *blur_b, float *out, int64_t n);
/* blurs: 6 planes (H,W); out: (capacity,4) floats (peak,row,col,scale) for scales 1..3 */
int siftmi_stage_local_maxmin(int32_t device_id, const float *blurs, int32_t W, int32_t H, int32_t octsize,
                              const siftmi_params *params, float *out, int64_t capacity, int64_t *n_out);
/* candidates (n,4) -> refined (peak,row,col,sigma) + detection scale, holes removed */
int siftmi_stage_interp(int32_t device_id, const float *blurs, int32_t W, int32_t H, const float *cand, int64_t n,
                        const siftmi_params *params, float *out, int32_t *out_scale, int64_t *n_out);
/* The two stages above with a plan's launch choices exposed (test hook: both forms of the extrema kernel, its strip
 * geometry, the band arguments, lists cut at their capacity).  Extra arguments:
 *   form           0: extrema_kernel<false> fills the candidate list, then refine_kernel runs on the device-side list, as a
 *                  plan chains them; 1: extrema_kernel<true>, the fused form (no candidate list: `cand` keeps its fill).
 *   rows           rows of a strip (0: by the plan's size rule); xcd_map: workgroup order (option "xcd_map")
 *   y_lo, y_hi     rows [y_lo, y_hi) of the detection area [border_dist, H - border_dist) only; y_lo = -1: all of it
 *   cand_capacity  slots of the candidate list the kernels are told of; kp_capacity: those of the refined list.  Each list
 *                  is followed by SIFTMI_STAGE_GUARD more slots the kernels are not told of, returned with it.
 *   cand           (cand_capacity + guard, 4) candidates (value, row, col, scale), form 0
 *   kp, kp_aux     (kp_capacity + guard, 4) refined (peak, row, col, sigma) and as many words: detection scale | octave << 8
 *   counters       5 raw device counters, not cut at a capacity: candidates appended (form 0; 0 in form 1), refined keypoints
 *                  appended, candidates read by the refinement per detection scale 1, 2, 3 (what the capacity rule is
 *                  evaluated from; in form 0 those of the candidates that were stored).
 * The lists are filled before the launch and returned whole -- the candidates with -1.0f (holes, the reference's fill: the
 * refinement skips them), the refined lists with 0xa5 bytes: a slot beyond a counter, beyond what a cut list holds, or one a
 * kernel reserved and did not write, comes back as the fill.  A plane with W or H <= 2 * border_dist launches nothing.
 * SIFTMI_EINVAL, nothing launched, for an unknown form, rows outside 0..4096, an octsize that is no power of two,
 * border_dist < 1 or a band that is empty or not inside the detection area. */
#define SIFTMI_STAGE_GUARD 64
int siftmi_stage_detect_ex(int32_t device_id, const float *blurs, int32_t W, int32_t H, int32_t octsize,
                           const siftmi_params *params, int32_t form, int32_t rows, int32_t xcd_map, int32_t y_lo, int32_t y_hi,
                           int64_t cand_capacity, int64_t kp_capacity, float *cand, float *kp, int32_t *kp_aux,
                           int32_t *counters);
/* The lazy detection chain of a plan (siftmi_plan_set_lazy_top) on five planes: the extrema launch that does not read plane 5 (scale 3
 * against 18 neighbours: provisional candidates), top_patch_kernel (plane 5 from plane 4 with `top_taps` on the 13 x 13 patch
 * around every provisional candidate, clipped to the plane; a candidate whose DoG4 3 x 3 holds a sample beyond it becomes a
 * hole, four times -1.0f), then the refinement launch.
 *   blurs5         (5, H, W) planes 0..4
 *   top_taps       n_taps (1..64) taps of the blur from plane 4 to plane 5
 *   rows .. kp_aux as siftmi_stage_detect_ex (form 0); `cand` comes back with the holes in it
 *   counters       as siftmi_stage_detect_ex; counters[0] counts the provisional entries too
 *   plane5         (H, W) the plane-5 buffer of the run: every float was SIFTMI_STAGE_TOP_FILL (a quiet NaN with a payload)
 *                  before the launches, so the samples no patch covers come back as the fill, and a refinement read outside
 *                  the patches would have turned a peak into NaN. */
#define SIFTMI_STAGE_TOP_FILL 0x7fc5a5a5u
int siftmi_stage_detect_lazy(int32_t device_id, const float *blurs5, const float *top_taps, int32_t n_taps, int32_t W, int32_t H,
                             int32_t octsize, const siftmi_params *params, int32_t rows, int32_t xcd_map, int32_t y_lo, int32_t y_hi,
                             int64_t cand_capacity, int64_t kp_capacity, float *cand, float *kp, int32_t *kp_aux,
                             int32_t *counters, float *plane5);
/* `compact` (openCL/algebra.cl:57-84, host side plan.py:758-795): rows [start, end) of kps (n,4) whose row field is not
 * -1 are moved up to follow the first `start` rows; out receives *n_out rows (start + survivors), survivors unordered */
int siftmi_stage_compact(int32_t device_id, const float *kps, int64_t n, int64_t start, int64_t end, float *out, int64_t *n_out);
int siftmi_stage_gradient(int32_t device_id, const float *img, float *grad, float *ori, int32_t W, int32_t H);
/* refined (n,4)+scale -> oriented (x,y,sigma*oct,angle)+scale, extras appended (capacity rows) */
int siftmi_stage_orientation(int32_t device_id, const float *blurs, int32_t W, int32_t H, int32_t octsize,
                             const float *kps, const int32_t *kp_scale, int64_t n, const siftmi_params *params,
                             float *out, int32_t *out_scale, int64_t capacity, int64_t *n_out);
int siftmi_stage_descriptor(int32_t device_id, const float *blurs, int32_t W, int32_t H, int32_t octsize,
                            const float *kps, const int32_t *kp_scale, int64_t n, uint8_t *desc);
/* The two stages above with a plan's launch choices exposed (test hooks: every form of the per-keypoint kernels).  The
 * entry points above are these with form = 0, blocks = 0.  Extra arguments:
 *   form        orientation: 0 the stage's form (a wave per keypoint), 1 a wave per keypoint, 2 a workgroup per keypoint;
 *               descriptor: 0 the stage's rule (row-interval wave form, the streaming form where a window has R > 127),
 *               1 row-interval, a wave per keypoint, 2 row-interval, a workgroup per keypoint, 3 streaming.
 *               + 4: the MAPS instance (orientation: any form; descriptor: forms 1 and 2 only): the stage first builds the
 *               gradient maps of planes 1..3 with the plan's map kernel, in the plan's layout, and the kernel reads them.
 *   blocks      workgroups of the launch (0: the stage's grid); also passed as the kernel's count-based cuts, so it holds.
 *   *form_used  (may be null) the form the launch selects, + 4 for MAPS (descriptor with n == 0: nothing launched, 0): the
 *               kernel launched, and for the two row forms the kernel's own count rule applied to the arguments it was given
 *               (the kernel does not report the form back).
 * SIFTMI_EINVAL, nothing launched and nothing written, for an unknown form, blocks < 0, MAPS with a detection scale outside
 * 1..3, MAPS with the streaming form, or a row-interval form for a list that holds a window of R > 127. */
int siftmi_stage_orientation_ex(int32_t device_id, const float *blurs, int32_t W, int32_t H, int32_t octsize,
                                const float *kps, const int32_t *kp_scale, int64_t n, const siftmi_params *params,
                                float *out, int32_t *out_scale, int64_t capacity, int64_t *n_out,
                                int32_t form, int32_t blocks, int32_t *form_used);
int siftmi_stage_descriptor_ex(int32_t device_id, const float *blurs, int32_t W, int32_t H, int32_t octsize,
                               const float *kps, const int32_t *kp_scale, int64_t n, uint8_t *desc,
                               int32_t form, int32_t blocks, int32_t *form_used);
/* The gradient-map kernel of the MAPS forms (image.cl:47-80 on planes 1..3 of every octave) over a pyramid of n_oct
 * octaves, octave o of W[o] x H[o] pixels.  planes: six planes per octave, back to back (a plan's plane buffer);
 * gmap / omap: three planes per octave, octave o from float 3 * sum_{p < o} W[p] H[p] (half of its plane offset).
 * Only the octaves [oct_lo, oct_hi) are computed; both maps are uploaded first and read back whole, so the others keep
 * what the caller put there.  blocks: workgroups of the grid stride (0: the plan's default). */
int siftmi_stage_gradient_maps(int32_t device_id, const float *planes, int32_t n_oct, const int32_t *W, const int32_t *H,
                               int32_t oct_lo, int32_t oct_hi, int32_t blocks, float *gmap, float *omap);
int siftmi_stage_shrink(int32_t device_id, const float *in, float *out, int32_t W, int32_t H);
int siftmi_stage_convert(int32_t device_id, const void *in, int32_t in_dtype, float *out, int32_t W, int32_t H);
/* device versions of the "siftmath v1" functions, elementwise over n floats (test hook).  fn: 0 exp, 1 exp2, 2 sin, 3 cos,
 * 4 atan2(a, b); 5 / 6 the fast paths expf_fast(a) / atan2f_fast(a, b); 7 div_by_reciprocal(a, b); 8 the candidate that
 * expf_fast_try returns, usable or not, and 9 its `ok` as 1.0f / 0.0f; 10 / 11 the same of atan2f_fast_try(a, b). */
int siftmi_stage_math(int32_t device_id, int32_t fn, const float *a,
                      const float *b, float *out, int64_t n);

#ifdef __cplusplus
}
#endif
#endif
