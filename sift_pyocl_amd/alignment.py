"""LinearAlign -- register images onto a reference frame with an affine map, on one MI355X.

Drop-in for the reference's ``sift_pyocl.LinearAlign`` (sift-src/alignment.py:76-360): constructor keywords,
the ``align(img, shift_only, return_all, double_check, relative, orsa)`` contract and the keys of the
``return_all`` dictionary are the reference's; the body is this package's own.  Device work per aligned frame:
``SiftPlan.keypoints`` -> ``MatchPlan.match`` (both keypoint lists stay in HBM) -> the affine warp kernel
(the arithmetic of openCL/transform.cl) through ``siftmi_plan_transform`` (include/siftmi.h).  The frame
uploaded for ``keypoints()`` stays staged on the device and is the one the warp reads.

Behavioural notes (deliberate):
  * the affine fit is a float64 least-squares solve (``utils.affine_least_squares``); the reference snapshot's
    ``utils.matching_correction`` stops before solving (utils.py:156-189);
  * the warp writes the whole ``outshape`` (the reference launches one work-item per *input* pixel and leaves
    the ``extra`` margin of its output undefined);
  * ``orsa=True`` needs the third-party ``feature`` module, exactly as in the reference; absent -> warning;
  * ``robust=True`` (extension, off by default) filters the matches with ``MatchPlan.consensus`` on the device before
    the fit: the pairs that agree on one affine map within ``robust_tol`` pixels are kept, the rest never reach it;
  * ``estimate="device"`` (extension, off by default) takes the affine map from ``MatchPlan.fit``: the same centred normal
    equations, summed on the device over the lists where ``match()`` read them, without the host's gathers;
  * ``median="device"`` (extension, off by default) takes every translation-only estimate from ``MatchPlan.shift``: the
    exact median displacement, selected on the device over the same lists, without the host's gathers.
"""
import ctypes as C
import logging
import os
import threading

import numpy

from . import _lib
from .match import MatchPlan, ratio_filter
from .plan import SiftPlan, StageEvent
from .utils import affine_least_squares, matching_correction  # noqa: F401  (matching_correction: reference API)

logger = logging.getLogger("sift.alignment")
try:
    import feature
except ImportError:
    feature = None

#: a fit needs three correspondences per degree of freedom of the affine map (alignment.py:262)
MIN_MATCHES_AFFINE = 3 * 6
#: rejection threshold of ``double_check`` in standard deviations (alignment.py:291-293)
OUTLIER_SIGMAS = 4


def arrow_start(kplist):
    """Tip of the scale/orientation arrow of every keypoint (reference helper, alignment.py:60-67):
    (x + scale*cos(angle), y + scale*sin(angle))."""
    length, theta = kplist.scale, kplist.angle
    return kplist.x + length * numpy.cos(theta), kplist.y + length * numpy.sin(theta)


def transform_pts(matrix, offset, x, y):
    """Apply the (y, x)-ordered affine map of the warp kernel to points (reference helper, alignment.py:70-73).
    Sums are formed in the reference's order so the float results are the same."""
    m = numpy.asarray(matrix)
    new_x = -offset[1] + y * m[1, 0] + x * m[1, 1]
    new_y = -offset[0] + x * m[0, 1] + y * m[0, 0]
    return new_x, new_y


def _as_yx_pair(extra):
    """``extra`` margin as a (y, x) tuple of ints; a scalar applies to both axes"""
    if hasattr(extra, "__len__"):
        return tuple(int(v) for v in extra[:2])
    return (int(extra),) * 2


def _zscore_flags(values, limit=OUTLIER_SIGMAS):
    """1 where a sample lies more than `limit` standard deviations from the mean (NaN z-scores compare False)"""
    with numpy.errstate(divide="ignore", invalid="ignore"):
        return (abs((values - values.mean()) / values.std()) > limit).astype(numpy.int8)


class LinearAlign(object):
    """Align images on a reference image based on an affine transformation (bi-linear + offset)"""

    def __init__(self, image, devicetype="GPU", profile=False, device=None, max_workgroup_size=None,
                 ROI=None, extra=0, context=None, init_sigma=None):
        """
        :param image: reference image on which the other images are aligned (2-D float-able, or H x W x 3 uint8)
        :param devicetype, max_workgroup_size, context: accepted for source compatibility with the reference, unused
        :param profile: collect kernel timings (``log_profile``)
        :param device: HIP device ordinal (default: SIFT_MI355X_DEVICE, LOCAL_RANK or 0)
        :param ROI: boolean mask; reference keypoints outside it are dropped
        :param extra: margin added around the output, an integer or a (y, x) pair
        :param init_sigma: blur width of the initial smoothing (default ``par.InitSigma`` = 1.6)
        """
        ndim = len(image.shape)
        if ndim not in (2, 3):
            raise RuntimeError("Unable to process image of shape %s" % (tuple(image.shape,)))
        self.RGB = ndim == 3
        self.shape = tuple(int(v) for v in image.shape[:2])
        self.extra = _as_yx_pair(extra)
        self.outshape = (self.shape[0] + 2 * self.extra[0], self.shape[1] + 2 * self.extra[1])
        self.profile = bool(profile)
        self.events = []
        self.ref = numpy.ascontiguousarray(image, numpy.float32)
        self.ROI = ROI
        self.ctx = context
        self.devicetype = "GPU"
        self.max_workgroup_size = max_workgroup_size
        if isinstance(device, (tuple, list)):       # the reference's (platform, device) pair: keep the device index
            device = device[-1]
        if device is None:
            device = os.environ.get("SIFT_MI355X_DEVICE", os.environ.get("LOCAL_RANK", 0))
        self.device = int(device)
        self.sift = SiftPlan(template=image, device=self.device, profile=self.profile, init_sigma=init_sigma)
        self.match = MatchPlan(device=self.device, profile=self.profile)
        self.fill_value = 0
        self.sem = threading.Semaphore()
        self.relative_transfo = None
        self.last_transform_ms = 0.0
        self.last_stack_ms = 0.0
        self._ref_dev = None
        self._set_reference(self.sift.keypoints(image))

    # ------------------------------------------------------------------ reference keypoints
    def _set_reference(self, kp):
        """Install `kp` (ROI-filtered) as the reference list and keep a copy resident on the device
        (the reference's buffers["ref_kp_gpu"], alignment.py:155-157)."""
        self.ref_kp = self._mask(kp)
        self._ref_heads = None               # dense (n, 4) copy of (x, y, scale, angle), built on first use
        self._upload_ref()

    def _upload_ref(self):
        """Device copy of the reference keypoints.  torch is only the allocator here: without it, or without a
        visible device, the host list is handed to every match() call instead."""
        self._ref_dev = None
        if not self.ref_kp.size:
            return
        try:
            import torch
            if not torch.cuda.is_available():
                return
            raw = numpy.ascontiguousarray(self.ref_kp).view(numpy.uint8).reshape(-1)
            self._ref_dev = torch.from_numpy(raw.copy()).to("cuda:%d" % self.device)
        except Exception as err:  # noqa: BLE001 -- any allocator problem: fall back to the host list
            logger.debug("reference keypoints stay on the host (%s)", err)
            self._ref_dev = None

    def _mask(self, kp):
        if self.ROI is None:
            return kp
        col = numpy.round(kp.x).astype(numpy.int32)
        row = numpy.round(kp.y).astype(numpy.int32)
        inside = self.ROI[(row, col)].astype(bool)
        logger.warning("Reducing keypoint list from %i to %i because of the ROI" % (kp.size, inside.sum()))
        return kp[inside]

    # ------------------------------------------------------------------ device warp
    def transform(self, matrix, offset, image=None, fill=None, mode=1, interp=None):
        """Affine warp on the device (transform.cl).  image=None warps the image staged by the last keypoints().

        :param interp: (extension) None or ``"linear"``: what `mode` says, the reference's 2 x 2
                       bilinear kernel for ``mode=1``; ``"cubic"``: the Catmull-Rom bicubic sampler (4 x 4 taps, a = -1/2, edge
                       pixels repeated, the same fill region).  Greyscale aligners and ``mode=1`` only: ``ValueError`` otherwise
        """
        interp = _lib.interp_code(interp, mode, self.RGB)
        matrix = numpy.ascontiguousarray(matrix, numpy.float32).reshape(4)
        offset = numpy.ascontiguousarray(offset, numpy.float32).reshape(2)
        if fill is None:
            fill = self.sift.minmax()[0]
        # the result image lives in a pinned block of the library's pool (recycled when the caller drops it): the copy out
        # of HBM runs at the link's rate, and no 64 MB mmap / munmap pair per aligned frame (see SiftPlan.keypoints)
        oshape, odtype = (self.outshape + (3,), numpy.uint8) if self.RGB else (self.outshape, numpy.float32)
        # (sift.pinned_results = False opts out, as for keypoints(); beyond the pool's limit -- _lib.pinned_pool -- the call gets an
        # ordinary array as well: a stack-alignment loop that keeps every aligned frame must not pin the whole stack)
        out = None
        if getattr(self.sift, "pinned_results", True):
            try:
                out = _lib.pinned_empty(int(numpy.prod(oshape)), odtype).reshape(oshape)
            except MemoryError:
                out = None
        if out is None:
            out = numpy.empty(oshape, odtype)
        ptr = None
        if image is not None:
            image = numpy.ascontiguousarray(image, numpy.uint8 if self.RGB else numpy.float32)
            assert image.shape[:2] == self.shape
            ptr = image.ctypes.data
        ms = C.c_double(0)
        _lib.check(_lib.lib().siftmi_plan_transform_ex(self.sift._handle, ptr, 0, 3 if self.RGB else 1, out.ctypes.data, 0,
                                                       self.outshape[1], self.outshape[0], matrix.ctypes.data, offset.ctypes.data,
                                                       C.c_float(fill), int(mode), interp, C.byref(ms)))
        self.last_transform_ms = ms.value
        if self.profile:
            self.events.append(("transform", StageEvent(ms.value)))
        return out

    # ------------------------------------------------------------------ host-side estimation
    @staticmethod
    def _xysa(kp):
        """(n, 4) float32 view of (x, y, scale, angle) of a keypoint array (no copy for contiguous records)"""
        a = numpy.ascontiguousarray(kp)
        return a.view(numpy.uint8).reshape(a.shape[0], 144)[:, :16].view(numpy.float32)

    @staticmethod
    def _affine(g0, g1):
        """Least-squares affine map g0 -> g1, returned in the kernel's (y, x) ordering: the six coefficients
        (a..f) of matching_correction are unpacked as in alignment.py:279-283."""
        a, b, c, d, e, f = affine_least_squares(g0[:, 0], g0[:, 1], g1[:, 0], g1[:, 1])[:6]
        return numpy.array([[e, d], [b, a]], dtype=numpy.float32), numpy.array([f, c], dtype=numpy.float32)

    @staticmethod
    def _median_shift(g0, g1):
        """Translation-only estimate: identity matrix and the median displacement, (dy, dx) order (alignment.py:268-271)"""
        delta = g1[:, :2] - g0[:, :2]
        return numpy.identity(2, dtype=numpy.float32), numpy.array([numpy.median(delta[:, 1]), numpy.median(delta[:, 0])], numpy.float32)

    @staticmethod
    def _inliers(g0, g1):
        """double_check (alignment.py:284-296): a pair is an outlier when its displacement length, its angle
        difference or its log scale ratio lies more than OUTLIER_SIGMAS standard deviations from the mean.
        Returns the boolean keep mask, or None when nothing is to be rejected."""
        shift = g1[:, :2] - g0[:, :2]
        votes = _zscore_flags(numpy.sqrt(shift[:, 0] * shift[:, 0] + shift[:, 1] * shift[:, 1]))
        votes = votes + _zscore_flags(g1[:, 3] - g0[:, 3])
        votes = votes + _zscore_flags(numpy.log(g1[:, 2] / g0[:, 2]))
        rejected = votes.sum()
        if rejected > 0 and not numpy.isinf(rejected):
            return votes == 0
        return None

    def _chain_relative(self, matrix, offset):
        """relative=True: compose this frame's map with the maps of the previous frames (homogeneous 3x3 product,
        newest on the left, alignment.py:309-318) and return the accumulated matrix / offset."""
        step = numpy.identity(3, dtype=numpy.float64)
        step[:2, :2] = matrix
        step[:2, 2] = offset
        self.relative_transfo = step if self.relative_transfo is None else numpy.dot(step, self.relative_transfo)
        return (numpy.ascontiguousarray(self.relative_transfo[:2, :2], dtype=numpy.float32),
                numpy.ascontiguousarray(self.relative_transfo[:2, 2], dtype=numpy.float32))

    # ------------------------------------------------------------------ public entry
    def align(self, img, shift_only=False, return_all=False, double_check=False, relative=False, orsa=False,
              robust=False, robust_tol=3.0, robust_hyp=2048, max_shift=None, estimate="host", match_metric="l1", match_ratio=None,
              median="host", interp=None):
        """Align `img` on the reference image.

        :param img: image to align (same shape as the reference)
        :param shift_only: estimate a translation only (also the fallback below 18 matches)
        :param return_all: return a dict with result / keypoint / matching / offset / matrix / rms instead of the image
        :param double_check: re-fit after rejecting 4-sigma outliers in displacement, angle and scale
        :param relative: make this frame the reference of the next one and accumulate the transformations
        :param orsa: filter the matches with ``feature.sift_orsa`` when that module is importable
        :param robust: (extension) keep only the matches that agree on one affine map (``MatchPlan.consensus`` with a fixed
                       seed: the same list of matches gives the same mask); the estimate, ``double_check`` and ``rms`` then
                       act on those.  ``return_all`` gains the key ``"inliers"``, the boolean mask over ``"matching"``.
        :param robust_tol: distance in pixels within which a match agrees with a candidate map
        :param robust_hyp: number of candidate maps tried
        :param max_shift: (extension) None, or a bound in pixels on how far a keypoint of `img` lies from its partner in the
                       reference frame, a scalar or an (x, y) pair: the matcher then compares each reference keypoint only with
                       the keypoints within that window (``MatchPlan.match(window=max_shift)``), which is many times faster on
                       dense frames; everything after the match is unchanged.  When the true displacement exceeds ``max_shift``
                       the true partners are not candidates: expect few or wrong matches, not an error.  On sparse frames a
                       keypoint with a single candidate always pairs with it; ``robust=True`` is recommended there.
        :param estimate: (extension) ``"host"`` (default): the affine map is fitted in numpy on the gathered positions.
                       ``"device"``: it comes from ``MatchPlan.fit`` on the two lists where the matcher read them (with the
                       consensus mask under ``robust``), and the matched positions are not gathered on the host at all.  Both
                       solve the same centred normal equations in float64 and differ in the order of the sums only: matrix
                       and offset agree to float32 rounding.  With ``return_all``, ``"rms"`` is then ``sqrt(ssr / n)`` of the
                       float64 map as the device computed it, not the residual of the float32 matrix and offset that the host
                       path reports.  The host path is taken all the same, with its exact results, under ``shift_only``,
                       under ``double_check``, when ORSA filtered the matches, below 18 usable pairs and for degenerate
                       (collinear) positions.
        :param match_metric: (extension) ``"l1"`` (default) or ``"l2"``, the descriptor distance of the matcher
        :param match_ratio: (extension) None, or the ratio of the ratio test.  With ``match_metric="l1"`` and no ratio the pairs
                       come from ``MatchPlan.match``, the reference's fixed rule, exactly as before.  Otherwise they are
                       ``ratio_filter(*MatchPlan.knn_window(ref, kp, 2, metric=match_metric, window=max_shift), ratio=match_ratio)``:
                       with ``"l2"`` and 0.8 that is Lowe's ratio test on Euclidean distances, inside the window when
                       ``max_shift`` is given and over the whole list when it is not; None stands for ``par.MatchRatio``.
                       Everything after the match is unchanged.
        :param median: (extension) ``"host"`` (default): a translation-only estimate (``shift_only``, fewer than 18 usable pairs)
                       is ``numpy.median`` of the gathered displacements.  ``"device"``: it is ``MatchPlan.shift`` on the two
                       lists where the matcher read them (with the consensus mask under ``robust``): the same median, value
                       for value, and without ``return_all`` the matched positions are not gathered on the host at all.  The
                       host path is taken all the same under ``double_check`` and when ORSA filtered the matches.
                       ``estimate=`` keeps its meaning; ``shift_only`` with ``estimate="device"`` alone stays the host path.
        :param interp: (extension) the sampler of the final warp, as for ``transform``: None or ``"linear"`` (bilinear) or
                       ``"cubic"`` (greyscale aligners only); the estimate is unchanged
        :return: the aligned image, the dict, or None when no keypoint matches
        """
        _lib.interp_code(interp, 1, self.RGB)
        if median not in ("host", "device"):
            raise ValueError("median must be 'host' or 'device', not %r" % (median,))
        if estimate not in ("host", "device"):
            raise ValueError("estimate must be 'host' or 'device', not %r" % (estimate,))
        if match_metric not in ("l1", "l2"):
            raise ValueError("match_metric must be 'l1' or 'l2', not %r" % (match_metric,))
        logger.debug("ref_keypoints: %s" % self.ref_kp.size)
        data = numpy.ascontiguousarray(img, numpy.uint8 if self.RGB else numpy.float32)
        with self.sem:
            kp = self.sift.keypoints(data)          # uploads `data`; it stays staged on the device for the warp
            logger.debug("mod image keypoints: %s" % kp.size)
            # both lists are matched where they lie in HBM: the reference list uploaded once, the new one still in the plan
            ref_list = self.ref_kp if self._ref_dev is None else self._ref_dev
            records = self.sift.device_records() if kp.size else kp
            if match_metric == "l1" and match_ratio is None:
                pairs = self.match.match(ref_list, records, raw_results=True, window=max_shift)
            else:
                pairs = ratio_filter(*self.match.knn_window(ref_list, records, 2, metric=match_metric, window=max_shift), ratio=match_ratio)
            n_pairs = pairs.shape[0]
            if n_pairs == 0:
                logger.warning("No matching keypoints")
                return None
            # Only (x, y, scale, angle) of the matched keypoints enter the fit: 16 bytes per keypoint are gathered, not
            # the 144-byte records; the reference's `matching` recarray (alignment.py:254-259) is only materialised for
            # ORSA and for return_all.
            ref_used = self.ref_kp
            # (the 16-byte heads are first packed into a dense (n, 4) array -- one strided pass -- and indexed there: a fancy
            # index straight into the 144-byte records took 13 ms for 2 x 195 k pairs, this takes 3)
            def gathered():
                if self._ref_heads is None:
                    self._ref_heads = numpy.ascontiguousarray(self._xysa(ref_used))
                return self._ref_heads[pairs[:, 0]], numpy.ascontiguousarray(self._xysa(kp))[pairs[:, 1]]

            # estimate="device": the fit reads the lists in HBM and the gathers wait until something else needs them
            on_device = estimate == "device" and not shift_only and not double_check and not (orsa and feature is not None)
            # median="device": so does the median, and the gathers wait until an affine fit on the host or return_all needs them
            dev_median = median == "device" and not double_check and not (orsa and feature is not None)
            g0, g1 = (None, None) if on_device or dev_median else gathered()

            def matched_records():
                both = numpy.recarray(shape=pairs.shape, dtype=MatchPlan.dtype_kp)
                both[:, 0] = ref_used[pairs[:, 0]]
                both[:, 1] = kp[pairs[:, 1]]
                return both

            matching = None
            if orsa and feature is None:
                logger.warning("feature is not available. No ORSA filtering (robust=True filters on the device)")
            elif orsa:
                matching = feature.sift_orsa(matched_records(), self.shape, 1)
                g0, g1 = self._xysa(numpy.ascontiguousarray(matching[:, 0])), self._xysa(numpy.ascontiguousarray(matching[:, 1]))

            inliers = None
            if robust:
                if matching is not None:        # ORSA kept a subset: the consensus runs on the records it returned
                    m0, m1 = numpy.ascontiguousarray(matching[:, 0]), numpy.ascontiguousarray(matching[:, 1])
                    idx = numpy.arange(m0.shape[0], dtype=numpy.int32)
                    found = self.match.consensus(m0, m1, numpy.stack([idx, idx], axis=1), n_hyp=robust_hyp, tol=robust_tol, seed=0)
                else:                           # both lists are still where match() read them
                    found = self.match.consensus(ref_list, self.sift.device_records(), pairs, n_hyp=robust_hyp, tol=robust_tol, seed=0)
                inliers = found[0]
                if found[1] is None:
                    logger.warning("No consensus among %s matches: all of them are used" % (n_pairs if g0 is None else g0.shape[0]))
                elif g0 is not None:
                    g0, g1 = g0[inliers], g1[inliers]
                    n_pairs = g0.shape[0]
            voters = inliers if robust and found[1] is not None else None      # what a device estimate takes as its mask

            def gathered_voters():
                a, b = gathered()
                return (a, b) if voters is None else (a[voters], b[voters])

            if dev_median and voters is not None:
                n_pairs = int(voters.sum())
            rms = None
            if on_device:
                model, rms, n_fit = self.match.fit(ref_list, self.sift.device_records(), pairs, mask=voters)
                if model is None or n_fit < MIN_MATCHES_AFFINE:      # too few or degenerate: the host path, from its gathers on
                    on_device, rms = False, None
                    if not dev_median:
                        g0, g1 = gathered_voters()
                        n_pairs = g0.shape[0]
            enough = n_pairs >= MIN_MATCHES_AFFINE
            if on_device:
                logger.debug("Common keypoints: %s" % n_fit)
                a, b, c, d, e, f = model
                matrix, offset = numpy.array([[e, d], [b, a]], dtype=numpy.float32), numpy.array([f, c], dtype=numpy.float32)
            elif shift_only or not enough:
                (logger.debug if shift_only else logger.warning)("Shift Only mode: Common keypoints: %s" % n_pairs)
                if dev_median:
                    moved = self.match.shift(ref_list, self.sift.device_records(), pairs, mask=voters)[0]
                    mdx, mdy = moved if moved is not None else (numpy.nan, numpy.nan)
                    matrix, offset = numpy.identity(2, dtype=numpy.float32), numpy.array([mdy, mdx], numpy.float32)
                else:
                    matrix, offset = self._median_shift(g0, g1)
            else:
                logger.debug("Common keypoints: %s" % n_pairs)
                if g0 is None:                      # median="device" with enough pairs for the host's affine fit
                    g0, g1 = gathered_voters()
                matrix, offset = self._affine(g0, g1)
            if return_all and rms is None and g0 is None:       # rms below is taken from the gathers (made before `relative`
                g0, g1 = gathered_voters()                      # replaces the reference the pairs index)
            if double_check and enough:
                logger.warning("Validating keypoints, %s,%s" % (matrix, offset))
                keep = self._inliers(g0, g1)
                if keep is not None:
                    matrix, offset = self._affine(g0[keep], g1[keep])
            if relative:
                self._set_reference(kp)             # this frame becomes the reference of the next one
                matrix, offset = self._chain_relative(matrix, offset)
            result = self.transform(matrix, offset, image=None, fill=self.sift.minmax()[0], mode=1, interp=interp)

        if not return_all:
            return result
        # residual of the fitted map on the matched keypoints, in pixels (alignment.py:349-351)
        # (written out instead of numpy.dot(matrix, src): a threaded BLAS has no business in a 2 x 2 product, see utils.py)
        if rms is None:
            sy, sx = g0[:, 1], g0[:, 0]
            ry = matrix[0, 0] * sy + matrix[0, 1] * sx + offset[0] - g1[:, 1]
            rx = matrix[1, 0] * sy + matrix[1, 1] * sx + offset[1] - g1[:, 0]
            rms = numpy.sqrt((ry * ry + rx * rx).mean())
        if matching is None:
            matching = matched_records()
        out = {"result": result, "keypoint": kp, "matching": matching, "offset": offset, "matrix": matrix, "rms": rms}
        if robust:
            out["inliers"] = inliers
        return out

    __call__ = align

    # ------------------------------------------------------------------ a whole stack in one pass
    def _batch_plan(self, lanes=None):
        """the ``BatchPlan`` of ``align_batch``, created on first use (and again when another number of lanes is asked for)"""
        from .batch import BatchPlan
        bp = getattr(self, "_batch", None)
        if bp is None or (lanes is not None and int(lanes) != bp.lanes):
            shape, dtype = (self.shape + (3,), numpy.uint8) if self.RGB else (self.shape, numpy.float32)
            bp = BatchPlan(shape=shape, dtype=dtype, device=self.device, init_sigma=self.sift._init_sigma, lanes=lanes)
            self._batch = bp
        return bp

    def _device_frames(self, images):
        """The frames of ``align_batch`` as device tensors of the aligner's frame type.  Host frames are converted as ``align``
        converts them and cross the link once, as one stack; device tensors are taken as they are."""
        import torch
        fshape = self.shape + ((3,) if self.RGB else ())
        ndtype = numpy.uint8 if self.RGB else numpy.float32
        tdtype = torch.uint8 if self.RGB else torch.float32
        dev = torch.device("cuda", self.device)
        if isinstance(images, numpy.ndarray) and images.ndim == len(fshape) + 1:
            if tuple(images.shape[1:]) != fshape:
                raise RuntimeError("the stack has frames of shape %s, the aligner takes %s" % (tuple(images.shape[1:]), fshape))
            if images.shape[0] == 0:
                return []
            whole = torch.from_numpy(numpy.ascontiguousarray(images, ndtype)).to(dev)       # a host stack: one copy
            return [whole[i] for i in range(whole.shape[0])]
        if hasattr(images, "shape") and len(images.shape) == len(fshape) + 1:
            images = [images[i] for i in range(int(images.shape[0]))]
        else:
            images = list(images)
        on_dev = [bool(getattr(f, "is_cuda", False)) for f in images]
        if any(on_dev) and not all(on_dev):
            raise RuntimeError("the frames of a stack must be all host arrays or all device tensors")
        for i, f in enumerate(images):
            if tuple(f.shape) != fshape:
                raise RuntimeError("frame %d has shape %s, the aligner takes %s" % (i, tuple(f.shape), fshape))
        if images and all(on_dev):
            for i, f in enumerate(images):
                if f.dtype != tdtype:
                    raise RuntimeError("device frame %d is %s, the aligner takes %s" % (i, f.dtype, tdtype))
            return [f.contiguous() for f in images]
        if not images:
            return []
        # separate host frames go straight into their plane of the device stack, one copy each: stacking them on the host first
        # costs more than the copies (64 frames of 2048 x 2048: 140 ms for stack and upload against the link's 20 ms)
        stack = torch.empty((len(images),) + fshape, dtype=tdtype, device=dev)
        for i, f in enumerate(images):
            host = f if hasattr(f, "numpy") else torch.from_numpy(numpy.ascontiguousarray(f, ndtype))      # the cast of align()
            stack[i].copy_(host)
        return [stack[i] for i in range(len(images))]

    @_lib.interp_keyword("_align_batch_interp")
    def align_batch(self, images, shift_only=False, robust=False, robust_tol=3.0, robust_hyp=2048, match_ratio=None, return_all=False,
                    out="host", lanes=None):
        """Align a stack of S frames on the reference image in one pass (extension): every stage runs
        once for the whole stack, each with one synchronisation -- ``BatchPlan.keypoints_batch_device`` -> ``minmax_batch`` (the
        fill values) -> ``MatchPlan.match_batch`` against the reference list -> ``consensus_batch`` under ``robust`` ->
        ``fit_batch`` / ``shift_batch`` -> ``BatchPlan.transform_batch``.  Keypoints, pairs and masks never leave the device; a
        host frame crosses the link once, into a device stack that both detection and the warp read.  Greyscale and RGB aligners,
        ``extra`` and ``ROI`` as for ``align``.

        Per frame the estimate is what ``align(estimate="device", median="device")`` computes, with one difference: a degenerate
        (collinear) segment of 18 pairs or more takes the median shift here; ``align`` takes the host's minimum-norm fit.  A frame is
        *affine* (mode 2) when ``fit_batch`` gives it a finite map from at least 18 pairs (never under ``shift_only``); any other
        frame with a usable pair takes ``shift_batch``'s median displacement (mode 1); a frame without one (mode 0) is not
        dropped as ``align`` returns None: its map is all NaN, its plane comes out as the frame's fill value, and a warning names it.
        Under ``robust`` a frame without a winning map uses all its pairs, as ``align`` does.

        Device memory beside the plans: ``S * (H * W + OH * OW)`` elements (the stack and the result); a stack that does not fit
        is the caller's to slice.  ``relative``, ``double_check``, ``orsa``, ``max_shift`` and ``match_metric`` have no batch form.

        :param images: S frames of the reference's shape: host arrays (converted as ``align`` converts them), device tensors of
                       the frame type (float32, or uint8 for RGB), or one (S, H, W[, 3]) stack of either
        :param shift_only: estimate translations only
        :param robust, robust_tol, robust_hyp: as for ``align`` (``consensus_batch`` with seed 0)
        :param match_ratio: None (``par.MatchRatio``) or the ratio of the matcher's test, as for ``match_batch``
        :param return_all: return a dict of per-frame arrays instead of the stack: ``result``, ``matrix`` (S, 2, 2), ``offset``
                       (S, 2), ``mode`` (S,) int8, ``n`` (pairs the estimate used), ``rms`` (``fit_batch``'s value where affine, NaN
                       elsewhere), ``fill``, ``counts``, ``keypoint`` (list of recarrays), ``pairs`` (M, 2) with indices local to the
                       frame, ``pair_counts``, and under ``robust`` ``inliers``, the bool (M,) mask over ``pairs`` that was used
        :param out: ``"host"``: the stack is a numpy array; ``"device"``: a torch tensor on the aligner's device
        :param lanes: lanes of the ``BatchPlan`` (created on first use); None: its default for the frame size
        :param interp: (keyword only) the sampler of the warp, as for ``transform``: None or
                       ``"linear"`` (bilinear) or ``"cubic"`` (greyscale aligners only); the estimate is unchanged
        :return: the aligned stack (S, OH, OW[, 3]), or the dict
        """
        return self._align_batch_interp(images, shift_only, robust, robust_tol, robust_hyp, match_ratio, return_all, out, lanes)

    def _align_batch_interp(self, images, shift_only, robust, robust_tol, robust_hyp, match_ratio, return_all, out, lanes, interp=None):
        """the body of ``align_batch``"""
        return self._align_batch(images, lambda ref, records, counts: self.match.match_batch(ref, None, records, counts, ratio=match_ratio, out="device"),
                                 shift_only, robust, robust_tol, robust_hyp, return_all, out, lanes, interp)

    @_lib.interp_keyword("_align_batch_window_interp")
    def align_batch_window(self, images, max_shift, expected_shift=None, shift_only=False, robust=False, robust_tol=3.0, robust_hyp=2048,
                           match_ratio=None, return_all=False, out="host", lanes=None):
        """``align_batch`` with the windowed matcher (extension): the match stage is
        ``MatchPlan.match_window_batch(ref, None, records, counts, window=max_shift, window_shift=expected_shift or (0, 0),
        ratio=match_ratio, out="device")``, which compares each reference keypoint only with the keypoints of a frame within
        ``max_shift`` pixels of its position moved by that frame's ``expected_shift`` -- many times fewer descriptor pairs on
        dense frames.  Every other stage, the decision rule and the result are ``align_batch``'s; ``max_shift=inf`` without an
        expected shift gives ``align_batch``'s results.  (The keywords live in a method of their own because ``align_batch``'s
        parameter list is pinned by the tests of row 15.)

        The warnings of ``align(max_shift=)`` hold per frame.  When the true displacement of a frame lies outside the window, the
        true partners are not candidates: expect few or wrong matches, not an error.  On sparse frames a keypoint with a single
        candidate always pairs with it; ``robust=True`` is recommended there.

        :param images: as for ``align_batch``
        :param max_shift: bound in pixels on how far a keypoint of a frame lies from its partner in the reference frame (after
                       the expected shift), a scalar or an (x, y) pair; ``inf`` is allowed.  Required
        :param expected_shift: None (no displacement expected), one ``(sx, sy)`` for all frames or an (S, 2) array with one per
                       frame, in (x, y) order: where a frame's keypoints are expected relative to their partners in the reference
        :param shift_only, robust, robust_tol, robust_hyp, match_ratio, return_all, out, lanes, interp: as for ``align_batch``
        :return: the aligned stack (S, OH, OW[, 3]), or ``align_batch``'s dict
        """
        return self._align_batch_window_interp(images, max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio,
                                               return_all, out, lanes)

    def _align_batch_window_interp(self, images, max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio,
                                   return_all, out, lanes, interp=None):
        """the body of ``align_batch_window``"""
        if max_shift is None:
            raise ValueError("align_batch_window needs max_shift; without a window the call is align_batch")
        shift = (0.0, 0.0) if expected_shift is None else expected_shift
        return self._align_batch(images, lambda ref, records, counts: self.match.match_window_batch(
            ref, None, records, counts, window=max_shift, window_shift=shift, ratio=match_ratio, out="device"),
            shift_only, robust, robust_tol, robust_hyp, return_all, out, lanes, interp)

    @_lib.interp_keyword("_stack_interp")
    def stack(self, images, reduce="mean", max_shift=None, expected_shift=None, shift_only=False, robust=False, robust_tol=3.0,
              robust_hyp=2048, match_ratio=None, empty=numpy.nan, return_all=False, out="host", lanes=None):
        """Align a stack of S frames on the reference image and combine them into ONE image (extension; DESIGN.md section 7 row
        17): the estimate of every frame is ``align_batch``'s (``align_batch_window``'s when ``max_shift`` is given), and the warp
        is ``BatchPlan.stack_batch``, which reduces the S warped frames pixel by pixel in the launch that samples them -- the
        aligned planes are never written and only the result crosses the link.  Greyscale aligners only.

        A pixel of the result combines the frames that cover it: those whose warped value there is not the fill.  ``"mean"`` and
        ``"sum"`` add them in the order of the stack; ``"median"`` (at most 64 frames) drops what only a few frames show --
        zingers, cosmic rays, a passing object.  A frame without a usable pair (mode 0) has an all-NaN map: it covers nothing, is
        left out everywhere, and still gets ``align_batch``'s warning.  The reference image takes part only if the caller puts it
        into `images`.

        :param images: as for ``align_batch``
        :param reduce: ``"mean"``, ``"sum"`` or ``"median"``
        :param max_shift, expected_shift: None for ``align_batch``'s matcher; otherwise the window of ``align_batch_window``
        :param shift_only, robust, robust_tol, robust_hyp, match_ratio, lanes: as for ``align_batch``
        :param empty: the value of a pixel that no frame covers
        :param return_all: return ``align_batch``'s dict without ``result`` and with ``stack``, the (OH, OW) float32 image, and
                       ``coverage``, the (OH, OW) int32 number of frames that cover each pixel
        :param out: ``"host"``: numpy arrays; ``"device"``: torch tensors on the aligner's device
        :param interp: (keyword only) the sampler of the warp, as for ``BatchPlan.stack_batch``: None
                       or ``"linear"`` (bilinear) or ``"cubic"``; estimate, coverage and reducers are unchanged
        :return: the combined image (OH, OW), or the dict
        """
        return self._stack_interp(images, reduce, max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio, empty,
                                  return_all, out, lanes)

    def _stack_interp(self, images, reduce, max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio, empty,
                      return_all, out, lanes, interp=None):
        """the body of ``stack``"""
        _lib.interp_code(interp, 1, self.RGB)
        if self.RGB:
            raise RuntimeError("stack combines float32 frames; an RGB aligner has no stack reduction")
        from .batch import BatchPlan
        if reduce not in BatchPlan.STACK_REDUCERS:
            raise ValueError("reduce must be one of %s, not %r" % (sorted(BatchPlan.STACK_REDUCERS), reduce))
        return self._stack(images, "stack_batch", lambda bp, frames, matrix, offset, fills: dict(zip(("stack", "coverage"), bp.stack_batch(
            frames, matrix, offset, fills, out_shape=self.outshape, mode=1, reduce=reduce, empty=empty, coverage=True, out=out, interp=interp))),
            max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio, return_all, out, lanes)

    @_lib.interp_keyword("_stack_clip_interp")
    def stack_clip(self, images, reject="sigma", trim=(0, 1), kappa=(3.0, 3.0), iters=3, weights=None, max_shift=None, expected_shift=None,
                   shift_only=False, robust=False, robust_tol=3.0, robust_hyp=2048, match_ratio=None, empty=numpy.nan, return_all=False,
                   out="host", lanes=None):
        """``stack`` with an outlier rejection in front of the mean (extension): the estimate of every
        frame is ``stack``'s and the warp is ``BatchPlan.stack_clip_batch``, which per output pixel drops samples by the chosen rule
        and returns the weighted mean of the rest, in the launch that samples the frames.  At most 64 frames; greyscale aligners
        only.  The mean keeps every zinger and the median gives up most of the stack's signal-to-noise; this keeps every sample
        that is not an outlier.

        ``reject="trim"`` drops the ``trim[1]`` largest and the ``trim[0]`` smallest live samples of a pixel (the largest first, and
        never the last sample); ``reject="sigma"`` drops, in at most `iters` passes, what lies more than ``kappa[0]`` standard
        deviations below or ``kappa[1]`` above the mean of the kept samples -- see ``BatchPlan.stack_clip_batch`` for both rules to
        the last bit.  n samples cannot hold a z-score above ``(n - 1) / sqrt(n)``: ``kappa = 3`` rejects nothing below 11 live
        frames.  ``trim`` is the rule for short stacks.

        :param images: as for ``align_batch``; at most 64 frames
        :param reject, trim, kappa, iters, weights: as for ``BatchPlan.stack_clip_batch``
        :param max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio, empty, out, lanes: as for ``stack``
        :param return_all: return ``stack``'s dict with ``kept`` beside ``coverage``: the (OH, OW) int32 number of frames that
                       survived in each pixel
        :param interp: (keyword only) as for ``stack``
        :return: the combined image (OH, OW), or the dict
        """
        return self._stack_clip_interp(images, reject, trim, kappa, iters, weights, max_shift, expected_shift, shift_only, robust, robust_tol,
                                       robust_hyp, match_ratio, empty, return_all, out, lanes)

    def _stack_clip_interp(self, images, reject, trim, kappa, iters, weights, max_shift, expected_shift, shift_only, robust, robust_tol,
                           robust_hyp, match_ratio, empty, return_all, out, lanes, interp=None):
        """the body of ``stack_clip``"""
        _lib.interp_code(interp, 1, self.RGB)
        if self.RGB:
            raise RuntimeError("stack_clip combines float32 frames; an RGB aligner has no stack reduction")
        from .batch import BatchPlan
        BatchPlan._clip_args(reject, trim, kappa, iters, weights)
        return self._stack(images, "stack_clip_batch", lambda bp, frames, matrix, offset, fills: dict(zip(
            ("stack", "coverage", "kept"), bp.stack_clip_batch(frames, matrix, offset, fills, out_shape=self.outshape, mode=1, reject=reject,
                                                               trim=trim, kappa=kappa, iters=iters, weights=weights, empty=empty, counts=True,
                                                               out=out, interp=interp))),
            max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio, return_all, out, lanes)

    def _stack(self, images, event, reduce, max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio, return_all,
               out, lanes):
        """the body of ``stack`` and ``stack_clip``: the estimate of every frame, then ``reduce(bp, frames, matrix, offset, fills)``,
        which returns the dict of the reduction's planes, ``stack`` first; `event` names the profile event"""
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device', not %r" % (out,))
        if max_shift is None:
            if expected_shift is not None:
                raise ValueError("expected_shift needs max_shift")
            matcher = lambda ref, records, counts: self.match.match_batch(ref, None, records, counts, ratio=match_ratio, out="device")  # noqa: E731
        else:
            shift = (0.0, 0.0) if expected_shift is None else expected_shift
            matcher = lambda ref, records, counts: self.match.match_window_batch(      # noqa: E731
                ref, None, records, counts, window=max_shift, window_shift=shift, ratio=match_ratio, out="device")
        with self.sem:
            bp = self._batch_plan(lanes)
            frames, matrix, offset, mode, fills, rest = self._estimate_batch(bp, images, matcher, shift_only, robust, robust_tol, robust_hyp)
            res = reduce(bp, frames, matrix, offset, fills)
            self.last_stack_ms = bp.last_stack_ms
            if self.profile:
                self.events.append((event, StageEvent(bp.last_stack_ms)))
            if not return_all:
                return res["stack"]
            res.update(rest())
            return res

    def stack_stream(self, images, chunk=32, reject=None, kappa=(3.0, 3.0), var=False, max_shift=None, expected_shift=None, shift_only=False,
                     robust=False, robust_tol=3.0, robust_hyp=2048, match_ratio=None, empty=numpy.nan, return_all=False, out="host",
                     lanes=None, *, interp=None):
        """``stack(reduce="mean")`` for a stack of any length (extension): the frames are read in slices
        of `chunk`, each slice is estimated as ``stack`` estimates it and added to a ``StackAccumulator``.  Device memory is one
        chunk of frames plus 16 to 24 bytes per output pixel; the mean is formed from float64 sums.  Greyscale aligners only.

        ``reject="sigma"`` makes two passes.  The first keeps the mean and the variance of every pixel and the map of every frame;
        the second reads the slices again, samples them with the kept maps -- detection and matching are not repeated -- and adds
        only what lies within ``kappa[0]`` standard deviations below and ``kappa[1]`` above the first pass's mean
        (``StackAccumulator.add(clip=...)``): one pass of ``stack_clip``'s sigma rule, without its cap of 64 frames.

        :param images: a sequence with ``len()`` and slice indexing whose slices ``align_batch`` accepts: a list, an (S, H, W)
                       array, a memmap
        :param chunk: frames per slice, >= 1
        :param reject: None or ``"sigma"``
        :param kappa: (kappa_low, kappa_high), each > 0; ``inf`` switches its side off
        :param var: also return the population variance of the kept samples of every pixel (float32, not rooted)
        :param max_shift, expected_shift, shift_only, robust, robust_tol, robust_hyp, match_ratio, empty, out, lanes, interp: as for
                       ``stack``; an (S, 2) `expected_shift` is sliced with the frames
        :param return_all: return a dict: ``stack``, ``coverage``, ``kept``, ``var`` if asked for, and ``matrix``, ``offset``,
                       ``mode``, ``n``, ``rms``, ``fill`` of every frame, concatenated over the slices
        :return: the combined image (OH, OW), ``(image, var)`` with `var`, or the dict
        """
        _lib.interp_code(interp, 1, self.RGB)
        if self.RGB:
            raise RuntimeError("stack_stream combines float32 frames; an RGB aligner has no stack reduction")
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device', not %r" % (out,))
        if reject not in (None, "sigma"):
            raise ValueError("reject must be None or 'sigma', not %r" % (reject,))
        if int(chunk) != chunk or chunk < 1:
            raise ValueError("chunk must be a whole number >= 1, not %r" % (chunk,))
        chunk = int(chunk)
        try:
            kl, kh = (float(numpy.float32(v)) for v in kappa)
        except (TypeError, ValueError):
            raise ValueError("kappa must be (kappa_low, kappa_high), not %r" % (kappa,))
        if not (kl > 0 and kh > 0):
            raise ValueError("kappa %r: each must be > 0 (inf switches its side off)" % (kappa,))
        S = len(images)
        shifts = None
        if max_shift is None:
            if expected_shift is not None:
                raise ValueError("expected_shift needs max_shift")
        else:
            shifts = numpy.asarray((0.0, 0.0) if expected_shift is None else expected_shift, numpy.float64)
        with self.sem:
            bp = self._batch_plan(lanes)
            first = bp.stack_accumulator(self.outshape, moments=bool(var) or reject == "sigma")
            kept_maps, rests = [], []
            total_ms = 0.0
            for at in range(0, S, chunk):
                if shifts is None:
                    matcher = lambda ref, records, counts: self.match.match_batch(ref, None, records, counts, ratio=match_ratio, out="device")  # noqa: E731
                else:
                    shift = shifts[at:at + chunk] if shifts.ndim == 2 else shifts
                    matcher = lambda ref, records, counts, shift=shift: self.match.match_window_batch(      # noqa: E731
                        ref, None, records, counts, window=max_shift, window_shift=shift, ratio=match_ratio, out="device")
                frames, matrix, offset, mode, fills, rest = self._estimate_batch(bp, images[at:at + chunk], matcher, shift_only, robust,
                                                                                 robust_tol, robust_hyp)
                first.add(frames, matrix, offset, fills, mode=1, interp=interp)
                total_ms += first.last_stack_ms
                kept_maps.append((matrix, offset, numpy.array(fills, numpy.float32)))
                if return_all:
                    rests.append(rest())
                del frames
            acc = first
            if reject == "sigma":
                center, spread = first.result(var=True, out="device")
                acc = bp.stack_accumulator(self.outshape, moments=bool(var))
                for i, at in enumerate(range(0, S, chunk)):
                    matrix, offset, fills = kept_maps[i]
                    frames = self._device_frames(images[at:at + chunk])
                    acc.add(frames, matrix, offset, fills, mode=1, interp=interp, clip=(center, spread), kappa=(kl, kh))
                    total_ms += acc.last_stack_ms
                    del frames
            planes = acc.result(empty=empty, var=bool(var), counts=True, out=out)
            self.last_stack_ms = total_ms
            if self.profile:
                self.events.append(("stack_stream", StageEvent(total_ms)))
            if not return_all:
                return (planes[0], planes[1]) if var else planes[0]
            res = {"stack": planes[0], "coverage": planes[-2], "kept": planes[-1]}
            if var:
                res["var"] = planes[1]
            blank = {"matrix": numpy.zeros((0, 2, 2), numpy.float32), "offset": numpy.zeros((0, 2), numpy.float32), "mode": numpy.zeros(0, numpy.int8),
                     "n": numpy.zeros(0, numpy.int64), "rms": numpy.zeros(0, numpy.float64), "fill": numpy.zeros(0, numpy.float32)}
            for k, none in blank.items():
                res[k] = numpy.concatenate([numpy.asarray(r[k]) for r in rests]) if rests else none
            return res

    def _estimate_batch(self, bp, images, matcher, shift_only, robust, robust_tol, robust_hyp):
        """The estimate of every frame of a stack, shared by ``align_batch`` and ``stack`` (called with the semaphore held):
        ``(frames, matrix, offset, mode, fills, rest)`` -- the device frames, the (S, 2, 2) / (S, 2) maps (all NaN for a frame
        without a usable pair, which is warned about here), the (S,) int8 modes, the fill values, and ``rest()``, which builds
        the other entries of the ``return_all`` dict."""
        import torch
        frames = self._device_frames(images)
        S = len(frames)
        ref_list = self.ref_kp if self._ref_dev is None else self._ref_dev
        counts, records = bp.keypoints_batch_device(frames)
        fills = bp.minmax_batch()[0]
        counts = numpy.asarray(counts, numpy.int64).reshape(S)
        dev = torch.device("cuda", self.device)
        if self.ref_kp.size and int(counts.sum()):
            pairs, pc = matcher(ref_list, records, counts)
        else:
            pairs, pc = torch.empty((0, 2), dtype=torch.int32, device=dev), numpy.zeros(S, numpy.int64)
        starts = numpy.concatenate([[0], numpy.cumsum(pc)]).astype(numpy.int64)
        lists = (ref_list, None, records, counts, pairs, pc)
        matched = int(pc.sum()) > 0
        mask = None
        if robust and matched:
            mask, winners = self.match.consensus_batch(*lists, n_hyp=robust_hyp, tol=robust_tol, seed=0, out="device")[:2]
            for s in numpy.nonzero(numpy.isnan(winners).any(axis=1) & (pc > 0))[0]:
                logger.warning("No consensus among %s matches of frame %d: all of them are used" % (pc[s], s))
                mask[int(starts[s]):int(starts[s + 1])] = 1
        matrix = numpy.full((S, 2, 2), numpy.nan, numpy.float32)
        offset = numpy.full((S, 2), numpy.nan, numpy.float32)
        mode = numpy.zeros(S, numpy.int8)
        used = numpy.zeros(S, numpy.int64)
        rms = numpy.full(S, numpy.nan, numpy.float64)
        affine = numpy.zeros(S, bool)
        if matched and not shift_only:
            models, fit_rms, n_fit = self.match.fit_batch(*lists, mask=mask)
            affine = numpy.isfinite(models).all(axis=1) & (n_fit >= MIN_MATCHES_AFFINE)
            a, b, c, d, e, f = (models[affine, k] for k in range(6))
            matrix[affine] = numpy.stack([e, d, b, a], axis=1).reshape(-1, 2, 2).astype(numpy.float32)
            offset[affine] = numpy.stack([f, c], axis=1).astype(numpy.float32)
            mode[affine], used[affine], rms[affine] = 2, n_fit[affine], fit_rms[affine]
        if matched and (~affine & (pc > 0)).any():
            moved, n_moved = self.match.shift_batch(*lists, mask=mask)
            shifted = ~affine & (n_moved > 0)
            matrix[shifted] = numpy.identity(2, dtype=numpy.float32)
            offset[shifted] = moved[shifted][:, ::-1]                    # (dx, dy) -> the kernel's (y, x) order
            mode[shifted], used[shifted] = 1, n_moved[shifted]
        for s in numpy.nonzero(mode == 0)[0]:
            logger.warning("No matching keypoints in frame %d: its plane is the fill value" % s)

        def rest():
            host = records.cpu().numpy()
            ends = numpy.cumsum(counts) * 144
            keypoint = [host[int(e - 144 * n):int(e)].copy().view(SiftPlan.dtype_kp).view(numpy.recarray) for e, n in zip(ends, counts)]
            res = {"matrix": matrix, "offset": offset, "mode": mode, "n": used, "rms": rms, "fill": fills,
                   "counts": counts, "keypoint": keypoint, "pairs": pairs.cpu().numpy(), "pair_counts": pc}
            if robust:
                res["inliers"] = mask.cpu().numpy().astype(bool) if mask is not None else numpy.zeros(0, bool)
            return res
        return frames, matrix, offset, mode, fills, rest

    def _align_batch(self, images, matcher, shift_only, robust, robust_tol, robust_hyp, return_all, out, lanes, interp=None):
        """the body of ``align_batch``: the estimate of every frame, then the warp; ``matcher(ref_list, records, counts)`` returns
        ``(pairs, pair_counts)`` with the pairs on the device"""
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device', not %r" % (out,))
        _lib.interp_code(interp, 1, self.RGB)
        with self.sem:
            bp = self._batch_plan(lanes)
            frames, matrix, offset, mode, fills, rest = self._estimate_batch(bp, images, matcher, shift_only, robust, robust_tol, robust_hyp)
            result = bp.transform_batch(frames, matrix, offset, fills, out_shape=self.outshape, mode=1, out=out, interp=interp)
            self.last_transform_ms = bp.last_transform_ms
            if self.profile:
                self.events.append(("transform_batch", StageEvent(bp.last_transform_ms)))
            if not return_all:
                return result
            res = {"result": result}
            res.update(rest())
            return res

    def log_profile(self):
        """Print the timing of every recorded device call (profile=True)"""
        if not self.profile:
            return
        total = 0.0
        # alignment.py:363-375 walks self.events; here the plans the aligner drives keep the events of their own stages
        # (the reference's aligner shares one queue with them and sees only its own three): all of them are listed
        for e in list(self.events) + list(self.sift.events) + list(self.match.events):
            if "__len__" in dir(e) and len(e) >= 2:
                et = 1e-6 * (e[1].profile.end - e[1].profile.start)
                print("%50s:\t%.3fms" % (e[0], et))
                total += et
        print("_" * 80)
        print("%50s:\t%.3fms" % ("Total execution time", total))
