"""MatchPlan -- brute-force keypoint matching on one MI355X through libsiftmi.so.

Mirror of the reference's ``sift_pyocl.MatchPlan`` (sift-src/match.py:52-327): same constructor
keywords, ``match(nkp1, nkp2, raw_results=False)`` contract and record type.  The distance is the
reference's: L1 over the 128 descriptor bytes, best / second best with strict '<', pair kept iff
``dist2 != 0 and dist1 / dist2 < par.MatchRatio ** 2`` (matching_cpu.cl:57-109).
"""
import ctypes as C
import logging
import os
import threading

import numpy

from . import _lib
from .param import par
from .plan import _pointer_of

logger = logging.getLogger("sift.match")


def ratio_filter(idx, dist, ratio=None):
    """The reference's ratio test (matching_cpu.cl:103-108) on the result of ``MatchPlan.knn`` (extension), with a ratio of the
    caller's choice: the pairs ``(i, idx[i, 0])`` of the rows with ``dist2 != 0 and dist1 / dist2 < float32(ratio ** 2)`` in
    float32, where ``dist1, dist2 = dist[i, 0], dist[i, 1]`` and a missing distance (-1) counts as ``1e12f``.  With the default
    ratio this is ``MatchPlan.match(kp1, kp2, raw_results=True)`` up to the order of the rows.  On ``knn(..., metric="l2")``
    results, whose distances are squared, it is Lowe's ratio test on Euclidean distances with ``ratio`` itself.  Pure numpy.

    :param idx, dist: the two ``(n1, k)`` int32 arrays of ``MatchPlan.knn``, ``k >= 2``
    :param ratio: None (``par.MatchRatio``) or a number with ``ratio ** 2 <= 1``: above 1 the brute-force scan pairs a query
                  without any candidate with index 0, which has no counterpart here
    :return: ``(m, 2)`` int32, ascending in i
    """
    idx = numpy.asarray(idx)
    dist = numpy.asarray(dist)
    if idx.ndim != 2 or idx.shape != dist.shape or idx.shape[1] < 2:
        raise ValueError("ratio_filter needs idx and dist of one shape (n1, k) with k >= 2, not %s and %s" % (idx.shape, dist.shape))
    r = par.MatchRatio if ratio is None else ratio
    th = numpy.float32(r * r)
    if not th <= numpy.float32(1):
        raise ValueError("ratio ** 2 must be <= 1, not %r" % (float(th),))
    f1 = numpy.where(dist[:, 0] < 0, numpy.float32(1e12), dist[:, 0].astype(numpy.float32)).astype(numpy.float32)
    f2 = numpy.where(dist[:, 1] < 0, numpy.float32(1e12), dist[:, 1].astype(numpy.float32)).astype(numpy.float32)
    with numpy.errstate(all="ignore"):
        keep = (f2 != 0) & (f1 / f2 < th)
    i = numpy.nonzero(keep)[0]
    return numpy.stack([i, idx[i, 0]], axis=1).astype(numpy.int32)


class MatchPlan(object):
    """Plan to compare sets of SIFT keypoints and find common ones.

    ::

        mp = sift_pyocl_amd.MatchPlan()
        pairs = mp.match(kp1, kp2)                  # (m, 2) recarray of matching keypoints
        idx = mp.match(kp1, kp2, raw_results=True)  # (m, 2) int32 indices
    """
    dtype_kp = numpy.dtype([('x', numpy.float32),
                            ('y', numpy.float32),
                            ('scale', numpy.float32),
                            ('angle', numpy.float32),
                            ('desc', (numpy.uint8, 128))
                            ])

    def __init__(self, size=16384, devicetype="CPU", profile=False, device=None, max_workgroup_size=None,
                 roi=None, context=None):
        self.profile = bool(profile)
        self.events = []
        self.kpsize = int(size)
        self.max_workgroup_size = max_workgroup_size
        self.ctx = context
        if isinstance(device, (tuple, list)):
            device = device[-1]
        if device is None:
            device = int(os.environ.get("SIFT_MI355X_DEVICE", os.environ.get("LOCAL_RANK", 0)))
        self.device = int(device)
        self.devicetype = "GPU"
        self.USE_CPU = (str(devicetype).upper() == "CPU")
        self._sem = threading.Semaphore()
        self._handle = C.c_void_p()
        L = _lib.lib()
        if L.siftmi_device_count() < 1:
            raise RuntimeError("sift_pyocl_amd needs a HIP device (MI355X); none is visible and there is no CPU fallback")
        _lib.check(L.siftmi_match_create(self.kpsize, self.device, int(self.profile), C.byref(self._handle)))
        self.roi = None
        if roi is not None:
            self.set_roi(roi)

    def __del__(self):
        h = getattr(self, "_handle", None)
        if h:
            try:
                _lib.lib().siftmi_match_destroy(h)
            except Exception:
                pass
            self._handle = None

    ROI_MODES = {0: 0, None: 0, False: 0, "off": 0, 1: 1, True: 1, "reference": 1, "matching_valid": 1, 2: 2, "strict": 2}

    def match(self, nkp1, nkp2, raw_results=False, roi_mode=0, mutual=False, window=None, window_shift=(0.0, 0.0)):
        """Calculate the matching of 2 keypoint lists

        :param nkp1, nkp2: numpy 1D recarray of keypoints (or device tensors of 144-byte records)
        :param raw_results: if true return the 2D array of indexes of matching keypoints (not the actual keypoints)
        :param roi_mode: 0 (default) ignores the region of interest, exactly like the reference, whose ``match`` never
                         reaches its ``matching_valid`` kernel; "reference" / 1 runs that kernel's semantics literally
                         (matching_cpu.cl:136-199); "strict" / 2 drops every keypoint that is not on a non-zero pixel.
                         A keypoint's pixel is ``(c, r) = (int)x, (int)y``, truncated toward zero (every coordinate in (-1, 1)
                         gives 0); it is inside the mask iff ``0 <= r < rows and 0 <= c < columns``, and on it iff the mask is
                         non-zero there (any non-zero int8, negative values included).  A coordinate ``v`` that is NaN, infinite
                         or has ``abs(v) >= 2**31`` is never converted: its keypoint is outside.  Mode 1 drops a first-list
                         keypoint that is inside and not on the mask and gives a second-list keypoint that is not on it the
                         distance 0; mode 2 leaves every keypoint that is not on the mask out
        :param mutual: keep only pairs that are nearest neighbours in both directions (extension)
        :param window: (extension) None, or the half width of a search window in pixels, a scalar or an ``(wx, wy)`` pair (x first,
                       like the record fields; ``inf`` is allowed).  Keypoint j of the second list is then a *candidate* of keypoint
                       i of the first iff ``abs((x2[j] - x1[i]) - sx) <= wx and abs((y2[j] - y1[i]) - sy) <= wy`` (float32), and
                       the reference's rule -- nearest and second nearest descriptor, ratio test -- sees the candidates only
                       (DESIGN.md section 7 row 6).  For lists whose partners are known to lie within a few pixels of each other
                       this compares a few hundred descriptors per keypoint instead of the whole list.  Consequences of the
                       rule: a keypoint without a candidate pairs with nothing; a keypoint with exactly ONE candidate always
                       pairs with it (the second distance keeps its initial 1e12, as in the reference when the second list has
                       one element), so a small window on sparse lists returns such lone-candidate pairs: ``mutual=True`` and
                       ``consensus()`` are the filters for those.  With ``mutual``, i must also be the nearest candidate of j.
                       Not defined together with ``roi_mode``.
        :param window_shift: ``(sx, sy)``, the expected displacement of the second list against the first (centre of the window)
        """
        assert len(nkp1.shape) == 1
        assert len(nkp2.shape) == 1
        p1, dev1, n1, keep1 = self._records(nkp1)
        p2, dev2, n2, keep2 = self._records(nkp2)
        with self._sem:
            L = _lib.lib()
            if min(n1, n2) > self.kpsize:      # match.py:241-243
                self.kpsize = min(n1, n2)
            cap = max(1, self.kpsize)
            pairs = numpy.empty((cap, 2), dtype=numpy.int32)
            n = C.c_int64(0)
            total = C.c_int64(0)
            ratio = numpy.float32(par.MatchRatio * par.MatchRatio)
            mode = self.ROI_MODES[roi_mode]
            if mode and self.roi is None:
                raise RuntimeError("roi_mode=%r needs a region of interest (set_roi)" % (roi_mode,))
            if window is None:
                _lib.check(L.siftmi_match_ex(self._handle, p1, n1, dev1, p2, n2, dev2, C.c_float(ratio), mode, int(bool(mutual)),
                                             pairs.ctypes.data, cap, C.byref(n), C.byref(total)), allow=(_lib.ECAPACITY,))
            else:
                if mode:
                    raise RuntimeError("window= together with roi_mode=%r is not defined" % (roi_mode,))
                wx, wy = (window if hasattr(window, "__len__") else (window, window))
                sx, sy = window_shift
                _lib.check(L.siftmi_match_window(self._handle, p1, n1, dev1, p2, n2, dev2, C.c_float(ratio), C.c_float(wx), C.c_float(wy),
                                                 C.c_float(sx), C.c_float(sy), int(bool(mutual)), pairs.ctypes.data, cap,
                                                 C.byref(n), C.byref(total)), allow=(_lib.ECAPACITY,))
            size = int(n.value)
            if self.profile:             # match.py:226-263: (label, event) pairs of this call, appended until reset_timer()
                self.events += self._stage_events()
            match = pairs[:size].copy()
            if raw_results:
                result = match
            else:
                if dev1 or dev2:
                    raise RuntimeError("raw_results=False needs host keypoint arrays")
                result = numpy.recarray(shape=(size, 2), dtype=self.dtype_kp)
                result[:, 0] = keep1[match[:size, 0]]
                result[:, 1] = keep2[match[:size, 1]]
        return result

    __call__ = match

    def consensus(self, kp1, kp2, pairs, n_hyp=2048, tol=3.0, seed=0, return_votes=False):
        """Tell the pairs of a ``match(..., raw_results=True)`` that agree on one affine map from the rest (extension; the
        reference's ``orsa=True`` needs the third-party ``feature`` module).  ``n_hyp`` maps are solved from pseudo-random
        triples of pairs, every pair votes for every map that brings its ``kp1`` position within ``tol`` pixels of its ``kp2``
        position, and the map with most votes wins.  Deterministic for given inputs, ``n_hyp``, ``tol`` and ``seed``
        (DESIGN.md section 7 row 5 is the exact arithmetic).

        :param kp1, kp2: the keypoint lists ``pairs`` indexes, numpy records or device tensors as for ``match``
        :param pairs: (M, 2) int32 indices, a numpy array or a device tensor
        :return: ``(mask, model, votes)``: bool (M,) voters of the winning map, its float32 (a, b, c, d, e, f) with
                 x' = a x + b y + c, y' = d x + e y + f (``utils.affine_least_squares`` order; None when no triple is
                 usable, the mask is then all False) and its vote count; with ``return_votes`` a fourth item
                 ``(votes_all, models_all)``: int32 (n_hyp,), float32 (n_hyp, 6) with unusable triples as NaN rows
        """
        p1, dev1, n1, keep1 = self._records(kp1)
        p2, dev2, n2, keep2 = self._records(kp2)
        pp, devp, pdtype, pshape, keepp = _pointer_of(pairs)
        if pdtype != numpy.int32 or len(pshape) != 2 or pshape[1] != 2:
            raise RuntimeError("pairs must be an (M, 2) int32 array")
        n_pairs, n_hyp = int(pshape[0]), int(n_hyp)
        mask = numpy.zeros(n_pairs, numpy.uint8)
        model = numpy.zeros(6, numpy.float32)
        votes_all = numpy.zeros(max(n_hyp, 0), numpy.int32) if return_votes else None
        models_all = numpy.zeros((max(n_hyp, 0), 6), numpy.float32) if return_votes else None
        winner, votes, ms = C.c_int32(-1), C.c_int32(0), C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_consensus(
                self._handle, p1, n1, dev1, p2, n2, dev2, pp if n_pairs else None, n_pairs, devp, n_hyp, C.c_float(tol),
                int(seed) & 0xFFFFFFFF, mask.ctypes.data, model.ctypes.data, C.byref(winner), C.byref(votes),
                votes_all.ctypes.data if return_votes else None, models_all.ctypes.data if return_votes else None, C.byref(ms)))
            if self.profile:
                from .plan import StageEvent
                self.events.append(("consensus", StageEvent(ms.value)))      # device time of the vote kernel
        result = (mask.view(numpy.bool_), model if winner.value >= 0 else None, int(votes.value))
        return result + ((votes_all, models_all),) if return_votes else result

    FIT_OK, FIT_EMPTY, FIT_DEGENERATE = 0, 1, 2

    def fit(self, kp1, kp2, pairs, mask=None, blocks=0, return_moments=False):
        """Least-squares affine map that sends the ``kp1`` positions of the pairs onto their ``kp2`` positions, computed on the
        device (extension; what ``utils.affine_least_squares`` computes on the host).  Centred normal equations in float64,
        every sum formed in one fixed order: deterministic for given inputs and ``blocks`` (DESIGN.md section 7 row 9 is the
        exact arithmetic).  A pair with an index outside its list or a non-finite coordinate is skipped.

        :param kp1, kp2: the keypoint lists ``pairs`` indexes, numpy records or device tensors as for ``match``
        :param pairs: (M, 2) int32 indices, a numpy array or a device tensor
        :param mask: None, or (M,) bool / uint8, a numpy array or a device tensor: only the pairs with a non-zero entry are
                     fitted (the mask of ``consensus``)
        :param blocks: workgroups the sums are spread over, 1 .. 1024 (part of the summation order); 0 picks by M
        :return: ``(model, rms, n)``: float64 (a, b, c, d, e, f) with x' = a x + b y + c, y' = d x + e y + f (the order of
                 ``consensus``), the root mean square residual of that map over the fitted pairs in pixels, and their number.
                 ``model`` is None and ``rms`` NaN when no pair is usable or the positions are degenerate (fewer than three,
                 collinear).  With ``return_moments`` a fourth item: the 20 float64 values of ``siftmi_match_fit`` (status,
                 n, four means, seven centred moments, the model, the sum of squared residuals).
        """
        p1, dev1, n1, keep1 = self._records(kp1)
        p2, dev2, n2, keep2 = self._records(kp2)
        pp, devp, pdtype, pshape, keepp = _pointer_of(pairs)
        if pdtype != numpy.int32 or len(pshape) != 2 or pshape[1] != 2:
            raise RuntimeError("pairs must be an (M, 2) int32 array")
        n_pairs = int(pshape[0])
        pm, devm, keepm = None, 0, None
        if mask is not None:
            if isinstance(mask, numpy.ndarray) and mask.dtype == numpy.bool_:
                mask = mask.view(numpy.uint8)
            pm, devm, mdtype, mshape, keepm = _pointer_of(mask)
            if mdtype.itemsize != 1 or mdtype.kind not in "bu" or tuple(mshape) != (n_pairs,):
                raise RuntimeError("mask must be an (M,) bool or uint8 array")
        raw = numpy.empty(20, numpy.float64)
        ms = C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_fit(self._handle, p1, n1, dev1, p2, n2, dev2, pp if n_pairs else None, n_pairs, devp,
                                                   pm if n_pairs else None, devm, int(blocks), raw.ctypes.data, C.byref(ms)))
            if self.profile:
                from .plan import StageEvent
                self.events.append(("fit", StageEvent(ms.value)))            # device time, gather to the last kernel
        ok = raw[0] == self.FIT_OK
        result = (raw[13:19].copy() if ok else None, float(numpy.sqrt(raw[19] / raw[1])) if ok else float("nan"), int(raw[1]))
        return result + (raw,) if return_moments else result

    def shift(self, kp1, kp2, pairs, mask=None, tol=None, blocks=0, return_ranks=False):
        """Median displacement of the ``kp2`` positions of the pairs against their ``kp1`` positions, computed on the device
        (extension; what ``numpy.median`` gives ``LinearAlign``'s translation-only estimate on the host).  Exact: per axis the
        two middle float32 displacements are selected in the total order of float32 and averaged as ``numpy.median`` does, so
        the value is numpy's bit for bit, up to the sign of a zero.  A pair with an index outside
        its list or a non-finite coordinate is skipped.

        :param kp1, kp2: the keypoint lists ``pairs`` indexes, numpy records or device tensors as for ``match``
        :param pairs: (M, 2) int32 indices, a numpy array or a device tensor
        :param mask: None, or (M,) bool / uint8, a numpy array or a device tensor: only the pairs with a non-zero entry count
                     (the mask of ``consensus``)
        :param tol: None, or a distance in pixels >= 0 (``inf`` is allowed): the result gains the bool (M,) mask of the counted
                    pairs whose displacement lies within ``tol`` of the median on both axes (float32)
        :param blocks: workgroups the pairs are spread over, 1 .. 1024; 0 picks by M.  The result does not depend on it
        :return: ``((dx, dy), n)``: two ``numpy.float32`` and the number of pairs counted; ``(None, 0)`` when no pair is usable.
                 With ``tol`` a third item, the keep mask; with ``return_ranks`` a last item, the six float32 values of
                 ``siftmi_match_shift`` (dx, dy, then the lower and upper middle displacement of x and of y; NaN without a pair).
        """
        p1, dev1, n1, keep1 = self._records(kp1)
        p2, dev2, n2, keep2 = self._records(kp2)
        pp, devp, pdtype, pshape, keepp = _pointer_of(pairs)
        if pdtype != numpy.int32 or len(pshape) != 2 or pshape[1] != 2:
            raise RuntimeError("pairs must be an (M, 2) int32 array")
        n_pairs = int(pshape[0])
        pm, devm, keepm = None, 0, None
        if mask is not None:
            if isinstance(mask, numpy.ndarray) and mask.dtype == numpy.bool_:
                mask = mask.view(numpy.uint8)
            pm, devm, mdtype, mshape, keepm = _pointer_of(mask)
            if mdtype.itemsize != 1 or mdtype.kind not in "bu" or tuple(mshape) != (n_pairs,):
                raise RuntimeError("mask must be an (M,) bool or uint8 array")
        raw = numpy.empty(6, numpy.float32)
        counts = numpy.zeros(2, numpy.int64)
        kept = numpy.zeros(n_pairs, numpy.uint8) if tol is not None else None
        ms = C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_shift(self._handle, p1, n1, dev1, p2, n2, dev2, pp if n_pairs else None, n_pairs, devp,
                                                     pm if n_pairs else None, devm, int(blocks), C.c_float(0.0 if tol is None else tol),
                                                     kept.ctypes.data if tol is not None else None, raw.ctypes.data,
                                                     counts.ctypes.data, C.byref(ms)))
            if self.profile:
                from .plan import StageEvent
                self.events.append(("shift", StageEvent(ms.value)))          # device time, gather to the last kernel
        n = int(counts[0])
        result = ((raw[0], raw[1]) if n else None, n)
        if tol is not None:
            result += (kept.view(numpy.bool_),)
        return result + (raw,) if return_ranks else result

    KNN_MAX = 8

    KNN_METRICS = {"l1": _lib.METRIC_L1, "l2": _lib.METRIC_L2SQ}

    def knn(self, kp1, kp2, k=2, metric="l1"):
        """The k nearest neighbours in ``kp2`` of every keypoint of ``kp1`` WITH their descriptor distances (extension; DESIGN.md
        section 7 rows 7 and 8).  Row i holds the k smallest ``(distance, index)`` over the whole second list in ascending order,
        the smaller index first among equal distances.  The distance is an int32 over the 128 descriptor bytes: with
        ``metric="l1"`` the L1 distance the reference's matcher uses (0 .. 32 640), with ``metric="l2"`` the SQUARED Euclidean
        distance (0 .. 8 323 200; no square root is taken).  Positions, the region of interest and ``par`` play no part, and
        the plan's ``kpsize`` is left alone.  ``ratio_filter(idx, dist, ratio)`` applies the reference's ratio test to the
        result; on ``"l2"`` distances that is Lowe's test on Euclidean distances with ``ratio`` itself.

        :param kp1, kp2: numpy records, device tensors of 144-byte records or ``SiftPlan.device_records()``, as for ``match``
        :param k: 1 .. 8
        :param metric: ``"l1"`` or ``"l2"``
        :return: ``(idx, dist)``, two int32 arrays of shape (n1, k); -1 in both where the second list has fewer than k keypoints
        """
        if not isinstance(metric, str) or metric not in self.KNN_METRICS:
            raise ValueError("metric must be 'l1' or 'l2', not %r" % (metric,))
        p1, dev1, n1, keep1 = self._records(kp1)
        p2, dev2, n2, keep2 = self._records(kp2)
        k = int(k)
        cols = min(max(k, 0), self.KNN_MAX)
        idx = numpy.empty((n1, cols), dtype=numpy.int32)
        dist = numpy.empty((n1, cols), dtype=numpy.int32)
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_knn_metric(self._handle, p1, n1, dev1, p2, n2, dev2, k, self.KNN_METRICS[metric],
                                                          idx.ctypes.data, dist.ctypes.data))
            if self.profile:
                self.events += self._stage_events(self.KNN_STAGE_LABELS)
        return idx, dist

    def knn_window(self, kp1, kp2, k=2, metric="l1", window=None, window_shift=(0.0, 0.0)):
        """``knn`` over the *candidates* of a keypoint only (extension): keypoint j of ``kp2`` is a
        candidate of keypoint i of ``kp1`` iff ``abs((x2[j] - x1[i]) - sx) <= wx and abs((y2[j] - y1[i]) - sy) <= wy`` in float32,
        every operation rounded on its own (``match(window=)``'s predicate; a NaN makes it false).  Row i holds the k smallest
        ``(distance, index)`` over the candidates of i in ascending order, the smaller index first among equal distances; the
        remaining slots of a row with fewer than k candidates -- none included -- hold -1 in both arrays.  The distance is
        ``knn``'s, on either metric.  The lists are binned on a grid of window-sized cells, so a query costs the descriptors of
        its neighbourhood instead of the whole list; the result does not depend on the grid.  ``par``, the region of interest and
        the plan's ``kpsize`` play no part.  ``window=None`` is ``knn(kp1, kp2, k, metric)`` itself, the same call.  (The keywords
        live in a method of their own because ``knn``'s parameter list is pinned by the tests of rows 7 and 8.)

        Two identities: (W1) ``ratio_filter(*knn_window(a, b, 2, window=w, window_shift=s))`` is
        ``match(a, b, raw_results=True, window=w, window_shift=s)`` as sorted rows -- a lone candidate always pairs, a query without
        candidates never does; (W3) candidacy is symmetric under an exchange of the lists with the shift negated, so
        ``knn_window(b, a, k, window=w, window_shift=(-sx, -sy))`` ranks the candidates of every ``kp2`` keypoint among ``kp1``.
        ``window=inf`` with a zero shift and finite coordinates gives the rows of ``knn``.

        :param kp1, kp2: numpy records, device tensors of 144-byte records or ``SiftPlan.device_records()``, as for ``match``
        :param k: 1 .. 8
        :param metric: ``"l1"`` or ``"l2"``
        :param window: None (the whole list), or the half width of the search window in pixels, a scalar or an ``(wx, wy)`` pair
                       (``inf`` is allowed; negative or NaN is an error)
        :param window_shift: ``(sx, sy)``, the expected displacement of the second list against the first (finite); needs ``window``
        :return: ``(idx, dist)``, two int32 arrays of shape (n1, k); -1 in both where a keypoint has fewer than k candidates
        """
        if window is None:
            if tuple(window_shift) != (0.0, 0.0):
                raise ValueError("window_shift=%r needs a window" % (window_shift,))
            return self.knn(kp1, kp2, k, metric)
        if not isinstance(metric, str) or metric not in self.KNN_METRICS:
            raise ValueError("metric must be 'l1' or 'l2', not %r" % (metric,))
        p1, dev1, n1, keep1 = self._records(kp1)
        p2, dev2, n2, keep2 = self._records(kp2)
        k = int(k)
        cols = min(max(k, 0), self.KNN_MAX)
        idx = numpy.empty((n1, cols), dtype=numpy.int32)
        dist = numpy.empty((n1, cols), dtype=numpy.int32)
        wx, wy = (window if hasattr(window, "__len__") else (window, window))
        sx, sy = window_shift
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_knn_window(self._handle, p1, n1, dev1, p2, n2, dev2, k, self.KNN_METRICS[metric],
                                                          C.c_float(wx), C.c_float(wy), C.c_float(sx), C.c_float(sy),
                                                          idx.ctypes.data, dist.ctypes.data))
            if self.profile:
                self.events += self._stage_events(self.KNN_STAGE_LABELS)
        return idx, dist

    BATCH_MAX_SEGMENTS = 65535
    BATCH_MAX_PART = 65472

    def match_batch(self, kp1, counts1, kp2, counts2, ratio=None, mutual=False, part_len=0, out="host"):
        """``match(kp1_s, kp2_s, raw_results=True)`` for S segment pairs in one call: one set of launches and one synchronisation
        (extension).  ``kp2`` holds the records of S lists back to back -- the result of
        ``BatchPlan.keypoints_batch_device`` is exactly this -- and ``counts2`` their lengths; ``kp1`` and ``counts1`` likewise, or
        ``counts1=None`` for ONE list that every segment is matched against (the reference frame of a stack).  Matching each frame
        against the one before it is two slices of one tensor with ``counts[:-1]`` and ``counts[1:]``.  Segment s gets ``match``'s
        rule with the threshold ``float32(ratio ** 2)``, indices local to the segment; a segment with an empty list on either side
        gives no pair, one whose second list has one element pairs every query with it.  The region of interest, windows and the
        plan's ``kpsize`` play no part.

        :param kp1, kp2: numpy records or device tensors of 144-byte records, as for ``match``
        :param counts1: None, or S non-negative ints that add up to the records of ``kp1``
        :param counts2: S non-negative ints that add up to the records of ``kp2``; S <= 65 535
        :param ratio: None (``par.MatchRatio``) or a number with ``ratio ** 2 <= 1``, as for ``ratio_filter``
        :param mutual: keep (i, j) only if i is also the nearest of j inside the segment (``match(mutual=True)``'s rule)
        :param part_len: elements of a second-list segment per partition of the scan: 0 (the library chooses) or a multiple of 64
                         up to 65 472.  The result does not depend on it
        :param out: ``"host"``: ``pairs`` is a numpy array; ``"device"``: a torch int32 tensor on the plan's device, whose slices
                    can go straight into ``consensus``, ``fit`` and ``shift``
        :return: ``(pairs, pair_counts)``: (M, 2) int32 and (S,) int64 (numpy either way).  The pairs of segment s are the rows
                 ``pairs[sum(pair_counts[:s]):][:pair_counts[s]]``; segments in order, ascending i inside a segment: the array
                 is fixed completely
        """
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device', not %r" % (out,))
        r = par.MatchRatio if ratio is None else ratio
        th = numpy.float32(r * r)
        if not th <= numpy.float32(1):
            raise ValueError("ratio ** 2 must be <= 1, not %r" % (float(th),))
        part_len = int(part_len)
        if part_len < 0 or part_len > self.BATCH_MAX_PART or part_len % 64:
            raise ValueError("part_len must be 0 or a multiple of 64 up to %d, not %d" % (self.BATCH_MAX_PART, part_len))
        p1, dev1, n1, keep1 = self._records(kp1)
        p2, dev2, n2, keep2 = self._records(kp2)
        c2 = numpy.ascontiguousarray([int(c) for c in counts2], dtype=numpy.int64).reshape(-1)
        S = len(c2)
        c1 = None if counts1 is None else numpy.ascontiguousarray([int(c) for c in counts1], dtype=numpy.int64).reshape(-1)
        if S > self.BATCH_MAX_SEGMENTS:
            raise ValueError("%d segments: more than %d" % (S, self.BATCH_MAX_SEGMENTS))
        if c1 is not None and len(c1) != S:
            raise ValueError("counts1 has %d entries, counts2 %d" % (len(c1), S))
        if (c2 < 0).any() or (c1 is not None and (c1 < 0).any()):
            raise ValueError("negative count")
        if int(c2.sum()) != n2 or (c1 is not None and int(c1.sum()) != n1):
            raise ValueError("the counts do not add up to the lists: %s of %d and %d of %d records" %
                             ("-" if c1 is None else int(c1.sum()), n1, int(c2.sum()), n2))
        rows = n1 * S if c1 is None else n1
        pair_counts = numpy.zeros(S, numpy.int64)
        if out == "device":
            import torch
            pairs = torch.empty((rows, 2), dtype=torch.int32, device=torch.device("cuda", self.device))
            pp = pairs.data_ptr()
        else:
            pairs = numpy.empty((rows, 2), dtype=numpy.int32)
            pp = pairs.ctypes.data
        if S == 0:
            return pairs[:0], pair_counts
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_batch(self._handle, p1, n1, dev1, p2, n2, dev2, S, None if c1 is None else c1.ctypes.data,
                                                     c2.ctypes.data, C.c_float(th), int(bool(mutual)), part_len, pp if rows else None,
                                                     int(out == "device"), pair_counts.ctypes.data))
            if self.profile:
                self.events += self._stage_events()
        total = int(pair_counts.sum())
        return (pairs[:total] if out == "device" else pairs[:total].copy()), pair_counts

    BATCH_MAX_GRID = 256

    def match_window_batch(self, kp1, counts1, kp2, counts2, window, window_shift=(0.0, 0.0), ratio=None, mutual=False, grid_max=0,
                           out="host"):
        """``match(kp1_s, kp2_s, raw_results=True, window=, window_shift=)`` for S segment pairs in one call: ``match_batch`` with
        the windowed matcher, one set of launches and one synchronisation (extension).  The lists,
        the counts, ``ratio``, ``mutual``, ``out`` and the result are ``match_batch``'s; keypoint j of segment s's second list is a
        *candidate* of keypoint i of its first list iff ``abs((x2[j] - x1[i]) - sx_s) <= wx and abs((y2[j] - y1[i]) - sy_s) <= wy``
        (float32, ``match(window=)``'s predicate), and the rule sees the candidates only.  Every list is binned on a grid of its
        own, so a segment far away or with non-finite coordinates costs the others nothing; no record of another segment can
        enter a segment's result.  As for ``match(window=)``: a keypoint without a candidate pairs with nothing, a keypoint with
        exactly ONE candidate always pairs with it; ``mutual=True`` and ``consensus_batch`` are the filters for those.  (The
        keywords live in a method of their own because ``match_batch``'s parameter list is pinned by the tests of row 12.)

        :param kp1, counts1, kp2, counts2: as for ``match_batch`` (``counts1=None``: ONE first list for every segment)
        :param window: the half width of the search window in pixels, a scalar or an ``(wx, wy)`` pair (x first; ``inf`` is allowed,
                       negative or NaN is an error).  Required: without a window the call is ``match_batch``
        :param window_shift: ``(sx, sy)``, the expected displacement of the second list against the first, for all segments, or an
                       (S, 2) array with one shift per segment; finite
        :param ratio: None (``par.MatchRatio``) or a number with ``ratio ** 2 <= 1``
        :param mutual: keep (i, j) only if i is also the nearest candidate of j inside the segment
        :param grid_max: 0 (the library chooses) or 1 .. 256, the most cells per axis of a segment's grid.  The result does not
                       depend on it
        :param out: ``"host"`` or ``"device"``, as for ``match_batch``
        :return: ``(pairs, pair_counts)`` exactly as ``match_batch`` returns them: segments in order, ascending i inside a
                 segment, indices local to the segment; they go straight into ``consensus_batch``, ``fit_batch`` and ``shift_batch``
        """
        if window is None:
            raise ValueError("match_window_batch needs a window; without one the call is match_batch(kp1, counts1, kp2, counts2)")
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device', not %r" % (out,))
        r = par.MatchRatio if ratio is None else ratio
        th = numpy.float32(r * r)
        if not th <= numpy.float32(1):
            raise ValueError("ratio ** 2 must be <= 1, not %r" % (float(th),))
        wx, wy = (numpy.float32(w) for w in (window if hasattr(window, "__len__") else (window, window)))
        if not (wx >= 0 and wy >= 0):
            raise ValueError("the window must be >= 0 (it may be infinite), not (%r, %r)" % (float(wx), float(wy)))
        grid_max = int(grid_max)
        if grid_max < 0 or grid_max > self.BATCH_MAX_GRID:
            raise ValueError("grid_max must be 0 .. %d, not %d" % (self.BATCH_MAX_GRID, grid_max))
        p1, dev1, n1, keep1 = self._records(kp1)
        p2, dev2, n2, keep2 = self._records(kp2)
        c2 = numpy.ascontiguousarray([int(c) for c in counts2], dtype=numpy.int64).reshape(-1)
        S = len(c2)
        c1 = None if counts1 is None else numpy.ascontiguousarray([int(c) for c in counts1], dtype=numpy.int64).reshape(-1)
        if S > self.BATCH_MAX_SEGMENTS:
            raise ValueError("%d segments: more than %d" % (S, self.BATCH_MAX_SEGMENTS))
        if c1 is not None and len(c1) != S:
            raise ValueError("counts1 has %d entries, counts2 %d" % (len(c1), S))
        if (c2 < 0).any() or (c1 is not None and (c1 < 0).any()):
            raise ValueError("negative count")
        if int(c2.sum()) != n2 or (c1 is not None and int(c1.sum()) != n1):
            raise ValueError("the counts do not add up to the lists: %s of %d and %d of %d records" %
                             ("-" if c1 is None else int(c1.sum()), n1, int(c2.sum()), n2))
        shifts = numpy.asarray(window_shift, dtype=numpy.float32)
        if shifts.shape == (2,):
            shifts = numpy.broadcast_to(shifts, (S, 2))
        if shifts.shape != (S, 2):
            raise ValueError("window_shift must be (sx, sy) or an (S, 2) array with S = %d, not of shape %r" % (S, shifts.shape))
        shifts = numpy.ascontiguousarray(shifts, dtype=numpy.float32)
        if not numpy.isfinite(shifts).all():
            raise ValueError("the window shift must be finite")
        rows = n1 * S if c1 is None else n1
        pair_counts = numpy.zeros(S, numpy.int64)
        if out == "device":
            import torch
            pairs = torch.empty((rows, 2), dtype=torch.int32, device=torch.device("cuda", self.device))
            pp = pairs.data_ptr()
        else:
            pairs = numpy.empty((rows, 2), dtype=numpy.int32)
            pp = pairs.ctypes.data
        if S == 0:
            return pairs[:0], pair_counts
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_window_batch(self._handle, p1, n1, dev1, p2, n2, dev2, S, None if c1 is None else c1.ctypes.data,
                                                            c2.ctypes.data, C.c_float(th), C.c_float(wx), C.c_float(wy), shifts.ctypes.data,
                                                            int(bool(mutual)), grid_max, pp if rows else None, int(out == "device"),
                                                            pair_counts.ctypes.data))
            if self.profile:
                self.events += self._stage_events()
        total = int(pair_counts.sum())
        return (pairs[:total] if out == "device" else pairs[:total].copy()), pair_counts

    BATCH_MAX_WORK = 1 << 20

    def _estimate_batch_args(self, kp1, counts1, kp2, counts2, pairs, pair_counts, mask):
        """the arguments ``fit_batch`` and ``shift_batch`` share, checked as ``match_batch`` checks its own"""
        p1, dev1, n1, keep1 = self._records(kp1)
        p2, dev2, n2, keep2 = self._records(kp2)
        pp, devp, pdtype, pshape, keepp = _pointer_of(pairs)
        if pdtype != numpy.int32 or len(pshape) != 2 or pshape[1] != 2:
            raise RuntimeError("pairs must be an (M, 2) int32 array")
        n_pairs = int(pshape[0])
        pm, devm, keepm = None, 0, None
        if mask is not None:
            if isinstance(mask, numpy.ndarray) and mask.dtype == numpy.bool_:
                mask = mask.view(numpy.uint8)
            pm, devm, mdtype, mshape, keepm = _pointer_of(mask)
            if mdtype.itemsize != 1 or mdtype.kind not in "bu" or tuple(mshape) != (n_pairs,):
                raise RuntimeError("mask must be an (M,) bool or uint8 array")
        c2 = numpy.ascontiguousarray([int(c) for c in counts2], dtype=numpy.int64).reshape(-1)
        S = len(c2)
        c1 = None if counts1 is None else numpy.ascontiguousarray([int(c) for c in counts1], dtype=numpy.int64).reshape(-1)
        pc = numpy.ascontiguousarray([int(c) for c in pair_counts], dtype=numpy.int64).reshape(-1)
        if S > self.BATCH_MAX_SEGMENTS:
            raise ValueError("%d segments: more than %d" % (S, self.BATCH_MAX_SEGMENTS))
        if c1 is not None and len(c1) != S:
            raise ValueError("counts1 has %d entries, counts2 %d" % (len(c1), S))
        if len(pc) != S:
            raise ValueError("pair_counts has %d entries, counts2 %d" % (len(pc), S))
        if (c2 < 0).any() or (c1 is not None and (c1 < 0).any()) or (pc < 0).any():
            raise ValueError("negative count")
        if int(c2.sum()) != n2 or (c1 is not None and int(c1.sum()) != n1):
            raise ValueError("the counts do not add up to the lists: %s of %d and %d of %d records" %
                             ("-" if c1 is None else int(c1.sum()), n1, int(c2.sum()), n2))
        if int(pc.sum()) != n_pairs:
            raise ValueError("pair_counts add up to %d, there are %d pairs" % (int(pc.sum()), n_pairs))
        args = (self._handle, p1, n1, dev1, p2, n2, dev2, S, None if c1 is None else c1.ctypes.data, c2.ctypes.data,
                pp if n_pairs else None, n_pairs, devp, pc.ctypes.data, pm if n_pairs else None, devm)
        return args, S, n_pairs, pc, (keep1, keep2, keepp, keepm, c1, c2)

    def fit_batch(self, kp1, counts1, kp2, counts2, pairs, pair_counts, mask=None, blocks=0, return_moments=False):
        """``fit(kp1_s, kp2_s, pairs_s, mask_s, blocks)`` for the S segments of a ``match_batch`` in one call: one set of launches and
        one synchronisation, every result bit for bit that of the single call (extension).  The first
        four arguments are ``match_batch``'s, ``pairs`` and ``pair_counts`` its results unchanged (indices local to the segment).
        An index outside its segment's own list makes the pair unused; a record of a neighbouring segment is never read.

        :param kp1, counts1, kp2, counts2: as for ``match_batch`` (``counts1=None``: one shared first list)
        :param pairs: (M, 2) int32 indices, a numpy array or a device tensor
        :param pair_counts: S non-negative ints that add up to M
        :param mask: None, or (M,) bool / uint8 aligned with the rows of ``pairs``, a numpy array or a device tensor
        :param blocks: workgroups per segment, 1 .. 1024 (part of the summation order); 0 picks by the segment's pairs as ``fit`` does
        :return: ``(models, rms, n)``: float64 (S, 6) with NaN rows where a segment has no usable pair or is degenerate, float64
                 (S,) ``sqrt(ssr / n)`` (NaN in those rows) and int64 (S,).  With ``return_moments`` a fourth item: float64 (S, 20),
                 the values of ``siftmi_match_fit`` per segment.
        """
        blocks = int(blocks)
        if blocks < 0 or blocks > 1024:
            raise ValueError("blocks must be 0 .. 1024, not %d" % blocks)
        args, S, n_pairs, pc, hold = self._estimate_batch_args(kp1, counts1, kp2, counts2, pairs, pair_counts, mask)
        work = int(numpy.minimum(256, -(-pc // 256)).sum()) if blocks == 0 else blocks * int((pc > 0).sum())
        if work > self.BATCH_MAX_WORK:
            raise ValueError("%d workgroups in all: more than %d" % (work, self.BATCH_MAX_WORK))
        raw = numpy.empty((S, 20), numpy.float64)
        ms = C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_fit_batch(*args, blocks, raw.ctypes.data, C.byref(ms)))
            if self.profile:
                from .plan import StageEvent
                self.events.append(("fit_batch", StageEvent(ms.value)))      # device time, first kernel to last
        ok = raw[:, 0] == self.FIT_OK
        models = numpy.where(ok[:, None], raw[:, 13:19], numpy.nan)
        with numpy.errstate(all="ignore"):
            rms = numpy.where(ok, numpy.sqrt(raw[:, 19] / raw[:, 1]), numpy.nan)
        result = (models, rms, raw[:, 1].astype(numpy.int64))
        return result + (raw,) if return_moments else result

    def shift_batch(self, kp1, counts1, kp2, counts2, pairs, pair_counts, mask=None, tol=None, return_ranks=False):
        """``shift(kp1_s, kp2_s, pairs_s, mask_s, tol)`` for the S segments of a ``match_batch`` in one call: one launch and one
        synchronisation, every result bit for bit that of the single call (extension).  Arguments as
        for ``fit_batch``; a median does not depend on the launch shape, so there is no ``blocks``.

        :param tol: None, or a distance in pixels >= 0 (``inf`` is allowed): the result gains the keep mask, every row tested
                    against the medians of its own segment, and the kept pairs per segment
        :return: ``(shifts, n)``: float32 (S, 2) ``(dx, dy)`` with NaN rows where no pair is usable, and int64 (S,).  With ``tol``
                 two more items: bool (M,) and int64 (S,); with ``return_ranks`` a last item, float32 (S, 6), the values of
                 ``siftmi_match_shift`` per segment.
        """
        if tol is not None and not float(tol) >= 0.0:
            raise ValueError("tol must be >= 0 (inf is allowed), not %r" % (tol,))
        args, S, n_pairs, pc, hold = self._estimate_batch_args(kp1, counts1, kp2, counts2, pairs, pair_counts, mask)
        raw = numpy.empty((S, 6), numpy.float32)
        counts = numpy.zeros((S, 2), numpy.int64)
        kept = numpy.zeros(n_pairs, numpy.uint8) if tol is not None else None
        ms = C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_shift_batch(*args, C.c_float(0.0 if tol is None else tol),
                                                           kept.ctypes.data if tol is not None else None, raw.ctypes.data,
                                                           counts.ctypes.data, C.byref(ms)))
            if self.profile:
                from .plan import StageEvent
                self.events.append(("shift_batch", StageEvent(ms.value)))    # device time of the kernel
        result = (raw[:, :2].copy(), counts[:, 0].copy())
        if tol is not None:
            result += (kept.view(numpy.bool_), counts[:, 1].copy())
        return result + (raw,) if return_ranks else result

    BATCH_MAX_HYP = 1 << 22

    def consensus_batch(self, kp1, counts1, kp2, counts2, pairs, pair_counts, n_hyp=2048, tol=3.0, seed=0, return_votes=False,
                        out="host"):
        """``consensus(kp1_s, kp2_s, pairs_s, n_hyp, tol, seed)`` for the S segments of a ``match_batch`` in one call: one set of
        launches and one synchronisation, every result bit for bit that of the single call (extension).
        The first six arguments are ``fit_batch``'s; ``n_hyp``, ``tol`` and ``seed`` are ``consensus``'s and hold for every segment.
        An index outside its segment's own list never votes; a record of a neighbouring segment is never read.

        :param kp1, counts1, kp2, counts2: as for ``match_batch`` (``counts1=None``: one shared first list)
        :param pairs: (M, 2) int32 indices local to the segment, a numpy array or a device tensor
        :param pair_counts: S non-negative ints that add up to M
        :param out: ``"host"``: ``mask`` is a numpy bool array; ``"device"``: a torch uint8 tensor on the plan's device that goes
                    into ``fit_batch(mask=)`` / ``shift_batch(mask=)`` as it is, and no mask is copied back
        :return: ``(mask, models, votes)``: (M,) aligned with the rows of ``pairs``, float32 (S, 6) with NaN rows where a segment has
                 no winner (fewer than three pairs, no usable triple: its mask rows are zero) and int32 (S,) votes of the winners;
                 with ``return_votes`` a fourth item ``(winners, votes_all, models_all)``: int32 (S,) with -1 for none, int32
                 (S, n_hyp), float32 (S, n_hyp, 6) with unusable triples as NaN rows
        """
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device', not %r" % (out,))
        n_hyp, tol = int(n_hyp), float(tol)
        if n_hyp < 1 or n_hyp > (1 << 20):
            raise ValueError("n_hyp must be 1 .. 2**20, not %d" % n_hyp)
        if not (abs(tol) <= float(numpy.finfo(numpy.float32).max) and tol > 0.0):      # finite as the float32 the library gets
            raise ValueError("tol must be finite and > 0, not %r" % (tol,))
        args, S, n_pairs, pc, hold = self._estimate_batch_args(kp1, counts1, kp2, counts2, pairs, pair_counts, None)
        if int((pc >= 3).sum()) * n_hyp > self.BATCH_MAX_HYP:
            raise ValueError("%d segments of three pairs or more x %d hypotheses: more than %d" % ((pc >= 3).sum(), n_hyp, self.BATCH_MAX_HYP))
        tiles = int((-(-pc // 1024)).sum())
        if tiles > self.BATCH_MAX_WORK:
            raise ValueError("%d tiles in all: more than %d" % (tiles, self.BATCH_MAX_WORK))
        if out == "device":
            import torch
            mask = torch.empty(n_pairs, dtype=torch.uint8, device=torch.device("cuda", self.device))
            pmask = mask.data_ptr()
        else:
            mask = numpy.empty(n_pairs, numpy.uint8)
            pmask = mask.ctypes.data
        models = numpy.empty((S, 6), numpy.float32)
        winners, votes = numpy.empty(S, numpy.int32), numpy.empty(S, numpy.int32)
        votes_all = numpy.empty((S, n_hyp), numpy.int32) if return_votes else None
        models_all = numpy.empty((S, n_hyp, 6), numpy.float32) if return_votes else None
        ms = C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_match_consensus_batch(
                *args[:-2], n_hyp, C.c_float(tol), int(seed) & 0xFFFFFFFF, pmask if n_pairs else None, int(out == "device"),
                models.ctypes.data, winners.ctypes.data, votes.ctypes.data, votes_all.ctypes.data if return_votes else None,
                models_all.ctypes.data if return_votes else None, C.byref(ms)))
            if self.profile:
                from .plan import StageEvent
                self.events.append(("consensus_batch", StageEvent(ms.value)))    # device time of the vote kernel
        result = (mask if out == "device" else mask.view(numpy.bool_), models, votes)
        return result + ((winners, votes_all, models_all),) if return_votes else result

    def _records(self, kp):
        if isinstance(kp, numpy.ndarray):
            arr = numpy.ascontiguousarray(kp)
            if arr.dtype.itemsize != 144:
                raise RuntimeError("keypoints must be 144-byte (x, y, scale, angle, desc[128]) records")
            return arr.ctypes.data, 0, int(arr.shape[0]), arr
        ptr, is_dev, dtype, shape, keep = _pointer_of(kp)
        nbytes = int(numpy.prod(shape)) * dtype.itemsize
        if nbytes % 144:
            raise RuntimeError("device keypoint buffer is not a whole number of 144-byte records")
        return ptr, is_dev, nbytes // 144, keep

    STAGE_LABELS = ("copy H->D KP_1", "copy H->D KP_2", "matching", "copy D->H match")
    KNN_STAGE_LABELS = ("copy H->D KP_1", "copy H->D KP_2", "knn", "copy D->H knn")

    def _stage_events(self, labels=STAGE_LABELS):
        """The reference's profiling events of one ``match`` call (match.py:226, 237, 261, 263) with the device time of each
        stage in place of the pyopencl event: ``evt.profile.end - evt.profile.start`` is nanoseconds, as there.  A stage that
        did not run (a device-resident list, no pair to copy back) has no entry -- the reference appends none either."""
        from .plan import StageEvent
        ms = (C.c_float * 4)()
        _lib.check(_lib.lib().siftmi_match_last_stage_ms(self._handle, ms))
        return [(label, StageEvent(v)) for label, v in zip(labels, ms) if v >= 0.0]

    def log_profile(self):
        """Print the recorded stage times (the reference's classes share this loop: alignment.py:363-375, plan.py:832-846)"""
        t = 0.0
        if self.profile:
            for label, evt in self.events:
                et = 1e-6 * (evt.profile.end - evt.profile.start)
                print("%50s:\t%.3fms" % (label, et))
                t += et
        print("_" * 80)
        print("%50s:\t%.3fms" % ("Total execution time", t))

    def kernel_ms(self):
        ms = C.c_float()
        _lib.check(_lib.lib().siftmi_match_last_kernel_ms(self._handle, C.byref(ms)))
        return ms.value

    def reset_timer(self):
        with self._sem:
            self.events = []

    def set_roi(self, roi):
        """Defines the region of interest (match.py:312-320): 2D array, non zero where pixels are valid.  As in the
        reference it has no effect on ``match()`` unless ``roi_mode`` is given.  The mask is converted as
        ``numpy.ascontiguousarray(roi, numpy.int8)`` converts it (the reference's line): a uint8 200 becomes -56 and stays
        valid, an int16 256 and a float 0.5 become 0.  A mask that is not 2D is refused and the mask in force stays."""
        with self._sem:
            roi = numpy.ascontiguousarray(roi, numpy.int8)
            if roi.ndim != 2:
                raise RuntimeError("the region of interest must be a 2D array")
            self.roi = roi
            _lib.check(_lib.lib().siftmi_match_set_roi(self._handle, self.roi.ctypes.data, self.roi.shape[1], self.roi.shape[0]))

    def unset_roi(self):
        """Unset the region of interest (match.py:322-327)"""
        with self._sem:
            self.roi = None
            _lib.check(_lib.lib().siftmi_match_set_roi(self._handle, None, 0, 0))
