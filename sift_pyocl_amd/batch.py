"""Batched multi-GPU path: independent images sharded over the GPUs of one node, one process per GPU
(torch.distributed; backend "nccl" is RCCL over xGMI on ROCm, "gloo" on CPU for tests), and ONE exchange
step at the end: an all-gather of the per-image keypoint records.

The reference has no multi-device code at all (one pyopencl.Context per plan, sift-src/plan.py:183);
a user would build one plan per device.  Images are independent, so the data path needs no
collective; only the result hand-back is a collective, and it is small (144 B per keypoint).
"""
import ctypes as C
import logging

import numpy

from . import _lib
from .param import par
from .plan import SiftPlan, _pointer_of

logger = logging.getLogger("sift.batch")
RECORD_BYTES = 144


class BatchPlan(SiftPlan):
    """Throughput form of ``SiftPlan`` for stacks of same-shape frames.

    ``lanes`` independent device plans take the frames round-robin; nothing waits on the host until a lane is
    reused, the records of the whole batch are parked on the device and come back in one copy
    (``siftmi_batch_*`` in include/siftmi.h).  Same constructor keywords as ``SiftPlan`` plus ``lanes`` (default: 16 for frames up to 2048 x 2048, 8 below 600 x 600, 2 for larger ones);
    ``keypoints_batch(images)`` returns one recarray per frame, each bit-identical to ``SiftPlan.keypoints``.
    """

    def __init__(self, *args, **kwargs):
        lanes = kwargs.pop("lanes", None)
        if lanes is None:
            # measured on MI355X: many one-stream lanes for small frames (dependent-launch latency), two three-stream lanes
            # for large ones (one frame nearly fills the GPU)
            shape = kwargs.get("shape") or (kwargs["template"].shape if kwargs.get("template") is not None else (args[0] if args else None))
            # (64 frames, ms per batch, 8 / 16 / 32 lanes: 2048^2 21.6 / 20.0 / 18.9, 1024^2 14.7 / 12.9, 512^2 10.2 / 11.1 --
            # the host thread needs ~0.12 ms to enqueue a frame, which is what bounds the smallest frames)
            px = int(shape[0]) * int(shape[1]) if shape is not None else 0
            lanes = 2 if px == 0 or px > 2048 * 2048 else (16 if px > 600 * 600 else 8)
        self.lanes = int(lanes)
        self._records_per_frame = 4096.0
        self._batch_frames = None            # frames of the last finished batch (minmax_batch)
        self.last_transform_ms = 0.0
        self.last_stack_ms = 0.0
        self._light = kwargs.get("profile") == "light"
        if kwargs.get("profile") and not self._light:
            raise RuntimeError("BatchPlan only supports profile='light' (blur brackets); profile a SiftPlan for per-stage events")
        kwargs["profile"] = False
        SiftPlan.__init__(self, *args, **kwargs)

    def _create(self, L):
        _lib.check(L.siftmi_batch_create(self.shape[0], self.shape[1], self._code, self.device, C.byref(self._params),
                                         self.lanes, C.byref(self._handle)))
        nbytes = C.c_int64()
        _lib.check(L.siftmi_batch_info(self._handle, None, C.byref(nbytes)))
        self.memory = int(nbytes.value)
        if self._light:
            _lib.check(L.siftmi_batch_set_profile(self._handle, 1))

    def _destroy(self, L, h):
        L.siftmi_batch_destroy(h)

    def set_option(self, name, value):
        """SiftPlan.set_option on every lane (``siftmi_batch_set_option``); results never depend on an option."""
        _lib.check(_lib.lib().siftmi_batch_set_option(self._handle, str(name).encode(), int(value)))

    def tail_timeouts(self):
        """(re-runs after a time-out of the small octaves' one-launch form, lanes that still use it): see SiftPlan.tail_timeouts"""
        n, on = C.c_int64(), C.c_int32()
        _lib.check(_lib.lib().siftmi_batch_tail_timeouts(self._handle, C.byref(n), C.byref(on)))
        return int(n.value), int(on.value)

    def blur_times(self):
        """profile='light': hipEvent time, launches and pixels of the full-resolution blur launches of the last batch"""
        ms = C.c_double(); nl = C.c_int64(); px = C.c_double()
        _lib.check(_lib.lib().siftmi_batch_blur_ms(self._handle, C.byref(ms), C.byref(nl), C.byref(px)))
        return {"blur0_ms": ms.value, "blur0_launches": nl.value, "blur0_pixels": px.value}

    def _sync_params(self, L):
        """`par` is read at call time, as in the reference"""
        key = (par.PeakThresh, par.EdgeThresh1, par.EdgeThresh, par.OriSigma, par.BorderDist, par.DoubleImSize)
        if key != self._par_key:
            params = self._current_params()
            _lib.check(L.siftmi_batch_set_params(self._handle, C.byref(params)))
            self._params, self._par_key = params, key

    def _marshal(self, images):
        """pointer table, element-type code, residency flag and keep-alive list of a batch of frames"""
        n = len(images)
        ptrs = (C.c_void_p * n)()
        keep = []
        dev_flags = set()
        code = None
        for i, image in enumerate(images):
            ptr, is_dev, dtype, shape, k = _pointer_of(image)
            assert tuple(shape[:2]) == tuple(self.shape)
            assert dtype in [self.dtype, numpy.float32]
            if dtype == numpy.float32 and len(shape) == 2:
                c = _lib.DTYPE_CODES["float32"]
            elif self.dtype == numpy.float64 and dtype == numpy.float64:
                k = k.float() if is_dev else k.astype(numpy.float32)
                ptr = k.data_ptr() if is_dev else k.ctypes.data
                c = _lib.DTYPE_CODES["float32"]
            elif len(shape) == 3 and dtype == numpy.uint8 and self.RGB:
                c = _lib.DTYPE_CODES["rgb8"]
            elif self.dtype in self.converter and len(shape) == 2:
                c = _lib.DTYPE_CODES[self.dtype.name]
            else:
                raise RuntimeError("invalid input format error (%s)" % (str(self.dtype)))
            if code is None:
                code = c
            elif c != code:
                raise RuntimeError("all frames of a batch must have the same element type")
            ptrs[i] = ptr
            keep.append(k)
            dev_flags.add(int(bool(is_dev)))
        if len(dev_flags) != 1:
            raise RuntimeError("the frames of a batch must be all host arrays or all device tensors")
        return ptrs, code, dev_flags.pop(), keep

    def keypoints_batch(self, images):
        """Keypoints of a sequence of frames (all numpy / host, or all device tensors).

        :return: list of numpy recarrays (x, y, scale, angle, desc[128]), one per frame, in input order
        """
        images = list(images)
        n = len(images)
        if n == 0:
            self._batch_frames = 0
            return []
        with self._sem:
            L = _lib.lib()
            self._sync_params(L)
            ptrs, code, is_dev, keep = self._marshal(images)
            counts = (C.c_int64 * n)()
            offsets = (C.c_int64 * n)()
            parked = C.c_int64(0)
            ovf = C.c_int32(0)
            self._batch_frames = None
            # Records are delivered frame by frame into host arrays while the batch runs.  Their capacity is a guess (1.5x
            # the records per frame of the previous batch); a frame that does not fit stays parked on the device and is
            # fetched afterwards.  Many lanes of small frames: the host must keep feeding the lanes, so everything is
            # parked and fetched with one copy at the end instead.
            direct = self.lanes <= 2
            outs = (C.c_void_p * n)()
            caps = (C.c_int64 * n)()
            arrays = [None] * n
            if direct:
                cap = int(1.5 * self._records_per_frame) + 256
                for i in range(n):
                    arrays[i] = numpy.empty(cap, dtype=self.dtype_kp)
                    outs[i] = arrays[i].ctypes.data
                    caps[i] = cap
            _lib.check(L.siftmi_batch_keypoints_into(self._handle, ptrs, n, code, is_dev, outs if direct else None,
                                                     caps if direct else None, counts, offsets, C.byref(parked), C.byref(ovf)))
            self._batch_frames = n
            self.overflow = bool(ovf.value)
            if self.overflow:
                logger.warning("Keypoint counter overflow: an octave of a frame needs more than %s entries, result cut to that per octave", self.kpsize)
            flat = numpy.empty(0, dtype=self.dtype_kp)      # a batch of blank frames parks nothing
            if parked.value:
                flat = numpy.empty(parked.value, dtype=self.dtype_kp)
                _lib.check(L.siftmi_batch_fetch(self._handle, flat.ctypes.data, 0, 0, parked.value))
            result = []
            for i in range(n):
                if offsets[i] < 0:
                    result.append(arrays[i][:counts[i]].view(numpy.recarray))
                else:
                    result.append(flat[offsets[i]:offsets[i] + counts[i]].view(numpy.recarray))
            self._records_per_frame = max(1.0, sum(counts) / float(n))
            del keep
        return result

    def keypoints_batch_device(self, images):
        """Same as ``keypoints_batch`` but the records stay in HBM: returns ``(counts, records)`` where `records` is a
        torch uint8 tensor on this plan's device holding the 144-byte records of frame 0, frame 1, ... back to back
        (``sum(counts) * 144`` bytes).  This is what the multi-GPU exchange (``gather_records_device``) consumes: no
        host staging between the descriptor kernels and the RCCL all-gather."""
        import torch
        images = list(images)
        n = len(images)
        dev = torch.device("cuda", self.device)
        if n == 0:
            self._batch_frames = 0
            return [], torch.empty(0, dtype=torch.uint8, device=dev)
        with self._sem:
            L = _lib.lib()
            self._sync_params(L)
            ptrs, code, is_dev, keep = self._marshal(images)
            counts = (C.c_int64 * n)()
            offsets = (C.c_int64 * n)()
            parked = C.c_int64(0)
            ovf = C.c_int32(0)
            self._batch_frames = None
            _lib.check(L.siftmi_batch_keypoints_into(self._handle, ptrs, n, code, is_dev, None, None, counts, offsets,
                                                     C.byref(parked), C.byref(ovf)))
            self._batch_frames = n
            self.overflow = bool(ovf.value)
            out = torch.empty(max(1, parked.value) * RECORD_BYTES, dtype=torch.uint8, device=dev)
            if parked.value:
                _lib.check(L.siftmi_batch_fetch(self._handle, out.data_ptr(), 1, 0, parked.value))
            # the arena holds the frames in retirement order; hand them back in input order
            cnt = [int(c) for c in counts]
            off = [int(o) for o in offsets]
            if any(off[i] != sum(cnt[:i]) for i in range(n)):
                parts = [out[off[i] * RECORD_BYTES:(off[i] + cnt[i]) * RECORD_BYTES] for i in range(n)]
                out = torch.cat(parts) if parts else out
            self._records_per_frame = max(1.0, sum(cnt) / float(n))
            del keep
        return cnt, out[:sum(cnt) * RECORD_BYTES]

    def keypoints(self, image):
        return self.keypoints_batch([image])[0]

    __call__ = keypoints

    def minmax_batch(self):
        """``(mins, maxs)`` of the frames of the last finished ``keypoints_batch`` / ``keypoints_batch_device``, two float32
        ``(S,)`` arrays in input order: for every frame the values ``SiftPlan.minmax()`` gives after ``keypoints(frame)``
        (``siftmi_batch_minmax``; nothing is launched).  RuntimeError when no batch has finished."""
        n = self._batch_frames
        if n is None:
            raise RuntimeError("no batch has finished on this plan")
        mins, maxs = numpy.empty(n, numpy.float32), numpy.empty(n, numpy.float32)
        if n:
            with self._sem:
                _lib.check(_lib.lib().siftmi_batch_minmax(self._handle, mins.ctypes.data, maxs.ctypes.data, n))
        return mins, maxs

    #: frames per call of ``transform_batch`` (one grid plane per frame)
    TRANSFORM_MAX_FRAMES = 65535

    def _warp_frames(self, images):
        """(pointer table, residency flag, keep-alive) of the frames of ``transform_batch``: float32 H x W, or uint8 H x W x 3 for an
        RGB plan; nothing is converted."""
        fshape = tuple(self.shape) + ((3,) if self.RGB else ())
        fdtype = numpy.dtype(numpy.uint8 if self.RGB else numpy.float32)
        if hasattr(images, "shape") and hasattr(images, "dtype") and len(images.shape) == len(fshape) + 1:
            images = [images[i] for i in range(int(images.shape[0]))]      # a stack: views of its frames
        else:
            images = list(images)
        n = len(images)
        if n > self.TRANSFORM_MAX_FRAMES:
            raise ValueError("%d frames: more than %d" % (n, self.TRANSFORM_MAX_FRAMES))
        ptrs = (C.c_void_p * max(n, 1))()
        keep, dev_flags = [], set()
        for i, image in enumerate(images):
            if not (isinstance(image, numpy.ndarray) or hasattr(image, "data_ptr") or hasattr(image, "__cuda_array_interface__")):
                raise RuntimeError("frame %d is neither a numpy array nor a tensor" % i)
            ptr, is_dev, dtype, shape, k = _pointer_of(image)
            if tuple(shape) != fshape:
                raise RuntimeError("frame %d has shape %s, the plan warps %s" % (i, tuple(shape), fshape))
            if numpy.dtype(dtype) != fdtype:
                raise RuntimeError("frame %d is %s, the plan warps %s" % (i, dtype, fdtype))
            dev_flags.add(int(bool(is_dev)))
            ptrs[i] = ptr
            keep.append(k)
        if len(dev_flags) > 1:
            raise RuntimeError("the frames of a batch must be all host arrays or all device tensors")
        is_dev = dev_flags.pop() if dev_flags else 0
        # (host frames are not stacked here: the library uploads every run of frames that lie back to back with one copy, so a
        # stack is one copy and separate arrays are one each -- a host-side numpy.stack costs more than the copies it saves)
        return ptrs, n, is_dev, keep

    def _warp_args(self, images, matrices, offsets, fills, out_shape, out):
        """The arguments ``transform_batch`` and ``stack_batch`` share, checked and marshalled: ``(ptrs, n, is_dev, keep, maps, fills,
        oh, ow)`` with `maps` the (n, 6) float32 table of the C ABI and `fills` a contiguous float32 (n,) array."""
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device', not %r" % (out,))
        ptrs, n, is_dev, keep = self._warp_frames(images)
        maps = numpy.empty((n, 6), numpy.float32)
        m = numpy.asarray(matrices, numpy.float32)
        if m.shape not in ((n, 2, 2), (n, 4)) and not (n == 0 and m.size == 0):
            raise ValueError("matrices must be (%d, 2, 2) or (%d, 4), not %s" % (n, n, m.shape))
        o = numpy.asarray(offsets, numpy.float32)
        if o.shape != (n, 2) and not (n == 0 and o.size == 0):
            raise ValueError("offsets must be (%d, 2), not %s" % (n, o.shape))
        maps[:, :4] = m.reshape(n, 4)
        maps[:, 4:] = o.reshape(n, 2)
        f = numpy.asarray(fills, numpy.float32)
        if f.ndim == 0:
            f = numpy.full(n, f, numpy.float32)
        if f.shape != (n,):
            raise ValueError("fills must be a scalar or (%d,), not %s" % (n, f.shape))
        f = numpy.ascontiguousarray(f)
        if self.RGB and n and not ((f >= 0) & (f <= 255)).all():
            raise ValueError("an RGB fill must lie in [0, 255]: a value outside converts a float that uint8 cannot hold")
        oh, ow = (int(v) for v in (self.shape if out_shape is None else out_shape))
        if oh < 0 or ow < 0:
            raise ValueError("negative output shape")
        return ptrs, n, is_dev, keep, maps, f, oh, ow

    def _host_result(self, oshape, odtype):
        """a numpy array for a result: in a pinned block of the library's pool when it fits, an ordinary one otherwise"""
        count = int(numpy.prod(oshape))
        if self.pinned_results and count:
            try:
                return _lib.pinned_empty(count, odtype).reshape(oshape)
            except MemoryError:                 # beyond the pool's limit (_lib.pinned_pool): an ordinary array
                pass
        return numpy.empty(oshape, odtype)

    @_lib.interp_keyword("_transform_batch")
    def transform_batch(self, images, matrices, offsets, fills=0.0, out_shape=None, mode=1, out="host"):
        """Affine warp of S frames of the plan's shape in one launch (``siftmi_batch_transform``): frame s of the result is bit
        for bit ``LinearAlign.transform(matrices[s], offsets[s], images[s], fills[s], mode)``.  One synchronisation, one upload of a
        host stack (separate host arrays: one each) and one copy back of a host result.  A map with a non-finite entry gives ``fills[s]`` wherever it reaches
        (all NaN: the whole plane).  Device memory: the result, plus the frames when they come from the host.

        :param images: S frames, all numpy arrays or all device tensors, or one (S, H, W[, 3]) stack: float32 H x W, or uint8
                       H x W x 3 for an RGB plan (nothing is converted)
        :param matrices: (S, 2, 2) or (S, 4), acting on (y, x) as in ``LinearAlign.transform``
        :param offsets: (S, 2)
        :param fills: a scalar or (S,); for an RGB plan every value must lie in [0, 255]
        :param out_shape: (OH, OW) of every output frame; None: the plan's shape
        :param mode: 1 = bilinear, anything else = the nearest-lower tap
        :param out: ``"host"``: a numpy array (in a pinned block of the library's pool when it fits, as ``LinearAlign.transform``
                    returns it); ``"device"``: a torch tensor on the plan's device
        :param interp: (keyword only) None or ``"linear"``: what `mode` says; ``"cubic"``: the Catmull-Rom bicubic sampler
                    (4 x 4 taps, edge pixels repeated; float32 plans and ``mode=1`` only, ``ValueError`` otherwise; DESIGN.md
                    section 7 row 19).  Frame s is then ``LinearAlign.transform(..., interp="cubic")`` bit for bit
        :return: (S, OH, OW) float32, or (S, OH, OW, 3) uint8
        """
        return self._transform_batch(images, matrices, offsets, fills, out_shape, mode, out)

    def _transform_batch(self, images, matrices, offsets, fills, out_shape, mode, out, interp=None):
        """the body of ``transform_batch``"""
        interp = _lib.interp_code(interp, mode, self.RGB)
        ptrs, n, is_dev, keep, maps, f, oh, ow = self._warp_args(images, matrices, offsets, fills, out_shape, out)
        oshape, odtype = ((n, oh, ow, 3), numpy.uint8) if self.RGB else ((n, oh, ow), numpy.float32)
        if out == "device":
            import torch
            result = torch.empty(oshape, dtype=torch.uint8 if self.RGB else torch.float32, device=torch.device("cuda", self.device))
            optr = result.data_ptr()
        else:
            result = self._host_result(oshape, odtype)
            optr = result.ctypes.data
        ms = C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_batch_transform_ex(self._handle, ptrs, n, is_dev, 3 if self.RGB else 1, optr, int(out == "device"),
                                                            ow, oh, maps.ctypes.data, f.ctypes.data, int(mode), interp, C.byref(ms)))
        self.last_transform_ms = ms.value
        del keep
        return result

    #: the reducers of ``stack_batch`` and their codes in include/siftmi.h
    STACK_REDUCERS = {"sum": 0, "mean": 1, "median": 2}
    #: frames a median may take (SIFTMI_STACK_MEDIAN_MAX)
    STACK_MEDIAN_MAX = 64

    @_lib.interp_keyword("_stack_batch")
    def stack_batch(self, images, matrices, offsets, fills=0.0, out_shape=None, mode=1, reduce="mean", empty=numpy.nan, coverage=False,
                    out="host"):
        """Warp S float32 frames as ``transform_batch`` does and reduce them to ONE plane in the same launch
        (``siftmi_batch_stack``): the S warped planes are never written, only the result crosses the
        link.  Per output pixel a frame is *live* where its warped value is not its fill for a geometric reason -- the source point
        lies in the frame, left of and above the cut at W - 0.5, H - 0.5; a map with a non-finite entry leaves its frame out wherever
        the entry reaches, an all-NaN map everywhere.  The result is, over the live frames of the pixel,

        * ``"sum"``: the float32 sum in the order of the frames,
        * ``"mean"``: that sum divided by their number,
        * ``"median"``: the median in the total order of float32 -- the middle value, or half the sum of the two middle ones
          (``numpy.median`` of the live values wherever they are finite); at most 64 frames,

        and `empty` where no frame is live.  Greyscale plans only.

        :param images, matrices, offsets, fills, out_shape, mode: as for ``transform_batch``
        :param reduce: ``"sum"``, ``"mean"`` or ``"median"``
        :param empty: the value of a pixel that no frame covers
        :param coverage: also return the number of live frames of every pixel
        :param out: ``"host"``: numpy arrays; ``"device"``: torch tensors on the plan's device
        :param interp: (keyword only) as for ``transform_batch``: ``"cubic"`` samples every frame with the bicubic kernel; live
                       frames, coverage and every reducer are unchanged
        :return: the (OH, OW) float32 plane, or ``(plane, coverage)`` with the (OH, OW) int32 counts
        """
        return self._stack_batch(images, matrices, offsets, fills, out_shape, mode, reduce, empty, coverage, out)

    def _stack_batch(self, images, matrices, offsets, fills, out_shape, mode, reduce, empty, coverage, out, interp=None):
        """the body of ``stack_batch``"""
        interp = _lib.interp_code(interp, mode, self.RGB)
        if self.RGB:
            raise RuntimeError("stack_batch reduces float32 frames; an RGB plan has no stack reduction")
        if reduce not in self.STACK_REDUCERS:
            raise ValueError("reduce must be one of %s, not %r" % (sorted(self.STACK_REDUCERS), reduce))
        ptrs, n, is_dev, keep, maps, f, oh, ow = self._warp_args(images, matrices, offsets, fills, out_shape, out)
        if reduce == "median" and n > self.STACK_MEDIAN_MAX:
            raise ValueError("a median takes at most %d frames, not %d" % (self.STACK_MEDIAN_MAX, n))
        if out == "device":
            import torch
            dev = torch.device("cuda", self.device)
            plane = torch.empty((oh, ow), dtype=torch.float32, device=dev)
            cover = torch.empty((oh, ow), dtype=torch.int32, device=dev) if coverage else None
            pptr, cptr = plane.data_ptr(), (cover.data_ptr() if coverage else None)
        else:
            plane = self._host_result((oh, ow), numpy.float32)
            cover = self._host_result((oh, ow), numpy.int32) if coverage else None
            pptr, cptr = plane.ctypes.data, (cover.ctypes.data if coverage else None)
        ms = C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_batch_stack_ex(self._handle, ptrs, n, is_dev, pptr, cptr, int(out == "device"), ow, oh,
                                                        maps.ctypes.data, f.ctypes.data, int(mode), interp, self.STACK_REDUCERS[reduce],
                                                        C.c_float(empty), C.byref(ms)))
        self.last_stack_ms = ms.value
        del keep
        return (plane, cover) if coverage else plane

    #: frames ``stack_clip_batch`` may take (SIFTMI_STACK_CLIP_MAX)
    STACK_CLIP_MAX = 64
    #: the rejection rules of ``stack_clip_batch`` and their codes in include/siftmi.h
    STACK_REJECTS = {"trim": 0, "sigma": 1}

    @classmethod
    def _clip_args(cls, reject, trim, kappa, iters, weights):
        """The rejection parameters of ``stack_clip_batch`` checked as the library checks them: ``(code, n_low, n_high, kappa_low,
        kappa_high, iters, weights)`` with `weights` None or a contiguous float32 vector (its length is the caller's to check)."""
        if reject not in cls.STACK_REJECTS:
            raise ValueError("reject must be one of %s, not %r" % (sorted(cls.STACK_REJECTS), reject))
        try:
            n_low, n_high = (int(v) for v in trim)
            kl, kh = (float(numpy.float32(v)) for v in kappa)
        except TypeError:
            raise ValueError("trim must be (n_low, n_high) and kappa (kappa_low, kappa_high)")
        if (n_low, n_high) != tuple(trim):
            raise ValueError("trim takes whole numbers, not %r" % (trim,))
        if n_low < 0 or n_high < 0 or n_low + n_high > cls.STACK_CLIP_MAX - 1:
            raise ValueError("trim %r: each count must be >= 0 and their sum at most %d" % (trim, cls.STACK_CLIP_MAX - 1))
        if not (kl > 0 and kh > 0):
            raise ValueError("kappa %r: each must be > 0 (inf switches its side off)" % (kappa,))
        if int(iters) != iters or iters < 0:
            raise ValueError("iters must be a whole number >= 0, not %r" % (iters,))
        if weights is not None:
            weights = numpy.ascontiguousarray(weights, numpy.float32)
            if weights.ndim != 1:
                raise ValueError("weights must be one value per frame, not shape %s" % (weights.shape,))
            if not (numpy.isfinite(weights) & (weights > 0)).all():
                raise ValueError("every weight must be finite and > 0")
        return cls.STACK_REJECTS[reject], n_low, n_high, kl, kh, int(iters), weights

    @_lib.interp_keyword("_stack_clip_batch")
    def stack_clip_batch(self, images, matrices, offsets, fills=0.0, out_shape=None, mode=1, reject="sigma", trim=(0, 1), kappa=(3.0, 3.0),
                         iters=3, weights=None, empty=numpy.nan, counts=False, out="host"):
        """Warp S <= 64 float32 frames as ``stack_batch`` does and reduce them to ONE plane in the same launch: per output pixel the
        weighted mean of the live samples that survive an outlier rejection (``siftmi_batch_stack_clip``; DESIGN.md section 7 row
        18).  Samples ``v_s``, live frames and coverage ``c`` are ``stack_batch``'s; everything is float32 with one rounding per
        operation, sums run over the kept frames in the order of the stack and start with their first value.

        * ``reject="trim"``, ``trim=(n_low, n_high)``: the live samples are ordered by value (the total order of float32 that
          ``reduce="median"`` uses; equal values by frame index); with ``h = min(n_high, c - 1)`` and ``l = min(n_low, c - 1 - h)`` the
          `h` largest and the `l` smallest are dropped.  At least one sample stays and the high side is served first; a positive NaN
          sorts above +inf and goes with the high side.
        * ``reject="sigma"``, ``kappa=(kappa_low, kappa_high)``, at most `iters` passes.  A pass over the n kept samples: stop when
          ``n < 3``; ``m = sum(v) / n``, ``d_s = v_s - m``, ``var = sum(d_s * d_s) / n``; sample s is dropped when
          ``d_s < 0 and d_s * d_s > kappa_low**2 * var`` or ``d_s > 0 and d_s * d_s > kappa_high**2 * var``.  A pass that would drop
          nothing ends the iteration; a pass that would drop every sample drops none and ends it.  The statistics are unweighted.
          A NaN or an infinity among the kept samples makes every comparison false: nothing is dropped.  ``kappa = inf``
          switches its side off.
        * the result is ``sum(w_s * v_s) / sum(w_s)`` over the kept samples, `empty` where no frame is live.  Without `weights`
          every ``w_s`` is 1: with nothing rejected (``trim=(0, 0)``, or ``iters=0``) the plane is ``stack_batch(reduce="mean")``'s
          bit for bit.

        n samples cannot hold a z-score above ``(n - 1) / sqrt(n)``: ``kappa = 3`` rejects nothing below 11 live frames.  ``trim``
        is the rule for short stacks.  Greyscale plans only.

        :param images, matrices, offsets, fills, out_shape, mode: as for ``transform_batch``; at most 64 frames
        :param reject: ``"sigma"`` or ``"trim"``; the parameters of the other rule are still checked
        :param trim: (n_low, n_high), each >= 0, their sum at most 63
        :param kappa: (kappa_low, kappa_high), each > 0; ``inf`` is allowed
        :param iters: passes of the sigma rule at most, >= 0
        :param weights: None, or S values, each finite and > 0
        :param empty: the value of a pixel that no frame covers
        :param counts: also return the number of live frames and of kept frames of every pixel
        :param out: ``"host"``: numpy arrays; ``"device"``: torch tensors on the plan's device
        :param interp: (keyword only) as for ``stack_batch``
        :return: the (OH, OW) float32 plane, or ``(plane, coverage, kept)`` with two (OH, OW) int32 planes
        """
        return self._stack_clip_batch(images, matrices, offsets, fills, out_shape, mode, reject, trim, kappa, iters, weights, empty, counts, out)

    def _stack_clip_batch(self, images, matrices, offsets, fills, out_shape, mode, reject, trim, kappa, iters, weights, empty, counts, out,
                          interp=None):
        """the body of ``stack_clip_batch``"""
        interp = _lib.interp_code(interp, mode, self.RGB)
        if self.RGB:
            raise RuntimeError("stack_clip_batch reduces float32 frames; an RGB plan has no stack reduction")
        code, n_low, n_high, kl, kh, iters, w = self._clip_args(reject, trim, kappa, iters, weights)
        ptrs, n, is_dev, keep, maps, f, oh, ow = self._warp_args(images, matrices, offsets, fills, out_shape, out)
        if n > self.STACK_CLIP_MAX:
            raise ValueError("a clipped mean takes at most %d frames, not %d" % (self.STACK_CLIP_MAX, n))
        if w is not None and w.shape != (n,):
            raise ValueError("weights must be one value per frame (%d), not shape %s" % (n, w.shape))
        if out == "device":
            import torch
            dev = torch.device("cuda", self.device)
            plane = torch.empty((oh, ow), dtype=torch.float32, device=dev)
            cover, kept = ((torch.empty((oh, ow), dtype=torch.int32, device=dev) for _ in range(2)) if counts else (None, None))
            pptr, cptr, kptr = plane.data_ptr(), (cover.data_ptr() if counts else None), (kept.data_ptr() if counts else None)
        else:
            plane = self._host_result((oh, ow), numpy.float32)
            cover, kept = ((self._host_result((oh, ow), numpy.int32) for _ in range(2)) if counts else (None, None))
            pptr, cptr, kptr = plane.ctypes.data, (cover.ctypes.data if counts else None), (kept.ctypes.data if counts else None)
        ms = C.c_double(0)
        with self._sem:
            _lib.check(_lib.lib().siftmi_batch_stack_clip_ex(self._handle, ptrs, n, is_dev, pptr, cptr, kptr, int(out == "device"), ow, oh,
                                                             maps.ctypes.data, f.ctypes.data, None if w is None else w.ctypes.data, int(mode),
                                                             interp, code, n_low, n_high, C.c_float(kl), C.c_float(kh), iters,
                                                             C.c_float(empty), C.byref(ms)))
        self.last_stack_ms = ms.value
        del keep
        return (plane, cover, kept) if counts else plane

    def stack_accumulator(self, out_shape=None, moments=False):
        """A ``StackAccumulator`` on this plan: the streaming form of ``stack_batch`` for stacks that are longer than one call
        should hold (``siftmi_batch_stack_accum``).  Greyscale plans only.

        :param out_shape: (OH, OW) of the result; None: the plan's shape
        :param moments: also keep the sum of squares, which ``result(var=True)`` needs
        """
        return StackAccumulator(self, out_shape, moments)

    def minmax(self):
        raise RuntimeError("BatchPlan keeps no per-frame min/max; use SiftPlan")

    def kernel_times(self):
        raise RuntimeError("BatchPlan does not collect per-stage events; profile a SiftPlan instead")


class StackAccumulator(object):
    """Per-pixel running sums of a stack that is fed chunk after chunk (``siftmi_batch_stack_accum``; DESIGN.md section 7 row
    20), made by ``BatchPlan.stack_accumulator``.  The state lives on the plan's device as zeroed torch tensors: ``s1`` (float64,
    the sum of the kept samples), ``s2`` (float64, the sum of their squares; with ``moments`` only), ``coverage`` and ``kept``
    (int32).  Device memory is one chunk of frames plus 16 to 24 bytes per output pixel, whatever the length of the stack, and any
    split of a stack into ``add`` calls gives the same state bit for bit.

    Samples and live frames are ``stack_batch``'s.  Per output pixel and live frame, in the order of the frames: ``coverage += 1``;
    with ``clip=(center, var)`` the sample ``v`` is rejected when ``d = v - center`` has ``d < 0 and d * d > kappa[0]**2 * var`` or
    ``d > 0 and d * d > kappa[1]**2 * var`` (float32; a NaN anywhere rejects nothing); otherwise ``s1 += v``, ``s2 += v * v`` (float64)
    and ``kept += 1``.  ``result`` gives ``s1 / kept`` and the population variance ``max(s2 / kept - mean**2, 0)``.  A first pass
    with ``moments`` and a second one into a fresh accumulator with ``clip=first.result(var=True, out="device")`` is a sigma clip
    of a stack of any length.
    """

    def __init__(self, plan, out_shape=None, moments=False):
        import torch
        if plan.RGB:
            raise RuntimeError("a stack accumulator adds float32 frames; an RGB plan has no stack reduction")
        oh, ow = (int(v) for v in (plan.shape if out_shape is None else out_shape))
        if oh < 0 or ow < 0:
            raise ValueError("negative output shape")
        self.plan = plan
        self.out_shape = (oh, ow)
        self.moments = bool(moments)
        dev = torch.device("cuda", plan.device)
        self._s1 = torch.zeros((oh, ow), dtype=torch.float64, device=dev)
        self._s2 = torch.zeros((oh, ow), dtype=torch.float64, device=dev) if self.moments else None
        self._coverage = torch.zeros((oh, ow), dtype=torch.int32, device=dev)
        self._kept = torch.zeros((oh, ow), dtype=torch.int32, device=dev)
        #: the number of frames added so far
        self.frames = 0
        self.last_stack_ms = 0.0

    def state(self):
        """the live state tensors: ``s1``, ``coverage``, ``kept`` and, with moments, ``s2``"""
        res = {"s1": self._s1, "coverage": self._coverage, "kept": self._kept}
        if self.moments:
            res["s2"] = self._s2
        return res

    def reset(self):
        """zero the state: the accumulator is as it was made"""
        for t in self.state().values():
            t.zero_()
        self.frames = 0

    def _plane(self, plane, name):
        """a clip plane as a contiguous float32 device tensor of the output's shape (host planes are uploaded)"""
        import torch
        dev = self._s1.device
        if isinstance(plane, torch.Tensor):
            if plane.dtype != torch.float32 or tuple(plane.shape) != self.out_shape:
                raise ValueError("%s must be float32 %s, not %s %s" % (name, self.out_shape, plane.dtype, tuple(plane.shape)))
            return plane.to(dev).contiguous()
        plane = numpy.asarray(plane)
        if plane.dtype != numpy.float32 or plane.shape != self.out_shape:
            raise ValueError("%s must be float32 %s, not %s %s" % (name, self.out_shape, plane.dtype, plane.shape))
        return torch.from_numpy(numpy.ascontiguousarray(plane)).to(dev)

    def add(self, images, matrices, offsets, fills=0.0, mode=1, *, interp=None, clip=None, kappa=(3.0, 3.0)):
        """Warp S more frames as ``stack_batch`` does and add them to the state in one launch.

        :param images, matrices, offsets, fills, mode: as for ``stack_batch``
        :param interp: as for ``stack_batch``
        :param clip: None, or ``(center, var)``: two (OH, OW) float32 planes, numpy arrays (uploaded) or device tensors
        :param kappa: (kappa_low, kappa_high) of the clip, each > 0; ``inf`` switches its side off
        :return: the accumulator
        """
        plan = self.plan
        code = _lib.interp_code(interp, mode, plan.RGB)
        ptrs, n, is_dev, keep, maps, f, oh, ow = plan._warp_args(images, matrices, offsets, fills, self.out_shape, "device")
        try:
            kl, kh = (float(numpy.float32(v)) for v in kappa)
        except (TypeError, ValueError):
            raise ValueError("kappa must be (kappa_low, kappa_high), not %r" % (kappa,))
        center = var = None
        if clip is not None:
            try:
                center, var = clip
            except (TypeError, ValueError):
                raise ValueError("clip must be (center, var)")
            center, var = self._plane(center, "the clip's centre"), self._plane(var, "the clip's variance")
            if not (kl > 0 and kh > 0):
                raise ValueError("kappa %r: each must be > 0 (inf switches its side off)" % (kappa,))
        ms = C.c_double(0)
        with plan._sem:
            _lib.check(_lib.lib().siftmi_batch_stack_accum(
                plan._handle, ptrs, n, is_dev, self._s1.data_ptr(), self._s2.data_ptr() if self.moments else None,
                self._coverage.data_ptr(), self._kept.data_ptr(), ow, oh, maps.ctypes.data, f.ctypes.data, int(mode), code,
                None if center is None else center.data_ptr(), None if var is None else var.data_ptr(), C.c_float(kl), C.c_float(kh),
                C.byref(ms)))
        self.last_stack_ms = plan.last_stack_ms = ms.value
        self.frames += n
        del keep, center, var
        return self

    def result(self, empty=numpy.nan, var=False, counts=False, out="host"):
        """The mean of the kept samples of every pixel, `empty` where none was kept.

        :param empty: the value of a pixel without a kept sample, in the mean and in the variance
        :param var: also return the population variance (float32, not rooted); needs ``moments``
        :param counts: also return ``coverage`` and ``kept``, the (OH, OW) int32 numbers of live and of kept samples
        :param out: ``"host"``: numpy arrays; ``"device"``: torch tensors on the plan's device (the counts are copies of the state)
        :return: ``mean``, or ``(mean[, var][, coverage, kept])``
        """
        if out not in ("host", "device"):
            raise ValueError("out must be 'host' or 'device', not %r" % (out,))
        if var and not self.moments:
            raise ValueError("the variance needs an accumulator made with moments=True")
        plan = self.plan
        oh, ow = self.out_shape
        if out == "device":
            import torch
            mean = torch.empty((oh, ow), dtype=torch.float32, device=self._s1.device)
            vplane = torch.empty((oh, ow), dtype=torch.float32, device=self._s1.device) if var else None
            mptr, vptr = mean.data_ptr(), (vplane.data_ptr() if var else None)
        else:
            mean = plan._host_result((oh, ow), numpy.float32)
            vplane = plan._host_result((oh, ow), numpy.float32) if var else None
            mptr, vptr = mean.ctypes.data, (vplane.ctypes.data if var else None)
        ms = C.c_double(0)
        with plan._sem:
            _lib.check(_lib.lib().siftmi_batch_stack_accum_result(
                plan._handle, self._s1.data_ptr(), self._s2.data_ptr() if self.moments else None, self._kept.data_ptr(), ow, oh, mptr, vptr,
                int(out == "device"), C.c_float(empty), C.byref(ms)))
        res = (mean,) + ((vplane,) if var else ())
        if counts:
            if out == "device":
                res += (self._coverage.clone(), self._kept.clone())
            else:
                res += (self._coverage.cpu().numpy(), self._kept.cpu().numpy())
        return res if len(res) > 1 else mean


def shard_indices(n_items, rank, world_size):
    """Round-robin ownership: image i is processed by rank i % world_size."""
    return list(range(rank, n_items, world_size))


def gather_records(local_records, n_items, rank, world_size, device=None, group=None):
    """All-gather per-image record arrays.

    :param local_records: list of (n_i,) dtype_kp arrays for the images owned by this rank, in the
                          order of shard_indices(n_items, rank, world_size)
    :return: list of n_items arrays (every rank gets every image's keypoints)
    """
    import torch
    import torch.distributed as dist

    mine = shard_indices(n_items, rank, world_size)
    assert len(mine) == len(local_records)
    per_rank = (n_items + world_size - 1) // world_size
    counts = torch.zeros(per_rank, dtype=torch.int64)
    for j, rec in enumerate(local_records):
        counts[j] = len(rec)
    dev = torch.device(device) if device is not None else torch.device("cpu")
    counts = counts.to(dev)
    all_counts = torch.empty(world_size * per_rank, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(all_counts, counts, group=group)
    all_counts = all_counts.cpu().view(world_size, per_rank)
    # one padded byte buffer per rank; the payload is latency- not bandwidth-bound
    max_total = int(all_counts.sum(dim=1).max().item())
    payload = torch.zeros(max(1, max_total) * RECORD_BYTES, dtype=torch.uint8)
    at = 0
    for rec in local_records:
        raw = numpy.ascontiguousarray(rec).view(numpy.uint8).reshape(-1)
        payload[at:at + raw.size] = torch.from_numpy(raw.copy())
        at += raw.size
    payload = payload.to(dev)
    gathered = torch.empty(world_size * payload.numel(), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(gathered, payload, group=group)
    gathered = gathered.cpu().numpy().reshape(world_size, -1)
    out = [None] * n_items
    for r in range(world_size):
        at = 0
        for j, idx in enumerate(shard_indices(n_items, r, world_size)):
            n = int(all_counts[r, j].item())
            chunk = gathered[r, at:at + n * RECORD_BYTES]
            out[idx] = chunk.copy().view(SiftPlan.dtype_kp).view(numpy.recarray)
            at += n * RECORD_BYTES
    return out


def gather_records_device(counts, records, n_items, rank, world_size, group=None):
    """The exchange step on device tensors (backend "nccl" = RCCL over xGMI): all-gather of the per-image counts, then
    of the record bytes padded to the largest per-rank total.  Nothing is staged through the host; the only host
    read-back is the (world_size x per_rank) count table that sizes the payload.

    :param counts: records per owned image, in the order of shard_indices(n_items, rank, world_size)
    :param records: torch uint8 device tensor, the owned images' records back to back
    :return: (all_counts, gathered): all_counts[r][j] = records of the j-th image of rank r (python ints); gathered =
             device uint8 tensor (world_size, max_total * 144): row r holds rank r's records back to back
    """
    import torch
    import torch.distributed as dist

    dev = records.device
    per_rank = (n_items + world_size - 1) // world_size
    mine = torch.zeros(per_rank, dtype=torch.int64)
    mine[:len(counts)] = torch.tensor([int(c) for c in counts], dtype=torch.int64) if counts else mine[:0]
    mine = mine.to(dev)
    table = torch.empty(world_size * per_rank, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(table, mine, group=group)
    table = table.view(world_size, per_rank)
    all_counts = table.cpu().tolist()                       # 8 bytes per image: sizes the payload
    max_total = max(1, max(sum(row) for row in all_counts))
    payload = torch.zeros(max_total * RECORD_BYTES, dtype=torch.uint8, device=dev)
    payload[:records.numel()] = records
    gathered = torch.empty(world_size * payload.numel(), dtype=torch.uint8, device=dev)
    dist.all_gather_into_tensor(gathered, payload, group=group)
    return all_counts, gathered.view(world_size, -1)


def split_gathered(all_counts, gathered, n_items, world_size):
    """Per-image numpy recarrays from the result of gather_records_device (one device-to-host copy of everything)."""
    host = gathered.cpu().numpy()
    out = [None] * n_items
    for r in range(world_size):
        at = 0
        for j, idx in enumerate(shard_indices(n_items, r, world_size)):
            n = int(all_counts[r][j])
            out[idx] = host[r, at:at + n * RECORD_BYTES].copy().view(SiftPlan.dtype_kp).view(numpy.recarray)
            at += n * RECORD_BYTES
    return out


def keypoints_batch(images, plan=None, rank=None, world_size=None, gather=True, device=None, **plan_kwargs):
    """Keypoints of a list of same-shape images, sharded over the ranks of the default process group.

    Each rank runs its share through a ``BatchPlan`` (pipelined, one result copy); without an initialised process
    group everything runs on one GPU.  Every rank must pass the same `images` list (only the owned ones are touched).
    A ``SiftPlan`` passed as `plan` is used frame by frame.  With the "nccl" backend (RCCL) the exchange runs on device
    tensors end to end (``gather_records_device``); other backends (the gloo rehearsal on CPU) stage through the host.
    """
    import torch.distributed as dist

    if rank is None or world_size is None:
        if dist.is_available() and dist.is_initialized():
            rank, world_size = dist.get_rank(), dist.get_world_size()
        else:
            rank, world_size = 0, 1
    mine = shard_indices(len(images), rank, world_size)
    plan_given = plan is not None
    if plan is None and mine:
        plan = BatchPlan(template=images[mine[0]], **plan_kwargs)
    # The exchange path must be the same on every rank, so it is chosen from rank-independent facts only: the backend
    # and the kind of plan the caller passed (a rank that owns no frame has no plan at all: plan is None there).
    nccl = gather and world_size > 1 and dist.is_initialized() and dist.get_backend() == "nccl"
    on_device = nccl and (plan is None or isinstance(plan, BatchPlan))
    if nccl:
        # ... and agreed explicitly: a rank without frames (plan is None) would pick the device path while ranks that were
        # handed a frame-by-frame SiftPlan pick the host-staged one -- two different collective sequences, i.e. a hang; the
        # same if only some ranks pass a plan.  One 12-byte all-reduce (MIN) settles "every rank can take the device path"
        # for everybody and shows whether `plan` was given on all ranks or on none (MIN of the flag and of its negation);
        # every rank takes part whatever it was handed, so a mismatch is an error on every rank instead of a hang on some.
        # (Cost: one small collective + one .item() per batch, ~30 us beside milliseconds of frames.)
        import torch
        flag = torch.tensor([1 if on_device else 0, 1 if plan_given else 0, 0 if plan_given else 1], dtype=torch.int32,
                            device=torch.device("cuda", torch.cuda.current_device()))
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        agreed = [int(v) for v in flag.tolist()]
        if agreed[1] == 0 and agreed[2] == 0:
            raise RuntimeError("keypoints_batch: `plan` was passed on some ranks and not on others; pass it on every rank or on none")
        on_device = bool(agreed[0])
    if on_device:
        import torch
        if isinstance(plan, BatchPlan):
            counts, records = plan.keypoints_batch_device([images[i] for i in mine])
        else:                                # empty shard (fewer frames than ranks): joins the collectives with nothing
            counts = []
            records = torch.empty(0, dtype=torch.uint8, device=torch.device("cuda", torch.cuda.current_device()))
        all_counts, gathered = gather_records_device(counts, records, len(images), rank, world_size)
        return split_gathered(all_counts, gathered, len(images), world_size)
    if nccl and device is None:              # frame-by-frame SiftPlan under RCCL: the collectives need device tensors
        import torch
        device = torch.device("cuda", torch.cuda.current_device())
    if isinstance(plan, BatchPlan):
        local = plan.keypoints_batch([images[i] for i in mine])
    else:
        local = [plan.keypoints(images[i]) for i in mine] if mine else []
    if not gather or world_size == 1:
        if world_size == 1:
            return local
        return {i: k for i, k in zip(mine, local)}
    return gather_records(local, len(images), rank, world_size, device=device)


def match_sharded(kp1, kp2, plan=None, rank=None, world_size=None, device=None, matcher=None):
    """``MatchPlan.match(kp1, kp2, raw_results=True)`` with the QUERIES split over the ranks: rank r scans the
    contiguous slice ``kp1[r * n1 // N : (r + 1) * n1 // N]`` against the whole second list (every rank holds it: 14.4 MB
    at 100 k keypoints), then one all-gather of the pair counts and one of the (i, j) pairs -- a query's result does not
    depend on any other query (matching_cpu.cl:67-108), so the union is the single-device result (in rank order; the
    reference does not define an order either).  Every rank returns all the pairs.

    :param kp1, kp2: host recarrays of 144-byte records, the same on every rank
    :param plan: a ``MatchPlan`` of this rank (created when None); `matcher(a, b) -> (n, 2) int array` replaces it (tests)
    """
    import torch
    import torch.distributed as dist

    if rank is None or world_size is None:
        if dist.is_available() and dist.is_initialized():
            rank, world_size = dist.get_rank(), dist.get_world_size()
        else:
            rank, world_size = 0, 1
    n1 = len(kp1)
    lo, hi = rank * n1 // world_size, (rank + 1) * n1 // world_size
    if matcher is None:
        if plan is None:
            from .match import MatchPlan
            plan = MatchPlan(size=max(1, min(hi - lo, len(kp2))))
        matcher = lambda a, b: plan.match(a, b, raw_results=True)      # noqa: E731
    mine = numpy.asarray(matcher(kp1[lo:hi], kp2), dtype=numpy.int32).reshape(-1, 2) if hi > lo and len(kp2) else numpy.empty((0, 2), numpy.int32)
    mine = mine.copy()
    mine[:, 0] += lo
    if world_size == 1:
        return mine
    return gather_pairs(mine, world_size, device=device)


def gather_pairs(mine, world_size, device=None, group=None):
    """The exchange of ``match_sharded``: all-gather of the pair counts, then of the (i, j) pairs padded to the largest
    count; with the "nccl" backend on device tensors.  Every rank returns the pairs of all ranks, in rank order."""
    import torch
    import torch.distributed as dist

    nccl = dist.get_backend(group) == "nccl"
    dev = torch.device(device) if device is not None else (torch.device("cuda", torch.cuda.current_device()) if nccl else torch.device("cpu"))
    counts = torch.empty(world_size, dtype=torch.int64, device=dev)
    dist.all_gather_into_tensor(counts, torch.tensor([len(mine)], dtype=torch.int64, device=dev), group=group)
    counts = counts.cpu().tolist()
    width = max(1, max(counts))
    payload = torch.zeros((width, 2), dtype=torch.int32)
    payload[:len(mine)] = torch.from_numpy(numpy.ascontiguousarray(mine, dtype=numpy.int32).reshape(-1, 2))
    gathered = torch.empty((world_size * width, 2), dtype=torch.int32, device=dev)
    dist.all_gather_into_tensor(gathered, payload.to(dev), group=group)
    gathered = gathered.cpu().numpy().reshape(world_size, width, 2)
    return numpy.concatenate([gathered[r, :counts[r]] for r in range(world_size)], axis=0)
