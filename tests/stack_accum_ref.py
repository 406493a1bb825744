"""The contract of siftmi_batch_stack_accum / siftmi_batch_stack_accum_result (include/siftmi.h; csrc/k_stack_accum.hpp; DESIGN.md
section 7 row 20) restated in numpy, written from the contract text, for tests/test_stack_accum_ref_host.py and
tests/test_gpu_stack_accum.py.  Nothing here imports the package: the GPU state and results are compared with what this file
computes, bit for bit.

State per output pixel o: s1, s2 binary64, coverage, kept int32, all zero before the first call.  A call, one rounding per operation:
    v_s, live_s   stack_ref.samples / warp_cubic_ref.samples_cubic: siftmi_batch_stack[_ex]'s sample and live flag of frame s
    clip given:   m = center[o], tl = (kappa_low * kappa_low) * var[o], th = (kappa_high * kappa_high) * var[o]        (binary32)
    for s ascending, live frames only:
        coverage += 1
        clip given:    d = v_s - m; q = d * d; rejected = (d < 0 && q > tl) || (d > 0 && q > th)  (binary32; NaN anywhere: not rejected)
        not rejected:  s1 = s1 + (double)v_s;  s2 = s2 + (double)v_s * (double)v_s  (the product is exact in binary64);  kept += 1
Result:
    k = kept; k == 0: mean = var = empty
    else M = s1 / (double)k; mean = (float)M; V = s2 / (double)k - M * M; var = (float)(V < 0 ? 0 : V)

The `rule` argument swaps ONE of these rules for a plausible wrong one (MUTANTS): the host test shows that each of them changes a
result on a crafted case, i.e. that the cases can tell the contract from its neighbours.
"""
import numpy as np

import stack_ref
import warp_cubic_ref

F = np.float32
D = np.float64
MUTANTS = ("float32_state", "clip_ge", "kappa_swapped", "clip_coverage", "var_unclamped")


def samples(frames, maps, fills, shape, out_shape, mode=1, interp=None):
    """(values, live) of a chunk under either sampler"""
    if interp == "cubic":
        assert mode == 1
        return warp_cubic_ref.samples_cubic(frames, maps, fills, shape, out_shape)
    assert interp in (None, "linear")
    return stack_ref.samples(frames, maps, fills, shape, out_shape, mode)


class State(object):
    """the four planes of one accumulator; s2 is None without second moments"""

    def __init__(self, out_shape, moments=True, rule=None):
        assert rule is None or rule in MUTANTS
        self.rule = rule
        self.real = F if rule == "float32_state" else D
        self.s1 = np.zeros(out_shape, self.real)
        self.s2 = np.zeros(out_shape, self.real) if moments else None
        self.coverage = np.zeros(out_shape, np.int32)
        self.kept = np.zeros(out_shape, np.int32)

    def copy(self):
        other = State(self.s1.shape, self.s2 is not None, self.rule)
        other.s1, other.coverage, other.kept = self.s1.copy(), self.coverage.copy(), self.kept.copy()
        other.s2 = None if self.s2 is None else self.s2.copy()
        return other

    def planes(self):
        return [p for p in (self.s1, self.s2, self.coverage, self.kept) if p is not None]

    def same(self, other):
        """bit for bit (a NaN sum matches any NaN sum: the payload of a NaN that arithmetic creates belongs to the hardware)"""
        a, b = self.planes(), other.planes()
        if len(a) != len(b):
            return False
        for p, q in zip(a, b):
            if p.dtype != q.dtype or p.shape != q.shape:
                return False
            if p.dtype.kind == "f":
                nan = np.isnan(p) & np.isnan(q)
                u = "u%d" % p.dtype.itemsize
                if not ((p.view(u) == q.view(u)) | nan).all():
                    return False
            elif not np.array_equal(p, q):
                return False
        return True

    def add_samples(self, vals, live, clip=None, kappa=(3.0, 3.0)):
        """one call: the samples (S, OH, OW) float32 and live flags of a chunk, frame after frame"""
        vals = np.asarray(vals)
        assert vals.dtype == F and live.dtype == bool and vals.shape == live.shape and vals.shape[1:] == self.s1.shape
        rule, real = self.rule, self.real
        with np.errstate(all="ignore"):
            if clip is not None:
                center, var = (np.asarray(p) for p in clip)
                assert center.dtype == F and var.dtype == F and center.shape == var.shape == self.s1.shape
                kl, kh = F(kappa[0]), F(kappa[1])
                if rule == "kappa_swapped":
                    kl, kh = kh, kl
                tl, th = (kl * kl) * var, (kh * kh) * var
                assert tl.dtype == F and th.dtype == F
            for s in range(vals.shape[0]):
                v, on = vals[s], live[s]
                keep = on
                if clip is not None:
                    d = v - center
                    q = d * d
                    assert q.dtype == F
                    if rule == "clip_ge":
                        rejected = ((d < 0) & (q >= tl)) | ((d > 0) & (q >= th))
                    else:
                        rejected = ((d < 0) & (q > tl)) | ((d > 0) & (q > th))
                    keep = on & ~rejected
                self.coverage = self.coverage + (keep if rule == "clip_coverage" else on).astype(np.int32)
                w = v.astype(real)
                self.s1 = np.where(keep, self.s1 + w, self.s1)
                if self.s2 is not None:
                    self.s2 = np.where(keep, self.s2 + w * w, self.s2)
                self.kept = self.kept + keep.astype(np.int32)
        assert self.s1.dtype == real and self.coverage.dtype == np.int32 and self.kept.dtype == np.int32
        return self

    def add(self, frames, maps, fills, shape, mode=1, interp=None, clip=None, kappa=(3.0, 3.0)):
        """one call from frames, maps [(M, off)] and fills, as siftmi_batch_stack_accum takes them"""
        if len(frames) == 0:
            return self
        vals, live = samples(frames, maps, fills, shape, self.s1.shape, mode, interp)
        return self.add_samples(vals, live, clip, kappa)

    def result(self, empty=np.nan, var=False):
        """mean float32, or (mean, var)"""
        assert not var or self.s2 is not None
        some = self.kept > 0
        k = np.where(some, self.kept, 1).astype(self.real)
        with np.errstate(all="ignore"):
            M = self.s1 / k
            mean = np.where(some, M.astype(F), F(empty)).astype(F)
            if not var:
                return mean
            V = self.s2 / k - M * M
            if self.rule != "var_unclamped":
                V = np.where(V < 0, self.real(0), V)
            return mean, np.where(some, V.astype(F), F(empty)).astype(F)
