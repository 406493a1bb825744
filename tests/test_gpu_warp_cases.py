"""Stage test of the affine warp (transform_kernel / transform_rgb_kernel, csrc/k_align.hpp) through the C ABI
(include/siftmi.h: siftmi_plan_transform) on the crafted cases of tests/warp_cases.py.  The expected bytes come from the numpy
restatement tests/warp_ref.py alone (checked on the CPU against the oracle and the reference's golden vectors by
tests/test_warp_ref_host.py); every comparison is bit equality, except that a NaN the restatement produces from special values
in the image (family 8) may carry any payload.

  * host path: every case with a host image and a host output
  * pointer paths: device image, device output inside a guarded buffer (0xa5 before and after, checked), RGB output at every
    byte alignment and RGB image at an odd address; the whole output-width list of family 5 again in the guarded form
  * the staged RGB frame (image = NULL), kernel_ms, empty outputs

Sensitivity, measured on scratch builds with one value-only change of k_align.hpp each (first test here that fails; whether
tests/test_gpu_align.py as it stood before this module fails too):
  1 cut at W instead of W - 0.5 (gray, RGB)        f1-rot30-gray-m1         align: fails
  2 gray `0 < tx` instead of `0 <= tx`             f1-identity-gray-m1      align: fails
  3 `mode != 0` instead of `mode == 1`             f3-mode-gray-m2          align: passes
  4 RGB q0 byte loop stops at k < 3                f1-zoom_corner-rgb-m1    align: fails (one pixel of golden case 3)
  5 RGB q1 byte loop stops at k < 3                f1-zoom_corner-rgb-m1    align: fails (one pixel of golden case 3)
  6 RGB px from shift 8c + 16                      f1-rot30-rgb-m1          align: fails
  7 RGB (uint8_t)(interp + 0.5f)                   f1-rot30-rgb-m1          align: fails
  8 RGB w[2] from b[7..10]                         f1-identity-rgb-m1       align: fails
"""
import ctypes as C
import math

import numpy as np
import pytest

import warp_cases as wc
from warp_ref import same, warp_ref

pytestmark = pytest.mark.gpu
GUARD_BYTES = 64 * 4                       # SIFTMI_STAGE_GUARD floats on either side of a device output
_plans = {}


def plan_for(case_image):
    """one SiftPlan per plane shape and element type, shared by every test of the module"""
    import sift_pyocl_amd as sp
    kind, shape = case_image
    rgb = kind in ("rgb", "sat")
    key = (shape, rgb)
    if key not in _plans:
        _plans[key] = sp.SiftPlan(shape=shape + (3,), dtype=np.uint8) if rgb else sp.SiftPlan(shape=shape, dtype=np.float32)
    return _plans[key]


def call(siftlib, plan, image_ptr, image_is_device, rgb, out_ptr, out_is_device, out_shape, M, off, fill, mode, want_rc=0):
    """siftmi_plan_transform with plain addresses; returns kernel_ms"""
    M = np.ascontiguousarray(M, np.float32).reshape(4); off = np.ascontiguousarray(off, np.float32).reshape(2)
    ms = C.c_double(-1.0)
    rc = siftlib.siftmi_plan_transform(plan._handle, image_ptr, image_is_device, 3 if rgb else 1, out_ptr, out_is_device,
                                       out_shape[1], out_shape[0], M.ctypes.data, off.ctypes.data, C.c_float(fill), mode, C.byref(ms))
    assert rc == want_rc, (rc, siftlib.siftmi_last_error())
    return ms.value


def expected(case):
    img = wc.image(case.image)
    want, counts = warp_ref(img, case.M, case.off, case.out_shape, case.fill, case.mode)
    wc.check_expect(case, counts)
    return img, want


def on_device(a, lead=0):
    """(tensor, address): the bytes of `a` in device memory, `lead` bytes behind the start of an allocation"""
    import torch
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    t = torch.empty(lead + raw.size, dtype=torch.uint8, device="cuda")
    t[lead:] = torch.from_numpy(raw.copy()).cuda()
    return t, t.data_ptr() + lead


def guarded_call(siftlib, case, lead=0, image_device=False, image_lead=0):
    """run `case` into a device buffer that sits `lead` bytes behind a 4-byte boundary inside a larger buffer of 0xa5 bytes;
    the payload must be the expected bytes and everything around it must still be 0xa5"""
    import torch
    img, want = expected(case)
    rgb = wc.is_rgb(case)
    assert rgb or (lead == 0 and image_lead == 0), "float32 pointers stay 4-byte aligned"
    plan = plan_for(case.image)
    nbytes = want.nbytes
    buf = torch.full((GUARD_BYTES + lead + nbytes + GUARD_BYTES + 4,), 0xa5, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 4 == 0
    start = GUARD_BYTES + lead
    if image_device:
        keep, iptr = on_device(img, image_lead)
        assert iptr % 4 == image_lead % 4
    else:
        keep, iptr = img, img.ctypes.data
    torch.cuda.synchronize()
    call(siftlib, plan, iptr, int(image_device), rgb, buf.data_ptr() + start, 1, case.out_shape, case.M, case.off, case.fill, case.mode)
    host = buf.cpu().numpy()
    del keep
    got = host[start:start + nbytes].view(want.dtype).reshape(want.shape)
    assert same(got, want), (case.name, lead, image_device, image_lead)
    assert (host[:start] == 0xa5).all(), (case.name, lead, "bytes before the output were written")
    assert (host[start + nbytes:] == 0xa5).all(), (case.name, lead, "bytes behind the output were written")


# ------------------------------------------------------------------------------------------------------------- host path
@pytest.mark.parametrize("case", wc.cases(), ids=lambda c: c.name)
def test_host_path(siftlib, case):
    img, want = expected(case)
    got = np.full(want.shape, 0x5a, want.dtype) if want.dtype == np.uint8 else np.full(want.shape, -77.0, want.dtype)
    ms = call(siftlib, plan_for(case.image), img.ctypes.data, 0, wc.is_rgb(case), got.ctypes.data, 0, case.out_shape, case.M, case.off,
              case.fill, case.mode)
    assert same(got, want, nan_any_payload=case.family == 8), case.name
    assert math.isfinite(ms) and ms >= 0.0


# --------------------------------------------------------------------------------------------------------- pointer paths
POINTER = [wc.by_name(pat % kind) for pat in wc.POINTER_CASES for kind in ("gray", "rgb")]


@pytest.mark.parametrize("case", POINTER, ids=lambda c: c.name)
def test_device_image(siftlib, case):
    import torch
    img, want = expected(case)
    keep, iptr = on_device(img)
    got = np.empty_like(want)
    torch.cuda.synchronize()
    call(siftlib, plan_for(case.image), iptr, 1, wc.is_rgb(case), got.ctypes.data, 0, case.out_shape, case.M, case.off, case.fill, case.mode)
    del keep
    assert same(got, want), case.name


@pytest.mark.parametrize("case", POINTER, ids=lambda c: c.name)
def test_device_output_between_guards(siftlib, case):
    guarded_call(siftlib, case)
    guarded_call(siftlib, case, image_device=True)


@pytest.mark.parametrize("case", [c for c in POINTER if wc.is_rgb(c)], ids=lambda c: c.name)
def test_rgb_unaligned_pointers(siftlib, case):
    for lead in (1, 2, 3):
        guarded_call(siftlib, case, lead=lead)
    guarded_call(siftlib, case, image_device=True, image_lead=1)
    guarded_call(siftlib, case, lead=3, image_device=True, image_lead=3)


@pytest.mark.parametrize("ow", wc.OUT_WIDTHS)
def test_rgb_output_widths_between_guards(siftlib, ow):
    """a dword store one element beyond a row or beyond the output shows here: family 5's widths, device output, all alignments"""
    for oh in wc.OUT_HEIGHTS:
        for name in ("ident", "rot30"):
            case = wc.by_name("f5-%s_%dx%d-rgb-m1" % (name, oh, ow))
            guarded_call(siftlib, case, lead=(oh + ow) % 4)
    guarded_call(siftlib, wc.by_name("f5-rot30_%dx%d-gray-m1" % (5, ow)))


# --------------------------------------------------------------------------------------------- empty outputs, kernel_ms
@pytest.mark.parametrize("kind", ["gray", "rgb"])
@pytest.mark.parametrize("out_shape", [(0, 7), (5, 0), (0, 0)])
def test_empty_output_writes_nothing(siftlib, kind, out_shape):
    import torch
    key = (kind, wc.SMALL)
    img = wc.image(key)
    host = np.full(64, 0x5a, np.uint8)
    ms = call(siftlib, plan_for(key), img.ctypes.data, 0, kind == "rgb", host.ctypes.data, 0, out_shape, [1, 0, 0, 1], [0, 0], 13.0, 1)
    assert ms == 0.0 and (host == 0x5a).all()
    dev = torch.full((64,), 0xa5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ms = call(siftlib, plan_for(key), img.ctypes.data, 0, kind == "rgb", dev.data_ptr() + 32, 1, out_shape, [1, 0, 0, 1], [0, 0], 13.0, 1)
    assert ms == 0.0 and bool((dev == 0xa5).all())


# ---------------------------------------------------------------------------------------------------------- staged frame
def test_staged_rgb_frame(siftlib):
    """image = NULL reads the frame keypoints() left on the device: RGB equals the explicit-image result; a request for the
    other element type is refused"""
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    case = wc.by_name("f1-rot30-rgb-m1")
    img, want = expected(case)
    plan = sp.SiftPlan(template=img)                     # a plan of its own: keypoints() must not disturb the shared ones
    plan.keypoints(img)
    got = np.empty_like(want)
    call(siftlib, plan, None, 0, True, got.ctypes.data, 0, case.out_shape, case.M, case.off, case.fill, case.mode)
    assert same(got, want)
    explicit = np.empty_like(want)
    call(siftlib, plan, img.ctypes.data, 0, True, explicit.ctypes.data, 0, case.out_shape, case.M, case.off, case.fill, case.mode)
    assert same(explicit, got)
    sentinel = np.full(case.out_shape, -77.0, np.float32)
    call(siftlib, plan, None, 0, False, sentinel.ctypes.data, 0, case.out_shape, case.M, case.off, case.fill, case.mode, want_rc=_lib.EINVAL)
    assert (sentinel == -77.0).all()


def test_staged_uint8_gray_frame_is_refused(siftlib):
    """a uint8 gray plan stages uint8 samples: neither a float32 nor an RGB warp may read them"""
    import sift_pyocl_amd as sp
    from sift_pyocl_amd import _lib
    img = np.ascontiguousarray(wc.image(("rgb", wc.SHAPE))[:, :, 0])
    plan = sp.SiftPlan(template=img)
    plan.keypoints(img)
    for rgb in (False, True):
        out = np.full(wc.OUT + ((3,) if rgb else ()), 0x5a, np.uint8 if rgb else np.float32)
        before = out.copy()
        call(siftlib, plan, None, 0, rgb, out.ctypes.data, 0, wc.OUT, [1, 0, 0, 1], [0, 0], 13.0, 1, want_rc=_lib.EINVAL)
        assert same(out, before)
