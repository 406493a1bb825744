#!/usr/bin/env python
"""Generate the fixture of tests/test_oracle_vs_ref.py from the reference's OWN kernels.

Runs only where /root/reference is mounted (oracle/Makefile `ref` target, see make_golden.py); the test itself
reads only what this script writes.  Nothing from the reference is copied: the outputs are data (synthetic inputs
-> reference outputs).  Inputs are regenerated from seeds by tests/util.py, except the two keypoint lists of the
match case, which the oracle computes and which are stored beside the reference's pairs.

    python tests/golden/make_ref_xcheck.py

Fixtures:
  ref_xcheck.npz   pipeline_<seed>                 sorted keypoints of the glibc-backed build, PIPELINE_CASES
                   glibc_<name>_rows / _records    the digest_cases() images through the glibc-backed build, stored as
                                                   the rows (sort_kp order) in which they differ from the siftmath-backed
                                                   build, whose digests are tests/golden/kp_digests.json
                   double_im_size                  sorted keypoints, DoubleImSize = 1, siftmath-backed build
                   to_float_<dtype>                converter outputs of converter_inputs()
                   taps_<i>                        Gaussian taps of XCHECK_SIGMAS[i]
                   match_k1 / match_k2 / match_pairs / match_total
                   valid_<step>_pairs / _total     matching_valid over matching_valid_steps()
  ref_xcheck.json  glibc_<name>                    kp_digest of the glibc-backed build's full output (the rows above
                                                   patched into the siftmath build's records must reproduce it)
                   transform                       {case: array_digest} of transform_xcheck_cases()
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import pyoracle, pyref  # noqa: E402
from util import (PIPELINE_CASES, XCHECK_SIGMAS, array_digest, converter_inputs, digest_cases, kp_digest,  # noqa: E402
                  matching_valid_inputs, matching_valid_steps, pipeline_input, smooth_noise, sort_kp, sort_rows,
                  transform_xcheck_cases)

GLIBC_CASES = ("smooth2048", "smooth1031x1537")


def rows_differing(a, b):
    return np.nonzero((a.view(np.uint8).reshape(len(a), -1) != b.view(np.uint8).reshape(len(b), -1)).any(axis=1))[0]


def main():
    assert pyref.build(), "needs /root/reference to build oracle/_ref"
    pyoracle.build()
    arrays, meta = {}, {}
    for seed, shape, smooth in PIPELINE_CASES:
        arrays["pipeline_%d" % seed] = sort_kp(pyref.keypoints(pipeline_input(seed, shape, smooth)))
    golden = json.load(open(os.path.join(HERE, "kp_digests.json")))
    for name in GLIBC_CASES:
        maker, shape, kw = digest_cases()[name]
        img = maker(shape, **kw)
        g = sort_kp(pyref.keypoints(img))
        pyref.use("siftmath")
        s = sort_kp(pyref.keypoints(img))
        pyref.use("glibc")
        assert kp_digest(s) == golden[name] and len(g) == len(s)
        rows = rows_differing(g, s)
        arrays["glibc_%s_rows" % name] = rows.astype(np.int32)
        arrays["glibc_%s_records" % name] = g[rows]
        meta["glibc_" + name] = kp_digest(g)
        print(name, len(g), "keypoints,", len(rows), "rows differ from the siftmath build")
    pyref.use("siftmath")
    pyref.PAR["DoubleImSize"] = 1
    arrays["double_im_size"] = sort_kp(pyref.keypoints(smooth_noise((200, 333), seed=21, sigma=2.5)))
    pyref.PAR["DoubleImSize"] = 0
    pyref.use("glibc")
    for name, raw in converter_inputs().items():
        arrays["to_float_" + name] = pyref.to_float(raw)
    for i, sigma in enumerate(XCHECK_SIGMAS):
        arrays["taps_%d" % i] = pyref.gaussian_taps(sigma, pyref.kernel_size(sigma))
    img = smooth_noise((220, 220), seed=31)
    k1 = pyoracle.keypoints(img)
    k2 = pyoracle.keypoints(np.roll(img, (3, 4), axis=(0, 1)))
    pairs, n = pyref.match(k1, k2, cap=len(k1))
    arrays.update(match_k1=k1, match_k2=k2, match_pairs=sort_rows(pairs), match_total=np.int64(n))
    a, b, roi = matching_valid_inputs()
    for label, bs in matching_valid_steps(b, roi):
        pairs, n = pyref.match_valid(a, bs, roi)
        arrays["valid_%s_pairs" % label] = sort_rows(pairs)
        arrays["valid_%s_total" % label] = np.int64(n)
    meta["transform"] = {name: array_digest(pyref.transform(im, M, off, out_shape=osh, fill=fill, mode=mode))
                         for name, im, M, off, osh, fill, mode in transform_xcheck_cases()}
    np.savez_compressed(os.path.join(HERE, "ref_xcheck.npz"), **arrays)
    with open(os.path.join(HERE, "ref_xcheck.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
