#!/usr/bin/env python
"""Generate tests/golden/roi_edges_ref.npz from the reference's OWN `matching_valid` kernel (oracle/Makefile `ref` target, driven
by oracle/pyref.py as in make_ref_xcheck.py) on the mode-1 cases of tests/roi_cases.py: the query-flag lists and the one-probe
forced-zero calls of every mask, restricted to probes with x and y in (-1, 2^31) (roi_cases.reference_cases) -- the cast of a
NaN or of anything beyond 2^31 is undefined in the reference too, and below -1 it reads in front of the mask, so it has no answer
to record there.

Runs only where the reference tree is mounted; tests/test_roi_cases_host.py reads only what this script writes.  Nothing from the
reference is copied: the inputs are regenerated from seeds by tests/roi_cases.py and only results are stored --

    pairs_<k> / offsets_<k> / totals_<k>   the sorted pairs of every case of mask k, concatenated; the row range of case c is
                                           offsets[c]:offsets[c + 1]; totals[c] is the kernel's counter
    digest_<k>                             roi_cases.digest() of the mask's cases
    masks                                  the mask names

    python tests/golden/make_roi_edges_ref.py
"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import roi_cases as rc  # noqa: E402
from oracle import pyref  # noqa: E402
from util import sort_rows  # noqa: E402


def save_npz(path, arrays):
    """numpy.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name in sorted(arrays):
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            z.writestr(info, buf.getvalue())


def main():
    assert pyref.build(), "needs the reference tree to build oracle/_ref"
    arrays = {"masks": np.array(list(rc.MASKS))}
    for k, mask in enumerate(rc.MASKS):
        cases = rc.reference_cases(mask)
        rows, offsets, totals = [], [0], []
        for c in cases:
            pairs, n = pyref.match_valid(c.a, c.b, c.roi, ratio=c.th, cap=len(c.a))
            assert n == len(pairs)
            rows.append(sort_rows(pairs.reshape(-1, 2)))
            offsets.append(offsets[-1] + len(pairs)); totals.append(n)
        arrays["pairs_%d" % k] = np.concatenate(rows).astype(np.int32)
        arrays["offsets_%d" % k] = np.array(offsets, np.int64)
        arrays["totals_%d" % k] = np.array(totals, np.int64)
        arrays["digest_%d" % k] = np.array(rc.digest(cases))
        print("%-14s %3d cases, %5d pairs" % (mask, len(cases), offsets[-1]))
    save_npz(os.path.join(HERE, "roi_edges_ref.npz"), arrays)


if __name__ == "__main__":
    main()
