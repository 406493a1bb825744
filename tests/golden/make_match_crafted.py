#!/usr/bin/env python
"""Generate tests/golden/match_crafted.npz from the reference's OWN matching kernel (oracle/Makefile `ref` target, driven by
oracle/pyref.py) on the crafted lists of tests/match_cases.py: the critical-ratio lists of three thresholds, the odd thresholds,
the extremes and the tie lists (GOLDEN_FAMILIES).

Runs only where the reference tree is mounted; tests/test_match_cases_host.py reads only what this script writes.  Nothing from
the reference is copied: the inputs are regenerated from seeds by tests/match_cases.py and only results are stored --

    pairs_<k> / offsets_<k> / totals_<k>   the sorted pairs of every case of family k, concatenated; the row range of case c
                                           is offsets[c]:offsets[c + 1]; totals[c] is the kernel's counter
    digest_<k>                             match_cases.digest() of the family's inputs
    families, n1                           the family names and the number of (identical) queries

    python tests/golden/make_match_crafted.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import match_cases as mc  # noqa: E402
from oracle import pyref  # noqa: E402
from util import sort_rows  # noqa: E402

GOLDEN_N1 = 3


def main():
    assert pyref.build(), "needs the reference tree to build oracle/_ref"
    arrays = {"families": np.array(mc.GOLDEN_FAMILIES), "n1": np.int64(GOLDEN_N1)}
    for k, name in enumerate(mc.GOLDEN_FAMILIES):
        cases = list(mc.family(name, GOLDEN_N1))
        rows, offsets, totals = [], [0], []
        for c in cases:
            pairs, n = pyref.match(c.a, c.b, ratio=c.th, cap=len(c.a))
            assert n == len(pairs)
            rows.append(sort_rows(pairs.reshape(-1, 2)))
            offsets.append(offsets[-1] + len(pairs)); totals.append(n)
        arrays["pairs_%d" % k] = np.concatenate(rows).astype(np.int32)
        arrays["offsets_%d" % k] = np.array(offsets, np.int64)
        arrays["totals_%d" % k] = np.array(totals, np.int64)
        arrays["digest_%d" % k] = np.array(mc.digest(cases))
        print("%-16s %4d cases, %4d of them pair" % (name, len(cases), int((np.array(totals) > 0).sum())))
    np.savez_compressed(os.path.join(HERE, "match_crafted.npz"), **arrays)


if __name__ == "__main__":
    main()
