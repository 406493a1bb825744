#!/usr/bin/env python
"""Generate tests/golden/math_hard.npz: float32 arguments of expf / atan2f whose binary64 value -- the one the defining
function rounds to binary32 (oracle.expf_f64_array / atan2f_f64_array) -- lies close to a binary32 rounding boundary, where
siftmath's device fast paths must hand over to the defining function (tests/math_hard_cases.py describes strata and bands;
tests/test_math_hard_host.py and tests/test_gpu_math_hard.py read the file).

Random arguments reach these bands about once in 4000 (within 65536 binary64 ulps) to once in 4 * 10^6 (within 64), so the
search is in C (oracle/math_hard_scan.c, `make -C oracle hardscan`).  The exp strata are finite sets of floats -- 2 * 10^9 with
|x| <= 80 -- and are walked exhaustively: a band that holds fewer arguments than KEEP asks for is stored whole (50 floats of
[-12, 0] lie within 64 ulps, 2 of the 7 * 10^6 at the ends of the reduction interval), a fuller one gives its first KEEP in a
hashed order.  atan2 operand pairs are drawn, ~10^9 per stratum, until every band is full; draw i depends on (SEED, stratum, i)
alone and the walk stops at a whole chunk.  Either way the file is reproduced byte for byte (about 40 s on 8 cores).
Stored: the arguments with their stratum and band, and the range cases (arguments outside the fast paths' guarded range).  No
expected values: the live oracle gives them.

    python tests/golden/make_math_hard.py
"""
import ctypes as C
import io
import os
import subprocess
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import math_hard_cases as mh  # noqa: E402
from oracle import pyoracle  # noqa: E402

SEED = 20261020
CHUNK = 1 << 27                 # draws per call of the search
MAX_CHUNKS = 40
KEEP = {mh.H0: 200, mh.H1: 3000, mh.G: 1500, mh.S: 6000}       # arguments kept per stratum and band


def scan_lib():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "hardscan"])
    L = C.CDLL(os.path.join(ROOT, "oracle", "libmathhardscan.so"))
    L.mh_scan_atan2.restype = C.c_int64
    L.mh_scan_atan2.argtypes = [C.c_int, C.c_uint64, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64]
    L.mh_scan_exp.restype = C.c_int64
    L.mh_scan_exp.argtypes = [C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_void_p, C.c_int64]
    return L


def mix(z):
    """splitmix64's finaliser on a uint64 array: the order in which a band's arguments are chosen"""
    z = z.astype(np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def report(name, stratum, what, band, keep):
    print("%-5s stratum %s: %s; in band %s, kept %s" % (
        name, "abc"[stratum], what, {mh.BAND_NAMES[k]: int((band == k).sum()) for k in sorted(KEEP)},
        {mh.BAND_NAMES[k]: int((band[keep] == k).sum()) for k in sorted(KEEP)}))


def search_exp(L, stratum):
    """Every float of the stratum is walked (the strata are finite: a band may hold fewer arguments than KEEP asks for, and then
    all of them are kept); where a band holds more, the first KEEP[band] in the order of mix(SEED + bits)."""
    cap = 1 << 22
    buf = np.empty(cap, np.uint32)
    found = []
    top = int(np.array([80.0], np.float32).view(np.uint32)[0]) + 1
    for lo, hi in ((0, top), (1 << 31, (1 << 31) + top)):
        for b0 in range(lo, hi, CHUNK):
            n = L.mh_scan_exp(stratum, b0, min(CHUNK, hi - b0), mh.D_MAX, buf.ctypes.data, cap)
            assert n <= cap
            found.append(buf[:n].copy())
    bits = np.sort(np.concatenate(found))
    x = bits.view(np.float32)
    band = mh.band_of(pyoracle.boundary_distance(pyoracle.expf_f64_array(x)))
    order = np.argsort(mix(bits.astype(np.uint64) + np.uint64(SEED)), kind="stable")
    keep = np.sort(np.concatenate([order[band[order] == k][:KEEP[k]] for k in sorted(KEEP)]))
    keep = keep[np.argsort(band[keep], kind="stable")]
    report("exp", stratum, "%d floats near a boundary" % bits.size, band, keep)
    return x[keep], x[keep], band[keep].astype(np.uint8)


def search_atan2(L, stratum):
    """the first KEEP[band] distinct operand pairs of every band, by draw index"""
    cap = CHUNK // 1000
    a = np.empty(cap, np.float32); b = np.empty(cap, np.float32); idx = np.empty(cap, np.int64)
    got_a, got_b = [], []
    for chunk in range(MAX_CHUNKS):
        n = L.mh_scan_atan2(stratum, SEED, chunk * CHUNK, CHUNK, mh.D_MAX, a.ctypes.data, b.ctypes.data, idx.ctypes.data, cap)
        assert n <= cap
        order = np.argsort(idx[:n])
        got_a.append(a[:n][order].copy()); got_b.append(b[:n][order].copy())
        ya, xa = np.concatenate(got_a), np.concatenate(got_b)
        # distinct arguments, first occurrence kept (the coarse gradient-like operands repeat)
        key = ya.view(np.uint32).astype(np.uint64) << np.uint64(32) | xa.view(np.uint32).astype(np.uint64)
        first = np.sort(np.unique(key, return_index=True)[1])
        ya, xa = ya[first], xa[first]
        band = mh.band_of(pyoracle.boundary_distance(pyoracle.atan2f_f64_array(ya, xa)))
        if all((band == k).sum() >= KEEP[k] for k in KEEP):
            break
    else:
        raise SystemExit("atan2 stratum %d: not enough arguments after %d chunks" % (stratum, MAX_CHUNKS))
    keep = np.concatenate([np.nonzero(band == k)[0][:KEEP[k]] for k in sorted(KEEP)])
    report("atan2", stratum, "%d draws" % ((chunk + 1) * CHUNK), band, keep)
    return ya[keep], xa[keep], band[keep].astype(np.uint8)


def write_npz(path, arrays):
    """np.savez_compressed with fixed member timestamps, so that the same arrays give the same bytes"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, arr in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arr), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    L = scan_lib()
    out = {}
    for func, name in ((0, "exp"), (1, "atan2")):
        ys, xs, strata, bands = [], [], [], []
        for stratum in range(3):
            y, x, band = search_exp(L, stratum) if func == 0 else search_atan2(L, stratum)
            ys.append(y); xs.append(x); bands.append(band); strata.append(np.full(y.size, stratum, np.uint8))
        if func == 0:                                             # 80.0f and its neighbours inside the guarded range: no band claimed
            edge = mh.exp_edge_inside()
            ys.append(edge); xs.append(edge); bands.append(np.full(edge.size, mh.NO_BAND, np.uint8)); strata.append(np.full(edge.size, 2, np.uint8))
            out["exp_x"] = np.concatenate(ys)
        else:
            out["atan2_y"] = np.concatenate(ys); out["atan2_x"] = np.concatenate(xs)
        out[name + "_stratum"] = np.concatenate(strata); out[name + "_band"] = np.concatenate(bands)
    out["exp_range_x"] = mh.exp_range_cases()
    out["atan2_range_y"], out["atan2_range_x"] = mh.atan2_range_cases()
    out["seed"] = np.int64(SEED)
    path = os.path.join(HERE, "math_hard.npz")
    write_npz(path, out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
