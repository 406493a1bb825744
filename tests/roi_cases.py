"""Crafted keypoint lists and masks for the brute-force matcher's region-of-interest rule (tests/roi_ref.py states it): which flag
a POSITION gets, at the edges of the conversion, of the bounds and of the mask.  What a flag does to a match is
match_cases.flag_cases' business; here every probe position's flag is readable from the pairs of one call.

  query      the probes are list 1 and share one descriptor; list 2 is two on-mask elements at L1 distance 100 and 5000 from it:
             a kept query yields (i, 0), a dropped one nothing.  Modes 1 and 2.
  query+     the same observable for mutual=True (identical queries would tie in the reverse scan and only the first would pair):
             every probe query i has a partner element i on the mask, within +-6 per byte; everything else is random bytes.
             (i, i) appears iff query i is kept.
  list       mode 2, plain and mutual: the probes are list 2, probe element j within +-6 per byte of its own on-mask query
             LEAD + j; LEAD random on-mask queries before them and TAIL random on-mask elements after the probes.
             (LEAD + j, j) appears iff j is not excluded, and nothing else.
  forced     mode 1, one probe per call: four on-mask queries of one descriptor, list 2 = [on-mask at 200, the probe at 3000,
             on-mask at 6000].  A forced zero takes every query, (i, 1); a probe on the mask leaves (i, 0).  With mutual the
             queries tie in the reverse scan and the first alone pairs.

Probe values (axis_values) go to x with y on each row, to y with x on each column, and to both together; the masks are the
shapes of MASKS.  A sweep over "every integer up to n" is complete for n <= 16 and on the last row / column of the 64 x 257 masks;
their first row and column get the integers next to 1, 64 and n (float32 holds every integer below 2^24 exactly, so no other k
converts differently; the large masks are there for the index r * rw + c at its ends).

numpy only, deterministic, nothing here imports the package or the oracle."""
import hashlib
from collections import OrderedDict

import numpy as np

import match_cases as mc

DTYPE_KP, RATIO = mc.DTYPE_KP, mc.RATIO
LEAD, TAIL = 3, 2
LAST_BELOW_2_31 = np.float32(2147483520.0)
NAN_BITS = (0x7FC00000, 0x7F800001, 0xFFC00000, 0xFFABCDEF)          # +NaN and -NaN, a quiet and a signalling payload each


def _bits(values):
    return np.array(values, np.float32).view(np.uint32)


def axis_values(n, ks=None):
    """float32 probe values for an axis of n pixels (ks: the integers whose two sides are probed, default 1 .. n), without
    repeats, as bit patterns kept exactly (the NaN payloads included)"""
    one, zero = np.float32(1), np.float32(0)
    v = [-1.0, np.nextafter(-one, zero), -0.5, -0.0, 0.0, np.nextafter(one, zero), 1.0]
    for k in (range(1, n + 1) if ks is None else ks):
        v += [np.nextafter(np.float32(k), zero), float(k)]
    v += [float(n), n + 0.5, LAST_BELOW_2_31, 2147483648.0, -2147483648.0, -2147483648.0 - 256.0, 3e38, np.inf, -np.inf]
    bits = np.concatenate([_bits(v), np.array(NAN_BITS, np.uint32)])
    _, first = np.unique(bits, return_index=True)
    return bits[np.sort(first)].view(np.float32)


def thin_ks(n):
    return sorted(k for k in {1, 2, 3, 63, 64, 65, n - 2, n - 1, n} if 1 <= k <= n)


def probe_positions(shape):
    """[(label, (N, 2) float32 of (x, y))]: one group of probes for a small mask, two for a large one (the complete x sweep on the
    last row is a list of its own)"""
    rh, rw = shape
    small = max(rh, rw) <= 16
    rows = range(rh) if small else (0, rh - 1)
    cols = range(rw) if small else (0, rw - 1)

    def sweep_x(r, ks):
        v = axis_values(rw, ks)
        return np.stack([v, np.full(len(v), r + 0.5, np.float32)], axis=1)

    def sweep_y(c, ks):
        v = axis_values(rh, ks)
        return np.stack([np.full(len(v), c + 0.5, np.float32), v], axis=1)

    if small:
        parts = [sweep_x(r, None) for r in rows] + [sweep_y(c, None) for c in cols]
        v = axis_values(max(rh, rw))
        parts.append(np.stack([v, v], axis=1))
        return [("probes", np.concatenate(parts).astype(np.float32))]
    rest = [sweep_x(0, thin_ks(rw)), sweep_y(0, thin_ks(rh)), sweep_y(rw - 1, None)]
    v = axis_values(max(rh, rw), thin_ks(min(rh, rw)))
    rest.append(np.stack([v, v], axis=1))
    return [("x sweep on the last row", sweep_x(rh - 1, None)), ("other probes", np.concatenate(rest).astype(np.float32))]


# ---------------------------------------------------------------------------------------------- masks
BYTES15 = np.array([0, 7, -3, 0, 1, 0, 0, -128, 2, 0, 127, -1, 0, 5, 0], np.int8)
CORNERS = ((0, 0), (0, 256), (63, 0), (63, 256))


def _values16():
    """every int8 value once, the 0 away from the corners"""
    v = np.random.default_rng(16).permutation(np.arange(-128, 128)).astype(np.int8).reshape(16, 16)
    assert (v != 0)[[0, 0, -1, -1], [0, -1, 0, -1]].all()
    return v


def _big(background, planted):
    m = np.full((64, 257), background, np.int8)
    for (r, c), v in zip(CORNERS, planted):
        m[r, c] = v
    return m


MASKS = OrderedDict([
    ("1x1", np.array([[-128]], np.int8)),
    ("1x7", np.array([[3, 0, -1, 0, 5, 0, -128]], np.int8)),
    ("7x1", np.array([[0], [5], [0], [-2], [0], [1], [0]], np.int8)),
    ("3x5", BYTES15.reshape(3, 5).copy()),
    ("5x3", BYTES15.reshape(5, 3).copy()),
    ("64x257 ones", _big(1, (0, 0, 0, 0))),
    ("64x257 zeros", _big(0, (-1, 2, -128, 127))),
    ("16x16 values", _values16()),
])


def mask_probes(name):
    roi = MASKS[name]
    if name == "16x16 values":                                        # one probe in every pixel: only the 0 masks out
        r, c = np.divmod(np.arange(256), 16)
        return [("every pixel", np.stack([c + 0.5, r + 0.25], axis=1).astype(np.float32))]
    return probe_positions(roi.shape)


def anchor(roi):
    """(x, y) inside the first non-zero pixel in row-major order: where the keypoints that are not probes sit"""
    r, c = np.argwhere(roi != 0)[0]
    return np.float32(c + 0.5), np.float32(r + 0.5)


# ---------------------------------------------------------------------------------------------- cases
class Case(object):
    """One matcher call.  kind: "query", "query+", "list" or "forced"; `probe` names the list ("a" / "b") whose rows `rows` are the
    probes, in the order of their positions."""

    def __init__(self, name, mask, kind, a, b, mode, mutual, probe, rows):
        self.name, self.mask, self.kind, self.a, self.b, self.mode, self.mutual = name, mask, kind, a, b, mode, mutual
        self.probe, self.rows, self.roi, self.th = probe, np.asarray(rows, np.int64), MASKS[mask], RATIO

    def probes(self):
        return (self.a if self.probe == "a" else self.b)[self.rows]

    def with_rows(self, keep):
        """the "query" case with the probes `keep` (bool per probe) only: its list 2 does not depend on the probes"""
        assert self.kind == "query" and len(keep) == len(self.rows) == len(self.a)
        a = self.a[np.asarray(keep, bool)]
        return Case(self.name, self.mask, self.kind, a, self.b, self.mode, self.mutual, "a", np.arange(len(a)))

    def read(self, pairs):
        """bool per probe from the pairs of the call: the query was kept ("query", "query+"), the element took part ("list"),
        the element's distance was forced to 0 ("forced")"""
        pairs = np.asarray(pairs).reshape(-1, 2)
        if self.kind in ("query", "query+"):
            return np.isin(self.rows, pairs[:, 0])
        if self.kind == "list":
            return np.isin(self.rows, pairs[:, 1])
        assert len(pairs) and len(set(pairs[:, 1].tolist())) == 1 and pairs[0, 1] in (0, 1)
        return np.array([pairs[0, 1] == 1])

    def flag(self, dropped, list_flag):
        """what read() must give, from the flags of the probes' list"""
        if self.kind in ("query", "query+"):
            return ~dropped[self.rows]
        return (list_flag[self.rows] != 2) if self.kind == "list" else (list_flag[self.rows] == 1)


def _at(k, xy):
    k["x"], k["y"] = xy[0], xy[1]
    return k


def _near(descs, rng):
    return np.clip(descs.astype(np.int64) + rng.integers(-6, 7, descs.shape), 0, 255).astype(np.uint8)


def _place(k, rows, pos):
    k["x"][rows] = pos[:, 0]; k["y"][rows] = pos[:, 1]
    assert np.array_equal(k["x"][rows].view(np.uint32), pos[:, 0].view(np.uint32))      # the NaN payloads survive
    return k


def query_case(mask, label, pos, mode, rng):
    base = mc.make_base(rng)
    a = _place(mc.queries(base, len(pos)), np.arange(len(pos)), pos)
    b = _at(mc.records(mc.descs_at(base, [100, 5000], rng)), anchor(MASKS[mask]))
    return Case("%s, %s: query flags, mode %d" % (mask, label, mode), mask, "query", a, b, mode, False, "a", np.arange(len(pos)))


def query_partner_case(mask, label, pos, mode, rng):
    n = len(pos)
    a = _place(mc.records(rng.integers(0, 256, (n, 128), dtype=np.uint8)), np.arange(n), pos)
    b = _at(mc.records(_near(a["desc"], rng)), anchor(MASKS[mask]))
    return Case("%s, %s: query flags, mode %d, mutual" % (mask, label, mode), mask, "query+", a, b, mode, True, "a", np.arange(n))


def list_case(mask, label, pos, mutual, rng):
    n = len(pos)
    b = mc.records(rng.integers(0, 256, (n + TAIL, 128), dtype=np.uint8))
    _at(b, anchor(MASKS[mask]))
    _place(b, np.arange(n), pos)
    a = mc.records(rng.integers(0, 256, (LEAD + n, 128), dtype=np.uint8))
    a["desc"][LEAD:] = _near(b["desc"][:n], rng)
    _at(a, anchor(MASKS[mask]))
    return Case("%s, %s: list flags, mode 2%s" % (mask, label, ", mutual" if mutual else ""), mask, "list", a, b, 2, mutual, "b", np.arange(n))


def forced_positions(roi):
    """the handful of probe positions of the one-probe calls: x varies on the anchor's row, y on the anchor's column"""
    rh, rw = roi.shape
    ax, ay = anchor(roi)
    f, zero, nan = np.float32, np.float32(0), None                   # None: a NaN, its bit pattern patched in below
    xs = [-0.5, 0.0, np.nextafter(f(1), zero), min(1, rw - 1) + 0.5, rw - 0.5, np.nextafter(f(rw), zero), float(rw), LAST_BELOW_2_31,
          2147483648.0, np.inf, nan, nan]
    ys = [-0.5, min(1, rh - 1) + 0.5, np.nextafter(f(rh), zero), float(rh), -np.inf, nan]
    pos = [(x, ay) for x in xs] + [(ax, y) for y in ys] + [(rw - 0.5, rh - 0.5), (nan, nan)]
    out = np.array([[0.0 if v is None else v for v in xy] for xy in pos], np.float32)
    holes = [(k, t) for k, xy in enumerate(pos) for t in (0, 1) if xy[t] is None]
    for n, (k, t) in enumerate(holes):
        out.view(np.uint32)[k, t] = NAN_BITS[(3 * n) % 4]
    return out


def forced_case(mask, k, xy, mutual, rng):
    base = mc.make_base(rng)
    a = _at(mc.queries(base, 4), anchor(MASKS[mask]))
    b = _at(mc.records(mc.descs_at(base, [200, 3000, 6000], rng)), anchor(MASKS[mask]))
    _place(b, np.array([1]), xy[None, :])
    return Case("%s: forced zero, probe %d at (%r, %r)%s" % (mask, k, float(xy[0]), float(xy[1]), ", mutual" if mutual else ""), mask, "forced", a, b, 1,
                mutual, "b", [1])


def cases(mask):
    """every case of one mask, deterministic"""
    rng = np.random.default_rng(1000 + list(MASKS).index(mask))
    out = []
    for label, pos in mask_probes(mask):
        for mode in (1, 2):
            out.append(query_case(mask, label, pos, mode, rng))
            out.append(query_partner_case(mask, label, pos, mode, rng))
        for mutual in (False, True):
            out.append(list_case(mask, label, pos, mutual, rng))
    for k, xy in enumerate(forced_positions(MASKS[mask])):
        for mutual in (False, True):
            out.append(forced_case(mask, k, xy, mutual, rng))
    return out


def reference_cases(mask):
    """the mode-1 cases on which the reference's `matching_valid` is defined: not mutual, and only the probes with both
    coordinates in (-1, 2^31).  The cast of a NaN or of |v| >= 2^31 is undefined there too, and the reference tests no lower
    bound: for int(v) < 0 it reads the bytes before the mask (the oracle's `r >= 0 && c >= 0` is what keeps that read out)."""
    out = []
    for c in cases(mask):
        if c.mode != 1 or c.mutual:
            continue
        p = c.probes()
        with np.errstate(invalid="ignore"):
            ok = (p["x"] > -1) & (p["x"] < np.float32(2147483648.0)) & (p["y"] > -1) & (p["y"] < np.float32(2147483648.0))
        if c.kind == "query":
            out.append(c.with_rows(ok))
        elif ok.all():
            out.append(c)
    return out


def digest(cases):
    """SHA-256 over the inputs of the cases: match_cases.digest (both lists, the threshold) and every case's mask, shape and mode"""
    h = hashlib.sha256(mc.digest(cases).encode())
    for c in cases:
        h.update(c.roi.tobytes()); h.update(repr((c.roi.shape, c.mode, c.mutual)).encode())
    return h.hexdigest()
