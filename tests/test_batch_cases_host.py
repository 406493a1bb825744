"""CPU checks of the cases of tests/batch_cases.py (the hand-back tests of tests/test_gpu_batch_cases.py), on the oracle alone.
They are conditions on the INPUTS: a GPU test can only tell a swapped frame, a wrong path or a lost copy if the frames differ,
if every capacity class occurs, if delivered and parked frames interleave, and if the arena cases regrow the arena where they
claim to.  A frame list that does not meet them has to change; the conditions stay."""
import itertools

import numpy as np
import pytest

import batch_cases as bc


def _assert_distinct(specs, shape, pix_per_kp=None):
    """frames with records have pairwise different record sets; every frame has its own (min, max)"""
    assert len(set(specs)) == len(specs)
    res = [bc.oracle_of(s, shape, pix_per_kp) for s in specs]
    for (sa, a), (sb, b) in itertools.combinations(zip(specs, res), 2):
        assert (np.float32(a[1][0]).tobytes(), np.float32(a[1][1]).tobytes()) != \
               (np.float32(b[1][0]).tobytes(), np.float32(b[1][1]).tobytes()), "%r and %r have the same (min, max)" % (sa, sb)
        if len(a[0]) or len(b[0]):
            assert len(a[0]) != len(b[0]) or not np.array_equal(bc.record_bytes(a[0]), bc.record_bytes(b[0])), \
                "%r and %r have the same records" % (sa, sb)
            # ... and share no record at all: a fetched range that strays into a neighbour shows
            both = set(r.tobytes() for r in bc.record_bytes(a[0])) & set(r.tobytes() for r in bc.record_bytes(b[0]))
            assert not both, "%r and %r share %d records" % (sa, sb, len(both))


@pytest.mark.parametrize("lanes", bc.SMALL_LANES)
def test_small_frames_are_told_apart(lanes):
    case = bc.small_case(lanes)
    _assert_distinct(case.specs(), bc.SMALL)
    kinds = {"blank": 0, "sparse": 0, "rich": 0}
    for s in case.specs():
        n = len(bc.oracle_of(s, bc.SMALL)[0])
        assert (n == 0) == (s[0] == "const"), "%r: %d records" % (s, n)
        kinds["blank" if n == 0 else "sparse" if n < 20 else "rich"] += 1
        assert n < 20 or n > 60
    assert min(kinds.values()) >= 1, kinds
    for n, specs, counts, _ in case.batches:
        assert len(specs) == n == len(set(specs))
        if n >= 3:                                     # each list mixes blank, sparse and rich frames
            assert min(counts) == 0 and any(0 < c < 20 for c in counts) and max(counts) > 60, (lanes, n, counts)


def test_small_batch_sizes():
    assert [bc.batch_sizes(L) for L in bc.SMALL_LANES] == [[1, 2, 3], [1, 2, 3, 4, 5], [1, 2, 3, 4, 6, 7], [1, 4, 5, 6, 10, 11]]
    firsts = {bc.small_batch(L, n)[0] for L, n in bc.small_ids()}
    assert len(firsts) >= 8                            # the batches do not all start with the same frame
    for L, n in bc.small_ids():
        short = bc.shorter_batch(L, n)
        assert 1 <= len(short) == len(set(short)) <= max(1, n - 1) and (len(short) < L or L == 1)
        assert short != bc.small_batch(L, n)[:len(short)]


@pytest.mark.parametrize("lanes", bc.SMALL_LANES)
def test_every_capacity_class_and_both_interleavings(lanes):
    """per case (one lane count, all its batches -- a batch of one or two frames cannot hold six classes or a frame between two
    others); and per batch of five frames or more on its own"""
    case = bc.small_case(lanes)
    seen, d_between, p_between = set(), 0, 0
    for n, specs, counts, matrix in case.batches:
        assert len(matrix) == 6 and all(len(row) == n for row in matrix)
        own = set()
        for row in matrix:
            flags = bc.delivered(counts, row)
            for c, (cls, cap, null), d in zip(counts, row, flags):
                assert cls in bc.CAP_CLASSES
                # the class says what it is, and the path follows from batch_retire's rule alone
                assert {bc.CAP_BELOW: c > 0 and cap == c - 1 and not null, bc.CAP_EXACT: cap == c and not null,
                        bc.CAP_ABOVE: cap == c + 1 and not null, bc.CAP_ZERO_EMPTY: cap == 0 and c == 0 and not null,
                        bc.CAP_ZERO_FULL: cap == 0 and c > 0 and not null, bc.CAP_NULL: null and cap > 100000}[cls]
                assert d == (cls in (bc.CAP_EXACT, bc.CAP_ABOVE, bc.CAP_ZERO_EMPTY))
                own.add(cls)
            d_between += bc.has_between(flags, True)
            p_between += bc.has_between(flags, False)
            offs, total = bc.expected_offsets(counts, row)
            assert total == sum(c for c, d in zip(counts, flags) if not d)
            assert [o for o in offs if o >= 0] == sorted(o for o in offs if o >= 0)
        for i in range(n):                             # every frame meets every class it can have
            got = {row[i][0] for row in matrix}
            assert got == ({bc.CAP_EXACT, bc.CAP_ABOVE, bc.CAP_ZERO_EMPTY, bc.CAP_NULL} if counts[i] == 0 else
                           set(bc.CAP_CLASSES) - {bc.CAP_ZERO_EMPTY})
        if n >= 5:
            assert own == set(bc.CAP_CLASSES), (lanes, n, own)
            assert any(bc.has_between(bc.delivered(counts, r), True) for r in matrix)
            assert any(bc.has_between(bc.delivered(counts, r), False) for r in matrix)
        seen |= own
    assert seen == set(bc.CAP_CLASSES)
    assert d_between >= 1 and p_between >= 1


@pytest.mark.parametrize("lanes", bc.ARENA_LANES)
def test_arena_case_regrows_once_with_records_parked(lanes):
    warm, main = bc.arena_warmup(lanes), bc.ARENA_MAIN
    assert len(warm) == lanes and not set(warm) & set(main)
    _assert_distinct(warm + main, bc.BIG)
    cw, cm = bc.counts_of(warm, bc.BIG), bc.counts_of(main, bc.BIG)
    assert all(0 < c < 100 for c in cm[:3]) and all(c > 6000 for c in cm[3:] + cw)
    ev_w, cap = bc.arena_replay(cw)
    assert ev_w == [(0, 0, bc.ARENA_START)] and cap == bc.ARENA_START       # the first allocation, no regrowth
    ev_m, cap2 = bc.arena_replay(cm, cap)
    print("lanes %d: warm-up %r, main %r, regrowth %r" % (lanes, cw, cm, ev_m))
    assert len(ev_m) == 1
    at, parked, size = ev_m[0]
    assert at == 7 and parked == sum(cm[:7]) > 20000 and size == cap2 == 2 * bc.ARENA_START
    assert bc.arena_replay(cm, cap2) == ([], cap2)                          # a second run of the main batch grows nothing
    assert sum(cm) * bc.RECORD_BYTES <= cap2


def test_arena_replay_is_the_rule():
    # one frame of a batch of 8 that alone asks for more than 4 MiB x 1.25 / 8: the projection doubles the first size
    assert bc.arena_replay([29127]) == ([(0, 0, 1 << 23)], 1 << 23)
    assert bc.arena_replay([5, 5, 5] + [9000] * 5)[0] == [(0, 0, 1 << 22), (6, 27015, 1 << 23)]
    assert bc.arena_replay([0, 0]) == ([], 0)


def test_fetch_ranges():
    counts, offsets = [5, 0, 7, 3, 0, 4], [0, 5, -1, 5, 8, 8]
    acc, ref = bc.fetch_ranges(offsets, counts)
    T = 12
    assert {(0, 0), (T, 0), (0, T), (0, 5), (5, 0), (5, 3), (8, 0), (8, 4), (4, 2), (7, 2), (T - 1, 1)} == set(acc)
    assert all(bc.range_accepted(f, c, T) for f, c in acc) and not any(bc.range_accepted(f, c, T) for f, c in ref)
    assert set(ref) == {(T, 1), (0, T + 1), (-1, 1), (0, -1), (2 ** 62, 2 ** 62), (2 ** 63 - 1, 1), (1, 2 ** 63 - 1)}
    assert all(-2 ** 63 <= v < 2 ** 63 for r in ref for v in r)
    # the check the library used to make lets three of the refused ranges through, those whose sum is 2^63: 2^63 * 144 is 0
    # modulo 2^64
    old = [r for r in ref if bc.old_range_check_accepts(r[0], r[1], T * bc.RECORD_BYTES)]
    assert old == [(2 ** 62, 2 ** 62), (2 ** 63 - 1, 1), (1, 2 ** 63 - 1)]
    assert all(bc.old_range_check_accepts(f, c, T * bc.RECORD_BYTES) for f, c in acc)


def test_overflow_case_flags_the_lattice_frame_only():
    ppk = bc.OVERFLOW_PIX_PER_KP
    specs = [bc.OVERFLOW_FLAGGED] + bc.OVERFLOW_PLAIN
    _assert_distinct(specs, bc.MID, ppk)
    kpsize = bc.MID[0] * bc.MID[1] // ppk
    assert bc.oracle_of(bc.OVERFLOW_FLAGGED, bc.MID, ppk)[2] and len(bc.oracle_of(bc.OVERFLOW_FLAGGED, bc.MID)[0]) > kpsize
    assert not bc.oracle_of(bc.OVERFLOW_FLAGGED, bc.MID)[2]                  # not at the default capacity
    for s in bc.OVERFLOW_PLAIN:
        k, _, ovf = bc.oracle_of(s, bc.MID, ppk)
        assert not ovf and 100 < len(k) < kpsize
        assert np.array_equal(bc.record_bytes(k), bc.record_bytes(bc.oracle_of(s, bc.MID)[0]))
    names = [n for n, _ in bc.overflow_batches()]
    assert names == ["first", "middle", "last"]
    for name, b in bc.overflow_batches():
        assert len(b) == 5 and b.index(bc.OVERFLOW_FLAGGED) == {"first": 0, "middle": 2, "last": 4}[name]


def test_python_sequence_straddles_the_first_guess():
    _assert_distinct(bc.PY_MIXED, bc.BIG)
    _assert_distinct(bc.PY_BLANK, bc.BIG)
    counts = bc.counts_of(bc.PY_MIXED, bc.BIG)
    assert bc.PY_FIRST_GUESS == 6400
    assert [c > bc.PY_FIRST_GUESS for c in counts] == [False, True, False, True] and min(counts) > 257
    assert bc.counts_of(bc.PY_BLANK, bc.BIG) == [0, 0, 0, 0]
