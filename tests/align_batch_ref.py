"""The decision rule of LinearAlign.align_batch (sift_pyocl_amd/alignment.py, steps 4 to 7 of its pipeline) restated in plain
numpy, one segment at a time, for tests/test_align_batch_ref_host.py and tests/test_gpu_align_batch.py.  It takes what the batch
calls of MatchPlan return (or the single calls, segment by segment, put into the same tables) and gives the mode, the matrix and
the offset of every frame:

    mode 2 (affine)  the segment's model is finite and was fitted to n >= 18 pairs, and shift_only is off:
                     model = (a, b, c, d, e, f) with x' = a x + b y + c, y' = d x + e y + f
                     matrix = [[e, d], [b, a]], offset = [f, c]          (the kernel's (y, x) order), rounded to float32
    mode 1 (shift)   any other segment whose median displacement (dx, dy) counted at least one pair:
                     matrix = identity, offset = [dy, dx]
    mode 0 (none)    no pair, or no usable one: matrix and offset all NaN (the warp then writes the frame's fill value)

and, under `robust`, the mask the estimates take: the consensus mask, with the rows of a segment that has pairs but no winning
map set to 1 (all its pairs are used).

numpy only; nothing here imports the package.
"""
import numpy as np

F = np.float32
MIN_MATCHES_AFFINE = 18


def used_mask(mask, models, pair_counts):
    """step 4: the consensus mask (M,) with every row of a no-winner segment (a NaN row of `models`) set"""
    mask = np.array(mask, dtype=np.uint8).reshape(-1)
    at = 0
    for s, n in enumerate(int(v) for v in pair_counts):
        if n > 0 and np.isnan(np.asarray(models)[s]).any():
            mask[at:at + n] = 1
        at += n
    assert at == len(mask)
    return mask


def align_batch_ref(pair_counts, models=None, n_fit=None, shifts=None, n_shift=None, shift_only=False):
    """(mode (S,) int8, matrix (S, 2, 2) float32, offset (S, 2) float32) from per-segment tables:
    models (S, 6) float64 with NaN rows and n_fit (S,) as fit_batch returns them (ignored under shift_only, may be None);
    shifts (S, 2) float32 (dx, dy) with NaN rows and n_shift (S,) as shift_batch returns them (None: no segment needs one)"""
    S = len(pair_counts)
    mode = np.zeros(S, np.int8)
    matrix = np.full((S, 2, 2), np.nan, F)
    offset = np.full((S, 2), np.nan, F)
    for s in range(S):
        if int(pair_counts[s]) == 0:
            continue
        if not shift_only and models is not None:
            m = np.asarray(models[s], np.float64)
            if np.isfinite(m).all() and int(n_fit[s]) >= MIN_MATCHES_AFFINE:
                a, b, c, d, e, f = (float(v) for v in m)
                mode[s] = 2
                matrix[s] = [[F(e), F(d)], [F(b), F(a)]]
                offset[s] = [F(f), F(c)]
                continue
        assert shifts is not None, "segment %d needs a shift and none was computed" % s
        if int(n_shift[s]) > 0:
            dx, dy = F(shifts[s][0]), F(shifts[s][1])
            mode[s] = 1
            matrix[s] = [[1, 0], [0, 1]]
            offset[s] = [dy, dx]
    return mode, matrix, offset
