"""A "wide" embedding of a genotype matrix for the subset paths (nps_score_cohort_def_subset), shared by
tests/test_decision_cases.py (the layout's properties, and the faults a subset run can commit, on the CPU) and
tests/test_gpu_special_values.py (the paths subset_gt2x and subset_ds32, which the decision, IEEE and exact matrices then
run).  Not a conftest.

widen(codes) spreads the n columns of `codes` over n_total > n samples and returns the mask that keeps exactly them, in
order: the subset run over the wide cohort must give what the oracle gives on `codes` as they stand -- N = n_kept = n in
every decision, while the layout (units of 32 samples, strips of 2 048) is that of n_total.  One deterministic layout of
the sample axis:

  1. h = n // 2 kept samples at the even positions 0, 2, .., 2 h - 2, the odd positions dropped: units with mixed masks;
  2. DROPPED_BLOCK = 96 dropped samples (at least two wholly dropped units), and LONG_DROPPED = 2 048 more when n >= 2 048:
     a wholly dropped stretch longer than a strip;
  3. the remaining n - h kept samples, contiguous: wholly kept units;
  4. TAIL = 13 dropped samples; n_total is no multiple of 32, so the last unit is ragged and its tail dropped.

The dropped columns are adversarial: code 2 (missing) in the even rows, code 3 (dosage 2) in the odd rows, so a tally that
leaks one dropped sample moves nmissing or neffect, and one that leaks them all moves them by n_total - n.
"""
import functools

import numpy as np

import decision_cases as dc

UNIT, STRIP = 32, 2048
DROPPED_BLOCK, LONG_DROPPED, TAIL = 96, 2048, 13


def keep_mask(n):
    """uint8[n_total]: 1 at the positions of the n kept samples, in order"""
    h = n // 2
    gap = DROPPED_BLOCK + (LONG_DROPPED if n >= 2048 else 0)
    keep = np.zeros(2 * h + gap + (n - h) + TAIL, np.uint8)
    keep[0:2 * h:2] = 1
    keep[2 * h + gap:2 * h + gap + (n - h)] = 1
    assert int(keep.sum()) == n and keep.size % UNIT != 0, (n, keep.size)
    return keep


@functools.lru_cache(maxsize=None)
def n_total(n):
    return keep_mask(n).size


def widen(codes):
    """[m, n] 2-bit codes -> (wide codes [m, n_total], keep uint8[n_total]); wide[:, keep != 0] == codes"""
    codes = np.asarray(codes, np.uint8)
    m, n = codes.shape
    keep = keep_mask(n)
    wide = np.empty((m, keep.size), np.uint8)
    wide[0::2] = 2
    wide[1::2] = 3
    wide[:, keep != 0] = codes
    return wide, keep


def ds_rows(wide_codes, rie):
    """the FORMAT/DS rows of the wide matrix (decision_cases.ds_rows)"""
    return dc.ds_rows(wide_codes, rie)


def unit_masks(keep):
    """per unit of 32 samples: (kept samples, samples) -- the last unit may be ragged"""
    n_units = (keep.size + UNIT - 1) // UNIT
    pad = np.zeros(n_units * UNIT, np.int64)
    pad[:keep.size] = keep
    size = np.full(n_units, UNIT)
    size[-1] = keep.size - UNIT * (n_units - 1)
    return pad.reshape(n_units, UNIT).sum(axis=1), size


def longest_dropped_run(keep):
    edges = np.flatnonzero(np.concatenate([[1], np.asarray(keep) != 0, [1]]))   # kept positions, fenced at both ends
    return int(np.max(np.diff(edges)) - 1)
