"""The streaming half of the engine (nps_push_*, nps_cohort_push_*) held to what its pinned staging rings and its open
batches are for:

  * the caller may reuse its buffer the moment a push returns: every push here comes from ONE buffer per kind, overwritten
    with other (valid, wrong) values right after the call, for many more rows than a ring has slots, with a ring that
    grows in mid-sequence;
  * a batch that fills is run and the statistics still come back in push order, no-data rows at the boundary included.

The oracle (refcpu.RefScorer) restates every sequence row by row; the bounds are those test_gpu_parity.py holds each path to.
"""
import numpy as np
import pytest

import exact_reference as er
from nimpress_amd import capi
from oracle import refcpu
from test_gpu_parity import (PARAM_GRID, REL_TOL, assert_ds_stats, assert_stats_equal, codes_to_bed, codes_to_pgen,
                             make_cohort, make_ds_cohort, oracle_scores, rel_err)

pytestmark = pytest.mark.gpu

KW = dict(imp_locus="ps", imp_missing="homref", imp_sample="int_ps", maxmis=0.2, mincs=10)
LOCUS_KINDS = (capi.ROW_UNCOVERED, capi.ROW_ABSENT, capi.ROW_FILTERED)


class Reused:
    """one buffer for every push of a kind: filled for the call, overwritten in place as soon as the call has returned"""

    def __init__(self, size, dtype, poison):
        self.buf = np.empty(size, dtype=dtype)
        self.poison = poison
        self.address = self.buf.ctypes.data

    def __call__(self, push, values, *args):
        self.buf[:] = values
        assert self.buf.ctypes.data == self.address
        push(self.buf, *args)
        self.buf[:] = self.poison


def polyploid_row(n, ploidy, rng):
    eaidx = int(rng.integers(0, 3))
    alle = rng.integers(-1, 3, size=(n, ploidy))
    alle[rng.uniform(size=n) < 0.04] = -1
    gts = (((alle + 1) << 1) | rng.integers(0, 2, size=(n, ploidy))).astype(np.int32)
    return gts.ravel(), eaidx


def check(sc, ref, betas, ds_rows, offset):
    """one flush, then finish, against the oracle: statistics in push order (the rows of `ds_rows` by assert_ds_stats'
    rule, every other row exactly), nloci, scores"""
    stats = sc.flush()
    scores, nloci = sc.finish(offset)
    ref_scores, ref_nloci = ref.finish(offset)
    assert nloci == ref_nloci
    assert len(stats) == len(ref.stats) == len(betas)
    is_ds = np.zeros(len(stats), bool)
    is_ds[ds_rows] = True
    assert_stats_equal(stats[~is_ds], [s for s, d in zip(ref.stats, is_ds) if not d])
    assert_ds_stats(stats[is_ds], [s for s, d in zip(ref.stats, is_ds) if d])
    assert rel_err(scores, ref_scores, betas, max(nloci, 1)) <= REL_TOL


def test_reused_caller_buffers_all_rings():
    """40 rows through the 8-slot ring of the diploid pushes (five times round: int32, int8 and int16 GT, packed, .bed
    under all four code maps), a FORMAT/DS row after every second of them and a polyploid row after every eighth
    (ploidy 3, 4, 3, 4, 3: the 2-slot rings go round many times and the polyploid one grows at the first ploidy 4),
    no-data rows between"""
    n = 777
    rng = np.random.default_rng(2024)
    gt = make_cohort(n, 40, 31, rng)
    dsc = make_ds_cohort(n, 20, 32, rng)
    nw, nb = (n + 15) // 16, (n + 3) // 4
    base = capi.live_resources()
    sc = capi.Scorer(n, capi.make_params(**KW))
    ref = refcpu.RefScorer(n, refcpu.make_params(**KW))
    gt_allele1 = 4                                      # (allele 1, unphased) in every call
    b_gt32, b_raw8, b_raw16 = (Reused(2 * n, t, gt_allele1) for t in (np.int32, np.int8, np.int16))
    b_packed, b_bed, b_ds = Reused(nw, np.uint32, 0xFFFFFFFF), Reused(nb, np.uint8, 0xFF), Reused(n, np.float32, 2.0)
    b_poly = {3: Reused(3 * n, np.int32, gt_allele1), 4: Reused(4 * n, np.int32, gt_allele1)}
    raw_kinds = ["gt32", "bed0", "raw8", "packed", "bed3", "raw16", "bed1", "bed2"]
    betas, ds_rows = [], []
    n_ds = n_poly = 0
    for j in range(40):
        kind = raw_kinds[(j + j // 8) % 8]              # (the kinds meet the slots in another order every round)
        codes, rie, beta, eaf = gt["codes"][j], bool(gt["rie"][j]), float(gt["beta"][j]), float(gt["eaf"][j])
        gts = refcpu.codes_to_gt(codes, n)
        if kind == "gt32":
            b_gt32(sc.push_gt, gts, 2, 1, rie, beta, eaf)
        elif kind == "raw8":
            b_raw8(sc.push_gt_raw, gts, 2, 1, rie, beta, eaf)
        elif kind == "raw16":
            b_raw16(sc.push_gt_raw, gts, 2, 1, rie, beta, eaf)
        elif kind == "packed":
            b_packed(sc.push_packed, codes[:nw], rie, beta, eaf)
        else:
            cmap = int(kind[3])
            row = codes_to_bed(codes, n, cmap) if cmap < 2 else codes_to_pgen(codes, n, cmap - 2)
            b_bed(sc.push_bed, row, cmap, rie, beta, eaf)
        ref.row_gt(gts, 2, 1, rie, beta, eaf)
        betas.append(beta)
        if j % 2 == 1:
            k = n_ds
            n_ds += 1
            b_ds(sc.push_ds, dsc["ds"][k], dsc["rie"][k], dsc["beta"][k], dsc["eaf"][k])
            ref.row_ds(dsc["ds"][k], bool(dsc["rie"][k]), dsc["beta"][k], dsc["eaf"][k])
            ds_rows.append(len(betas))
            betas.append(dsc["beta"][k])
        if j % 8 == 5:
            ploidy = (3, 4)[n_poly % 2]
            n_poly += 1
            gts, eaidx = polyploid_row(n, ploidy, rng)
            beta, eaf = float(rng.normal(0, 0.1)), float(rng.uniform(0.1, 0.5))
            b_poly[ploidy](sc.push_gt, gts, ploidy, eaidx, eaidx == 0, beta, eaf)
            ref.row_gt(gts, ploidy, eaidx, eaidx == 0, beta, eaf)
            betas.append(beta)
        if j % 7 == 3:
            sc.push_locus(LOCUS_KINDS[j % 3], rie, beta * 0.5, eaf)
            ref.row_locus(LOCUS_KINDS[j % 3], rie, beta * 0.5, eaf)
            betas.append(beta * 0.5)
    assert (n_ds, n_poly) == (20, 5)
    check(sc, ref, betas, ds_rows, -0.75)
    sc.close()
    assert capi.live_resources() == base


def test_gt_batch_rolls_over_in_push_order():
    """n = 33: the open batch holds 4096 rows.  4096 + 5 packed rows from one reused buffer, a no-data row behind the
    row that fills the batch and another behind the first row of the next one"""
    n, cap = 33, 4096
    rng = np.random.default_rng(33)
    co = make_cohort(n, 64, 34, rng)
    gts = [refcpu.codes_to_gt(co["codes"][j], n) for j in range(64)]
    beta_of = np.round(rng.normal(0, 0.02, cap + 5), 4)
    sc = capi.Scorer(n, capi.make_params(**KW))
    ref = refcpu.RefScorer(n, refcpu.make_params(**KW))
    b_packed = Reused((n + 15) // 16, np.uint32, 0xFFFFFFFF)
    betas = []
    for r in range(cap + 5):
        j, beta = r % 64, float(beta_of[r])
        b_packed(sc.push_packed, co["codes"][j], co["rie"][j], beta, co["eaf"][j])
        ref.row_gt(gts[j], 2, 1, bool(co["rie"][j]), beta, co["eaf"][j])
        betas.append(beta)
        if r in (cap - 1, cap):
            sc.push_locus(LOCUS_KINDS[r % 3], 0, 0.03, 0.2)
            ref.row_locus(LOCUS_KINDS[r % 3], False, 0.03, 0.2)
            betas.append(0.03)
    check(sc, ref, betas, [], 0.25)
    sc.close()


def test_ds_batch_rolls_over_in_push_order():
    """n = 33: the open FORMAT/DS batch holds 1024 rows.  1024 + 3 rows, push_ds and ploidy-3 push_gt in turn, each from
    one reused buffer, no-data rows on both sides of the boundary"""
    n, cap = 33, 1024
    rng = np.random.default_rng(35)
    dsc = make_ds_cohort(n, 64, 36, rng)
    poly = [polyploid_row(n, 3, rng) for _ in range(16)]
    beta_of = np.round(rng.normal(0, 0.02, cap + 3), 4)
    sc = capi.Scorer(n, capi.make_params(**KW))
    ref = refcpu.RefScorer(n, refcpu.make_params(**KW))
    b_ds, b_poly = Reused(n, np.float32, 2.0), Reused(3 * n, np.int32, 4)
    betas, ds_rows = [], []
    for r in range(cap + 3):
        beta = float(beta_of[r])
        if r % 2 == 0:
            j = (r // 2) % 64
            b_ds(sc.push_ds, dsc["ds"][j], dsc["rie"][j], beta, dsc["eaf"][j])
            ref.row_ds(dsc["ds"][j], bool(dsc["rie"][j]), beta, dsc["eaf"][j])
            ds_rows.append(len(betas))
        else:
            gts, eaidx = poly[(r // 2) % 16]
            b_poly(sc.push_gt, gts, 3, eaidx, eaidx == 0, beta, 0.3)
            ref.row_gt(gts, 3, eaidx, eaidx == 0, beta, 0.3)
        betas.append(beta)
        if r in (cap - 1, cap):
            sc.push_locus(LOCUS_KINDS[r % 3], 0, 0.03, 0.2)
            ref.row_locus(LOCUS_KINDS[r % 3], False, 0.03, 0.2)
            betas.append(0.03)
    check(sc, ref, betas, ds_rows, 0.25)
    sc.close()


def test_cohort_ring_reused_buffers_and_growth():
    """rows 0..11 of a NPS_FMT_GT2 cohort by nps_cohort_push_bed and nps_cohort_push_gt_raw in turn, from reused buffers;
    int8 GT at first, int32 from row 7 on (four times the bytes: the ring grows in mid-sequence)"""
    n, m = 777, 12
    rng = np.random.default_rng(12)
    co = make_cohort(n, m, 13, rng)
    kw = PARAM_GRID[0]
    base = capi.live_resources()
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2)
    b_bed = Reused((n + 3) // 4, np.uint8, 0xFF)
    b_raw8, b_raw32 = Reused(2 * n, np.int8, 4), Reused(2 * n, np.int32, 4)
    for j in range(m):
        if j % 2 == 0:
            a1 = (j // 2) % 2
            b_bed(lambda buf, row, a: dev.push_bed(row, buf, a), codes_to_bed(co["codes"][j], n, a1), j, a1)
        else:
            b = b_raw8 if j < 7 else b_raw32
            b(lambda buf, row: dev.push_gt_raw(row, buf, 2, 1), refcpu.codes_to_gt(co["codes"][j], n), j)
    assert np.array_equal(er.unpack(dev.download(0, m), n), er.unpack(co["codes"][:m], n))
    sc = capi.Scorer(n, capi.make_params(**kw))
    sc.score_cohort(dev, capi.row_descs(co["beta"], co["eaf"], None, co["rie"]), 0, capi.MODE_TWOPASS)
    stats = sc.flush()
    scores, nloci = sc.finish(0.25)
    sc.close()
    dev.close()
    ref_scores, ref_stats, ref_nloci = oracle_scores(co, kw, 0.25)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    assert rel_err(scores, ref_scores, co["beta"], max(nloci, 1)) <= REL_TOL
    assert capi.live_resources() == base
