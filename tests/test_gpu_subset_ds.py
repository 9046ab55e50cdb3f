"""Scoring a chosen subset of a resident cohort's samples on NPS_FMT_DS32 cohorts (ds_tally_masked_kernel,
nps_ds.hip), against the references run on the kept columns alone: statistics against the oracle's row loop
(refcpu.RefScorer.row_ds with n = n_kept: counts, used and reason exact, the float64 neffect as tests/test_gpu_parity.py
compares it), scores against the double-double sums of tests/exact_reference.py within f64_bound, the bar
tests/test_gpu_exact.py holds the dosage paths to.  Inputs and the assertion that the subset run decided differently from
a whole-cohort run: tests/test_gpu_subset.py."""
import numpy as np
import pytest

import exact_reference as er
from nimpress_amd import capi
from oracle import refcpu
from test_gpu_parity import PARAM_GRID, assert_ds_stats
from test_gpu_subset import assert_decided_differently, design_rows, keep_pattern, make_score, run_subset, run_whole

pytestmark = pytest.mark.gpu


def make_ds(n, m, keep, kw, rng):
    """float32 dosages [m, n] in [0, 2] with three decimals, two in a hundred missing (NaN), the designed rows on top"""
    k = rng.integers(0, 2001, size=(m, n)).astype(np.float32)
    ds = (k / np.float32(1000.0)).astype(np.float32)
    ds[rng.random((m, n), dtype=np.float32) < 0.02] = np.nan

    def fill(row, idx):
        x = ds[row]
        x[np.isnan(x)] = 0.5
        x[idx] = np.nan
    design_rows(n, m, keep, kw, rng, fill)
    return ds


def references(ds, keep, kw, beta, eaf, rie):
    sub = np.ascontiguousarray(ds[:, keep != 0])
    sc = refcpu.RefScorer(sub.shape[1], refcpu.make_params(**kw))
    for j in range(sub.shape[0]):
        sc.row_ds(sub[j], bool(rie[j]), beta[j], eaf[j])
    _, nloci = sc.finish(0.0)
    dos = np.where(rie[:, None] == 1, 2.0 - sub.astype(np.float64), sub.astype(np.float64))
    return sc.stats, nloci, er.dd_reference(dos, beta, eaf, rie, kw)


CASES = [((1, 1), "all"), ((5, 3), "alternate"), ((5, 3), "first"), ((5, 3), "last"),
         ((1027, 130), "alternate"), ((1027, 130), "half"), ((1027, 130), "first"), ((1027, 130), "last"),
         ((1027, 130), "unit_dropped"), ((1027, 130), "ragged_last"),
         ((70000, 40), "half"), ((70000, 40), "strip_dropped"), ((70000, 40), "ragged_last")]


@pytest.mark.parametrize("k", range(len(CASES)), ids=["%dx%d-%s" % (s[0], s[1], p) for s, p in CASES])
def test_ds32_subset_vs_references_on_the_kept_columns(k):
    (n, m), pattern = CASES[k]
    pk = k % len(PARAM_GRID)
    kw = PARAM_GRID[pk]
    rng = np.random.default_rng(n * 13 + m + k)
    keep = keep_pattern(n, pattern, rng)
    ds = make_ds(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    dev.upload(0, ds)
    sset = capi.SampleSet(keep)
    got, nloci, stats = run_subset(dev, n, kw, descs, sset, 0.0)
    if n > 1:
        _, _, whole = run_whole(dev, n, kw, descs, 0.0)
    sset.close()
    dev.close()
    ref_stats, ref_nloci, (hi, lo, ab, nl, _, _, _) = references(ds, keep, kw, beta, eaf, rie)
    assert got.shape == (int(keep.sum()),)
    assert nloci == ref_nloci == nl
    assert_ds_stats(stats, ref_stats)
    ok = np.isfinite(got)
    assert np.array_equal(ok, np.isfinite(hi + lo)), "NaN positions differ"
    assert np.all(er.sum_error(got, nl, hi, lo)[ok] <= er.f64_bound(ab, nl, got, nl)[ok])
    if n > 1:
        assert_decided_differently(n, kw, stats, whole)


@pytest.mark.parametrize("shape", [(1, 1), (1027, 130), (70000, 40)])
def test_ds32_every_sample_kept_is_the_two_pass_run(shape):
    """the masked tally adds the same terms in the same tree: statistics (the float64 neffect included) and scores equal bit
    for bit to NPS_MODE_TWOPASS on the same context parameters; finish_subset == finish"""
    n, m = shape
    rng = np.random.default_rng(n + m)
    kw = PARAM_GRID[(n + m) % len(PARAM_GRID)]
    keep = np.ones(n, np.uint8)
    ds = make_ds(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    dev.upload(0, ds)
    sset = capi.SampleSet(keep)
    sc = capi.Scorer(n, capi.make_params(**kw))
    sd = capi.ScoreDef(descs)
    sc.score_cohort_def_subset(dev, sd, sset)
    stats = sc.flush()
    scores, nloci = sc.finish_subset(sset, 0.5)
    plain, nloci_plain = sc.finish(0.5)
    sc.close()
    sd.close()
    sset.close()
    two, nloci_two, stats_two = run_whole(dev, n, kw, descs, 0.5)
    dev.close()
    assert nloci == nloci_plain == nloci_two
    assert stats.tobytes() == stats_two.tobytes()
    assert scores.tobytes() == plain.tobytes() == two.tobytes()


def test_ds32_subset_runs_accumulate_and_resources_return():
    """rows 0 .. 63 and then 64 .. 129 with one set equal one run over all 130 rows' references; nothing is held afterwards"""
    n, m = 1027, 130
    rng = np.random.default_rng(130)
    kw = PARAM_GRID[0]
    keep = keep_pattern(n, "half", rng)
    ds = make_ds(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    dev.upload(0, ds)
    start = capi.live_resources()
    sset = capi.SampleSet(keep)
    sc = capi.Scorer(n, capi.make_params(**kw))
    d1, d2 = capi.ScoreDef(descs[:64]), capi.ScoreDef(descs[64:])
    sc.score_cohort_def_subset(dev, d1, sset, 0)
    sc.score_cohort_def_subset(dev, d2, sset, 64)
    stats = sc.flush()
    got, nloci = sc.finish_subset(sset, 0.0)
    for o in (sc, d1, d2, sset):
        o.close()
    assert capi.live_resources() == start
    dev.close()
    ref_stats, ref_nloci, (hi, lo, ab, nl, _, _, _) = references(ds, keep, kw, beta, eaf, rie)
    assert nloci == ref_nloci == nl
    assert_ds_stats(stats, ref_stats)
    ok = np.isfinite(got)
    assert np.array_equal(ok, np.isfinite(hi + lo))
    assert np.all(er.sum_error(got, nl, hi, lo)[ok] <= er.f64_bound(ab, nl, got, nl)[ok])
