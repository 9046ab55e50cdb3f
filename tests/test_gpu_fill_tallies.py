"""Strip cohorts (NPS_FMT_GT2X) that are FILLED WITH REAL ROWS carry their whole-row tallies from the moment the rows are
written: the fill kernels (nps_mx.hip: fill_gt2x_kernel -- plain rows, PLINK .bed / .pgen rows, a NPS_FMT_GT2 cohort)
count tallyAlleles (nimpress.nim:32-47) while they write the units.  Validity is kept per superblock of 128 rows;
NPS_MODE_AUTO scores a run whose superblocks are all valid with the tallies given where a strip has one row team (more than
262 144 samples) or where the tallies were asked for; synthetic cohorts are scored exactly as before.

Bars as in tests/test_gpu_mx.py: tallies / decisions / nloci bit-exact against the CPU oracle, scores within 1e-6 relative
with the counted 2^-50 escape (check_scores below is that file's, with a count of its own), and rtol 1e-12 / atol 1e-18
with NaNs at the same samples between two kernels on one cohort."""
import threading

import numpy as np
import pytest

import score_compare
from nimpress_amd import capi
from oracle import refcpu
from test_gpu_parity import PARAM_GRID, assert_stats_equal, codes_to_bed, codes_to_pgen, make_cohort, oracle_scores, rel_err

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6


def check_scores(scores, ref_scores, beta, nloci):
    """the bar of tests/test_gpu_mx.py::check_scores: 1e-6 relative (floored at 1e-12 of the beta scale), or an absolute
    difference below 2^-50 of the mean absolute weight for at most 1 in 1000 samples (at most 2 below 2000 samples)"""
    got, ref = np.asarray(scores), np.asarray(ref_scores)
    ok = score_compare.assert_special_equal(got, ref)
    if not ok.any():
        return 0
    sb = score_compare.beta_scale(beta, nloci)
    d = np.abs(got[ok] - ref[ok])
    plain = REL_TOL * np.maximum(np.abs(ref[ok]), 1e-12 * sb)
    tol = np.maximum(plain, 2.0 ** -50 * sb)
    escaped = int(np.count_nonzero((d > plain) & (d <= tol)))
    print("check_scores: max |d| %.3g, max relative %.3g, %d of %d samples through the 2^-50 escape" % (
        d.max(), rel_err(got, ref, beta, max(nloci, 1)), escaped, ok.sum()))
    assert escaped <= max(2, int(ok.sum()) // 1000), "%d of %d samples pass only through the 2^-50 escape" % (escaped, ok.sum())
    assert not np.any(d > tol), "%d samples differ (max |d| %.3g)" % (np.count_nonzero(d > tol), d.max())
    return escaped


def run_pass(dev, n, kw, descs, offset=0.0, row0=0, mode=capi.MODE_AUTO):
    sc = capi.Scorer(n, capi.make_params(**kw))
    sc.profile_enable(True)
    sc.score_cohort(dev, descs, row0, mode)
    p = sc.profile_get(reset=True)
    stats = sc.flush()
    scores, nloci = sc.finish(offset)
    sc.close()
    return p, stats, scores, nloci


def given(p):
    """the pass was ONE read with the tallies given: no tally pass, no in-pass kernel, the given-tallies kernel"""
    return p.n_tally == 0 and p.n_fused == 0 and p.n_accumulate >= 1


def in_pass(p):
    return p.n_fused >= 1 and p.n_accumulate == 0


def assert_tallies_are_the_oracles(dev, co, row0=0, nrows=None):
    """nps_cohort_row_tallies against tallyAlleles of the oracle (refcpu.score_packed's row statistics: nmissing, neffect
    before any ref_is_effect flip does not exist there -- rie = 0 for the count)"""
    nrows = co["m"] - row0 if nrows is None else nrows
    zeros = np.zeros(co["m"], np.int32)
    _, ref_stats, _ = refcpu.score_packed(co["codes"], co["n"], zeros, zeros, np.zeros(co["m"]), np.full(co["m"], 0.1),
                                          refcpu.make_params(**PARAM_GRID[0]), 0.0)
    nm, ne = dev.row_tallies(row0, nrows)
    want_nm = np.array([s[1] for s in ref_stats], dtype=np.uint64)[row0:row0 + nrows]
    want_ne = np.array([s[2] for s in ref_stats])[row0:row0 + nrows]
    assert np.array_equal(nm, want_nm)
    assert np.array_equal(ne.astype(np.float64), want_ne)


SHAPES = [(1, 1), (33, 129), (2049, 257), (70_000, 300), (300_001, 300)]


@pytest.mark.parametrize("shape", SHAPES)
def test_uploaded_rows_carry_their_tallies_before_any_scoring(shape):
    """upload of plain rows, conversion from a row-layout cohort, upload of .bed / .pgen rows under every code map: the
    cohort has its tallies at once, bit for bit the oracle's, and no scoring call was made"""
    n, m = shape
    rng = np.random.default_rng(n * 11 + m)
    co = make_cohort(n, m, 2024 + n, rng)
    words = (n + 15) // 16
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    assert not dev.has_tallies() and not dev.rows_tallied(0, m)
    dev.upload(0, co["codes"])
    assert dev.has_tallies() and dev.rows_tallied(0, m)
    assert_tallies_are_the_oracles(dev, co)
    assert np.array_equal(dev.download(0, m), co["codes"][:, :words])
    dev.close()

    src = capi.Cohort(n, m)
    src.upload(0, co["codes"])
    conv = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    conv.convert_from(src)
    assert conv.has_tallies()
    assert_tallies_are_the_oracles(conv, co)
    assert np.array_equal(conv.download(0, m), co["codes"][:, :words])
    conv.close()

    # every code map (NPS_MAP_BED_A2 = 0, _BED_A1 = 1, _PGEN_ALT = 2, _PGEN_REF = 3), mixed over the rows
    maps = rng.integers(0, 4, m).astype(np.uint8)
    maps[:min(m, 4)] = np.arange(4, dtype=np.uint8)[:min(m, 4)]
    rows = np.stack([codes_to_bed(co["codes"][j], n, int(maps[j])) if maps[j] < 2 else
                     codes_to_pgen(co["codes"][j], n, int(maps[j]) - 2) for j in range(m)])
    src.upload_bed(0, rows, maps)
    bed = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    bed.upload_bed(0, rows, maps)
    assert bed.has_tallies()
    assert_tallies_are_the_oracles(bed, co)
    assert np.array_equal(bed.download(0, m), src.download(0, m))
    assert np.array_equal(bed.download(0, m), co["codes"][:, :words])
    bed.close()
    src.close()


@pytest.mark.parametrize("shape,seed", [((300_001, 300), 4242), ((530_000, 130), 4242), ((1_050_000, 300), 4242)])
def test_first_pass_over_an_uploaded_cohort_is_one_read_with_the_tallies_given(shape, seed):
    n, m = shape
    rng = np.random.default_rng(n + m)
    co = make_cohort(n, m, seed, rng)
    kw = PARAM_GRID[(n + m) % len(PARAM_GRID)]
    descs = capi.row_descs(co["beta"], co["eaf"], None, co["rie"])
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, co["codes"])
    p, stats, scores, nloci = run_pass(dev, n, kw, descs)
    print("first pass: n_tally %d n_fused %d n_accumulate %d" % (p.n_tally, p.n_fused, p.n_accumulate))
    assert given(p)
    ref_scores, ref_stats, ref_nloci = oracle_scores(co, kw, 0.0)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, co["beta"], nloci)
    # another kernel on the same cohort: the in-pass kernel where its grid exists, else tally pass + accumulation
    mode = capi.MODE_FUSED if n == 300_001 else capi.MODE_TWOPASS
    p2, stats2, other, nloci2 = run_pass(dev, n, kw, descs, mode=mode)
    assert (in_pass(p2) if mode == capi.MODE_FUSED else (p2.n_tally >= 1 and p2.n_accumulate >= 1))
    assert nloci2 == nloci
    assert_stats_equal(stats2, [tuple(s) for s in ref_stats])
    ok = ~np.isnan(scores)
    assert np.array_equal(np.isnan(other), ~ok)
    assert np.allclose(other[ok], scores[ok], rtol=1e-12, atol=1e-18)
    dev.close()


def test_small_cohorts_are_served_but_not_rerouted():
    n, m = 70_000, 1500
    co = make_cohort(n, m, 4321, np.random.default_rng(5))
    descs = capi.row_descs(co["beta"], co["eaf"], None, co["rie"])
    kw = PARAM_GRID[0]
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, co["codes"])
    assert dev.has_tallies()
    p, stats, first, nloci = run_pass(dev, n, kw, descs)
    assert in_pass(p)                                   # several row teams per strip: the pass that counts is as fast
    dev.keep_tallies()                                  # asked for: no read, and the next pass runs with them given
    assert dev.has_tallies()
    p, stats2, again, nloci2 = run_pass(dev, n, kw, descs)
    assert given(p)
    ref_scores, ref_stats, ref_nloci = oracle_scores(co, kw, 0.0)
    assert nloci == nloci2 == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    assert_stats_equal(stats2, [tuple(s) for s in ref_stats])
    check_scores(first, ref_scores, co["beta"], nloci)
    check_scores(again, ref_scores, co["beta"], nloci)
    dev.close()


def test_partial_rewrite_keeps_the_other_superblocks():
    n, m = 300_001, 512
    rng = np.random.default_rng(404)
    co = make_cohort(n, m, 777, rng)
    kw = PARAM_GRID[0]
    descs = capi.row_descs(co["beta"], co["eaf"], None, co["rie"])
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, co["codes"])
    # new rows into superblock 1 only
    other = make_cohort(n, 128, 778, np.random.default_rng(405), force_missing_rows=False)
    codes = co["codes"].copy()
    codes[128:256] = other["codes"]
    co1 = dict(co, codes=codes)
    dev.upload(128, other["codes"])
    assert dev.has_tallies()
    assert_tallies_are_the_oracles(dev, co1)
    p, stats, scores, nloci = run_pass(dev, n, kw, descs)
    assert given(p)
    ref_scores, ref_stats, ref_nloci = oracle_scores(co1, kw, 0.0)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, co["beta"], nloci)
    # the generator into superblock 2 only: that superblock carries nothing, the others keep theirs
    dev.synth_at(256, 256, co["seed"] + 9, co["th"][256:384], co["tm"][256:384], co["tmi"][256:384])
    assert not dev.has_tallies()
    assert dev.rows_tallied(0, 256) and not dev.rows_tallied(256, 128) and dev.rows_tallied(384, 128)
    assert not dev.rows_tallied(0, m)
    with pytest.raises(capi.NpsError):
        dev.row_tallies(0, m)
    codes2 = codes.copy()
    codes2[256:384] = refcpu.synth_rows(n, 256, 128, co["seed"] + 9, co["th"][256:384], co["tm"][256:384], co["tmi"][256:384])
    co2 = dict(co, codes=codes2)
    assert_tallies_are_the_oracles(dev, co2, 0, 256)
    head = dict(co2, m=256, codes=codes2[:256], beta=co["beta"][:256], eaf=co["eaf"][:256], rie=co["rie"][:256])
    p, stats, scores, nloci = run_pass(dev, n, kw, descs[:256])
    assert given(p)                                     # rows 0..255: every superblock of the run is valid
    ref_scores, ref_stats, ref_nloci = oracle_scores(head, kw, 0.0)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, head["beta"], nloci)
    p, stats, scores, nloci = run_pass(dev, n, kw, descs)
    assert in_pass(p) and p.n_tally == 0                # the whole cohort: as before this change (512 rows: counted in the pass)
    ref_scores, ref_stats, ref_nloci = oracle_scores(co2, kw, 0.0)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, co["beta"], nloci)
    assert not dev.has_tallies()
    dev.close()


def test_synthetic_cohorts_are_scored_as_before():
    """the benchmark's path: a cohort from the generator carries no tallies and NPS_MODE_AUTO counts them in the pass,
    every time (500 000 samples: the resident grid covers the chip)"""
    n, m = 500_000, 2000
    rng = np.random.default_rng(77)
    eaf = np.round(rng.uniform(0.01, 0.5, m), 4)
    miss = rng.uniform(0.0, 0.1, m)
    beta = np.round(rng.normal(0, 0.02, m), 4)
    th, tm, tmi = refcpu.hwe_thresholds(eaf, miss)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.synth(0, 1234, th, tm, tmi)
    assert not dev.has_tallies() and not dev.rows_tallied(0, 128)
    descs = capi.row_descs(beta, eaf)
    for _ in range(2):
        p, _, _, _ = run_pass(dev, n, PARAM_GRID[0], descs)
        assert in_pass(p) and p.n_tally == 0
        assert not dev.has_tallies()
    dev.close()


def test_two_threads_score_one_uploaded_cohort():
    """two contexts on two threads score one uploaded cohort three times each under NPS_MODE_AUTO (280 000 samples: one row
    team per strip): every pass runs with the write-time tallies given and all six results are the single-threaded one,
    bit for bit"""
    n, m = 280_000, 2048
    rng = np.random.default_rng(99)
    eaf = np.round(rng.uniform(0.01, 0.5, m), 4)
    miss = rng.uniform(0.0, 0.1, m)
    miss[::7] = 0.3
    beta = np.round(rng.normal(0, 0.02, m), 4)
    th, tm, tmi = refcpu.hwe_thresholds(eaf, miss)
    codes = refcpu.synth_rows(n, 0, m, 31, th, tm, tmi)
    descs = capi.row_descs(beta, eaf)
    out, errs = {}, []

    def work(tag, dev, passes):
        try:
            sc = capi.Scorer(n, capi.make_params())
            sc.profile_enable(True)
            res = []
            for _ in range(passes):
                sc.reset()
                sc.score_cohort(dev, descs, 0, capi.MODE_AUTO)
                p = sc.profile_get(reset=True)
                res.append(sc.finish(0.0) + (given(p),))
            sc.close()
            out[tag] = res
        except Exception as e:     # noqa: BLE001
            errs.append((tag, repr(e)))

    ref_dev = capi.Cohort(n, m, fmt=capi.FMT_GT_AUTO)
    ref_dev.upload(0, codes)
    work("ref", ref_dev, 1)
    ref_dev.close()
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT_AUTO)
    dev.upload(0, codes)
    assert dev.has_tallies()
    ts = [threading.Thread(target=work, args=(k, dev, 3)) for k in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    assert dev.has_tallies()
    ref_scores, ref_nloci, ref_given = out["ref"][0]
    assert ref_given
    for k in range(2):
        assert len(out[k]) == 3
        for scores, nloci, was_given in out[k]:
            assert was_given
            assert nloci == ref_nloci
            assert np.array_equal(scores.view(np.int64), ref_scores.view(np.int64))
    dev.close()


@pytest.mark.parametrize("n,geometry", [(253_952, (124, 2, 2048)), (264_192, (134, 1, 1984))])
def test_fused_geometry_reports_the_grid_the_pass_ran_on(n, geometry):
    """on both sides of the switch to strips of 62 units (124 strips, two row teams: the layout's strips of 2048 samples;
    129 strips, one team: 134 strips of 62 units = 1984 samples) nps_fused_geometry tells the grid of the single-read
    kernel, and that kernel and its fold agree on it: a device-generated cohort scored once under NPS_MODE_FUSED gives the
    oracle's statistics and scores on the same rows"""
    m = 256
    co = make_cohort(n, m, 606 + n, np.random.default_rng(n))
    kw = PARAM_GRID[0]
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.synth(0, co["seed"], co["th"], co["tm"], co["tmi"])
    sc = capi.Scorer(n, capi.make_params(**kw))
    assert sc.fused_geometry(m, capi.FMT_GT2X) == geometry
    sc.close()
    p, stats, scores, nloci = run_pass(dev, n, kw, capi.row_descs(co["beta"], co["eaf"], None, co["rie"]), mode=capi.MODE_FUSED)
    assert in_pass(p) and p.n_tally == 0
    ref_scores, ref_stats, ref_nloci = oracle_scores(co, kw, 0.0)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, co["beta"], nloci)
    dev.close()
