"""Every group of a sample partition in one pass over a dosage cohort (nps_score_cohort_def_groups, nps_groups.hip).

Group k of the grouped run is held to what tests/test_gpu_subset_ds.py holds the subset run with {label == k} to -- the
oracle's row loop and the double-double sums on the group's columns alone -- and, bit for bit, to that subset run itself, to
the NPS_FMT_DS16 cohort of the same values, and (one group of everybody) to the two-pass whole-cohort run.

Inputs: make_ds of tests/test_gpu_subset_ds.py (three-decimal dosages, so the rows upload losslessly to NPS_FMT_DS16) with
design_rows of tests/test_gpu_subset.py placing the missing genotypes for keep = (label == 0): rows 1 and 5 leave group 0
under --maxmis and every other group's samples all missing, rows 2 and 6 do the opposite, row 3 puts group 0 below --mincs.
Every case with --maxmis < 1.0 and two groups or more asserts that some row's reason differs between group 0 and group 1."""
import functools

import numpy as np
import pytest

import exact_reference as er
import seam_cases as sc
from nimpress_amd import capi
from test_gpu_parity import PARAM_GRID, assert_ds_stats
from test_gpu_subset import _status, make_score, run_subset, run_whole
from test_gpu_subset_ds import make_ds, references

pytestmark = pytest.mark.gpu

NONE = capi.GROUP_NONE


def make_labels(n, G, pattern, rng):
    i = np.arange(n)
    if pattern == "all":
        return np.zeros(n, np.uint8)
    if pattern == "one_none":                # two groups in turn, the last sample in none
        lab = (i % G).astype(np.uint8)
        lab[n - 1] = NONE
        return lab
    if pattern == "interleaved":
        return (i % G).astype(np.uint8)
    if pattern in ("random", "random_none"):
        lab = rng.integers(0, G, n).astype(np.uint8)
        if pattern == "random_none":
            lab[rng.random(n) < 0.1] = NONE
        lab[:G] = np.arange(G)               # (nobody's group is empty)
        return lab
    if pattern == "contiguous":              # borders at odd samples: inside a lane-of-four and inside a block of 256
        border = [0] + [(k * n // G) | 1 for k in range(1, G)] + [n]
        lab = np.zeros(n, np.uint8)
        for k in range(G):
            lab[border[k]:border[k + 1]] = k
        return lab
    if pattern == "single_ends":             # group 0 is the first sample alone, group G - 1 the last one alone
        lab = (1 + (i - 1) * (G - 2) // (n - 2)).astype(np.uint8)
        lab[0], lab[n - 1] = 0, G - 1
        return lab
    if pattern == "contiguous_hole":         # two groups, samples 2048 .. 4095 in none: whole blocks of 256 without a group
        lab = (i >= n // 2 + 1).astype(np.uint8)
        lab[2048:4096] = NONE
        return lab
    raise ValueError(pattern)


CASES = [(1, 1, 1, "all"), (5, 3, 2, "one_none")]
CASES += [(1027, 130, G, p) for G in (3, 5, 8) for p in ("interleaved", "random", "contiguous", "single_ends", "random_none")]
CASES += [(70000, 40, 8, "random"), (70000, 40, 2, "contiguous_hole")]
IDS = ["%dx%d-G%d-%s" % c for c in CASES]
WIDE = [k for k, c in enumerate(CASES) if c[0] >= 1027]


def run_groups(dev, n, kw, descs, groups, offset, pieces=None):
    s = capi.Scorer(n, capi.make_params(**kw))
    defs = []
    for r0, r1 in pieces or [(0, len(descs))]:
        defs.append(capi.ScoreDef(descs[r0:r1]))
        s.score_cohort_def_groups(dev, defs[-1], groups, r0)
    stats = s.flush_groups()
    scores, nloci = s.finish_groups(groups, offset)
    for o in [s] + defs:
        o.close()
    return scores, nloci, stats


@functools.lru_cache(maxsize=None)
def case(k):
    """the inputs of case k and its grouped run on a NPS_FMT_DS32 cohort: made once, shared by the tests, changed by none"""
    n, m, G, pattern = CASES[k]
    kw = PARAM_GRID[k % len(PARAM_GRID)]
    rng = np.random.default_rng(n * 17 + m + 5 * k)
    label = make_labels(n, G, pattern, rng)
    assert sorted(set(label.tolist()) - {NONE}) == list(range(G))
    ds = make_ds(n, m, (label == 0).astype(np.uint8), kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    dev.upload(0, ds)
    groups = capi.SampleGroups(label, G)
    assert groups.n_groups == G and [groups.size(g) for g in range(G)] == [int((label == g).sum()) for g in range(G)]
    scores, nloci, stats = run_groups(dev, n, kw, descs, groups, 0.0)
    groups.close()
    dev.close()
    for a in (label, ds, beta, eaf, rie, descs, scores, nloci, stats):
        a.setflags(write=False)
    return dict(n=n, m=m, G=G, kw=kw, label=label, ds=ds, beta=beta, eaf=eaf, rie=rie, descs=descs, scores=scores, nloci=nloci,
                stats=stats)


def nan_bits(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_groups_vs_references_on_each_group_s_columns(k):
    c = case(k)
    G, kw, label, stats, scores = c["G"], c["kw"], c["label"], c["stats"], c["scores"]
    assert stats.shape == (c["m"], G) and scores.shape == (c["n"],) and c["nloci"].shape == (G,)
    if kw["maxmis"] < 1.0 and G >= 2:
        assert np.any(stats["reason"][:, 0] != stats["reason"][:, 1]), "no row decides differently for groups 0 and 1"
    for g in range(G):
        keep = (label == g).astype(np.uint8)
        ref_stats, ref_nloci, (hi, lo, ab, nl, _, _, _) = references(c["ds"], keep, kw, c["beta"], c["eaf"], c["rie"])
        got = scores[label == g]
        assert int(c["nloci"][g]) == ref_nloci == nl, g
        assert_ds_stats(stats[:, g], ref_stats)
        ok = np.isfinite(got)
        assert np.array_equal(ok, np.isfinite(hi + lo)), "group %d: NaN positions differ" % g
        assert np.all(er.sum_error(got, nl, hi, lo)[ok] <= er.f64_bound(ab, nl, got, nl)[ok]), g
    assert np.all(nan_bits(scores[label == NONE]) == 0x7ff8000000000000)


@pytest.mark.parametrize("k", range(len(CASES)), ids=IDS)
def test_each_group_is_its_subset_run_bit_for_bit(k):
    c = case(k)
    n, label = c["n"], c["label"]
    dev = capi.Cohort(n, c["m"], fmt=capi.FMT_DS32)
    dev.upload(0, c["ds"])
    for g in range(c["G"]):
        sset = capi.SampleSet(label == g)
        sub, nloci, stats = run_subset(dev, n, c["kw"], c["descs"], sset, 0.0)
        sset.close()
        assert stats.tobytes() == np.ascontiguousarray(c["stats"][:, g]).tobytes(), g
        assert sub.tobytes() == np.ascontiguousarray(c["scores"][label == g]).tobytes(), g
        assert nloci == int(c["nloci"][g]), g
    dev.close()


@pytest.mark.parametrize("k", WIDE, ids=[IDS[k] for k in WIDE])
def test_ds16_cohort_gives_the_bits_of_the_ds32_cohort(k):
    c = case(k)
    dev = capi.Cohort(c["n"], c["m"], fmt=capi.FMT_DS16)
    dev.upload(0, c["ds"])
    groups = capi.SampleGroups(c["label"], c["G"])
    scores, nloci, stats = run_groups(dev, c["n"], c["kw"], c["descs"], groups, 0.0)
    groups.close()
    dev.close()
    assert stats.tobytes() == c["stats"].tobytes()
    assert np.array_equal(nloci, c["nloci"])
    assert scores.tobytes() == c["scores"].tobytes()


@pytest.mark.parametrize("shape", [(1, 1), (1027, 130), (70000, 40)])
def test_one_group_of_everybody_is_the_two_pass_run(shape):
    n, m = shape
    rng = np.random.default_rng(n + m)
    kw = PARAM_GRID[(n + m) % len(PARAM_GRID)]
    label = np.zeros(n, np.uint8)
    ds = make_ds(n, m, np.ones(n, np.uint8), kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    dev.upload(0, ds)
    groups = capi.SampleGroups(label, 1)
    scores, nloci, stats = run_groups(dev, n, kw, descs, groups, 0.5)
    groups.close()
    two, nloci_two, stats_two = run_whole(dev, n, kw, descs, 0.5)
    dev.close()
    assert stats.shape == (m, 1) and nloci.tolist() == [nloci_two]
    assert stats.tobytes() == stats_two.tobytes()
    assert scores.tobytes() == two.tobytes()


def test_grouped_calls_accumulate_and_resources_return():
    """rows 0 .. 63 and then 64 .. 129 with one groups object: the results of one call over all 130 rows, which the first test
    holds to the references; nothing is held afterwards"""
    k = CASES.index((1027, 130, 5, "random_none"))
    c = case(k)
    dev = capi.Cohort(c["n"], c["m"], fmt=capi.FMT_DS32)
    dev.upload(0, c["ds"])
    start = capi.live_resources()
    groups = capi.SampleGroups(c["label"], c["G"])
    assert capi.live_resources() > start          # a groups object counts
    scores, nloci, stats = run_groups(dev, c["n"], c["kw"], c["descs"], groups, 0.0, pieces=[(0, 64), (64, 130)])
    groups.close()
    assert capi.live_resources() == start
    dev.close()
    assert stats.tobytes() == c["stats"].tobytes()
    assert np.array_equal(nloci, c["nloci"])
    # (the row chunks of the accumulation differ between one call and two: the sums agree within the references' bound)
    ok = np.isfinite(scores)
    assert np.array_equal(ok, np.isfinite(c["scores"]))
    for g in range(c["G"]):
        keep = (c["label"] == g).astype(np.uint8)
        _, _, (hi, lo, ab, nl, _, _, _) = references(c["ds"], keep, c["kw"], c["beta"], c["eaf"], c["rie"])
        got = scores[c["label"] == g]
        fin = np.isfinite(got)
        assert np.array_equal(fin, np.isfinite(hi + lo))
        assert np.all(er.sum_error(got, nl, hi, lo)[fin] <= er.f64_bound(ab, nl, got, nl)[fin]), g


def test_block_seam_of_the_two_pass_loop():
    """2 samples in 2 groups, 1 048 579 rows at the 256-byte stride: the run crosses score_run_ds's block of 1 048 576 rows;
    each group's statistics and scores are its subset run's, bit for bit"""
    n, m = 2, sc.DS_TALL[1]
    rng = np.random.default_rng(m)
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    seam = sc.assert_crosses("score_run_ds two-pass blocks", sc.seam_ds_twopass(dev.row_stride), m)
    ds = (rng.integers(0, 2001, size=(m, n)) / 1000.0).astype(np.float32)
    ds[rng.random((m, n)) < 0.02] = np.nan
    ds[seam:, 0] = [2.0, 1.0, np.nan]          # the rows behind the seam outweigh the sum in front of it
    ds[seam:, 1] = [np.nan, 2.0, 1.0]
    beta = np.round(rng.normal(0, 0.02, m), 4)
    beta[seam:] = [37.5, -112.25, 64.0]
    eaf = np.round(rng.uniform(0.01, 0.5, m), 4)
    rie = (rng.uniform(size=m) < 0.25).astype(np.int32)
    descs = capi.row_descs(beta, eaf, None, rie)
    kw = dict(imp_locus="ps", imp_missing="homref", imp_sample="int_ps", maxmis=0.05, mincs=1)
    dev.upload(0, ds)
    label = np.array([0, 1], np.uint8)
    groups = capi.SampleGroups(label, 2)
    scores, nloci, stats = run_groups(dev, n, kw, descs, groups, 0.25)
    groups.close()
    assert stats.shape == (m, 2)
    for g in range(2):
        sset = capi.SampleSet(label == g)
        sub, nloci_sub, stats_sub = run_subset(dev, n, kw, descs, sset, 0.25)
        sset.close()
        assert nloci_sub == int(nloci[g])
        assert stats_sub.tobytes() == np.ascontiguousarray(stats[:, g]).tobytes(), g
        assert sub.tobytes() == scores[g:g + 1].tobytes(), g
        assert np.isfinite(sub[0])
    dev.close()


def test_finish_groups_device_writes_the_same_scores():
    import torch
    k = CASES.index((1027, 130, 3, "random_none"))
    c = case(k)
    n = c["n"]
    dev = capi.Cohort(n, c["m"], fmt=capi.FMT_DS32)
    dev.upload(0, c["ds"])
    groups = capi.SampleGroups(c["label"], c["G"])
    s = capi.Scorer(n, capi.make_params(**c["kw"]))
    sd = capi.ScoreDef(c["descs"])
    s.score_cohort_def_groups(dev, sd, groups)
    host, nloci = s.finish_groups(groups, 0.75)
    buf = torch.full((n + 1,), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()    # (the fill runs on torch's stream, the finish on the context's)
    nloci_dev = s.finish_groups_device(groups, 0.75, buf.data_ptr())
    got = buf.cpu().numpy()
    for o in (s, sd, groups, dev):
        o.close()
    assert np.array_equal(nloci_dev, nloci)
    assert got[:-1].tobytes() == host.tobytes()
    assert got[-1] == -1.0      # nothing behind the samples' scores
    assert np.any(np.isnan(host)) and np.all(nan_bits(host[c["label"] == NONE]) == 0x7ff8000000000000)


def test_refusals_leave_the_context_as_it_was():
    import torch
    k = CASES.index((1027, 130, 3, "interleaved"))
    c = case(k)
    n, m, kw, descs, label = c["n"], c["m"], c["kw"], c["descs"], c["label"]
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    dev.upload(0, c["ds"])
    groups = capi.SampleGroups(label, 3)
    twin = capi.SampleGroups(label, 3)                      # the same labels, another object
    other = capi.SampleGroups(np.zeros(n + 1, np.uint8), 1)
    sset = capi.SampleSet(label == 0)
    sd = capi.ScoreDef(descs)
    s = capi.Scorer(n, capi.make_params(**kw))
    whole, nloci_whole, stats_whole = run_whole(dev, n, kw, descs, 0.0)
    buf = torch.zeros(n, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()

    def check(refused):
        for want, word, call in refused:
            status, text = _status(call)
            assert status == want, (want, word, status, text)
            assert word in text + ".", (word, text)

    def plain_run_is_the_plain_result():
        s.reset()
        s.score_cohort(dev, descs, 0, capi.MODE_TWOPASS)
        stats = s.flush()
        scores, nloci = s.finish(0.0)
        assert nloci == nloci_whole and stats.tobytes() == stats_whole.tobytes() and scores.tobytes() == whole.tobytes()

    # ---- a context that is not grouped
    strips = []
    refused = []
    for fmt, name in ((capi.FMT_GT2, "NPS_FMT_GT2"), (capi.FMT_GT2X, "NPS_FMT_GT2X"), (capi.FMT_GT2M, "NPS_FMT_GT2M")):
        co = capi.Cohort(n, m, fmt=fmt)
        strips.append(co)
        refused.append((capi.E_UNSUPPORTED, "this one is %s." % name, lambda co=co: s.score_cohort_def_groups(co, sd, groups)))
    refused.append((capi.E_INVAL, "samples", lambda: s.score_cohort_def_groups(dev, sd, other)))
    refused.append((capi.E_STATE, "grouped", lambda: s.flush_groups()))
    refused.append((capi.E_STATE, "grouped", lambda: s.finish_groups(groups, 0.0)))
    if capi.device_count() > 1:   # a groups object on another device
        far = capi.SampleGroups(label, 3, device=1)
        refused.append((capi.E_INVAL, "device", lambda: s.score_cohort_def_groups(dev, sd, far)))
    check(refused)
    plain_run_is_the_plain_result()
    # ---- a grouped call after plain rows (the plain rows stay what they were)
    check([(capi.E_STATE, "ungrouped rows", lambda: s.score_cohort_def_groups(dev, sd, groups))])
    again, nloci_again = s.finish(0.0)
    assert nloci_again == nloci_whole and again.tobytes() == whole.tobytes()
    # ---- a grouped context
    s.reset()
    s.score_cohort_def_groups(dev, sd, groups)
    row = np.zeros(n, np.float32)
    check([(capi.E_INVAL, "groups object", lambda: s.score_cohort_def_groups(dev, sd, twin)),
           (capi.E_INVAL, "groups object", lambda: s.finish_groups(twin, 0.0)),
           (capi.E_INVAL, "samples", lambda: s.score_cohort_def_groups(dev, sd, other)),
           (capi.E_STATE, "nps_score_cohort", lambda: s.score_cohort(dev, descs, 0, capi.MODE_TWOPASS)),
           (capi.E_STATE, "nps_score_cohort_def", lambda: s.score_cohort_def(dev, sd, 0, capi.MODE_TWOPASS)),
           (capi.E_STATE, "nps_score_cohort_def_subset", lambda: s.score_cohort_def_subset(dev, sd, sset)),
           (capi.E_STATE, "nps_push_ds", lambda: s.push_ds(row, 0, 0.1, 0.2)),
           (capi.E_STATE, "nps_push_gt", lambda: s.push_gt(np.zeros(2 * n, np.int32), 2, 0, 0, 0.1, 0.2)),
           (capi.E_STATE, "nps_push_packed", lambda: s.push_packed(np.zeros((n + 15) // 16, np.uint32), 0, 0.1, 0.2)),
           (capi.E_STATE, "nps_push_bed", lambda: s.push_bed(np.zeros((n + 3) // 4, np.uint8), 0, 0, 0.1, 0.2)),
           (capi.E_STATE, "nps_push_locus", lambda: s.push_locus(capi.ROW_ABSENT, 0, 0.1, 0.2)),
           (capi.E_STATE, "nps_finish", lambda: s.finish(0.0)),
           (capi.E_STATE, "nps_finish_device", lambda: s.finish_device(0.0, buf.data_ptr())),
           (capi.E_STATE, "nps_finish_subset", lambda: s.finish_subset(sset, 0.0)),
           (capi.E_STATE, "nps_partial_device", lambda: s.partial_device(buf.data_ptr())),
           (capi.E_STATE, "nps_flush", lambda: s.flush())])
    s.sync()                                                # nps_flush(ctx, NULL, ..) still synchronises
    stats = s.flush_groups()
    scores, nloci = s.finish_groups(groups, 0.0)
    assert stats.tobytes() == c["stats"].tobytes() and scores.tobytes() == c["scores"].tobytes()
    assert np.array_equal(nloci, c["nloci"])
    plain_run_is_the_plain_result()
    for o in [s, sd, sset, groups, twin, other, dev] + strips:
        o.close()
