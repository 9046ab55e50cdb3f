"""Scoring a chosen subset of a resident cohort's samples (nps_score_cohort_def_subset, nps_subset.hip) on NPS_FMT_GT2X
cohorts, against the CPU oracle run on the column-subset matrix: the plain rows are unpacked, the kept columns taken and
repacked, and refcpu.score_packed scores them with n = n_kept.  nloci and all five statistics fields bit-exact, scores
within check_scores of tests/test_gpu_mx.py (its cap on escapes included).

Rows are uploaded, so that the missing genotypes sit where the test wants them (see design_rows): in every multi-sample
case some rows have them concentrated in the dropped samples and some in the kept ones, at counts that put the subset's
missing rate and the whole cohort's on different sides of --maxmis, and its genotyped count and the whole cohort's on
different sides of --mincs.  Each case then asserts that the subset run really decided differently from a whole-cohort run
with the same parameters:

  * a row whose `reason` differs -- wherever the parameters allow one: with --maxmis 1.0 (PARAM_GRID 4, 5, 6) no row is ever
    over the rate (nmissing / N > 1.0 is false for every count), in either run;
  * with --mincs 3000, a row whose ngenotyped lies on the other side of 3000 -- wherever the cohort has 3000 samples (a
    smaller one is below --mincs in both runs).
"""
import ctypes as C

import numpy as np
import pytest

from nimpress_amd import capi
from oracle import refcpu
from test_gpu_mx import check_scores
from test_gpu_parity import PARAM_GRID, assert_stats_equal

pytestmark = pytest.mark.gpu

PATTERNS = ["alternate", "half", "first", "last", "unit_dropped", "strip_dropped", "ragged_last"]


def keep_pattern(n, pattern, rng):
    """uint8[n], or None where the pattern does not apply to n samples (it would keep nobody, or everybody)"""
    n_units, P = (n + 31) // 32, (n + 2047) // 2048
    k = np.zeros(n, np.uint8)
    if pattern == "all":
        k[:] = 1
    elif pattern == "alternate":
        k[::2] = 1
    elif pattern == "half":
        k[rng.random(n) < 0.5] = 1
    elif pattern == "first":
        k[0] = 1
    elif pattern == "last":
        k[n - 1] = 1
    elif pattern == "unit_dropped":
        if n_units < 2:
            return None
        u = (n_units - 1) // 2
        k[:] = 1
        k[32 * u:32 * u + 32] = 0
    elif pattern == "strip_dropped":
        if P < 2:
            return None
        s = (P - 1) // 2
        k[:] = 1
        k[2048 * s:2048 * s + 2048] = 0
    elif pattern == "ragged_last":     # only the last unit of the layout, which has fewer than 32 samples
        if n_units < 2 or n % 32 == 0:
            return None
        k[32 * (n_units - 1):] = 1
    else:
        raise ValueError(pattern)
    if n > 1 and (k.all() or not k.any()):
        return None
    return k


def pack(codes):
    """[rows, n] 2-bit codes -> [rows, ceil(n / 16)] uint32, sample i in bits 2 (i % 16) of word i / 16 (exact_reference.unpack, inverted)"""
    m, n = codes.shape
    words = (n + 15) // 16
    c = np.zeros((m, words * 16), np.uint8)
    c[:, :n] = codes
    b = c[:, 0::4] | (c[:, 1::4] << 2) | (c[:, 2::4] << 4) | (c[:, 3::4] << 6)   # four samples per byte, little-endian words
    return np.ascontiguousarray(b).view("<u4")


def last_count_not_over(n, rate):
    """largest k in 0 .. n with not (k / n > rate), the reference's own expression (nimpress.nim:565); -1: none"""
    k = min(n, int(rate * n) + 2)
    while k >= 0 and k / n > rate:
        k -= 1
    return k


def design_rows(n, m, keep, kw, rng, fill):
    """Which samples of which rows are missing.  fill(row, idx): make row `row` missing at samples idx and nowhere else.
      rows 1, 5 (A): every dropped sample missing, and as many kept ones as --maxmis just allows the SUBSET: the whole cohort
                     is over the rate (whenever more than one sample is dropped), the subset is not
      rows 2, 6 (B): no dropped sample missing, and one kept sample more than --maxmis allows the subset: the subset is over
                     the rate, the whole cohort is not (whenever the dropped samples are many enough to dilute it)
      row 3     (C): --mincs genotyped kept samples less one, every dropped sample genotyped: the subset is below --mincs, the
                     whole cohort is not
      row 4        : three in ten of all samples missing"""
    kept, dropped = np.nonzero(keep)[0], np.nonzero(keep == 0)[0]
    t = last_count_not_over(kept.size, kw["maxmis"])
    for r in (1, 5):
        if r < m:
            fill(r, np.concatenate([dropped, kept[:max(t, 0)]]))
    for r in (2, 6):
        if r < m:
            fill(r, kept[:min(kept.size, t + 1)] if t < kept.size else kept[:(kept.size * 3 + 4) // 5])
    if 3 < m:
        g = int(kw["mincs"]) - 1
        fill(3, kept[g:] if 0 < g < kept.size else kept[:0])
    if 4 < m:
        fill(4, np.nonzero(rng.random(n) < 0.3)[0])


def make_codes(n, m, keep, kw, rng):
    """plain NPS_CODE_* codes [m, n]: Hardy-Weinberg-like dosages, two in a hundred missing, the designed rows on top"""
    lut = np.array([0] * 55 + [1] * 30 + [3] * 13 + [2] * 2, np.uint8)
    codes = lut[rng.integers(0, 100, size=(m, n), dtype=np.uint8)]

    def fill(row, idx):
        x = codes[row]
        x[x == 2] = 0
        x[idx] = 2
    design_rows(n, m, keep, kw, rng, fill)
    return codes


def make_score(m, rng):
    beta = np.round(rng.normal(0, 0.02, m), 4)
    eaf = np.round(rng.uniform(0.01, 0.5, m), 4)
    rie = (rng.uniform(size=m) < 0.25).astype(np.int32)
    return beta, eaf, rie


def run_subset(dev, n, kw, descs, sset, offset, row0=0):
    sc = capi.Scorer(n, capi.make_params(**kw))
    sd = capi.ScoreDef(descs)
    sc.score_cohort_def_subset(dev, sd, sset, row0)
    stats = sc.flush()
    scores, nloci = sc.finish_subset(sset, offset)
    sc.close()
    sd.close()
    return scores, nloci, stats


def run_whole(dev, n, kw, descs, offset, mode=capi.MODE_TWOPASS):
    sc = capi.Scorer(n, capi.make_params(**kw))
    sc.score_cohort(dev, descs, 0, mode)
    stats = sc.flush()
    scores, nloci = sc.finish(offset)
    sc.close()
    return scores, nloci, stats


def assert_decided_differently(n, kw, stats, whole):
    """the case proves something about N = n_kept (module docstring)"""
    if kw["maxmis"] < 1.0:
        assert np.any(stats["reason"] != whole["reason"]), "no row's reason differs from the whole-cohort run"
    if kw["mincs"] == 3000 and n >= 3000:
        assert np.any((stats["ngenotyped"] >= 3000) != (whole["ngenotyped"] >= 3000)), "no row's ngenotyped crosses --mincs"


SMALL = [(33, 129), (2049, 257), (4100, 40)]
LARGE = [((70000, 300), ["half", "strip_dropped", "ragged_last"]),   # 35 strips: three groups of sixteen in the tally grid
         ((530000, 130), ["alternate", "strip_dropped"])]             # more strips than compute units
CASES = [((1, 1), "all", 0)]
for _shape in SMALL:
    for _p in PATTERNS:
        if keep_pattern(_shape[0], _p, np.random.default_rng(0)) is not None:
            # (4 100 samples, half kept: --mincs 3000 -- n_kept is below it, the cohort is not)
            CASES.append((_shape, _p, 5 if (_shape, _p) == ((4100, 40), "half") else len(CASES) % len(PARAM_GRID)))
for _shape, _ps in LARGE:
    for _p in _ps:
        CASES.append((_shape, _p, len(CASES) % len(PARAM_GRID)))
CASES.append(((4100, 40), "half", 6))


@pytest.mark.parametrize("shape,pattern,pk", CASES, ids=["%dx%d-%s-pk%d" % (s[0], s[1], p, k) for s, p, k in CASES])
def test_gt2x_subset_vs_oracle_on_the_kept_columns(shape, pattern, pk):
    n, m = shape
    rng = np.random.default_rng(n * 31 + m + 7 * pk)
    kw = PARAM_GRID[pk]
    keep = keep_pattern(n, pattern, rng)
    codes = make_codes(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT_AUTO)
    assert dev.fmt == capi.FMT_GT2X
    dev.upload(0, pack(codes))
    sset = capi.SampleSet(keep)
    n_kept = int(keep.sum())
    assert sset.n_kept == n_kept
    scores, nloci, stats = run_subset(dev, n, kw, descs, sset, 0.25)
    if n > 1:
        _, _, whole = run_whole(dev, n, kw, descs, 0.25)
    sset.close()
    dev.close()
    sub = pack(codes[:, keep != 0])
    ref_scores, ref_stats, ref_nloci = refcpu.score_packed(sub, n_kept, np.zeros(m, np.int32), rie, beta, eaf,
                                                           refcpu.make_params(**kw), 0.25)
    assert scores.shape == (n_kept,)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, beta, nloci)
    if n > 1:
        assert_decided_differently(n, kw, stats, whole)


@pytest.mark.parametrize("shape", [(1, 1), (2049, 257), (70000, 300)])
def test_gt2x_every_sample_kept_is_the_two_pass_run(shape):
    """statistics and scores equal bit for bit to NPS_MODE_TWOPASS on the same context parameters; finish_subset == finish"""
    n, m = shape
    rng = np.random.default_rng(n + m)
    kw = PARAM_GRID[(n + m) % len(PARAM_GRID)]
    keep = np.ones(n, np.uint8)
    codes = make_codes(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, pack(codes))
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


def test_gt2x_subset_runs_accumulate():
    """a 384-row cohort scored as rows 0 .. 255 and then 256 .. 383 with one set: the oracle on all 384 rows"""
    n, m = 4100, 384
    rng = np.random.default_rng(384)
    kw = PARAM_GRID[0]
    keep = keep_pattern(n, "half", rng)
    codes = make_codes(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, pack(codes))
    sset = capi.SampleSet(keep)
    sc = capi.Scorer(n, capi.make_params(**kw))
    d1, d2 = capi.ScoreDef(descs[:256]), capi.ScoreDef(descs[256:])
    sc.score_cohort_def_subset(dev, d1, sset, 0)
    sc.score_cohort_def_subset(dev, d2, sset, 256)
    stats = sc.flush()
    scores, nloci = sc.finish_subset(sset, 0.0)
    for o in (sc, d1, d2, sset, dev):
        o.close()
    n_kept = int(keep.sum())
    ref_scores, ref_stats, ref_nloci = refcpu.score_packed(pack(codes[:, keep != 0]), n_kept, np.zeros(m, np.int32), rie, beta,
                                                           eaf, refcpu.make_params(**kw), 0.0)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, beta, nloci)


def test_finish_subset_device_writes_the_same_scores():
    """nps_finish_subset_device into a caller's device buffer of n_kept doubles: the bits nps_finish_subset copies out"""
    import torch
    n, m = 2049, 129
    rng = np.random.default_rng(12)
    kw = PARAM_GRID[0]
    keep = keep_pattern(n, "half", rng)
    codes = make_codes(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, pack(codes))
    sset = capi.SampleSet(keep)
    sc = capi.Scorer(n, capi.make_params(**kw))
    sd = capi.ScoreDef(capi.row_descs(beta, eaf, None, rie))
    sc.score_cohort_def_subset(dev, sd, sset)
    host, nloci = sc.finish_subset(sset, 0.75)
    buf = torch.full((sset.n_kept + 1,), -1.0, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()    # (the fill runs on torch's stream, the gather on the context's)
    nloci_dev = sc.finish_subset_device(sset, 0.75, buf.data_ptr())
    got = buf.cpu().numpy()
    for o in (sc, sd, sset, dev):
        o.close()
    assert nloci_dev == nloci
    assert got[:-1].tobytes() == host.tobytes()
    assert got[-1] == -1.0      # nothing behind the kept samples' scores


def test_gt2x_banded_definition_is_scored():
    """a definition whose weights span more than 2^30 is scored in magnitude bands, one masked tally per band"""
    n, m = 2049, 130
    rng = np.random.default_rng(5)
    kw = PARAM_GRID[0]
    keep = keep_pattern(n, "alternate", rng)
    codes = make_codes(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    beta[::3] *= 2.0 ** -40
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, pack(codes))
    sset = capi.SampleSet(keep)
    scores, nloci, stats = run_subset(dev, n, kw, descs, sset, 0.0)
    sset.close()
    dev.close()
    n_kept = int(keep.sum())
    ref_scores, ref_stats, ref_nloci = refcpu.score_packed(pack(codes[:, keep != 0]), n_kept, np.zeros(m, np.int32), rie, beta,
                                                           eaf, refcpu.make_params(**kw), 0.0)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, beta, nloci)


def test_subset_leaves_the_cohort_s_kept_tallies_alone():
    """an uploaded strip cohort carries whole-cohort tallies: a subset run neither uses nor changes them"""
    n, m = 4100, 130
    rng = np.random.default_rng(9)
    kw = PARAM_GRID[0]
    keep = keep_pattern(n, "half", rng)
    codes = make_codes(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, pack(codes))
    assert dev.rows_tallied(0, m)
    nm0, ne0 = dev.row_tallies()
    sset = capi.SampleSet(keep)
    _, _, stats = run_subset(dev, n, kw, descs, sset, 0.0)
    sset.close()
    assert dev.rows_tallied(0, m)
    nm1, ne1 = dev.row_tallies()
    dev.close()
    assert np.array_equal(nm0, nm1) and np.array_equal(ne0, ne1)
    assert np.array_equal(nm0, (codes == 2).sum(axis=1))
    assert np.array_equal(stats["nmissing"], (codes[:, keep != 0] == 2).sum(axis=1))


# ---- refusals
def _status(call):
    try:
        call()
    except capi.NpsError as e:
        return e.status, str(e)
    return capi.NPS_OK, ""


def test_refusals_leave_the_context_as_it_was():
    n, m = 2049, 130
    rng = np.random.default_rng(77)
    kw = PARAM_GRID[0]
    keep = keep_pattern(n, "half", rng)
    codes = make_codes(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    descs = capi.row_descs(beta, eaf, None, rie)
    L = capi.load()
    h = C.c_void_p()
    # creation
    assert L.nps_sampleset_create(C.byref(h), 0, n, None) == capi.E_INVAL
    assert L.nps_sampleset_create(C.byref(h), 0, 0, keep.ctypes.data) == capi.E_INVAL
    assert L.nps_sampleset_create(C.byref(h), 0, n, np.zeros(n, np.uint8).ctypes.data) == capi.E_INVAL
    assert not h.value

    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, pack(codes))
    sset = capi.SampleSet(keep)
    sd = capi.ScoreDef(descs)
    sc = capi.Scorer(n, capi.make_params(**kw))
    refused = []
    # the set's samples differ from the context's and the cohort's
    other = capi.SampleSet(np.ones(n + 1, np.uint8))
    refused.append((capi.E_INVAL, "samples", lambda: sc.score_cohort_def_subset(dev, sd, other)))
    refused.append((capi.E_INVAL, "samples", lambda: sc.finish_subset(other, 0.0)))
    # a strip cohort is scored from a superblock boundary
    sd_short = capi.ScoreDef(descs[:2])
    refused.append((capi.E_INVAL, "128", lambda: sc.score_cohort_def_subset(dev, sd_short, sset, 64)))
    # the three formats without a masked tally, named
    others = []
    for fmt, name in ((capi.FMT_GT2, "NPS_FMT_GT2"), (capi.FMT_GT2M, "NPS_FMT_GT2M"), (capi.FMT_DS16, "NPS_FMT_DS16")):
        co = capi.Cohort(n, m, fmt=fmt)
        others.append(co)
        refused.append((capi.E_UNSUPPORTED, "this one is %s." % name, lambda co=co: sc.score_cohort_def_subset(co, sd, sset)))
    # a row of the strip path's IEEE special pass, named
    sp = descs.copy()
    sp["beta"][17] = np.inf
    sd_special = capi.ScoreDef(sp)
    refused.append((capi.E_UNSUPPORTED, "row 17", lambda: sc.score_cohort_def_subset(dev, sd_special, sset)))
    if capi.device_count() > 1:   # a set on another device
        far = capi.SampleSet(keep, device=1)
        refused.append((capi.E_INVAL, "device", lambda: sc.score_cohort_def_subset(dev, sd, far)))
    for want, word, call in refused:
        status, text = _status(call)
        assert status == want, (want, word, status, text)
        assert word in text + ".", (word, text)
    # scoring afterwards on the same context gives the result of a fresh context
    sc.score_cohort_def_subset(dev, sd, sset)
    stats = sc.flush()
    scores, nloci = sc.finish_subset(sset, 0.0)
    sc.close()
    fresh, nloci_fresh, stats_fresh = run_subset(dev, n, kw, descs, sset, 0.0)
    assert nloci == nloci_fresh
    assert stats.tobytes() == stats_fresh.tobytes()
    assert scores.tobytes() == fresh.tobytes()
    for o in [dev, sset, sd, other, sd_short, sd_special] + others:
        o.close()


def test_resources_return_to_their_starting_value():
    n, m = 2049, 130
    rng = np.random.default_rng(3)
    kw = PARAM_GRID[0]
    keep = keep_pattern(n, "alternate", rng)
    codes = make_codes(n, m, keep, kw, rng)
    beta, eaf, rie = make_score(m, rng)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, pack(codes))
    start = capi.live_resources()
    sset = capi.SampleSet(keep)
    assert capi.live_resources() > start          # a sample set counts
    run_subset(dev, n, kw, capi.row_descs(beta, eaf, None, rie), sset, 0.0)
    sset.close()
    assert capi.live_resources() == start
    dev.close()
