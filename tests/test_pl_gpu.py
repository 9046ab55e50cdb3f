"""GPU tests of FORMAT/PL (include/nps.h above nps_push_pl): the device decode against the numpy restatement bit for bit
through the resident seam (nps_cohort_push_pl + nps_cohort_download), streamed rows against the same rows pushed as
dosages and against the oracle, REF-effect rows against the float64 bound of tests/exact_reference.py, resident scoring of
pushed rows, and refusals that leave nothing behind."""
import ctypes as C

import numpy as np
import pytest

import exact_reference as er
import pl_reference as plr
from nimpress_amd import capi
from oracle import refcpu
from test_gpu_parity import PARAM_GRID, REL_TOL, assert_ds_stats, rel_err

pytestmark = pytest.mark.gpu

WIDTHS = (np.int8, np.int16, np.int32)


@pytest.fixture(scope="module")
def table():
    return capi.pl_likelihoods()


# ------------------------------------------------------------------------------------------------------------------
# decode exactness
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4099])
def test_device_decode_equals_reference_bit_for_bit(table, n):
    """every (alleles, effect allele, width) as one row of a DS32 cohort of n samples: a 256-thread block, its last partial
    block and the 16-byte tail read (3-byte samples: int8, A = 2; 72-byte samples: int16, A = 8); rows pushed out of
    order, one row pushed twice (the second push wins)"""
    rng = np.random.default_rng(7000 + n)
    cases = [(A, dt, e) for A in (2, 3, 4, 8) for dt in WIDTHS for e in range(A)]
    vectors = {(A, dt): plr.random_pl(rng, n, A, dt) for A in (2, 3, 4, 8) for dt in WIDTHS}
    dev = capi.Cohort(n, len(cases), fmt=capi.FMT_DS32)
    order = rng.permutation(len(cases))
    twice = int(order[len(order) // 2])
    A, dt, e = cases[twice]
    dev.push_pl(twice, plr.random_pl(rng, n, A, dt), A, e)          # overwritten below
    for r in order:
        A, dt, e = cases[r]
        dev.push_pl(int(r), vectors[(A, dt)], A, e)
    got = dev.download(0, len(cases))
    dev.close()
    n_nan = 0
    for r, (A, dt, e) in enumerate(cases):
        ref = plr.pl_dosage(vectors[(A, dt)], A, e, table)
        assert plr.same_bits(got[r], ref), (n, A, dt, e, got[r][:8], ref[:8])
        n_nan += int(np.isnan(ref).sum())
    if n >= 255:
        assert 0.05 <= n_nan / (n * len(cases)) <= 0.40


# ------------------------------------------------------------------------------------------------------------------
# streamed rows
def pl_rows(rng, n, m, effect_ref):
    """m PL records of n samples: (typed vector, A, e); the share of missing samples runs from 3 % to 40 % over the rows"""
    rows = []
    for j in range(m):
        A = (2, 3, 4, 2)[j % 4]
        dt = WIDTHS[j % 3]
        e = 0 if effect_ref else 1 + j % (A - 1)
        share = 0.03 + 0.37 * j / max(m - 1, 1)
        rows.append((plr.random_pl(rng, n, A, dt, p_bad=share * 0.7, p_flat=share * 0.3), A, e))
    return rows


def random_gt(rng, n):
    alle = rng.integers(-1, 2, size=(n, 2))
    alle[rng.uniform(size=n) < 0.03] = -1
    return (((alle + 1) << 1) | rng.integers(0, 2, size=(n, 2))).astype(np.int32)


@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
def test_streamed_pl_equals_streamed_dosages_and_oracle(table, pk):
    """effect allele an ALT, ref_is_effect = 0: 40 rows of nps_push_pl against nps_push_ds of the numpy rows on a second
    context -- statistics identical in every field, scores in every bit -- and both against the oracle's row_ds, with
    no-data rows and GT rows between them.  --maxmis 0.15 under every imputation mode: some PL rows go over it, not all"""
    n, m = 300, 40
    kw = dict(PARAM_GRID[pk], maxmis=0.15)
    rng = np.random.default_rng(300 + pk)
    rows = pl_rows(rng, n, m, effect_ref=False)
    a, b = capi.Scorer(n, capi.make_params(**kw)), capi.Scorer(n, capi.make_params(**kw))
    ref = refcpu.RefScorer(n, refcpu.make_params(**kw))
    betas, is_pl = [], []
    for j, (pl, A, e) in enumerate(rows):
        beta, eaf = float(rng.normal(0, 0.1)), float(rng.uniform(0.05, 0.6))
        ds = plr.pl_dosage(pl, A, e, table)
        a.push_pl(pl, A, e, 0, beta, eaf)
        b.push_ds(ds, 0, beta, eaf)
        ref.row_ds(ds, False, beta, eaf)
        betas.append(beta)
        is_pl.append(True)
        if j % 5 == 1:
            kind = [capi.ROW_UNCOVERED, capi.ROW_ABSENT, capi.ROW_FILTERED][j % 3]
            for s in (a, b):
                s.push_locus(kind, j % 2, beta * 0.5, eaf)
            ref.row_locus(kind, bool(j % 2), beta * 0.5, eaf)
            betas.append(beta * 0.5)
            is_pl.append(False)
        if j % 7 == 3:
            gts = random_gt(rng, n)
            for s in (a, b):
                s.push_gt(gts.ravel(), 2, 1, 0, -beta, eaf)
            ref.row_gt(gts.ravel(), 2, 1, False, -beta, eaf)
            betas.append(-beta)
            is_pl.append(False)
    sa, sb = a.flush(), b.flush()
    (ga, na), (gb, nb) = a.finish(0.25), b.finish(0.25)
    a.close()
    b.close()
    assert sa.tobytes() == sb.tobytes()
    assert na == nb and ga.tobytes() == gb.tobytes()
    over = sa["reason"][np.array(is_pl)] == capi.REASON_MAXMIS
    assert 0 < int(over.sum()) < m
    ref_scores, ref_nloci = ref.finish(0.25)
    assert na == ref_nloci
    assert_ds_stats(sa, ref.stats)
    assert rel_err(ga, ref_scores, betas, max(na, 1)) <= REL_TOL


def expected_decisions(dos, kw):
    n = dos.shape[1]
    nm = np.isnan(dos).sum(axis=1)
    over = nm / float(n) > kw["maxmis"]
    used = np.where(over, kw["imp_locus"] != "ignore", True)
    return nm, over, used


@pytest.mark.parametrize("pk", [0, 1, 2, 3, 6])
def test_streamed_pl_effect_allele_is_ref(table, pk):
    """e = 0, ref_is_effect = 1: the row counts REF itself (no 2 - DS; the flag only selects the homref value): scores within
    the float64 bound of the double-double reference on the numpy dosages, nmissing / used / reason / nloci exact"""
    n, m = 300, 40
    kw = PARAM_GRID[pk]
    rng = np.random.default_rng(900 + pk)
    rows = pl_rows(rng, n, m, effect_ref=True)
    beta = np.round(rng.normal(0, 0.05, m), 4)
    eaf = np.round(rng.uniform(0.05, 0.6, m), 4)
    rie = np.ones(m, np.int32)
    dos = np.stack([plr.pl_dosage(pl, A, e, table) for pl, A, e in rows]).astype(np.float64)
    sc = capi.Scorer(n, capi.make_params(**kw))
    for j, (pl, A, e) in enumerate(rows):
        sc.push_pl(pl, A, e, 1, beta[j], eaf[j])
    stats = sc.flush()
    got, nloci = sc.finish(0.0)
    sc.close()
    nm, over, used = expected_decisions(dos, kw)
    assert np.array_equal(stats["nmissing"], nm) and np.array_equal(stats["ngenotyped"], n - nm)
    assert np.array_equal(stats["reason"], np.where(over, capi.REASON_MAXMIS, capi.REASON_GENOTYPED))
    assert np.array_equal(stats["used"], used.astype(np.int32))
    hi, lo, ab, nl, _, _, _ = er.dd_reference(dos, beta, eaf, rie, kw)
    assert nloci == nl == int(used.sum())
    ok = np.isfinite(got)
    assert ok.any() or kw["imp_sample"] in ("fail", "int_fail") or kw["imp_locus"] == "fail"
    assert np.array_equal(ok, np.isfinite(hi))
    assert np.all(er.sum_error(got, nl, hi, lo)[ok] <= er.f64_bound(ab, nl, got, nl)[ok])
    # the tallied sums are those of the REF counts themselves, not of 2 - DS
    assert np.allclose(stats["neffect"][~over], np.nansum(dos, axis=1)[~over], rtol=1e-9, atol=0.0)


# ------------------------------------------------------------------------------------------------------------------
# resident: rows pushed into a DS32 cohort, scored with the single-score and the multi-score entry points
def streamed(rows, rie, beta, eaf, kw):
    sc = capi.Scorer(rows[0][0].shape[0], capi.make_params(**kw))
    for j, (pl, A, e) in enumerate(rows):
        sc.push_pl(pl, A, e, int(rie[j]), beta[j], eaf[j])
    stats = sc.flush()
    scores, nloci = sc.finish(0.0)
    sc.close()
    return stats, scores, nloci


@pytest.mark.parametrize("pk", [0, 1])
def test_resident_pl_rows(table, pk):
    n, m, S = 1000, 40, 2
    kw = PARAM_GRID[pk]
    rng = np.random.default_rng(40 + pk)
    rows = pl_rows(rng, n, m, effect_ref=False)
    rows = [(pl, A, 0 if j % 3 == 0 else e) for j, (pl, A, e) in enumerate(rows)]        # every third row counts REF
    rie = np.array([1 if e == 0 else 0 for _, _, e in rows], np.int32)
    betas = [np.round(rng.normal(0, 0.05, m), 4), np.round(rng.normal(0, 0.2, m), 4)]
    eaf = np.round(rng.uniform(0.05, 0.6, m), 4)
    dos = np.stack([plr.pl_dosage(pl, A, e, table) for pl, A, e in rows]).astype(np.float64)
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    for j in rng.permutation(m):
        dev.push_pl(int(j), rows[j][0], rows[j][1], rows[j][2])
    flags = rie | capi.RIE_COUNTS_EFFECT
    want = [streamed(rows, rie, betas[s], eaf, kw) for s in range(S)]
    refs = [er.dd_reference(dos, betas[s], eaf, rie, kw) for s in range(S)]

    def within_bar(got, nloci, s):
        hi, lo, ab, nl = refs[s][:4]
        assert nloci == nl == want[s][2]
        ok = np.isfinite(got)
        assert np.array_equal(ok, np.isfinite(want[s][1]))
        assert np.all(er.sum_error(got, nl, hi, lo)[ok] <= er.f64_bound(ab, nl, got, nl)[ok])
        # against the streamed result of the same rows: two results inside one bar are within twice the bar of each other
        assert np.all(er.sum_error(want[s][1], nl, hi, lo)[ok] <= er.f64_bound(ab, nl, want[s][1], nl)[ok])
        bar = 2 * er.f64_bound(ab, nl, got, nl) / (2.0 * max(nl, 1))
        assert np.all(np.abs(got - want[s][1])[ok] <= bar[ok])

    for mode in (capi.MODE_AUTO, capi.MODE_TWOPASS):
        sc = capi.Scorer(n, capi.make_params(**kw))
        sdef = capi.ScoreDef(capi.row_descs(betas[0], eaf, None, flags))
        sc.score_cohort_def(dev, sdef, 0, mode)
        stats = sc.flush()
        got, nloci = sc.finish(0.0)
        sc.close()
        sdef.close()
        for f in ("ngenotyped", "nmissing", "used", "reason"):
            assert np.array_equal(stats[f], want[0][0][f]), (mode, f)
        assert np.allclose(stats["neffect"], want[0][0]["neffect"], rtol=1e-9, atol=0.0)
        within_bar(got, nloci, 0)

    msc = capi.MultiScorer(n, capi.make_params(**kw), S)
    mdef = capi.MultiDef(np.stack([capi.row_descs(betas[s], eaf, None, flags) for s in range(S)]))
    msc.score_cohort(dev, mdef)
    nmiss, sums, _ = msc.row_tallies()
    got, nloci = msc.finish(np.zeros(S))
    msc.close()
    mdef.close()
    dev.close()
    assert np.array_equal(nmiss, want[0][0]["nmissing"])
    assert np.allclose(sums, want[0][0]["neffect"], rtol=1e-9, atol=0.0)
    for s in range(S):
        within_bar(got[s], int(nloci[s]), s)


# ------------------------------------------------------------------------------------------------------------------
# refusals
def test_refusals_leave_state_untouched(table):
    base = capi.live_resources()
    L = capi.load()
    n, m = 300, 6
    kw = PARAM_GRID[0]
    rng = np.random.default_rng(77)
    rows = pl_rows(rng, n, m, effect_ref=False)
    beta, eaf = np.round(rng.normal(0, 0.05, m), 4), np.full(m, 0.3)
    clean = streamed(rows, np.zeros(m, np.int32), beta, eaf, kw)

    def refused_ctx(h, pl, A, e):
        p = pl.ctypes.data
        held = capi.live_resources()
        assert L.nps_push_pl(h, p, 3, A, e, 0, 0.5, 0.5) == capi.E_INVAL               # elem_bytes
        assert L.nps_push_pl(h, p, 0, A, e, 0, 0.5, 0.5) == capi.E_INVAL
        assert L.nps_push_pl(h, p, pl.dtype.itemsize, A, -1, 0, 0.5, 0.5) == capi.E_INVAL     # eaidx
        assert L.nps_push_pl(h, p, pl.dtype.itemsize, A, A, 0, 0.5, 0.5) == capi.E_INVAL
        assert L.nps_push_pl(h, None, pl.dtype.itemsize, A, e, 0, 0.5, 0.5) == capi.E_INVAL   # NULL with n > 0
        assert L.nps_push_pl(h, p, pl.dtype.itemsize, 1, 0, 0, 0.5, 0.5) == capi.E_UNSUPPORTED  # alleles
        assert L.nps_push_pl(h, p, pl.dtype.itemsize, 9, 0, 0, 0.5, 0.5) == capi.E_UNSUPPORTED
        assert b"alleles" in L.nps_last_error()
        assert capi.live_resources() == held

    sc = capi.Scorer(n, capi.make_params(**kw))
    for j, (pl, A, e) in enumerate(rows):
        refused_ctx(sc._h, pl, A, e)
        sc.push_pl(pl, A, e, 0, beta[j], eaf[j])
    stats = sc.flush()
    got, nloci = sc.finish(0.0)
    sc.close()
    assert stats.tobytes() == clean[0].tobytes() and got.tobytes() == clean[1].tobytes() and nloci == clean[2]

    # the resident seam
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    gt2 = capi.Cohort(n, 4, fmt=capi.FMT_GT2)
    ds16 = capi.Cohort(n, 4, fmt=capi.FMT_DS16)
    for j, (pl, A, e) in enumerate(rows):
        p, eb = pl.ctypes.data, pl.dtype.itemsize
        held = capi.live_resources()
        assert L.nps_cohort_push_pl(dev._h, j, p, 3, A, e) == capi.E_INVAL
        assert L.nps_cohort_push_pl(dev._h, j, p, eb, A, A) == capi.E_INVAL
        assert L.nps_cohort_push_pl(dev._h, j, p, eb, A, -1) == capi.E_INVAL
        assert L.nps_cohort_push_pl(dev._h, j, None, eb, A, e) == capi.E_INVAL
        assert L.nps_cohort_push_pl(dev._h, m, p, eb, A, e) == capi.E_INVAL             # row outside the cohort
        assert L.nps_cohort_push_pl(dev._h, j, p, eb, 1, 0) == capi.E_UNSUPPORTED
        assert L.nps_cohort_push_pl(dev._h, j, p, eb, 9, 0) == capi.E_UNSUPPORTED
        assert L.nps_cohort_push_pl(gt2._h, 0, p, eb, A, e) == capi.E_UNSUPPORTED       # not a DS32 cohort
        assert L.nps_cohort_push_pl(ds16._h, 0, p, eb, A, e) == capi.E_UNSUPPORTED
        assert capi.live_resources() == held
        dev.push_pl(j, pl, A, e)
    got_rows = dev.download(0, m)
    for j, (pl, A, e) in enumerate(rows):
        assert plr.same_bits(got_rows[j], plr.pl_dosage(pl, A, e, table))
    for c in (dev, gt2, ds16):
        c.close()
    assert capi.live_resources() == base
