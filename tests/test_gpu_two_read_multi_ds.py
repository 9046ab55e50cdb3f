"""GPU parity tests of the multi-score path over dosage cohorts (nps_multi_ds.hip): S score definitions over a
NPS_FMT_DS32 / NPS_FMT_DS16 cohort in two reads of the genotypes (nps_score_cohort_multi), every score against the
oracle run once per score -- refcpu.RefScorer fed row_ds / row_locus for the rows the score lists (the reference's loop,
nimpress.nim:634-641, S times; NPS_ROW_NOT_IN_SCORE rows are not rows of that score).

Bars: nloci, nmissing and NaN positions exact; scores within test_gpu_multi's REL_TOL (floored); the row tallies bit for
bit those of the single-score streaming path; a definition's column bit for bit the same whatever shares the pass; one
realistic case within exact_reference.f64_bound of the double-double reference."""
import numpy as np
import pytest

import exact_reference as er
from nimpress_amd import capi
from oracle import refcpu
from test_gpu_exact import PARAM_GRID as EXACT_PARAM_GRID
from test_gpu_multi import PARAM_GRID, REL_TOL, make_case, rel_err
from test_gpu_parity import make_ds16_cohort, make_ds_cohort

pytestmark = pytest.mark.gpu

FMTS = {"ds32": (capi.FMT_DS32, make_ds_cohort), "ds16": (capi.FMT_DS16, make_ds16_cohort)}


def make_ds_case(n, m, S, seed, fmt, with_kinds=True):
    """a dosage cohort (missing rate 0-10 % per row: both --maxmis branches occur) and S definitions with their own beta /
    eaf / effect allele and the row kinds of test_gpu_multi.make_case"""
    co = FMTS[fmt][1](n, m, 1000 + seed, np.random.default_rng(seed))
    descs = make_case(n, m, S, seed, with_kinds=with_kinds)[4]
    return np.ascontiguousarray(co["ds"]), descs


def upload(ds, fmt):
    m, n = ds.shape
    dev = capi.Cohort(n, m, fmt=FMTS[fmt][0])
    dev.upload(0, ds)
    return dev


def oracle_add(sc, ds, d):
    """the rows of one definition, in order, into a RefScorer"""
    for j in range(d.size):
        k = int(d["kind"][j])
        if k == capi.ROW_NOT_IN_SCORE:
            continue
        if k == capi.ROW_PRESENT:
            sc.row_ds(ds[j], bool(d["ref_is_effect"][j]), float(d["beta"][j]), float(d["eaf"][j]))
        else:
            sc.row_locus(k, bool(d["ref_is_effect"][j]), float(d["beta"][j]), float(d["eaf"][j]))


def oracle_scores(ds, descs, params_kw, offsets):
    out, nl = [], []
    for s in range(descs.shape[0]):
        sc = refcpu.RefScorer(ds.shape[1], refcpu.make_params(**params_kw))
        oracle_add(sc, ds, descs[s])
        scores, nloci = sc.finish(float(offsets[s]))
        out.append(scores.copy())
        nl.append(nloci)
    return np.stack(out), np.array(nl)


def assert_scores(got, nloci, ref, ref_nloci, descs):
    assert np.array_equal(np.asarray(nloci).astype(np.int64), ref_nloci)
    for s in range(descs.shape[0]):
        keep = descs[s]["kind"] != capi.ROW_NOT_IN_SCORE
        err = rel_err(got[s], ref[s], float(np.sum(np.abs(descs[s]["beta"][keep]))), int(ref_nloci[s]))
        assert err <= REL_TOL, (s, err)


def run(dev, descs, params_kw, offsets, row0=0):
    msc = capi.MultiScorer(dev.n_samples, capi.make_params(**params_kw), descs.shape[0])
    mdef = capi.MultiDef(descs)
    msc.score_cohort(dev, mdef, row0)
    got, nloci = msc.finish(offsets)
    got = got.copy()
    msc.close()
    mdef.close()
    return got, nloci


SHAPES = [(1, 1, 1), (3, 7, 2), (1023, 9, 3), (1025, 17, 8), (4099, 129, 5), (257, 300, 6)]


@pytest.mark.parametrize("fmt", list(FMTS))
@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
@pytest.mark.parametrize("shape", SHAPES)
def test_multi_ds_vs_oracle(shape, pk, fmt):
    """(3, 7): fewer than four live samples in the only lane; (1025, 17): a second block and a ragged eight-row unroll"""
    n, m, S = shape
    kw = PARAM_GRID[pk]
    ds, descs = make_ds_case(n, m, S, 100 * pk + n + m, fmt)
    dev = upload(ds, fmt)
    offsets = np.linspace(-0.5, 0.5, S)
    msc = capi.MultiScorer(n, capi.make_params(**kw), S)
    mdef = capi.MultiDef(descs)
    msc.score_cohort(dev, mdef)
    got, nloci = msc.finish(offsets)
    got = got.copy()
    nm, sm, sf = msc.row_tallies()
    assert np.array_equal(nm, np.isnan(ds).sum(axis=1).astype(np.uint64))
    ref, ref_nloci = oracle_scores(ds, descs, kw, offsets)
    assert_scores(got, nloci, ref, ref_nloci, descs)
    # after a reset the same call gives the same bits
    msc.reset()
    msc.score_cohort(dev, mdef)
    again, nloci2 = msc.finish(offsets)
    assert np.array_equal(again, got, equal_nan=True) and np.array_equal(nloci, nloci2)
    for x in (msc, mdef, dev):
        x.close()


@pytest.mark.parametrize("fmt", list(FMTS))
def test_multi_ds_row_tallies_equal_the_streaming_path_bit_for_bit(fmt):
    """nmissing, sum and sum_flipped of a pass == nmissing / neffect of nps_flush for the same rows pushed with nps_push_ds,
    ref_is_effect 0 and 1.  4 099 samples: the plain loop alone; 7 173: thread 0 alone takes one turn of the eight-fold
    unrolled loop; 8 193: every thread does, and thread 0 a lane-of-four more"""
    m = 40
    for n in (4099, 7173, 8193):
        ds, descs = make_ds_case(n, m, 1, 7, fmt, with_kinds=False)
        dev = upload(ds, fmt)
        msc = capi.MultiScorer(n, capi.make_params(), 1)
        mdef = capi.MultiDef(descs)
        msc.score_cohort(dev, mdef)
        nm, sm, sf = msc.row_tallies()
        nm2, sm2, sf2 = msc.row_tallies(first=5, n=3)
        assert np.array_equal(nm2, nm[5:8]) and np.array_equal(sm2, sm[5:8]) and np.array_equal(sf2, sf[5:8])
        for rie, got in ((0, sm), (1, sf)):
            sc = capi.Scorer(n, capi.make_params())
            for j in range(m):
                sc.push_ds(ds[j], rie, 0.01, 0.3)
            st = sc.flush()
            sc.close()
            assert np.array_equal(st["nmissing"], nm), n
            assert np.array_equal(st["neffect"].view(np.int64), got.view(np.int64)), (n, rie)
        for x in (msc, mdef, dev):
            x.close()


def test_multi_ds_column_is_independent_of_the_other_definitions():
    """eight definitions: each column of the S = 8 pass equals, bit for bit, the definition scored alone and as column 3 of
    an S = 5 pass (the row-chunk plan never depends on S)"""
    n, m = 4099, 129
    ds, descs = make_ds_case(n, m, 8, 11, "ds32")
    dev = upload(ds, "ds32")
    kw = PARAM_GRID[1]
    all8, nl8 = run(dev, descs, kw, np.zeros(8))
    for s in range(8):
        one, nl1 = run(dev, descs[s:s + 1], kw, np.zeros(1))
        assert nl1[0] == nl8[s] and np.array_equal(one[0].view(np.int64), all8[s].view(np.int64)), s
        five = np.stack([descs[(s + 1) % 8], descs[(s + 5) % 8], descs[(s + 2) % 8], descs[s], descs[(s + 3) % 8]])
        got5, nl5 = run(dev, five, kw, np.zeros(5))
        assert nl5[3] == nl8[s] and np.array_equal(got5[3].view(np.int64), all8[s].view(np.int64)), s
    dev.close()


def test_multi_ds_row_chunk_seam():
    """the smallest row count whose accumulation plan has at least two row chunks and a last chunk shorter than the others"""
    n, S = 1025, 2
    msc = capi.MultiScorer(n, capi.make_params(), S)
    found = None
    for m in range(1, 4097):
        chunks, per = msc.geometry(m, capi.FMT_DS32)
        assert chunks * per >= m > (chunks - 1) * per
        if chunks >= 2 and m % per:
            found = (m, chunks, per)
            break
    msc.close()
    assert found, ("the row-chunk loop of multi_ds_accumulate_kernel (grid.y, nps_multi_ds.hip: multi_ds_plan) has no plan "
                   "with two chunks and a ragged last one for 1 025 samples and up to 4 096 rows")
    m = found[0]
    for fmt in FMTS:
        ds, descs = make_ds_case(n, m, S, 23, fmt)
        dev = upload(ds, fmt)
        assert capi.MultiScorer(n, capi.make_params(), S).geometry(m, FMTS[fmt][0]) == found[1:]
        got, nloci = run(dev, descs, PARAM_GRID[0], np.zeros(S))
        ref, ref_nloci = oracle_scores(ds, descs, PARAM_GRID[0], np.zeros(S))
        assert_scores(got, nloci, ref, ref_nloci, descs)
        dev.close()


def test_multi_ds_calls_accumulate():
    """rows 0 .. 255 and 256 .. m of one cohort as two calls == the one call; a context that scores a GT2M cohort and then a
    DS32 cohort == the oracle fed both blocks in order"""
    n, m, S = 257, 300, 3
    kw = PARAM_GRID[0]
    ds, descs = make_ds_case(n, m, S, 31, "ds32")
    dev = upload(ds, "ds32")
    offsets = np.array([0.0, 0.25, -0.25])
    one, nl1 = run(dev, descs, kw, offsets)
    msc = capi.MultiScorer(n, capi.make_params(**kw), S)
    a, b = capi.MultiDef(np.ascontiguousarray(descs[:, :256])), capi.MultiDef(np.ascontiguousarray(descs[:, 256:]))
    msc.score_cohort(dev, a, 0)
    msc.score_cohort(dev, b, 256)
    two, nl2 = msc.finish(offsets)
    ref, ref_nloci = oracle_scores(ds, descs, kw, offsets)
    assert np.array_equal(nl1, nl2)
    assert_scores(two, nl2, ref, ref_nloci, descs)
    assert_scores(two, nl2, one, ref_nloci, descs)
    for x in (msc, a, b, dev):
        x.close()

    # a 2-bit block of 128 rows, then a dosage block of 130 rows, one context
    mg, md = 128, 130
    eaf_c, th, tm, tmi, gdescs = make_case(n, mg, S, 77, with_kinds=False)
    codes = refcpu.synth_rows(n, 0, mg, 5, th, tm, tmi)
    gt = capi.Cohort(n, mg, fmt=capi.FMT_GT2M)
    gt.synth(0, 5, th, tm, tmi)
    ds, ddescs = make_ds_case(n, md, S, 78, "ds32")
    dev = upload(ds, "ds32")
    msc = capi.MultiScorer(n, capi.make_params(**kw), S)
    g, d = capi.MultiDef(gdescs), capi.MultiDef(ddescs)
    msc.score_cohort(gt, g)
    with pytest.raises(capi.NpsError) as e:      # (the last pass was on 2-bit genotypes)
        msc.row_tallies(0, 1)
    assert e.value.status == capi.E_STATE
    msc.score_cohort(dev, d)
    got, nloci = msc.finish(offsets)
    ref, ref_nloci = [], []
    for s in range(S):
        sc = refcpu.RefScorer(n, refcpu.make_params(**kw))
        for j in range(mg):
            sc.row_gt(refcpu.codes_to_gt(codes[j], n), 2, 1, bool(gdescs[s]["ref_is_effect"][j]), float(gdescs[s]["beta"][j]),
                      float(gdescs[s]["eaf"][j]))
        oracle_add(sc, ds, ddescs[s])
        scores, nl = sc.finish(float(offsets[s]))
        ref.append(scores.copy())
        ref_nloci.append(nl)
    both = np.concatenate([gdescs, ddescs], axis=1)
    assert_scores(got, nloci, np.stack(ref), np.array(ref_nloci), both)
    for x in (msc, g, d, dev, gt):
        x.close()


def test_multi_ds_takes_any_finite_dosage_and_the_counts_effect_bit():
    """-0.25 and 2.5 are scored as the oracle scores those floats (the [0, 2] range belongs to the fused kernel); a
    descriptor with RIE_COUNTS_EFFECT | 1 is not flipped and imputes homref as 2"""
    n, m, S = 300, 12, 2
    rng = np.random.default_rng(3)
    ds = rng.choice(np.array([-0.25, 0.0, 0.5, 1.0, 1.5, 2.0, 2.5, np.nan], np.float32), size=(m, n),
                    p=[.1, .3, .1, .2, .1, .1, .05, .05]).astype(np.float32)
    descs = make_case(n, m, S, 9, with_kinds=False)[4]
    dev = upload(ds, "ds32")
    for pk in (0, 2):
        got, nloci = run(dev, descs, PARAM_GRID[pk], np.zeros(S))
        ref, ref_nloci = oracle_scores(ds, descs, PARAM_GRID[pk], np.zeros(S))
        assert_scores(got, nloci, ref, ref_nloci, descs)
    dev.close()
    # rows that already count the effect allele: the oracle gets 2 - DS (exact for these values) with ref_is_effect = 1, which
    # flips it back and imputes homref as 2
    ds = rng.choice(np.array([0.0, 0.5, 1.0, 1.5, 2.0, np.nan], np.float32), size=(m, n),
                    p=[.3, .1, .3, .1, .1, .1]).astype(np.float32)
    kw = dict(imp_locus="homref", imp_missing="homref", imp_sample="homref", maxmis=0.10, mincs=0)
    counted = descs.copy()
    counted["ref_is_effect"] = capi.RIE_COUNTS_EFFECT | 1
    mirrored = descs.copy()
    mirrored["ref_is_effect"] = 1
    dev = upload(ds, "ds32")
    got, nloci = run(dev, counted, kw, np.zeros(S))
    ref, ref_nloci = oracle_scores((np.float32(2.0) - ds).astype(np.float32), mirrored, kw, np.zeros(S))
    assert 0 < int((np.isnan(ds).mean(axis=1) > 0.10).sum()) < m      # both the sample and the locus imputation
    assert_scores(got, nloci, ref, ref_nloci, counted)
    dev.close()


def test_multi_ds_realistic_cohort_within_f64_bar():
    """as test_gpu_exact.test_realistic_ds_cohort_within_f64_bar: n = 2 500, m = 300, S = 3, parameter sets 0 and 6"""
    n, m, S = 2500, 300, 3
    for fmt in FMTS:
        co = FMTS[fmt][1](n, m, 17, np.random.default_rng(17))
        ds = np.ascontiguousarray(co["ds"])
        rng = np.random.default_rng(18)
        betas = [co["beta"], np.round(rng.normal(0, 0.2, m), 4), -co["beta"]]
        ries = [co["rie"], 1 - co["rie"], co["rie"]]
        descs = np.stack([capi.row_descs(betas[s], co["eaf"], None, ries[s]) for s in range(S)])
        dev = upload(ds, fmt)
        for pk in (0, 6):
            p = EXACT_PARAM_GRID[pk]
            got, nl_got = run(dev, descs, p, np.zeros(S))
            for s in range(S):
                dos = np.where(ries[s][:, None] == 1, 2.0 - ds.astype(np.float64), ds.astype(np.float64))
                hi, lo, ab, nl, _, _, _ = er.dd_reference(dos, betas[s], co["eaf"], ries[s], p)
                assert int(nl_got[s]) == nl
                ok = np.isfinite(got[s])
                assert np.all(er.sum_error(got[s], nl, hi, lo)[ok] <= er.f64_bound(ab, nl, got[s], nl)[ok]), (fmt, pk, s)
        dev.close()


def test_multi_ds_refusals_leave_nothing_behind():
    base = capi.live_resources()
    n, m, S = 64, 128, 2
    descs = np.zeros((S, m), dtype=capi.ROW_DESC_DTYPE)
    descs["beta"] = 0.01
    descs["eaf"] = 0.3
    msc = capi.MultiScorer(n, capi.make_params(), S)
    mdef = capi.MultiDef(descs)
    gx = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    wide = capi.Cohort(n + 1, m, fmt=capi.FMT_DS32)
    held = capi.live_resources()
    with pytest.raises(capi.NpsError) as e:
        msc.score_cohort(gx, mdef)
    assert e.value.status == capi.E_INVAL and all(f in str(e.value) for f in ("NPS_FMT_GT2M", "NPS_FMT_DS32", "NPS_FMT_DS16"))
    with pytest.raises(capi.NpsError) as e:
        msc.score_cohort(wide, mdef)
    assert e.value.status == capi.E_INVAL
    with pytest.raises(capi.NpsError) as e:
        msc.row_tallies(0, 1)
    assert e.value.status == capi.E_STATE
    with pytest.raises(capi.NpsError) as e:
        msc.geometry(m, capi.FMT_GT2M)
    assert e.value.status == capi.E_UNSUPPORTED
    assert capi.live_resources() == held
    dev.upload(0, np.ones((m, n), np.float32))
    msc.score_cohort(dev, mdef)
    got, nloci = msc.finish(np.zeros(S))
    assert np.array_equal(nloci, [m, m]) and np.allclose(got, 0.005)
    with pytest.raises(capi.NpsError) as e:
        msc.row_tallies(m, 1)
    assert e.value.status == capi.E_INVAL
    msc.reset()
    with pytest.raises(capi.NpsError) as e:
        msc.row_tallies(0, 1)
    assert e.value.status == capi.E_STATE
    for x in (msc, mdef, gx, dev, wide):
        x.close()
    assert capi.live_resources() == base
