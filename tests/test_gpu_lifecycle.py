"""Who owns the device resources of the engine (nps_own.h), seen from outside:

  * buffers that grow on demand give, reused, the bits a fresh context gives (small run, larger run, small run on ONE
    context against the same runs on new ones), and the oracle's scores within the bar of the path's own parity tests;
  * every object gives back what it took: nps_live_resources() before create == after destroy, whatever was done between;
  * a refused call leaves nothing behind and the objects it was made on usable.
"""
import numpy as np
import pytest

import exact_reference as er
import special_cases as spc
from nimpress_amd import capi
from oracle import refcpu
from score_compare import assert_scores
from test_gpu_multi import REL_TOL as MULTI_REL_TOL
from test_gpu_multi import oracle_scores as multi_oracle
from test_gpu_multi import rel_err as multi_rel_err
from test_gpu_mx import check_scores
from test_gpu_parity import REL_TOL, assert_ds_stats, assert_stats_equal, codes_to_bed, make_cohort, rel_err, same_floats

pytestmark = pytest.mark.gpu

SIZES = (777, 4000)        # a ragged tail in words, units and strips; 62-unit strips
ROWS = (128, 1300, 128)    # PRESENT rows of the three runs: one superblock, eleven (not a multiple of 128), one again
SPECIALS = (2, 40, 2)      # special rows (a non-finite beta) of the three runs of the "special" definitions
M = max(ROWS)
PARAMS = dict(spc.P0)
OFFSET = 0.25


class Shape:
    """M rows of codes over n samples, the cohorts that hold them (made on first use) and the oracle's results"""

    def __init__(self, n):
        self.n = n
        co = make_cohort(n, M, 77 + n, np.random.default_rng(n))
        self.packed, self.beta, self.eaf, self.rie = co["codes"], co["beta"], co["eaf"], co["rie"]
        self.thresholds = (co["th"], co["tm"], co["tmi"])
        self.beta_b = np.round(np.random.default_rng(n + 1).normal(0, 0.05, M), 4)   # the second score of the multi runs
        self.cohorts, self.ref = {}, {}

    def ds_rows(self):
        """FORMAT/DS holds the ALT dosage: 2 - dosage where the effect allele is REF"""
        dos = spc.dosages(er.unpack(self.packed, self.n))
        return np.where(self.rie[:, None] == 1, 2.0 - dos, dos).astype(np.float32)

    def cohort(self, key):
        if key not in self.cohorts:
            fmt = {"gt2": capi.FMT_GT2, "gt2x": capi.FMT_GT2X, "gt2x_kept": capi.FMT_GT2X, "ds32": capi.FMT_DS32,
                   "ds16": capi.FMT_DS16, "gt2m": capi.FMT_GT2M}[key]
            co = capi.Cohort(self.n, M, fmt=fmt)
            if key == "gt2m":
                co.convert_from(self.cohort("gt2"))
            else:
                co.upload(0, self.ds_rows() if key in ("ds32", "ds16") else self.packed)
            if key == "gt2x_kept":
                co.keep_tallies()
            self.cohorts[key] = co
        return self.cohorts[key]

    def definition(self, variant, run):
        """the definition of run 0, 1 or 2 over the first ROWS[run] cohort rows"""
        m = ROWS[run]
        beta = self.beta[:m].copy()
        if variant == "special":   # (+inf, -inf and NaN betas, spread over the rows)
            rows = np.linspace(0, m - 1, SPECIALS[run]).astype(int)
            beta[rows] = np.array([spc.INF, -spc.INF, spc.NAN])[np.arange(rows.size) % 3]
        elif variant == "two_band":   # (as exact_reference.two_band_design: the odd rows 2^-31 of their size)
            beta = np.where(np.arange(m) % 2 == 0, beta, beta * 2.0 ** -31)
            assert len(er.strip_bands(beta, self.eaf[:m])[1]) == 2
        return dict(kind=np.zeros(m, np.int32), rie=self.rie[:m], beta=beta, eaf=self.eaf[:m])

    def oracle(self, variant, run):
        key = (variant, ROWS[run], SPECIALS[run] if variant == "special" else 0)
        if key not in self.ref:
            d = self.definition(variant, run)
            scores, stats, nloci = refcpu.score_packed(self.packed[:ROWS[run]], self.n, d["kind"], d["rie"], d["beta"],
                                                       d["eaf"], refcpu.make_params(**PARAMS), OFFSET)
            self.ref[key] = (scores, [tuple(s) for s in stats], nloci)
        return self.ref[key]

    def close(self):
        for co in self.cohorts.values():
            co.close()
        self.cohorts.clear()


_SHAPES = {}


@pytest.fixture(scope="module")
def shapes():
    def get(n):
        if n not in _SHAPES:
            _SHAPES[n] = Shape(n)
        return _SHAPES[n]
    yield get
    for v in _SHAPES.values():
        v.close()
    _SHAPES.clear()


def new_scorer(n):
    return capi.Scorer(n, capi.make_params(**PARAMS))


def run(sc, co, d, mode):
    sc.score_cohort(co, capi.row_descs(d["beta"], d["eaf"], d["kind"], d["rie"]), 0, mode)
    stats = sc.flush()
    scores, nloci = sc.finish(OFFSET)
    return scores, nloci, stats


def assert_same_run(a, b, what):
    """bit for bit: scores (NaN payloads included), nloci and the row statistics"""
    assert a[1] == b[1], what
    assert a[0].tobytes() == b[0].tobytes(), what
    assert a[2].tobytes() == b[2].tobytes(), what


def assert_oracle(D, variant, r, got, key, what):
    """the oracle's nloci, row statistics and scores, each by the helper and the bar of the parity tests of the path:
    tests/test_gpu_parity.py for the row layout and the DS layouts, tests/test_gpu_mx.py for the strip layout,
    tests/test_gpu_special_values.py for a definition with special rows"""
    scores, nloci, stats = got
    ref, ref_stats, ref_nloci = D.oracle(variant, r)
    beta = D.definition(variant, r)["beta"]
    assert nloci == ref_nloci, what
    (assert_ds_stats if key.startswith("ds") else assert_stats_equal)(stats, ref_stats)
    if variant == "special":
        assert_scores(scores, ref, beta, max(nloci, 1), what)
    elif key.startswith("gt2x"):
        check_scores(scores, ref, beta, nloci)
    else:
        assert rel_err(scores, ref, beta, max(nloci, 1)) <= REL_TOL, what


# path -> (cohort, mode)
PATHS = {
    "gt2_fused": ("gt2", capi.MODE_FUSED),
    "gt2_twopass": ("gt2", capi.MODE_TWOPASS),
    "gt2x_in_pass": ("gt2x", capi.MODE_FUSED),
    "gt2x_tallies_given": ("gt2x_kept", capi.MODE_AUTO),
    "gt2x_twopass": ("gt2x", capi.MODE_TWOPASS),
    "ds32_fused": ("ds32", capi.MODE_FUSED),
    "ds32_twopass": ("ds32", capi.MODE_TWOPASS),
    "ds16_fused": ("ds16", capi.MODE_FUSED),
}
RUNS = [(p, "plain") for p in PATHS] + [(p, v) for p in PATHS if p.startswith("gt2x") for v in ("special", "two_band")]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("path,variant", RUNS)
def test_grown_buffers_reused_equal_fresh(shapes, n, path, variant):
    """128, 1 300 and 128 rows again on ONE context (nps_reset between): the per-row buffers grow once and are reused;
    each run equals the same run on a new context bit for bit, and the oracle within the path's bar"""
    D = shapes(n)
    key, mode = PATHS[path]
    co = D.cohort(key)
    reused = new_scorer(n)
    for r in range(len(ROWS)):
        what = "%s %s run %d (%d rows x %d samples)" % (path, variant, r, ROWS[r], n)
        d = D.definition(variant, r)
        got = run(reused, co, d, mode)
        fresh = new_scorer(n)
        assert_same_run(got, run(fresh, co, d, mode), what)
        fresh.close()
        assert_oracle(D, variant, r, got, key, what)
        reused.reset()
    reused.close()


def multi_descs(D, m):
    descs = np.zeros((2, m), dtype=capi.ROW_DESC_DTYPE)
    for s, beta in enumerate((D.beta, D.beta_b)):
        descs[s]["beta"], descs[s]["eaf"], descs[s]["ref_is_effect"] = beta[:m], D.eaf[:m], D.rie[:m]
    return descs


def run_multi(msc, co, descs, offsets):
    mdef = capi.MultiDef(descs)
    msc.score_cohort(co, mdef)
    out = msc.finish(offsets)
    mdef.close()
    return out


def assert_multi_oracle(D, descs, got, nloci, offsets, what):
    ref, ref_nloci = multi_oracle(D.packed[:descs.shape[1]], D.n, descs, PARAMS, offsets)
    assert np.array_equal(nloci.astype(np.int64), ref_nloci), what
    for s in range(descs.shape[0]):
        assert multi_rel_err(got[s], ref[s], float(np.sum(np.abs(descs[s]["beta"]))), int(ref_nloci[s])) <= MULTI_REL_TOL, what


@pytest.mark.parametrize("n", SIZES)
def test_multi_grown_buffers_reused_equal_fresh(shapes, n):
    D = shapes(n)
    co = D.cohort("gt2m")
    offsets = np.array([-0.5, 0.5])
    reused = capi.MultiScorer(n, capi.make_params(**PARAMS), 2)
    for r, m in enumerate(ROWS):
        what = "multi run %d (%d rows x %d samples)" % (r, m, n)
        descs = multi_descs(D, m)
        got, nloci = run_multi(reused, co, descs, offsets)
        fresh = capi.MultiScorer(n, capi.make_params(**PARAMS), 2)
        again, nloci2 = run_multi(fresh, co, descs, offsets)
        fresh.close()
        assert got.tobytes() == again.tobytes() and np.array_equal(nloci, nloci2), what
        if r == 0:
            assert_multi_oracle(D, descs, got, nloci, offsets, what)
        reused.reset()
    reused.close()


# ---- lifecycle balance ------------------------------------------------------------------------------------------------
N_LIFE = 777


def test_context_gives_back_what_it_took(shapes):
    """streamed GT, DS and polyploid rows (the polyploid ring regrows), resident runs in every layout, profiling on with
    its spans never resolved"""
    D = shapes(N_LIFE)
    cohorts = [D.cohort(k) for k in ("gt2", "gt2x", "ds32")]
    d = D.definition("special", 0)
    base = capi.live_resources()
    sc = new_scorer(N_LIFE)
    assert capi.live_resources() > base
    sc.profile_enable(True)
    ds = D.ds_rows()
    for j in range(3):
        sc.push_gt_raw(refcpu.codes_to_gt(D.packed[j], N_LIFE).astype(np.int8), 2, 1, D.rie[j], D.beta[j], D.eaf[j])
        sc.push_ds(ds[j], D.rie[j], D.beta[j], D.eaf[j])
    for ploidy in (3, 4):   # (the wider record makes the pinned ring regrow)
        sc.push_gt(np.arange(N_LIFE * ploidy, dtype=np.int32) % 2, ploidy, 1, 0, 0.01, 0.2)
    sc.flush()
    for co, mode in zip(cohorts + cohorts[:1], [capi.MODE_AUTO] * 3 + [capi.MODE_TWOPASS]):
        sc.reset()
        run(sc, co, d, mode)
    sc.close()   # (profile_get was never called: the spans' events are still held)
    assert capi.live_resources() == base


def test_twenty_context_cycles_leave_nothing(shapes):
    D = shapes(N_LIFE)
    co, d = D.cohort("gt2x"), D.definition("plain", 0)
    base = capi.live_resources()
    for _ in range(20):
        sc = new_scorer(N_LIFE)
        run(sc, co, d, capi.MODE_AUTO)
        sc.close()
    assert capi.live_resources() == base


@pytest.mark.parametrize("key", ["gt2", "gt2x", "gt2m", "ds32", "ds16"])
def test_cohort_gives_back_what_it_took(shapes, key):
    """upload, download, the synthetic fill, nps_cohort_convert, nps_cohort_keep_tallies, nps_cohort_push_* (twice: the
    second, longer row makes the pinned ring regrow) -- whatever the format takes"""
    D = shapes(N_LIFE)
    n, m = N_LIFE, 256
    fmt = {"gt2": capi.FMT_GT2, "gt2x": capi.FMT_GT2X, "gt2m": capi.FMT_GT2M, "ds32": capi.FMT_DS32, "ds16": capi.FMT_DS16}[key]
    rows = D.ds_rows()[:m] if key in ("ds32", "ds16") else D.packed[:m]
    base = capi.live_resources()
    co = capi.Cohort(n, m, fmt=fmt)
    assert capi.live_resources() > base
    th, tm, tmi = (t[:m] for t in D.thresholds)
    co.synth(0, 5, th, tm, tmi)
    if key == "gt2m" or key == "gt2x":
        src = capi.Cohort(n, m)
        src.upload(0, D.packed[:m])
        co.convert_from(src)
        src.close()
    if key != "gt2m":
        co.upload(0, rows)
        back = co.download(0, m)
        assert same_floats(back, rows) if key in ("ds32", "ds16") else np.array_equal(er.unpack(back, n), er.unpack(rows, n))
    if key == "gt2x":
        co.synth(128, 5, th[128:], tm[128:], tmi[128:])   # (these superblocks carry no tallies now)
        co.keep_tallies()
        assert co.has_tallies()
    if key == "gt2":
        co.push_bed(0, codes_to_bed(D.packed[0], n, 1), 1)
        co.push_gt_raw(1, refcpu.codes_to_gt(D.packed[1], n).astype(np.int8), 2, 1)
        co.push_bed(2, codes_to_bed(D.packed[2], n, 0), 0)
        co.push_gt_raw(3, refcpu.codes_to_gt(D.packed[3], n).astype(np.int32), 2, 1)   # four times the bytes
        assert np.array_equal(er.unpack(co.download(0, 4), n), er.unpack(D.packed[:4], n))
    co.close()
    assert capi.live_resources() == base


def test_definitions_and_multi_give_back_what_they_took(shapes):
    D = shapes(N_LIFE)
    co = D.cohort("gt2m")
    base = capi.live_resources()
    for variant in ("plain", "special", "two_band"):   # (one, three and two device copies of the rows, plus the bands')
        d = D.definition(variant, 1)
        sdef = capi.ScoreDef(capi.row_descs(d["beta"], d["eaf"], d["kind"], d["rie"]))
        assert capi.live_resources() > base
        sdef.close()
        assert capi.live_resources() == base
    msc = capi.MultiScorer(N_LIFE, capi.make_params(**PARAMS), 2)
    for m in ROWS:
        run_multi(msc, co, multi_descs(D, m), np.zeros(2))
        msc.reset()
    msc.close()
    assert capi.live_resources() == base


def test_create_then_destroy_balances():
    base = capi.live_resources()
    for make in (lambda: new_scorer(N_LIFE),
                 lambda: capi.Cohort(N_LIFE, 130), lambda: capi.Cohort(N_LIFE, 130, fmt=capi.FMT_GT2X),
                 lambda: capi.Cohort(N_LIFE, 130, fmt=capi.FMT_GT2M), lambda: capi.Cohort(N_LIFE, 130, fmt=capi.FMT_DS32),
                 lambda: capi.Cohort(N_LIFE, 130, fmt=capi.FMT_DS16),
                 lambda: capi.ScoreDef(capi.row_descs([0.5, spc.INF], [0.1, 0.2])), lambda: capi.ScoreDef(capi.row_descs([], [])),
                 lambda: capi.MultiDef(np.zeros((2, 5), dtype=capi.ROW_DESC_DTYPE)),
                 lambda: capi.MultiScorer(N_LIFE, capi.make_params(**PARAMS), 2)):
        obj = make()
        obj.close()
        assert capi.live_resources() == base


# ---- refusals ---------------------------------------------------------------------------------------------------------
def refused(status, call):
    """the call fails with `status` and holds nothing afterwards; returns the message"""
    before = capi.live_resources()
    with pytest.raises(capi.NpsError) as ei:
        call()
    assert ei.value.status == status, ei.value
    assert capi.live_resources() == before
    return str(ei.value)


def assert_still_scores(D, co, mode, key):
    sc = new_scorer(D.n)
    assert_oracle(D, "plain", 0, run(sc, co, D.definition("plain", 0), mode), key, "after a refusal")
    sc.close()


def test_refused_ds16_upload_leaves_nothing(shapes):
    D = shapes(N_LIFE)
    rows = D.ds_rows()[:ROWS[0]]
    co = capi.Cohort(D.n, ROWS[0], fmt=capi.FMT_DS16)
    co.upload(0, rows)
    bad = rows[4:7].copy()
    bad[1, 10] = np.float32(0.12345)   # five places: not the value of a code
    msg = refused(capi.E_UNSUPPORTED, lambda: co.upload(4, bad))
    assert "row 5 " in msg, msg
    co.upload(4, rows[4:7])   # (the rows of a refused range are undefined)
    assert_still_scores(D, co, capi.MODE_FUSED, "ds16")
    co.close()


@pytest.mark.parametrize("key", ["gt2", "gt2x"])
def test_refused_unaligned_upload_leaves_nothing(shapes, key):
    D = shapes(N_LIFE)
    co = D.cohort(key)
    refused(capi.E_INVAL, lambda: co.upload(1, D.packed[1:5]))
    assert_still_scores(D, co, capi.MODE_AUTO, key)


@pytest.mark.parametrize("key", ["gt2", "gt2x"])
def test_refused_bed_code_map_leaves_nothing(shapes, key):
    D = shapes(N_LIFE)
    co = D.cohort(key)
    bed = np.stack([codes_to_bed(D.packed[j], D.n, 0) for j in range(4)])
    refused(capi.E_INVAL, lambda: co.upload_bed(0, bed, [0, 1, 9, 0]))
    assert_still_scores(D, co, capi.MODE_AUTO, key)


def test_refused_synth_without_thresholds_leaves_nothing(shapes):
    D = shapes(N_LIFE)
    co = D.cohort("gt2x")
    th, tm, _ = (np.ascontiguousarray(t[:128], dtype=np.uint32) for t in D.thresholds)
    refused(capi.E_INVAL, lambda: capi._check(capi.load().nps_cohort_synth_rows(co._h, 0, 128, 0, 5, th.ctypes.data,
                                                                                 tm.ctypes.data, None)))
    assert_still_scores(D, co, capi.MODE_AUTO, "gt2x")


def test_refused_scoredef_leaves_nothing(shapes):
    D = shapes(N_LIFE)
    d = D.definition("special", 1)   # (device copies would have been made of these rows)
    kind = d["kind"].copy()
    kind[-1] = 7
    refused(capi.E_INVAL, lambda: capi.ScoreDef(capi.row_descs(d["beta"], d["eaf"], kind, d["rie"])))
    assert_still_scores(D, D.cohort("gt2x"), capi.MODE_AUTO, "gt2x")


@pytest.mark.parametrize("what", ["eaf_inf", "beta_span"])
def test_refused_multidef_leaves_nothing(shapes, what):
    D = shapes(N_LIFE)
    m = ROWS[0]
    descs = multi_descs(D, m)
    bad = descs.copy()
    if what == "eaf_inf":
        bad[1]["eaf"][m - 1] = spc.INF
    else:   # |beta| spans 2^26 > 2^25
        bad[1]["beta"][:] = 1.0
        bad[1]["beta"][m - 1] = 2.0 ** -26
    msc = capi.MultiScorer(D.n, capi.make_params(**PARAMS), 2)
    refused(capi.E_UNSUPPORTED, lambda: capi.MultiDef(bad))
    offsets = np.array([0.0, 1.0])
    got, nloci = run_multi(msc, D.cohort("gt2m"), descs, offsets)
    assert_multi_oracle(D, descs, got, nloci, offsets, "after a refusal")
    msc.close()
