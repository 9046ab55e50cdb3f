"""The --maxmis and --mincs decisions at their exact boundaries on every scoring path, against the oracle.

Every score row is decided twice before any arithmetic: `nmissing / nsamples > maxmis` (nimpress.nim:565-571; a strict
`>`, a float64 quotient, the true sample count) picks locus or sample imputation and with --imputelocus ignore whether the
row counts in nloci; `ngenotyped >= mincs` (nimpress.nim:471) picks the cohort's own frequency or the fall-back.  The
row-layout, streaming, DS two-pass and multi-score kernels do the division; the strip kernels and the single-read DS
kernel compare the count with an integer the host found by bisection; rows with a non-finite beta of a strip cohort are
decided again by the row-layout kernels.  The cohorts here (tests/decision_cases.py) hold one row with exactly k missing
samples for every k in t - 1 .. t + 2 of every threshold: decimal rates, rates that equal a quotient k0 / n exactly, and
0, -0, 1, nextafter(1, 0), 5e-324, +inf, NaN, -1.  tests/test_decision_cases.py vouches for the oracle on these cases and
shows that this module's comparison rejects each of thirteen ways of getting a decision wrong -- and four more that only
a subset run can commit (the paths subset_gt2x and subset_ds32: every threshold here is taken with N = n_kept, while the
layout's sample count is another).
"""
import numpy as np
import pytest

import decision_cases as dc
from nimpress_amd import capi
from oracle import refcpu
from test_gpu_multi import REL_TOL, oracle_scores, rel_err
from test_gpu_special_values import EARLIER_PATHS, PATHS, STRIP_PATHS, Data, refused

pytestmark = pytest.mark.gpu

SMALL = [(n, dc.table(n).nb) for n in dc.SMALL_N]   # 777: a ragged tail in words, units and strips; 4 000: 62-unit strips
# 4 000 x 260: three superblocks, the last ragged, the whole strip-plan case list; 70 000 x 1 000: 35 strips and several row teams, every team decides
# boundary rows; 300 001 x 200: 147 strips, one team, the given-tallies kernel on an uploaded cohort -- these two on the
# shorter list (--maxmis 0.05, two exact quotients, 1.0 and nextafter(1, 0) under ignore, 0.05 under ps, the --mincs
# triple, the infinite betas, the two bands): the oracle's pass over 70 M and 60 M genotypes is most of a case's time
STRIP_SHAPES = [(4000, 260), (70000, 1000), (300001, 200)]


class DecisionData(Data):
    """Data (tests/test_gpu_special_values.py) over the boundary rows of n samples, repeated in order up to m rows"""

    def __init__(self, n, m):
        self.T = dc.table(n)
        self.n, self.m = n, m
        self.packed = np.ascontiguousarray(dc.cycle(dc.pack(self.T.codes()), m))
        self.rie = dc.row_rie(m)
        self.cohorts, self.ref, self._ds = {}, {}, None

    def ds_rows(self):
        if self._ds is None:
            self._ds = dc.ds_rows(dc.cycle(self.T.codes(), self.m), self.rie)
        return self._ds

    def oracle(self, name):
        if name not in self.ref:
            d = self.T.definition(name, self.m)
            scores, stats, nloci = refcpu.score_packed(self.packed[: d["kind"].size], self.n, d["kind"], d["rie"], d["beta"],
                                                       d["eaf"], refcpu.make_params(**d["params"]), d["offset"])
            self.ref[name] = (d, scores, stats, nloci)
        return self.ref[name]


_DATA = {}


@pytest.fixture(scope="module")
def data():
    def get(shape):
        if shape not in _DATA:
            for other in list(_DATA):   # one large shape at a time on the device
                if other not in SMALL:
                    _DATA.pop(other).close()
            _DATA[shape] = DecisionData(*shape)
        return _DATA[shape]
    yield get
    for v in _DATA.values():
        v.close()
    _DATA.clear()


def check(D, name, path):
    d, ref, ref_stats, ref_nloci = D.oracle(name)
    what = "%s on %s (%d x %d)" % (name, path, D.n, D.m)
    if refused(path, d, lambda: PATHS[path](D, d), what):   # (the infinite betas on subset_gt2x and multi_*, two bands on multi_*)
        return
    scores, nloci, stats = PATHS[path](D, d)
    dc.compare(scores, nloci, stats, ref, ref_stats, ref_nloci, d["beta"], what)


SMALL_RUNS = [(s, name) for s in SMALL for name in dc.table(s[0]).specs()]


def ids(runs):
    return ["-".join(["%dx%d" % r[0]] + list(r[1:])) for r in runs]


@pytest.mark.parametrize("shape,name", SMALL_RUNS, ids=ids(SMALL_RUNS))
@pytest.mark.parametrize("path", EARLIER_PATHS)
def test_decisions_small(data, path, shape, name):
    check(data(shape), name, path)


def strip_runs(paths_of):
    return [(s, p, name) for s in STRIP_SHAPES for p in paths_of(s)
            for name in dc.table(s[0]).specs(reduced=True if s == (4000, 260) else "large")]


STRIP_RUNS = strip_runs(lambda s: STRIP_PATHS + (["ds32_fused", "ds32_twopass"] if s == (4000, 260) else []))
# the subset runs (tests/test_gpu_subset_multi_matrices.py): N = n_kept = n in the decisions, the layout that of the wide
# cohort (tests/wide_cases.py) -- 8 157 samples for 4 000 (the masked dosage tally's unrolled loop and its tail), 107 157
# for 70 000 (53 strips: four groups of sixteen in the masked strip tally)
SUBSET_STRIP_RUNS = strip_runs(lambda s: {(4000, 260): ["subset_gt2x", "subset_ds32"], (70000, 1000): ["subset_gt2x"]}.get(s, []))


@pytest.mark.parametrize("shape,path,name", STRIP_RUNS, ids=ids(STRIP_RUNS))
def test_decisions_strip_plans(data, shape, path, name):
    """ds32_fused takes the integer threshold, ds32_twopass does the division"""
    check(data(shape), name, path)


def multi_names(n):
    specs = dc.table(n).specs()
    return [k for k, (p, _, _, _) in specs.items()
            if (k.startswith("maxmis_") and p["imp_locus"] in ("ps", "ignore", "fail")) or not k.startswith("maxmis_")]


MULTI_RUNS = [(s, name) for s in SMALL for name in multi_names(s[0])]


@pytest.mark.parametrize("shape,name", MULTI_RUNS, ids=ids(MULTI_RUNS))
def test_decisions_multi_score(data, shape, name):
    """NPS_FMT_GT2M, two definitions in one pass: the boundary definition, and a copy with other betas that does not list
    every seventh row.  nloci per score exact, scores as tests/test_gpu_multi.py holds them at 56-bit missing weights.
    nps_multidef_create refuses an infinite beta and a beta span past 2^25 by contract: the refusal is asserted."""
    D = data(shape)
    d = D.oracle(name)[0]
    rows = d["kind"].size
    descs = np.stack([capi.row_descs(d["beta"], d["eaf"], d["kind"], d["rie"])] * 2)
    descs[1]["beta"] = -1.5 * np.roll(np.where(np.isfinite(d["beta"]), d["beta"], 0.03), 5)
    if name == "two_band":
        descs[1]["beta"] = np.where(np.arange(rows) % 2 == 0, 0.02, -0.03)
    descs[1]["kind"][np.arange(rows) % 7 == 3] = capi.ROW_NOT_IN_SCORE
    if name in ("beta_inf_at_t", "two_band"):
        with pytest.raises(capi.NpsError) as ei:
            capi.MultiDef(descs)
        assert ei.value.status == capi.E_UNSUPPORTED
        descs = descs[1:]   # the other definition alone is scored
    S = descs.shape[0]
    offsets = np.array([d["offset"], -0.25])[:S]
    msc = capi.MultiScorer(D.n, capi.make_params(**d["params"]), S)
    mdef = capi.MultiDef(descs)
    msc.score_cohort(D.cohort("gt2m"), mdef)
    got, nloci = msc.finish(offsets)
    msc.close()
    mdef.close()
    ref, ref_nloci = oracle_scores(D.packed[:rows], D.n, descs, d["params"], offsets)
    assert np.array_equal(nloci.astype(np.int64), ref_nloci), name
    for s in range(S):
        keep = descs[s]["kind"] != capi.ROW_NOT_IN_SCORE
        err = rel_err(got[s], ref[s], float(np.sum(np.abs(descs[s]["beta"][keep]))), int(ref_nloci[s]))
        assert err <= REL_TOL, (name, s, err)
