"""The subset paths (nps_score_cohort_def_subset on NPS_FMT_GT2X and NPS_FMT_DS32) and the multi-score paths over dosage
cohorts (nps_score_cohort_multi on NPS_FMT_DS32 and NPS_FMT_DS16) through the three matrices of the earlier paths, with
those modules' own cases, checks and bars -- nothing is restated here:

  * IEEE special values       tests/test_gpu_special_values.py  check, check_multi_gt2m
  * decision boundaries       tests/test_gpu_decisions.py       check
  * exact designs, digit probes, realistic bars
                              tests/test_gpu_exact.py           check_exact, check_two_band, check_digit_probes, check_realistic

The paths are the last four entries of test_gpu_special_values.PATHS (LATER_PATHS).  The subset paths score a wider cohort
whose kept columns are the case's genotypes (tests/wide_cases.py): the sample count of every decision is n_kept = n, that
of the layout is n_total, and the dropped columns are adversarial.  What a path refuses by contract is predicted from the
descriptors (test_gpu_special_values.expected_refusal, written from include/nps.h) and the refusal asserted.
NPS_FMT_GT2M gets every special definition here too (test_multi_score_special_definitions): the definitions of
|beta| = 1e-300, 4.9e-324, 1e300 and 1e307 and the signed zero betas on the matrix cores, and the refusal of |beta| =
DBL_MAX, whose weight bound has no fixed-point scale.
"""
import numpy as np
import pytest

import special_cases as spc
import test_gpu_decisions as tdec
import test_gpu_exact as tex
import test_gpu_special_values as tsv
from nimpress_amd import capi
from score_compare import assert_scores
from test_gpu_parity import PARAM_GRID
from test_gpu_special_values import LATER_PATHS

pytestmark = pytest.mark.gpu


def holder(make, small):
    """get(*key) -> the data object of that key, made on first use; one large shape at a time on the device"""
    held = {}

    def get(*key):
        if key not in held:
            for other in list(held):
                if other[0] not in small:
                    held.pop(other).close()
            held[key] = make(*key)
        return held[key]

    def close():
        for v in held.values():
            v.close()
        held.clear()
    return get, close


@pytest.fixture(scope="module")
def special_data():
    get, close = holder(lambda shape: tsv.Data(*shape), [tsv.SMALL])
    yield get
    close()


@pytest.fixture(scope="module")
def decision_data():
    get, close = holder(lambda shape: tdec.DecisionData(*shape), tdec.SMALL)
    yield get
    close()


@pytest.fixture(scope="module")
def exact_data():
    get, close = holder(lambda shape, over=True: tex.ExactData(*shape, over=over), [tex.SMALL])
    yield get
    close()


@pytest.fixture(scope="module")
def real():
    D = tex.RealData(3000, 400)
    yield D
    D.close()


# ---- IEEE special values
@pytest.mark.parametrize("name", list(spc.CASES))
@pytest.mark.parametrize("path", LATER_PATHS)
def test_special_definition_small(special_data, path, name):
    tsv.check(special_data(tsv.SMALL), name, path)


@pytest.mark.parametrize("name", tsv.STRIP_CASES)
@pytest.mark.parametrize("shape,path", tsv.SUBSET_STRIP_RUNS)
def test_special_definition_strip_plans(special_data, shape, path, name):
    tsv.check(special_data(shape), name, path)


@pytest.mark.parametrize("name", [k for k in spc.CASES if k not in spc.EAF_CASES])
def test_multi_score_special_definitions(special_data, name):
    """NPS_FMT_GT2M (the eaf cases: test_gpu_special_values.test_multi_score_eaf)"""
    tsv.check_multi_gt2m(special_data(tsv.SMALL), name)


def test_multi_score_gt2m_refusal_names_the_score_and_spares_the_context(special_data):
    """finite betas without a fixed-point scale (|beta| = DBL_MAX): the definition is created, a NPS_FMT_GT2M pass refuses
    it naming the score and leaves the context as it was, a dosage pass of the same definition scores it"""
    D = special_data(tsv.SMALL)
    d, ref, _, ref_nloci = D.oracle("magnitude_dbl_max")
    ok, ok_ref = D.oracle("magnitude_1e300")[:2]
    rows = np.stack([tsv.descs(ok), tsv.descs(d)])
    mdef, good = capi.MultiDef(rows), capi.MultiDef(rows[:1])
    msc, one = capi.MultiScorer(D.n, capi.make_params(**d["params"]), 2), capi.MultiScorer(D.n, capi.make_params(**d["params"]), 1)
    try:
        one.score_cohort(D.cohort("gt2m"), good)
        with pytest.raises(capi.NpsError) as ei:
            msc.score_cohort(D.cohort("gt2m"), mdef)
        assert ei.value.status == capi.E_UNSUPPORTED and "score 1" in str(ei.value)
        msc.score_cohort(D.cohort("ds32"), mdef)          # (nothing was added by the refused call)
        got, nloci = msc.finish([ok["offset"], d["offset"]])
        want, nl1 = one.finish([ok["offset"]])
        assert int(nloci[1]) == ref_nloci and int(nloci[0]) == int(nl1[0])
        assert_scores(got[1], ref, d["beta"], max(ref_nloci, 1), "magnitude_dbl_max on a dosage pass")
        assert_scores(got[0], ok_ref, ok["beta"], max(ref_nloci, 1), "magnitude_1e300 beside it")
        assert_scores(want[0], ok_ref, ok["beta"], max(ref_nloci, 1), "magnitude_1e300 on NPS_FMT_GT2M")
    finally:
        for x in (msc, one, mdef, good):
            x.close()


# ---- decision boundaries
@pytest.mark.parametrize("shape,name", tdec.SMALL_RUNS, ids=tdec.ids(tdec.SMALL_RUNS))
@pytest.mark.parametrize("path", LATER_PATHS)
def test_decisions_small(decision_data, path, shape, name):
    tdec.check(decision_data(shape), name, path)


@pytest.mark.parametrize("shape,path,name", tdec.SUBSET_STRIP_RUNS, ids=tdec.ids(tdec.SUBSET_STRIP_RUNS))
def test_decisions_strip_plans(decision_data, shape, path, name):
    tdec.check(decision_data(shape), name, path)


# ---- exact designs, digit probes, realistic bars
@pytest.mark.parametrize("over", [True, False])
@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
@pytest.mark.parametrize("path", LATER_PATHS)
def test_exact_design_small(exact_data, path, pk, over):
    tex.check_exact(exact_data(tex.SMALL, over), ("plain", pk), path)


@pytest.mark.parametrize("pk", [0, 1, 6])
def test_exact_two_band_definition(exact_data, pk):
    tex.check_two_band(exact_data, "subset_gt2x", pk)


@pytest.mark.parametrize("shape,path,n_bands", [(s, p, b) for s, p in tex.SUBSET_PROBE_RUNS for b in tex.PROBE_BANDS])
def test_digit_probes_strip(exact_data, shape, path, n_bands):
    tex.check_digit_probes(exact_data(shape), shape, path, n_bands)


@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
@pytest.mark.parametrize("path", LATER_PATHS)
def test_realistic_within_path_bar(real, path, pk):
    tex.check_realistic(real, path, pk)
