"""The boundary cases of the --maxmis and --mincs decisions (tests/decision_cases.py) before the GPU suite relies on them
(tests/test_gpu_decisions.py).  No GPU.

* The oracle (oracle/refcpu.c) and the numpy restatement of the reference's row loop agree bit for bit on every case of
  the small shapes, and in used / reason / nloci at the strip-plan sample counts.
* Every way of getting a decision wrong that decision_cases.FAULTS lists moves at least one row of at least one case of
  the small shapes, and what the faulty scorer returns for that case is rejected by the comparison the GPU test makes
  (decision_cases.compare: nloci, assert_stats_equal, score_compare.assert_scores).  The row statistics have no column
  for the --mincs decision (a row is used and "genotyped" either way), so for mincs_gt, mincs_vs_n and ngen_padded the
  moved decision is the one the scorer takes (Decide.enough), and the rejection rests on the scores and ngenotyped.
* The rows have exactly the missing counts asked for, where asked for, and every t equals the scan's result.
* The faults of a subset run (decision_cases.SUBSET_FAULTS: the layout's sample count where n_kept belongs, tallies that
  count dropped samples) are rejected at 777 and at 4 000 samples each, and the wide embedding the subset paths score
  (tests/wide_cases.py) has the units its layout promises.
"""
import numpy as np
import pytest

import decision_cases as dc
import exact_reference as er
import special_cases as spc
import wide_cases as wc
from oracle import refcpu

SMALL_CASES = [(n, name) for n in dc.SMALL_N for name in dc.table(n).specs()]
# (the case lists tests/test_gpu_decisions.py runs on its strip plans)
STRIP_CASES = [(n, name) for n in dc.STRIP_N for name in dc.table(n).specs(reduced=True if n == 4000 else "large")]


def oracle(packed, n, d):
    return refcpu.score_packed(packed[: d["kind"].size], n, d["kind"], d["rie"], d["beta"], d["eaf"], refcpu.make_params(**d["params"]),
                               d["offset"])


_PACKED = {}


def packed(n):
    if n not in _PACKED:
        _PACKED[n] = dc.pack(dc.table(n).codes())
    return _PACKED[n]


def same_bits(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64),
                                                                        b[~np.isnan(b)].view(np.int64))


@pytest.mark.parametrize("n,name", SMALL_CASES)
def test_oracle_equals_reference_small(n, name):
    """scores, row statistics and nloci, bit for bit: the same operations in the same order"""
    T = dc.table(n)
    d = T.definition(name)
    got, stats, nloci = oracle(packed(n), n, d)
    want, want_stats, want_nloci = dc.reference(T.codes(), d)
    assert nloci == want_nloci
    assert np.array_equal(stats, want_stats), name
    assert same_bits(got, want), name
    used, reason, nl = dc.decisions(n, T.row_missing(d), d)
    assert np.array_equal(used, want_stats["used"]) and np.array_equal(reason, want_stats["reason"]) and nl == nloci


@pytest.mark.parametrize("n,name", STRIP_CASES)
def test_oracle_decisions_at_strip_plan_sample_counts(n, name):
    """used, reason and nloci of the boundary rows at 4 000, 70 000 and 300 001 samples (the strip-plan cohorts repeat
    these very rows)"""
    T = dc.table(n)
    d = T.definition(name)
    _, stats, nloci = oracle(packed(n), n, d)
    used, reason, nl = dc.decisions(n, T.row_missing(d), d)
    assert np.array_equal(stats["nmissing"], T.row_missing(d).astype(np.float64))
    assert np.array_equal(stats["used"], used) and np.array_equal(stats["reason"], reason) and nloci == nl


def moved(n, name, fault):
    """does the fault take another decision than the reference for some row of the case, where the decision can matter
    (the --mincs one fills a row's missing samples: none in the row without any, and NaN either way in the all-missing
    row under int_fail, 0 / 0 or the fall-back)"""
    T, F = dc.table(n), dc.FAULTS[fault]
    p, rows = T.specs()[name][0], T.specs()[name][3]
    for j, k in enumerate(T.counts[:rows]):
        o = dc.EXACT.over(k, n, p["maxmis"])
        if F.over(F.tally(j, k, 0.0, n)[0], n, p["maxmis"]) != o:
            return True
        if not o and p["imp_sample"] in ("int_ps", "int_fail") and k > 0 and (k < n or p["imp_sample"] == "int_ps") and \
                F.enough(k, n, p["mincs"]) != dc.EXACT.enough(k, n, p["mincs"]):
            return True
    return False


def rejected(got, ref, beta, with_stats, what):
    try:
        dc.compare(got[0], got[2], got[1] if with_stats else None, ref[0], ref[1], ref[2], beta, what)
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("fault", list(dc.FAULTS))
def test_every_fault_is_rejected_on_the_small_shapes(fault):
    """--maxmis faults: every case they move a row of is rejected with the row statistics (used / reason differ), every
    such case under --imputelocus ignore also without them (nloci moves with the row; the partial-sum paths return no
    statistics).  Without statistics a moved row can hide elsewhere: an all-missing row below --mincs gets 2 eaf at every
    sample whether as the locus' constant or as each sample's value, and under `fail` every sample is NaN already.
    --mincs faults (no column of the statistics shows that decision): every --mincs case they move a row of is rejected,
    the int_ps ones by the scores alone."""
    killers = [(n, name) for n, name in SMALL_CASES if moved(n, name, fault)]
    assert killers, "no case of the small shapes tells %s from the reference: the case table is short" % fault
    seen = 0
    for n, name in killers:
        T = dc.table(n)
        d = T.definition(name)
        what = "%s, %s at %d" % (fault, name, n)
        ref = dc.reference(T.codes(), d)
        bad = dc.reference(T.codes(), d, dc.FAULTS[fault])
        dc.compare(ref[0], ref[2], ref[1], ref[0], ref[1], ref[2], d["beta"], what)   # (the comparison accepts the truth)
        if fault in dc.MAXMIS_FAULTS:
            assert (bad[1]["used"] != ref[1]["used"]).any() or (bad[1]["reason"] != ref[1]["reason"]).any(), what
            assert rejected(bad, ref, d["beta"], True, what), what
            assert d["params"]["imp_locus"] != "ignore" or rejected(bad, ref, d["beta"], False, what), what
        elif name.startswith("mincs_"):
            assert rejected(bad, ref, d["beta"], True, what), what
            assert not name.endswith("int_ps") or rejected(bad, ref, d["beta"], False, what), what
        seen += rejected(bad, ref, d["beta"], False, what)
    assert seen and any(name.startswith("mincs_triple") or fault in dc.MAXMIS_FAULTS for _, name in killers)


@pytest.mark.parametrize("n", dc.SMALL_N)
@pytest.mark.parametrize("fault", list(dc.SUBSET_FAULTS))
def test_subset_faults_are_rejected_at_each_small_shape(fault, n):
    """the mistakes of a subset run (the layout's n_total where n_kept belongs, tallies that count dropped samples): at
    each of the two small sample counts on its own, some case is rejected by the comparison -- with the statistics, as
    the subset paths return them"""
    T = dc.table(n)
    assert wc.n_total(n) > n
    for name in T.specs():
        if not moved(n, name, fault):
            continue
        d = T.definition(name)
        ref = dc.reference(T.codes(), d)
        bad = dc.reference(T.codes(), d, dc.FAULTS[fault])
        if rejected(bad, ref, d["beta"], True, "%s, %s at %d" % (fault, name, n)):
            return
    raise AssertionError("no case at %d samples rejects %s" % (n, fault))


@pytest.mark.parametrize("n", [33, 777, 1500, 3000, 4000, 70000])
def test_wide_layout_is_what_the_subset_paths_need(n):
    rng = np.random.default_rng(n)
    codes = rng.integers(0, 4, size=(5, n), dtype=np.uint8)
    wide, keep = wc.widen(codes)
    assert keep.dtype == np.uint8 and wide.shape == (5, keep.size) and keep.size == wc.n_total(n)
    assert np.array_equal(wide[:, keep != 0], codes)                       # the kept columns, in order
    assert (wide[0::2][:, keep == 0] == 2).all() and (wide[1::2][:, keep == 0] == 3).all()
    kept, size = wc.unit_masks(keep)
    assert keep.size % wc.UNIT != 0 and size[-1] < wc.UNIT and not keep[-wc.TAIL:].any()   # ragged last unit, dropped tail
    assert np.count_nonzero(kept[:-1] == 0) >= 2                            # wholly dropped units
    assert np.count_nonzero((kept > 0) & (kept < size)) >= 1                # mixed masks
    if n >= 128:                                                            # wholly kept units
        assert np.count_nonzero(kept[:-1] == wc.UNIT) >= 1
    if n >= 2048:
        assert wc.longest_dropped_run(keep) >= 2048
    if n == 4000:    # the eight-fold unrolled loop of the masked dosage tally and its tail loop both run
        assert keep.size > 7168
    if n == 70000:   # four groups of sixteen strips in the masked strip tally
        assert (keep.size + wc.STRIP - 1) // wc.STRIP == 53
    # a leak shows: the tallies over the wide matrix differ from the kept ones in every row
    nm, ne = dc.tallies(codes)
    nmw, new = dc.tallies(wide)
    assert ((nmw != nm) | (new != ne)).all() and np.abs((nmw - nm) + (new - ne)).min() >= keep.size - n
    ds = wc.ds_rows(wide, np.array([0, 1, 0, 1, 0]))
    assert ds.dtype == np.float32 and np.array_equal(np.isnan(ds).sum(axis=1), nmw)


# which threshold of which shape tells which fault from the reference (a scan over the boundary counts, run once):
# removing one of these thresholds from the table fails here
KILLS = {(777, "q49"): ["ge", "mul"], (777, "0.05"): ["pad16", "pad32", "pad2048"], (4000, "0.05"): ["ge", "f32q"],
         (4000, "q9"): ["ge", "rcp"], (4000, "q1001"): ["mul", "rcp"], (70000, "q21"): ["mul"], (70000, "q11"): ["f32q"],
         (300001, "q5"): ["rcp"], (300001, "q13"): ["mul", "rcp"], (777, "below_one"): ["f32", "t_plus_1", "t_minus_1"],
         (4000, "below_one"): ["f32"], (70000, "below_one"): ["f32"], (300001, "below_one"): ["f32"]}


@pytest.mark.parametrize("n,label", list(KILLS))
def test_threshold_kills_the_faults_it_is_there_for(n, label):
    T = dc.table(n)
    for loc in ("ignore", "ps"):
        name = "maxmis_%s_%s" % (label, loc)
        assert name in T.specs(reduced=True) and (loc == "ps" or name in T.specs(reduced="large"))
        d = T.definition(name)
        want = dc.decisions(n, T.row_missing(d), d)
        for fault in KILLS[(n, label)]:
            got = dc.decisions(n, T.row_missing(d), d, dc.FAULTS[fault])
            assert not (np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])), (fault, name)
            assert loc != "ignore" or got[2] != want[2]   # ignore turns a wrong decision into a wrong nloci


@pytest.mark.parametrize("n", sorted(set(dc.SMALL_N + dc.STRIP_N)))
def test_rows_and_thresholds_are_what_the_table_says(n):
    T = dc.table(n)
    codes = T.codes()
    nmiss, neff = dc.tallies(codes)
    assert nmiss.tolist() == T.counts and sorted(T.counts) == dc.row_counts(n)
    # every threshold's t by the scan; the decimal ones as written down, the exact quotients at their k0
    th = dc.thresholds(n)
    assert tuple(dc.threshold_t(n, th["%g" % r]) for r in dc.DECIMALS) == dc.T_DECIMAL[n]
    for k0 in dc.K0[n]:
        assert dc.threshold_t(n, th["q%d" % k0]) == k0 and float(k0) / float(n) == th["q%d" % k0]
    assert [dc.threshold_t(n, th[e]) for e in ("zero", "neg_zero", "denormal", "one", "below_one", "pinf", "nan",
                                                "minus_one")] == [0, 0, 0, n, n - 1, n, n, -1]
    for r in th.values():
        t = dc.threshold_t(n, r)
        assert all(k in T.row_of for k in (t - 1, t, t + 1, t + 2) if 0 <= k <= n)
        assert t == n or dc.EXACT.over(t + 1, n, r)
        assert t < 0 or not dc.EXACT.over(t, n, r)
    # where the missing samples are: both ends of the row, and every strip as soon as there are enough of them
    strips = (n + dc.STRIP - 1) // dc.STRIP
    for j, k in enumerate(T.counts):
        miss = np.nonzero(codes[j] == 2)[0]
        if k >= 2:
            assert miss[0] == 0 and miss[-1] == n - 1
            assert np.unique(miss // dc.STRIP).size >= min(k - 2, strips)
    # the genotyped samples' own frequency is far from 2 eaf
    full = [j for j, k in enumerate(T.counts) if n - k >= 500]
    assert all(abs(neff[j] / (n - T.counts[j]) - 2 * dc.AF) < 0.1 for j in full) and abs(2 * dc.AF - 2 * dc.EAF) >= 0.5
    # packing, the dosage rows, and the rows repeated up to a ragged final superblock
    pk = dc.pack(codes)
    assert np.array_equal(er.unpack(pk, n), codes)
    m = 260
    rie = dc.row_rie(m)
    cyc = dc.cycle(codes, m)
    assert all(np.array_equal(cyc[j], codes[j % T.nb]) for j in (0, 127, 128, m - 1)) and cyc.shape == (m, n)
    ds = dc.ds_rows(cyc[:6], rie[:6])
    assert ds.dtype == np.float32 and np.array_equal(np.isnan(ds).sum(axis=1), nmiss[:6])
    dos = spc.dosages(cyc[:6])
    assert np.array_equal(np.nan_to_num(ds[1], nan=-1), np.nan_to_num(2.0 - dos[1], nan=-1)) and rie[1] == 1
    assert np.array_equal(np.nan_to_num(ds[0], nan=-1), np.nan_to_num(dos[0], nan=-1)) and rie[0] == 0


@pytest.mark.parametrize("n", dc.SMALL_N + dc.STRIP_N[1:])
def test_special_definitions_are_what_their_names_say(n):
    T = dc.table(n)
    m = T.nb if n in dc.SMALL_N else 200
    d = T.definition("beta_inf_at_t", m)
    t = dc.threshold_t(n, 0.05)
    at = np.isinf(d["beta"])
    assert set(np.nonzero(at)[0] % T.nb) == {T.row_of[t], T.row_of[t + 1]}
    used, reason, _ = dc.decisions(n, T.row_missing(d), d)
    assert used[at].min() == 0 and used[at].max() == 1   # one of the two rows is dropped, the other scored
    d2 = T.definition("two_band", m)
    band, F = er.strip_bands(d2["beta"], d2["eaf"])
    assert len(F) == 2 and d2["beta"].max() / d2["beta"].min() > 2.0 ** 30
    used2 = dc.decisions(n, T.row_missing(d2), d2)[0]
    assert all((used2[band == b] == 0).any() and (used2[band == b] == 1).any() for b in (0, 1))
    for name in T.specs():   # no row's decision hides behind a zero beta
        beta = T.definition(name, m)["beta"]
        assert (np.isfinite(beta).all() or name == "beta_inf_at_t") and (np.abs(beta) >= 1e-12).all()
