"""IEEE special values on every scoring path that takes a single-score definition, against the oracle.

The definitions (tests/special_cases.py) put +-inf and NaN betas, +-inf and NaN eafs, signed zero betas, infinite and NaN
offsets, whole definitions at |beta| = 1e-300, 4.9e-324, 1e300, 1e307 and DBL_MAX, and banded definitions with an infinite
row on explicit genotypes (hom-ref, het, hom-alt and missing samples at known positions, an all-hom-ref row, a row without a
missing sample, a row over --maxmis, a fully missing row).  The reference accumulates in plain float64, so every path must
give its NaN, +inf and -inf at the same samples and its finite samples within the usual bar (tests/score_compare.py), and
row statistics bit for bit.  The multi-score path refuses an infinite eaf (as it refuses a non-finite beta) and scores a NaN
eaf.  tests/test_oracle_special_values.py vouches for the oracle on exactly these definitions.

PATHS is the table the decision and exact matrices run as well (tests/test_gpu_decisions.py, tests/test_gpu_exact.py).  Its
last four entries: subset_gt2x and subset_ds32 score the same genotypes as the kept columns of a wider cohort
(tests/wide_cases.py) with nps_score_cohort_def_subset -- the sample count of the decisions is n_kept = n, that of the
layout n_total; multi_ds32 and multi_ds16 score the definition beside a decoy in one nps_score_cohort_multi pass over a
dosage cohort and check that pass's row tallies.  What a path refuses by contract is predicted from the descriptors
(expected_refusal, written from include/nps.h) and the refusal asserted; everywhere else the scores are.
"""
import re
import time
import warnings

import numpy as np
import pytest

import decision_cases as dc
import exact_reference as er
import special_cases as spc
import wide_cases as wc
from nimpress_amd import capi
from oracle import refcpu
from score_compare import assert_scores
from test_gpu_parity import assert_stats_equal, codes_to_bed

pytestmark = pytest.mark.gpu

SMALL = (777, 13)
# strip plans: 62-unit strips (2 layout strips, 3 virtual); one strip with 16 row teams; 35 strips x 7 teams; 147 strips,
# one team each
STRIP_SHAPES = [(4000, 13), (1500, 2000), (70000, 1000), (300000, 200)]
STRIP_CASES = ["beta_pinf", "beta_nan", "beta_pinf_ninf", "beta_inf_maxmis_ps", "eaf_pinf_sample_ps", "eaf_nan_sample_ps",
               "eaf_ninf_locus_ps", "magnitude_1e-300", "magnitude_1e307", "magnitude_dbl_max", "banded_inf_row_dropped"]


class Data:
    """explicit codes of one shape, the cohorts that hold them (made on first use) and the oracle's results"""

    def __init__(self, n, m):
        self.n, self.m = n, m
        self.codes = spc.base_codes(n, m)
        self.packed = spc.pack(self.codes)
        self.rie = (np.arange(m) % 5 == spc.ROW_OVER).astype(np.int32)   # == special_cases.definition's PRESENT rows
        self.cohorts = {}
        self.ref = {}

    def cohort(self, key):
        if key in self.cohorts:
            return self.cohorts[key]
        n, m = self.n, self.m
        if key in ("gt2", "gt2_opt"):
            co = capi.Cohort(n, m)
            co.upload(0, self.packed)
            if key == "gt2_opt":
                co.optimize()
        elif key in ("gt2x", "gt2x_kept"):
            co = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
            co.upload(0, self.packed)
            if key == "gt2x_kept":
                co.keep_tallies()
        elif key == "gt2x_row0":   # 128 other rows first: the definition's rows start at cohort row 128
            co = capi.Cohort(n, 128 + m, fmt=capi.FMT_GT2X)
            co.upload(0, spc.pack(np.stack([spc.row_codes(n, 1000 + j) for j in range(128)])))
            co.upload(128, self.packed)
        elif key in ("ds32", "ds16"):
            co = capi.Cohort(n, m, fmt=capi.FMT_DS32 if key == "ds32" else capi.FMT_DS16)
            co.upload(0, self.ds_rows())
        elif key == "gt2m":
            co = capi.Cohort(n, m, fmt=capi.FMT_GT2M)
            co.convert_from(self.cohort("gt2"))
        elif key in ("gt2x_wide", "ds32_wide"):
            # the same genotypes as the kept columns of a wider cohort (tests/wide_cases.py), dropped columns adversarial
            t0 = time.time()
            wide, keep = wc.widen(self.unpacked())
            m = wide.shape[0]
            co = capi.Cohort(keep.size, m, fmt=capi.FMT_GT2X if key == "gt2x_wide" else capi.FMT_DS32)
            for r0 in range(0, m, 128):   # (superblocks of the strip layout; one block's packing in memory at a time)
                blk = wide[r0:r0 + 128]
                co.upload(r0, spc.pack(blk) if key == "gt2x_wide" else wc.ds_rows(blk, self.rie[r0:r0 + 128]))
            if n >= 70000:
                warnings.warn("wide %s cohort of %d x %d (kept %d): built in %.1f s" % (key, keep.size, m, n, time.time() - t0))
        elif key == "wide_set":   # the sample set that keeps the n columns of the wide cohorts
            co = capi.SampleSet(wc.keep_mask(n))
            assert co.n_kept == n
        self.cohorts[key] = co
        return co

    def unpacked(self):
        """[rows of self.packed, n] 2-bit codes"""
        if getattr(self, "_unpacked", None) is None:
            self._unpacked = er.unpack(self.packed, self.n)
        return self._unpacked

    def ds_rows(self):
        """FORMAT/DS holds the ALT dosage: 2 - dosage where the effect allele is REF"""
        dos = spc.dosages(self.codes)
        return np.where(self.rie[:, None] == 1, 2.0 - dos, dos).astype(np.float32)

    def oracle(self, name):
        if name not in self.ref:
            d = spc.definition(name, self.m)
            scores, stats, nloci = refcpu.score_packed(self.packed, self.n, d["kind"], d["rie"], d["beta"], d["eaf"],
                                                       refcpu.make_params(**d["params"]), d["offset"])
            self.ref[name] = (d, scores, [tuple(s) for s in stats], nloci)
        return self.ref[name]

    def close(self):
        for co in self.cohorts.values():
            co.close()
        self.cohorts.clear()


_DATA = {}


@pytest.fixture(scope="module")
def data():
    def get(shape):
        if shape not in _DATA:
            for other in list(_DATA):   # one large shape at a time on the device
                if other != SMALL:
                    _DATA.pop(other).close()
            _DATA[shape] = Data(*shape)
        return _DATA[shape]
    yield get
    for v in _DATA.values():
        v.close()
    _DATA.clear()


def descs(d):
    return capi.row_descs(d["beta"], d["eaf"], d["kind"], d["rie"])


def stream(D, d, how):
    sc = capi.Scorer(D.n, capi.make_params(**d["params"]))
    r = 0
    for j in range(d["kind"].size):
        k, rie, beta, eaf = int(d["kind"][j]), int(d["rie"][j]), float(d["beta"][j]), float(d["eaf"][j])
        if k != spc.PRESENT:
            sc.push_locus(k, rie, beta, eaf)
            continue
        row = D.packed[r]
        if how == "push_packed":
            sc.push_packed(row, rie, beta, eaf)
        elif how == "push_gt_raw":   # int8 GT vector of a BCF record
            sc.push_gt_raw(refcpu.codes_to_gt(row, D.n).astype(np.int8), 2, 1, rie, beta, eaf)
        elif how == "push_bed":
            sc.push_bed(codes_to_bed(row, D.n, r % 2), r % 2, rie, beta, eaf)
        else:
            sc.push_ds(D.ds_rows()[r], rie, beta, eaf)
        r += 1
    stats = sc.flush()
    scores, nloci = sc.finish(d["offset"])
    sc.close()
    return scores, nloci, stats


def resident(D, d, key, mode, row0=0):
    sc = capi.Scorer(D.n, capi.make_params(**d["params"]))
    sc.score_cohort(D.cohort(key), descs(d), row0, mode)
    stats = sc.flush()
    scores, nloci = sc.finish(d["offset"])
    sc.close()
    return scores, nloci, stats


def partial_sharded(D, d, key):
    """nps_partial_device of two contexts over two row shards (GT2: 8 rows | the rest; GT2X: the whole definition in
    one), summed, then nps_normalize_device"""
    import torch
    kind = d["kind"]
    present = np.cumsum(kind == spc.PRESENT)
    cut = int(np.searchsorted(present, 8, side="right")) if key == "gt2" and present[-1] > 8 else kind.size
    shards = [(0, slice(0, cut)), (int(present[cut - 1]) if cut else 0, slice(cut, kind.size))]
    total, nl, scs = None, 0, []
    for row0, sl in shards:
        dd = dict(d, kind=kind[sl], rie=d["rie"][sl], beta=d["beta"][sl], eaf=d["eaf"][sl])
        if dd["kind"].size == 0:
            continue
        sc = capi.Scorer(D.n, capi.make_params(**d["params"]))
        sc.score_cohort(D.cohort(key), descs(dd), row0, capi.MODE_AUTO)
        part = torch.empty(D.n, dtype=torch.float64, device="cuda")
        nl += sc.partial_device(part.data_ptr())
        total = part if total is None else total + part
        scs.append(sc)
    # the sum of the shards is torch's work on torch's stream; a context's stream does not wait for it
    # (hipStreamNonBlocking): without this the normalisation can run first and the sum then overwrites it
    torch.cuda.synchronize()
    scs[0].normalize_device(total.data_ptr(), nl, d["offset"])
    torch.cuda.synchronize()
    out = total.cpu().numpy()
    for sc in scs:
        sc.close()
    return out, nl, None


def subset(D, d, key):
    """nps_score_cohort_def_subset over the wide cohort with the set that keeps exactly D's samples: N = n_kept = D.n in
    every decision, the layout that of n_total samples -- the oracle's result on D as it stands"""
    co, sset = D.cohort(key), D.cohort("wide_set")
    sc = capi.Scorer(co.n_samples, capi.make_params(**d["params"]))
    sd = capi.ScoreDef(descs(d))
    try:
        sc.score_cohort_def_subset(co, sd, sset)
        stats = sc.flush()
        scores, nloci = sc.finish_subset(sset, d["offset"])
    finally:
        sc.close()
        sd.close()
    assert scores.shape == (D.n,)
    return scores, nloci, stats


def decoy(d):
    """a second definition for a multi-score pass: other betas (finite, within a factor of two), a finite eaf, the case's
    kinds and effect alleles, every seventh row not listed"""
    j = np.arange(d["kind"].size)
    out = capi.row_descs(np.where(j % 2 == 0, 0.02, -0.03) * (1.0 + (j % 5) / 8.0), np.full(j.size, 0.25), d["kind"], d["rie"])
    out["kind"][j % 7 == 3] = capi.ROW_NOT_IN_SCORE
    return out


def positional(D, d, key):
    """a cohort of one row per descriptor for the multi-score paths (position j is cohort row j): D's rows at the PRESENT
    positions, dosage 2 at every sample of the rows without data -- no score may read those.  The caller closes it."""
    rows, present = d["kind"].size, d["kind"] == spc.PRESENT
    codes = np.full((rows, D.n), 3, np.uint8)
    codes[present] = D.unpacked()[: int(present.sum())]
    if key == "gt2m":
        plain = capi.Cohort(D.n, rows)
        plain.upload(0, spc.pack(codes))
        co = capi.Cohort(D.n, rows, fmt=capi.FMT_GT2M)
        co.convert_from(plain)
        plain.close()
    else:
        co = capi.Cohort(D.n, rows, fmt=capi.FMT_DS32 if key == "ds32" else capi.FMT_DS16)
        co.upload(0, dc.ds_rows(codes, d["rie"]))
    return co


def multi(D, d, key):
    """nps_score_cohort_multi of two definitions -- the case's and decoy(d) -- over the NPS_FMT_GT2M, NPS_FMT_DS32 or
    NPS_FMT_DS16 cohort; the scores of definition 0.  On a dosage cohort the pass's row tallies of the PRESENT rows are
    asserted here: nmissing the count of code 2, sum (sum_flipped where the effect allele is REF) the effect-allele count
    of tallyAlleles, bit for bit -- integers, so the float64 sums are exact."""
    rows, present = d["kind"].size, d["kind"] == spc.PRESENT
    mdef = capi.MultiDef(np.stack([descs(d), decoy(d)]))   # (a refusal of the definition comes from here)
    co = msc = None
    try:
        co = D.cohort(key) if present.all() else positional(D, d, key)
        msc = capi.MultiScorer(D.n, capi.make_params(**d["params"]), 2)
        if key != "gt2m":
            chunks, per = msc.geometry(rows, co.fmt)
            assert chunks * per >= rows > (chunks - 1) * per
            # (a row chunk is at least 16 rows long: the definitions of special_cases are one chunk, added in the
            # reference's order, so a sum overflows where the reference's does)
            assert chunks == 1 or rows > 16
        msc.score_cohort(co, mdef)
        got, nloci = msc.finish([d["offset"], -0.25])
        got = got[0].copy()
        if key != "gt2m":
            nm, sm, sf = msc.row_tallies()
            codes = D.unpacked()[: int(present.sum())]
            nmiss, neffect = dc.tallies(codes)
            assert np.array_equal(nm[present], nmiss.astype(np.uint64))
            tally = np.where(d["rie"][present] == 1, sf[present], sm[present])
            assert np.array_equal(tally.view(np.int64), neffect.astype(np.float64).view(np.int64))
    finally:
        mdef.close()
        if msc is not None:
            msc.close()
        if co is not None and not present.all():
            co.close()
    return got, int(nloci[0]), None


PATHS = {
    "push_packed": lambda D, d: stream(D, d, "push_packed"),
    "push_gt_raw": lambda D, d: stream(D, d, "push_gt_raw"),
    "push_bed": lambda D, d: stream(D, d, "push_bed"),
    "push_ds": lambda D, d: stream(D, d, "push_ds"),
    "gt2_twopass": lambda D, d: resident(D, d, "gt2", capi.MODE_TWOPASS),
    "gt2_fused": lambda D, d: resident(D, d, "gt2", capi.MODE_FUSED),
    "gt2_auto": lambda D, d: resident(D, d, "gt2", capi.MODE_AUTO),
    "gt2_optimized": lambda D, d: resident(D, d, "gt2_opt", capi.MODE_AUTO),
    "gt2x_fused": lambda D, d: resident(D, d, "gt2x", capi.MODE_FUSED),
    "gt2x_twopass": lambda D, d: resident(D, d, "gt2x", capi.MODE_TWOPASS),
    "gt2x_kept_tallies": lambda D, d: resident(D, d, "gt2x_kept", capi.MODE_AUTO),
    "gt2x_row0_128": lambda D, d: resident(D, d, "gt2x_row0", capi.MODE_AUTO, 128),
    "ds32_fused": lambda D, d: resident(D, d, "ds32", capi.MODE_FUSED),
    "ds32_twopass": lambda D, d: resident(D, d, "ds32", capi.MODE_TWOPASS),
    "ds16_fused": lambda D, d: resident(D, d, "ds16", capi.MODE_FUSED),
    "partial_shards_gt2": lambda D, d: partial_sharded(D, d, "gt2"),
    "partial_gt2x": lambda D, d: partial_sharded(D, d, "gt2x"),
    "subset_gt2x": lambda D, d: subset(D, d, "gt2x_wide"),
    "subset_ds32": lambda D, d: subset(D, d, "ds32_wide"),
    "multi_ds32": lambda D, d: multi(D, d, "ds32"),
    "multi_ds16": lambda D, d: multi(D, d, "ds16"),
}
STRIP_PATHS = ["gt2x_fused", "gt2x_twopass", "gt2x_kept_tallies"]
# The last four entries run the same matrices from tests/test_gpu_subset_multi_matrices.py, a module of their own: the
# ids and the order of the runs over the earlier paths, here and in the modules that import PATHS, stay as they were.
LATER_PATHS = ["subset_gt2x", "subset_ds32", "multi_ds32", "multi_ds16"]
EARLIER_PATHS = [p for p in PATHS if p not in LATER_PATHS]


def expected_refusal(path, d):
    """What include/nps.h says a path refuses, from the descriptors alone: (status, the first row the message names, or
    None where it names none), or None where the definition is scored.
      subset_gt2x    NPS_E_UNSUPPORTED naming the first PRESENT row that NPS_FMT_GT2X cohorts score in their IEEE pass
                     (nps_score_cohort_def_subset; the rows: nps_scoredef_create) -- a non-finite beta, an infinite eaf, a
                     non-zero beta with |beta| (4 + max(2, 2 |eaf|)) outside [2^-900, 2^1000), a NaN eaf counting as 0
      subset_ds32    any beta the two-pass kernels take: nothing
      multi_*        NPS_E_UNSUPPORTED naming the first listed row with a non-finite beta or an infinite eaf; without a row,
                     non-zero |beta| that span more than 2^25 (nps_multidef_create)
      multi_gt2m     also, naming the score: finite betas whose weight bound max|beta| (3 + max(2, 2 max|eaf|)) is not
                     finite (nps_score_cohort_multi on a NPS_FMT_GT2M cohort)"""
    kind, beta, eaf = d["kind"], d["beta"], d["eaf"]
    if path == "subset_gt2x":
        for j in np.nonzero(kind == spc.PRESENT)[0]:
            b, e = float(beta[j]), float(eaf[j])
            if not np.isfinite(b) or np.isinf(e):
                return capi.E_UNSUPPORTED, int(j)
            bound = abs(b) * (4.0 + max(2.0, 2.0 * (0.0 if np.isnan(e) else abs(e))))
            if b != 0.0 and not 2.0 ** -900 <= bound < 2.0 ** 1000:
                return capi.E_UNSUPPORTED, int(j)
    elif path.startswith("multi_"):
        for j in range(kind.size):
            if not np.isfinite(beta[j]) or np.isinf(eaf[j]):
                return capi.E_UNSUPPORTED, j
        mag = np.abs(beta[beta != 0.0])
        if mag.size and float(mag.max()) / float(mag.min()) > 2.0 ** 25:
            return capi.E_UNSUPPORTED, None
        if path == "multi_gt2m" and beta.size:
            fin = np.abs(eaf[np.isfinite(eaf)])
            if not np.isfinite(float(np.abs(beta).max()) * (3.0 + max(2.0, 2.0 * float(fin.max() if fin.size else 0.0)))):
                return capi.E_UNSUPPORTED, None
    return None


def refused(path, d, call, what):
    """where expected_refusal predicts one: run `call`, assert the refusal (status, and the row where one is named) and
    return True; else False, nothing run"""
    want = expected_refusal(path, d)
    if want is None:
        return False
    with pytest.raises(capi.NpsError) as ei:
        call()
    assert ei.value.status == want[0], "%s: %s" % (what, ei.value)
    if want[1] is not None:
        assert re.search(r"row %d\b" % want[1], str(ei.value)), "%s: row %d not named in: %s" % (what, want[1], ei.value)
    return True


def check(D, name, path):
    d, ref, ref_stats, ref_nloci = D.oracle(name)
    what = "%s on %s (%d x %d)" % (name, path, D.n, D.m)
    if refused(path, d, lambda: PATHS[path](D, d), what):
        return
    scores, nloci, stats = PATHS[path](D, d)
    assert nloci == ref_nloci, what
    if stats is not None:
        assert_stats_equal(stats, ref_stats)
    assert_scores(scores, ref, d["beta"], max(nloci, 1), what)


@pytest.mark.parametrize("name", list(spc.CASES))
@pytest.mark.parametrize("path", EARLIER_PATHS)
def test_special_definition_small(data, path, name):
    check(data(SMALL), name, path)


# (the 62-unit strips are a plan of the single-read kernel only)
STRIP_RUNS = [(s, p) for s in STRIP_SHAPES for p in STRIP_PATHS if s != (4000, 13) or p == "gt2x_fused"]
# the subset run of the strip cohort (one strip, 16 row teams; tests/test_gpu_subset_multi_matrices.py): mostly the
# refusal rule over the strip-plan case list
SUBSET_STRIP_RUNS = [((1500, 2000), "subset_gt2x")]


@pytest.mark.parametrize("name", STRIP_CASES)
@pytest.mark.parametrize("shape,path", STRIP_RUNS)
def test_special_definition_strip_plans(data, shape, path, name):
    check(data(shape), name, path)


def check_multi_gt2m(D, name):
    """NPS_FMT_GT2M, one special definition beside the decoy: a non-finite beta and an infinite eaf are refused with
    NPS_E_UNSUPPORTED naming the row, a beta span past 2^25 and a weight bound that is not finite (|beta| = DBL_MAX; the
    latter by nps_score_cohort_multi, naming the score) without one; everything else is scored on the matrix cores: NaN,
    +inf and -inf at the reference's samples, the finite samples within the bar"""
    d, ref, _, ref_nloci = D.oracle(name)
    what = name + " on multi_gt2m"
    if refused("multi_gt2m", d, lambda: multi(D, d, "gt2m"), what):
        return
    got, nloci, _ = multi(D, d, "gt2m")
    assert nloci == ref_nloci
    assert_scores(got, ref, d["beta"], max(ref_nloci, 1), what)


@pytest.mark.parametrize("name", spc.EAF_CASES)
def test_multi_score_eaf(data, name):
    """NPS_FMT_GT2M: an infinite eaf is refused with NPS_E_UNSUPPORTED naming the row; a NaN eaf is scored.  (The other
    special definitions: tests/test_gpu_subset_multi_matrices.py test_multi_score_special_definitions.)"""
    check_multi_gt2m(data(SMALL), name)


def test_multi_score_refuses_non_finite_beta(data):
    D = data(SMALL)
    for name in ("beta_pinf", "beta_nan"):
        d = D.oracle(name)[0]
        with pytest.raises(capi.NpsError) as ei:
            capi.MultiDef(descs(d)[None, :])
        assert ei.value.status == capi.E_UNSUPPORTED and "row 0" in str(ei.value)
