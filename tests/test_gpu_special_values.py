"""IEEE special values on every scoring path that takes a single-score definition, against the oracle.

The definitions (tests/special_cases.py) put +-inf and NaN betas, +-inf and NaN eafs, signed zero betas, infinite and NaN
offsets, whole definitions at |beta| = 1e-300, 4.9e-324, 1e300, 1e307 and DBL_MAX, and banded definitions with an infinite
row on explicit genotypes (hom-ref, het, hom-alt and missing samples at known positions, an all-hom-ref row, a row without a
missing sample, a row over --maxmis, a fully missing row).  The reference accumulates in plain float64, so every path must
give its NaN, +inf and -inf at the same samples and its finite samples within the usual bar (tests/score_compare.py), and
row statistics bit for bit.  The multi-score path refuses an infinite eaf (as it refuses a non-finite beta) and scores a NaN
eaf.  tests/test_oracle_special_values.py vouches for the oracle on exactly these definitions.
"""
import numpy as np
import pytest

import special_cases as spc
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
        self.cohorts[key] = co
        return co

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
}
STRIP_PATHS = ["gt2x_fused", "gt2x_twopass", "gt2x_kept_tallies"]


def check(D, name, path):
    d, ref, ref_stats, ref_nloci = D.oracle(name)
    scores, nloci, stats = PATHS[path](D, d)
    what = "%s on %s (%d x %d)" % (name, path, D.n, D.m)
    assert nloci == ref_nloci, what
    if stats is not None:
        assert_stats_equal(stats, ref_stats)
    assert_scores(scores, ref, d["beta"], max(nloci, 1), what)


@pytest.mark.parametrize("name", list(spc.CASES))
@pytest.mark.parametrize("path", list(PATHS))
def test_special_definition_small(data, path, name):
    check(data(SMALL), name, path)


# (the 62-unit strips are a plan of the single-read kernel only)
STRIP_RUNS = [(s, p) for s in STRIP_SHAPES for p in STRIP_PATHS if s != (4000, 13) or p == "gt2x_fused"]


@pytest.mark.parametrize("name", STRIP_CASES)
@pytest.mark.parametrize("shape,path", STRIP_RUNS)
def test_special_definition_strip_plans(data, shape, path, name):
    check(data(shape), name, path)


@pytest.mark.parametrize("name", spc.EAF_CASES)
def test_multi_score_eaf(data, name):
    """NPS_FMT_GT2M: an infinite eaf is refused with NPS_E_UNSUPPORTED naming the row; a NaN eaf is scored"""
    D = data(SMALL)
    d, ref, _, ref_nloci = D.oracle(name)
    rows = descs(d)[None, :]
    if np.isinf(d["eaf"]).any():
        with pytest.raises(capi.NpsError) as ei:
            capi.MultiDef(rows)
        assert ei.value.status == capi.E_UNSUPPORTED and "row %d" % int(np.nonzero(np.isinf(d["eaf"]))[0][0]) in str(ei.value)
        return
    msc = capi.MultiScorer(D.n, capi.make_params(**d["params"]), 1)
    mdef = capi.MultiDef(rows)
    msc.score_cohort(D.cohort("gt2m"), mdef)
    got, nloci = msc.finish([d["offset"]])
    msc.close()
    mdef.close()
    assert int(nloci[0]) == ref_nloci
    assert_scores(got[0], ref, d["beta"], max(ref_nloci, 1), name + " on multi")


def test_multi_score_refuses_non_finite_beta(data):
    D = data(SMALL)
    for name in ("beta_pinf", "beta_nan"):
        d = D.oracle(name)[0]
        with pytest.raises(capi.NpsError) as ei:
            capi.MultiDef(descs(d)[None, :])
        assert ei.value.status == capi.E_UNSUPPORTED and "row 0" in str(ei.value)
