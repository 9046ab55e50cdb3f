"""Score definitions with IEEE special values (+-inf, NaN, signed zeros, subnormal and near-overflow betas) over explicit
genotypes, shared by tests/test_oracle_special_values.py (the oracle against a numpy restatement of the reference's row
loop) and tests/test_gpu_special_values.py (every scoring path against the oracle).  Not a conftest.

Genotype rows (2-bit codes: 0 = dosage 0, 1 = dosage 1, 3 = dosage 2, 2 = missing; 16 samples per uint32, low bits first).
Every ordinary row j has samples 0, 1, 2 at hom-ref, het, hom-alt, sample 3 + j missing (none of the others is missing
at samples 0 .. 3) and about 1 in 64 other samples missing; the rows
with a role are ROW_A and ROW_B (ordinary, the rows that get a special beta or eaf), ROW_ALLREF (every sample
hom-ref), ROW_NOMISS (no missing sample), ROW_OVER (about 30 % missing: over --maxmis 0.05) and ROW_ALLMISS (every sample
missing); the rows after them are ordinary.
"""
import sys

import numpy as np

ROW_A, ROW_B, ROW_ALLREF, ROW_NOMISS, ROW_OVER, ROW_ALLMISS = 0, 1, 2, 3, 4, 5
N_ROLES = 6
# kinds and imputation names as in include/nps.h / oracle/refcpu.py
PRESENT, UNCOVERED, ABSENT, FILTERED = 0, 1, 2, 3
INF, NAN, DBL_MAX = float("inf"), float("nan"), sys.float_info.max


def row_codes(n, j):
    """the codes of row j over n samples (uint8, one per sample)"""
    i = np.arange(n, dtype=np.uint64)
    h = ((i * np.uint64(2654435761) + np.uint64(j) * np.uint64(40503) + np.uint64(12345)) * np.uint64(2246822519)) \
        % np.uint64(1 << 32)
    h = (h >> np.uint64(7)).astype(np.int64)
    c = np.array([0, 1, 3], dtype=np.uint8)[h % 3]
    if j == ROW_ALLREF:
        return np.zeros(n, np.uint8)
    if j == ROW_ALLMISS:
        return np.full(n, 2, np.uint8)
    if j == ROW_OVER:
        c[(h >> 3) % 10 < 3] = 2           # ~30 % missing: over --maxmis 0.05, under 1.0
    elif j != ROW_NOMISS:
        c[(h >> 3) % 64 == 0] = 2
    known = np.array([0, 1, 3, 1], np.uint8)[: min(n, 4)]
    c[: known.size] = known
    if j != ROW_NOMISS and 3 + j < n:
        c[3 + j] = 2   # (sample 3 is missing in ROW_A only, sample 3 + j in row j)
    return c


def pack(codes):
    """[rows, n] codes -> [rows, ceil(n/16)] uint32"""
    rows, n = codes.shape
    w = (n + 15) // 16
    pad = np.zeros((rows, w * 16), np.uint32)
    pad[:, :n] = codes
    sh = (np.arange(16, dtype=np.uint32) * 2)[None, None, :]
    return np.bitwise_or.reduce(pad.reshape(rows, w, 16) << sh, axis=2).astype(np.uint32)


def base_codes(n, m):
    return np.stack([row_codes(n, j) for j in range(m)]) if m else np.zeros((0, n), np.uint8)


def dosages(codes):
    """codes -> effect-allele dosages, NaN = missing"""
    return np.array([0.0, 1.0, np.nan, 2.0])[codes]


P0 = dict(imp_locus="ps", imp_missing="homref", imp_sample="int_ps", maxmis=0.05, mincs=100)


def _p(**kw):
    d = dict(P0)
    d.update(kw)
    return d


# name -> (params, {row: beta}, {row: eaf}, host rows [(position among the descriptors, kind, rie, beta, eaf)],
#          offset, magnitude of the whole definition or None, banded)
CASES = {
    "beta_pinf": (P0, {ROW_A: INF}, {}, [], 0.0, None, False),
    "beta_ninf": (P0, {ROW_A: -INF}, {}, [], 0.0, None, False),
    "beta_nan": (P0, {ROW_A: NAN}, {}, [], 0.0, None, False),
    "beta_pinf_ninf": (P0, {ROW_A: INF, ROW_B: -INF}, {}, [], 0.0, None, False),
    "beta_inf_maxmis_ps": (P0, {ROW_OVER: -INF}, {}, [], 0.0, None, False),
    "beta_inf_maxmis_homref": (_p(imp_locus="homref"), {ROW_OVER: INF}, {}, [], 0.0, None, False),
    "beta_inf_maxmis_ignore": (_p(imp_locus="ignore"), {ROW_OVER: INF}, {}, [], 0.0, None, False),
    "beta_inf_absent": (P0, {}, {}, [(1, ABSENT, 0, INF, 0.2)], 0.0, None, False),
    "beta_inf_absent_ignored": (_p(imp_missing="ignore"), {}, {}, [(1, ABSENT, 0, INF, 0.2)], 0.0, None, False),
    "beta_inf_uncovered": (P0, {}, {}, [(3, UNCOVERED, 0, -INF, 0.3)], 0.0, None, False),
    "beta_inf_filtered": (_p(imp_locus="homref"), {}, {}, [(0, FILTERED, 1, INF, 0.3)], 0.0, None, False),
    "eaf_nan_sample_ps": (_p(imp_sample="ps", maxmis=1.0), {}, {ROW_A: NAN}, [], 0.0, None, False),
    "eaf_pinf_sample_ps": (_p(imp_sample="ps", maxmis=1.0), {}, {ROW_A: INF}, [], 0.0, None, False),
    "eaf_ninf_sample_ps": (_p(imp_sample="ps", maxmis=1.0), {}, {ROW_A: -INF}, [], 0.0, None, False),
    "eaf_nan_int_ps_fallback": (_p(maxmis=1.0, mincs=10 ** 9), {}, {ROW_A: NAN}, [], 0.0, None, False),
    "eaf_pinf_int_ps_fallback": (_p(maxmis=1.0, mincs=10 ** 9), {}, {ROW_A: INF}, [], 0.0, None, False),
    "eaf_ninf_int_ps_fallback": (_p(maxmis=1.0, mincs=10 ** 9), {}, {ROW_A: -INF}, [], 0.0, None, False),
    "eaf_nan_locus_ps": (P0, {}, {ROW_OVER: NAN}, [], 0.0, None, False),
    "eaf_pinf_locus_ps": (P0, {}, {ROW_OVER: INF}, [], 0.0, None, False),
    "eaf_ninf_locus_ps": (P0, {}, {ROW_OVER: -INF}, [], 0.0, None, False),
    "beta_pzero_fail": (_p(imp_sample="fail"), {ROW_A: 0.0}, {}, [], 0.0, None, False),
    "beta_nzero_fail": (_p(imp_sample="fail"), {ROW_A: -0.0}, {}, [], 0.0, None, False),
    "beta_pzero_int_fail": (_p(imp_sample="int_fail", mincs=10 ** 9), {ROW_A: 0.0}, {}, [], 0.0, None, False),
    "beta_nzero_int_fail": (_p(imp_sample="int_fail", mincs=10 ** 9), {ROW_A: -0.0}, {}, [], 0.0, None,
                            False),
    "all_missing_row_int_ps": (_p(maxmis=1.0, mincs=0), {}, {}, [], 0.0, None, False),
    # --maxmis below zero: every row is over it (nmissing / N > maxmis), --imputelocus ignore drops them all: nloci = 0
    "every_row_dropped": (_p(imp_locus="ignore", imp_missing="ignore", maxmis=-1.0), {}, {},
                          [(2, ABSENT, 0, 0.5, 0.2)], 0.0, None, False),
    "offset_pinf": (P0, {}, {}, [], INF, None, False),
    "offset_ninf": (P0, {}, {}, [], -INF, None, False),
    "offset_nan": (P0, {}, {}, [], NAN, None, False),
    "magnitude_1e-300": (P0, {}, {}, [], 0.0, 1e-300, False),
    "magnitude_subnormal": (P0, {}, {}, [], 0.0, 4.9e-324, False),
    "magnitude_1e300": (P0, {}, {}, [], 0.0, 1e300, False),
    "magnitude_1e307": (P0, {}, {}, [], 0.0, 1e307, False),
    "magnitude_dbl_max": (P0, {}, {}, [], 0.0, DBL_MAX, False),
    "banded_inf_row": (P0, {ROW_A: INF}, {}, [], 0.0, None, True),
    "banded_inf_row_dropped": (_p(imp_locus="ignore"), {ROW_OVER: INF}, {}, [], 0.0, None, True),
}
EAF_CASES = [k for k in CASES if k.startswith("eaf_")]


def definition(name, m):
    """the case's descriptors over m cohort rows: kind, ref_is_effect, beta, eaf (host rows inserted), params, offset"""
    params, betas, eafs, host, offset, mag, banded = CASES[name]
    rng = np.random.default_rng(20261016)
    beta = np.round(rng.normal(0.0, 0.02, m), 4)
    eaf = np.round(rng.uniform(0.01, 0.5, m), 4)
    rie = (np.arange(m) % 5 == ROW_OVER).astype(np.int32)   # (the over-maxmis row has ref = effect: homref imputes 2)
    if mag is not None:
        j = np.arange(m)
        if mag >= 1e306:   # one sign: where the reference overflows, it does so in any order of the same terms
            beta = np.full(m, mag) if mag == DBL_MAX else mag * (1.0 + (j % 16) / 64.0)
        elif mag < 1e-320:
            beta = np.where(j % 3 == 1, -mag, mag)
        else:
            beta = np.where(j % 3 == 1, -1.0, 1.0) * mag * (1.0 + (j % 16) / 16.0)
    if banded:   # |beta| spans 10 .. 1e-12: magnitude bands on the strip path
        j = np.arange(m)
        beta = np.where(j % 2 == 0, 10.0 * (1.0 + j / m), 1e-12 * (1.0 + j / m))
    for r, b in betas.items():
        if r < m:
            beta[r] = b
    for r, e in eafs.items():
        if r < m:
            eaf[r] = e
    kind = np.zeros(m, np.int32)
    for pos, k, ri, b, e in sorted(host, key=lambda h: -h[0]):
        pos = min(pos, m)
        kind = np.insert(kind, pos, k)
        rie = np.insert(rie, pos, ri)
        beta = np.insert(beta, pos, b)
        eaf = np.insert(eaf, pos, e)
    return dict(kind=kind, rie=rie.astype(np.int32), beta=beta.astype(np.float64), eaf=eaf.astype(np.float64),
                params=params, offset=offset)
