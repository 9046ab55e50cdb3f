"""The sixteen score rows of the AF-mismatch warning tests and the oracle's decisions about them.  Shared by the
end-to-end run (tests/test_gpu_cli.py, the command line on a 100 000-sample BCF) and by the CPU test of the host's
warning writer (tests/test_host_logic.py): both must log exactly `expected_warnings(...)`."""
from oracle import refcpu

CONTIG = "7"
ALT = "C"       # the one ALT allele of every record in the file

# (pos, ref, ea, eaf, ALT allele count, missing samples, FILTER, in file?) for n = 100 000 samples
ROWS = [
    (1000, "A", "C", 0.30, 60000, 0, [], True),        # exactly the expectation: p = 1
    (1100, "A", "C", 0.30, 60050, 0, ["PASS"], True),  # near the mean: betacf -> NaN -> no warning
    (1200, "A", "C", 0.30, 60600, 0, [], True),        # p = 0.0034
    (1300, "A", "C", 0.30, 60700, 0, [], True),        # p = 0.00065 -> warned
    (1400, "A", "C", 0.30, 59300, 0, [], True),        # p = 0.00063 -> warned (x below the mean)
    (1500, "A", "C", 0.30, 59400, 0, [], True),        # p = 0.0034
    (1600, "G", "C", 0.10, 40000, 0, [], True),        # far off: p = 0 -> warned
    (1700, "A", "A", 0.70, 60700, 0, [], True),        # effect allele = REF, 139 300 REF alleles: warned
    (1800, "A", "C", 0.30, 0, 0, [], False),           # absent, eaf 0.3: "cohort EAF is 0" warned
    (1900, "A", "C", 1e-7, 0, 0, [], False),           # absent, eaf 1e-7: p = 1
    (2000, "A", "C", float("nan"), 90000, 0, [], True),  # eaf NaN: no test
    (2100, "A", "C", 0.30, 10000, 10000, [], True),    # 10 % missing: over --maxmis, no AF test
    (2200, "A", "C", 0.30, 60120, 1000, [], True),     # 1 % missing: 198 000 trials, p = 0.00042 -> warned
    (2300, "A", "C", 0.30, 60000, 1000, [], True),     # 1 % missing: p = 0.0033
    (2400, "A", "C", 0.30, 10000, 0, ["FAIL"], True),  # FILTER: locus-imputed, no AF test
    (2500, "A", "G", 0.30, 60700, 0, [], True),        # ea not among the ALT alleles -> absent -> warned
]

# nps_row_kind (include/nps.h): what getImputedDosages decides before it looks at a genotype
ROW_PRESENT, ROW_UNCOVERED, ROW_ABSENT, ROW_FILTERED = 0, 1, 2, 3


def row_state(row, n):
    """(kind, nmissing, neffect) of one row: findVariant / FILTER (nim:536-558), then tallyAlleles' counts"""
    pos, ref, ea, eaf, x, nmiss, filt, present = row
    if not present or (ea != ref and ea != ALT):           # findVariant returns nil (nim:536-541)
        return ROW_ABSENT, 0, 0
    if filt == ["FAIL"]:
        return ROW_FILTERED, 0, 0
    return ROW_PRESENT, nmiss, (2 * (n - nmiss) - x) if ea == ref else x   # tallyAlleles counts the EFFECT allele


def expected_warnings(rows, n, afmisp=0.001, maxmis=0.05):
    """the oracle's decisions and texts, in score-file order (nimpress.nim:537-541, 554-557, 565-579; the literal
    O(n) binomTest): (the warning texts, the number of NaN p-values among the genotyped rows' tests)"""
    fmt = refcpu.format_score
    expected, n_nan = [], 0
    for row in rows:
        pos, ref, ea, eaf = row[:4]
        var = "%s:%d:%s:%s" % (CONTIG, pos, ref, ea)
        kind, nmiss, neff = row_state(row, n)
        if kind == ROW_ABSENT:
            if eaf == eaf and refcpu.binom_test(0, 2 * n, eaf) < afmisp:
                expected.append("Variant %s cohort EAF is 0 in %d samples.  This is highly unlikely given "
                                "polygenic score EAF of %s" % (var, n, fmt(eaf)))
            continue
        if kind == ROW_FILTERED:
            expected.append('Variant %s has a FILTER flag set (value "FAIL").  Imputing all dosages at this locus.' % var)
            continue
        if nmiss / n > maxmis:
            expected.append("Locus %s:%d-%d has %s%% of samples missing a genotype. This exceeds the missingness "
                            "threshold; imputing all dosages at this locus." % (CONTIG, pos, pos, fmt(nmiss / n * 100)))
            continue
        nobs = (n - nmiss) * 2
        if eaf == eaf:
            p = refcpu.binom_test(neff, nobs, eaf)
            n_nan += int(p != p)
            if p < afmisp:
                expected.append("Variant %s cohort EAF is %s in %d samples.  This is highly unlikely given "
                                "polygenic score EAF of %s" % (var, fmt(neff / nobs), n, fmt(eaf)))
    return expected, n_nan
