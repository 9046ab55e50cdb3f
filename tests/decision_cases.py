"""Score rows that sit on the two threshold decisions every row goes through before any arithmetic, shared by
tests/test_decision_cases.py (the oracle against a numpy restatement, and the fault list against the comparison) and
tests/test_gpu_decisions.py (every scoring path against the oracle).  Not a conftest.

* --maxmis: the reference drops to locus imputation when `nmissing / nsamples > maxmis` (nimpress.nim:565-571): a strict
  `>`, a float64 quotient, the true sample count.
* --mincs: the reference imputes the cohort's own frequency when `ngenotyped >= mincs` (nimpress.nim:471), else 2 eaf
  (int_ps) or NaN (int_fail).

For every threshold of a shape, t is the largest missing count that is NOT over it, found by a scan with the reference's
own expression (threshold_t); the cohort has one row with exactly k missing samples for every k in t - 1 .. t + 2.  Score
rows carry eaf = 0.05 while the genotypes are drawn at allele frequency 0.3, so the internal imputation value (about 0.6)
is far from 2 eaf = 0.1 and from the constants 0 and 2: a flipped decision moves a row's terms by a multiple of |beta|.
"""
import functools

import numpy as np

import special_cases as spc

SEED = 20261017
STRIP = 2048             # samples of a strip of the strip layout: the missing samples of a row spread over all of them
EAF = 0.05               # of every score row
AF = 0.3                 # of the genotypes
SMALL_N = (777, 4000)
STRIP_N = (4000, 70000, 300001)
LOCI = ("ps", "homref", "fail", "ignore")
PS_ON_STRIPS = ("0.05", "zero", "one", "below_one")

DECIMALS = (0.03, 0.05, 0.07, 0.1, 0.2, 0.5)
# Exact-quotient rates maxmis = fl(k0 / n): the reference's quotient EQUALS the bar at k0 missing samples, so one ulp of
# error anywhere flips the decision.  Chosen once by this scan over FAULTS (not recomputed by any test):
#   for k0 in range(1, n): r = k0 / n; t = threshold_t(n, r)       # == k0
#       killed = [f for f in FAULTS if any(FAULTS[f].over(k, n, r) != (k / n > r) for k in (t - 1, t, t + 1, t + 2))]
# `ge` dies at every k0.  The first k0 that kill `mul` (fl(fl(k0 / n) n) < k0: k0 itself comes out over), `rcp`
# (fl(k0 fl(1 / n)) > fl(k0 / n)) and `f32q` (the float32 quotient rounds up), and one count past 1 000:
#      777: mul 49, 51, 53, 98;   rcp none below 777;     f32q 1, 2, 4, 7 .. 47
#    4 000: mul 1001, 1003;       rcp 9, 13, 18, 1001;    f32q 1, 2, 3 .. 1001
#   70 000: mul 21, 42, 1002;     rcp none below 2 100;   f32q 1, 2, 3 .. 11
#  300 001: mul 13, 26, 49;       rcp 5, 9, 10, 13;       f32q 3, 6, 7
# (the decimal rates kill pad16 / pad32 / pad2048 at 777, `ge` and `f32q` at 4 000, where 0.05 n, 0.07 n, 0.1 n and 0.2 n
# are exact quotients; nextafter(1, 0) kills `f32` at every n: 1.0f is not over 1.0f)
K0 = {777: (47, 49, 98), 4000: (9, 1001), 70000: (11, 21, 1002), 300001: (5, 13)}
# t of the decimal rates, by the same scan (literals: tests/test_decision_cases.py compares them with threshold_t)
T_DECIMAL = {777: (23, 38, 54, 77, 155, 388), 4000: (120, 200, 280, 400, 800, 2000),
             70000: (2100, 3500, 4900, 7000, 14000, 35000), 300001: (9000, 15000, 21000, 30000, 60000, 150000)}
# the --mincs triple: mincs = n - K0_MINCS[n], rows with K0_MINCS[n] - 1, K0_MINCS[n], K0_MINCS[n] + 1 missing samples
# (t of --maxmis 0.05 and its neighbours) have ngenotyped = mincs + 1, mincs, mincs - 1
K0_MINCS = {777: 38, 4000: 200, 70000: 3500, 300001: 15000}


@functools.lru_cache(maxsize=None)
def threshold_t(n, r):
    """the largest k in 0 .. n with not (k / n > r), by a scan over every k with the reference's expression; -1: none"""
    with np.errstate(invalid="ignore"):
        over = np.arange(n + 1, dtype=np.float64) / np.float64(n) > np.float64(r)
    assert not (over[:-1] & ~over[1:]).any()   # monotone
    return int(np.count_nonzero(~over)) - 1


def thresholds(n, reduced=False):
    """label -> --maxmis of shape n (reduced: the strip-plan list; "large": the shorter one of the two large cohorts,
    where the oracle's own pass over the cohort is most of a case's time)"""
    out = {"%g" % r: r for r in (DECIMALS if reduced != "large" else (0.05,))}
    for k0 in K0[n][:2] if reduced == "large" else K0[n]:
        out["q%d" % k0] = float(k0) / float(n)
    out.update({"one": 1.0, "below_one": float(np.nextafter(1.0, 0.0))})
    if reduced != "large":
        out["zero"] = 0.0
    if not reduced:
        out.update({"neg_zero": -0.0, "denormal": 5e-324, "pinf": float("inf"), "nan": float("nan"), "minus_one": -1.0})
    return out


def row_counts(n):
    """the missing counts of the boundary rows of shape n: t - 1 .. t + 2 of every threshold, inside 0 .. n"""
    ks = set()
    for r in thresholds(n).values():
        t = threshold_t(n, r)
        ks.update(k for k in (t - 1, t, t + 1, t + 2) if 0 <= k <= n)
    return sorted(ks)


def missing_order(n, j, seed=SEED):
    """a permutation of the samples, seeded by the row: samples 0 and n - 1 first, then one sample of every strip in
    turn (the strips in a random order, a random sample of each), so that the first k of it spread over all strips"""
    rng = np.random.default_rng([seed, j])
    strips = (n + STRIP - 1) // STRIP
    grid = np.arange(strips * STRIP, dtype=np.int64).reshape(strips, STRIP)
    grid[grid >= n] = -1
    grid = rng.permuted(grid, axis=1)
    grid[-1] = np.concatenate([grid[-1][grid[-1] >= 0], grid[-1][grid[-1] < 0]])   # the ragged strip runs out early
    perm = rng.permutation(grid, axis=0).T.ravel()
    ends = [0, n - 1] if n > 1 else [0]
    return np.concatenate([np.array(ends, np.int64), perm[(perm > 0) & (perm != n - 1)]])


def boundary_codes(n, counts, seed=SEED):
    """[len(counts), n] 2-bit codes (special_cases' coding): row j has exactly counts[j] missing samples, the first
    counts[j] of missing_order(n, j); the others are drawn at allele frequency AF"""
    out = np.empty((len(counts), n), np.uint8)
    for j, k in enumerate(counts):
        rng = np.random.default_rng([seed, j, 1])
        u = rng.random(n)
        c = np.where(u < AF * AF, 3, np.where(u < AF * AF + 2 * AF * (1 - AF), 1, 0)).astype(np.uint8)
        c[missing_order(n, j, seed)[:k]] = 2
        out[j] = c
    return out


pack = spc.pack


def cycle(rows, m):
    """the rows repeated in order up to m rows: row j is rows[j % len(rows)], so with m past a multiple of 128 boundary
    rows fall at rows 0, 127, 128 and the last row of a ragged final superblock"""
    return rows[np.arange(m) % rows.shape[0]]


def ds_rows(codes, rie):
    """float32 FORMAT/DS rows of the codes: the ALT dosage (2 - dosage where REF is the effect allele), NaN = missing"""
    dos = spc.dosages(codes)
    return np.where(np.asarray(rie)[:, None] == 1, 2.0 - dos, dos).astype(np.float32)


def row_rie(m):
    return (np.arange(m) % 3 == 1).astype(np.int32)


class Table:
    """the thresholds, boundary rows and score definitions of one sample count.  Row order: the counts up to
    K0_MINCS[n] + 2 ascending (the `head`), the all-missing row, then the others ascending -- the --mincs definitions
    score the head alone (with the all-missing row where the case asks for it): under int_fail every row below --mincs
    turns its missing samples into NaN, and the rows with hundreds of missing samples would leave no finite sample to
    see a flipped row by."""

    def __init__(self, n):
        self.n = n
        ks = row_counts(n)
        head = [k for k in ks if k <= K0_MINCS[n] + 2]
        self.head = len(head)
        self.counts = head + [n] + [k for k in ks if k > K0_MINCS[n] + 2 and k != n]
        self.nb = len(self.counts)
        self.row_of = {k: j for j, k in enumerate(self.counts)}
        self._codes = None

    def codes(self):
        if self._codes is None:
            self._codes = boundary_codes(self.n, self.counts)
        return self._codes

    def specs(self, reduced=False):
        """name -> (params, betas of boundary rows {missing count: beta}, two_band, rows scored or None for all)"""
        n, out = self.n, {}
        p0 = dict(imp_locus="ps", imp_missing="homref", imp_sample="int_ps", maxmis=0.05, mincs=100)
        for label, r in thresholds(n, reduced).items():
            # (the strip-plan list: every threshold under ignore, where nloci shows the decision on every path; under ps
            # the ones whose quotient is the point)
            on_ps = label == "0.05" if reduced == "large" else label[0] == "q" or label in PS_ON_STRIPS
            for loc in (LOCI if not reduced else ("ignore", "ps") if on_ps else ("ignore",)):
                out["maxmis_%s_%s" % (label, loc)] = (dict(p0, maxmis=r, imp_locus=loc), {}, False, None)
        k0 = K0_MINCS[n]
        assert all(self.row_of[k] < self.head for k in (k0 - 1, k0, k0 + 1, 0)) and self.row_of[n] == self.head
        mincs = {"triple": n - k0} if reduced else {"triple": n - k0, "zero": 0, "minus_one": -1, "n": n, "n_plus_1": n + 1}
        for label, v in mincs.items():
            for smp in (("int_fail",) if reduced else ("int_ps", "int_fail")):
                out["mincs_%s_%s" % (label, smp)] = (dict(p0, maxmis=1.0, imp_sample=smp, mincs=v), {}, False,
                                                     self.head + (label == "zero"))
        t = threshold_t(n, 0.05)
        # the rows at t and t + 1 go through mx_special_pass on the strip paths: one definition decided by both
        # formulations in one call
        out["beta_inf_at_t"] = (dict(p0, imp_locus="ignore"), {t: spc.INF, t + 1: spc.INF}, False, None)
        out["two_band"] = (dict(p0, imp_locus="ignore"), {}, True, None)
        return out

    def definition(self, name, m=None):
        """the case's descriptors over a cohort of m rows (cohort row j holds boundary row j % nb); the --mincs cases
        score its first rows only"""
        m = self.nb if m is None else m
        params, betas, two_band, rows = self.specs()[name]
        j = np.arange(m)
        rng = np.random.default_rng(SEED + 1)
        beta = np.round(rng.uniform(0.01, 0.05, m), 4) * np.where(rng.random(m) < 0.5, -1.0, 1.0)
        if two_band:   # |beta| spans more than 2^30: two magnitude bands on the strip paths
            beta = np.where(j % 2 == 0, 10.0 * (1.0 + j / m), 1e-12 * (1.0 + j / m))
        for k, b in betas.items():
            beta[j % self.nb == self.row_of[k]] = b
        rows = m if rows is None else rows
        return dict(kind=np.zeros(rows, np.int32), rie=row_rie(m)[:rows], beta=beta.astype(np.float64)[:rows],
                    eaf=np.full(rows, EAF), params=params, offset=0.125)

    def row_missing(self, d):
        """the missing count of every row the definition scores"""
        return np.array(self.counts)[np.arange(d["kind"].size) % self.nb]


_TABLES = {}


def table(n):
    if n not in _TABLES:
        _TABLES[n] = Table(n)
    return _TABLES[n]


# ---- the two decisions, and the ways to get them wrong
class Decide:
    """the reference's decisions (k missing of n samples)"""

    def over(self, k, n, r):          # nimpress.nim:565
        return float(k) / float(n) > r

    def tally(self, j, k, neffect, n):   # row j's (nmissing, neffect) as counted; a subset run counts the kept samples
        return k, neffect

    def ngen(self, k, n):
        return n - k

    def enough(self, k, n, mincs):    # nimpress.nim:471
        return float(self.ngen(k, n)) >= float(mincs)


def _fault(**methods):
    return type("Fault", (Decide,), methods)()


def _pad(n, p):
    return (n + p - 1) // p * p


def _f32(x):
    with np.errstate(over="ignore", under="ignore"):
        return np.float32(x)


EXACT = Decide()
FAULTS = {
    "ge": _fault(over=lambda s, k, n, r: float(k) / float(n) >= r),
    "mul": _fault(over=lambda s, k, n, r: float(k) > r * float(n)),
    "rcp": _fault(over=lambda s, k, n, r: float(k) * (1.0 / float(n)) > r),
    "f32": _fault(over=lambda s, k, n, r: bool(_f32(k) / _f32(n) > _f32(r))),
    "f32q": _fault(over=lambda s, k, n, r: float(_f32(k) / _f32(n)) > r),
    "pad16": _fault(over=lambda s, k, n, r: float(k) / float(_pad(n, 16)) > r),
    "pad32": _fault(over=lambda s, k, n, r: float(k) / float(_pad(n, 32)) > r),
    "pad2048": _fault(over=lambda s, k, n, r: float(k) / float(_pad(n, 2048)) > r),
    "t_plus_1": _fault(over=lambda s, k, n, r: k > threshold_t(n, r) + 1),
    "t_minus_1": _fault(over=lambda s, k, n, r: k > threshold_t(n, r) - 1),
    "mincs_gt": _fault(enough=lambda s, k, n, mincs: float(n - k) > float(mincs)),
    "mincs_vs_n": _fault(enough=lambda s, k, n, mincs: float(n) >= float(mincs)),
    "ngen_padded": _fault(ngen=lambda s, k, n: _pad(n, 16) - k),
}


def _n_total(n):
    import wide_cases
    return wide_cases.n_total(n)


def _leak(s, j, k, neffect, n):
    """the tallies of row j taken over the wide matrix of wide_cases.widen: its dropped columns are missing in the even
    rows and hold dosage 2 in the odd ones"""
    extra = _n_total(n) - n
    return (k + extra, neffect) if j % 2 == 0 else (k, neffect + 2.0 * extra)


# What a subset run (nps_score_cohort_def_subset) can get wrong: the sample count of the decisions is n_kept = n, that of
# the layout is n_total (tests/wide_cases.py) -- a mix-up of the two in the --maxmis quotient, in ngenotyped or in the
# --mincs test, and tallies that count dropped samples.
SUBSET_FAULTS = {
    "over_whole": _fault(over=lambda s, k, n, r: float(k) / float(_n_total(n)) > r),
    "ngen_whole": _fault(ngen=lambda s, k, n: _n_total(n) - k),
    "enough_whole": _fault(enough=lambda s, k, n, mincs: float(_n_total(n) - k) >= float(mincs)),
    "leak": _fault(tally=_leak),
}
FAULTS.update(SUBSET_FAULTS)
MINCS_FAULTS = ["mincs_gt", "mincs_vs_n", "ngen_padded", "ngen_whole", "enough_whole"]
MAXMIS_FAULTS = [f for f in FAULTS if f not in MINCS_FAULTS]

REASON_GENOTYPED, REASON_MAXMIS = 0, 4   # include/nps.h, oracle/refcpu.py REASON_NAMES


def tallies(codes):
    """per row (nmissing, neffect) as tallyAlleles counts them (nimpress.nim:32-47)"""
    return (codes == 2).sum(axis=1), (codes == 1).sum(axis=1) + 2 * (codes == 3).sum(axis=1)


def decisions(n, nmissing, d, decide=None):
    """(used, reason) of every row and nloci, from the rows' missing counts alone (every row is genotyped)"""
    decide, p = decide or EXACT, d["params"]
    over = np.array([decide.over(int(k), n, p["maxmis"]) for k in nmissing])
    used = np.where(over & (p["imp_locus"] == "ignore"), 0, 1).astype(np.int32)
    return used, np.where(over, REASON_MAXMIS, REASON_GENOTYPED).astype(np.int32), int(used.sum())


def reference(codes, d, decide=None):
    """the reference's row loop (nimpress.nim:626-649 with getImputedDosages :484-585) in numpy float64, rows in score
    order, one product then `+=`, then `/ (2 nloci)` and `+ offset` -- the order of
    tests/test_oracle_special_values.py restated_scores -- with the two decisions taken by `decide` (None: the
    reference's own).  Every row of d is a genotyped row, row j of the codes.  Returns scores, stats (oracle/refcpu.py STAT_DTYPE) and
    nloci."""
    from oracle.refcpu import STAT_DTYPE
    decide, p, n = decide or EXACT, d["params"], codes.shape[1]
    assert (d["kind"] == spc.PRESENT).all() and d["kind"].size <= codes.shape[0]
    scores, nloci = np.zeros(n), 0
    stats = np.zeros(d["kind"].size, STAT_DTYPE)
    for j in range(d["kind"].size):
        rie, beta, eaf = bool(d["rie"][j]), d["beta"][j], d["eaf"][j]
        dos = spc.dosages(codes[j])
        miss = np.isnan(dos)
        k, neffect = decide.tally(j, int(miss.sum()), float(np.sum(dos[~miss])), n)
        ngen = decide.ngen(k, n)
        used, reason = 1, REASON_GENOTYPED
        if decide.over(k, n, p["maxmis"]):             # :565-571
            reason = REASON_MAXMIS
            if p["imp_locus"] == "ignore":
                used = 0
            else:                                      # imputeLocusDosages :417-447
                dos = np.full(n, {"ps": eaf * 2.0, "homref": 2.0 if rie else 0.0, "fail": np.nan}[p["imp_locus"]])
        else:                                          # imputeSampleDosages :450-481
            s = p["imp_sample"]
            if s == "ps":
                v = eaf * 2.0
            elif s == "homref":
                v = 2.0 if rie else 0.0
            elif s == "fail":
                v = np.nan
            elif decide.enough(k, n, p["mincs"]):
                with np.errstate(invalid="ignore", divide="ignore"):
                    v = np.float64(neffect) / np.float64(ngen)
            else:
                v = eaf * 2.0 if s == "int_ps" else np.nan
            dos = np.where(miss, v, dos)
        stats[j] = (ngen, k, neffect, used, reason)
        if not used:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            scores += dos * beta                       # :639-641
        nloci += 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        scores = scores / (float(nloci) * 2.0)         # :643-645
        scores = scores + d["offset"]                  # :647-649
    return scores, stats, nloci


def compare(scores, nloci, stats, ref, ref_stats, ref_nloci, beta, what=""):
    """what tests/test_gpu_decisions.py asks of a path: nloci equal, the row statistics bit for bit where the path
    returns them, the scores within tests/score_compare.py's bar"""
    from score_compare import assert_scores
    from test_gpu_parity import assert_stats_equal
    assert nloci == ref_nloci, "%s: nloci %d, reference %d" % (what, nloci, ref_nloci)
    if stats is not None:
        assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    assert_scores(scores, ref, beta, max(nloci, 1), what)
