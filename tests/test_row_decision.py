"""The per-row decisions every scoring path shares (nimpress_amd/csrc/nps_row_decision.h), without a GPU.
tests/native/decision_driver.cpp includes that header alone and is compiled with plain g++; the kernels and the host's
no-data rows call the same functions (ds_fused_kernel alone keeps a copy: DESIGN.md 1.2), so what is pinned here is
the rule itself, and the GPU suites (tests/test_gpu_decisions.py and the others) pin every path to the oracle.

* maxmis_threshold equals the scan decision_cases.threshold_t, and over_maxmis(k) == (k > maxmis_threshold): the two
  spellings of `nmissing / nsamples > --maxmis` the kernels use are one decision.
* decide_row gives the oracle's used / reason for every case of the boundary table, by either spelling.
* RowDecision.imp is, bit for bit, the dosage the oracle scores: a single row at beta = 1.0 and offset 0 comes out of
  the reference's loop as dosage x 1.0 / (2 x 1) + 0 = dosage / 2, and halving is exact, so twice the score IS the dosage.
* no_data_row gives the oracle's used / reason / dosage for ABSENT, UNCOVERED and FILTERED rows.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import decision_cases as dc
import special_cases as spc
from oracle import refcpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUIET_NAN = 0x7ff8000000000000
ALL_N = sorted(set(dc.SMALL_N + dc.STRIP_N))
REASONS = {spc.UNCOVERED: 1, spc.ABSENT: 2, spc.FILTERED: 3}   # nps_reason of a row kind, include/nps.h


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("decision") / "decision_driver")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", "-I", os.path.join(ROOT, "nimpress_amd", "csrc"),
                        "-o", exe, os.path.join(ROOT, "tests", "native", "decision_driver.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert not r.stderr.strip(), r.stderr[-2000:]   # -Wall -Wextra clean

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [a.split() for a in answers]
    return ask


def hx(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def prm(p):
    """<prm> of a decision_cases / special_cases parameter dict"""
    return "%d %d %d %s %d" % (refcpu.LOCUS[p["imp_locus"]], refcpu.MISSING[p["imp_missing"]], refcpu.SAMPLE[p["imp_sample"]],
                               hx(p["maxmis"]), p["mincs"])


def boundary_ks(n, r):
    t = dc.threshold_t(n, r)
    return [k for k in (t - 1, t, t + 1, t + 2) if 0 <= k <= n]


@pytest.mark.parametrize("n", ALL_N)
def test_maxmis_threshold_is_the_scan(driver, n):
    th = dc.thresholds(n)
    assert {"neg_zero", "denormal", "pinf", "nan", "minus_one", "below_one"} <= set(th) and all("q%d" % k in th for k in dc.K0[n])
    got = driver(["thr %d %s" % (n, hx(r)) for r in th.values()])
    for (label, r), (t,) in zip(th.items(), got):
        assert int(t) == dc.threshold_t(n, r), (n, label)


@pytest.mark.parametrize("n", ALL_N)
def test_over_maxmis_is_the_threshold_comparison(driver, n):
    """at the boundary counts of every threshold, and at every count of the smallest shape: this equality is what lets
    some kernels compare integers and the others divide"""
    q = [(k, r) for r in dc.thresholds(n).values() for k in (range(n + 1) if n == 777 else boundary_ks(n, r))]
    over = driver(["over %d %d %s" % (k, n, hx(r)) for k, r in q])
    thr = driver(["thr %d %s" % (n, hx(r)) for _, r in q])
    for (k, r), (o,), (t,) in zip(q, over, thr):
        assert int(o) == int(k > int(t)) == int(dc.EXACT.over(k, n, r)), (n, k, r)


_ORACLE = {}


def oracle_stats(n, name):
    """the oracle's row statistics of a case of the boundary table (as tests/test_decision_cases.py scores it)"""
    if (n, name) not in _ORACLE:
        T = dc.table(n)
        d = T.definition(name)
        packed = dc.pack(T.codes())
        _ORACLE[(n, name)] = refcpu.score_packed(packed[: d["kind"].size], n, d["kind"], d["rie"], d["beta"], d["eaf"],
                                                 refcpu.make_params(**d["params"]), d["offset"])[1]
    return _ORACLE[(n, name)]


@pytest.mark.parametrize("spelling", [0, 1], ids=["division", "threshold"])
@pytest.mark.parametrize("n", dc.SMALL_N)
def test_decide_row_against_the_oracle(driver, n, spelling):
    T = dc.table(n)
    nmiss, neff = dc.tallies(T.codes())
    assert len(T.specs()) >= 60
    for name in T.specs():
        d = T.definition(name)
        m = d["kind"].size
        got = driver(["row %s %d %d %d %s %s %d" % (prm(d["params"]), spelling, n, nmiss[j], hx(neff[j]), hx(d["eaf"][j]), d["rie"][j])
                      for j in range(m)])
        used = np.array([int(g[0]) for g in got])
        reason = np.array([int(g[1]) for g in got])
        want = oracle_stats(n, name)
        assert np.array_equal(used, want["used"]) and np.array_equal(reason, want["reason"]), (n, name)
        dec_used, dec_reason, _ = dc.decisions(n, T.row_missing(d), d)
        assert np.array_equal(used, dec_used) and np.array_equal(reason, dec_reason), (n, name)
        # row_stat: the record the kernels store
        for j, g in enumerate(got):
            assert (float(g[4]), float(g[5]), int(g[7]), int(g[8])) == (want["ngenotyped"][j], want["nmissing"][j], want["used"][j],
                                                                       want["reason"][j]), (n, name, j)
            assert g[6] == hx(want["neffect"][j]), (n, name, j)
            assert int(g[2]) == (1 if reason[j] == dc.REASON_GENOTYPED else 2 if used[j] else 0), (n, name, j)


def score_one(n, packed_row, kind, rie, eaf, p):
    return refcpu.score_packed(packed_row, n, [kind], [rie], [1.0], [eaf], refcpu.make_params(**p), 0.0)


def assert_dosage(scores, imp_hex, what, spelled=True):
    """twice every score is the dosage, bit for bit.  NaN: every score is NaN, and the header's is the quiet NaN wherever
    the rule spells it (spelled = False: the quotient 0 / 0 of an all-missing row, whose sign the hardware chooses)"""
    imp = struct.unpack("<d", struct.pack("<Q", int(imp_hex, 16)))[0]
    if np.isnan(imp):
        assert (int(imp_hex, 16) == QUIET_NAN or not spelled) and np.isnan(scores).all(), what
    else:
        assert scores.size and all(hx(2.0 * s) == imp_hex for s in scores), (what, imp, scores[:4])


@pytest.mark.parametrize("n", dc.SMALL_N)
def test_imp_is_the_oracles_dosage_bit_for_bit(driver, n):
    T = dc.table(n)
    codes = T.codes()
    nmiss, neff = dc.tallies(codes)
    k0 = dc.K0_MINCS[n]
    q = float(dc.K0[n][0]) / float(n)
    assert dc.threshold_t(n, 0.05) == k0 and dc.threshold_t(n, q) == dc.K0[n][0]
    # (rate, missing count): the boundary rows of one decimal rate and one exact quotient, and the all-missing row over
    # the rate (a locus constant) and under it (0 / 0, or the fall-back); under --maxmis 1 the rows around --mincs
    rows = [(r, k) for r in (0.05, q) for k in boundary_ks(n, r)] + [(0.05, n), (1.0, n)] + [(1.0, k) for k in (k0 - 1, k0, k0 + 1)]
    cases, lines = [], []
    for r, k in rows:
        j = T.row_of[k]
        assert nmiss[j] == k
        for smp in refcpu.SAMPLE:
            for loc in refcpu.LOCUS:
                for rie in (0, 1):
                    for mincs in (n - k0, 0):   # n - k0: the rows with k0 - 1, k0, k0 + 1 missing samples have ngenotyped = mincs + 1, mincs, mincs - 1
                        p = dict(imp_locus=loc, imp_missing="homref", imp_sample=smp, maxmis=r, mincs=mincs)
                        cases.append((j, k, rie, p))
                        lines.append("row %s 0 %d %d %s %s %d" % (prm(p), n, k, hx(neff[j]), hx(dc.EAF), rie))
    got = driver(lines)
    packed = dc.pack(codes)
    seen, ngen_vs_mincs = set(), set()
    for (j, k, rie, p), g in zip(cases, got):
        used, reason, mode, imp = int(g[0]), int(g[1]), int(g[2]), g[3]
        scores, stats, nloci = score_one(n, packed[j:j + 1], spc.PRESENT, rie, dc.EAF, p)
        what = (n, k, rie, p)
        assert (used, reason) == (stats["used"][0], stats["reason"][0]) and nloci == used, what
        if mode == 1:
            assert used == 1 and reason == dc.REASON_GENOTYPED, what
            quotient = p["imp_sample"].startswith("int") and n - k >= p["mincs"]
            assert_dosage(scores[codes[j] == 2], imp, what, spelled=not (quotient and k == n))
            if p["imp_sample"].startswith("int") and p["mincs"]:
                ngen_vs_mincs.add(n - k - p["mincs"])
        elif mode == 2:
            assert used == 1 and reason == dc.REASON_MAXMIS, what
            assert_dosage(scores, imp, what)
        else:
            assert mode == 0 and used == 0 and reason == dc.REASON_MAXMIS and p["imp_locus"] == "ignore" and np.isnan(scores).all(), what
        seen.add((mode, p["imp_sample"] if mode == 1 else p["imp_locus"], rie, k == n))
    # every setting was scored in the mode it acts in, with both ref_is_effect values, the all-missing row included
    assert {(1, s, rie, am) for s in refcpu.SAMPLE for rie in (0, 1) for am in (False, True)} <= seen
    assert {(2, loc, rie, am) for loc in refcpu.LOCUS if loc != "ignore" for rie in (0, 1) for am in (False, True)} <= seen
    assert {(0, "ignore", rie, am) for rie in (0, 1) for am in (False, True)} <= seen
    assert {-1, 0, 1} <= ngen_vs_mincs


def test_no_data_row_against_the_oracle(driver):
    n = 5
    none = np.zeros((0, 1), np.uint32)
    cases = [(kind, mis, loc, rie) for kind in (spc.ABSENT, spc.UNCOVERED, spc.FILTERED) for mis in refcpu.MISSING
             for loc in refcpu.LOCUS for rie in (0, 1)]
    params = [dict(imp_locus=loc, imp_missing=mis, imp_sample="int_ps", maxmis=0.05, mincs=100) for _, mis, loc, _ in cases]
    got = driver(["nodata %s %d %s %d" % (prm(p), kind, hx(dc.EAF), rie) for (kind, _, _, rie), p in zip(cases, params)])
    used_seen = set()
    for (kind, mis, loc, rie), p, g in zip(cases, params, got):
        used, reason, mode, imp = int(g[0]), int(g[1]), int(g[2]), g[3]
        scores, stats, nloci = score_one(n, none, kind, rie, dc.EAF, p)
        what = (kind, mis, loc, rie)
        assert (used, reason) == (stats["used"][0], stats["reason"][0]) and reason == REASONS[kind] and nloci == used, what
        assert mode == (2 if used else 0), what
        if used:
            assert_dosage(scores, imp, what)
        else:
            assert np.isnan(scores).all(), what
        used_seen.add((kind, used))
    assert used_seen == {(k, u) for k in REASONS for u in (0, 1)}


def test_the_nan_is_the_quiet_nan(driver):
    (bits,), = driver(["nan"])
    assert int(bits, 16) == QUIET_NAN
    # and it is what the rules return where the reference's dosage is NaN
    p = dict(imp_locus="fail", imp_missing="homref", imp_sample="int_fail", maxmis=0.05, mincs=100)
    got = driver(["row %s 0 777 %d %s %s 0" % (prm(p), k, hx(100.0), hx(dc.EAF)) for k in (700, 10)] +
                 ["row %s 0 777 10 %s %s 0" % (prm(dict(p, imp_sample="fail")), hx(100.0), hx(dc.EAF)),
                  "nodata %s %d %s 0" % (prm(p), spc.FILTERED, hx(dc.EAF))])
    assert [int(g[2]) for g in got] == [2, 1, 1, 2]
    assert int(got[0][3], 16) == QUIET_NAN and int(got[2][3], 16) == QUIET_NAN and int(got[3][3], 16) == QUIET_NAN
    assert got[1][3] == hx(100.0 / 767.0)   # enough genotyped samples: the cohort's own frequency
