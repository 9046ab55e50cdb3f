"""The oracle (oracle/refcpu.c) on score definitions with IEEE special values, against a direct numpy restatement of the
reference's row loop (nimpress.nim:626-649 with getImputedDosages :484-585): row order, float64, one product then `+=`,
then `/ (2 nloci)` and `+ offset`.  The GPU suite judges every path by this oracle on exactly these definitions
(tests/test_gpu_special_values.py), so the oracle is vouched for on them first.  No GPU."""
import ctypes
import ctypes.util

import numpy as np
import pytest

import special_cases as spc
from oracle import refcpu
from score_compare import assert_special_equal, rel_err, special_mismatch

LOCUS_IGNORE = "ignore"


def restated_scores(codes, d):
    """nimpress.nim:626-649, sample-vectorised, rows in score-file order"""
    p, n = d["params"], codes.shape[1]
    scores = np.zeros(n)
    nloci = 0
    r = 0
    for j in range(d["kind"].size):
        kind, rie, beta, eaf = int(d["kind"][j]), bool(d["rie"][j]), d["beta"][j], d["eaf"][j]

        def locus_value():   # imputeLocusDosages :417-447 (None: drop the row)
            if p["imp_locus"] == LOCUS_IGNORE:
                return None
            return {"ps": eaf * 2.0, "homref": 2.0 if rie else 0.0, "fail": np.nan}[p["imp_locus"]]

        if kind == spc.ABSENT:     # :536-551
            v = (2.0 if rie else 0.0) if p["imp_missing"] == "homref" else None
            dos = None if v is None else np.full(n, v)
        elif kind in (spc.UNCOVERED, spc.FILTERED):   # :526-531, :553-558
            v = locus_value()
            dos = None if v is None else np.full(n, v)
        else:
            dos = spc.dosages(codes[r])
            r += 1
            miss = np.isnan(dos)
            nmissing, ngenotyped = float(miss.sum()), float((~miss).sum())
            neffect = float(np.sum(dos[~miss]))
            if nmissing / float(n) > p["maxmis"]:   # :565-571
                v = locus_value()
                dos = None if v is None else np.full(n, v)
            else:                                   # imputeSampleDosages :450-481
                s = p["imp_sample"]
                if s == "ps":
                    v = eaf * 2.0
                elif s == "homref":
                    v = 2.0 if rie else 0.0
                elif s == "fail":
                    v = np.nan
                elif ngenotyped >= float(p["mincs"]):
                    with np.errstate(invalid="ignore", divide="ignore"):
                        v = np.float64(neffect) / np.float64(ngenotyped)
                else:
                    v = eaf * 2.0 if s == "int_ps" else np.nan
                dos = np.where(miss, v, dos)
        if dos is None:
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            scores += dos * beta      # :639-641, one product then +=
        nloci += 1
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        scores = scores / (float(nloci) * 2.0)   # :643-645
        scores = scores + d["offset"]            # :647-649
    return scores, nloci


def oracle(codes, d):
    present = codes[:int((d["kind"] == spc.PRESENT).sum())]
    return refcpu.score_packed(spc.pack(present), codes.shape[1], d["kind"], d["rie"], d["beta"], d["eaf"],
                               refcpu.make_params(**d["params"]), d["offset"])


@pytest.mark.parametrize("name", list(spc.CASES))
@pytest.mark.parametrize("shape", [(37, 9), (777, 13)])
def test_oracle_equals_restated_loop(name, shape):
    """bit for bit: the same operations in the same order, special values included"""
    n, m = shape
    codes = spc.base_codes(n, m)
    d = spc.definition(name, m)
    got, _, nloci = oracle(codes, d)
    want, want_nloci = restated_scores(codes, d)
    assert nloci == want_nloci
    assert special_mismatch(got, want) is None, special_mismatch(got, want)
    fin = np.isfinite(want)
    assert np.array_equal(got[fin], want[fin]), name


def test_special_cases_reach_the_special_values():
    """the definitions do what their names say: infinities of both signs and NaN where meant, finite scores where meant"""
    n, m = 777, 13
    codes = spc.base_codes(n, m)
    res = {k: restated_scores(codes, spc.definition(k, m)) for k in spc.CASES}
    s = {k: v[0] for k, v in res.items()}
    assert np.isposinf(s["beta_pinf"][1:3]).all() and np.isnan(s["beta_pinf"][0])   # 0 x inf at the hom-ref sample
    assert np.isneginf(s["beta_ninf"][1:3]).all()
    assert np.isnan(s["beta_nan"]).all()
    assert np.isnan(s["beta_pinf_ninf"][1:3]).all()                     # +inf + -inf at a sample het in both rows
    assert np.isneginf(s["beta_inf_maxmis_ps"]).all() and np.isposinf(s["beta_inf_maxmis_homref"]).all()
    assert np.isfinite(s["beta_inf_maxmis_ignore"]).all() and np.isfinite(s["beta_inf_absent_ignored"]).all()
    assert np.isnan(s["beta_inf_absent"]).all() and np.isneginf(s["beta_inf_uncovered"]).all()
    assert np.isposinf(s["beta_inf_filtered"]).all()
    for e in ("pinf", "ninf"):
        for k in ("eaf_%s_sample_ps" % e, "eaf_%s_int_ps_fallback" % e):
            assert np.isinf(s[k][3]) and np.isfinite(s[k][:3]).all()         # sample 3 is missing in row A
        assert np.isinf(s["eaf_%s_locus_ps" % e]).all()
    assert np.isnan(s["eaf_nan_locus_ps"]).all() and np.isnan(s["eaf_nan_sample_ps"][3])
    for k in ("beta_pzero_fail", "beta_nzero_fail", "beta_pzero_int_fail", "beta_nzero_int_fail"):
        assert np.isnan(s[k][3]) and np.isfinite(s[k][:3]).all()             # 0 x NaN stays NaN
    assert np.isnan(s["all_missing_row_int_ps"]).all()                       # 0 / 0 imputes NaN
    assert res["every_row_dropped"][1] == 0 and np.isnan(s["every_row_dropped"]).all()
    assert np.isposinf(s["offset_pinf"]).all() and np.isneginf(s["offset_ninf"]).all() and np.isnan(s["offset_nan"]).all()
    assert np.isfinite(s["magnitude_1e-300"]).all() and np.isfinite(s["magnitude_subnormal"]).all()
    assert (np.abs(s["magnitude_1e-300"]) < 1e-295).all() and (s["magnitude_1e-300"] != 0).any()
    assert np.isfinite(s["magnitude_1e300"]).all()
    assert np.isposinf(s["magnitude_1e307"]).any() and np.isfinite(s["magnitude_1e307"]).any()
    assert np.isposinf(s["magnitude_dbl_max"]).any()
    assert np.isfinite(s["banded_inf_row_dropped"]).all() and not np.isfinite(s["banded_inf_row"]).any()


# the spellings a score file may hold: the oracle's reader (Nim parseFloat) and the host's (C strtod) read the same doubles
SPELLINGS = ["inf", "-inf", "nan", "NaN", "1e400", "-1e400", "4.9e-324", "1.7976931348623157e308", "-0.0"]


def test_score_file_spellings_parse_alike():
    libc = ctypes.CDLL(ctypes.util.find_library("c"))
    libc.strtod.restype = ctypes.c_double
    libc.strtod.argtypes = [ctypes.c_char_p, ctypes.POINTER(ctypes.c_char_p)]
    for sp in SPELLINGS:
        a = refcpu.nim_parse_float(sp)
        end = ctypes.c_char_p()
        b = libc.strtod(sp.encode(), ctypes.byref(end))
        assert end.value == b"", sp   # the whole field is consumed, as nimpress_text.cpp parseFloatNim demands
        assert (np.isnan(a) and np.isnan(b)) or np.float64(a).tobytes() == np.float64(b).tobytes(), (sp, a, b)
    assert refcpu.nim_parse_float("1e400") == float("inf") and refcpu.nim_parse_float("4.9e-324") == 5e-324


def test_score_compare_rejects_special_mismatches():
    beta = np.array([0.1, -0.2, 0.3])
    ref = np.array([1.0, np.inf, -np.inf, np.nan, 0.5])
    assert_special_equal(ref.copy(), ref)
    assert rel_err(ref.copy(), ref, beta, 3) == 0.0
    for bad in ([1.0, -np.inf, -np.inf, np.nan, 0.5],     # +inf against -inf
                [1.0, 7.0, -np.inf, np.nan, 0.5],         # finite against +inf
                [1.0, np.inf, -np.inf, np.inf, 0.5],      # +inf against NaN
                [np.nan, np.inf, -np.inf, np.nan, 0.5]):  # NaN against finite
        assert special_mismatch(np.array(bad), ref) is not None, bad
        with pytest.raises(AssertionError):
            rel_err(np.array(bad), ref, beta, 3)


def test_score_compare_floor_ignores_infinite_betas():
    """an infinite beta elsewhere in the definition must not hide a finite error: the floor counts finite betas only"""
    ref = np.array([0.25, -0.5, 1.0])
    got = ref + np.array([0.0, 1e-3, 0.0])
    beta = np.array([0.1, np.inf, -0.2, np.nan])
    assert rel_err(got, ref, beta, 4) > 1e-4
    with pytest.raises(AssertionError):
        from score_compare import assert_scores
        assert_scores(got, ref, beta, 4)
    assert rel_err(ref.copy(), ref, beta, 4) == 0.0


def test_gpu_helpers_reject_special_mismatches():
    """the suite's own helpers (tests/test_gpu_parity.py rel_err, tests/test_gpu_mx.py check_scores) go through the same
    checks: they reject +inf against -inf and an error behind an infinite beta, and accept equal special patterns"""
    import test_gpu_mx
    import test_gpu_parity
    ref = np.array([1.0, np.inf, -np.inf, np.nan, 0.5])
    beta = np.array([0.1, np.inf, 0.3])
    n_esc = len(test_gpu_mx.ESCAPES)
    for f in (lambda g: test_gpu_parity.rel_err(g, ref, beta, 3) <= 1e-6,
              lambda g: test_gpu_mx.check_scores(g, ref, beta, 3) is not None):
        assert f(ref.copy())
        for bad in ([1.0, -np.inf, -np.inf, np.nan, 0.5], [1.0, 3.0, -np.inf, np.nan, 0.5],
                    [1.0, np.inf, -np.inf, np.inf, 0.5]):
            with pytest.raises(AssertionError):
                f(np.array(bad))
        with pytest.raises(AssertionError):
            assert f(ref + np.array([0.0, 0.0, 0.0, 0.0, 1e-3]))
    del test_gpu_mx.ESCAPES[n_esc:]   # (this module's calls are not the GPU module's samples)
