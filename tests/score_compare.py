"""IEEE-exact comparison of scores with the oracle's (not a conftest: imported by the modules that use it).

The reference adds `dosage * beta` in plain float64 (nimpress.nim:639-641), so a definition with an infinite beta or eaf
gives +inf, -inf and NaN at particular samples.  A comparison first demands those three sets to be equal, then holds the
finite samples to the relative bar.  The floor of that bar, sum |beta| / (2 nloci), is taken over the FINITE betas: an
infinite beta must not make the tolerance infinite for every sample.
"""
import math
import sys

import numpy as np

REL_TOL = 1e-6


def special_mismatch(got, ref):
    """None when NaN, +inf and -inf sit at the same samples of `got` and `ref`; else a message that names them"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    if got.shape != ref.shape:
        return "shapes differ: %s against %s" % (got.shape, ref.shape)
    for name, f in (("NaN", np.isnan), ("+inf", np.isposinf), ("-inf", np.isneginf)):
        a, b = f(got), f(ref)
        if not np.array_equal(a, b):
            idx = np.nonzero(a != b)[0]
            return "%s positions differ at %d samples, first %s: got %s, reference %s" % (
                name, idx.size, idx[:8], got[idx[:8]], ref[idx[:8]])
    return None


def assert_special_equal(got, ref):
    """the IEEE special values agree sample by sample; returns the mask of the samples whose reference is finite"""
    msg = special_mismatch(got, ref)
    assert msg is None, msg
    return np.isfinite(np.asarray(ref, dtype=np.float64))


def beta_scale(beta, nloci):
    """sum |beta| / (2 nloci) over the finite betas (the scale of the floors; DBL_MAX where even that overflows)"""
    b = np.asarray(beta, dtype=np.float64).ravel()
    b = np.abs(b[np.isfinite(b)])
    with np.errstate(over="ignore"):
        sb = float(np.sum(b)) / max(2.0 * nloci, 1.0)
        if not math.isfinite(sb):
            sb = min(float(np.sum(b / max(2.0 * nloci, 1.0))), sys.float_info.max)
    return sb


def rel_err(got, ref, beta, nloci):
    """max |d| / max(|ref|, 1e-12 * sum|beta| / (2 nloci)) over the finite samples, after the special values agree"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    ok = assert_special_equal(got, ref)
    if not ok.any():
        return 0.0
    floor = 1e-12 * beta_scale(beta, nloci)
    return float(np.max(np.abs(got[ok] - ref[ok]) / np.maximum(np.abs(ref[ok]), max(floor, 1e-300))))


def assert_scores(got, ref, beta, nloci, what=""):
    """special values exact; every finite sample within 1e-6 relative of |ref| floored at 1e-12 of the scale, or (terms
    that cancel to almost nothing) within 2^-50 of the scale -- tests/test_gpu_mx.py check_scores' bar, without its count
    of escapes (these definitions are a few rows long).  No 1e-300 absolute floor: definitions of |beta| = 1e-300 and
    subnormal betas are held to their own scale."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    msg = special_mismatch(got, ref)
    assert msg is None, "%s: %s" % (what, msg)
    ok = np.isfinite(ref)
    if not ok.any():
        return
    sb = beta_scale(beta, nloci)
    d = np.abs(got[ok] - ref[ok])
    tol = np.maximum(REL_TOL * np.maximum(np.abs(ref[ok]), 1e-12 * sb), 2.0 ** -50 * sb)
    bad = np.nonzero(~(d <= tol))[0]
    if bad.size:
        idx = np.nonzero(ok)[0][bad]
        raise AssertionError("%s: %d finite samples differ, first %s: got %s, reference %s" % (
            what, bad.size, idx[:8], got[idx[:8]], ref[idx[:8]]))
