"""CPU-side checks of the FORMAT/PL entry points (include/nps.h): libnps.so exports them, the binding knows them, the
likelihood table is what the header says, and without a device no context exists to push into."""
import ctypes as C
import math

import numpy as np

from nimpress_amd import capi

NEW = ["nps_push_pl", "nps_cohort_push_pl", "nps_pl_likelihoods"]


def test_library_exports_the_new_symbols():
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), "libnps.so does not export %s" % name
        assert name in capi.SYMBOLS
    assert capi.load().nps_abi_version() == 1


def test_likelihood_table():
    """T[k] = pow(10, -k / 10) in float64: T[0] = 1, strictly decreasing, T[255] > 0, every entry within 2 ulp of Python's
    own power (two good pow implementations may differ in the last bit)"""
    t = capi.pl_likelihoods()
    assert t.dtype == np.float64 and t.shape == (256,)
    assert t[0] == 1.0
    assert np.all(np.diff(t) < 0)
    assert t[255] > 0
    for k in range(256):
        ref = 10.0 ** (-k / 10.0)
        assert abs(t[k] - ref) <= 2 * math.ulp(ref), (k, t[k], ref)
    assert np.array_equal(t, capi.pl_likelihoods())                  # built once
    assert capi.load().nps_pl_likelihoods(None) == capi.E_INVAL      # needs a buffer, not a device


def test_null_handles_are_errors_not_crashes():
    L = capi.load()
    pl = np.zeros(3, np.int8)
    assert L.nps_push_pl(None, pl.ctypes.data, 1, 2, 1, 0, 0.1, 0.2) == capi.E_INVAL
    # argument errors come first, whatever the handle
    assert L.nps_cohort_push_pl(None, 0, pl.ctypes.data, 3, 2, 1) == capi.E_INVAL          # elem_bytes
    assert L.nps_cohort_push_pl(None, 0, pl.ctypes.data, 1, 9, 1) == capi.E_UNSUPPORTED    # alleles
    assert L.nps_cohort_push_pl(None, 0, pl.ctypes.data, 1, 1, 0) == capi.E_UNSUPPORTED
    assert L.nps_cohort_push_pl(None, 0, pl.ctypes.data, 1, 2, 2) == capi.E_INVAL          # eaidx
    assert L.nps_cohort_push_pl(None, 0, pl.ctypes.data, 1, 2, -1) == capi.E_INVAL
    assert L.nps_cohort_push_pl(None, 0, pl.ctypes.data, 1, 2, 1) == capi.E_INVAL          # the handle
    assert b"NULL" in L.nps_last_error()


def test_no_context_without_a_device():
    """where no GPU is visible nps_push_pl is unreachable: nps_create answers NPS_E_NODEVICE and nothing is held"""
    if capi.device_count() > 0:
        return
    h = C.c_void_p()
    p = capi.make_params()
    assert capi.load().nps_create(C.byref(h), 0, 64, C.byref(p)) == capi.E_NODEVICE
    assert not h.value and capi.live_resources() == 0
    co = C.c_void_p()
    assert capi.load().nps_cohort_create(C.byref(co), 0, 64, 4, capi.FMT_DS32) == capi.E_NODEVICE
    assert not co.value and capi.live_resources() == 0
