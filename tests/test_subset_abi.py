"""CPU-side checks of the sample-subset entry points (include/nps.h): the header declares them, libnps.so exports them, the
binding knows them, and the argument errors that need no device are errors, not crashes."""
import ctypes as C
import os
import re

import numpy as np

from nimpress_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nps_sampleset_create", "nps_sampleset_n_samples", "nps_sampleset_n_kept", "nps_sampleset_destroy",
       "nps_score_cohort_def_subset", "nps_finish_subset", "nps_finish_subset_device"]


def test_header_declares_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "nps.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), "include/nps.h does not declare %s" % name
    assert "typedef struct nps_sampleset nps_sampleset;" in text
    assert int(re.search(r"#define NPS_ABI_VERSION (\d+)", text).group(1)) == 1   # new symbols only


def test_library_exports_the_new_symbols():
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), "libnps.so does not export %s" % name
        assert name in capi.SYMBOLS
    assert capi.load().nps_abi_version() == 1


def test_binding_has_the_new_classes():
    assert hasattr(capi, "SampleSet") and hasattr(capi.SampleSet, "n_kept") and hasattr(capi.SampleSet, "close")
    assert hasattr(capi.Scorer, "score_cohort_def_subset") and hasattr(capi.Scorer, "finish_subset")


def test_argument_errors_need_no_device():
    """keep == NULL, n_samples == 0 and a set that keeps nobody are refused before a device is looked for; NULL handles are
    errors; nothing is held afterwards"""
    L = capi.load()
    before = capi.live_resources()
    h = C.c_void_p()
    keep = np.ones(40, np.uint8)
    assert L.nps_sampleset_create(None, 0, 40, keep.ctypes.data) == capi.E_INVAL
    assert L.nps_sampleset_create(C.byref(h), 0, 40, None) == capi.E_INVAL and not h.value
    assert b"keep" in L.nps_last_error()
    assert L.nps_sampleset_create(C.byref(h), 0, 0, keep.ctypes.data) == capi.E_INVAL and not h.value
    none = np.zeros(40, np.uint8)
    assert L.nps_sampleset_create(C.byref(h), 0, 40, none.ctypes.data) == capi.E_INVAL and not h.value
    assert b"none" in L.nps_last_error()
    assert L.nps_sampleset_n_kept(None) == 0 and L.nps_sampleset_n_samples(None) == 0
    L.nps_sampleset_destroy(None)
    assert L.nps_score_cohort_def_subset(None, None, 0, None, None) == capi.E_INVAL
    assert L.nps_finish_subset(None, None, 0.0, None, None) == capi.E_INVAL
    assert L.nps_finish_subset_device(None, None, 0.0, None, None) == capi.E_INVAL
    assert capi.live_resources() == before


def test_no_sample_set_without_a_device():
    if capi.device_count() > 0:
        return
    h = C.c_void_p()
    keep = np.ones(40, np.uint8)
    assert capi.load().nps_sampleset_create(C.byref(h), 0, 40, keep.ctypes.data) == capi.E_NODEVICE
    assert not h.value and capi.live_resources() == 0
