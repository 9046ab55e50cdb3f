"""CPU-side checks of the sample-group entry points (include/nps.h): the header declares them, libnps.so exports them, the
binding knows them, and the argument errors that need no device are errors, not crashes -- with the offending sample or
group named."""
import ctypes as C
import os
import re

import numpy as np

from nimpress_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["nps_samplegroups_create", "nps_samplegroups_n_groups", "nps_samplegroups_n_samples", "nps_samplegroups_size",
       "nps_samplegroups_destroy", "nps_score_cohort_def_groups", "nps_flush_groups", "nps_finish_groups",
       "nps_finish_groups_device"]


def test_header_declares_the_new_symbols():
    text = open(os.path.join(ROOT, "include", "nps.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), "include/nps.h does not declare %s" % name
    assert "typedef struct nps_samplegroups nps_samplegroups;" in text
    assert int(re.search(r"#define NPS_GROUPS_MAX (\d+)", text).group(1)) == 8 == capi.GROUPS_MAX
    assert int(re.search(r"#define NPS_GROUP_NONE (\d+)", text).group(1)) == 255 == capi.GROUP_NONE
    assert int(re.search(r"#define NPS_ABI_VERSION (\d+)", text).group(1)) == 1   # new symbols only


def test_library_exports_the_new_symbols():
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), "libnps.so does not export %s" % name
        assert name in capi.SYMBOLS
    assert capi.load().nps_abi_version() == 1


def test_binding_has_the_new_classes():
    assert hasattr(capi, "SampleGroups")
    for attr in ("n_groups", "size", "close"):
        assert hasattr(capi.SampleGroups, attr)
    for attr in ("score_cohort_def_groups", "flush_groups", "finish_groups", "finish_groups_device"):
        assert hasattr(capi.Scorer, attr)


def test_argument_errors_need_no_device():
    """every NPS_E_INVAL of nps_samplegroups_create comes back before a device is looked for, the sample or group named;
    NULL handles are errors; nothing is held afterwards"""
    L = capi.load()
    before = capi.live_resources()
    h = C.c_void_p()
    lab = (np.arange(40) % 3).astype(np.uint8)

    def create(labels, n, G):
        rc = L.nps_samplegroups_create(C.byref(h), 0, n, labels.ctypes.data if labels is not None else None, G)
        assert not h.value
        return rc, L.nps_last_error()

    assert L.nps_samplegroups_create(None, 0, 40, lab.ctypes.data, 3) == capi.E_INVAL
    rc, text = create(None, 40, 3)
    assert rc == capi.E_INVAL and b"label" in text
    rc, text = create(lab, 0, 3)
    assert rc == capi.E_INVAL and b"no samples" in text
    for G in (0, -1, 9):
        rc, text = create(lab, 40, G)
        assert rc == capi.E_INVAL and b"n_groups %d" % G in text
    bad = lab.copy()
    bad[17] = 3                                  # a label >= n_groups that is not 255
    bad[30] = 254
    rc, text = create(bad, 40, 3)
    assert rc == capi.E_INVAL and b"sample 17 " in text and b"label 3" in text
    hole = lab.copy()
    hole[hole == 1] = capi.GROUP_NONE            # a group without a sample
    rc, text = create(hole, 40, 3)
    assert rc == capi.E_INVAL and b"group 1 " in text
    rc, text = create(lab, 40, 4)                # ... and the one past the labels used
    assert rc == capi.E_INVAL and b"group 3 " in text
    rc, text = create(np.full(40, capi.GROUP_NONE, np.uint8), 40, 2)
    assert rc == capi.E_INVAL and b"NPS_GROUP_NONE" in text
    # NULL handles
    assert L.nps_samplegroups_n_groups(None) == 0 and L.nps_samplegroups_n_samples(None) == 0
    assert L.nps_samplegroups_size(None, 0) == 0
    L.nps_samplegroups_destroy(None)
    assert L.nps_score_cohort_def_groups(None, None, 0, None, None) == capi.E_INVAL
    assert L.nps_flush_groups(None, None, 0, None) == capi.E_INVAL
    assert L.nps_finish_groups(None, None, 0.0, None, None) == capi.E_INVAL
    assert L.nps_finish_groups_device(None, None, 0.0, None, None) == capi.E_INVAL
    assert capi.live_resources() == before


def test_no_sample_groups_without_a_device():
    if capi.device_count() > 0:
        return
    h = C.c_void_p()
    lab = (np.arange(40) % 3).astype(np.uint8)
    assert capi.load().nps_samplegroups_create(C.byref(h), 0, 40, lab.ctypes.data, 3) == capi.E_NODEVICE
    assert not h.value and capi.live_resources() == 0
