"""CPU-side checks of the two entry points the dosage multi-score path adds (include/nps.h): libnps.so exports them, the
binding knows them, and without a context they answer with a status -- they never crash."""
import ctypes as C

from nimpress_amd import capi

NEW = ["nps_multi_row_tallies", "nps_multi_geometry"]


def test_library_exports_the_new_symbols():
    lib = C.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert hasattr(lib, name), "libnps.so does not export %s" % name
        assert name in capi.SYMBOLS
    assert capi.RIE_COUNTS_EFFECT == 2


def test_null_context_is_an_error_not_a_crash():
    L = capi.load()
    nm = (C.c_uint64 * 4)()
    a, b = (C.c_double * 4)(), (C.c_double * 4)()
    assert L.nps_multi_row_tallies(None, 0, 4, nm, a, b) in (capi.E_INVAL, capi.E_NODEVICE)
    assert L.nps_multi_row_tallies(None, 0, 0, None, None, None) in (capi.E_INVAL, capi.E_NODEVICE)
    chunks, per = C.c_uint32(7), C.c_uint32(7)
    for fmt in (capi.FMT_DS32, capi.FMT_DS16, capi.FMT_GT2M, 99):
        assert L.nps_multi_geometry(None, fmt, 1000, C.byref(chunks), C.byref(per)) in (capi.E_INVAL, capi.E_NODEVICE)
    assert (chunks.value, per.value) == (7, 7)          # a refused call writes nothing
    assert b"NULL" in L.nps_last_error()


def test_no_context_without_a_device():
    """where no GPU is visible a multi-score context cannot exist: NPS_E_NODEVICE, nothing held"""
    if capi.device_count() > 0:
        return
    h = C.c_void_p()
    p = capi.make_params()
    assert capi.load().nps_multi_create(C.byref(h), 0, 64, C.byref(p), 2) == capi.E_NODEVICE
    assert not h.value and capi.live_resources() == 0
