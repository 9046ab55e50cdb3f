"""The host's decode of a FORMAT/GT vector into a float32 dosage row (decodeGtDosage, hook nh_decode_gt_dosage) -- what
the one-pass route over FORMAT/DS files uploads for a record that is scored from GT -- held to the oracle's getRawDosages
(RefScorer.row_gt, nimpress.nim:367-391) through the tallies the row produces: ngenotyped, nmissing, neffect.  No GPU."""
import numpy as np
import pytest

from nimpress_amd import host
from oracle import refcpu

PAD32 = np.int32(-2147483647)          # bcf_int32_vector_end
PAD = {np.int8: np.int8(-127), np.int16: np.int16(-32767), np.int32: PAD32}


def encode(alleles, rng):
    """allele indices (-1 = missing allele, -2 = vector-end pad) -> bcf_get_genotypes values, phase bits at random"""
    a = np.asarray(alleles, dtype=np.int64)
    v = ((a + 1) << 1) | rng.integers(0, 2, a.shape)
    return np.where(a == -2, np.int64(PAD32), v).astype(np.int32)


def typed(gts32, dtype):
    out = gts32.astype(dtype)
    out[gts32 == PAD32] = PAD[dtype]
    return out


def oracle_tallies(gts32, n, ploidy, eaidx):
    sc = refcpu.RefScorer(n, refcpu.make_params(maxmis=1.0))
    sc.row_gt(gts32, ploidy, eaidx, False, 0.01, 0.3)
    ngen, nmiss, neff = sc.stats[0][:3]
    sc.finish(0.0)
    return int(ngen), int(nmiss), float(neff)


def cases():
    rng = np.random.default_rng(12)
    n = 501
    dip = rng.choice([0, 1, 2, -1], size=(n, 2), p=[0.5, 0.3, 0.15, 0.05])
    yield "diploid", dip, 2
    hap = dip.copy()
    hap[rng.random(n) < 0.4, 1] = -2                     # haploid samples in a diploid record: the second value is a pad
    yield "haploid in diploid", hap, 2
    half = rng.choice([0, 1], size=(n, 2))
    half[::3, 0] = -1                                    # one allele missing, the other called: the sample is missing
    half[1::3, 1] = -1
    yield "half missing", half, 2
    tri = rng.choice([0, 1, 2, -1], size=(n, 3), p=[0.4, 0.4, 0.15, 0.05])
    tri[rng.random(n) < 0.2, 2] = -2
    yield "ploidy 3", tri, 3
    yield "one sample", np.array([[1, 1]]), 2


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32])
@pytest.mark.parametrize("name,alleles,ploidy", list(cases()), ids=[c[0] for c in cases()])
def test_decode_equals_the_oracle_tallies(name, alleles, ploidy, dtype):
    rng = np.random.default_rng(3)
    n = alleles.shape[0]
    gts32 = encode(alleles, rng).reshape(-1)
    for eaidx in (0, 1, 2):
        row = host.decode_gt_dosage(typed(gts32, dtype), ploidy, eaidx)
        assert row.dtype == np.float32 and row.shape == (n,)
        ngen, nmiss, neff = oracle_tallies(gts32, n, ploidy, eaidx)
        assert int(np.isnan(row).sum()) == nmiss and n - nmiss == ngen
        assert float(np.nansum(row.astype(np.float64))) == neff
        # and sample by sample: the count of the effect allele among the called alleles, NaN where any allele is missing
        want = np.where((alleles == -1).any(axis=1), np.nan, (alleles == eaidx).sum(axis=1)).astype(np.float32)
        assert np.array_equal(row, want, equal_nan=True), (name, eaidx)
    if ploidy == 3:
        assert np.nanmax(host.decode_gt_dosage(typed(gts32, dtype), ploidy, 1)) == 3.0


def test_code_maps_of_bed_and_pgen_records():
    """.bed: 0 = hom A1, 1 = missing, 2 = het, 3 = hom A2; .pgen: the number of ALT alleles, 3 = missing"""
    codes = np.array([0b11100100, 0b00000001], dtype=np.uint8)      # samples 0..4: codes 0, 1, 2, 3, 1
    nan = np.nan
    for code_map, want in ((0, [0, nan, 1, 2, nan]), (1, [2, nan, 1, 0, nan]), (2, [0, 1, 2, nan, 1]), (3, [2, 1, 0, nan, 1])):
        got = host.decode_code_dosage(codes, 5, code_map)
        assert np.array_equal(got, np.array(want, np.float32), equal_nan=True), code_map


def test_bad_arguments_are_refused():
    L = host.load()
    out = np.zeros(4, np.float32)
    g = np.zeros(8, np.int32)
    assert L.nh_decode_gt_dosage(g.ctypes.data, 3, 4, 2, 1, out.ctypes.data) == -1      # no 3-byte elements
    assert L.nh_decode_gt_dosage(g.ctypes.data, 4, 4, 0, 1, out.ctypes.data) == -1      # ploidy
    assert L.nh_decode_gt_dosage(None, 4, 4, 2, 1, out.ctypes.data) == -1
    assert L.nh_decode_code_dosage(g.ctypes.data, 4, 7, out.ctypes.data) == -1
