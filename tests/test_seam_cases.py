"""tests/seam_cases.py without a GPU: the vectorised .bed / .pgen byte builder against codes_to_bed / codes_to_pgen, the
population-count tallies against the oracle's row statistics, and every shape of tests/test_gpu_seams.py against the seam
formulas, with the strides the formulas imply (no library)."""
import numpy as np
import pytest

import seam_cases as sc
from oracle import refcpu
from test_gpu_parity import assert_ds_stats, assert_stats_equal, codes_to_bed, codes_to_pgen


@pytest.mark.parametrize("n", [1, 4, 5, 16, 33, 64, 70])
def test_file_rows_are_codes_to_bed_and_codes_to_pgen(n):
    rng = np.random.default_rng(n)
    m = 41
    codes = sc.random_codes(n, m, rng)
    maps = (np.arange(m) % 4).astype(np.uint8)
    want = np.stack([codes_to_bed(codes[j], n, int(maps[j])) if maps[j] < 2 else codes_to_pgen(codes[j], n, int(maps[j]) - 2)
                     for j in range(m)])
    assert np.array_equal(sc.file_rows(codes, n, maps, set_padding=False), want)
    got = sc.file_rows(codes, n, maps)
    assert got.shape == (m, (n + 3) // 4)
    if n % 4:
        pad = 0xFF & ~((1 << (2 * (n % 4))) - 1)
        assert np.all(got[:, -1] & pad == pad)
        got = got.copy()
        got[:, -1] &= 0xFF & ~pad
    assert np.array_equal(got, want)


def test_code_maps_hold_every_map():
    maps = sc.code_maps(1000, np.random.default_rng(0))
    assert maps.dtype == np.uint8 and set(np.unique(maps)) == {0, 1, 2, 3}


@pytest.mark.parametrize("n", [1, 33, 1001])
def test_popcount_tallies_are_the_oracles(n):
    m = 3000
    rng = np.random.default_rng(7 * n)
    eaf = np.round(rng.uniform(0.01, 0.5, m), 4)
    miss = rng.uniform(0.0, 0.4, m)
    th, tm, tmi = refcpu.hwe_thresholds(eaf, miss)
    codes = refcpu.synth_rows(n, 0, m, 99, th, tm, tmi)
    zeros = np.zeros(m, np.int32)
    _, stats, _ = refcpu.score_packed(codes, n, zeros, zeros, np.zeros(m), np.full(m, 0.1), refcpu.make_params(), 0.0)
    nm, ne = sc.popcount_tallies(codes)
    assert nm.dtype == np.uint64 and ne.dtype == np.uint64
    assert np.array_equal(nm, stats["nmissing"].astype(np.uint64))
    assert np.array_equal(ne.astype(np.float64), stats["neffect"])
    # ... and of random words (every code, missing included, at every position)
    codes = sc.random_codes(n, 200, rng)
    plain = ((codes[:, :, None] >> (2 * np.arange(16, dtype=np.uint32))) & 3).reshape(200, -1)[:, :n]
    nm, ne = sc.popcount_tallies(codes)
    assert np.array_equal(nm, (plain == 2).sum(axis=1).astype(np.uint64))
    assert np.array_equal(ne, ((plain == 1) + 2 * (plain == 3)).sum(axis=1).astype(np.uint64))


def test_stats_mismatch_is_the_existing_helpers_criterion():
    m = 5000
    rng = np.random.default_rng(5)
    th, tm, tmi = refcpu.hwe_thresholds(np.round(rng.uniform(0.01, 0.5, m), 4), rng.uniform(0.0, 0.1, m))
    codes = refcpu.synth_rows(40, 0, m, 3, th, tm, tmi)
    zeros = np.zeros(m, np.int32)
    _, ref, _ = refcpu.score_packed(codes, 40, zeros, zeros, np.zeros(m), np.full(m, 0.1), refcpu.make_params(), 0.0)
    gpu = np.zeros(m, dtype=[("ngenotyped", "<u8"), ("nmissing", "<u8"), ("neffect", "<f8"), ("used", "<i4"), ("reason", "<i4")])
    for k in gpu.dtype.names:
        gpu[k] = ref[k]
    assert sc.stats_mismatch(gpu, ref).size == 0
    sc.assert_all_stats(assert_stats_equal, gpu, ref, 4000)
    sc.assert_all_stats(assert_ds_stats, gpu, ref, 4000, neffect_rel=1e-9)
    for row, field, delta in ((7, "ngenotyped", 1), (4095, "nmissing", 1), (4999, "neffect", 1.0), (0, "used", 1),
                              (2500, "reason", 1), (4100, "neffect", 1e-12)):
        g = gpu.copy()
        g[field][row] += delta
        assert list(sc.stats_mismatch(g, ref)) == [row]
        with pytest.raises(AssertionError):
            sc.assert_all_stats(assert_stats_equal, g, ref, 4000)
        with pytest.raises(AssertionError):
            assert_stats_equal(g[row:row + 1], ref[row:row + 1])
        loose = delta == 1e-12     # within the float64-sum tolerance of the dosage path
        assert (sc.stats_mismatch(g, ref, 1e-9).size == 0) == loose
        if loose:
            sc.assert_all_stats(assert_ds_stats, g, ref, 4000, neffect_rel=1e-9)
            assert_ds_stats(g[row:row + 1], ref[row:row + 1])
        else:
            with pytest.raises(AssertionError):
                sc.assert_all_stats(assert_ds_stats, g, ref, 4000, neffect_rel=1e-9)


def test_seam_formulas_give_the_documented_rows():
    """the figures DESIGN.md "Seams" states, from the formulas"""
    n, m = sc.TALL_ROW
    stride = sc.gt2_stride_bytes(n)
    assert stride == 256
    assert sc.seam_gt2_upload(stride) == 262_140
    assert sc.seam_gt2_transfer(stride) == 262_144
    assert sc.seam_cohort_parity() == 262_140
    assert sc.seam_gt2_twopass(stride) == 393_216
    assert sc.seam_ds_twopass(sc.ds32_stride_bytes(sc.DS_TALL[0])) == 1_048_576
    assert sc.seam_ds16_transfer(sc.DS_TALL[0]) == 1_048_576
    assert sc.seam_gt2x_fill(sc.TALL_STRIP[0]) == 4_194_304
    assert sc.seam_gt2x_download(sc.TALL_STRIP[0]) == 8_388_480
    assert sc.seam_fill_gt2x_from_gt2() == 4_194_304 and sc.seam_convert_gt2m() == 8_388_480
    assert sc.seam_mx_special(sc.SPECIAL[0]) == 258_108
    assert sc.seam_mx_special(5000) == 4 * ((64 << 20) // ((313 + 320) * 4) // 4)
    n = sc.WIDE[0]
    assert sc.gt2_stride_bytes(n) == 4416 * 4
    assert sc.seam_gt2_upload(sc.gt2_stride_bytes(n)) == 15_196
    assert sc.seam_gt2_transfer(sc.gt2_stride_bytes(n)) == 3_796
    assert sc.seam_gt2x_fill(n) == 15_232 == sc.seam_gt2x_download(n)


def test_every_shape_has_rows_on_both_sides_of_its_seams():
    n, m = sc.TALL_ROW
    stride = sc.gt2_stride_bytes(n)
    up = sc.assert_crosses("gt2_upload", sc.seam_gt2_upload(stride), m, 4)
    sc.assert_ragged("gt2_upload", up, m, 4)
    down = sc.assert_crosses("gt2_transfer", sc.seam_gt2_transfer(stride), m, 4)
    sc.assert_ragged("gt2_transfer", down, m, 4)
    sc.assert_crosses("launch_cohort_parity", sc.seam_cohort_parity(), m, 4)
    two = sc.assert_crosses("score_run_gt2", sc.seam_gt2_twopass(stride), m, 4)
    sc.assert_ragged("score_run_gt2", two, m, 4)
    # the windows [262 136, +16) and [262 136, +8) hold both seams
    assert 262_136 % 4 == 0 and 262_136 < up < down < 262_136 + 16 and 262_136 < up < 262_136 + 8
    assert n % 16 and n % 32

    n, m = sc.TALL_STRIP
    fill = sc.assert_crosses("gt2x_fill", sc.seam_gt2x_fill(n), m, 128)
    assert m - 2 * fill == 129                                     # chunks of 4 194 304, 4 194 304 and 129 rows
    down = sc.assert_crosses("gt2x_download", sc.seam_gt2x_download(n), m, 128)
    sc.assert_ragged("gt2x_download", down, m, 128)
    assert sc.seam_gt2x_download_budget(n) > m                     # (the launch limit is what splits this call)
    # [129, +8 388 480): the most rows one launch takes, unaligned, over both fill seams
    assert 129 + down <= m and 129 < fill and 2 * fill < 129 + down
    sc.assert_crosses("launch_fill_gt2x_from_gt2", sc.seam_fill_gt2x_from_gt2(), m, 128)
    conv = sc.assert_crosses("launch_convert_gt2m", sc.seam_convert_gt2m(), m, 128)
    sc.assert_ragged("launch_convert_gt2m", conv, m, 128)
    assert (m + 127) // 128 == 65_538 and m % 128 == 1
    assert 4_194_176 < fill < 4_194_176 + 385 and 65_534 * 128 < conv < m

    n, m = sc.WIDE
    stride = sc.gt2_stride_bytes(n)
    up = sc.assert_crosses("gt2_upload (wide)", sc.seam_gt2_upload(stride), m, 4)
    sc.assert_ragged("gt2_upload (wide)", up, m, 4)
    down = sc.assert_crosses("gt2_transfer (wide)", sc.seam_gt2_transfer(stride), m, 4)
    sc.assert_ragged("gt2_transfer (wide)", m // down * down, m, 4)
    assert 15_192 % 4 == 0 and 15_192 < up < 15_192 + 12         # the window [15 192, +12) holds the upload seam
    fill = sc.assert_crosses("gt2x_fill (wide)", sc.seam_gt2x_fill(n), m, 128)
    assert m - fill == 129
    sc.assert_crosses("gt2x_download (wide)", sc.seam_gt2x_download(n), m, 128)
    assert 129 + fill <= m and 129 < fill < 129 + fill           # [129, +15 232): one full chunk over the fill seam
    assert n % 16 and n % 32

    n, m = sc.DS_TALL
    sc.assert_crosses("ds16_transfer", sc.seam_ds16_transfer(n), m)
    sc.assert_crosses("score_run_ds", sc.seam_ds_twopass(sc.ds32_stride_bytes(n)), m)
    n, m = sc.SPECIAL
    sp = sc.assert_crosses("mx_special_pass", sc.seam_mx_special(n), m, 4)
    assert m - sp == 5


def test_assert_crosses_fails_by_name():
    with pytest.raises(AssertionError, match="gt2_upload"):
        sc.assert_crosses("gt2_upload", 262_140, 262_142, 4)
    with pytest.raises(AssertionError, match="ds16_transfer"):
        sc.assert_crosses("ds16_transfer", 1_048_576, 1_048_576)
