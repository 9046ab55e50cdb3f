"""Shapes, seams and host-side data of tests/test_gpu_seams.py (not a conftest: imported by that module and by
tests/test_seam_cases.py, which checks these helpers without a GPU).

A SEAM is the first row that a second kernel launch or a second staging chunk of one C-ABI call handles.  Every formula
here restates the chunk size of one host-side loop of nimpress_amd/csrc (DESIGN.md "Seams" names the loops); the tests
assert, before anything else, that their shape has at least one full unit of rows on each side of the seam, so a changed
budget fails by name instead of leaving a test that crosses nothing.

Codes are the C-ABI's: 2 bits per sample, 16 samples per uint32, low bits first; 0 = dosage 0, 1 = dosage 1, 3 = dosage 2,
2 = missing.
"""
import numpy as np

MIB = 1 << 20

# ---- the shapes (samples, rows)
TALL_ROW = (33, 393_223)         # NPS_FMT_GT2: upload, download, parity and two-pass seams; a last group of 3 rows
TALL_STRIP = (33, 8_388_737)     # 65 538 superblocks, the last of one row
WIDE = (70_001, 15_361)          # the byte-budget branch of the same min()
DS_TALL = (1, 1_048_579)         # NPS_FMT_DS16 staging chunks, NPS_FMT_DS32 two-pass blocks
SPECIAL = (5, 258_113)           # batches of special rows of a NPS_FMT_GT2X run


# ---- strides, as the library lays rows out (nps_kernels.h: words_for, stride_words_for, ds_stride_floats)
def words_for(n):
    return (n + 15) // 16


def gt2_stride_bytes(n):
    """row stride of a NPS_FMT_GT2 cohort (== nps_cohort_row_stride): the word count padded to 64 words"""
    return (max(words_for(n), 1) + 63) // 64 * 64 * 4


def ds32_stride_bytes(n):
    """row stride of a NPS_FMT_DS32 cohort: samples padded to 64 floats"""
    return (max(n, 1) + 63) // 64 * 64 * 4


def gt2x_stage_words(n):
    """staging row of gt2x_fill / gt2x_download: the word count rounded up to 4"""
    return (words_for(n) + 3) // 4 * 4


# ---- the seams: rows per launch / chunk of each loop
def seam_gt2_upload(row_stride):
    sw = row_stride // 4
    return min(max(4, (256 * MIB) // (sw * 4)) // 4 * 4, 4 * 65535)


def seam_gt2_transfer(row_stride):
    sw = row_stride // 4
    return 4 * max(1, (64 * MIB) // (sw * 16))


def seam_cohort_parity():
    return 4 * 65535


def seam_gt2_twopass(row_stride):
    return (max(64, (96 * MIB) // row_stride) + 15) // 16 * 16


def seam_ds_twopass(row_stride):
    return max(2048, (256 * MIB) // row_stride)


def seam_gt2x_fill(n):
    return min(max(128, (256 * MIB) // (gt2x_stage_words(n) * 4) // 128 * 128), 128 * 32768)


def seam_gt2x_download_budget(n):
    """the staging budget of gt2x_download alone"""
    return max(128, (256 * MIB) // (gt2x_stage_words(n) * 4) // 128 * 128)


GT2X_TO_ROWS_LAUNCH = 128 * 65535   # rows one launch_gt2x_to_rows takes (grid.y)


def seam_gt2x_download(n):
    return min(seam_gt2x_download_budget(n), GT2X_TO_ROWS_LAUNCH)


def seam_fill_gt2x_from_gt2():
    return 128 * 32768


def seam_convert_gt2m():
    return 128 * 65535


def seam_ds16_transfer(n):
    return (256 * MIB) // ((max(n, 1) + 63) // 64 * 64 * 4)


def seam_mx_special(n):
    row_bytes = (words_for(n) + gt2_stride_bytes(n) // 4) * 4
    return min(max(4, (64 * MIB) // row_bytes // 4 * 4), 65532 * 4)


def assert_crosses(loop, seam, nrows, unit=1):
    """rows [0, nrows) of one call have at least one full unit (row, group of 4, superblock of 128) on each side of the
    loop's seam"""
    assert seam >= unit and nrows - seam >= unit, (
        "%s: a call of %d rows no longer has a full unit of %d row(s) on both sides of the seam at row %d -- the loop's "
        "chunk size changed: move the test's shape with it" % (loop, nrows, unit, seam))
    return seam


def assert_ragged(loop, seam, nrows, unit):
    """the piece after the (last) seam is ragged: no multiple of the unit"""
    assert (nrows - seam) % unit != 0, "%s: the second piece of %d rows is a multiple of %d" % (loop, nrows - seam, unit)


# ---- row statistics of very many rows
def stats_mismatch(gpu_stats, ref_stats, neffect_rel=0.0):
    """the rows at which test_gpu_parity.assert_stats_equal (neffect_rel = 0: neffect equal as float64) or assert_ds_stats
    (neffect_rel = 1e-9, of max(1, |reference|)) would fail, found without a Python loop over a million rows; the caller
    hands a slice around the first of them to that helper, which then fails with its own message"""
    g, r = np.asarray(gpu_stats), np.asarray(ref_stats)
    assert g.shape == r.shape
    ok = (g["ngenotyped"].astype(np.int64) == r["ngenotyped"].astype(np.int64)) & \
         (g["nmissing"].astype(np.int64) == r["nmissing"].astype(np.int64)) & \
         (g["used"] == r["used"]) & (g["reason"] == r["reason"])
    ge, re = g["neffect"].astype(np.float64), r["neffect"].astype(np.float64)
    if neffect_rel:
        with np.errstate(invalid="ignore"):
            ok &= np.abs(ge - re) <= neffect_rel * np.maximum(1.0, np.abs(re))
    else:
        ok &= ge == re
    return np.nonzero(~ok)[0]


def assert_all_stats(helper, gpu_stats, ref_stats, seam, neffect_rel=0.0, margin=2048):
    """`helper` (assert_stats_equal / assert_ds_stats) holds for every row: applied itself to the rows around the seam and
    to the rows around the first mismatch, if stats_mismatch finds one"""
    assert len(gpu_stats) == len(ref_stats)
    lo = max(0, seam - margin)
    helper(gpu_stats[lo:seam + margin], ref_stats[lo:seam + margin])
    bad = stats_mismatch(gpu_stats, ref_stats, neffect_rel)
    if bad.size:
        lo = max(0, int(bad[0]) - 4)
        helper(gpu_stats[lo:lo + 64], ref_stats[lo:lo + 64])
    assert bad.size == 0, "%d rows differ, first %s" % (bad.size, bad[:8])


# ---- data
def popcount_tallies(codes):
    """(nmissing, neffect) of every row of [rows, words] uint32 codes whose padding bits are zero: tallyAlleles
    (nimpress.nim:32-47) as population counts -- missing = code 2, neffect = (code 1) + 2 (code 3)"""
    codes = np.ascontiguousarray(codes, dtype=np.uint32)
    m55 = np.uint32(0x55555555)
    nm, ne = np.empty(codes.shape[0], np.uint64), np.empty(codes.shape[0], np.uint64)
    step = max(1, (1 << 24) // max(codes.shape[1], 1))      # 64 MiB of codes at a time: the temporaries stay small
    for r in range(0, codes.shape[0], step):
        c = codes[r:r + step]
        lo, hi = c & m55, (c >> np.uint32(1)) & m55
        both = np.bitwise_count(lo & hi).sum(axis=1, dtype=np.uint64)
        nm[r:r + step] = np.bitwise_count(hi).sum(axis=1, dtype=np.uint64) - both
        ne[r:r + step] = np.bitwise_count(lo).sum(axis=1, dtype=np.uint64) + both
    return nm, ne


def code_maps(m, rng):
    """a NPS_MAP_* (0 .bed effect A2, 1 .bed effect A1, 2 .pgen effect ALT, 3 .pgen effect REF) per row: random, with a
    fixed pattern of period 5 on top so that a run of rows indexed from the wrong start never sees its own maps"""
    maps = rng.integers(0, 4, m).astype(np.uint8)
    maps[::5] = (np.arange(maps[::5].size) % 4).astype(np.uint8)
    return maps


def file_rows(codes, n, maps, set_padding=True):
    """[rows, words] native codes -> [rows, ceil(n/4)] bytes of PLINK .bed / .pgen rows that encode the same calls under
    each row's code map (tests/test_gpu_parity.py codes_to_bed / codes_to_pgen, vectorised); set_padding: the bits of the
    last byte past sample n are all SET (the files leave them zero; the library must not read them)"""
    codes = np.ascontiguousarray(codes, dtype="<u4")
    maps = np.asarray(maps, dtype=np.uint8)
    nb = (n + 3) // 4
    src = codes.view(np.uint8).reshape(codes.shape[0], -1)[:, :nb]
    out = np.empty((codes.shape[0], nb), dtype=np.uint8)
    m55 = np.uint8(0x55)
    for k in range(4):
        sel = np.nonzero(maps == k)[0]
        if sel.size == 0:
            continue
        w = src[sel]
        lo, hi = w & m55, (w >> np.uint8(1)) & m55
        if k == 0:      # .bed, effect A2: 0 -> 0 (hom A1), 1 -> 2 (het), 3 -> 3 (hom A2), missing -> 1
            v = hi | (lo << np.uint8(1))
        elif k == 1:    # .bed, effect A1: 0 -> 3, 1 -> 2, 3 -> 0, missing -> 1
            v = ~w
        elif k == 2:    # .pgen, effect ALT: the ALT count 0, 1, 2; missing -> 3
            v = w ^ hi
        else:           # .pgen, effect REF: 0 -> 2, 1 -> 1, 3 -> 0; missing -> 3
            v = ((~lo & m55) << np.uint8(1)) | (hi ^ lo)
        out[sel] = v
    if n % 4:
        keep = np.uint8((1 << (2 * (n % 4))) - 1)
        out[:, -1] &= keep
        if set_padding:
            out[:, -1] |= np.uint8(~keep & 0xFF)
    return out


def random_codes(n, m, rng):
    """[m, words] random 32-bit words, the bits past sample n cleared: any 2-bit code is a genotype"""
    w = words_for(n)
    codes = rng.integers(0, 1 << 32, size=(m, w), dtype=np.uint32)
    if n % 16:
        codes[:, -1] &= np.uint32((1 << (2 * (n % 16))) - 1)
    return codes
