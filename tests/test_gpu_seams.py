"""Every host-side loop that cuts one C-ABI call into several kernel launches or staging chunks, crossed once.

The other GPU modules pin the arithmetic; their shapes fit one launch and one chunk of every loop in nps_cohort.hip, nps_resident.hip,
nps_kernels.hip, nps_mx.hip and nps_multi.hip (the generator's 32 768-row launches excepted).  Here each case is the smallest
shape with rows on both sides of a SEAM -- the first row a second launch or chunk handles -- with a ragged second piece, so
that a wrong second-chunk offset, a stage buffer that still holds the previous chunk, a code map indexed from the chunk
start, or a row number that forgets the chunk's first row cannot pass.  tests/seam_cases.py recomputes every seam from the
loop's formula and the cohort's row stride, and every test first asserts that its shape still crosses it (DESIGN.md
"Seams" lists loop, limit and test).

Bars are the existing ones: rows and tallies bit for bit; statistics by assert_stats_equal / assert_ds_stats and scores
within REL_TOL (tests/test_gpu_parity.py) on the row and DS paths; check_scores of tests/test_gpu_mx.py on the strip path;
REL_TOL of tests/test_gpu_multi.py for the multi-score pass; assert_scores (tests/score_compare.py), the bar
tests/test_gpu_special_values.py holds magnitude_1e-300 to, for the special rows.
"""
import ctypes as C

import numpy as np
import pytest

import seam_cases as sc
import special_cases as spc
import test_gpu_multi as tmulti
from conftest import need_free_hbm
from nimpress_amd import capi
from oracle import refcpu
from score_compare import assert_scores
from test_gpu_mx import check_scores
from test_gpu_parity import (PARAM_GRID, REL_TOL, assert_ds_stats, assert_stats_equal, make_cohort, oracle_scores, rel_err,
                             same_floats)

pytestmark = pytest.mark.gpu


def sub_cohort(co, r0, k):
    """rows [r0, r0 + k) of a make_cohort dict, as a cohort of their own"""
    return dict(co, m=k, **{key: co[key][r0:r0 + k] for key in ("codes", "beta", "eaf", "rie", "th", "tm", "tmi")})


def score(dev, n, kw, descs, row0=0, mode=capi.MODE_AUTO, offset=0.0):
    s = capi.Scorer(n, capi.make_params(**kw))
    s.score_cohort(dev, descs, row0, mode)
    stats = s.flush()
    scores, nloci = s.finish(offset)
    s.close()
    return scores, nloci, stats


def assert_tallies(dev, want, row0=0, nrows=None):
    nm, ne = dev.row_tallies(row0, nrows)
    nrows = nm.size
    assert np.array_equal(nm, want[0][row0:row0 + nrows]), "nmissing differs first at row %d" % (
        row0 + int(np.argmax(nm != want[0][row0:row0 + nrows])))
    assert np.array_equal(ne, want[1][row0:row0 + nrows]), "neffect differs first at row %d" % (
        row0 + int(np.argmax(ne != want[1][row0:row0 + nrows])))


def assert_rows(got, want, row0=0):
    if not np.array_equal(got, want):
        bad = np.nonzero(np.any(got != want, axis=1))[0]
        raise AssertionError("%d of %d rows differ, first at rows %s" % (bad.size, got.shape[0], row0 + bad[:8]))


# ---------------------------------------------------------------------------------------------------------------------
# tall row layout: 33 samples x 393 223 rows, NPS_FMT_GT2 (100 MB on the device)
@pytest.fixture(scope="module")
def tall_row():
    n, m = sc.TALL_ROW
    co = make_cohort(n, m, 20261019, np.random.default_rng(393))
    co["kw"] = PARAM_GRID[0]
    # the 7 rows of the second two-pass block weigh as much as all the others together (whose sum is of the order of
    # 0.02 sqrt(m) = 12): a block accumulated from the wrong rows is far outside the relative bar
    two = sc.seam_gt2_twopass(sc.gt2_stride_bytes(n))
    co["beta"][two:] = np.array([25.0, -18.5, 31.25, -27.0, 22.75, -35.5, 29.0])[:m - two]
    # ... and five of them have no missing genotype (33 samples: two missing are over --maxmis 0.05 and the row is imputed
    # for everyone, whatever its codes), two keep the generator's missing rate
    co["tmi"][two:][[0, 1, 3, 4, 6]] = 0
    co["codes"][two:] = refcpu.synth_rows(n, two, m - two, co["seed"], co["th"][two:], co["tm"][two:], co["tmi"][two:])
    co["ref"] = oracle_scores(co, co["kw"], 0.0)
    co["codes"].setflags(write=False)
    return co


def tall_row_seams(dev, m):
    """the seams of the four row-layout loops at this cohort's stride, each with whole groups of 4 on both sides"""
    stride = dev.row_stride
    assert stride == sc.gt2_stride_bytes(dev.n_samples)
    up = sc.assert_crosses("gt2_upload", sc.seam_gt2_upload(stride), m, 4)
    down = sc.assert_crosses("gt2_transfer", sc.seam_gt2_transfer(stride), m, 4)
    par = sc.assert_crosses("launch_cohort_parity", sc.seam_cohort_parity(), m, 4)
    two = sc.assert_crosses("score_run_gt2 two-pass blocks", sc.seam_gt2_twopass(stride), m, 4)
    for name, s in (("gt2_upload", up), ("gt2_transfer", down), ("launch_cohort_parity", par), ("score_run_gt2", two)):
        sc.assert_ragged(name, s, m, 4)
    return up, down, par, two


def seam_tall_row_upload_and_download_cross_their_chunks(tall_row):
    n, m = sc.TALL_ROW
    dev = capi.Cohort(n, m)
    up, down, _, _ = tall_row_seams(dev, m)
    dev.upload(0, tall_row["codes"])                       # gt2_upload: chunks of 262 140 and 131 083 rows
    assert_rows(dev.download(0, m), tall_row["codes"])     # gt2_transfer: chunks of 262 144 and 131 079 rows
    r0 = 262_136
    assert r0 % 4 == 0 and r0 < up < down < r0 + 16
    assert_rows(dev.download(r0, 16), tall_row["codes"][r0:r0 + 16], r0)
    dev.close()


def seam_tall_row_upload_bed_indexes_the_code_map_from_the_call_start(tall_row):
    n, m = sc.TALL_ROW
    dev = capi.Cohort(n, m)
    tall_row_seams(dev, m)
    maps = sc.code_maps(m, np.random.default_rng(33))
    rows = sc.file_rows(tall_row["codes"], n, maps)        # (the six padding bits of every row's last byte are set)
    assert rows.shape == (m, 9) and np.all(rows[:, -1] >> 2 == 0x3F)
    dev.upload_bed(0, rows, maps)
    assert_rows(dev.download(0, m), tall_row["codes"])     # the native codes, zero padding
    dev.close()


def seam_tall_row_optimize_and_rewrite_cross_the_parity_launches(tall_row):
    n, m = sc.TALL_ROW
    dev = capi.Cohort(n, m)
    _, _, par, _ = tall_row_seams(dev, m)
    dev.upload(0, tall_row["codes"])
    dev.optimize()                                         # launch_cohort_parity: 65 535 row groups, then 32 771
    assert_rows(dev.download(0, m), tall_row["codes"])     # (the parity layout is undone on the copy, chunk by chunk)
    r0 = 262_136
    assert r0 < par < r0 + 8
    want = tall_row["codes"].copy()
    want[r0:r0 + 8] = sc.random_codes(n, 8, np.random.default_rng(8))
    dev.upload(r0, want[r0:r0 + 8])                        # un-optimizes the whole cohort first, across the same seam
    got = dev.download(0, m)
    assert_rows(got, want)
    changed = np.nonzero(np.any(got != tall_row["codes"], axis=1))[0]
    assert changed.size and changed.min() >= r0 and changed.max() < r0 + 8
    dev.close()


def seam_tall_row_two_pass_blocks(tall_row, layout):
    """NPS_MODE_TWOPASS over 393 223 rows: a block of 393 216 rows and one of 7 (13 M genotypes against
    refcpu.score_packed)"""
    n, m = sc.TALL_ROW
    dev = capi.Cohort(n, m)
    tall_row_seams(dev, m)
    dev.upload(0, tall_row["codes"])
    if layout == "optimized":
        dev.optimize()
    descs = capi.row_descs(tall_row["beta"], tall_row["eaf"], None, tall_row["rie"])
    scores, nloci, stats = score(dev, n, tall_row["kw"], descs, mode=capi.MODE_TWOPASS)
    dev.close()
    ref_scores, ref_stats, ref_nloci = tall_row["ref"]
    assert nloci == ref_nloci
    two = sc.seam_gt2_twopass(sc.gt2_stride_bytes(n))
    assert sum(1 for r in ref_stats[two:] if r["reason"] == capi.REASON_GENOTYPED) >= 4, "the second block's rows are scored from their codes"
    sc.assert_all_stats(assert_stats_equal, stats, ref_stats, sc.seam_gt2_twopass(sc.gt2_stride_bytes(n)))
    err = rel_err(scores, ref_scores, tall_row["beta"], max(nloci, 1))
    print("two-pass, %s layout: relative error %.3g" % (layout, err))
    assert err <= REL_TOL


# ---------------------------------------------------------------------------------------------------------------------
# tall strip layout and conversions: 33 samples x 8 388 737 rows (65 538 superblocks, the last of one row)
@pytest.fixture(scope="module")
def tall_strip():
    n, m = sc.TALL_STRIP
    co = make_cohort(n, m, 20261020, np.random.default_rng(8388))
    co["tallies"] = sc.popcount_tallies(co["codes"])
    co["kw"] = PARAM_GRID[0]
    co["codes"].setflags(write=False)
    return co


def tall_strip_seams():
    n, m = sc.TALL_STRIP
    fill = sc.assert_crosses("gt2x_fill", sc.seam_gt2x_fill(n), m, 128)
    assert m - 2 * fill == 129, "gt2x_fill: chunks of 4 194 304, 4 194 304 and 129 rows"
    down = sc.assert_crosses("gt2x_download", sc.seam_gt2x_download(n), m, 128)
    sc.assert_ragged("gt2x_download", down, m, 128)
    assert sc.seam_gt2x_download_budget(n) > m, "gt2x_download: the launch limit, not the staging budget, splits this call"
    return fill, down


def strip_window(tall_strip, dev, r0, k):
    """NPS_MODE_AUTO over cohort rows [r0, r0 + k) against the oracle on just those rows"""
    n = sc.TALL_STRIP[0]
    w = sub_cohort(tall_strip, r0, k)
    scores, nloci, stats = score(dev, n, tall_strip["kw"], capi.row_descs(w["beta"], w["eaf"], None, w["rie"]), row0=r0)
    ref_scores, ref_stats, ref_nloci = oracle_scores(w, tall_strip["kw"], 0.0)
    assert nloci == ref_nloci
    assert_stats_equal(stats, [tuple(s) for s in ref_stats])
    check_scores(scores, ref_scores, w["beta"], nloci)


def check_filled_strip_cohort(tall_strip, dev):
    """after a fill in one call: tallies everywhere, the rows back in ONE download, and in the largest single launch"""
    n, m = sc.TALL_STRIP
    fill, down = tall_strip_seams()
    assert dev.has_tallies() and dev.rows_tallied(0, m)
    assert_tallies(dev, tall_strip["tallies"])
    assert_rows(dev.download(0, m), tall_strip["codes"])   # 65 538 superblocks: more than one launch_gt2x_to_rows takes
    assert 129 + down <= m and 129 < fill and 2 * fill < 129 + down
    assert_rows(dev.download(129, down), tall_strip["codes"][129:129 + down], 129)   # 65 535 superblocks, unaligned


def seam_tall_strip_upload_in_one_call(tall_strip):
    n, m = sc.TALL_STRIP
    fill, _ = tall_strip_seams()
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, tall_strip["codes"])
    check_filled_strip_cohort(tall_strip, dev)
    assert 4_194_176 < fill < 4_194_176 + 385
    strip_window(tall_strip, dev, 4_194_176, 385)          # rows of the first and of the second fill chunk
    dev.close()


def seam_tall_strip_upload_bed_in_one_call(tall_strip):
    n, m = sc.TALL_STRIP
    tall_strip_seams()
    maps = sc.code_maps(m, np.random.default_rng(65538))
    rows = sc.file_rows(tall_strip["codes"], n, maps)
    assert np.all(rows[:, -1] >> 2 == 0x3F)
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload_bed(0, rows, maps)
    check_filled_strip_cohort(tall_strip, dev)
    dev.close()


def seam_tall_strip_synth_then_keep_tallies(tall_strip):
    """mx_tally_kernel over 65 538 superblocks in one nps_cohort_keep_tallies"""
    n, m = sc.TALL_STRIP
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.synth(0, tall_strip["seed"], tall_strip["th"], tall_strip["tm"], tall_strip["tmi"])
    assert not dev.has_tallies()
    dev.keep_tallies()
    assert dev.has_tallies() and dev.rows_tallied(0, m)
    assert_tallies(dev, tall_strip["tallies"])
    dev.close()


def seam_tall_strip_conversions_cross_their_launches(tall_strip):
    """a NPS_FMT_GT2 source from the generator (2.1 GB) into NPS_FMT_GT2X (launches of 32 768, 32 768 and 2 superblocks) and
    into NPS_FMT_GT2M (65 535 and 3)"""
    need_free_hbm(6)
    n, m = sc.TALL_STRIP
    fill = sc.assert_crosses("launch_fill_gt2x_from_gt2", sc.seam_fill_gt2x_from_gt2(), m, 128)
    conv = sc.assert_crosses("launch_convert_gt2m", sc.seam_convert_gt2m(), m, 128)
    sc.assert_ragged("launch_convert_gt2m", conv, m, 128)
    src = capi.Cohort(n, m)
    src.synth(0, tall_strip["seed"], tall_strip["th"], tall_strip["tm"], tall_strip["tmi"])
    x = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    x.convert_from(src)
    assert x.has_tallies() and x.rows_tallied(0, m)
    assert_tallies(x, tall_strip["tallies"])
    assert_rows(x.download(0, m), tall_strip["codes"])
    assert 4_194_176 < fill < 4_194_176 + 385
    strip_window(tall_strip, x, 4_194_176, 385)
    x.close()
    g = capi.Cohort(n, m, fmt=capi.FMT_GT2M)
    g.convert_from(src)
    src.close()
    assert_tallies(g, tall_strip["tallies"])
    # two scores over the rows from superblock 65 534 to the end: superblock 65 535 is the first of the second launch, the
    # last one holds a single row
    r0 = 65_534 * 128
    k = m - r0
    assert r0 < conv < m and k == 385
    _, _, _, _, descs = tmulti.make_case(n, k, 2, 65534)
    kw = tmulti.PARAM_GRID[0]
    offsets = np.array([-0.5, 0.5])
    msc = capi.MultiScorer(n, capi.make_params(**kw), 2)
    mdef = capi.MultiDef(descs)
    msc.score_cohort(g, mdef, r0)
    got, nloci = msc.finish(offsets)
    msc.close()
    mdef.close()
    g.close()
    ref, ref_nloci = tmulti.oracle_scores(tall_strip["codes"][r0:], n, descs, kw, offsets)
    assert np.array_equal(nloci.astype(np.int64), ref_nloci)
    for s in range(2):
        keep = descs[s]["kind"] != capi.ROW_NOT_IN_SCORE
        assert tmulti.rel_err(got[s], ref[s], float(np.sum(np.abs(descs[s]["beta"][keep]))), int(ref_nloci[s])) <= tmulti.REL_TOL, s


# ---------------------------------------------------------------------------------------------------------------------
# wide: 70 001 samples x 15 361 rows, the byte-budget branch of the same min()
@pytest.fixture(scope="module")
def wide():
    n, m = sc.WIDE
    codes = sc.random_codes(n, m, np.random.default_rng(70001))
    tallies = sc.popcount_tallies(codes)
    codes.setflags(write=False)
    return dict(codes=codes, tallies=tallies)


def seam_wide_row_layout_upload_and_download(wide):
    n, m = sc.WIDE
    dev = capi.Cohort(n, m)
    stride = dev.row_stride
    assert stride == sc.gt2_stride_bytes(n)
    up = sc.assert_crosses("gt2_upload (byte budget)", sc.seam_gt2_upload(stride), m, 4)
    assert up < 4 * 65535
    sc.assert_ragged("gt2_upload (byte budget)", up, m, 4)
    down = sc.assert_crosses("gt2_transfer (byte budget)", sc.seam_gt2_transfer(stride), m, 4)
    sc.assert_ragged("gt2_transfer (byte budget)", m // down * down, m, 4)
    dev.upload(0, wide["codes"])                           # chunks of 15 196 and 165 rows
    assert_rows(dev.download(0, m), wide["codes"])         # a chunk every 3 796 rows
    r0 = 15_192
    assert r0 % 4 == 0 and r0 < up < r0 + 12
    assert_rows(dev.download(r0, 12), wide["codes"][r0:r0 + 12], r0)
    dev.close()


def seam_wide_strip_layout_fill_and_download(wide, how):
    n, m = sc.WIDE
    fill = sc.assert_crosses("gt2x_fill (byte budget)", sc.seam_gt2x_fill(n), m, 128)
    assert fill < 128 * 32768 and m - fill == 129          # the second chunk: one full superblock and one row
    down = sc.assert_crosses("gt2x_download (byte budget)", sc.seam_gt2x_download(n), m, 128)
    assert down < sc.GT2X_TO_ROWS_LAUNCH
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    if how == "upload":
        dev.upload(0, wide["codes"])
    else:
        maps = sc.code_maps(m, np.random.default_rng(15361))
        rows = sc.file_rows(wide["codes"], n, maps)
        assert np.all(rows[:, -1] >> 2 == 0x3F)
        dev.upload_bed(0, rows, maps)
    assert dev.has_tallies() and dev.rows_tallied(0, m)
    assert_tallies(dev, wide["tallies"])
    assert_rows(dev.download(0, m), wide["codes"])
    assert 129 + down <= m and 129 < fill < 129 + down     # one full download chunk that lies over the fill seam
    assert_rows(dev.download(129, down), wide["codes"][129:129 + down], 129)
    dev.close()


# ---------------------------------------------------------------------------------------------------------------------
# small shapes that still cross
@pytest.fixture(scope="module")
def ds_tall():
    n, m = sc.DS_TALL
    rng = np.random.default_rng(1048579)
    eaf = np.round(rng.uniform(0.01, 0.5, m), 4)
    miss = rng.uniform(0.0, 0.10, m)
    th, tm, tmi = refcpu.hwe_thresholds(eaf, miss)
    return dict(n=n, m=m, eaf=eaf, th=th, tm=tm, tmi=tmi, beta=np.round(rng.normal(0, 0.02, m), 4),
                rie=(rng.uniform(size=m) < 0.3).astype(np.int32))


def seam_ds16_staging_chunks_and_the_row_an_error_names(ds_tall):
    n, m = sc.DS_TALL
    seam = sc.assert_crosses("ds16_transfer", sc.seam_ds16_transfer(n), m)
    rows = refcpu.synth_rows_ds16(n, 0, m, 16, ds_tall["th"], ds_tall["tm"], ds_tall["tmi"])
    rows[seam:, 0] = [np.nan, np.float32("0.1234"), np.float32("1.5")]   # the second chunk: a missing value and two dosages
    assert np.isnan(rows[:seam]).any()
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS16)
    dev.upload(0, rows)                                    # chunks of 1 048 576 and 3 rows
    assert same_floats(dev.download(0, m), rows)
    for bad_row in (seam + 1, 5):                          # a value that is no four-place decimal, in either chunk
        r2 = rows.copy()
        r2[bad_row, 0] = np.float32(1.0) / np.float32(3.0)
        with pytest.raises(capi.NpsError) as ei:
            dev.upload(0, r2)
        assert ei.value.status == capi.E_UNSUPPORTED
        assert "row %d holds" % bad_row in str(ei.value), str(ei.value)
    dev.close()


def oracle_ds_rows(ds, rie, beta, eaf, kw, offset):
    """refcpu.RefScorer.row_ds for every row of a [rows, n] float32 matrix, without a numpy conversion per row"""
    L = refcpu.lib()
    m, n = ds.shape
    ds = np.ascontiguousarray(ds, dtype=np.float32)
    params = refcpu.make_params(**kw)
    state = L.ref_begin(n, C.byref(params))
    stats = np.zeros(m, dtype=refcpu.STAT_DTYPE)
    assert stats.itemsize == C.sizeof(refcpu.RefLocusStat)
    row_ds = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p)(("ref_row_ds", L))
    p_ds, p_st = ds.ctypes.data, stats.ctypes.data
    for j, (r, b, e) in enumerate(zip(rie.tolist(), beta.tolist(), eaf.tolist())):
        row_ds(state, p_ds + 4 * n * j, r, b, e, p_st + 32 * j)
    scores = np.empty(n, dtype=np.float64)
    nloci = C.c_int64(0)
    L.ref_finish(state, float(offset), scores.ctypes.data_as(C.POINTER(C.c_double)), C.byref(nloci))
    return scores, stats, int(nloci.value)


def seam_ds32_two_pass_blocks(ds_tall):
    n, m = sc.DS_TALL
    rows = refcpu.synth_rows_ds(n, 0, m, 32, ds_tall["th"], ds_tall["tm"], ds_tall["tmi"])
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32)
    seam = sc.assert_crosses("score_run_ds two-pass blocks", sc.seam_ds_twopass(dev.row_stride), m)
    # the 3 rows of the second block outweigh the first block's sum (of the order of 0.02 sqrt(m) = 20): hom, het, missing
    rows[seam:, 0] = [2.0, 1.0, np.nan]
    beta = ds_tall["beta"].copy()
    beta[seam:] = [37.5, -112.25, 64.0]
    ds_tall = dict(ds_tall, beta=beta)
    assert dev.row_stride == sc.ds32_stride_bytes(n)
    dev.upload(0, rows)
    kw = dict(imp_locus="ps", imp_missing="homref", imp_sample="int_ps", maxmis=0.05, mincs=100)
    descs = capi.row_descs(ds_tall["beta"], ds_tall["eaf"], None, ds_tall["rie"])
    scores, nloci, stats = score(dev, n, kw, descs, mode=capi.MODE_TWOPASS, offset=0.25)   # blocks of 1 048 576 and 3 rows
    dev.close()
    ref_scores, ref_stats, ref_nloci = oracle_ds_rows(rows, ds_tall["rie"], ds_tall["beta"], ds_tall["eaf"], kw, 0.25)
    assert nloci == ref_nloci
    sc.assert_all_stats(assert_ds_stats, stats, ref_stats, sc.seam_ds_twopass(sc.ds32_stride_bytes(n)), neffect_rel=1e-9)
    assert rel_err(scores, ref_scores, ds_tall["beta"], max(nloci, 1)) <= REL_TOL


@pytest.fixture(scope="module")
def special():
    n, m = sc.SPECIAL
    rng = np.random.default_rng(258113)
    th, tm, tmi = refcpu.hwe_thresholds(np.round(rng.uniform(0.05, 0.5, m), 4), rng.uniform(0.0, 0.1, m))
    codes = refcpu.synth_rows(n, 0, m, 5, th, tm, tmi)
    d = spc.definition("magnitude_1e-300", m)              # every beta ~1e-300: every PRESENT row is special
    assert np.all(d["kind"] == spc.PRESENT) and np.all(np.abs(d["beta"]) * 6.0 < 2.0 ** -900) and np.all(d["beta"] != 0.0)
    ref = refcpu.score_packed(codes, n, d["kind"], d["rie"], d["beta"], d["eaf"], refcpu.make_params(**d["params"]), d["offset"])
    return dict(codes=codes, d=d, ref=ref)


def seam_special_rows_in_two_batches(special, mode):
    n, m = sc.SPECIAL
    batch = sc.assert_crosses("mx_special_pass", sc.seam_mx_special(n), m, 4)
    assert m - batch == 5                                  # 258 108 special rows in the first batch, 5 in the second
    d = special["d"]
    dev = capi.Cohort(n, m, fmt=capi.FMT_GT2X)
    dev.upload(0, special["codes"])
    scores, nloci, stats = score(dev, n, d["params"], capi.row_descs(d["beta"], d["eaf"], d["kind"], d["rie"]), mode=mode,
                                 offset=d["offset"])
    dev.close()
    ref_scores, ref_stats, ref_nloci = special["ref"]
    assert nloci == ref_nloci
    sc.assert_all_stats(assert_stats_equal, stats, ref_stats, batch)
    assert_scores(scores, ref_scores, d["beta"], max(nloci, 1), "magnitude_1e-300 over %d x %d" % (n, m))


# ---------------------------------------------------------------------------------------------------------------------
# The cases above (seam_*: one per loop and path, each asserting its own seam first) run from two tests, one per layout
# family, in the order of DESIGN.md "Seams"; a failing case stops its test with the case's own message.
def test_row_layout_dosage_and_special_row_seams(tall_row, wide, ds_tall, special):
    seam_tall_row_upload_and_download_cross_their_chunks(tall_row)
    seam_tall_row_upload_bed_indexes_the_code_map_from_the_call_start(tall_row)
    seam_tall_row_optimize_and_rewrite_cross_the_parity_launches(tall_row)
    for layout in ("optimized", "plain"):
        seam_tall_row_two_pass_blocks(tall_row, layout)
    seam_wide_row_layout_upload_and_download(wide)
    seam_ds16_staging_chunks_and_the_row_an_error_names(ds_tall)
    seam_ds32_two_pass_blocks(ds_tall)
    for mode in (capi.MODE_AUTO, capi.MODE_TWOPASS):
        seam_special_rows_in_two_batches(special, mode)


def test_strip_layout_and_conversion_seams(tall_strip, wide):
    seam_tall_strip_upload_in_one_call(tall_strip)
    seam_tall_strip_upload_bed_in_one_call(tall_strip)
    seam_tall_strip_synth_then_keep_tallies(tall_strip)
    seam_tall_strip_conversions_cross_their_launches(tall_strip)
    for how in ("upload", "upload_bed"):
        seam_wide_strip_layout_fill_and_download(wide, how)
