"""The dosage row tallies are one kernel template (ds_tally_kernel, nimpress_amd/csrc/nps_ds_common.h) and its copy under
a sample mask (ds_tally_masked_kernel, nps_ds.hip), and the paths that use them promise each other equal bits:
nps_push_ds + nps_flush, the two-pass run on a DS32 cohort, the subset run, and nps_multi_row_tallies on DS32 and DS16
cohorts.  Here they are held to each other and to tests/ds_tally_tree.py, the
tree restated in numpy, bit for bit, at the sample counts where the kernel changes its way: the ends of a lane-of-four
(1, 3, 4, 5), of a block's first sweep (1023 .. 1025), and of the first and second turn of the eight-fold unrolled loop
-- 7 168 samples are 1 792 lanes-of-four (nobody unrolls), 7 169 and 7 173 make thread 0 alone unroll, 8 192 every thread
with no tail, 8 193 and 9 221 with a tail, 16 389 a second turn."""
import numpy as np
import pytest

from ds_tally_tree import ds_tally_tree
from nimpress_amd import capi

pytestmark = pytest.mark.gpu

SAMPLES = [1, 3, 4, 5, 1023, 1024, 1025, 7168, 7169, 7173, 8192, 8193, 9221, 16389]
M = 6


def make_rows(n, rng):
    """float32[6, n] of decimals with at most four places (the value of DS16 code k, as the oracle forms it), so that the
    same rows upload losslessly to DS16: none missing, all missing, about 10 % missing, all 2.0, two random rows"""
    k = rng.integers(0, 20001, size=(M, n))
    ds = (k.astype(np.float64) * 1e-4).astype(np.float32)
    ds[1] = np.nan
    ds[2, rng.random(n) < 0.10] = np.nan
    ds[3] = 2.0
    for r in (4, 5):
        ds[r, rng.random(n) < 0.03] = np.nan
    return ds


def tree(ds, keep=None):
    t = [ds_tally_tree(row, keep) for row in ds]
    return (np.array([x[0] for x in t], np.uint64), np.array([x[1] for x in t], np.float64),
            np.array([x[2] for x in t], np.float64))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_stats(st, nm, neff, what):
    assert np.array_equal(st["nmissing"].astype(np.uint64), nm), what
    assert np.array_equal(bits(st["neffect"]), bits(neff)), what


@pytest.mark.parametrize("n", SAMPLES)
def test_every_dosage_tally_has_the_bits_of_the_tree(n):
    rng = np.random.default_rng(n)
    ds = make_rows(n, rng)
    rie = np.arange(M, dtype=np.int32) % 2
    descs = capi.row_descs(np.full(M, 0.01), np.full(M, 0.3), None, rie)
    nm, s, f = tree(ds)
    neff = np.where(rie == 1, f, s)
    params = capi.make_params()

    sc = capi.Scorer(n, params)
    for j in range(M):
        sc.push_ds(ds[j], int(rie[j]), 0.01, 0.3)
    assert_stats(sc.flush(), nm, neff, "nps_push_ds + nps_flush")

    dev = capi.Cohort(n, M, fmt=capi.FMT_DS32)
    dev.upload(0, ds)
    sd = capi.ScoreDef(descs)
    sc.reset()
    sc.score_cohort_def(dev, sd, 0, capi.MODE_TWOPASS)
    assert_stats(sc.flush(), nm, neff, "NPS_MODE_TWOPASS")

    half = (rng.random(n) < 0.5).astype(np.uint8)
    half[n // 2] = 1       # (no set is empty)
    last = np.zeros(n, np.uint8)
    last[n - 1] = 1
    keeps = [("every sample kept", np.ones(n, np.uint8)), ("a random half", half), ("only the last sample", last)]
    if n >= 2048:
        wave = np.ones(n, np.uint8)
        wave[1024:1280] = 0     # exactly the 1 KiB one wave skips
        keeps.append(("samples 1024 .. 1279 dropped", wave))
    for what, keep in keeps:
        knm, ks, kf = tree(ds, keep)
        sset = capi.SampleSet(keep)
        sc.reset()
        sc.score_cohort_def_subset(dev, sd, sset)
        assert_stats(sc.flush(), knm, np.where(rie == 1, kf, ks), what)
        sset.close()
    sc.close()
    sd.close()

    dev16 = capi.Cohort(n, M, fmt=capi.FMT_DS16)
    dev16.upload(0, ds)
    mdef = capi.MultiDef(descs[None, :])
    for what, co in (("nps_multi_row_tallies, DS32", dev), ("nps_multi_row_tallies, DS16", dev16)):
        msc = capi.MultiScorer(n, params, 1)
        msc.score_cohort(co, mdef)
        mnm, ms, mf = msc.row_tallies()
        msc.close()
        assert np.array_equal(mnm, nm), what
        assert np.array_equal(bits(ms)[rie == 0], bits(s)[rie == 0]), what
        assert np.array_equal(bits(mf)[rie == 1], bits(f)[rie == 1]), what
        assert np.array_equal(bits(ms), bits(s)) and np.array_equal(bits(mf), bits(f)), what   # (and the other sum of each row)
    for x in (mdef, dev16, dev):
        x.close()
