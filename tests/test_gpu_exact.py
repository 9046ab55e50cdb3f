"""Every scoring path held to the error bar its own arithmetic implies (tests/exact_reference.py, DESIGN.md "Numerics").

* Exact designs (dyadic betas and eafs, power-of-two genotyped counts): every path of tests/test_gpu_special_values.py
  and the multi-score path give the integer reference's bits, over all seven imputation settings, at the special-value
  tests' shapes and strip plans, with rows over --maxmis (s_const) and a two-band definition.
* Digit probes: full-mantissa betas whose fixed-point images fill all fourteen hexadecimal digits; the strip paths give
  the correctly rounded exact integer sum, bit for bit.
* Realistic inputs (make_cohort, make_ds_cohort): within the path's bar of the double-double reference.
* Saturated digit columns at full size: 522 240 samples (255 strips, one row team), 2 100 superblocks; some digit
  column passes 2^23 inside one flush window of 1 024 superblocks.
"""
import time
import warnings

import numpy as np
import pytest

import exact_reference as er
import special_cases as spc
from conftest import need_free_hbm
from nimpress_amd import capi
from test_gpu_parity import PARAM_GRID, make_cohort, make_ds16_cohort, make_ds_cohort
from test_gpu_special_values import EARLIER_PATHS, PATHS, STRIP_PATHS, STRIP_SHAPES, Data, refused

pytestmark = pytest.mark.gpu

SMALL = (777, 40)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64),
                                                                        b[~np.isnan(b)].view(np.int64))


def assert_same_bits(got, ref, what):
    if same_bits(got, ref):
        return
    got, ref = np.asarray(got), np.asarray(ref)
    bad = np.nonzero(~((got == ref) | (np.isnan(got) & np.isnan(ref))))[0]
    raise AssertionError("%s: %d samples differ from the exact reference, first %s: got %r, exact %r" % (
        what, bad.size, bad[:6], got[bad[:6]].tolist(), ref[bad[:6]].tolist()))


class ExactData(Data):
    """Data (tests/test_gpu_special_values.py) over the codes of an exact design; definitions keyed (kind, pk)"""

    def __init__(self, n, m, over=True, seed=5):
        self.n, self.m = n, m
        self.codes, self.beta, self.eaf, self.rie = er.exact_design(n, m, seed + n, over=over)
        self.beta2 = er.two_band_design(n, m, seed + n)[1]
        self.packed = spc.pack(self.codes)
        self.cohorts, self.ref = {}, {}

    def definition(self, key):
        what, pk = key
        beta = self.beta
        if what == "two_band":   # (the same codes: exact_design draws them before the betas)
            beta = self.beta2
        return dict(kind=np.zeros(self.m, np.int32), rie=self.rie, beta=beta, eaf=self.eaf, params=PARAM_GRID[pk],
                    offset=0.375)

    def exact(self, key):
        if key not in self.ref:
            d = self.definition(key)
            ref, nl, _ = er.integer_reference(er.codes_dosages(self.codes), d["beta"], d["eaf"], d["rie"], d["params"],
                                              d["offset"])
            self.ref[key] = (d, ref, nl)
        return self.ref[key]


_DATA = {}


@pytest.fixture(scope="module")
def data():
    def get(shape, over=True):
        key = (shape, over)
        if key not in _DATA:
            for other in list(_DATA):
                if other[0] != SMALL:
                    _DATA.pop(other).close()
            _DATA[key] = ExactData(*shape, over=over)
        return _DATA[key]
    yield get
    for v in _DATA.values():
        v.close()
    _DATA.clear()


def check_exact(D, key, path):
    d, ref, nl = D.exact(key)
    what = "%s pk %d on %s (%d x %d)" % (key[0], key[1], path, D.n, D.m)
    assert not refused(path, d, lambda: PATHS[path](D, d), what), what + ": an exact design no path refuses"
    scores, nloci, _ = PATHS[path](D, d)
    assert nloci == nl
    assert_same_bits(scores, ref, what)


@pytest.mark.parametrize("over", [True, False])
@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
@pytest.mark.parametrize("path", EARLIER_PATHS)
def test_exact_design_small(data, path, pk, over):
    """rows over --maxmis (s_const on the strip paths) with `over`; without, every row's missing genotypes imputed"""
    check_exact(data(SMALL, over), ("plain", pk), path)


STRIP_RUNS = [(s, p) for s in STRIP_SHAPES for p in STRIP_PATHS if s != (4000, 13) or p == "gt2x_fused"]


@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
@pytest.mark.parametrize("shape,path", STRIP_RUNS)
def test_exact_design_strip_plans(data, shape, path, pk):
    check_exact(data(shape), ("plain", pk), path)


@pytest.mark.parametrize("pk", [0, 1, 6])
@pytest.mark.parametrize("path", STRIP_PATHS + ["gt2x_row0_128", "partial_gt2x", "gt2_fused", "push_packed"])
def test_exact_two_band_definition(data, path, pk):
    check_two_band(data, path, pk)


def check_two_band(data, path, pk):
    """(subset_gt2x: the strip arithmetic under the mask, one masked tally per band)"""
    D = data((1500, 60) if path in STRIP_PATHS + ["subset_gt2x"] else SMALL)
    assert len(er.strip_bands(D.definition(("two_band", pk))["beta"], D.eaf)[1]) == 2
    check_exact(D, ("two_band", pk), path)


def run_multi(D, d, wbits, mbits):
    """score d and its negation in one multi-score pass; returns (scores [2, n], nloci)"""
    msc = capi.MultiScorer(D.n, capi.make_params(**d["params"]), 2)
    if mbits != 56:
        msc.set_missing_weight_bits(mbits)
    rows = np.stack([capi.row_descs(d["beta"], d["eaf"], None, d["rie"]),
                     capi.row_descs(-d["beta"], d["eaf"], None, d["rie"])])
    mdef = capi.MultiDef(rows, weight_bits=wbits)
    msc.score_cohort(D.cohort("gt2m"), mdef)
    got, nloci = msc.finish([d["offset"], -d["offset"]])
    msc.close()
    mdef.close()
    return got, int(nloci[0])


def assert_multi_bound(D, d, got, nl, wbits, mbits, what, quant=True):
    """got[0] and -got[1] (scored with offset 0) within multi_bound of the double-double sum"""
    assert d["offset"] == 0.0
    dos = er.codes_dosages(D.codes)
    hi, lo, ab, nl_ref, Dm, b, over = er.dd_reference(dos, d["beta"], d["eaf"], d["rie"], d["params"])
    assert nl == nl_ref
    _, rows, _ = er.impute(dos, d["beta"], d["eaf"], d["rie"], d["params"])
    ND = 7 if wbits == 49 else 6
    for k, sign in ((0, 1.0), (1, -1.0)):
        g = sign * got[k]
        ok = np.isfinite(g)
        assert np.array_equal(ok, np.isfinite(hi + lo)), what
        if quant:
            bar = er.multi_bound(Dm, b, d["eaf"][rows], over, ~np.isnan(dos[rows]), ab, g, nl, ND, mbits, d["beta"],
                                 np.isnan(dos).sum(axis=0))
        else:   # digit probes: every weight an exact integer of the scale, only the fold's roundings remain
            bar = er.multi_bound(Dm, np.zeros_like(b), d["eaf"][rows], over, ~np.isnan(dos[rows]), ab, g, nl, ND, 56,
                                 d["beta"])
        err = er.sum_error(g, nl, hi, lo)
        assert np.all(err[ok] <= bar[ok]), "%s: error %.3g of the bar" % (what, float(np.max(err[ok] / bar[ok])))


# the settings whose imputed weights are known before the tally (ps / homref / fail): on the exact design every
# missing-weight coefficient lies on the 32- and 40-bit grids, so weight_digits (nps_multi.hip:291-295) rounds nothing
MULTI_EXACT_COARSE = (1, 2, 4)


@pytest.mark.parametrize("wbits", [49, 41])
@pytest.mark.parametrize("mbits", [56, 40, 32])
@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
def test_exact_design_multi_score(data, pk, mbits, wbits):
    """NPS_FMT_GT2M: exact int8 digit sums.  Bit for bit with full-width missing weights, and with 40 / 32-bit ones
    where the design's weights lie on the coarse grid; in the int_* settings the ratio neffect / 777 of the rows without
    a missing sample is rounded in the prefix coefficients it shares with other rows: those runs are held to the
    documented truncation bound (include/nps.h)"""
    D = data(SMALL)
    d, ref, nl = D.exact(("plain", pk))
    got, nloci = run_multi(D, d, wbits, mbits)
    assert nloci == nl
    what = "multi pk %d, %d / %d bits" % (pk, wbits, mbits)
    if mbits == 56 or pk in MULTI_EXACT_COARSE:
        assert_same_bits(got[0], ref, what)
        assert_same_bits(got[1], -ref, what + " (negated)")
    else:
        d0 = dict(d, offset=0.0)
        assert_multi_bound(D, d0, run_multi(D, d0, wbits, mbits)[0], nl, wbits, mbits, what)


@pytest.mark.parametrize("wbits", [49, 41])
@pytest.mark.parametrize("mbits", [56, 40, 32])
@pytest.mark.parametrize("pk", [0, 1, 3, 6])
def test_realistic_multi_score_within_bar(real, pk, mbits, wbits):
    D, p = real, PARAM_GRID[pk]
    co = D.co
    d = dict(kind=np.zeros(D.m, np.int32), rie=co["rie"], beta=co["beta"], eaf=co["eaf"], params=p, offset=0.0)
    got, nl = run_multi(D, d, wbits, mbits)
    assert_multi_bound(D, d, got, nl, wbits, mbits, "realistic multi pk %d, %d / %d bits" % (pk, wbits, mbits))


@pytest.mark.parametrize("wbits", [49, 41])
def test_digit_probes_multi(data, wbits):
    """betas whose images beta 2^F are integers filling all ND base-256 digits (8 ND - 12 bits), homref imputation:
    every weight exact, so only the fold's roundings separate the result from the exact sum"""
    D = data(SMALL)
    ND = 7 if wbits == 49 else 6
    L = 8 * ND - 12
    rng = np.random.default_rng(8)
    mant = rng.integers(2 ** (L - 1), 2 ** L, D.m, dtype=np.int64)
    beta = np.where(rng.uniform(size=D.m) < 0.5, -1.0, 1.0) * np.ldexp(mant.astype(np.float64), -4 - L + 1)
    F, _ = er.multi_scale(beta, np.full(D.m, 0.25), ND)
    assert np.all(np.abs(beta) * 2.0 ** F == np.round(np.abs(beta) * 2.0 ** F))
    assert np.abs(beta * 2.0 ** F).min() >= 2.0 ** (8 * ND - 13)
    d = dict(kind=np.zeros(D.m, np.int32), rie=D.rie, beta=beta, eaf=np.full(D.m, 0.25), params=PROBE_PARAMS,
             offset=0.0)
    got, nl = run_multi(D, d, wbits, 56)
    assert nl == D.m
    assert_multi_bound(D, d, got, nl, wbits, 56, "multi digit probes, %d bits" % wbits, quant=False)


# ---- digit probes
PROBE_PARAMS = dict(imp_locus="ps", imp_missing="homref", imp_sample="homref", maxmis=1.0, mincs=0)


PROBE_RUNS = STRIP_RUNS + [((1500, 2000), "gt2x_row0_128"), ((1500, 2000), "partial_gt2x")]
# (the subset run is the strip arithmetic; the design's power-of-two genotyped counts hold because N = n_kept = n)
SUBSET_PROBE_RUNS = [((1500, 2000), "subset_gt2x")]
PROBE_BANDS = (1, 3, 4, 5, 6, 7, 8)
INT_PS_PROBE = dict(imp_locus="ps", imp_missing="homref", imp_sample="int_ps", maxmis=1.0, mincs=0)


@pytest.mark.parametrize("shape,path,n_bands", [(s, p, b) for s, p in PROBE_RUNS for b in PROBE_BANDS])
def test_digit_probes_strip(data, shape, path, n_bands):
    check_digit_probes(data(shape), shape, path, n_bands)


def check_digit_probes(D, shape, path, n_bands):
    """full-mantissa betas, one set per magnitude band (beta 2^F_b = 53-bit integers over fourteen digits): bit for bit
    what the kernels' arithmetic gives -- each band's exact integer sum rounded once, scaled, the bands added in order
    (nps_mx.hip:604-607); under homref a missing genotype weighs 0 or 2 w1, under int_ps rn(fl(imp w1)) with the
    design's power-of-two genotyped counts (nps_mx_common.h:166-170)"""
    beta, eaf = er.banded_probe_betas(D.m, n_bands, 3), np.full(D.m, 0.25)
    assert len(er.strip_bands(beta, eaf)[1]) == min(n_bands, D.m)
    for params in (PROBE_PARAMS, INT_PS_PROBE):
        d = dict(kind=np.zeros(D.m, np.int32), rie=D.rie, beta=beta, eaf=eaf, params=params, offset=0.0)
        ref = er.banded_probe_reference(D.codes, beta, eaf, D.rie, params)
        scores, nloci, _ = PATHS[path](D, d)
        assert nloci == D.m
        assert_same_bits(scores, ref, "digit probes, %d bands, %s, on %s %s" % (n_bands, params["imp_sample"], path,
                                                                                shape))


# ---- realistic inputs
class RealData(Data):
    def __init__(self, n, m, seed=21):
        self.n, self.m = n, m
        self.co = make_cohort(n, m, seed, np.random.default_rng(seed), max_miss=0.03)
        self.codes = er.unpack(self.co["codes"], n)
        self.packed = self.co["codes"]
        self.rie = self.co["rie"]
        self.cohorts, self.ref = {}, {}


GT2X_PATHS = STRIP_PATHS + ["gt2x_row0_128", "partial_gt2x", "subset_gt2x"]


@pytest.fixture(scope="module")
def real():
    D = RealData(3000, 400)
    yield D
    D.close()


@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
@pytest.mark.parametrize("path", EARLIER_PATHS)
def test_realistic_within_path_bar(real, path, pk):
    check_realistic(real, path, pk)


def check_realistic(D, path, pk):
    """within the path's bar of the double-double reference: strip_bound on the NPS_FMT_GT2X paths, f64_bound elsewhere"""
    p = PARAM_GRID[pk]
    co = D.co
    d = dict(kind=np.zeros(D.m, np.int32), rie=co["rie"], beta=co["beta"], eaf=co["eaf"], params=p, offset=0.0)
    dos = er.codes_dosages(D.codes)
    hi, lo, ab, nl, Dm, b, over = er.dd_reference(dos, co["beta"], co["eaf"], co["rie"], p)
    assert not refused(path, d, lambda: PATHS[path](D, d), path), path + ": a realistic definition no path refuses"
    got, nloci, _ = PATHS[path](D, d)
    assert nloci == nl
    ok = np.isfinite(got)
    assert np.array_equal(ok, np.isfinite(hi + lo)), "NaN positions differ"
    err = er.sum_error(got, nl, hi, lo)
    if path in GT2X_PATHS:
        _, rows, _ = er.impute(dos, co["beta"], co["eaf"], co["rie"], p)
        bar = er.strip_bound(Dm, b, co["eaf"][rows], over, ~np.isnan(dos[rows]), ab, got, nl)
    else:
        bar = er.f64_bound(ab, nl, got, nl)
    worst = float(np.max(err[ok] / bar[ok])) if ok.any() else 0.0
    assert worst <= 1.0, "%s pk %d: error %.3g of the bar" % (path, pk, worst)


@pytest.mark.parametrize("fmt", ["ds32", "ds16"])
def test_realistic_ds_cohort_within_f64_bar(fmt):
    """non-integer dosages (make_ds_cohort, make_ds16_cohort) through the single-read DS kernels"""
    n, m = 2500, 300
    co = (make_ds_cohort if fmt == "ds32" else make_ds16_cohort)(n, m, 17, np.random.default_rng(17))
    ds = co["ds"]
    dev = capi.Cohort(n, m, fmt=capi.FMT_DS32 if fmt == "ds32" else capi.FMT_DS16)
    dev.upload(0, np.ascontiguousarray(ds))
    for pk in (0, 6):
        p = PARAM_GRID[pk]
        sc = capi.Scorer(n, capi.make_params(**p))
        sc.score_cohort(dev, capi.row_descs(co["beta"], co["eaf"], None, co["rie"]), 0, capi.MODE_FUSED)
        got, nl_got = sc.finish(0.0)
        sc.close()
        dos = np.where(co["rie"][:, None] == 1, 2.0 - ds.astype(np.float64), ds.astype(np.float64))
        hi, lo, ab, nl, _, _, _ = er.dd_reference(dos, co["beta"], co["eaf"], co["rie"], p)
        assert nl_got == nl
        ok = np.isfinite(got)
        assert np.all(er.sum_error(got, nl, hi, lo)[ok] <= er.f64_bound(ab, nl, got, nl)[ok])
    dev.close()


# ---- saturated digit columns, full size
SAT_N, SAT_SB = 522240, 3100


def test_full_size_saturated_digit_columns():
    """255 strips (the single-read kernel on a 256-CU part: one row team), 3 100 superblocks: three whole flush windows
    and a tail; digit column 11 of the samples missing in every row at 75 x 131 072 = 9.8e6 > 2^23 inside a window.  The
    CPU mirror shows that a window twice as long misses the exact result (tests/test_exact_reference.py).  Scored by
    the single-read kernel and, after keep_tallies(), by the given-tallies kernel, whose plan deals the superblocks to
    Q teams (1 034 / 1 033 / 1 033 with Q = 3): every team crosses a window, and the teams differ in length
    (n_t and n_flush per team, nps_mxg.hip, nps_mx.hip:589).  The run time is reported as a warning."""
    import torch
    need_free_hbm(60)
    t0 = time.time()
    block, beta, eaf, rie = er.saturation_design(SAT_N, SAT_SB, 5)
    m = beta.size
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    sc = capi.Scorer(SAT_N, capi.make_params(**er.SAT_PARAMS))
    slices, teams, _ = sc.fused_geometry(m, capi.FMT_GT2X)
    sc.close()
    if slices == 0:
        pytest.skip("no resident grid for 255 strips on this part")
    assert (slices, teams) == (255, 1), (slices, teams)
    Q = er.given_teams(255, cus, SAT_SB)
    longest, shortest = (SAT_SB + Q - 1) // Q, SAT_SB // Q
    assert Q >= 2 and shortest > er.FLUSH_SB and longest != shortest, (Q, longest, shortest)
    samples = list(range(64))
    assert er.column_peak(block, beta, samples) >= 2 ** 23
    assert er.column_peak(block, beta, samples, Q=Q) >= 2 ** 23
    ref = er.saturation_reference(block, beta)
    co = capi.Cohort(SAT_N, m, fmt=capi.FMT_GT2X)
    try:
        rows = np.ascontiguousarray(np.tile(spc.pack(block), (16, 1)))
        for r0 in range(0, m, rows.shape[0]):
            co.upload(r0, rows[: min(rows.shape[0], m - r0)])
        del rows
        descs = capi.row_descs(beta, eaf, None, rie)
        for mode, label in ((capi.MODE_FUSED, "single read"), (None, "tallies given")):
            if mode is None:
                co.keep_tallies()
                mode = capi.MODE_AUTO
            sc = capi.Scorer(SAT_N, capi.make_params(**er.SAT_PARAMS))
            sc.score_cohort(co, descs, 0, mode)
            got, nloci = sc.finish(0.0)
            sc.close()
            assert nloci == m
            assert_same_bits(got, ref, "saturated columns, " + label)
    finally:
        co.close()
    warnings.warn("full-size saturation test (%d samples x %d superblocks, given-tallies Q = %d): %.1f s" % (
        SAT_N, SAT_SB, Q, time.time() - t0))
