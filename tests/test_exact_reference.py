"""CPU checks of tests/exact_reference.py: the references against math.fsum and fractions.Fraction, the oracle
bit-identical to the integer reference on exact designs, the numpy mirror of the strip kernels within its bar, and
every fault the mirror can be given rejected by the new bars (the subtle ones accepted by the old 1e-6 bar)."""
import math
from fractions import Fraction

import numpy as np
import pytest

import exact_reference as er
import score_compare
import special_cases as spc
from oracle import refcpu
from test_gpu_parity import PARAM_GRID, make_cohort


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)].view(np.int64),
                                                                        b[~np.isnan(b)].view(np.int64))


def test_dd_sum_against_fsum_and_fraction():
    rng = np.random.default_rng(1)
    m, n = 300, 17
    D = rng.choice([0.0, 1.0, 2.0, 1.0 / 3.0, 0.7], size=(m, n))
    b = np.round(rng.normal(0, 0.02, m), 4) * np.where(np.arange(m) % 7 == 0, 1e8, 1.0)
    hi, lo, ab = er.dd_sum(D, b)
    for i in range(n):
        exact = sum(Fraction(float(D[j, i])) * Fraction(float(b[j])) for j in range(m))
        assert abs(Fraction(float(hi[i])) + Fraction(float(lo[i])) - exact) <= Fraction(m * m) * Fraction(2) ** -106 * \
            Fraction(float(ab[i])) * 2
        p, e = er.two_prod(D[:, i], b)   # TwoProduct is exact: fsum of both halves is the correctly rounded sum
        assert math.fsum(list(p) + list(e)) == float(exact)
        assert float(hi[i]) == float(exact)


@pytest.mark.parametrize("pk", range(len(PARAM_GRID)))
@pytest.mark.parametrize("over", [True, False])
def test_oracle_and_mirror_exact_on_exact_designs(pk, over):
    p = PARAM_GRID[pk]
    for n, m in [(777, 40), (4000, 13), (1500, 90)]:
        codes, beta, eaf, rie = er.exact_design(n, m, 5 + n, over=over)
        ref, nl, _ = er.integer_reference(er.codes_dosages(codes), beta, eaf, rie, p, 0.375)
        got, _, onl = refcpu.score_packed(spc.pack(codes), n, np.zeros(m, np.int32), rie, beta, eaf,
                                          refcpu.make_params(**p), 0.375)
        assert onl == nl and same_bits(got, ref), (pk, n, m)
        mir, mnl = er.strip_mirror(codes, beta, eaf, rie, p, 0.375)
        assert mnl == nl and same_bits(mir, ref), (pk, n, m)


def test_oracle_ds_exact_on_quarter_grid():
    n, m = 1030, 30
    codes, beta, eaf, rie = er.exact_design(n, m, 3)
    rng = np.random.default_rng(4)
    ds = np.where(codes == 2, np.nan, rng.integers(0, 9, size=codes.shape) / 4.0).astype(np.float32)
    for p in PARAM_GRID:
        dos = np.where(rie[:, None] == 1, 2.0 - ds, ds)
        ref, nl, _ = er.integer_reference(dos, beta, eaf, rie, p, -0.25)
        sc = refcpu.RefScorer(n, refcpu.make_params(**p))
        for j in range(m):
            sc.row_ds(ds[j], bool(rie[j]), beta[j], eaf[j])
        got, onl = sc.finish(-0.25)
        assert onl == nl and same_bits(got, ref)


def test_mirror_exact_on_two_band_design():
    codes, beta, eaf, rie = er.two_band_design(130, 60, 9)
    assert len(er.strip_bands(beta, eaf)[1]) == 2
    for p in PARAM_GRID:
        ref, _, _ = er.integer_reference(er.codes_dosages(codes), beta, eaf, rie, p, 0.0)
        assert same_bits(er.strip_mirror(codes, beta, eaf, rie, p)[0], ref)


# ---- the mutation table
PROBE_PARAMS = dict(imp_locus="ps", imp_missing="homref", imp_sample="homref", maxmis=1.0, mincs=0)
REALISTIC_PARAMS = PARAM_GRID[6]


def probe_case():
    n, m = 64, 300
    rng = np.random.default_rng(1)
    codes = rng.choice(np.array([0, 1, 2, 3], np.uint8), size=(m, n), p=[0.4, 0.3, 0.05, 0.25])
    beta, eaf = er.probe_betas(m, 3), np.full(m, 0.25)
    rie = (np.arange(m) % 3 == 0).astype(np.int32)
    return codes, beta, eaf, rie


def realistic_case():
    """4000 x 1000, four-decimal betas, about 0.05 % missing genotypes (seeded: the old bar accepts drop5 and
    imp_float32 on it)"""
    n, m = 4000, 1000
    co = make_cohort(n, m, 84, np.random.default_rng(7), max_miss=0.001, force_missing_rows=False)
    return er.unpack(co["codes"], n), co["beta"], co["eaf"], co["rie"], co


def realistic_check(codes, beta, eaf, rie, mutation):
    """(within the strip bar, within the old bar) of the mirror with `mutation`"""
    p = REALISTIC_PARAMS
    dos = er.codes_dosages(codes)
    hi, lo, ab, nl, D, b, over = er.dd_reference(dos, beta, eaf, rie, p)
    _, rows, _ = er.impute(dos, beta, eaf, rie, p)
    got, _ = er.strip_mirror(codes, beta, eaf, rie, p, 0.0, mutation=mutation)
    bar = er.strip_bound(D, b, eaf[rows], over, ~np.isnan(dos[rows]), ab, got, nl)
    new_ok = bool(np.all(er.sum_error(got, nl, hi, lo) <= bar))
    ref, _, _ = refcpu.score_packed(spc.pack(codes), codes.shape[1], np.zeros(beta.size, np.int32), rie, beta, eaf,
                                    refcpu.make_params(**p), 0.0)
    try:
        score_compare.assert_scores(got, ref, beta, nl)
        old_ok = True
    except AssertionError:
        old_ok = False
    return new_ok, old_ok


SUBTLE = ["drop5", "imp_float32"]   # accepted by the old bar on the realistic case


@pytest.fixture(scope="module")
def cases():
    blk, sb, se, sr = er.saturation_design(32, 2100, 5)
    return dict(probe=probe_case(), realistic=realistic_case(), sat=(blk, sb, se, sr),
                two=er.two_band_design(130, 60, 9))


@pytest.mark.parametrize("mutation", er.MUTATIONS)
def test_mutations_fail_the_new_bar(cases, mutation):
    """every fault is rejected on the design that can show it; the unmutated mirror passes all of them"""
    fails = []
    codes, beta, eaf, rie = cases["probe"]
    ref = er.probe_reference(codes, beta, eaf, rie, er.strip_scale(beta, eaf))
    got = er.strip_mirror(codes, beta, eaf, rie, PROBE_PARAMS, mutation=mutation)[0]
    fails.append(("digit probes", not same_bits(got, ref)))
    codes, beta, eaf, rie, _ = cases["realistic"]
    new_ok, old_ok = realistic_check(codes, beta, eaf, rie, mutation)
    fails.append(("realistic", not new_ok))
    if mutation in SUBTLE or mutation == "none":
        assert old_ok, "the old 1e-6 bar should accept %s: it documents the gap" % mutation
    blk, sb, se, sr = cases["sat"]
    got = er.strip_mirror(np.tile(blk, (sb.size // 128, 1)), sb, se, sr, er.SAT_PARAMS, mutation=mutation)[0]
    fails.append(("saturated columns", not same_bits(got, er.saturation_reference(blk, sb))))
    codes, beta, eaf, rie = cases["two"]
    ref, _, _ = er.integer_reference(er.codes_dosages(codes), beta, eaf, rie, PARAM_GRID[0], 0.0)
    got = er.strip_mirror(codes, beta, eaf, rie, PARAM_GRID[0], mutation=mutation)[0]
    fails.append(("two bands", not same_bits(got, ref)))
    if mutation == "none":
        assert not any(f for _, f in fails), fails
    else:
        assert any(f for _, f in fails), "%s passes every bar: %s" % (mutation, fails)
    if mutation in SUBTLE:
        assert dict(fails)["realistic"], "%s must fail the strip bar on realistic inputs" % mutation


SAT_SB = 3100   # superblocks of the full-size saturation design (tests/test_gpu_exact.py): three windows, and past 2^24
               # in one window twice as long (at 1025 superblocks a doubled window would stay below 2^24 and pass)


def test_saturation_design_reaches_two_to_the_23():
    blk, sb, _, _ = er.saturation_design(32, SAT_SB, 5)
    peak = er.column_peak(blk, sb, list(range(32)))
    assert 2 ** 23 <= peak < 2 ** 24
    assert er.column_peak(blk, sb, list(range(32)), flush_sb=2 * er.FLUSH_SB) > 2 ** 24


def test_oracle_within_f64_bar_on_realistic_inputs():
    codes, beta, eaf, rie, co = realistic_case()
    for p in PARAM_GRID:
        dos = er.codes_dosages(codes)
        hi, lo, ab, nl, D, b, over = er.dd_reference(dos, beta, eaf, rie, p)
        got, _, _ = refcpu.score_packed(co["codes"], co["n"], np.zeros(co["m"], np.int32), rie, beta, eaf,
                                        refcpu.make_params(**p), 0.0)
        ok = np.isfinite(got)
        assert np.all(er.sum_error(got, nl, hi, lo)[ok] <= er.f64_bound(ab, nl, got, nl)[ok])
