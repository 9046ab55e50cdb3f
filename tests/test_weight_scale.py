"""The fixed-point weight scales of a definition (nimpress_amd/csrc/nps_scale.h), without a GPU: which rows the strip
kernels cannot carry, the magnitude bands and scale exponents of the others, and the one scale per score of a multi-score
definition.  tests/native/scale_driver.cpp includes that header alone and is compiled with plain g++: the rules need
neither HIP nor a device.  Every quantity is an integer or a float64 compared by its bit pattern: no tolerances.  The numpy
copies of the rules are tests/exact_reference.py's strip_scale, strip_bands and multi_scale."""
import math
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

import exact_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESENT, UNCOVERED, ABSENT, FILTERED, NOT_IN_SCORE = 0, 1, 2, 3, 4   # nps_row_kind, NPS_ROW_NOT_IN_SCORE (include/nps.h)
NAN, INF, DBL_MAX = float("nan"), float("inf"), sys.float_info.max
TINY = 5e-324                                                        # the smallest subnormal


def bits(x):
    return "%016x" % struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def unbits(s):
    return struct.unpack("<d", struct.pack("<Q", int(s, 16)))[0]


def below(x):
    return math.nextafter(x, 0.0)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("scale") / "scale_driver")
    r = subprocess.run([gxx, "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-I",
                        os.path.join(ROOT, "nimpress_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "scale_driver.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "warning" not in r.stderr, r.stderr[-2000:]

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [a.split() for a in answers]
    return ask


def bands_query(beta, eaf):
    return "bands %d " % len(beta) + " ".join(bits(b) + " " + bits(e) for b, e in zip(beta, eaf))


def parse_bands(a, m):
    """-> mx_bound bits, special rows, band per row, {band: (bound bits, F)} of the bands that cost a pass, in order"""
    k = int(a[1])
    special = [int(x) for x in a[2:2 + k]]
    band = [int(x) for x in a[2 + k:2 + k + m]]
    u = int(a[2 + k + m])
    rest = a[3 + k + m:]
    assert len(rest) == 3 * u
    used = [(int(rest[3 * i]), rest[3 * i + 1], int(rest[3 * i + 2])) for i in range(u)]
    assert [b for b, _, _ in used] == sorted(set(b for b, _, _ in used))
    return a[0], special, band, {b: (bound, F) for b, bound, F in used}


def ask_bands(driver, beta, eaf):
    a, = driver([bands_query(beta, eaf)])
    return parse_bands(a, len(beta))


# ------------------------------------------------------------------------------------------------------------------
# the strip path: against exact_reference.strip_scale / strip_bands
def random_definition(rng):
    """1 .. 64 rows, finite eaf, no special row: bounds between 2^-300 and 2^100, one or several bands, some zero betas"""
    m = int(rng.integers(1, 65))
    spread = float(rng.choice([1.0, 25.0, 40.0, 100.0, 300.0]))
    beta = rng.choice([-1.0, 1.0], m) * rng.uniform(1.0, 2.0, m) * np.exp2(rng.integers(-20, 20) - np.floor(rng.uniform(0, spread, m)))
    beta[rng.uniform(size=m) < 0.1] = 0.0
    if rng.uniform() < 0.05:
        beta[:] = 0.0
    eaf = np.where(rng.uniform(size=m) < 0.8, rng.uniform(0.0, 1.0, m), rng.uniform(-3.0, 3.0, m))
    return beta, eaf


def check_against_reference(driver, designs):
    answers = driver([bands_query(b, e) for b, e in designs])
    for (beta, eaf), a in zip(designs, answers):
        mx_bound, special, band, used = parse_bands(a, beta.size)
        want_band, want_F = er.strip_bands(beta, eaf)
        assert special == []
        assert band == [int(b) for b in want_band]
        assert {b: F for b, (_, F) in used.items()} == {b: F for b, F in enumerate(want_F) if F is not None}
        v = np.abs(beta) * (4.0 + np.maximum(2.0, 2.0 * np.abs(eaf)))
        assert mx_bound == bits(v.max())
        for b, (bound, F) in used.items():      # a band's own bound and scale: strip_scale of its rows
            sel = (want_band == b) & (v > 0)
            assert bound == bits(v[sel].max() if sel.any() else 0.0)
            assert F == er.strip_scale(beta[sel], eaf[sel])


def test_bands_and_scales_are_the_reference_copys(driver):
    rng = np.random.default_rng(20240611)
    designs = [random_definition(rng) for _ in range(400)]
    assert sum(len(set(er.strip_bands(b, e)[0])) > 1 for b, e in designs) > 100   # (banded definitions among them)
    check_against_reference(driver, designs)


@pytest.mark.parametrize("n_bands", range(1, 9))
def test_banded_probe_designs(driver, n_bands):
    rng = np.random.default_rng(n_bands)
    designs = []
    for m in (n_bands, 24, 61):
        beta = er.banded_probe_betas(m, n_bands, seed=100 + m)
        designs.append((beta, rng.uniform(0.0, 1.0, m)))
        designs.append((beta, np.zeros(m)))
    check_against_reference(driver, designs)
    _, _, band, used = ask_bands(driver, *designs[2])
    assert band == [j % n_bands for j in range(24)] and sorted(used) == list(range(n_bands))


def test_band_edges(driver):
    """eaf = 0: a row's bound is 6 |beta|.  Under a top row of beta = 1 (bound 6 < 2^3) a row of beta = 2^-g has the exponent
    gap e_top - e_v = g exactly"""
    gaps = [29, 30, 59, 60, 239, 240, 400]
    beta = np.array([1.0] + [2.0 ** -g for g in gaps] + [0.0, -0.0])
    mx_bound, special, band, used = ask_bands(driver, beta, np.zeros(beta.size))
    assert special == [] and mx_bound == bits(6.0)
    assert band[1:8] == [0, 1, 1, 2, 7, 7, 7]           # 240 / 30 = 8 and 400 / 30 = 13: clamped to kMxMaxBands - 1
    assert band[0] == 0 and band[8:] == [0, 0]          # a zero beta is in band 0 ...
    assert sorted(used) == [0, 1, 2, 7]                 # bands 3 .. 6 are empty: no pass
    # ... and contributes to no bound: each band's is its largest row's, the scale 56 - e2 with bound < 2^e2
    assert used[0] == (bits(6.0), 53)
    assert used[1] == (bits(6.0 * 2.0 ** -30), 53 + 30)
    assert used[2] == (bits(6.0 * 2.0 ** -60), 53 + 60)
    assert used[7] == (bits(6.0 * 2.0 ** -239), 53 + 239)
    # only zero betas: band 0 alone, bound 0, scale 56
    assert ask_bands(driver, np.zeros(3), np.array([0.1, 0.2, 5.0])) == (bits(0.0), [], [0, 0, 0], {0: (bits(0.0), 56)})
    # band 0 counts as present even where only its zero betas and special rows are left in it -- it never is empty of the
    # top row, so: the top row alone and one row two bands down
    _, _, band, used = ask_bands(driver, np.array([3.0, 0.0, 3.0 * 2.0 ** -61]), np.zeros(3))
    assert band == [0, 0, 2] and sorted(used) == [0, 2]


def test_special_rows_are_left_out_of_the_plan(driver):
    """the plan is made with the special rows at beta = eaf = 0: band 0, part of no bound"""
    beta = np.array([NAN, 1.0, INF, 2.0 ** -40, DBL_MAX, 0.5, TINY, -INF])
    eaf = np.array([0.1, 0.2, 0.3, NAN, 0.0, INF, 0.0, 0.5])
    mx_bound, special, band, used = ask_bands(driver, beta, eaf)
    assert special == [0, 2, 4, 5, 6, 7]
    assert mx_bound == bits(1.0 * (4.0 + 2.0))
    assert band == [0, 0, 0, 1, 0, 0, 0, 0]
    assert used == {0: (bits(6.0), 53), 1: (bits(2.0 ** -40 * 6.0), 93)}      # (a NaN eaf: span 2)


# (beta, eaf) -> (special, bound); eaf = 2 makes the bound 8 |beta|, exact
SPECIAL = [
    ((NAN, 0.3), (1, 0.0)), ((INF, 0.3), (1, 0.0)), ((-INF, 0.3), (1, 0.0)),
    ((1.0, INF), (1, 0.0)), ((1.0, -INF), (1, 0.0)), ((0.0, INF), (1, 0.0)),
    ((1.0, NAN), (0, 6.0)), ((-1.0, NAN), (0, 6.0)),
    ((2.0 ** -903, 2.0), (0, 2.0 ** -900)), ((below(2.0 ** -903), 2.0), (1, below(2.0 ** -900))),
    ((below(2.0 ** 997), -2.0), (0, below(2.0 ** 1000))), ((-2.0 ** 997, 2.0), (1, 2.0 ** 1000)),
    ((0.0, 0.3), (0, 0.0)), ((-0.0, 1e300), (0, 0.0)), ((0.0, NAN), (0, 0.0)), ((0.0, 0.0), (0, 0.0)),
    ((DBL_MAX, 0.0), (1, INF)), ((-DBL_MAX, 0.5), (1, INF)),
    ((TINY, 0.0), (1, TINY * 6.0)), ((-TINY, 0.0), (1, TINY * 6.0)),
    ((0.25, 0.5), (0, 1.5)), ((0.25, -1.5), (0, 0.25 * 7.0)),
]


def test_special_rows_by_hand(driver):
    answers = driver(["special %s %s" % (bits(b), bits(e)) for (b, e), _ in SPECIAL])
    for ((b, e), (sp, bound)), a in zip(SPECIAL, answers):
        assert (int(a[0]), a[1]) == (sp, bits(bound)), (b, e)


def test_imputation_span(driver):
    cases = [(0.0, 2.0), (0.3, 2.0), (-1.0, 2.0), (1.0, 2.0), (below(-1.0), 2.0), (1.5, 3.0), (-2.5, 5.0), (NAN, 2.0), (INF, 2.0),
             (-INF, 2.0), (DBL_MAX, INF)]
    answers = driver(["span " + bits(e) for e, _ in cases])
    assert [a[0] for a in answers] == [bits(s) for _, s in cases]
    assert answers[4][0] == bits(2.0)      # 2 |eaf| one ulp under 2: the max holds it at 2


def test_scale_exponent(driver):
    """56 - e2 with bound < 2^e2, clamped to +-1000.  No finite double reaches the lower clamp (DBL_MAX < 2^1024 gives
    -968): the upper one is reached from 2^-945 down."""
    cases = [(0.0, 56), (-1.0, 56), (NAN, 56), (1.0, 55), (below(1.0), 56), (6.0, 53), (2.0 ** -900, 955), (2.0 ** -944, 999),
             (below(2.0 ** -944), 1000), (2.0 ** -1000, 1000), (TINY, 1000), (below(2.0 ** 1000), -944), (2.0 ** 1000, -945),
             (DBL_MAX, -968)]
    answers = driver(["exp " + bits(b) for b, _ in cases])
    assert [int(a[0]) for a in answers] == [F for _, F in cases]
    rng = np.random.default_rng(5)
    v = rng.uniform(1.0, 2.0, 200) * np.exp2(rng.integers(-1070, 1023, 200))
    answers = driver(["exp " + bits(x) for x in v])
    assert [int(a[0]) for a in answers] == [er.strip_scale(np.array([x / 6.0]), np.zeros(1)) if x / 6.0 * 6.0 == x else
                                            min(1000, max(-1000, 56 - math.frexp(x)[1])) for x in v]


# ------------------------------------------------------------------------------------------------------------------
# the multi-score path: against exact_reference.multi_scale
def multi_query(rows, S, ND):
    """rows: S lists of (kind, beta, eaf)"""
    n_desc = len(rows[0])
    assert len(rows) == S and all(len(r) == n_desc for r in rows)
    return "multi %d %d %d " % (S, n_desc, ND) + " ".join("%d %s %s" % (k, bits(b), bits(e)) for r in rows for k, b, e in r)


def ok(a, S):
    assert a[0] == "ok" and len(a) == 2 + S, a
    return int(a[1]), [int(x) for x in a[2:]]


def refused(a):
    assert a[0] == "refused", a
    return a[1], int(a[2]), int(a[3]), unbits(a[4]), unbits(a[5])


@pytest.mark.parametrize("ND", [6, 7])
def test_multi_scale_is_the_reference_copys(driver, ND):
    rng = np.random.default_rng(ND)
    queries, want = [], []
    for _ in range(150):
        S, n = int(rng.integers(1, 9)), int(rng.integers(1, 40))
        rows = []
        for s in range(S):
            span = int(rng.integers(0, 17 if ND == 6 else 25))       # (max / min < 2^(span + 1): inside the limit)
            beta = rng.choice([-1.0, 1.0], n) * rng.uniform(1.0, 2.0, n) * np.exp2(rng.integers(-300, 300) + rng.integers(0, span + 1, n))
            beta[rng.uniform(size=n) < 0.1] = 0.0
            eaf = np.where(rng.uniform(size=n) < 0.8, rng.uniform(0.0, 1.0, n), rng.uniform(-3.0, 3.0, n))
            kind = rng.integers(PRESENT, FILTERED + 1, n)             # every row is in the score
            rows.append(list(zip(kind, beta, eaf)))
            want.append(er.multi_scale(beta, eaf, ND)[0])
        queries.append((multi_query(rows, S, ND), S))
    got = []
    for a, (_, S) in zip(driver([q for q, _ in queries]), queries):
        no_scale, F = ok(a, S)
        assert no_scale == -1
        got += F
    assert got == want


@pytest.mark.parametrize("ND", [6, 7])
def test_multi_scale_by_hand(driver, ND):
    F0 = 8 * ND - 9
    row = lambda beta, eaf=0.25, kind=PRESENT: (kind, beta, eaf)      # noqa: E731
    ref = lambda beta, eaf: er.multi_scale(np.array(beta), np.array(eaf), ND)[0]   # noqa: E731

    # rows the score file does not list are ignored, whatever they hold
    a, = driver([multi_query([[row(0.5), row(NAN, INF, NOT_IN_SCORE), row(2.0 ** 200, 9.0, NOT_IN_SCORE), row(-0.75)]], 1, ND)])
    assert ok(a, 1) == (-1, [ref([0.5, -0.75], [0.25, 0.25])])
    # a NaN eaf is left out of the largest |eaf|
    a, = driver([multi_query([[row(0.5, NAN), row(0.3, 3.0, ABSENT), row(0.3, NAN)]], 1, ND)])
    assert ok(a, 1) == (-1, [ref([0.5, 0.3], [3.0, 3.0])])
    assert ref([0.5, 0.3], [3.0, 3.0]) != ref([0.5, 0.3], [0.0, 0.0])            # (and that eaf matters here)
    # an all-zero score: e = 0
    a, = driver([multi_query([[row(0.0), row(-0.0, 7.0)], [row(1.0), row(1.0)]], 2, ND)])
    assert ok(a, 2) == (-1, [F0, ref([1.0, 1.0], [0.25, 0.25])])

    # the span limit: max / min exactly 2^25 (2^17) is accepted, one ulp more is refused and names the score
    limit = 2.0 ** (25 if ND == 7 else 17)
    over = math.nextafter(limit, INF)
    a, b = driver([multi_query([[row(1.0), row(3.0)], [row(-1.0), row(limit)]], 2, ND),
                   multi_query([[row(1.0), row(3.0)], [row(0.0), row(-1.0), row(over)][1:]], 2, ND)])
    assert ok(a, 2) == (-1, [ref([1.0, 3.0], [0.25] * 2), ref([1.0, limit], [0.25] * 2)])
    assert refused(b) == ("span", 1, 0, 1.0, over)
    a, = driver([multi_query([[row(0.0), row(3.0 * over, 0.1, FILTERED), row(-3.0)]], 1, ND)])   # (zeros are not the minimum)
    assert refused(a) == ("span", 0, 0, 3.0, 3.0 * over)

    # non-finite numbers and kinds: the first in the order score, row
    a, b, c, d, e = driver([
        multi_query([[row(1.0), row(1.0), row(1.0)], [row(1.0), row(1.0), row(NAN)]], 2, ND),
        multi_query([[row(1.0), row(1.0, -INF, UNCOVERED), row(INF)], [row(NAN), row(1.0), row(1.0)]], 2, ND),
        multi_query([[row(1.0), row(1.0, 0.25, 5)]], 1, ND),
        multi_query([[row(1.0), row(1.0)], [row(1.0, 0.25, -1), row(NAN)]], 2, ND),
        multi_query([[row(1.0), row(2.0 ** 40), row(-INF)], [row(1.0, 0.25, 7), row(1.0), row(1.0)]], 2, ND)])
    assert refused(a)[:3] == ("beta", 1, 2)
    assert refused(b)[:3] == ("eaf", 0, 1)
    assert refused(c)[:3] == ("kind", 0, 1)
    assert refused(d)[:3] == ("kind", 1, 0)
    assert refused(e)[:3] == ("beta", 0, 2)       # (a row's refusal comes before its score's span)

    # |beta| = DBL_MAX: the bound is not finite -- no scale, named by the first such score, and no refusal
    a, = driver([multi_query([[row(1.0), row(2.0)], [row(DBL_MAX), row(0.0)], [row(-DBL_MAX), row(DBL_MAX)]], 3, ND)])
    assert ok(a, 3) == (1, [ref([1.0, 2.0], [0.25] * 2), F0, F0])
    a, = driver([multi_query([[row(DBL_MAX / 8.0, 0.0)]], 1, ND)])                    # (bound 5/8 DBL_MAX: finite, scaled)
    assert ok(a, 1) == (-1, [F0 - 1024])
