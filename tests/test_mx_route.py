"""The strip path's host policy (nimpress_amd/csrc/nps_mx_route.h), without a GPU: which route nps_score_cohort_def takes for
a NPS_FMT_GT2X run, the plan it runs with, and the given-tallies plan's team choice against its Python copy in
tests/exact_reference.py.  tests/native/route_driver.cpp includes that header alone and is compiled with plain g++: the
policy needs neither HIP nor a device."""
import os
import shutil
import subprocess

import pytest

import exact_reference as er

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AUTO, TWOPASS, FUSED = 0, 1, 2   # NPS_MODE_*, include/nps.h
CUS = 256


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("route") / "route_driver")
    r = subprocess.run([gxx, "-std=c++17", "-Wall", "-Wextra", "-I", os.path.join(ROOT, "nimpress_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "route_driver.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def ask(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        return [a.split() for a in answers]
    return ask


def route(driver, n, m, rows, row0=0, valid=0, asked=0, expect=0, mode=AUTO, cus=CUS):
    a, = driver(["route %d %d %d %d %d %d %d %d %d" % (cus, n, m, rows, row0, valid, asked, expect, mode)])
    keys = ("ok", "refused", "route", "count_first", "given", "P", "Q", "grid_P", "grid_nu_last", "grid_U")
    return {k: (v if k == "route" else int(v)) for k, v in zip(keys, a)}


# (n samples, m, cohort rows, row0, valid, asked, expect, mode) -> (route, count_cohort_first), at 256 compute units
ROUTES = [
    # 70 000 samples: 35 strips, 7 row teams
    ((70_000, 1500, 1500, 0, 0, 0, 0, AUTO), ("InPass", 0)),
    ((70_000, 1500, 1500, 0, 1, 0, 0, AUTO), ("InPass", 0)),
    ((70_000, 1500, 1500, 0, 1, 1, 0, AUTO), ("GivenKept", 0)),
    # 300 001 samples: 147 strips, one team, the grid does not cover the chip
    ((300_001, 1024, 1024, 0, 0, 0, 0, AUTO), ("InPassKeep", 0)),
    ((300_001, 1023, 1023, 0, 0, 0, 0, AUTO), ("InPass", 0)),
    ((300_001, 16384, 65536, 0, 0, 0, 0, AUTO), ("GivenKept", 1)),
    ((300_001, 16384, 65537, 0, 0, 0, 0, AUTO), ("InPass", 0)),
    ((300_001, 16383, 65532, 0, 0, 0, 0, AUTO), ("InPass", 0)),
    ((300_001, 300, 300, 0, 1, 0, 0, AUTO), ("GivenKept", 0)),
    ((300_001, 300, 300, 0, 1, 0, 0, FUSED), ("InPass", 0)),
    # the step from two row teams to one
    ((262_144, 2048, 2048, 0, 0, 0, 0, AUTO), ("InPass", 0)),
    ((262_145, 2048, 2048, 0, 0, 0, 0, AUTO), ("InPassKeep", 0)),
    # nine tenths of the chip: 230 strips do not cover it, 231 do
    ((471_040, 1024, 1024, 0, 0, 0, 0, AUTO), ("InPassKeep", 0)),
    ((471_041, 2048, 2048, 0, 0, 0, 0, AUTO), ("InPass", 0)),
    ((471_041, 2048, 2048, 0, 0, 0, 2, AUTO), ("InPassKeep", 0)),
    ((500_000, 16384, 65536, 0, 0, 0, 2, AUTO), ("InPass", 0)),
    # the last resident grid (255 strips) and the first shape without one
    ((522_240, 2048, 2048, 0, 0, 0, 0, AUTO), ("InPass", 0)),
    ((522_241, 2048, 2048, 0, 0, 0, 0, AUTO), ("GivenKept", 1)),
    ((522_241, 1000, 4001, 0, 0, 0, 0, AUTO), ("GivenTallied", 0)),
    # NPS_MODE_TWOPASS never uses kept tallies
    ((70_000, 1500, 1500, 0, 1, 1, 0, TWOPASS), ("GivenTallied", 0)),
    ((300_001, 300, 300, 0, 1, 1, 0, TWOPASS), ("GivenTallied", 0)),
]


@pytest.mark.parametrize("query,want", ROUTES)
def test_route(driver, query, want):
    r = route(driver, *query)
    print(query, "->", r)
    assert r["ok"] == 1 and r["refused"] == 0
    assert (r["route"], r["count_first"]) == want
    # the plan is the route's: the given-tallies kernel's for the two Given* routes, a resident grid otherwise
    assert r["given"] == (1 if want[0].startswith("Given") else 0)
    assert r["grid_U"] == 64 or (r["grid_U"] == 62 and not r["given"] and r["Q"] == 1)


def test_strips_and_teams_of_the_table(driver):
    for n, P, Q in [(70_000, 35, 7), (300_001, 147, 1), (262_144, 128, 2), (262_145, 129, 1), (471_040, 230, 1),
                    (471_041, 231, 1), (522_240, 255, 1)]:
        r = route(driver, n, 2048, 2048, mode=FUSED)
        assert (r["P"], r["Q"], r["given"], r["refused"]) == (P, Q, 0, 0), (n, r)


def test_fused_mode_is_refused_beyond_the_resident_grid(driver):
    r = route(driver, 522_241, 2048, 2048, mode=FUSED)
    assert r["ok"] == 1 and r["refused"] == 1 and r["route"] == "InPass" and r["P"] == 256


def test_shape_beyond_the_kernels_is_not_ok(driver):
    for mode in (AUTO, TWOPASS, FUSED):
        assert route(driver, 2 ** 27, 2048, 2048, mode=mode)["ok"] == 0
    assert route(driver, 65535 * 2048, 2048, 2048)["ok"] == 1   # (the most strips a grid dimension holds)


def test_strips_of_62_units_are_resolved_in_the_plan(driver):
    """500 000 samples = 15 625 units: 245 strips of the layout, 253 of 62 units, the last of 15 625 - 252 x 62 = 1"""
    r = route(driver, 500_000, 65536, 65536, expect=2)
    assert r["route"] == "InPassKeep"
    assert (r["P"], r["Q"], r["grid_P"], r["grid_nu_last"], r["grid_U"]) == (245, 1, 253, 1, 62)
    (ok, given, P, Q, gP, gnu, gU), = driver(["plan %d 500000 65536 1" % CUS])   # given tallies: the layout's strips
    assert (int(ok), int(given), int(P), int(gP), int(gnu), int(gU)) == (1, 1, 245, 245, 15625 - 244 * 64, 64)


@pytest.mark.parametrize("cus", [256, 304])
def test_team_choice_is_the_reference_copys(driver, cus):
    """exact_reference.given_teams is a copy of the given-tallies plan's team choice: held to mx_plan_for at every strip count"""
    n_sb = 4096   # (more superblocks than any team count: the choice itself, not its clamp)
    ans = driver(["plan %d %d %d 1" % (cus, 2048 * P, 128 * n_sb) for P in range(1, 601)])
    for P, a in zip(range(1, 601), ans):
        assert int(a[0]) == 1 and int(a[1]) == 1 and int(a[2]) == P
        assert int(a[3]) == er.given_teams(P, cus, n_sb), (cus, P)
    if cus == 256:
        assert int(ans[146][3]) == 12   # 147 strips: the example in mx_plan_for's own comment
    # the clamp to the run's superblocks
    (_, _, _, q, *_), = driver(["plan %d 300001 300 1" % cus])
    assert int(q) == er.given_teams(147, cus, 3) == 3
