"""The labels of a sample partition (nimpress_amd/csrc/nps_group_labels.h), without a GPU: tests/native/group_labels_driver.cpp
includes that header alone and is compiled with g++ -fsanitize=address,undefined.  What the library uploads for a groups
object -- the group sizes, the label bytes padded with 255 to a multiple of 64, one presence byte per 256 samples -- and what
it refuses are checked against loops over the label bytes written here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 3, 4, 5, 255, 256, 257, 1027]
PATTERNS = ["interleaved", "contiguous", "single_first_last", "some_none"]
NONE = 255


def labels(n, G, pattern):
    """uint8[n] with every group 0 .. G - 1 present, or None where n samples cannot hold the pattern"""
    if n < G:
        return None
    i = np.arange(n)
    if pattern == "interleaved":
        return (i % G).astype(np.uint8)
    if pattern == "contiguous":                 # blocks of nearly equal length: borders at no particular multiple
        return (i * G // n).astype(np.uint8)
    if pattern == "single_first_last":          # group 0 is sample 0 alone, group G - 1 the last sample alone
        if G < 3 or n < G:
            return None
        lab = (1 + (i - 1) * (G - 2) // max(n - 2, 1)).astype(np.uint8)
        lab[0], lab[n - 1] = 0, G - 1
        return lab
    if pattern == "some_none":                  # every seventh sample in no group, the others interleaved
        lab = (i % G).astype(np.uint8)
        lab[(i % 7 == 3) & (i >= G)] = NONE
        return lab
    raise ValueError(pattern)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("groups") / "group_labels_driver")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "nimpress_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "group_labels_driver.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def ask(queries):
        lines = ["%d %d %s" % (lab.size, G, lab.tobytes().hex()) for lab, G in queries]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        res = []
        for a in answers:
            err, size, lab, pres = (part.split() for part in a.split("|"))
            res.append(([int(x) for x in err], [int(x) for x in size], [int(x, 16) for x in lab], [int(x, 16) for x in pres]))
        return res
    return ask


@pytest.mark.parametrize("pattern", PATTERNS)
def test_labels_against_a_loop_over_the_bytes(driver, pattern):
    queries = [(labels(n, G, pattern), G) for n in SIZES for G in (1, 2, 3, 5, 8) if labels(n, G, pattern) is not None]
    assert len(queries) >= 8
    for (lab, G), (err, size, padded, pres) in zip(queries, driver(queries)):
        n = lab.size
        assert err[0] == 0, (n, G, pattern, err)
        want_size, want_pres = [0] * G, [0] * ((n + 255) // 256)
        for i in range(n):
            if lab[i] != NONE:
                want_size[lab[i]] += 1
                want_pres[i // 256] |= 1 << int(lab[i])
        assert size == want_size, (n, G, pattern)
        # the label bytes as given, then 255 up to the rows' padding: a multiple of 64 samples
        assert len(padded) == (n + 63) // 64 * 64
        assert padded[:n] == [int(x) for x in lab] and all(b == NONE for b in padded[n:]), (n, G, pattern)
        # one presence byte per 256 samples, zero bytes up to a multiple of four
        assert len(pres) == ((n + 255) // 256 + 3) // 4 * 4
        assert pres[:len(want_pres)] == want_pres and not any(pres[len(want_pres):]), (n, G, pattern)


def test_what_is_refused_and_who_is_named(driver):
    bad = np.array([0, 1, 2, 1, 0], np.uint8)           # sample 2 carries label 2 of 2 groups
    none = np.full(300, NONE, np.uint8)
    empty = np.array([0, 2, 0, NONE, 2], np.uint8)      # group 1 of 3 has nobody
    far = (np.arange(600) % 2).astype(np.uint8)
    far[599] = 254                                      # the first bad sample is the last one
    got = driver([(bad, 2), (none, 1), (empty, 3), (far, 2)])
    assert got[0][0] == [1, 2, 0]
    assert got[1][0][0] == 2
    assert got[2][0] == [3, 0, 1]
    assert got[3][0] == [1, 599, 0]
    assert all(g[1:] == ([], [], []) for g in got)
