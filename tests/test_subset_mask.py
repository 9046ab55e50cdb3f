"""The sample mask of a subset run (nimpress_amd/csrc/nps_subset_mask.h), without a GPU: tests/native/subset_driver.cpp includes
that header alone and is compiled with g++ -fsanitize=address,undefined.  What the library uploads for a set -- the 1-bit
words, the unit words of the strip layout, n_kept and the gather index -- is checked against a loop over the keep bytes
written here."""
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 31, 32, 33, 2047, 2048, 2049, 4100]
PATTERNS = ["all", "first", "last", "alternate", "unit_dropped", "strip_dropped"]


def keep_bytes(n, pattern):
    """0 = drop, anything else = keep: the kept samples carry different non-zero bytes"""
    k = np.zeros(n, np.uint8)
    if pattern == "all":
        k[:] = 1
    elif pattern == "first":
        k[0] = 255
    elif pattern == "last":
        k[n - 1] = 2
    elif pattern == "alternate":
        k[::2] = 128
    elif pattern == "unit_dropped":      # the second unit of 32 samples (the only one, where there is no second)
        k[:] = 7
        u = 1 if n > 32 else 0
        k[32 * u:32 * u + 32] = 0
    elif pattern == "strip_dropped":     # the second strip of 2048 samples (the only one, where there is no second)
        k[:] = 1
        s = 1 if n > 2048 else 0
        k[2048 * s:2048 * s + 2048] = 0
    return k


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("subset") / "subset_driver")
    r = subprocess.run([gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "nimpress_amd", "csrc"), "-o", exe,
                        os.path.join(ROOT, "tests", "native", "subset_driver.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]

    def ask(keeps):
        lines = ["%d %s" % (k.size, k.tobytes().hex()) for k in keeps]
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        answers = out.stdout.splitlines()
        assert len(answers) == len(lines)
        res = []
        for a in answers:
            kept, bits, unit, prefix, pos = (part.split() for part in a.split("|"))
            res.append((int(kept[0]), [int(w, 16) for w in bits], [int(w, 16) for w in unit], [int(w, 16) for w in prefix],
                        [int(p) for p in pos]))
        return res
    return ask


@pytest.mark.parametrize("pattern", PATTERNS)
def test_mask_against_a_loop_over_the_bytes(driver, pattern):
    keeps = [keep_bytes(n, pattern) for n in SIZES]
    for n, keep, (n_kept, bits, unit, prefix, pos) in zip(SIZES, keeps, driver(keeps)):
        n_units = (n + 31) // 32
        want_bits, want_unit, want_pos, kept = [0] * n_units, [0] * n_units, [], 0
        want_prefix = []
        for i in range(n):
            if i % 32 == 0:
                want_prefix.append(kept)
            if keep[i] != 0:
                want_bits[i // 32] |= 1 << (i % 32)
                want_unit[i // 32] |= 3 << (2 * (i % 32))
                want_pos.append(kept)
                kept += 1
        assert n_kept == kept == int(np.count_nonzero(keep)), (n, pattern)
        assert unit == want_unit, (n, pattern)
        assert len(unit) == n_units
        # the 1-bit words and the prefix are padded to a multiple of four words: no bit, and every kept sample in front
        assert len(bits) == len(prefix) == (n_units + 3) // 4 * 4
        assert bits[:n_units] == want_bits and not any(bits[n_units:]), (n, pattern)
        assert prefix[:n_units] == want_prefix and all(p == kept for p in prefix[n_units:]), (n, pattern)
        # the gather index: kept sample i goes to its rank among the kept samples
        assert pos == want_pos == list(range(kept)), (n, pattern)
        # bits of samples beyond n are zero
        if n % 32:
            assert bits[n_units - 1] >> (n % 32) == 0
            assert unit[n_units - 1] >> (2 * (n % 32)) == 0
