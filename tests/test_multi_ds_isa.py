"""Build-time guard of the dosage multi-score accumulation (nps_multi_ds.hip): a lane holds 4 x S float64 accumulators, and
the kernel is worth its two reads only while they live in registers.  The compiler's own resource remarks must report no
scratch and room for at least two waves per SIMD for every instantiation (S = 1 .. 8, float32 and DS16 elements).  Reads
the remarks only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nimpress_amd", "csrc", "nps_multi_ds.hip")


def test_every_accumulation_instantiation_is_scratch_free(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-parameter",
                        "--cuda-device-only", "-c", SRC, "-o", str(tmp_path / "nps_multi_ds.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, {}
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in (("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
                         ("vgprs", r" VGPRs: (\d+)")):
            m = re.search(pat, ln)
            if m and name:
                seen[name][key] = int(m.group(1))
    # multi_ds_accumulate_kernel<S, float> / <S, unsigned short>: ...ILi<S>Ef... / ...ILi<S>Et...
    for S in range(1, 9):
        for elem in "ft":
            hits = [v for k, v in seen.items() if "multi_ds_accumulate_kernelILi%dE%sE" % (S, elem) in k]
            assert len(hits) == 1, (S, elem, sorted(seen))
            assert hits[0]["scratch"] == 0, (S, elem, hits[0])
            assert hits[0]["occupancy"] >= 2, (S, elem, hits[0])
    # the other kernels of the file spill nothing either
    assert all(v.get("scratch") == 0 for v in seen.values()), seen
