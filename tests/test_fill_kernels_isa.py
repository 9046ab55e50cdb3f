"""Build-time guard for the strip layout's fill-and-tally kernels (nps_mx.hip: fill_gt2x_kernel, one instantiation per
source -- plain rows, PLINK .bed / .pgen rows, a NPS_FMT_GT2 cohort).  They move a cohort once and count its whole-row
tallies from registers and LDS; a spilled register would turn every tile into scratch traffic.  The compiler's own
resource remarks must say ScratchSize 0 and no spilled VGPRs for each of them (hipcc cross-compiles without a GPU)."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nimpress_amd", "csrc")

# template <int SRC> fill_gt2x_kernel: 0 plain rows, 1 .bed / .pgen rows, 2 NPS_FMT_GT2 cohort
KERNELS = ["fill_gt2x_kernelILi0E", "fill_gt2x_kernelILi1E", "fill_gt2x_kernelILi2E"]


def test_fill_and_tally_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-parameter",
                        "--cuda-device-only", "-c", os.path.join(CSRC, "nps_mx.hip"), "-o", str(tmp_path / "nps_mx.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, scratch, spills = None, {}, {}
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", ln)
        if m and name:
            scratch[name] = int(m.group(1))
        m = re.search(r"VGPRs Spill: (\d+)", ln)
        if m and name:
            spills[name] = int(m.group(1))
    for k in KERNELS:
        hits = [nm for nm in scratch if k in nm]
        assert hits, (k, sorted(scratch))
        for nm in hits:
            assert scratch[nm] == 0, (nm, scratch[nm])
            assert nm in spills and spills[nm] == 0, (nm, spills.get(nm))
    # the kernels they replace are gone with their last caller
    assert not [nm for nm in scratch if "rows_to_gt2x_kernel" in nm or "gt2_to_gt2x_kernel" in nm]
