"""Build-time guard of the FORMAT/PL decode (nps_pl.hip): a thread walks its sample's likelihoods in LDS with no array of
its own, so the compiler's resource remarks must report no scratch and no spilled register for the three instantiations
(int8, int16, int32).  Reads the remarks only: resource usage, nothing else.

Run as a script (python tests/test_pl_isa.py) it writes the figures to profiles/pl_kernel_resources.txt."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nimpress_amd", "csrc", "nps_pl.hip")
KEYS = (("sgprs", r" SGPRs: (\d+)"), ("vgprs", r" VGPRs: (\d+)"), ("agprs", r" AGPRs: (\d+)"),
        ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"), ("sgpr_spill", r"SGPRs Spill: (\d+)"),
        ("vgpr_spill", r"VGPRs Spill: (\d+)"), ("occupancy", r"Occupancy \[waves/SIMD\]: (\d+)"),
        ("lds", r"LDS Size \[bytes/block\]: (\d+)"))
ELEMS = {"a": "int8_t", "s": "int16_t", "i": "int32_t"}      # Itanium mangling of the template argument


def kernel_resources(workdir):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-parameter",
                        "--cuda-device-only", "-c", SRC, "-o", os.path.join(workdir, "nps_pl.o"),
                        "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    name, seen = None, {}
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            seen[name] = {}
        for key, pat in KEYS:
            m = re.search(pat, ln)
            if m and name:
                seen[name][key] = int(m.group(1))
    return seen


def decode_instances(seen):
    out = {}
    for code, elem in ELEMS.items():
        hits = [v for k, v in seen.items() if "decode_pl_kernelI%sE" % code in k]
        assert len(hits) == 1, (elem, sorted(seen))
        out[elem] = hits[0]
    return out


def test_decode_pl_kernels_use_no_scratch(tmp_path):
    seen = kernel_resources(str(tmp_path))
    if seen is None:
        pytest.skip("no hipcc")
    for elem, res in decode_instances(seen).items():
        assert res["scratch"] == 0, (elem, res)
        assert res.get("sgpr_spill", 0) == 0 and res.get("vgpr_spill", 0) == 0, (elem, res)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        inst = decode_instances(kernel_resources(d))
    lines = ["decode_pl_kernel<T> (nimpress_amd/csrc/nps_pl.hip), gfx950, -O3 -ffp-contract=off: the compiler's resource remarks",
             "(-Rpass-analysis=kernel-resource-usage).  LDS is dynamic: 2048 B of likelihoods + 256 x G x sizeof(T) B of samples.", ""]
    for elem, res in inst.items():
        lines.append("%-8s %s" % (elem, "  ".join("%s=%d" % (k, res[k]) for k, _ in KEYS if k in res)))
    path = os.path.join(ROOT, "profiles", "pl_kernel_resources.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    sys.stdout.write("\n".join(lines) + "\n")
