"""Build-time guard of the grouped dosage kernels (nps_groups.hip): the tally keeps a float64 sum and a count per group, the
accumulation four running sums and the sample's labels, and both are worth their read only while all of that lives in
registers.  The compiler's own resource remarks must report no scratch for any kernel of the unit and room for at least two
waves per SIMD for every tally (G = 2, 4, 8; float32 and DS16 elements) and accumulation instantiation.  Reads the remarks
only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "nimpress_amd", "csrc", "nps_groups.hip")


def test_every_kernel_is_scratch_free_and_the_streaming_ones_keep_two_waves(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    r = subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-Wno-unused-parameter",
                        "--cuda-device-only", "-c", SRC, "-o", str(tmp_path / "nps_groups.o"),
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
    # groups_tally_kernel<float, G> / <unsigned short, G>: ...If Li<G>E... / ...It Li<G>E...
    wanted = ["groups_tally_kernelI%sLi%dEE" % (elem, G) for elem in "ft" for G in (2, 4, 8)]
    wanted += ["groups_accumulate_kernelI%sEE" % elem for elem in "ft"]
    for w in wanted:
        hits = [v for k, v in seen.items() if w in k]
        assert len(hits) == 1, (w, sorted(seen))
        assert hits[0]["scratch"] == 0, (w, hits[0])
        assert hits[0]["occupancy"] >= 2, (w, hits[0])
    for w in ("groups_params_kernel", "groups_finish_kernel"):
        assert len([k for k in seen if w in k]) == 1, (w, sorted(seen))
    # no kernel of the unit spills
    assert len(seen) == len(wanted) + 2
    assert all(v.get("scratch") == 0 for v in seen.values()), seen
