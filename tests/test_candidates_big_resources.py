"""Build-time guard for nhdfit_candidates_big's three kernels (nhd_amd/csrc/big_candidates_kernel.h): the compiler's own resource report
of the gfx950 code object, as tests/test_candidates_general_resources.py reads it (hipcc cross-compiles without a GPU), with k_big_map's
beside it in the same object - k_big_cand_map runs the same routines.  No instruction is inspected.

k_big_cand_map has four instantiations: sharing or not, and the wavefront form of the mapping (wide_map_wave's lines, inlined) or the
one-thread form (wide_map, inlined): no device function of its own stands between a kernel and the report, so each kernel's figures
are all of its code's."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_big_candidates_kernel_resources(tmp_path):
    """The three new kernels are in the gfx950 code object, scan and pick in two instantiations (ENABLE_SHARING arithmetic or not), map
    in four (and the wavefront or the one-thread form); none spills a VGPR; no k_big_cand_map has more VGPRs, a larger private segment
    or more spilled SGPRs than k_big_map beside it."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "nhd_amd", "csrc", "nhdfit.hip")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--cuda-device-only", "-c", src,
                          "-o", str(tmp_path / "dev.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    usage, name = {}, None
    for line in res.stderr.splitlines():
        mt = re.search(r"Function Name: (\S+)", line)
        if mt:
            name = mt.group(1)
            usage[name] = {}
            continue
        mt = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if mt and name:
            usage[name][mt.group(1).strip()] = int(mt.group(2))
    one = lambda part: [v for k, v in usage.items() if part in k]      # noqa: E731
    big_map = [v for k, v in usage.items() if "k_big_map" in k]
    scan, pick, mapk = one("k_big_cand_scan"), one("k_big_cand_pick"), one("k_big_cand_map")
    assert len(big_map) == 1 and len(scan) == 2 and len(pick) == 2 and len(mapk) == 4, list(usage)
    print({"k_big_map": big_map[0], "k_big_cand_scan": scan, "k_big_cand_pick": pick, "k_big_cand_map": mapk})
    for ours in scan + pick + mapk:
        assert ours.get("VGPRs Spill", 0) == 0, ours
    for ours in mapk:
        for field in ("VGPRs", "ScratchSize", "SGPRs Spill"):
            assert ours.get(field, 0) <= big_map[0].get(field, 0), (field, ours, big_map)
