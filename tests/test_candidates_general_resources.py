"""Build-time guard for nhdfit_candidates_general's two kernels (nhd_amd/csrc/wide_candidates_kernel.h): the compiler's own resource
report of the gfx950 code object, as tests/test_kernel_resources.py reads it (hipcc cross-compiles without a GPU), beside k_wide_room's
in the same object - they run the same routines."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_wide_candidates_kernel_resources(tmp_path):
    """Both new kernels are in the gfx950 code object, each in its two instantiations (ENABLE_SHARING arithmetic or not);
    k_wide_cand_map's static LDS is at most 42 KB (three blocks to a CU); none has more VGPRs, more spilled SGPRs or VGPRs, or a larger
    private segment than k_wide_room beside it (same routines)."""
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
    room, scan, mapk = one("k_wide_room"), one("k_wide_cand_scan"), one("k_wide_cand_map")
    assert len(room) == 1 and len(scan) == 2 and len(mapk) == 2, list(usage)
    print({"k_wide_room": room[0], "k_wide_cand_scan": scan, "k_wide_cand_map": mapk})
    assert all(v["LDS Size"] <= 42 * 1024 for v in mapk), mapk
    for ours in scan + mapk:
        for field in ("VGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize"):
            assert ours.get(field, 0) <= room[0].get(field, 0), (field, ours, room)
