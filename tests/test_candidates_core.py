"""k_cand_list's pick (nhd_amd/csrc/candidates_kernel.h cand_pick_wave, cut out of the header and run on emulated lanes -
tests/harness/candidates_pick_emul.cpp) against a scalar statement of the selection order; the resources of the kernel's two
instantiations (hipcc only, no GPU); and the C-ABI's refusals and record sizes."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nhd_amd import _lib, pack
from tests.harness import candidates_twin as ct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREF = 0x80000000


def block_records(blocks, k):
    """What the scan posts per block: `blocks` = per block the feasible nodes in index order as (index, preferred)."""
    return [([i | (PREF if p else 0) for i, p in b][:k], [i for i, p in b if p][:k]) for b in blocks]


def scalar_pick(blocks, k):
    """The selection order in ten lines: the preferred nodes in index order, then the others in index order, cut at k."""
    nodes = [x for b in blocks for x in b]
    assert [i for i, _ in nodes] == sorted(i for i, _ in nodes)
    first = [i | PREF for i, p in nodes if p]
    rest = [i for i, p in nodes if not p]
    return (first + rest)[:k]


def random_blocks(rng, nb, density, pref_share):
    blocks, base = [], 0
    for _ in range(nb):
        size = int(rng.integers(1, 300))
        hit = np.flatnonzero(rng.random(size) < density)
        blocks.append([(base + int(i), bool(rng.random() < pref_share)) for i in hit])
        base += size
    return blocks


@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_pick_equals_the_scalar_statement_on_random_records(k):
    rng = np.random.default_rng(1400 + k)
    seen_short, seen_full = 0, 0
    for nb in range(1, 10):
        for density, pref_share in ((0.0, 0.5), (0.02, 0.3), (0.3, 0.05), (0.9, 0.5), (0.5, 0.0), (0.5, 1.0)):
            blocks = random_blocks(rng, nb, density, pref_share)
            want = scalar_pick(blocks, k)
            assert ct.pick(block_records(blocks, k), k).tolist() == want, (nb, density, pref_share)
            seen_short += len(want) < k
            seen_full += len(want) == k
    assert seen_short and seen_full


@pytest.mark.parametrize("k", [1, 2, 7, 64])
def test_pick_on_the_named_cases(k):
    gpu = lambda lo, hi: [(i, False) for i in range(lo, hi)]      # noqa: E731
    cases = {
        # the preferred nodes run out mid-list while a feasible GPU node has a lower index than all of them
        "preferred run out": [gpu(0, 3) + [(5, True)], [(70, True)] + gpu(71, 140)],
        # a block with no hit between two with hits, and one at either end
        "empty blocks": [[], [(9, False), (11, True)], [], [(200, True), (201, False)], []],
        # more than K hits in the first block (K = 64: 100 of them), the preferred ones beyond its first K
        "first block overflows": [gpu(0, 100) + [(100, True), (101, True)], [(300, True)] + gpu(301, 310)],
        # every hit preferred, more than K of them in each block
        "all preferred": [[(i, True) for i in range(0, 130, 2)], [(i, True) for i in range(200, 330, 2)]],
        "nothing": [[], [], []],
    }
    for name, blocks in cases.items():
        assert ct.pick(block_records(blocks, k), k).tolist() == scalar_pick(blocks, k), name


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_candidates_kernel_resources(tmp_path):
    """Exactly two instantiations of k_cand_list; the wavefront one (G4 = false) has no private segment and spills no vector
    registers (the compiler's own resource report): the generic set model's scratch arrays belong to the other."""
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
    ours = {k: v for k, v in usage.items() if "k_cand_list" in k}
    assert len(ours) == 2, list(usage)
    wave = [v for k, v in ours.items() if "k_cand_listILb0E" in k]
    assert len(wave) == 1 and wave[0]["ScratchSize"] == 0 and wave[0].get("VGPRs Spill", 0) == 0, wave


def test_refusals_without_a_context_and_record_sizes(tmp_path):
    """A NULL context or group is NHDFIT_E_INVAL whatever K says (K = 0 and 65 on a live context: tests/test_candidates_gpu.py); the
    two records are 32 bytes in the header - as a C compiler lays them out - and in pack's numpy mirrors, field by field."""
    lib = _lib.load()
    buf = (ctypes.c_uint8 * 4096)()
    for k in (0, 1, 64, 65):
        assert lib.nhdfit_candidates(None, buf, 1, 0.0, None, k, buf, buf) == -1
        assert lib.nhdfit_group_candidates(None, buf, 1, 0.0, None, k, buf, buf, None) == -1
    assert pack.CANDIDATE.itemsize == 32 and pack.CANDIDATES_SUM.itemsize == 32 and pack.CANDIDATES_MAX_K == 64
    fields = [("nhdfit_candidate", pack.CANDIDATE, ("score", "map", "reserved")),
              ("nhdfit_candidates_sum", pack.CANDIDATES_SUM, ("feasible", "preferred", "returned", "not_evaluated", "form", "reserved"))]
    text = ['#include <stddef.h>', '#include "nhdfit.h"']
    for rec, dt, names in fields:
        text.append(f"_Static_assert(sizeof({rec}) == {dt.itemsize}, \"{rec}\");")
        text += [f"_Static_assert(offsetof({rec}, {f}) == {dt.fields[f][1]}, \"{rec}.{f}\");" for f in names]
    text.append("_Static_assert(NHDFIT_CANDIDATES_MAX_K == 64 && NHDFIT_ABI_VERSION == 9, \"limits\");")
    src = tmp_path / "sizes.c"
    src.write_text("\n".join(text) + "\n")
    res = subprocess.run(["gcc", "-std=c11", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
