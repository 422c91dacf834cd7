"""nhdfit_headroom_limits on the MI355X (`pytest -m gpu`): the device's stage for every (template, node) against the reference's
stored answers on the synth and fixture inputs, against the host twin at sizes where indexing can go wrong (chunks, slabs, both
kernel forms, the cap), against plain nhdfit_headroom byte for byte, against nhdfit_explain where no replica fits, against the
independent oracle (its own run, the C oracle's stage on the node it leaves) on 4 096 nodes; the absence of side effects; shards
and the group entry; wide nodes; and the kernels' resources (hipcc only, no GPU).  Nothing here reads the reference tree: its
answers come from tests/golden/refanswers/tests.test_headroom_limit_reference.json."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import STAGES, Engine, GroupEngine
from nhd_amd.matcher import HipMatcher
from oracle import coracle
from tests import headroom_check as hc
from tests import headroom_limit_check as lc
from tests import test_headroom_gpu as hg
from tests import util
from tests.harness import headroom_limit_twin as twin
from tests.harness.headroom_limit_twin import HeadroomLimitHarnessEngine
from workload import refmodel, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, STOPPED, NOT_EVALUATED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED, pack.HEADROOM_NOT_EVALUATED
NO_WIDE = np.zeros(0, pack.WIDE)
FINAL_BYTES = 208                                    # sizeof(HeadroomFinal): one (template, node) of a slab


def _device(clock):
    return HipMatcher(device=0, clock=lambda: clock)


def histogram(stages):
    return np.stack([(stages == k).sum(1) for k in range(STAGES)], 1).astype(np.uint32)


def consistent(sums, counts, hist, stages, n):
    assert np.array_equal(hist, histogram(stages))
    assert np.array_equal(hist.sum(1) + sums["stopped"] + sums["not_evaluated"], np.full(len(sums), n))
    assert hist[:, lc.BUSY].sum() == 0
    assert np.array_equal(stages == lc.NONE, (counts & (STOPPED | NOT_EVALUATED)) != 0)


# ---- the stored reference answers --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_synth_stages_equal_the_reference(cfg):
    got, answers = lc.matcher_synth(_device, cfg)
    lc.same_where_not_stopped(answers, lc.stored(f"test_synth_configurations[{cfg}]"))
    lc.check_identities(got, hc.SYNTH_NODES)


@pytest.mark.gpu
@pytest.mark.parametrize("with_groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("golden", hc.IDS)
def test_golden_stages_equal_the_reference(golden, with_groups):
    got, answers = lc.matcher_golden(_device, hc.GOLDENS[hc.IDS.index(golden)], with_groups)
    want = lc.stored(f"test_goldens[{golden}-{'groups' if with_groups else 'plain'}]")
    lc.same_where_not_stopped(answers, want)
    lc.check_identities(got, len(want[0][0]))


@pytest.mark.gpu
def test_saturated_stages_equal_the_reference():
    got, answers = lc.matcher_synth(_device, 4, cap=2)
    lc.same_where_not_stopped(answers, lc.stored("test_saturation"))
    assert sum(h.limits["FITS"] for h in got) >= 10


# ---- the host twin at awkward sizes; plain headroom; nhdfit_explain ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n,cap,slab_templates", [(5, 3001, 512, None), (4, 2001, 2, None), (4, 130, 512, 1), (5, 37, 512, 3)],
                         ids=["c5-3001", "c4-2001-cap2", "c4-130-slab1", "c5-37-slab3"])
def test_device_equals_the_twin_plain_headroom_and_explain(cfg, n, cap, slab_templates):
    """Four templates of one to four groups (both kernel forms).  130 nodes: three chunks, the last with two live lanes; 37: less than
    one chunk.  slab_templates: the budget of final states holds that many templates, so the four take several slabs (4 and 2)."""
    specs = hg.four_templates(cfg)
    spec, pk, table, tops, reqs, eng = hg.engine_for(cfg, n, specs)
    pitch = (n + 63) // 64 * 64
    slab = None if slab_templates is None else slab_templates * pitch * FINAL_BYTES
    sums, counts, hist, stages = eng.headroom_limits(reqs, max_per_node=cap, per_node=True, _slab_bytes=slab)
    t_sums, t_counts, t_hist, t_stages = twin.headroom_limits(pk, table, NO_WIDE, reqs, max_per_node=cap)
    assert np.array_equal(counts, t_counts) and np.array_equal(stages, t_stages), np.argwhere(stages != t_stages)[:10].tolist()
    assert np.array_equal(hist, t_hist) and sums.tobytes() == t_sums.tobytes()
    consistent(sums, counts, hist, stages, n)
    assert sums["form"].tolist() == [pack.HEADROOM_FORM_WAVE] * 3 + [pack.HEADROOM_FORM_GENERIC]
    if slab is not None:                                                 # the answers do not depend on the budget
        s2, c2, h2, st2 = eng.headroom_limits(reqs, max_per_node=cap, per_node=True)
        assert np.array_equal(st2, stages) and np.array_equal(h2, hist) and np.array_equal(c2, counts) and s2.tobytes() == sums.tobytes()
    # counts only: the same histogram without the stage matrix
    s3, c3, h3, st3 = eng.headroom_limits(reqs, max_per_node=cap)
    assert c3 is None and st3 is None and np.array_equal(h3, hist) and s3.tobytes() == sums.tobytes()
    # plain headroom: byte for byte
    p_sums, p_counts = eng.headroom(reqs, max_per_node=cap, per_node=True)
    assert p_sums.tobytes() == sums.tobytes() and p_counts.tobytes() == counts.tobytes()
    # a candidate without room: nhdfit_explain's stage once nothing is busy
    _, ex = eng.explain(reqs, spec.clock_now + 1.0e6, per_node=True)
    zero = counts == 0
    assert np.array_equal(stages[zero], ex[zero]) and zero.sum() > 0
    k = counts & COUNT
    assert (k[stages == lc.FITS] == cap).all()
    if cap == 2:
        assert (stages == lc.FITS).sum() > 100 and ((k == 2) & (stages != lc.FITS)).sum() > 0
    if n > 1000:
        assert (k > 0).any(1).all() and len(np.unique(stages[k > 0])) >= 3
    eng.close()


# ---- the independent oracle ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_device_equals_the_independent_oracle():
    """Configuration 4's first 4 096 nodes, four templates: every pair the device reports with at least one replica against
    independent_limit (count, stopped flag and stage).  The pairs with 0 replicas are left to the C oracle's verdict with nothing
    busy (0 exactly where it says no) and to nhdfit_explain's stage (the test above); at least 200 pairs per template are compared.
    four_templates' own four-group template (PCI, three GPUs) has room on 109 of these nodes only, so the fourth template here is the
    three-group one plus the first group of the GPU-less two-group one, in the three-group template's map type: 1 354 nodes."""
    cfg, n = 4, 4096
    one, two, three, _ = hg.four_templates(cfg)
    specs = [one, two, three, dict(three, groups=[dict(g) for g in three["groups"]] + [dict(two["groups"][0])])]
    assert sorted(len(s["groups"]) for s in specs) == [1, 2, 3, 4]
    spec, pk, table, tops, reqs, eng = hg.engine_for(cfg, n, specs)
    sums, counts, hist, stages = eng.headroom_limits(reqs, max_per_node=lc.CAP, per_node=True)
    _, ex = eng.explain(reqs, spec.clock_now + 1.0e6, per_node=True)
    eng.close()
    consistent(sums, counts, hist, stages, n)
    k = counts & COUNT
    cl = coracle.Cluster.from_spec(spec)
    _, feas = cl.find(cl.pods_from_tops(tops, None), spec.clock_now + 1.0e6, threads=coracle.usable_cpus())
    assert np.array_equal(k > 0, feas.astype(bool))
    assert np.array_equal(stages[counts == 0], ex[counts == 0])
    todo = k > 0
    assert (todo.sum(1) >= 200).all(), todo.sum(1).tolist()
    want_k, want_st = lc.oracle_synth(cfg, n, specs, todo)
    assert np.array_equal(counts[todo].astype(np.int64), want_k[todo])
    assert np.array_equal(stages[todo], want_st[todo]), np.argwhere(todo & (stages != want_st))[:10].tolist()


# ---- no side effects ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_headroom_limits_leave_no_trace():
    specs = hg.four_templates(4)
    spec, pk, table, tops, reqs, eng = hg.engine_for(4, 5000, specs)
    now = spec.clock_now
    pods, groups = synth.make_pods(4, n_pods=300)
    batch = pk.digest_many([refmodel.make_topology(s) for s in pods], groups)
    eng.set_dictionary(pk)
    before = hg._planes(eng.download())
    s0, b0, m0 = eng.find(batch, now, want_bitmap=True, want_map=True)
    st0 = eng.stats()
    sums, counts, hist, stages = eng.headroom_limits(reqs, per_node=True)
    st1 = eng.stats()
    for f in ("launches", "fit_ms_total", "fit_ms_last", "digest_ms_last", "step_ms_last", "evals_last", "bytes_last", "small_finds", "batch_finds",
              "big_nic_steps_max"):
        assert getattr(st0, f) == getattr(st1, f), f
    for a, b in zip(before, hg._planes(eng.download())):
        assert a.tobytes() == b.tobytes()
    s1, b1, m1 = eng.find(batch, now, want_bitmap=True, want_map=True)
    assert np.array_equal(s0, s1) and np.array_equal(b0, b1) and m0.tobytes() == m1.tobytes()
    # steps in flight
    eng.stage(batch)
    for _ in range(3):
        eng.enqueue(now)
    s_in, c_in, h_in, st_in = eng.headroom_limits(reqs, per_node=True)
    f1 = eng.fetch(want_bitmap=True, want_map=True)
    assert np.array_equal(c_in, counts) and np.array_equal(s_in, sums) and np.array_equal(h_in, hist) and np.array_equal(st_in, stages)
    assert np.array_equal(f1[0], s0) and np.array_equal(f1[1], b0) and f1[2].tobytes() == m0.tobytes()
    eng.close()


# ---- shards and the group entry ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_shards_and_the_group_entry_equal_one_device():
    cfg, n = 4, 2001
    specs = hg.four_templates(cfg)
    spec, pk, table, tops, reqs, eng = hg.engine_for(cfg, n, specs)
    grp = GroupEngine([0, 0, 0], engine_factory=Engine)
    grp.set_dictionary(pk)
    grp.upload(table)
    assert len([1 for lo, hi in grp._bounds if hi > lo]) == 3
    keep = np.random.default_rng(9800).random(n) < 0.7
    for cand in (None, hg.mask_words(keep)):
        s1, c1, h1, st1 = eng.headroom_limits(reqs, cand=cand, per_node=True)
        s3, c3, h3, st3 = grp.headroom_limits(reqs, cand=cand, per_node=True)
        assert np.array_equal(c1, c3) and np.array_equal(s1, s3) and np.array_equal(h1, h3) and np.array_equal(st1, st3)
        consistent(s1, c1, h1, st1, n)
        if cand is not None:
            assert (st1[:, ~keep] == lc.NOT_CANDIDATE).all()
    grp.close()
    eng.close()
    spec = synth.make_cluster(3, n_nodes=700)
    nl = spec.build_nodes()
    tops = [refmodel.make_topology(s) for s in hg.four_templates(3)]
    a = HipMatcher(device=0, clock=lambda: spec.clock_now).HeadroomMany(nl, tops, per_node=True, limits=True)
    b = HipMatcher(devices=[0], clock=lambda: spec.clock_now).HeadroomMany(nl, tops, per_node=True, limits=True)
    for x, y in zip(a, b):
        assert x.error is None and y.error is None and x.replicas > 0
        assert x.limits == y.limits and np.array_equal(x.limit_stages, y.limit_stages) and x.limit_summary() == y.limit_summary()
        assert np.array_equal(x.per_node, y.per_node) and x.summary() == y.summary()


# ---- wide nodes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_wide_nodes_on_the_device():
    nl = util.mixed_cluster(9500, 120)
    rng = np.random.default_rng(95)
    tops = [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(12)]
    m = _device(util.CLOCK)
    dev = m.HeadroomMany(nl, tops, per_node=True, max_per_node=37, limits=True)
    tw = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomLimitHarnessEngine).HeadroomMany(nl, tops, per_node=True, max_per_node=37, limits=True)
    wide = np.array([nm in set(m.wide_nodes) for nm in nl])
    assert 10 < wide.sum() < len(nl) - 10
    lc.check_identities(dev, len(nl))
    for a, b in zip(dev, tw):
        assert np.array_equal(a.limit_stages, b.limit_stages) and a.limits == b.limits and np.array_equal(a.per_node, b.per_node)
        assert (a.limit_stages[wide] == pack.LIMIT_NONE).all() and ((a.flags[wide] & NOT_EVALUATED) != 0).all()
        assert (a.limit_stages[~wide] < STAGES).all()


# ---- resources (no GPU needed) -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_limit_kernel_resources(tmp_path):
    """k_limit_stage keeps its 640-byte views in LDS: no private segment, no vector register spilled (the compiler's own resource
    report; it spills 8 SGPRs into VGPR lanes, as k_explain spills 25).  The kernels named k_headroom are still exactly two."""
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
    ours = [v for k, v in usage.items() if "k_limit_stage" in k]
    assert len(ours) == 1, list(usage)
    assert ours[0]["ScratchSize"] == 0 and ours[0].get("VGPRs Spill", 0) == 0, ours
    assert 40 * 1024 <= ours[0]["LDS Size"] <= 48 * 1024, ours                  # the views: three blocks per CU
    assert len([k for k in usage if "k_headroom" in k]) == 2, list(usage)
