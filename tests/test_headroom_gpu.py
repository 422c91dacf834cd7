"""nhdfit_headroom on the MI355X (`pytest -m gpu`): the device's entry for every (template, node) against the reference's stored
answers on the synth and fixture inputs, against the independent oracle (oracle/nhd_oracle.py, which travels) on every node of the
BASELINE shapes, against the host twin on further seeded clusters; its two consequences (the sum is what ScheduleBatch(apply=False)
places, a commit lowers its node's headroom by one); the absence of side effects; candidate mask, InitialNodeFilter, shards and the
group entry; both kernel forms; and k_headroom's resources (hipcc only, no GPU).  Nothing here reads the reference tree: its
answers come from tests/golden/refanswers/tests.test_headroom_reference.json."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import Engine, GroupEngine, winner_index
from nhd_amd.matcher import HipMatcher
from oracle import coracle
from oracle import nhd_oracle as O
from tests import headroom_check as hc
from tests import util
from tests.harness.headroom_twin import HeadroomHarnessEngine
from workload import planes, refmodel, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, STOPPED, NOT_EVALUATED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED, pack.HEADROOM_NOT_EVALUATED


def _device(clock):
    return HipMatcher(device=0, clock=lambda: clock)


def mask_words(keep, extra_high_bits=False):
    n = len(keep)
    bits = np.zeros(((n + 63) // 64) * 64, bool)
    bits[:n] = keep
    if extra_high_bits:
        bits[n:] = True
    return np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))


def check_sums(sums, counts, cap):
    """The summary records are the summaries of the entries."""
    k = counts & COUNT
    assert np.array_equal(sums["replicas"], k.sum(1, dtype=np.uint64))
    assert np.array_equal(sums["nodes_with_room"], (k > 0).sum(1))
    assert np.array_equal(sums["max_on_one_node"], k.max(1, initial=0))
    assert np.array_equal(sums["saturated"], ((k > 0) & (k >= cap)).sum(1))
    assert np.array_equal(sums["stopped"], ((counts & STOPPED) != 0).sum(1))
    assert np.array_equal(sums["not_evaluated"], ((counts & NOT_EVALUATED) != 0).sum(1))


# ---- the stored reference answers --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_synth_entries_equal_the_reference(cfg):
    got, entries = hc.matcher_synth(_device, cfg)
    assert entries == hc.stored(f"test_synth_configurations[{cfg}]")
    assert all(h.form == pack.HEADROOM_FORM_WAVE and h.not_evaluated == 0 for h in got)


@pytest.mark.gpu
@pytest.mark.parametrize("with_groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("golden", hc.IDS)
def test_golden_entries_equal_the_reference(golden, with_groups):
    got, entries = hc.matcher_golden(_device, hc.GOLDENS[hc.IDS.index(golden)], with_groups)
    assert entries == hc.stored(f"test_goldens[{golden}-{'groups' if with_groups else 'plain'}]")


# ---- BASELINE shapes against the independent oracle -------------------------------------------------------------------------------------
four_templates = hc.four_templates          # (tests/headroom_check.py: the CPU suite takes them from there)


def engine_for(cfg, n, specs, groups=None):
    spec = synth.make_cluster(cfg, n_nodes=n)
    tops = [refmodel.make_topology(s) for s in specs]
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many(tops, groups)
    pk.close_signatures()
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    return spec, pk, table, tops, reqs, eng


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n", [(2, 4096), (3, 16384), (4, 65536), (5, 32768)], ids=["c2-whole", "c3-whole", "c4-65536", "c5-shard"])
def test_baseline_shapes_equal_the_independent_oracle(cfg, n):
    """Config 2 whole, config 3 whole, config 4 at 65 536 nodes and a config 5 shard, four templates each (four_templates): EVERY node's
    entry - count and stopped flag - equals the independent oracle's loop (find_node on the one node + commit, busy window out of
    the way), spread over the box's cores by node ranges.  No node is sampled; a pair the C oracle's exhaustive per-node verdict
    (with nothing busy) rules out has 0 without the Python loop.  The three- and the four-group template report their forms."""
    specs = four_templates(cfg)
    assert sorted(len(s["groups"]) for s in specs) == [1, 2, 3, 4]
    spec, pk, table, tops, reqs, eng = engine_for(cfg, n, specs)
    sums, counts = eng.headroom(reqs, max_per_node=hc.CAP, per_node=True)
    eng.close()
    check_sums(sums, counts, hc.CAP)
    assert sums["form"].tolist() == [pack.HEADROOM_FORM_WAVE] * 3 + [pack.HEADROOM_FORM_GENERIC]
    assert (sums["not_evaluated"] == 0).all()
    cl = coracle.Cluster.from_spec(spec)
    _, feas = cl.find(cl.pods_from_tops(tops, None), spec.clock_now + 1.0e6, threads=coracle.usable_cpus())     # (nothing is busy by then)
    assert np.array_equal((counts & COUNT) > 0, feas.astype(bool))       # phase A is the oracle's verdict
    want = hc.oracle_synth(cfg, n, specs, maybe=feas.astype(bool))
    assert np.array_equal(counts.astype(np.int64), want), np.argwhere(counts != want)[:10].tolist()
    k = counts & COUNT
    assert k.max() >= 3 and (k > 0).any(1).all(), k.max(1).tolist()                     # (the inputs say something for every template)


# ---- a regression net: the host twin on further seeded clusters (the same shared headers - not parity) --------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(4))
def test_device_equals_the_host_twin_on_random_clusters(seed):
    """Heterogeneous random clusters (one- and two-socket nodes, odd switch layouts, half-used SMT pairs) and random pods of one to
    four groups, NUMA / PCI / invalid map types: device entries == host twin entries.  The twin is built from the same shared
    headers, so this is a net for the device-only parts (the wavefront forms, the launch), not evidence of parity."""
    rng = np.random.default_rng(9100 + seed)
    nl = util.random_cluster(9100 + seed, 300, occupancy=0.15)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(40)]
    dev = _device(util.CLOCK).HeadroomMany(nl, tops, per_node=True, max_per_node=64)
    twin = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomHarnessEngine).HeadroomMany(nl, tops, per_node=True, max_per_node=64)
    seen = 0
    for a, b in zip(dev, twin):
        assert a.error is None and b.error is None
        assert np.array_equal(a.per_node, b.per_node) and np.array_equal(a.flags, b.flags)
        assert (a.replicas, a.nodes_with_room, a.max_on_one_node, a.saturated, a.stopped, a.form) == \
               (b.replicas, b.nodes_with_room, b.max_on_one_node, b.saturated, b.stopped, b.form)
        seen += a.replicas
    assert seen > 100, seen


# ---- the two consequences ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [2, 4])
def test_sum_is_what_schedule_batch_places_and_a_commit_takes_one(cfg):
    """GPU-less templates on 3 000 nodes: `replicas` equals the placements ScheduleBatch(apply=False) makes from replicas + 1 copies
    (one copy stays unplaced); after ScheduleOne's commit (nhdfit_find_commit) the winner's headroom is one less and every other
    node's is unchanged."""
    n = 3000
    all_specs, _ = synth.make_pods(cfg, n_pods=256)
    specs = [s for s in all_specs if not any(g["gpus"] for g in s["groups"])][:3]
    assert len(specs) == 3
    spec, pk, table, tops, reqs, eng = engine_for(cfg, n, specs)
    now = spec.clock_now
    sums, counts = eng.headroom(reqs, per_node=True)
    assert (sums["saturated"] == 0).all() and (sums["replicas"] > n // 4).all()
    for p in range(len(specs)):
        total = int(sums["replicas"][p])
        node, _, _, status = eng.schedule_batch(np.repeat(reqs[p:p + 1], total + 1), now, pk, apply=False)
        assert int((node >= 0).sum()) == total and (status[node >= 0] == 0).all()
        placed = np.bincount(node[node >= 0] - eng.global_base, minlength=n)
        assert np.array_equal(placed, counts[p] & COUNT)                 # ... and node by node
    s2, c2 = eng.headroom(reqs, per_node=True)
    assert np.array_equal(c2, counts) and np.array_equal(s2, sums)       # (the batch was not applied)
    score, mp, place, done = eng.find_commit(reqs[0], now, now)
    assert score and done and int(place["status"]) == 0
    w = winner_index(score) - eng.global_base
    s3, c3 = eng.headroom(reqs[:1], per_node=True)
    want = counts[0].copy()
    assert want[w] & COUNT >= 1
    want[w] -= 1
    assert np.array_equal(c3[0], want) and int(s3["replicas"][0]) == int(sums["replicas"][0]) - 1
    eng.close()


# ---- no side effects ----------------------------------------------------------------------------------------------------------------------
def _planes(t):
    return [np.array(getattr(t, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]


@pytest.mark.gpu
def test_headroom_leaves_no_trace():
    """The mirror (nhdfit_download_nodes: all planes, busy times among them), nhdfit_get_stats and a following nhdfit_find are
    identical before and after; called with pipelined steps left in flight, the ledger drains them and their fetched results are
    what they are without the call in between."""
    specs = four_templates(4)
    spec, pk, table, tops, reqs, eng = engine_for(4, 5000, specs)
    now = spec.clock_now
    pods, groups = synth.make_pods(4, n_pods=300)
    batch = pk.digest_many([refmodel.make_topology(s) for s in pods], groups)
    eng.set_dictionary(pk)
    before = _planes(eng.download())
    s0, b0, m0 = eng.find(batch, now, want_bitmap=True, want_map=True)
    one0 = eng.find(batch[:1], now, want_bitmap=False, want_map=True)
    st0 = eng.stats()
    sums, counts = eng.headroom(reqs, per_node=True)
    st1 = eng.stats()
    for f in ("launches", "fit_ms_total", "fit_ms_last", "digest_ms_last", "step_ms_last", "evals_last", "bytes_last", "small_finds", "batch_finds",
              "big_nic_steps_max"):
        assert getattr(st0, f) == getattr(st1, f), f
    for a, b in zip(before, _planes(eng.download())):
        assert a.tobytes() == b.tobytes()
    s1, b1, m1 = eng.find(batch, now, want_bitmap=True, want_map=True)
    assert np.array_equal(s0, s1) and np.array_equal(b0, b1) and m0.tobytes() == m1.tobytes()
    one1 = eng.find(batch[:1], now, want_bitmap=False, want_map=True)
    assert np.array_equal(one0[0], one1[0]) and one0[2].tobytes() == one1[2].tobytes()
    # steps in flight
    eng.stage(batch)
    for _ in range(3):
        eng.enqueue(now)
    s_in, c_in = eng.headroom(reqs, per_node=True)
    f1 = eng.fetch(want_bitmap=True, want_map=True)
    assert np.array_equal(c_in, counts) and np.array_equal(s_in, sums)
    assert np.array_equal(f1[0], s0) and np.array_equal(f1[1], b0) and f1[2].tobytes() == m0.tobytes()
    eng.close()


# ---- candidate mask, InitialNodeFilter, shards, the group entry ------------------------------------------------------------------------------
@pytest.mark.gpu
def test_candidate_mask_and_node_groups():
    """3 001 nodes (not a multiple of 64) of config 5: outside the mask every entry is 0, inside it is the unmasked entry (bits past
    the last node change nothing); with the pods' node groups (NHDFIT_RF_INITIAL_FILTER) the nodes the oracle's InitialNodeFilter
    drops have 0 and the others their entry without the filter."""
    cfg, n = 5, 3001
    specs = four_templates(cfg)
    _, pgroups = synth.make_pods(cfg, n_pods=4)
    spec, pk, table, tops, reqs, eng = engine_for(cfg, n, specs)
    sums, counts = eng.headroom(reqs, per_node=True)
    assert (sums["nodes_with_room"] > 100).all()
    keep = np.random.default_rng(9300).random(n) < 0.6
    s1, c1 = eng.headroom(reqs, cand=mask_words(keep), per_node=True)
    assert np.array_equal(c1, np.where(keep[None, :], counts, 0))
    check_sums(s1, c1, 512)
    s2, c2 = eng.headroom(reqs, cand=mask_words(keep, extra_high_bits=True), per_node=True)
    assert np.array_equal(c2, c1) and np.array_equal(s2, s1)
    filtered = pk.digest_many(tops, pgroups)
    eng.set_dictionary(pk)
    assert (filtered["flags"] & pack.RF_INITIAL_FILTER != 0).all()
    s3, c3 = eng.headroom(filtered, per_node=True)
    nl = spec.build_nodes()
    names = list(nl)
    dropped = 0
    for p in range(len(specs)):
        kept = set(O.initial_node_filter(nl, pgroups[p]))
        inside = np.array([nm in kept for nm in names])
        assert np.array_equal(c3[p], np.where(inside, counts[p], 0)), p
        dropped += int((~inside).sum())
    assert dropped > n
    check_sums(s3, c3, 512)
    eng.close()


@pytest.mark.gpu
def test_three_shards_and_the_group_entry_equal_one_device():
    """GroupEngine over three contexts on device 0 (2 001 nodes): entries in global node order and summed records equal one
    context's, with and without a candidate mask; HipMatcher(devices=[0]) - the group entry, nhdfit_group_headroom - gives what
    HipMatcher(device=0) gives."""
    cfg, n = 4, 2001
    specs = four_templates(cfg)
    spec, pk, table, tops, reqs, eng = engine_for(cfg, n, specs)
    grp = GroupEngine([0, 0, 0], engine_factory=Engine)
    grp.set_dictionary(pk)
    grp.upload(table)
    assert len([1 for lo, hi in grp._bounds if hi > lo]) == 3
    keep = np.random.default_rng(9400).random(n) < 0.7
    for cand in (None, mask_words(keep)):
        s1, c1 = eng.headroom(reqs, cand=cand, per_node=True)
        s3, c3 = grp.headroom(reqs, cand=cand, per_node=True)
        assert np.array_equal(c1, c3) and np.array_equal(s1, s3)
        assert (s1["replicas"] > 0).all()
    grp.close()
    eng.close()
    spec = synth.make_cluster(3, n_nodes=700)
    nl = spec.build_nodes()
    tops = [refmodel.make_topology(s) for s in four_templates(3)]
    a = HipMatcher(device=0, clock=lambda: spec.clock_now).HeadroomMany(nl, tops, per_node=True)
    b = HipMatcher(devices=[0], clock=lambda: spec.clock_now).HeadroomMany(nl, tops, per_node=True)
    for x, y in zip(a, b):
        assert x.error is None and y.error is None and x.replicas > 0
        assert np.array_equal(x.per_node, y.per_node) and np.array_equal(x.flags, y.flags) and x.summary() == y.summary() and x.form == y.form


# ---- the cap; wide nodes --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_cap_and_wide_nodes_on_the_device():
    """A template that asks for nothing saturates every candidate at max_per_node; the wide nodes of a mixed cluster carry
    NOT_EVALUATED and no number, the ordinary ones what the host twin gives them."""
    nl = util.mixed_cluster(9500, 120)
    nothing = refmodel.make_topology(dict(map_type="NUMA", hugepages_gb=0, misc=0, misc_smt=False,
                                          groups=[dict(proc=0, helpers=0, rx=0.0, tx=0.0, proc_smt=False, helper_smt=False, gpus=[])]))
    rng = np.random.default_rng(95)
    tops = [nothing] + [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(12)]
    m = _device(util.CLOCK)
    dev = m.HeadroomMany(nl, tops, per_node=True, max_per_node=37)
    twin = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomHarnessEngine).HeadroomMany(nl, tops, per_node=True, max_per_node=37)
    wide = np.array([nm in set(m.wide_nodes) for nm in nl])
    assert 10 < wide.sum() < len(nl) - 10
    for a, b in zip(dev, twin):
        assert np.array_equal(a.per_node, b.per_node) and np.array_equal(a.flags, b.flags)
        assert a.not_evaluated == int(wide.sum()) and ((a.flags & NOT_EVALUATED) != 0).tolist() == wide.tolist() and (a.per_node[wide] == 0).all()
    h = dev[0]
    assert set(np.unique(h.per_node).tolist()) == {0, 37}                # (a node without a NIC on some NUMA node hosts no group: 0)
    full = int((h.per_node == 37).sum())
    assert full > 20 and h.saturated == full and h.replicas == 37 * full and h.max_on_one_node == 37
    assert all(x.saturated == int((x.per_node == 37).sum()) for x in dev)


# ---- resources (no GPU needed) -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_headroom_kernel_resources(tmp_path):
    """The wavefront instantiation of k_headroom has no private segment and spills no vector registers (the compiler's own resource
    report, in the style of test_kernel_resources.py); the generic set model's scratch arrays belong to the other instantiation."""
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
    ours = {k: v for k, v in usage.items() if "k_headroom" in k}
    assert len(ours) == 2, list(usage)
    wave = [v for k, v in ours.items() if "k_headroomILb0E" in k]
    assert len(wave) == 1 and wave[0]["ScratchSize"] == 0 and wave[0].get("VGPRs Spill", 0) == 0, wave
    assert all(v.get("VGPRs Spill", 0) == 0 for v in ours.values()), ours
