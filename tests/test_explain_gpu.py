"""nhdfit_explain on the MI355X: the device's stage for every (pod, node) against the reference's stored stages on the
golden fixtures, its counts against nhdfit_find's verdict bitmap and a vectorised host computation at BASELINE shapes, its counts
and per-node stages against the C stage oracle (oracle_explain) on random, wide, big-pod, masked and sharded inputs, the
absence of side effects and the group entry (`pytest -m gpu`); and k_explain's resources (hipcc only, no GPU).  Nothing here reads the
reference tree: its answers come from tests/golden/refanswers/tests.test_explain_reference.json."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import Engine, GroupEngine
from nhd_amd.matcher import STAGES, HipMatcher
from oracle import coracle
from oracle import nhd_oracle as O
from tests import explain_check, util
from tests.test_big_core import big_spec
from workload import planes, refmodel, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITS = STAGES.index("FITS")
LATE = [STAGES.index(s) for s in ("NIC", "PCI", "NUMA")]
WHOLE_MATRIX_CPUS = 8             # the whole-matrix oracle comparisons below skip, visibly, on hosts with fewer usable CPUs


def unpack_bitmap(bm, n):
    """chunk-major [chunks][P] words -> [P][n] 0/1"""
    chunks, P = bm.shape
    bits = np.unpackbits(bm.view(np.uint8).reshape(chunks, P, 8), axis=2, bitorder="little")
    return bits.transpose(1, 0, 2).reshape(P, chunks * 64)[:, :n]


@pytest.mark.gpu
@pytest.mark.parametrize("golden", explain_check.IDS)
def test_golden_stages_equal_the_reference(golden):
    path = explain_check.GOLDENS[explain_check.IDS.index(golden)]
    got = explain_check.explain(path, lambda clock: HipMatcher(device=0, clock=lambda: clock))
    assert got == explain_check.stored(golden)


def _baseline(cfg, n, P):
    spec = synth.make_cluster(cfg, n_nodes=n)
    pods, groups = synth.make_pods(cfg, n_pods=P)
    tops = [refmodel.make_topology(s) for s in pods]
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many(tops, groups)
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    return spec, table, reqs, eng


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n,P", [(4, 65536, 4096), (5, 32768, 2048), (3, 4000, 300), (2, 700, 120)],
                         ids=["c4-65536x4096", "c5-shard", "c3-small", "c2-small"])
def test_counts_against_the_verdict_bitmap(cfg, n, P):
    """Every pod's counts sum to the node count; FITS is the popcount of its column of nhdfit_find's bitmap; stages 0..5 equal the
    host computation (and, at the small shapes, the per-node stages 6..8 are what is left over: not FITS, not 0..5).  At the small
    shapes every count and every per-node stage also equals the C stage oracle's; the full-size shapes have their own test of that,
    test_counts_equal_the_stage_oracle."""
    spec, table, reqs, eng = _baseline(cfg, n, P)
    now = spec.clock_now
    score, bm, _ = eng.find(reqs, now, want_map=False)
    counts, stages = eng.explain(reqs, now, per_node=n * P <= 1 << 22)
    assert counts.shape == (P, len(STAGES)) and (counts.sum(1) == n).all()
    feas = unpack_bitmap(bm, n)
    assert np.array_equal(counts[:, FITS], feas.sum(1))
    host = explain_check.host_stages_upto_cpu(table, reqs, now)
    for k in range(6):
        assert np.array_equal(counts[:, k], (host == k).sum(1)), k
    assert np.array_equal(counts[:, 6:].sum(1), (host == 6).sum(1))
    if stages is not None:
        assert np.array_equal(stages == FITS, feas.astype(bool))
        assert np.array_equal(np.minimum(stages, 6), host)
        assert np.array_equal(counts, np.stack([(stages == k).sum(1) for k in range(len(STAGES))], 1))
    if n * P <= 1 << 22:                 # the stage oracle on every pair (the full-size shapes: test_counts_equal_the_stage_oracle)
        cl = coracle.Cluster.from_spec(spec)
        want_c, want_s = cl.explain(oracle_pods(cl, cfg, P), now, per_node=True, threads=coracle.usable_cpus())
        assert np.array_equal(counts, want_c)
        assert np.array_equal(stages, want_s)
    eng.close()


def oracle_pods(cl, cfg, P):
    specs, groups = synth.make_pods(cfg, n_pods=P)
    return cl.pods_from_tops([refmodel.make_topology(s) for s in specs], groups)


def late_stages_seen(counts, which=LATE):
    """Teeth: the inputs reach NIC, PCI and NUMA (`which`), so a swap of any two of them cannot pass."""
    tot = np.asarray(counts).reshape(-1, len(STAGES)).sum(0)
    assert (tot[which] > 0).all(), tot.tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("cfg,n,P", [(4, 65536, 4096), (5, 32768, 2048)], ids=["c4-65536x4096", "c5-shard"])
def test_counts_equal_the_stage_oracle(cfg, n, P):
    """The full-size shapes of test_counts_against_the_verdict_bitmap: all ten count columns of every pod equal the C stage
    oracle's (oracle_explain) over every one of the n x P pairs."""
    if coracle.usable_cpus() < WHOLE_MATRIX_CPUS:
        pytest.skip(f"fewer than {WHOLE_MATRIX_CPUS} usable CPUs: the whole-matrix stage oracle would take too long")
    spec, table, reqs, eng = _baseline(cfg, n, P)
    counts, _ = eng.explain(reqs, spec.clock_now)
    eng.close()
    cl = coracle.Cluster.from_spec(spec)
    want, _ = cl.explain(oracle_pods(cl, cfg, P), spec.clock_now, threads=coracle.usable_cpus())
    assert np.array_equal(counts, want)
    late_stages_seen(counts, LATE if cfg == 4 else LATE[1:])        # (config 5's eight NICs per NUMA node never run short)


def oracle_stages(nl, tops, now, groups=None, cand=None):
    cl = coracle.Cluster.from_nodes(nl)
    return cl.explain(cl.pods_from_tops(tops, groups), now, cand=cand, per_node=True, threads=coracle.usable_cpus())[1]


@pytest.mark.gpu
@pytest.mark.parametrize("occupancy", [0.3, 0.6])
def test_random_clusters_stage_matrix_equals_the_oracle(occupancy):
    """util.random_cluster (1- and 2-socket nodes, mixed NIC speeds and switches, maintenance, busy, inactive nodes) against
    random NUMA / PCI / invalid pods of up to four groups, some of them with node groups: every (pod, node) stage is the oracle's."""
    seed = 8300 + int(occupancy * 10)
    nl = util.random_cluster(seed, 3000, occupancy=occupancy)
    rng = np.random.default_rng(seed)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(300)]
    groups = [None if rng.random() < 0.7 else list(rng.choice(["default", "alpha", "beta"], size=1)) for _ in tops]
    m = HipMatcher(device=0, clock=lambda: util.CLOCK)
    ex = m.ExplainNodes(nl, tops, pod_groups=groups, per_node=True)
    assert all(e.error is None and e.unmirrored == 0 for e in ex)
    got = np.stack([e.stages for e in ex])
    want = oracle_stages(nl, tops, util.CLOCK, groups)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10].tolist()
    late_stages_seen(np.stack([np.bincount(r, minlength=len(STAGES)) for r in want]))


@pytest.mark.gpu
def test_wide_nodes_stage_matrix_equals_the_oracle():
    """util.mixed_cluster: 3- and 4-socket nodes and sockets of up to 128 cores (the wide records) among ordinary ones."""
    nl = util.mixed_cluster(8400, 2500, wide_share=0.4)
    rng = np.random.default_rng(8400)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(200)]
    m = HipMatcher(device=0, clock=lambda: util.CLOCK)
    ex = m.ExplainNodes(nl, tops, per_node=True)
    assert all(e.error is None and e.unmirrored == 0 for e in ex)
    assert sum(v.numa_nodes > 2 for v in nl.values()) > 100
    got = np.stack([e.stages for e in ex])
    want = oracle_stages(nl, tops, util.CLOCK)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10].tolist()
    late_stages_seen(np.stack([np.bincount(r, minlength=len(STAGES)) for r in want]))


@pytest.mark.gpu
def test_big_pods_stage_matrix_equals_the_oracle():
    """Pods of 5..8 processing groups (nhdfit_explain_big) on a c4-shaped cluster of 4 000 nodes.  A pod the device returns with
    `error` set (its NIC search beyond the budget) is left out and counted; such pods must stay a small minority."""
    spec = synth.make_cluster(4, n_nodes=4000)
    nl = spec.build_nodes()
    rng = np.random.default_rng(8500)
    tops = [refmodel.make_topology(big_spec(rng, 5, 8)) for _ in range(32)]
    assert all(pack.needs_general_path(t) for t in tops)
    m = HipMatcher(device=0, clock=lambda: spec.clock_now)
    ex = m.ExplainNodes(nl, tops, per_node=True)
    ok = [i for i, e in enumerate(ex) if e.error is None]
    assert len(ok) >= 0.8 * len(tops), [e.error for e in ex if e.error is not None]
    assert all(ex[i].unmirrored == 0 for i in ok)
    got = np.stack([ex[i].stages for i in ok])
    want = oracle_stages(nl, [tops[i] for i in ok], spec.clock_now)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10].tolist()
    late_stages_seen(np.stack([np.bincount(r, minlength=len(STAGES)) for r in want]))


def mask_words(keep, extra_high_bits=False):
    """n booleans -> the uint64 words nhdfit_explain takes; `extra_high_bits` sets every bit of the last word past n."""
    n = len(keep)
    bits = np.zeros(((n + 63) // 64) * 64, bool)
    bits[:n] = keep
    if extra_high_bits:
        bits[n:] = True
    return np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))


@pytest.mark.gpu
def test_candidate_masks_against_the_oracle():
    """Random candidate masks on 3 001 nodes (not a multiple of 64): outside the mask the stage is NOT_CANDIDATE, inside it is
    the oracle's; bits set in the last word past the node count change nothing."""
    cfg, n, P = 4, 3001, 256
    spec, table, reqs, eng = _baseline(cfg, n, P)
    now = spec.clock_now
    cl = coracle.Cluster.from_spec(spec)
    pods = oracle_pods(cl, cfg, P)
    rng = np.random.default_rng(8600)
    seen = np.zeros(len(STAGES), np.int64)
    for share in (0.9, 0.5, 0.05):
        keep = rng.random(n) < share
        counts, stages = eng.explain(reqs, now, cand=mask_words(keep), per_node=True)
        want_c, want_s = cl.explain(pods, now, cand=keep, per_node=True, threads=coracle.usable_cpus())
        assert (stages[:, ~keep] == 0).all()
        assert np.array_equal(stages, want_s) and np.array_equal(counts, want_c)
        c2, s2 = eng.explain(reqs, now, cand=mask_words(keep, extra_high_bits=True), per_node=True)
        assert np.array_equal(c2, counts) and np.array_equal(s2, stages)
        seen += counts.sum(0).astype(np.int64)
    late_stages_seen(seen)
    eng.close()


@pytest.mark.gpu
def test_three_shards_on_one_device_against_the_oracle():
    """GroupEngine over three contexts on device 0 (as test_mode_b_across_shards_on_the_device builds it) on 2 001 nodes: the
    stages, put together in global node order, and the summed counts equal the oracle's, with and without a candidate mask."""
    cfg, n, P = 4, 2001, 200
    spec = synth.make_cluster(cfg, n_nodes=n)
    specs, groups = synth.make_pods(cfg, n_pods=P)
    tops = [refmodel.make_topology(s) for s in specs]
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many(tops, groups)
    grp = GroupEngine([0, 0, 0], engine_factory=Engine)
    grp.set_dictionary(pk)
    grp.upload(table)
    assert len([1 for lo, hi in grp._bounds if hi > lo]) == 3
    cl = coracle.Cluster.from_spec(spec)
    pods = cl.pods_from_tops(tops, groups)
    keep = np.random.default_rng(8700).random(n) < 0.7
    seen = np.zeros(len(STAGES), np.int64)
    for cand in (None, keep):
        counts, stages = grp.explain(reqs, spec.clock_now, cand=None if cand is None else mask_words(cand), per_node=True)
        want_c, want_s = cl.explain(pods, spec.clock_now, cand=cand, per_node=True, threads=coracle.usable_cpus())
        assert np.array_equal(stages, want_s) and np.array_equal(counts, want_c)
        seen += counts.sum(0).astype(np.int64)
    late_stages_seen(seen)
    grp.close()


@pytest.mark.gpu
def test_explain_leaves_no_trace_and_follows_the_mirror():
    """FindNodes and its bitmaps are bit-identical before and after explain; after commits and deltas (attached mode) explain
    describes the state the mirror holds - FITS per node is the oracle's verdict on the mutated objects."""
    spec = synth.make_cluster(4, n_nodes=1500)
    nl = spec.build_nodes()
    pods, groups = synth.make_pods(4, n_pods=200)
    tops = [refmodel.make_topology(s) for s in pods]
    now = spec.clock_now
    m = HipMatcher(device=0, clock=lambda: now)
    m.attach(nl)
    before = m.FindNodes(nl, tops, pod_groups=groups)
    reqs = m.packer.digest_many(tops, groups)
    s0, b0, _ = m.engine.find(reqs, now, want_map=False)
    st0 = m.engine.stats()
    ex = m.ExplainNodes(nl, tops, pod_groups=groups, per_node=True)
    st1 = m.engine.stats()
    assert (st0.launches, st0.fit_ms_last, st0.small_finds, st0.batch_finds) == (st1.launches, st1.fit_ms_last, st1.small_finds, st1.batch_finds)
    s1, b1, _ = m.engine.find(reqs, now, want_map=False)
    assert np.array_equal(s0, s1) and np.array_equal(b0, b1)
    assert m.FindNodes(nl, tops, pod_groups=groups) == before
    for e, res in zip(ex, before):
        assert (res[0] is None) == (e.counts["FITS"] == 0) and e.total == len(nl)
    # commit winners through the reference mutators and flip scalar state: the mirror takes deltas / re-packs
    names = list(nl)
    for top, res in zip(tops[:40], m.FindNodes(nl, tops[:40])):
        if res[0] is not None and O.evaluate_node(nl[res[0]], top, now) is not None:
            O.commit(nl[res[0]], top, res[1], now)
            m.mark_dirty(res[0])
    nl[names[5]].maintenance = True
    nl[names[9]].busy_time = now - 1.0
    nl[names[11]].active = False
    for e, top in zip(m.ExplainNodes(nl, tops[:60], per_node=True), tops[:60]):
        want = [O.evaluate_node(nl[x], top, now) is not None for x in names]
        assert [int(v) == FITS for v in e.stages] == want
        assert e.stages[5] == STAGES.index("MAINTENANCE")


@pytest.mark.gpu
def test_group_entry_equals_one_device():
    """HipMatcher(devices=[0]): the group entry (nhdfit_group_explain: counts summed over the shards, stages put together) gives what
    one context gives.  (One device of the box: a group of one communicator per device cannot hold the same device twice.)"""
    spec = synth.make_cluster(3, n_nodes=900)
    nl = spec.build_nodes()
    pods, groups = synth.make_pods(3, n_pods=150)
    tops = [refmodel.make_topology(s) for s in pods]
    one = HipMatcher(device=0, clock=lambda: spec.clock_now)
    grp = HipMatcher(devices=[0], clock=lambda: spec.clock_now)
    a = one.ExplainNodes(nl, tops, pod_groups=groups, per_node=True)
    b = grp.ExplainNodes(nl, tops, pod_groups=groups, per_node=True)
    for x, y in zip(a, b):
        assert x.counts == y.counts and np.array_equal(x.stages, y.stages)
    sub = {k: v for i, (k, v) in enumerate(nl.items()) if i % 3}
    grp.attach(nl)
    one.attach(nl)
    for x, y in zip(one.ExplainNodes(sub, tops[:30]), grp.ExplainNodes(sub, tops[:30])):
        assert x.counts == y.counts and x.total == len(sub)


@pytest.mark.gpu
def test_one_pod_with_every_stage_summary():
    """One pod against a random cluster: the summary sentence names the counts the per-node stages give."""
    nl = util.random_cluster(8100, 300, occupancy=0.6)
    rng = np.random.default_rng(81)
    m = HipMatcher(device=0, clock=lambda: util.CLOCK)
    for _ in range(10):
        top = refmodel.make_topology(util.random_pod_spec(rng))
        e = m.ExplainNode(nl, top, per_node=True)
        assert e.total == len(nl) and e.summary().startswith(f"{e.counts['FITS']}/{len(nl)} nodes are available")
        assert [e.counts[s] for s in STAGES] == np.bincount(e.stages, minlength=len(STAGES)).tolist()


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_explain_kernel_resources(tmp_path):
    """k_explain (both request forms) and its view pass have no private segment - every value of a pair lives in registers - and
    spill no vector registers (the compiler's own resource report, in the style of test_kernel_resources.py)."""
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
    ours = {k: v for k, v in usage.items() if "k_explain" in k}
    assert len(ours) == 3, list(usage)
    for k, v in ours.items():
        assert v["ScratchSize"] == 0 and v.get("VGPRs Spill", 0) == 0, (k, v)
        if "views" in k:
            assert v.get("SGPRs Spill", 0) == 0, (k, v)
