"""nhdfit_explain on the MI355X: the device's stage for every (pod, node) against the reference's stored stages on the
golden fixtures, its counts against nhdfit_find's verdict bitmap and a vectorised host computation at BASELINE shapes, the
absence of side effects and the group entry (`pytest -m gpu`); and k_explain's resources (hipcc only, no GPU).  Nothing here reads the
reference tree: its answers come from tests/golden/refanswers/tests.test_explain_reference.json."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import Engine
from nhd_amd.matcher import STAGES, HipMatcher
from oracle import nhd_oracle as O
from tests import explain_check, util
from workload import planes, refmodel, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FITS = STAGES.index("FITS")


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


def host_stages_upto_cpu(table, reqs, now):
    """Stages 0..5 per (pod, node) by numpy over the planes (ordinary nodes, ordinary requests); 6 stands for "beyond the CPU
    stage".  The GPU and CPU stages are asked per distinct (node free resources, request demand) pair."""
    n = table.n
    flags = table.p2["flags"].astype(np.int64)
    U = table.detail["numa_nodes"].astype(np.int64)
    smt = (flags & pack.NF_SMT) != 0
    free = table.p0["t0"] & table.p1["t1"]
    fc = np.stack([np.array([bin(int(x)).count("1") for x in free[:, u]]) for u in range(2)], 1)
    gmask = table.p2["gpu_free"].astype(np.int64)
    g1 = table.p2["gpu_numa1"].astype(np.int64)
    fg = np.stack([np.array([bin(int(x)).count("1") for x in gmask & ~g1]), np.array([bin(int(x)).count("1") for x in gmask & g1])], 1)
    nkey = np.stack([U, smt, fg[:, 0], fg[:, 1], fc[:, 0], fc[:, 1]], 1)
    ncls, ninv = np.unique(nkey, axis=0, return_inverse=True)
    busy = (now - table.p4["busy_time"]) < O.MIN_BUSY_SECS
    out = np.zeros((len(reqs), n), np.uint8)
    memo = {}
    for i, r in enumerate(reqs):
        G = int(r["n_groups"])
        gp = [int(x) for x in r["gpus"][:G]]
        st = np.full(n, 6, np.uint8)

        def verdicts(smt_c):
            cpu = [int(x) for x in (r["cpu_smt"] if smt_c else r["cpu_nosmt"])[:G]] + [int(r["misc_smt"] if smt_c else r["misc_nosmt"])]
            key = (tuple(gp), tuple(cpu))
            if key not in memo:
                gv, cv = np.zeros(len(ncls), bool), np.zeros(len(ncls), bool)
                for k, (u, s, a0, a1, c0, c1) in enumerate(ncls.tolist()):
                    for p in itertools.product(range(u), repeat=G):
                        t = [0, 0]
                        for g, x in zip(p, gp):
                            t[g] += x
                        gv[k] |= t[0] <= a0 and t[1] <= a1
                    for p in itertools.product(range(u), repeat=G + 1):
                        t = [0, 0]
                        for g, x in zip(p, cpu):
                            t[g] += x
                        cv[k] |= t[0] <= c0 and t[1] <= c1
                memo[key] = (gv, cv)
            return memo[key]
        for smt_c in (False, True):
            gv, cv = verdicts(smt_c)
            sel = smt == smt_c
            st[sel & ~cv[ninv]] = 5
            st[sel & ~gv[ninv]] = 4
        if sum(gp):
            st[busy] = 3
        st[table.p2["hp_free"] < int(r["hugepages_gb"])] = 2
        st[(flags & pack.NF_MAINTENANCE) != 0] = 1
        if int(r["flags"]) & pack.RF_INITIAL_FILTER:
            st[((flags & pack.NF_ACTIVE) == 0) | ((table.p3["groups"] & np.uint64(int(r["groups"]))) == 0)] = 0
        out[i] = st
    return out


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
    host computation (and, at the small shapes, the per-node stages 6..8 are what is left over: not FITS, not 0..5)."""
    spec, table, reqs, eng = _baseline(cfg, n, P)
    now = spec.clock_now
    score, bm, _ = eng.find(reqs, now, want_map=False)
    counts, stages = eng.explain(reqs, now, per_node=n * P <= 1 << 22)
    assert counts.shape == (P, len(STAGES)) and (counts.sum(1) == n).all()
    feas = unpack_bitmap(bm, n)
    assert np.array_equal(counts[:, FITS], feas.sum(1))
    host = host_stages_upto_cpu(table, reqs, now)
    for k in range(6):
        assert np.array_equal(counts[:, k], (host == k).sum(1)), k
    assert np.array_equal(counts[:, 6:].sum(1), (host == 6).sum(1))
    if stages is not None:
        assert np.array_equal(stages == FITS, feas.astype(bool))
        assert np.array_equal(np.minimum(stages, 6), host)
        assert np.array_equal(counts, np.stack([(stages == k).sum(1) for k in range(len(STAGES))], 1))
    eng.close()


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
