"""Shared by the CPU and GPU tests of explain: the reference-generated fixtures (tests/golden/*.json, beyond/, big/, sharing/)
read as one snapshot each - every pod against the fixture's cluster, with InitialNodeFilter where the fixture names the pods'
node groups - and the reference's stage for every (pod, node) of it (tests/explain_reference.py), stored with the CPU test
module's answers (tests/golden/refanswers/tests.test_explain_reference.json) so the GPU box holds the device to them."""
import glob
import itertools
import json
import os

import numpy as np

from nhd_amd import pack
from oracle import nhd_oracle as O
from tests import refanswers, util
from tests.explain_reference import NOT_CANDIDATE, reference_stages
from workload import refmodel

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "*.json"))) + \
    [p for d in ("beyond", "big", "sharing") for p in sorted(glob.glob(os.path.join(HERE, "golden", d, "*.json")))]
IDS = [os.path.relpath(p, os.path.join(HERE, "golden"))[:-5] for p in GOLDENS]
STORE = "tests.test_explain_reference"          # module whose stored answers hold the fixtures' stages


def load(path):
    """(case, pod specs, pod node groups or None, sharing)"""
    with open(path) as f:
        case = json.load(f)
    pods = case["pods"]
    if "spec" in pods[0]:
        return case, [p["spec"] for p in pods], [p["groups"] for p in pods], False
    return case, pods, None, os.path.basename(os.path.dirname(path)) == "sharing"


class sharing_flag:
    """refmodel.ENABLE_SHARING (and the reference's own constant, given its namespace) set for a `with` block."""

    def __init__(self, on, ref=None):
        self.on, self.ref = on, ref

    def __enter__(self):
        self.saved = refmodel.ENABLE_SHARING
        refmodel.ENABLE_SHARING = self.on or self.saved
        if self.ref is not None and self.on:
            self.ref.node_mod.ENABLE_SHARING = True

    def __exit__(self, *exc):
        refmodel.ENABLE_SHARING = self.saved
        if self.ref is not None and self.on:
            self.ref.node_mod.ENABLE_SHARING = False


def explain(path, matcher_factory):
    """The stages HipMatcher.ExplainNodes gives for the fixture: one list per pod, in node order."""
    case, specs, groups, sharing = load(path)
    with sharing_flag(sharing):
        nl = util.build_cluster(case["nodes"])
        tops = [refmodel.make_topology(s) for s in specs]
        m = matcher_factory(case["clock"])
        got = m.ExplainNodes(nl, tops, pod_groups=groups, now=case["clock"], per_node=True)
    assert all(e.unmirrored == 0 and e.total == len(nl) for e in got)
    return [e.stages.tolist() for e in got]


def reference(path, ref):
    """The reference's stages for the fixture (the reference tree must be present)."""
    from oracle import ref_loader
    from oracle import nhd_oracle as O
    case, specs, groups, sharing = load(path)
    ref_loader.VirtualClock(case["clock"]).install()
    out = []
    with sharing_flag(sharing, ref):
        nl = util.build_cluster(case["nodes"], ref)
        for p, s in enumerate(specs):
            sub = nl if groups is None else O.initial_node_filter(nl, groups[p])
            st = reference_stages(ref, sub, refmodel.make_topology(s, ref))
            out.append([st.get(n, NOT_CANDIDATE) for n in nl])
    return out


def stored(golden_id):
    """The stored reference stages of one fixture (as test_explain_reference.py::test_goldens recorded them)."""
    v = refanswers._load(STORE).get(f"test_goldens[{golden_id}]")
    assert v is not None, f"no stored reference stages for {golden_id}"
    return refanswers.decode(v[0])


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
