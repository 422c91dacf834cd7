"""Shared by the CPU and GPU tests of headroom: the inputs that are held to the UNMODIFIED reference - the five workload/synth.py
configurations at 48 nodes with their first pods as templates, and every pod spec of the fixtures tests/golden/*.json against its
fixture's cluster, with and without the fixtures' node groups - the reference's answer for every (template, node) of them
(tests/headroom_reference.py), stored with the CPU test module's answers
(tests/golden/refanswers/tests.test_headroom_reference.json) so the GPU box holds the device to them, and the same loop on the
independent oracle for inputs of any size.

An answer is one integer per (template, node), encoded as the device encodes its entries (include/nhdfit.h): replicas, plus
NHDFIT_HEADROOM_STOPPED where the reference's SetPhysicalIdsFromMapping raised or returned None."""
import glob
import json
import multiprocessing
import os

import numpy as np

from nhd_amd import pack
from oracle import nhd_oracle as O
from tests import refanswers, util
from tests.headroom_reference import independent_headroom, reference_headroom
from workload import refmodel, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "*.json")))
IDS = [os.path.basename(p)[:-5] for p in GOLDENS]
STORE = "tests.test_headroom_reference"
SYNTH_NODES, SYNTH_TEMPLATES = 48, 8
CAP = 512                                            # HipMatcher.Headroom's default max_per_node


def entry(k, stopped):
    return int(k) | (pack.HEADROOM_STOPPED if stopped else 0)


def synth_case(cfg):
    spec = synth.make_cluster(cfg, n_nodes=SYNTH_NODES)
    specs, groups = synth.make_pods(cfg, n_pods=SYNTH_TEMPLATES)
    return spec, specs, groups


def load_golden(path):
    with open(path) as f:
        case = json.load(f)
    return case, [p["spec"] for p in case["pods"]], [p["groups"] for p in case["pods"]]


def reference_synth(ref, cfg):
    """[template][node] entries of the reference for a synth configuration (every node a candidate: FindNode's argument as given)."""
    from oracle import ref_loader
    spec, specs, _ = synth_case(cfg)
    ref_loader.VirtualClock(spec.clock_now).install()
    return [[entry(*reference_headroom(ref, lambda: spec.build_node(i, ref), lambda: refmodel.make_topology(s, ref), CAP)) for i in range(spec.n)]
            for s in specs]


def reference_golden(ref, path, with_groups):
    """[pod][node] entries of the reference for a fixture; with_groups: nodes InitialNodeFilter drops for the pod have 0."""
    from oracle import ref_loader
    case, specs, groups = load_golden(path)
    ref_loader.VirtualClock(case["clock"]).install()
    descs = case["nodes"]
    plain = util.build_cluster(descs)                       # (stand-ins: the node filter reads labels and flags only)
    out = []
    for p, s in enumerate(specs):
        keep = set(O.initial_node_filter(plain, groups[p])) if with_groups else set(plain)
        out.append([entry(*reference_headroom(ref, lambda: refmodel.build_node(d, ref), lambda: refmodel.make_topology(s, ref), CAP))
                    if d["name"] in keep else 0 for d in descs])
    return out


def matcher_synth(matcher_factory, cfg):
    """(results of HipMatcher.HeadroomMany(per_node=True), entries [template][node]) for a synth configuration."""
    spec, specs, _ = synth_case(cfg)
    nl = spec.build_nodes()
    m = matcher_factory(spec.clock_now)
    got = m.HeadroomMany(nl, [refmodel.make_topology(s) for s in specs], per_node=True, max_per_node=CAP)
    return got, entries_of(got)


def matcher_golden(matcher_factory, path, with_groups):
    case, specs, groups = load_golden(path)
    nl = util.build_cluster(case["nodes"])
    m = matcher_factory(case["clock"])
    got = m.HeadroomMany(nl, [refmodel.make_topology(s) for s in specs], pod_groups=groups if with_groups else None, per_node=True, max_per_node=CAP)
    return got, entries_of(got)


def entries_of(results):
    for h in results:
        assert h.error is None, h.error
    return [(h.per_node.astype(np.int64) | h.flags.astype(np.int64)).tolist() for h in results]


def stored(test_id):
    """The stored reference entries of one case (as tests/test_headroom_reference.py recorded them)."""
    v = refanswers._load(STORE).get(test_id)
    assert v is not None, f"no stored reference answers for {test_id}"
    return refanswers.decode(v[0])


def four_templates(cfg):
    """Four templates of the configuration's own pods that cover one, two, three and four processing groups (the fourth is put
    together from the three-group one and a group of the one-group one, in the other map type), and - where the configuration draws
    them - pods with and without GPUs, NUMA and PCI mode."""
    specs, _ = synth.make_pods(cfg, n_pods=256)

    def pick(G, gpu, pci):
        def score(s):
            has_gpu = any(g["gpus"] for g in s["groups"])
            return (has_gpu == gpu) + (((s["map_type"] == "PCI") == pci))
        return max((s for s in specs if len(s["groups"]) == G), key=score)
    one, two, three = pick(1, True, True), pick(2, False, False), pick(3, True, False)
    four = dict(three, groups=[dict(g) for g in three["groups"]] + [dict(one["groups"][0])], map_type="PCI" if three["map_type"] == "NUMA" else "NUMA")
    if cfg == 2:                                             # (the configuration draws NUMA pods only, and no GPUs)
        four["map_type"] = "NUMA"
    return [one, two, three, four]


# ---- the independent oracle on inputs of any size, spread over the usable cores by node ranges ----------------------------------------
def _oracle_range(args):
    cfg, n, seed_specs, lo, hi, cap, skip = args
    spec = synth.make_cluster(cfg, n_nodes=n)
    out = np.zeros((len(seed_specs), hi - lo), np.int64)
    for i in range(lo, hi):
        if skip is not None and not skip[:, i - lo].any():
            continue
        desc = spec.describe(i)
        for p, s in enumerate(seed_specs):
            if skip is not None and not skip[p, i - lo]:
                continue
            out[p, i - lo] = entry(*independent_headroom(lambda: refmodel.build_node(desc), lambda: refmodel.make_topology(s), cap, now=spec.clock_now))
    return lo, out


def oracle_synth(cfg, n, specs, cap=CAP, procs=None, maybe=None):
    """[template][node] entries of the independent oracle (oracle/nhd_oracle.py: find_node on the one node + commit, the busy window out
    of the way) for the first `n` nodes of a synth configuration and the pod specs `specs`; fresh processes (spawn: the caller may hold
    a GPU) share the nodes out by ranges.  `maybe` [template][node] bool: pairs known to have 0 are left out (None: every pair)."""
    from oracle import coracle
    procs = max(1, min(16, coracle.usable_cpus())) if procs is None else procs
    step = max(64, (n + procs * 8 - 1) // (procs * 8))
    jobs = [(cfg, n, specs, lo, min(n, lo + step), cap, None if maybe is None else np.ascontiguousarray(maybe[:, lo:min(n, lo + step)]))
            for lo in range(0, n, step)]
    out = np.zeros((len(specs), n), np.int64)
    if procs == 1 or len(jobs) == 1:
        parts = [_oracle_range(j) for j in jobs]
    else:
        with multiprocessing.get_context("spawn").Pool(procs) as pool:
            parts = pool.map(_oracle_range, jobs, chunksize=1)
    for lo, part in parts:
        out[:, lo:lo + part.shape[1]] = part
    return out
