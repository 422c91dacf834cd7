"""Candidates as the UNMODIFIED reference defines them (include/nhdfit.h, nhdfit_candidates), and the inputs the CPU and the GPU
tests hold to it.

    candidates[j] = Matcher().FindNode(nl without candidates[0..j-1], a fresh top)          nhd/Matcher.py:65-452

until FindNode answers (None,) or K entries are out: the scheduler's own first-fit (SelectNode, nhd/Matcher.py:393-421) on a dict
that loses each answer - where it would go next once a bind had failed (nhd/NHDScheduler.py:291-345).  FindNode changes neither the
nodes nor the dict.

Inputs: the five workload/synth.py configurations at 48 nodes with their first 8 pods, and every pod of the fixtures
tests/golden/*.json against its fixture's cluster, with and without the fixtures' node groups (InitialNodeFilter,
nhd/NHDScheduler.py:235-247).  The answers are stored with tests/test_candidates_reference.py's
(tests/golden/refanswers/tests.test_candidates_reference.json), where the GPU tests read them too."""
import glob
import json
import os

from oracle import nhd_oracle as O
from tests import refanswers, util
from workload import refmodel, synth

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "*.json")))
IDS = [os.path.basename(p)[:-5] for p in GOLDENS]
STORE = "tests.test_candidates_reference"
SYNTH_NODES, SYNTH_PODS = 48, 8
K = 8


def entry(result):
    """(name, mapping) as FindNode returns it - the reference's lists, the matcher's tuples - in one comparable form."""
    name, mp = result
    return (name, tuple(mp["gpu"]), tuple(mp["cpu"]), tuple(tuple(x) for x in mp["nic"]))


def iterate(find_node, nl, make_top, k=K):
    """The definition: `find_node(nl, top)` on a dict that loses each answer."""
    rest, out = dict(nl), []
    while len(out) < k and rest:
        r = find_node(rest, make_top())
        if r[0] is None:
            break
        out.append(entry(r))
        del rest[r[0]]
    return out


def synth_case(cfg):
    spec = synth.make_cluster(cfg, n_nodes=SYNTH_NODES)
    specs, groups = synth.make_pods(cfg, n_pods=SYNTH_PODS)
    return spec, specs, groups


def load_golden(path):
    with open(path) as f:
        case = json.load(f)
    return case, [p["spec"] for p in case["pods"]], [p["groups"] for p in case["pods"]]


def reference_synth(ref, cfg):
    """[pod] lists of the reference for a synth configuration (every node a candidate: FindNode's argument as given)."""
    from oracle import ref_loader
    spec, specs, _ = synth_case(cfg)
    ref_loader.VirtualClock(spec.clock_now).install()
    nodes = [spec.build_node(i, ref) for i in range(spec.n)]
    nl = {n.name: n for n in nodes}
    return [iterate(ref_loader.find_node, nl, lambda: refmodel.make_topology(s, ref)) for s in specs]


def reference_golden(ref, path, with_groups):
    """[pod] lists of the reference for a fixture; with_groups: FindNode is handed what InitialNodeFilter leaves of the cluster."""
    from oracle import ref_loader
    case, specs, groups = load_golden(path)
    ref_loader.VirtualClock(case["clock"]).install()
    nl = util.build_cluster(case["nodes"], ref)
    plain = util.build_cluster(case["nodes"])                # (stand-ins: the node filter reads labels and flags only)
    out = []
    for p, s in enumerate(specs):
        keep = O.initial_node_filter(plain, groups[p]) if with_groups else plain
        out.append(iterate(ref_loader.find_node, {nm: nd for nm, nd in nl.items() if nm in keep}, lambda: refmodel.make_topology(s, ref)))
    return out


def lists_of(results):
    for c in results:
        assert c.error is None, c.error
    return [[entry(e) for e in c.entries] for c in results]


def matcher_synth(matcher_factory, cfg, k=K):
    """(results of HipMatcher.CandidatesMany, [pod] lists) for a synth configuration."""
    spec, specs, _ = synth_case(cfg)
    m = matcher_factory(spec.clock_now)
    got = m.CandidatesMany(spec.build_nodes(), [refmodel.make_topology(s) for s in specs], k=k)
    return got, lists_of(got)


def matcher_golden(matcher_factory, path, with_groups, k=K):
    case, specs, groups = load_golden(path)
    m = matcher_factory(case["clock"])
    got = m.CandidatesMany(util.build_cluster(case["nodes"]), [refmodel.make_topology(s) for s in specs], k=k,
                           pod_groups=groups if with_groups else None)
    return got, lists_of(got)


def stored(test_id):
    """The stored reference lists of one case (as tests/test_candidates_reference.py recorded them)."""
    v = refanswers._load(STORE).get(test_id)
    assert v is not None, f"no stored reference answers for {test_id}"
    return refanswers.decode(v[0])
