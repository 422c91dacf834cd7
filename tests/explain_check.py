"""Shared by the CPU and GPU tests of explain: the reference-generated fixtures (tests/golden/*.json, beyond/, big/, sharing/)
read as one snapshot each - every pod against the fixture's cluster, with InitialNodeFilter where the fixture names the pods'
node groups - and the reference's stage for every (pod, node) of it (tests/explain_reference.py), stored with the CPU test
module's answers (tests/golden/refanswers/tests.test_explain_reference.json) so the GPU box holds the device to them."""
import glob
import json
import os

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
