"""Shared by the CPU and GPU tests of candidates for big requests (nhdfit_candidates_big): the inputs that are held to the UNMODIFIED
reference's definition (tests/candidates_reference.iterate over Matcher().FindNode, K = 8) - every pod of the general path of the
fixtures tests/golden/big/*.json against its fixture's cluster, and seeded tests/test_big_core.big_spec pods on
tests/headroom_general_check.py's three clusters (plain nodes and wide ones mixed, two ENABLE_SHARING clusters) - the reference's lists,
stored with the CPU test module's answers (tests/golden/refanswers/tests.test_candidates_big_reference.json) so the GPU box holds the
device to them.

The fixtures of tests/golden/big name no node groups (their pods are bare specs), so there is no second, filtered run of them.  The
seeded pods are run a second time WITH node groups on two of the clusters (GROUPED): the reference's FindNode is handed what
InitialNodeFilter (nhd/NHDScheduler.py:235-247) leaves, the entry under test is handed the whole cluster and `pod_groups`."""
import json

import numpy as np

from nhd_amd import pack
from tests import big_check
from tests import candidates_reference as cr
from tests import headroom_general_check as gc
from tests import refanswers, util
from tests.test_big_core import big_spec
from workload import refmodel

STORE = "tests.test_candidates_big_reference"
K = cr.K
FIXTURES = big_check.FIXTURES
FIXTURE_IDS = [p.rsplit("/", 1)[-1][:-5] for p in FIXTURES]
# seeds of the clusters' pods: five or six groups (the reference enumerates 4^G x 4^(G+1) tuples on a four-socket node)
CLUSTER_SEEDS = {"mixed": 4100, "sharing_random": 4101, "sharing_mixed": 4102}
CLUSTER_PODS = {"mixed": 8, "sharing_random": 8, "sharing_mixed": 4}     # (the reference takes twenty seconds and more per pod on the last)


# the clusters that are run with node groups as well, and the groups pod p asks for: GROUP_CYCLE[p % 3]
GROUPED = ("mixed", "sharing_random")
GROUP_CYCLE = (["default"], ["alpha", "beta"], ["beta"])


def cluster_groups(name):
    return [list(GROUP_CYCLE[p % len(GROUP_CYCLE)]) for p in range(CLUSTER_PODS[name])]


def cluster_keep(descs, groups):
    """Per pod, the names InitialNodeFilter keeps."""
    from oracle import nhd_oracle as O
    plain = util.build_cluster(descs)
    return [set(O.initial_node_filter(plain, g)) for g in groups]


def cluster_specs(name):
    rng = np.random.default_rng(CLUSTER_SEEDS[name])
    return [big_spec(rng, 5, 6) for _ in range(CLUSTER_PODS[name])]


def load_fixture(path):
    """(case, [pod index of the fixture], their specs): the fixture's pods of the general path."""
    with open(path) as f:
        case = json.load(f)
    idx = [p for p, s in enumerate(case["pods"]) if pack.needs_general_path(refmodel.make_topology(s))]
    return case, idx, [case["pods"][p] for p in idx]


def reference_lists(ref, descs, specs, sharing, clock, k=K, keep=None):
    """[pod] lists of the reference on the cluster `descs` (keep: per pod the names FindNode is handed, or None: all)."""
    from oracle import ref_loader
    ref_loader.VirtualClock(clock).install()
    with gc.sharing_all(sharing, ref):
        nl = util.build_cluster(descs, ref)
        return [cr.iterate(ref_loader.find_node, nl if keep is None else {nm: nd for nm, nd in nl.items() if nm in keep[p]},
                           lambda: refmodel.make_topology(s, ref), k=k) for p, s in enumerate(specs)]


def matcher_lists(matcher_factory, descs, specs, sharing, clock, k=K, pod_groups=None):
    """(matcher, nl, results of CandidatesMany(big=True), [pod] lists, [pod] FITS counts of ExplainNodes on the same matcher)"""
    with gc.sharing_all(sharing):
        nl = util.build_cluster(descs)
        m = matcher_factory(clock)
        tops = [refmodel.make_topology(s) for s in specs]
        assert all(pack.needs_general_path(t) for t in tops)
        got = m.CandidatesMany(nl, tops, k=k, pod_groups=pod_groups, now=clock, big=True)
        fits = [e.counts.get("FITS", 0) for e in m.ExplainNodes(nl, [refmodel.make_topology(s) for s in specs], pod_groups, now=clock)]
    return m, nl, got, cr.lists_of(got), fits


def consistent(results, lists, fits, k=K):
    """A list is as long as the summary says, no node is named twice, `form` is the big entry's, `feasible` is explain's FITS."""
    for c, row, f in zip(results, lists, fits):
        assert c.error is None and len(row) == min(k, c.feasible) and c.preferred <= c.feasible
        assert len({e[0] for e in row}) == len(row)
        assert c.form == pack.CANDIDATES_FORM_BIG
        assert c.feasible == f


def stored(test_id, k=0):
    """Stored reference answer `k` of one case (as tests/test_candidates_big_reference.py recorded it)."""
    v = refanswers._load(STORE).get(test_id)
    assert v is not None and len(v) > k, f"no stored reference answers for {test_id}"
    return refanswers.decode(v[k])
