"""Shared by the CPU and GPU tests of headroom on the general path (nhdfit_headroom_general): the inputs that are held to the
UNMODIFIED reference's loop (tests/headroom_reference.py) - wide nodes of a mixed cluster, ENABLE_SHARING clusters with all three
switches flipped (the stand-ins', the reference's node module's, the independent oracle's), the fixtures tests/golden/beyond/*.json
and tests/golden/sharing/*.json with their own pods, and a template that asks for nothing - the reference's answer for every
(template, node) of them, stored with the CPU test module's answers
(tests/golden/refanswers/tests.test_headroom_general_reference.json) so the GPU box holds the device to them.

An answer is encoded as the device encodes its entries (tests/headroom_check.entry)."""
import glob
import json
import os

import numpy as np

from oracle import nhd_oracle as O
from tests import refanswers, util
from tests.headroom_check import entries_of, entry
from tests.headroom_reference import independent_headroom, reference_headroom
from workload import refmodel

HERE = os.path.dirname(os.path.abspath(__file__))
STORE = "tests.test_headroom_general_reference"
CAP = 37
NOTHING = dict(map_type="NUMA", hugepages_gb=0, misc=0, misc_smt=False,
               groups=[dict(proc=0, helpers=0, rx=0.0, tx=0.0, proc_smt=False, helper_smt=False, gpus=[])])
# name -> (ENABLE_SHARING, node descriptions, only the nodes drawn from the wide generator)
CLUSTERS = {
    "mixed": (False, lambda: util.mixed_cluster_desc(9800, 90, occupancy=0.1), True),
    "sharing_random": (True, lambda: util.random_cluster_desc(9900, 30, occupancy=0.1), False),
    "sharing_mixed": (True, lambda: util.mixed_cluster_desc(9901, 40, occupancy=0.1), False),
}
PAIRS = {"mixed": (420, 41, 12), "sharing_random": (360, 37, 9), "sharing_mixed": (480, 56, 13)}   # pairs, with room, with more than one replica
FIXTURES = [p for d in ("beyond", "sharing") for p in sorted(glob.glob(os.path.join(HERE, "golden", d, "*.json")))]
FIXTURE_IDS = [os.path.relpath(p, os.path.join(HERE, "golden"))[:-5] for p in FIXTURES]


def templates():
    rng = np.random.default_rng(98)
    return [util.random_pod_spec(rng, max_groups=4) for _ in range(12)]


class sharing_all:
    """ENABLE_SHARING for a `with` block: the stand-in node objects' constant (what the packer mirrors by), the independent oracle's,
    and - given its namespace - the reference's own."""

    def __init__(self, on, ref=None):
        self.on, self.ref = on, ref

    def __enter__(self):
        self.saved = (refmodel.ENABLE_SHARING, O.ENABLE_SHARING)
        if self.on:
            refmodel.ENABLE_SHARING = O.ENABLE_SHARING = True
            if self.ref is not None:
                self.ref.node_mod.ENABLE_SHARING = True

    def __exit__(self, *exc):
        refmodel.ENABLE_SHARING, O.ENABLE_SHARING = self.saved
        if self.ref is not None and self.on:
            self.ref.node_mod.ENABLE_SHARING = False


def reference_entries(ref, descs, specs, sharing, clock, cap=CAP, keep=None):
    """[template][node of descs] entries of the reference (0 for nodes `keep` [template] -> set of names leaves out)."""
    from oracle import ref_loader
    ref_loader.VirtualClock(clock).install()
    with sharing_all(sharing, ref):
        return [[entry(*reference_headroom(ref, lambda: refmodel.build_node(d, ref), lambda: refmodel.make_topology(s, ref), cap))
                 if keep is None or d["name"] in keep[p] else 0 for d in descs] for p, s in enumerate(specs)]


def oracle_entries(descs, specs, sharing, clock, cap=CAP):
    """The same loop on the independent oracle."""
    with sharing_all(sharing):
        return [[entry(*independent_headroom(lambda: refmodel.build_node(d), lambda: refmodel.make_topology(s), cap, now=clock)) for d in descs]
                for s in specs]


def matcher_entries(matcher_factory, descs, specs, sharing, clock, cap=CAP, pod_groups=None, **kw):
    """(matcher, results of HeadroomMany(general=True, per_node=True), entries [template][node])"""
    with sharing_all(sharing):
        nl = util.build_cluster(descs)
        m = matcher_factory(clock)
        got = m.HeadroomMany(nl, [refmodel.make_topology(s) for s in specs], pod_groups=pod_groups, per_node=True, max_per_node=cap, general=True, **kw)
    return m, got, entries_of(got)


def cluster_case(name):
    """(ENABLE_SHARING, node descriptions, whether only the nodes mirrored as wide records are held to the reference)"""
    sharing, descs, wide_only = CLUSTERS[name]
    return sharing, descs(), wide_only


def selection(descs, wide_only):
    """Indices into `descs` of the nodes a cluster case holds to the reference: all, or the ones drawn from the wide generator
    (util.random_wide_node_desc, names w....: 3-4 sockets, up to 128 cores per socket - and a few at the edge of the fast layout)."""
    return [i for i, d in enumerate(descs) if not wide_only or d["name"].startswith("w")]


def _names_groups(path):
    with open(path) as f:
        return "spec" in json.load(f)["pods"][0]


# (fixture id, with its node groups): every fixture plain, and with node groups where it names them
FIXTURE_CASES = [(i, g) for i, p in zip(FIXTURE_IDS, FIXTURES) for g in ([False, True] if _names_groups(p) else [False])]


def load_fixture(path):
    """(case, pod specs, pod node groups or None, sharing)"""
    with open(path) as f:
        case = json.load(f)
    pods = case["pods"]
    sharing = os.path.basename(os.path.dirname(path)) == "sharing"
    if "spec" in pods[0]:
        return case, [p["spec"] for p in pods], [p["groups"] for p in pods], sharing
    return case, pods, None, sharing


def fixture_keep(case, groups):
    """Per pod, the names InitialNodeFilter keeps."""
    plain = util.build_cluster(case["nodes"])
    return [set(O.initial_node_filter(plain, g)) for g in groups]


def stored(test_id, k=0):
    """Stored reference answer `k` of one case (as tests/test_headroom_general_reference.py recorded it)."""
    v = refanswers._load(STORE).get(test_id)
    assert v is not None and len(v) > k, f"no stored reference answers for {test_id}"
    return refanswers.decode(v[k])


# ---- shapes and consequences the CPU twin and the device are both put through ------------------------------------------------------------
def seam_descs(seed, n_wide, n_plain):
    """A mixed cluster with exactly `n_wide` nodes the packer mirrors as wide records among `n_plain` others, in the order drawn."""
    from nhd_amd.matcher import HipMatcher
    from tests.harness.headroom_general_twin import HeadroomGeneralHarnessEngine
    pool = util.mixed_cluster_desc(seed, 4 * (n_wide + n_plain), wide_share=0.6, occupancy=0.1)
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomGeneralHarnessEngine)
    m.HeadroomMany(util.build_cluster(pool), [refmodel.make_topology(NOTHING)])
    assert m.unmirrored == {}
    wide = set(m.wide_nodes)
    out, w, p = [], 0, 0
    for d in pool:
        if d["name"] in wide:
            if w < n_wide:
                out.append(d)
                w += 1
        elif p < n_plain:
            out.append(d)
            p += 1
    assert (w, p) == (n_wide, n_plain)
    return out


# templates of one, two, three and four processing groups, small enough for most nodes to take several
FOUR = [
    dict(map_type="PCI", hugepages_gb=0, misc=1, misc_smt=True,
         groups=[dict(proc=2, helpers=1, rx=10.0, tx=5.0, proc_smt=False, helper_smt=True, gpus=[1])]),
    dict(map_type="NUMA", hugepages_gb=1, misc=0, misc_smt=False,
         groups=[dict(proc=3, helpers=0, rx=5.0, tx=5.0, proc_smt=True, helper_smt=False, gpus=[]),
                 dict(proc=2, helpers=2, rx=22.5, tx=0.0, proc_smt=False, helper_smt=False, gpus=[])]),
    dict(map_type="NUMA", hugepages_gb=0, misc=2, misc_smt=False,
         groups=[dict(proc=2, helpers=0, rx=5.0, tx=12.25, proc_smt=False, helper_smt=False, gpus=[1]),
                 dict(proc=2, helpers=1, rx=0.1, tx=0.0, proc_smt=True, helper_smt=True, gpus=[]),
                 dict(proc=4, helpers=0, rx=0.0, tx=0.0, proc_smt=False, helper_smt=False, gpus=[])]),
    dict(map_type="PCI", hugepages_gb=0, misc=1, misc_smt=False,
         groups=[dict(proc=2, helpers=0, rx=5.0, tx=5.0, proc_smt=False, helper_smt=False, gpus=[]),
                 dict(proc=2, helpers=0, rx=0.0, tx=0.0, proc_smt=True, helper_smt=False, gpus=[]),
                 dict(proc=3, helpers=1, rx=0.0, tx=0.0, proc_smt=False, helper_smt=True, gpus=[]),
                 dict(proc=2, helpers=0, rx=0.0, tx=0.0, proc_smt=False, helper_smt=False, gpus=[])]),
]


GPULESS = dict(map_type="NUMA", hugepages_gb=1, misc=1, misc_smt=False,
               groups=[dict(proc=3, helpers=1, rx=5.0, tx=5.0, proc_smt=False, helper_smt=True, gpus=[]),
                       dict(proc=2, helpers=0, rx=10.0, tx=0.0, proc_smt=True, helper_smt=False, gpus=[])])


def check_sum_is_what_schedule_batch_places(matcher_factory, sharing=False):
    """A GPU-less template on a 60-node mixed cluster: `replicas` of HeadroomMany(general=True) equals what ScheduleBatch(apply=False)
    places out of replicas + 1 copies (one stays unplaced), node by node - the only route to the number without the entry."""
    with sharing_all(sharing):
        nl = util.mixed_cluster(9870, 60, occupancy=0.5)
        top = refmodel.make_topology(GPULESS)
        m = matcher_factory(util.CLOCK)
        h = m.Headroom(nl, top, per_node=True, general=True)
        assert h.error is None and h.not_evaluated == 0 and h.saturated == 0 and h.stopped == 0
        wide = np.array([nm in set(m.wide_nodes) for nm in nl])
        assert h.replicas > 60 and int(h.per_node[wide].sum()) > 20 and (sharing or int(h.per_node[~wide].sum()) > 20)
        got = m.ScheduleBatch(nl, [refmodel.make_topology(GPULESS) for _ in range(h.replicas + 1)], now=util.CLOCK, apply=False)
    placed = [r[0] for r in got if r[0] is not None]
    assert len(placed) == h.replicas
    names = list(nl)
    assert np.array_equal(np.bincount([names.index(nm) for nm in placed], minlength=len(names)), h.per_node)
    return h


def check_a_commit_on_a_wide_winner_takes_one(matcher_factory, sharing=False):
    """FindNode + CommitPlacement on a wide winner lowers that node's count by exactly one and nobody else's."""
    with sharing_all(sharing):
        nl = util.mixed_cluster(9871, 60, occupancy=0.3)
        m = matcher_factory(util.CLOCK)
        m.attach(nl)
        top = refmodel.make_topology(GPULESS)
        before = m.Headroom(nl, top, per_node=True, general=True)
        wide = {nm: nl[nm] for nm in m.wide_nodes}
        assert len(wide) >= 10
        res = m.FindNode(wide, top)
        assert res[0] in wide
        w = list(nl).index(res[0])
        assert before.per_node[w] >= 2
        m.CommitPlacement(res[0], top, res[1])
        after = m.Headroom(nl, refmodel.make_topology(GPULESS), per_node=True, general=True)
    want = before.per_node.copy()
    want[w] -= 1
    assert np.array_equal(after.per_node, want) and not after.flags.any() and after.replicas == before.replicas - 1
    return before
