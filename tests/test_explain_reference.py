"""nhdfit_explain's stage function (nhd_amd/csrc/explain_core.h) on its host build, through HipMatcher.ExplainNodes, against
the stage at which the UNMODIFIED reference drops each node (tests/explain_reference.py: derived from its own intermediate
results; live where the reference tree exists, its stored answers elsewhere - tests/refanswers.py).  Also: FITS is exactly
the oracle's verdict, and the counts account for every node of `nl`."""
import numpy as np
import pytest

from nhd_amd.matcher import STAGES, UNMIRRORED, HipMatcher
from oracle import nhd_oracle as O
from tests import explain_check, util
from tests.explain_reference import FITS, reference_stages
from tests.harness.explain_twin import ExplainHarnessEngine
from tests.test_big_core import big_spec
from tests.test_big_vs_reference import few_nics
from workload import refmodel


@pytest.fixture
def refclock(refans):
    from oracle import ref_loader
    return ref_loader.VirtualClock(util.CLOCK).install() if refans.live else None


def _check(refans, descs, specs, sharing=False):
    ref = refans.ref
    nl = util.build_cluster(descs)
    names = list(nl)
    tops = [refmodel.make_topology(s) for s in specs]
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=ExplainHarnessEngine)
    got = m.ExplainNodes(nl, tops, per_node=True)
    assert len(got) == len(tops)
    if refans.live:
        if sharing:
            ref.node_mod.ENABLE_SHARING = True
        nl_ref = util.build_cluster(descs, ref)
    seen = set()
    try:
        for s, top, e in zip(specs, tops, got):
            want = refans.take(lambda: [reference_stages(ref, nl_ref, refmodel.make_topology(s, ref))[n] for n in nl_ref])
            assert e.stages.tolist() == want, (s, e.stages.tolist(), want)
            assert e.unmirrored == 0 and sum(e.counts.values()) == len(nl)
            assert [e.counts[st] for st in STAGES] == np.bincount(e.stages, minlength=len(STAGES)).tolist()
            if s["map_type"] in ("NUMA", "PCI"):
                assert [x == FITS for x in want] == [O.evaluate_node(nl[n], top, util.CLOCK) is not None for n in names], s
            seen.update(want)
    finally:
        if refans.live and sharing:
            ref.node_mod.ENABLE_SHARING = False
    return seen


@pytest.mark.parametrize("seed", range(4))
def test_random_clusters(refans, refclock, seed):
    """Ordinary nodes with maintenance, hugepage-short and busy ones; NUMA, PCI, invalid and GPU-less pods."""
    rng = np.random.default_rng(7300 + seed)
    descs = util.random_cluster_desc(7300 + seed, 24)
    specs = [util.random_pod_spec(rng, max_groups=4) for _ in range(24)]
    for s in specs[::3]:
        for g in s["groups"]:
            g["gpus"] = []
    seen = _check(refans, descs, specs)
    assert len(seen) >= 6, seen


def test_every_stage_is_reached(refans, refclock):
    """Over a few clusters the random pods hit every stage but NOT_CANDIDATE (stage 0 has its own test on the device)."""
    seen = set()
    for seed in range(3):
        rng = np.random.default_rng(7400 + seed)
        descs = util.random_cluster_desc(7400 + seed, 20, occupancy=0.5)
        specs = [util.random_pod_spec(rng, max_groups=4) for _ in range(20)]
        for s in specs:
            if s["map_type"] == "NONE":
                s["map_type"] = "PCI"
        seen |= _check(refans, descs, specs)
    assert seen >= set(range(1, 10)), sorted(seen)


@pytest.mark.parametrize("seed", range(2))
def test_big_pods(refans, refclock, seed):
    """Pods with 5..8 processing groups (nhdfit_explain_big) on ordinary and wide nodes."""
    rng = np.random.default_rng(7500 + seed)
    descs = few_nics(util.mixed_cluster_desc(7500 + seed, 12, wide_share=0.3 if seed else 0.0, occupancy=0.08), 3)
    specs = [big_spec(rng, 5, 6 if seed else 7) for _ in range(6)]
    _check(refans, descs, specs)


@pytest.mark.parametrize("seed", range(2))
def test_wide_nodes(refans, refclock, seed):
    """mixed_cluster: 3- and 4-socket nodes and sockets of up to 128 cores, answered by their wide records."""
    rng = np.random.default_rng(7600 + seed)
    descs = few_nics(util.mixed_cluster_desc(7600 + seed, 16, wide_share=0.5), 4)
    specs = [util.random_pod_spec(rng, max_groups=3) for _ in range(16)]
    _check(refans, descs, specs)


@pytest.fixture
def sharing(monkeypatch):
    monkeypatch.setattr(refmodel, "ENABLE_SHARING", True)
    monkeypatch.setattr(O, "ENABLE_SHARING", True)


def test_sharing_cluster(refans, refclock, sharing):
    """nhd/Node.py:20 ENABLE_SHARING = True: NICs priced at speed * pct - speed_used (every node a wide record with its share)."""
    rng = np.random.default_rng(7700)
    descs = util.random_cluster_desc(7700, 14, occupancy=0.1)
    for d in descs:
        d["nic_speed_used"] = [[float(rng.choice([0, 0, 10, 20, 22.5, 47.5])), float(rng.choice([0, 0, 5, 15, 89.5]))] for _ in d["nic_pods_used"]]
    specs = [util.random_pod_spec(rng, max_groups=3) for _ in range(16)]
    _check(refans, descs, specs, sharing=True)


def test_subsets_unmirrored_nodes_and_the_summary():
    """The host logic of ExplainNodes: a subset of the attached dict (nodes outside it are not counted), a node no layout holds
    (reported on its own, UNMIRRORED per node), and the Kubernetes-style sentence."""
    descs = util.random_cluster_desc(7800, 40)
    nl = util.build_cluster(descs)
    names = list(nl)
    odd = refmodel.build_node(dict(descs[3], name=names[3]))
    odd.numa_nodes = odd.sockets = 9                      # beyond both layouts: never mirrored
    nl[names[3]] = odd
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=ExplainHarnessEngine)
    m.attach(nl)
    assert names[3] in m.unmirrored
    sub = {n: nl[n] for n in names[::2]}
    rng = np.random.default_rng(78)
    tops = [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(6)]
    for e, top in zip(m.ExplainNodes(sub, tops, per_node=True), tops):
        assert e.unmirrored == 0 and e.total == len(sub) and len(e.stages) == len(sub)
        want = [O.evaluate_node(sub[n], top, util.CLOCK) is not None for n in sub] if top.map_type.name.endswith(("NUMA", "PCI")) else None
        if want is not None:
            assert [x == FITS for x in e.stages] == want
    e = m.ExplainNode(nl, tops[0], per_node=True)
    assert e.unmirrored == 1 and e.stages[3] == UNMIRRORED and e.total == len(nl)
    text = e.summary()
    assert text.startswith(f"{e.counts['FITS']}/{len(nl)} nodes are available") and "1 not mirrored on the device" in text
    res = m.FindNode(nl, tops[0])
    assert (res[0] is None) == (e.counts["FITS"] == 0)


@pytest.mark.parametrize("golden", explain_check.IDS)
def test_goldens(refans, golden):
    """The reference-generated fixtures, every pod against the fixture's cluster: the host build's stage for every (pod, node) is
    the reference's.  These stored answers are what tests/test_explain_gpu.py holds the device to."""
    path = explain_check.GOLDENS[explain_check.IDS.index(golden)]
    want = refans.take(lambda: explain_check.reference(path, refans.ref))
    got = explain_check.explain(path, lambda clock: HipMatcher(clock=lambda: clock, engine_factory=ExplainHarnessEngine))
    assert got == want
