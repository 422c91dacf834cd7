"""Pins oracle/nhd_oracle.py (the CPU restatement) to the UNMODIFIED reference: live where the reference tree exists,
through its stored answers elsewhere (tests/refanswers.py)."""
import numpy as np
import pytest

from workload import refmodel, synth
from oracle import nhd_oracle as O
from tests import util


class _Clock:
    t = util.CLOCK


@pytest.fixture
def refclock(refans):
    from oracle import ref_loader
    return ref_loader.VirtualClock(util.CLOCK).install() if refans.live else _Clock()


@pytest.mark.parametrize("seed", range(12))
def test_random_clusters_match_reference(refans, refclock, seed):
    from oracle import ref_loader
    ref = refans.ref
    nl = util.random_cluster(1000 + seed, 24, ref)
    rng = np.random.default_rng(seed)
    hits = 0
    for _ in range(25):
        spec = util.random_pod_spec(rng)
        top = refmodel.make_topology(spec, ref)
        want = refans.take(lambda: ref_loader.find_node(nl, top))
        got = O.find_node(nl, top, util.CLOCK)
        assert got == want, (spec, got, want)
        hits += want[0] is not None
    assert hits > 0


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_synthetic_configs_match_reference(refans, refclock, cfg):
    from oracle import ref_loader
    ref = refans.ref
    spec = synth.make_cluster(cfg, n_nodes=48)
    refclock.t = spec.clock_now
    nl = spec.build_nodes(ref)
    pods, pgroups = synth.make_pods(cfg, n_pods=12)
    for ps, pg in zip(pods, pgroups):
        top = refmodel.make_topology(ps, ref)
        sub = O.initial_node_filter(nl, pg)
        assert O.find_node(sub, top, spec.clock_now) == refans.take(lambda: ref_loader.find_node(sub, top))
    refclock.t = util.CLOCK


def _parsed(n):
    return ((n.sockets, n.numa_nodes, n.smt_enabled, n.cores_per_proc, n.groups, n.maintenance),
            [(c.core, c.socket, c.sibling, c.used) for c in n.cores],
            [(k.ifname, k.speed, k.numa_node, k.pciesw, k.idx, k.mac) for k in n.nics],
            [(g.device_id, g.numa_node, g.pciesw) for g in n.gpus],
            n.mem.free_hugepages_gb)


def test_standins_parse_like_reference(refans):
    rng = np.random.default_rng(5)
    for i in range(40):
        lab = util.random_labels(rng)

        def parse():
            a = refans.ref.Node("x"); assert a.ParseLabels(lab); a.SetHugepages(16, 9)
            return _parsed(a)
        a = refans.take(parse)
        b = _parsed(refmodel.node_from_labels("x", lab, (16, 9)))
        for x, y in zip(a, b):
            assert x == y


def test_oracle_same_on_standins_and_reference_objects(refans, refclock):
    """The oracle reads objects by attribute only: stand-ins and reference objects must agree."""
    rng = np.random.default_rng(77)
    nl_ref = util.random_cluster(4242, 20, refans.ref) if refans.live else None
    nl_std = util.random_cluster(4242, 20, None)
    for _ in range(30):
        spec = util.random_pod_spec(rng)
        assert refans.take(lambda: O.find_node(nl_ref, refmodel.make_topology(spec, refans.ref), util.CLOCK)) == \
               O.find_node(nl_std, refmodel.make_topology(spec), util.CLOCK)
