"""nhdfit_headroom's arithmetic on the CPU: the kernel's own per-node loop (headroom_kernel.h headroom_run_wave: the wavefront forms
of the mapping and of the commit step) on emulated lanes against the scalar twin on the same inputs; the cap; the two consequences of
the definition (the sum over the nodes is what the scheduler's loop places, a commit takes exactly one from its node); wide nodes
and ENABLE_SHARING mirrors are NOT_EVALUATED and add nothing."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from tests import edge_check, explain_check, harness, util
from tests.harness import headroom_twin
from tests.harness.headroom_twin import HeadroomHarnessEngine, HeadroomWaveEngine
from workload import planes, refmodel, synth

COUNT, STOPPED, NOT_EVALUATED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED, pack.HEADROOM_NOT_EVALUATED
NOTHING = dict(map_type="NUMA", hugepages_gb=0, misc=0, misc_smt=False,
               groups=[dict(proc=0, helpers=0, rx=0.0, tx=0.0, proc_smt=False, helper_smt=False, gpus=[])])


def _both(nl, tops, clock=util.CLOCK, **kw):
    a = HipMatcher(clock=lambda: clock, engine_factory=HeadroomHarnessEngine).HeadroomMany(nl, tops, per_node=True, **kw)
    b = HipMatcher(clock=lambda: clock, engine_factory=HeadroomWaveEngine).HeadroomMany(nl, tops, per_node=True, **kw)
    return a, b


def _same(a, b):
    for x, y in zip(a, b):
        assert x.error is None and y.error is None
        assert np.array_equal(x.per_node, y.per_node) and np.array_equal(x.flags, y.flags)
        assert (x.replicas, x.nodes_with_room, x.max_on_one_node, x.saturated, x.stopped, x.not_evaluated, x.form) == \
               (y.replicas, y.nodes_with_room, y.max_on_one_node, y.saturated, y.stopped, y.not_evaluated, y.form)


@pytest.mark.parametrize("seed", range(3))
def test_wavefront_loop_equals_the_scalar_twin_on_random_clusters(seed):
    """Heterogeneous clusters - one-socket nodes among them, which the wavefront instantiation answers without the set model - and
    pods of one to four groups (the fourth: the generic instantiation), NUMA / PCI / invalid."""
    rng = np.random.default_rng(9600 + seed)
    nl = util.random_cluster(9600 + seed, 120, occupancy=0.1)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(30)]
    a, b = _both(nl, tops, max_per_node=64)
    _same(a, b)
    assert sum(x.replicas for x in a) > 50
    one_socket = np.array([nd.sockets == 1 for nd in nl.values()])
    assert one_socket.any() and sum(int(x.per_node[one_socket].sum()) for x in a) > 0      # the one-NUMA-node shortcut is exercised
    forms = {x.form for x in a}
    assert forms == {pack.HEADROOM_FORM_WAVE, pack.HEADROOM_FORM_GENERIC}


def test_wavefront_loop_equals_the_scalar_twin_at_the_edges_of_the_record_formats():
    """workload/edge_inputs.py's clusters (sockets of 33..64 cores, 9..16 NICs per NUMA node, pods_used up to 3, free hugepages around
    the tile's table) and pods; the runs that end at a commit the reference raises on included."""
    replicas = stopped = 0
    for seed in (2, 9, 12, 22, 30, 33):
        descs, specs = edge_check.wave_case(seed)
        a, b = _both(util.build_cluster(descs), [refmodel.make_topology(s) for s in specs], max_per_node=8)
        _same(a, b)
        replicas += sum(x.replicas for x in a)
        stopped += sum(x.stopped for x in a)
    assert replicas >= 40 and stopped >= 1, (replicas, stopped)


@pytest.mark.parametrize("cfg", [2, 3, 4, 5])
def test_wavefront_loop_equals_the_scalar_twin_on_synth(cfg):
    spec = synth.make_cluster(cfg, n_nodes=160)
    specs, groups = synth.make_pods(cfg, n_pods=24)
    a, b = _both(spec.build_nodes(), [refmodel.make_topology(s) for s in specs], clock=spec.clock_now)
    _same(a, b)
    assert sum(x.replicas for x in a) > 500


@pytest.mark.parametrize("engine", [HeadroomHarnessEngine, HeadroomWaveEngine], ids=["scalar", "wave"])
def test_cap(engine):
    """A template that asks for nothing fits for ever: every candidate that takes it at all is reported as max_per_node and counted
    in `saturated`; with a larger cap the same nodes, the larger number."""
    nl = util.random_cluster(9700, 80)
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=engine)
    top = refmodel.make_topology(NOTHING)
    h = m.Headroom(nl, top, per_node=True, max_per_node=23)
    assert set(np.unique(h.per_node).tolist()) == {0, 23}
    full = int((h.per_node == 23).sum())
    assert full > 20 and (h.saturated, h.replicas, h.max_on_one_node, h.nodes_with_room) == (full, 23 * full, 23, full)
    assert "reached the limit of 23 per node" in h.summary()
    h2 = m.Headroom(nl, top, per_node=True, max_per_node=150)
    assert np.array_equal(h2.per_node == 150, h.per_node == 23) and h2.saturated == full
    sub = {k: v for i, (k, v) in enumerate(nl.items()) if i % 2}       # candidates only
    h3 = m.Headroom(sub, top, per_node=True, max_per_node=23)
    assert h3.nodes == len(sub) and h3.by_node() == {k: v for k, v in h.by_node().items() if k in sub}
    with pytest.raises(ValueError):
        m.Headroom(nl, top, max_per_node=0)
    with pytest.raises(ValueError):
        m.Headroom(nl, top, max_per_node=1 << 14)


@pytest.mark.parametrize("cfg", [2, 4])
def test_sum_is_what_the_scheduler_loop_places(cfg):
    """Consequence 1: a commit only changes its own node and the replicas are identical, so for a GPU-less template the sum over the
    nodes equals the placements ScheduleBatch(apply=False) makes from replicas + 1 copies - node by node."""
    spec = synth.make_cluster(cfg, n_nodes=200)
    all_specs, _ = synth.make_pods(cfg, n_pods=128)
    specs = [s for s in all_specs if not any(g["gpus"] for g in s["groups"])][:4]
    nl = spec.build_nodes()
    names = list(nl)
    m = HipMatcher(clock=lambda: spec.clock_now, engine_factory=HeadroomHarnessEngine)
    for s in specs:
        top = refmodel.make_topology(s)
        h = m.Headroom(nl, top, per_node=True)
        assert h.replicas > 50 and h.saturated == 0 and h.stopped == 0
        res = m.ScheduleBatch(nl, [refmodel.make_topology(s) for _ in range(h.replicas + 1)], apply=False)
        placed = [r[0] for r in res if r[0] is not None]
        assert len(placed) == h.replicas
        assert np.array_equal(np.bincount([names.index(x) for x in placed], minlength=len(names)), h.per_node)


def test_a_commit_takes_one_from_its_node():
    """Consequence 2: committing one replica of the template (the winner FindNode picks, the host build's commit step on the mirror)
    lowers that node's headroom for the template by exactly one and nobody else's - replica after replica, until nothing fits."""
    spec = synth.make_cluster(4, n_nodes=96)
    specs, _ = synth.make_pods(4, n_pods=12)
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    none = np.zeros(0, pack.WIDE)
    total = 0
    for s in specs[:6]:
        req = pk.digest_many([refmodel.make_topology(s)])
        pk.close_signatures()
        t = pack.NodeTable(list(table.names), *[np.array(getattr(table, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")], np.array(table.origin))
        _, counts = headroom_twin.headroom(pk, t, none, req)
        for _ in range(40):
            score, _, maps = harness.find(pk, t, req, spec.clock_now + 1.0e6)          # (nothing is busy by then)
            if not score[0]:
                break
            w = int(0x7FFFFFFFFFFFFFFF - (int(score[0]) & 0x7FFFFFFFFFFFFFFF))
            status, _ = harness.commit(pk, t, w, req[0], maps[0], 0.0)
            assert status == 0
            _, after = headroom_twin.headroom(pk, t, none, req)
            want = counts.copy()
            assert want[0, w] & COUNT >= 1
            want[0, w] -= 1
            assert np.array_equal(after, want)
            counts = after
            total += 1
        else:
            continue
        assert (counts & COUNT).sum() == 0                   # FindNode finds nothing exactly when no node has headroom left
    assert total > 100


def test_wide_nodes_are_not_evaluated():
    nl = util.mixed_cluster(9800, 90)
    rng = np.random.default_rng(98)
    tops = [refmodel.make_topology(NOTHING)] + [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(10)]
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomHarnessEngine)
    got = m.HeadroomMany(nl, tops, per_node=True, max_per_node=9)
    _same(got, HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomWaveEngine).HeadroomMany(nl, tops, per_node=True, max_per_node=9))
    wide = np.array([nm in set(m.wide_nodes) for nm in nl])
    assert 10 < wide.sum() < len(nl) - 10
    for h in got:
        assert ((h.flags & NOT_EVALUATED) != 0).tolist() == wide.tolist() and h.not_evaluated == int(wide.sum())
        assert (h.per_node[wide] == 0).all() and h.replicas == int(h.per_node[~wide].sum())
        assert f"{int(wide.sum())} not evaluated" in h.summary()
    assert got[0].replicas > 0
    # only the ordinary nodes as candidates: nothing is left unevaluated
    sub = {k: v for k, v in nl.items() if k not in set(m.wide_nodes)}
    for h, full in zip(m.HeadroomMany(sub, tops, per_node=True, max_per_node=9), got):
        assert h.not_evaluated == 0 and h.replicas == full.replicas and np.array_equal(h.per_node, full.per_node[~wide])


def test_a_sharing_mirror_is_not_evaluated():
    """ENABLE_SHARING: every node is mirrored for the general path - every entry carries NOT_EVALUATED, `replicas` is 0."""
    with explain_check.sharing_flag(True):
        nl = util.random_cluster(9900, 30)
        tops = [refmodel.make_topology(NOTHING), refmodel.make_topology(util.random_pod_spec(np.random.default_rng(99)))]
        m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomHarnessEngine)
        got = m.HeadroomMany(nl, tops, per_node=True)
    assert m.packer.sharing
    for h in got:
        assert h.error is None and h.not_evaluated == len(nl) and h.replicas == 0 and h.nodes_with_room == 0
        assert (h.flags == NOT_EVALUATED).all() and (h.per_node == 0).all()
