"""Node.IsBusy at its binary64 boundary, without a GPU.  The reference asks `(now - busy_time) < 30.0` (nhd/Node.py:847-850); every
form of find, explain, the wide-node and the big-pod kernel ask `busy_time >= busy_from` with busy_from = fit_core.h
busy_threshold(now) found on the host.  Here: busy_threshold itself against a bisection in Python's own floats
(tests/busy_check.py) over clocks from 2^-10 to 1e18, and a cluster whose 130 nodes are stamped with the 130 consecutive doubles
around the threshold through the host twin - verdict bitmap, explain's BUSY stage and mode B (which subtracts) against IsBusy
and the Python oracle.  tests/test_busy_boundary_gpu.py holds the device to the same cluster."""
import copy
import functools
import math

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import STAGES, HipMatcher
from oracle import nhd_oracle as O
from tests import busy_check as bc
from tests import harness, sched_standin, util
from tests.harness.explain_twin import ExplainHarnessEngine
from workload import refmodel
from workload.refmodel import NFD

N_NODES = 130                   # two full 64-node chunks and a ragged tail of two
BUSY, FITS = STAGES.index("BUSY"), STAGES.index("FITS")


# ---- busy_threshold itself ---------------------------------------------------------------------------------------------------------
def disagreements(clocks):
    """(now, busy_threshold(now), least_busy(now)) wherever the two differ."""
    return [(now, got, want) for now in clocks for got, want in [(harness.busy_threshold(now), bc.least_busy(now))] if got != want]


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_threshold_at_the_listed_clocks(now):
    want = bc.self_check(now)
    got = harness.busy_threshold(now)
    print(f"now {now!r}: busy_threshold {got!r}, least busy double {want!r}")
    assert got == want


def test_threshold_at_zero_and_around_the_powers_of_two():
    clocks = [0.0]
    for e in range(-10, 61):
        p = 2.0 ** e
        clocks += [math.nextafter(p, 0.0), p, math.nextafter(p, math.inf)]
    for now in clocks:
        bc.self_check(now)
    bad = disagreements(clocks)
    assert not bad, (len(bad), bad[:5])


def test_threshold_at_seeded_clocks():
    """5 000 clocks uniform in [29, 31] - around the interval (29.75, 30.25) in which `now - 30.0` is exact and its ulp far finer
    than the threshold's distance from it - and 20 000 log-uniform in [1e-3, 1e18]."""
    rng = np.random.default_rng(3030)
    near = rng.uniform(29.0, 31.0, 5000).tolist()
    wide = (10.0 ** rng.uniform(-3.0, 18.0, 20000)).tolist()
    for now in near[:200] + wide[:200]:
        bc.self_check(now)
    bad = disagreements(near + wide)
    inside = [b for b in bad if 29.75 < b[0] < 30.25]
    print(f"{len(bad)} of {len(near) + len(wide)} clocks disagree, {len(inside)} of them in (29.75, 30.25)")
    assert not bad, (len(bad), len(inside), bad[:5])


# ---- the cluster around the threshold ----------------------------------------------------------------------------------------------
def node_labels():
    """An SMT node of two sockets, 16 physical cores, two 100 Gb/s NICs and two GPUs each, every NIC and GPU of a socket on one switch."""
    lab = {NFD + "nfd-extras-cpu.numSockets": "2", NFD + "nfd-extras-cpu.num_cores": "32", NFD + "cpu-hardware_multithreading": "true",
           "DATA_PLANE_VLAN": "7", "DATA_DEFAULT_GW": "10.1.0.1/32"}
    for j in range(4):
        numa = j // 2
        lab[NFD + f"nfd-extras-nic.eth{j}.mlx.{0xABC000 + j:012x}.100000Mbs.{numa}.{0x10 * (numa + 1):x}.{j}.0"] = "true"
        lab[NFD + f"nfd-extras-gpu.{j}.V100.{numa}.{0x10 * (numa + 1):x}"] = "true"
    return lab


def stamped_descs(stamps):
    return [dict(name=f"n{i:04d}", labels=node_labels(), hugepages=[16, 16], active=True, used_cores=[], used_gpus=[], nic_pods_used=[],
                 busy_time=t) for i, t in enumerate(stamps)]


def stamped_cluster(now, stamps=None):
    """130 identical idle nodes, node i stamped with the (i - 64)-th double counted from least_busy(now); the expected busy vector."""
    stamps = bc.stamps(now, N_NODES) if stamps is None else stamps
    nl = {d["name"]: refmodel.build_node(d) for d in stamped_descs(stamps)}
    busy = np.array([bc.is_busy(now, t) for t in stamps])
    assert 0 < int(busy.sum()) < N_NODES, "both answers are in the case"
    assert [float(nd.busy_time) for nd in nl.values()] == list(stamps)
    return nl, busy


def _group(gpus=(), rx=5.0, tx=5.0):
    return dict(proc=2, helpers=0, rx=rx, tx=tx, proc_smt=True, helper_smt=True, gpus=list(gpus))


def pod_specs():
    """One-, three- and four-group pods with a GPU, a pod without, and a five-group pod with a GPU (the general path)."""
    def pod(groups, map_type="NUMA"):
        return dict(map_type=map_type, hugepages_gb=0, misc=1, misc_smt=True, groups=groups)
    return [pod([_group([1])]),
            pod([_group([1]), _group(), _group()], "PCI"),
            pod([_group(), _group([1]), _group(), _group([1])]),
            pod([_group()]),
            pod([_group(), _group(), _group([1]), _group(), _group()])]


GPU_PODS, PLAIN_POD, BIG_POD = (0, 1, 2, 4), 3, 4


def pods():
    tops = [refmodel.make_topology(s) for s in pod_specs()]
    assert [len(t.proc_groups) for t in tops] == [1, 3, 4, 1, 5] and pack.needs_general_path(tops[BIG_POD])
    assert [any(len(pg.group_gpus) for pg in t.proc_groups) for t in tops] == [True, True, True, False, True]
    return tops


def jsonable(res):
    if res[0] is None:
        return [None]
    return [res[0], {"gpu": [int(x) for x in res[1]["gpu"]], "cpu": [int(x) for x in res[1]["cpu"]], "nic": [[int(a), int(b)] for a, b in res[1]["nic"]]}]


def bits_of(bitmap, p, n=N_NODES):
    """Column p of a chunk-major verdict bitmap [chunks][P] as n booleans."""
    return np.unpackbits(np.ascontiguousarray(bitmap[:, p]).view(np.uint8), bitorder="little").astype(bool)[:n]


def around_threshold(nl):
    """The eight nodes next to the threshold: four stamped under it, the one stamped with it, three above."""
    return {nm: nl[nm] for nm in list(nl)[60:68]}


def boundary_batch(tops):
    """The five pods and three more one-group GPU pods: more pods with GPUs than around_threshold() has nodes under the threshold
    (each commit stamps its node with `now`), so the last node mode B fills is the one stamped just under the threshold."""
    return list(tops) + [tops[0]] * 3


def check_mode_b(m, nl, busy, now):
    """ScheduleBatch of matcher `m` against the oracle's loop: the five pods on the whole cluster, then boundary_batch() on the
    nodes around the threshold, which it fills up to the threshold exactly."""
    names = list(nl)
    tops = pods()
    for cluster, batch in ((nl, tops), (around_threshold(nl), boundary_batch(tops))):
        got = m.ScheduleBatch(cluster, batch, now=now)
        want = O.schedule_sequence(copy.deepcopy(cluster), batch, [None] * len(batch), now)
        assert [jsonable(r) for r in got] == [jsonable(w) for w in want]
        gpu_pods = [p for p in range(len(batch)) if p > BIG_POD or p in GPU_PODS]
        gpu_nodes = [names.index(got[p][0]) for p in gpu_pods if got[p][0] is not None]
        assert gpu_nodes and not busy[gpu_nodes].any() and len(set(gpu_nodes)) == len(gpu_nodes)
        assert got[PLAIN_POD][0] is not None
    # the second batch took every node under the threshold, the one stamped just below it last, and its other pods stay pending
    free = [i for i in range(60, 68) if not busy[i]]
    assert gpu_nodes == free and 0 < len(free) < len(gpu_pods)
    assert [got[p][0] is None for p in gpu_pods] == [False] * len(free) + [True] * (len(gpu_pods) - len(free))


def schedule_one_check(now, matcher_factory):
    """The five pods, pod after pod, through ScheduleOne in attached mode with the scheduler's own mutators behind each call,
    against the oracle's find_node + commit on a second copy of the cluster: a node that has just been committed to is stamped
    `now` and is busy for the next pod with GPUs at the same clock."""
    clock = lambda: now                                               # noqa: E731
    nl, busy = stamped_cluster(now)
    nl = sched_standin.adopt(nl, clock)
    ref_nl, _ = stamped_cluster(now)
    names = list(nl)
    m = matcher_factory(clock)
    m.attach(nl)
    taken = []
    for p, (top, ref_top) in enumerate(zip(pods(), pods())):
        want = O.find_node(ref_nl, ref_top, now)
        rec = {}
        O.commit(ref_nl[want[0]], ref_top, want[1], now, rec)
        got = m.ScheduleOne(nl, top)
        assert jsonable(got) == jsonable(want), p
        assert m.last_placements == [rec], p
        assert sched_standin.attempt_scheduling(nl, m, top, None, match=got) == want[0]
        if p in GPU_PODS:
            assert not busy[names.index(want[0])] and want[0] not in taken, p
            taken.append(want[0])
    assert all(nl[nm].busy_time == now for nm in taken)
    return m


@functools.lru_cache(maxsize=None)
def _mixed_cluster():
    """util.mixed_cluster (built once; every check writes its own stamps over it) and, per (pod, node), whether the oracle lets
    the pod onto the node with the busy window out of the way."""
    nl = util.mixed_cluster(3030, N_NODES, occupancy=0.1)
    for nd in nl.values():
        nd.busy_time = -1.0e300
    idle = np.array([[O.feasible(nd, top, 0.0) for nd in nl.values()] for top in pods()])
    return nl, idle


def mixed_cluster_check(now, matcher_factory):
    """util.mixed_cluster with the stamps around the threshold written over it: the verdict of every (pod, node) pair - wide
    nodes by the wide-node pass, the five-group pod by the big-pod pass - against the oracle on that node alone."""
    stamps = bc.stamps(now, N_NODES)
    nl, idle = _mixed_cluster()
    for nd, t in zip(nl.values(), stamps):
        nd.busy_time = t
    busy = np.array([bc.is_busy(now, t) for t in stamps])
    tops = pods()
    m = matcher_factory(lambda: now)
    found = m.FindNodes(nl, tops, now=now)
    assert [jsonable(r) for r in found] == [jsonable(O.find_node(nl, t, now)) for t in tops]
    assert m.unmirrored == {}
    nodes = list(nl.values())
    wide = np.array([nm in set(m.wide_nodes) for nm in nl])
    maint = np.array([bool(nd.maintenance) for nd in nodes])
    assert (wide & busy).any() and (wide & ~busy).any(), "the wide nodes' stamps straddle the threshold"
    feas = np.array([[O.feasible(nd, top, now) for nd in nodes] for top in tops])
    for p in range(len(tops)):
        assert np.array_equal(feas[p], idle[p] if p == PLAIN_POD else idle[p] & ~busy), p
    for p in (0, 2, BIG_POD):                                         # IsBusy alone decides wide nodes, both ways (the PCI pod fits too few of them)
        assert (idle[p] & wide & busy).any() and (idle[p] & wide & ~busy).any(), p
    small = [p for p in range(len(tops)) if p != BIG_POD]
    reqs = m.packer.digest_many([tops[p] for p in small])
    _, bitmap, _ = m.engine.find(reqs, now, want_bitmap=True, want_map=False)
    for k, p in enumerate(small):
        got = bits_of(bitmap, k)
        assert np.array_equal(got, feas[p]), (p, [nodes[i].name for i in np.flatnonzero(got != feas[p])])
    for p, e in enumerate(m.ExplainNodes(nl, tops, now=now, per_node=True)):
        assert e.error is None
        assert np.array_equal(e.stages == FITS, feas[p]), (p, [nodes[i].name for i in np.flatnonzero((e.stages == FITS) != feas[p])])
        want_busy = np.zeros(N_NODES, bool) if p == PLAIN_POD else busy & ~maint
        assert np.array_equal(e.stages == BUSY, want_busy), (p, [nodes[i].name for i in np.flatnonzero((e.stages == BUSY) != want_busy)])
    return m


def test_an_idle_node_takes_every_pod():
    nl, _ = stamped_cluster(bc.CLOCKS[0])
    node = next(iter(nl.values()))
    node.busy_time = -1.0e9
    assert all(O.feasible(node, top, 1.0e6) for top in pods())


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_verdicts_and_stages_through_the_host_twin(now):
    """The find forms' `busy_time >= busy_from` on every node around the threshold: verdict bitmap ~busy for a pod with GPUs, all
    ones for one without; the general path's verdicts for the five-group pod; explain's BUSY stage exactly on the busy nodes."""
    nl, busy = stamped_cluster(now)
    tops = pods()
    m = HipMatcher(clock=lambda: now, engine_factory=ExplainHarnessEngine)
    found = m.FindNodes(nl, tops, now=now)
    assert [jsonable(r) for r in found] == [jsonable(O.find_node(nl, t, now)) for t in tops]
    names = list(nl)
    for p in GPU_PODS:
        assert found[p][0] is not None and not busy[names.index(found[p][0])], p
    small = [p for p in range(len(tops)) if p != BIG_POD]
    reqs = m.packer.digest_many([tops[p] for p in small])
    _, bitmap, _ = m.engine.find(reqs, now, want_bitmap=True, want_map=False)
    for k, p in enumerate(small):
        want = np.ones(N_NODES, bool) if p == PLAIN_POD else ~busy
        assert np.array_equal(bits_of(bitmap, k), want), (p, np.flatnonzero(bits_of(bitmap, k) != want).tolist())
    big = np.array([m.packer.digest_big(tops[BIG_POD])], dtype=pack.BIG_REQ)
    fits, _, exhausted = harness.big_eval(m.packer, m.engine.table, m.engine._wide_records(), big, now)
    assert not exhausted and np.array_equal(fits[:, 0].astype(bool), ~busy)
    for p, e in enumerate(m.ExplainNodes(nl, tops, now=now, per_node=True)):
        assert e.error is None
        if p == PLAIN_POD:
            assert (e.stages == FITS).all(), p
        else:
            assert np.array_equal(e.stages == BUSY, busy), (p, np.flatnonzero((e.stages == BUSY) != busy).tolist())
            assert (e.stages[~busy] == FITS).all(), p
            assert e.counts["BUSY"] == int(busy.sum())


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_mode_b_through_the_host_twin(now):
    """ScheduleBatch (snapshot rows from the threshold form, refreshed after each commit by the subtraction form) against the
    oracle's loop at the same clock: each commit stamps its node with `now`, so later pods with GPUs skip it."""
    nl, busy = stamped_cluster(now)
    check_mode_b(HipMatcher(clock=lambda: now, engine_factory=harness.HarnessEngine), nl, busy, now)


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_schedule_one_through_the_host_twin(now):
    schedule_one_check(now, lambda clock: HipMatcher(clock=clock, engine_factory=harness.HarnessEngine))


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_wide_nodes_and_the_big_pod_through_the_host_twin(now):
    mixed_cluster_check(now, lambda clock: HipMatcher(clock=clock, engine_factory=ExplainHarnessEngine))
