"""HipMatcher.ScheduleOne - FindNode and the commit step for one pod in one device call - on the host twin (no GPU needed).
The harness engine has no find_commit, so every call here takes the form ScheduleOne composes from FindNodes + CommitPlacement; the
bookkeeping around it (ids queued for the scheduler's own mutators, the busy time SetBusy writes afterwards, unapplied placements)
is the same code the one-launch form runs behind (tests/test_schedule_one_gpu.py holds that form to the same replays on the device).
`one_check` below is shared with the GPU file."""
import ctypes

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from oracle import nhd_oracle as O
from tests import harness, sched_check, sched_standin, util
from tests.test_big_core import big_spec
from tests.test_wide_core import norm
from workload import refmodel, synth


class TickingClock:
    """A clock that moves on every reading (time.monotonic under a scheduler): the time SetBusy stamps is later than the one the
    match - and with it ScheduleOne's commit - read."""

    def __init__(self, t, step=0.0005):
        self.t, self.step, self.readings = t, step, []

    def __call__(self):
        self.t += self.step
        self.readings.append(self.t)
        return self.t


def ids_written_into(node, top):
    """What SetPhysicalIdsFromMapping wrote into the pod's topology, in pack.expand_placement's terms."""
    pos = {g.device_id: k for k, g in enumerate(node.gpus)}
    return {"groups": [{"cores": [c.core for g in pg.group_gpus for c in g.cpu_cores] + [c.core for c in pg.proc_cores],
                        "helpers": [c.core for c in pg.misc_cores], "gpus": [pos[g.device_id] for g in pg.group_gpus]}
                       for pg in top.proc_groups], "misc": [c.core for c in top.misc_cores]}


def one_check(case, clock, engine_factory=None, devices=None):
    """The scheduler loop of a tests/golden/sched fixture with ScheduleOne where sched_standin.attempt_scheduling calls FindNode.
    Returns everything a test wants to look at."""
    spec = synth.make_cluster(case["config"], n_nodes=case["n_nodes"])
    pods, groups = synth.make_pods(case["config"], n_pods=case["n_pods"])
    for p in pods:
        p["misc_smt"] = True
    nodes = sched_standin.adopt(spec.build_nodes(), clock)
    tops = [refmodel.make_topology(p) for p in pods]
    m = HipMatcher(clock=clock, engine_factory=engine_factory, devices=devices)
    events = []                                                  # (pod index, what, detail) of every engine call inside the loop
    state = {"pod": -1}
    eng = m.engine

    def spy(name, detail=lambda a, k: None):
        orig = getattr(eng, name, None)
        if orig is None:
            return

        def wrapped(*a, **k):
            events.append((state["pod"], name, detail(a, k)))
            return orig(*a, **k)
        setattr(eng, name, wrapped)
    for name in ("upload", "find", "commit", "find_commit"):
        spy(name)
    spy("apply_deltas", lambda a, k: [int(x) for x in np.asarray(a[0]).reshape(-1)["op"]])
    m.attach(nodes)
    del events[:]
    binds, called_at = [], []
    for k, (top, grp) in enumerate(zip(tops, groups)):
        state["pod"] = k
        if hasattr(clock, "readings"):
            called_at.append(len(clock.readings))                # index of the reading this call takes
        else:
            clock.t += case["dt"]
        filt = O.initial_node_filter(nodes, grp)
        match = m.ScheduleOne(filt, top)
        assert len(m.last_placements) == 1
        ids = m.last_placements[0]
        bound = sched_standin.attempt_scheduling(nodes, m, top, grp, match=match)
        assert (bound is None) == (ids is None)
        if bound is not None:
            assert ids == ids_written_into(nodes[bound], top), k
        binds.append(bound)
    state["pod"] = len(tops)
    return dict(nodes=nodes, m=m, binds=binds, events=events, tops=tops, groups=groups, spec=spec, pods=pods, called_at=called_at)


def oracle_loop(case, now_of, busy_of):
    """The oracle's own loop (O.find_node, O.commit) on a second copy of the fixture's nodes: pod k is matched at now_of(k) and its
    node stamped busy_of(k).  Returns (nodes, binds, index of the first pod whose commit the reference would fail or None)."""
    spec = synth.make_cluster(case["config"], n_nodes=case["n_nodes"])
    pods, groups = synth.make_pods(case["config"], n_pods=case["n_pods"])
    for p in pods:
        p["misc_smt"] = True
    nodes = spec.build_nodes()
    binds = []
    for k, (p, grp) in enumerate(zip(pods, groups)):
        top = refmodel.make_topology(p)
        res = O.find_node(O.initial_node_filter(nodes, grp), top, now_of(k))
        if res[0] is not None:
            try:
                O.commit(nodes[res[0]], top, res[1], busy_of(k))
            except O.CommitFailure:
                return nodes, binds, k
        binds.append(res[0])
    return nodes, binds, None


@pytest.mark.parametrize("path", sched_check.FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_reference_scheduler_loops_through_schedule_one(path):
    case = sched_check.load(path)
    r = one_check(case, sched_check.Clock(case["clock0"]), engine_factory=harness.HarnessEngine)
    nodes, m, binds, events = r["nodes"], r["m"], r["binds"], r["events"]
    assert binds == case["binds"]
    assert sched_check.packed(nodes) == case["final"]
    assert sched_check.mirror_state(m) == case["final"]
    assert not [e for e in events if e[1] == "upload"]                   # nothing was re-packed and re-uploaded
    # the fixtures' virtual clock gives SetBusy the very time the call committed: the reason is dropped, nothing goes out
    assert not [e for e in events if e[1] == "apply_deltas"]
    bound = [k for k, b in enumerate(binds) if b is not None]
    assert [e[0] for e in events if e[1] == "commit"] == bound           # the engine's commit: once per bound pod, none behind the mutators
    assert len(bound) > 0


@pytest.mark.parametrize("path", sched_check.FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_busy_time_written_after_the_call_follows_as_one_correction(path):
    case = sched_check.load(path)
    clock = TickingClock(case["clock0"])
    r = one_check(case, clock, engine_factory=harness.HarnessEngine)
    nodes, m, binds, events, called_at = r["nodes"], r["m"], r["binds"], r["events"], r["called_at"]
    # pod k: ScheduleOne took reading called_at[k] (ONE reading for `now` and the committed busy time), SetBusy the one behind it
    assert all(called_at[k + 1] - called_at[k] == (2 if binds[k] is not None else 1) for k in range(len(binds) - 1))
    rd = clock.readings
    ref_nodes, ref_binds, failed = oracle_loop(case, lambda k: rd[called_at[k]], lambda k: rd[called_at[k] + 1])
    assert failed is None and binds == ref_binds
    m.FindNode(nodes, r["tops"][0])                                      # any other call flushes the correction that is still pending
    assert sched_check.packed(nodes) == sched_check.packed(ref_nodes)
    assert sched_check.mirror_state(m) == sched_check.packed(nodes)      # busy times included
    # the composed form carries the correction as a delta: nothing but SET_BUSY records, at most one per bound pod, in front of the
    # next call's find
    deltas = [e for e in events if e[1] == "apply_deltas" and e[0] < len(binds)]
    assert deltas and all(e[2] == [pack.DELTA_SET_BUSY] for e in deltas)
    assert len(deltas) <= sum(b is not None for b in binds)
    for k in range(len(binds)):
        mine = [e[1] for e in events if e[0] == k and e[1] != "upload"]
        assert mine in (["find"], ["find", "commit"], ["apply_deltas", "find"], ["apply_deltas", "find", "commit"]), (k, mine)
        if "apply_deltas" in mine:                                       # (the time SetBusy wrote behind the last pod that was bound)
            assert any(binds[j] is not None for j in range(k))
    assert not [e for e in events if e[1] == "upload"]


def test_a_sharded_mirror_commits_on_the_shard_that_owns_the_winner():
    """GroupEngine.find_commit (three host-twin shards): the group's find, the correction as a SET_BUSY delta to its owner, the
    commit on the owner's context - the replay under the advancing clock, against the oracle's loop."""
    case = dict(config=5, n_nodes=192, n_pods=120, clock0=small_case()["clock0"], dt=0.0)      # (three shards of 64 nodes)
    clock = TickingClock(case["clock0"])
    r = one_check(case, clock, engine_factory=harness.HarnessEngine, devices=[0, 1, 2])
    nodes, m, binds, events, called_at = r["nodes"], r["m"], r["binds"], r["events"], r["called_at"]
    rd = clock.readings
    ref_nodes, ref_binds, failed = oracle_loop(case, lambda k: rd[called_at[k]], lambda k: rd[called_at[k] + 1])
    assert failed is None and binds == ref_binds
    assert [e[0] for e in events if e[1] == "find_commit"] == list(range(len(binds)))
    assert [e[0] for e in events if e[1] == "commit"] == [k for k, b in enumerate(binds) if b is not None]
    assert all(e[2] == [pack.DELTA_SET_BUSY] for e in events if e[1] == "apply_deltas")
    assert len({m.engine._shard_of(m._index[b]) for b in binds if b is not None}) > 1      # (winners on more than one shard)
    m.FindNode(nodes, r["tops"][0])
    assert sched_check.packed(nodes) == sched_check.packed(ref_nodes) == sched_check.mirror_state(m)


def small_case():
    return sched_check.load(sched_check.FIXTURES[0])


def cluster_and_pods(case, clock):
    spec = synth.make_cluster(case["config"], n_nodes=case["n_nodes"])
    pods, groups = synth.make_pods(case["config"], n_pods=case["n_pods"])
    for p in pods:
        p["misc_smt"] = True
    nodes = sched_standin.adopt(spec.build_nodes(), clock)
    return nodes, [refmodel.make_topology(p) for p in pods], groups


def test_a_placement_nobody_applies_is_repacked_before_the_next_call():
    case = small_case()
    clock = sched_check.Clock(case["clock0"])
    nodes, tops, groups = cluster_and_pods(case, clock)
    m = HipMatcher(clock=clock, engine_factory=harness.HarnessEngine)
    m.attach(nodes)
    before = sched_check.packed(nodes)
    k = next(k for k in range(len(tops)) if m.FindNode(O.initial_node_filter(nodes, groups[k]), tops[k])[0] is not None)
    first = m.ScheduleOne(O.initial_node_filter(nodes, groups[k]), tops[k])
    assert first[0] is not None and m.last_placements[0] is not None
    assert sched_check.mirror_state(m) != before                          # the mirror holds the commit ...
    again = m.ScheduleOne(O.initial_node_filter(nodes, groups[k]), tops[k])
    assert again == first and sched_check.packed(nodes) == before         # ... the objects never did: the node was re-packed, the same answer
    m.FindNode(nodes, tops[k])
    assert sched_check.mirror_state(m) == before
    # and one that IS applied stays
    match = m.ScheduleOne(O.initial_node_filter(nodes, groups[k]), tops[k])
    assert sched_standin.attempt_scheduling(nodes, m, tops[k], groups[k], match=match) == first[0]
    m.FindNode(nodes, tops[k])
    assert sched_check.mirror_state(m) == sched_check.packed(nodes) != before


def test_schedule_one_between_find_node_and_schedule_batch_calls():
    case = small_case()
    clock = TickingClock(case["clock0"])
    nodes, tops, groups = cluster_and_pods(case, clock)
    m = HipMatcher(clock=clock, engine_factory=harness.HarnessEngine)
    m.attach(nodes)
    bound = 0
    k = 0
    while k + 4 <= min(len(tops), 64):
        for j, form in enumerate(("one", "find", "one")):
            top, grp = tops[k + j], groups[k + j]
            if form == "one":
                match = m.ScheduleOne(O.initial_node_filter(nodes, grp), top)
                bound += sched_standin.attempt_scheduling(nodes, m, top, grp, match=match) is not None
            else:
                bound += sched_standin.attempt_scheduling(nodes, m, top, grp) is not None
        now = clock()
        matches = m.ScheduleBatch(nodes, tops[k + 3:k + 4], pod_groups=groups[k + 3:k + 4], now=now, apply=True)
        bound += sched_standin.attempt_scheduling(nodes, m, tops[k + 3], groups[k + 3], match=matches[0]) is not None
        k += 4
    assert bound >= 16
    m.FindNode(nodes, tops[0])
    assert sched_check.mirror_state(m) == sched_check.packed(nodes)


def trimmed(descs):
    for d in descs:                                                     # (the oracle enumerates like the reference: few NICs keep it quick)
        keep, lab = 0, {}
        for k, v in d["labels"].items():
            if "nfd-extras-nic" in k:
                keep += 1
                if keep > 4:
                    continue
            lab[k] = v
        d["labels"] = lab
        d["nic_pods_used"] = d["nic_pods_used"][:sum(1 for k in lab if "nfd-extras-nic" in k and "10000Mbs" not in k.replace("100000Mbs", ""))]
    return descs


@pytest.mark.parametrize("seed", [0, 2])
def test_big_pods_and_wide_nodes_through_schedule_one(seed):
    """A cluster with wide nodes and pods of five and more processing groups among ordinary ones: ScheduleOne composes these from
    FindNodes + CommitPlacement - node, mapping and physical ids of every pod against the oracle's FindNode + commit loop.
    (Seeds for which the ORACLE's loop puts pods on wide nodes and places big pods - with seed 1 it uses no wide node at all.)"""
    descs = trimmed(util.mixed_cluster_desc(47000 + seed, 24, wide_share=0.35, occupancy=0.1))
    nl, ref_nl = util.build_cluster(descs), util.build_cluster(descs)
    rng = np.random.default_rng(100 + seed)
    specs = []
    for _ in range(22):
        s = big_spec(rng, 5, 6) if rng.random() < 0.5 else util.random_pod_spec(rng)
        s["misc_smt"] = True
        if s["map_type"] == "NONE":
            s["map_type"] = "NUMA"
        specs.append(s)
    tops = [refmodel.make_topology(s) for s in specs]
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=harness.HarnessEngine)
    m.attach(nl)
    assert m.wide_nodes
    placed_big = placed_wide = 0
    for top in tops:
        want = O.find_node(ref_nl, top, util.CLOCK)
        rec = {}
        if want[0] is not None:
            try:
                O.commit(ref_nl[want[0]], top, want[1], util.CLOCK, rec)
            except O.CommitFailure:
                break
        got = m.ScheduleOne(nl, top)
        assert norm(got) == norm(want)
        assert m.last_placements == [rec if want[0] is not None else None]
        if got[0] is not None:
            O.commit(nl[got[0]], top, got[1], util.CLOCK)              # the caller's side; the objects carry no mutator hooks of their own here,
            m.mark_dirty(got[0])                                         # so the node is re-packed from its object
            placed_big += len(top.proc_groups) > 4
            placed_wide += got[0] in m.wide_nodes
    assert placed_big >= 2 and placed_wide >= 1


def test_null_context_is_an_argument_error():
    from nhd_amd import _lib
    lib = _lib.load()
    z = ctypes.c_uint64(0)
    assert lib.nhdfit_find_commit(None, None, 0.0, None, 0.0, -1, 0.0, None, None, None, None) == -1
    assert lib.nhdfit_find_commit_counts(None, ctypes.byref(z), ctypes.byref(z)) == -1
