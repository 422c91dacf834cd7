"""FindNode and the commit step for one pod in ONE launch (nhdfit_find_commit, k_find1_commit) on the device: against the independent
sequential oracle at the shapes the mode-B test uses, the reference-generated scheduler loops, the Python oracle's loop on
heterogeneous clusters, nhdfit_find + nhdfit_commit on a second context, and the host twin around the other forms of find.
nhdfit_find_commit_counts says which form a call took: a test that passes through the composed form proves nothing about the new
kernel, so the counts are asserted wherever the one-launch form must have run.  Run with `pytest -m gpu`; once more with
NHDFIT_LIBRARY=nhd_amd/libnhdfit_tuning.so, whose stream ledger checks see the new writer."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import winner_index
from oracle import coracle
from oracle import nhd_oracle as O
from tests import sched_check, sched_standin, util
from tests.test_gpu_parity import as_jsonable, mirror_equals_seq_records
from tests.test_schedule_one import TickingClock, one_check, oracle_loop
from workload import planes, refmodel, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine_cls():
    from nhd_amd.engine import Engine
    return Engine


def context(engine_cls, pk, table):
    eng = engine_cls(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    return eng


def copy_of(table):
    return pack.NodeTable(list(table.names), *[np.array(getattr(table, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")], np.array(table.origin))


def find_then_commit(eng, req, now, busy_time, cand=None):
    """nhdfit_find with one pod + nhdfit_commit on its winner: what nhdfit_find_commit answers, call for call."""
    score, _, maps = eng.find(req.reshape(1), now, cand=cand, want_bitmap=False, want_map=True)
    s = int(score[0])
    if not s or not int(maps[0]["valid"]):
        return s, maps[0], np.zeros((), pack.PLACEMENT), False
    return s, maps[0], eng.commit(winner_index(s) - eng.global_base, req, maps[0], busy_time), True


def same_answer(a, b, tag):
    assert a[0] == b[0], tag
    assert a[1].tobytes() == b[1].tobytes(), tag
    assert a[2].tobytes() == b[2].tobytes(), tag
    assert a[3] == b[3], tag


def same_mirror(a, b):
    got, want = a.download(), b.download()
    for f in ("p0", "p1", "p2", "p3", "p4", "detail"):
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f


@pytest.mark.parametrize("cfg,n,P", [(2, 4096, 256), (3, 16384, 1024), (4, 65536, 4096), (5, 32768, 2048)],
                         ids=["c2-whole", "c3-whole", "c4-65536x4096", "c5-shard"])
def test_find_commit_pod_after_pod_vs_independent_oracle(engine_cls, cfg, n, P):
    """P calls of Engine.find_commit, pod after pod, busy_time = now: node, mapping and physical ids of every pod and the mirror
    afterwards against oracle/seq_oracle.py (which compiles none of the product's headers).  Every pod of these generators has at
    most three processing groups and the mode-B test asserts that no commit at these shapes would raise: configs 2-4 must take the
    one-launch form for every call."""
    from oracle import seq_oracle
    spec = synth.make_cluster(cfg, n_nodes=n)
    pods, groups = synth.make_pods(cfg, n_pods=P)
    tops = [refmodel.make_topology(s) for s in pods]
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many(tops, groups)
    pk.close_signatures()
    assert int(reqs["n_groups"].max()) <= 3
    eng = context(engine_cls, pk, table)
    now = spec.clock_now
    sc = seq_oracle.SeqCluster(coracle.Cluster.from_spec(spec))
    win, omaps, oids, n_def = seq_oracle.schedule_sequence(sc, tops, groups, now)
    assert n_def == len(tops), "the oracle met a commit the reference raises on at pod %d" % n_def
    for i in range(P):
        score, m, place, done = eng.find_commit(reqs[i], now, now)
        node = winner_index(score) if score else -1
        assert node == int(win[i]), (i, node, int(win[i]))
        assert done == (node >= 0), i
        if node < 0:
            continue
        assert int(place["status"]) != pack.COMMIT_WOULD_RAISE, i
        G = int(reqs[i]["n_groups"])
        got_map = {"gpu": [int(x) for x in m["gpu"][:G]], "cpu": [int(x) for x in m["cpu"][:G + 1]],
                   "nic": [[int(a), int(b)] for a, b in zip(m["nic_numa"][:G], m["nic_idx"][:G])]}
        om = omaps[i]
        assert got_map == {"gpu": list(om["gpu"]), "cpu": list(om["cpu"]), "nic": [list(x) for x in om["nic"]]}, (i, got_map, om)
        phys = int(spec.phys[node])
        ids = pack.expand_placement(place, G, phys // 2, phys, [int(reqs[i]["gpus"][g]) for g in range(G)])
        assert ids == oids[i], (i, ids, oids[i])
    want = np.asarray(win, np.int64)
    mirror_equals_seq_records(eng.download(), sc, sorted(set(int(x) for x in want if x >= 0)))
    placed, distinct = int((want >= 0).sum()), len(set(int(x) for x in want if x >= 0))
    assert placed > (P // 2 if P <= 4096 and cfg != 2 else P // 8) and distinct > placed // (8 if cfg != 2 else 64)
    fused, composed = eng.find_commit_counts()
    print(f"find_commit c{cfg} {n} nodes x {P} pods: fused {fused}, composed {composed}, placed {placed}")
    if cfg in (2, 3, 4):
        assert composed == 0 and fused == P
    else:
        assert fused + composed == P
    eng.close()


@pytest.mark.parametrize("path", sched_check.FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_reference_scheduler_loops_through_schedule_one_on_gpu(path):
    case = sched_check.load(path)
    r = one_check(case, sched_check.Clock(case["clock0"]))
    nodes, m, binds, events = r["nodes"], r["m"], r["binds"], r["events"]
    assert binds == case["binds"]
    assert sched_check.packed(nodes) == case["final"]
    assert sched_check.mirror_state(m) == case["final"]
    assert not [e for e in events if e[1] in ("upload", "apply_deltas", "commit", "find")]
    calls = [e[0] for e in events if e[1] == "find_commit"]
    assert calls == sorted(set(calls)) and set(k for k, b in enumerate(binds) if b is not None) <= set(calls)     # one device call per pod
    assert max(len(t.proc_groups) for t in r["tops"]) <= 3
    assert m.engine.find_commit_counts() == (len(calls), 0)               # (no commit of these loops fails: the reference ran them)
    m.engine.close()


@pytest.mark.parametrize("path", sched_check.FIXTURES, ids=lambda p: p.split("/")[-1][:-5])
def test_busy_time_written_after_the_call_rides_in_the_next_launch(path):
    """The replay under a clock that advances on every reading: SetBusy's time differs from the committed one and rides in the next
    ScheduleOne as `prev` - not one nhdfit_apply_deltas inside the loop - and objects and mirror agree, busy times included, with
    the oracle's own loop at the times the clock handed out."""
    case = sched_check.load(path)
    clock = TickingClock(case["clock0"])
    r = one_check(case, clock)
    nodes, m, binds, events, called_at = r["nodes"], r["m"], r["binds"], r["events"], r["called_at"]
    rd = clock.readings
    ref_nodes, ref_binds, failed = oracle_loop(case, lambda k: rd[called_at[k]], lambda k: rd[called_at[k] + 1])
    assert failed is None and binds == ref_binds
    assert not [e for e in events if e[0] < len(binds) and e[1] in ("upload", "apply_deltas", "commit", "find")]
    assert max(len(t.proc_groups) for t in r["tops"]) <= 3
    calls = [e[0] for e in events if e[1] == "find_commit"]
    assert calls == sorted(set(calls)) and set(k for k, b in enumerate(binds) if b is not None) <= set(calls)
    assert m.engine.find_commit_counts() == (len(calls), 0)              # (the oracle fails no commit: every call took the one launch)
    m.FindNode(nodes, r["tops"][0])                                      # any other call flushes the correction that is still pending
    assert sched_check.packed(nodes) == sched_check.packed(ref_nodes)
    assert sched_check.mirror_state(m) == sched_check.packed(nodes)
    m.engine.close()


def test_the_correction_turns_a_gpu_pod_away_and_reaches_the_mirror(engine_cls):
    """One node.  Its stored busy time is long past; `prev` says SetBusy stamped it five seconds ago: a pod with GPUs is turned away
    (nhd/Matcher.py IsBusy, 30 s) by the launch that carries the correction, and plane 4 holds the time afterwards."""
    spec = synth.make_cluster(4, n_nodes=256)
    pods, groups = synth.make_pods(4, n_pods=256)
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    tops = [refmodel.make_topology(s) for s in pods]
    reqs = pk.digest_many(tops)
    pk.close_signatures()
    now = spec.clock_now
    v = int(np.flatnonzero((table.p2["flags"] & pack.NF_HAS_GPU) != 0)[0])
    one = copy_of(table).slice(v, v + 1)
    one.p4["busy_time"][0] = now - 500.0
    eng = context(engine_cls, pk, one)
    gpu_pods = [i for i in range(len(reqs)) if int(reqs[i]["gpus"].sum()) > 0 and int(reqs[i]["n_groups"]) <= 3]
    i = next(i for i in gpu_pods if int(eng.find(reqs[i:i + 1], now, want_bitmap=False)[0][0]))     # a GPU pod this node takes as it stands
    score, _, _, done = eng.find_commit(reqs[i], now, now, prev=(0, now - 5.0))
    assert score == 0 and not done
    assert float(eng.download().p4["busy_time"][0]) == now - 5.0
    assert eng.find_commit_counts() == (1, 0)
    # the stored time alone would not have: a second context without the correction places the pod
    eng2 = context(engine_cls, pk, one)
    score, _, _, done = eng2.find_commit(reqs[i], now, now)
    assert score != 0 and done and float(eng2.download().p4["busy_time"][0]) == now
    # and the correction is in the mirror when the winner is that very node: a later time that lets the pod in again
    score, _, _, done = eng.find_commit(reqs[i], now + 100.0, now + 100.0, prev=(0, now - 400.0))
    assert score != 0 and done and float(eng.download().p4["busy_time"][0]) == now + 100.0
    from nhd_amd import _lib
    with pytest.raises(_lib.NhdFitError):
        eng.find_commit(reqs[i], now, now, prev=(1, now))                 # prev_node >= n
    eng.close()
    eng2.close()


def test_candidate_mask_and_initial_filter_equal_find_plus_commit(engine_cls):
    spec = synth.make_cluster(4, n_nodes=4096)
    pods, groups = synth.make_pods(4, n_pods=300)
    tops = [refmodel.make_topology(s) for s in pods]
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many(tops, groups)
    assert (reqs["flags"] & pack.RF_INITIAL_FILTER).all()
    pk.close_signatures()
    a, b = context(engine_cls, pk, table), context(engine_cls, pk, copy_of(table))
    now = spec.clock_now
    rng = np.random.default_rng(11)
    masks = [None, rng.integers(0, 2 ** 63, size=(4096 + 63) // 64, dtype=np.uint64), rng.integers(0, 2 ** 63, size=(4096 + 63) // 64, dtype=np.uint64) &
             rng.integers(0, 2 ** 63, size=(4096 + 63) // 64, dtype=np.uint64)]
    placed = one_launch = 0
    for i in range(len(reqs)):
        cand = masks[(i // 20) % 3]
        got = a.find_commit(reqs[i], now, now + 1e-3 * i, cand=cand)
        same_answer(got, find_then_commit(b, reqs[i], now, now + 1e-3 * i, cand=cand), i)
        if got[0] and cand is not None:
            v = winner_index(got[0])
            assert int(cand[v >> 6]) >> (v & 63) & 1, i
        placed += got[3]
        # (three groups at most, no wide node: one launch, unless the commit is one the reference raises on)
        one_launch += int(reqs[i]["n_groups"]) <= 3 and not (got[3] and int(got[2]["status"]) == pack.COMMIT_WOULD_RAISE)
    assert placed > 100
    same_mirror(a, b)
    assert a.find_commit_counts() == (one_launch, len(reqs) - one_launch) and one_launch > len(reqs) // 2
    assert b.find_commit_counts() == (0, 0)
    a.close()
    b.close()


def hetero_inputs(seed):
    rng = np.random.default_rng(seed)
    specs = []
    for _ in range(160):
        s = util.random_pod_spec(rng)
        s["misc_smt"] = True
        if s["map_type"] == "NONE":
            s["map_type"] = "NUMA"
        specs.append(s)
    return specs


@pytest.mark.parametrize("seed", range(6))
def test_heterogeneous_clusters_pod_after_pod_through_schedule_one(seed):
    """The six random clusters of test_mode_b_heterogeneous_clusters_on_gpu, pod after pod through HipMatcher.ScheduleOne in attached
    mode (the placements applied with the stand-in's mutators), against the Python oracle's loop on a second copy of the nodes up to
    the first commit the oracle fails.  Seeds 0-3 and 5 meet none; no pod has more than three groups: nothing is composed."""
    clock = sched_check.Clock(util.CLOCK)
    nl = sched_standin.adopt(util.random_cluster(71000 + seed, 60, occupancy=0.15), clock)
    ref_nl = util.random_cluster(71000 + seed, 60, occupancy=0.15)
    specs = hetero_inputs(seed)
    tops, ref_tops = [refmodel.make_topology(s) for s in specs], [refmodel.make_topology(s) for s in specs]
    assert max(len(t.proc_groups) for t in tops) <= 3
    from nhd_amd.matcher import HipMatcher
    m = HipMatcher(clock=clock)
    m.attach(nl)
    k = placed = 0
    for top, ref_top in zip(tops, ref_tops):
        want = O.find_node(ref_nl, ref_top, util.CLOCK)
        rec = {}
        if want[0] is not None:
            try:
                O.commit(ref_nl[want[0]], ref_top, want[1], util.CLOCK, rec)
            except O.CommitFailure:
                break
        got = m.ScheduleOne(nl, top)
        assert as_jsonable(got) == as_jsonable(want), k
        assert m.last_placements == [rec if want[0] is not None else None], k
        assert sched_standin.attempt_scheduling(nl, m, top, None, match=got) == want[0]
        placed += want[0] is not None
        k += 1
    assert k >= 10 and placed >= 5                                        # (seed 4 stops at pod 11: a commit the reference would fail)
    fused, composed = m.engine.find_commit_counts()
    print(f"seed {seed}: {k} pods, {placed} placed, fused {fused}, composed {composed}")
    assert fused + composed == k
    if seed != 4:
        assert k == len(tops) and composed == 0
    m.FindNode(nl, tops[0])
    assert sched_check.mirror_state(m) == sched_check.packed(nl)
    m.engine.close()


def test_a_commit_the_reference_raises_on_goes_composed(engine_cls):
    """Seed 4 of the clusters above at the engine level: pods 0..11, the oracle fails the commit of pod 11.  The launch reports "found,
    not committed" and the call finishes with k_commit: placement record (NHDFIT_COMMIT_WOULD_RAISE) and the whole mirror afterwards
    equal, byte for byte, what nhdfit_find + nhdfit_commit leave on a second context."""
    seed = 4
    nl = util.random_cluster(71000 + seed, 60, occupancy=0.15)
    ref_nl = util.random_cluster(71000 + seed, 60, occupancy=0.15)
    specs = hetero_inputs(seed)
    first_failure = None
    for k, s in enumerate(specs):
        top = refmodel.make_topology(s)
        want = O.find_node(ref_nl, top, util.CLOCK)
        if want[0] is not None:
            try:
                O.commit(ref_nl[want[0]], top, want[1], util.CLOCK)
            except O.CommitFailure:
                first_failure = k
                break
    assert first_failure == 11
    pk = pack.Packer()
    table = pk.pack_nodes(nl)
    reqs = pk.digest_many([refmodel.make_topology(s) for s in specs[:12]])
    pk.close_signatures()
    a, b = context(engine_cls, pk, table), context(engine_cls, pk, copy_of(table))
    for i in range(12):
        got = a.find_commit(reqs[i], util.CLOCK, util.CLOCK)
        same_answer(got, find_then_commit(b, reqs[i], util.CLOCK, util.CLOCK), i)
        assert a.find_commit_counts() == ((i + 1, 0) if i < 11 else (11, 1)), i
    assert got[3] and int(got[2]["status"]) == pack.COMMIT_WOULD_RAISE
    same_mirror(a, b)
    a.close()
    b.close()


def test_find_commit_behind_every_other_form_of_find(engine_cls):
    """One context: pipelined steps left in flight, a whole-batch find, a mode-B batch with its commits kept - a find_commit behind
    each (the writer's rule: it waits for every stream that may hold work), against the host twin driven through the same sequence."""
    from tests import harness
    spec = synth.make_cluster(4, n_nodes=4096)
    pods, groups = synth.make_pods(4, n_pods=400)
    for p in pods:
        p["misc_smt"] = True
    tops = [refmodel.make_topology(s) for s in pods]
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many(tops, groups)
    reqs = reqs[np.flatnonzero(reqs["n_groups"] <= 3)]
    pk.close_signatures()
    eng = context(engine_cls, pk, table)
    twin = harness.HarnessEngine(0)
    twin.set_dictionary(pk)
    twin.upload(copy_of(table))
    now = spec.clock_now
    calls = 0

    def one(i, tag):
        nonlocal calls
        bt = now + 1.0 + calls
        got = eng.find_commit(reqs[i], now, bt)
        same_answer(got, find_then_commit(twin, reqs[i], now, bt), tag)
        calls += 1
        return got[3]

    committed = 0
    for rnd in range(3):
        k = 40 * rnd
        batch = slice(0, 200 + rnd)
        eng.stage(reqs[batch])                                              # pipelined steps left in flight on both pipes
        eng.enqueue(now); eng.enqueue(now); eng.enqueue(now)
        committed += one(k, "with steps in flight")
        score, _, maps = eng.find(reqs[batch], now, want_bitmap=False, want_map=True)      # k_findn
        hs, _, hm = twin.find(reqs[batch], now, want_bitmap=False, want_map=True)
        assert np.array_equal(score, hs) and np.array_equal(maps[score != 0], hm[score != 0]), "whole batch behind a find_commit"
        committed += one(k + 1, "behind a whole-batch find")
        sub = slice(100 + 20 * rnd, 160 + 20 * rnd)                         # mode B, commits kept
        node, maps_b, places, status = eng.schedule_batch(reqs[sub], now, pk, apply=True)
        hn, hm_b, hp, hst = twin.schedule_batch(reqs[sub], now, pk, apply=True)
        assert np.array_equal(node, hn) and np.array_equal(status, hst) and places.tobytes() == hp.tobytes()
        committed += one(k + 2, "behind mode B")
        committed += one(k + 3, "behind a find_commit")
        score, _, maps = eng.find(reqs[k:k + 30], now, want_bitmap=False, want_map=True)   # k_find
        hs, _, hm = twin.find(reqs[k:k + 30], now, want_bitmap=False, want_map=True)
        assert np.array_equal(score, hs) and np.array_equal(maps[score != 0], hm[score != 0]), "one tile behind a find_commit"
    assert committed >= 8
    got, want = eng.download(), twin.download()
    for f in ("p0", "p1", "p2", "p3", "p4", "detail"):
        assert getattr(got, f).tobytes() == getattr(want, f).tobytes(), f
    assert eng.find_commit_counts() == (calls, 0)
    eng.close()
