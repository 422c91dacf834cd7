"""Node.IsBusy at its binary64 boundary on the MI355X (`pytest -m gpu`): the cluster of tests/test_busy_boundary.py - 130 nodes
stamped with the 130 consecutive doubles around the smallest stamp the reference calls busy - through every consumer of the
launch's `busy_from` (the step kernel staged and pipelined, the single-launch finds of one pod, one tile and a whole batch, the
find of find_commit, explain, the wide-node and the big-pod kernel, shards) and through the two kernels that subtract (mode B's
decision and commit kernels).  The expectation is Python's own float arithmetic (tests/busy_check.py) and the Python oracle."""
import copy

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import Engine, GroupEngine, winner_index
from nhd_amd.matcher import HipMatcher
from oracle import nhd_oracle as O
from tests import busy_check as bc
from tests import test_busy_boundary as bb
from tests.test_busy_boundary import BIG_POD, BUSY, FITS, GPU_PODS, N_NODES, PLAIN_POD, bits_of, jsonable

pytestmark = pytest.mark.gpu

SMALL = [p for p in range(5) if p != BIG_POD]           # the pods of the table-driven pass, in the order of their request records


def engine_case(now):
    nl, busy = bb.stamped_cluster(now)
    tops = bb.pods()
    pk = pack.Packer()
    table = pk.pack_nodes(nl)
    reqs = pk.digest_many([tops[p] for p in SMALL])
    big = np.array([pk.digest_big(tops[BIG_POD])], dtype=pack.BIG_REQ)
    pk.close_signatures()
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    assert eng.n_wide == 0
    return nl, busy, tops, pk, table, reqs, big, eng


def verdicts(bitmap, P=len(SMALL)):
    return np.stack([bits_of(bitmap, k) for k in range(P)])


def expected_verdicts(busy):
    return np.stack([np.ones(N_NODES, bool) if p == PLAIN_POD else ~busy for p in SMALL])


def winners(score):
    return [winner_index(s) if s else -1 for s in score.tolist()]


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_every_form_of_find_and_explain(now):
    nl, busy, tops, pk, table, reqs, big, eng = engine_case(now)
    names = list(nl)
    want_v = expected_verdicts(busy)
    want = [O.find_node(nl, tops[p], now) for p in SMALL]
    want_w = [names.index(w[0]) for w in want]
    assert all(not busy[w] for w, p in zip(want_w, SMALL) if p in GPU_PODS)
    # the step kernel: staged, with the verdict matrix
    score, bm, maps = eng.find(reqs, now, want_bitmap=True, want_map=True)
    got_v = verdicts(bm)
    assert np.array_equal(got_v, want_v), np.argwhere(got_v != want_v).tolist()
    assert winners(score) == want_w and maps["valid"].all()
    for k, (gpu, cpu, nic_numa, nic_idx, _) in enumerate(pack.unpack_mappings(maps)):
        G = int(reqs[k]["n_groups"])
        assert jsonable((want[k][0], {"gpu": gpu[:G], "cpu": cpu[:G + 1], "nic": list(zip(nic_numa[:G], nic_idx[:G]))})) == jsonable(want[k]), k
    # pipelined: steps on both pipes, then the fetch
    eng.stage(reqs)
    eng.enqueue(now); eng.enqueue(now); eng.enqueue(now)
    s2, b2, m2 = eng.fetch(want_bitmap=True, want_map=True)
    assert np.array_equal(s2, score) and np.array_equal(b2, bm) and np.array_equal(m2, maps)
    # one launch for a whole batch (more than one pod tile; pods of up to three groups), for one tile and for one pod
    before = eng.stats()
    small_finds, batch_finds = int(before.small_finds), int(before.batch_finds)
    upto3 = [k for k in range(len(SMALL)) if int(reqs[k]["n_groups"]) <= 3]
    assert len(upto3) == 3
    sn, _, mn = eng.find(np.concatenate([reqs[upto3]] * 23), now, want_bitmap=False, want_map=True)
    assert int(eng.stats().batch_finds) == batch_finds + 1
    assert np.array_equal(sn, np.concatenate([score[upto3]] * 23)) and np.array_equal(mn, np.concatenate([maps[upto3]] * 23))
    st, _, mt = eng.find(reqs[upto3], now, want_bitmap=False, want_map=True)
    assert np.array_equal(st, score[upto3]) and np.array_equal(mt, maps[upto3])
    for k in upto3:
        s1, _, m1 = eng.find(reqs[k:k + 1], now, want_bitmap=False, want_map=True)
        assert int(s1[0]) == int(score[k]) and np.array_equal(m1, maps[k:k + 1]), k
    assert int(eng.stats().small_finds) == small_finds + 1 + len(upto3)
    s4, _, m4 = eng.find(reqs, now, want_bitmap=False, want_map=True)               # with the four-group pod: no verdict matrix asked for
    assert np.array_equal(s4, score) and np.array_equal(m4, maps)
    # the big-pod kernel
    sb, mb = eng.big_find(big, now)
    wb = O.find_node(nl, tops[BIG_POD], now)
    assert winners(sb) == [names.index(wb[0])] and not busy[names.index(wb[0])] and int(mb[0]["valid"])
    # explain: ordinary and big requests
    for rq, pods_of in ((reqs, SMALL), (big, [BIG_POD])):
        counts, stages = eng.explain(rq, now, per_node=True)
        for k, p in enumerate(pods_of):
            if p == PLAIN_POD:
                assert (stages[k] == FITS).all()
            else:
                assert np.array_equal(stages[k] == BUSY, busy), (p, np.flatnonzero((stages[k] == BUSY) != busy).tolist())
                assert (stages[k][~busy] == FITS).all() and int(counts[k][BUSY]) == int(busy.sum())
    # three shards on one device: the matrix put together from the shards' is one context's
    grp = GroupEngine([0, 0, 0], engine_factory=Engine)
    grp.set_dictionary(pk)
    grp.upload(table)
    assert [hi - lo for lo, hi in grp._bounds] == [64, 64, 2]
    sg, _, mg = grp.find(reqs, now, want_map=True)
    assert np.array_equal(sg, score) and np.array_equal(mg, maps)
    parts = [s.find(reqs, now, want_bitmap=True, want_map=False)[1] for s in grp.shards]
    assert np.array_equal(np.concatenate(parts, axis=0), bm)
    cg, stg = grp.explain(reqs, now, per_node=True)
    c1, st1 = eng.explain(reqs, now, per_node=True)
    assert np.array_equal(cg, c1) and np.array_equal(stg, st1)
    grp.close()
    eng.close()


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_find_commit_pod_after_pod(now):
    """Engine.find_commit for the pods of the table-driven pass, then HipMatcher.ScheduleOne for all five with the scheduler's
    mutators behind each call: every answer is the oracle's find_node on the state its own commits left, so a node that has just
    been committed to (stamped `now`) is busy for the next pod with GPUs."""
    nl, busy, tops, pk, table, reqs, big, eng = engine_case(now)
    names = list(nl)
    onl = copy.deepcopy(nl)
    taken, touched = [], set()
    for k, p in enumerate(SMALL):
        want = O.find_node(onl, tops[p], now)
        O.commit(onl[want[0]], tops[p], want[1], now)
        score, mp, place, done = eng.find_commit(reqs[k], now, now)
        G = int(reqs[k]["n_groups"])
        assert score and done, p
        got = (names[winner_index(score)], {"gpu": mp["gpu"][:G], "cpu": mp["cpu"][:G + 1], "nic": list(zip(mp["nic_numa"][:G], mp["nic_idx"][:G]))})
        assert done and jsonable(got) == jsonable(want), p
        touched.add(names.index(want[0]))
        if p in GPU_PODS:
            assert not busy[names.index(want[0])] and want[0] not in taken, p
            taken.append(want[0])
    assert eng.find_commit_counts() == (3, 1)                         # (the four-group pod: nhdfit_find + nhdfit_commit)
    after = eng.download().p4["busy_time"]
    touched = sorted(touched)
    assert (after[touched] == now).all()
    rest = np.setdiff1d(np.arange(N_NODES), touched)
    assert np.array_equal(after[rest], table.p4["busy_time"][rest])
    eng.close()
    m = bb.schedule_one_check(now, lambda clock: HipMatcher(clock=clock))
    assert m.engine.find_commit_counts() == (3, 1)                    # (four groups: composed on the device side; five: FindNodes + CommitPlacement)
    m.engine.close()


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_matcher_calls(now):
    """HipMatcher on the device: FindNode pod by pod (the lone-pod launch), ExplainNodes, ScheduleBatch (mode B: the decision
    kernel and the commit kernel subtract) against the oracle's loop, and Headroom, which promises IsBusy() false."""
    nl, busy = bb.stamped_cluster(now)
    tops = bb.pods()
    names = list(nl)
    m = HipMatcher(clock=lambda: now)
    for p, top in enumerate(tops):
        want = O.find_node(nl, top, now)
        assert jsonable(m.FindNode(nl, top)) == jsonable(want), p
        if p in GPU_PODS:
            assert not busy[names.index(want[0])], p
    for p, e in enumerate(m.ExplainNodes(nl, tops, now=now, per_node=True)):
        assert e.error is None
        if p == PLAIN_POD:
            assert (e.stages == FITS).all()
        else:
            assert np.array_equal(e.stages == BUSY, busy) and (e.stages[~busy] == FITS).all() and e.counts["BUSY"] == int(busy.sum()), p
    bb.check_mode_b(m, nl, busy, now)
    # headroom: the stamps do not count
    idle, _ = bb.stamped_cluster(now)
    for nd in idle.values():
        nd.busy_time = 0.0
    for limits in (False, True):
        for p in SMALL:
            a = m.Headroom(nl, tops[p], per_node=True, limits=limits)
            b = m.Headroom(idle, tops[p], per_node=True, limits=limits)
            assert a.error is None and np.array_equal(a.per_node, b.per_node) and np.array_equal(a.flags, b.flags)
            assert (a.per_node > 0).all() and not a.flags.any() and a.replicas == b.replicas == int(a.per_node.sum())
            if limits:
                assert a.limits == b.limits and np.array_equal(a.limit_stages, b.limit_stages) and a.limits["BUSY"] == 0
    m.engine.close()


@pytest.mark.parametrize("now", bc.CLOCKS, ids=bc.CLOCK_IDS)
def test_wide_nodes_and_the_big_pod_on_a_mixed_cluster(now):
    """util.mixed_cluster with the same stamps written over it: the wide nodes (wide_kernel.h) and the five-group pod
    (big_kernel.h) held to the oracle node by node."""
    m = bb.mixed_cluster_check(now, lambda clock: HipMatcher(clock=clock))
    assert m.engine.wide_count() == len(m.wide_nodes)
    m.engine.close()
