"""nhd/Node.py:20 ENABLE_SHARING = True across shards, on the host build: every node is a wide record that carries its NICs'
speed_used (nhdfit_wide_share), and the mode-B entries that commit and then put the shards back (GroupEngine.schedule_batch and
sharding.schedule_batch_sharded with apply=False) must restore those records with the planes - against the Python oracle with its
switch flipped, bit for bit on the mirror.  Also: the digest cache of FindNode -> CommitPlacement under sharing."""
import copy
import os

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

from nhd_amd import pack
from nhd_amd import sharding as shard
from nhd_amd._lib import NhdFitError
from nhd_amd.matcher import HipMatcher
from oracle import nhd_oracle as O
from tests import harness, util
from tests.harness.explain_twin import ExplainHarnessEngine
from tests.test_shard_gloo import _free_port
from tests.wide_check import as_jsonable
from workload import dist as dist_util
from workload import refmodel

FIELDS = ("p0", "p1", "p2", "p3", "p4", "detail")


@pytest.fixture
def sharing(monkeypatch):
    monkeypatch.setattr(refmodel, "ENABLE_SHARING", True)
    monkeypatch.setattr(O, "ENABLE_SHARING", True)


def _traffic(rng, max_groups):
    s = util.random_pod_spec(rng, max_groups=max_groups)
    for g in s["groups"]:
        g["rx"] = float(rng.choice([0, 5, 10, 22.5, 25, 40, 0.1, 33.3]))
        g["tx"] = float(rng.choice([0, 5, 12.25, 25, 45, 0.7]))
        if rng.random() < 0.75:
            g["gpus"] = []
    s["misc_smt"] = True
    if s["map_type"] == "NONE":
        s["map_type"] = "NUMA"
    if s["map_type"] == "PCI":                      # (a PCI pod's GPUs must sit on its NIC's switch, or the reference's commit step
        for g in s["groups"]:                       #  raises half-way through - long batches would meet that sooner or later)
            g["gpus"] = []
    return s


def sharing_problem(seed, n, P, n_big=0):
    """(node descriptions, pod specs) of a sharing cluster: speed_used as test_sharing's fixture chooses them - some NICs close to
    their capacity, now and then one beyond it (its whole node is out).  Pods of 1..4 processing groups, `n_big` of them replaced
    by pods of 5..7 groups (the general path's requests) spread over the batch."""
    rng = np.random.default_rng(seed)
    descs = util.random_cluster_desc(seed, n, occupancy=0.1)
    for d in descs:
        d["nic_speed_used"] = [[float(rng.choice([0, 0, 10, 20, 22.5, 47.5], p=[0.3, 0.2, 0.2, 0.15, 0.1, 0.05])),
                                float(rng.choice([0, 0, 5, 15, 89.5], p=[0.3, 0.3, 0.2, 0.15, 0.05]))] for _ in d["nic_pods_used"]]
    specs = [_traffic(rng, pack.MAX_GROUPS) for _ in range(P)]
    for k in range(n_big):
        s = _traffic(rng, 7)
        while len(s["groups"]) <= pack.MAX_GROUPS:
            s = _traffic(rng, 7)
        specs[(k * P) // n_big + P // (2 * n_big)] = s
    return descs, specs


def speeds_matter(nl, tops, now):
    """Part of the fixture: the oracle with every speed_used zeroed answers at least one pod differently.  Otherwise a mirror that has
    silently stopped sharing (NICs priced at their full capacity) would pass every comparison with the oracle."""
    bare = copy.deepcopy(nl)
    for node in bare.values():
        for nic in node.nics:
            nic.speed_used = [0.0, 0.0]
    return any(as_jsonable(O.find_node(nl, t, now)) != as_jsonable(O.find_node(bare, t, now)) for t in tops)


def assert_tables_equal(a: pack.NodeTable, b: pack.NodeTable):
    """Two downloads of a mirror: planes, wide records and speed_used records, bit for bit."""
    assert a.n == b.n
    for f in FIELDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    assert sorted(a.wide or {}) == sorted(b.wide or {})
    for i, rec in (a.wide or {}).items():
        assert rec.tobytes() == b.wide[i].tobytes(), ("wide", i)
    assert sorted(a.share or {}) == sorted(b.share or {})
    for i, rec in (a.share or {}).items():
        assert rec.tobytes() == b.share[i].tobytes(), ("share", i)


def share_of(node) -> np.ndarray:
    """Node.nics[].speed_used of an oracle node in the order of a nhdfit_wide_share record (Packer.pack_share)."""
    used = np.zeros(pack.WIDE_SHARE["used"].shape)
    cnt = [0] * pack.WIDE_MAX_NUMA
    for nic in node.nics:
        u = nic.numa_node
        if 0 <= u < node.numa_nodes:
            used[u][cnt[u]] = [float(x) for x in nic.speed_used]
            cnt[u] += 1
    return used


def assert_speed_used_equals(share: dict, onl):
    """Every NIC's speed_used of the mirror (a download's share records) == the oracle's node objects, f64 for f64."""
    assert sorted(share) == list(range(len(onl)))
    for i, node in enumerate(onl.values()):
        assert share[i]["used"].tobytes() == share_of(node).tobytes(), node.name


# ---- (a), (b): GroupEngine.schedule_batch(apply=False) over host-twin shards -------------------------------------------------
@pytest.mark.parametrize("ndev", [2, 3])
@pytest.mark.parametrize("seed,n,P,n_big", [(9900, 200, 120, 0), (9901, 160, 100, 4), (9902, 250, 140, 0)])
def test_sharded_batch_without_apply_under_sharing_against_the_oracle(sharing, seed, n, P, n_big, ndev):
    """GroupEngine.schedule_batch(apply=False) over host-twin shards under ENABLE_SHARING: the oracle's loop over the whole cluster,
    the mirror bit for bit as before (speed_used included), FindNodes / ExplainNodes as before, then apply=True and every NIC's
    speed_used as the oracle's objects.  With pods of 5..7 groups the batch is cut at them (HipMatcher._run_with_big)."""
    descs, specs = sharing_problem(seed, n, P, n_big)
    tops = [refmodel.make_topology(s) for s in specs]
    nl = util.build_cluster(descs)
    assert speeds_matter(nl, tops, util.CLOCK)
    ids = []
    onl = copy.deepcopy(nl)
    want = O.schedule_sequence(onl, tops, [None] * P, util.CLOCK, ids_out=ids)
    big = [pack.needs_general_path(t) for t in tops]
    assert sum(big) == n_big
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=ExplainHarnessEngine, devices=list(range(ndev)))
    m.attach(nl)
    assert m.packer.sharing and len(m.wide_nodes) == n
    before = m.engine.download()
    assert before.share is not None and len(before.share) == n
    found = m.FindNodes(nl, tops, now=util.CLOCK)
    assert [as_jsonable(r) for r in found] == [as_jsonable(O.find_node(nl, t, util.CLOCK)) for t in tops]
    explained = [e.counts for e in m.ExplainNodes(nl, tops, now=util.CLOCK)]

    got = m.ScheduleBatch(nl, tops, now=util.CLOCK)                                # apply=False: the shards are put back
    if not any(big):                                                                # (pods of 5..7 groups: the touched nodes are re-packed
        assert_tables_equal(m.engine.download(), before)                            #  from their objects before the next call)
    assert [as_jsonable(r) for r in got] == [as_jsonable(w) for w in want]
    assert m.last_placements == ids
    placed = [w for w in want if w[0] is not None]
    names = list(nl)
    assert len(placed) >= 20
    assert any(names.index(w[0]) >= m.engine._bounds[0][1] for w in placed), "the case must place pods past the first shard"
    assert [as_jsonable(r) for r in m.FindNodes(nl, tops, now=util.CLOCK)] == [as_jsonable(r) for r in found]
    assert [e.counts for e in m.ExplainNodes(nl, tops, now=util.CLOCK)] == explained
    assert_tables_equal(m.engine.download(), before)

    again = m.ScheduleBatch(nl, tops, now=util.CLOCK, apply=True)
    assert [as_jsonable(r) for r in again] == [as_jsonable(w) for w in want]
    assert m.last_placements == ids
    assert_speed_used_equals(m.engine.download().share, onl)


# ---- (d): download / upload round trips ----------------------------------------------------------------------------------
@pytest.mark.parametrize("ndev", [1, 3])
def test_download_upload_round_trip_keeps_speed_used(sharing, ndev):
    """upload(download(a, b)) at the whole table, a slice inside one shard and a slice across two leaves the mirror as it was -
    speed_used included, with the commits of an applied batch in it (values the node objects do not hold)."""
    n = 200
    descs, specs = sharing_problem(9910, n, 60)
    nl = util.build_cluster(descs)
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=harness.HarnessEngine, devices=None if ndev == 1 else list(range(ndev)))
    m.attach(nl)
    packed = m.engine.download()
    assert sum(r[0] is not None for r in m.ScheduleBatch(nl, [refmodel.make_topology(s) for s in specs], now=util.CLOCK, apply=True)) >= 20
    before = m.engine.download()
    assert any(before.share[i].tobytes() != packed.share[i].tobytes() for i in range(n)), "the batch must have changed speed_used"
    cut = shard.shard_bounds(n, max(ndev, 2), 1)[0]
    for a, b in ((0, n), (10, 50), (cut - 20, cut + 30)):
        t = m.engine.download(a, b - a)
        assert t.share is not None and sorted(t.share) == list(range(b - a)), (a, b)
        m.engine.upload(t, first=a, capacity=n)
        assert_tables_equal(m.engine.download(), before)
        for k, s in enumerate(getattr(m.engine, "shards", [m.engine])):             # and each shard on its own
            lo, hi = m.engine._bounds[k] if ndev > 1 else (0, n)
            if hi > lo:
                assert_tables_equal(s.download(), before.slice(lo, hi))


@pytest.mark.parametrize("ndev", [1, 3])
def test_a_partial_slice_without_speed_used_changes_nothing(sharing, ndev):
    """Under ENABLE_SHARING a slice without speed_used records - a partial one, one across two shards, the whole table - is refused
    before the mirror is touched; only an emptied mirror (reset_nodes) takes a table without them."""
    n = 200
    descs, specs = sharing_problem(9911, n, 30)
    nl = util.build_cluster(descs)
    tops = [refmodel.make_topology(s) for s in specs]
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=harness.HarnessEngine, devices=None if ndev == 1 else list(range(ndev)), strict=True)
    m.attach(nl)
    before = m.engine.download()
    cut = shard.shard_bounds(n, max(ndev, 2), 1)[0]
    for a, b in ((20, 30), (cut - 10, cut + 10), (0, n)):
        bare = m.engine.download(a, b - a)
        bare.share = None
        with pytest.raises(NhdFitError):
            m.engine.upload(bare, first=a, capacity=n)
        assert_tables_equal(m.engine.download(), before)
    assert [as_jsonable(r) for r in m.FindNodes(nl, tops, now=util.CLOCK)] == [as_jsonable(O.find_node(nl, t, util.CLOCK)) for t in tops]
    m.engine.reset_nodes()
    m.engine.upload(bare)
    assert not m.engine.download().share


@pytest.mark.parametrize("ndev", [1, 3])
def test_a_repack_without_sharing_switches_the_mirror_off_and_back(monkeypatch, ndev):
    """HipMatcher re-packing a cluster whose module no longer shares NICs empties the engine first (reset_nodes ends sharing): the
    mirror then answers as the oracle without sharing, and once the constant is back, as the oracle with it."""
    descs, specs = sharing_problem(9912, 200, 40)
    tops = [refmodel.make_topology(s) for s in specs]
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=harness.HarnessEngine, devices=None if ndev == 1 else list(range(ndev)), strict=True)
    want = {}
    for on in (True, False):
        monkeypatch.setattr(O, "ENABLE_SHARING", on)
        nl = util.build_cluster(descs)
        want[on] = [as_jsonable(O.find_node(nl, t, util.CLOCK)) for t in tops]
    assert want[True] != want[False], "the case must tell the two modes apart"
    for on in (True, False, True):
        monkeypatch.setattr(refmodel, "ENABLE_SHARING", on)
        monkeypatch.setattr(O, "ENABLE_SHARING", on)
        nl = util.build_cluster(descs)
        m.attach(nl)
        assert bool(m.packer.sharing) == on and bool(m.engine.download().share) == on
        assert [as_jsonable(r) for r in m.FindNodes(nl, tops, now=util.CLOCK)] == want[on]


# ---- (c): one process per shard (gloo), apply=False then apply=True ----------------------------------------------------------
def _sharing_case(seed, n, P):
    descs, specs = sharing_problem(seed, n, P)
    return util.build_cluster(descs), [refmodel.make_topology(s) for s in specs]


def _worker_mode_b_sharing(rank, world, port, seed, n, P, out_dir):
    # a fresh process: the parent's monkeypatch does not reach it
    refmodel.ENABLE_SHARING = True
    O.ENABLE_SHARING = True
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    nl, tops = _sharing_case(seed, n, P)
    names = list(nl)
    lo, hi = shard.shard_bounds(n, world, rank)
    pk = pack.Packer()
    whole = pk.pack_nodes(nl)                             # (one dictionary for every rank: the whole cluster is packed, the shard uploaded)
    assert pk.sharing
    reqs = pk.digest_many(tops)
    pk.close_signatures()
    eng = harness.HarnessEngine(0)
    eng.set_dictionary(pk)
    eng.upload(whole.slice(lo, hi), global_base=lo)
    bits = np.zeros(((hi - lo + 63) // 64) * 64, np.uint8)
    bits[:hi - lo] = [len(nl[nm].gpus) == 0 for nm in names[lo:hi]]
    nogpu = np.packbits(bits, bitorder="little").view(np.uint64).copy()
    before = eng.download()
    found = eng.find(reqs, util.CLOCK, want_bitmap=False)
    transport = dist_util.TorchTransport(dist)
    res = {}
    for apply in (False, True):
        node, maps, places, status = shard.schedule_batch_sharded(eng, reqs, util.CLOCK, pk, nogpu, transport, apply=apply, chunk=32)
        ids = []
        for i in range(P):
            if node[i] < 0:
                ids.append(None)
                continue
            nd = nl[names[int(node[i])]]
            G = int(reqs[i]["n_groups"])
            gpus = [int(reqs[i]["gpus"][g]) for g in range(G)]
            cpp = int(nd.cores_per_proc)
            assert int(places[i]["status"]) == pack.COMMIT_WIDE                  # (every node is a wide record)
            ids.append(pack.expand_wide_placement(eng.last_wide_places[i], G, cpp, cpp * int(nd.sockets), gpus))
        res[apply] = {"node": node.tolist(), "ids": ids}
        if not apply:
            assert_tables_equal(eng.download(), before)
            again = eng.find(reqs, util.CLOCK, want_bitmap=False)
            assert np.array_equal(again[0], found[0]) and again[2].tobytes() == found[2].tobytes()
    after = eng.download()
    res["share"] = {str(i + lo): after.share[i]["used"].tolist() for i in range(hi - lo)}
    import json
    with open(os.path.join(out_dir, f"share{rank}.json"), "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,seed,n,P", [(2, 9920, 200, 120), (3, 9921, 180, 110)])
def test_mode_b_one_process_per_shard_under_sharing_equals_the_scheduler_loop(tmp_path, sharing, world, seed, n, P):
    """sharding.schedule_batch_sharded under gloo on a sharing cluster, apply=False then apply=True: on every rank the decisions and
    physical ids of the oracle's loop over the whole cluster; apply=False leaves the rank's shard as it was (speed_used included, the
    rank's own finds unchanged); after apply=True every NIC's speed_used equals the oracle's objects."""
    import json
    port = _free_port()
    mp.spawn(_worker_mode_b_sharing, args=(world, port, seed, n, P, str(tmp_path)), nprocs=world, join=True)
    nl, tops = _sharing_case(seed, n, P)
    assert speeds_matter(nl, tops, util.CLOCK)
    names = list(nl)
    ids = []
    onl = copy.deepcopy(nl)
    want = O.schedule_sequence(onl, tops, [None] * P, util.CLOCK, ids_out=ids)
    want_node = [-1 if r[0] is None else names.index(r[0]) for r in want]
    assert sum(v >= shard.shard_bounds(n, world, 1)[0] for v in want_node) >= 3, "the case must place pods past the first shard"
    share = {}
    for rank in range(world):
        with open(tmp_path / f"share{rank}.json") as f:
            got = json.load(f)
        for apply in ("false", "true"):
            assert got[apply]["node"] == want_node, (rank, apply)
            assert got[apply]["ids"] == ids, (rank, apply)
        share.update({int(i): np.array(u) for i, u in got["share"].items()})
    assert sorted(share) == list(range(n))
    for i, node in enumerate(onl.values()):
        assert share[i].tobytes() == share_of(node).tobytes(), node.name


# ---- the digest cache of FindNode -> CommitPlacement -----------------------------------------------------------------------
def test_a_cached_request_committed_after_a_repack_still_notes_its_speeds(sharing):
    """ADVICE r06 (second finding): CommitPlacement reuses the record FindNode digested; a full re-pack in between (pack_nodes starts
    share_exact afresh) must not let a non-dyadic speed reach the mirror unnoticed - after the commit share_exact is False and the next
    group with several RX / TX cores is turned away."""
    descs = util.random_cluster_desc(9800, 6, occupancy=0.05)
    for d in descs:
        d["nic_speed_used"] = [[0.0, 0.0] for _ in d["nic_pods_used"]]
    nl = util.build_cluster(descs)
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=harness.HarnessEngine)
    m.attach(nl)
    split = refmodel.make_topology(dict(map_type="NUMA", hugepages_gb=0, misc=0, misc_smt=True,
                                        groups=[dict(proc=4, helpers=0, rx=10.0, tx=5.0, more_nic_pairs=[(2.5, 2.5)], gpus=[], proc_smt=False, helper_smt=False)]))
    odd = refmodel.make_topology(dict(map_type="NUMA", hugepages_gb=0, misc=0, misc_smt=True,
                                      groups=[dict(proc=2, helpers=0, rx=0.1, tx=5.0, gpus=[], proc_smt=False, helper_smt=False)]))
    r = m.FindNode(nl, odd)
    assert r[0] is not None and not m.packer.share_exact
    m.attach(nl)                                                                    # a full re-pack: every speed_used of the mirror is dyadic
    assert m.packer.share_exact
    ids = m.CommitPlacement(r[0], odd, r[1], busy_time=util.CLOCK)                  # 0.1 Gb/s reaches the mirror's speed_used
    rec = {}
    O.commit(copy.deepcopy(nl)[r[0]], odd, r[1], util.CLOCK, rec)
    assert ids == rec
    assert not m.packer.share_exact
    assert m.FindNode(nl, split) == (None,)


def test_the_digest_cache_holds_a_copy_and_is_spent_by_a_commit(sharing):
    descs = util.random_cluster_desc(9801, 6, occupancy=0.05)
    for d in descs:
        d["nic_speed_used"] = [[0.0, 0.0] for _ in d["nic_pods_used"]]
    nl = util.build_cluster(descs)
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=harness.HarnessEngine)
    m.attach(nl)
    top = refmodel.make_topology(dict(map_type="NUMA", hugepages_gb=0, misc=0, misc_smt=True,
                                      groups=[dict(proc=2, helpers=0, rx=10.0, tx=5.0, gpus=[], proc_smt=False, helper_smt=False)]))
    r = m.FindNode(nl, top)
    assert r[0] is not None
    assert m._digest_cache[0] is top
    m.CommitPlacement(r[0], top, r[1], busy_time=util.CLOCK)
    assert m._digest_cache is None
    m.FindNode(nl, top)
    assert m._digest_cache is not None
    m.attach(nl)
    assert m._digest_cache is None
