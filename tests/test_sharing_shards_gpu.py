"""nhd/Node.py:20 ENABLE_SHARING = True across shards on the MI355X (`pytest -m gpu`): the device forms of tests/test_sharing_shards.py.
Mode B that commits and puts the shards back (GroupEngine.schedule_batch and sharding.schedule_batch_sharded with apply=False) must
restore the NICs' speed_used records with the planes, and a slice refused for lack of them must leave the device as it was - each
held against the Python oracle with its switch flipped, on clusters where zeroing every speed_used changes an answer."""
import copy

import numpy as np
import pytest

from nhd_amd import sharding
from nhd_amd._lib import NhdFitError
from nhd_amd.engine import Engine
from nhd_amd.matcher import HipMatcher
from oracle import nhd_oracle as O
from tests import util
from tests.test_sharing_shards import assert_speed_used_equals, assert_tables_equal, sharing_problem, speeds_matter
from tests.wide_check import as_jsonable
from workload import refmodel

pytestmark = pytest.mark.gpu


@pytest.fixture
def sharing(monkeypatch):
    monkeypatch.setattr(refmodel, "ENABLE_SHARING", True)
    monkeypatch.setattr(O, "ENABLE_SHARING", True)


def _case(seed, n, P, n_big=0):
    descs, specs = sharing_problem(seed, n, P, n_big)
    nl = util.build_cluster(descs)
    tops = [refmodel.make_topology(s) for s in specs]
    assert speeds_matter(nl, tops, util.CLOCK)
    return nl, tops


def _shard_shares(engine):
    return [s.wide_share_download().copy() for s in engine.shards]


@pytest.mark.parametrize("seed,n_big", [(9960, 0), (9961, 3)])
def test_group_of_shards_on_one_gpu_restores_speed_used(sharing, seed, n_big):
    """(e) HipMatcher(devices=[0, 0, 0]) - three device contexts on one MI355X - ScheduleBatch(apply=False) on a sharing cluster: the
    oracle's loop over the whole cluster, the mirror bit for bit as before (every shard's speed_used included), FindNodes / ExplainNodes
    as before; then apply=True equals the oracle again and leaves every NIC's speed_used as the oracle's objects."""
    n, P = 512, 120
    nl, tops = _case(seed, n, P, n_big)
    ids = []
    onl = copy.deepcopy(nl)
    want = O.schedule_sequence(onl, tops, [None] * P, util.CLOCK, ids_out=ids)
    m = HipMatcher(clock=lambda: util.CLOCK, devices=[0, 0, 0], engine_factory=Engine)
    m.attach(nl)
    assert m.packer.sharing and len(m.wide_nodes) == n
    before = m.engine.download()
    shares = _shard_shares(m.engine)
    assert before.share is not None and len(before.share) == n
    found = m.FindNodes(nl, tops, now=util.CLOCK)
    assert [as_jsonable(r) for r in found] == [as_jsonable(O.find_node(nl, t, util.CLOCK)) for t in tops]
    explained = [e.counts for e in m.ExplainNodes(nl, tops, now=util.CLOCK)]

    got = m.ScheduleBatch(nl, tops, now=util.CLOCK)                                 # apply=False
    if not n_big:                                                                   # (pods of 5..7 groups: the touched nodes are re-packed
        assert_tables_equal(m.engine.download(), before)                            #  from their objects before the next call)
        for a, b in zip(_shard_shares(m.engine), shares):
            assert a.tobytes() == b.tobytes()
    assert [as_jsonable(r) for r in got] == [as_jsonable(w) for w in want]
    assert m.last_placements == ids
    names = list(nl)
    placed = [w for w in want if w[0] is not None]
    assert len(placed) >= 30
    assert any(names.index(w[0]) >= m.engine._bounds[0][1] for w in placed), "the case must place pods past the first shard"
    assert [as_jsonable(r) for r in m.FindNodes(nl, tops, now=util.CLOCK)] == [as_jsonable(r) for r in found]
    assert [e.counts for e in m.ExplainNodes(nl, tops, now=util.CLOCK)] == explained
    assert_tables_equal(m.engine.download(), before)
    for a, b in zip(_shard_shares(m.engine), shares):
        assert a.tobytes() == b.tobytes()

    again = m.ScheduleBatch(nl, tops, now=util.CLOCK, apply=True)
    assert [as_jsonable(r) for r in again] == [as_jsonable(w) for w in want]
    assert m.last_placements == ids
    assert_speed_used_equals(m.engine.download().share, onl)
    m.engine.close()


def test_one_rccl_rank_restores_its_whole_shard_with_speed_used(sharing):
    """(f) sharding.schedule_batch_sharded over the engine's own communicator of one rank, apply=False: the restore covers the whole
    shard (the case that used to switch the sharing arithmetic off without a word).  Decisions as the oracle's loop; afterwards the
    device's speed_used is what it was and HipMatcher's FindNodes on the same engine answers as the oracle."""
    n, P = 384, 120
    nl, tops = _case(9962, n, P)
    names = list(nl)
    want = O.schedule_sequence(copy.deepcopy(nl), tops, [None] * P, util.CLOCK)      # (before attach: it hooks the matcher into the objects)
    m = HipMatcher(clock=lambda: util.CLOCK, strict=True)
    m.attach(nl)
    eng = m.engine
    before = eng.download()
    share = eng.wide_share_download().copy()
    assert len(share) == n
    eng.comm_init(1, 0, eng.unique_id())
    try:
        reqs = m.packer.digest_many(tops)
        bits = np.zeros(((n + 63) // 64) * 64, np.uint8)
        bits[:n] = [len(nd.gpus) == 0 for nd in nl.values()]
        nogpu = np.packbits(bits, bitorder="little").view(np.uint64).copy()
        node, _, _, _ = sharding.schedule_batch_sharded(eng, reqs, util.CLOCK, m.packer, nogpu, sharding.RcclTransport(eng), apply=False, chunk=48)
        assert node.tolist() == [-1 if w[0] is None else names.index(w[0]) for w in want]
        assert (node >= 0).sum() >= 30
        assert eng.wide_share_download().tobytes() == share.tobytes()
        assert_tables_equal(eng.download(), before)
        assert [as_jsonable(r) for r in m.FindNodes(nl, tops, now=util.CLOCK)] == [as_jsonable(O.find_node(nl, t, util.CLOCK)) for t in tops]
    finally:
        eng.comm_destroy()
        eng.close()


def test_a_refused_slice_changes_nothing_on_the_device(sharing):
    """(g) Under ENABLE_SHARING an Engine.upload of a slice without speed_used records raises NhdFitError before any nhdfit_* call: the
    device keeps its records and its sharing arithmetic, and FindNodes still answers exactly as the oracle."""
    n, P = 256, 60
    nl, tops = _case(9963, n, P)
    m = HipMatcher(clock=lambda: util.CLOCK, strict=True)
    m.attach(nl)
    eng = m.engine
    before = eng.download()
    share = eng.wide_share_download().copy()
    bare = eng.download(40, 30)
    bare.share = None
    with pytest.raises(NhdFitError):
        eng.upload(bare, first=40, capacity=n)
    whole = eng.download()
    whole.share = None
    with pytest.raises(NhdFitError):
        eng.upload(whole)
    assert eng.sharing
    assert eng.wide_share_download().tobytes() == share.tobytes()
    assert_tables_equal(eng.download(), before)
    assert [as_jsonable(r) for r in m.FindNodes(nl, tops, now=util.CLOCK)] == [as_jsonable(O.find_node(nl, t, util.CLOCK)) for t in tops]
    eng.close()


@pytest.mark.parametrize("devices", [None, [0, 0, 0]], ids=["one-context", "three-shards"])
def test_a_repack_without_sharing_switches_the_device_off_and_back(monkeypatch, devices):
    """HipMatcher re-packing a cluster whose module no longer shares NICs empties the engine first (Engine.reset_nodes ends sharing on
    the device): the device then answers as the oracle without sharing; with the constant back, as the oracle with it."""
    descs, specs = sharing_problem(9964, 200, 40)
    tops = [refmodel.make_topology(s) for s in specs]
    want = {}
    for on in (True, False):
        monkeypatch.setattr(O, "ENABLE_SHARING", on)
        nl = util.build_cluster(descs)
        want[on] = [as_jsonable(O.find_node(nl, t, util.CLOCK)) for t in tops]
    assert want[True] != want[False], "the case must tell the two modes apart"
    m = HipMatcher(clock=lambda: util.CLOCK, devices=devices, engine_factory=Engine if devices else None, strict=True)
    for on in (True, False, True):
        monkeypatch.setattr(refmodel, "ENABLE_SHARING", on)
        monkeypatch.setattr(O, "ENABLE_SHARING", on)
        nl = util.build_cluster(descs)
        m.attach(nl)
        assert bool(m.packer.sharing) == on and bool(m.engine.download().share) == on
        assert [as_jsonable(r) for r in m.FindNodes(nl, tops, now=util.CLOCK)] == want[on]
    m.engine.close()
