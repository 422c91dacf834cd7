"""HipMatcher.Headroom's host logic (no GPU): over a fake engine - what reaches the engine (candidate mask, the pods' node groups,
the cap, a closed dictionary) and how its records come back (`nl` order, by_node(), the summary sentence) - and over the host twin:
two shards give what one gives, and a template no request record can express comes back with `error` set and everything not
evaluated (strict raises) instead of a guessed number."""
import logging

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd._lib import NhdFitError
from nhd_amd.matcher import Headroom, HipMatcher
from tests import harness, util
from tests.harness.headroom_twin import HeadroomHarnessEngine
from tests.test_big_core import big_spec
from workload import refmodel


class FakeEngine(harness.HarnessEngine):
    """Records the call and answers entry = node index (+ flags on two nodes)."""
    calls = []

    def headroom(self, reqs, cand=None, max_per_node=512, per_node=False):
        FakeEngine.calls.append(dict(reqs=np.array(reqs), cand=None if cand is None else np.array(cand), cap=max_per_node, per_node=per_node,
                                     nsig=len(self.packer.dictionary_arrays()[1]) - 1))
        P, n = len(reqs), self.n
        e = np.tile(np.arange(n, dtype=np.uint16), (P, 1))
        e[:, 3] |= pack.HEADROOM_STOPPED
        e[:, 5] = pack.HEADROOM_NOT_EVALUATED
        if cand is not None:
            bits = np.unpackbits(np.asarray(cand).view(np.uint8), bitorder="little")[:n].astype(bool)
            e[:, ~bits] = 0
        k = e & pack.HEADROOM_COUNT_MASK
        sums = np.zeros(P, pack.HEADROOM_SUM)
        sums["replicas"], sums["nodes_with_room"], sums["max_on_one_node"] = k.sum(1), (k > 0).sum(1), k.max(1)
        sums["stopped"], sums["not_evaluated"] = ((e & pack.HEADROOM_STOPPED) != 0).sum(1), ((e & pack.HEADROOM_NOT_EVALUATED) != 0).sum(1)
        sums["saturated"], sums["form"] = (k >= max_per_node).sum(1), pack.HEADROOM_FORM_WAVE
        return sums, (e if per_node else None)


def test_what_reaches_the_engine_and_how_it_comes_back():
    FakeEngine.calls = []
    nl = util.random_cluster(8800, 70)
    names = list(nl)
    rng = np.random.default_rng(88)
    tops = [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(3)]
    groups = [["default"], ["alpha", "beta"], ["beta"]]
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=FakeEngine)
    m.attach(nl)
    got = m.HeadroomMany(nl, tops, pod_groups=groups, per_node=True, max_per_node=40)
    call = FakeEngine.calls[-1]
    assert call["cand"] is None and call["cap"] == 40 and call["per_node"] and len(call["reqs"]) == 3
    assert (call["reqs"]["flags"] & pack.RF_INITIAL_FILTER != 0).all()
    want = m.packer.digest_many(tops, groups)
    assert call["reqs"].tobytes() == want.tobytes()
    h = got[1]
    assert h.nodes == 70 and h.per_node.tolist() == [0, 1, 2, 3, 4, 0] + list(range(6, 70)) and h.by_node()[names[9]] == 9
    assert h.flags[3] == pack.HEADROOM_STOPPED and h.flags[5] == pack.HEADROOM_NOT_EVALUATED and h.flags.astype(bool).sum() == 2
    assert (h.replicas, h.nodes_with_room, h.max_on_one_node, h.saturated, h.stopped, h.not_evaluated) == (sum(range(70)) - 5, 68, 69, 30, 1, 1)
    # a subset of the attached dict: the candidate mask, results in the subset's order
    sub = {k: nl[k] for k in names[10:50:3]}
    one = m.Headroom(sub, tops[0], per_node=True)
    call = FakeEngine.calls[-1]
    bits = np.unpackbits(call["cand"].view(np.uint8), bitorder="little")[:70].astype(bool)
    assert bits.tolist() == [nm in sub for nm in names] and call["cap"] == 512
    assert one.nodes == len(sub) and one.by_node() == {k: names.index(k) for k in sub} and list(one.by_node()) == list(sub)
    assert (call["reqs"]["flags"] & pack.RF_INITIAL_FILTER == 0).all()
    # without per_node there is no per-node array, and by_node() says so
    lean = m.Headroom(nl, tops[0])
    assert lean.per_node is None and lean.flags is None and lean.replicas == h.replicas and not FakeEngine.calls[-1]["per_node"]
    with pytest.raises(ValueError):
        lean.by_node()
    assert m.HeadroomMany(nl, []) == [] and m.Headroom({}, tops[0], per_node=True).replicas == 0


def test_summary_text():
    h = Headroom(65536, replicas=1234, nodes_with_room=410, max_on_one_node=7)
    assert h.summary() == "1 234 more replicas on 410 of 65 536 nodes (most on one node: 7)"
    assert repr(h) == "Headroom('1 234 more replicas on 410 of 65 536 nodes (most on one node: 7)')"
    h = Headroom(2000, replicas=1024000, nodes_with_room=2000, max_on_one_node=512, saturated=2000, stopped=3, not_evaluated=12, unmirrored=1, max_per_node=512)
    assert h.summary() == ("1 024 000 more replicas on 2 000 of 2 000 nodes (most on one node: 512); 2 000 reached the limit of 512 per node, "
                           "3 stopped at a placement the scheduler would fail on, 12 not evaluated, 1 not mirrored on the device")
    h = Headroom(30, not_evaluated=30, error="it takes the general path")
    assert h.summary() == "the pod was not evaluated against the 30 nodes: it takes the general path."


def test_pods_the_call_cannot_express(caplog):
    nl = util.random_cluster(8900, 40)
    rng = np.random.default_rng(89)
    ok = util.random_pod_spec(rng)
    ok["map_type"] = "NUMA"
    odd = util.random_pod_spec(rng)
    odd["groups"][0]["proc"] = 300                           # a group of more than 255 cores: beyond the request record
    huge = dict(ok, hugepages_gb=pack.MAX_HUGEPAGES_GB + 1)  # beyond the pod tile: the general path's
    tops = [refmodel.make_topology(s) for s in (ok, odd, big_spec(rng, 5, 6), huge)]
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomHarnessEngine)
    with caplog.at_level(logging.ERROR):
        a, b, c, d = m.HeadroomMany(nl, tops, per_node=True)
    assert a.error is None and a.per_node is not None and a.not_evaluated == 0
    for h, word in ((b, "request record"), (c, "general path"), (d, "general path")):
        assert h.error is not None and word in h.error
        assert (h.replicas, h.nodes_with_room, h.max_on_one_node, h.not_evaluated, h.per_node, h.nodes) == (0, 0, 0, len(nl), None, len(nl))
        assert "not evaluated" in h.summary() and "more replicas" not in h.summary()
    assert sum("not evaluated" in r.message for r in caplog.records) == 3
    alone = m.Headroom(nl, tops[0], per_node=True)           # the evaluated template is what it is on its own
    assert np.array_equal(alone.per_node, a.per_node) and alone.replicas == a.replicas
    strict = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomHarnessEngine, strict=True)
    for bad in tops[1:]:
        with pytest.raises(pack.UnsupportedNode):
            strict.HeadroomMany(nl, [tops[0], bad])
    with pytest.raises(pack.UnsupportedNode):
        m.Headroom(nl, tops[2], strict=True)
    assert strict.Headroom(nl, tops[0]).replicas == a.replicas


class _Failing(HeadroomHarnessEngine):
    def headroom(self, reqs, cand=None, max_per_node=512, per_node=False):
        raise NhdFitError(-6, "headroom: the dictionary's signature stream does not fit the block's LDS")


def test_a_device_error_is_reported_not_raised():
    nl = util.random_cluster(9000, 20)
    top = refmodel.make_topology(util.random_pod_spec(np.random.default_rng(90)))
    h = HipMatcher(clock=lambda: util.CLOCK, engine_factory=_Failing).Headroom(nl, top)
    assert h.error is not None and "signature stream" in h.error and h.not_evaluated == len(nl) and h.replicas == 0
    with pytest.raises(NhdFitError):
        HipMatcher(clock=lambda: util.CLOCK, engine_factory=_Failing, strict=True).Headroom(nl, top)


def test_two_shards_equal_one():
    nl = util.random_cluster(9050, 150, occupancy=0.1)       # shards of 128 + 22 nodes
    rng = np.random.default_rng(905)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(16)]
    one = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomHarnessEngine)
    two = HipMatcher(clock=lambda: util.CLOCK, engine_factory=HeadroomHarnessEngine, devices=[0, 1])
    assert len(two.engine.shards) == 2
    sub = {k: v for i, (k, v) in enumerate(nl.items()) if i % 3}
    for cands in (nl, sub):
        for x, y in zip(one.HeadroomMany(cands, tops, per_node=True), two.HeadroomMany(cands, tops, per_node=True)):
            assert np.array_equal(x.per_node, y.per_node) and np.array_equal(x.flags, y.flags) and x.summary() == y.summary() and x.form == y.form
        one.attach(nl)
        two.attach(nl)
    assert sum(x.replicas for x in one.HeadroomMany(nl, tops)) > 50
