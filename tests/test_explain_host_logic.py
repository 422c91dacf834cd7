"""HipMatcher.ExplainNodes' host logic on the host build of the stage function (no GPU): a mirror cut into two shards gives
what one gives (counts summed over the shards, per-node stages put together in node order), and a pod the device cannot
evaluate is reported as such - logged, `error` set - instead of being charged to the cluster."""
import logging

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd._lib import NhdFitError
from nhd_amd.matcher import STAGES, HipMatcher
from tests import util
from tests.harness.explain_twin import ExplainHarnessEngine
from tests.test_big_core import big_spec
from workload import refmodel


def _pair():
    one = HipMatcher(clock=lambda: util.CLOCK, engine_factory=ExplainHarnessEngine)
    two = HipMatcher(clock=lambda: util.CLOCK, engine_factory=ExplainHarnessEngine, devices=[0, 1])
    return one, two


def test_two_shards_equal_one():
    nl = util.random_cluster(8200, 150)                      # shards of 128 + 22 nodes (multiples of 64)
    rng = np.random.default_rng(82)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(12)]
    tops += [refmodel.make_topology(big_spec(rng, 5, 6)) for _ in range(2)]
    one, two = _pair()
    assert len(two.engine.shards) == 2
    for x, y in zip(one.ExplainNodes(nl, tops, per_node=True), two.ExplainNodes(nl, tops, per_node=True)):
        assert x.counts == y.counts and np.array_equal(x.stages, y.stages) and y.total == len(nl)
        assert [y.counts[s] for s in STAGES] == np.bincount(y.stages, minlength=len(STAGES)).tolist()
    one.attach(nl)
    two.attach(nl)
    sub = {k: v for i, (k, v) in enumerate(nl.items()) if i % 3}   # a candidate mask across both shards
    for x, y in zip(one.ExplainNodes(sub, tops, per_node=True), two.ExplainNodes(sub, tops, per_node=True)):
        assert x.counts == y.counts and np.array_equal(x.stages, y.stages) and y.total == len(sub) == sum(y.counts.values())


def test_a_pod_no_record_can_express_is_not_blamed_on_the_cluster(caplog):
    nl = util.random_cluster(8300, 30)
    rng = np.random.default_rng(83)
    ok = util.random_pod_spec(rng)
    odd = util.random_pod_spec(rng)
    odd["groups"][0]["proc"] = 300                           # a group of more than 255 cores: beyond the request record
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=ExplainHarnessEngine)
    with caplog.at_level(logging.ERROR):
        a, b = m.ExplainNodes(nl, [refmodel.make_topology(ok), refmodel.make_topology(odd)], per_node=True)
    assert a.error is None and sum(a.counts.values()) == len(nl)
    assert b.error is not None and "request record" in b.error and b.stages is None
    assert sum(b.counts.values()) == 0 and b.total == len(nl)
    assert "not evaluated" in b.summary() and "not candidates" not in b.summary()
    assert any("not evaluated" in r.message for r in caplog.records)
    assert m.FindNodes(nl, [refmodel.make_topology(odd)]) == [(None,)]


class _BudgetOut(ExplainHarnessEngine):
    def explain(self, reqs, now, cand=None, per_node=False):
        if reqs.dtype == pack.BIG_REQ:
            raise NhdFitError(-6, "a big request's NIC stage ran out of search budget on some node")
        return super().explain(reqs, now, cand=cand, per_node=per_node)


def test_a_search_beyond_its_budget_is_reported_not_raised():
    nl = util.random_cluster(8400, 20)
    rng = np.random.default_rng(84)
    tops = [refmodel.make_topology(util.random_pod_spec(rng)), refmodel.make_topology(big_spec(rng, 5, 6))]
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=_BudgetOut)
    a, b = m.ExplainNodes(nl, tops)
    assert a.error is None and b.error is not None and "budget" in b.error and sum(b.counts.values()) == 0
    strict = HipMatcher(clock=lambda: util.CLOCK, engine_factory=_BudgetOut, strict=True)
    with pytest.raises(NhdFitError):
        strict.ExplainNodes(nl, tops)
