"""HipMatcher.Candidates / CandidatesMany(big=...) on the host twin (tests/harness/candidates_big_twin.py), without a GPU: the default
never reaches the new entry; big=True answers all pods of the general path with ONE candidates_big call beside the one candidates call
of the others, whatever `general` says and on any mirror; `error` and `strict`; K out of range; a pod beyond the big record; a search
budget that runs out; no side effects."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd._lib import NhdFitError
from nhd_amd.matcher import HipMatcher
from tests import headroom_general_check as gc
from tests import util
from tests.harness.candidates_big_twin import CandidatesBigHarnessEngine
from tests.test_big_core import big_spec
from tests.test_candidates_big_core import seam_specs
from workload import refmodel


class Spy(CandidatesBigHarnessEngine):
    """Records the calls of either entry: ("small", pods, general) / ("big", pods)."""
    calls = None

    def candidates(self, reqs, now, k, cand=None, **kw):
        Spy.calls.append(("small", len(reqs), bool(kw.get("general", False))))
        return super().candidates(reqs, now, k, cand=cand, **kw)

    def candidates_big(self, reqs, now, k, cand=None):
        Spy.calls.append(("big", len(reqs)))
        return super().candidates_big(reqs, now, k, cand=cand)


def _matcher(engine=CandidatesBigHarnessEngine, **kw):
    return HipMatcher(clock=lambda: util.CLOCK, engine_factory=engine, **kw)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.error is None and y.error is None
        assert x.entries == y.entries and (x.feasible, x.preferred, x.k, x.nodes) == (y.feasible, y.preferred, y.k, y.nodes)


def _tops():
    """An ordinary pod, two of the general path, another ordinary one, a third of the general path."""
    big = seam_specs()
    return [refmodel.make_topology(s) for s in (gc.GPULESS, big[0], big[1], gc.FOUR[0], big[2])]


@pytest.mark.parametrize("name", ["plain", "mixed", "sharing_random"])
def test_routes(name):
    """big=False: today's calls, with and without `general` - candidates_big is never called.  big=True: one candidates_big call for
    the three pods of the general path; the others go where `general` sends them - the device entry where it answers the mirror, the
    composed form elsewhere.  Whatever the route, the answers are the composed form's."""
    sharing = name.startswith("sharing")
    with gc.sharing_all(sharing):
        nl = util.random_cluster(1720, 60, occupancy=0.15) if name == "plain" else util.build_cluster(gc.cluster_case(name)[1])
        m = _matcher(Spy)
        seen = {}
        for general in (False, True):
            for big in (False, True):
                Spy.calls = []
                kw = dict(general=True) if general else {}
                if big:
                    kw["big"] = True
                got = m.CandidatesMany(nl, _tops(), k=5, now=util.CLOCK, **kw)
                seen[general, big] = (got, list(Spy.calls))
                one = m.Candidates(nl, _tops()[1], k=5, now=util.CLOCK, **kw)
                assert one.entries == got[1].entries
    plain_mirror = name == "plain"
    for general in (False, True):
        small = [("small", 2, general)] if general or plain_mirror else []
        assert seen[general, False][1] == small
        assert seen[general, True][1] == small + [("big", 3)]
        assert not any(c[0] == "big" for c in seen[general, False][1])
    base = seen[False, False][0]
    for key, (got, _) in seen.items():
        _same(base, got)
        for p in (1, 2, 4):
            assert got[p].form == (pack.CANDIDATES_FORM_BIG if key[1] else 0)
    assert sum(len(base[p].entries) for p in (1, 2, 4)) >= 6


def test_k_out_of_range_a_nine_group_pod_and_strict():
    rng = np.random.default_rng(1740)
    nl = util.mixed_cluster(1740, 30, occupancy=0.1)
    ok = refmodel.make_topology(seam_specs()[0])
    none = refmodel.make_topology(dict(util.random_pod_spec(rng), groups=[]))
    beyond = refmodel.make_topology(big_spec(rng, 9, 9))
    assert pack.needs_general_path(ok) and not pack.needs_general_path(beyond)
    m = _matcher()
    for k in (0, 65, -1):
        with pytest.raises(ValueError):
            m.Candidates(nl, ok, k=k, big=True)
        with pytest.raises(ValueError):
            m.CandidatesMany(nl, [ok], k=k, big=True)
    got = m.CandidatesMany(nl, [ok, none, beyond], k=3, now=util.CLOCK, big=True)
    assert got[0].error is None and len(got[0].entries) == 3 and got[0].form == pack.CANDIDATES_FORM_BIG
    for c in got[1:]:
        assert c.error is not None and c.entries == [] and c.feasible == 0
    for bad in (none, beyond):
        with pytest.raises(pack.UnsupportedNode):
            m.CandidatesMany(nl, [ok, bad], k=3, now=util.CLOCK, strict=True, big=True)
    assert m.CandidatesMany(nl, [], k=3, big=True) == []
    assert [(c.entries, c.error) for c in m.CandidatesMany({}, [ok], k=3, big=True)] == [([], None)]

    # a group of more cores than the big record holds: beyond it too
    huge = seam_specs()[0]
    huge["groups"][0]["proc"] = 300
    top = refmodel.make_topology(huge)
    assert pack.needs_general_path(top)
    c = m.Candidates(nl, top, k=3, now=util.CLOCK, big=True)
    assert c.error is not None and c.entries == []
    with pytest.raises(pack.UnsupportedNode):
        m.Candidates(nl, top, k=3, now=util.CLOCK, big=True, strict=True)

    class Failing(CandidatesBigHarnessEngine):
        def candidates_big(self, reqs, now, k, cand=None):
            raise NhdFitError(-6, "the set model of a big request's mapping outgrew its table")

    mf = _matcher(Failing)
    c = mf.Candidates(nl, ok, k=3, big=True)
    assert c.entries == [] and "outgrew its table" in c.error
    assert not mf._mirror_foreign                        # (the call writes nothing: the mirror is what it was)
    with pytest.raises(NhdFitError):
        _matcher(Failing, strict=True).Candidates(nl, ok, k=3, big=True)


def test_a_search_budget_that_runs_out_fails_the_call(caplog):
    """A (pod, node) pair whose NIC search runs out of steps (a tiny budget injected into the twin): `error`, an empty list, and the
    log says why - no half-answered list; strict raises."""
    nl = util.random_cluster(49500, 16, occupancy=0.0)
    tops = [refmodel.make_topology(s) for s in seam_specs()]
    free = _matcher().CandidatesMany(nl, tops, k=4, now=util.CLOCK, big=True)
    assert all(c.error is None for c in free) and sum(len(c.entries) for c in free) >= 4       # (the NIC stage is reached)

    class Tight(CandidatesBigHarnessEngine):
        nic_budget = 3
    with caplog.at_level("ERROR"):
        got = _matcher(Tight).CandidatesMany(nl, tops, k=4, now=util.CLOCK, big=True)
    assert all(c.error is not None and c.entries == [] and c.feasible == 0 for c in got)
    assert "search budget" in caplog.text
    with pytest.raises(NhdFitError):
        _matcher(Tight, strict=True).CandidatesMany(nl, tops, k=4, now=util.CLOCK, big=True)
    m = _matcher(Tight)
    m.attach(nl)
    reqs = np.array([m.packer.digest_big(t) for t in tops], dtype=pack.BIG_REQ)
    with pytest.raises(NhdFitError):
        m.engine.candidates_big(reqs, util.CLOCK, 4)


@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
def test_no_side_effects(sharing):
    """The mirror - planes, wide records, share records - downloaded before and after a call is the same bytes, the call twice gives
    the same answer, and FindNodes answers as before."""
    with gc.sharing_all(sharing):
        nl = util.mixed_cluster(9891, 90, occupancy=0.1)
        tops = lambda: [refmodel.make_topology(s) for s in seam_specs()]      # noqa: E731
        m = _matcher()
        found = m.FindNodes(nl, tops(), now=util.CLOCK)
        eng = m.engine

        def state():
            t = eng.download()
            out = [np.array(getattr(t, f)).tobytes() for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
            out.append(eng.wide_download().tobytes())
            if sharing:
                out.append(eng.wide_share_download().tobytes())
            return out
        before = state()
        a = m.CandidatesMany(nl, tops(), k=16, now=util.CLOCK, big=True)
        assert state() == before
        b = m.CandidatesMany(nl, tops(), k=16, now=util.CLOCK, big=True)
        _same(a, b)
        assert m.FindNodes(nl, tops(), now=util.CLOCK) == found
    assert sum(len(c.entries) for c in a) > 10 and len(m.wide_nodes) > 10
