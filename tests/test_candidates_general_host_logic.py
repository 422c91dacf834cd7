"""HipMatcher.Candidates / CandidatesMany(general=...) on the host twin (tests/harness/candidates_general_twin.py), without a GPU: the
default never reaches the new entry; general=True answers every ordinary pod with the device entry on any mirror and still composes
pods of the general path; on a plain mirror it changes nothing; `error` and `strict`; K out of range; three twin shards equal one twin."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd._lib import NhdFitError
from nhd_amd.matcher import HipMatcher
from tests import candidates_general_check as cg
from tests import candidates_reference as cr
from tests import headroom_general_check as gc
from tests import util
from tests.harness.candidates_general_twin import CandidatesGeneralHarnessEngine
from tests.test_big_core import big_spec
from workload import refmodel


class Spy(CandidatesGeneralHarnessEngine):
    """Counts the calls of either entry."""
    calls = None

    def candidates(self, reqs, now, k, cand=None, **kw):
        Spy.calls.append((len(reqs), bool(kw.get("general", False))))
        return super().candidates(reqs, now, k, cand=cand, **kw)


def _matcher(engine=CandidatesGeneralHarnessEngine, **kw):
    return HipMatcher(clock=lambda: util.CLOCK, engine_factory=engine, **kw)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.error is None and y.error is None
        assert x.entries == y.entries and (x.feasible, x.preferred, x.k, x.nodes) == (y.feasible, y.preferred, y.k, y.nodes)


def _tops():
    return [refmodel.make_topology(s) for s in cg.templates()]


@pytest.mark.parametrize("name", ["plain", "mixed", "sharing_random"])
def test_the_default_never_reaches_the_new_entry(name):
    """general=False: today's routes - the plain entry on a plain mirror, no device entry at all where the mirror has wide records;
    general=True: one call of the new entry for all ordinary pods, on any mirror, and the composed form's answer."""
    sharing = name.startswith("sharing")
    with gc.sharing_all(sharing):
        nl = util.random_cluster(1720, 60, occupancy=0.15) if name == "plain" else util.build_cluster(gc.cluster_case(name)[1])
        m = _matcher(Spy)
        Spy.calls = []
        old = m.CandidatesMany(nl, _tops(), k=5, now=util.CLOCK)
        assert Spy.calls == ([(18, False)] if name == "plain" else [])
        assert m.Candidates(nl, _tops()[0], k=5, now=util.CLOCK).entries == old[0].entries
        assert all(not general for _, general in Spy.calls)
        Spy.calls = []
        new = m.CandidatesMany(nl, _tops(), k=5, now=util.CLOCK, general=True)
        assert Spy.calls == [(18, True)]
        assert m.Candidates(nl, _tops()[0], k=5, now=util.CLOCK, general=True).entries == new[0].entries
    _same(old, new)
    assert sum(len(c.entries) for c in new) > 20
    wide = bool(m.wide_nodes)
    assert wide == (name != "plain")
    assert all(bool(c.form & pack.CANDIDATES_FORM_WIDE) == wide for c in new) and not any(c.form & pack.CANDIDATES_FORM_WIDE for c in old)


def test_a_big_pod_is_still_composed():
    """A pod of 5..8 groups beside ordinary ones under general=True: the ordinary ones take the new entry, the big one does not, and its
    list is FindNodes iterated on a dict that loses each answer."""
    rng = np.random.default_rng(1730)
    nl = util.mixed_cluster(1730, 50, occupancy=0.1)
    big = refmodel.make_topology(big_spec(rng))
    assert pack.needs_general_path(big)
    tops = [refmodel.make_topology(gc.GPULESS), big, refmodel.make_topology(gc.FOUR[0])]
    m = _matcher(Spy)
    Spy.calls = []
    got = m.CandidatesMany(nl, tops, k=4, now=util.CLOCK, general=True)
    assert Spy.calls == [(2, True)]
    assert all(c.error is None for c in got) and got[1].form == 0 and got[0].form & pack.CANDIDATES_FORM_WIDE
    fresh = _matcher()
    want = cr.iterate(lambda sub, t: fresh.FindNodes(sub, [t], now=util.CLOCK)[0], nl, lambda: big, k=4)
    assert [cr.entry(e) for e in got[1].entries] == want
    _same([got[0], got[2]], m.CandidatesMany(nl, [tops[0], tops[2]], k=4, now=util.CLOCK))


def test_k_out_of_range_errors_and_strict():
    rng = np.random.default_rng(1740)
    nl = util.mixed_cluster(1740, 30, occupancy=0.1)
    ok = refmodel.make_topology(gc.GPULESS)
    none = refmodel.make_topology(dict(util.random_pod_spec(rng), groups=[]))
    beyond = refmodel.make_topology(big_spec(rng, 9, 9))
    m = _matcher()
    for k in (0, 65, -1):
        with pytest.raises(ValueError):
            m.Candidates(nl, ok, k=k, general=True)
        with pytest.raises(ValueError):
            m.CandidatesMany(nl, [ok], k=k, general=True)
    got = m.CandidatesMany(nl, [ok, none, beyond], k=3, now=util.CLOCK, general=True)
    assert got[0].error is None and len(got[0].entries) == 3
    for c in got[1:]:
        assert c.error is not None and c.entries == [] and c.feasible == 0
    for bad in (none, beyond):
        with pytest.raises(pack.UnsupportedNode):
            m.CandidatesMany(nl, [ok, bad], k=3, now=util.CLOCK, strict=True, general=True)
    assert m.CandidatesMany(nl, [], k=3, general=True) == []
    assert [(c.entries, c.error) for c in m.CandidatesMany({}, [ok], k=3, general=True)] == [([], None)]

    class Failing(CandidatesGeneralHarnessEngine):
        def candidates(self, reqs, now, k, cand=None, general=False):
            assert general
            raise NhdFitError(-6, "the set model of a wide node's mapping outgrew its table")

    c = _matcher(Failing).Candidates(nl, ok, k=3, general=True)
    assert c.entries == [] and "outgrew its table" in c.error
    with pytest.raises(NhdFitError):
        _matcher(Failing, strict=True).Candidates(nl, ok, k=3, general=True)


@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
@pytest.mark.parametrize("k", [1, 8, 64])
def test_three_twin_shards_equal_one_twin(k, sharing):
    """GroupEngine over three twin shards (sharding.merge_candidates, unchanged): every shard ranks its own wide records with its
    global base; the merged lists and sums are the unsharded twin's."""
    with gc.sharing_all(sharing):
        nl = util.mixed_cluster(1750, 75, occupancy=0.1)
        one = _matcher().CandidatesMany(nl, _tops(), k=k, now=util.CLOCK, general=True)
        grp = _matcher(devices=[0, 0, 0])
        assert len(grp.engine.shards) == 3
        many = grp.CandidatesMany(nl, _tops(), k=k, now=util.CLOCK, general=True)
    _same(one, many)
    assert [c.form for c in one] == [c.form for c in many] and all(c.form & pack.CANDIDATES_FORM_WIDE for c in one)
    assert sum(len(c.entries) for c in one) > 2 * k and max(c.feasible for c in one) > min(k, 30)
    names = np.array(list(nl))
    owners = {int(np.flatnonzero(names == e[0])[0]) * 3 // len(names) for c in one for e in c.entries}
    assert len(owners) >= 2 or k == 1                           # (the lists draw on more than one shard)
