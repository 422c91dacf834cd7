"""nhdfit_headroom_limits' host twin (tests/harness/headroom_limit_twin.cpp) on random clusters: the identities of include/nhdfit.h
(histogram + stopped + not evaluated = nodes, BUSY never, FITS only at the cap), counts and sums equal to plain headroom's twin, a
node without room charged with the stage the explain twin names on the untouched mirror, candidate masks and node groups, wide
nodes, and what HipMatcher makes of it (Headroom.limits, limit_stages, limit_summary(); summary() unchanged)."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import STAGES, UNMIRRORED, HipMatcher
from oracle import nhd_oracle as O
from tests import headroom_limit_check as lc
from tests import util
from tests.harness.explain_twin import ExplainHarnessEngine
from tests.harness.headroom_limit_twin import HeadroomLimitHarnessEngine
from tests.harness.headroom_twin import HeadroomHarnessEngine
from workload import refmodel


class TwinEngine(HeadroomLimitHarnessEngine, ExplainHarnessEngine):
    pass


def _matcher(factory=TwinEngine):
    return HipMatcher(clock=lambda: util.CLOCK, engine_factory=factory)


def _mask_words(keep):
    bits = np.zeros(((len(keep) + 63) // 64) * 64, bool)
    bits[:len(keep)] = keep
    return np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))


@pytest.mark.parametrize("seed", range(3))
def test_identities_and_plain_headroom(seed):
    rng = np.random.default_rng(9700 + seed)
    nl = util.random_cluster(9700 + seed, 150, occupancy=0.2)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(24)]
    m = _matcher()
    got = m.HeadroomMany(nl, tops, per_node=True, max_per_node=2, limits=True)
    plain = _matcher(HeadroomHarnessEngine).HeadroomMany(nl, tops, per_node=True, max_per_node=2)
    lc.check_identities(got, len(nl))
    for a, b in zip(got, plain):
        assert np.array_equal(a.per_node, b.per_node) and np.array_equal(a.flags, b.flags)
        assert a.summary() == b.summary() and repr(a) == repr(b) and a.form == b.form
        assert b.limits is None and b.limit_stages is None
        with pytest.raises(ValueError):
            b.limit_summary()
    # a node without room: the stage ExplainNodes gives the pod on the untouched mirror once nothing is busy
    ex = m.ExplainNodes(nl, tops, now=util.CLOCK + 1.0e6, per_node=True)
    none = 0
    for a, x in zip(got, ex):
        zero = (a.per_node == 0) & (a.flags == 0)
        assert np.array_equal(a.limit_stages[zero], x.stages[zero])
        assert (a.limit_stages[zero] != lc.FITS).all()
        none += int(zero.sum())
    assert none > 500 and sum(h.replicas for h in got) > 100
    assert sum(h.limits["FITS"] for h in got) > 0 and len({s for h in got for s, k in h.limits.items() if k}) >= 6


def test_candidate_mask_and_node_groups():
    rng = np.random.default_rng(9710)
    nl = util.random_cluster(9710, 130, occupancy=0.2)
    names = list(nl)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=3)) for _ in range(12)]
    m = _matcher()
    base = m.HeadroomMany(nl, tops, per_node=True, limits=True)
    all_groups = sorted({g for v in nl.values() for g in v.groups})
    pgroups = [[all_groups[int(rng.integers(len(all_groups)))]] for _ in tops]
    filt = m.HeadroomMany(nl, tops, pod_groups=pgroups, per_node=True, limits=True)
    dropped = 0
    for p, (a, b) in enumerate(zip(base, filt)):
        kept = set(O.initial_node_filter(nl, pgroups[p]))
        inside = np.array([nm in kept for nm in names])
        assert (b.limit_stages[~inside] == lc.NOT_CANDIDATE).all() and (b.per_node[~inside] == 0).all()
        assert np.array_equal(b.limit_stages[inside], a.limit_stages[inside]) and np.array_equal(b.per_node[inside], a.per_node[inside])
        dropped += int((~inside).sum())
    assert dropped > len(nl)
    lc.check_identities(filt, len(nl))
    # a candidate mask, at the engine: exactly the nodes outside it become NOT_CANDIDATE
    reqs = m.packer.digest_many(tops)
    keep = rng.random(len(nl)) < 0.6
    s0, c0, h0, st0 = m.engine.headroom_limits(reqs, per_node=True)
    s1, c1, h1, st1 = m.engine.headroom_limits(reqs, cand=_mask_words(keep), per_node=True)
    assert (st1[:, ~keep] == lc.NOT_CANDIDATE).all() and np.array_equal(st1[:, keep], st0[:, keep])
    assert np.array_equal(c1, np.where(keep[None, :], c0, 0))
    assert np.array_equal(h1, np.stack([(st1 == k).sum(1) for k in range(len(STAGES))], 1))


def test_wide_nodes_and_the_matcher_fields():
    nl = util.mixed_cluster(9500, 120)
    rng = np.random.default_rng(97)
    tops = [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(10)]
    m = _matcher()
    got = m.HeadroomMany(nl, tops, per_node=True, max_per_node=37, limits=True)
    wide = np.array([nm in set(m.wide_nodes) for nm in nl])
    assert 10 < wide.sum() < len(nl) - 10
    lc.check_identities(got, len(nl))
    for h in got:
        assert (h.limit_stages[wide] == pack.LIMIT_NONE).all() and ((h.flags[wide] & pack.HEADROOM_NOT_EVALUATED) != 0).all()
        assert (h.limit_stages[~wide] < len(STAGES)).all() and h.not_evaluated == int(wide.sum())
        assert set(h.limits) == set(STAGES)
    h = max(got, key=lambda x: x.replicas)
    text = h.limit_summary()
    assert text.startswith("further replicas are held back by: ") and " nodes" in text
    top_stage = max((s for s in STAGES[:-1]), key=lambda s: h.limits[s])
    assert text.split(": ", 1)[1].startswith(f"{m_text(top_stage)} on {h.limits[top_stage]} nodes")
    # limits=False: nothing changes, nothing is filled in
    plain = m.HeadroomMany(nl, tops, per_node=True, max_per_node=37)
    assert [x.summary() for x in plain] == [x.summary() for x in got] and all(x.limits is None and x.limit_stages is None for x in plain)
    one = m.Headroom(nl, tops[0], per_node=True, max_per_node=37, limits=True)
    assert one.limits == got[0].limits and np.array_equal(one.limit_stages, got[0].limit_stages)
    assert m.Headroom(nl, tops[0], max_per_node=37, limits=True).limit_stages is None


def m_text(stage):
    from nhd_amd.matcher import _STAGE_TEXT
    return _STAGE_TEXT[stage]


def test_a_template_that_cannot_be_evaluated_and_no_nodes():
    nl = util.random_cluster(9720, 40)
    rng = np.random.default_rng(9720)
    ok = refmodel.make_topology(util.random_pod_spec(rng))
    spec = util.random_pod_spec(rng)
    spec["groups"] = [dict(spec["groups"][0]) for _ in range(6)]           # six processing groups: the general path, no headroom
    big = refmodel.make_topology(spec)
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=TwinEngine, strict=False)
    a, b = m.HeadroomMany(nl, [ok, big], per_node=True, limits=True)
    assert b.error is not None and b.limits == {s: 0 for s in STAGES} and b.limit_stages is None
    assert a.error is None and sum(a.limits.values()) + a.stopped + a.not_evaluated == len(nl)
    assert b.limit_summary() == b.summary()
    empty = m.HeadroomMany({}, [ok], per_node=True, limits=True)[0]
    assert empty.limits == {s: 0 for s in STAGES} and len(empty.limit_stages) == 0


def test_a_subset_of_the_attached_mirror_and_an_unmirrored_node():
    """The host logic of HeadroomMany(limits=True): a node no layout holds is charged to no stage and carries UNMIRRORED per node (the
    device sees its placeholder: NOT_CANDIDATE, taken off the histogram again); with a strict subset of the attached dict the nodes
    outside it are not counted, and the nodes inside it keep the stage they have in the whole cluster."""
    descs = util.random_cluster_desc(9730, 40, occupancy=0.2)
    nl = util.build_cluster(descs)
    names = list(nl)
    odd = refmodel.build_node(dict(descs[3], name=names[3]))
    odd.numa_nodes = odd.sockets = 9                      # beyond both layouts: never mirrored
    nl[names[3]] = odd
    m = _matcher()
    m.attach(nl)
    assert names[3] in m.unmirrored
    rng = np.random.default_rng(9730)
    tops = [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(8)]
    whole = m.HeadroomMany(nl, tops, per_node=True, limits=True)
    lc.check_identities(whole, len(nl))
    for h in whole:
        assert h.unmirrored == 1 and h.limit_stages[3] == UNMIRRORED and h.per_node[3] == 0 and h.flags[3] == 0
        assert sum(h.limits.values()) + h.stopped + h.not_evaluated == len(nl) - 1
        assert h.limits == {s: int((np.delete(h.limit_stages, 3) == k).sum()) for k, s in enumerate(STAGES)}
    for keep in (names[::2], names[1::2]):                # without and with the unmirrored node
        sub = {n: nl[n] for n in keep}
        pos = [names.index(n) for n in keep]
        part = m.HeadroomMany(sub, tops, per_node=True, limits=True)
        for h, w in zip(part, whole):
            assert h.nodes == len(sub) and h.unmirrored == int(names[3] in sub)
            assert np.array_equal(h.limit_stages, w.limit_stages[pos]) and np.array_equal(h.per_node, w.per_node[pos])
            assert sum(h.limits.values()) + h.stopped + h.not_evaluated + h.unmirrored == len(sub)
            seen = h.limit_stages[h.limit_stages != UNMIRRORED] if h.unmirrored else h.limit_stages
            assert h.limits == {s: int((seen == k).sum()) for k, s in enumerate(STAGES)}
    assert sum(h.replicas for h in whole) > 0
