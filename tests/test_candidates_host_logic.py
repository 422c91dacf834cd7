"""HipMatcher.Candidates / CandidatesMany on the host twin (tests/harness/candidates_twin.py), without a GPU: entries[0] is FindNode's
answer; the composed path (wide mirrors, pods of the general path, ENABLE_SHARING) equals FindNodes iterated on a dict that loses
each answer; `error` and `strict`; an empty `nl`; attached and stateless mirrors; and the merge of three shards - sharding.merge_candidates,
and the group entry's own text (nhd_amd/csrc/candidates_merge.h) - equals the unsharded answer."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import Candidates, HipMatcher
from nhd_amd.sharding import merge_candidates, shard_bounds
from oracle import nhd_oracle as O
from tests import candidates_reference as cr
from tests import util
from tests.harness import candidates_twin as ct
from tests.test_big_core import big_spec
from workload import planes, refmodel, synth


def _twin(clock=util.CLOCK, **kw):
    return HipMatcher(clock=lambda: clock, engine_factory=ct.CandidatesHarnessEngine, **kw)


def iterated(nl, top, k, groups=None):
    """FindNodes of a fresh matcher on a dict that loses each answer."""
    m = _twin()
    return cr.iterate(lambda sub, t: m.FindNodes(sub, [t], pod_groups=None if groups is None else [groups], now=util.CLOCK)[0], nl, lambda: top, k=k)


@pytest.mark.parametrize("attached", [False, True], ids=["stateless", "attached"])
def test_first_entry_is_find_node_and_the_list_is_the_iterated_find(attached):
    rng = np.random.default_rng(1410)
    nl = util.random_cluster(1410, 90, occupancy=0.2)
    tops = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(24)]
    m = _twin()
    if attached:
        m.attach(nl)
    got = m.CandidatesMany(nl, tops, k=5, now=util.CLOCK)
    found = m.FindNodes(nl, tops, now=util.CLOCK)
    placed = 0
    for c, top, first in zip(got, tops, found):
        assert isinstance(c, Candidates) and c.error is None and c.k == 5 and c.nodes == len(nl)
        assert (c.entries[0] if c.entries else (None,)) == first
        assert [cr.entry(e) for e in c.entries] == iterated(nl, top, 5)
        assert len(c.entries) == min(5, c.feasible) and c.feasible == m.ExplainNode(nl, top, now=util.CLOCK).counts["FITS"]
        assert m.Candidates(nl, top, k=5, now=util.CLOCK).entries == c.entries
        for name, mp in c.entries:                           # the independent oracle on that node alone
            assert cr.entry(O.find_node({name: nl[name]}, top, util.CLOCK)) == cr.entry((name, mp))
        assert (c.summary().startswith(f"first {len(c.entries)} of {c.feasible} feasible")) if c.entries else c.summary().startswith("no feasible node")
        placed += bool(c.entries)
    assert placed >= 8
    sub = {nm: nl[nm] for j, nm in enumerate(nl) if j % 3}      # a filtered dict: the candidate mask
    for c, top in zip(m.CandidatesMany(sub, tops[:8], k=64, now=util.CLOCK), tops):
        assert [cr.entry(e) for e in c.entries] == iterated(sub, top, 64) and c.nodes == len(sub)


def test_node_groups_and_the_preferred_count():
    spec = synth.make_cluster(3, n_nodes=60)
    nl = spec.build_nodes()
    specs, groups = synth.make_pods(3, n_pods=48)
    tops = [refmodel.make_topology(s) for s in specs]
    m = HipMatcher(clock=lambda: spec.clock_now, engine_factory=ct.CandidatesHarnessEngine)
    got = m.CandidatesMany(nl, tops, k=64, pod_groups=groups)
    seen_pref = 0
    for c, s, top, g in zip(got, specs, tops, groups):
        kept = O.initial_node_filter(nl, g)
        want = cr.iterate(lambda sub, t: O.find_node(sub, t, spec.clock_now), kept, lambda: top, k=64)
        assert [cr.entry(e) for e in c.entries] == want
        cpu_only = not any(gr["gpus"] for gr in s["groups"])
        first_gpu = next((j for j, e in enumerate(c.entries) if len(nl[e[0]].gpus) > 0), len(c.entries))
        if cpu_only and c.feasible <= 64:
            assert c.preferred == first_gpu and all(len(nl[e[0]].gpus) > 0 for e in c.entries[first_gpu:])
            seen_pref += 0 < c.preferred < c.feasible
        elif not cpu_only:
            assert c.preferred == 0
    assert seen_pref > 0


@pytest.fixture
def sharing(monkeypatch):
    monkeypatch.setattr(refmodel, "ENABLE_SHARING", True)
    monkeypatch.setattr(O, "ENABLE_SHARING", True)


def _composed_equals_iterated(nl, tops, k=4):
    m = _twin()
    got = m.CandidatesMany(nl, tops, k=k, now=util.CLOCK)
    listed = 0
    for c, top in zip(got, tops):
        assert c.error is None
        assert [cr.entry(e) for e in c.entries] == iterated(nl, top, k)
        assert c.feasible == _twin().ExplainNode(nl, top, now=util.CLOCK).counts["FITS"] and len(c.entries) == min(k, c.feasible)
        cpu_only = not any(len(g.group_gpus) > 0 for g in top.proc_groups)
        assert c.preferred == (sum(1 for e in iterated(nl, top, len(nl)) if len(nl[e[0]].gpus) == 0) if cpu_only else 0)
        listed += len(c.entries)
    return m, listed


def test_composed_on_a_wide_mirror_and_for_a_big_pod():
    rng = np.random.default_rng(1420)
    nl = util.mixed_cluster(1420, 60)
    tops = [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(8)]
    m, listed = _composed_equals_iterated(nl, tops)
    assert 5 < len(pack.Packer().pack_nodes(nl).wide) < len(nl) - 5 and listed > 8
    # pods of the general path on an ordinary cluster, beside ordinary pods of the same call (those take the device entry)
    nl = util.random_cluster(1421, 60, occupancy=0.1)
    tops = [refmodel.make_topology(big_spec(rng)) for _ in range(4)] + [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(4)]
    assert [pack.needs_general_path(t) for t in tops] == [True] * 4 + [False] * 4
    m, listed = _composed_equals_iterated(nl, tops)
    assert listed > 8 and not m._table.wide


def test_composed_under_enable_sharing(sharing):
    rng = np.random.default_rng(1430)
    descs = util.random_cluster_desc(1430, 16, occupancy=0.1)
    for d in descs:
        d["nic_speed_used"] = [[float(rng.choice([0, 10, 22.5])), float(rng.choice([0, 5, 15]))] for _ in d["nic_pods_used"]]
    nl = util.build_cluster(descs)
    tops = []
    while len(tops) < 8:
        s = util.random_pod_spec(rng, max_groups=3)
        if s["map_type"] != "NONE":
            s["misc_smt"] = True
            tops.append(refmodel.make_topology(s))
    m, listed = _composed_equals_iterated(nl, tops)
    assert m.packer.sharing and listed > 8


def test_errors_strict_and_an_empty_dict(caplog):
    rng = np.random.default_rng(1440)
    nl = util.random_cluster(1440, 30, occupancy=0.1)
    ok = refmodel.make_topology(util.random_pod_spec(rng))
    none = refmodel.make_topology(dict(util.random_pod_spec(rng), groups=[]))
    beyond = refmodel.make_topology(big_spec(rng, 9, 9))    # more groups than the big record holds
    m = _twin()
    got = m.CandidatesMany(nl, [ok, none, beyond], k=3, now=util.CLOCK)
    assert got[0].error is None and [cr.entry(e) for e in got[0].entries] == iterated(nl, ok, 3)
    for c in got[1:]:
        assert c.error is not None and c.entries == [] and c.feasible == 0 and "not evaluated" in c.summary()
    for bad in (none, beyond):
        with pytest.raises(pack.UnsupportedNode):
            m.CandidatesMany(nl, [ok, bad], k=3, now=util.CLOCK, strict=True)
        with pytest.raises(pack.UnsupportedNode):
            _twin(strict=True).Candidates(nl, bad, k=3, now=util.CLOCK)
    for k in (0, 65):
        with pytest.raises(ValueError):
            m.Candidates(nl, ok, k=k)
    assert m.CandidatesMany(nl, [], k=3) == []
    empty = m.CandidatesMany({}, [ok, ok], k=3)
    assert [(c.entries, c.feasible, c.error) for c in empty] == [([], 0, None)] * 2


def test_a_device_error_comes_back_as_error_or_raises():
    from nhd_amd._lib import NhdFitError

    class Failing(ct.CandidatesHarnessEngine):
        def candidates(self, reqs, now, k, cand=None):
            raise NhdFitError(-6, "the dictionary has too many NIC signatures")

    rng = np.random.default_rng(1441)
    nl = util.random_cluster(1441, 20, occupancy=0.1)
    top = refmodel.make_topology(util.random_pod_spec(rng))
    c = HipMatcher(clock=lambda: util.CLOCK, engine_factory=Failing).Candidates(nl, top, k=3)
    assert c.entries == [] and "too many NIC signatures" in c.error
    with pytest.raises(NhdFitError):
        HipMatcher(clock=lambda: util.CLOCK, engine_factory=Failing, strict=True).Candidates(nl, top, k=3)


@pytest.mark.parametrize("k", [1, 8, 64])
def test_three_shards_merge_to_the_unsharded_answer(k):
    """Three twin shards of a 450-node cluster (each with its global base): sharding.merge_candidates and the group entry's merge
    header both give the unsharded twin's records, byte for byte, with each entry's owner; GroupEngine over twins gives the same."""
    cfg, n = 4, 450
    spec = synth.make_cluster(cfg, n_nodes=n)
    specs, _ = synth.make_pods(cfg, n_pods=24)
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many([refmodel.make_topology(s) for s in specs])
    keep = np.random.default_rng(1450).random(n) < 0.6
    bits = np.zeros(((n + 63) // 64) * 64, bool)
    bits[:n] = keep
    mask = np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))
    for cand in (None, mask):
        whole = ct.candidates(pk, table, [], reqs, spec.clock_now, k, cand=cand)
        bounds = [shard_bounds(n, 3, r) for r in range(3)]
        parts = [ct.candidates(pk, table.slice(lo, hi), [], reqs, spec.clock_now, k, cand=None if cand is None else cand[lo // 64:(hi + 63) // 64],
                               global_base=lo) for lo, hi in bounds]
        for sums, entries, owner in (merge_candidates([p[0] for p in parts], [p[1] for p in parts], k), ct.merge(parts, k)):
            assert sums.tobytes() == whole[0].tobytes() and entries.tobytes() == whole[1].tobytes()
            for p in range(len(reqs)):
                got = int(sums[p]["returned"])
                idx = [0x7FFFFFFFFFFFFFFF - (int(s) & 0x7FFFFFFFFFFFFFFF) for s in entries[p]["score"][:got]]
                assert owner[p, :got].tolist() == [next(r for r, (lo, hi) in enumerate(bounds) if lo <= i < hi) for i in idx]
                assert (owner[p, got:] == -1).all()
        assert (whole[0]["feasible"] > k).any() and (whole[0]["returned"] > 0).all()
    from nhd_amd.engine import GroupEngine
    grp = GroupEngine([0, 1, 2], engine_factory=ct.CandidatesHarnessEngine)
    grp.set_dictionary(pk)
    grp.upload(table)
    sums, entries = grp.candidates(reqs, spec.clock_now, k, cand=mask)
    assert sums.tobytes() == whole[0].tobytes() and entries.tobytes() == whole[1].tobytes()
