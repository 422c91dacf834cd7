"""nhdfit_candidates_general on the MI355X (`pytest -m gpu`): k_wide_cand_scan / k_wide_cand_map's lists against the reference's
stored answers (tests/golden/refanswers/tests.test_candidates_general_reference.json), against FindNode, the composed form (existing
code) and explain on the same inputs; against the host twin across every 64-slot chunk seam of the wide records, with more blocks than
chunks, without an ordinary node and with K above `feasible`; candidate masks that drop or keep only the wide nodes; a wide node inside
the busy window; the absence of side effects; a call behind steps in flight; shards and the group entry.  Nothing here reads the
reference tree."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import Engine, winner_index
from nhd_amd.matcher import HipMatcher
from oracle import nhd_oracle as O
from tests import candidates_general_check as cg
from tests import candidates_reference as cr
from tests import headroom_general_check as gc
from tests import util
from tests.harness import candidates_twin as ct
from tests.harness.candidates_general_twin import CandidatesGeneralHarnessEngine
from workload import refmodel

WIDE = pack.CANDIDATES_FORM_WIDE


def _device(clock=util.CLOCK):
    return HipMatcher(device=0, clock=lambda: clock)


def _twin(clock=util.CLOCK):
    return HipMatcher(clock=lambda: clock, engine_factory=CandidatesGeneralHarnessEngine)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.error is None and y.error is None
        assert x.entries == y.entries and (x.feasible, x.preferred, x.k, x.nodes) == (y.feasible, y.preferred, y.k, y.nodes)


def _tops(specs):
    return [refmodel.make_topology(s) for s in specs]


def _against_what_exists(descs, specs, sharing, clock, want, pod_groups=None):
    """The device's lists equal `want`; entry 0 is FindNodes'; the whole list is the composed form's (general=False, a second
    matcher); feasible is explain's FITS; at the C entry nothing is left unevaluated and `form` carries the wide bit."""
    m, nl, got, lists, fits = cg.matcher_lists(_device, descs, specs, sharing, clock, pod_groups=pod_groups)
    assert m.unmirrored == {} and lists == want
    cg.consistent(got, lists, fits)
    with gc.sharing_all(sharing):
        found = m.FindNodes(nl, _tops(specs), pod_groups=pod_groups, now=clock)
        composed = _device(clock).CandidatesMany(util.build_cluster(descs), _tops(specs), k=cg.K, pod_groups=pod_groups, now=clock)
        small = [p for p, s in enumerate(specs) if not pack.needs_general_path(refmodel.make_topology(s))]
        reqs = m.packer.digest_many([refmodel.make_topology(specs[p]) for p in small], None if pod_groups is None else [pod_groups[p] for p in small])
        sums, entries = m.engine.candidates(reqs, clock, cg.K, general=True)
    for c, first in zip(got, found):
        assert (c.entries[0] if c.entries else (None,)) == first
    _same(got, composed)
    assert (sums["not_evaluated"] == 0).all() and ((sums["form"] & WIDE) != 0).all()
    assert sums["feasible"].tolist() == [got[p].feasible for p in small] and sums["preferred"].tolist() == [got[p].preferred for p in small]
    assert np.array_equal(sums["returned"], np.minimum(sums["feasible"], cg.K))
    for j in range(len(small)):
        r = int(sums[j]["returned"])
        assert entries[j][r:].tobytes() == bytes(32 * (cg.K - r)) and (entries[j]["reserved"] == 0).all()
    return m, got


# ---- the stored reference answers, FindNode, the composed form, explain --------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gc.CLUSTERS))
def test_cluster_lists_equal_the_reference(name):
    sharing, descs, _ = gc.cluster_case(name)
    m, got = _against_what_exists(descs, cg.templates(), sharing, util.CLOCK, cg.stored(f"test_clusters[{name}]"))
    for (cluster, t), (feasible, preferred) in cg.FACTS.items():
        if cluster == name:
            assert (got[t].feasible, got[t].preferred) == (feasible, preferred)
    assert all(c.form & WIDE for c in got)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture,with_groups", gc.FIXTURE_CASES, ids=[f"{f}-{'groups' if g else 'plain'}" for f, g in gc.FIXTURE_CASES])
def test_fixture_lists_equal_the_reference(fixture, with_groups):
    case, specs, groups, sharing = gc.load_fixture(gc.FIXTURES[gc.FIXTURE_IDS.index(fixture)])
    want = cg.stored(f"test_fixtures[{fixture}-{'groups' if with_groups else 'plain'}]")
    _against_what_exists(case["nodes"], specs, sharing, case["clock"], want, pod_groups=groups if with_groups else None)


# ---- the host twin across the seams -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_plain", [0, 1, 65])
@pytest.mark.parametrize("n_wide", [1, 63, 64, 65, 129])
def test_device_equals_the_twin_across_the_seams(n_wide, n_plain):
    """1, 63, 64, 65 and 129 wide records - every 64-slot chunk boundary; the scan launches a block per chunk - among 0, 1 and 65
    ordinary nodes, K = 1, 2 and 64 (above `feasible` for most pods): every list and every sum equals the twin's."""
    descs = gc.seam_descs(9880, n_wide, n_plain)
    specs = list(gc.FOUR) + [gc.GPULESS]
    listed = 0
    for k in (1, 2, 64):
        md, _, dev, _, fits = cg.matcher_lists(_device, descs, specs, False, util.CLOCK, k=k)
        mt, _, twin, _, _ = cg.matcher_lists(_twin, descs, specs, False, util.CLOCK, k=k)
        assert len(md.wide_nodes) == n_wide and md.wide_nodes == mt.wide_nodes
        _same(dev, twin)
        assert [c.form for c in dev] == [c.form for c in twin] and all(c.form & WIDE for c in dev)
        assert [c.feasible for c in dev] == fits
        listed += sum(len(c.entries) for c in dev)
        if k == 64:
            reqs = md.packer.digest_many(_tops(specs))
            ds, de = md.engine.candidates(reqs, util.CLOCK, k, general=True)
            ts, te = mt.engine.candidates(reqs, util.CLOCK, k, general=True)
            assert ds.tobytes() == ts.tobytes() and de.tobytes() == te.tobytes()
            assert (ds["not_evaluated"] == 0).all() and (ds["feasible"] < k).any()
    assert listed > 0


@pytest.mark.gpu
def test_a_mirror_without_wide_records_is_byte_equal_to_candidates():
    """n_wide == 0: sums (`form` included) and entries are nhdfit_candidates' byte for byte."""
    descs = gc.seam_descs(9880, 0, 70)
    m, _, got, _, _ = cg.matcher_lists(_device, descs, list(gc.FOUR) + [gc.GPULESS], False, util.CLOCK)
    reqs = m.packer.digest_many(_tops(list(gc.FOUR) + [gc.GPULESS]))
    s0, e0 = m.engine.candidates(reqs, util.CLOCK, 8)
    s1, e1 = m.engine.candidates(reqs, util.CLOCK, 8, general=True)
    assert m.engine.n_wide == 0 and s0.tobytes() == s1.tobytes() and e0.tobytes() == e1.tobytes()
    assert not (s1["form"] & WIDE).any() and int(s1["feasible"].sum()) > 20 and not any(c.form & WIDE for c in got)


# ---- candidate masks, the busy window ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_masks_that_drop_every_wide_node_and_keep_only_wide_nodes():
    """A subset `nl` of an attached cluster is the candidate mask: without the wide nodes the list is the ordinary nodes' (the wide
    launch runs and finds no candidate), with them alone the planes' list is empty; either way the twin's and the composed form's."""
    sharing, descs, _ = gc.cluster_case("mixed")
    nl = util.build_cluster(descs)
    specs = cg.templates()
    md, mt, mc = _device(), _twin(), _device()
    for m in (md, mt, mc):
        m.attach(nl)
    wide = set(md.wide_nodes)
    assert 10 < len(wide) < len(nl) - 10 and wide == set(mt.wide_nodes)
    for keep_wide in (False, True):
        sub = {nm: nd for nm, nd in nl.items() if (nm in wide) == keep_wide}
        dev = md.CandidatesMany(sub, _tops(specs), k=8, now=util.CLOCK, general=True)
        _same(dev, mt.CandidatesMany(sub, _tops(specs), k=8, now=util.CLOCK, general=True))
        _same(dev, mc.CandidatesMany(sub, _tops(specs), k=8, now=util.CLOCK))
        assert all((e[0] in wide) == keep_wide for c in dev for e in c.entries) and sum(len(c.entries) for c in dev) > 20
        assert all(c.form & WIDE and c.nodes == len(sub) for c in dev)


@pytest.mark.gpu
def test_a_wide_node_inside_the_busy_window():
    """A wide node stamped three seconds before `now`: it leaves the list of a pod that requests GPUs and stays in the list of one that
    does not - as in FindNode on the same nodes (the independent oracle, iterated)."""
    _, descs, _ = gc.cluster_case("mixed")
    for d in descs:
        d["busy_time"] = util.CLOCK - 500.0
    specs = [gc.FOUR[0], gc.GPULESS]
    m0, nl0, before, lists0, _ = cg.matcher_lists(_device, descs, specs, False, util.CLOCK, k=64)
    wide = set(m0.wide_nodes)
    both = [e[0] for e in lists0[0] if e[0] in wide and e[0] in {x[0] for x in lists0[1]}]
    assert both and before[0].feasible < 64 and before[1].feasible < 64
    victim = both[0]
    next(d for d in descs if d["name"] == victim)["busy_time"] = util.CLOCK - 3.0
    m1, nl1, after, lists1, _ = cg.matcher_lists(_device, descs, specs, False, util.CLOCK, k=64)
    assert [e for e in lists0[0] if e[0] != victim] == lists1[0] and after[0].feasible == before[0].feasible - 1
    assert lists1[1] == lists0[1] and victim in {e[0] for e in lists1[1]}
    for row, s in zip(lists1, specs):
        assert row == cr.iterate(lambda sub, t: O.find_node(sub, t, util.CLOCK), nl1, lambda: refmodel.make_topology(s), k=64)


# ---- no side effects, steps in flight ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
def test_candidates_general_leaves_no_trace(sharing):
    """Headroom(general=True, per_node=True), FindNodes, nhdfit_get_stats, the wide records and the share records are identical before
    and after a call; the call twice gives the same bytes; behind staged steps left in flight it gives them again, and the steps'
    fetched results are what they are without the call in between."""
    descs = util.mixed_cluster_desc(9891, 90, occupancy=0.1)
    specs = list(gc.FOUR) + [gc.GPULESS]
    with gc.sharing_all(sharing):
        nl = util.build_cluster(descs)
        m = _device()
        found = m.FindNodes(nl, _tops(specs), now=util.CLOCK)
        room = m.HeadroomMany(nl, _tops(specs), per_node=True, max_per_node=gc.CAP, general=True)
        eng = m.engine
        reqs = m.packer.digest_many(_tops(specs))
        planes = [np.array(getattr(eng.download(), f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
        wide, share = eng.wide_download().copy(), (eng.wide_share_download().copy() if sharing else None)
        s0, b0, m0 = eng.find(reqs, util.CLOCK, want_bitmap=True, want_map=True)
        st0 = eng.stats()
        sums, entries = eng.candidates(reqs, util.CLOCK, 16, general=True)
        st1 = eng.stats()
        for f in ("launches", "fit_ms_total", "fit_ms_last", "digest_ms_last", "step_ms_last", "evals_last", "bytes_last", "small_finds", "batch_finds",
                  "big_nic_steps_max"):
            assert getattr(st0, f) == getattr(st1, f), f
        for a, b in zip(planes, [np.array(getattr(eng.download(), f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]):
            assert a.tobytes() == b.tobytes()
        assert eng.wide_download().tobytes() == wide.tobytes()
        if sharing:
            assert eng.wide_share_download().tobytes() == share.tobytes()
        again = eng.candidates(reqs, util.CLOCK, 16, general=True)
        assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == entries.tobytes()
        # steps in flight
        eng.stage(reqs)
        for _ in range(3):
            eng.enqueue(util.CLOCK)
        s_in, e_in = eng.candidates(reqs, util.CLOCK, 16, general=True)
        f1 = eng.fetch(want_bitmap=True, want_map=True)
        assert s_in.tobytes() == sums.tobytes() and e_in.tobytes() == entries.tobytes()
        assert np.array_equal(f1[0], s0) and np.array_equal(f1[1], b0) and f1[2].tobytes() == m0.tobytes()
        assert m.FindNodes(nl, _tops(specs), now=util.CLOCK) == found
        after = m.HeadroomMany(nl, _tops(specs), per_node=True, max_per_node=gc.CAP, general=True)
    for a, b in zip(room, after):
        assert np.array_equal(a.per_node, b.per_node) and np.array_equal(a.flags, b.flags) and a.replicas == b.replicas
    assert int(sums["returned"].sum()) > 20 and ((sums["form"] & WIDE) != 0).all() and len(wide) > 10
    assert any(r[0] is not None for r in found)


@pytest.mark.gpu
def test_k_outside_1_to_64_is_refused():
    _, descs, _ = gc.cluster_case("mixed")
    m, _, _, _, _ = cg.matcher_lists(_device, descs, [gc.GPULESS], False, util.CLOCK)
    reqs = m.packer.digest_many(_tops([gc.GPULESS]))
    from nhd_amd._lib import NhdFitError
    for k in (0, 65):
        with pytest.raises(NhdFitError):
            m.engine.candidates(reqs, util.CLOCK, k, general=True)
    assert int(m.engine.candidates(reqs, util.CLOCK, 64, general=True)[0]["returned"][0]) == 61


# ---- shards and the group entry -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_shards_and_the_group_entry_equal_one_device():
    """Three shards on one GPU == one device.  A group of three contexts on ONE device cannot be created (its communicator wants
    distinct devices), so the pieces are held one by one: three device contexts as shards, each with its own wide records and global
    base, under sharding.merge_candidates (GroupEngine over Engine) and under the text the group entry merges with
    (candidates_merge.h, as the host twin exports it); and the group entry itself, nhdfit_group_candidates_general with one shard
    (HipMatcher(devices=[0])), against HipMatcher(device=0)."""
    nl = util.mixed_cluster(9883, 330, occupancy=0.1)           # (wide nodes all along the node axis: in every shard)
    specs = list(gc.FOUR) + [gc.GPULESS, gc.NOTHING]
    one = _device()
    three = HipMatcher(devices=[0, 0, 0], engine_factory=Engine, clock=lambda: util.CLOCK)
    grp1 = HipMatcher(devices=[0], clock=lambda: util.CLOCK)
    crossing = 0
    for k in (2, 8, 64):
        a = one.CandidatesMany(nl, _tops(specs), k=k, now=util.CLOCK, general=True)
        for other in (three, grp1):
            b = other.CandidatesMany(nl, _tops(specs), k=k, now=util.CLOCK, general=True)
            _same(a, b)
            assert [c.form for c in a] == [c.form for c in b]
        reqs = one.packer.digest_many(_tops(specs))
        s1, e1 = one.engine.candidates(reqs, util.CLOCK, k, general=True)
        parts = [sh.candidates(reqs, util.CLOCK, k, general=True) for sh in three.engine.shards]
        sm, em, owner = ct.merge(parts, k)
        assert sm.tobytes() == s1.tobytes() and em.tobytes() == e1.tobytes()
        for p in range(len(reqs)):
            got = int(s1[p]["returned"])
            assert owner[p, :got].tolist() == [three.engine._shard_of(winner_index(s)) for s in e1[p]["score"][:got].tolist()]
            crossing += len(set(owner[p, :got].tolist())) > 1
    assert len(three.engine.shards) == 3 and all(s.n_wide > 0 for s in three.engine.shards)
    assert crossing > 0 and (s1["not_evaluated"] == 0).all() and ((s1["form"] & WIDE) != 0).all() and sum(len(c.entries) for c in a) > 100
