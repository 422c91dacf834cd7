"""nhdfit_candidates_big on the MI355X (`pytest -m gpu`): k_big_cand_scan / _pick / _map's lists against the reference's stored answers
(tests/golden/refanswers/tests.test_candidates_big_reference.json), against nhdfit_big_find, K successive nhdfit_big_find calls with a
shrinking mask and nhdfit_explain_big on the same inputs; against the host twin across every 64-unit chunk seam of both ranges;
candidate masks; the absence of side effects; a call behind steps in flight; shards and the group entry.  Nothing here reads the
reference tree.

Not here: P in two slabs (the entry takes at most 65 535 pods in one launch and refuses more); the search budget running out (driven on
the twin, tests/test_candidates_big_host_logic.py).  Pods of eight groups on nodes of three or four sockets are the fixtures' own
(big_quad, big_tri), at K <= 4 there."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd._lib import NhdFitError
from nhd_amd.engine import Engine, winner_index
from nhd_amd.matcher import STAGES, HipMatcher
from tests import candidates_big_check as cb
from tests import headroom_general_check as gc
from tests import util
from tests.harness import candidates_big_twin as bt
from tests.test_candidates_big_core import seam_specs, shrinking_finds
from workload import refmodel

BIG = pack.CANDIDATES_FORM_BIG
FITS = STAGES.index("FITS")


def _device(clock=util.CLOCK):
    return HipMatcher(device=0, clock=lambda: clock)


def _twin(clock=util.CLOCK):
    return HipMatcher(clock=lambda: clock, engine_factory=bt.CandidatesBigHarnessEngine)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.error is None and y.error is None
        assert x.entries == y.entries and (x.feasible, x.preferred, x.k, x.nodes, x.form) == (y.feasible, y.preferred, y.k, y.nodes, y.form)


def _tops(specs):
    return [refmodel.make_topology(s) for s in specs]


def _against_what_exists(descs, specs, sharing, clock, want, k=cb.K, unmasked_find=True, pod_groups=None):
    """The device's lists equal `want` (the reference's, cut at k); at the C entry: out[p][0] is nhdfit_big_find's score word and
    mapping bytes, the list is k successive nhdfit_big_find calls with a shrinking mask, feasible is nhdfit_explain_big's FITS,
    nothing is left unevaluated, entries past `returned` are zero."""
    m, nl, got, lists, fits = cb.matcher_lists(_device, descs, specs, sharing, clock, k=k, pod_groups=pod_groups)
    assert m.unmirrored == {} and lists == [row[:k] for row in want]
    cb.consistent(got, lists, fits, k=k)
    with gc.sharing_all(sharing):
        reqs = np.array([m.packer.digest_big(t, None if pod_groups is None else pod_groups[p]) for p, t in enumerate(_tops(specs))],
                        dtype=pack.BIG_REQ)
        sums, entries = m.engine.candidates_big(reqs, clock, k)
        counts, _ = m.engine.explain(reqs, clock)
        if unmasked_find:                                  # nhdfit_big_find without a mask, all pods in one call
            score, maps = m.engine.big_find(reqs, clock)
            for p in range(len(reqs)):
                first = entries[p][0]
                assert int(first["score"]) == int(score[p]) and (not score[p] or first["map"].tobytes() == maps[p].tobytes())
        for p in range(len(reqs)):
            r = int(sums[p]["returned"])
            assert r == min(k, int(sums[p]["feasible"])) == len(lists[p])
            # (the first of the successive finds is nhdfit_big_find on the whole mask: out[p][0] is its score word and mapping bytes)
            assert [(int(e["score"]), e["map"].tobytes()) for e in entries[p][:r]] == shrinking_finds(m.engine, reqs[p], clock, k)
            assert entries[p][r:].tobytes() == bytes(48 * (k - r)) and (entries[p]["reserved"] == 0).all()
    assert sums["feasible"].tolist() == counts[:, FITS].tolist() == [c.feasible for c in got]
    assert sums["preferred"].tolist() == [c.preferred for c in got]
    assert (sums["not_evaluated"] == 0).all() and (sums["form"] == BIG).all()
    return m, got


# ---- the stored reference answers, nhdfit_big_find, successive finds, explain ----------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gc.CLUSTERS))
def test_cluster_lists_equal_the_reference(name):
    sharing, descs, _ = gc.cluster_case(name)
    _, got = _against_what_exists(descs, cb.cluster_specs(name), sharing, util.CLOCK, cb.stored(f"test_clusters[{name}]"))
    assert sum(len(c.entries) >= 2 for c in got) >= 2


@pytest.mark.gpu
@pytest.mark.parametrize("name", cb.GROUPED)
def test_cluster_lists_with_node_groups_equal_the_reference(name):
    """`pod_groups` given: the request records carry the groups and the kernels apply InitialNodeFilter themselves; the reference
    was handed the filtered dict."""
    sharing, descs, _ = gc.cluster_case(name)
    groups = cb.cluster_groups(name)
    _, got = _against_what_exists(descs, cb.cluster_specs(name), sharing, util.CLOCK, cb.stored(f"test_clusters_with_node_groups[{name}]"),
                                  pod_groups=groups)
    keep = cb.cluster_keep(descs, groups)
    assert all(e[0] in kp for c, kp in zip(got, keep) for e in c.entries) and any(len(c.entries) >= 2 for c in got)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", cb.FIXTURE_IDS)
def test_fixture_lists_equal_the_reference(fixture):
    """big_quad and big_tri - pods of up to eight groups on nodes of three and four sockets, the mappings nhdfit_big_find already
    makes there in the existing suite - at K = 2 and 3 (a one-thread mapping of seven or eight groups on four sockets takes a good part
    of a second); the others at the stored K = 8."""
    case, idx, specs = cb.load_fixture(cb.FIXTURES[cb.FIXTURE_IDS.index(fixture)])
    k = {"big_quad": 2, "big_tri": 3}.get(fixture, cb.K)
    _against_what_exists(case["nodes"], specs, False, case["clock"], cb.stored(f"test_fixtures[{fixture}]"), k=k,
                         unmasked_find=k == cb.K)


# ---- the host twin across the seams ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_wide", [0, 1, 65])
@pytest.mark.parametrize("n_plain", [1, 63, 64, 65, 129])
def test_device_equals_the_twin_across_the_seams(n_plain, n_wide):
    """1, 63, 64, 65 and 129 ordinary nodes among 0, 1 and 65 wide records - every 64-unit chunk boundary of either range; the scan
    launches a block per chunk - at K = 1, 2 and 64 (above `feasible` for most pods): sums and entries are the twin's bytes."""
    descs = gc.seam_descs(9880, n_wide, n_plain)
    nl = util.build_cluster(descs)
    specs = seam_specs()
    md, mt = _device(), _twin()
    md.attach(nl)
    mt.attach(nl)
    assert len(md.wide_nodes) == n_wide and md.wide_nodes == mt.wide_nodes
    reqs = np.array([md.packer.digest_big(t) for t in _tops(specs)], dtype=pack.BIG_REQ)
    listed = 0
    for k in (1, 2, 64):
        ds, de = md.engine.candidates_big(reqs, util.CLOCK, k)
        ts, te = mt.engine.candidates_big(reqs, util.CLOCK, k)
        assert ds.tobytes() == ts.tobytes() and de.tobytes() == te.tobytes()
        _same(md.CandidatesMany(nl, _tops(specs), k=k, now=util.CLOCK, big=True), mt.CandidatesMany(nl, _tops(specs), k=k, now=util.CLOCK, big=True))
        listed += int(ds["returned"].sum())
    assert listed > 0 or n_plain + n_wide < 3


@pytest.mark.gpu
@pytest.mark.parametrize("pods", [600, 1200])
def test_blocks_that_sweep_several_chunks(pods):
    """Enough pods in one call that a pod's share of the chip's block slots is smaller than its chunk counts - 600 pods: two blocks per
    range, 1 200: one - on 129 ordinary nodes (three chunks) and 65 wide records (two): a scan block sweeps two or three chunks and
    carries its counts and firsts across them (125 feasible nodes for the first pod, K = 64 cuts its list).  The first three pods are
    the seam pods, the others ask for more hugepages than any node has (nothing to map: the call stays short); every pod's sums and
    entries are the twin's bytes."""
    descs = gc.seam_descs(9880, 65, 129)
    nl = util.build_cluster(descs)
    md, mt = _device(), _twin()
    md.attach(nl)
    mt.attach(nl)
    assert md.engine.n == 194 and md.engine.n_wide == 65
    four = np.array([md.packer.digest_big(t) for t in _tops(seam_specs() + seam_specs()[:1])], dtype=pack.BIG_REQ)
    four["hugepages_gb"][3] = 1 << 20
    reqs = np.concatenate([four[:3], np.repeat(four[3:], pods - 3)])
    for k in (2, 64):
        ts, te = mt.engine.candidates_big(four, util.CLOCK, k)
        ds, de = md.engine.candidates_big(reqs, util.CLOCK, k)
        assert ds[:3].tobytes() == ts[:3].tobytes() and de[:3].tobytes() == te[:3].tobytes()
        assert ds[3:].tobytes() == np.repeat(ts[3:], pods - 3).tobytes() and not de[3:].tobytes().strip(b"\0")
        assert int(ts["feasible"][0]) > 64 and int(ts["returned"][:3].sum()) > 3 and int(ts["feasible"][3]) == 0


@pytest.mark.gpu
def test_masks_only_wide_only_ordinary_and_none():
    """A subset `nl` of an attached cluster is the candidate mask: the wide nodes alone, the ordinary nodes alone, and at the C entry a
    mask without a node - the twin's answers."""
    _, descs, _ = gc.cluster_case("mixed")
    nl = util.build_cluster(descs)
    specs = seam_specs()
    md, mt = _device(), _twin()
    md.attach(nl)
    mt.attach(nl)
    wide = set(md.wide_nodes)
    assert 10 < len(wide) < len(nl) - 10 and wide == set(mt.wide_nodes)
    for keep_wide in (False, True):
        sub = {nm: nd for nm, nd in nl.items() if (nm in wide) == keep_wide}
        dev = md.CandidatesMany(sub, _tops(specs), k=8, now=util.CLOCK, big=True)
        _same(dev, mt.CandidatesMany(sub, _tops(specs), k=8, now=util.CLOCK, big=True))
        assert all((e[0] in wide) == keep_wide for c in dev for e in c.entries) and sum(len(c.entries) for c in dev) > 3
    reqs = np.array([md.packer.digest_big(t) for t in _tops(specs)], dtype=pack.BIG_REQ)
    sums, entries = md.engine.candidates_big(reqs, util.CLOCK, 8, cand=np.zeros((md.engine.n + 63) // 64, np.uint64))
    assert not sums["feasible"].any() and not sums["returned"].any() and entries.tobytes() == bytes(entries.nbytes) and (sums["form"] == BIG).all()


# ---- no side effects, steps in flight --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
def test_candidates_big_leaves_no_trace(sharing):
    """FindNodes, nhdfit_get_stats (big_nic_steps_max among them), the planes, the wide records and the share records are identical
    before and after a call; the call twice gives the same bytes; behind staged steps left in flight it gives them again, and the
    steps' fetched results are what they are without the call in between."""
    descs = util.mixed_cluster_desc(9891, 90, occupancy=0.1)
    specs = seam_specs()
    small = [gc.FOUR[0], gc.GPULESS]
    with gc.sharing_all(sharing):
        nl = util.build_cluster(descs)
        m = _device()
        found = m.FindNodes(nl, _tops(specs) + _tops(small), now=util.CLOCK)
        eng = m.engine
        reqs = np.array([m.packer.digest_big(t) for t in _tops(specs)], dtype=pack.BIG_REQ)
        small_reqs = m.packer.digest_many(_tops(small))
        planes = [np.array(getattr(eng.download(), f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
        wide, share = eng.wide_download().copy(), (eng.wide_share_download().copy() if sharing else None)
        s0, b0, m0 = eng.find(small_reqs, util.CLOCK, want_bitmap=True, want_map=True)
        st0 = eng.stats()
        sums, entries = eng.candidates_big(reqs, util.CLOCK, 16)
        st1 = eng.stats()
        for f in ("launches", "fit_ms_total", "fit_ms_last", "digest_ms_last", "step_ms_last", "evals_last", "bytes_last", "small_finds", "batch_finds",
                  "big_nic_steps_max"):
            assert getattr(st0, f) == getattr(st1, f), f
        for a, b in zip(planes, [np.array(getattr(eng.download(), f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]):
            assert a.tobytes() == b.tobytes()
        assert eng.wide_download().tobytes() == wide.tobytes()
        if sharing:
            assert eng.wide_share_download().tobytes() == share.tobytes()
        again = eng.candidates_big(reqs, util.CLOCK, 16)
        assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == entries.tobytes()
        # steps in flight
        eng.stage(small_reqs)
        for _ in range(3):
            eng.enqueue(util.CLOCK)
        s_in, e_in = eng.candidates_big(reqs, util.CLOCK, 16)
        f1 = eng.fetch(want_bitmap=True, want_map=True)
        assert s_in.tobytes() == sums.tobytes() and e_in.tobytes() == entries.tobytes()
        assert np.array_equal(f1[0], s0) and np.array_equal(f1[1], b0) and f1[2].tobytes() == m0.tobytes()
        assert m.FindNodes(nl, _tops(specs) + _tops(small), now=util.CLOCK) == found
    assert int(sums["returned"].sum()) > 10 and (sums["form"] == BIG).all() and len(wide) > 10
    assert any(r[0] is not None for r in found)


@pytest.mark.gpu
def test_k_and_p_out_of_range_are_refused():
    _, descs, _ = gc.cluster_case("mixed")
    m = _device()
    m.attach(util.build_cluster(descs))
    reqs = np.array([m.packer.digest_big(t) for t in _tops(seam_specs()[:1])], dtype=pack.BIG_REQ)
    for k in (0, 65):
        with pytest.raises(NhdFitError):
            m.engine.candidates_big(reqs, util.CLOCK, k)
    with pytest.raises(NhdFitError):
        m.engine.candidates_big(np.repeat(reqs, 65536), util.CLOCK, 1)
    sums, _ = m.engine.candidates_big(reqs, util.CLOCK, 64)
    assert int(sums[0]["returned"]) == min(64, int(sums[0]["feasible"])) > 8


# ---- shards and the group entry --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_shards_and_the_group_entry_equal_one_device():
    """Three shards on one GPU == one device.  A group of three contexts on ONE device cannot be created (its communicator wants
    distinct devices), so the pieces are held one by one: three device contexts as shards, each with its own wide records and global
    base, under sharding.merge_candidates (GroupEngine over Engine) and under the text the group entry merges with
    (candidates_merge.h, as the host twin exports it for the big entry); and the group entry itself, nhdfit_group_candidates_big with
    one shard (HipMatcher(devices=[0])), against HipMatcher(device=0)."""
    nl = util.mixed_cluster(9883, 330, occupancy=0.1)           # (wide nodes all along the node axis: in every shard)
    specs = seam_specs()
    one = _device()
    three = HipMatcher(devices=[0, 0, 0], engine_factory=Engine, clock=lambda: util.CLOCK)
    grp1 = HipMatcher(devices=[0], clock=lambda: util.CLOCK)
    crossing = 0
    for k in (2, 8, 64):
        a = one.CandidatesMany(nl, _tops(specs), k=k, now=util.CLOCK, big=True)
        for other in (three, grp1):
            _same(a, other.CandidatesMany(nl, _tops(specs), k=k, now=util.CLOCK, big=True))
        reqs = np.array([one.packer.digest_big(t) for t in _tops(specs)], dtype=pack.BIG_REQ)
        s1, e1 = one.engine.candidates_big(reqs, util.CLOCK, k)
        parts = [sh.candidates_big(reqs, util.CLOCK, k) for sh in three.engine.shards]
        sm, em, owner = bt.merge(parts, k)
        assert sm.tobytes() == s1.tobytes() and em.tobytes() == e1.tobytes()
        for p in range(len(reqs)):
            got = int(s1[p]["returned"])
            assert owner[p, :got].tolist() == [three.engine._shard_of(winner_index(s)) for s in e1[p]["score"][:got].tolist()]
            crossing += len(set(owner[p, :got].tolist())) > 1
    assert len(three.engine.shards) == 3 and all(s.n_wide > 0 for s in three.engine.shards)
    assert crossing > 0 and (s1["not_evaluated"] == 0).all() and (s1["form"] == BIG).all() and sum(len(c.entries) for c in a) > 50
