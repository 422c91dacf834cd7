"""nhdfit_candidates_big's host twin against the code that exists, on the CPU: entry 0 is FindNodes' answer, the list is the composed
form's (HipMatcher._candidates_composed on a second matcher) and successive big_find calls with a shrinking candidate mask (the
composed form at the C-ABI), `feasible` is ExplainNodes' FITS - across every 64-unit chunk seam of both ranges, under masks, with a
node inside the busy window; and the kernel's own record logic and two-range pick (big_candidates_kernel.h, cut out of the header and
run on emulated lanes) against a scalar statement of the selection order."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import winner_index
from nhd_amd.matcher import HipMatcher
from tests import candidates_big_check as cb
from tests import candidates_reference as cr
from tests import headroom_general_check as gc
from tests import util
from tests.harness import candidates_big_twin as bt
from workload import refmodel


def _twin(clock=util.CLOCK):
    return HipMatcher(clock=lambda: clock, engine_factory=bt.CandidatesBigHarnessEngine)


def _group(**kw):
    return dict(dict(proc=2, helpers=0, rx=5.0, tx=0.0, proc_smt=True, helper_smt=False, gpus=[]), **kw)


def seam_specs():
    """Three pods of five and six groups, light enough for a fair share of the test clusters' nodes: [0] requests no GPU (preferred
    nodes exist for it), [1] requests two GPUs, [2] one, mapped by PCI."""
    return [dict(map_type="NUMA", hugepages_gb=0, misc=1, misc_smt=True, groups=[_group() for _ in range(5)]),
            dict(map_type="NUMA", hugepages_gb=1, misc=2, misc_smt=True,
                 groups=[_group(proc=3, rx=10.0, tx=10.0) for _ in range(3)] + [_group(gpus=[0]), _group(gpus=[1]), _group()]),
            dict(map_type="PCI", hugepages_gb=0, misc=0, misc_smt=True,
                 groups=[_group(rx=0.0, tx=5.0, proc_smt=False) for _ in range(4)] + [_group(gpus=[1])])]


def shrinking_finds(engine, req, now, k, cand=None):
    """The composed form at the C-ABI: k successive big_find calls, each without the nodes already answered.
    [(score, mapping bytes)]"""
    n = engine.n
    mask = np.full((n + 63) // 64, ~np.uint64(0), np.uint64) if cand is None else np.array(cand, np.uint64)
    out = []
    for _ in range(k):
        score, maps = engine.big_find(np.asarray(req).reshape(1), now, cand=mask)
        if not score[0]:
            break
        out.append((int(score[0]), maps[0].tobytes()))
        v = winner_index(int(score[0])) - engine.global_base
        mask[v >> 6] &= ~(np.uint64(1) << np.uint64(v & 63))
    return out


def check_against_what_exists(make, descs, specs, ks=(1, 2, 64), composed_k=2):
    """`make()` answers with the entry under test.  For every k: list and sums against successive finds on the same mirror, FITS
    and FindNodes; up to composed_k entries against the composed form on a second twin matcher.  Returns the entries listed."""
    nl = util.build_cluster(descs)
    tops = lambda: [refmodel.make_topology(s) for s in specs]      # noqa: E731
    m = make()
    found = m.FindNodes(nl, tops(), now=util.CLOCK)
    fits = [e.counts.get("FITS", 0) for e in m.ExplainNodes(nl, tops(), now=util.CLOCK)]
    composed = _twin().CandidatesMany(nl, tops(), k=composed_k, now=util.CLOCK)
    reqs = np.array([m.packer.digest_big(t) for t in tops()], dtype=pack.BIG_REQ)
    listed = 0
    for k in ks:
        got = m.CandidatesMany(nl, tops(), k=k, now=util.CLOCK, big=True)
        sums, entries = m.engine.candidates_big(reqs, util.CLOCK, k)
        for p, c in enumerate(got):
            assert c.error is None and c.form == pack.CANDIDATES_FORM_BIG and c.feasible == fits[p]
            assert (c.entries[0] if c.entries else (None,)) == found[p]
            assert c.entries[:composed_k] == composed[p].entries[:k] and (c.feasible, c.preferred) == (composed[p].feasible, composed[p].preferred)
            want = shrinking_finds(m.engine, reqs[p], util.CLOCK, k)
            r = int(sums[p]["returned"])
            assert r == len(want) == min(k, fits[p]) == len(c.entries)
            assert [(int(e["score"]), e["map"].tobytes()) for e in entries[p][:r]] == want
            assert entries[p][r:].tobytes() == bytes(48 * (k - r)) and (entries[p]["reserved"] == 0).all()
            listed += r
        assert (sums["not_evaluated"] == 0).all() and (sums["form"] == pack.CANDIDATES_FORM_BIG).all()
    return listed


@pytest.mark.parametrize("n_wide", [0, 1, 65])
@pytest.mark.parametrize("n_plain", [1, 63, 64, 65, 129])
def test_twin_equals_what_exists_across_the_seams(n_plain, n_wide):
    """1, 63, 64, 65 and 129 ordinary nodes - every 64-node chunk boundary - among 0, 1 and 65 wide records, K = 1, 2 and 64."""
    descs = gc.seam_descs(9880, n_wide, n_plain)
    listed = check_against_what_exists(_twin, descs, seam_specs())
    assert listed > 0 or n_plain + n_wide < 3, listed


def test_the_whole_composed_list():
    """K = 64 against the composed form itself, entry by entry, where it is affordable."""
    descs = gc.seam_descs(9880, 20, 45)
    assert check_against_what_exists(_twin, descs, seam_specs(), ks=(64,), composed_k=64) > 30


def test_masks_only_wide_only_ordinary_and_none():
    """A subset `nl` of an attached cluster is the candidate mask: the wide nodes alone, the ordinary nodes alone - either way the
    composed form's lists; a mask without a node: nothing feasible, nothing listed."""
    _, descs, _ = gc.cluster_case("mixed")
    nl = util.build_cluster(descs)
    specs = seam_specs()
    tops = lambda: [refmodel.make_topology(s) for s in specs]      # noqa: E731
    m, mc = _twin(), _twin()
    m.attach(nl)
    mc.attach(nl)
    wide = set(m.wide_nodes)
    assert 10 < len(wide) < len(nl) - 10
    total = 0
    for keep_wide in (False, True):
        sub = {nm: nd for nm, nd in nl.items() if (nm in wide) == keep_wide}
        got = m.CandidatesMany(sub, tops(), k=8, now=util.CLOCK, big=True)
        want = mc.CandidatesMany(sub, tops(), k=8, now=util.CLOCK)
        for x, y in zip(got, want):
            assert x.error is None and x.entries == y.entries and (x.feasible, x.preferred, x.nodes) == (y.feasible, y.preferred, y.nodes)
        assert all((e[0] in wide) == keep_wide for c in got for e in c.entries)
        total += sum(len(c.entries) for c in got)
    assert total > 6
    reqs = np.array([m.packer.digest_big(t) for t in tops()], dtype=pack.BIG_REQ)
    sums, entries = m.engine.candidates_big(reqs, util.CLOCK, 8, cand=np.zeros((m.engine.n + 63) // 64, np.uint64))
    assert not sums["feasible"].any() and not sums["returned"].any() and entries.tobytes() == bytes(entries.nbytes)
    assert (sums["form"] == pack.CANDIDATES_FORM_BIG).all()


def test_a_node_inside_the_busy_window():
    """A node stamped three seconds before `now` leaves the list of a pod that requests GPUs and stays in the list of one that does
    not - as in the composed form on the same nodes."""
    _, descs, _ = gc.cluster_case("mixed")
    for d in descs:
        d["busy_time"] = util.CLOCK - 500.0
    specs = seam_specs()
    tops = lambda: [refmodel.make_topology(s) for s in specs]      # noqa: E731
    before = _twin().CandidatesMany(util.build_cluster(descs), tops(), k=64, now=util.CLOCK, big=True)
    names = [[e[0] for e in c.entries] for c in before]
    both = [nm for nm in names[1] if nm in names[0]]             # (specs[0] has no GPU, specs[1] requests some)
    assert both and all(c.feasible < 64 for c in before)
    victim = both[0]
    next(d for d in descs if d["name"] == victim)["busy_time"] = util.CLOCK - 3.0
    nl = util.build_cluster(descs)
    after = _twin().CandidatesMany(nl, tops(), k=64, now=util.CLOCK, big=True)
    assert [e for e in before[1].entries if e[0] != victim] == after[1].entries and after[1].feasible == before[1].feasible - 1
    assert after[0].entries == before[0].entries
    composed = _twin().CandidatesMany(nl, tops(), k=64, now=util.CLOCK)
    assert [c.entries for c in after] == [c.entries for c in composed]


def test_node_groups_are_filtered_as_findnodes_filters_them():
    """pod_groups given: the request record carries the groups and the entry applies InitialNodeFilter itself, as FindNodes does."""
    nl = util.mixed_cluster(1730, 50, occupancy=0.1)
    labels = sorted({g for nd in nl.values() for g in getattr(nd, "groups", [])})
    specs = seam_specs()
    tops = lambda: [refmodel.make_topology(s) for s in specs]      # noqa: E731
    groups = [labels[:1] or ["default"]] * len(specs)
    m = _twin()
    got = m.CandidatesMany(nl, tops(), k=8, pod_groups=groups, now=util.CLOCK, big=True)
    want = _twin().CandidatesMany(nl, tops(), k=8, pod_groups=groups, now=util.CLOCK)
    found = m.FindNodes(nl, tops(), pod_groups=groups, now=util.CLOCK)
    for x, y, f in zip(got, want, found):
        assert x.error is None and x.entries == y.entries and (x.feasible, x.preferred) == (y.feasible, y.preferred)
        assert (x.entries[0] if x.entries else (None,)) == f


# ---- the kernel's record logic and two-range pick on emulated lanes ------------------------------------------------------------------------
def _scalar_list(planes, wide, k, pref_bit):
    """The selection order, as it reads: preferred nodes by index, then the others by index; cut at k."""
    hits = [(not pref, index) for ok, pref, index in list(planes) + list(wide) if ok]
    return [index | (0 if not_pref else pref_bit) for not_pref, index in sorted(hits)[:k]]


@pytest.mark.parametrize("k", [1, 2, 8, 64])
def test_emulated_scan_and_pick_equal_the_selection_order(k):
    """Random verdicts over both ranges - the wide records' indexes scattered among the planes' (whose units at those indexes are
    placeholders that never fit) - at 1, 63, 64, 65, 129 and 300 units, with one block per range, a block per chunk and block counts
    that do not divide the chunks: the list, the counts and the records' bounds against the scalar statement."""
    L = bt.scan_lib()
    pref_bit = int(L.we_big_cand_pref_bit())
    rng = np.random.default_rng(4300 + k)
    cases = 0
    for n in (1, 63, 64, 65, 129, 300):
        for n_wide in (0, 1, 65):
            if n_wide > n:
                continue
            widx = np.sort(rng.choice(n, size=n_wide, replace=False))
            for density, gpuless in ((0.0, True), (0.05, True), (0.5, True), (1.0, True), (0.3, False)):
                def draw(indexes, dead=()):
                    units = []
                    for i in indexes:
                        ok = bool(rng.random() < density) and i not in dead
                        units.append((ok, gpuless and bool(rng.random() < 0.4), int(i)))
                    return units
                planes, wide = draw(range(n), set(widx.tolist())), draw(widx)
                chunks, wchunks = (n + 63) // 64, (n_wide + 63) // 64
                for nbp, nbw in {(1, min(1, wchunks)), (chunks, wchunks), (max(1, chunks - 1), max(min(1, wchunks), wchunks - 1))}:
                    got, feasible, preferred, recs = bt.scan_pick(planes, wide, nbp, nbw, k, global_base=int(rng.integers(0, 1 << 20)))
                    assert got.tolist() == _scalar_list(planes, wide, k, pref_bit)
                    every = planes + wide
                    assert feasible == sum(u[0] for u in every) and preferred == sum(u[0] and u[1] for u in every)
                    assert (recs[:, 0] <= k).all() and (recs[:, 1] <= recs[:, 0]).all() and not recs[:, 2:4].any()
                    cases += 1
    assert cases >= 100


@pytest.mark.parametrize("k", [1, 8, 64])
def test_three_twin_shards_equal_one_twin(k):
    """GroupEngine over three twin shards (sharding.merge_candidates with the big entry's record) and the group entry's merge header
    (candidates_merge.h, instantiated for the big entry) over the shards' parts: the unsharded twin's lists and sums."""
    from nhd_amd import sharding
    for sharing in (False, True):
        with gc.sharing_all(sharing):
            nl = util.mixed_cluster(1750, 200, occupancy=0.1)
            specs = seam_specs()
            tops = lambda: [refmodel.make_topology(s) for s in specs]      # noqa: E731
            one = _twin()
            a = one.CandidatesMany(nl, tops(), k=k, now=util.CLOCK, big=True)
            grp = HipMatcher(clock=lambda: util.CLOCK, engine_factory=bt.CandidatesBigHarnessEngine, devices=[0, 0, 0])
            assert len(grp.engine.shards) == 3
            b = grp.CandidatesMany(nl, tops(), k=k, now=util.CLOCK, big=True)
            reqs = np.array([one.packer.digest_big(t) for t in tops()], dtype=pack.BIG_REQ)
            s1, e1 = one.engine.candidates_big(reqs, util.CLOCK, k)
            parts = [sh.candidates_big(reqs, util.CLOCK, k) for sh in grp.engine.shards if sh.n]     # (shards are cut at 64-node chunks)
            assert len(parts) >= 2
        for x, y in zip(a, b):
            assert x.error is None and y.error is None and x.entries == y.entries
            assert (x.feasible, x.preferred, x.k, x.nodes, x.form) == (y.feasible, y.preferred, y.k, y.nodes, y.form)
        sm, em, owner = bt.merge(parts, k)
        sp, ep, owner_p = sharding.merge_candidates([p[0] for p in parts], [p[1] for p in parts], k, entry_dtype=pack.BIG_CANDIDATE)
        assert sm.tobytes() == s1.tobytes() == sp.tobytes() and em.tobytes() == e1.tobytes() == ep.tobytes()
        assert np.array_equal(owner, owner_p)
        assert sum(len(c.entries) for c in a) > min(k, 3)
    assert cr.K == cb.K
