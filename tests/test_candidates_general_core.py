"""nhdfit_candidates_general's arithmetic on the CPU: the kernel's own mapping routine (wide_candidates_kernel.h
wide_map_on_state_wave: the stages with lane = tuple, the set model on the first lane - cut out of the header and run on emulated
lanes) against the scalar wide_map for every feasible (template, wide record) pair of the three clusters, bit for bit; the merge rule
k_wide_cand_map's blocks run (candidates_merge.h cand_merged_entry) against a sort by score of the union."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import STAGES, HipMatcher
from tests import candidates_general_check as cg
from tests import headroom_general_check as gc
from tests import util
from tests.harness import candidates_general_twin as gt
from workload import refmodel


@pytest.mark.parametrize("name", list(gc.CLUSTERS))
def test_emulated_lanes_equal_the_scalar_mapping(name):
    """wide_map_on_state_wave's text on 64 emulated lanes gives the scalar wide_map's mapping and code for every pair explain calls
    FITS: all 24 bytes of the record.  The lanes agree among themselves (the emulation reports it) and every ballot is reached by all
    of them (it would hang).  The inputs say something: pairs of every group count, mapped."""
    sharing, descs, _ = gc.cluster_case(name)
    specs = cg.templates()
    with gc.sharing_all(sharing):
        nl = util.build_cluster(descs)
        m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=gt.CandidatesGeneralHarnessEngine)
        tops = [refmodel.make_topology(s) for s in specs]
        ex = m.ExplainNodes(nl, tops, now=util.CLOCK, per_node=True)
        reqs = m.packer.digest_many([refmodel.make_topology(s) for s in specs])
    wide, share = m.engine._wide_records(), m.engine._share_records()
    assert (share is not None) == sharing and len(wide) >= 16
    fits = np.stack([e.stages == STAGES.index("FITS") for e in ex])[:, wide["index"]]
    mw, rw, ms, rs = gt.wide_map_wave(m.packer, wide, share, reqs, fits)
    assert fits.sum() > 100
    assert mw.tobytes() == ms.tobytes() and np.array_equal(rw, rs)
    assert (rw[fits] == 1).all() and (mw["valid"][fits] == 1).all() and not rw[~fits].any()
    groups = {int(reqs["n_groups"][p]) for p in range(len(reqs)) if fits[p].any()}
    assert groups == {1, 2, 3, 4} or name != "mixed", groups


def _scores(rng, n, lo=1, hi=1 << 40):
    return np.sort(rng.choice(np.arange(lo, hi, 7919, dtype=np.uint64), size=n, replace=False))[::-1]


@pytest.mark.parametrize("k", [1, 8, 64])
def test_merge_is_a_sort_by_score_of_the_union(k):
    """Entry j of the planes' list and the wide list merged, for every j below K: the j-th of the union sorted by descending score,
    named by its own list and position; past the union's end there is no entry.  Either list empty, both empty, one entirely in
    front of the other, interleaved.  Two entries never tie: a score names one node (distinct indices), asserted on the inputs."""
    rng = np.random.default_rng(1700 + k)
    cases = []
    for na, nb in [(0, 0), (0, k), (k, 0), (k, k), (1, k), (k // 2, k // 3), (min(64, k + 3), 2)]:
        pool = _scores(rng, na + nb)
        pick = rng.permutation(na + nb) < na
        cases.append((pool[pick], pool[~pick]))
    hi, lo = _scores(rng, k, lo=1 << 41, hi=1 << 42), _scores(rng, k)
    cases += [(hi, lo), (lo, hi)]
    for a, b in cases:
        union = [(int(s), False, i) for i, s in enumerate(a)] + [(int(s), True, i) for i, s in enumerate(b)]
        assert len({u[0] for u in union}) == len(union)                 # no ties
        union.sort(key=lambda u: -u[0])
        for j in range(k):
            want = (union[j][1], union[j][2]) if j < len(union) else None
            assert gt.merged_entry(a, b, j) == want, (len(a), len(b), j)


def test_the_twin_without_wide_records_is_the_plain_twin():
    """n_wide == 0: the same bytes, no new bit."""
    from tests.harness import candidates_twin as ct
    nl = util.random_cluster(1710, 70, occupancy=0.15)
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=gt.CandidatesGeneralHarnessEngine)
    tops = [refmodel.make_topology(s) for s in cg.templates()]
    m.FindNodes(nl, tops, now=util.CLOCK)
    reqs = m.packer.digest_many(tops)
    plain = ct.candidates(m.packer, m.engine.table, [], reqs, util.CLOCK, 8)
    general = gt.candidates_general(m.packer, m.engine.table, [], None, reqs, util.CLOCK, 8)
    assert plain[0].tobytes() == general[0].tobytes() and plain[1].tobytes() == general[1].tobytes()
    assert not (general[0]["form"] & pack.CANDIDATES_FORM_WIDE).any() and general[0]["feasible"].sum() > 50
