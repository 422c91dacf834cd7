"""nhdfit_candidates_general's host twin (tests/harness/candidates_general_twin.cpp: wide_fits / wide_map per wide record over
wide_core.h's scalar forms, merged with the planes' list by the rule of candidates_merge.h), through
HipMatcher.CandidatesMany(general=True), against candidates as the UNMODIFIED reference defines them
(tests/candidates_reference.iterate over Matcher().FindNode on a dict that loses each answer, K = 8; live where the reference tree
exists, its stored answers elsewhere - tests/refanswers.py).  Every entry - name and mapping - must agree and the list must end where
the reference's ends; no pod is skipped.  The stored answers are what tests/test_candidates_general_gpu.py holds the device to."""
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from tests import candidates_general_check as cg
from tests import headroom_general_check as gc
from tests import util
from tests.harness.candidates_general_twin import CandidatesGeneralHarnessEngine


def _twin(clock):
    return HipMatcher(clock=lambda: clock, engine_factory=CandidatesGeneralHarnessEngine)


@pytest.mark.parametrize("name", list(gc.CLUSTERS))
def test_clusters(refans, name):
    """(a) a mixed cluster whose wide nodes interleave with the others, (b) two ENABLE_SHARING clusters (all three switches flipped),
    eighteen templates of one to four groups.  The inputs say something: cg.FACTS - lists that interleave wide and ordinary nodes, a
    feasible four-group pod, lists of preferred nodes only and one that crosses the preferred seam."""
    sharing, descs, _ = gc.cluster_case(name)
    specs = cg.templates()
    assert len(specs) == 18
    want = refans.take(lambda: cg.reference_lists(refans.ref, descs, specs, sharing, util.CLOCK))
    m, nl, got, lists, fits = cg.matcher_lists(_twin, descs, specs, sharing, util.CLOCK)
    assert m.unmirrored == {}
    assert lists == want
    cg.consistent(got, lists, fits)
    wide = set(m.wide_nodes)
    if sharing:
        assert len(wide) == len(descs)
    assert all(c.form & pack.CANDIDATES_FORM_WIDE for c in got)
    for (cluster, t), (feasible, preferred) in cg.FACTS.items():
        if cluster == name:
            assert (got[t].feasible, got[t].preferred) == (feasible, preferred), (cluster, t)
    gpus = lambda row: [len(nl[e[0]].gpus) > 0 for e in row]      # noqa: E731
    if name == "mixed":
        kinds = [e[0] in wide for e in want[cg.T_FOUR0]]
        assert len(kinds) == 8 and 3 <= sum(kinds) <= 5 and kinds[0] != kinds[1]      # wide and ordinary nodes interleaved
        assert sorted(e[0] in wide for e in want[cg.T_FOUR3]) == [False, True]       # four groups: one wide, one ordinary
        row = want[cg.T_GPULESS]
        assert not any(gpus(row)) and 0 < sum(e[0] in wide for e in row) < 8           # all preferred, wide and ordinary mixed
    if name == "sharing_random":
        assert gpus(want[cg.T_FOUR1]) == [False] * 7 + [True]                          # the list crosses the preferred seam
    if name == "sharing_mixed":
        assert gpus(want[cg.T_NOTHING]) == [False] * 8


@pytest.mark.parametrize("fixture,with_groups", gc.FIXTURE_CASES, ids=[f"{f}-{'groups' if g else 'plain'}" for f, g in gc.FIXTURE_CASES])
def test_fixtures(refans, fixture, with_groups):
    """(c) every pod of the reference-generated fixtures of the general path against its fixture's cluster; with the fixture's node
    groups (where it names them) FindNode is handed what InitialNodeFilter leaves, and the twin applies the filter itself.  Every node
    of every fixture is mirrored - beyond_layout's three- and four-socket and 96-core-socket nodes as wide records."""
    case, specs, groups, sharing = gc.load_fixture(gc.FIXTURES[gc.FIXTURE_IDS.index(fixture)])
    keep = gc.fixture_keep(case, groups) if with_groups else None
    want = refans.take(lambda: cg.reference_lists(refans.ref, case["nodes"], specs, sharing, case["clock"], keep=keep))
    m, nl, got, lists, fits = cg.matcher_lists(_twin, case["nodes"], specs, sharing, case["clock"], pod_groups=groups if with_groups else None)
    assert m.unmirrored == {}
    assert lists == want
    cg.consistent(got, lists, fits)
    assert max(len(row) for row in want) >= 1
