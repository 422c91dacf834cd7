"""nhdfit_candidates_big's host twin (tests/harness/candidates_big_twin.cpp: wide_view / wide_fits / wide_map per node over
wide_core.h's scalar forms, ranked by one sort of the score words), through HipMatcher.CandidatesMany(big=True), against candidates
as the UNMODIFIED reference defines them (tests/candidates_reference.iterate over Matcher().FindNode on a dict that loses each answer,
K = 8; live where the reference tree exists - a few minutes: the reference enumerates every tuple of a pod of 5..8 groups - its stored
answers elsewhere, tests/refanswers.py).  Every entry - name and mapping - must agree and the list must end where the reference's ends;
no pod is skipped.  The stored answers are what tests/test_candidates_big_gpu.py holds the device to."""
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from tests import candidates_big_check as cb
from tests import headroom_general_check as gc
from tests import util
from tests.harness.candidates_big_twin import CandidatesBigHarnessEngine


def _twin(clock):
    return HipMatcher(clock=lambda: clock, engine_factory=CandidatesBigHarnessEngine)


def _gpuless(spec):
    return not any(len(g["gpus"]) > 0 for g in spec["groups"])


def _crosses_the_seam(nl, spec, row):
    """The list of a pod without GPUs goes from nodes without GPUs on to nodes with them."""
    has = [len(nl[e[0]].gpus) > 0 for e in row]
    return _gpuless(spec) and has == sorted(has) and has[0] is False and has[-1] is True


@pytest.mark.parametrize("name", list(gc.CLUSTERS))
def test_clusters(refans, name):
    """Seeded pods of five or six groups (cb.CLUSTER_PODS of them) on (a) a mixed cluster whose wide nodes interleave with the others,
    (b) two ENABLE_SHARING clusters (all three switches flipped).  The reference's lists say something by themselves: on the mixed cluster
    lists that interleave wide and ordinary nodes, on a sharing cluster a list of two or more entries and one that crosses the
    preferred seam."""
    sharing, descs, _ = gc.cluster_case(name)
    specs = cb.cluster_specs(name)
    want = refans.take(lambda: cb.reference_lists(refans.ref, descs, specs, sharing, util.CLOCK))
    m, nl, got, lists, fits = cb.matcher_lists(_twin, descs, specs, sharing, util.CLOCK)
    assert m.unmirrored == {}
    assert lists == want
    cb.consistent(got, lists, fits)
    wide = set(m.wide_nodes)
    if sharing:
        assert len(wide) == len(descs)
        assert sum(len(row) >= 2 for row in want) >= 2
    if name == "mixed":
        mixed = [row for row in want if 0 < sum(e[0] in wide for e in row) < len(row)]
        assert len(mixed) >= 2 and any([e[0] in wide for e in row] != sorted(e[0] in wide for e in row) for row in mixed)
    if name == "sharing_random":
        assert any(len(row) >= 2 and _crosses_the_seam(nl, s, row) for s, row in zip(specs, want))


@pytest.mark.parametrize("name", cb.GROUPED)
def test_clusters_with_node_groups(refans, name):
    """The same pods with node groups (cb.GROUP_CYCLE) on a mixed and a sharing cluster: the reference's FindNode on what
    InitialNodeFilter leaves of the cluster, the entry on the whole cluster with `pod_groups` - it applies the filter itself.  The
    filter says something: it drops nodes for every pod, and at least one list differs from the unfiltered one."""
    sharing, descs, _ = gc.cluster_case(name)
    specs, groups = cb.cluster_specs(name), cb.cluster_groups(name)
    keep = cb.cluster_keep(descs, groups)
    assert all(0 < len(kp) < len(descs) for kp in keep)
    want = refans.take(lambda: cb.reference_lists(refans.ref, descs, specs, sharing, util.CLOCK, keep=keep))
    m, nl, got, lists, fits = cb.matcher_lists(_twin, descs, specs, sharing, util.CLOCK, pod_groups=groups)
    assert m.unmirrored == {}
    assert lists == want
    cb.consistent(got, lists, fits)
    assert all(e[0] in kp for row, kp in zip(want, keep) for e in row)
    assert want != cb.stored(f"test_clusters[{name}]")
    assert sum(len(row) >= 1 for row in want) >= 2 and any(len(row) >= 2 for row in want)


@pytest.mark.parametrize("fixture", cb.FIXTURE_IDS)
def test_fixtures(refans, fixture):
    """Every pod of the general path of the reference-generated fixtures tests/golden/big against its fixture's cluster (they name no
    node groups).  The reference's own `feasible` rows of the fixture say which lists K cuts."""
    case, idx, specs = cb.load_fixture(cb.FIXTURES[cb.FIXTURE_IDS.index(fixture)])
    assert len(idx) >= 5
    want = refans.take(lambda: cb.reference_lists(refans.ref, case["nodes"], specs, False, case["clock"]))
    m, nl, got, lists, fits = cb.matcher_lists(_twin, case["nodes"], specs, False, case["clock"])
    assert m.unmirrored == {}
    assert lists == want
    cb.consistent(got, lists, fits)
    feasible = [case["feasible"][p].count("1") for p in idx]
    assert [c.feasible for c in got] == feasible and [len(row) for row in want] == [min(cb.K, f) for f in feasible]
    for p, row in zip(idx, want):                          # entry 0 is the fixture's own FindNode answer
        assert case["snapshot"][p][0] == (row[0][0] if row else None)
    if fixture == "big_mixed":
        assert max(feasible) > cb.K and sum(f >= 2 for f in feasible) >= 9
    assert max(feasible) >= 2


def test_the_stored_lists_say_something():
    """Over all the stored answers: at least 12 lists of two or more entries, a list cut by K (eight entries where the fixture's
    own row counts more feasible nodes), a list of a pod without GPUs that crosses the preferred seam."""
    rows, cut, seam = [], 0, 0
    for name in gc.CLUSTERS:
        sharing, descs, _ = gc.cluster_case(name)
        with gc.sharing_all(sharing):
            nl = util.build_cluster(descs)
        for s, row in zip(cb.cluster_specs(name), cb.stored(f"test_clusters[{name}]")):
            rows.append(row)
            seam += bool(row) and _crosses_the_seam(nl, s, row)
    for fixture, path in zip(cb.FIXTURE_IDS, cb.FIXTURES):
        case, idx, specs = cb.load_fixture(path)
        nl = util.build_cluster(case["nodes"])
        for p, s, row in zip(idx, specs, cb.stored(f"test_fixtures[{fixture}]")):
            rows.append(row)
            cut += len(row) == cb.K and case["feasible"][p].count("1") > cb.K
            seam += bool(row) and _crosses_the_seam(nl, s, row)
    assert sum(len(row) >= 2 for row in rows) >= 12
    assert cut >= 1 and seam >= 1
    assert pack.CANDIDATES_FORM_BIG == 8
