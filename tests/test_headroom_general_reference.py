"""nhdfit_headroom_general's host twin (tests/harness/headroom_general_twin.cpp: the loop k_wide_room runs per wide record, over
wide_core.h's scalar forms), through HipMatcher.HeadroomMany(general=True), against headroom as the UNMODIFIED reference defines it
(tests/headroom_reference.py: FindNode -> SetPhysicalIdsFromMapping -> ClaimPodNICResources back to back on a private rebuild of the
node; live where the reference tree exists, its stored answers elsewhere - tests/refanswers.py).  Count AND stopped flag of every
(template, node) must agree; no pair is skipped.  The stored answers are what tests/test_headroom_general_gpu.py holds the device to."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from tests import headroom_general_check as gc
from tests import util
from tests.harness.headroom_general_twin import HeadroomGeneralHarnessEngine
from workload import refmodel

COUNT, STOPPED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED


def _twin(clock):
    return HipMatcher(clock=lambda: clock, engine_factory=HeadroomGeneralHarnessEngine)


def _consistent(results, entries, cap):
    """The summary of every template is the summary of its entries; nothing is left unevaluated."""
    for h, row in zip(results, entries):
        e = np.asarray(row)
        k = e & COUNT
        assert h.error is None and h.not_evaluated == 0
        assert (h.replicas, h.nodes_with_room, h.max_on_one_node) == (int(k.sum()), int((k > 0).sum()), int(k.max(initial=0)))
        assert h.stopped == int((e & STOPPED != 0).sum()) and h.saturated == int((k >= cap).sum())


@pytest.mark.parametrize("name", list(gc.CLUSTERS))
def test_clusters(refans, name):
    """(a) the nodes drawn wide of a mixed cluster, (b) two ENABLE_SHARING clusters (all three switches flipped), twelve templates of
    one to four groups, bound 37.  The independent oracle agrees with the reference on every pair; the inputs say something: pairs
    with room, and pairs that take more than one replica (under ENABLE_SHARING: several replicas priced against each other)."""
    sharing, descs, wide_only = gc.cluster_case(name)
    specs = gc.templates()
    sel = gc.selection(descs, wide_only)
    part = [descs[i] for i in sel]
    want = refans.take(lambda: gc.reference_entries(refans.ref, part, specs, sharing, util.CLOCK))
    m, got, entries = gc.matcher_entries(_twin, descs, specs, sharing, util.CLOCK)
    assert m.unmirrored == {}
    assert [[row[i] for i in sel] for row in entries] == want
    _consistent(got, entries, gc.CAP)
    if sharing:
        assert len(m.wide_nodes) == len(descs) and all(h.form & pack.HEADROOM_FORM_WIDE for h in got)
    assert gc.oracle_entries(part, specs, sharing, util.CLOCK) == want
    w = np.asarray(want)
    k = w & COUNT
    assert (k.size, int((k > 0).sum()), int((k > 1).sum())) == gc.PAIRS[name]
    assert (k > 0).sum() > 0 and (k > 1).sum() > 0
    assert not (w & STOPPED).any()                            # (none of these runs ends at a commit the reference raises on)


@pytest.mark.parametrize("fixture,with_groups", gc.FIXTURE_CASES, ids=[f"{f}-{'groups' if g else 'plain'}" for f, g in gc.FIXTURE_CASES])
def test_fixtures(refans, fixture, with_groups):
    """(c) every pod of the reference-generated fixtures of the general path against its fixture's cluster; with the fixture's node
    groups (where it names them) the nodes InitialNodeFilter drops have 0.  Every node of every fixture is mirrored - the
    three- and four-socket and the 96-core-socket nodes of beyond_layout as wide records - so every pair is compared."""
    case, specs, groups, sharing = gc.load_fixture(gc.FIXTURES[gc.FIXTURE_IDS.index(fixture)])
    keep = gc.fixture_keep(case, groups) if with_groups else None
    want = refans.take(lambda: gc.reference_entries(refans.ref, case["nodes"], specs, sharing, case["clock"], cap=gc.CAP, keep=keep))
    m, got, entries = gc.matcher_entries(_twin, case["nodes"], specs, sharing, case["clock"], pod_groups=groups if with_groups else None)
    assert m.unmirrored == {}                                  # (beyond_layout's quad-socket and wide-socket nodes are wide records: no pair is left out)
    assert entries == want
    for h in got:
        assert h.not_evaluated == 0 and h.unmirrored == 0
    assert (np.asarray(want) & COUNT).max() >= 1


@pytest.mark.parametrize("name", ["mixed", "sharing_random"])
def test_a_template_that_asks_for_nothing_saturates(refans, name):
    """(d) it fits for ever: every node the reference matches at all reaches the bound, wide and shared ones as the others."""
    sharing, descs, _ = gc.cluster_case(name)
    want = refans.take(lambda: gc.reference_entries(refans.ref, descs, [gc.NOTHING], sharing, util.CLOCK))
    m, got, entries = gc.matcher_entries(_twin, descs, [gc.NOTHING], sharing, util.CLOCK)
    assert entries == want
    _consistent(got, entries, gc.CAP)
    assert set(want[0]) == {0, gc.CAP} and got[0].saturated == want[0].count(gc.CAP) > len(descs) // 2
    wide = [i for i, d in enumerate(descs) if d["name"] in set(m.wide_nodes)]
    assert len(wide) >= 10 and sum(want[0][i] == gc.CAP for i in wide) > len(wide) // 2
    assert refmodel.ENABLE_SHARING is False
