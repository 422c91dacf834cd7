"""nhdfit_headroom's host twin (tests/harness/headroom_twin.cpp: the kernel's loop over the shared headers' scalar forms), through
HipMatcher.HeadroomMany, against headroom as the UNMODIFIED reference defines it (tests/headroom_reference.py: FindNode ->
SetPhysicalIdsFromMapping -> ClaimPodNICResources back to back on a private rebuild of the node, busy window out of the way; live
where the reference tree exists, its stored answers elsewhere - tests/refanswers.py).  Count AND stopped flag of every
(template, node) must agree.  The stored answers are what tests/test_headroom_gpu.py holds the device to."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from tests import headroom_check as hc
from tests.harness.headroom_twin import HeadroomHarnessEngine


def _twin(clock):
    return HipMatcher(clock=lambda: clock, engine_factory=HeadroomHarnessEngine)


def _consistent(results, entries, n):
    """The summary of every template is the summary of its entries; nothing is left unevaluated."""
    for h, row in zip(results, entries):
        k = np.asarray(row) & pack.HEADROOM_COUNT_MASK
        assert len(row) == n and h.nodes == n
        assert (h.replicas, h.nodes_with_room, h.max_on_one_node) == (int(k.sum()), int((k > 0).sum()), int(k.max(initial=0)))
        assert h.stopped == int((np.asarray(row) & pack.HEADROOM_STOPPED != 0).sum())
        assert h.not_evaluated == 0 and h.unmirrored == 0 and h.saturated == int((k >= hc.CAP).sum())
        assert h.by_node() == dict(zip(h._names, k.tolist()))


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_synth_configurations(refans, cfg):
    """The five BASELINE configurations at 48 nodes, their first pods as templates, every node a candidate.  The inputs say something:
    on configurations 2-5 at least half of the pairs have headroom >= 1 and some node takes >= 4 replicas."""
    want = refans.take(lambda: hc.reference_synth(refans.ref, cfg))
    got, entries = hc.matcher_synth(_twin, cfg)
    assert entries == want
    _consistent(got, entries, hc.SYNTH_NODES)
    k = np.asarray(want) & pack.HEADROOM_COUNT_MASK
    assert k.shape == (hc.SYNTH_TEMPLATES, hc.SYNTH_NODES)
    if cfg >= 2:
        assert (k >= 1).sum() * 2 >= k.size, int((k >= 1).sum())
        assert k.max() >= 4, int(k.max())
    else:
        assert k.min() >= 2                                  # config 1: an empty cluster, every node takes several


@pytest.mark.parametrize("with_groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("golden", hc.IDS)
def test_goldens(refans, golden, with_groups):
    """Every pod spec of the reference-generated fixtures against its fixture's cluster; with the fixtures' node groups the nodes
    InitialNodeFilter drops have headroom 0.  A run the reference ends by raising is compared as flagged, never dropped."""
    path = hc.GOLDENS[hc.IDS.index(golden)]
    want = refans.take(lambda: hc.reference_golden(refans.ref, path, with_groups))
    got, entries = hc.matcher_golden(_twin, path, with_groups)
    assert entries == want
    _consistent(got, entries, len(want[0]))
