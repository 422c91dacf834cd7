"""nhdfit_candidates' host twin (tests/harness/candidates_twin.cpp: the definition over the shared headers' scalar forms), through
HipMatcher.CandidatesMany, against candidates as the UNMODIFIED reference defines them (tests/candidates_reference.py:
Matcher().FindNode on a dict that loses each answer, K = 8; live where the reference tree exists, its stored answers elsewhere -
tests/refanswers.py).  Every entry - name and mapping - must agree, and the list must end where the reference's ends.  The stored
answers are what tests/test_candidates_gpu.py holds the device to."""
import pytest

from nhd_amd.matcher import HipMatcher
from tests import candidates_reference as cr
from tests.harness.candidates_twin import CandidatesHarnessEngine


def _twin(clock):
    return HipMatcher(clock=lambda: clock, engine_factory=CandidatesHarnessEngine)


def _consistent(results, lists):
    """A list is as long as the summary says, and no node is named twice."""
    for c, row in zip(results, lists):
        assert len(row) == min(cr.K, c.feasible) and c.preferred <= c.feasible
        assert len({e[0] for e in row}) == len(row)


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_synth_configurations(refans, cfg):
    """The five BASELINE configurations at 48 nodes, their first 8 pods, every node a candidate.  The inputs say something: some pod
    of every configuration has a list of more than one entry."""
    want = refans.take(lambda: cr.reference_synth(refans.ref, cfg))
    got, lists = cr.matcher_synth(_twin, cfg)
    assert lists == want
    _consistent(got, lists)
    assert len(want) == cr.SYNTH_PODS and max(len(row) for row in want) > 1


@pytest.mark.parametrize("with_groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("golden", cr.IDS)
def test_goldens(refans, golden, with_groups):
    """Every pod of the reference-generated fixtures against its fixture's cluster; with the fixtures' node groups FindNode is handed
    what InitialNodeFilter leaves, and the kernel applies the filter itself."""
    path = cr.GOLDENS[cr.IDS.index(golden)]
    want = refans.take(lambda: cr.reference_golden(refans.ref, path, with_groups))
    got, lists = cr.matcher_golden(_twin, path, with_groups)
    assert lists == want
    _consistent(got, lists)
