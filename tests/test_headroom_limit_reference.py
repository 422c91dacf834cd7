"""nhdfit_headroom_limits' host twin (tests/harness/headroom_limit_twin.cpp), through HipMatcher.HeadroomMany(limits=True), against the
stage that ends each node's run as the UNMODIFIED reference defines it (tests/headroom_limit_reference.py: the reference's own run,
then the stage its filter names on the node object the run left behind; live where the reference tree exists, its stored answers
elsewhere - tests/refanswers.py).  Count and stopped flag of every (template, node) must agree, and the stage of every pair that is
not stopped.  What the semantics promise - FITS only at the cap, BUSY never, the stages that end runs - is asserted on the
REFERENCE's answers.  The stored answers are what tests/test_headroom_limit_gpu.py holds the device to."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from tests import headroom_check as hc
from tests import headroom_limit_check as lc
from tests.harness.headroom_limit_twin import HeadroomLimitHarnessEngine


def _twin(clock):
    return HipMatcher(clock=lambda: clock, engine_factory=HeadroomLimitHarnessEngine)


def _pairs(want):
    """(count, stopped, stage) arrays over every pair of a stored case."""
    e = np.asarray(want[0], np.int64).reshape(-1)
    st = np.asarray([s for row in want[1] for s in lc.undigits(row)], np.int64)
    return e & pack.HEADROOM_COUNT_MASK, (e & pack.HEADROOM_STOPPED) != 0, st


def _reference_keeps_its_promises(want, cap):
    k, stopped, st = _pairs(want)
    assert ((st == lc.NONE) == stopped).all()
    assert (st != lc.BUSY).all()
    assert (k[st == lc.FITS] == cap).all()                               # below the cap a run never ends at FITS
    return k, stopped, st


@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_synth_configurations(refans, cfg):
    want = refans.take(lambda: lc.reference_synth(refans.ref, cfg))
    got, answers = lc.matcher_synth(_twin, cfg)
    lc.same_where_not_stopped(answers, want)
    lc.check_identities(got, hc.SYNTH_NODES)
    _reference_keeps_its_promises(want, lc.CAP)


@pytest.mark.parametrize("with_groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("golden", hc.IDS)
def test_goldens(refans, golden, with_groups):
    path = hc.GOLDENS[hc.IDS.index(golden)]
    want = refans.take(lambda: lc.reference_golden(refans.ref, path, with_groups))
    got, answers = lc.matcher_golden(_twin, path, with_groups)
    lc.same_where_not_stopped(answers, want)
    lc.check_identities(got, len(want[0][0]))
    _reference_keeps_its_promises(want, lc.CAP)


def test_the_inputs_cover_the_stages():
    """On the reference's answers of the cases above: each of HUGEPAGES, GPU, CPU, NIC, PCI and NUMA ends at least one run of at least
    one replica; MAINTENANCE and NOT_CANDIDATE occur; the run of fixture random3 the reference fails on carries no stage."""
    cases = {}
    for cfg in [1, 2, 3, 4, 5]:
        cases[f"synth{cfg}"] = _pairs(lc.stored(f"test_synth_configurations[{cfg}]"))
    for g in hc.IDS:
        for w in ("plain", "groups"):
            cases[f"{g}-{w}"] = _pairs(lc.stored(f"test_goldens[{g}-{w}]"))
    k = np.concatenate([c[0] for c in cases.values()])
    st = np.concatenate([c[2] for c in cases.values()])
    for stage in (lc.HUGEPAGES, lc.GPU, lc.CPU, lc.NIC, lc.PCI, lc.NUMA):
        assert ((st == stage) & (k >= 1)).any(), lc.STAGE_NAMES[stage]
    assert (st == lc.MAINTENANCE).any() and (st == lc.NOT_CANDIDATE).any()
    k3, stopped3, st3 = cases["random3-plain"]
    assert stopped3.sum() >= 1 and (st3[stopped3] == lc.NONE).all()


def test_saturation(refans):
    """Synth configuration 4 again with max_per_node = 2, the twin against the reference pair by pair.  On the REFERENCE's answers:
    a run ends at FITS exactly where it reached the cap AND the reference's run with the larger cap goes further - the run stopped
    there, not the node.  "FITS <=> count == cap" alone does not hold on the reference: of the 147 pairs that reach 2 replicas, 61
    are FITS and 86 ran out of a resource with the second replica (hugepages 10, GPU 17, CPU 10, NIC 20, PCI 22, NUMA 7); no FITS
    pair is below the cap."""
    want = refans.take(lambda: lc.reference_synth(refans.ref, 4, cap=2))
    got, answers = lc.matcher_synth(_twin, 4, cap=2)
    lc.same_where_not_stopped(answers, want)
    lc.check_identities(got, hc.SYNTH_NODES)
    k, stopped, st = _reference_keeps_its_promises(want, 2)
    k37, stopped37, st37 = _pairs(lc.stored("test_synth_configurations[4]"))
    assert not stopped.any() and not stopped37.any()
    assert np.array_equal(st == lc.FITS, (k == 2) & (k37 > 2))
    assert np.array_equal(st[k37 <= 2], st37[k37 <= 2]) and np.array_equal(k, np.minimum(k37, 2))   # a run the cap did not cut ends as without it
    assert (st == lc.FITS).sum() >= 10 and all(h.saturated == int((h.per_node == 2).sum()) for h in got)
