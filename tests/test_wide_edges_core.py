"""The kernel's own per-record loop (wide_room_kernel.h wide_room_run_wave, on emulated lanes: tests/harness/wide_room_wave_emul.cpp)
against the scalar twin on the edge inputs of tests/wide_edge_check.py: runs that end STOPPED - the branch behind `status !=
kCommitOk`, with and without replicas in front of the flag - and shared NICs whose count the rounding of a binary64 addition decides."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from tests import headroom_general_check as gc
from tests import util
from tests import wide_edge_check as ec
from tests.harness import headroom_general_twin as gt
from tests.harness.explain_twin import ExplainHarnessEngine
from tests.harness.headroom_general_twin import HeadroomGeneralHarnessEngine
from workload import refmodel

COUNT, STOPPED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED


def _twin(clock=util.CLOCK):
    return HipMatcher(clock=lambda: clock, engine_factory=HeadroomGeneralHarnessEngine)


@pytest.mark.parametrize("name", ec.CASES + ["seam65"])
def test_emulated_lanes_equal_the_scalar_twin(name):
    """Every (template, wide record) of the case: the entry of the 64 emulated lanes is the scalar loop's - count and flag, field for
    field - and the scalar loop's is the reference's stored one (so the comparison is about the inputs it is meant to be about)."""
    sharing, descs, specs, cap, sel = ec.case(name)
    m, got, entries = gc.matcher_entries(_twin, descs, specs, sharing, util.CLOCK, cap=cap)
    wide, share = m.engine._wide_records(), m.engine._share_records()
    assert (share is not None) == sharing and len(wide) == len(sel)
    assert wide["index"].tolist() == sel
    with gc.sharing_all(sharing):
        reqs = m.packer.digest_many([refmodel.make_topology(s) for s in specs])
    lanes = gt.wide_room_wave(m.packer, wide, share, reqs, max_per_node=cap)
    scalar = np.asarray(entries)[:, wide["index"]].astype(np.uint16)
    assert np.array_equal(lanes, scalar)
    assert scalar.tolist() == ec.stored(name)
    if name not in ("bandwidth", "split"):
        flagged = lanes[(lanes & STOPPED) != 0]
        assert len(flagged) >= 3 and ((flagged & COUNT) >= 1).any()
    else:
        assert not (lanes & STOPPED).any() and ((lanes & COUNT) > 1).sum() >= 6


class _EveryPathEngine(HeadroomGeneralHarnessEngine, ExplainHarnessEngine):
    """The host builds of find, commit and batch, of headroom_general() and of explain() in one engine."""


@pytest.mark.parametrize("walk", ec.WALKS, ids=ec.WALK_IDS)
def test_every_path_prices_a_shared_nic_alike(walk):
    """The host builds of the find, commit, explain, batch and headroom paths on one node of set C (wide_edge_check.check_shared_nic_walk;
    tests/test_wide_edges_gpu.py puts the device through the same)."""
    ec.check_shared_nic_walk(lambda clock: HipMatcher(clock=lambda: clock, engine_factory=_EveryPathEngine), *ec.walk_pair(*walk))
