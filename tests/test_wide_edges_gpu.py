"""The edge inputs of tests/wide_edge_check.py on the MI355X (`pytest -m gpu`): k_wide_room's entries for runs that end STOPPED - alone,
beside a template that runs the same node to exhaustion, on both sides of a 64-slot chunk seam - and for shared NICs whose count the
rounding of a binary64 addition decides, against the reference's stored answers
(tests/golden/refanswers/tests.test_wide_edges_reference.json) and the host twin; every other path that prices a shared NIC - find,
commit, explain, batch, a re-pack - on the same nodes; shards and the group entry; the absence of side effects around a call that
returned STOPPED entries.  All comparisons are integer or byte equality.  Nothing here reads the reference tree."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import Engine
from nhd_amd.matcher import HipMatcher
from tests import headroom_general_check as gc
from tests import util
from tests import wide_edge_check as ec
from tests.harness.headroom_general_twin import HeadroomGeneralHarnessEngine
from tests.test_headroom_general_gpu import _same
from workload import refmodel

COUNT, STOPPED, NOT_EVALUATED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED, pack.HEADROOM_NOT_EVALUATED


def _device(clock=util.CLOCK):
    return HipMatcher(device=0, clock=lambda: clock)


def _twin(clock=util.CLOCK):
    return HipMatcher(clock=lambda: clock, engine_factory=HeadroomGeneralHarnessEngine)


# ---- 1. the stored reference answers and the twin ----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ec.CASES + ["seam65"])
def test_entries_equal_the_reference_and_the_twin(name):
    """Count and flag of every (template, node) the case holds to the reference are the reference's; every field of every summary is
    the twin's (`stopped`, `replicas` with the counts in front of a flag, `saturated`); the wide launch ran."""
    sharing, descs, specs, cap, sel = ec.case(name)
    md, dev, entries = gc.matcher_entries(_device, descs, specs, sharing, util.CLOCK, cap=cap)
    assert md.unmirrored == {} and md.wide_nodes == [descs[i]["name"] for i in sel]
    want = ec.stored(name)
    assert [[row[i] for i in sel] for row in entries] == want
    mt, twin, _ = gc.matcher_entries(_twin, descs, specs, sharing, util.CLOCK, cap=cap)
    _same(dev, twin)
    assert all(h.form & pack.HEADROOM_FORM_WIDE and h.not_evaluated == 0 for h in dev)
    w = np.asarray(want)
    assert sum(h.stopped for h in dev) >= int((w & STOPPED != 0).sum()) and sum(h.replicas for h in dev) >= int((w & COUNT).sum()) > 0
    assert name in ("bandwidth", "split") or (w & STOPPED).any()


# ---- 2. the seam under two bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cap", [2, 37])
@pytest.mark.parametrize("name", ["seam", "seam65"])
def test_stopped_records_on_both_sides_of_the_chunk_seam(name, cap):
    """STOPPED records at wide slots 0, 63 and 64 - one of them behind two replicas, which the bound 2 turns into a saturated run that
    never reaches its failing commit: entries and sums are the twin's, the flag stays on its own record (the record behind it has
    room and no flag), and the ordinary nodes' entries are nhdfit_headroom's byte for byte."""
    sharing, descs, specs, _, sel = ec.case(name)
    md, dev, entries = gc.matcher_entries(_device, descs, specs, sharing, util.CLOCK, cap=cap)
    mt, twin, _ = gc.matcher_entries(_twin, descs, specs, sharing, util.CLOCK, cap=cap)
    assert md.wide_nodes == mt.wide_nodes == [descs[i]["name"] for i in sel] and len(sel) == (65 if name == "seam65" else 66)
    _same(dev, twin)
    ref = ec.stored(name)
    for t, slot in enumerate(ec.SEAM_SLOTS):
        e = entries[t][sel[slot]]
        if ref[t][slot] & COUNT >= cap:
            assert e == cap                                    # (the bound comes first)
        else:
            assert e == ref[t][slot] and e & STOPPED
        if slot + 1 < len(sel):
            after = entries[t][sel[slot + 1]]
            assert after == min(ref[t][slot + 1], cap) and after & COUNT >= 1
    wide = np.zeros(len(descs), bool)
    wide[sel] = True
    nl = util.build_cluster(descs)
    plain = md.HeadroomMany(nl, [refmodel.make_topology(s) for s in specs], per_node=True, max_per_node=cap)
    for a, b in zip(plain, dev):
        assert a.per_node[~wide].tobytes() == b.per_node[~wide].tobytes() and a.flags[~wide].tobytes() == b.flags[~wide].tobytes()
        assert (a.flags[wide] == NOT_EVALUATED).all() and a.not_evaluated == len(sel) and b.not_evaluated == 0
    assert sum(int(h.per_node[~wide].sum()) for h in dev) > 0


# ---- 3. every path that prices a shared NIC ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("walk", ec.WALKS, ids=ec.WALK_IDS)
def test_every_path_prices_a_shared_nic_alike(walk):
    """wide_edge_check.check_shared_nic_walk on the device: find after commits, explain (the register restatement of explain_core.h),
    headroom, batch and a re-pack from CPython's own additions, against the reference's stored count of the pair."""
    ec.check_shared_nic_walk(_device, *ec.walk_pair(*walk))


# ---- 4. shards and the group entry ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stopped_off", "stopped_on", "bandwidth"])
def test_three_shards_and_the_group_entry_equal_one_context(name):
    """The case's nodes spread over a 150-node cluster, so that each of three contexts on device 0 answers for some of them: their
    entries are still the reference's, and three shards and HipMatcher(devices=[0]) - nhdfit_group_headroom_general - give every field
    one context gives."""
    sharing, descs, specs, cap, sel = ec.case(name)
    descs, at = ec.spread(descs)
    _, one, entries = gc.matcher_entries(_device, descs, specs, sharing, util.CLOCK, cap=cap)
    assert [[row[i] for i in at] for row in entries] == ec.stored(name)
    three, got3, _ = gc.matcher_entries(lambda clock: HipMatcher(devices=[0, 0, 0], engine_factory=Engine, clock=lambda: clock), descs, specs,
                                        sharing, util.CLOCK, cap=cap)
    assert len(three.engine.shards) == 3 and all(s.n_wide > 0 for s in three.engine.shards)
    assert {i // 64 for i in at} == {0, 1, 2}
    _same(one, got3)
    _, group, _ = gc.matcher_entries(lambda clock: HipMatcher(devices=[0], clock=lambda: clock), descs, specs, sharing, util.CLOCK, cap=cap)
    _same(one, group)


# ---- 5. no trace -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["stopped_off", "stopped_on", "seam"])
def test_a_call_that_returns_stopped_entries_leaves_no_trace(name):
    """Planes, wide records, share records and nhdfit_get_stats are byte for byte what they were; a FindNodes behind the call answers
    what it answered in front of it."""
    sharing, descs, specs, cap, sel = ec.case(name)
    with gc.sharing_all(sharing):
        nl = util.build_cluster(descs)
        tops = [refmodel.make_topology(s) for s in specs]
        m = _device()
        found = m.FindNodes(nl, tops)
        eng = m.engine
        fields = ("p0", "p1", "p2", "p3", "p4", "detail")
        planes = [np.array(getattr(eng.download(), f)) for f in fields]
        wide, share, st0 = eng.wide_download().copy(), (eng.wide_share_download().copy() if sharing else None), eng.stats()
        got = m.HeadroomMany(nl, tops, per_node=True, max_per_node=cap, general=True)
        st1 = eng.stats()
        assert sum(h.stopped for h in got) >= 3 and any(h.stopped and h.replicas for h in got) and len(wide) == len(sel)
        for f in ("launches", "fit_ms_total", "fit_ms_last", "digest_ms_last", "step_ms_last", "evals_last", "bytes_last", "small_finds", "batch_finds",
                  "big_nic_steps_max"):
            assert getattr(st0, f) == getattr(st1, f), f
        for a, b in zip(planes, [np.array(getattr(eng.download(), f)) for f in fields]):
            assert a.tobytes() == b.tobytes()
        assert eng.wide_download().tobytes() == wide.tobytes()
        if sharing:
            assert eng.wide_share_download().tobytes() == share.tobytes()
        assert m.FindNodes(nl, tops) == found
    assert any(r[0] is not None for r in found)
