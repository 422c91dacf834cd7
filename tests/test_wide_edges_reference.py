"""The edge inputs of tests/wide_edge_check.py - wide records whose run ends STOPPED, such records on both sides of a 64-slot chunk
seam, shared NICs whose count is decided by binary64 rounding - through the host twin (HeadroomGeneralHarnessEngine) against headroom
as the UNMODIFIED reference defines it (tests/headroom_reference.py; live where the reference tree exists, its stored answers
elsewhere) and against the independent oracle.  Count AND stopped flag of every (template, node) agree; no pair is skipped.  What
the inputs are meant to be is asserted here from the reference's answers (and fractions.Fraction) alone; the stored answers are what
tests/test_wide_edges_gpu.py holds the device to."""
from fractions import Fraction

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from tests import headroom_general_check as gc
from tests import util
from tests import wide_edge_check as ec
from tests.harness.headroom_general_twin import HeadroomGeneralHarnessEngine
from tests.test_headroom_general_reference import _consistent
from workload.refmodel import NFD

COUNT, STOPPED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED


def _twin(clock):
    return HipMatcher(clock=lambda: clock, engine_factory=HeadroomGeneralHarnessEngine)


def _stopped_set_is_what_it_should_be(want, sharing):
    """A: template 2i ends node i STOPPED, template 2i + 1 runs it to exhaustion; twelve pairs, both map types, three and four
    NUMA nodes, a template of several groups, three pairs with replicas in front of the flag, one of them with two."""
    descs, specs = ec.stopped_case(sharing)
    flagged = [want[2 * i][i] for i in range(len(descs))]
    assert len(flagged) >= 12 and all(e & STOPPED for e in flagged)
    assert all(not want[2 * i + 1][i] & STOPPED and want[2 * i + 1][i] & COUNT >= 1 for i in range(len(descs)))   # (never a property of the node)
    assert {specs[2 * i]["map_type"] for i in range(len(descs))} == {"PCI", "NUMA"}
    assert {3, 4} <= {int(d["labels"][NFD + "nfd-extras-cpu.numSockets"]) for d in descs}
    assert any(len(specs[2 * i]["groups"]) > 1 for i in range(len(descs)))
    counts = [e & COUNT for e in flagged]
    assert sum(k >= 1 for k in counts) >= 3 and max(counts) >= 2, counts


def _seam_is_what_it_should_be(want):
    """B: STOPPED at wide slots 0, 63 and 64 under the slot's own template, one of them behind replicas; the record behind each has
    room under that template and no flag."""
    for t, slot in enumerate(ec.SEAM_SLOTS):
        assert want[t][slot] & STOPPED, (t, slot)
        assert want[t][slot + 1] & COUNT >= 1 and not want[t][slot + 1] & STOPPED, (t, slot)
    assert any(want[t][slot] & COUNT >= 1 for t, slot in enumerate(ec.SEAM_SLOTS))
    assert len(want[0]) == 66


def _bandwidth_is_what_it_should_be(want):
    """C: per direction, six (NIC, demand) pairs whose count differs from exact arithmetic - the shortest of at most five replicas -
    six that agree, four of them with the last replica exactly on the capacity; two-group templates that differ, that agree, and
    that differ from themselves in the other group order; two NICs filled one after the other."""
    tpl = ec.bw_templates()
    single = list(enumerate(ec.BW_SPEEDS))                    # (node index, Gb/s) of the one-NIC nodes
    for kind in ("rx", "tx", "both"):
        differ, agree, landed = [], [], 0
        for (k, demands), row in zip(tpl, want):
            if k != kind or demands in [(d,) for d in ec.BW_ASYMMETRIC]:
                continue
            for i, s in single:
                assert not row[i] & STOPPED
                exact = ec.exact_count([s], demands)
                if exact >= ec.BW_CAP:
                    continue
                (differ if row[i] != exact else agree).append(row[i])
                need = max(Fraction(repr(demands[0][0])), Fraction(repr(demands[0][1])))
                landed += row[i] == exact and (Fraction(9, 10) * s) % need == 0
        assert len(differ) >= 6 and len(agree) >= 6 and landed >= 4 and min(differ) <= 5, (kind, differ, agree, landed)
    two = {(s, demands[0][0], demands[1][0]): (row[i], ec.exact_count([s], demands))
           for (k, demands), row in zip(tpl, want) if k == "two" for i, s in single}
    assert sum(a != b for a, b in two.values()) >= 2 and sum(a == b for a, b in two.values()) >= 2
    assert two[(100, 7.2, 1.8)][0] != two[(100, 1.8, 7.2)][0]   # (the same two demands: the order of the additions decides)
    fills = 0
    for (k, demands), row in zip(tpl, want):                  # (e) 40 G, then 100 G: the sum of the two NICs' own runs
        if k == "rx" and row[1] + row[2] < ec.BW_CAP:
            assert row[4] == row[1] + row[2]
            fills += 1
    assert fills >= 6
    assert max(max(row) for row in want) == ec.BW_CAP          # (the bound is reached, and nothing runs past about 100 replicas)


def _split_is_what_it_should_be(want):
    """(f) the last replica of a group of two pairs lands on the capacity: 8 x (2.5 + 2.0) = 36, 9 x (2.25 + 0.25) = 22.5."""
    assert [want[0][0], want[1][1], want[2][0], want[3][1]] == [8, 9, 8, 9]


@pytest.mark.parametrize("name", ec.CASES)
def test_reference(refans, name):
    sharing, descs, specs, cap, sel = ec.case(name)
    part = [descs[i] for i in sel]
    want = refans.take(lambda: gc.reference_entries(refans.ref, part, specs, sharing, util.CLOCK, cap=cap))
    if name.startswith("stopped"):
        _stopped_set_is_what_it_should_be(want, sharing)
    elif name == "seam":
        _seam_is_what_it_should_be(want)
    elif name == "bandwidth":
        _bandwidth_is_what_it_should_be(want)
    else:
        _split_is_what_it_should_be(want)
    assert gc.oracle_entries(part, specs, sharing, util.CLOCK, cap=cap) == want
    for variant in ([name, "seam65"] if name == "seam" else [name]):
        sharing, descs, specs, cap, sel = ec.case(variant)
        m, got, entries = gc.matcher_entries(_twin, descs, specs, sharing, util.CLOCK, cap=cap)
        assert m.unmirrored == {}
        assert m.wide_nodes == [descs[i]["name"] for i in sel]   # (every node held to the reference is a wide record, in this order)
        assert [[row[i] for i in sel] for row in entries] == (want if variant == name else [row[:-1] for row in want])
        _consistent(got, entries, cap)
        assert all(h.form & pack.HEADROOM_FORM_WIDE for h in got)
        e = np.asarray(entries)
        assert sum(h.stopped for h in got) == int((e & STOPPED != 0).sum()) and sum(h.replicas for h in got) == int((e & COUNT).sum())
    if name != "split" and name != "bandwidth":
        assert (np.asarray(want) & STOPPED).any()
