"""Clusters and pods drawn at the EDGES of the record formats (tools/soak_extreme.py: 64- and 128-core sockets, 16 NICs / 8 GPUs per
NUMA node, a dozen NIC speeds, arbitrary isolcpus sets, busy times around the 30 s window, hugepage requests around the tile's table,
pods of 1..6 groups): the product's host build against the Python oracle - FindNodes, FindNode behind InitialNodeFilter, ScheduleBatch
with commits and ids, op streams mirrored as deltas - and, in the build container, against the unmodified reference.  The long
form is the tool itself (1 500 seeds / 24 000 pods / 739 op streams and 2 550 pods against the reference: no mismatch).
The entries the tool does not drive - ExplainNodes, Headroom with its limits, ScheduleOne - meet the same clusters below, on their
host twins against the C stage oracle, the independent headroom oracle and the Python oracle's loop, and a handful of seeds against
the unmodified reference; tests/test_format_edges_gpu.py holds the device to the same oracles (tests/edge_check.py has the checks)."""
import importlib.util
import os
import sys

import pytest

from nhd_amd.matcher import HipMatcher
from oracle import ref_loader
from tests import edge_check, harness, util
from workload import edge_inputs
from tests.harness.explain_twin import ExplainHarnessEngine
from tests.harness.headroom_limit_twin import HeadroomLimitHarnessEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def soak_module():
    spec = importlib.util.spec_from_file_location("soak_extreme", os.path.join(ROOT, "tools", "soak_extreme.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("first,with_ref", [(0, False), (21, False), (12000, True)])   # (seed 24: nodes beyond every record - never matched, the rest as the oracle says)
def test_edges_of_the_record_formats(monkeypatch, first, with_ref):
    if with_ref and not ref_loader.available():
        pytest.skip("reference tree not present (GPU box)")
    monkeypatch.setattr(sys, "argv", ["soak_extreme.py", "12", str(first)] + (["--ref"] if with_ref else []))
    assert soak_module().main() == 0


# the node descriptions and pod specs of three of the seeds above, as tools/soak_extreme.py drew them when its generators still lived in
# the tool itself (sha256 of their JSON form): the seeds the suite names stand for the same clusters as before the generators moved
DRAWS = {0: "370f3f070102df0b545ef05a261c2fda9d087c319cbf3fd0b2a122dc9cd2a7ba",
         21: "97b436bc99600273fcb4d06a49d2e94310f1479c668231bed707c72c4cd02e65",
         12000: "acdff0bd0e466b2810ac3ddac2972ed8792c90dd7a4c75f2bfee1f031413a45f"}


def test_the_named_seeds_stand_for_the_same_clusters():
    assert {seed: edge_inputs.draw_hash(seed) for seed in DRAWS} == DRAWS and edge_inputs.CLOCK == util.CLOCK
    soak = soak_module()                                  # the tool draws through the shared module
    assert soak.edge_node is edge_inputs.edge_node and soak.edge_pod is edge_inputs.edge_pod and soak.soak_draw is edge_inputs.soak_draw


class TwinEngine(HeadroomLimitHarnessEngine, ExplainHarnessEngine):
    pass


def _twin():
    return HipMatcher(clock=lambda: util.CLOCK, engine_factory=TwinEngine)


@pytest.mark.parametrize("first", [0, 12, 24])
def test_explain_and_headroom_limits_at_the_edges(first):
    """Twelve 14-node edge clusters each (seed 24 among them: nodes no record holds), 16 pods of up to four groups: every (pod, node)
    stage of ExplainNodes against the C stage oracle, count, STOPPED flag and limit stage of every fast-layout node from
    HeadroomMany(limits=True) - and the plain entry's figures - against independent_limit; wide nodes are NOT_EVALUATED and
    nothing else is."""
    tot = {}
    for seed in range(first, first + 12):
        for k, v in edge_check.check_new_entries(_twin(), seed).items():
            tot[k] = tot.get(k, 0) + v
    print(f"seeds {first}..{first + 11}:", tot)
    assert tot["pairs"] >= 12 * 13 * 16 and tot["fits"] >= 40 and tot["replicas"] >= 25 and tot["33..64-core nodes"] >= 30
    if first == 12:
        assert tot["stopped runs"] >= 1                   # (seed 22)
    if first == 24:
        assert tot["unmirrored"] >= 1


@pytest.mark.parametrize("seed", [2, 7, 22, 30, 33])
def test_explain_and_headroom_limits_at_the_edges_vs_reference(ref, seed):
    """The same two entries against the UNMODIFIED reference (its filter's own intermediate results, its own FindNode -> commit
    runs); seed 22 holds a run the reference ends by raising, 30 and 33 are NIC-heavy."""
    got = edge_check.check_new_entries_against_reference(ref, _twin(), seed)
    print(f"seed {seed}:", got)
    assert got["pairs through the reference's loop"] >= 80 and got["replicas"] >= 3


@pytest.mark.parametrize("seed", [0, 1, 5, 8, 16, 26])
def test_schedule_one_at_the_edges(seed):
    """The six clusters of the device test, pod after pod through ScheduleOne on the host engine (composed from FindNodes +
    CommitPlacement there) against the Python oracle's FindNode + commit loop."""
    got = edge_check.check_schedule_one(lambda clock: HipMatcher(clock=clock, engine_factory=harness.HarnessEngine), seed, fused_form=False)
    print(got)
    assert got["pods"] >= 10 and got["placed"] >= 5 and got["placed on 33..64-core nodes"] >= 1
