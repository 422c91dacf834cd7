"""The DEVICE at the edges of the record formats (`pytest -m gpu`; workload/edge_inputs.py draws the inputs, tests/edge_check.py holds the
checks the CPU suite runs on the host twins): sockets whose core masks use bits 32..63, 9..16 NICs and 8 GPUs per NUMA node, up to
14 switches, pods_used of 2..3, free hugepages around the tile's table, NIC speeds at the 11 000 Mb/s threshold, rx values on either
side of the speed * 0.9 capacities.  Everything goes ctypes -> C-ABI on device 0, against the Python oracle, the C oracle and the
independent headroom oracle; nothing here reads the reference tree.

(a) tools/soak_extreme.py's own checks - FindNodes, filtered FindNode, ScheduleBatch, op streams, the three-shard legs on three
    contexts of device 0 - over three short seed ranges;
(b) every form of find on ONE 600-node edge cluster (ten chunks, 126 wide nodes): the staged path, three pipelined steps, the
    general path's pods, and - on a second context that holds the 474 fast-layout nodes, because a mirror with wide records takes
    neither single-launch form - the single-launch batch, and on a third without the three NIC-heavy nodes whose signatures keep
    the dictionary out of a block's LDS the one-pod launch; unmasked, then with candidate masks that keep only the nodes with
    33..64 cores per socket, then only the NIC-heavy ones;
(c) nhdfit_explain / nhdfit_explain_big over all 57 600 pairs;  (d) nhdfit_headroom and nhdfit_headroom_limits for four templates, on the
    whole cluster (its dictionary is read from global memory) and without those three nodes (the dictionary staged in LDS);
(e) ScheduleOne pod after pod on six 14-node edge clusters, the one-launch form (k_find1_commit) asserted by its counter.
Each test prints the figures that show it is not vacuous; the conditions on them are asserted."""
import importlib.util
import os

import numpy as np
import pytest

from nhd_amd import pack
from tests import edge_check as C
from workload import edge_inputs as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASKS = ["unmasked", "33..64 cores", "NIC-heavy"]


def _matcher(clock=None):
    from nhd_amd.matcher import HipMatcher
    return HipMatcher(device=0, clock=clock or (lambda: C.NOW))


# ---- (a) the soak's own checks -----------------------------------------------------------------------------------------------------------
SOAK_RANGES = [0, 5, 21]                                   # four seeds each


def test_the_soak_ranges_hold_every_kind_of_seed():
    """By the tool's own rules (edge_inputs.soak_draw; its op streams run on even seeds, its sharded legs on seed % 4 == 1)."""
    seeds = [s for first in SOAK_RANGES for s in range(first, first + 4)]
    drawn = {s: E.soak_draw(s) for s in seeds}
    assert any(d[1] > 0 for d in drawn.values())                                # a NIC-heavy seed
    assert any(d[2] == 6 for d in drawn.values())                               # a six-group seed: the general path (k_big_eval)
    assert 24 in seeds and any(max(E.shape_of(x)[2]) > 16 for x in drawn[24][3])    # nodes no record holds
    assert sum(s % 2 == 0 for s in seeds) >= 2 and sum(s % 4 == 1 for s in seeds) >= 2


@pytest.mark.parametrize("first", SOAK_RANGES)
def test_the_soak_on_the_device(first):
    spec = importlib.util.spec_from_file_location("soak_extreme", os.path.join(ROOT, "tools", "soak_extreme.py"))
    soak = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(soak)
    got = soak.run(4, first, device=True)
    print("edge soak on the device:", got)
    assert got["mismatches"] == 0
    assert got["pods"] == 64 and got["placed"] > 0 and got["op_streams"] > 0 and got["sharded"] > 0
    if first == 21:
        assert got["unmirrored"] > 0


# ---- (b) every form of find on one cluster that spans tiles -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    return C.big_case()


@pytest.fixture(scope="module")
def whole(case):
    """The whole cluster on one context: fast-layout nodes in the planes, 126 wide records beside them."""
    m = _matcher()
    m._full_upload(case.nl)
    assert m._names == case.names and m.engine.wide_count() == int(case.wide.sum()) and not m.unmirrored
    yield m
    m.engine.close()


@pytest.fixture(scope="module")
def fast(case):
    """(matcher, indices): the fast-layout nodes alone - a mirror the single-launch forms of find accept."""
    ctx = np.flatnonzero(~case.wide)
    m = _matcher()
    m._full_upload({case.names[i]: case.nl[case.names[i]] for i in ctx})
    assert m.engine.wide_count() == 0 and not m.unmirrored
    yield m, ctx
    m.engine.close()


@pytest.fixture(scope="module")
def lone(case):
    """(matcher, indices): the fast-layout nodes whose dictionary - every NIC state a commit can produce interned, as the one-pod
    launches want it - fits a block's LDS (BigCase.fits_lds: three NIC-heavy nodes left out, fifteen stay)."""
    ctx = np.flatnonzero(~case.wide & case.fits_lds)
    m = _matcher()
    m._full_upload(case.sub(~case.wide & case.fits_lds))
    m.packer.close_signatures()
    m.engine.set_dictionary(m.packer)
    words, sigs = C.dict_stream(case.sub(~case.wide & case.fits_lds))
    assert words <= C.LONE_WORDS and sigs <= C.LONE_SIGS and m.engine.wide_count() == 0
    assert int((~case.fits_lds).sum()) <= 3 and int((case.heavy & case.fits_lds).sum()) >= 10
    yield m, ctx
    m.engine.close()


def test_the_oracle_alone_says_the_input_sits_at_the_edges(case):
    fig = case.figures()
    print("600-node edge cluster, by the C oracle alone:", fig)
    assert fig["33..64-core nodes"] >= 150 and fig["feasible pairs on 33..64-core nodes"] >= 500
    assert fig["NIC-heavy nodes"] >= 10 and fig["feasible pairs on NIC-heavy nodes"] >= 100
    assert fig["pods placed"] >= 70
    assert fig["pods placed on 33..64-core nodes only"] >= 20 and fig["pods placed on NIC-heavy nodes only"] >= 20
    assert fig["wide nodes"] >= 100 and fig["pods of the general path"] >= 5
    assert sum(1 for d in case.descs if E.nic_heavy(d) and max(E.shape_of(d)[2]) == 16) >= 1


def _keep(case, mask):
    return dict(C.masks_of(case))[mask]


@pytest.mark.parametrize("mask", MASKS)
def test_staged_find_on_the_whole_cluster(case, whole, mask):
    """nhdfit_find with a bitmap (the staged path: k_step's tiles, the wide pass behind them): every verdict, wide nodes' columns
    included, every winner, every winner's mapping; the pods of the general path (nhdfit_big_find) beside them."""
    keep = _keep(case, mask)
    cand = None if keep is None else E.mask_words(keep)
    ctx = np.arange(case.n)
    small = [p for p in range(case.PODS) if not case.general[p]]
    big = [p for p in range(case.PODS) if case.general[p]]
    reqs = whole.packer.digest_many([case.tops[p] for p in small])
    before = whole.engine.stats()
    score, bm, maps = whole.engine.find(reqs, C.NOW, cand=cand, want_bitmap=True, want_map=True)
    after = whole.engine.stats()
    assert (after.small_finds, after.batch_finds) == (before.small_finds, before.batch_finds) and after.launches > before.launches
    placed = C.check_find(case, ctx, small, keep, score, bm, maps, f"staged, {mask}")
    bigs = np.array([whole.packer.digest_big(case.tops[p]) for p in big], dtype=pack.BIG_REQ)
    score, maps = whole.engine.big_find(bigs, C.NOW, cand=cand)
    placed += C.check_find(case, ctx, big, keep, score, None, maps, f"general path, {mask}")
    print(f"staged find, {mask}: {len(small)} + {len(big)} pods, {placed} placed")
    assert placed >= (70 if keep is None else 20)


def test_three_pipelined_steps_fetched_afterwards(case, whole, fast):
    """nhdfit_stage_requests, three nhdfit_enqueue_step, nhdfit_fetch (the pipelined form takes no candidate mask): on the whole
    cluster and on the fast-layout nodes alone."""
    small = [p for p in range(case.PODS) if not case.general[p]]
    for m, ctx, tag in ((whole, np.arange(case.n), "whole"), (fast[0], fast[1], "fast layout")):
        reqs = m.packer.digest_many([case.tops[p] for p in small])
        m.engine.stage(reqs)
        for _ in range(3):
            m.engine.enqueue(C.NOW)
        score, bm, maps = m.engine.fetch(want_bitmap=True, want_map=True)
        placed = C.check_find(case, ctx, small, None, score, bm, maps, f"pipelined, {tag}")
        print(f"three pipelined steps, {tag}: {len(small)} pods, {placed} placed")
        assert placed >= 50


def _single_launch_pods(case):
    """The pods both single-launch forms take: at most three groups, the table-driven pass - of all 192, so that they are more than a tile."""
    pods = [p for p in range(case.ALL_PODS) if not case.general[p] and case.G[p] <= 3]
    assert len(pods) > 64
    return pods


@pytest.mark.parametrize("mask", MASKS)
def test_single_launch_batch(case, fast, mask):
    """nhdfit_find without a bitmap for more than a tile of pods (k_findn): `batch_finds` says the one launch ran."""
    m, ctx = fast
    keep = _keep(case, mask)
    pods = _single_launch_pods(case)
    reqs = m.packer.digest_many([case.tops[p] for p in pods])
    before = m.engine.stats()
    score, _, maps = m.engine.find(reqs, C.NOW, cand=None if keep is None else E.mask_words(keep[ctx]), want_bitmap=False, want_map=True)
    after = m.engine.stats()
    assert after.batch_finds == before.batch_finds + 1, "the single-launch batch form did not run"
    placed = C.check_find(case, ctx, pods, keep, score, None, maps, f"single-launch batch, {mask}")
    print(f"single-launch batch, {mask}: {len(pods)} pods, {placed} placed")
    assert placed >= 20


@pytest.mark.parametrize("mask", MASKS)
def test_one_pod_launch_for_each_pod(case, lone, mask):
    """nhdfit_find for one pod at a time on the mirror whose dictionary fits a block's LDS - the condition under which the call is
    the table-free launch (k_find1); on a larger dictionary it is the tile form with one pod.  `small_finds` counts every call."""
    m, ctx = lone
    keep = _keep(case, mask)
    cand = None if keep is None else E.mask_words(keep[ctx])
    pods = _single_launch_pods(case)
    reqs = m.packer.digest_many([case.tops[p] for p in pods])
    before = m.engine.stats()
    score, maps = np.zeros(len(pods), np.uint64), np.zeros(len(pods), pack.MAPPING)
    for k in range(len(pods)):
        s, _, mp = m.engine.find(reqs[k:k + 1], C.NOW, cand=cand, want_bitmap=False, want_map=True)
        score[k], maps[k] = s[0], mp[0]
    assert m.engine.stats().small_finds == before.small_finds + len(pods), "a one-pod find did not take the single launch"
    placed = C.check_find(case, ctx, pods, keep, score, None, maps, f"one-pod launch, {mask}")
    print(f"one-pod launches, {mask}: {len(pods)} pods, {placed} placed")
    assert placed >= 20


# ---- (c) explain ------------------------------------------------------------------------------------------------------------------------------
def test_explain_every_pair(case):
    m = _matcher()
    fig = C.check_explain(m, case)
    print("explain on the 600-node edge cluster:", fig)
    assert fig["pairs"] == 57600 and fig["pods of the general path"] >= 5
    m.engine.close()


# ---- (d) headroom and its limits -----------------------------------------------------------------------------------------------------------------
def test_headroom_and_its_limits(case):
    """Four templates (one each of 1..4 groups: the pod with the most feasible nodes) on the whole 600-node cluster, max_per_node=8:
    count, STOPPED flag and limit stage of every fast-layout node against independent_limit, NOT_EVALUATED exactly on the wide nodes,
    forms WAVE, WAVE, WAVE, GENERIC, 381 replicas by the oracle.  With every NIC state a commit can produce interned, this cluster's
    dictionary is a stream of 21 944 16-bit words (2 649 signatures; node e0297 with 15 + 8 NICs holds 13 094 of them) - beyond the
    6 144 words k_headroom stages in LDS: the blocks derive their template's masks off the stream in global memory.  (Until this
    test met it, such a dictionary made nhdfit_headroom return NHDFIT_E_LIMIT.)"""
    words, sigs = C.dict_stream(case.nl)
    assert words > C.LONE_WORDS and sigs <= C.LONE_SIGS
    m = _matcher()
    fig = C.check_headroom(m, case, cap=8)
    print("headroom on the 600-node edge cluster:", fig)
    assert fig["replicas"] >= 300
    m.engine.close()


def test_headroom_and_its_limits_with_the_dictionary_in_lds(case):
    """The same check on the 597 nodes whose dictionary fits the LDS slice (BigCase.fits_lds; all 126 wide nodes and 15 of the 18
    NIC-heavy ones are among them, three with 16 NICs on a NUMA node) - k_headroom's staged form at the edges: 354 replicas by the oracle."""
    words, sigs = C.dict_stream(case.sub(case.fits_lds))
    assert words <= C.LONE_WORDS and sigs <= C.LONE_SIGS
    m = _matcher()
    fig = C.check_headroom(m, case, cap=8, keep=case.fits_lds)
    print("headroom on the 597 nodes of the edge cluster whose dictionary fits LDS:", fig)
    assert fig["nodes"] >= 595 and fig["replicas"] >= 300
    m.engine.close()


# ---- (e) ScheduleOne ----------------------------------------------------------------------------------------------------------------------------
ONE_SEEDS = [0, 1, 5, 8, 16, 26]          # by the oracle alone: at least five pods placed in each, pods placed on 33..64-core nodes in each


@pytest.mark.parametrize("seed", ONE_SEEDS)
def test_schedule_one_pod_after_pod(seed):
    fig = C.check_schedule_one(_matcher, seed, fused_form=True)
    print("ScheduleOne at the edges:", fig)
    assert fig["pods"] >= 10 and fig["placed"] >= 5 and fig["fused"] > 0
    assert fig["placed on 33..64-core nodes"] >= 1
