"""nhdfit_headroom_general on the MI355X (`pytest -m gpu`): k_wide_room's entry for every (template, wide record) against the
reference's stored answers (tests/golden/refanswers/tests.test_headroom_general_reference.json), against the host twin across the
64-slot chunk and ticket seams, on one and on no wide record, on an ENABLE_SHARING mirror; the planes' entries byte for byte
nhdfit_headroom's; candidate mask, node groups, shards and the group entry; the absence of side effects; the two consequences of
the definition; and k_wide_room's resources (hipcc only, no GPU).  Nothing here reads the reference tree."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import Engine
from nhd_amd.matcher import HipMatcher
from oracle import nhd_oracle as O
from tests import headroom_general_check as gc
from tests import util
from tests.harness.headroom_general_twin import HeadroomGeneralHarnessEngine
from workload import refmodel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNT, STOPPED, NOT_EVALUATED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED, pack.HEADROOM_NOT_EVALUATED


def _device(clock=util.CLOCK):
    return HipMatcher(device=0, clock=lambda: clock)


def _twin(clock=util.CLOCK):
    return HipMatcher(clock=lambda: clock, engine_factory=HeadroomGeneralHarnessEngine)


def _same(a, b):
    for x, y in zip(a, b):
        assert x.error is None and y.error is None
        assert np.array_equal(x.per_node, y.per_node) and np.array_equal(x.flags, y.flags)
        assert (x.replicas, x.nodes_with_room, x.max_on_one_node, x.saturated, x.stopped, x.not_evaluated, x.form) == \
               (y.replicas, y.nodes_with_room, y.max_on_one_node, y.saturated, y.stopped, y.not_evaluated, y.form)


def mask_words(keep, extra_high_bits=False):
    n = len(keep)
    bits = np.zeros(((n + 63) // 64) * 64, bool)
    bits[:n] = keep
    if extra_high_bits:
        bits[n:] = True
    return np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))


# ---- the stored reference answers --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(gc.CLUSTERS))
def test_cluster_entries_equal_the_reference(name):
    sharing, descs, wide_only = gc.cluster_case(name)
    sel = gc.selection(descs, wide_only)
    m, got, entries = gc.matcher_entries(_device, descs, gc.templates(), sharing, util.CLOCK)
    assert [[row[i] for i in sel] for row in entries] == gc.stored(f"test_clusters[{name}]")
    assert all(h.not_evaluated == 0 and h.form & pack.HEADROOM_FORM_WIDE for h in got)


@pytest.mark.gpu
@pytest.mark.parametrize("fixture,with_groups", gc.FIXTURE_CASES, ids=[f"{f}-{'groups' if g else 'plain'}" for f, g in gc.FIXTURE_CASES])
def test_fixture_entries_equal_the_reference(fixture, with_groups):
    case, specs, groups, sharing = gc.load_fixture(gc.FIXTURES[gc.FIXTURE_IDS.index(fixture)])
    want = gc.stored(f"test_fixtures[{fixture}-{'groups' if with_groups else 'plain'}]")
    m, got, entries = gc.matcher_entries(_device, case["nodes"], specs, sharing, case["clock"], pod_groups=groups if with_groups else None)
    assert m.unmirrored == {} and entries == want
    assert all(h.not_evaluated == 0 for h in got)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["mixed", "sharing_random"])
def test_a_template_that_asks_for_nothing_saturates(name):
    sharing, descs, _ = gc.cluster_case(name)
    m, got, entries = gc.matcher_entries(_device, descs, [gc.NOTHING], sharing, util.CLOCK)
    assert entries == gc.stored(f"test_a_template_that_asks_for_nothing_saturates[{name}]")
    assert got[0].saturated == entries[0].count(gc.CAP) > len(descs) // 2 and got[0].max_on_one_node == gc.CAP


# ---- the host twin: chunk and ticket seams, one and no wide record, a sharing mirror -----------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cap", [2, 37])
@pytest.mark.parametrize("n_wide,n_plain", [(65, 135), (129, 201), (1, 70)], ids=["65-of-200", "129-of-330", "1-of-71"])
def test_device_equals_the_twin_across_the_seams(n_wide, n_plain, cap):
    """65 and 129 wide records - one past a 64-slot chunk, one past two: the ticket seams - and a single one, among ordinary nodes:
    every entry and every sum equals the twin's; the planes' entries are byte for byte nhdfit_headroom's on the same mirror."""
    descs = gc.seam_descs(9880, n_wide, n_plain)
    md, dev, _ = gc.matcher_entries(_device, descs, gc.FOUR, False, util.CLOCK, cap=cap)
    mt, twin, _ = gc.matcher_entries(_twin, descs, gc.FOUR, False, util.CLOCK, cap=cap)
    assert len(md.wide_nodes) == n_wide and md.wide_nodes == mt.wide_nodes
    _same(dev, twin)
    wide = np.array([d["name"] in set(md.wide_nodes) for d in descs])
    assert n_wide == 1 or sum(int(h.per_node[wide].sum()) for h in dev) > n_wide // 2
    nl = util.build_cluster(descs)
    plain = md.HeadroomMany(nl, [refmodel.make_topology(s) for s in gc.FOUR], per_node=True, max_per_node=cap)
    for a, b in zip(plain, dev):
        assert a.per_node[~wide].tobytes() == b.per_node[~wide].tobytes() and a.flags[~wide].tobytes() == b.flags[~wide].tobytes()
        assert (a.flags[wide] == NOT_EVALUATED).all() and a.not_evaluated == n_wide and b.not_evaluated == 0


@pytest.mark.gpu
def test_no_wide_record_is_byte_equal_to_headroom():
    """A mirror without wide records: sums (`form` included) and entries are nhdfit_headroom's byte for byte."""
    descs = gc.seam_descs(9880, 0, 70)
    m, got, _ = gc.matcher_entries(_device, descs, gc.FOUR, False, util.CLOCK)
    reqs = m.packer.digest_many([refmodel.make_topology(s) for s in gc.FOUR])
    s0, c0 = m.engine.headroom(reqs, max_per_node=gc.CAP, per_node=True)
    s1, c1 = m.engine.headroom_general(reqs, max_per_node=gc.CAP, per_node=True)
    assert m.engine.n_wide == 0 and s0.tobytes() == s1.tobytes() and c0.tobytes() == c1.tobytes()
    assert int(s1["replicas"].sum()) == sum(h.replicas for h in got) > 50


@pytest.mark.gpu
def test_a_sharing_mirror_of_130_nodes():
    """ENABLE_SHARING: every node a wide record with its share record (three chunks, the last of two slots)."""
    descs = util.mixed_cluster_desc(9890, 130, occupancy=0.1)
    md, dev, _ = gc.matcher_entries(_device, descs, gc.FOUR + [gc.NOTHING], True, util.CLOCK)
    mt, twin, _ = gc.matcher_entries(_twin, descs, gc.FOUR + [gc.NOTHING], True, util.CLOCK)
    assert len(md.wide_nodes) == 130
    _same(dev, twin)
    assert sum(h.replicas for h in dev[:4]) > 200 and max(h.max_on_one_node for h in dev[:4]) > 2


# ---- candidate mask, node groups, shards, the group entry ------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_candidate_mask_and_node_groups():
    """Outside the mask every entry is 0 - a wide record's as well - inside it is the unmasked entry; bits past the last node change
    nothing.  With the pods' node groups the nodes InitialNodeFilter drops have 0 and the others their entry without the filter."""
    descs = gc.seam_descs(9880, 65, 136)
    nl = util.build_cluster(descs)
    tops = [refmodel.make_topology(s) for s in gc.FOUR]
    m = _device()
    full = m.HeadroomMany(nl, tops, per_node=True, max_per_node=gc.CAP, general=True)
    reqs = m.packer.digest_many(tops)
    n = len(nl)
    keep = np.random.default_rng(9881).random(n) < 0.6
    s0, c0 = m.engine.headroom_general(reqs, max_per_node=gc.CAP, per_node=True)
    assert [row.tolist() for row in c0] == [(h.per_node | h.flags).tolist() for h in full]
    for high in (False, True):
        s1, c1 = m.engine.headroom_general(reqs, cand=mask_words(keep, high), max_per_node=gc.CAP, per_node=True)
        assert np.array_equal(c1, np.where(keep[None, :], c0, 0))
        assert np.array_equal(s1["replicas"], (c1 & COUNT).sum(1, dtype=np.uint64)) and (s1["not_evaluated"] == 0).all()
        assert np.array_equal(s1["nodes_with_room"], ((c1 & COUNT) > 0).sum(1)) and np.array_equal(s1["max_on_one_node"], (c1 & COUNT).max(1))
    wide = np.array([nm in set(m.wide_nodes) for nm in nl])
    assert (c0[:, wide & ~keep] > 0).any()
    rng = np.random.default_rng(9882)
    groups = [list(rng.choice(["default", "alpha", "beta"], size=int(rng.integers(1, 3)), replace=False)) for _ in tops]
    grouped = m.HeadroomMany(nl, tops, pod_groups=groups, per_node=True, max_per_node=gc.CAP, general=True)
    dropped = 0
    for h, f, g in zip(grouped, full, groups):
        inside = np.array([nm in set(O.initial_node_filter(nl, g)) for nm in nl])
        assert np.array_equal(h.per_node, np.where(inside, f.per_node, 0)) and h.not_evaluated == 0
        dropped += int((f.per_node[wide & ~inside] > 0).sum())
    assert dropped > 0


@pytest.mark.gpu
def test_three_shards_and_the_group_entry_equal_one_device():
    """Three contexts on device 0, each with its own wide records, and HipMatcher(devices=[0]) - the group entry,
    nhdfit_group_headroom_general - give what one context gives."""
    nl = util.mixed_cluster(9883, 330, occupancy=0.1)           # (wide nodes all along the node axis: in every shard)
    tops = [refmodel.make_topology(s) for s in gc.FOUR]
    one = _device().HeadroomMany(nl, tops, per_node=True, max_per_node=gc.CAP, general=True)
    three = HipMatcher(devices=[0, 0, 0], engine_factory=Engine, clock=lambda: util.CLOCK)
    assert len(three.engine.shards) == 3
    _same(one, three.HeadroomMany(nl, tops, per_node=True, max_per_node=gc.CAP, general=True))
    assert all(s.n_wide > 0 for s in three.engine.shards)
    _same(one, HipMatcher(devices=[0], clock=lambda: util.CLOCK).HeadroomMany(nl, tops, per_node=True, max_per_node=gc.CAP, general=True))
    assert sum(h.replicas for h in one) > 100


# ---- no side effects ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
def test_headroom_general_leaves_no_trace(sharing):
    """The planes, the wide records, the share records and nhdfit_get_stats are identical before and after, and a FindNodes behind
    the call answers what it answered in front of it."""
    descs = util.mixed_cluster_desc(9891, 90, occupancy=0.1)
    with gc.sharing_all(sharing):
        nl = util.build_cluster(descs)
        tops = [refmodel.make_topology(s) for s in gc.FOUR]
        m = _device()
        found = m.FindNodes(nl, tops)
        eng = m.engine
        planes = [np.array(getattr(eng.download(), f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
        wide, share, st0 = eng.wide_download().copy(), (eng.wide_share_download().copy() if sharing else None), eng.stats()
        got = m.HeadroomMany(nl, tops, per_node=True, max_per_node=gc.CAP, general=True)
        st1 = eng.stats()
        assert sum(h.replicas for h in got) > 50 and len(wide) > 10
        for f in ("launches", "fit_ms_total", "fit_ms_last", "digest_ms_last", "step_ms_last", "evals_last", "bytes_last", "small_finds", "batch_finds",
                  "big_nic_steps_max"):
            assert getattr(st0, f) == getattr(st1, f), f
        for a, b in zip(planes, [np.array(getattr(eng.download(), f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]):
            assert a.tobytes() == b.tobytes()
        assert eng.wide_download().tobytes() == wide.tobytes()
        if sharing:
            assert eng.wide_share_download().tobytes() == share.tobytes()
        assert m.FindNodes(nl, tops) == found
    assert any(r[0] is not None for r in found)


# ---- the two consequences ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
def test_sum_is_what_schedule_batch_places(sharing):
    gc.check_sum_is_what_schedule_batch_places(_device, sharing)


@pytest.mark.gpu
@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
def test_a_commit_on_a_wide_winner_takes_one(sharing):
    gc.check_a_commit_on_a_wide_winner_takes_one(_device, sharing)


# ---- resources (no GPU needed) -----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_wide_room_kernel_resources(tmp_path):
    """Exactly one function is k_wide_room, and its LDS leaves room for two blocks on a CU (at most 80 KB; three fit).  Private
    segment and spills are printed, not pinned (profiles/r12/README.md records them)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "nhd_amd", "csrc", "nhdfit.hip")
    res = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--cuda-device-only", "-c", src,
                          "-o", str(tmp_path / "dev.o"), "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-2000:]
    usage, name = {}, None
    for line in res.stderr.splitlines():
        mt = re.search(r"Function Name: (\S+)", line)
        if mt:
            name = mt.group(1)
            usage[name] = {}
            continue
        mt = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\d+)", line)
        if mt and name:
            usage[name][mt.group(1).strip()] = int(mt.group(2))
    ours = {k: v for k, v in usage.items() if "k_wide_room" in k}
    assert len(ours) == 1, list(usage)
    (k, v), = ours.items()
    print(k, v)
    assert 0 < v["LDS Size"] <= 80 * 1024, v
    for other in ("k_headroom", "k_explain", "k_limit_stage", "k_find", "k_map_tiles", "k_step"):
        assert other not in k
