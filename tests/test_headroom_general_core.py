"""nhdfit_headroom_general's arithmetic and host logic on the CPU: the kernel's own per-record loop (wide_room_kernel.h
wide_room_run_wave: the stages with lane = tuple, the set model and the commit step on the first lane) on emulated lanes against the
scalar twin on the same records; what the opt-in changes (wide candidates get a figure and join the sums) and what it does not (the
nodes of the planes, a mirror without wide records, every default)."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.matcher import HipMatcher
from oracle import nhd_oracle as O
from tests import headroom_general_check as gc
from tests import util
from tests.harness import headroom_general_twin as gt
from tests.harness.headroom_general_twin import HeadroomGeneralHarnessEngine
from workload import refmodel

COUNT, STOPPED, NOT_EVALUATED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED, pack.HEADROOM_NOT_EVALUATED


def _twin(clock=util.CLOCK):
    return HipMatcher(clock=lambda: clock, engine_factory=HeadroomGeneralHarnessEngine)


def _specs(seed, count=12):
    """Templates of one to four groups, NUMA and PCI, one of an invalid map type among them."""
    rng = np.random.default_rng(seed)
    specs = [util.random_pod_spec(rng, max_groups=4) for _ in range(count)]
    for g, s in zip((1, 2, 3, 4), specs):                     # (every group count, whatever the draw)
        while len(s["groups"]) < g:
            s["groups"].append(dict(s["groups"][0]))
        del s["groups"][g:]
    specs[0]["map_type"], specs[1]["map_type"], specs[4]["map_type"] = "NUMA", "PCI", "NONE"
    return specs


def _same(a, b):
    for x, y in zip(a, b):
        assert x.error is None and y.error is None
        assert np.array_equal(x.per_node, y.per_node) and np.array_equal(x.flags, y.flags)
        assert x.summary() == y.summary() and x.form == y.form
        assert (x.replicas, x.nodes_with_room, x.max_on_one_node, x.saturated, x.stopped, x.not_evaluated, x.unmirrored) == \
               (y.replicas, y.nodes_with_room, y.max_on_one_node, y.saturated, y.stopped, y.not_evaluated, y.unmirrored)


# ---- the kernel's loop on emulated lanes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
@pytest.mark.parametrize("seed", [9810, 9811, 9812])
def test_emulated_lanes_equal_the_scalar_twin(seed, sharing):
    """wide_room_run_wave's text on 64 emulated lanes gives the scalar loop's entry for every (template, wide record): 1..4 NUMA nodes,
    sockets below 64, above 64 and of 128 cores, templates of 1..4 groups in NUMA, PCI and an invalid map type, the bound reached by
    some.  The lanes agree among themselves (the emulation reports it) and every ballot is reached by all of them (it would hang)."""
    descs = util.mixed_cluster_desc(seed, 36, wide_share=0.8 if sharing else 0.9, occupancy=0.1)
    specs = _specs(seed) + [gc.NOTHING]
    m, got, entries = gc.matcher_entries(_twin, descs, specs, sharing, util.CLOCK, cap=5)
    wide, share = m.engine._wide_records(), m.engine._share_records()
    assert (share is not None) == sharing and len(wide) >= 16
    reqs = m.packer.digest_many([refmodel.make_topology(s) for s in specs])
    assert sorted(set(reqs["n_groups"].tolist())) == [1, 2, 3, 4]
    assert {1, 2} < set(reqs["map_type"].tolist())                     # NHDFIT_MAP_NUMA, NHDFIT_MAP_PCI, and one that never matches
    lanes = gt.wide_room_wave(m.packer, wide, share, reqs, max_per_node=5)
    assert np.array_equal(lanes, np.asarray(entries)[:, wide["index"]].astype(np.uint16))
    k = lanes & COUNT
    assert (k > 0).sum() > 20 and (k > 1).sum() > 5 and (k == 5).sum() >= len(wide) // 2
    U, cpp = wide["numa_nodes"], wide["cores_per_proc"]
    room = (k[:-1] > 0).any(0)                                # (by a template that asks for something)
    assert set(U[room].tolist()) >= ({1, 2, 3, 4} if sharing else {3, 4}), sorted(set(U[room].tolist()))
    assert (cpp[room] < 64).any() or not sharing
    assert (cpp[room] > 64).any() and (cpp == 128).any()


# ---- what the opt-in changes, and what it does not ---------------------------------------------------------------------------------------
def test_without_wide_nodes_general_changes_nothing():
    """An ordinary cluster: general=True equals general=False in every field (the wide launch does not run: `form` has no wide bit)."""
    nl = util.random_cluster(9820, 60, occupancy=0.15)
    tops = [refmodel.make_topology(s) for s in _specs(9820)]
    m = _twin()
    a = m.HeadroomMany(nl, tops, per_node=True, max_per_node=9)
    b = m.HeadroomMany(nl, tops, per_node=True, max_per_node=9, general=True)
    assert m.wide_nodes == [] and sum(h.replicas for h in a) > 50
    _same(a, b)
    assert all(h.form in (pack.HEADROOM_FORM_WAVE, pack.HEADROOM_FORM_GENERIC) for h in b)


def test_mixed_cluster_planes_bit_for_bit_and_sums():
    """A mixed cluster: the nodes of the planes have the plain entry's entries bit for bit; every wide candidate has a figure
    (not_evaluated == 0, no flag) that the independent oracle's loop confirms; the sums are the summaries of the entries; the
    defaults still flag the wide nodes and count nothing for them."""
    descs = util.mixed_cluster_desc(9830, 70, occupancy=0.1)
    nl = util.build_cluster(descs)
    specs = _specs(9830)
    tops = [refmodel.make_topology(s) for s in specs]
    m = _twin()
    plain = m.HeadroomMany(nl, tops, per_node=True, max_per_node=9)
    gen = m.HeadroomMany(nl, tops, per_node=True, max_per_node=9, general=True)
    wide = np.array([nm in set(m.wide_nodes) for nm in nl])
    assert 10 < wide.sum() < len(nl) - 10
    want = np.asarray(gc.oracle_entries([d for d, w in zip(descs, wide) if w], specs, False, util.CLOCK, cap=9))
    extra = 0
    for p, (a, b) in enumerate(zip(plain, gen)):
        assert a.error is None and b.error is None
        # the defaults: flagged, no number
        assert ((a.flags & NOT_EVALUATED) != 0).tolist() == wide.tolist() and a.not_evaluated == int(wide.sum()) and (a.per_node[wide] == 0).all()
        assert not a.form & pack.HEADROOM_FORM_WIDE and b.form == a.form | pack.HEADROOM_FORM_WIDE
        # the planes
        assert np.array_equal(a.per_node[~wide], b.per_node[~wide]) and np.array_equal(a.flags[~wide], b.flags[~wide])
        # the wide records
        assert b.not_evaluated == 0 and not (b.flags & NOT_EVALUATED).any()
        assert ((b.per_node[wide].astype(np.int64) | b.flags[wide]) == want[p]).all()
        k = b.per_node.astype(np.int64)
        assert (b.replicas, b.nodes_with_room, b.max_on_one_node) == (int(k.sum()), int((k > 0).sum()), int(k.max()))
        assert b.saturated == int((k >= 9).sum()) and b.stopped == int(((b.flags & STOPPED) != 0).sum())
        assert b.replicas == a.replicas + int(k[wide].sum())
        extra += int(k[wide].sum())
    assert extra > 30


def test_candidate_subsets_and_node_groups():
    """A subset of the attached nodes: its entries are the whole call's, the others are not counted.  With the pods' node groups the
    nodes InitialNodeFilter drops have 0 - wide ones as the others - and the rest their entry without the filter."""
    nl = util.mixed_cluster(9840, 80, occupancy=0.1)
    tops = [refmodel.make_topology(s) for s in _specs(9840, 8)]
    m = _twin()
    full = m.HeadroomMany(nl, tops, per_node=True, max_per_node=7, general=True)
    names = list(nl)
    rng = np.random.default_rng(9840)
    keep = rng.random(len(names)) < 0.6
    sub = {nm: nl[nm] for nm, k in zip(names, keep) if k}
    assert any(nm in sub for nm in m.wide_nodes) and any(nm not in sub for nm in m.wide_nodes)
    for h, f in zip(m.HeadroomMany(sub, tops, per_node=True, max_per_node=7, general=True), full):
        assert np.array_equal(h.per_node, f.per_node[keep]) and np.array_equal(h.flags, f.flags[keep])
        assert h.not_evaluated == 0 and h.replicas == int(f.per_node[keep].sum()) and h.nodes == len(sub)
    groups = [list(rng.choice(["default", "alpha", "beta"], size=int(rng.integers(1, 3)), replace=False)) for _ in tops]
    grouped = m.HeadroomMany(nl, tops, pod_groups=groups, per_node=True, max_per_node=7, general=True)
    dropped_wide = 0
    for h, f, g in zip(grouped, full, groups):
        inside = np.array([nm in set(O.initial_node_filter(nl, g)) for nm in names])
        assert np.array_equal(h.per_node, np.where(inside, f.per_node, 0)) and h.not_evaluated == 0
        dropped_wide += int((f.per_node[~inside] > 0).sum())
    assert dropped_wide > 0


def test_three_harness_shards_equal_one_engine():
    """sharding: every shard answers for its own wide records, the sums add up (the wide bit of `form` if any shard ran it)."""
    nl = util.mixed_cluster(9850, 75, occupancy=0.1)
    tops = [refmodel.make_topology(s) for s in _specs(9850, 8)]
    one = _twin().HeadroomMany(nl, tops, per_node=True, max_per_node=7, general=True)
    grp = HipMatcher(clock=lambda: util.CLOCK, devices=[0, 0, 0], engine_factory=HeadroomGeneralHarnessEngine)
    assert len(grp.engine.shards) == 3
    _same(one, grp.HeadroomMany(nl, tops, per_node=True, max_per_node=7, general=True))
    assert sum(h.replicas for h in one) > 50


def test_limits_and_big_templates_stay_out():
    """general=True with limits=True raises; a template of 5..8 groups still comes back with `error` (strict: raises)."""
    nl = util.mixed_cluster(9860, 20, occupancy=0.1)
    small = refmodel.make_topology(_specs(9860)[0])
    big_spec = dict(_specs(9860)[3])
    big_spec["groups"] = [dict(g) for g in (big_spec["groups"] * 2)[:6]]
    big = refmodel.make_topology(big_spec)
    m = _twin()
    with pytest.raises(ValueError):
        m.HeadroomMany(nl, [small], general=True, limits=True)
    with pytest.raises(ValueError):
        m.Headroom(nl, small, general=True, limits=True)
    got = m.HeadroomMany(nl, [small, big], per_node=True, general=True, strict=False)
    assert got[0].error is None and got[0].not_evaluated == 0
    assert got[1].error is not None and "general path" in got[1].error and got[1].not_evaluated == len(nl) and got[1].replicas == 0
    with pytest.raises(pack.UnsupportedNode):
        m.HeadroomMany(nl, [big], general=True, strict=True)
    assert m.Headroom(nl, small, general=True).replicas == got[0].replicas


def test_defaults_still_flag_a_sharing_mirror():
    """ENABLE_SHARING without the keyword: every entry NOT_EVALUATED, as before; with it: numbers, and a template that asks for
    nothing saturates."""
    with gc.sharing_all(True):
        nl = util.random_cluster(9900, 30, occupancy=0.1)
        tops = [refmodel.make_topology(gc.NOTHING), refmodel.make_topology(util.random_pod_spec(np.random.default_rng(99)))]
        m = _twin()
        old = m.HeadroomMany(nl, tops, per_node=True)
        new = m.HeadroomMany(nl, tops, per_node=True, max_per_node=11, general=True)
    assert m.packer.sharing
    for h in old:
        assert h.error is None and h.not_evaluated == len(nl) and h.replicas == 0 and (h.flags == NOT_EVALUATED).all()
    assert all(h.not_evaluated == 0 and not h.flags.any() for h in new)
    assert set(new[0].per_node.tolist()) == {0, 11} and new[0].saturated > len(nl) // 2


# ---- the two consequences of the definition, on the twin (tests/test_headroom_general_gpu.py puts the device through the same) -----------
@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
def test_sum_is_what_schedule_batch_places(sharing):
    gc.check_sum_is_what_schedule_batch_places(_twin, sharing)


@pytest.mark.parametrize("sharing", [False, True], ids=["mixed", "sharing"])
def test_a_commit_on_a_wide_winner_takes_one(sharing):
    gc.check_a_commit_on_a_wide_winner_takes_one(_twin, sharing)
