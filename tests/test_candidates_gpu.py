"""nhdfit_candidates on the MI355X (`pytest -m gpu`): the device's lists against the reference's stored answers on the synth and
fixture inputs (tests/golden/refanswers/tests.test_candidates_reference.json - nothing here reads the reference tree); against what
exists on seeded clusters - entry 0 is nhdfit_find's answer, the whole list is K successive finds with the earlier winners cleared
from the mask, `feasible` is nhdfit_explain's FITS count and the popcount of the bitmap row, every mapping is the independent
oracle's (oracle/nhd_oracle.py) on that node alone; the shapes at which the launch can go wrong; the absence of side effects; shards
and the group entry.  Every comparison is exact."""
import ctypes

import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd._lib import NhdFitError
from nhd_amd.engine import Engine, GroupEngine, winner_index
from nhd_amd.matcher import STAGES, HipMatcher
from oracle import nhd_oracle as O
from tests import candidates_reference as cr
from tests import edge_check as ec
from tests import harness, util
from tests.headroom_check import four_templates
from workload import planes, refmodel, synth

FITS = STAGES.index("FITS")
PREF_BIT = 1 << 63


def _device(clock):
    return HipMatcher(device=0, clock=lambda: clock)


def mask_words(keep, extra_high_bits=False):
    n = len(keep)
    bits = np.zeros(((n + 63) // 64) * 64, bool)
    bits[:n] = keep
    if extra_high_bits:
        bits[n:] = True
    return np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))


def engine_on(pk, table):
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    return eng


def engine_for(cfg, n, specs, groups=None):
    spec = synth.make_cluster(cfg, n_nodes=n)
    tops = [refmodel.make_topology(s) for s in specs]
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many(tops, groups)
    return spec, pk, table, tops, reqs, engine_on(pk, table)


def successive_finds(eng, req, now, k, keep):
    """The composed form: k nhdfit_find calls of the one pod, each with the earlier winners cleared from the mask."""
    keep = np.array(keep, bool)
    out = []
    for _ in range(k):
        score, _, maps = eng.find(req.reshape(1), now, cand=mask_words(keep), want_bitmap=False, want_map=True)
        if not score[0]:
            break
        out.append((int(score[0]), maps[0].tobytes()))
        keep[winner_index(score[0]) - eng.global_base] = False
    return out


def listed(sums, entries, p):
    """Pod p's list as (score, mapping bytes); everything past `returned` is zero bytes."""
    got = int(sums[p]["returned"])
    assert entries[p][got:].tobytes() == bytes(32 * (entries.shape[1] - got))
    assert (entries[p]["reserved"] == 0).all()
    return [(int(e["score"]), e["map"].tobytes()) for e in entries[p][:got]]


def check_against_what_exists(eng, reqs, now, k, keep, n, pods=None):
    """One call at K = k under the mask `keep` (n booleans or None) against the existing entries, for the pods `pods` (all)."""
    keep_b = np.ones(n, bool) if keep is None else np.asarray(keep, bool)
    cand = None if keep is None else mask_words(keep_b)
    sums, entries = eng.candidates(reqs, now, k, cand=cand)
    _, bitmap, _ = eng.find(reqs, now, cand=cand, want_bitmap=True, want_map=False)
    fits = ec.unpack_bitmap(bitmap, n)
    counts, _ = eng.explain(reqs, now, cand=cand)
    assert np.array_equal(sums["feasible"], fits.sum(1)) and np.array_equal(sums["feasible"], counts[:, FITS])
    assert np.array_equal(sums["returned"], np.minimum(sums["feasible"], k)) and (sums["not_evaluated"] == 0).all()
    for p in (range(len(reqs)) if pods is None else pods):
        got = listed(sums, entries, p)
        assert got == successive_finds(eng, reqs[p], now, k, keep_b), (p, k)
        idx = [winner_index(s) - eng.global_base for s, _ in got]
        assert all(fits[p, i] for i in idx) and len(set(idx)) == len(idx)
        pref = [bool(s & PREF_BIT) for s, _ in got]
        assert pref == sorted(pref, reverse=True) and sum(pref) == min(k, int(sums[p]["preferred"]))
    return sums, entries


def check_mappings(nl, tops, now, sums, entries, base=0):
    """Each entry's mapping is the independent oracle's find_node on that node alone."""
    names, seen = list(nl), 0
    for p, top in enumerate(tops):
        G = len(top.proc_groups)
        rows = pack.unpack_mappings(np.ascontiguousarray(entries[p]["map"][:int(sums[p]["returned"])]))
        for e, (gpu, cpu, nic_numa, nic_idx, valid) in zip(entries[p]["score"].tolist(), rows):
            name = names[winner_index(e) - base]
            want = O.find_node({name: nl[name]}, top, now)
            assert want[0] == name and valid == 1, (p, name)
            assert (tuple(gpu[:G]), tuple(cpu[:G + 1]), list(zip(nic_numa[:G], nic_idx[:G]))) == \
                   (tuple(want[1]["gpu"]), tuple(want[1]["cpu"]), [tuple(x) for x in want[1]["nic"]]), (p, name)
            seen += 1
    return seen


# ---- the stored reference answers --------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cfg", [1, 2, 3, 4, 5])
def test_synth_lists_equal_the_reference(cfg):
    got, lists = cr.matcher_synth(_device, cfg)
    assert lists == cr.stored(f"test_synth_configurations[{cfg}]")
    assert all(c.form == pack.CANDIDATES_FORM_WAVE and len(c.entries) == min(cr.K, c.feasible) for c in got)


@pytest.mark.gpu
@pytest.mark.parametrize("with_groups", [False, True], ids=["plain", "groups"])
@pytest.mark.parametrize("golden", cr.IDS)
def test_golden_lists_equal_the_reference(golden, with_groups):
    got, lists = cr.matcher_golden(_device, cr.GOLDENS[cr.IDS.index(golden)], with_groups)
    assert lists == cr.stored(f"test_goldens[{golden}-{'groups' if with_groups else 'plain'}]")


# ---- against what exists ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_small_clusters_against_find_explain_and_the_oracle(n):
    """Heterogeneous random clusters of 1, 63, 64, 65 and 129 nodes, random pods of one to four groups (NUMA / PCI / invalid map
    types), K = 1, 2 and 64, with and without a mask that carries stray bits beyond n: the list is K successive finds, `feasible`
    is explain's and the bitmap's count, every mapping the independent oracle's.  An invalid map type gives an empty list."""
    rng = np.random.default_rng(1400 + n)
    nl = util.random_cluster(1400 + n, n, occupancy=0.15)
    specs = [util.random_pod_spec(rng, max_groups=4) for _ in range(10)]
    specs.append(dict(specs[0], map_type="NONE"))
    tops = [refmodel.make_topology(s) for s in specs]
    pk = pack.Packer()
    table = pk.pack_nodes(nl)
    assert not table.wide and not pk.unmirrored
    reqs = pk.digest_many(tops)
    eng = engine_on(pk, table)
    keep = rng.random(n) < 0.7
    mapped = 0
    for k in (1, 2, 64):
        sums, entries = check_against_what_exists(eng, reqs, util.CLOCK, k, None, n)
        mapped += check_mappings(nl, tops, util.CLOCK, sums, entries)
        assert sums[-1]["feasible"] == 0 and sums[-1]["returned"] == 0 and not entries[-1].tobytes().strip(b"\0")
        forms = [pack.CANDIDATES_FORM_GENERIC if s["map_type"] != "NONE" and len(s["groups"]) == 4 else pack.CANDIDATES_FORM_WAVE for s in specs]
        assert sums["form"].tolist() == forms
        s1, e1 = check_against_what_exists(eng, reqs, util.CLOCK, k, keep, n)
        s2, e2 = eng.candidates(reqs, util.CLOCK, k, cand=mask_words(keep, extra_high_bits=True))
        assert s1.tobytes() == s2.tobytes() and e1.tobytes() == e2.tobytes()
    assert mapped >= (3 if n > 1 else 0)
    eng.close()


@pytest.mark.gpu
def test_config_2_whole_several_blocks_per_pod():
    """Config 2 whole (4 096 nodes, 64 chunks: several blocks scan one pod, several chunks each) with templates of one, two, three
    and four groups - `form` tells them apart - at K = 1, 2 and 64; candidates only in the last chunk of a block's range and the
    first of the next, forced by the mask (with one pod the launch cuts the 64 chunks into eight blocks of eight; the mask keeps
    chunks 7|8, 15|16, ... and, for the wavefronts' pieces inside a block, 1|2 and 3|4); feasible less than, equal to and more than
    K; P = 1, 3 and 130 with identical pods getting identical lists."""
    cfg, n = 2, 4096
    specs = four_templates(cfg)
    spec, pk, table, tops, reqs, eng = engine_for(cfg, n, specs)
    now = spec.clock_now
    for k in (1, 2, 64):
        sums, entries = check_against_what_exists(eng, reqs, now, k, None, n)
        assert sums["form"].tolist() == [pack.CANDIDATES_FORM_WAVE] * 3 + [pack.CANDIDATES_FORM_GENERIC]
        assert (sums["feasible"] > 64).all()
    chunk = np.arange(n) // 64
    seams = np.isin(chunk, [1, 2, 3, 4, 7, 8, 15, 16, 23, 24, 31, 32, 39, 40, 47, 48, 55, 56, 63])
    for p in range(len(reqs)):                               # one pod per call: the cut described above
        check_against_what_exists(eng, reqs[p:p + 1], now, 64, seams, n)
        check_against_what_exists(eng, reqs[p:p + 1], now, 64, np.isin(chunk, [23, 24]), n)
    # feasible < K, == K, > K: the mask keeps 1, 2, 3 of pod 0's feasible nodes, far apart
    _, bitmap, _ = eng.find(reqs[:1], now, want_bitmap=True, want_map=False)
    feas = np.flatnonzero(ec.unpack_bitmap(bitmap, n)[0])
    for count in (1, 2, 3):
        keep = np.zeros(n, bool)
        keep[feas[np.linspace(0, len(feas) - 1, count).astype(int)]] = True
        sums, _ = check_against_what_exists(eng, reqs[:1], now, 2, keep, n)
        assert (int(sums[0]["feasible"]), int(sums[0]["returned"])) == (count, min(count, 2))
    # P = 1, 3, 130
    one = eng.candidates(reqs[:1], now, 8)
    three = eng.candidates(reqs[[0, 2, 0]], now, 8)
    many_idx = np.arange(130) % 4
    many = check_against_what_exists(eng, reqs[many_idx], now, 8, None, n, pods=[0, 1, 2, 3, 129])
    for sums, entries, idx in ((three[0], three[1], [0, 2, 0]), (many[0], many[1], many_idx)):
        for j, p in enumerate(idx):
            if p == 0:
                assert sums[j].tobytes() == one[0][0].tobytes() and entries[j].tobytes() == one[1][0].tobytes()
            assert sums[j].tobytes() == many[0][p].tobytes() and entries[j].tobytes() == many[1][p].tobytes()
    eng.close()


@pytest.mark.gpu
def test_preferred_nodes_run_out_before_a_lower_gpu_node():
    """A pod without GPUs on a mixed cluster: the mask leaves a feasible GPU node, two feasible nodes without GPUs behind it and a
    further GPU node.  The two come first, then the GPU nodes in index order; a pod that requests GPUs takes index order."""
    cfg, n = 3, 512
    all_specs, _ = synth.make_pods(cfg, n_pods=64)
    cpu_only = next(s for s in all_specs if not any(g["gpus"] for g in s["groups"]))
    with_gpu = next(s for s in all_specs if any(g["gpus"] for g in s["groups"]))
    spec, pk, table, tops, reqs, eng = engine_for(cfg, n, [cpu_only, with_gpu])
    now = spec.clock_now
    _, bitmap, _ = eng.find(reqs, now, want_bitmap=True, want_map=False)
    fits = ec.unpack_bitmap(bitmap, n).astype(bool)
    has_gpu = (table.p2["flags"] & pack.NF_HAS_GPU) != 0
    g = np.flatnonzero(fits[0] & has_gpu)
    plain = np.flatnonzero(fits[0] & ~has_gpu)
    plain = plain[plain > g[0]][:2]
    g2 = g[g > plain[1]][0]
    order = [int(plain[0]), int(plain[1]), int(g[0]), int(g2)]
    keep = np.zeros(n, bool)
    keep[order] = True
    for k in (1, 2, 3, 64):
        sums, entries = check_against_what_exists(eng, reqs[:1], now, k, keep, n)
        got = [(winner_index(s) - eng.global_base, bool(s & PREF_BIT)) for s in entries[0]["score"][:int(sums[0]["returned"])].tolist()]
        assert got == list(zip(order, [True, True, False, False]))[:k]
        assert (int(sums[0]["feasible"]), int(sums[0]["preferred"])) == (4, 2)
    sums, entries = check_against_what_exists(eng, reqs[1:], now, 64, fits[1] & (np.arange(n) < 200), n)
    idx = [winner_index(s) - eng.global_base for s in entries[0]["score"][:int(sums[0]["returned"])].tolist()]
    assert len(idx) > 4 and idx == sorted(idx) and int(sums[0]["preferred"]) == 0 and not (entries[0]["score"] & np.uint64(PREF_BIT)).any()
    check_mappings(spec.build_nodes(), tops[:1], now, *eng.candidates(reqs[:1], now, 64, cand=mask_words(keep)))
    eng.close()


@pytest.mark.gpu
def test_busy_at_the_threshold_and_one_double_below():
    """A pod that requests GPUs, two of its feasible nodes stamped with busy_threshold(now) and with the double below it: the first
    is busy and not listed, the second is listed; a pod without GPUs lists both."""
    cfg, n = 3, 512
    all_specs, _ = synth.make_pods(cfg, n_pods=64)
    with_gpu = next(s for s in all_specs if any(g["gpus"] for g in s["groups"]))
    cpu_only = next(s for s in all_specs if not any(g["gpus"] for g in s["groups"]))
    spec = synth.make_cluster(cfg, n_nodes=n)
    now = spec.clock_now
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = pk.digest_many([refmodel.make_topology(with_gpu), refmodel.make_topology(cpu_only)])
    eng = engine_on(pk, table)
    _, bitmap, _ = eng.find(reqs, now, want_bitmap=True, want_map=False)
    both = np.flatnonzero(ec.unpack_bitmap(bitmap, n).astype(bool).all(0))
    at, below = int(both[0]), int(both[1])
    edge = harness.busy_threshold(now)
    table.p4["busy_time"][at], table.p4["busy_time"][below] = edge, np.nextafter(edge, -np.inf)
    eng.upload(table)
    keep = np.zeros(n, bool)
    keep[[at, below, int(both[2])]] = True
    sums, entries = check_against_what_exists(eng, reqs, now, 8, keep, n)
    idx = [[winner_index(s) - eng.global_base for s in entries[p]["score"][:int(sums[p]["returned"])].tolist()] for p in range(2)]
    assert idx[0] == [below, int(both[2])] and sorted(idx[1]) == [at, below, int(both[2])]
    eng.close()


@pytest.mark.gpu
def test_node_groups_on_the_device():
    """NHDFIT_RF_INITIAL_FILTER: with the pods' node groups the lists are the successive finds of the filtered requests, and name
    only nodes the oracle's InitialNodeFilter keeps."""
    cfg, n = 5, 1000
    specs = four_templates(cfg)
    _, pgroups = synth.make_pods(cfg, n_pods=4)
    spec, pk, table, tops, reqs, eng = engine_for(cfg, n, specs, pgroups)
    assert (reqs["flags"] & pack.RF_INITIAL_FILTER != 0).all()
    sums, entries = check_against_what_exists(eng, reqs, spec.clock_now, 64, None, n)
    nl = spec.build_nodes()
    names = list(nl)
    plain = eng.candidates(pk.digest_many(tops), spec.clock_now, 64)[0]
    assert (sums["feasible"] < plain["feasible"]).any() and (sums["feasible"] > 0).any()
    for p in range(len(specs)):
        kept = set(O.initial_node_filter(nl, pgroups[p]))
        assert all(names[winner_index(s) - eng.global_base] in kept for s in entries[p]["score"][:int(sums[p]["returned"])].tolist())
    eng.close()


@pytest.mark.gpu
def test_the_edge_cluster_whose_dictionary_is_beyond_the_lds_slice():
    """The 600-node edge cluster (tests/edge_check.py): its dictionary's stream is read from global memory.  The planes' nodes of the
    ordinary pods' lists against the C oracle's verdicts in selection order and the Python oracle's mappings; the wide nodes are
    counted, not listed."""
    case = ec.big_case()
    assert ec.dict_stream(case.nl)[0] > ec.LONE_WORDS
    pods = [p for p in range(case.PODS) if not case.general[p] and case.G[p] <= 4][:12]
    pk = pack.Packer()
    table = pk.pack_nodes(case.nl)
    reqs = pk.digest_many([case.tops[p] for p in pods])
    eng = engine_on(pk, table)
    sums, entries = eng.candidates(reqs, ec.NOW, 8)
    _, feas = case.oracle_find(pods)
    has_gpu = np.array([len(nd.gpus) > 0 for nd in case.nl.values()])
    listed_any = 0
    for j, p in enumerate(pods):
        ok = feas[j].astype(bool) & ~case.wide
        needs = any(len(g.group_gpus) > 0 for g in case.tops[p].proc_groups)
        order = list(np.flatnonzero(ok)) if needs else list(np.flatnonzero(ok & ~has_gpu)) + list(np.flatnonzero(ok & has_gpu))
        got = [winner_index(s) - eng.global_base for s in entries[j]["score"][:int(sums[j]["returned"])].tolist()]
        assert got == [int(i) for i in order[:8]], p
        assert int(sums[j]["feasible"]) == int(ok.sum()) and int(sums[j]["not_evaluated"]) == int(case.wide.sum())
        rows = pack.unpack_mappings(np.ascontiguousarray(entries[j]["map"][:len(got)]))
        for i, (gpu, cpu, nic_numa, nic_idx, valid) in zip(got, rows):
            ref, G = case.mapping(i, p), int(case.G[p])
            assert valid == 1 and tuple(gpu[:G]) == tuple(ref["gpu"]) and tuple(cpu[:G + 1]) == tuple(ref["cpu"])
            assert list(zip(nic_numa[:G], nic_idx[:G])) == [tuple(x) for x in ref["nic"]]
        listed_any += len(got)
    assert listed_any > 20
    eng.close()


@pytest.mark.gpu
def test_wide_records_are_counted_and_the_matcher_composes():
    """A mixed cluster: at the C entry the candidates held as wide records are counted in not_evaluated - with a mask, those of the
    mask - and the list ranks the nodes of the planes; HipMatcher.Candidates (composed) equals the iterated FindNodes, wide nodes
    among its entries."""
    nl = util.mixed_cluster(1450, 120)
    rng = np.random.default_rng(1450)
    tops = [refmodel.make_topology(util.random_pod_spec(rng)) for _ in range(6)]
    pk = pack.Packer()
    table = pk.pack_nodes(nl)
    wide = np.zeros(len(nl), bool)
    wide[sorted(table.wide)] = True
    assert 10 < wide.sum() < len(nl) - 10
    wide_names = {nm for nm, w in zip(nl, wide) if w}
    got = _device(util.CLOCK).CandidatesMany(nl, tops, k=6)
    fresh = _device(util.CLOCK)
    on_wide = 0
    for c, top in zip(got, tops):
        want = cr.iterate(lambda sub, t: fresh.FindNodes(sub, [t], now=util.CLOCK)[0], nl, lambda: top, k=6)
        assert c.error is None and [cr.entry(e) for e in c.entries] == want
        assert c.feasible == fresh.ExplainNode(nl, top, now=util.CLOCK).counts["FITS"]
        on_wide += sum(1 for e in c.entries if e[0] in wide_names)
    assert on_wide > 0
    reqs = pk.digest_many(tops)
    eng = engine_on(pk, table)
    keep = np.random.default_rng(3).random(len(nl)) < 0.5
    for mask in (None, keep):
        sums, entries = eng.candidates(reqs, util.CLOCK, 6, cand=None if mask is None else mask_words(mask))
        assert (sums["not_evaluated"] == int((wide if mask is None else wide & mask).sum())).all()
        for p in range(len(tops)):
            assert not any(wide[winner_index(s) - eng.global_base] for s in entries[p]["score"][:int(sums[p]["returned"])].tolist())
    eng.close()


# ---- refusals on a live context ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_k_outside_1_to_64_and_missing_outputs_are_refused():
    spec, pk, table, tops, reqs, eng = engine_for(2, 64, four_templates(2))
    for k in (0, 65):
        with pytest.raises(NhdFitError) as e:
            eng.candidates(reqs, spec.clock_now, k)
        assert e.value.code == -1
    buf = (ctypes.c_uint8 * 4096)()
    assert eng.lib.nhdfit_candidates(eng.ctx, reqs.ctypes.data_as(ctypes.c_void_p), 1, 0.0, None, 8, None, buf) == -1
    big = reqs.copy()
    big["hugepages_gb"][0] = 5000
    with pytest.raises(NhdFitError) as e:
        eng.candidates(big, spec.clock_now, 8)
    assert e.value.code == -6
    assert eng.candidates(reqs, spec.clock_now, 64)[0]["returned"].max() > 0
    eng.close()


# ---- no side effects ----------------------------------------------------------------------------------------------------------------------
def _planes(t):
    return [np.array(getattr(t, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]


@pytest.mark.gpu
def test_candidates_leave_no_trace():
    """The mirror (Engine.download: all planes, busy times among them), nhdfit_get_stats and the finds that follow are identical
    before and after; called with pipelined steps in flight, their fetched results are what they are without the call in between;
    the call twice gives the same bytes."""
    specs = four_templates(4)
    spec, pk, table, tops, reqs, eng = engine_for(4, 5000, specs)
    now = spec.clock_now
    pods, groups = synth.make_pods(4, n_pods=300)
    batch = pk.digest_many([refmodel.make_topology(s) for s in pods], groups)
    eng.set_dictionary(pk)
    before = _planes(eng.download())
    s0, b0, m0 = eng.find(batch, now, want_bitmap=True, want_map=True)
    one0 = eng.find(batch[:1], now, want_bitmap=False, want_map=True)
    st0 = eng.stats()
    sums, entries = eng.candidates(reqs, now, 16)
    st1 = eng.stats()
    for f in ("launches", "fit_ms_total", "fit_ms_last", "digest_ms_last", "step_ms_last", "evals_last", "bytes_last", "small_finds", "batch_finds",
              "big_nic_steps_max"):
        assert getattr(st0, f) == getattr(st1, f), f
    for a, b in zip(before, _planes(eng.download())):
        assert a.tobytes() == b.tobytes()
    s1, b1, m1 = eng.find(batch, now, want_bitmap=True, want_map=True)
    assert np.array_equal(s0, s1) and np.array_equal(b0, b1) and m0.tobytes() == m1.tobytes()
    one1 = eng.find(batch[:1], now, want_bitmap=False, want_map=True)
    assert np.array_equal(one0[0], one1[0]) and one0[2].tobytes() == one1[2].tobytes()
    again = eng.candidates(reqs, now, 16)
    assert again[0].tobytes() == sums.tobytes() and again[1].tobytes() == entries.tobytes() and sums["returned"].max() == 16
    # steps in flight
    eng.stage(batch)
    for _ in range(3):
        eng.enqueue(now)
    s_in, e_in = eng.candidates(reqs, now, 16)
    f1 = eng.fetch(want_bitmap=True, want_map=True)
    assert s_in.tobytes() == sums.tobytes() and e_in.tobytes() == entries.tobytes()
    assert np.array_equal(f1[0], s0) and np.array_equal(f1[1], b0) and f1[2].tobytes() == m0.tobytes()
    eng.close()


# ---- shards and the group entry -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_three_shards_on_one_gpu_equal_one_device():
    """Three shards on one GPU == one device.  A group of three contexts on ONE device cannot be created (its communicator wants
    distinct devices), so the pieces are held one by one: three device contexts as shards (GroupEngine over Engine: the lists cross
    the shards' seams) under sharding.merge_candidates; the same three shards' answers through the text nhdfit_group_candidates
    merges with (candidates_merge.h, as the host twin exports it), owners included; and the group entry itself,
    HipMatcher(devices=[0]), against HipMatcher(device=0).  With and without a mask and the pods' node groups."""
    from tests.harness import candidates_twin as ct
    cfg, n = 3, 700
    specs, pgroups = synth.make_pods(cfg, n_pods=12)
    specs = list(specs) + four_templates(cfg)
    spec, pk, table, tops, reqs, eng = engine_for(cfg, n, specs)
    grp = GroupEngine([0, 0, 0], engine_factory=Engine)
    grp.set_dictionary(pk)
    grp.upload(table)
    assert len([1 for lo, hi in grp._bounds if hi > lo]) == 3
    keep = np.random.default_rng(1470).random(n) < 0.7
    crossing = 0
    for cand in (None, mask_words(keep)):
        for k in (2, 64):
            s1, e1 = eng.candidates(reqs, spec.clock_now, k, cand=cand)
            s3, e3 = grp.candidates(reqs, spec.clock_now, k, cand=cand)
            assert s1.tobytes() == s3.tobytes() and e1.tobytes() == e3.tobytes()
            parts = [sh.candidates(reqs, spec.clock_now, k, cand=None if cand is None else np.ascontiguousarray(cand[lo // 64:(hi + 63) // 64]))
                     for sh, (lo, hi) in zip(grp.shards, grp._bounds)]
            sm, em, owner = ct.merge(parts, k)
            assert sm.tobytes() == s1.tobytes() and em.tobytes() == e1.tobytes()
            for p in range(len(reqs)):
                got = int(s1[p]["returned"])
                assert owner[p, :got].tolist() == [grp._shard_of(winner_index(s)) for s in e1[p]["score"][:got].tolist()]
                assert (owner[p, got:] == -1).all()
                crossing += len(set(owner[p, :got].tolist())) > 1
    assert crossing > 0 and (s1["feasible"] > 0).any()
    grp.close()
    eng.close()
    nl = spec.build_nodes()
    one = _device(spec.clock_now)
    for other in (HipMatcher(devices=[0], clock=lambda: spec.clock_now), HipMatcher(devices=[0, 0, 0], engine_factory=Engine, clock=lambda: spec.clock_now)):
        for groups in (None, list(pgroups) + list(pgroups[:4])):
            a = one.CandidatesMany(nl, tops, k=8, pod_groups=groups)
            b = other.CandidatesMany(nl, tops, k=8, pod_groups=groups)
            for x, y in zip(a, b):
                assert x.error is None and y.error is None
                assert x.entries == y.entries and (x.feasible, x.preferred, x.form) == (y.feasible, y.preferred, y.form) and x.summary() == y.summary()
            assert sum(len(x.entries) for x in a) > 20
