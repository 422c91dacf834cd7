"""Shared by the CPU and GPU tests at the edges of the record formats (workload/edge_inputs.py): the checks that hold a HipMatcher - on a
host twin or on the device - to the oracles there.  Every check takes the matcher (or a factory of matchers) and nothing else that
depends on the engine, so the CPU suite runs on the twins what the GPU suite runs through the C-ABI.

* BigCase: ONE cluster of 600 edge nodes (several chunks, 126 wide nodes among them) with 192 pods of up to four groups, the C
  oracle's verdicts for them, and the Python oracle's mapping per (node, pod), computed once per process and never changed.
* check_find / check_explain / check_headroom: the forms of find, nhdfit_explain and nhdfit_headroom(_limits) on it.
* small_case / check_new_entries: the same entries on 14-node edge clusters (quick enough for a dozen seeds on the CPU).
* schedule_one_case / check_schedule_one: ScheduleOne pod after pod on 14 fast-layout edge nodes against the oracle's loop."""
import functools
import json

import numpy as np

from nhd_amd import pack
from oracle import coracle
from oracle import nhd_oracle as O
from workload import edge_inputs as E
from tests import headroom_limit_check as lc
from tests import sched_check, sched_standin, util
from tests.headroom_limit_reference import independent_limit
from workload import refmodel

NOW = util.CLOCK
NOTHING_BUSY = util.CLOCK + 1.0e6
COUNT, STOPPED, NOT_EVALUATED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED, pack.HEADROOM_NOT_EVALUATED
FORMS = [pack.HEADROOM_FORM_WAVE] * 3 + [pack.HEADROOM_FORM_GENERIC]


def unpack_bitmap(bm, n):
    """chunk-major [chunks][P] words -> [P][n] 0/1"""
    chunks, P = bm.shape
    bits = np.unpackbits(bm.view(np.uint8).reshape(chunks, P, 8), axis=2, bitorder="little")
    return bits.transpose(1, 0, 2).reshape(P, chunks * 64)[:, :n]


def winners(score):
    return np.where(score == 0, -1, (0x7FFFFFFFFFFFFFFF - (score & np.uint64(0x7FFFFFFFFFFFFFFF))).astype(np.int64))


def wide_indices(nl):
    """Indices of the nodes of `nl` the fast layout does not hold (the packer's own verdict), and the names no record holds."""
    pk = pack.Packer()
    t = pk.pack_nodes(nl)
    return sorted(t.wide or {}), dict(pk.unmirrored)


LONE_WORDS, LONE_SIGS = 6144, 4096          # step_digest.h kDictLdsWords, step_kernel.h kLoneMaxSigs


def dict_stream(nl):
    """(16-bit words, signatures) of the dictionary of `nl` with every NIC state a commit can produce interned, as nhdfit_set_dictionary
    lays it out (DictView::flat: an offset per signature and one more, a pool count per signature, a word per pool, a word per
    (class, count) pair, padded to an even count).  The launches that answer for ONE pod against the nodes directly stage this
    stream in LDS: k_find1 and k_find1_commit exist only where it fits (a longer one takes the tile form / the composed form),
    k_headroom reads a longer one from global memory."""
    pk = pack.Packer()
    pk.pack_nodes(nl)
    pk.close_signatures()
    _, sig_off, pool_off, _, _, _, nsig, _, _ = pk.dictionary_arrays()
    pools = int(sig_off[nsig])
    words = (nsig + 1) + nsig + pools + int(pool_off[pools])
    return words + (words & 1), int(nsig)


def as_jsonable(res):
    if res[0] is None:
        return [None]
    return [res[0], {"gpu": list(res[1]["gpu"]), "cpu": list(res[1]["cpu"]), "nic": [list(x) for x in res[1]["nic"]]}]


# ---- the 600-node cluster ------------------------------------------------------------------------------------------------------------------
class BigCase:
    PODS, ALL_PODS = E.BIG_PODS, 2 * E.BIG_PODS

    def __init__(self):
        self.descs, self.specs = E.big_edge_case(self.ALL_PODS)
        self.nl = util.build_cluster(self.descs)
        self.names = list(self.nl)
        self.n = len(self.names)
        self.tops = [refmodel.make_topology(s) for s in self.specs]
        self.general = np.array([pack.needs_general_path(t) for t in self.tops])     # (hugepage requests beyond the tile: nhdfit_big_*)
        self.G = np.array([len(s["groups"]) for s in self.specs])
        self.cl = coracle.Cluster.from_nodes(self.nl)
        self.opods = self.cl.pods_from_tops(self.tops)
        wide, unmirrored = wide_indices(self.nl)
        assert not unmirrored
        self.wide = np.zeros(self.n, bool)
        self.wide[wide] = True
        self.upper = np.array([E.upper_half_cores(d) for d in self.descs])           # bits 32..63 of a socket's core mask
        self.heavy = np.array([E.nic_heavy(d) for d in self.descs])                  # 9..16 NICs on a NUMA node
        assert not (self.wide & (self.upper | self.heavy)).any()
        # the nodes whose dictionary fits the one-pod launches' LDS: all but the NIC-heavy nodes with the longest signature streams of
        # their own, left out one by one until the rest fits (the whole cluster's stream has 21 944 words, one node's 13 094 of them)
        self.fits_lds = np.ones(self.n, bool)
        own = sorted(((dict_stream({self.names[i]: self.nl[self.names[i]]})[0], int(i)) for i in np.flatnonzero(self.heavy)), reverse=True)
        while not self._fits(self.fits_lds):
            self.fits_lds[own.pop(0)[1]] = False
        self._found = {}
        self._mapping = {}

    def sub(self, keep):
        """The node dict of the nodes where `keep`, in cluster order."""
        return {self.names[i]: self.nl[self.names[i]] for i in np.flatnonzero(keep)}

    def _fits(self, keep):
        words, sigs = dict_stream(self.sub(keep))
        return words <= LONE_WORDS and sigs <= LONE_SIGS

    def oracle_find(self, pods, keep=None):
        """The C oracle's (winners as indices of the whole cluster, verdicts [len(pods)][n]) for the pods `pods` (indices) among the
        nodes of `keep` (n booleans; None: all) - it runs on the masked view, nodes outside it are never feasible."""
        keep = np.ones(self.n, bool) if keep is None else np.asarray(keep, bool)
        key = (tuple(int(p) for p in pods), keep.tobytes())
        if key not in self._found:
            idx = np.flatnonzero(keep)
            w, f = self.cl.subset(keep).find(self.opods[list(pods)], NOW, threads=coracle.usable_cpus())
            full = np.zeros((len(pods), self.n), np.uint8)
            full[:, idx] = f
            self._found[key] = (np.where(w >= 0, idx[np.maximum(w, 0)], -1), full)
        return self._found[key]

    def mapping(self, node, pod):
        """The Python oracle's mapping of pod `pod` on node `node` alone (the node objects are never changed)."""
        key = (int(node), json.dumps(self.specs[pod], sort_keys=True))
        if key not in self._mapping:
            v = self.nl[self.names[node]]
            self._mapping[key] = O.find_node({v.name: v}, self.tops[pod], NOW)[1]
        return self._mapping[key]

    def figures(self):
        """What the oracle alone says of the first PODS pods on this input: the conditions that keep the checks from going vacuous."""
        first = list(range(self.PODS))
        w, f = self.oracle_find(first)
        return {"nodes": self.n, "wide nodes": int(self.wide.sum()), "33..64-core nodes": int(self.upper.sum()), "NIC-heavy nodes": int(self.heavy.sum()),
                "pods": len(first), "pods of the general path": int(self.general[:self.PODS].sum()), "feasible pairs": int(f.sum()),
                "feasible pairs on 33..64-core nodes": int(f[:, self.upper].sum()), "feasible pairs on NIC-heavy nodes": int(f[:, self.heavy].sum()),
                "pods placed": int((w >= 0).sum()), "winners on 33..64-core nodes": int(self.upper[w[w >= 0]].sum()),
                "pods placed on 33..64-core nodes only": int((self.oracle_find(first, self.upper)[0] >= 0).sum()),
                "pods placed on NIC-heavy nodes only": int((self.oracle_find(first, self.heavy)[0] >= 0).sum())}


@functools.lru_cache(maxsize=None)
def big_case():
    return BigCase()


def check_find(case, ctx, pods, keep, score, bm, maps, tag):
    """One answer of a find (any form) on a context that holds the nodes `ctx` (indices of the whole cluster, ascending) for the pods
    `pods` under the candidate mask `keep` (n booleans or None): winners and - where `bm` is given - the whole verdict matrix against
    the C oracle, every winner's mapping against the Python oracle on that node alone.  Returns the number of pods placed."""
    ctx = np.asarray(ctx)
    inside = np.zeros(case.n, bool)
    inside[ctx] = True
    want_w, want_f = case.oracle_find(pods, inside if keep is None else inside & keep)
    got_local = winners(score)
    got_w = np.where(got_local >= 0, ctx[np.clip(got_local, 0, len(ctx) - 1)], -1)
    assert (got_local < len(ctx)).all(), tag
    assert np.array_equal(got_w, want_w), (tag, np.flatnonzero(got_w != want_w)[:10].tolist())
    if bm is not None:
        got_f = unpack_bitmap(bm, len(ctx))
        assert np.array_equal(got_f, want_f[:, ctx]), (tag, np.argwhere(got_f != want_f[:, ctx])[:10].tolist())
    if maps is not None:
        rows = pack.unpack_big_mappings(maps) if maps.dtype == pack.BIG_MAPPING else pack.unpack_mappings(maps)
        for k, p in enumerate(pods):
            if want_w[k] < 0:
                continue
            ref, G = case.mapping(want_w[k], p), int(case.G[p])
            gpu, cpu, nic_numa, nic_idx, valid = rows[k]
            assert valid == 1, (tag, p)
            assert tuple(gpu[:G]) == tuple(ref["gpu"]) and tuple(cpu[:G + 1]) == tuple(ref["cpu"]), (tag, p)
            assert list(zip(nic_numa[:G], nic_idx[:G])) == [tuple(x) for x in ref["nic"]], (tag, p)
    return int((want_w >= 0).sum())


def masks_of(case):
    """(label, n booleans or None): no mask, only the nodes with 33..64 cores per socket, only the NIC-heavy nodes."""
    return [("unmasked", None), ("33..64 cores", case.upper), ("NIC-heavy", case.heavy)]


def check_explain(m, case):
    """ExplainNodes over every pair of the first BigCase.PODS pods (those of the general path included) against the C stage oracle."""
    P = case.PODS
    ex = m.ExplainNodes(case.nl, case.tops[:P], now=NOW, per_node=True)
    assert [e.error for e in ex] == [None] * P and all(e.unmirrored == 0 for e in ex)
    want_c, want_s = case.cl.explain(case.opods[:P], NOW, per_node=True, threads=coracle.usable_cpus())
    got = np.stack([e.stages for e in ex])
    assert np.array_equal(got, want_s), np.argwhere(got != want_s)[:10].tolist()
    from nhd_amd.matcher import STAGES
    assert np.array_equal(np.array([[e.counts[s] for s in STAGES] for e in ex]), want_c)
    hist = want_c.sum(0)
    assert (hist > 0).all(), hist.tolist()                                      # every stage code 0..9 occurs
    return {"pairs": int(want_s.size), "pods of the general path": int(case.general[:P].sum()), "stage histogram": hist.tolist()}


def templates_of(case, keep=None):
    """For each group count 1..4 the pod (of the table-driven pass, among the first PODS) with the most feasible nodes among `keep`."""
    first = [p for p in range(case.PODS) if not case.general[p]]
    _, f = case.oracle_find(first, keep)
    room = f.sum(1)
    out = []
    for G in (1, 2, 3, 4):
        out.append(max((p for p in first if case.G[p] == G), key=lambda p: (int(room[first.index(p)]), -p)))
    return out


def oracle_limits(descs, specs, todo, cap):
    """(entries, stages) [template][node] of independent_limit where `todo`; elsewhere 0 / NONE."""
    k = np.zeros(todo.shape, np.int64)
    st = np.full(todo.shape, lc.NONE, np.int64)
    for p, i in np.argwhere(todo):
        a, stopped, stage = independent_limit(lambda: refmodel.build_node(descs[i]), lambda: refmodel.make_topology(specs[p]), cap)
        k[p, i], st[p, i] = lc.hc.entry(a, stopped), stage
    return k, st


def check_headroom_results(got, plain, nl, descs, specs, wide, cap, cl=None):
    """HeadroomMany(limits=True, per_node=True) results `got` (and the plain entry's `plain`) for the templates `specs` on the nodes
    `descs`: the NOT_EVALUATED nodes are exactly `wide` (n booleans); count, STOPPED flag and stage of every other node equal
    independent_limit.  Nodes the C oracle's verdict with nothing busy rules out have 0 replicas and the C oracle's stage without the
    Python loop (what independent_limit gives there: no replica, the untouched node's stage).  Returns the replicas in all."""
    n = len(descs)
    cl = coracle.Cluster.from_nodes(nl) if cl is None else cl
    opods = cl.pods_from_tops([refmodel.make_topology(s) for s in specs])
    _, feas = cl.find(opods, NOTHING_BUSY, threads=coracle.usable_cpus())
    _, stage0 = cl.explain(opods, NOTHING_BUSY, per_node=True, threads=coracle.usable_cpus())
    todo = feas.astype(bool) & ~wide[None, :]
    want_k, want_st = oracle_limits(descs, specs, todo, cap)
    want_st = np.where(todo, want_st, stage0)
    lc.check_identities(got, n)
    for p, (h, q) in enumerate(zip(got, plain)):
        assert h.error is None and q.error is None and h.unmirrored == 0
        flags = h.flags.astype(np.int64)
        assert np.array_equal((flags & NOT_EVALUATED) != 0, wide), p                  # the only permitted omission
        entries = h.per_node.astype(np.int64) | flags
        fast = ~wide
        assert np.array_equal(entries[fast], want_k[p][fast]), (p, np.flatnonzero(fast & (entries != want_k[p]))[:10].tolist())
        stopped = (flags & STOPPED) != 0
        assert (h.limit_stages[stopped | wide] == pack.LIMIT_NONE).all(), p
        live = fast & ~stopped
        assert np.array_equal(h.limit_stages[live].astype(np.int64), want_st[p][live]), (p, np.flatnonzero(live & (h.limit_stages != want_st[p]))[:10].tolist())
        # the plain entry: the same figures, no stages
        assert np.array_equal(q.per_node, h.per_node) and np.array_equal(q.flags, h.flags) and q.summary() == h.summary() and q.form == h.form
        assert q.limits is None and q.limit_stages is None
    return {"replicas": int(sum(h.replicas for h in got)), "stopped runs": int(sum(h.stopped for h in got)),
            "pairs through the Python oracle's loop": int(todo.sum())}


def check_headroom(m, case, cap=8, keep=None):
    """The four templates of templates_of on the 600-node cluster (or its nodes `keep`), limits and the plain entry."""
    keep = np.ones(case.n, bool) if keep is None else keep
    tpl = templates_of(case, keep)
    assert [int(case.G[p]) for p in tpl] == [1, 2, 3, 4]
    specs = [case.specs[p] for p in tpl]
    tops = [case.tops[p] for p in tpl]
    nl = case.sub(keep)
    got = m.HeadroomMany(nl, tops, per_node=True, max_per_node=cap, limits=True)
    plain = m.HeadroomMany(nl, tops, per_node=True, max_per_node=cap)
    assert [h.error for h in got] == [None] * 4, got[0].error
    assert set(m.wide_nodes) == {case.names[i] for i in np.flatnonzero(case.wide & keep)}
    assert [h.form for h in got] == FORMS
    out = check_headroom_results(got, plain, nl, [case.descs[i] for i in np.flatnonzero(keep)], specs, case.wide[keep], cap, cl=case.cl.subset(keep))
    out["nodes"] = int(keep.sum())
    out["templates"] = tpl
    out["feasible nodes"] = [int(case.oracle_find([p], keep)[1].sum()) for p in tpl]
    return out


# ---- 14-node clusters: the newer entries -------------------------------------------------------------------------------------------------------
def small_case(seed):
    """(node descriptions, pod specs) of tools/soak_extreme.py's seed, the pods cut to four groups at most (more take no headroom);
    hugepage requests beyond the tile stay: nhdfit_explain_big answers them, headroom names them as not evaluable."""
    _, _, _, descs, specs = E.soak_draw(seed)
    for s in specs:
        del s["groups"][4:]
    return descs, specs


def wave_case(seed):
    """small_case for the emulated wavefront forms, which take request records only: hugepage requests beyond the tile's table are
    clamped to its last row (pack.MAX_HUGEPAGES_GB; Packer.digest_many raises beyond), map types no request takes become PCI."""
    descs, specs = small_case(seed)
    for s in specs:
        s["hugepages_gb"] = min(s["hugepages_gb"], pack.MAX_HUGEPAGES_GB)
        if s["map_type"] not in ("NUMA", "PCI"):
            s["map_type"] = "PCI"
    return descs, specs


def check_new_entries(m, seed, cap=6):
    """ExplainNodes(per_node) against the C stage oracle and HeadroomMany(limits, per_node) + the plain entry against independent_limit
    on one 14-node edge cluster.  Nodes no record holds (seed 24's) are left to HipMatcher.unmirrored and out of the oracle's view."""
    from nhd_amd.matcher import STAGES, UNMIRRORED
    descs, specs = small_case(seed)
    nl = util.build_cluster(descs)
    tops = [refmodel.make_topology(s) for s in specs]
    ex = m.ExplainNodes(nl, tops, now=NOW, per_node=True)
    off = np.array([nm in m.unmirrored for nm in nl])
    live_descs = [d for d, o in zip(descs, off) if not o]
    live = {d["name"]: nl[d["name"]] for d in live_descs}
    cl = coracle.Cluster.from_nodes(live)
    opods = cl.pods_from_tops(tops)
    want_c, want_s = cl.explain(opods, NOW, per_node=True)
    assert [e.error for e in ex] == [None] * len(tops)
    got = np.stack([e.stages for e in ex])
    assert (got[:, off] == UNMIRRORED).all() and all(e.unmirrored == int(off.sum()) for e in ex)
    assert np.array_equal(got[:, ~off], want_s), (seed, np.argwhere(got[:, ~off] != want_s)[:10].tolist())
    assert np.array_equal(np.array([[e.counts[s] for s in STAGES] for e in ex]), want_c)
    # headroom: the templates a request record can express
    idx = [p for p, t in enumerate(tops) if not pack.needs_general_path(t)]
    sub = [tops[p] for p in idx]
    lim = m.HeadroomMany(live, sub, per_node=True, max_per_node=cap, limits=True)
    plain = m.HeadroomMany(live, sub, per_node=True, max_per_node=cap)
    wide = np.array([nm in set(m.wide_nodes) for nm in live])
    out = check_headroom_results(lim, plain, live, live_descs, [specs[p] for p in idx], wide, cap, cl=cl)
    out.update({"pairs": int(want_s.size), "fits": int(want_c[:, lc.FITS].sum()), "unmirrored": int(off.sum()),
                "33..64-core nodes": sum(E.upper_half_cores(d) for d in live_descs)})
    return out


# ---- ScheduleOne, pod after pod ------------------------------------------------------------------------------------------------------------------
ONE_NODES, ONE_PODS = 14, 64


def schedule_one_case(seed):
    """14 edge nodes of the FAST layout (a mirror with a wide node composes every ScheduleOne from FindNodes + CommitPlacement: the
    one-launch form, k_find1_commit, never runs there - so the draws the packer would hold as wide records are skipped) and 64 edge
    pods of up to four groups, map type forced to NUMA / PCI and misc_cores_smt on, as the other ScheduleOne tests force them."""
    rng = np.random.default_rng(660000 + seed)
    descs = []
    while len(descs) < ONE_NODES:
        d = E.edge_node(rng, f"e{len(descs):04d}", rng.random() < 0.12, occupancy=float(rng.choice(E.OCCUPANCIES)))
        wide, unmirrored = wide_indices({d["name"]: refmodel.build_node(d)})       # (the packer's own verdict on the node)
        if not wide and not unmirrored:
            descs.append(d)
    specs = []
    for _ in range(ONE_PODS):
        s = E.edge_pod(rng, 4)
        s["misc_smt"] = True
        if s["map_type"] not in ("NUMA", "PCI"):
            s["map_type"] = "NUMA"
        specs.append(s)
    return descs, specs


def oracle_schedule_one(descs, specs):
    """The oracle's loop alone: [(winner or None, mapping, ids)] up to the first commit it fails."""
    nl = util.build_cluster(descs)
    out = []
    for s in specs:
        top = refmodel.make_topology(s)
        want = O.find_node(nl, top, NOW)
        rec = {}
        if want[0] is not None:
            try:
                O.commit(nl[want[0]], top, want[1], NOW, rec)
            except O.CommitFailure:
                break
        out.append((want, rec if want[0] is not None else None))
    return out


def check_schedule_one(matcher_factory, seed, fused_form, matcher=None):
    """ScheduleOne in attached mode, pod after pod, the placements applied with the stand-in's mutators: result and placement record
    of every pod against the oracle's FindNode + commit on a second copy, mirror == objects at the end.  fused_form: the engine has
    nhdfit_find_commit - then find_commit_counts() must say that every pod of at most three groups took the ONE launch (no commit
    in the loop is one the reference raises on: the loop ends in front of the first), a four-group pod the composed form inside
    the library, and a pod of the general path neither (HipMatcher composes it).  `matcher`: a matcher that has been in use (detached;
    it is given this case's clock and attached to this case's nodes) instead of a new one - its counters move as a new one's do."""
    descs, specs = schedule_one_case(seed)
    want = oracle_schedule_one(descs, specs)
    clock = sched_check.Clock(NOW)
    nl = sched_standin.adopt(util.build_cluster(descs), clock)
    if matcher is None:
        m = matcher_factory(clock)
    else:
        m = matcher
        m.clock = clock
    base = m.engine.find_commit_counts() if fused_form else None
    m.attach(nl)
    assert m.wide_nodes == [] and not m.unmirrored
    words, sigs = dict_stream(util.build_cluster(descs))
    assert words <= LONE_WORDS and sigs <= LONE_SIGS                        # (the one-launch form exists for this mirror)
    upper = {d["name"] for d in descs if E.upper_half_cores(d)}
    placed = on_upper = fused_want = composed_want = 0
    tops = [refmodel.make_topology(s) for s in specs]
    for k, ((w, rec), top) in enumerate(zip(want, tops)):
        before = m.engine.find_commit_counts() if fused_form else None
        got = m.ScheduleOne(nl, top)
        assert as_jsonable(got) == as_jsonable(w), (seed, k)
        assert m.last_placements == [rec], (seed, k)
        assert sched_standin.attempt_scheduling(nl, m, top, None, match=got) == w[0]
        placed += w[0] is not None
        on_upper += w[0] in upper
        if fused_form:
            after = m.engine.find_commit_counts()
            general, G = pack.needs_general_path(top), len(top.proc_groups)
            step = (0, 0) if general else (1, 0) if G <= 3 else (0, 1)
            assert (after[0] - before[0], after[1] - before[1]) == step, (seed, k, G, general)
            fused_want += step[0]
            composed_want += step[1]
    m.FindNode(nl, tops[0])                                                 # any other call flushes the correction that is still pending
    assert sched_check.mirror_state(m) == sched_check.packed(nl)
    out = {"seed": seed, "pods": len(want), "placed": placed, "placed on 33..64-core nodes": on_upper}
    if fused_form:
        end = m.engine.find_commit_counts()
        assert (end[0] - base[0], end[1] - base[1]) == (fused_want, composed_want) and fused_want > 0
        out.update({"fused": fused_want, "composed": composed_want})
    return out


def check_new_entries_against_reference(ref, m, seed, cap=6):
    """check_new_entries' two entries against the UNMODIFIED reference (build container only) on the pods the reference answers in
    reasonable time (three groups at most): every (pod, node) stage against tests/explain_reference.py, count, STOPPED flag and
    limit stage of every fast-layout node against tests/headroom_limit_reference.py."""
    from oracle import ref_loader
    from tests.explain_reference import reference_stages
    from tests.headroom_limit_reference import reference_limit
    ref_loader.VirtualClock(NOW).install()
    descs, specs = small_case(seed)
    specs = [s for s in specs if len(s["groups"]) <= 3]
    nl = util.build_cluster(descs)
    assert not wide_indices(nl)[1]
    nl_ref = util.build_cluster(descs, ref)
    tops = [refmodel.make_topology(s) for s in specs]
    ex = m.ExplainNodes(nl, tops, now=NOW, per_node=True)
    for s, e in zip(specs, ex):
        want = reference_stages(ref, nl_ref, refmodel.make_topology(s, ref))
        assert e.error is None and e.stages.tolist() == [want[n] for n in nl_ref], (seed, s)
    idx = [p for p, t in enumerate(tops) if not pack.needs_general_path(t)]
    got = m.HeadroomMany(nl, [tops[p] for p in idx], per_node=True, max_per_node=cap, limits=True)
    wide = {nm for nm in m.wide_nodes}
    replicas = pairs = 0
    for p, h in zip(idx, got):
        assert h.error is None
        for i, d in enumerate(descs):
            if d["name"] in wide:
                assert int(h.flags[i]) & NOT_EVALUATED
                continue
            k, stopped, stage = reference_limit(ref, lambda: refmodel.build_node(d, ref), lambda: refmodel.make_topology(specs[p], ref), cap)
            assert int(h.per_node[i]) | int(h.flags[i]) == lc.hc.entry(k, stopped), (seed, p, d["name"])
            assert int(h.limit_stages[i]) == stage, (seed, p, d["name"], int(h.limit_stages[i]), stage)
            replicas += k
            pairs += 1
    return {"pods": len(specs), "pairs through the reference's loop": pairs, "replicas": replicas}
