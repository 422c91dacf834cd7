"""For the tests that walk winners across the grid seams of the find and explain launches: the rungs (cluster sizes
that sit ON the host-side cuts of the node axis), the candidate masks that push winners over each cut, the checks that hold an
engine - the device's or a host twin - to the oracles under them, and the figures the oracle alone gives for every rung.

The scheduler takes the FIRST feasible node and the synthetic clusters are dense in feasible nodes, so an unmasked find decides
everything inside chunk 0.  A straddle mask (candidates = nodes >= 64 c - 1) moves the first candidate to the last node of chunk c - 1:
some pods win on it or behind it in that chunk, the others beyond the boundary, in the chunk another wavefront / block / work item
starts with.  An island mask keeps the GPU nodes of one early chunk and one far GPU-less node: a GPU-less pod has feasible nodes in
the island and must still be given the far node (Matcher.py:393-421), which some other block finds.

The cuts, all computed on the host (nhd_amd/csrc/nhdfit.hip unless named otherwise; chunks = ceil(n / 64), tiles = ceil(P / 64)):
  (a) build_items, :1230-1255.  rec_bytes = chunks * 64 * (16 * (max_wcls + 1) + 8); small_shard = rec_bytes <= 2 MiB - with pods of
      all three row widths (max_wcls = 2) that is chunks <= 585.  by_xcd = chunks >= 32 * nw and (nw == 8 or the batch find) and not
      small_shard: every tile is cut at chunks * r / 8 (the step, nw = 8) or chunks * r / 16 (k_findn, nw = 4); otherwise at
      chunks * b / nb;
  (b) enqueue_step, :1475.  geom_big = tiles * ceil(chunks / 32) >= CUs (256): the 512-thread form (nw = 8), the only one that takes (a)'s eighths;
  (c) find_small, :1682.  k_find runs ceil(chunks / 32) fit blocks (at most one per CU);
  (d) lone_find_args, :1598.  k_find1 / k_find1_commit run ceil(chunks / 8) blocks;
  (e) step_kernel.h:232.  k_rows_t turns the verdict matrix into rows by groups of 16 chunks;
  (f) find_batch, :1798.  k_findn reads up to 512 requests from the host block and copies more;
  (g) explain_kernel.h:12.  16 pods per explain block.

Rung  cfg      n  chunks  what it sits on
  A     4     65       2  one node past a chunk: one block everywhere, two chunks for its wavefronts
  B     5    513       9  (d) 8 -> 9 chunks: a second k_find1 block that holds ONE chunk (one node); (c) one k_find block
  C     3  2 049      33  (c) 32 -> 33 chunks: a second k_find block with one chunk; (e) two full groups and one chunk; (d) 5 blocks
  D     5  8 197     129  (c) 5 blocks, (d) 17, (e) 9 groups; 129 >= 128 but 129 * 3 584 B = 0.44 MiB is a small shard: (a) cuts at
                          chunks * b / nb; sparse feasibility (config 5's node groups): winners up to 130 nodes behind a mask's start
  E     4 37 438     585  (a) 585 * 3 584 B = 2 096 640 B <= 2 MiB, 586 chunks would be over: the LARGEST small shard - k_findn by
                          chunks * b / nb; at 900 pods (15 tiles, 15 * 19 = 285 >= 256: nw = 8) the step takes the few-long-blocks form (nb <= 8)
  F     4 41 003     641  (a) over 2 MiB and ragged for 8 and 16 (641 = 8 * 80 + 1): k_findn by sixteenths; at 900 pods
                          (15 * 21 = 315 >= 256) the step by eighths; at 130 pods (3 * 21 < 256) the 256-thread step, chunks * b / nb
E and F with 900 pods also send k_findn down (f)'s copy path.  (E is one node larger than 37 437: there node 64 * 584 - 1, the
only candidate in front of the last boundary, fits no pod, and a straddle mask without a winner on either side checks nothing.)

Every rung has 130 pods of synth.make_pods (one to three groups) and six four-group pods behind them (the groups of pairs of its
two-group pods joined); the single-launch forms refuse four groups and get the 130.  What is held to what: winners to the C oracle on
the masked view of the cluster (the test never restates the preference rule), the verdict matrix to the C oracle's matrix, every
winner's mapping to the Python oracle on that node alone, stages to the C stage oracle, the bits at and beyond n of the last
chunk's bitmap words to zero."""
import functools
import hashlib
import json
import multiprocessing

import numpy as np

from nhd_amd import pack
from oracle import coracle
from oracle import nhd_oracle as O
from tests.edge_check import unpack_bitmap
from workload import planes, refmodel, synth

RUNGS = {"A": (4, 65), "B": (5, 513), "C": (3, 2049), "D": (5, 8197), "E": (4, 37438), "F": (4, 41003)}
PODS, FOURS, MANY_PODS = 130, 6, 900
MAX_MASKS = 16
POD_AXIS = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 511, 512, 513]       # on rung C's cluster: (g) 16, a tile's 64, (f) 512
SCORE_MASK = 0x7FFFFFFFFFFFFFFF


def winners(score, base=0):
    """Node index per pod (-1: none) of packed scores whose indices start at `base`."""
    score = np.asarray(score, np.uint64)
    return np.where(score == 0, -1, (SCORE_MASK - (score & np.uint64(SCORE_MASK))).astype(np.int64) - base)


def mask_words(keep):
    """n booleans -> the uint64 candidate words of the C-ABI, the bits at and beyond n of the last word SET: they must not matter."""
    n = len(keep)
    bits = np.ones(((n + 63) // 64) * 64, bool)
    bits[:n] = keep
    return np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))


def four_group_pods(specs, groups, k=FOURS):
    """k four-group pods: the groups of consecutive pairs of the two-group pods of `specs` joined (everything else of the pair's first)."""
    twos = [i for i, s in enumerate(specs) if len(s["groups"]) == 2]
    assert len(twos) >= 2 * k
    out_s, out_g = [], []
    for a, b in zip(twos[0:2 * k:2], twos[1:2 * k:2]):
        out_s.append(dict(specs[a], groups=[dict(g) for g in specs[a]["groups"]] + [dict(g) for g in specs[b]["groups"]]))
        out_g.append(groups[a])
    return out_s, out_g


class Rung:
    """One cluster of synth.make_cluster(cfg, n) with its pods, the C oracle's view of both, and the oracles' answers (memoised,
    never changed).  `n_pods` pods of one to three groups come first (indices [0, n_pods)), the four-group pods behind them."""

    def __init__(self, name, cfg, n, n_pods=PODS, fours=FOURS):
        self.name, self.cfg, self.n, self.n_small = name, cfg, n, n_pods
        self.chunks = (n + 63) // 64
        self.spec = synth.make_cluster(cfg, n_nodes=n)
        self.now = self.spec.clock_now
        specs, groups = synth.make_pods(cfg, n_pods=n_pods)
        if fours:
            fs, fg = four_group_pods(specs, groups, fours)
            specs, groups = specs + fs, groups + fg
        self.specs, self.groups = specs, groups
        self.P = len(specs)
        self.tops = [refmodel.make_topology(s) for s in specs]
        self.G = np.array([len(s["groups"]) for s in specs])
        assert (self.G[:n_pods] <= 3).all() and (self.G[n_pods:] == 4).all()
        self.cl = coracle.Cluster.from_spec(self.spec)
        self.opods = self.cl.pods_from_tops(self.tops, self.groups)
        self.has_gpu = np.asarray(self.spec.n_gpus) > 0
        self.pod_wants_gpu = np.array([any(g["gpus"] for g in s["groups"]) for s in specs])
        self._won, self._mapping, self._feas, self._cuts, self._packed = {}, {}, None, None, None

    # ---- the engine's side of the inputs -------------------------------------------------------------------------------------------
    def packed(self):
        """(packer with its signatures closed, node table, request records of all pods): built once, never changed (an engine copies
        what it is given)."""
        if self._packed is None:
            pk = pack.Packer()
            table = planes.planes_from_spec(pk, self.spec)
            reqs = pk.digest_many(self.tops, self.groups)
            pk.close_signatures()
            self._packed = (pk, table, reqs)
        return self._packed

    def big_reqs(self, pk, pods):
        return np.array([pk.digest_big(self.tops[p], self.groups[p]) for p in pods], dtype=pack.BIG_REQ)

    def input_hash(self):
        """sha256 over the cluster's columns and the pod specs: the rung stands for the same input on every machine."""
        h = hashlib.sha256()
        for f in ("phys", "smt", "core_used", "n_gpus", "gpu_used", "nic_used", "hp_free", "maintenance", "active", "busy", "group_bits"):
            h.update(np.ascontiguousarray(getattr(self.spec, f)).tobytes())
        h.update(json.dumps([self.specs, self.groups], sort_keys=True).encode())
        return h.hexdigest()

    # ---- the oracles ------------------------------------------------------------------------------------------------------------------
    def feas(self):
        """The C oracle's verdict matrix [P][n] of the whole cluster, unmasked."""
        if self._feas is None:
            self._feas = self.cl.find(self.opods, self.now, threads=coracle.usable_cpus())[1].astype(bool)
        return self._feas

    def oracle_winners(self, keep, pods=None):
        """The C oracle's winners (indices of the whole cluster, -1: none) for the pods `pods` (indices; None: all) among the nodes of
        `keep` (n booleans or None): it runs on the masked view, whose winners are mapped back.  (A pod's winner does not depend on
        the other pods of the call: one run per mask serves every form.)"""
        key = None if keep is None else np.asarray(keep, bool).tobytes()
        if key not in self._won:
            if keep is None:
                w = self.cl.find(self.opods, self.now, want_feas=False, threads=coracle.usable_cpus())[0]
            else:
                idx = np.flatnonzero(keep)
                w = np.full(self.P, -1, np.int64)
                if len(idx):
                    w = self.cl.subset(keep).find(self.opods, self.now, want_feas=False, threads=coracle.usable_cpus())[0]
                    w = np.where(w >= 0, idx[np.maximum(w, 0)], -1)
            self._won[key] = w
        return self._won[key] if pods is None else self._won[key][np.asarray(pods)]

    def oracle_matrix(self, keep):
        """The C oracle's verdict matrix under the mask: its verdict on every node inside, nothing outside."""
        return self.feas() if keep is None else self.feas() & np.asarray(keep, bool)[None, :]

    def _mapping_key(self, node, pod):
        return (int(node), json.dumps(self.specs[pod], sort_keys=True))           # (pods of one spec share the answer)

    def _one_mapping(self, node, pod):
        v = self.spec.build_node(int(node))
        return O.find_node({v.name: v}, self.tops[pod], self.now)[1]

    def mapping(self, node, pod):
        """The Python oracle's mapping of pod `pod` on node `node` alone."""
        key = self._mapping_key(node, pod)
        if key not in self._mapping:
            self._mapping[key] = self._one_mapping(node, pod)
        return self._mapping[key]

    def prefetch_mappings(self, masks):
        """The Python oracle's mapping of every winner under `masks`, once per rung.  The oracle takes 1 to 30 ms per pair (config 5's
        sixteen NICs per node) and a rung has up to 2 000 distinct (winner, request) pairs: beyond a few hundred they are shared
        out over the usable cores (fresh processes, as headroom_check.oracle_synth starts them: the caller may hold a GPU)."""
        need = {}
        for _, keep in masks:
            for p, node in enumerate(self.oracle_winners(keep)):
                if node >= 0 and self._mapping_key(node, p) not in self._mapping:
                    need[self._mapping_key(node, p)] = (int(node), p)
        procs = min(16, coracle.usable_cpus())
        if len(need) < 400 or procs == 1:
            return
        keys, pairs = list(need), list(need.values())
        jobs = [(self.cfg, self.n, self.n_small, self.P - self.n_small, pairs[k::4 * procs]) for k in range(4 * procs)]
        with multiprocessing.get_context("spawn").Pool(procs) as pool:
            parts = pool.map(_mappings_of, jobs, chunksize=1)
        for k, part in enumerate(parts):
            for key, ref in zip(keys[k::4 * procs], part):
                self._mapping[key] = ref

    # ---- masks ---------------------------------------------------------------------------------------------------------------------------
    def straddle(self, c):
        keep = np.zeros(self.n, bool)
        keep[64 * c - 1:] = True
        return keep

    def straddles_both_sides(self, c):
        """By the C oracle alone: under the straddle mask of boundary c some pod wins in front of node 64 c and some pod at or beyond it."""
        w = self.oracle_winners(self.straddle(c))
        return bool(((w >= 0) & (w < 64 * c)).any() and (w >= 64 * c).any())

    def boundaries(self):
        """The chunk boundaries c (candidates = nodes >= 64 c - 1) of this rung's straddle masks.  Rungs of a few chunks: every c.
        Otherwise c = 1 and c = chunks - 1, then, in this order until the list of masks is full: the second block of k_find (32) and
        of k_find1 (8), k_rows_t's second group (16) and the last multiple of 8 where the rung is small; cuts of the eighths and
        sixteenths, chunks * r / 8 and chunks * r / 16 in turn, where it is large; seeded boundaries, so that a later change of a cut still
        meets some.  Of the cuts and the seeded boundaries only those are taken at which the oracle alone puts winners on both sides
        (node 64 c - 1 may be one that fits no pod: in maintenance, say); at least two seeded ones stay."""
        if self._cuts is None:
            ch, room = self.chunks, MAX_MASKS - 4
            if ch <= 9:
                self._cuts = list(range(1, ch))
                return self._cuts
            rng = np.random.default_rng(1100 + self.n)
            seeded = [int(c) for c in rng.permutation(np.arange(2, ch - 1))]
            if ch <= 160:
                fixed = [32 * (ch // 32), 8, 16, 32, 8 * ((ch - 1) // 8), 24, 64, 96]
            else:
                fixed = [ch * r // d for r, d in ((1, 8), (1, 16), (7, 8), (15, 16), (4, 8), (9, 16), (3, 8), (5, 16), (5, 8), (11, 16), (2, 8), (3, 16), (6, 8), (13, 16), (7, 16))]
            out = [1, ch - 1]
            for c in fixed:
                if len(out) < room - 2 and 1 <= c < ch and c not in out and self.straddles_both_sides(c):
                    out.append(c)
            for c in seeded:
                if len(out) < room and c not in out and self.straddles_both_sides(c):
                    out.append(c)
            self._cuts = out
        return self._cuts

    def island(self, chunk=0):
        """(keep, far node): the GPU nodes of chunk `chunk` plus the single last GPU-less node of the cluster."""
        far = int(np.flatnonzero(~self.has_gpu)[-1])
        keep = np.zeros(self.n, bool)
        keep[chunk * 64:min(self.n, chunk * 64 + 64)] = self.has_gpu[chunk * 64:chunk * 64 + 64]
        keep[far] = True
        return keep, far

    def masks(self):
        """[(label, n booleans or None)], at most MAX_MASKS: none, all zero, only node n - 1, the island, the straddles."""
        none, last = np.zeros(self.n, bool), np.zeros(self.n, bool)
        last[self.n - 1] = True
        out = [("none", None), ("all zero", none), ("only the last node", last), ("island", self.island()[0])]
        for c in self.boundaries():
            out.append((f"straddle {c}", self.straddle(c)))
        assert len(out) <= MAX_MASKS
        return out

    # ---- what the oracle alone says: the conditions that keep the checks from going vacuous -----------------------------------------------
    def straddle_figures(self):
        """{c: (pods that win in front of node 64 c, pods that win at or beyond it)} by the C oracle under each straddle mask."""
        out = {}
        for label, keep in self.masks():
            if label.startswith("straddle"):
                c = int(label.split()[1])
                w = self.oracle_winners(keep)
                out[c] = (int(((w >= 0) & (w < 64 * c)).sum()), int((w >= 64 * c).sum()))
        return out

    def island_figures(self):
        """(pods that win the far node although the island holds a feasible node for them, pods that win inside the island)."""
        keep, far = self.island()
        w = self.oracle_winners(keep)
        inside = keep.copy()
        inside[far] = False
        could = (self.feas() & inside[None, :]).any(1)
        return int(((w == far) & could).sum()), int(((w >= 0) & (w != far)).sum())

    def chunks_without_a_pair(self):
        """Chunks of the unmasked cluster in which no (pod, node) pair is feasible."""
        per_node = np.zeros(self.chunks * 64, bool)
        per_node[:self.n] = self.feas().any(0)
        return np.flatnonzero(~per_node.reshape(self.chunks, 64).any(1)).tolist()


def _mappings_of(args):
    cfg, n, n_pods, fours, pairs = args
    r = Rung("", cfg, n, n_pods=n_pods, fours=fours)
    return [r._one_mapping(node, pod) for node, pod in pairs]


@functools.lru_cache(maxsize=None)
def rung(name, n_pods=PODS):
    cfg, n = RUNGS[name]
    r = Rung(name, cfg, n, n_pods=n_pods, fours=FOURS if n_pods == PODS else 0)
    if n_pods != PODS:
        r._cuts = rung(name).boundaries()               # the same cluster with more pods: the same masks
    return r


@functools.lru_cache(maxsize=None)
def pod_axis_rung():
    """Rung C's cluster with the first 513 pods of its configuration (no four-group pods: every form takes every prefix)."""
    cfg, n = RUNGS["C"]
    return Rung("C-pods", cfg, n, n_pods=max(POD_AXIS), fours=0)


def dictionary_fits_a_block(pk):
    """Whether the lone-pod launches (k_find1, k_find1_commit) exist for this dictionary: its 16-bit stream (DictView::flat) within
    step_digest.h kDictLdsWords = 6 144 words, at most step_kernel.h kLoneMaxSigs = 4 096 signatures."""
    _, sig_off, pool_off, _, _, _, nsig, _, _ = pk.dictionary_arrays()
    pools = int(sig_off[nsig])
    words = (nsig + 1) + nsig + pools + int(pool_off[pools])
    return words + (words & 1) <= 6144 and int(nsig) <= 4096


# ---- the checks ------------------------------------------------------------------------------------------------------------------------------
def check_find(r, pods, keep, score, bm, maps, tag, base=0):
    """One answer of a find (any form) for the pods `pods` (indices into the rung's) under the mask `keep`: winners against the C
    oracle on the masked view, the verdict matrix (where `bm` is given) against the C oracle's and its padding bits against zero,
    every winner's mapping (where `maps` is given) against the Python oracle on that node alone.  `base`: the context's global_base.
    Returns the winners."""
    pods = np.asarray(pods)
    want_w = r.oracle_winners(keep, pods)
    got_w = winners(score, base)
    assert np.array_equal(got_w, want_w), (tag, [(int(pods[k]), int(got_w[k]), int(want_w[k])) for k in np.flatnonzero(got_w != want_w)[:8]])
    if bm is not None:
        assert bm.shape == (r.chunks, len(pods)), tag
        got_f = unpack_bitmap(bm, r.n).astype(bool)
        want_f = r.oracle_matrix(keep)[pods]
        assert np.array_equal(got_f, want_f), (tag, np.argwhere(got_f != want_f)[:8].tolist())
        if r.n % 64:
            stray = bm[-1] >> np.uint64(r.n % 64)
            assert not stray.any(), (tag, "bits at and beyond n in the last chunk's words", np.flatnonzero(stray)[:8].tolist())
    if maps is not None:
        rows = pack.unpack_big_mappings(maps) if maps.dtype == pack.BIG_MAPPING else pack.unpack_mappings(maps)
        for k, p in enumerate(pods):
            if want_w[k] < 0:
                continue
            ref, G = r.mapping(want_w[k], int(p)), int(r.G[p])
            gpu, cpu, nic_numa, nic_idx, valid = rows[k]
            assert valid == 1, (tag, int(p))
            assert tuple(gpu[:G]) == tuple(ref["gpu"]) and tuple(cpu[:G + 1]) == tuple(ref["cpu"]), (tag, int(p))
            assert list(zip(nic_numa[:G], nic_idx[:G])) == [tuple(x) for x in ref["nic"]], (tag, int(p))
    return want_w


def check_explain(r, eng, reqs, labels):
    """nhdfit_explain with stages per node under the masks `labels` of the rung: counts and stages against the C stage oracle."""
    masks = dict(r.masks())
    for label in labels:
        keep = masks[label]
        counts, stages = eng.explain(reqs, r.now, cand=None if keep is None else mask_words(keep), per_node=True)
        want_c, want_s = r.cl.explain(r.opods, r.now, cand=keep, per_node=True, threads=coracle.usable_cpus())
        assert np.array_equal(stages, want_s), (r.name, label, np.argwhere(stages != want_s)[:8].tolist())
        assert np.array_equal(counts, want_c), (r.name, label)


def explain_masks(r):
    """Three of the rung's masks for explain: none, the island, the straddle in the middle of its list."""
    cuts = [label for label, _ in r.masks() if label.startswith("straddle")]
    return ["none", "island", cuts[len(cuts) // 2]]


def mask_sequence(r):
    """The rung's masks in turn, then one straddle mask twice and none: the small finds keep the mask they uploaded last and compare
    the next one with it (upload_small_cand, nhdfit.hip:1606-1617)."""
    masks = r.masks()
    again = next(m for m in masks if m[0].startswith("straddle"))
    return masks + [again, again, masks[0]]


def few_masks(r):
    """none, all zero, the island and two straddles (the first cut behind c = 1 and c = chunks - 1, and the last of the list): for the
    cases whose oracle runs are long (900 pods) or many (the pod axis)."""
    masks = r.masks()
    cuts = [m for m in masks if m[0].startswith("straddle")]
    return [masks[0], masks[1], masks[3], cuts[min(2, len(cuts) - 1)], cuts[-1]]


def as_find(big):
    """nhdfit_big_find's (scores, mappings) in the shape of a find's answer."""
    return big[0], None, big[1]


def walk(r, find, pods, tag, masks=None, base=0):
    """`find(cand words or None) -> (score, bitmap or None, mappings or None)` under every mask of `masks` (default: mask_sequence)
    through check_find.  Returns [(label, winners)]."""
    out = []
    masks = mask_sequence(r) if masks is None else masks
    r.prefetch_mappings(masks)
    for label, keep in masks:
        score, bm, maps = find(None if keep is None else mask_words(keep))
        out.append((label, check_find(r, pods, keep, score, bm, maps, f"rung {r.name}, {tag}, mask {label}", base)))
    return out


# ---- headroom and its limits under masks (rungs A and B) -----------------------------------------------------------------------------------
HEADROOM_CAP = 8


def check_headroom(r, engine_factory, specs, labels):
    """nhdfit_headroom and nhdfit_headroom_limits on an engine of `engine_factory` (a packer of its own: the templates are digested
    into it) for the templates `specs` under the masks `labels`: entries against
    headroom_check.oracle_synth(maybe = the mask's feasible pairs), entries and limit stages against independent_limit
    (headroom_limit_check.oracle_synth); a pair without room has the C stage oracle's stage with nothing busy; nodes outside the
    mask read 0 / NOT_CANDIDATE.  Returns the replicas the oracle counts under each mask."""
    from tests import headroom_check as hc
    from tests import headroom_limit_check as lc
    tops = [refmodel.make_topology(s) for s in specs]
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, r.spec)
    reqs = pk.digest_many(tops, None)
    pk.close_signatures()
    eng = engine_factory()
    eng.set_dictionary(pk)
    eng.upload(table)
    opods = r.cl.pods_from_tops(tops, None)
    idle = r.now + 1.0e6                                                       # (nothing is busy by then)
    feas = r.cl.find(opods, idle, threads=coracle.usable_cpus())[1].astype(bool)
    masks = dict(r.masks())
    union = np.zeros(r.n, bool)
    for label in labels:
        union |= np.ones(r.n, bool) if masks[label] is None else masks[label]
    all_k, all_st = lc.oracle_synth(r.cfg, r.n, specs, feas & union[None, :], cap=HEADROOM_CAP, procs=1)
    out = {}
    for label in labels:
        keep = np.ones(r.n, bool) if masks[label] is None else masks[label]
        cand = None if masks[label] is None else mask_words(keep)
        todo = feas & keep[None, :]
        stage0 = r.cl.explain(opods, idle, cand=keep, per_node=True, threads=coracle.usable_cpus())[1]
        want_k = np.where(todo, all_k, 0)
        want_st = np.where(todo, all_st, stage0)
        sums, counts, hist, stages = eng.headroom_limits(reqs, cand=cand, max_per_node=HEADROOM_CAP, per_node=True)
        tag = (r.name, label)
        assert np.array_equal(counts.astype(np.int64), want_k), (tag, np.argwhere(counts != want_k)[:8].tolist())
        assert not counts[:, ~keep].any() and (stages[:, ~keep] == lc.NOT_CANDIDATE).all(), tag
        stopped = (counts & pack.HEADROOM_STOPPED) != 0
        assert (stages[stopped] == pack.LIMIT_NONE).all(), tag
        assert np.array_equal(stages[~stopped].astype(np.int64), want_st[~stopped]), (tag, np.argwhere(~stopped & (stages != want_st))[:8].tolist())
        p_sums, p_counts = eng.headroom(reqs, cand=cand, max_per_node=HEADROOM_CAP, per_node=True)
        plain = hc.oracle_synth(r.cfg, r.n, specs, cap=HEADROOM_CAP, procs=1, maybe=todo)
        assert np.array_equal(p_counts.astype(np.int64), plain), (tag, np.argwhere(p_counts != plain)[:8].tolist())
        assert p_sums.tobytes() == sums.tobytes(), tag
        out[label] = int((want_k & pack.HEADROOM_COUNT_MASK).sum())
    eng.close()
    return out


def headroom_masks(r):
    """Three masks for headroom: the island, only the last node, the straddle of the last boundary (the one-node chunk of rungs A
    and B).  (Not none: the Python oracle's loop takes a minute for all 513 nodes of rung B.)"""
    return ["island", "only the last node", f"straddle {r.chunks - 1}"]
