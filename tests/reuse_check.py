"""For the tests that hold ONE context to the oracles while its mirror is replaced under it (tests/test_reuse.py on the host twins,
tests/test_reuse_gpu.py on the device).  Every other device test builds a fresh context per case; the product empties the same context
(Engine.reset_nodes -> nhdfit_set_node_count(0)), sends another dictionary and uploads another cluster whenever a node joins or leaves
(HipMatcher._full_upload).  What a context carries across that seam: the padding lanes of the last chunk, the class table behind the
node records, the origin records, the wide records, the shadow of the candidate mask the small finds keep, buffers sized for the
larger mirror.

Chain 1 (same dictionary): one config-4 cluster X of 257 nodes; the context holds X[0:257], then X[0:65] (emptied and uploaded, or
  truncated), then X[0:129] (X[65:129] appended at 65, within the capacity), then the cut X[0:40] + X[164:257] (133 nodes: three chunks, as the
  129 nodes in front of it - the candidate words of one stop fit the next).  At the 65-node stop the
  lanes 65..127 of the device's second chunk still hold live nodes of X.  (257, not 193: of config 4's 193-node cluster node 191 fits
  all 136 pods, so the straddle mask of its last boundary has no winner beyond it; 257 is the smallest multiple of 64 plus 1 at which
  every straddle mask of every stop has winners on both sides - tests/test_reuse.py asserts it from the oracle alone.)
Chain 2 (the dictionary changes): the seam rungs D (config 5, 8 197 nodes, 151 signatures) -> A (config 4, 65 nodes, 9) -> C (config 3,
  2 049) -> B (config 5, 513) through one context.

Every answer is bit-exact against the oracles tests/seam_check.py and tests/edge_check.py use: the C oracle for winners, verdict matrix
and stages (on `coracle.Cluster.subset`, the masked view), the Python oracle for every winner's mapping, independent_limit for
headroom, the host twin for raw records and statuses.  A View is a Rung's cluster cut to some of its nodes, with the Rung's interface
as far as the seam checks use it."""
import functools

import numpy as np

from nhd_amd import pack
from oracle import coracle
from tests import edge_check as C
from tests import harness
from tests import headroom_limit_check as lc
from tests import seam_check as S
from tests.headroom_check import four_templates
from workload import planes, refmodel

FORMS = ["staged", "k_findn", "k_find", "k_find1", "scores only"]
X_CFG, X_N = 4, 257                       # the smallest multiple of 64 plus 1 the conditions of tests/test_reuse.py hold at
STOPS = ["whole", "shrunk", "grown", "cut"]
HEADROOM_CAP = S.HEADROOM_CAP
PLANES = ("p0", "p1", "p2", "p3", "p4", "detail")
CHAIN2 = ["D", "A", "C", "B"]


def take(table, idx):
    """The rows `idx` of a node table as a table of their own (copies; origin records included)."""
    idx = np.asarray(idx)
    return pack.NodeTable([table.names[i] for i in idx] if table.names else [], *[np.array(getattr(table, f)[idx]) for f in PLANES],
                          None if table.origin is None else np.array(table.origin[idx]))


class View:
    """The nodes `idx` (ascending indices into a Rung's cluster) as a cluster of their own: what a context holds at one stop."""

    def __init__(self, rung, idx, name):
        self.rung, self.idx, self.name = rung, np.asarray(idx), name
        self.n, self.chunks = len(self.idx), (len(self.idx) + 63) // 64
        self.cfg, self.now, self.P, self.n_small, self.G = rung.cfg, rung.now, rung.P, rung.n_small, rung.G
        self.opods, self.specs = rung.opods, rung.specs
        self.member = np.zeros(rung.n, bool)
        self.member[self.idx] = True
        self.local = np.full(rung.n, -1, np.int64)
        self.local[self.idx] = np.arange(self.n)
        self.cl = rung.cl.subset(self.member)
        self.has_gpu = rung.has_gpu[self.idx]

    def full(self, keep):
        """A mask over this view's nodes (None: all of them) as a mask over the rung's cluster."""
        out = np.zeros(self.rung.n, bool)
        out[self.idx] = True if keep is None else np.asarray(keep, bool)
        return out

    def oracle_winners(self, keep, pods=None):
        w = self.rung.oracle_winners(self.full(keep), pods)
        return np.where(w >= 0, self.local[np.maximum(w, 0)], -1)

    def oracle_matrix(self, keep):
        f = self.rung.feas()[:, self.idx]
        return f if keep is None else f & np.asarray(keep, bool)[None, :]

    def mapping(self, node, pod):
        return self.rung.mapping(self.idx[int(node)], pod)

    def prefetch_mappings(self, masks):
        pass                                                 # (a few hundred pairs of config 4: the rung memoises them)

    def straddle(self, c):
        keep = np.zeros(self.n, bool)
        keep[64 * c - 1:] = True
        return keep

    def island(self):
        far = int(np.flatnonzero(~self.has_gpu)[-1])
        keep = np.zeros(self.n, bool)
        keep[:64] = self.has_gpu[:64]
        keep[far] = True
        return keep, far

    def masks(self):
        """Rung.masks' list for this view: none, all zero, only the last node, the island, a straddle per chunk boundary."""
        none, last = np.zeros(self.n, bool), np.zeros(self.n, bool)
        last[self.n - 1] = True
        return [("none", None), ("all zero", none), ("only the last node", last), ("island", self.island()[0])] + \
               [(f"straddle {c}", self.straddle(c)) for c in range(1, self.chunks)]


def few_masks(v):
    """A short list shaped like seam_check.few_masks: none, all zero, the island, the first and the last straddle."""
    masks = v.masks()
    cuts = [m for m in masks if m[0].startswith("straddle")]
    return [masks[0], masks[1], masks[3], cuts[0]] + ([cuts[-1]] if len(cuts) > 1 else [])


# ---- chain 1 -----------------------------------------------------------------------------------------------------------------------------
class Chain1:
    """Cluster X, its 130 + 6 pods and four headroom templates digested into ONE packer with its signatures closed (built once, never
    changed), and the view of every stop."""

    def __init__(self):
        self.x = S.Rung("X", X_CFG, X_N)
        self.templates = four_templates(X_CFG)
        self.ttops = [refmodel.make_topology(s) for s in self.templates]
        self.pk = pack.Packer()
        self.table = planes.planes_from_spec(self.pk, self.x.spec)
        self.reqs = self.pk.digest_many(self.x.tops, self.x.groups)
        self.treqs = self.pk.digest_many(self.ttops, None)
        self.pk.close_signatures()
        cut = np.r_[0:40, X_N - 93:X_N]
        self.views = {"whole": View(self.x, np.arange(X_N), f"X[0:{X_N}]"), "shrunk": View(self.x, np.arange(65), "X[0:65]"),
                      "grown": View(self.x, np.arange(129), "X[0:129]"), "cut": View(self.x, cut, f"X[0:40] + X[{X_N - 93}:{X_N}]")}

    def padding_figures(self):
        """By the C oracle alone, for the 65-node stop: (nodes of X[65:128] feasible for at least 10 pods, {mask: pods whose winner
        would be one of those nodes if the lanes 65..127 of the second chunk - where the device still holds them, and where every
        candidate mask of the C-ABI has its bits set - were read})."""
        v = self.views["shrunk"]
        stale = np.zeros(X_N, bool)
        stale[65:128] = True
        nodes = int((self.x.feas()[:, 65:128].sum(0) >= 10).sum())
        moved = {}
        for label, keep in v.masks():
            inside = self.x.oracle_winners(v.full(keep))
            leaked = self.x.oracle_winners(v.full(keep) | stale)
            moved[label] = int(((leaked != inside) & (leaked >= 65) & (leaked < 128)).sum())
        return nodes, moved

    def straddle_figures(self):
        """{stop: {label: (pods that win in front of the boundary, pods that win at or beyond it)}} for every straddle mask of every stop."""
        out = {}
        for stop, v in self.views.items():
            out[stop] = {}
            for label, keep in v.masks():
                if label.startswith("straddle"):
                    c = int(label.split()[1])
                    w = v.oracle_winners(keep)
                    out[stop][label] = (int(((w >= 0) & (w < 64 * c)).sum()), int((w >= 64 * c).sum()))
        return out


@functools.lru_cache(maxsize=None)
def chain1():
    return Chain1()


def install_stop(c, eng, stop, by_truncate=False):
    """Brings the ONE engine of chain 1 to `stop` the way the chain says."""
    v = c.views[stop]
    if stop == "whole":
        eng.upload(take(c.table, v.idx))
    elif stop == "shrunk":
        if by_truncate:
            eng.truncate(65)
        else:
            eng.reset_nodes()
            eng.upload(take(c.table, v.idx))
    elif stop == "grown":
        eng.upload(take(c.table, np.arange(65, 129)), first=65)         # within the capacity of 257: the node count grows in place
    else:
        eng.reset_nodes()
        eng.upload(take(c.table, v.idx))
    assert eng.n == v.n
    return v


# ---- the forms of a find, the form that ran asserted where the engine has statistics (the device) ---------------------------------------
def counted(eng, field, step, call):
    if not hasattr(eng, "stats"):
        return call()
    before = eng.stats()
    out = call()
    after = eng.stats()
    moved = {f: getattr(after, f) - getattr(before, f) for f in ("small_finds", "batch_finds")}
    assert moved == {"small_finds": step if field == "small_finds" else 0, "batch_finds": step if field == "batch_finds" else 0}, (field, moved)
    return out


def one_by_one(eng, reqs, pods, now, cand):
    score, maps = np.zeros(len(pods), np.uint64), np.zeros(len(pods), pack.MAPPING)
    for k, p in enumerate(pods):
        s, _, mp = eng.find(reqs[p:p + 1], now, cand=cand, want_bitmap=False, want_map=True)
        score[k], maps[k] = s[0], mp[0]
    return score, None, maps


def run_form(r, eng, pk, reqs, form, masks, base=0):
    """tests/test_seams_gpu.py run_form on a Rung or a View: one form of nhdfit_find under `masks`, through seam_check.check_find (which
    also holds the bits at and beyond n of the last chunk's bitmap words to zero)."""
    small = np.arange(r.n_small)
    if form == "staged":
        pods = np.arange(r.P)
        return S.walk(r, lambda cand: counted(eng, None, 0, lambda: eng.find(reqs, r.now, cand=cand, want_bitmap=True, want_map=True)), pods, form, masks, base)
    if form == "k_findn":
        return S.walk(r, lambda cand: counted(eng, "batch_finds", 1, lambda: eng.find(reqs[small], r.now, cand=cand, want_bitmap=False, want_map=True)), small, form, masks, base)
    if form == "k_find":
        pods = small[:64]
        return S.walk(r, lambda cand: counted(eng, "small_finds", 1, lambda: eng.find(reqs[pods], r.now, cand=cand, want_bitmap=False, want_map=True)), pods, form, masks, base)
    if form == "k_find1":
        assert S.dictionary_fits_a_block(pk)
        pods = small[::3]
        return S.walk(r, lambda cand: counted(eng, "small_finds", len(pods), lambda: one_by_one(eng, reqs, pods, r.now, cand)), pods, form, masks, base)
    assert form == "scores only"
    S.walk(r, lambda cand: counted(eng, "batch_finds", 1, lambda: eng.find(reqs[small], r.now, cand=cand, want_bitmap=False, want_map=False)), small, form, masks, base)
    return S.walk(r, lambda cand: counted(eng, "small_finds", 1, lambda: eng.find(reqs[small[64:128]], r.now, cand=cand, want_bitmap=False, want_map=False)), small[64:128], form, masks, base)


def check_carried_mask(v, eng, reqs, words):
    """The candidate words the previous stop's last small find uploaded, sent again unchanged as this stop's first small find: where
    the chunk count is the same the library compares them with its shadow and uploads nothing (upload_small_cand)."""
    if words is None or len(words) != v.chunks:
        return False
    keep = np.unpackbits(words.view(np.uint8), bitorder="little")[:v.n].astype(bool)
    assert S.mask_words(keep).tobytes() == words.tobytes()
    pods = np.arange(64)
    score, _, maps = counted(eng, "small_finds", 1, lambda: eng.find(reqs[pods], v.now, cand=words, want_bitmap=False, want_map=True))
    S.check_find(v, pods, keep, score, None, maps, f"{v.name}, the previous stop's mask re-sent")
    return True


def last_small_find(v, eng, reqs):
    """This stop's last small find, under its last straddle mask: (the words it uploaded, pods placed)."""
    label, keep = v.masks()[-1]
    words = S.mask_words(keep)
    pods = np.arange(64)
    score, _, maps = counted(eng, "small_finds", 1, lambda: eng.find(reqs[pods], v.now, cand=words, want_bitmap=False, want_map=True))
    won = S.check_find(v, pods, keep, score, None, maps, f"{v.name}, last small find, mask {label}")
    return words, int((won >= 0).sum())


def check_find_commit(v, eng, pk, reqs, table):
    """nhdfit_find_commit (the twin: find, then commit) for the first pod the oracle places in the LAST chunk under the last straddle
    mask: score and mapping against the oracles, the one launch by its counter, placement and the node's records against a fresh host
    twin of this stop's table.  The node is put back afterwards (a one-node slice inside the mirror) and read back."""
    label, keep = v.masks()[-1]
    words = S.mask_words(keep)
    want = v.oracle_winners(keep)[:v.n_small]
    p = int(np.flatnonzero(want >= 64 * (v.chunks - 1))[0])
    node = int(want[p])
    if hasattr(eng, "find_commit"):
        assert S.dictionary_fits_a_block(pk)
        before = eng.find_commit_counts()
        score, mp, place, done = eng.find_commit(reqs[p], v.now, v.now, cand=words)
        after = eng.find_commit_counts()
        assert (after[0] - before[0], after[1] - before[1]) == (1, 0), (v.name, "the one-launch form did not run")
        assert done
    else:
        s, _, m = eng.find(reqs[p:p + 1], v.now, cand=words, want_bitmap=False, want_map=True)
        score, mp = int(s[0]), m[0]
        place = eng.commit(node, reqs[p], mp, v.now)
    S.check_find(v, [p], keep, np.array([score], np.uint64), None, np.array([mp]), f"{v.name}, find_commit, mask {label}")
    assert int(place["status"]) == pack.COMMIT_OK
    twin = harness.HarnessEngine(0)
    twin.set_dictionary(pk)
    twin.upload(table)
    assert twin.commit(node, reqs[p], mp, v.now).tobytes() == place.tobytes(), v.name
    got, ref = eng.download(node, 1), twin.download(node, 1)
    for f in PLANES:
        assert getattr(got, f).tobytes() == getattr(ref, f).tobytes(), (v.name, f)
    eng.upload(table.slice(node, node + 1), first=node, capacity=eng.n)
    back = eng.download(node, 1)
    for f in PLANES:
        assert getattr(back, f).tobytes() == getattr(table, f)[node:node + 1].tobytes(), (v.name, f)
    return node


def check_headroom_view(c, v, eng, labels):
    """seam_check.check_headroom for a view of chain 1, on the engine as it stands (the templates are in the chain's packer): entries
    and limit stages of nhdfit_headroom_limits, and the plain entry's figures, against independent_limit on X's own nodes
    (headroom_limit_check.oracle_synth); a pair without room has the C stage oracle's stage with nothing busy; nodes outside the
    mask read 0 / NOT_CANDIDATE.  Returns the replicas the oracle counts under each mask."""
    opods = c.x.cl.pods_from_tops(c.ttops, None)
    idle = v.now + 1.0e6
    feas = v.cl.find(opods, idle, threads=coracle.usable_cpus())[1].astype(bool)
    masks = dict(v.masks())
    union = np.zeros(v.n, bool)
    for label in labels:
        union |= np.ones(v.n, bool) if masks[label] is None else masks[label]
    todo_x = np.zeros((len(c.templates), c.x.n), bool)
    todo_x[:, v.idx] = feas & union[None, :]
    all_k, all_st = lc.oracle_synth(X_CFG, X_N, c.templates, todo_x, cap=HEADROOM_CAP, procs=1)
    all_k, all_st = all_k[:, v.idx], all_st[:, v.idx]
    out = {}
    for label in labels:
        keep = np.ones(v.n, bool) if masks[label] is None else masks[label]
        cand = None if masks[label] is None else S.mask_words(keep)
        todo = feas & keep[None, :]
        stage0 = v.cl.explain(opods, idle, cand=keep, per_node=True, threads=coracle.usable_cpus())[1]
        want_k, want_st = np.where(todo, all_k, 0), np.where(todo, all_st, stage0)
        sums, counts, hist, stages = eng.headroom_limits(c.treqs, cand=cand, max_per_node=HEADROOM_CAP, per_node=True)
        tag = (v.name, label)
        assert np.array_equal(counts.astype(np.int64), want_k), (tag, np.argwhere(counts != want_k)[:8].tolist())
        assert not counts[:, ~keep].any() and (stages[:, ~keep] == lc.NOT_CANDIDATE).all(), tag
        stopped = (counts & pack.HEADROOM_STOPPED) != 0
        assert (stages[stopped] == pack.LIMIT_NONE).all(), tag
        assert np.array_equal(stages[~stopped].astype(np.int64), want_st[~stopped]), (tag, np.argwhere(~stopped & (stages != want_st))[:8].tolist())
        p_sums, p_counts = eng.headroom(c.treqs, cand=cand, max_per_node=HEADROOM_CAP, per_node=True)
        assert np.array_equal(p_counts.astype(np.int64), want_k), (tag, np.argwhere(p_counts != want_k)[:8].tolist())
        assert p_sums.tobytes() == sums.tobytes(), tag
        out[label] = int((want_k & pack.HEADROOM_COUNT_MASK).sum())
    return out


def drive_chain1(eng, by_truncate):
    """All four stops of chain 1 on `eng` (its dictionary set, nothing uploaded).  Returns the figures of the run."""
    c = chain1()
    eng.set_dictionary(c.pk)
    words, fig = None, {}
    for stop in STOPS:
        v = install_stop(c, eng, stop, by_truncate)
        table = take(c.table, v.idx)
        masks = few_masks(v)
        carried = check_carried_mask(v, eng, c.reqs, words)
        placed = 0
        for form in FORMS:
            placed += sum(int((w >= 0).sum()) for _, w in run_form(v, eng, c.pk, c.reqs, form, masks))
        S.check_explain(v, eng, c.reqs, ["none", "island", masks[-1][0]])
        node = check_find_commit(v, eng, c.pk, c.reqs, table)
        fig[stop] = {"nodes": v.n, "winners checked": placed, "carried mask": carried, "find_commit on node": node}
        if stop == "shrunk":
            fig[stop]["replicas"] = check_headroom_view(c, v, eng, S.headroom_masks(v))
        words, last = last_small_find(v, eng, c.reqs)
        assert placed >= 10 * len(masks) and last >= 1
    return fig


# ---- chain 2 -----------------------------------------------------------------------------------------------------------------------------
def class_count(table):
    """Distinct (socket, free GPUs on it, NUMA-mode signature, PCI-mode signature) tuples of a packed table: the node classes the
    device interns for it (fit_core.h xkey), before the clamp of the GPU count to the dictionary's table."""
    free, numa1 = table.p2["gpu_free"], table.p2["gpu_numa1"]
    seen = set()
    for u in range(2):
        f = np.array([bin(int(x)).count("1") for x in (free & numa1 if u else free & ~numa1)])
        seen |= {(u, int(a), int(b), int(c)) for a, b, c in zip(f, table.p3["sig_numa"][:, u], table.p3["sig_pci"][:, u])}
    return len(seen)


def make_layout(W, max_cores, max_gpus, nsig, ngs, hp_rows, x_cap):
    """fit_core.h make_layout: the byte offsets of a tile image of W assignments per row."""
    align16 = lambda x: (x + 15) & ~15
    row, fc_dim, fg_dim = W * 8, max_cores + 1, max_gpus + 1
    wc_stride, x_stride = 2 * W * 8 + 16, 16 if W == 2 else W * 8 + 16
    off_a1 = fg_dim * row
    off_r0 = off_a1 + fg_dim * row
    off_r1 = off_r0 + nsig * row
    off_hot = align16(off_r1 + nsig * row)
    hot_x = 4 * fc_dim * wc_stride + align16((1 + 2 * ngs) * 8)
    hot_bytes = hot_x + x_cap * x_stride + align16(hp_rows * 8)
    return {"row": row, "off_a1": off_a1, "off_r1": off_r1, "off_hot": off_hot, "bytes": off_hot + hot_bytes}


def stale_row_reach(prev_tables, pk):
    """Had the classes of `prev_tables` stayed in the table (they did until nhdfit_set_node_count forgot them), the digest role would
    form an X row for each from `off_r1 + sig * row` and `off_a1 + free GPUs * row` of a tile image laid out for `pk`'s dictionary
    (step_digest.h): per row width W (the furthest byte such a read ends at, the image's size with the fewest X rows a context
    provisions, 32, and two hugepage rows - the smallest image)."""
    sig = max(int(max(t.p3["sig_numa"].max(), t.p3["sig_pci"].max())) for t in prev_tables)
    free = max(max(bin(int(x)).count("1") for x in t.p2["gpu_free"]) for t in prev_tables)
    nsig = int(pk.dictionary_arrays()[6])
    out = {}
    for W in (2, 4, 8, 16):
        L = make_layout(W, pk.max_cores_per_numa, pk.max_gpus_per_numa, nsig, max(1, len(pk.group_sets)), 2, 32)
        out[W] = (max(L["off_r1"] + (sig + 1) * L["row"], L["off_a1"] + (free + 1) * L["row"]), L["bytes"])
    return sig, out


def install_rung(eng, name, forget):
    r = S.rung(name)
    pk, table, reqs = r.packed()
    eng.reset_nodes()
    if forget:
        eng.forget_dictionary()
    eng.set_dictionary(pk)
    eng.upload(table)
    return r, pk, table, reqs


class Lent:
    """An engine handed to a check that closes what it is given: everything but close()."""

    def __init__(self, eng):
        self._eng = eng

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def close(self):
        pass


STAT_FIELDS = ("nodes", "nsig", "ncls", "lds_bytes")


def staged_stats(eng, r, reqs):
    """The statistics a staged find of all pods leaves (unmasked; its answer checked)."""
    score, bm, maps = eng.find(reqs, r.now, want_bitmap=True, want_map=True)
    S.check_find(r, np.arange(r.P), None, score, bm, maps, f"rung {r.name}, staged, for the statistics")
    st = eng.stats()
    return {f: int(getattr(st, f)) for f in STAT_FIELDS}


def drive_chain2(eng, forget, fresh_factory=None):
    """D -> A -> C -> B through `eng`.  `fresh_factory` (the device): a context of its own per stop, given the same stop, whose
    statistics after the same staged find the reused context's must equal."""
    fig = {}
    for name in CHAIN2:
        r, pk, table, reqs = install_rung(eng, name, forget)
        if fresh_factory is not None:
            fresh = fresh_factory()
            fresh.set_dictionary(pk)
            fresh.upload(table)
            want = staged_stats(fresh, r, reqs)
            fresh.close()
            got = staged_stats(eng, r, reqs)
            assert got == want, (name, got, want)
            fig[name] = got
        if name == "D":                                          # only the previous occupant: the seam tests own the rest
            small = np.arange(r.n_small)
            score, _, maps = counted(eng, "batch_finds", 1, lambda: eng.find(reqs[small], r.now, want_bitmap=False, want_map=True))
            S.check_find(r, small, None, score, None, maps, "rung D, k_findn")
            score, bm, maps = eng.find(reqs, r.now, want_bitmap=True, want_map=True)
            S.check_find(r, np.arange(r.P), None, score, bm, maps, "rung D, staged")
            continue
        for form in FORMS:
            won = run_form(r, eng, pk, reqs, form, S.few_masks(r))
            assert sum(int((w >= 0).sum()) for _, w in won) >= 10
        S.check_explain(r, eng, reqs, S.explain_masks(r))
        if name in "AB":
            def lend():
                eng.reset_nodes()
                if forget:
                    eng.forget_dictionary()
                return Lent(eng)
            got = S.check_headroom(r, lend, four_templates(r.cfg), S.headroom_masks(r))
            assert got["island"] >= 20 and got["only the last node"] >= 1
    return fig


# ---- origin records and deltas across the seam -----------------------------------------------------------------------------------------------
def draw_deltas(table, now, n, seed=11):
    """A RESET first, then n TAKE / GIVE / RESET / scalar deltas drawn as test_apply_deltas_through_the_abi draws them."""
    rng = np.random.default_rng(seed)
    d = np.zeros(n + 1, pack.DELTA)
    d["node"] = rng.integers(0, table.n, n + 1)
    d["op"] = rng.choice([pack.DELTA_TAKE, pack.DELTA_GIVE, pack.DELTA_RESET, pack.DELTA_SET_FLAGS, pack.DELTA_SET_BUSY, pack.DELTA_SET_HUGEPAGES],
                         size=n + 1, p=[0.35, 0.35, 0.05, 0.1, 0.1, 0.05])
    d["op"][0] = pack.DELTA_RESET
    valid = table.origin["t0"][d["node"]]
    d["t0"] = rng.integers(0, 1 << 62, (n + 1, 2)).astype(np.uint64) & valid
    d["t1"] = rng.integers(0, 1 << 62, (n + 1, 2)).astype(np.uint64) & valid
    d["gpus"] = rng.integers(0, 16, n + 1)
    d["hugepages_gb"] = rng.integers(0, 9, n + 1)
    d["hp_total"] = 64
    d["flags_mask"] = pack.NF_MAINTENANCE | pack.NF_ACTIVE
    d["flags_value"] = rng.integers(0, 4, n + 1)
    d["busy_time"] = now - rng.integers(0, 100, n + 1)
    d["nic_n"] = rng.integers(0, 3, n + 1)
    d["nic"][:, 0] = (rng.integers(0, 2, n + 1) << 4) | rng.integers(0, 2, n + 1)
    d["nic"][:, 1] = (rng.integers(0, 2, n + 1) << 4) | rng.integers(0, 2, n + 1)
    return d


def without_origin(table):
    return pack.NodeTable(list(table.names), *[np.array(getattr(table, f)) for f in PLANES], None)


def check_origin_across_the_seam(eng, fresh_factory, error):
    """D -> A on `eng`, A's table uploaded as Engine.download returns it (no origin records): apply_deltas fails with NHDFIT_E_STATE
    as on a fresh context - on the parent it went through, against D's origin records.  Then A's own origin records go up and a RESET
    plus 300 deltas leave statuses and all six planes as harness.apply_deltas leaves them, and a find equals a fresh context's that
    was given the final planes."""
    d_rung, a_rung = S.rung("D"), S.rung("A")
    pk_d, table_d, _ = d_rung.packed()
    pk, table, reqs = a_rung.packed()
    assert table_d.origin is not None and table.origin is not None
    reset = np.zeros(1, pack.DELTA)
    reset["node"], reset["op"] = 7, pack.DELTA_RESET
    for ctx, was_d in ((fresh_factory(), False), (eng, True)):
        if was_d:
            ctx.set_dictionary(pk_d)
            ctx.upload(table_d)
            ctx.reset_nodes()
        ctx.set_dictionary(pk)
        ctx.upload(without_origin(table))
        try:
            ctx.apply_deltas(reset)
        except error as e:
            assert e.code == -5, (was_d, e)                     # NHDFIT_E_STATE
        else:
            raise AssertionError(("a RESET went through without origin records", "reused context" if was_d else "fresh context"))
        got = ctx.download()
        for f in PLANES:
            assert getattr(got, f).tobytes() == getattr(table, f).tobytes(), (was_d, f)
        if not was_d:
            ctx.close()
    eng.upload(table)                                            # A's own origin records
    deltas = draw_deltas(table, a_rung.now, 300)
    status = eng.apply_deltas(deltas)
    twin = pack.NodeTable(list(table.names), *[np.array(getattr(table, f)) for f in PLANES + ("origin",)])
    want = harness.apply_deltas(pk, twin, deltas)
    assert np.array_equal(status, want)
    assert (status == pack.DELTA_OK).sum() > 100
    got = eng.download()
    for f in PLANES:
        assert getattr(got, f).tobytes() == getattr(twin, f).tobytes(), f
    fresh = fresh_factory()
    fresh.set_dictionary(pk)
    fresh.upload(twin)
    for cand in (None, S.mask_words(a_rung.straddle(1))):
        a = eng.find(reqs, a_rung.now, cand=cand, want_bitmap=True, want_map=True)
        b = fresh.find(reqs, a_rung.now, cand=cand, want_bitmap=True, want_map=True)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        s1 = eng.find(reqs[:64], a_rung.now, cand=cand, want_bitmap=False, want_map=True)
        s2 = fresh.find(reqs[:64], a_rung.now, cand=cand, want_bitmap=False, want_map=True)
        assert s1[0].tobytes() == s2[0].tobytes() and s1[2].tobytes() == s2[2].tobytes()
    fresh.close()
    return {"deltas": len(deltas), "ok": int((status == pack.DELTA_OK).sum()), "repack": int((status == pack.DELTA_REPACK).sum())}


def check_gap_refusals(eng, error):
    """Engine.upload (or the twin's) refuses a slice behind a gap and a slice at first > 0 that would grow the capacity, the mirror
    byte-identical afterwards."""
    r = S.rung("A")
    pk, table, _ = r.packed()
    eng.set_dictionary(pk)
    eng.upload(table.slice(0, 40), capacity=50)
    before = eng.download()
    for first, count in ((41, 5), (40, 20), (10, 45)):           # a gap; appended beyond the capacity; inside, but beyond the capacity
        try:
            eng.upload(table.slice(first, first + count), first=first)
        except error as e:
            assert e.code == -1, e                               # NHDFIT_E_INVAL
        else:
            raise AssertionError((first, count, "not refused"))
        assert eng.n == 40
        after = eng.download()
        for f in PLANES:
            assert getattr(after, f).tobytes() == getattr(before, f).tobytes(), (first, f)
    eng.upload(table.slice(40, 50), first=40)                    # appended within the capacity: taken
    got = eng.download()
    assert eng.n == 50
    for f in PLANES:
        assert getattr(got, f).tobytes() == getattr(table, f)[:50].tobytes(), f


# ---- wide records across the seam, on one matcher -----------------------------------------------------------------------------------------------
def wide_steps(case):
    return [("whole", np.ones(case.n, bool)), ("fast layout", ~case.wide), ("dictionary in LDS", ~case.wide & case.fits_lds),
            ("whole again", np.ones(case.n, bool))]


def check_wide_step(m, case, tag, member):
    """HipMatcher._full_upload of the nodes `member` of the 600-node edge cluster on the matcher as it stands, then the staged form
    and the single-launch forms that mirror admits under edge_check.masks_of, and the wide records against the packer's own count."""
    from workload import edge_inputs as E
    m._full_upload(case.sub(member))
    ctx = np.flatnonzero(member)
    assert m._names == [case.names[i] for i in ctx] and not m.unmirrored
    n_wide = int(case.wide[member].sum())
    assert len(m._table.wide or {}) == n_wide and m.engine.wide_count() == n_wide, tag
    lone = tag == "dictionary in LDS"
    if lone:
        m.packer.close_signatures()
        m.engine.set_dictionary(m.packer)
    small = [p for p in range(case.PODS) if not case.general[p]]
    single = [p for p in range(case.ALL_PODS) if not case.general[p] and case.G[p] <= 3]
    placed = 0
    for label, keep in C.masks_of(case):
        cand = None if keep is None else E.mask_words(keep[ctx])
        reqs = m.packer.digest_many([case.tops[p] for p in small])
        score, bm, maps = counted(m.engine, None, 0, lambda: m.engine.find(reqs, C.NOW, cand=cand, want_bitmap=True, want_map=True))
        placed += C.check_find(case, ctx, small, keep, score, bm, maps, f"{tag}, staged, {label}")
        if n_wide:
            continue                                             # (a mirror with wide records takes neither single-launch form)
        reqs = m.packer.digest_many([case.tops[p] for p in single])
        score, _, maps = counted(m.engine, "batch_finds", 1, lambda: m.engine.find(reqs, C.NOW, cand=cand, want_bitmap=False, want_map=True))
        placed += C.check_find(case, ctx, single, keep, score, None, maps, f"{tag}, single-launch batch, {label}")
        if lone:
            pods = single[::3]
            score, _, maps = counted(m.engine, "small_finds", len(pods), lambda: one_by_one(m.engine, reqs, range(0, len(single), 3), C.NOW, cand))
            placed += C.check_find(case, ctx, pods, keep, score, None, maps, f"{tag}, one-pod launch, {label}")
    return placed


def check_wide_truncate(m, case):
    """On the whole cluster: the mirror cut to one past its last wide record, then to a count between two wide records - the wide
    records read back are the prefix, and a staged find is the oracle's on those nodes."""
    recs = m.engine.wide_download()
    idx = recs["index"].astype(np.int64)
    assert len(idx) == int(case.wide.sum()) and (np.diff(idx) > 0).all()
    k = next(k for k in range(len(idx) // 2, len(idx) - 1) if idx[k + 1] - idx[k] >= 2)
    small = [p for p in range(case.PODS) if not case.general[p]]
    reqs = m.packer.digest_many([case.tops[p] for p in small])
    out = []
    for n in (int(idx[-1]) + 1, int(idx[k + 1])):
        m.engine.truncate(n)
        keep = recs[idx < n]
        assert m.engine.n == n and m.engine.wide_count() == len(keep) == m.engine.n_wide
        assert m.engine.wide_download().tobytes() == keep.tobytes(), n
        score, bm, maps = m.engine.find(reqs, C.NOW, want_bitmap=True, want_map=True)
        C.check_find(case, np.arange(n), small, None, score, bm, maps, f"truncated to {n}")
        out.append((n, len(keep)))
    assert out[1][1] == k + 1 < out[0][1] == len(idx)
    return out


EDGE_SEEDS = [0, 24, 22, 30, 5, 12]        # 24: nodes no record holds; 22: a STOPPED run; 30: NIC-heavy
