"""Thin object wrapper over the C-ABI: one :class:`Engine` = one nhdfit_ctx = one GPU."""
from __future__ import annotations

import ctypes
import operator
import weakref
from typing import Optional, Tuple

import numpy as np

from . import _lib, pack

SCORE_MASK = 0x7FFFFFFFFFFFFFFF
STAGES = 10                      # NHDFIT_STAGES of include/nhdfit.h (the stage codes: matcher.STAGES)


def _p(a: Optional[np.ndarray]):
    """Address of the array's buffer for a c_void_p parameter (every libnhdfit prototype is declared in _lib._SIGS, so a plain
    int converts; half the cost of .ctypes.data_as - this sits on FindNode's per-pod path).  The caller keeps `a` alive."""
    return None if a is None else a.ctypes.data


class Engine:
    def __init__(self, device: int = 0):
        self.lib = _lib.load()
        h = ctypes.c_void_p()
        rc = self.lib.nhdfit_create(device, ctypes.byref(h))
        if rc != 0:
            raise _lib.NhdFitError(rc, (self.lib.nhdfit_last_error(None) or b"?").decode())
        self.ctx = h
        self.device = device
        self.n = 0
        self.capacity = 0                # what nhdfit_reserve_nodes has been asked for so far (it only grows)
        self.P = 0
        self.global_base = 0
        self._dict_version = -1
        self._dict_of = None             # the packer that version belongs to (weakly held)
        self.n_wide = 0

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.nhdfit_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    def _chk(self, rc):
        _lib.check(self.ctx, rc)

    # ---- state ------------------------------------------------------------------------
    def set_dictionary(self, packer: pack.Packer):
        # (the version counts one packer's growth: two packers may well stand at the same count with different dictionaries)
        if self._dict_version == packer.dict_version and self._dict_of is not None and self._dict_of() is packer:
            return
        caps, sig_off, pool_off, glimit, cc, ncls, nsig, npools, ncc = packer.dictionary_arrays()
        gs = packer.group_set_array()
        self._chk(self.lib.nhdfit_set_dictionary(self.ctx, packer.max_cores_per_numa, packer.max_gpus_per_numa,
                                                 _p(gs), len(packer.group_sets), _p(caps), ncls, _p(sig_off), nsig, _p(pool_off), _p(glimit),
                                                 npools, _p(cc), ncc))
        self._dict_version = packer.dict_version
        self._dict_of = weakref.ref(packer)

    def forget_dictionary(self):
        """The next set_dictionary uploads whatever packer it is given (a NEW Packer restarts its version count)."""
        self._dict_version = -1

    def upload(self, table: pack.NodeTable, global_base: int = 0, first: int = 0, capacity: Optional[int] = None):
        """Full upload (first == 0 and nothing uploaded yet) or delta upload of `table` at `first`.  Under ENABLE_SHARING every slice
        carries its nodes' speed_used records (`table.share`, as download() returns them); a slice without them raises before anything
        on the device changes.  (A mirror that is to stop sharing is emptied first: reset_nodes.)"""
        sharing = getattr(self, "_share", None) is not None
        whole = first == 0 and table.n >= self.n
        if sharing and table.n and not table.share:
            # (a table packed with the constant off, or a restore from a download that lost the records: never continue with the
            #  shipped arithmetic silently - and never after nhdfit_wide_upload has already switched the sharing arithmetic off)
            raise _lib.NhdFitError(-5, "ENABLE_SHARING: the uploaded slice [%d, %d) carries no speed_used records" % (first, first + table.n))
        if table.share and len(table.share) != table.n:
            missing = next(i for i in range(table.n) if i not in table.share)
            raise _lib.NhdFitError(-5, "ENABLE_SHARING: node %d of the uploaded slice carries no speed_used record" % (first + missing))
        cap = max(capacity or 0, first + table.n)
        if first > self.n:
            # (nhdfit_upload_nodes refuses it too: nothing has been written to the nodes in between)
            raise _lib.NhdFitError(-1, "node records [%d,%d) are missing" % (self.n, first))
        if first > 0 and cap > self.capacity:
            # growing the capacity discards the mirror's contents: the slice would stand behind nodes that are gone
            raise _lib.NhdFitError(-1, "a slice at %d that grows the capacity from %d to %d would discard the nodes in front of it: "
                                   "upload the whole table" % (first, self.capacity, cap))
        self._chk(self.lib.nhdfit_reserve_nodes(self.ctx, cap, global_base))
        self.capacity = max(self.capacity, cap)
        arrs = [np.ascontiguousarray(x) for x in (table.p0, table.p1, table.p2, table.p3, table.p4, table.detail)]
        self._chk(self.lib.nhdfit_upload_nodes(self.ctx, first, table.n, *[_p(a) for a in arrs]))
        if table.origin is not None and table.n:
            origin = np.ascontiguousarray(table.origin)          # (bound to a name: _p hands out a bare address)
            self._chk(self.lib.nhdfit_upload_origin(self.ctx, first, table.n, _p(origin)))
        if sharing and not whole and self.n_wide:
            # ENABLE_SHARING, delta upload: device-side commits (wide_commit, schedule_batch) added rx / tx to speed_used records this
            # host copy has never seen - fetch them before nhdfit_wide_upload switches sharing off, so that the nodes OUTSIDE the slice
            # go back up as the device left them (a wide record showing the cores taken beside a speed_used that forgot the claim).
            # The fetch covers the slice's own nodes too, speculative commits of an apply=False batch included; the slice's records
            # are written over them below, so a restore puts back what it carries
            dev = self.wide_share_download()
            if len(dev):
                self._share[:len(dev)] = dev
        if table.n and (table.wide or self.n_wide):               # nodes beyond the fast layout: their records replace those of this range
            recs = table.wide_records(first)
            self._chk(self.lib.nhdfit_wide_upload(self.ctx, first, table.n, _p(recs) if len(recs) else None, len(recs)))
            self.n_wide = self.wide_count()
        self.n = max(self.n, first + table.n)
        # nhd/Node.py:20 ENABLE_SHARING = True: every node is a wide record and carries its NICs' speed_used (nhdfit_wide_share).  The
        # device wants the records of ALL wide nodes after every wide upload: this engine keeps them by node index
        if table.share:
            if not sharing or len(self._share) < self.n:
                grown = np.zeros(self.n, pack.WIDE_SHARE)
                if sharing:
                    grown[:len(self._share)] = self._share
                self._share = grown
            for i, rec in table.share.items():
                self._share[first + i] = rec
            if self.n_wide != self.n:
                raise _lib.NhdFitError(-5, "ENABLE_SHARING: a node of the mirror is not held by the general path")
            share = np.ascontiguousarray(self._share[:self.n])
            self._chk(self.lib.nhdfit_wide_share_upload(self.ctx, _p(share), len(share)))
        self.global_base = global_base

    def wide_count(self) -> int:
        k = ctypes.c_uint32(0)
        self._chk(self.lib.nhdfit_wide_count(self.ctx, ctypes.byref(k)))
        return int(k.value)

    def wide_download(self) -> np.ndarray:
        """The mirror's wide records (ascending node index) as they are now - after device-side commits."""
        k = ctypes.c_uint32(0)
        out = np.zeros(self.wide_count(), pack.WIDE)
        self._chk(self.lib.nhdfit_wide_download(self.ctx, _p(out) if len(out) else None, len(out), ctypes.byref(k)))
        return out

    def wide_share_download(self) -> np.ndarray:
        """The NICs' speed_used per wide record (ascending node index) as the device's commits left them; empty without ENABLE_SHARING."""
        k = ctypes.c_uint32(0)
        out = np.zeros(self.wide_count(), pack.WIDE_SHARE)
        self._chk(self.lib.nhdfit_wide_share_download(self.ctx, _p(out) if len(out) else None, len(out), ctypes.byref(k)))
        return out[:int(k.value)]

    def wide_commit(self, node: int, req: np.ndarray, mapping: np.ndarray, busy_time: float) -> np.ndarray:
        out = np.zeros((), pack.WIDE_PLACEMENT)
        req = np.ascontiguousarray(req)
        mapping = np.ascontiguousarray(mapping)
        self._chk(self.lib.nhdfit_wide_commit(self.ctx, int(node), _p(req), _p(mapping), float(busy_time), _p(out)))
        return out

    def wide_placements(self) -> np.ndarray:
        """Placements the last schedule_batch made on wide nodes (`pod` = index in that call's batch, `node` = local index)."""
        k = ctypes.c_uint32(0)
        self._chk(self.lib.nhdfit_wide_placements(self.ctx, None, 0, ctypes.byref(k)))
        out = np.zeros(int(k.value), pack.WIDE_PLACEMENT)
        if len(out):
            self._chk(self.lib.nhdfit_wide_placements(self.ctx, _p(out), len(out), ctypes.byref(k)))
        return out

    def apply_deltas(self, deltas: np.ndarray) -> np.ndarray:
        """K3 (nhdfit_apply_deltas): release / reclaim / reset / scalar writes applied to the device mirror in array order.
        `deltas["node"]` = local index.  Returns the per-delta status (pack.DELTA_OK / DELTA_REPACK)."""
        deltas = np.ascontiguousarray(deltas, dtype=pack.DELTA).reshape(-1)
        status = np.zeros(len(deltas), np.uint8)
        if len(deltas):
            self._chk(self.lib.nhdfit_apply_deltas(self.ctx, _p(deltas), len(deltas), _p(status)))
        return status

    @property
    def sharing(self) -> bool:
        """ENABLE_SHARING: the mirror holds speed_used records beside its wide records."""
        return getattr(self, "_share", None) is not None

    def reset_nodes(self):
        """An empty mirror: whether it shares NICs is up to the next upload (a table with or without speed_used records)."""
        self._chk(self.lib.nhdfit_set_node_count(self.ctx, 0))
        if getattr(self, "_share", None) is not None:
            self._chk(self.lib.nhdfit_wide_share_upload(self.ctx, None, 0))
            self._share = None
        self.n = 0
        self.n_wide = 0

    def truncate(self, n: int):
        """The mirror cut to its first `n` nodes (nhdfit_set_node_count): wide, speed_used and origin records past the new end go with
        their nodes; truncate(0) is reset_nodes()."""
        n = int(n)
        if n == 0:
            return self.reset_nodes()
        if n > self.n:
            raise _lib.NhdFitError(-1, "truncate(%d) of a mirror of %d nodes" % (n, self.n))
        self._chk(self.lib.nhdfit_set_node_count(self.ctx, n))
        self.n = n
        if self.n_wide:
            self.n_wide = self.wide_count()
        if getattr(self, "_share", None) is not None:
            self._share = self._share[:n].copy()          # (the device keeps the prefix of its own records, commits included)

    def set_outputs(self, bitmap=True, mapping=True):
        self._chk(self.lib.nhdfit_set_outputs(self.ctx, int(bitmap), int(mapping)))

    # ---- one-shot ---------------------------------------------------------------------
    def find(self, reqs: np.ndarray, now: float, cand: Optional[np.ndarray] = None, want_bitmap=True, want_map=True):
        reqs = np.ascontiguousarray(reqs)
        P = len(reqs)
        score = np.zeros(P, np.uint64)
        bitmap = np.zeros(((self.n + 63) // 64, P), np.uint64) if want_bitmap else None
        maps = np.zeros(P, pack.MAPPING) if want_map else None
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
            assert cand.shape == ((self.n + 63) // 64,)
        self._chk(self.lib.nhdfit_find(self.ctx, _p(reqs), P, float(now), _p(cand), _p(score), _p(bitmap), _p(maps)))
        self.P = P
        return score, bitmap, maps

    def find_sequential(self, reqs: np.ndarray, now: float, cand: Optional[np.ndarray] = None):
        """Mode B (sequential commit inside the batch): (node index or -1, mappings, status) per pod."""
        reqs = np.ascontiguousarray(reqs)
        P = len(reqs)
        node = np.zeros(P, np.int64)
        maps = np.zeros(P, pack.MAPPING)
        status = np.zeros(P, np.int32)
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
        self._chk(self.lib.nhdfit_find_sequential(self.ctx, _p(reqs), P, float(now), _p(cand), _p(node), _p(maps), _p(status)))
        self.P = P
        return node, maps, status

    def schedule_batch(self, reqs: np.ndarray, now: float, packer: pack.Packer, cand: Optional[np.ndarray] = None, apply: bool = True):
        """Mode B with the commit step on the device (nhdfit_schedule_batch): (node index or -1, mappings, placements,
        status) per pod.  apply=True leaves the commits in the device mirror.  A commit that puts a node into a NIC
        state the dictionary has no signature for stops the device pass; the state is interned here (`packer`), the
        node's plane 3 patched, and the pods that are left go out as a new batch (the mirror holds the placements made
        so far) - with Packer.close_signatures() up front this never happens."""
        reqs = np.ascontiguousarray(reqs)
        P = len(reqs)
        node = np.zeros(P, np.int64)
        maps = np.zeros(P, pack.MAPPING)
        places = np.zeros(P, pack.PLACEMENT)
        status = np.zeros(P, np.int32)
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
        first = 0
        self.last_wide_places = {}                                  # pod index of THIS call -> nhdfit_wide_placement (pods that landed on wide nodes)
        while first < P:
            done = ctypes.c_uint32(0)
            self._chk(self.lib.nhdfit_schedule_batch(self.ctx, _p(reqs[first:]), P - first, float(now), _p(cand), int(apply),
                                                     _p(node[first:]), _p(maps[first:]), _p(places[first:]), _p(status[first:]),
                                                     ctypes.byref(done)))
            last = first + done.value
            if self.n_wide:
                for wp in self.wide_placements():
                    self.last_wide_places[first + int(wp["pod"])] = wp.copy()
            # (vectorised: a Python loop over the pods here was 0.25-0.4 ms per 4 096 pods - a tenth of the whole call)
            stuck = (node[first:last][status[first:last] == pack.COMMIT_NEW_SIG] - self.global_base).tolist()
            if last < P and not (apply and stuck):
                raise _lib.NhdFitError(-5, "the device stopped a sequential batch early without a NIC state to intern")
            patched = []
            for v in stuck if apply else []:
                one = self.download(v, 1)
                sn, sp = packer.sigs_from_detail(one.detail[0])
                one.p3[0]["sig_numa"] = sn
                one.p3[0]["sig_pci"] = sp
                patched.append((v, one))
            if patched:
                self.set_dictionary(packer)
                for v, one in patched:
                    self.upload(one, global_base=self.global_base, first=v, capacity=self.n)
            first = last
        self.P = P
        return node, maps, places, status

    def commit(self, node: int, req: np.ndarray, mapping: np.ndarray, busy_time: float) -> np.ndarray:
        """The commit step for one placement (nhdfit_commit): updates the device mirror, returns the placement record."""
        out = np.zeros((), pack.PLACEMENT)
        req = np.ascontiguousarray(req)
        mapping = np.ascontiguousarray(mapping)
        self._chk(self.lib.nhdfit_commit(self.ctx, int(node), _p(req), _p(mapping), float(busy_time), _p(out)))
        return out

    def find_commit(self, req: np.ndarray, now: float, busy_time: float, cand: Optional[np.ndarray] = None, prev: Optional[Tuple[int, float]] = None):
        """FindNode for ONE pod and the commit step on its winner in one call (nhdfit_find_commit; one launch where the lone-pod form
        of the find applies): (score, mapping, placement, committed).  `req`: one pack.REQ record; `prev` = (local node index, busy
        time): as if a SET_BUSY delta for that node had been applied first."""
        req = np.ascontiguousarray(req).reshape(-1)[:1]
        score = np.zeros(1, np.uint64)
        maps = np.zeros(1, pack.MAPPING)
        place = np.zeros((), pack.PLACEMENT)
        done = ctypes.c_int(0)
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
            assert cand.shape == ((self.n + 63) // 64,)
        pn, pt = (-1, 0.0) if prev is None else (int(prev[0]), float(prev[1]))
        self._chk(self.lib.nhdfit_find_commit(self.ctx, _p(req), float(now), _p(cand), float(busy_time), pn, pt, _p(score), _p(maps), _p(place),
                                              ctypes.byref(done)))
        self.P = 1
        return int(score[0]), maps[0], place, bool(done.value)

    def find_commit_counts(self) -> Tuple[int, int]:
        """(fused, composed): find_commit calls of this context by the form they took (nhdfit_find_commit_counts)."""
        f, c = ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._chk(self.lib.nhdfit_find_commit_counts(self.ctx, ctypes.byref(f), ctypes.byref(c)))
        return int(f.value), int(c.value)

    # ---- pods with 5..8 processing groups: the general path over every node (nhdfit_big_find / nhdfit_big_commit) --------
    def big_find(self, reqs: np.ndarray, now: float, cand: Optional[np.ndarray] = None, want_map=True):
        """Mode A for big requests (pack.BIG_REQ): (scores, mappings pack.BIG_MAPPING)."""
        reqs = np.ascontiguousarray(reqs, dtype=pack.BIG_REQ)
        P = len(reqs)
        score = np.zeros(P, np.uint64)
        maps = np.zeros(P, pack.BIG_MAPPING) if want_map else None
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
            assert cand.shape == ((self.n + 63) // 64,)
        if P:
            self._chk(self.lib.nhdfit_big_find(self.ctx, _p(reqs), P, float(now), _p(cand), _p(score), _p(maps)))
        return score, maps

    # ---- the query entries: explain, headroom, headroom_general, headroom_limits -----------------------------------------------------
    def _query(self, fn, reqs: np.ndarray, cand: Optional[np.ndarray], outputs, before=(), after=(), last=()):
        """One query entry: allocates its outputs - `outputs`: per output (shape behind [P], dtype), or None for one the caller did not
        ask for - normalises and checks `cand`, and calls fn(ctx, reqs, P, *before, cand, *after, *outputs, *last).  Nodes outside
        `cand` are no candidates; nothing of the mirror changes."""
        P = len(reqs)
        outs = tuple(None if o is None else np.zeros((P,) + o[0], o[1]) for o in outputs)
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
            assert cand.shape == ((self.n + 63) // 64,)
        if P:
            self._chk(fn(self.ctx, _p(reqs), P, *before, _p(cand), *after, *[_p(o) for o in outs], *last))
        return outs

    def explain(self, reqs: np.ndarray, now: float, cand: Optional[np.ndarray] = None, per_node: bool = False):
        """(counts [P][STAGES] uint32, stages [P][n] uint8 or None) for ordinary (pack.REQ) or big (pack.BIG_REQ) requests: the stage
        at which each node turned each pod away (nhdfit_explain / nhdfit_explain_big).  Nodes outside `cand` count as NOT_CANDIDATE."""
        reqs = np.ascontiguousarray(reqs)
        fn = self.lib.nhdfit_explain_big if reqs.dtype == pack.BIG_REQ else self.lib.nhdfit_explain
        return self._query(fn, reqs, cand, [((STAGES,), np.uint32), ((self.n,), np.uint8) if per_node else None], before=(float(now),))

    def _headroom(self, fn, reqs, cand, max_per_node, per_node, limits=False, last=()):
        outputs = [((), pack.HEADROOM_SUM), ((self.n,), np.uint16) if per_node else None]
        if limits:
            outputs += [((STAGES,), np.uint32), ((self.n,), np.uint8) if per_node else None]
        return self._query(fn, np.ascontiguousarray(reqs, dtype=pack.REQ), cand, outputs, after=(int(max_per_node),), last=last)

    def headroom(self, reqs: np.ndarray, cand: Optional[np.ndarray] = None, max_per_node: int = 512, per_node: bool = False):
        """(sums [P] pack.HEADROOM_SUM, entries [P][n] uint16 or None) for ordinary requests (pack.REQ): per node the replicas that
        fit back to back (pack.HEADROOM_COUNT_MASK) and the STOPPED / NOT_EVALUATED bits (nhdfit_headroom).  Nodes outside `cand`
        have 0."""
        return self._headroom(self.lib.nhdfit_headroom, reqs, cand, max_per_node, per_node)

    def headroom_general(self, reqs: np.ndarray, cand: Optional[np.ndarray] = None, max_per_node: int = 512, per_node: bool = False):
        """headroom() with a figure for every candidate held as a wide record - wide nodes, every node of an ENABLE_SHARING mirror -
        instead of NOT_EVALUATED (nhdfit_headroom_general); the nodes of the planes are answered as headroom() answers them."""
        return self._headroom(self.lib.nhdfit_headroom_general, reqs, cand, max_per_node, per_node)

    def headroom_limits(self, reqs: np.ndarray, cand: Optional[np.ndarray] = None, max_per_node: int = 512, per_node: bool = False,
                        _slab_bytes: Optional[int] = None):
        """(sums, entries or None, limits [P][STAGES] uint32, stages [P][n] uint8 or None): headroom() - the same sums and entries -
        and the stage that ended each node's run (nhdfit_headroom_limits): per template the nodes per stage, and per node the stage
        code or pack.LIMIT_NONE where the entry is flagged.  `_slab_bytes`: the device-memory budget of the runs' final states (tests:
        a small one makes the call take several slabs of templates; the library's entry outside include/nhdfit.h takes it)."""
        if _slab_bytes is None:
            return self._headroom(self.lib.nhdfit_headroom_limits, reqs, cand, max_per_node, per_node, limits=True)
        return self._headroom(self.lib.nhdfit_headroom_limits_slab, reqs, cand, max_per_node, per_node, limits=True, last=(int(_slab_bytes),))

    def candidates(self, reqs: np.ndarray, now: float, k: int, cand: Optional[np.ndarray] = None, general: bool = False):
        """(sums [P] pack.CANDIDATES_SUM, entries [P][k] pack.CANDIDATE) for ordinary requests (pack.REQ): per pod the first k nodes
        FindNode would pick, in the order it would get there, each with its mapping (nhdfit_candidates); entries past `returned` are
        all zero.  Candidates held as wide records are counted in `not_evaluated`, not listed - with `general`
        (nhdfit_candidates_general) they are ranked and mapped with the others."""
        k = int(k)
        return self._query(self.lib.nhdfit_candidates_general if general else self.lib.nhdfit_candidates, np.ascontiguousarray(reqs, dtype=pack.REQ), cand,
                           [((), pack.CANDIDATES_SUM), ((k,), pack.CANDIDATE)], before=(float(now),), after=(k,))

    def candidates_big(self, reqs: np.ndarray, now: float, k: int, cand: Optional[np.ndarray] = None):
        """(sums [P] pack.CANDIDATES_SUM, entries [P][k] pack.BIG_CANDIDATE) for big requests (pack.BIG_REQ): candidates() over every
        mirrored node - the planes' nodes and the wide records, on any mirror - ranked and mapped in one call (nhdfit_candidates_big);
        entries[0] is big_find's answer, `not_evaluated` is 0."""
        k = int(k)
        return self._query(self.lib.nhdfit_candidates_big, np.ascontiguousarray(reqs, dtype=pack.BIG_REQ), cand,
                           [((), pack.CANDIDATES_SUM), ((k,), pack.BIG_CANDIDATE)], before=(float(now),), after=(k,))

    def big_commit(self, node: int, req: np.ndarray, mapping: np.ndarray, busy_time: float) -> np.ndarray:
        """The commit step of a big request on node `node` (ordinary or wide): updates the mirror, returns pack.BIG_PLACEMENT."""
        out = np.zeros((), pack.BIG_PLACEMENT)
        req = np.ascontiguousarray(req, dtype=pack.BIG_REQ)
        mapping = np.ascontiguousarray(mapping, dtype=pack.BIG_MAPPING)
        self._chk(self.lib.nhdfit_big_commit(self.ctx, int(node), _p(req), _p(mapping), float(busy_time), _p(out)))
        return out

    def download(self, first: int = 0, count: Optional[int] = None) -> pack.NodeTable:
        count = self.n - first if count is None else count
        t = pack.empty_table(count)
        t.origin = None                                     # not read back: uploading this table leaves the origin records alone
        self._chk(self.lib.nhdfit_download_nodes(self.ctx, first, count, _p(t.p0), _p(t.p1), _p(t.p2), _p(t.p3), _p(t.p4), _p(t.detail)))
        if self.n_wide:
            recs = self.wide_download()
            t.wide = {int(w["index"]) - first: w.copy() for w in recs if first <= int(w["index"]) < first + count}
            if getattr(self, "_share", None) is not None:           # ENABLE_SHARING: the NICs' speed_used as the device's commits left them,
                share = self.wide_share_download()                  # in the order of the wide records - so that upload(download()) restores them
                if len(share) != len(recs):
                    raise _lib.NhdFitError(-5, "ENABLE_SHARING: %d speed_used records for %d wide records" % (len(share), len(recs)))
                t.share = {int(w["index"]) - first: share[k].copy() for k, w in enumerate(recs) if first <= int(w["index"]) < first + count}
        return t

    # ---- pipelined --------------------------------------------------------------------
    def stage(self, reqs: np.ndarray):
        reqs = np.ascontiguousarray(reqs)
        self._chk(self.lib.nhdfit_stage_requests(self.ctx, _p(reqs), len(reqs)))
        self.P = len(reqs)

    def enqueue(self, now: float):
        self._chk(self.lib.nhdfit_enqueue_step(self.ctx, float(now)))

    def sync(self):
        self._chk(self.lib.nhdfit_sync(self.ctx))

    def fetch(self, want_bitmap=False, want_map=True):
        score = np.zeros(self.P, np.uint64)
        bitmap = np.zeros(((self.n + 63) // 64, self.P), np.uint64) if want_bitmap else None
        maps = np.zeros(self.P, pack.MAPPING) if want_map else None
        self._chk(self.lib.nhdfit_fetch(self.ctx, _p(score), _p(bitmap), _p(maps)))
        return score, bitmap, maps

    def stats(self) -> _lib.Stats:
        s = _lib.Stats()
        self._chk(self.lib.nhdfit_get_stats(self.ctx, ctypes.byref(s)))
        return s

    def reset_stats(self):
        self._chk(self.lib.nhdfit_reset_stats(self.ctx))

    # ---- collective -------------------------------------------------------------------
    def unique_id(self) -> bytes:
        buf = ctypes.create_string_buffer(128)
        rc = self.lib.nhdfit_comm_unique_id(buf)
        if rc != 0:
            raise _lib.NhdFitError(rc, (self.lib.nhdfit_last_error(None) or b"?").decode())
        return buf.raw

    def comm_init(self, nranks: int, rank: int, uid: bytes):
        self._chk(self.lib.nhdfit_comm_init(self.ctx, nranks, rank, ctypes.c_char_p(uid)))

    def comm_destroy(self):
        self._chk(self.lib.nhdfit_comm_destroy(self.ctx))

    def comm_rank(self):
        """(rank, ranks) of the context's communicator; (0, 1) without one."""
        r, n = ctypes.c_int(0), ctypes.c_int(1)
        self._chk(self.lib.nhdfit_comm_rank(self.ctx, ctypes.byref(r), ctypes.byref(n)))
        return r.value, n.value

    def comm_sendrecv(self, send: np.ndarray, dst: int, recv: np.ndarray, src: int) -> None:
        """One grouped ncclSend / ncclRecv over the context's communicator (nhdfit_comm_sendrecv): `send` goes to rank `dst`,
        `recv` is filled from rank `src`; either may be None (with its peer -1)."""
        if send is not None:
            send = np.ascontiguousarray(send)
        if recv is not None and not recv.flags["C_CONTIGUOUS"]:
            raise ValueError("recv buffer must be contiguous")
        self._chk(self.lib.nhdfit_comm_sendrecv(self.ctx, send.ctypes.data if send is not None else None, send.nbytes if send is not None else 0, int(dst),
                                                recv.ctypes.data if recv is not None else None, recv.nbytes if recv is not None else 0, int(src)))

    def comm_allreduce_sum_u8(self, buf: np.ndarray) -> None:
        """In-place element-wise sum of a contiguous uint8 array over the ranks (nhdfit_comm_allreduce_sum_u8)."""
        if buf.dtype != np.uint8 or not buf.flags["C_CONTIGUOUS"]:
            raise ValueError("a contiguous uint8 array")
        self._chk(self.lib.nhdfit_comm_allreduce_sum_u8(self.ctx, buf.ctypes.data, buf.nbytes))


class _ShardView(Engine):
    """An Engine whose context belongs to a group (the group destroys it)."""

    def __init__(self, lib, ctx, device):  # noqa: D401 - no nhdfit_create here
        self.lib = lib
        self.ctx = ctypes.c_void_p(ctx)
        self.device = device
        self.n = 0
        self.capacity = 0
        self.P = 0
        self.global_base = 0
        self._dict_version = -1
        self._dict_of = None
        self.n_wide = 0

    def close(self):
        self.ctx = None


class GroupEngine:
    """One process, several GPUs: the node axis of the mirror cut into contiguous shards (multiples of 64 nodes), one
    context per device, winners picked by ONE all-reduce(max) of the packed scores over xGMI inside libnhdfit
    (nhdfit_group_find).  Presents the Engine interface HipMatcher uses, so `HipMatcher(devices=[0, 1, ...])` lets the
    reference's unmodified one-thread scheduler (nhd/NHDScheduler.py:43,50,277) drive all GPUs of the node.
    `engine_factory` (tests only): build the shards from host-twin engines and reduce on the host instead."""

    def __init__(self, devices, engine_factory=None):
        self.devices = list(devices)
        if not self.devices:
            raise ValueError("GroupEngine needs at least one device")
        self.n = 0
        self.P = 0
        self.global_base = 0
        self.group = None
        self._bounds = []
        self.last_wide_places = {}
        if engine_factory is not None:
            self.lib = None
            self.shards = [engine_factory(d) for d in self.devices]
        else:
            self.lib = _lib.load()
            g = ctypes.c_void_p()
            devs = (ctypes.c_int * len(self.devices))(*self.devices)
            rc = self.lib.nhdfit_group_create(devs, len(self.devices), ctypes.byref(g))
            if rc != 0:
                raise _lib.NhdFitError(rc, (self.lib.nhdfit_last_error(None) or b"?").decode())
            self.group = g
            self.shards = [_ShardView(self.lib, self.lib.nhdfit_group_ctx(g, k), d) for k, d in enumerate(self.devices)]

    def close(self):
        if self.group is not None:
            self.lib.nhdfit_group_destroy(self.group)
            self.group = None
        for s in self.shards:
            s.close()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass

    # ---- state ------------------------------------------------------------------------
    def set_dictionary(self, packer: pack.Packer):
        for s in self.shards:
            s.set_dictionary(packer)

    def forget_dictionary(self):
        for s in self.shards:
            s.forget_dictionary()

    def reset_nodes(self):
        for s in self.shards:
            s.reset_nodes()
        self.n = 0
        self._bounds = []

    def _shard_of(self, i: int) -> int:
        for k, (lo, hi) in enumerate(self._bounds):
            if lo <= i < hi:
                return k
        raise IndexError(i)

    def upload(self, table: pack.NodeTable, global_base: int = 0, first: int = 0, capacity: Optional[int] = None):
        """Full upload (first == 0: defines the shard bounds) or delta upload of a run of nodes at `first` (Engine.upload: the
        speed_used records under ENABLE_SHARING)."""
        from .sharding import shard_bounds
        if first == 0 and (not self._bounds or table.n >= self.n):
            if table.n and not table.share and any(getattr(s, "sharing", False) for s in self.shards):
                # (the shards are emptied below: Engine.upload would not see that this table drops the speed_used records)
                raise _lib.NhdFitError(-5, "ENABLE_SHARING: the uploaded table carries no speed_used records (reset_nodes first to stop sharing)")
            n = table.n
            self._bounds = [shard_bounds(n, len(self.shards), r) for r in range(len(self.shards))]
            for s, (lo, hi) in zip(self.shards, self._bounds):
                s.reset_nodes()
                if hi > lo:
                    s.upload(table.slice(lo, hi), global_base=lo)
                else:
                    s.global_base = lo
            self.n = n
            self._has_gpu = self._gpu_flags(table)
            return
        self._has_gpu[first:first + table.n] = self._gpu_flags(table)
        lo_i = first
        while lo_i < first + table.n:                               # a run may straddle shards
            k = self._shard_of(lo_i)
            lo, hi = self._bounds[k]
            hi_i = min(first + table.n, hi)
            self.shards[k].upload(table.slice(lo_i - first, hi_i - first), global_base=lo, first=lo_i - lo, capacity=hi - lo)
            lo_i = hi_i

    @staticmethod
    def _gpu_flags(table: pack.NodeTable) -> np.ndarray:
        """len(Node.gpus) > 0 per node of `table` (Matcher.SelectNode's preference, nhd/Matcher.py:401-413): the planes' flag - and,
        for a wide node, its record's GPU count (its entry in the planes is a placeholder without flags)."""
        has = np.array((table.p2["flags"] & pack.NF_HAS_GPU) != 0)
        for i, rec in (table.wide or {}).items():
            has[i] = int(rec["n_gpus"]) > 0
        return has

    def set_outputs(self, bitmap=True, mapping=True):
        for s in self.shards:
            s.set_outputs(bitmap, mapping)

    def _nogpu_words(self, k: int) -> np.ndarray:
        """Shard k's nodes without a GPU installed, one bit per node (static per node: the hardware)."""
        lo, hi = self._bounds[k]
        bits = np.zeros(((hi - lo + 63) // 64) * 64, np.uint8)
        bits[:hi - lo] = ~self._has_gpu[lo:hi]
        return np.packbits(bits, bitorder="little").view(np.uint64).copy()

    # ---- one-shot ---------------------------------------------------------------------
    def find(self, reqs: np.ndarray, now: float, cand: Optional[np.ndarray] = None, want_bitmap=False, want_map=True):
        reqs = np.ascontiguousarray(reqs)
        P = len(reqs)
        cands = None
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
            cands = [np.ascontiguousarray(cand[lo // 64:(hi + 63) // 64]) if hi > lo else None for lo, hi in self._bounds]
        self.P = P
        if self.group is None:                                      # host twin shards: reduce here
            score = np.zeros(P, np.uint64)
            maps = np.zeros(P, pack.MAPPING)
            parts = []
            for k, s in enumerate(self.shards):
                if self._bounds[k][1] > self._bounds[k][0]:
                    parts.append((k, s.find(reqs, now, cand=None if cands is None else cands[k], want_bitmap=False, want_map=want_map)))
            for k, (sc, _, mp) in parts:
                score = np.maximum(score, sc)
            for k, (sc, _, mp) in parts:
                lo, hi = self._bounds[k]
                idx = np.where(score == 0, -1, (SCORE_MASK - (score & np.uint64(SCORE_MASK))).astype(np.int64))
                own = (sc == score) & (idx >= lo) & (idx < hi)
                if want_map:
                    maps[own] = mp[own]
            return score, None, (maps if want_map else None)
        score = np.zeros(P, np.uint64)
        maps = np.zeros(P, pack.MAPPING) if want_map else None
        owner = np.zeros(P, np.int32)
        cptr = None
        if cands is not None:                                       # (`cands` keeps the per-shard arrays alive across the call)
            cptr = (ctypes.c_void_p * len(self.shards))(*[None if c is None else c.ctypes.data for c in cands])
        rc = self.lib.nhdfit_group_find(self.group, _p(reqs), P, float(now), cptr, _p(score), _p(maps), _p(owner))
        if rc != 0:
            raise _lib.NhdFitError(rc, (self.lib.nhdfit_group_last_error(self.group) or b"?").decode())
        return score, None, maps

    def schedule_batch(self, reqs: np.ndarray, now: float, packer: pack.Packer, cand: Optional[np.ndarray] = None, apply: bool = True):
        """Mode B over all shards, exactly the one-by-one loop's decisions (nhd/NHDScheduler.py:425-437 with
        Matcher.SelectNode's order, nhd/Matcher.py:401-413): a pod takes the first feasible node of the cluster, a pod
        without GPUs the first feasible GPU-less node if there is one.  Two facts make that separable by shard:
          * nodes without GPUs only ever receive pods without GPUs, so their state evolves under that subsequence alone:
            the GPU-less pods walk the shards' GPU-less nodes in shard order, each shard's sequential pass
            (nhdfit_schedule_batch, candidates = its GPU-less nodes) handing the pods it could not place to the next;
          * whatever is left of them and the pods with GPUs then walk the shards in the same manner over all nodes:
            a pod reaches shard s iff no node of shards < s could take it at its turn, and shard s's state depends
            only on the pods placed there before.  (A GPU-less node that refused a pod only lost resources since.)
        Each pass runs on ONE device; a pod costs a pass only on the shards it is offered to.  apply=False restores the
        shards from copies taken up front."""
        reqs = np.ascontiguousarray(reqs)
        P = len(reqs)
        node = np.full(P, -1, np.int64)
        maps = np.zeros(P, pack.MAPPING)
        places = np.zeros(P, pack.PLACEMENT)
        status = np.zeros(P, np.int32)
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
        live = [k for k, (lo, hi) in enumerate(self._bounds) if hi > lo]
        saved = {} if apply else {k: self.shards[k].download(0, self._bounds[k][1] - self._bounds[k][0]) for k in live}
        nogpu = {k: self._nogpu_words(k) for k in live}
        wants_gpu = reqs["gpus"].sum(axis=1) > 0
        touched = {}
        self.last_wide_places = {}

        def offer(pods: np.ndarray, gpu_less_nodes_only: bool) -> np.ndarray:
            for k in live:
                if len(pods) == 0:
                    break
                lo, hi = self._bounds[k]
                mask = None if cand is None else np.ascontiguousarray(cand[lo // 64:(hi + 63) // 64])
                if gpu_less_nodes_only:
                    mask = nogpu[k] if mask is None else mask & nogpu[k]
                    if not mask.any():
                        continue
                nd, mp, pl, st = self.shards[k].schedule_batch(reqs[pods], now, packer, cand=mask, apply=True)
                for j, wp in getattr(self.shards[k], "last_wide_places", {}).items():   # pods that landed on a wide node of this shard
                    wp = wp.copy()
                    wp["node"] = int(wp["node"]) + lo                                    # (global node index, as `node` below)
                    self.last_wide_places[int(pods[j])] = wp
                got = nd >= 0
                node[pods[got]] = nd[got]
                maps[pods[got]] = mp[got]
                places[pods[got]] = pl[got]
                status[pods[got]] = st[got]
                if got.any():
                    a, b = int(nd[got].min()) - lo, int(nd[got].max()) - lo + 1
                    touched[k] = (min(a, touched[k][0]), max(b, touched[k][1])) if k in touched else (a, b)
                pods = pods[~got]
            return pods

        left = offer(np.flatnonzero(~wants_gpu), True)
        rest = np.sort(np.concatenate([np.flatnonzero(wants_gpu), left]))
        offer(rest, False)
        if not apply:
            for k, (a, b) in touched.items():
                lo, hi = self._bounds[k]
                self.shards[k].upload(saved[k].slice(a, b), global_base=lo, first=a, capacity=hi - lo)
        self.P = P
        return node, maps, places, status

    def find_sequential(self, reqs: np.ndarray, now: float, cand: Optional[np.ndarray] = None, packer: Optional[pack.Packer] = None):
        if packer is None:
            raise ValueError("GroupEngine.find_sequential needs the packer (NIC states are interned on the way)")
        node, maps, _, status = self.schedule_batch(reqs, now, packer, cand=cand, apply=False)
        return node, maps, status

    def commit(self, node: int, req, mapping, busy_time):
        k = self._shard_of(node)
        return self.shards[k].commit(node - self._bounds[k][0], req, mapping, busy_time)

    def wide_commit(self, node: int, req, mapping, busy_time):
        k = self._shard_of(node)
        return self.shards[k].wide_commit(node - self._bounds[k][0], req, mapping, busy_time)

    def find_commit(self, req: np.ndarray, now: float, busy_time: float, cand: Optional[np.ndarray] = None, prev: Optional[Tuple[int, float]] = None):
        """Engine.find_commit over the shards (node indices global): the group's find, then the commit on the context that owns the
        winner - composed by nature, the winner is known only behind the all-reduce.  `prev` travels as a SET_BUSY delta to its owner."""
        req = np.ascontiguousarray(req).reshape(-1)[:1]
        if prev is not None:
            d = np.zeros(1, pack.DELTA)
            d["node"], d["op"], d["busy_time"] = int(prev[0]), pack.DELTA_SET_BUSY, float(prev[1])
            self.apply_deltas(d)
        score, _, maps = self.find(req, now, cand=cand, want_bitmap=False, want_map=True)
        s = int(score[0])
        if not s or not int(maps[0]["valid"]):
            return s, maps[0], np.zeros((), pack.PLACEMENT), False
        return s, maps[0], self.commit(winner_index(s), req[0], maps[0], busy_time), True

    def big_find(self, reqs: np.ndarray, now: float, cand: Optional[np.ndarray] = None, want_map=True):
        """Big requests over every shard: each device runs the general pass on its nodes (nhdfit_big_find), the score words -
        which carry the global node index - are max-merged and the owner's mapping kept.  (A rare path: the merge of
        len(shards) x P words is done here, not by a collective.)"""
        reqs = np.ascontiguousarray(reqs, dtype=pack.BIG_REQ)
        P = len(reqs)
        score = np.zeros(P, np.uint64)
        maps = np.zeros(P, pack.BIG_MAPPING)
        parts = []
        for k, s in enumerate(self.shards):
            lo, hi = self._bounds[k]
            if hi > lo:
                mask = None if cand is None else np.ascontiguousarray(np.ascontiguousarray(cand, dtype=np.uint64)[lo // 64:(hi + 63) // 64])
                parts.append((k, s.big_find(reqs, now, cand=mask, want_map=want_map)))
        for k, (sc, mp) in parts:
            score = np.maximum(score, sc)
        idx = np.where(score == 0, -1, (SCORE_MASK - (score & np.uint64(SCORE_MASK))).astype(np.int64))
        for k, (sc, mp) in parts:
            lo, hi = self._bounds[k]
            own = (sc == score) & (idx >= lo) & (idx < hi)
            if want_map:
                maps[own] = mp[own]
        return score, (maps if want_map else None)

    # ---- the query entries over every shard ------------------------------------------------------------------------------------------
    def _query(self, reqs: np.ndarray, cand: Optional[np.ndarray], per_node: bool, outputs, group_entry: Optional[str], shard_call,
               before=(), after=()):
        """One query over every shard.  `outputs` states the entry's results in their order: (shape behind [P], dtype, merge) for one
        the shards' parts are merged into - merge(total, part) - and (None, dtype) for a per-node one, [P][n] in global node order
        (None without `per_node`).  With a group - and a `group_entry` for these requests - libnhdfit's group entry is called:
        entry(group, reqs, P, *before, masks, *after, *outputs), one pointer per shard for the masks and the per-node outputs;
        otherwise shard_call(shard, mask) answers for every shard that has nodes."""
        P = len(reqs)
        out = [np.zeros((P,) + o[0], o[1]) if o[0] is not None else np.zeros((P, self.n), o[1]) if per_node else None for o in outputs]
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
        masks = [None if cand is None else np.ascontiguousarray(cand[lo // 64:(hi + 63) // 64]) for lo, hi in self._bounds]
        if not P:
            return tuple(out)
        scattered = [j for j, o in enumerate(outputs) if o[0] is None and per_node]
        parts = {j: [None] * len(self.shards) for j in scattered}
        if self.group is not None and group_entry is not None:
            def pointers(arrays):
                return (ctypes.c_void_p * len(arrays))(*[None if x is None else x.ctypes.data for x in arrays])
            for j in scattered:
                parts[j] = [np.zeros((P, hi - lo), outputs[j][1]) if hi > lo else None for lo, hi in self._bounds]
            args = [_p(out[j]) if o[0] is not None else pointers(parts[j]) if per_node else None for j, o in enumerate(outputs)]
            rc = getattr(self.lib, group_entry)(self.group, _p(reqs), P, *before, pointers(masks) if cand is not None else None, *after, *args)
            if rc != 0:
                raise _lib.NhdFitError(rc, (self.lib.nhdfit_group_last_error(self.group) or b"?").decode())
        else:
            for k, s in enumerate(self.shards):
                if self._bounds[k][1] > self._bounds[k][0]:
                    for j, (o, part) in enumerate(zip(outputs, shard_call(s, masks[k]))):
                        if o[0] is not None:
                            o[2](out[j], part)
                        elif per_node:
                            parts[j][k] = part
        for j in scattered:
            for (lo, hi), part in zip(self._bounds, parts[j]):
                if part is not None:
                    out[j][:, lo:hi] = part
        return tuple(out)

    def explain(self, reqs: np.ndarray, now: float, cand: Optional[np.ndarray] = None, per_node: bool = False):
        """Engine.explain over every shard: counts summed over the devices (nhdfit_group_explain for ordinary requests; big ones
        shard by shard), stages put together in global node order."""
        reqs = np.ascontiguousarray(reqs)
        return self._query(reqs, cand, per_node, [((STAGES,), np.uint32, operator.iadd), (None, np.uint8)],
                           None if reqs.dtype == pack.BIG_REQ else "nhdfit_group_explain",
                           lambda s, mask: s.explain(reqs, now, cand=mask, per_node=per_node), before=(float(now),))

    def _headroom(self, method: str, reqs, cand, max_per_node, per_node, limits=False):
        reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
        outputs = [((), pack.HEADROOM_SUM, _add_headroom_sums), (None, np.uint16)]
        if limits:
            outputs += [((STAGES,), np.uint32, operator.iadd), (None, np.uint8)]
        return self._query(reqs, cand, per_node, outputs, "nhdfit_group_" + method,
                           lambda s, mask: getattr(s, method)(reqs, cand=mask, max_per_node=max_per_node, per_node=per_node),
                           after=(int(max_per_node),))

    def headroom(self, reqs: np.ndarray, cand: Optional[np.ndarray] = None, max_per_node: int = 512, per_node: bool = False):
        """Engine.headroom over every shard: the sums merged over the devices (nhdfit_group_headroom), the entries put together in
        global node order."""
        return self._headroom("headroom", reqs, cand, max_per_node, per_node)

    def headroom_general(self, reqs: np.ndarray, cand: Optional[np.ndarray] = None, max_per_node: int = 512, per_node: bool = False):
        """Engine.headroom_general over every shard (nhdfit_group_headroom_general), as headroom()."""
        return self._headroom("headroom_general", reqs, cand, max_per_node, per_node)

    def headroom_limits(self, reqs: np.ndarray, cand: Optional[np.ndarray] = None, max_per_node: int = 512, per_node: bool = False):
        """Engine.headroom_limits over every shard: sums merged and histograms added over the devices (nhdfit_group_headroom_limits),
        entries and stages put together in global node order."""
        return self._headroom("headroom_limits", reqs, cand, max_per_node, per_node, limits=True)

    def candidates(self, reqs: np.ndarray, now: float, k: int, cand: Optional[np.ndarray] = None, general: bool = False):
        """Engine.candidates over every shard: the shards' lists merged per pod by descending score, the sums added
        (nhdfit_group_candidates / _general; shards of host twins: sharding.merge_candidates, the same rule).  The scores carry global
        indices."""
        from .sharding import merge_candidates
        reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
        k = int(k)
        if self.group is not None:
            return self._query(reqs, cand, False, [((), pack.CANDIDATES_SUM, None), ((k,), pack.CANDIDATE, None), ((k,), np.int32, None)],
                               "nhdfit_group_candidates_general" if general else "nhdfit_group_candidates", None, before=(float(now),), after=(k,))[:2]
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
        more = {"general": True} if general else {}
        parts = [s.candidates(reqs, now, k, cand=None if cand is None else np.ascontiguousarray(cand[lo // 64:(hi + 63) // 64]), **more)
                 for s, (lo, hi) in zip(self.shards, self._bounds) if hi > lo]
        if not parts or not len(reqs):
            return np.zeros(len(reqs), pack.CANDIDATES_SUM), np.zeros((len(reqs), k), pack.CANDIDATE)
        return merge_candidates([p[0] for p in parts], [p[1] for p in parts], k)[:2]

    def candidates_big(self, reqs: np.ndarray, now: float, k: int, cand: Optional[np.ndarray] = None):
        """Engine.candidates_big over every shard, merged as candidates() merges (nhdfit_group_candidates_big; shards of host twins:
        sharding.merge_candidates with the big entry's record)."""
        from .sharding import merge_candidates
        reqs = np.ascontiguousarray(reqs, dtype=pack.BIG_REQ)
        k = int(k)
        if self.group is not None:
            return self._query(reqs, cand, False, [((), pack.CANDIDATES_SUM, None), ((k,), pack.BIG_CANDIDATE, None), ((k,), np.int32, None)],
                               "nhdfit_group_candidates_big", None, before=(float(now),), after=(k,))[:2]
        if cand is not None:
            cand = np.ascontiguousarray(cand, dtype=np.uint64)
        parts = [s.candidates_big(reqs, now, k, cand=None if cand is None else np.ascontiguousarray(cand[lo // 64:(hi + 63) // 64]))
                 for s, (lo, hi) in zip(self.shards, self._bounds) if hi > lo]
        if not parts or not len(reqs):
            return np.zeros(len(reqs), pack.CANDIDATES_SUM), np.zeros((len(reqs), k), pack.BIG_CANDIDATE)
        return merge_candidates([p[0] for p in parts], [p[1] for p in parts], k, entry_dtype=pack.BIG_CANDIDATE)[:2]

    def big_commit(self, node: int, req, mapping, busy_time):
        k = self._shard_of(node)
        out = self.shards[k].big_commit(node - self._bounds[k][0], req, mapping, busy_time)
        out["node"] = node
        return out

    @property
    def n_wide(self) -> int:
        return sum(getattr(s, "n_wide", 0) for s in self.shards)

    def apply_deltas(self, deltas: np.ndarray) -> np.ndarray:
        """Deltas with GLOBAL node indices, routed to the shards that own the nodes (order kept per shard)."""
        deltas = np.ascontiguousarray(deltas, dtype=pack.DELTA).reshape(-1)
        status = np.zeros(len(deltas), np.uint8)
        owner = np.array([self._shard_of(int(v)) for v in deltas["node"]], dtype=np.int64)
        for k in np.unique(owner):
            sel = np.flatnonzero(owner == k)
            part = deltas[sel].copy()
            part["node"] -= self._bounds[int(k)][0]
            status[sel] = self.shards[int(k)].apply_deltas(part)
        return status

    def download(self, first: int = 0, count: Optional[int] = None) -> pack.NodeTable:
        count = self.n - first if count is None else count
        out = pack.empty_table(count)
        out.origin = None
        i = first
        while i < first + count:
            k = self._shard_of(i)
            lo, hi = self._bounds[k]
            j = min(first + count, hi)
            part = self.shards[k].download(i - lo, j - i)
            for f in ("p0", "p1", "p2", "p3", "p4", "detail"):
                getattr(out, f)[i - first:j - first] = getattr(part, f)
            for q, w in (part.wide or {}).items():
                out.wide[q + i - first] = w
            if part.share:                                          # ENABLE_SHARING: the shards' speed_used records, as the wide ones
                out.share = out.share or {}
                for q, r in part.share.items():
                    out.share[q + i - first] = r
            i = j
        return out

    def stats(self):
        return self.shards[0].stats()


def _add_headroom_sums(sums: np.ndarray, part: np.ndarray) -> None:
    """A shard's pack.HEADROOM_SUM records into the group's (what nhdfit_group_headroom does with them)."""
    for f in ("replicas", "nodes_with_room", "saturated", "stopped", "not_evaluated"):
        sums[f] += part[f]
    sums["max_on_one_node"] = np.maximum(sums["max_on_one_node"], part["max_on_one_node"])
    # (the planes' instantiation: the larger; the wide launch's bit: whether any shard ran it)
    sums["form"] = np.maximum(sums["form"] & 3, part["form"] & 3) | ((sums["form"] | part["form"]) & pack.HEADROOM_FORM_WIDE)


def winner_index(score: int) -> int:
    return SCORE_MASK - (int(score) & SCORE_MASK)
