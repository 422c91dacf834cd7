"""HipMatcher - drop-in for ``nhd.Matcher.Matcher`` (nhd/Matcher.py:21-63).

    self.matcher = Matcher()                                   nhd/NHDScheduler.py:50
    match = self.matcher.FindNode(filt_nodes, top)             nhd/NHDScheduler.py:277
    match[0] -> node name or None,  match[1] -> {'gpu': (..), 'cpu': (..), 'nic': [(numa, idx), ..]}

Same contract: ``FindNode(nl, top)`` returns ``(name, mapping)`` or the 1-tuple ``(None,)``, never
mutates ``nl``/``top``, breaks ties by ``nl`` iteration order, is called from one thread.  The per-node
Python loops are replaced by one pass of the gfx950 kernels over a packed mirror of the cluster
(DESIGN.md).  If libnhdfit.so or the GPU is missing, construction raises - there is no CPU path.

Two ways to keep the device mirror current:

* stateless (default): every call packs ``nl`` again.  Always right, O(N) Python per call.
* ``attach(nodes)``: ``nodes`` is the scheduler's long-lived ``self.nodes`` dict.  Nodes are packed
  once; afterwards only nodes touched through the reference's own mutators (nhd/Node.py:144, 530,
  587, 644, 663, 843, 308) or whose ``active`` / ``maintenance`` / ``groups`` / ``busy_time`` were
  assigned are re-packed (dirty tracking by swapping in a thin subclass).  ``FindNode(nl, top)`` then
  accepts any subset ``nl`` of ``nodes`` in the same relative order (what InitialNodeFilter
  produces, nhd/NHDScheduler.py:235-247) and turns it into a candidate bitmask.

``FindNodes(nl, tops, pod_groups)`` is the batch form (every pod against one snapshot).  ``ScheduleOne(nl, top)`` is FindNode
and the commit step on the winner in one device call (attached mode: the scheduler's own mutators then find the mirror current).
"""
from __future__ import annotations

import logging
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import pack
from ._lib import NhdFitError
from .engine import Engine, GroupEngine, winner_index

_MUTATORS = ("SetPhysicalIdsFromMapping", "RemoveResourcesFromTopology", "AddResourcesFromTopology",
             "ResetResources", "ClaimPodNICResources", "SetBusy", "SetGroups", "SetHugepages", "ParseLabels")
_WATCHED = frozenset(("active", "maintenance", "groups", "busy_time"))
_tracked_cache: Dict[type, type] = {}


def _tracked_class(base: type) -> type:
    """Subclass of the node's own class that reports state changes to the matcher owning it."""
    cls = _tracked_cache.get(base)
    if cls is not None:
        return cls

    def __setattr__(self, key, value):
        base.__setattr__(self, key, value)
        if key in _WATCHED:
            hook = self.__dict__.get("_nhdfit_dirty")
            if hook is not None:
                hook(self, key)

    ns = {"__setattr__": __setattr__}
    for name in _MUTATORS:
        orig = getattr(base, name, None)
        if orig is None:
            continue

        def make(orig, name):
            def wrapper(self, *a, **kw):
                ok = False
                out = None
                try:
                    out = orig(self, *a, **kw)
                    ok = True
                    return out
                finally:
                    hook = self.__dict__.get("_nhdfit_dirty")
                    if hook is not None:
                        # the commit step of AttemptScheduling (nhd/NHDScheduler.py:289-304) is mirrored on the device
                        # instead of re-packing the node: see HipMatcher._on_commit / _on_claim
                        # and so are the release / reclaim / reset paths and SetHugepages (row f2: nhdfit_apply_deltas)
                        done = False
                        owner = self.__dict__["_nhdfit_owner"]
                        if ok and name == "SetPhysicalIdsFromMapping":
                            done = owner._on_commit(self, *a, **kw)
                        elif ok and name == "ClaimPodNICResources":
                            done = owner._on_claim(self, *a, **kw)
                        elif ok and name in ("RemoveResourcesFromTopology", "AddResourcesFromTopology") and out is not False:
                            done = owner._on_topology(self, name, *a, **kw)    # (False: the reference gave up half-way, Node.py:543-545 - re-pack)
                        elif ok and name == "ResetResources":
                            done = owner._on_queued_scalar(self, "reset")
                        elif ok and name == "SetHugepages":
                            done = owner._on_queued_scalar(self, "hugepages")
                        elif ok and name == "SetGroups":
                            done = True                              # the assignment to .groups inside it was seen by __setattr__
                        if not done:
                            hook(self, name)
            wrapper.__name__ = orig.__name__
            return wrapper
        ns[name] = make(orig, name)
    cls = type("Tracked" + base.__name__, (base,), ns)
    _tracked_cache[base] = cls
    return cls


# What list(set(itertools.product(range(2), repeat=k))) gives under the CPython set / tuple-hash behaviour the device-side
# model (nhd_amd/csrc/winner_map.h) reproduces (CPython 3.8 - 3.12, 64-bit).  FindNode's mapping is "bit-identical to the
# reference" relative to the interpreter that would run the reference - i.e. this one: if it orders sets differently
# (another Python implementation, a future change of tuple hashing) the model no longer speaks for it and HipMatcher
# refuses to start instead of returning mappings the reference would not.
_SET_ORDER_PROBES = {
    1: [(0,), (1,)],
    2: [(0, 1), (1, 0), (1, 1), (0, 0)],
    3: [(1, 0, 1), (1, 1, 0), (0, 1, 0), (0, 0, 0), (1, 0, 0), (0, 0, 1), (1, 1, 1), (0, 1, 1)],
    4: [(0, 0, 0, 1), (0, 0, 1, 0), (0, 1, 0, 1), (0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 0), (0, 1, 0, 0), (1, 1, 1, 0),
        (0, 1, 1, 0), (0, 0, 0, 0), (1, 0, 1, 0), (1, 0, 0, 1), (1, 1, 0, 1), (1, 0, 0, 0), (0, 0, 1, 1), (1, 1, 1, 1)],
}
_SET_INTERSECTION_PROBE = [(1, 0, 1), (1, 1, 1), (0, 0, 0), (0, 1, 1)]


# ---- explain: the stage at which each node turned a pod away (include/nhdfit.h NHDFIT_STAGE_*, in the reference's order) ----
STAGES = ("NOT_CANDIDATE", "MAINTENANCE", "HUGEPAGES", "BUSY", "GPU", "CPU", "NIC", "PCI", "NUMA", "FITS")
UNMIRRORED = 255                 # per-node stage of a node listed in HipMatcher.unmirrored (never evaluated on the device)
_STAGE_TEXT = {"NOT_CANDIDATE": "not candidates (node group / inactive)", "MAINTENANCE": "in maintenance",
               "HUGEPAGES": "short of hugepages", "BUSY": "busy (deployed to within the last few seconds)", "GPU": "short of GPUs",
               "CPU": "short of CPU cores", "NIC": "short of NIC bandwidth", "PCI": "short of GPUs on the NICs' PCIe switches",
               "NUMA": "without a NUMA-aligned placement"}


class Explanation:
    """Why the nodes of one FindNode call turned one pod away: `counts` (stage name -> nodes, every node charged with the first
    stage that drops it; "FITS" = the nodes FindNode chooses among), `unmirrored` (nodes of `nl` the device does not hold -
    they never match and are not blamed on a stage) and, when asked for, `stages` (uint8 per node in `nl` order: the stage
    code, or UNMIRRORED).  `error`: why the pod itself could not be evaluated (a request no record can express, a NIC search
    beyond its budget) - then no node is charged with anything: every count is 0 and `stages` is None."""

    def __init__(self, counts: Dict[str, int], unmirrored: int, stages: Optional[np.ndarray] = None, error: Optional[str] = None,
                 nodes: Optional[int] = None):
        self.counts = counts
        self.unmirrored = unmirrored
        self.stages = stages
        self.error = error
        self.nodes = sum(counts.values()) + unmirrored if nodes is None else nodes

    @property
    def total(self) -> int:
        """Nodes of `nl`."""
        return self.nodes

    def summary(self) -> str:
        """The Kubernetes-style sentence: "0/65536 nodes are available: 12 in maintenance, 4100 short of hugepages, ..."."""
        if self.error is not None:
            return f"the pod was not evaluated against the {self.total} nodes: {self.error}."
        parts = [f"{self.counts[s]} {_STAGE_TEXT[s]}" for s in STAGES[:-1] if self.counts.get(s)]
        if self.unmirrored:
            parts.append(f"{self.unmirrored} not mirrored on the device")
        head = f"{self.counts.get('FITS', 0)}/{self.total} nodes are available"
        return head + (": " + ", ".join(parts) + "." if parts else ".")

    def __repr__(self) -> str:
        return f"Explanation({self.summary()!r})"


def _spaced(v: int) -> str:
    return f"{int(v):,}".replace(",", " ")


class Headroom:
    """How many more replicas of one pod template the nodes of `nl` can take (HipMatcher.Headroom): `replicas` (the sum - what the
    scheduler's first-fit loop would place once busy windows have passed), `nodes_with_room`, `max_on_one_node`, `saturated` (nodes
    that reached `max_per_node`), `stopped` (nodes whose run ended at a commit the reference raises on: their count is what
    succeeded before it), `not_evaluated` (wide nodes, ENABLE_SHARING mirrors: no figure), `unmirrored` (nodes of `nl` the device
    does not hold: they never match) and, when asked for, `per_node` (uint16 counts in `nl` order) with `flags` (the STOPPED /
    NOT_EVALUATED bits of include/nhdfit.h beside them).  `form`: which kernel instantiation answered (pack.HEADROOM_FORM_*).
    `error`: why the template itself could not be evaluated - then nothing is a number: every node counts as not evaluated.
    Asked for with limits=True: `limits` (stage name -> nodes of `nl` whose run ended at that stage - the resource that ran out
    first; "FITS" occurs only on nodes that reached `max_per_node` with room left - a node may also run out of a resource with the
    very replica that reaches the bound; stopped, not evaluated and unmirrored nodes are charged to no stage) and, with
    per_node=True, `limit_stages` (uint8 per node in `nl` order: the stage code, or 255 = pack.LIMIT_NONE = UNMIRRORED for a
    node without one - `flags` tells a stopped or not evaluated node, whose flag is set, from an unmirrored one).  Both are None
    otherwise."""

    def __init__(self, nodes: int, names: Optional[List[str]] = None, replicas: int = 0, nodes_with_room: int = 0, max_on_one_node: int = 0,
                 saturated: int = 0, stopped: int = 0, not_evaluated: int = 0, unmirrored: int = 0, form: int = 0, max_per_node: int = 0,
                 per_node: Optional[np.ndarray] = None, flags: Optional[np.ndarray] = None, error: Optional[str] = None,
                 limits: Optional[Dict[str, int]] = None, limit_stages: Optional[np.ndarray] = None):
        self.limits, self.limit_stages = limits, limit_stages
        self.nodes, self._names = nodes, names
        self.replicas, self.nodes_with_room, self.max_on_one_node = int(replicas), int(nodes_with_room), int(max_on_one_node)
        self.saturated, self.stopped, self.not_evaluated, self.unmirrored = int(saturated), int(stopped), int(not_evaluated), int(unmirrored)
        self.form, self.max_per_node = int(form), int(max_per_node)
        self.per_node, self.flags, self.error = per_node, flags, error

    def by_node(self) -> Dict[str, int]:
        """name -> replicas (per_node=True calls only)."""
        if self.per_node is None:
            raise ValueError("by_node() needs the per-node counts: ask for per_node=True" if self.error is None else f"not evaluated: {self.error}")
        return {nm: int(k) for nm, k in zip(self._names, self.per_node)}

    def summary(self) -> str:
        """"1 234 more replicas on 410 of 65 536 nodes (most on one node: 7)", and what qualifies it."""
        if self.error is not None:
            return f"the pod was not evaluated against the {_spaced(self.nodes)} nodes: {self.error}."
        text = f"{_spaced(self.replicas)} more replicas on {_spaced(self.nodes_with_room)} of {_spaced(self.nodes)} nodes (most on one node: {_spaced(self.max_on_one_node)})"
        notes = []
        if self.saturated:
            notes.append(f"{_spaced(self.saturated)} reached the limit of {_spaced(self.max_per_node)} per node")
        if self.stopped:
            notes.append(f"{_spaced(self.stopped)} stopped at a placement the scheduler would fail on")
        if self.not_evaluated:
            notes.append(f"{_spaced(self.not_evaluated)} not evaluated")
        if self.unmirrored:
            notes.append(f"{_spaced(self.unmirrored)} not mirrored on the device")
        return text + ("; " + ", ".join(notes) if notes else "")

    def limit_summary(self) -> str:
        """"further replicas are held back by: short of CPU cores on 40 210 nodes, short of NIC bandwidth on 12 001, ..." (limits=True
        calls only), the stages ordered by the nodes they hold."""
        if self.limits is None:
            raise ValueError("limit_summary() needs the limits: ask for limits=True")
        if self.error is not None:
            return f"the pod was not evaluated against the {_spaced(self.nodes)} nodes: {self.error}."
        held = sorted(((k, s) for s, k in self.limits.items() if k and s != "FITS"), key=lambda x: -x[0])
        parts = [f"{_STAGE_TEXT[s]} on {_spaced(k)}" + (" nodes" if i == 0 else "") for i, (k, s) in enumerate(held)]
        text = "further replicas are held back by: " + ", ".join(parts) if parts else "nothing holds further replicas back"
        if self.limits.get("FITS"):
            text += f"; {_spaced(self.limits['FITS'])} nodes reached the limit of {_spaced(self.max_per_node)} per node with room left"
        return text

    def __repr__(self) -> str:
        return f"Headroom({self.summary()!r})"


class Candidates:
    """Where one pod could go, in the order the scheduler would get there (HipMatcher.Candidates): `entries` - `(name, mapping)`
    tuples exactly as FindNode returns them; entries[0] is FindNode's answer, entries[j] what FindNode answers once the j nodes in
    front of it are out of `nl`; empty where FindNode answers (None,) - `feasible` (every node of `nl` that FindNode chooses among:
    the FITS count of ExplainNode), `preferred` (those of them without GPUs, for a pod without GPUs: the scheduler takes them first;
    0 otherwise) and `k`, the length asked for.  `error`: why the pod itself could not be evaluated - then the list is empty and
    says nothing about the cluster."""

    def __init__(self, entries: List[Tuple], feasible: int = 0, preferred: int = 0, k: int = 0, nodes: int = 0, form: int = 0,
                 error: Optional[str] = None):
        self.entries = entries
        self.feasible, self.preferred, self.k, self.nodes, self.form = int(feasible), int(preferred), int(k), int(nodes), int(form)
        self.error = error

    def summary(self) -> str:
        """"first 8 of 412 feasible nodes (of 65 536; 17 without GPUs come first): node-3, node-9, ..."."""
        if self.error is not None:
            return f"the pod was not evaluated against the {_spaced(self.nodes)} nodes: {self.error}."
        if not self.entries:
            return f"no feasible node among {_spaced(self.nodes)}."
        pref = f"; {_spaced(self.preferred)} without GPUs come first" if self.preferred else ""
        return (f"first {len(self.entries)} of {_spaced(self.feasible)} feasible nodes (of {_spaced(self.nodes)}{pref}): "
                + ", ".join(e[0] for e in self.entries))

    def __repr__(self) -> str:
        return f"Candidates({self.summary()!r})"


def check_interpreter_set_model() -> None:
    import itertools
    for k, want in _SET_ORDER_PROBES.items():
        if list(set(itertools.product(range(2), repeat=k))) != want:
            raise RuntimeError("this Python interpreter iterates sets of int tuples in a different order than the set model of "
                               "libnhdfit (CPython 3.8-3.12): FindNode's NUMA mapping would differ from the reference Matcher's")
    a = set(itertools.product(range(2), repeat=3))
    b = {t for t in a if sum(t) != 1}
    c = {t for t in a if t[0] == 0 or t[2] == 1}
    if list(a & b & c) != _SET_INTERSECTION_PROBE:
        raise RuntimeError("this Python interpreter intersects sets in a different order than the set model of libnhdfit")


class HipMatcher:
    def __init__(self, device: int = 0, clock=time.monotonic, engine_factory=None, devices: Optional[Sequence[int]] = None,
                 strict: bool = False):
        """`devices=[0, 1, ...]`: shard the mirror over several GPUs of this process (engine.GroupEngine: node axis
        cut into contiguous shards, one RCCL all-reduce(max) of the packed scores per call picks the winners) - the
        reference's one-thread scheduler keeps calling FindNode exactly as before.
        `engine_factory(device)` exists for the test-suite only (it injects the host build of the
        kernels' arithmetic so the host logic of this class can be exercised without a GPU); the
        default is the HIP engine, which raises when the library or a gfx950 GPU is missing.
        `strict=False` (default) keeps FindNode's contract - `(name, mapping)` or `(None,)`, never an exception
        (nhd/Matcher.py:47-63) - where the device layout cannot hold something: a node beyond the
        layout's capacities (include/nhdfit.h) never matches and is listed in `self.unmirrored` (name -> reason), a
        request beyond them or a device error makes the call answer `(None,)` (the scheduler leaves the pod pending and
        tries again, nhd/NHDScheduler.py:278-287); each is logged.  `strict=True` raises instead."""
        self.logger = logging.getLogger(__name__)
        self.strict = strict
        self.last_placements: List[Optional[dict]] = []    # physical ids per pod of the last ScheduleBatch (see there)
        self._warned: set = set()
        check_interpreter_set_model()
        if devices is not None:
            self.engine = GroupEngine(devices, engine_factory)
        else:
            self.engine = (engine_factory or Engine)(device)
        self.packer = pack.Packer(strict=strict)
        self.clock = clock
        self._attached: Optional[Dict[str, object]] = None
        self._index: Dict[str, int] = {}
        self._names: List[str] = []
        self._table: Optional[pack.NodeTable] = None
        self._dirty: Dict[str, object] = {}
        self._mirror_foreign = False                       # the mirror holds a dict other than the attached one
        self._reasons: Dict[str, set] = {}
        self._claims: Dict[str, frozenset] = {}
        self._batch_ids: Dict[str, list] = {}              # ScheduleBatch(apply=True): ids the device already committed, per node, in order
        self._deltas: List[np.ndarray] = []                # release / reclaim / reset / SetHugepages waiting for the device, in call order
        # ScheduleOne: (winner, busy time committed on the device, its ids) of the last call - what the scheduler's SetBusy writes
        # behind it is recognised by these (_on_commit), and a later time rides in the next ScheduleOne instead of a delta of its own
        self._one: Optional[Tuple[str, float, dict]] = None
        self.delta_stats = {"applied": 0, "repacked": 0}
        self._uploaded_ids: Optional[Tuple[int, ...]] = None
        # candidate masks of the filtered dicts seen lately, by (length, first, middle, last name) -> [(names, mask)]: pods of a few
        # node groups take turns in the pending list, each group with its own filtered dict (nhd/NHDScheduler.py:235-247)
        self._last_subset: Optional[Dict[tuple, List[Tuple[List[str], np.ndarray]]]] = None
        self._subset_count = self._subset_names = 0
        self._digest_cache: Optional[Tuple[object, np.ndarray]] = None     # (topology, request record) of the last one-pod FindNode

    # ---- mirror maintenance -------------------------------------------------------------
    def attach(self, nodes: Dict[str, object]) -> None:
        """Mirror `nodes` (the scheduler's self.nodes) persistently and track changes to it."""
        self._attached = nodes
        self._mirror_foreign = False
        # a fresh dictionary: NIC signatures, capacity classes and group sets of nodes that left the cluster (or of states
        # nothing is in any more) do not pile up over the life of a scheduler that re-attaches after node churn
        self.packer = pack.Packer(strict=self.strict)
        self.engine.forget_dictionary()
        for node in nodes.values():
            if type(node) not in _tracked_cache.values():
                node.__class__ = _tracked_class(type(node))
            node.__dict__["_nhdfit_dirty"] = self._mark
            node.__dict__["_nhdfit_owner"] = self
        self._full_upload(nodes)
        self.packer.close_signatures()                 # every NIC state a commit can produce gets its signature now
        self.engine.set_dictionary(self.packer)
        self._dirty.clear()
        self._reasons.clear()
        self._deltas = []
        self._claims = {}

    def detach(self) -> None:
        if self._attached:
            for node in self._attached.values():
                node.__dict__.pop("_nhdfit_dirty", None)
                node.__dict__.pop("_nhdfit_owner", None)
        self._attached = None

    # ---- commit step mirrored on the device (row f1) ---------------------------------------
    def _off_planes(self, name: str) -> bool:
        """The node is not (only) held by the five planes: a wide node (its record is re-uploaded whenever it changes - the
        general path has no delta form) or one no layout holds (never matches; nothing to keep current)."""
        i = self._index.get(name)
        return name in self.packer.unmirrored or (i is not None and self._table is not None and bool(self._table.wide) and i in self._table.wide)

    def _mapping_record(self, mapping, big: bool = False) -> np.ndarray:
        G = len(mapping["gpu"])
        m = np.zeros((), pack.BIG_MAPPING if big or G > pack.MAX_GROUPS else pack.MAPPING)
        m["gpu"][:G] = mapping["gpu"]
        m["cpu"][:G + 1] = mapping["cpu"]
        m["nic_numa"][:G] = [x[0] for x in mapping["nic"]]
        m["nic_idx"][:G] = [x[1] for x in mapping["nic"]]
        m["valid"] = 1
        return m

    def CommitPlacement(self, name: str, top, mapping, busy_time: Optional[float] = None) -> dict:
        """The commit step of AttemptScheduling (SetBusy / SetPhysicalIdsFromMapping / ClaimPodNICResources,
        nhd/NHDScheduler.py:289-304) applied to the DEVICE mirror of attached node `name` (nhdfit_commit); returns
        the physical ids the reference would write into `top` (pack.expand_placement).  The Node object itself is
        not touched."""
        i = self._index[name]
        node = self._attached[name] if self._attached is not None else None
        bt = float(node.busy_time if busy_time is None and node is not None else busy_time)
        if pack.needs_general_path(top):                                                # a pod with 5..8 processing groups (or beyond the hugepage table): the general path's commit step
            return self._commit_big(i, node, self.packer.digest_big(top), self._mapping_record(mapping, big=True), bt)
        cached, self._digest_cache = self._digest_cache, None         # the record FindNode made of this very topology a moment ago (the scheduler
        if cached is not None and cached[0] is top:                   # commits what it has just matched, nhd/NHDScheduler.py:277-304) - spent here
            req = cached[1]
            if self.packer.sharing:                                   # its speeds reach speed_used as digest() would have noted them (a full re-pack
                for g in range(int(req["n_groups"])):                 # since the find started share_exact afresh)
                    self.packer._note_share_value(req["rx"][g])
                    self.packer._note_share_value(req["tx"][g])
        else:
            req = self.packer.digest(top)
        if self.packer.sharing and int(req["flags"]) & pack.RF_NIC_SPLIT and not self.packer.share_exact:
            # (the cached record was admitted when every speed in the mirror was still a multiple of 2^-20; one that is not arrived since)
            raise pack.UnsupportedNode("a processing group with several RX / TX cores (ENABLE_SHARING), and the mirror's speeds are no longer all "
                                       "multiples of 2^-20 Gb/s: the commit's sum would not be the reference's core-by-core accumulation")
        if self._table is not None and self._table.wide and i in self._table.wide:      # a wide node: the general path's commit step
            place = self.engine.wide_commit(i, req, self._mapping_record(mapping), bt)
            G = int(req["n_groups"])
            cpp = int(node.cores_per_proc) if node is not None else int(self._table.wide[i]["cores_per_proc"])
            U = int(node.sockets) if node is not None else int(self._table.wide[i]["numa_nodes"])
            return pack.expand_wide_placement(place, G, cpp, cpp * U, [int(req["gpus"][g]) for g in range(G)])
        place = self.engine.commit(i, req, self._mapping_record(mapping), bt)
        if int(place["status"]) == pack.COMMIT_NEW_SIG:        # cannot happen after close_signatures(); handled anyway
            one = self.engine.download(i, 1)
            sn, sp = self.packer.sigs_from_detail(one.detail[0])
            one.p3[0]["sig_numa"], one.p3[0]["sig_pci"] = sn, sp
            self.engine.set_dictionary(self.packer)
            self.engine.upload(one, first=i, capacity=len(self._names))
        cpp = int(node.cores_per_proc) if node is not None else 0
        G = int(req["n_groups"])
        return pack.expand_placement(place, G, cpp, cpp * int(node.sockets) if node is not None else 0,
                                     [int(req["gpus"][g]) for g in range(G)])

    def _commit_big(self, i: int, node, req, mapping_rec, busy_time: float) -> dict:
        """nhdfit_big_commit on node i (ordinary or wide) -> the physical ids (pack.expand_wide_placement: a big placement
        carries two mask words per batch whichever form the node is mirrored in)."""
        place = self.engine.big_commit(i, req, mapping_rec, busy_time)
        wide = self._table is not None and self._table.wide and i in self._table.wide
        if not wide and int(place["status"]) == pack.COMMIT_NEW_SIG:    # cannot happen after close_signatures(); handled anyway
            one = self.engine.download(i, 1)
            sn, sp = self.packer.sigs_from_detail(one.detail[0])
            one.p3[0]["sig_numa"], one.p3[0]["sig_pci"] = sn, sp
            self.engine.set_dictionary(self.packer)
            self.engine.upload(one, first=i, capacity=len(self._names))
        G = int(req["n_groups"])
        if node is not None:
            cpp, U = int(node.cores_per_proc), int(node.sockets)
        elif wide:
            cpp, U = int(self._table.wide[i]["cores_per_proc"]), int(self._table.wide[i]["numa_nodes"])
        else:
            cpp, U = 0, 0
        return pack.expand_wide_placement(place, G, cpp, cpp * U, [int(req["gpus"][g]) for g in range(G)])

    def _on_commit(self, node, mapping, top) -> bool:
        """After the reference's own SetPhysicalIdsFromMapping succeeded on an attached node: the same commit on the
        device mirror, checked against what the reference just wrote into `top`.  True = the mirror is current."""
        if self._attached is None or node.name not in self._index or self._waits_for_repack(node.name) or self._off_planes(node.name):
            self._batch_ids.pop(node.name, None)
            return False
        pending = self._batch_ids.get(node.name)
        if not pending and self._deltas:
            self._flush_deltas()                               # releases queued before this commit reach the device first
            if self._waits_for_repack(node.name):
                return False
        from_batch = bool(pending)
        if pending:                                            # ScheduleBatch(apply=True) committed this placement on the device already
            ids = pending.pop(0)
            if not pending:
                del self._batch_ids[node.name]
        else:
            try:
                ids = self.CommitPlacement(node.name, top, mapping)
            except Exception:  # noqa: BLE001 - any doubt: fall back to re-packing the node
                return False
        pos = {g.device_id: k for k, g in enumerate(node.gpus)}
        want = {"groups": [{"cores": [c.core for g in pg.group_gpus for c in g.cpu_cores] + [c.core for c in pg.proc_cores],
                            "helpers": [c.core for c in pg.misc_cores], "gpus": [pos[g.device_id] for g in pg.group_gpus]}
                           for pg in top.proc_groups], "misc": [c.core for c in top.misc_cores]}
        if ids != want:
            self._batch_ids.pop(node.name, None)
            return False
        claim = set()
        for gi, pg in enumerate(top.proc_groups):
            if any(getattr(c.nic_dir, "value", c.nic_dir) in (1, 2) for c in pg.proc_cores):
                numa, idx = mapping["nic"][gi]
                claim.add(next(k for k, n in enumerate(node.nics) if n.idx == idx and n.numa_node == numa))
        self._claims[node.name] = frozenset(claim)             # the device already zeroed these NICs' capacities
        # SetBusy marked the node.  A commit made for this very call carried the node's busy time; a placement the device
        # committed earlier inside a batch carried the batch's `now` - the busy time SetBusy wrote since (time.monotonic(),
        # nhd/Node.py:843-845) then follows as a delta of its own
        carried = set() if from_batch else {"busy_time", "SetBusy"}
        one = self._one
        if from_batch and one is not None and one[2] is ids and float(node.busy_time) == one[1]:
            carried = {"busy_time", "SetBusy"}                 # ScheduleOne committed this very time (a scheduler on a virtual clock, or one
                                                               # that hands its SetBusy time in): nothing left to send
        left = self._reasons.get(node.name, set()) - carried
        if left:
            self._reasons[node.name] = left                    # cordon / maintenance / groups written earlier still go out as deltas
        else:
            self._dirty.pop(node.name, None)
            self._reasons.pop(node.name, None)
        return True

    def _on_claim(self, node, nidx) -> bool:
        want = self._claims.pop(node.name, None) if hasattr(self, "_claims") else None
        return want is not None and frozenset(nidx) == want

    # ---- release / reclaim / reset mirrored on the device (row f2, "K3") ---------------------
    _SCALAR_REASONS = frozenset(("active", "maintenance", "groups", "busy_time", "SetBusy", "SetGroups"))

    def _on_topology(self, node, name, top) -> bool:
        """After the reference's RemoveResourcesFromTopology / AddResourcesFromTopology ran on an attached node: the same
        change as a delta record for nhdfit_apply_deltas (sent with the next flush).  True = no re-pack needed."""
        if self._attached is None or node.name not in self._index or self._waits_for_repack(node.name) or self._off_planes(node.name):
            return False
        try:
            op = pack.DELTA_TAKE if name == "RemoveResourcesFromTopology" else pack.DELTA_GIVE
            self._deltas.append(self.packer.delta_from_topology(self._index[node.name], node, top, op))
        except Exception:  # noqa: BLE001 - any doubt (ids outside the node ...): re-pack
            return False
        return True

    def _on_queued_scalar(self, node, what: str) -> bool:
        if self._attached is None or node.name not in self._index or self._waits_for_repack(node.name) or self._off_planes(node.name):
            return False
        self._deltas.append(self.packer.delta_scalar(self._index[node.name], node, what))
        return True

    def _flush_deltas(self) -> None:
        """Queued deltas -> device.  A node whose delta comes back with a status (pods_used out of the tracked range, NIC
        state without a signature) is re-packed from its object like any other dirty node."""
        if not self._deltas:
            return
        q = [d for d in self._deltas if not self._waits_for_repack(self._names[int(d["node"])])]
        self._deltas = []
        if not q:
            return
        self.engine.set_dictionary(self.packer)            # a SetGroups may have interned a new group set
        status = self.engine.apply_deltas(np.array(q, dtype=pack.DELTA))
        self.delta_stats["applied"] += len(q)
        for d, st in zip(q, status):
            if st != pack.DELTA_OK:
                name = self._names[int(d["node"])]
                if not self._waits_for_repack(name):
                    self.delta_stats["repacked"] += 1
                self._mark(self._attached[name], "delta-status")

    def _mark(self, node, reason: str = "") -> None:
        self._dirty[node.name] = node
        self._reasons.setdefault(node.name, set()).add(reason)

    def _waits_for_repack(self, name: str) -> bool:
        """The node waits for a re-pack: its pending change is more than writes to scalar fields (those travel as deltas of their
        own and commute with commits and releases).  Asked per node: every commit of a pending list asks it, and a set over ALL
        dirty nodes per question made the scheduler's loop quadratic in the list's length (round 6: 512 pods, 109 k look-ups)."""
        return name in self._dirty and (not self._reasons.get(name, {""}) <= self._SCALAR_REASONS or self._off_planes(name))

    @property
    def _dirty_strict(self):
        """All such nodes (diagnostics and tests; the hot paths ask _waits_for_repack)."""
        return {nm for nm in self._dirty if self._waits_for_repack(nm)}

    def mark_dirty(self, name: str) -> None:
        if self._attached is not None and name in self._attached:
            self._mark(self._attached[name], "explicit")

    def _full_upload(self, nl: Dict[str, object]) -> None:
        self._last_subset = None                           # node indices change
        self._digest_cache = None                          # (a re-pack notes the mirror's speeds afresh, Packer.share_exact)
        table = self.packer.pack_nodes(nl)
        self._table = table
        self._names = table.names
        self._index = {nm: i for i, nm in enumerate(table.names)}
        self.engine.reset_nodes()
        self.engine.set_dictionary(self.packer)
        if table.n:
            self.engine.upload(table)

    def _flush_dirty(self) -> None:
        if any(nm not in self._index for nm in self._dirty):
            self._full_upload(self._attached)          # nodes were added or removed
            self._dirty.clear()
            self._reasons.clear()
            self._deltas = []
            return
        # writes to scalar fields (cordon / maintenance / groups / busy time, nhd/NHDScheduler.py:533-570) travel as deltas too
        for name in [nm for nm in self._dirty if self._reasons.get(nm, {""}) <= self._SCALAR_REASONS and not self._off_planes(nm)]:
            node, why = self._dirty.pop(name), self._reasons.pop(name)
            i = self._index[name]
            if why & {"active", "maintenance"}:
                self._deltas.append(self.packer.delta_scalar(i, node, "active"))
            if why & {"groups", "SetGroups"}:
                self._deltas.append(self.packer.delta_scalar(i, node, "groups"))
            if why & {"busy_time", "SetBusy"}:
                self._deltas.append(self.packer.delta_scalar(i, node, "busy_time"))
        self._flush_deltas()
        if not self._dirty:
            return
        one = pack.empty_table(1)
        for name, node in self._dirty.items():
            i = self._index[name]
            self.packer.pack_node_into(node, one, 0)
            for f in ("p0", "p1", "p2", "p3", "p4", "detail", "origin"):
                getattr(self._table, f)[i] = getattr(one, f)[0]
            if self._table.wide is None:
                self._table.wide = {}
            if one.wide and 0 in one.wide:                     # a wide node: its record travels with the (placeholder) planes
                self._table.wide[i] = one.wide[0].copy()
            else:
                self._table.wide.pop(i, None)
            if self._table.share is None:
                self._table.share = {}
            if one.share and 0 in one.share:                   # ... and, under ENABLE_SHARING, its NICs' speed_used
                self._table.share[i] = one.share[0].copy()
            else:
                self._table.share.pop(i, None)
        self.engine.set_dictionary(self.packer)        # signatures may have been added
        idx = sorted(self._index[nm] for nm in self._dirty)
        lo = 0
        while lo < len(idx):                           # upload contiguous runs
            hi = lo
            while hi + 1 < len(idx) and idx[hi + 1] == idx[hi] + 1:
                hi += 1
            self.engine.upload(self._table.slice(idx[lo], idx[hi] + 1), first=idx[lo], capacity=self._table.n)
            lo = hi + 1
        self._dirty.clear()
        self._reasons.clear()

    def _candidates(self, nl: Dict[str, object]) -> Optional[np.ndarray]:
        """Bitmask [chunks] (bit = node) of the attached nodes that are in `nl`; None when nl is everything."""
        n = len(self._names)
        names = list(nl)
        if len(names) == n and names == self._names:          # C-speed comparison (identical str objects short-cut)
            return None
        # pods of one node group get the same filtered dict from InitialNodeFilter time after time: the masks of the subsets seen
        # lately are kept, and recognising one is a C-speed list comparison instead of a dictionary look-up per node
        key = (len(names), names[0], names[len(names) // 2], names[-1]) if names else (0,)
        if self._last_subset is not None:
            for cached, cached_mask in self._last_subset.get(key, ()):
                if names == cached:                            # (identical str objects short-cut: a pointer comparison per name)
                    return cached_mask
        idx = np.fromiter(map(self._index.__getitem__, names), dtype=np.int64, count=len(names))
        if len(idx) > 1 and not np.all(idx[1:] > idx[:-1]):
            raise ValueError("FindNode: `nl` must keep the relative order of the attached node dict")
        bits = np.zeros(((n + 63) // 64) * 64, dtype=bool)
        bits[idx] = True
        mask = np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))
        if self._last_subset is None or self._subset_names + len(names) > (1 << 22):   # (bounded: four million names kept, then start over)
            self._last_subset, self._subset_count, self._subset_names = {}, 0, 0
        self._last_subset.setdefault(key, []).append((names, mask))
        self._subset_count += 1
        self._subset_names += len(names)
        return mask

    # ---- the reference interface ----------------------------------------------------------
    def FindNode(self, nl: Dict[str, object], top) -> Tuple:
        return self.FindNodes(nl, [top])[0]

    def ScheduleBatch(self, nl: Dict[str, object], tops: Sequence[object],
                      pod_groups: Optional[Sequence[Sequence[str]]] = None, now: Optional[float] = None,
                      apply: bool = False) -> List[Tuple]:
        """Mode B: the result list the scheduler loop would produce by calling FindNode and committing each
        winner before the next pod (nhd/NHDScheduler.py:289-304, 425-437) - decided AND committed on the device in
        one pass (nhdfit_schedule_batch).  `self.last_placements[i]` holds pod i's physical ids (the lists
        SetPhysicalIdsFromMapping would write into its topology, pack.expand_placement) or None.
        The node objects are NOT modified: apply each placement with the node's own SetBusy /
        SetPhysicalIdsFromMapping / ClaimPodNICResources, exactly as AttemptScheduling does.  apply=True keeps the
        commits in the device mirror (attached mode: the reference mutators that follow are then recognised as
        already mirrored); apply=False restores it."""
        return self._run(nl, tops, pod_groups, now, sequential=True, apply=apply)

    def ScheduleOne(self, nl: Dict[str, object], top, pod_groups: Optional[Sequence[str]] = None, now: Optional[float] = None,
                    busy_time: Optional[float] = None) -> Tuple:
        """FindNode for one pod AND the commit step on its winner in the device mirror, in one device call (nhdfit_find_commit: one
        launch where the lone-pod form of the find applies).  Returns what FindNode returns - `(name, mapping)` or `(None,)`; the
        contract is ScheduleBatch(apply=True)'s with one pod: `self.last_placements == [ids]`, the node objects are NOT touched, and
        in attached mode the scheduler's own SetBusy / SetPhysicalIdsFromMapping / ClaimPodNICResources that follow
        (nhd/NHDScheduler.py:289-304) find their work mirrored already; a placement the caller never applies makes the node re-pack
        from its object before the next call.  `busy_time`: what the commit writes as the node's busy time; with `now` and
        `busy_time` both left out ONE reading of the clock serves as both, given alone each is used as given and the other read from
        the clock.  The time SetBusy writes afterwards does not go out as a delta of its own: equal to the committed one it is
        dropped, otherwise it rides in the next ScheduleOne (any other call flushes it as an ordinary SET_BUSY delta first).
        Pods of the general path, mirrors with wide nodes, ENABLE_SHARING and engines without find_commit are composed from
        FindNodes + CommitPlacement: the same answer."""
        try:
            return self._schedule_one(nl, top, pod_groups, now, busy_time)
        except NhdFitError as e:
            if self.strict:
                raise
            self.logger.error("ScheduleOne: the device path failed (%s): the pod is answered (None,)", e)
            self._mirror_foreign = True                   # whatever the mirror holds now, rebuild it before the next call
            self._last_subset = None
            self._one = None
            self.last_placements = [None]
            return (None,)

    _BUSY_REASONS = frozenset(("busy_time", "SetBusy"))

    def _schedule_one(self, nl, top, pod_groups, now, busy_time) -> Tuple:
        if len(top.proc_groups) == 0 and len(nl):
            raise IndexError("pod without processing groups (the reference fails the same way, Matcher.py:346)")
        self.last_placements = [None]
        if len(nl) == 0:
            return (None,)
        if now is None and busy_time is None:
            now = busy_time = self.clock()
        else:
            now = self.clock() if now is None else now
            busy_time = self.clock() if busy_time is None else busy_time
        groups = None if pod_groups is None else [pod_groups]
        one, self._one = self._one, None
        if self._attached is None:                         # stateless: every call packs `nl` again - ScheduleBatch's path serves it
            return self._run_checked(nl, [top], groups, now, sequential=True, apply=True)[0]
        if not hasattr(self.engine, "find_commit") or pack.needs_general_path(top) or self.packer.sharing or (self._table is not None and self._table.wide):
            return self._schedule_one_composed(nl, top, groups, now, busy_time)
        # the one pending correction: the last winner, dirty for nothing but the time SetBusy wrote behind the commit
        late = None
        if one is not None and one[0] in self._dirty and one[0] not in self._batch_ids and self._reasons.get(one[0], {""}) <= self._BUSY_REASONS:
            late = self._dirty.pop(one[0])
            self._reasons.pop(one[0], None)
        cand = self._sync_mirror(nl)
        beyond: List[Tuple[int, str]] = []
        reqs = self.packer.digest_many([top], groups, unsupported=beyond)
        if beyond or self._mirror_foreign or self.packer.sharing or self._table.wide:
            if late is not None:
                self._mark(late, "busy_time")              # (travels as a delta after all)
            if beyond:
                self.logger.error("the pod cannot be expressed as a request record and is answered (None,): %s", beyond[0][1])
                return (None,)
            return self._schedule_one_composed(nl, top, groups, now, busy_time)
        prev = None
        if late is not None and late.name in self._index and not self._off_planes(late.name):
            prev = (self._index[late.name], float(late.busy_time))
        self.packer.close_signatures()                     # every NIC state a commit can produce has a signature
        self.engine.set_dictionary(self.packer)
        score, mp, place, done = self.engine.find_commit(reqs[0], now, busy_time, cand=cand, prev=prev)
        if not score:
            return (None,)
        i = winner_index(score) - self.engine.global_base
        name = self._names[i]
        gpu, cpu, nic_numa, nic_idx, valid = pack.unpack_mappings(mp.reshape(1))[0]
        if not valid or not done:
            raise RuntimeError(f"internal error: no mapping / no commit produced for feasible node {name}")
        status = int(place["status"])
        if status == pack.COMMIT_NEW_SIG:                  # cannot happen after close_signatures(); handled anyway (CommitPlacement)
            fix = self.engine.download(i, 1)
            sn, sp = self.packer.sigs_from_detail(fix.detail[0])
            fix.p3[0]["sig_numa"], fix.p3[0]["sig_pci"] = sn, sp
            self.engine.set_dictionary(self.packer)
            self.engine.upload(fix, first=i, capacity=len(self._names))
        elif status == pack.COMMIT_WOULD_RAISE:
            self.logger.warning("ScheduleOne: the reference's commit step would have failed on node %s", name)
        G = int(reqs[0]["n_groups"])
        nd = self._attached.get(name)
        if nd is not None:
            cpp = int(nd.cores_per_proc)
            ids = pack.expand_placement(place, G, cpp, cpp * int(nd.sockets), [int(reqs[0]["gpus"][g]) for g in range(G)])
            self.last_placements = [ids]
            self._batch_ids.setdefault(name, []).append(ids)    # the reference mutators that follow find their work mirrored already
            self._one = (name, float(busy_time), ids)
        return (name, {"gpu": gpu[:G], "cpu": cpu[:G + 1], "nic": list(zip(nic_numa[:G], nic_idx[:G]))})

    def _schedule_one_composed(self, nl, top, groups, now, busy_time) -> Tuple:
        """ScheduleOne from the existing methods: FindNodes' path, then CommitPlacement on the winner."""
        r = self._run_checked(nl, [top], groups, now, sequential=False)[0]
        self.last_placements = [None]
        if r[0] is None:
            return r
        if self._mirror_foreign or r[0] not in self._attached:     # `nl` is not (part of) the attached dict: as the stateless form
            return self._run_checked(nl, [top], groups, now, sequential=True, apply=True)[0]
        ids = self.CommitPlacement(r[0], top, r[1], busy_time=busy_time)
        self.last_placements = [ids]
        if self._off_planes(r[0]):                         # a wide record is re-packed from the object before the next call (no delta form)
            self._mark(self._attached[r[0]], "wide-batch")
        else:
            self._batch_ids.setdefault(r[0], []).append(ids)
            self._one = (r[0], float(busy_time), ids)
        return r

    def FindNodes(self, nl: Dict[str, object], tops: Sequence[object],
                  pod_groups: Optional[Sequence[Sequence[str]]] = None, now: Optional[float] = None) -> List[Tuple]:
        """Mode-A batch: every pod of `tops` against the same snapshot of `nl`.  With `pod_groups`
        the kernel applies InitialNodeFilter itself (nl = all nodes); without, `nl` is taken as already
        filtered, exactly like the argument of Matcher.FindNode."""
        return self._run(nl, tops, pod_groups, now, sequential=False)

    def FindNodesFromConfigs(self, nl: Dict[str, object], cfg_texts: Sequence[str],
                             pod_groups: Optional[Sequence[Sequence[str]]] = None, now: Optional[float] = None,
                             sequential: bool = False) -> List[Tuple]:
        """Batch matching straight from the pods' Triad libconfig texts: no
        TriadCfgParser / CfgTopology object graph per pending pod (nhd/NHDScheduler.py:262-277) - the texts are
        digested by host C++ in libnhdfit.so (nhd_amd/wire.py).  A text for which the reference's CfgToTopology
        returns None yields `(None,)`, like the scheduler skipping that pod.  The caller parses the config of a
        pod it actually binds (the commit step needs the CfgTopology, nhd/NHDScheduler.py:289-304)."""
        from . import wire
        if not cfg_texts:
            return []
        reqs, codes = wire.digest_configs(cfg_texts)
        big_reqs = {}
        for i in np.flatnonzero(codes > wire.WIRE_NONE):
            if codes[i] == wire.WIRE_LIMIT:                  # more than four processing groups: up to eight ride the general path
                big_reqs[int(i)] = wire.digest_config_big(cfg_texts[int(i)])       # (raises what the limit really is beyond that)
            else:                                            # what the reference would raise on: report it properly
                wire.digest_config(cfg_texts[int(i)])
        # a hugepage request beyond the tile's table digests without a code: such a pod is a big request too, as FindNodes(tops)
        # routes it (pack.needs_general_path) - staged with the others it would fail the whole call with NHDFIT_E_LIMIT
        for i in np.flatnonzero((codes == 0) & (reqs["hugepages_gb"] > pack.MAX_HUGEPAGES_GB)):
            big_reqs[int(i)] = wire.digest_config_big(cfg_texts[int(i)])
        skip = codes == wire.WIRE_NONE                       # all-zero (= never matching) requests
        # (the pods' group bits are filled in by _run, after the mirror - and with it the dictionary - is current)
        for i in np.flatnonzero(~skip):
            if int(i) not in big_reqs and reqs[i]["n_groups"] == 0 and len(nl):
                raise IndexError("pod without processing groups (the reference fails the same way, Matcher.py:346)")
        out = self._run(nl, None, pod_groups, now, sequential, reqs=reqs, big_reqs=big_reqs)
        return [(None,) if skip[i] else out[i] for i in range(len(cfg_texts))]

    def ExplainNode(self, nl: Dict[str, object], top, now: Optional[float] = None, per_node: bool = False) -> Explanation:
        """ExplainNodes for one pod."""
        return self.ExplainNodes(nl, [top], now=now, per_node=per_node)[0]

    def _without_unmirrored(self, cand: Optional[np.ndarray]) -> Tuple[Optional[np.ndarray], List[int]]:
        """(`cand` without the nodes the device does not hold, their indices): a stage query leaves them out of the call - their
        placeholders would be charged to a stage - and reports them on their own."""
        off = [self._index[nm] for nm in self.packer.unmirrored if nm in self._index]
        if off:
            n = len(self._names)
            bits = np.zeros(((n + 63) // 64) * 64, dtype=bool)
            if cand is None:
                bits[:n] = True
            else:
                bits[:] = np.unpackbits(cand.view(np.uint8), bitorder="little").astype(bool)
            bits[off] = False
            cand = np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))
        return cand, off

    def _outside(self, cand: Optional[np.ndarray]) -> int:
        """Nodes of the mirror outside `cand` - not in the caller's `nl`, or unmirrored: the device charges them NOT_CANDIDATE."""
        n = len(self._names)
        return 0 if cand is None else n - int(np.unpackbits(cand.view(np.uint8), bitorder="little")[:n].sum())

    def ExplainNodes(self, nl: Dict[str, object], tops: Sequence[object], pod_groups: Optional[Sequence[Sequence[str]]] = None,
                     now: Optional[float] = None, per_node: bool = False) -> List[Explanation]:
        """Why each node of `nl` turned each pod of `tops` away, counted on the device (nhdfit_explain): one Explanation per pod,
        for the same mirror state FindNodes(nl, tops, pod_groups, now) answers from (pending changes are flushed the same way).
        Pods with 5..8 processing groups (or hugepage requests beyond the pod tile) take nhdfit_explain_big, as FindNodes routes
        them; wide and ENABLE_SHARING nodes are answered by their own records.  Nothing about the mirror changes.  A pod that cannot
        be evaluated - a request no record can express, a big request whose NIC search runs out of budget - is logged and comes back
        with `error` set and nothing charged to the cluster (strict=True raises instead); other device errors raise."""
        n_pods = len(tops)
        for top in tops:
            if len(top.proc_groups) == 0 and len(nl):
                raise IndexError("pod without processing groups (the reference fails the same way, Matcher.py:346)")
        if n_pods == 0:
            return []
        if len(nl) == 0:
            return [Explanation({s: 0 for s in STAGES}, 0, np.zeros(0, np.uint8) if per_node else None, nodes=0) for _ in range(n_pods)]
        now = self.clock() if now is None else now
        cand = self._sync_mirror(nl)
        n = len(self._names)
        cand, off = self._without_unmirrored(cand)
        outside = self._outside(cand)
        n_unmirrored = sum(1 for nm in nl if nm in self.packer.unmirrored)
        is_big = [pack.needs_general_path(top) for top in tops]
        big_recs = {}
        for p in range(n_pods):
            if is_big[p]:
                try:
                    big_recs[p] = self.packer.digest_big(tops[p], None if pod_groups is None else pod_groups[p])
                except pack.UnsupportedNode:               # beyond the big record too: the ordinary digest reports it (an all-zero record)
                    if self.strict:
                        raise
                    is_big[p] = False
        small_idx = [p for p in range(n_pods) if not is_big[p]]
        errors: Dict[int, str] = {}
        counts = np.zeros((n_pods, len(STAGES)), np.int64)
        stages = np.zeros((n_pods, n), np.uint8) if per_node else None
        if small_idx:
            beyond: List[Tuple[int, str]] = []
            reqs = self.packer.digest_many([tops[p] for p in small_idx], None if pod_groups is None else [pod_groups[p] for p in small_idx],
                                           unsupported=beyond)
            for k, why in beyond:                          # (an all-zero record: the kernel would charge every node NOT_CANDIDATE)
                self.logger.error("explain: pod %d of the call cannot be expressed as a request record and is not evaluated: %s", small_idx[k], why)
                errors[small_idx[k]] = f"it cannot be expressed as a request record ({why})"
            c, st = self.engine.explain(reqs, now, cand=cand, per_node=per_node)
            counts[small_idx] = c
            if per_node:
                stages[small_idx] = st
        if big_recs:
            big_idx = sorted(big_recs)
            try:
                c, st = self.engine.explain(np.array([big_recs[p] for p in big_idx], dtype=pack.BIG_REQ), now, cand=cand, per_node=per_node)
                counts[big_idx] = c
                if per_node:
                    stages[big_idx] = st
            except NhdFitError as e:                       # (NHDFIT_E_LIMIT: a NIC search beyond its budget - nothing is known for these pods)
                if self.strict:
                    raise
                self.logger.error("explain: the pods with 5..8 processing groups of the call are not evaluated (%s)", e)
                for p in big_idx:
                    errors[p] = f"the device could not evaluate it ({e})"
        counts[:, 0] -= outside                            # (the kernel counts every node of the mirror outside `cand` as NOT_CANDIDATE)
        order = None
        if per_node:
            order = np.fromiter((self._index[nm] for nm in nl), dtype=np.int64, count=len(nl))
            if off:
                stages[:, off] = UNMIRRORED
        out = []
        for p in range(n_pods):
            if p in errors:
                out.append(Explanation({s: 0 for s in STAGES}, n_unmirrored, None, error=errors[p], nodes=len(nl)))
                continue
            out.append(Explanation({s: int(counts[p, k]) for k, s in enumerate(STAGES)}, n_unmirrored,
                                   stages[p, order] if per_node else None, nodes=len(nl)))
        return out

    def Headroom(self, nl: Dict[str, object], top, pod_groups: Optional[Sequence[str]] = None, per_node: bool = False,
                 max_per_node: int = 512, strict: Optional[bool] = None, limits: bool = False, general: bool = False) -> Headroom:
        """HeadroomMany for one pod template."""
        return self.HeadroomMany(nl, [top], None if pod_groups is None else [pod_groups], per_node=per_node, max_per_node=max_per_node,
                                 strict=strict, limits=limits, general=general)[0]

    def HeadroomMany(self, nl: Dict[str, object], tops: Sequence[object], pod_groups: Optional[Sequence[Sequence[str]]] = None,
                     per_node: bool = False, max_per_node: int = 512, strict: Optional[bool] = None, limits: bool = False,
                     general: bool = False) -> List[Headroom]:
        """How many more replicas of each pod template of `tops` the nodes of `nl` can take, counted on the device (nhdfit_headroom):
        per node the number of times FindNode -> SetPhysicalIdsFromMapping -> ClaimPodNICResources succeeds back to back on a private
        copy of the node, busy windows out of the way (capacity, not rate: there is no `now`).  The mirror state is the one
        FindNodes(nl, tops, pod_groups) answers from (pending changes are flushed the same way); nothing about it changes.
        `max_per_node` (1..16383) bounds a node's run - a template that asks for nothing would fit for ever.  Without
        `general`, wide nodes and ENABLE_SHARING mirrors are reported as not evaluated, never as a number.  A template no request record can express (5..8
        processing groups, hugepages beyond the pod tile, an unsupported request) or a device error comes back with `error` set
        and everything not evaluated - `strict=True` (default: the matcher's) raises instead.
        limits=True (nhdfit_headroom_limits): the same figures and, per template, the stage that ended each node's run - the stage
        ExplainNode would name for the template on the node in the state its last replica left it, nothing busy (Headroom.limits,
        Headroom.limit_stages, Headroom.limit_summary()).
        general=True (nhdfit_headroom_general): wide nodes and the nodes of an ENABLE_SHARING mirror are counted as well - the same
        sequence on a private copy of the node's wide record and, under ENABLE_SHARING, of its NICs' speed_used, so that each replica
        is priced against what the earlier ones use - and are part of every sum; the other nodes are answered exactly as without it.
        What the packer refuses under ENABLE_SHARING (several RX / TX cores of a group at speeds that do not add exactly) stays
        refused, templates of 5..8 processing groups still come back with `error`, and limits=True is not available with it
        (ValueError)."""
        if general and limits:
            raise ValueError("general=True and limits=True: the limits are answered for the fast layout only (nhdfit_headroom_limits)")
        strict = self.strict if strict is None else strict
        n_pods = len(tops)
        if n_pods == 0:
            return []
        if not 1 <= int(max_per_node) <= pack.HEADROOM_COUNT_MASK:
            raise ValueError(f"max_per_node is {max_per_node} (1 .. {pack.HEADROOM_COUNT_MASK})")
        names = list(nl)
        if len(nl) == 0:
            return [Headroom(0, names, max_per_node=max_per_node, per_node=np.zeros(0, np.uint16) if per_node else None,
                             flags=np.zeros(0, np.uint16) if per_node else None, limits={s: 0 for s in STAGES} if limits else None,
                             limit_stages=np.zeros(0, np.uint8) if limits and per_node else None) for _ in range(n_pods)]
        errors: Dict[int, str] = {}
        for p, top in enumerate(tops):
            if len(top.proc_groups) == 0:
                errors[p] = "it has no processing groups (the reference fails on such a pod, Matcher.py:346)"
            elif pack.needs_general_path(top):
                errors[p] = "it takes the general path (5..8 processing groups or a hugepage request beyond the pod tile), which headroom does not cover"
        if errors and strict:
            raise pack.UnsupportedNode(f"headroom: pod {min(errors)} of the call: {errors[min(errors)]}")
        cand = self._sync_mirror(nl)
        n_unmirrored = sum(1 for nm in nl if nm in self.packer.unmirrored)
        idx = [p for p in range(n_pods) if p not in errors]
        sums, counts, hist, stages = None, None, None, None
        if idx:
            beyond: List[Tuple[int, str]] = []
            reqs = self.packer.digest_many([tops[p] for p in idx], None if pod_groups is None else [pod_groups[p] for p in idx], unsupported=beyond)
            for k, why in beyond:
                if strict:
                    raise pack.UnsupportedNode(f"headroom: pod {idx[k]} of the call: {why}")
                errors[idx[k]] = f"it cannot be expressed as a request record ({why})"
            try:
                self.packer.close_signatures()             # every NIC state a commit can produce has a signature
                self.engine.set_dictionary(self.packer)
                if limits:
                    cand, off = self._without_unmirrored(cand)     # (as ExplainNodes: their count is 0 either way)
                    sums, counts, hist, stages = self.engine.headroom_limits(reqs, cand=cand, max_per_node=int(max_per_node), per_node=per_node)
                elif general:
                    sums, counts = self.engine.headroom_general(reqs, cand=cand, max_per_node=int(max_per_node), per_node=per_node)
                else:
                    sums, counts = self.engine.headroom(reqs, cand=cand, max_per_node=int(max_per_node), per_node=per_node)
            except NhdFitError as e:
                if strict:
                    raise
                for p in idx:
                    errors.setdefault(p, f"the device could not evaluate it ({e})")
        for p in sorted(errors):
            self.logger.error("headroom: pod %d of the call is not evaluated: %s", p, errors[p])
        order = np.fromiter((self._index[nm] for nm in nl), dtype=np.int64, count=len(nl)) if per_node else None
        outside = 0
        if limits and hist is not None:
            outside = self._outside(cand)
            if per_node and off:
                stages[:, off] = UNMIRRORED
        out = []
        for p in range(n_pods):
            if p in errors:
                out.append(Headroom(len(nl), names, not_evaluated=len(nl), unmirrored=n_unmirrored, max_per_node=max_per_node, error=errors[p],
                                    limits={s: 0 for s in STAGES} if limits else None))
                continue
            k = idx.index(p)
            sm = sums[k]
            e = counts[k][order] if per_node else None
            lim = None
            if limits:
                lim = {s: int(hist[k, j]) for j, s in enumerate(STAGES)}
                lim["NOT_CANDIDATE"] -= outside
            out.append(Headroom(len(nl), names, replicas=sm["replicas"], nodes_with_room=sm["nodes_with_room"], max_on_one_node=sm["max_on_one_node"],
                                saturated=sm["saturated"], stopped=sm["stopped"], not_evaluated=sm["not_evaluated"], unmirrored=n_unmirrored,
                                form=sm["form"], max_per_node=max_per_node,
                                per_node=None if e is None else (e & np.uint16(pack.HEADROOM_COUNT_MASK)),
                                flags=None if e is None else (e & np.uint16(pack.HEADROOM_STOPPED | pack.HEADROOM_NOT_EVALUATED)),
                                limits=lim, limit_stages=stages[k][order] if limits and per_node else None))
        return out

    def Candidates(self, nl: Dict[str, object], top, k: int = 8, pod_groups: Optional[Sequence[str]] = None, now: Optional[float] = None,
                   strict: Optional[bool] = None, general: bool = False, big: bool = False) -> Candidates:
        """CandidatesMany for one pod."""
        return self.CandidatesMany(nl, [top], k=k, pod_groups=None if pod_groups is None else [pod_groups], now=now, strict=strict,
                                   general=general, big=big)[0]

    def CandidatesMany(self, nl: Dict[str, object], tops: Sequence[object], k: int = 8, pod_groups: Optional[Sequence[Sequence[str]]] = None,
                       now: Optional[float] = None, strict: Optional[bool] = None, general: bool = False, big: bool = False) -> List[Candidates]:
        """Where else each pod of `tops` could go: per pod the first `k` (1..64) nodes of `nl` in the order the scheduler would get to
        them, each with the mapping FindNode gives for it, picked and mapped on the device in one call (nhdfit_candidates).
        entries[0] is FindNode's answer; entries[j] is what Matcher().FindNode answers on `nl` without the j nodes in front of it
        (nhd/Matcher.py:393-421: index order; for a pod without GPUs the nodes without GPUs first) - what a scheduler tries next
        when a bind fails (nhd/NHDScheduler.py:291-345), and the feasible set a caller's own policy chooses from.  The mirror state
        is the one FindNodes(nl, tops, pod_groups, now) answers from; nothing about it changes.
        Pods of the general path (5..8 processing groups, hugepages beyond the pod tile), mirrors with wide nodes and ENABLE_SHARING
        are composed from FindNodes with the earlier answers left out of `nl`, and ExplainNodes' FITS count: the same answer, slower.
        general=True (nhdfit_candidates_general): every pod that is not of the general path is answered by the device call on ANY
        mirror - plain, with wide nodes, ENABLE_SHARING - the wide records ranked and mapped with the others; pods of the general
        path are still composed unless `big` is given.
        big=True (nhdfit_candidates_big): every pod of the general path - 5..8 processing groups, hugepages beyond the pod tile - is
        digested as a big request, and all of them are answered by ONE device call on whatever mirror is attached: every mirrored
        node, wide records included, ranked and mapped as FindNode would.  The other pods go where `general` sends them.
        A pod no request record can express, or a device error, comes back with `error` set and an empty list - `strict=True`
        (default: the matcher's) raises instead."""
        strict = self.strict if strict is None else strict
        k = int(k)
        if not 1 <= k <= pack.CANDIDATES_MAX_K:
            raise ValueError(f"k is {k} (1 .. {pack.CANDIDATES_MAX_K})")
        n_pods = len(tops)
        if n_pods == 0:
            return []
        if len(nl) == 0:
            return [Candidates([], k=k) for _ in range(n_pods)]
        errors: Dict[int, str] = {}
        for p, top in enumerate(tops):
            if len(top.proc_groups) == 0:
                errors[p] = "it has no processing groups (the reference fails on such a pod, Matcher.py:346)"
        if errors and strict:
            raise pack.UnsupportedNode(f"candidates: pod {min(errors)} of the call: {errors[min(errors)]}")
        now = self.clock() if now is None else now
        cand = self._sync_mirror(nl)
        out: Dict[int, Candidates] = {}
        # mirrors the plain device entry does not list: every pod is composed
        whole = not general and (self.packer.sharing or bool(self._table.wide))
        idx = [p for p in range(n_pods) if p not in errors and not whole and not pack.needs_general_path(tops[p])]
        if idx:
            beyond: List[Tuple[int, str]] = []
            reqs = self.packer.digest_many([tops[p] for p in idx], None if pod_groups is None else [pod_groups[p] for p in idx], unsupported=beyond)
            for j, why in beyond:
                if strict:
                    raise pack.UnsupportedNode(f"candidates: pod {idx[j]} of the call: {why}")
                errors[idx[j]] = f"it cannot be expressed as a request record ({why})"
            try:
                sums, entries = self.engine.candidates(reqs, now, k, cand=cand, **({"general": True} if general else {}))
            except NhdFitError as e:
                if strict:
                    raise
                sums = None
                for p in idx:
                    errors.setdefault(p, f"the device could not evaluate it ({e})")
            base = self.engine.global_base
            for j, p in enumerate(idx):
                if p in errors:
                    continue
                G = int(reqs[j]["n_groups"])
                got = int(sums[j]["returned"])
                rows = pack.unpack_mappings(np.ascontiguousarray(entries[j]["map"][:got]))
                listed = []
                for e, (gpu, cpu, nic_numa, nic_idx, valid) in zip(entries[j]["score"][:got].tolist(), rows):
                    name = self._names[winner_index(e) - base]
                    if not valid:
                        raise RuntimeError(f"internal error: no mapping produced for feasible node {name}")
                    listed.append((name, {"gpu": gpu[:G], "cpu": cpu[:G + 1], "nic": list(zip(nic_numa[:G], nic_idx[:G]))}))
                out[p] = Candidates(listed, feasible=sums[j]["feasible"], preferred=sums[j]["preferred"], k=k, nodes=len(nl), form=sums[j]["form"])
        if big:                                            # the pods of the general path: one device call on any mirror
            self._candidates_big(tops, pod_groups, k, now, cand, strict, len(nl), errors, out)
        for p in range(n_pods):                            # the rest is composed (behind the device call: it matches subsets of `nl`)
            if p in errors or p in out:
                continue
            try:
                out[p] = self._candidates_composed(nl, tops[p], k, None if pod_groups is None else pod_groups[p], now)
            except (NhdFitError, pack.UnsupportedNode) as e:
                if strict:
                    raise
                if isinstance(e, NhdFitError):
                    self._mirror_foreign = True            # whatever the mirror holds now, rebuild it before the next call
                    self._last_subset = None
                errors[p] = f"the device could not evaluate it ({e})"
        for p in sorted(errors):
            self.logger.error("candidates: pod %d of the call is not evaluated: %s", p, errors[p])
            out[p] = Candidates([], k=k, nodes=len(nl), error=errors[p])
        return [out[p] for p in range(n_pods)]

    def _candidates_big(self, tops, pod_groups, k, now, cand, strict, n_nodes, errors, out) -> None:
        """CandidatesMany(big=True) for the pods of the general path: their big request records through ONE engine.candidates_big
        call; answers into `out`, the pods that cannot be answered into `errors`."""
        idx, recs = [], []
        for p, top in enumerate(tops):
            if p in errors or p in out or not pack.needs_general_path(top):
                continue
            try:
                recs.append(self.packer.digest_big(top, None if pod_groups is None else pod_groups[p]))
                idx.append(p)
            except pack.UnsupportedNode as e:              # beyond the big record too (a group of more than 255 cores ...)
                if strict:
                    raise pack.UnsupportedNode(f"candidates: pod {p} of the call: {e}") from None
                errors[p] = f"it cannot be expressed as a request record ({e})"
        if not idx:
            return
        reqs = np.array(recs, dtype=pack.BIG_REQ)
        try:
            sums, entries = self.engine.candidates_big(reqs, now, k, cand=cand)
        except NhdFitError as e:                           # (the call writes nothing: the mirror is what it was)
            if strict:
                raise
            for p in idx:
                errors[p] = f"the device could not evaluate it ({e})"
            return
        base = self.engine.global_base
        for j, p in enumerate(idx):
            G = int(reqs[j]["n_groups"])
            got = int(sums[j]["returned"])
            rows = pack.unpack_big_mappings(np.ascontiguousarray(entries[j]["map"][:got]))
            listed = []
            for e, (gpu, cpu, nic_numa, nic_idx, valid) in zip(entries[j]["score"][:got].tolist(), rows):
                name = self._names[winner_index(e) - base]
                if not valid:
                    raise RuntimeError(f"internal error: no mapping produced for feasible node {name}")
                listed.append((name, {"gpu": gpu[:G], "cpu": cpu[:G + 1], "nic": list(zip(nic_numa[:G], nic_idx[:G]))}))
            out[p] = Candidates(listed, feasible=sums[j]["feasible"], preferred=sums[j]["preferred"], k=k, nodes=n_nodes, form=sums[j]["form"])

    def _candidates_composed(self, nl, top, k, groups, now) -> Candidates:
        """Candidates from the existing methods, as ScheduleOne composes: FindNodes again and again on `nl` without the earlier
        answers (the definition itself), the counts from ExplainNodes' stages."""
        ex = self.ExplainNodes(nl, [top], None if groups is None else [groups], now=now, per_node=True)[0]
        if ex.error is not None:
            raise pack.UnsupportedNode(ex.error)
        fits = ex.stages == STAGES.index("FITS")
        preferred = 0
        if not any(len(g.group_gpus) > 0 for g in top.proc_groups):
            preferred = sum(1 for nm, ok in zip(nl, fits) if ok and len(nl[nm].gpus) == 0)
        listed: List[Tuple] = []
        rest = nl
        while len(listed) < k:
            r = self._run_checked(rest, [top], None if groups is None else [groups], now, sequential=False)[0]
            if r[0] is None:
                break
            listed.append(r)
            rest = {nm: nd for nm, nd in rest.items() if nm != r[0]}
            if not rest:
                break
        return Candidates(listed, feasible=int(fits.sum()), preferred=preferred, k=k, nodes=len(nl))

    @property
    def unmirrored(self) -> Dict[str, str]:
        """Nodes NEITHER layout holds (more than four sockets, more than 128 physical cores per socket ...; name -> reason): they never
        match, everything else is answered for.  Nodes beyond the fast layout but within the general path's (wide nodes) are not here:
        they are answered for exactly, by enumeration (`wide_nodes`)."""
        return self.packer.unmirrored

    @property
    def wide_nodes(self) -> List[str]:
        """Names of the mirrored nodes the general path serves (3-4 sockets, 65-128 physical cores per socket, ...)."""
        if self._table is None or not self._table.wide:
            return []
        return [self._names[i] for i in sorted(self._table.wide)]

    def _warn_unmirrored(self) -> None:
        for name, why in self.packer.unmirrored.items():
            if name not in self._warned:
                self._warned.add(name)
                self.logger.warning("node %s is not mirrored on the device and will never be selected: %s", name, why)

    def _sync_mirror(self, nl: Dict[str, object]) -> Optional[np.ndarray]:
        """Bring the device mirror up to what the node objects say before a call on `nl` (pending deltas and dirty nodes of the
        attached dict flushed, or `nl` packed anew); returns the candidate mask of `nl` (None: every mirrored node)."""
        cand = None
        known = False
        if self._attached is not None:
            if len(self._attached) != len(self._names) or self._mirror_foreign:
                self.attach(self._attached)                # nodes were added / removed, or a foreign dict was matched in between
            if nl is self._attached:                       # the scheduler's own dict: nothing to look up, O(1) in the node count
                known = True
            else:
                try:
                    cand = self._candidates(nl)
                    known = True
                except KeyError:                           # names the attached dict does not hold: stateless for this call
                    known = False
        if self._batch_ids:
            # placements of an earlier ScheduleBatch(apply=True) the caller never applied to its node objects: the mirror holds
            # commits the objects do not - those nodes are re-packed from their objects
            for name in list(self._batch_ids):
                nd = self._attached.get(name) if self._attached is not None else None
                if nd is not None:
                    self._mark(nd, "unapplied-batch")
            self._batch_ids.clear()
        if known:
            self._flush_dirty()
        else:
            self._full_upload(nl)
            self._mirror_foreign = self._attached is not None
        self._warn_unmirrored()
        return cand

    def _run(self, nl, tops, pod_groups, now, sequential, reqs=None, apply=False, big_reqs=None):
        try:
            return self._run_checked(nl, tops, pod_groups, now, sequential, reqs, apply, big_reqs)
        except NhdFitError as e:
            if self.strict:
                raise
            n_pods = len(tops) if reqs is None else len(reqs)
            self.logger.error("FindNode: the device path failed (%s): %d pod(s) answered (None,)", e, n_pods)
            self._mirror_foreign = True                   # whatever the mirror holds now, rebuild it before the next call
            self._last_subset = None
            self.last_placements = [None] * n_pods
            return [(None,) for _ in range(n_pods)]

    def _run_checked(self, nl, tops, pod_groups, now, sequential, reqs=None, apply=False, big_reqs=None):
        if reqs is None:
            if not tops:
                self.last_placements = []
                return []
            for top in tops:
                if len(top.proc_groups) == 0 and len(nl):
                    raise IndexError("pod without processing groups (the reference fails the same way, Matcher.py:346)")
        n_pods = len(tops) if reqs is None else len(reqs)
        if len(nl) == 0:
            return [(None,) for _ in range(n_pods)]
        now = self.clock() if now is None else now
        cand = self._sync_mirror(nl)
        if reqs is not None and self.packer.sharing:       # digested from config texts, and speed_used prices the NICs (nhd/Node.py:754)
            for arr in (reqs, *(big_reqs or {}).values()):
                for rq in (arr if arr.ndim else [arr]):
                    if int(rq["n_groups"]) == 0:
                        continue
                    why = self.packer.admit_wire_request(rq)
                    if why is not None:
                        if self.strict:
                            raise pack.UnsupportedNode(why)
                        self.logger.error("a pod of the call cannot be answered exactly and is answered (None,): %s", why)
                        rq["n_groups"] = 0                 # (an all-zero group count never matches)
        # (nhd/Node.py:20 ENABLE_SHARING = True: the packer mirrored every node for the general path, whose NIC stage prices a NIC at
        #  speed * pct - speed_used[x] as the reference does - nothing to route here: the table pass finds placeholders only)
        if reqs is None and any(pack.needs_general_path(top) for top in tops):
            # pods the table pass cannot express but the general path answers (5..8 processing groups, huge hugepage requests)
            is_big = [pack.needs_general_path(top) for top in tops]
            big_recs = []
            for p in range(n_pods):
                if not is_big[p]:
                    continue
                try:
                    big_recs.append(self.packer.digest_big(tops[p], None if pod_groups is None else pod_groups[p]))
                except pack.UnsupportedNode:               # beyond the big record too (a group of more than 255 cores ...): strict raises,
                    if self.strict:                        # otherwise the pod goes the ordinary pods' way below and is answered (None,), logged
                        raise
                    is_big[p] = False
            small_idx = [p for p in range(n_pods) if not is_big[p]]
            beyond = []
            small = self.packer.digest_many([tops[p] for p in small_idx], None if pod_groups is None else [pod_groups[p] for p in small_idx],
                                            unsupported=beyond)
            for k, why in beyond:
                self.logger.error("pod %d of the call cannot be expressed as a request record and is answered (None,): %s", small_idx[k], why)
            bigs = np.array(big_recs, dtype=pack.BIG_REQ) if big_recs else np.zeros(0, pack.BIG_REQ)
            return self._run_with_big(nl, is_big, small, bigs, now, cand, sequential, apply)
        if reqs is not None and big_reqs:                  # digested from config texts (FindNodesFromConfigs)
            is_big = [p in big_reqs for p in range(n_pods)]
            small = reqs[[p for p in range(n_pods) if not is_big[p]]]
            bigs = np.array([big_reqs[p] for p in range(n_pods) if is_big[p]], dtype=pack.BIG_REQ)
            if pod_groups is not None:
                for arr, idx in ((small, [p for p in range(n_pods) if not is_big[p]]), (bigs, [p for p in range(n_pods) if is_big[p]])):
                    for k, p in enumerate(idx):
                        arr[k]["flags"] |= pack.RF_INITIAL_FILTER
                        arr[k]["groups"] = self.packer.group_bits_known(pod_groups[p])
            return self._run_with_big(nl, is_big, small, bigs, now, cand, sequential, apply)
        if reqs is None:
            beyond: List[Tuple[int, str]] = []
            reqs = self.packer.digest_many(tops, pod_groups, unsupported=beyond)
            if n_pods == 1 and not beyond:
                self._digest_cache = (tops[0], reqs[0].copy())     # CommitPlacement of the same topology object does not digest it again
            for i, why in beyond:
                self.logger.error("pod %d of the call cannot be expressed as a request record and is answered (None,): %s", i, why)
        elif pod_groups is not None:                       # requests digested from config texts: InitialNodeFilter in the kernel
            for i in range(n_pods):
                reqs[i]["flags"] |= pack.RF_INITIAL_FILTER
                reqs[i]["groups"] = self.packer.group_bits_known(pod_groups[i])
        places = None
        if sequential:
            self.packer.close_signatures()                 # every NIC state a commit can produce has a signature
            self.engine.set_dictionary(self.packer)
            node, maps, places, status = self.engine.schedule_batch(reqs, now, self.packer, cand=cand, apply=apply)
            if (status == pack.COMMIT_WOULD_RAISE).any():
                self.logger.warning("mode B: the reference's commit step would have failed for pod %d",
                                    int(np.flatnonzero(status == pack.COMMIT_WOULD_RAISE)[0]))
            index = (node - self.engine.global_base).tolist()
        else:
            score, _, maps = self.engine.find(reqs, now, cand=cand, want_bitmap=False, want_map=True)
            base = self.engine.global_base
            index = [winner_index(s) - base if s else -1 for s in score.tolist()]
        out: List[Tuple] = []
        self.last_placements = [None] * n_pods
        rows = pack.unpack_mappings(maps)                  # (gpu[4], cpu[5], nic_numa[4], nic_idx[4], valid) per pod as Python ints: one pass
        n_groups = reqs["n_groups"].tolist()
        names = self._names
        place_rows = pack.unpack_placements(places) if places is not None and self._attached is not None else None   # (Python ints, one C call)
        gpus_of = reqs["gpus"].tolist() if place_rows is not None else None
        for p in range(n_pods):
            i = index[p]
            if i < 0:
                out.append((None,))
                continue
            name = names[i]
            G = n_groups[p]
            if places is not None and self._attached is not None:
                nd = self._attached.get(name)
                if nd is not None and place_rows[p][55] == pack.COMMIT_WIDE:            # (status) the pod landed on a wide node
                    wp = getattr(self.engine, "last_wide_places", {}).get(p)
                    if wp is not None:
                        self.last_placements[p] = pack.expand_wide_placement(wp, G, int(nd.cores_per_proc), int(nd.cores_per_proc) * int(nd.sockets),
                                                                             gpus_of[p][:G])
                    if apply:                                  # its record is re-packed from the object before the next call, whether or not
                        self._mark(nd, "wide-batch")           # the caller applies the placement to it (no delta form on the general path)
                elif nd is not None:
                    self.last_placements[p] = pack.expand_placement(place_rows[p], G, int(nd.cores_per_proc), int(nd.cores_per_proc) * int(nd.sockets),
                                                                    gpus_of[p][:G])
                    if apply:                                  # the reference mutators that follow find their work mirrored already
                        self._batch_ids.setdefault(nd.name, []).append(self.last_placements[p])
            gpu, cpu, nic_numa, nic_idx, valid = rows[p]
            if not valid:
                raise RuntimeError(f"internal error: no mapping produced for feasible node {name}")
            out.append((name, {"gpu": gpu[:G], "cpu": cpu[:G + 1],                                          # (tuples of plain ints, as the reference's hold)
                               "nic": list(zip(nic_numa[:G], nic_idx[:G]))}))
        return out

    # ---- pods with 5..8 processing groups (nhdfit_big_req): the general path ---------------------------------------------
    def _run_with_big(self, nl, big, small_reqs, big_reqs, now, cand, sequential, apply):
        """FindNodes / ScheduleBatch for a call that holds pods the table-driven pass cannot express: more than pack.MAX_GROUPS
        processing groups (the reference takes any group count, nhd/Matcher.py:118,203,242) or a hugepage request beyond the pod
        tile's table.  `big[p]` says which; `small_reqs` / `big_reqs` are the two kinds' records in pod order.  A big pod is a
        nhdfit_big_req answered on the device by the general path (nhdfit_big_find: every node by explicit enumeration, the same
        score word, the general CPython set model for its mapping; nhdfit_big_commit for its commit step); the other pods of the
        call take the table-driven pass as always.  Mode A: two device calls, results interleaved.  Mode B: the scheduler's loop
        (nhd/NHDScheduler.py:425-437) cut at the big pods - every run of ordinary pods between two of them is ONE device batch
        (nhdfit_schedule_batch, commits left in the mirror), every big pod is decided and committed on the device before the run
        behind it is matched."""
        n_pods = len(big)
        small_idx = [p for p in range(n_pods) if not big[p]]
        big_idx = [p for p in range(n_pods) if big[p]]
        n_groups = [0] * n_pods
        for k, p in enumerate(small_idx):
            n_groups[p] = int(small_reqs[k]["n_groups"])
        for k, p in enumerate(big_idx):
            n_groups[p] = int(big_reqs[k]["n_groups"])
        base = self.engine.global_base
        names = self._names
        out: List[Tuple] = [(None,)] * n_pods
        self.last_placements = [None] * n_pods

        def answer(p, i, row):
            G = n_groups[p]
            gpu, cpu, nic_numa, nic_idx, valid = row
            if not valid:
                raise RuntimeError(f"internal error: no mapping produced for feasible node {names[i]}")
            out[p] = (names[i], {"gpu": gpu[:G], "cpu": cpu[:G + 1], "nic": list(zip(nic_numa[:G], nic_idx[:G]))})

        if not sequential:
            if small_idx:
                score, _, maps = self.engine.find(small_reqs, now, cand=cand, want_bitmap=False, want_map=True)
                rows = pack.unpack_mappings(maps)
                for k, s in enumerate(score.tolist()):
                    if s:
                        answer(small_idx[k], winner_index(s) - base, rows[k])
            score, maps = self.engine.big_find(big_reqs, now, cand=cand)
            rows = pack.unpack_big_mappings(maps)
            for k, s in enumerate(score.tolist()):
                if s:
                    answer(big_idx[k], winner_index(s) - base, rows[k])
            return out

        self.packer.close_signatures()                     # every NIC state a commit can produce has a signature
        self.engine.set_dictionary(self.packer)
        objects = self._attached if self._attached is not None else nl
        touched = []
        pos_small = {p: k for k, p in enumerate(small_idx)}
        pos_big = {p: k for k, p in enumerate(big_idx)}

        def record(p, i, ids, on_wide):
            touched.append(names[i])
            nd = objects.get(names[i])
            if nd is None:
                return
            self.last_placements[p] = ids
            if self._attached is not None and apply:
                if on_wide:
                    self._mark(nd, "wide-batch")           # a wide record is re-packed from the object before the next call (no delta form)
                else:
                    self._batch_ids.setdefault(nd.name, []).append(ids)     # the reference mutators that follow find their work mirrored already

        p = 0
        while p < n_pods:
            if big[p]:
                req = big_reqs[pos_big[p]]
                score, maps = self.engine.big_find(big_reqs[pos_big[p]:pos_big[p] + 1], now, cand=cand)
                if score[0]:
                    i = winner_index(int(score[0])) - base
                    answer(p, i, pack.unpack_big_mappings(maps)[0])
                    ids = self._commit_big(i, objects.get(names[i]), req, maps[0], now)
                    record(p, i, ids, self._table is not None and bool(self._table.wide) and i in self._table.wide)
                p += 1
                continue
            # a run of ordinary pods between two big ones: one device batch (the decision engine), commits left in the mirror
            q = p
            while q < n_pods and not big[q]:
                q += 1
            ka, kb = pos_small[p], pos_small[p] + (q - p)
            node, maps, places, status = self.engine.schedule_batch(small_reqs[ka:kb], now, self.packer, cand=cand, apply=True)
            if (status == pack.COMMIT_WOULD_RAISE).any():
                self.logger.warning("mode B: the reference's commit step would have failed for pod %d",
                                    p + int(np.flatnonzero(status == pack.COMMIT_WOULD_RAISE)[0]))
            rows = pack.unpack_mappings(maps)
            wide_places = getattr(self.engine, "last_wide_places", {})
            for j in range(q - p):
                if node[j] < 0:
                    continue
                i = int(node[j]) - base
                answer(p + j, i, rows[j])
                nd = objects.get(names[i])
                on_wide = int(places[j]["status"]) == pack.COMMIT_WIDE
                ids = None
                if nd is not None:
                    G = n_groups[p + j]
                    gp = [int(small_reqs[ka + j]["gpus"][g]) for g in range(G)]
                    cpp, n_log = int(nd.cores_per_proc), int(nd.cores_per_proc) * int(nd.sockets)
                    if on_wide:
                        wp = wide_places.get(j)
                        ids = pack.expand_wide_placement(wp, G, cpp, n_log, gp) if wp is not None else None
                    else:
                        ids = pack.expand_placement(places[j], G, cpp, n_log, gp)
                record(p + j, i, ids, on_wide)
            p = q
        if not apply:
            # the mirror goes back to what the node objects say (nobody applied anything to them): attached - those nodes are
            # re-packed before the next call; stateless - every call packs `nl` again anyway
            if self._attached is not None:
                for name in touched:
                    nd = self._attached.get(name)
                    if nd is not None:
                        self._mark(nd, "unapplied-batch")
        return out
