"""Soak at the EDGES of the record formats (`python tools/soak_extreme.py <seeds> [first seed] [--ref] [--device]`; `--ref` needs
the reference tree): clusters and pods drawn so that the limits of include/nhdfit.h are met often (workload/edge_inputs.py holds the
generators) - sockets of 1..64 physical cores next to wide ones of 65..128, up to 16 NICs and 8 GPUs per NUMA node, a dozen distinct
NIC speeds (the capacity classes), up to 14 PCIe switches, pods_used of 0..3, arbitrary isolcpus sets, busy times on either side of
the 30 s window, hugepage requests around the tile's table (1 022 GiB) - and pods of 1..6 processing groups with core counts that
often do not fit.  The product's host build (HipMatcher on tests/harness: the kernels' own arithmetic compiled for the host) or, with
--device, the HIP library on device 0, against the Python oracle - FindNodes, filtered FindNode, ScheduleBatch with commits and
physical ids, op streams mirrored as deltas, every fourth seed the same through a mirror of three shards (three contexts on
device 0 under --device) - and with --ref against the UNMODIFIED reference Matcher on every pod the reference answers in reasonable
time.  Short ranges of it run in the suite: tests/test_format_edges.py (host build), tests/test_format_edges_gpu.py (device)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nhd_amd.matcher import HipMatcher  # noqa: E402
from oracle import nhd_oracle as O  # noqa: E402
from tests import harness, sched_standin, util  # noqa: E402
from tests import delta_check as D  # noqa: E402
from workload.edge_inputs import NAMES, SPEEDS, edge_labels, edge_node, edge_pod, soak_draw, states_agree  # noqa: E402,F401
from tests.test_wide_core import norm  # noqa: E402
from workload import refmodel  # noqa: E402


def run(n_seeds, first=0, with_ref=False, device=False):
    """The soak over seeds first .. first + n_seeds - 1; returns its counters (`mismatches` among them).  device: the same checks
    through the C-ABI on GPU 0, the three shards as three contexts on that device."""
    EF = {} if device else {"engine_factory": harness.HarnessEngine}
    if device:
        from nhd_amd.engine import Engine
        SHARDS = {"devices": [0, 0, 0], "engine_factory": Engine}
    else:
        SHARDS = {"devices": [0, 1, 2], "engine_factory": harness.HarnessEngine}
    ref = None
    if with_ref:
        from oracle import ref_loader
        ref = ref_loader.load()
        ref_loader.VirtualClock(util.CLOCK).install()
    t0 = time.time()
    bad = pods = placed = refchecked = unmirrored = streams = sharded = 0
    for seed in range(first, first + n_seeds):
        # (NIC-heavy nodes meet pods of one or two groups, pods of five or six groups meet nodes of at most two NICs per NUMA node; seed
        # % 7 == 3: a few nodes beyond EVERY record - listed in HipMatcher.unmirrored, every other node is answered for as the oracle
        # answers without them: edge_inputs.soak_draw)
        rng, heavy_share, max_groups, descs, specs = soak_draw(seed)
        nl = util.build_cluster(descs)
        tops = [refmodel.make_topology(s) for s in specs]
        pgs = [list(rng.choice(NAMES, size=int(rng.integers(1, 4)), replace=False)) if rng.random() < 0.3 else None for _ in specs]
        m = HipMatcher(clock=lambda: util.CLOCK, **EF)
        m.attach(nl)
        unmirrored += len(m.unmirrored)
        live = {k: v for k, v in nl.items() if k not in m.unmirrored}      # (a node no record holds never matches: a documented deviation)
        got = m.FindNodes(nl, tops)
        for p, (s, top) in enumerate(zip(specs, tops)):
            want = O.find_node(live, top, util.CLOCK)
            pods += 1
            placed += want[0] is not None
            if norm(got[p]) != norm(want):
                bad += 1
                print("FIND product != oracle seed", seed, "pod", p, s, norm(got[p]), norm(want), flush=True)
            if ref is not None and len(s["groups"]) <= 3 and not heavy_share:
                nl_ref = util.build_cluster([d for d in descs if d["name"] in live], ref)
                rwant = ref_loader.find_node(nl_ref, refmodel.make_topology(s, ref))
                refchecked += 1
                if norm(rwant) != norm(want):
                    bad += 1
                    print("FIND oracle != REFERENCE seed", seed, "pod", p, s, norm(want), norm(rwant), flush=True)
        if seed % 4 == 1:                    # the same through a mirror sharded over three host-twin shards (engine.GroupEngine)
            ms = HipMatcher(clock=lambda: util.CLOCK, **SHARDS)
            ms.attach(util.build_cluster(descs))
            gs = ms.FindNodes(ms._attached, tops)
            if [norm(x) for x in gs] != [norm(x) for x in got]:
                bad += 1
                print("SHARDED FIND mismatch seed", seed, flush=True)
            sharded += 1
        # InitialNodeFilter in front (filtered dict handed to FindNode) for the pods that carry groups
        for p, (top, pg) in enumerate(zip(tops, pgs)):
            if pg is None:
                continue
            sub = O.initial_node_filter(nl, pg)
            g1 = m.FindNode(sub, top)
            want = O.find_node({k: v for k, v in sub.items() if k in live}, top, util.CLOCK)
            if norm(g1) != norm(want):
                bad += 1
                print("FILTERED FIND mismatch seed", seed, "pod", p, pg, norm(g1), norm(want), flush=True)
        # mode B on twin clusters: the product's batch against the oracle's sequential loop with commits
        nl_b, nl_o = util.build_cluster(descs), util.build_cluster(descs)
        for s in specs:
            if s["map_type"] not in ("NUMA", "PCI"):
                s["map_type"] = "NUMA"
        tops = [refmodel.make_topology(s) for s in specs]
        mb = HipMatcher(clock=lambda: util.CLOCK, **EF)
        mb.attach(nl_b)
        live_o = {k: v for k, v in nl_o.items() if k not in mb.unmirrored}
        try:
            res = mb.ScheduleBatch(nl_b, tops, now=util.CLOCK)
        except AssertionError as e:
            print("mode B assertion seed", seed, e, flush=True)
            bad += 1
            continue
        want, ids = [], []
        for top in tops:
            r = O.find_node(live_o, top, util.CLOCK)
            rec = {}
            if r[0] is not None:
                try:
                    O.commit(live_o[r[0]], top, r[1], util.CLOCK, rec)
                except O.CommitFailure:
                    break                                   # the reference's commit step would raise here: the batch is defined up to this pod
            want.append(r)
            ids.append(rec if r[0] is not None else None)
        k = len(want)
        if seed % 4 == 1:
            nl_s = util.build_cluster(descs)
            ms = HipMatcher(clock=lambda: util.CLOCK, **SHARDS)
            ms.attach(nl_s)
            rs = ms.ScheduleBatch(nl_s, tops, now=util.CLOCK)
            if [norm(x) for x in rs[:k]] != [norm(w) for w in want] or ms.last_placements[:k] != ids:
                bad += 1
                print("SHARDED MODE B mismatch seed", seed, flush=True)
        if [norm(x) for x in res[:k]] != [norm(w) for w in want]:
            bad += 1
            print("MODE B decisions mismatch seed", seed, [(norm(a), norm(b)) for a, b in zip(res[:k], want) if norm(a) != norm(b)][:2], flush=True)
        elif mb.last_placements[:k] != ids:
            bad += 1
            print("MODE B ids mismatch seed", seed, flush=True)
        # op streams on the edge cluster (attached mode): one ScheduleBatch(apply=True) for the pending list, the node objects brought
        # along by their own mutators, then releases / reclaims / resets / scalar writes mirrored as deltas - finds on the way
        # against the oracle on the objects' state, objects == device mirror at the end
        if seed % 2 == 0:
            clock = D.Clock(util.CLOCK)
            nodes = sched_standin.adopt(util.build_cluster(descs), clock)
            P = 12
            for s in specs:
                s["misc_smt"] = True                        # (the reference's own unwind path is broken)
            fresh_specs = [edge_pod(rng, min(3, max_groups)) for _ in range(D.N_FRESH)]
            for s in fresh_specs:
                s["misc_smt"] = True
            tops = [refmodel.make_topology(s) for s in specs[:P] + fresh_specs]
            grps = [["default"] + list(rng.choice(NAMES, size=2, replace=False)) for _ in tops]
            md = HipMatcher(clock=clock, **EF)
            md.attach(nodes)
            try:
                binds = sched_standin.check_pending_pods_batched(nodes, md, tops[:P], grps[:P], now=clock.t)
            except (IndexError, AssertionError, O.CommitFailure):   # a commit the reference itself would fail on (short of cores / of GPUs on the NIC's switch)
                binds = None
            if binds is not None:
                placed_b = [(i, b) for i, b in enumerate(binds) if b is not None]
                for k, op in enumerate(D.make_ops(seed, list(nodes), placed_b, 60, util.CLOCK)):
                    if op[0] == "find":
                        j = P + op[2]
                        sub = O.initial_node_filter(nodes, grps[j])
                        got1 = md.FindNode(sub, tops[j])
                        want1 = O.find_node({k2: v for k2, v in sub.items() if k2 not in md.unmirrored}, tops[j], clock.t)
                        if norm(got1) != norm(want1):
                            bad += 1
                            print("OP-STREAM find mismatch seed", seed, "op", k, norm(got1), norm(want1), flush=True)
                    else:
                        D.apply_op(nodes, tops, op)
                md.FindNode(nodes, tops[P])
                if not states_agree(nodes, md):
                    bad += 1
                    print("OP-STREAM objects != mirror seed", seed, flush=True)
                final = md.FindNodes(nodes, tops[P:])
                for j, g1 in enumerate(final):
                    w1 = O.find_node({k2: v for k2, v in nodes.items() if k2 not in md.unmirrored}, tops[P + j], clock.t)
                    if norm(g1) != norm(w1):
                        bad += 1
                        print("OP-STREAM final find mismatch seed", seed, "pod", j, norm(g1), norm(w1), flush=True)
                streams += 1
        if (seed - first) % 10 == 9:
            print("seed", seed, "pods", pods, "placed", placed, "ref-checked", refchecked, "unmirrored nodes", unmirrored, "op streams", streams, "sharded", sharded, "mismatches", bad,
                  "seconds", round(time.time() - t0, 1), flush=True)
    print("seeds", n_seeds, "from", first, "pods", pods, "placed", placed, "ref-checked", refchecked, "unmirrored nodes", unmirrored,
          "op streams", streams, "sharded", sharded, "mismatches", bad, "seconds", round(time.time() - t0, 1))
    return {"seeds": n_seeds, "first": first, "pods": pods, "placed": placed, "ref_checked": refchecked, "unmirrored": unmirrored,
            "op_streams": streams, "sharded": sharded, "mismatches": bad}


def main():
    n_seeds = int(sys.argv[1])
    first = int(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[2].isdigit() else 0
    return run(n_seeds, first, with_ref="--ref" in sys.argv, device="--device" in sys.argv)["mismatches"]


if __name__ == "__main__":
    sys.exit(1 if main() else 0)
