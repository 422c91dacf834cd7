#!/usr/bin/env python3
"""Cost of nhdfit_headroom through ctypes (median / min ms of repeated calls behind a warm-up; one JSON line):

  * one GPU-less template of BASELINE config 2 (4 096 nodes) and one template of config 4 (65 536 nodes), whole cluster, sums only and
    with the per-node entries;
  * against the only route to the same total without the call: nhdfit_schedule_batch(apply=0) over replicas + 1 copies of the
    template, same mirror (`--route-only=R2,R4`: that leg alone, given the two totals - a copy of this file in a checkout of the parent
    commit, which has no nhdfit_headroom, gives the same-box comparison);
  * one template on a cluster with no room at all (every node in maintenance) against nhdfit_find for the same pod;
  * `--limits`: on each of the three shapes nhdfit_headroom_limits as well, histogram only and with the per-node entries and stages,
    and nhdfit_explain for the one pod beside it (the nearest existing price of one stage per node);
  * `--general`: nhdfit_headroom_general - on the shapes above (mirrors without wide records: the second launch is skipped) beside
    nhdfit_headroom, and on two mirrors with wide records against the only other route to their total, nhdfit_schedule_batch(apply=0)
    over replicas + 1 copies: an ENABLE_SHARING mirror of config 2 (4 096 nodes, every node a wide record) and config 4 at 65 536
    nodes with every hundredth node a wide one.  Both routes must report the same total (asserted).

`python tools/time_headroom.py` on the GPU box; kernel time from a separate
`rocprofv3 --kernel-trace --stats -- python tools/time_headroom.py --kernels` run (headroom calls only; with `--limits` the
limits calls too: k_limit_stage beside k_headroom; with `--general` the general calls: k_wide_room)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from nhd_amd import pack
from nhd_amd.engine import Engine
from workload import planes, refmodel, synth

ROUTE = [a for a in sys.argv[1:] if a.startswith("--route-only=")]       # --route-only=<replicas c2>,<replicas c4>: the totals a full run printed
ROUTE_ONLY, KERNELS, LIMITS, GENERAL = bool(ROUTE), "--kernels" in sys.argv, "--limits" in sys.argv, "--general" in sys.argv
TOTALS = dict(zip(("c2", "c4"), (int(x) for x in ROUTE[0].split("=")[1].split(",")))) if ROUTE else {}


def timed(fn, reps):
    fn(); fn()
    xs = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); xs.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(xs)), "ms_min": float(min(xs))}


def limits_legs(r, eng, req, now, reps):
    sums, _, hist, _ = eng.headroom_limits(req)
    r["limits"] = {s: int(k) for s, k in zip(("NOT_CANDIDATE", "MAINTENANCE", "HUGEPAGES", "BUSY", "GPU", "CPU", "NIC", "PCI", "NUMA", "FITS"), hist[0]) if k}
    r["limits_hist"] = timed(lambda: eng.headroom_limits(req), reps)
    r["limits_per_node"] = timed(lambda: eng.headroom_limits(req, per_node=True), reps)
    if not KERNELS:
        r["explain_one"] = timed(lambda: eng.explain(req, now + 1.0e6), reps)


def shape(cfg, n, want_gpu, full=False):
    spec = synth.make_cluster(cfg, n_nodes=n)
    if full:
        spec.maintenance[:] = True
    pods, _ = synth.make_pods(cfg, n_pods=64)
    s = next(s for s in pods if any(g["gpus"] for g in s["groups"]) == want_gpu and len(s["groups"]) == 2)
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    req = pk.digest_many([refmodel.make_topology(s)])
    pk.close_signatures()
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    return spec, pk, req, eng


out = {}
for key, cfg, n in (("c2", 2, 4096), ("c4", 4, 65536)):
    spec, pk, req, eng = shape(cfg, n, want_gpu=False)
    r = {"nodes": n}
    if not ROUTE_ONLY:
        sums, _ = eng.headroom(req)
        r.update(replicas=int(sums["replicas"][0]), nodes_with_room=int(sums["nodes_with_room"][0]), max_on_one_node=int(sums["max_on_one_node"][0]),
                 form=int(sums["form"][0]))
        r["headroom_sums"] = timed(lambda: eng.headroom(req), 30)
        r["headroom_per_node"] = timed(lambda: eng.headroom(req, per_node=True), 30)
        if LIMITS:
            limits_legs(r, eng, req, spec.clock_now, 30)
        if GENERAL:
            gsums, _ = eng.headroom_general(req)
            assert gsums.tobytes() == sums.tobytes()
            r["general_sums"] = timed(lambda: eng.headroom_general(req), 30)
    if not KERNELS:
        total = r["replicas"] if "replicas" in r else TOTALS[key]
        copies = np.repeat(req, total + 1)
        node = eng.schedule_batch(copies, spec.clock_now, pk, apply=False)[0]
        r["route_placed"] = int((node >= 0).sum())
        r["route_schedule_batch"] = timed(lambda: eng.schedule_batch(copies, spec.clock_now, pk, apply=False), 5)
    out[key] = r
    eng.close()
if not ROUTE_ONLY:
    spec, pk, req, eng = shape(4, 65536, want_gpu=False, full=True)
    sums, _ = eng.headroom(req)
    out["c4_no_room"] = {"nodes": 65536, "replicas": int(sums["replicas"][0]), "headroom_sums": timed(lambda: eng.headroom(req), 50)}
    if LIMITS:
        limits_legs(out["c4_no_room"], eng, req, spec.clock_now, 50)
    if not KERNELS:
        out["c4_no_room"]["find_one"] = timed(lambda: eng.find(req, spec.clock_now, want_bitmap=False, want_map=True), 50)
    eng.close()


def general_leg(eng, pk, req, now, reps):
    """nhdfit_headroom_general against schedule_batch(apply=0) over replicas + 1 copies on a mirror with wide records."""
    sums, counts = eng.headroom_general(req, per_node=True)
    total = int(sums["replicas"][0])
    assert int(sums["not_evaluated"][0]) == 0 and int(sums["saturated"][0]) == 0
    r = {"nodes": eng.n, "wide": eng.n_wide, "replicas": total, "nodes_with_room": int(sums["nodes_with_room"][0]),
         "max_on_one_node": int(sums["max_on_one_node"][0]), "form": int(sums["form"][0])}
    r["general_sums"] = timed(lambda: eng.headroom_general(req), reps)
    r["general_per_node"] = timed(lambda: eng.headroom_general(req, per_node=True), reps)
    r["plain_sums"] = timed(lambda: eng.headroom(req), reps)             # (the planes' launch alone: wide candidates flagged)
    if not KERNELS:
        copies = np.repeat(req, total + 1)
        node = eng.schedule_batch(copies, now, pk, apply=False)[0]
        r["route_placed"] = int((node >= 0).sum())
        assert r["route_placed"] == total, (r["route_placed"], total)
        assert np.array_equal(np.bincount(node[node >= 0] - eng.global_base, minlength=eng.n), counts[0] & pack.HEADROOM_COUNT_MASK)
        r["route_schedule_batch"] = timed(lambda: eng.schedule_batch(copies, now, pk, apply=False), 3)
    return r


if GENERAL and not ROUTE_ONLY:
    from nhd_amd.matcher import HipMatcher
    from oracle import nhd_oracle
    from tests import util
    # an ENABLE_SHARING mirror of config 2: every node a wide record with its share record
    spec = synth.make_cluster(2, n_nodes=4096)
    pods, _ = synth.make_pods(2, n_pods=64)
    s = next(s for s in pods if not any(g["gpus"] for g in s["groups"]) and len(s["groups"]) == 2)
    refmodel.ENABLE_SHARING = nhd_oracle.ENABLE_SHARING = True
    try:
        nl = spec.build_nodes()
        m = HipMatcher(device=0, clock=lambda: spec.clock_now)
        h = m.Headroom(nl, refmodel.make_topology(s), general=True)
        assert h.error is None and m.packer.sharing and len(m.wide_nodes) == len(nl)
        req = m.packer.digest_many([refmodel.make_topology(s)])
        out["c2_sharing"] = general_leg(m.engine, m.packer, req, spec.clock_now, 10)
        assert out["c2_sharing"]["replicas"] == h.replicas
        m.engine.close()
    finally:
        refmodel.ENABLE_SHARING = nhd_oracle.ENABLE_SHARING = False
    # config 4 at 65 536 nodes, every hundredth node one beyond the fast layout
    spec = synth.make_cluster(4, n_nodes=65536)
    pods, _ = synth.make_pods(4, n_pods=64)
    s = next(s for s in pods if not any(g["gpus"] for g in s["groups"]) and len(s["groups"]) == 2)
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    rng = np.random.default_rng(12)
    for i in range(50, 65536, 100):
        while True:
            d = util.random_wide_node_desc(rng, f"w{i:05d}", occupancy=0.1)
            node = refmodel.build_node(d)
            if node.sockets > 2 or node.cores_per_proc > 64:
                break
        pk.pack_node_into(node, table, i)
    assert len(table.wide) == 655 and not pk.unmirrored
    req = pk.digest_many([refmodel.make_topology(s)])
    pk.close_signatures()
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    out["c4_one_percent_wide"] = general_leg(eng, pk, req, spec.clock_now, 10)
    eng.close()
print(json.dumps(out))
