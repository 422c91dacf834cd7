#!/usr/bin/env python3
"""Cost of nhdfit_candidates against the calls it replaces, through ctypes on one GPU: config 4 at 65 536 nodes, one pod.

Timed forms (each call ends in a stream wait inside the library, the host clock is around the call):
  candidates K=1 / K=8 / K=64   nhdfit_candidates for one pod
  find                          nhdfit_find of the same pod (the single-launch form)
  composed K=8                  K successive nhdfit_find calls, the earlier winners cleared from the candidate mask - existing code: the baseline
  candidates 64 pods K=8        one call for 64 pods
Protocol: every form is warmed up, then ROUNDS rounds; a round times every form CALLS times, the forms alternating call by call;
per round and form the median; reported: the median of the rounds' medians and their spread (min .. max).  The lists of the new
call and of the composed form are compared before anything is timed.

`--general`: nhdfit_candidates_general on two mirrors with wide records (tools/time_headroom.py --general's): an ENABLE_SHARING mirror
of config 2 (4 096 nodes, every node a wide record) and config 4 at 65 536 nodes with every hundredth node a wide one.  Per mirror, one
pod at K = 1, 8, 64 and 64 pods at K = 8, each against the composed form at the C-ABI on the same mirror - K successive nhdfit_find
calls with a shrinking mask, per pod - same protocol, the lists compared first.  `--kernels`: the general calls alone, for a separate
`rocprofv3 --kernel-trace --stats -- python tools/time_candidates.py --general --kernels` run (k_wide_cand_scan, k_wide_cand_map).

`--big`: nhdfit_candidates_big for pods of 5..8 groups (seeded tests/test_big_core.big_spec pods) on config 4 at 65 536 nodes and on
the 4 096-node ENABLE_SHARING mirror of config 2.  Per mirror, one pod and 64 pods at K = 1, 8, 64, each against the composed form at
the C-ABI on the same mirror - K successive nhdfit_big_find calls with a shrinking mask, per pod - and one pod's nhdfit_big_find; same
protocol, the lists compared first.  `--kernels`: the new calls alone, for a separate `rocprofv3 --kernel-trace --stats` run
(k_big_cand_scan, k_big_cand_pick, k_big_cand_map).
usage: time_candidates.py [cfg:nodes] [calls per round] [rounds] [--general [--kernels] | --big [--kernels]]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from nhd_amd import pack  # noqa: E402
from nhd_amd.engine import Engine, winner_index  # noqa: E402
from workload import planes, refmodel, synth  # noqa: E402

GENERAL, KERNELS, BIG = "--general" in sys.argv, "--kernels" in sys.argv, "--big" in sys.argv
argv = [a for a in sys.argv if not a.startswith("--")]
cfg, n = (int(x) for x in (argv[1] if len(argv) > 1 else "4:65536").split(":"))
calls = int(argv[2]) if len(argv) > 2 else 50
rounds = int(argv[3]) if len(argv) > 3 else 7


def measure(forms):
    """{form: [median us of each round]}: warm-up, then `rounds` rounds of `calls` calls, the forms alternating call by call."""
    for fn in forms.values():
        for _ in range(3):
            fn()
    if BIG:                                                    # (calls of milliseconds to seconds: say how far the run is)
        print(f"warmed up {len(forms)} forms", file=sys.stderr, flush=True)
    medians = {name: [] for name in forms}
    for r in range(rounds):
        if BIG:
            print(f"round {r + 1} of {rounds}", file=sys.stderr, flush=True)
        ts = {name: [] for name in forms}
        for _ in range(calls):
            for name, fn in forms.items():
                t0 = time.perf_counter()
                fn()
                ts[name].append(time.perf_counter() - t0)
        for name in forms:
            medians[name].append(sorted(ts[name])[calls // 2] * 1e6)
    return medians


def spread(m):
    m = sorted(m)
    return {"us_median": round(m[len(m) // 2], 1), "us_min": round(m[0], 1), "us_max": round(m[-1], 1)}


def general_leg(eng, reqs, now):
    """One mirror with wide records: the new entry against K successive finds per pod, lists compared first."""
    chunks = (eng.n + 63) // 64
    full = np.full(chunks, np.uint64(0xFFFFFFFFFFFFFFFF))

    def composed(pods, k):
        out = []
        for p in range(len(pods)):
            mask, row = full.copy(), []
            for _ in range(k):
                score, _, maps = eng.find(pods[p:p + 1], now, cand=mask, want_bitmap=False, want_map=True)
                if not score[0]:
                    break
                i = winner_index(score[0]) - eng.global_base
                mask[i >> 6] &= ~(np.uint64(1) << np.uint64(i & 63))
                row.append((int(score[0]), maps[0].tobytes()))
            out.append(row)
        return out

    one = reqs[:1]
    sums, entries = eng.candidates(reqs, now, 8, cand=full, general=True)
    got = [[(int(e["score"]), e["map"].tobytes()) for e in entries[p][:int(sums[p]["returned"])]] for p in range(len(reqs))]
    same = got == composed(reqs, 8)
    assert same, "nhdfit_candidates_general and the composed form disagree"
    assert (sums["not_evaluated"] == 0).all() and (sums["form"] & pack.CANDIDATES_FORM_WIDE).all()
    rec = {"nodes": eng.n, "wide": eng.n_wide, "pods": len(reqs), "feasible_first_pod": int(sums[0]["feasible"]),
           "listed_64pods_K8": int(sums["returned"].sum()), "lists_equal": bool(same)}
    forms = {f"general_K{k}": (lambda k=k: eng.candidates(one, now, k, cand=full, general=True)) for k in (1, 8, 64)}
    forms["general_64pods_K8"] = lambda: eng.candidates(reqs, now, 8, cand=full, general=True)
    if not KERNELS:
        forms.update({f"composed_K{k}": (lambda k=k: composed(one, k)) for k in (1, 8, 64)})
        forms["composed_64pods_K8"] = lambda: composed(reqs, 8)
    for name, m in measure(forms).items():
        rec[name] = spread(m)
    if not KERNELS:
        for case in ("K1", "K8", "K64", "64pods_K8"):
            new, base = rec["general_" + case], rec["composed_" + case]
            rec[case + "_faster_beyond_spread"] = bool(new["us_max"] < base["us_min"])
            rec[case + "_speedup"] = round(base["us_median"] / new["us_median"], 2)
    return rec


def big_leg(eng, reqs, now):
    """One mirror: nhdfit_candidates_big against K successive nhdfit_big_find calls per pod, lists compared first."""
    chunks = (eng.n + 63) // 64
    full = np.full(chunks, np.uint64(0xFFFFFFFFFFFFFFFF))

    def composed(pods, k):
        out = []
        for p in range(len(pods)):
            mask, row = full.copy(), []
            for _ in range(k):
                score, maps = eng.big_find(pods[p:p + 1], now, cand=mask)
                if not score[0]:
                    break
                i = winner_index(score[0]) - eng.global_base
                mask[i >> 6] &= ~(np.uint64(1) << np.uint64(i & 63))
                row.append((int(score[0]), maps[0].tobytes()))
            out.append(row)
        return out

    sums, entries = eng.candidates_big(reqs, now, 8, cand=full)
    first = next(p for p in range(len(reqs)) if sums[p]["feasible"] >= 64)      # the one-pod forms' pod: a list of 64 exists
    one = reqs[first:first + 1]
    got = [[(int(e["score"]), e["map"].tobytes()) for e in entries[p][:int(sums[p]["returned"])]] for p in range(len(reqs))]
    same = got == composed(reqs, 8)
    assert same, "nhdfit_candidates_big and the composed form disagree"
    print(f"{eng.n} nodes: lists compared", file=sys.stderr, flush=True)
    assert (sums["not_evaluated"] == 0).all() and (sums["form"] == pack.CANDIDATES_FORM_BIG).all()
    rec = {"nodes": eng.n, "wide": eng.n_wide, "pods": len(reqs), "one_pod": first, "one_pod_groups": int(one[0]["n_groups"]),
           "feasible_one_pod": int(sums[first]["feasible"]), "feasible_64pods": sums["feasible"].tolist(), "listed_64pods_K8": int(sums["returned"].sum()), "lists_equal": bool(same)}
    forms = {f"big_K{k}": (lambda k=k: eng.candidates_big(one, now, k, cand=full)) for k in (1, 8, 64)}
    forms.update({f"big_64pods_K{k}": (lambda k=k: eng.candidates_big(reqs, now, k, cand=full)) for k in (1, 8, 64)})
    if not KERNELS:
        forms["big_find"] = lambda: eng.big_find(one, now, cand=full)
        forms.update({f"composed_K{k}": (lambda k=k: composed(one, k)) for k in (1, 8, 64)})
        forms.update({f"composed_64pods_K{k}": (lambda k=k: composed(reqs, k)) for k in (1, 8, 64)})
    for name, m in measure(forms).items():
        rec[name] = spread(m)
    if not KERNELS:
        for case in ("K1", "K8", "K64", "64pods_K1", "64pods_K8", "64pods_K64"):
            new, base = rec["big_" + case], rec["composed_" + case]
            rec[case + "_faster_beyond_spread"] = bool(new["us_max"] < base["us_min"])
            rec[case + "_speedup"] = round(base["us_median"] / new["us_median"], 2)
    return rec


if BIG:
    from nhd_amd.matcher import HipMatcher
    from oracle import nhd_oracle
    from tests.test_big_core import big_spec
    out = {"calls_per_round": calls, "rounds": rounds}
    rng = np.random.default_rng(18)
    specs = [big_spec(rng) for _ in range(64)]
    # config 4 at 65 536 nodes
    spec = synth.make_cluster(4, n_nodes=65536)
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    reqs = np.array([pk.digest_big(refmodel.make_topology(s)) for s in specs], dtype=pack.BIG_REQ)
    pk.close_signatures()
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    out["c4_65536"] = big_leg(eng, reqs, spec.clock_now)
    eng.close()
    # an ENABLE_SHARING mirror of config 2: every node a wide record with its share record
    spec = synth.make_cluster(2, n_nodes=4096)
    refmodel.ENABLE_SHARING = nhd_oracle.ENABLE_SHARING = True
    try:
        nl = spec.build_nodes()
        m = HipMatcher(device=0, clock=lambda: spec.clock_now)
        tops = [refmodel.make_topology(s) for s in specs]
        c = m.Candidates(nl, tops[0], k=8, big=True)
        assert c.error is None and m.packer.sharing and len(m.wide_nodes) == len(nl)
        reqs = np.array([m.packer.digest_big(t) for t in tops], dtype=pack.BIG_REQ)
        out["c2_sharing"] = big_leg(m.engine, reqs, spec.clock_now)
        m.engine.close()
    finally:
        refmodel.ENABLE_SHARING = nhd_oracle.ENABLE_SHARING = False
    print(json.dumps(out))
    sys.exit(0)

if GENERAL:
    from nhd_amd.matcher import HipMatcher
    from oracle import nhd_oracle
    from tests import util
    out = {"calls_per_round": calls, "rounds": rounds}
    # an ENABLE_SHARING mirror of config 2: every node a wide record with its share record
    spec = synth.make_cluster(2, n_nodes=4096)
    pods, _ = synth.make_pods(2, n_pods=256)
    refmodel.ENABLE_SHARING = nhd_oracle.ENABLE_SHARING = True
    try:
        nl = spec.build_nodes()
        m = HipMatcher(device=0, clock=lambda: spec.clock_now)
        tops = [refmodel.make_topology(s) for s in pods if len(s["groups"]) <= 4][:64]
        c = m.Candidates(nl, tops[0], k=8, general=True)
        assert c.error is None and m.packer.sharing and len(m.wide_nodes) == len(nl)
        out["c2_sharing"] = general_leg(m.engine, m.packer.digest_many(tops), spec.clock_now)
        m.engine.close()
    finally:
        refmodel.ENABLE_SHARING = nhd_oracle.ENABLE_SHARING = False
    # config 4 at 65 536 nodes, every hundredth node one beyond the fast layout
    spec = synth.make_cluster(4, n_nodes=65536)
    pods, _ = synth.make_pods(4, n_pods=256)
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    rng = np.random.default_rng(12)
    for i in range(50, 65536, 100):
        while True:
            node = refmodel.build_node(util.random_wide_node_desc(rng, f"w{i:05d}", occupancy=0.1))
            if node.sockets > 2 or node.cores_per_proc > 64:
                break
        pk.pack_node_into(node, table, i)
    assert len(table.wide) == 655 and not pk.unmirrored
    reqs = pk.digest_many([refmodel.make_topology(s) for s in pods])       # (no node groups: the wide nodes are candidates)
    reqs = reqs[reqs["n_groups"] <= 3][:64]
    pk.close_signatures()
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    out["c4_one_percent_wide"] = general_leg(eng, reqs, spec.clock_now)
    eng.close()
    print(json.dumps(out))
    sys.exit(0)

spec = synth.make_cluster(cfg, n_nodes=n)
pods, groups = synth.make_pods(cfg, n_pods=256)
pk = pack.Packer()
table = planes.planes_from_spec(pk, spec)
reqs = pk.digest_many([refmodel.make_topology(s) for s in pods], groups)
reqs = reqs[reqs["n_groups"] <= 3][:64]
eng = Engine(0)
eng.set_dictionary(pk)
eng.upload(table)
now = spec.clock_now
one = reqs[:1]
chunks = (n + 63) // 64
full = np.full(chunks, np.uint64(0xFFFFFFFFFFFFFFFF))


def composed(k):
    mask = full.copy()
    out = []
    for _ in range(k):
        score, _, maps = eng.find(one, now, cand=mask, want_bitmap=False, want_map=True)
        if not score[0]:
            break
        i = winner_index(score[0]) - eng.global_base
        mask[i >> 6] &= ~(np.uint64(1) << np.uint64(i & 63))
        out.append((int(score[0]), maps[0].tobytes()))
    return out


forms = {
    "candidates_K1": lambda: eng.candidates(one, now, 1, cand=full),
    "candidates_K8": lambda: eng.candidates(one, now, 8, cand=full),
    "candidates_K64": lambda: eng.candidates(one, now, 64, cand=full),
    "find": lambda: eng.find(one, now, cand=full, want_bitmap=False, want_map=True),
    "composed_K8": lambda: composed(8),
    "candidates_64pods_K8": lambda: eng.candidates(reqs, now, 8, cand=full),
}
sums, entries = eng.candidates(one, now, 8, cand=full)
same = [(int(e["score"]), e["map"].tobytes()) for e in entries[0][:int(sums[0]["returned"])]] == composed(8)
assert same, "nhdfit_candidates and the composed form disagree"
for fn in forms.values():
    for _ in range(5):
        fn()
medians = {name: [] for name in forms}
for _ in range(rounds):
    ts = {name: [] for name in forms}
    for _ in range(calls):
        for name, fn in forms.items():
            t0 = time.perf_counter()
            fn()
            ts[name].append(time.perf_counter() - t0)
    for name in forms:
        medians[name].append(sorted(ts[name])[calls // 2] * 1e6)
rec = {"config": cfg, "nodes": n, "calls_per_round": calls, "rounds": rounds, "feasible": int(sums[0]["feasible"]), "lists_equal": bool(same)}
for name, m in medians.items():
    m = sorted(m)
    rec[name] = {"us_median": round(m[len(m) // 2], 1), "us_min": round(m[0], 1), "us_max": round(m[-1], 1)}
new, base = rec["candidates_K8"], rec["composed_K8"]
rec["K8_faster_beyond_spread"] = bool(new["us_max"] < base["us_min"])
rec["K8_speedup"] = round(base["us_median"] / new["us_median"], 2)
eng.close()
print(json.dumps(rec))
