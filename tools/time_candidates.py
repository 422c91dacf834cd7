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
usage: time_candidates.py [cfg:nodes] [calls per round] [rounds]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

from nhd_amd import pack  # noqa: E402
from nhd_amd.engine import Engine, winner_index  # noqa: E402
from workload import planes, refmodel, synth  # noqa: E402

cfg, n = (int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "4:65536").split(":"))
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 7

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
