#!/usr/bin/env python3
"""Cost of nhdfit_explain (counts only) at BASELINE config 4 - 65 536 nodes, 4 096 pods and one pod - against nhdfit_find on the
same requests, through ctypes (median / min ms of repeated calls; one JSON line).  `python tools/time_explain.py` on the GPU box."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from nhd_amd import pack
from nhd_amd.engine import Engine
from workload import planes, refmodel, synth

spec = synth.make_cluster(4, n_nodes=65536)
pods, groups = synth.make_pods(4, n_pods=4096)
pk = pack.Packer()
table = planes.planes_from_spec(pk, spec)
reqs = pk.digest_many([refmodel.make_topology(s) for s in pods], groups)
eng = Engine(0)
eng.set_dictionary(pk)
eng.upload(table)
now = spec.clock_now


def timed(fn, reps):
    fn(); fn()
    xs = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); xs.append((time.perf_counter() - t0) * 1e3)
    return {"ms_median": float(np.median(xs)), "ms_min": float(min(xs))}


out = {"nodes": table.n, "pods": len(reqs),
       "find_batch": timed(lambda: eng.find(reqs, now, want_bitmap=False, want_map=True), 20),
       "explain_batch": timed(lambda: eng.explain(reqs, now), 5),
       "find_one": timed(lambda: eng.find(reqs[:1], now, want_bitmap=False, want_map=True), 50),
       "explain_one": timed(lambda: eng.explain(reqs[:1], now), 50)}
out["stage_totals_batch"] = eng.explain(reqs, now)[0].sum(0).tolist()
print(json.dumps(out))
