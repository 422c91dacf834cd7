"""Shared by the CPU and GPU tests of headroom limits: tests/headroom_check.py's inputs (the five synth configurations at 48 nodes x 8
templates, every pod of the fixtures tests/golden/*.json with and without node groups) with the reference's (count, stopped, stage)
of every pair (tests/headroom_limit_reference.py), stored with the CPU test module's answers
(tests/golden/refanswers/tests.test_headroom_limit_reference.json) so the GPU box holds the device to them, and the same on the
independent oracle for inputs of any size.

A stored case is [entries [template][node] as tests/headroom_check.py encodes them, one string per template: a stage digit per node
('x': no stage - the run stopped)]."""
import multiprocessing

import numpy as np

from nhd_amd import pack
from oracle import nhd_oracle as O
from tests import headroom_check as hc
from tests import refanswers, util
from tests.headroom_limit_reference import NONE, independent_limit, reference_limit
from workload import refmodel, synth

STORE = "tests.test_headroom_limit_reference"
CAP = 37                                             # max_per_node of the stored cases
NOT_CANDIDATE, MAINTENANCE, HUGEPAGES, BUSY, GPU, CPU, NIC, PCI, NUMA, FITS = range(10)


def digits(row):
    return "".join("x" if s == NONE else str(int(s)) for s in row)


def undigits(text):
    return [NONE if ch == "x" else int(ch) for ch in text]


def _case(triples):
    """[[(k, stopped, stage)]] -> the stored form."""
    return [[[hc.entry(k, stopped) for k, stopped, _ in row] for row in triples], [digits([st for _, _, st in row]) for row in triples]]


def reference_synth(ref, cfg, cap=CAP):
    from oracle import ref_loader
    spec, specs, _ = hc.synth_case(cfg)
    ref_loader.VirtualClock(spec.clock_now).install()
    return _case([[reference_limit(ref, lambda: spec.build_node(i, ref), lambda: refmodel.make_topology(s, ref), cap) for i in range(spec.n)]
                  for s in specs])


def reference_golden(ref, path, with_groups, cap=CAP):
    """With the fixture's node groups, a node InitialNodeFilter drops for the pod is (0, False, NOT_CANDIDATE): FindNode never sees it."""
    from oracle import ref_loader
    case, specs, groups = hc.load_golden(path)
    ref_loader.VirtualClock(case["clock"]).install()
    descs = case["nodes"]
    plain = util.build_cluster(descs)
    out = []
    for p, s in enumerate(specs):
        keep = set(O.initial_node_filter(plain, groups[p])) if with_groups else set(plain)
        out.append([reference_limit(ref, lambda: refmodel.build_node(d, ref), lambda: refmodel.make_topology(s, ref), cap)
                    if d["name"] in keep else (0, False, NOT_CANDIDATE) for d in descs])
    return _case(out)


def answers_of(results):
    """HipMatcher.HeadroomMany(limits=True, per_node=True) results in the stored form."""
    return [hc.entries_of(results), [digits(h.limit_stages.tolist()) for h in results]]


def matcher_synth(matcher_factory, cfg, cap=CAP):
    spec, specs, _ = hc.synth_case(cfg)
    m = matcher_factory(spec.clock_now)
    got = m.HeadroomMany(spec.build_nodes(), [refmodel.make_topology(s) for s in specs], per_node=True, max_per_node=cap, limits=True)
    return got, answers_of(got)


def matcher_golden(matcher_factory, path, with_groups, cap=CAP):
    case, specs, groups = hc.load_golden(path)
    m = matcher_factory(case["clock"])
    got = m.HeadroomMany(util.build_cluster(case["nodes"]), [refmodel.make_topology(s) for s in specs], pod_groups=groups if with_groups else None,
                         per_node=True, max_per_node=cap, limits=True)
    return got, answers_of(got)


def stored(test_id):
    v = refanswers._load(STORE).get(test_id)
    assert v is not None, f"no stored reference answers for {test_id}"
    return refanswers.decode(v[0])


def same_where_not_stopped(got, want):
    """Count and stopped flag of every pair, the stage of every pair that is not stopped (there the reference has none)."""
    assert got[0] == want[0]
    for p, (a, b) in enumerate(zip(got[1], want[1])):
        e = np.asarray(want[0][p])
        live = (e & pack.HEADROOM_STOPPED) == 0
        a, b = np.asarray(undigits(a)), np.asarray(undigits(b))
        assert np.array_equal(a[live], b[live]), (p, np.flatnonzero(live & (a != b))[:10].tolist())
        assert (a[~live] == NONE).all(), p


def check_identities(results, n):
    """Per template: the histogram is the histogram of the stages, with the stopped and not evaluated nodes it sums to the node
    count, BUSY never occurs, FITS only where the count reached the cap (a node may also run out exactly there: test_saturation)."""
    for h in results:
        st = h.limit_stages
        assert h.limits == {s: int((st == k).sum()) for k, s in enumerate(STAGE_NAMES)}
        assert sum(h.limits.values()) + h.stopped + h.not_evaluated + h.unmirrored == n == h.nodes
        assert h.limits["BUSY"] == 0
        flagged = h.flags != 0
        assert (st[flagged] == NONE).all() and int((st[~flagged] >= len(STAGE_NAMES)).sum()) == h.unmirrored      # (UNMIRRORED: no flag, no stage)
        assert (h.per_node[st == FITS] == h.max_per_node).all() and not flagged[st == FITS].any()


STAGE_NAMES = ("NOT_CANDIDATE", "MAINTENANCE", "HUGEPAGES", "BUSY", "GPU", "CPU", "NIC", "PCI", "NUMA", "FITS")


# ---- the independent oracle on inputs of any size, spread over the usable cores by node ranges ----------------------------------------
def _oracle_range(args):
    cfg, n, seed_specs, lo, hi, cap, todo = args
    spec = synth.make_cluster(cfg, n_nodes=n)
    k = np.zeros((len(seed_specs), hi - lo), np.int64)
    st = np.full((len(seed_specs), hi - lo), NONE, np.uint8)
    for i in range(lo, hi):
        if not todo[:, i - lo].any():
            continue
        desc = spec.describe(i)
        for p, s in enumerate(seed_specs):
            if todo[p, i - lo]:
                a, stopped, stage = independent_limit(lambda: refmodel.build_node(desc), lambda: refmodel.make_topology(s), cap, now=spec.clock_now + 1.0e6)
                k[p, i - lo], st[p, i - lo] = hc.entry(a, stopped), stage
    return lo, k, st


def oracle_synth(cfg, n, specs, todo, cap=CAP, procs=None):
    """(entries, stages) [template][node] of independent_limit for the pairs of `todo` [template][node] bool among the first `n` nodes
    of a synth configuration (elsewhere 0 / NONE); fresh processes (spawn: the caller may hold a GPU) share the nodes out by ranges."""
    from oracle import coracle
    procs = max(1, min(16, coracle.usable_cpus())) if procs is None else procs
    step = max(64, (n + procs * 8 - 1) // (procs * 8))
    jobs = [(cfg, n, specs, lo, min(n, lo + step), cap, np.ascontiguousarray(todo[:, lo:min(n, lo + step)])) for lo in range(0, n, step)]
    k = np.zeros((len(specs), n), np.int64)
    st = np.full((len(specs), n), NONE, np.uint8)
    if procs == 1 or len(jobs) == 1:
        parts = [_oracle_range(j) for j in jobs]
    else:
        with multiprocessing.get_context("spawn").Pool(procs) as pool:
            parts = pool.map(_oracle_range, jobs, chunksize=1)
    for lo, a, b in parts:
        k[:, lo:lo + a.shape[1]] = a
        st[:, lo:lo + a.shape[1]] = b
    return k, st
