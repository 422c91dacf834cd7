"""oracle_stage / oracle_explain (oracle/nhd_oracle.c, coracle.Cluster.explain): the stage at which the reference drops each
node, restated in C over the flat per-core / GPU / NIC records, pinned here so that tests/test_explain_gpu.py can hold the
device to it at shapes no stored answer covers.

  - the reference's own stages (tests/explain_reference.py), stored with tests/test_explain_reference.py, on the same seeded
    inputs that module builds - and, where the reference tree is present, asked live as well;
  - FITS is exactly oracle_feasible's verdict at BASELINE shapes (c1, a c2 shard, a c3 shard);
  - stages 0..5 are the vectorised host computation of tests/explain_check.py on the same shapes;
  - the pinned inputs reach NIC, PCI and NUMA (and every other stage), so a swap of any two codes would fail here."""
import numpy as np
import pytest

from nhd_amd import pack
from oracle import coracle, ref_loader
from tests import explain_check, refanswers, util
from tests.explain_reference import FITS, NIC, NUMA, PCI, reference_stages
from tests.test_big_core import big_spec
from tests.test_big_vs_reference import few_nics
from workload import planes, refmodel, synth

STORE = explain_check.STORE


def stored(test):
    v = refanswers._load(STORE).get(test)
    assert v is not None, f"no stored reference stages for {test}"
    return [refanswers.decode(x) for x in v]


def random_clusters(seed):
    rng = np.random.default_rng(7300 + seed)
    descs = util.random_cluster_desc(7300 + seed, 24)
    specs = [util.random_pod_spec(rng, max_groups=4) for _ in range(24)]
    for s in specs[::3]:
        for g in s["groups"]:
            g["gpus"] = []
    return [(descs, specs)]


def every_stage():
    out = []
    for seed in range(3):
        rng = np.random.default_rng(7400 + seed)
        descs = util.random_cluster_desc(7400 + seed, 20, occupancy=0.5)
        specs = [util.random_pod_spec(rng, max_groups=4) for _ in range(20)]
        for s in specs:
            if s["map_type"] == "NONE":
                s["map_type"] = "PCI"
        out.append((descs, specs))
    return out


def big_pods(seed):
    rng = np.random.default_rng(7500 + seed)
    descs = few_nics(util.mixed_cluster_desc(7500 + seed, 12, wide_share=0.3 if seed else 0.0, occupancy=0.08), 3)
    return [(descs, [big_spec(rng, 5, 6 if seed else 7) for _ in range(6)])]


def wide_nodes(seed):
    rng = np.random.default_rng(7600 + seed)
    descs = few_nics(util.mixed_cluster_desc(7600 + seed, 16, wide_share=0.5), 4)
    return [(descs, [util.random_pod_spec(rng, max_groups=3) for _ in range(16)])]


# the seeded inputs of tests/test_explain_reference.py, by the id its stored answers carry (one answer per pod, in order)
SEEDED = {f"test_random_clusters[{s}]": (random_clusters, s) for s in range(4)}
SEEDED["test_every_stage_is_reached"] = (lambda _: every_stage(), None)
SEEDED.update({f"test_big_pods[{s}]": (big_pods, s) for s in range(2)})
SEEDED.update({f"test_wide_nodes[{s}]": (wide_nodes, s) for s in range(2)})
PLAIN_GOLDENS = [g for g, p in zip(explain_check.IDS, explain_check.GOLDENS) if not explain_check.load(p)[3]]


def oracle_stages(nl, tops, now, groups=None):
    cl = coracle.Cluster.from_nodes(nl)
    counts, st = cl.explain(cl.pods_from_tops(tops, groups), now, per_node=True, threads=4)
    assert np.array_equal(counts, np.stack([(st == k).sum(1) for k in range(coracle.STAGES)], 1))
    return st


@pytest.mark.parametrize("test", list(SEEDED))
def test_seeded_inputs_equal_the_stored_reference_stages(test):
    make, seed = SEEDED[test]
    want = stored(test)
    got, k, seen = [], 0, set()
    for descs, specs in make(seed):
        st = oracle_stages(util.build_cluster(descs), [refmodel.make_topology(s) for s in specs], util.CLOCK)
        for s, row in zip(specs, st.tolist()):
            assert row == want[k], (test, k, s, row, want[k])
            seen.update(row)
            k += 1
        got.append(st)
    assert k == len(want)
    if ref_loader.available():                       # the reference itself, live
        ref = ref_loader.load()
        ref_loader.VirtualClock(util.CLOCK).install()
        for (descs, specs), st in zip(make(seed), got):
            nl_ref = util.build_cluster(descs, ref)
            for s, row in zip(specs, st.tolist()):
                live = reference_stages(ref, nl_ref, refmodel.make_topology(s, ref))
                assert row == [live[n] for n in nl_ref], (test, s)
    if test == "test_every_stage_is_reached":
        assert seen >= set(range(1, 10)), sorted(seen)


@pytest.mark.parametrize("golden", PLAIN_GOLDENS)
def test_goldens_equal_the_stored_reference_stages(golden):
    """The reference-generated fixtures without ENABLE_SHARING (InitialNodeFilter where the fixture names node groups)."""
    path = explain_check.GOLDENS[explain_check.IDS.index(golden)]
    case, specs, groups, _ = explain_check.load(path)
    st = oracle_stages(util.build_cluster(case["nodes"]), [refmodel.make_topology(s) for s in specs], case["clock"], groups)
    assert st.tolist() == explain_check.stored(golden)
    if ref_loader.available() and not golden.startswith("big/"):   # (the big fixtures take minutes in the reference; their
        assert st.tolist() == explain_check.reference(path, ref_loader.load())   # stored stages are held to it live by test_explain_reference)


def test_the_pinned_inputs_reach_nic_pci_and_numa():
    """Teeth: the stored stages the oracle is held to above contain every one of NIC, PCI and NUMA (and FITS) many times over,
    in ordinary, wide and big-pod inputs alike - a swap of any two of those codes in the oracle cannot pass this module."""
    seen = np.zeros(coracle.STAGES, np.int64)
    for test in SEEDED:
        for row in stored(test):
            seen += np.bincount(row, minlength=coracle.STAGES)
    for g in PLAIN_GOLDENS:
        for row in explain_check.stored(g):
            seen += np.bincount(row, minlength=coracle.STAGES)
    for k in (NIC, PCI, NUMA, FITS):
        assert seen[k] >= 10, (k, seen.tolist())
    assert (seen[1:] > 0).all(), seen.tolist()
    wide_big = np.zeros(coracle.STAGES, np.int64)
    for test in ("test_big_pods[0]", "test_big_pods[1]", "test_wide_nodes[0]", "test_wide_nodes[1]"):
        for row in stored(test):
            wide_big += np.bincount(row, minlength=coracle.STAGES)
    assert (wide_big[[NIC, NUMA, FITS]] > 0).all(), wide_big.tolist()


def baseline(cfg, n, P, seed=None):
    spec = synth.make_cluster(cfg, n_nodes=n, seed=seed)
    specs, groups = synth.make_pods(cfg, n_pods=P, seed=seed)
    tops = [refmodel.make_topology(s) for s in specs]
    cl = coracle.Cluster.from_spec(spec)
    return spec, tops, groups, cl, cl.pods_from_tops(tops, groups)


@pytest.mark.parametrize("cfg,n,P", [(1, 32, 1), (2, 1024, 96), (3, 2048, 128), (4, 1500, 120)],
                         ids=["c1", "c2-shard", "c3-shard", "c4-shard"])
def test_fits_and_the_early_stages_at_baseline_shapes(cfg, n, P):
    """FITS is oracle_feasible's verdict on every pair; stages 0..5 are explain_check.host_stages_upto_cpu's (computed from the
    packed planes, a path that shares nothing with the C records); the later stages are exactly what is left over."""
    spec, tops, groups, cl, pods = baseline(cfg, n, P)
    now = spec.clock_now
    threads = coracle.usable_cpus()
    counts, st = cl.explain(pods, now, per_node=True, threads=threads)
    _, feas = cl.find(pods, now, threads=threads)
    assert np.array_equal(st == FITS, feas.astype(bool))
    pk = pack.Packer()
    table = planes.planes_from_spec(pk, spec)
    host = explain_check.host_stages_upto_cpu(table, pk.digest_many(tops, groups), now)
    assert np.array_equal(np.minimum(st, 6), host)
    assert np.array_equal(counts, np.stack([(st == k).sum(1) for k in range(coracle.STAGES)], 1))
    assert (counts.sum(1) == n).all()
    c2, none = cl.explain(pods, now, threads=threads)
    assert none is None and np.array_equal(c2, counts)
    if cfg >= 3:
        assert counts[:, FITS].sum() > 0 and counts[:, NIC].sum() + counts[:, NUMA].sum() + counts[:, PCI].sum() > 0


def test_candidate_mask_and_subset():
    """Nodes outside `cand` are NOT_CANDIDATE and the rest keep their stage; Cluster.subset is the masked view in order."""
    spec, tops, groups, cl, pods = baseline(3, 777, 40)
    now = spec.clock_now
    _, full = cl.explain(pods, now, per_node=True, threads=4)
    keep = np.random.default_rng(5).random(cl.n) < 0.6
    counts, st = cl.explain(pods, now, cand=keep, per_node=True, threads=4)
    assert (st[:, ~keep] == 0).all() and np.array_equal(st[:, keep], full[:, keep])
    assert (counts[:, 0] == (~keep).sum() + (full[:, keep] == 0).sum(1)).all()
    sub = cl.subset(keep)
    _, sst = sub.explain(sub.pods_from_tops(tops, groups), now, per_node=True, threads=4)
    assert np.array_equal(sst, full[:, keep])


@pytest.mark.parametrize("shape", ["c4-shard", "random", "wide"])
def test_host_build_of_the_explain_stages_equals_the_oracle(shape):
    """nhdfit_explain's stage function on its host build (tests/harness/explain_twin: explain_core.h compiled for the CPU) equals
    the oracle on every (pod, node) pair, at shapes beyond the stored answers - what tests/test_explain_gpu.py asks of the device."""
    from nhd_amd.matcher import HipMatcher
    from tests.harness.explain_twin import ExplainHarnessEngine
    if shape == "c4-shard":
        spec, tops, groups, cl, pods = baseline(4, 1500, 120)
        nl, now = spec.build_nodes(), spec.clock_now
    else:
        nl = util.random_cluster(8800, 600, occupancy=0.5) if shape == "random" else util.mixed_cluster(8801, 500, wide_share=0.4)
        rng = np.random.default_rng(8800)
        tops, groups, now = [refmodel.make_topology(util.random_pod_spec(rng, max_groups=4)) for _ in range(80)], None, util.CLOCK
    m = HipMatcher(clock=lambda: now, engine_factory=ExplainHarnessEngine)
    got = np.stack([e.stages for e in m.ExplainNodes(nl, tops, pod_groups=groups, per_node=True)])
    want = oracle_stages(nl, tops, now, groups)
    assert np.array_equal(got, want), np.argwhere(got != want)[:10].tolist()
    seen = np.bincount(want.reshape(-1), minlength=coracle.STAGES)
    assert (seen[[NIC, NUMA, FITS]] > 0).all() and (shape != "c4-shard" or seen[PCI] > 0), seen.tolist()
