"""Shared by the CPU and GPU tests of the two branches of headroom on the general path that decide answers and that random clusters
do not reach (tests/test_wide_edges_reference.py, tests/test_wide_edges_core.py, tests/test_wide_edges_gpu.py):

  A  wide records whose run ends STOPPED - FindNode answers the node, SetPhysicalIdsFromMapping then fails on the placement
     (wide_room_run_wave's `status != kCommitOk` branch, wide_commit's kCommitWouldRaise arms) - with ENABLE_SHARING off and on, each
     beside a template that runs the same node to exhaustion;
  B  such records at wide slots 0, 63 and 64 of one mirror - the last bit of one 64-slot chunk, the first of the next - among records
     with room and a few ordinary nodes;
  C  shared NICs whose replica count is decided by the rounding of `speed * 0.9 - speed_used[x]`, speed_used accumulated in
     binary64 one commit after the other: big empty SMT sockets (cores never end the run), NICs of 25 / 40 / 100 / 200 Gb/s.

The pairs of A were found once by running the independent oracle's loop (tests/headroom_reference.independent_headroom) over
edge_draw(seed) for seeds 0..19 999 per mode (0..49 999 with sharing off for the runs with replicas in front of the flag); the
triples of C (d) by the same loop over the values of BW_VALUES.  profiles/r14/README.md has the yields.  Only the seeds are kept:
everything is regenerated from tests/util.py's generators, and every property the sets are meant to have is asserted from the
reference's answers in tests/test_wide_edges_reference.py, which also stores them
(tests/golden/refanswers/tests.test_wide_edges_reference.json) for the GPU box."""
import functools
from fractions import Fraction

import numpy as np

from nhd_amd import pack
from tests import headroom_general_check as gc
from oracle import nhd_oracle as O
from tests import refanswers, util
from tests.headroom_reference import LONG_AGO
from workload import refmodel
from workload.refmodel import NFD

STORE = "tests.test_wide_edges_reference"
COUNT, STOPPED = pack.HEADROOM_COUNT_MASK, pack.HEADROOM_STOPPED
POOL = gc.FOUR + [gc.GPULESS]                                  # neighbour templates beyond a draw's own four


# ---- A: STOPPED runs ----------------------------------------------------------------------------------------------------------------
def edge_draw(seed):
    """(node description, four templates) of one seed of the search: a node of the wide generator at an occupancy drawn from
    {0, 0.05, 0.1, 0.3}, active and without the maintenance label, and four templates of up to four groups."""
    rng = np.random.default_rng(200000 + seed)
    occupancy = float(rng.choice([0.0, 0.05, 0.1, 0.3]))
    d = util.random_wide_node_desc(rng, f"e{seed:05d}", occupancy)
    d["active"] = True
    d["labels"].pop(refmodel.MAINT_LABEL, None)
    return d, [util.random_pod_spec(rng, max_groups=4) for _ in range(4)]


# (seed, which of the draw's four templates ends the node's run STOPPED, the neighbour template that runs the same node to exhaustion:
#  0..3 the draw's own, 4.. POOL[n - 4])
STOPPED_PAIRS = {
    False: [(3909, 3, 0), (14397, 2, 1), (27792, 0, 1), (35624, 1, 2), (353, 3, 2), (6899, 2, 1), (261, 2, 1), (650, 0, 1), (804, 1, 0),
            (4180, 0, 1), (5346, 0, 1), (9230, 1, 2), (12308, 2, 4)],
    True: [(3909, 3, 0), (8423, 2, 1), (10660, 2, 0), (11022, 3, 0), (14070, 3, 0), (14397, 2, 1), (17027, 0, 1), (353, 3, 2), (610, 2, 1),
           (1784, 0, 2), (6107, 0, 1), (6620, 2, 4), (6899, 2, 1)],
}


def neighbour_spec(specs, n):
    return specs[n] if n < 4 else POOL[n - 4]


@functools.lru_cache(maxsize=None)
def stopped_case(sharing):
    """(node descriptions [N], templates [2N]: template 2i ends node i STOPPED, template 2i + 1 runs node i to exhaustion)"""
    descs, specs = [], []
    for seed, t, nb in STOPPED_PAIRS[sharing]:
        d, own = edge_draw(seed)
        descs.append(d)
        specs += [own[t], neighbour_spec(own, nb)]
    return descs, specs


# ---- B: the chunk seam ------------------------------------------------------------------------------------------------------------------
SEAM_SLOTS = (0, 63, 64)
# the STOPPED pair at each of SEAM_SLOTS (seed, template of the draw); fillers are drawn from the wide generator at SEAM_FILL_SEED
SEAM_PAIRS = [(14397, 2), (261, 2), (499, 2)]             # (slot 0 counts two replicas in front of its flag)
SEAM_FILL_SEED = 9895
SEAM_AFTER = {1: 43, 65: 19}                                  # wide slot -> seed of edge_draw: the record behind a STOPPED one, with room for its template
SEAM_PLAIN_AT = (0, 7, 40, 64, 66)                            # ordinary nodes go in front of these wide slots (66: behind the last)


@functools.lru_cache(maxsize=None)
def seam_case(n_wide=66):
    """(node descriptions, templates, names of the wide records in slot order): SEAM_PAIRS' nodes at wide slots 0, 63 and 64, the
    record behind each one with room for its template, fillers from the wide generator in between and five ordinary nodes around
    the seam.  n_wide = 65 drops the last wide record: slot 64 is then alone in its chunk."""
    rng = np.random.default_rng(SEAM_FILL_SEED)
    plain = np.random.default_rng(SEAM_FILL_SEED + 1)
    at = dict(zip(SEAM_SLOTS, SEAM_PAIRS))
    descs, specs, names = [], [], []
    for slot in range(66):
        if slot in SEAM_PLAIN_AT:
            descs.append(util.random_node_desc(plain, f"p{slot:02d}", 0.1))
        if slot in at:
            d, own = edge_draw(at[slot][0])
            specs.append(own[at[slot][1]])
        elif slot in SEAM_AFTER:
            d = edge_draw(SEAM_AFTER[slot])[0]
        else:
            while True:                                       # (a node the packer mirrors as a wide record with sharing off)
                d = util.random_wide_node_desc(rng, "", 0.1)
                sockets = int(d["labels"][NFD + "nfd-extras-cpu.numSockets"])
                if sockets >= 3 or int(d["labels"][NFD + "nfd-extras-cpu.num_cores"]) // sockets > 64:
                    break
        d = dict(d, name=f"b{slot:02d}")
        descs.append(d)
        names.append(d["name"])
    descs.append(util.random_node_desc(plain, "p66", 0.1))
    if n_wide == 65:
        descs = [d for d in descs if d["name"] != "b65"]
        names = names[:65]
    return descs, specs + [gc.GPULESS], names


# ---- C: shared-NIC bandwidth at the rounding boundary -----------------------------------------------------------------------------------
BW_CAP = 110
BW_SPEEDS = (25, 40, 100, 200)
# per-replica demands in Gb/s: the first seven end some NIC's run one replica short of exact arithmetic, the others do not - 2.5, 4.5 and
# 7.5 land the last replica on the capacity itself (remainder 0.0, which still fits)
BW_VALUES = (7.2, 3.6, 1.8, 0.6, 0.3, 1.2, 0.9, 2.5, 4.5, 7.5, 5.0, 9.0)
# (d) two groups on the one NIC of NUMA node 0: (rx of group 0, rx of group 1)
BW_TWO_GROUP = [(7.2, 1.8), (1.8, 7.2), (7.2, 0.3), (0.3, 7.2), (2.5, 7.5), (3.6, 0.9)]
BW_ASYMMETRIC = [(7.2, 3.6), (1.8, 4.5), (2.5, 7.2)]          # (rx, tx) of one group: the tighter direction ends the run


def nic_node_desc(name, nics, sockets=4, cpp=128):
    """An empty SMT node of `sockets` x `cpp` cores whose NICs are `nics`: (Gb/s, NUMA node) each, all behind switch 0x10."""
    lab = {NFD + "nfd-extras-cpu.numSockets": str(sockets), NFD + "nfd-extras-cpu.num_cores": str(sockets * cpp),
           NFD + "cpu-hardware_multithreading": "true", "DATA_PLANE_VLAN": "7", "DATA_DEFAULT_GW": "10.1.0.1/32"}
    for j, (gbps, numa) in enumerate(nics):
        lab[NFD + f"nfd-extras-nic.eth{j}.mlx.{0xABE000 + j:012x}.{gbps * 1000}Mbs.{numa}.10.{j}.0"] = "true"
    return dict(name=name, labels=lab, hugepages=[16, 16], active=True, used_cores=[], used_gpus=[], nic_pods_used=[0] * len(nics),
                busy_time=util.CLOCK - 500.0)


def bw_spec(*groups):
    """A NUMA template of one two-core SMT group per (rx, tx): one physical core a replica and group, no GPU, no hugepages."""
    return dict(map_type="NUMA", hugepages_gb=0, misc=0, misc_smt=False,
                groups=[dict(proc=2, helpers=0, rx=float(rx), tx=float(tx), proc_smt=True, helper_smt=False, gpus=[]) for rx, tx in groups])


def bw_nodes():
    """One NIC of each speed on NUMA node 0 of its own node; (e) a 40 G and a 100 G NIC on NUMA node 0 of one node, in that order."""
    return [nic_node_desc(f"c{s:03d}", [(s, 0)]) for s in BW_SPEEDS] + [nic_node_desc("c40+100", [(40, 0), (100, 0)])]


def bw_templates():
    """[(kind, demands)]: `demands` the (rx, tx) of every group."""
    out = [("rx", ((v, 0.0),)) for v in BW_VALUES]
    out += [("tx", ((0.0, v),)) for v in BW_VALUES]
    out += [("both", ((v, v),)) for v in BW_VALUES]
    out += [("both", (d,)) for d in BW_ASYMMETRIC]
    out += [("two", ((a, 0.0), (b, 0.0))) for a, b in BW_TWO_GROUP]
    return out


def exact_count(nic_gbps, demands, cap=BW_CAP):
    """Replicas by exact rational arithmetic: the NICs of `nic_gbps` filled one after the other, 0.9 and every demand the decimal
    it is written as."""
    needs = [sum(Fraction(repr(float(d[x]))) for d in demands) for x in (0, 1)]
    return min(sum(min(int(Fraction(9, 10) * s / n) for n in needs if n) for s in nic_gbps), cap)


# (f) a group with two RX/TX pairs of dyadic speeds: the request carries the group's sum, the reference adds core by core.  It has
# a mirror of its own: one speed that is no multiple of 2^-20 in a packer turns such groups away (Packer.share_exact).
def split_case():
    """(nodes, templates): 4.5 = 2.5 + 2.0 on 40 G ends on the capacity after 8, 2.5 = 2.25 + 0.25 on 25 G after 9 - rx, then tx."""
    def spec(a, b, tx):
        g = dict(proc=4, helpers=0, proc_smt=True, helper_smt=False, gpus=[])
        g.update(dict(rx=0.0, tx=a, more_nic_pairs=[(0.0, b)]) if tx else dict(rx=a, tx=0.0, more_nic_pairs=[(b, 0.0)]))
        return dict(map_type="NUMA", hugepages_gb=0, misc=0, misc_smt=False, groups=[g])
    return [nic_node_desc("s040", [(40, 0)]), nic_node_desc("s025", [(25, 0)])], \
           [spec(2.5, 2.0, False), spec(2.25, 0.25, False), spec(2.5, 2.0, True), spec(2.25, 0.25, True)]


# ---- the cases as the tests run them ------------------------------------------------------------------------------------------------------
CASES = ["stopped_off", "stopped_on", "seam", "bandwidth", "split"]


@functools.lru_cache(maxsize=None)
def case(name):
    """(ENABLE_SHARING, node descriptions, templates, bound, indices of the nodes held to the reference)"""
    if name in ("stopped_off", "stopped_on"):
        descs, specs = stopped_case(name == "stopped_on")
        return name == "stopped_on", descs, specs, gc.CAP, list(range(len(descs)))
    if name in ("seam", "seam65"):
        descs, specs, names = seam_case(65 if name == "seam65" else 66)
        return False, descs, specs, gc.CAP, [i for i, d in enumerate(descs) if d["name"] in set(names)]
    if name == "bandwidth":
        descs = bw_nodes()
        return True, descs, [bw_spec(*d) for _, d in bw_templates()], BW_CAP, list(range(len(descs)))
    descs, specs = split_case()
    return True, descs, specs, gc.CAP, list(range(len(descs)))


def spread(descs, n=150, seed=9896):
    """(`n` node descriptions, positions of `descs` among them): `descs` at even distances among ordinary nodes - three blocks of 64
    nodes, so every shard of a three-shard engine holds some of them."""
    rng = np.random.default_rng(seed)
    at = [round(i * (n - 1) / max(1, len(descs) - 1)) for i in range(len(descs))]
    out = [util.random_node_desc(rng, f"q{i:03d}", 0.1) for i in range(n)]
    for i, d in zip(at, descs):
        out[i] = d
    return out, at


def stored(name):
    """The reference's stored entries [template][held node] of one case ("seam65": "seam" without its last wide record)."""
    if name == "seam65":
        return [row[:-1] for row in stored("seam")]
    v = refanswers._load(STORE).get(f"test_reference[{name}]")
    assert v is not None, f"no stored reference answers for {name}"
    return refanswers.decode(v[0])


# ---- every path that prices a shared NIC, one (node, template) pair of C at a time ------------------------------------------------------
# (node of bw_nodes(), kind, demands): the eight pairs whose count differs from exact arithmetic, five that end on the capacity, the
# other direction and both, two groups on one NIC in both orders, two NICs one after the other
WALKS = [("c040", "rx", ((7.2, 0.0),)), ("c040", "rx", ((3.6, 0.0),)), ("c040", "rx", ((1.8, 0.0),)), ("c040", "rx", ((0.6, 0.0),)),
         ("c025", "rx", ((0.3, 0.0),)), ("c100", "rx", ((1.2, 0.0),)), ("c100", "rx", ((0.9, 0.0),)), ("c200", "rx", ((1.8, 0.0),)),
         ("c025", "rx", ((2.5, 0.0),)), ("c040", "rx", ((4.5, 0.0),)), ("c100", "rx", ((4.5, 0.0),)), ("c100", "rx", ((7.5, 0.0),)),
         ("c200", "rx", ((7.5, 0.0),)),
         ("c040", "tx", ((0.0, 7.2),)), ("c040", "tx", ((0.0, 4.5),)), ("c040", "both", ((7.2, 7.2),)), ("c025", "both", ((2.5, 2.5),)),
         ("c040", "both", ((7.2, 3.6),)),
         ("c100", "two", ((7.2, 0.0), (1.8, 0.0))), ("c100", "two", ((1.8, 0.0), (7.2, 0.0))), ("c100", "two", ((7.2, 0.0), (0.3, 0.0))),
         ("c100", "two", ((2.5, 0.0), (7.5, 0.0))),
         ("c40+100", "rx", ((7.2, 0.0),)), ("c40+100", "rx", ((4.5, 0.0),))]
WALK_IDS = [f"{n}-{'+'.join(f'{rx:g}/{tx:g}' for rx, tx in d)}" for n, _, d in WALKS]


def walk_pair(node, kind, demands):
    """(node description, template, the reference's stored count) of one of WALKS"""
    descs = bw_nodes()
    i = [d["name"] for d in descs].index(node)
    t = bw_templates().index((kind, demands))
    return descs[i], bw_spec(*demands), stored("bandwidth")[t][i]


def check_shared_nic_walk(matcher_factory, desc, spec, N):
    """One node, one template, N the reference's count.  ScheduleBatch(apply=False) places N of N + 1 copies and leaves the mirror as
    it was.  Then FindNode + CommitPlacement on the mirror, k = 0 .. N times: FindNode still answers the node for every k < N and
    (None,) at k == N, where ExplainNode names NIC; Headroom(general=True) is N - k; and a fresh matcher packed from a node object
    that took the same k commits in CPython (the oracle's commit: speed_used += speed, one addition per core) gives the same
    headroom from a share record that is byte for byte the committing matcher's.  Every k for N <= 10; 0, N - 1 and N beyond."""
    name = desc["name"]
    ks = set(range(N + 1)) if N <= 10 else {0, N - 1, N}
    with gc.sharing_all(True):
        nl = {name: refmodel.build_node(desc)}
        shadow = refmodel.build_node(desc)
        m = matcher_factory(util.CLOCK)
        m.attach(nl)
        got = m.ScheduleBatch(nl, [refmodel.make_topology(spec) for _ in range(N + 1)], now=util.CLOCK, apply=False)
        assert [r[0] for r in got] == [name] * N + [None]
        for k in range(N + 1):
            if k in ks:
                h = m.Headroom(nl, refmodel.make_topology(spec), per_node=True, general=True, max_per_node=BW_CAP)
                assert h.error is None and h.form & pack.HEADROOM_FORM_WIDE and not h.flags.any()
                assert (int(h.per_node[0]), h.replicas, h.not_evaluated, h.stopped) == (N - k, N - k, 0, 0), (k, h)
                fresh = matcher_factory(util.CLOCK)
                h2 = fresh.Headroom({name: shadow}, refmodel.make_topology(spec), per_node=True, general=True, max_per_node=BW_CAP)
                assert h2.error is None and int(h2.per_node[0]) == N - k and not h2.flags.any(), (k, h2)
                assert fresh.engine.wide_share_download().tobytes() == m.engine.wide_share_download().tobytes(), k
            top = refmodel.make_topology(spec)
            res = m.FindNode(nl, top)
            if k == N:
                assert res == (None,)
                ex = m.ExplainNode(nl, refmodel.make_topology(spec), now=util.CLOCK)
                assert ex.error is None and ex.counts["NIC"] == 1 and ex.total == 1, ex
                break
            assert res[0] == name, (k, res)
            m.CommitPlacement(name, top, res[1])
            shadow.busy_time = LONG_AGO
            top2 = refmodel.make_topology(spec)
            O.commit(shadow, top2, O.find_node({name: shadow}, top2, util.CLOCK)[1], LONG_AGO)
        used = m.engine.wide_share_download()["used"][0]
    assert N == 0 or used.max() > 0
    return used
