"""Clusters and pods drawn at the EDGES of the record formats (include/nhdfit.h), shared by tools/soak_extreme.py and the tests that
hold the host twins and the device to the oracles there (it lives beside workload/synth.py, not under tests/, because the tool
draws from it): sockets of 1..64 physical cores next to wide ones of 65..128, up to 16 NICs
and 8 GPUs per NUMA node, a dozen distinct NIC speeds (the capacity classes, two of them below the 11 000 Mb/s threshold), up to 14
PCIe switches, pods_used of 0..3, arbitrary isolcpus sets, busy times on either side of the 30 s window, free hugepages around the
tile's table (1 022 GiB) - and pods of 1..6 processing groups with core counts that often do not fit, rx values on either side of
the speed * 0.9 capacities.  The order of the draws is part of the interface: the seeds the suite names stand for fixed clusters
(tests/test_format_edges.py pins three of them by their hash)."""
import hashlib
import json
import re

import numpy as np

from workload import refmodel
from workload.refmodel import NFD

SPEEDS = [9000, 10999, 11000, 12000, 20000, 25000, 40000, 50000, 56000, 100000, 200000, 400000, 11001, 33000]   # two below Node.py:403's threshold
NAMES = ["default"] + ["grp%02d" % k for k in range(40)]
OCCUPANCIES = [0.0, 0.1, 0.3, 0.6]
CLOCK = 1.0e6                                        # the suite's virtual clock (tests/util.py CLOCK)


def edge_labels(rng, heavy, few=False, beyond=False):
    wide = rng.random() < 0.25
    if wide:
        sockets = int(rng.choice([1, 2, 3, 4], p=[0.1, 0.4, 0.25, 0.25]))
        cpp = int(rng.choice([65, 66, 96, 127, 128, 7, 20]))
    else:
        sockets = int(rng.choice([1, 2], p=[0.2, 0.8]))
        cpp = int(rng.choice([2, 3, 5, 8, 16, 31, 32, 33, 48, 63, 64]))
    phys = cpp * sockets
    smt = rng.random() < 0.6
    lab = {NFD + "nfd-extras-cpu.numSockets": str(sockets), NFD + "nfd-extras-cpu.num_cores": str(phys)}
    if smt:
        lab[NFD + "cpu-hardware_multithreading"] = "true"
    mode = rng.random()
    if mode < 0.5:                                         # arbitrary isolcpus: a few ranges anywhere in the logical id space
        total = phys * (2 if smt else 1)
        spans = []
        for _ in range(int(rng.integers(1, 5))):
            a = int(rng.integers(0, total))
            spans.append((a, min(total - 1, a + int(rng.integers(0, max(1, total // 2))))))
        lab[NFD + "nfd-extras-cpu.isolcpus"] = "_".join(f"{a}-{b}" for a, b in spans)
    elif mode < 0.8:
        spans = [(s * cpp + 1, (s + 1) * cpp - 1) for s in range(sockets) if cpp > 1]
        if smt:
            spans += [(phys + s * cpp + 1, phys + (s + 1) * cpp - 1) for s in range(sockets) if cpp > 1]
        if spans:
            lab[NFD + "nfd-extras-cpu.isolcpus"] = "_".join(f"{a}-{b}" for a, b in spans)
    n_sw = int(rng.integers(1, 8 if wide else 7))          # switches per NUMA node (<= 14 per node on the fast layout)
    per_numa = [int(rng.integers(0, 17)) if heavy else int(rng.choice([0, 1, 2] if few else [0, 1, 2, 3, 4])) for _ in range(sockets)]
    if beyond and rng.random() < 0.5:
        per_numa[int(rng.integers(0, sockets))] = int(rng.integers(17, 21))      # more NICs on a NUMA node than any record holds: the node never matches
    speeds = rng.choice(SPEEDS, size=int(rng.integers(1, 5)), replace=False)
    j = 0
    for numa in range(sockets):
        for _ in range(per_numa[numa]):
            sw = 0x10 * (numa + 1) + int(rng.integers(0, n_sw))
            if wide and rng.random() < 0.05:
                sw = 0x90                                  # one switch seen from several NUMA nodes (general path only)
            lab[NFD + f"nfd-extras-nic.eth{j}.mlx.{0xABE000 + j:012x}.{int(rng.choice(speeds))}Mbs.{numa}.{sw:x}.{j}.0"] = "true"
            j += 1
    g = 0
    for numa in range(sockets):
        for _ in range(9 if beyond and rng.random() < 0.3 else int(rng.choice([0, 1, 2, 4, 8], p=[0.4, 0.15, 0.2, 0.15, 0.1]))):
            if g >= 32:
                break
            sw = 0x10 * (numa + 1) + int(rng.integers(0, n_sw))
            lab[NFD + f"nfd-extras-gpu.{g}.V100.{numa}.{sw:x}"] = "true"
            g += 1
    lab["DATA_PLANE_VLAN"] = "7"
    lab["DATA_DEFAULT_GW"] = "10.1.0.1/32"
    if rng.random() < 0.6:
        lab["NHD_GROUP"] = ".".join(rng.choice(NAMES, size=int(rng.integers(1, 5)), replace=False))
    if rng.random() < 0.04:
        lab[refmodel.MAINT_LABEL] = "scheduled"
    return lab


def edge_node(rng, name, heavy, occupancy, few=False, beyond=False):
    lab = edge_labels(rng, heavy, few, beyond)
    phys = int(lab[NFD + "nfd-extras-cpu.num_cores"])
    smt = (NFD + "cpu-hardware_multithreading") in lab
    used = []
    for c in range(phys):
        r = rng.random()
        if r < occupancy:
            used.append(c)
            if smt and rng.random() < 0.7:
                used.append(c + phys)
        elif smt and r < occupancy + 0.08:
            used.append(c + phys)
    ngpu = sum(1 for k in lab if "nfd-extras-gpu" in k)
    nnic = 0
    for k in lab:
        if "nfd-extras-nic" in k and int(re.search(r"\.(\d+)Mbs\.", k).group(1)) >= 11000:          # (Node.py:403: slower NICs are not kept)
            nnic += 1
    return dict(name=name, labels=lab, hugepages=[2048, int(rng.choice([0, 1, 16, 1021, 1022, 1023, 2047]))], active=bool(rng.random() > 0.04),
                used_cores=sorted(used), used_gpus=[g for g in range(ngpu) if rng.random() < 0.3],
                nic_pods_used=[int(rng.choice([0, 0, 0, 1, 2, 3])) for _ in range(nnic)],
                busy_time=CLOCK - float(rng.choice([0.0, 29.99, 30.0, 30.01, 500.0, 500.0, 500.0])))


def edge_pod(rng, max_groups):
    groups = []
    G = int(rng.integers(1, max_groups + 1))
    for _ in range(G):
        ng = int(rng.choice([0, 1, 2, 3], p=[0.5, 0.3, 0.15, 0.05]))
        groups.append(dict(proc=int(rng.choice([2, 2, 3, 4, 6, 9, 17, 33])) if G <= 3 else int(rng.integers(2, 5)),
                           helpers=int(rng.choice([0, 0, 1, 2, 5])),
                           rx=float(rng.choice([0, 0, 0.1, 1e-9, 5, 9.9, 10.8, 18, 22.5, 22.500001, 36, 45, 50.4, 89.99999, 90, 90.00001, 180, 360])),
                           tx=float(rng.choice([0, 0, 5, 9.9, 10.8, 12.25, 22.5, 45, 90, 180])),
                           proc_smt=bool(rng.random() < 0.5), helper_smt=bool(rng.random() < 0.5),
                           gpus=[int(rng.integers(0, 4)) for _ in range(ng)]))
    return dict(map_type=str(rng.choice(["NUMA", "PCI", "NONE", "BOGUS"], p=[0.5, 0.42, 0.04, 0.04])),
                hugepages_gb=int(rng.choice([0, 0, 1, 16, 17, 1021, 1022, 1023, 2000])), misc=int(rng.choice([0, 1, 2, 3, 7])),
                misc_smt=bool(rng.random() < 0.5), groups=groups)


def states_agree(nodes, m):
    """delta_check.state_of(nodes) == delta_check.mirror_state(m) for the nodes the five planes hold (a wide node's entry there is a
    placeholder; its record is re-uploaded whole and the finds that follow check it)."""
    from nhd_amd import pack
    from tests import delta_check as D
    skip = set(m.wide_nodes) | set(m.unmirrored)
    pk = pack.Packer()
    t_obj = pk.pack_nodes(nodes)
    t_dev = m.engine.download()
    for i, name in enumerate(m._names):
        if name in skip:
            continue
        if D._row(pk, t_obj, i) != D._row(m.packer, t_dev, i):
            print("   state differs on", name, D._row(pk, t_obj, i), D._row(m.packer, t_dev, i), flush=True)
            return False
        sn, sp = m.packer.sigs_from_detail(t_dev.detail[i])
        if [int(x) for x in t_dev.p3[i]["sig_numa"]] != sn or [int(x) for x in t_dev.p3[i]["sig_pci"]] != sp:
            print("   signature ids differ on", name, flush=True)
            return False
        if m.packer.group_sets[int(t_dev.p4[i]["group_set"])] != int(t_dev.p3[i]["groups"]):
            print("   group set differs on", name, flush=True)
            return False
    return True


# ---- the soak's clusters, seed by seed ---------------------------------------------------------------------------------------------------
def soak_draw(seed, n_nodes=14, n_pods=16):
    """What tools/soak_extreme.py draws first for `seed`: (rng, heavy share, largest group count, node descriptions, pod specs); the
    generator is handed back because the tool goes on drawing from it (node groups of the pods, fresh pods of the op streams).
    seed % 3 == 0: NIC-heavy nodes against pods of one or two groups (the oracle enumerates K^G NIC choices per NUMA assignment in
    Python); seed % 5 == 0: pods of up to six groups against nodes of at most two NICs per NUMA node; seed % 7 == 3 on a NIC-heavy
    seed: a few nodes beyond EVERY record (17..20 NICs or nine GPUs on a NUMA node) - they never match (HipMatcher.unmirrored)."""
    rng = np.random.default_rng(880000 + seed)
    heavy_share = 0.12 if seed % 3 == 0 else 0.0
    max_groups = 2 if heavy_share else 6 if seed % 5 == 0 else 4 if seed % 2 else 3
    descs = [edge_node(rng, f"e{i:04d}", rng.random() < heavy_share, occupancy=float(rng.choice(OCCUPANCIES)), few=max_groups > 4,
                       beyond=bool(heavy_share) and seed % 7 == 3 and rng.random() < 0.3) for i in range(n_nodes)]
    specs = [edge_pod(rng, max_groups) for _ in range(n_pods)]
    return rng, heavy_share, max_groups, descs, specs


def draw_hash(seed):
    """sha256 over the node descriptions and pod specs of soak_draw(seed): the draw order, pinned."""
    _, _, _, descs, specs = soak_draw(seed)
    return hashlib.sha256(json.dumps([descs, specs], sort_keys=True).encode()).hexdigest()


# ---- what a description puts at which edge -----------------------------------------------------------------------------------------------
def shape_of(desc):
    """(sockets, physical cores per socket, NICs kept per NUMA node, GPUs per NUMA node) of a node description."""
    lab = desc["labels"]
    sockets = int(lab[NFD + "nfd-extras-cpu.numSockets"])
    cpp = int(lab[NFD + "nfd-extras-cpu.num_cores"]) // sockets
    nics, gpus = [0] * sockets, [0] * sockets
    for k in lab:
        if "nfd-extras-nic" in k:
            mt = re.search(r"\.(\d+)Mbs\.(\d+)\.", k)
            if int(mt.group(1)) >= 11000:
                nics[int(mt.group(2))] += 1
        elif "nfd-extras-gpu" in k:
            gpus[int(k.split(".")[-2])] += 1
    return sockets, cpp, nics, gpus


def upper_half_cores(desc):
    """A one- or two-socket node with 33..64 physical cores per socket: bits 32..63 of its sockets' core masks are in use."""
    sockets, cpp, _, _ = shape_of(desc)
    return sockets <= 2 and 33 <= cpp <= 64


def nic_heavy(desc):
    """A one- or two-socket node of at most 64 cores per socket with 9..16 NICs on a NUMA node."""
    sockets, cpp, nics, _ = shape_of(desc)
    return sockets <= 2 and cpp <= 64 and 9 <= max(nics) <= 16


# ---- one cluster that spans tiles ----------------------------------------------------------------------------------------------------------
BIG_SEED, BIG_NODES, BIG_PODS, BIG_HEAVY = 424242, 600, 96, 0.08


def big_edge_case(n_pods=BIG_PODS):
    """(node descriptions, pod specs): 600 edge nodes (NIC-heavy share 0.08) and pods of up to four groups from one generator.  More
    than BIG_PODS pods: the first BIG_PODS stay the same ones."""
    rng = np.random.default_rng(BIG_SEED)
    descs = [edge_node(rng, f"e{i:04d}", rng.random() < BIG_HEAVY, occupancy=float(rng.choice(OCCUPANCIES))) for i in range(BIG_NODES)]
    specs = [edge_pod(rng, 4) for _ in range(n_pods)]
    return descs, specs


def mask_words(keep):
    """n booleans -> the uint64 candidate words of the C-ABI."""
    n = len(keep)
    bits = np.zeros(((n + 63) // 64) * 64, bool)
    bits[:n] = keep
    return np.ascontiguousarray(np.packbits(bits.reshape(-1, 64), axis=1, bitorder="little").view("<u8").reshape(-1))
