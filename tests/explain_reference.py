"""The stage at which the UNMODIFIED reference drops each node for a pod, derived from its own intermediate results rather than
from its log text (nhd/Matcher.py:65-391).  The codes are include/nhdfit.h's NHDFIT_STAGE_* (nhd_amd.matcher.STAGES):

    FilterPodResources drops a node           MAINTENANCE if node.maintenance, else HUGEPAGES
    FilterNumaTopology returns (None, None)   every remaining node was dropped at BUSY (a GPU pod on a busy node) or GPU
    a node absent from gpu_cands              BUSY
    an empty gpu_cands / cpu_cands / nic_cands entry   GPU / CPU / NIC
    IntersectResources drops the node         PCI if its NIC list is empty after the PCI pruning, else NUMA
    the node survives                         FITS

A pod whose map type is neither NUMA nor PCI makes the reference return before it filters anything it reports
(Matcher.py:45-47): every node is NOT_CANDIDATE, as on the device.  Everything runs on deep copies of the filter's results,
with the reference's print()s swallowed."""
import contextlib
import copy
import io

NOT_CANDIDATE, MAINTENANCE, HUGEPAGES, BUSY, GPU, CPU, NIC, PCI, NUMA, FITS = range(10)


def reference_stages(ref, nl, top):
    """{node name: stage code} for every node of `nl` (the dict FindNode would be given) and the reference topology `top`."""
    m = ref.Matcher()
    maptype = ref.TopologyMapType
    if top.map_type not in (maptype.TOPOLOGY_MAP_NUMA, maptype.TOPOLOGY_MAP_PCI):
        return {n: NOT_CANDIDATE for n in nl}
    out = {}
    with contextlib.redirect_stdout(io.StringIO()):
        kept = m.FilterPodResources(nl, top)
        for n, v in nl.items():
            if n not in kept:
                out[n] = MAINTENANCE if v.maintenance else HUGEPAGES
        filts = m.FilterNumaTopology(kept, top)
        if filts[0] is None:                                # Matcher.py:145-147: every node dropped at busy or GPU
            want_gpu = sum(top.GetTotalGpusRequested()) > 0
            for n, v in kept.items():
                out[n] = BUSY if want_gpu and v.IsBusy() else GPU
            return out
        res, cand = filts
        for n in kept:
            if n not in res["gpu"]:
                out[n] = BUSY
            elif not res["gpu"][n]:
                out[n] = GPU
            elif not res["cpu"][n]:
                out[n] = CPU
            elif not res["nic"].get(n):
                out[n] = NIC
        if cand:
            after = m.IntersectResources(kept, copy.deepcopy(filts), top.map_type)
            for n in cand:
                if n in after[1]:
                    out[n] = FITS
                elif top.map_type == maptype.TOPOLOGY_MAP_PCI and not after[0]["nic"][n]:
                    out[n] = PCI
                else:
                    out[n] = NUMA
    assert set(out) == set(nl)
    return out
