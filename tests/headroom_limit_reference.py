"""The stage that ends a node's headroom run as the UNMODIFIED reference defines it (include/nhdfit.h, nhdfit_headroom_limits): the
reference's own run (tests/headroom_reference.py: FindNode -> SetPhysicalIdsFromMapping -> ClaimPodNICResources back to back on a
private rebuild of the node) and then, on the node object the run leaves behind, with busy_time put long ago, the stage at which
the reference's filter drops it for a fresh topology (tests/explain_reference.py, from the filter's own intermediate results).  A
run the reference ends by raising leaves a half-committed node: no stage (NONE).

`independent_limit` is the same over the independent oracle's run, with the C oracle's stage (oracle/coracle.py, oracle_explain) on
the final node - it travels where the reference does not."""
from oracle import coracle
from tests.explain_reference import reference_stages
from tests.headroom_reference import LONG_AGO, independent_headroom, reference_headroom

NONE = 255                                           # NHDFIT_LIMIT_NONE


def _keeping(build_node, kept):
    def build():
        kept.append(build_node())
        return kept[-1]
    return build


def reference_limit(ref, build_node, make_top, cap):
    """(replicas, stopped, stage) for the node `build_node()` returns (a fresh reference Node) and the template `make_top()`."""
    kept = []
    k, stopped = reference_headroom(ref, _keeping(build_node, kept), make_top, cap)
    if stopped:
        return k, stopped, NONE
    node, = kept
    node.busy_time = LONG_AGO
    return k, stopped, reference_stages(ref, {node.name: node}, make_top())[node.name]


def independent_limit(build_node, make_top, cap, now=1.0e6):
    """(replicas, stopped, stage) by the independent oracle's run and the C oracle's stage on the node it leaves behind."""
    kept = []
    k, stopped = independent_headroom(_keeping(build_node, kept), make_top, cap, now=now)
    if stopped:
        return k, stopped, NONE
    node, = kept
    node.busy_time = LONG_AGO
    cl = coracle.Cluster.from_nodes({node.name: node})
    _, stages = cl.explain(cl.pods_from_tops([make_top()]), now, per_node=True)
    return k, stopped, int(stages[0, 0])
