"""Shared by the CPU and GPU tests of candidates on the general path (nhdfit_candidates_general): the inputs that are held to the
UNMODIFIED reference's definition (tests/candidates_reference.iterate over Matcher().FindNode, K = 8) - tests/headroom_general_check.py's
three clusters (wide nodes of a mixed cluster, two ENABLE_SHARING clusters with all three switches flipped) against eighteen templates,
and the fixtures tests/golden/beyond/*.json and tests/golden/sharing/*.json with their own pods - the reference's lists, stored with the
CPU test module's answers (tests/golden/refanswers/tests.test_candidates_general_reference.json) so the GPU box holds the device to
them.

gc.templates() alone has no pod with a preferred node and no feasible four-group pod: gc.FOUR, gc.GPULESS and gc.NOTHING carry that
ground, and FACTS pins what the inputs say (feasible, preferred of five (cluster, template) pairs) so that they cannot silently stop
saying anything."""
from nhd_amd.matcher import STAGES
from tests import candidates_reference as cr
from tests import headroom_general_check as gc
from tests import refanswers, util
from workload import refmodel

STORE = "tests.test_candidates_general_reference"
K = cr.K


def templates():
    """gc.templates() (12) + gc.FOUR (4) + gc.GPULESS + gc.NOTHING"""
    return gc.templates() + list(gc.FOUR) + [gc.GPULESS, gc.NOTHING]


T_FOUR0, T_FOUR1, T_FOUR3, T_GPULESS, T_NOTHING = 12, 13, 15, 16, 17
# (cluster, template) -> (feasible, preferred): the composed form on the host twin at K = 8 gave these before the entry existed
FACTS = {("mixed", T_FOUR0): (26, 0), ("mixed", T_FOUR3): (2, 0), ("mixed", T_GPULESS): (61, 18),
         ("sharing_random", T_FOUR1): (21, 7), ("sharing_mixed", T_NOTHING): (34, 12)}


def reference_lists(ref, descs, specs, sharing, clock, keep=None, k=K):
    """[pod] lists of the reference on the cluster `descs` (keep: per pod the names FindNode is handed, or None: all)."""
    from oracle import ref_loader
    ref_loader.VirtualClock(clock).install()
    with gc.sharing_all(sharing, ref):
        nl = util.build_cluster(descs, ref)
        return [cr.iterate(ref_loader.find_node, nl if keep is None else {nm: nd for nm, nd in nl.items() if nm in keep[p]},
                           lambda: refmodel.make_topology(s, ref), k=k) for p, s in enumerate(specs)]


def matcher_lists(matcher_factory, descs, specs, sharing, clock, pod_groups=None, k=K, general=True):
    """(matcher, nl, results of CandidatesMany(general=...), [pod] lists, [pod] FITS counts of ExplainNodes on the same matcher)"""
    with gc.sharing_all(sharing):
        nl = util.build_cluster(descs)
        m = matcher_factory(clock)
        tops = [refmodel.make_topology(s) for s in specs]
        got = m.CandidatesMany(nl, tops, k=k, pod_groups=pod_groups, now=clock, general=general)
        fits = [e.counts.get("FITS", 0) for e in m.ExplainNodes(nl, [refmodel.make_topology(s) for s in specs], pod_groups, now=clock)]
    return m, nl, got, cr.lists_of(got), fits


def consistent(results, lists, fits, k=K):
    """A list is as long as the summary says, no node is named twice, nothing is left unevaluated, `feasible` is explain's FITS."""
    for c, row, f in zip(results, lists, fits):
        assert c.error is None and len(row) == min(k, c.feasible) and c.preferred <= c.feasible
        assert len({e[0] for e in row}) == len(row)
        assert c.feasible == f


def stored(test_id, k=0):
    """Stored reference answer `k` of one case (as tests/test_candidates_general_reference.py recorded it)."""
    v = refanswers._load(STORE).get(test_id)
    assert v is not None and len(v) > k, f"no stored reference answers for {test_id}"
    return refanswers.decode(v[k])


assert "FITS" in STAGES
