"""One context reused while its mirror is replaced, on the CPU (tests/reuse_check.py has the chains and the checks): the conditions under
which the device tests say something, asserted from the oracles and the packed tables alone, and every chain on the host twins - which
shows the chains and checks sound before a device runs them.  tests/test_reuse_gpu.py holds the device to the same oracles."""
import pytest

from nhd_amd._lib import NhdFitError
from nhd_amd.matcher import HipMatcher
from tests import edge_check as C
from tests import harness
from tests import reuse_check as R
from tests import seam_check as S
from tests import util
from tests.harness.explain_twin import ExplainHarnessEngine
from tests.harness.headroom_limit_twin import HeadroomLimitHarnessEngine


class TwinEngine(HeadroomLimitHarnessEngine, ExplainHarnessEngine):
    pass


# ---- what the oracles alone say ---------------------------------------------------------------------------------------------------------------
def test_the_padding_lanes_of_the_shrunk_stop_would_change_answers():
    """At the 65-node stop of chain 1 the lanes 65..127 hold live nodes of X.  By the C oracle alone: at least 10 of them are feasible
    for at least 10 pods each, and under some mask at least 10 pods would be given one of them instead of their winner inside X[0:65]
    (or instead of none) if those lanes were read - a kernel that read a padding lane would answer differently."""
    c = R.chain1()
    assert c.x.n == 257 and c.x.cfg == 4 and c.x.P == S.PODS + S.FOURS
    nodes, moved = c.padding_figures()
    print(f"X[65:128]: {nodes} nodes feasible for at least 10 pods; pods that would move there, per mask of the 65-node stop: {moved}")
    assert nodes >= 10
    assert max(moved.values()) >= 10 and moved["straddle 1"] >= 1


def test_every_straddle_of_every_stop_has_winners_on_both_sides():
    c = R.chain1()
    fig = c.straddle_figures()
    print("chain 1, (pods that win in front of the boundary, at or beyond it):", fig)
    assert {stop: len(f) for stop, f in fig.items()} == {"whole": 4, "shrunk": 1, "grown": 2, "cut": 2}
    for stop, f in fig.items():
        assert all(front >= 1 and beyond >= 1 for front, beyond in f.values()), (stop, f)
    for stop, v in c.views.items():                              # the island: some pod is given the far node
        keep, far = v.island()
        assert (v.oracle_winners(keep) == far).any(), stop
        assert (v.oracle_winners(v.masks()[-1][1])[:v.n_small] >= 64 * (v.chunks - 1)).any(), stop       # find_commit's pod exists


def test_the_class_tables_of_chain_2_differ_in_size():
    """Distinct (socket, free GPUs, NUMA signature, PCI signature) tuples of the packed tables: D needs more X rows than the 32 a
    context starts with (fit_core.h kMinXCap), A does not - so that A's lds_bytes on a context that held D equals a fresh context's
    only if the class table was forgotten with D's nodes."""
    counts = {name: R.class_count(S.rung(name).packed()[1]) for name in R.CHAIN2}
    sigs = {name: int(S.rung(name).packed()[0].dictionary_arrays()[6]) for name in R.CHAIN2}
    print("chain 2: node classes", counts, "signatures", sigs)
    assert counts["D"] > 32 >= counts["A"]
    assert sigs["D"] > sigs["A"]


def test_the_stale_class_rows_of_chain_2_stayed_inside_the_tile_image():
    """Before the class table was forgotten with its nodes, the digest role formed an X row for every class of every earlier occupant
    from rows of the CURRENT dictionary's image named by the old class: by fit_core.h make_layout, at chain 2's shapes that read ends
    inside the image at every seam and row width even with the fewest X rows a context provisions (the node tables of D name
    signature ids up to 28 of their 151, a row is at most 128 B: less than 4 KB behind off_r1, and the hot section behind the R
    rows is 20 KB and more).  So running the chain on a library without the reset reads no memory outside the image's buffer."""
    seen = []
    for prev, nxt in zip(R.CHAIN2, R.CHAIN2[1:]):
        seen.append(S.rung(prev).packed()[1])
        sig, reach = R.stale_row_reach(seen, S.rung(nxt).packed()[0])
        print(f"{prev} -> {nxt}: largest signature id named so far {sig}; per row width (read ends at, image bytes) {reach}")
        assert sig <= 28
        assert all(end <= size for end, size in reach.values()), (prev, nxt, reach)


# ---- the chains on the host twins ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("by_truncate", [False, True], ids=["emptied", "truncated"])
def test_chain_1_on_the_host_twin(by_truncate):
    fig = R.drive_chain1(TwinEngine(0), by_truncate)
    print("chain 1 on the twin:", fig)
    assert fig["cut"]["carried mask"] and fig["shrunk"]["replicas"]["island"] >= 5


@pytest.mark.parametrize("forget", [True, False], ids=["forgotten", "kept"])
def test_chain_2_on_the_host_twin(forget):
    R.drive_chain2(TwinEngine(0), forget)


def test_origin_records_and_deltas_across_the_seam_on_the_host_twin():
    fig = R.check_origin_across_the_seam(harness.HarnessEngine(0), lambda: harness.HarnessEngine(0), NhdFitError)
    print(fig)
    assert fig["repack"] >= 1


def test_the_twin_refuses_gap_uploads():
    R.check_gap_refusals(harness.HarnessEngine(0), NhdFitError)


def test_the_twin_truncates_as_the_library_does():
    """HarnessEngine.truncate: planes, wide and origin bound of the prefix; truncate(0) empties."""
    r = S.rung("A")
    pk, table, _ = r.packed()
    eng = harness.HarnessEngine(0)
    eng.set_dictionary(pk)
    eng.upload(table)
    assert eng.origin_hi == 65
    eng.truncate(40)
    assert eng.n == 40 and eng.origin_hi == 40 and eng.download().p0.tobytes() == table.p0[:40].tobytes()
    with pytest.raises(NhdFitError):
        eng.truncate(41)
    eng.truncate(0)
    assert eng.n == 0 and eng.origin_hi == 0


def _twin_matcher(clock=None):
    return HipMatcher(clock=clock or (lambda: util.CLOCK), engine_factory=TwinEngine)


def test_wide_records_across_the_seam_on_the_host_twin():
    case = C.big_case()
    m = _twin_matcher()
    placed = {tag: R.check_wide_step(m, case, tag, member) for tag, member in R.wide_steps(case)}
    print("wide records across the seam, pods placed per step:", placed)
    assert all(v >= 100 for v in placed.values())
    cuts = R.check_wide_truncate(m, case)
    print("truncated to (nodes, wide records):", cuts)


def test_a_chain_of_edge_seeds_through_one_twin_matcher():
    m = _twin_matcher()
    tot = {}
    for seed in R.EDGE_SEEDS + R.EDGE_SEEDS[::-1]:
        for k, v in C.check_new_entries(m, seed).items():
            tot[k] = tot.get(k, 0) + v
    print("edge seeds", R.EDGE_SEEDS, "and back:", tot)
    assert tot["unmirrored"] >= 2 and tot["stopped runs"] >= 2 and tot["replicas"] >= 20


def test_reattach_on_one_twin_matcher():
    m = HipMatcher(clock=lambda: util.CLOCK, engine_factory=harness.HarnessEngine)
    for seed in (0, 5):
        got = C.check_schedule_one(None, seed, fused_form=False, matcher=m)
        assert got["pods"] >= 10 and got["placed"] >= 5
        m.detach()
