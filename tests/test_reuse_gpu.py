"""The DEVICE with ONE context reused while its mirror is replaced (`pytest -m gpu`; tests/reuse_check.py has the chains, the views and
the checks, tests/test_reuse.py asserts from the oracles alone that they say something and runs them on the host twins).  Every other
device test builds a fresh context per case; here the same nhdfit_ctx is emptied, given another dictionary and another cluster, cut
and grown in place, as HipMatcher._full_upload does whenever a node joins or leaves.  Everything is bit-exact: winners, verdict matrix
and stages against the C oracle on the masked view, every winner's mapping against the Python oracle on that node alone, headroom
against independent_limit, raw records and statuses against the host twin; the bits at and beyond n of the last chunk's bitmap words
are zero.  Nothing here reads the reference tree."""

import numpy as np
import pytest

from nhd_amd._lib import NhdFitError
from nhd_amd.engine import Engine
from tests import edge_check as C
from tests import reuse_check as R
from tests import seam_check as S

pytestmark = pytest.mark.gpu


def _matcher(clock=None):
    from nhd_amd.matcher import HipMatcher
    return HipMatcher(device=0, clock=clock or (lambda: C.NOW))


@pytest.mark.parametrize("by_truncate", [False, True], ids=["emptied", "truncated"])
def test_chain_1_shrink_grow_in_place_cut(by_truncate):
    """X[0:257] -> X[0:65] (reset_nodes + upload, or truncate(65)) -> X[65:129] appended at 65 -> reset_nodes + the cut, on one
    context with one dictionary.  At every stop: the previous stop's candidate words re-sent where they fit, the five forms of find
    under five masks (the form that ran asserted by nhdfit_get_stats), explain per node, find_commit for the first pod the oracle
    places in the last chunk, headroom and its limits on the 65-node stop.  There the lanes 65..127 of the second chunk's records
    held live nodes of X until the records were rewritten: 35 pods would win one of them under the straddle mask if a lane were read."""
    eng = Engine(0)
    fig = R.drive_chain1(eng, by_truncate)
    print("chain 1 on the device:", fig)
    assert fig["cut"]["carried mask"] and fig["shrunk"]["replicas"]["island"] >= 5
    eng.close()


def test_a_reused_context_reports_what_a_fresh_one_reports():
    """D (91 node classes: 128 provisioned X rows) and then A (18 classes) on one context: after the same staged find `nodes`, `nsig`,
    `ncls` and `lds_bytes` of nhdfit_get_stats equal those of a context that has only ever held A - the class table went with D's
    nodes.  (Until nhdfit_set_node_count forgot the classes, x_cap stayed at 128 and lds_bytes at D's size.)"""
    eng = Engine(0)
    got = {}
    for name in ("D", "A"):
        r, pk, table, reqs = R.install_rung(eng, name, forget=True)
        fresh = Engine(0)
        fresh.set_dictionary(pk)
        fresh.upload(table)
        want = R.staged_stats(fresh, r, reqs)
        fresh.close()
        got[name] = R.staged_stats(eng, r, reqs)
        assert got[name] == want, (name, got[name], want)
    print("statistics after the same staged find, reused == fresh:", got)
    assert got["D"]["lds_bytes"] > got["A"]["lds_bytes"]
    eng.close()


@pytest.mark.parametrize("forget", [True, False], ids=["forgotten", "kept"])
def test_chain_2_the_dictionary_changes_under_the_context(forget):
    """D -> A -> C -> B through one context (reset_nodes, set_dictionary, upload at each arrow; Engine.forget_dictionary called or
    not).  D is only the previous occupant (one k_findn, one staged find); at A, C and B the five forms under seam_check.few_masks,
    explain, on A and B headroom with its limits on the reused context, and at every stop the statistics of a fresh context.

    The stale-row read the class table's reset removes stayed inside the tile image at these shapes even before (fit_core.h
    make_layout; tests/test_reuse.py test_the_stale_class_rows_of_chain_2_stayed_inside_the_tile_image computes it): D's node table
    names signature ids up to 28, a row is at most 128 B, so `off_r1 + sig * row` ends at most 5 632 B into an image of 43 632 B and
    more at A and C, 23 808 B into 83 680 B at B.  What the reset changes here is what the context provisions and reports, which
    the statistics show."""
    eng = Engine(0)
    fig = R.drive_chain2(eng, forget, fresh_factory=lambda: Engine(0))
    print("chain 2 on the device, statistics per stop (reused == fresh):", fig)
    assert fig["D"]["lds_bytes"] > fig["A"]["lds_bytes"] and fig["A"]["nodes"] == 65 and fig["B"]["nsig"] == fig["D"]["nsig"]
    eng.close()


def test_origin_records_and_deltas_across_the_seam():
    """After D -> A, A's table as Engine.download returns it (no origin records): nhdfit_apply_deltas fails with NHDFIT_E_STATE as on
    a fresh context, the mirror untouched (D's origin records used to answer the RESET).  With A's own origin records a RESET and 300
    deltas equal harness.apply_deltas in statuses and all six planes, and the finds behind them equal a fresh context's."""
    eng = Engine(0)
    fig = R.check_origin_across_the_seam(eng, lambda: Engine(0), NhdFitError)
    print("deltas across the seam:", fig)
    assert fig["repack"] >= 1
    eng.close()


def test_gap_uploads_are_refused():
    """nhdfit_upload_nodes with first = n + 1 returns NHDFIT_E_INVAL and leaves the mirror byte-identical; Engine.upload refuses a gap
    and a slice at first > 0 beyond the capacity before any device call."""
    r = S.rung("A")
    pk, table, _ = r.packed()
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table.slice(0, 40), capacity=50)
    before = eng.download()
    one = [np.ascontiguousarray(getattr(table, f)[45:46]) for f in R.PLANES]
    rc = eng.lib.nhdfit_upload_nodes(eng.ctx, 41, 1, *[a.ctypes.data for a in one])
    assert rc == -1 and b"[40,41) are missing" in eng.lib.nhdfit_last_error(eng.ctx)
    assert eng.lib.nhdfit_download_nodes(eng.ctx, 0, 41, None, None, None, None, None, None) == -1      # still 40 nodes
    after = eng.download()
    for f in R.PLANES:
        assert getattr(after, f).tobytes() == getattr(before, f).tobytes(), f
    assert eng.lib.nhdfit_upload_nodes(eng.ctx, 40, 1, *[a.ctypes.data for a in one]) == 0              # appended: taken
    assert eng.lib.nhdfit_download_nodes(eng.ctx, 0, 41, None, None, None, None, None, None) == 0
    eng.close()
    eng = Engine(0)
    R.check_gap_refusals(eng, NhdFitError)
    eng.close()


def test_wide_records_across_the_seam():
    """HipMatcher._full_upload of the 600-node edge cluster on ONE matcher: whole (126 wide records), the fast-layout nodes, those
    whose dictionary fits a block's LDS, the whole cluster again - after each the staged form and the single-launch forms that
    mirror admits, and nhdfit_wide_count against the packer's count.  Then the mirror is cut to one past its last wide record and to
    a count between two wide records: the records read back are the prefix."""
    case = C.big_case()
    m = _matcher()
    placed = {tag: R.check_wide_step(m, case, tag, member) for tag, member in R.wide_steps(case)}
    print("wide records across the seam, pods placed per step:", placed)
    assert all(v >= 100 for v in placed.values())
    cuts = R.check_wide_truncate(m, case)
    print("truncated to (nodes, wide records):", cuts)
    m.engine.close()


def test_a_chain_of_edge_seeds_through_one_matcher():
    """edge_check.check_new_entries over six 14-node edge clusters through ONE matcher, then the same six in reverse: seed 24 holds
    nodes no record holds, seed 22 a STOPPED run, seed 30 is NIC-heavy."""
    m = _matcher()
    tot = {}
    for seed in R.EDGE_SEEDS + R.EDGE_SEEDS[::-1]:
        for k, v in C.check_new_entries(m, seed).items():
            tot[k] = tot.get(k, 0) + v
    print("edge seeds", R.EDGE_SEEDS, "and back:", tot)
    assert tot["unmirrored"] >= 2 and tot["stopped runs"] >= 2 and tot["replicas"] >= 20
    m.engine.close()


def test_reattach_on_one_matcher():
    """check_schedule_one over two seeds on ONE matcher: attach, run, detach, attach the next - on the second seed
    nhdfit_find_commit_counts moves as on a fresh matcher."""
    m = _matcher()
    for seed in (0, 5):
        got = C.check_schedule_one(None, seed, fused_form=True, matcher=m)
        print("ScheduleOne on a matcher in use:", got)
        assert got["pods"] >= 10 and got["placed"] >= 5 and got["fused"] > 0
        m.detach()
    m.engine.close()
