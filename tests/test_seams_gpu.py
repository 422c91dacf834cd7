"""The DEVICE on the seams of its grids (`pytest -m gpu`; tests/seam_check.py has the rungs, the masks, the checks and the derivation of
the form each rung takes; tests/test_seams.py asserts, from the oracles alone, that every mask puts winners on both sides of its
seam).  Everything goes ctypes -> C-ABI on device 0 with a fresh context per case and every mask through it in turn - then one
mask twice and none again, for the mask the small finds keep.  Winners are the C oracle's on the masked view, the verdict matrix is
the C oracle's, every winner's mapping the Python oracle's on that node alone, stages the C stage oracle's, and the bits at and
beyond n of the last chunk's bitmap words are zero.  Nothing here reads the reference tree."""
import numpy as np
import pytest

from nhd_amd import pack
from nhd_amd.engine import Engine
from tests import harness
from tests import seam_check as S

pytestmark = pytest.mark.gpu
ALL = list(S.RUNGS)
FORMS = ["staged", "k_findn", "k_find", "k_find1", "scores only"]


def device_of(r, global_base=0):
    pk, table, reqs = r.packed()
    eng = Engine(0)
    eng.set_dictionary(pk)
    eng.upload(table, global_base=global_base)
    return eng, pk, table, reqs


def counted(eng, field, step, call):
    """call() with the statistic `field` (small_finds / batch_finds) asserted to move by `step`, the other one not at all."""
    before = eng.stats()
    out = call()
    after = eng.stats()
    moved = {f: getattr(after, f) - getattr(before, f) for f in ("small_finds", "batch_finds")}
    assert moved == {"small_finds": step if field == "small_finds" else 0, "batch_finds": step if field == "batch_finds" else 0}, (field, moved)
    return out


def one_by_one(eng, reqs, pods, now, cand):
    """nhdfit_find for one pod at a time: (scores, None, mappings) of the pods `pods`."""
    score, maps = np.zeros(len(pods), np.uint64), np.zeros(len(pods), pack.MAPPING)
    for k, p in enumerate(pods):
        s, _, mp = eng.find(reqs[p:p + 1], now, cand=cand, want_bitmap=False, want_map=True)
        score[k], maps[k] = s[0], mp[0]
    return score, None, maps


def run_form(r, eng, pk, reqs, form, masks=None, base=0):
    """One form of nhdfit_find under the masks, the form that ran asserted where nhdfit_get_stats can tell."""
    small = np.arange(r.n_small)                                  # (the single-launch forms refuse four groups)
    if form == "staged":                                          # the bitmap is asked for: stage, the step's launches, fetch
        pods = np.arange(r.P)
        return S.walk(r, lambda cand: counted(eng, None, 0, lambda: eng.find(reqs, r.now, cand=cand, want_bitmap=True, want_map=True)), pods, form, masks, base)
    if form == "k_findn":                                         # more than a tile, no bitmap: ONE launch, `batch_finds`
        return S.walk(r, lambda cand: counted(eng, "batch_finds", 1, lambda: eng.find(reqs[small], r.now, cand=cand, want_bitmap=False, want_map=True)), small, form, masks, base)
    if form == "k_find":                                          # at most a tile, no bitmap: ONE launch, `small_finds`
        pods = small[:64]
        return S.walk(r, lambda cand: counted(eng, "small_finds", 1, lambda: eng.find(reqs[pods], r.now, cand=cand, want_bitmap=False, want_map=True)), pods, form, masks, base)
    if form == "k_find1":                                         # one pod, the dictionary in a block's LDS: the table-free launch
        assert S.dictionary_fits_a_block(pk)
        pods = small[::3]
        return S.walk(r, lambda cand: counted(eng, "small_finds", len(pods), lambda: one_by_one(eng, reqs, pods, r.now, cand)), pods, form, masks, base)
    assert form == "scores only"                                  # neither bitmap nor mappings: k_findn, then k_find, without their mapping tails
    S.walk(r, lambda cand: counted(eng, "batch_finds", 1, lambda: eng.find(reqs[small], r.now, cand=cand, want_bitmap=False, want_map=False)), small, form, masks, base)
    return S.walk(r, lambda cand: counted(eng, "small_finds", 1, lambda: eng.find(reqs[small[64:128]], r.now, cand=cand, want_bitmap=False, want_map=False)), small[64:128], form, masks, base)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ALL)
def test_find_across_the_seams(name, form):
    r = S.rung(name)
    eng, pk, table, reqs = device_of(r)
    won = run_form(r, eng, pk, reqs, form)
    placed = sum(int((w >= 0).sum()) for _, w in won)
    print(f"rung {name} ({r.n} nodes, {r.chunks} chunks), {form}: {len(won)} masks, {placed} winners checked")
    assert placed >= 10 * len(won)
    eng.close()


@pytest.mark.parametrize("form", FORMS[:4])
def test_find_across_the_seams_with_a_global_base(form):
    """Rung C once more on a context whose nodes start at global index 2**32 + 5: the winners are read as global indices."""
    r = S.rung("C")
    base = 2 ** 32 + 5
    eng, pk, table, reqs = device_of(r, global_base=base)
    won = run_form(r, eng, pk, reqs, form, masks=S.few_masks(r), base=base)
    assert sum(int((w >= 0).sum()) for _, w in won) >= 100
    eng.close()


@pytest.mark.parametrize("P", S.POD_AXIS)
def test_the_pod_axis(P):
    """The first P pods of the pod-axis rung through the staged form, the single launch their count takes (k_find1 for one, k_find up
    to a tile, k_findn beyond; more than 512: its copy path) and explain (16 pods per block)."""
    r = S.pod_axis_rung()
    eng, pk, table, reqs = device_of(r)
    pods, masks = np.arange(P), S.few_masks(r)
    S.walk(r, lambda cand: eng.find(reqs[:P], r.now, cand=cand, want_bitmap=True, want_map=True), pods, f"staged, {P} pods", masks)
    field = "small_finds" if P <= 64 else "batch_finds"
    S.walk(r, lambda cand: counted(eng, field, 1, lambda: eng.find(reqs[:P], r.now, cand=cand, want_bitmap=False, want_map=True)), pods, f"single launch, {P} pods", masks)
    for label, keep in masks[2:4]:
        counts, stages = eng.explain(reqs[:P], r.now, cand=S.mask_words(keep), per_node=True)
        want_c, want_s = r.cl.explain(r.opods[:P], r.now, cand=keep, per_node=True, threads=S.coracle.usable_cpus())
        assert np.array_equal(stages, want_s) and np.array_equal(counts, want_c), (P, label)
    eng.close()


@pytest.mark.parametrize("name", ["E", "F"])
def test_many_pods_across_the_seams(name):
    """900 pods (15 tiles) on E and F: tiles * ceil(chunks / 32) >= 256, so the step runs as k_step<512> - on F the only form that cuts
    the node axis into eighths, on E the few-long-blocks form - and k_findn copies its requests (more than 512 pods).  k_findn under
    five masks; the unmasked pipelined form (stage, 1 / 3 / 9 steps, fetch with the verdict matrix)."""
    r = S.rung(name, S.MANY_PODS)
    assert r.P == S.MANY_PODS and ((r.P + 63) // 64) * ((r.chunks + 31) // 32) >= 256
    eng, pk, table, reqs = device_of(r)
    pods = np.arange(r.P)
    won = S.walk(r, lambda cand: counted(eng, "batch_finds", 1, lambda: eng.find(reqs, r.now, cand=cand, want_bitmap=False, want_map=True)), pods, "k_findn, 900 pods", S.few_masks(r))
    assert sum(int((w >= 0).sum()) for _, w in won) >= 2000
    for steps in (1, 3, 9):
        eng.stage(reqs)
        for _ in range(steps):
            eng.enqueue(r.now)
        score, bm, maps = eng.fetch(want_bitmap=True, want_map=True)
        S.check_find(r, pods, None, score, bm, maps, f"rung {name}, {steps} pipelined steps")
    # the staged form under the masks: k_step<512> with a candidate mask
    S.walk(r, lambda cand: eng.find(reqs, r.now, cand=cand, want_bitmap=True, want_map=True), pods, "staged, 900 pods", S.few_masks(r))
    eng.close()


@pytest.mark.parametrize("name", ALL)
def test_find_commit_across_the_seams(name):
    """nhdfit_find_commit under four masks (none, the island, the first and the last straddle), each on a fresh context, for the first
    pod the oracle places at or beyond the mask's seam: score and mapping against the oracles, the ONE launch (k_find1_commit)
    asserted by its counter, placement record and the committed node's records against the host twin's commit."""
    r = S.rung(name)
    pk, table, reqs = r.packed()
    assert S.dictionary_fits_a_block(pk)
    masks = dict(r.masks())
    far = r.island()[1]
    for label, beyond in (("none", 0), ("island", far), ("straddle 1", 64), (f"straddle {r.chunks - 1}", 64 * (r.chunks - 1))):
        keep = masks[label]
        want = r.oracle_winners(keep)[:r.n_small]
        p = int(np.flatnonzero(want >= beyond)[0])
        eng, _, _, _ = device_of(r)
        score, mp, place, done = eng.find_commit(reqs[p], r.now, r.now, cand=None if keep is None else S.mask_words(keep))
        assert eng.find_commit_counts() == (1, 0), (label, "the one-launch form did not run")
        S.check_find(r, [p], keep, np.array([score], np.uint64), None, np.array([mp]), f"rung {name}, find_commit, mask {label}")
        assert done and int(place["status"]) == pack.COMMIT_OK, label
        twin = harness.HarnessEngine(0)
        twin.set_dictionary(pk)
        twin.upload(table)
        node = int(want[p])
        assert twin.commit(node, reqs[p], mp, r.now).tobytes() == place.tobytes(), label
        got, ref = eng.download(node, 1), twin.download(node, 1)
        for f in ("p0", "p1", "p2", "p3", "p4", "detail"):
            assert getattr(got, f).tobytes() == getattr(ref, f).tobytes(), (label, f)
        # the mirror behind the commit: the next find sees the node as the twin does
        s2, b2, _ = eng.find(reqs[:r.n_small], r.now + 100.0, cand=None if keep is None else S.mask_words(keep), want_bitmap=True, want_map=False)
        t2, tb, _ = twin.find(reqs[:r.n_small], r.now + 100.0, cand=None if keep is None else S.mask_words(keep), want_bitmap=True, want_map=False)
        assert np.array_equal(s2, t2) and np.array_equal(b2, tb), label
        eng.close()


@pytest.mark.parametrize("name", list("ABCD"))
def test_the_general_path_across_the_seams(name):
    """nhdfit_big_find for the same pods as big requests (k_big_eval over every node, k_big_map for the winners)."""
    r = S.rung(name)
    eng, pk, table, reqs = device_of(r)
    pods = np.arange(r.P)
    bigs = r.big_reqs(pk, pods)
    eng.set_dictionary(pk)
    won = S.walk(r, lambda cand: S.as_find(eng.big_find(bigs, r.now, cand=cand)), pods, "general path")
    assert sum(int((w >= 0).sum()) for _, w in won) >= 10 * len(won)
    eng.close()


@pytest.mark.parametrize("name", ALL)
def test_explain_across_the_seams(name):
    r = S.rung(name)
    eng, pk, table, reqs = device_of(r)
    S.check_explain(r, eng, reqs, S.explain_masks(r))
    eng.close()


@pytest.mark.parametrize("name", list("AB"))
def test_headroom_across_the_seams(name):
    """nhdfit_headroom and nhdfit_headroom_limits for four templates (one to four groups) under three masks: the one-node last chunk
    of rungs A and B alone, behind a straddle, and beside the island; nodes outside the mask read 0."""
    from tests.headroom_check import four_templates
    r = S.rung(name)
    got = S.check_headroom(r, lambda: Engine(0), four_templates(r.cfg), S.headroom_masks(r))
    print(f"rung {name}: replicas by the oracle under each mask {got}")
    assert got["island"] >= 20 and got["only the last node"] >= 1
