"""The rungs, masks and checks of tests/seam_check.py on the CPU: the conditions under which the checks say something, asserted from the
oracles alone (winners on both sides of every straddled boundary, pods that jump from the island to the far node, a feasible pair
in every chunk), the rung inputs pinned by hash, and every check on the host twins (tests/harness: find with a candidate mask and
with the verdict matrix, the general path for the same pods as big requests, explain, headroom with its limits) for rungs A..D, the
pod-axis rungs, and E and F at 130 pods.  tests/test_seams_gpu.py holds the device to the same oracles under the same masks."""
import numpy as np
import pytest

from tests import seam_check as S
from tests.harness.explain_twin import ExplainHarnessEngine
from tests.harness.headroom_limit_twin import HeadroomLimitHarnessEngine

# sha256 of each rung's cluster columns and pod specs (Rung.input_hash): the names stand for the same inputs on every machine
HASHES = {"A": "0d2cbf7708b987da402465a09b593e455fdaba849fe4c3469f4222a627d6b883",
          "B": "05841c2fb75de1a2c57fe1a393f4a86a3227af166345e513b13b21fb2c09f671",
          "C": "0e4a28c3af0c641d61dbbc5cd8c80906757613435f712fc7f407b3a08a3b8040",
          "D": "00ddb3ff10b1471c43e17c67046750b25428118f52c90ab81954022636cea647",
          "E": "9c9284a6c65c9bd3cc37b3f8171959ff0d172f64e69f124441bbcdc30702ead1",
          "F": "e3ca38a78e27d44bc9af06d55c1b11044ed05abf3f9d8356d1c2cd74f7cda112"}

# By the C oracle alone, per rung: the chunk boundaries of its straddle masks with (pods that win in front of node 64 c, pods that win
# at or beyond it), and (pods that jump from the island to the far node, pods that win inside the island)
FIGURES = {
    "A": ({1: (57, 15)}, (15, 119)),
    "B": ({1: (37, 99), 2: (21, 115), 3: (2, 134), 4: (4, 132), 5: (18, 118), 6: (11, 125), 7: (2, 133), 8: (11, 1)}, (1, 135)),
    "C": ({1: (111, 25), 32: (96, 25), 8: (24, 112), 16: (111, 25), 24: (19, 117), 31: (103, 33), 3: (111, 25), 6: (73, 63), 15: (42, 94),
           26: (110, 26), 27: (96, 40), 18: (110, 26)}, (25, 111)),
    "D": ({1: (2, 134), 128: (14, 48), 8: (18, 118), 16: (2, 134), 32: (10, 126), 64: (26, 110), 96: (2, 134), 72: (17, 119), 65: (33, 103),
           62: (8, 128), 58: (9, 127), 55: (26, 110)}, (1, 132)),
    "E": ({1: (86, 50), 584: (16, 120), 73: (115, 21), 36: (28, 108), 511: (14, 122), 548: (119, 17), 292: (9, 127), 329: (16, 120),
           219: (104, 32), 182: (92, 44), 512: (16, 120), 497: (99, 37)}, (16, 120)),
    "F": ({1: (106, 30), 640: (83, 51), 80: (115, 21), 40: (99, 37), 560: (112, 24), 600: (67, 69), 360: (16, 120), 240: (116, 20),
           200: (119, 17), 400: (3, 133), 271: (12, 124), 37: (16, 120)}, (16, 120))}


# The chunk boundaries of each rung's straddle masks, in the order of its mask list (Rung.boundaries), and the cuts and seeded
# boundaries it passes over because node 64 c - 1 fits no pod there: if workload/synth.py or the oracle ever changes, this says so
# before the figures above do
CUTS = {"A": [1], "B": [1, 2, 3, 4, 5, 6, 7, 8],
        "C": [1, 32, 8, 16, 24, 31, 3, 6, 15, 26, 27, 18],
        "D": [1, 128, 8, 16, 32, 64, 96, 72, 65, 62, 58, 55],
        "E": [1, 584, 73, 36, 511, 548, 292, 329, 219, 182, 512, 497],
        "F": [1, 640, 80, 40, 560, 600, 360, 240, 200, 400, 271, 37]}
PASSED_OVER = {"C": [12], "D": [38], "F": [320]}


class TwinEngine(HeadroomLimitHarnessEngine, ExplainHarnessEngine):
    pass


def twin_of(r, global_base=0):
    pk, table, reqs = r.packed()
    eng = TwinEngine(0)
    eng.set_dictionary(pk)
    eng.upload(table, global_base=global_base)
    return eng, pk, reqs


@pytest.mark.parametrize("name", list(S.RUNGS))
def test_the_rungs_are_the_same_inputs_and_sit_on_their_seams(name):
    r = S.rung(name)
    assert r.input_hash() == HASHES[name]
    chunks = {"A": 2, "B": 9, "C": 33, "D": 129, "E": 585, "F": 641}[name]
    assert r.chunks == chunks and r.n % 64 != 0 and r.P == S.PODS + S.FOURS
    # build_items' small-shard rule for a batch of all three row widths: 3 584 bytes of records per chunk against 2 MiB
    assert sorted(set(r.G.tolist())) == [1, 2, 3, 4]
    assert (chunks * 3584 <= 2 << 20) == (name != "F") and (name != "E" or (chunks + 1) * 3584 > 2 << 20)
    if name == "F":
        assert chunks % 8 and chunks % 16 and chunks >= 256
    labels = [label for label, _ in r.masks()]
    assert len(labels) <= S.MAX_MASKS and labels[:4] == ["none", "all zero", "only the last node", "island"]
    assert f"straddle {chunks - 1}" in labels and "straddle 1" in labels
    for label, keep in r.masks():
        if keep is not None:
            words = S.mask_words(keep)
            assert words.shape == (chunks,) and int(words[-1]) >> (r.n % 64) == (1 << (64 - r.n % 64)) - 1      # the padding bits are set


@pytest.mark.parametrize("name", list(S.RUNGS))
def test_the_oracle_alone_puts_winners_on_both_sides_of_every_seam(name):
    r = S.rung(name)
    assert r.boundaries() == CUTS[name]
    for c in PASSED_OVER.get(name, []):
        assert not r.straddles_both_sides(c), c
    straddle, island = r.straddle_figures(), r.island_figures()
    print(f"rung {name}: straddle {straddle}, island {island}")
    assert (straddle, island) == FIGURES[name]
    assert all(front >= 1 and beyond >= 1 for front, beyond in straddle.values()), straddle
    assert island[0] >= 1, island
    assert r.chunks_without_a_pair() == []
    assert (r.oracle_winners(dict(r.masks())["all zero"]) == -1).all()
    assert (r.oracle_winners(dict(r.masks())["only the last node"]) >= 0).any()          # the last chunk's only live lanes decide something
    if r.chunks > 9:
        cuts = r.boundaries()
        assert len(cuts) == S.MAX_MASKS - 4
        if r.chunks > 160:
            eighths = {r.chunks * k // 8 for k in range(1, 8)}
            sixteenths = {r.chunks * k // 16 for k in range(1, 16, 2)}
            assert len(eighths & set(cuts)) >= 3 and len(sixteenths & set(cuts)) >= 3, cuts
        else:
            assert {8, 16, 32} <= set(cuts), cuts
    # unmasked, the winners never leave the first chunk or two: the reason for the masks
    assert r.oracle_winners(None).max() < 128


@pytest.mark.parametrize("name", ["E", "F"])
def test_the_oracle_alone_puts_many_pods_on_both_sides(name):
    """E and F with 900 pods under the five masks their device case uses (the masks of the 130-pod rung: the same cluster)."""
    r = S.rung(name, S.MANY_PODS)
    assert r.P == S.MANY_PODS and [label for label, _ in r.masks()] == [label for label, _ in S.rung(name).masks()]
    for label, keep in S.few_masks(r):
        w = r.oracle_winners(keep)
        if label.startswith("straddle"):
            c = int(label.split()[1])
            assert ((w >= 0) & (w < 64 * c)).sum() >= 10 and (w >= 64 * c).sum() >= 10, (label, c)
        if label == "island":
            assert (w == r.island()[1]).sum() >= 10


def test_the_pod_axis_rung_is_rung_c_with_its_own_pods():
    """(synth.make_pods draws the group counts of all its pods first: the first 130 of 513 are not the 130 of rung C.)"""
    r, c = S.pod_axis_rung(), S.rung("C")
    assert r.n == c.n and r.P == 513 and r.spec.core_used.tobytes() == c.spec.core_used.tobytes() and (r.G <= 3).all()
    fig = r.straddle_figures()
    print(f"pod-axis rung: straddle {fig}, island {r.island_figures()}")
    assert r.island_figures()[0] >= 1
    assert all(front >= 1 and beyond >= 1 for front, beyond in fig.values()), fig


@pytest.mark.parametrize("name", list(S.RUNGS))
def test_find_on_the_host_twin(name):
    """The staged form's answer (verdict matrix, winners, mappings) and the scores-only form under every mask, the same mask twice
    and none again; on rungs A..D the same pods as big requests through the general path."""
    r = S.rung(name)
    eng, pk, reqs = twin_of(r)
    pods = np.arange(r.P)
    # (E and F: five masks - under all of them the twin's sweeps and the oracle's mappings take eight seconds a rung)
    S.walk(r, lambda cand: eng.find(reqs, r.now, cand=cand, want_bitmap=True, want_map=True), pods, "twin, staged", masks=S.few_masks(r) if name in "EF" else None)
    S.walk(r, lambda cand: eng.find(reqs, r.now, cand=cand, want_bitmap=False, want_map=False), pods, "twin, scores only", masks=S.few_masks(r))
    if name in "ABCD":
        bigs = r.big_reqs(pk, pods)
        S.walk(r, lambda cand: S.as_find(eng.big_find(bigs, r.now, cand=cand)), pods, "twin, general path", masks=S.few_masks(r))


def test_find_on_the_host_twin_with_a_global_base():
    r = S.rung("C")
    base = 2 ** 32 + 5
    eng, pk, reqs = twin_of(r, global_base=base)
    S.walk(r, lambda cand: eng.find(reqs, r.now, cand=cand, want_bitmap=True, want_map=True), np.arange(r.P), "twin, global base", masks=S.few_masks(r), base=base)


@pytest.mark.parametrize("P", S.POD_AXIS)
def test_the_pod_axis_on_the_host_twin(P):
    r = S.pod_axis_rung()
    eng, pk, reqs = twin_of(r)
    pods = np.arange(P)
    S.walk(r, lambda cand: eng.find(reqs[:P], r.now, cand=cand, want_bitmap=True, want_map=True), pods, f"twin, {P} pods", masks=S.few_masks(r))


@pytest.mark.parametrize("name", list("ABCD"))
def test_explain_on_the_host_twin(name):
    r = S.rung(name)
    eng, pk, reqs = twin_of(r)
    S.check_explain(r, eng, reqs, S.explain_masks(r))


@pytest.mark.parametrize("name", list("AB"))
def test_headroom_on_the_host_twin(name):
    from tests.headroom_check import four_templates
    r = S.rung(name)
    got = S.check_headroom(r, lambda: TwinEngine(0), four_templates(r.cfg), S.headroom_masks(r))
    print(f"rung {name}: replicas by the oracle under each mask {got}")
    assert got["island"] >= 20 and got["only the last node"] >= 1
