"""The merge of the shards' headroom summary records is stated twice: in C (nhd_amd/csrc/headroom_merge.h, what libnhdfit.so's
group entries run) and in Python (engine._add_headroom_sums, what a GroupEngine of harness engines runs).  This holds the two to
each other on the host."""
import ctypes
import itertools

import numpy as np

from nhd_amd import engine, pack
from tests.harness import headroom_twin

WIDE = pack.HEADROOM_FORM_WIDE


def _records():
    """Summary records that cover what a shard can hand in: every form with and without the wide bit, an all-zero part (an empty
    shard), small and large maxima, counts at the top of their 32 bits and a replica count beyond them."""
    recs = [(0, 0, 0, 0, 0, 0, 0)]
    for form in (0, pack.HEADROOM_FORM_WAVE, pack.HEADROOM_FORM_GENERIC):
        for wide in (0, WIDE):
            recs.append((1000 + form, 7, 3 + 500 * form, 2, 1, 5, form | wide))
    recs.append((2 ** 32 + 12345, 2 ** 32 - 2, 16383, 2 ** 32 - 3, 2 ** 32 - 1, 2 ** 32 - 4, pack.HEADROOM_FORM_WAVE))
    recs.append((2 ** 40, 1, 1, 0, 0, 2, pack.HEADROOM_FORM_GENERIC | WIDE))
    return np.array(recs, dtype=pack.HEADROOM_SUM)


def _c_merge(sums, part):
    p = ctypes.c_void_p
    headroom_twin.lib().hx_merge_headroom_sums(p(sums.ctypes.data), p(part.ctypes.data), ctypes.c_uint32(len(sums)))


def test_python_merge_of_headroom_sums_is_the_c_merge():
    """Every ordered pair of the records - running value on one side, a shard's part on the other, so each form, the zero record
    and the smaller and the larger maximum meet on either side - and then three parts in a row into one running value, merged by
    headroom_merge.h's merge_headroom_sums (through the host twin) and by engine._add_headroom_sums: the same records, field by
    field.  (32-bit counts that add up beyond 2^32 wrap in both; the replica count has 64 bits.)
    Until a hardware run with more than one device exists this is the only place the C rule meets two shards: the one-shard group
    of the GPU tests merges nothing, and their several-shard groups are built from engines and merged in Python."""
    recs = _records()
    pairs = list(itertools.product(range(len(recs)), repeat=2))
    running, part = recs[[a for a, _ in pairs]], recs[[b for _, b in pairs]]
    got_c, got_py = running.copy(), running.copy()
    _c_merge(got_c, part)
    engine._add_headroom_sums(got_py, part)
    for f in pack.HEADROOM_SUM.names:
        assert (got_c[f] == got_py[f]).all(), (f, [pairs[i] for i in np.flatnonzero(got_c[f] != got_py[f])])
    # what the rule says, on a pair whose answer is plain to see: counts add, the maxima take the larger, the wide bit is ORed
    a, b = recs[2], recs[5]                                             # the wide bit alone, 1000 replicas; GENERIC, 1002
    i = pairs.index((2, 5))
    assert got_c[i]["replicas"] == int(a["replicas"]) + int(b["replicas"]) and got_c[i]["not_evaluated"] == 10
    assert got_c[i]["max_on_one_node"] == max(a["max_on_one_node"], b["max_on_one_node"])
    assert got_c[i]["form"] == pack.HEADROOM_FORM_GENERIC | WIDE
    # three shards: from zero, as the group entries start
    for trio in itertools.permutations(range(len(recs)), 3):
        total_c, total_py = np.zeros(1, pack.HEADROOM_SUM), np.zeros(1, pack.HEADROOM_SUM)
        for k in trio:
            _c_merge(total_c, recs[k:k + 1].copy())
            engine._add_headroom_sums(total_py, recs[k:k + 1])
        assert total_c.tobytes() == total_py.tobytes(), trio
