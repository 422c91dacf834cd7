"""Host builds of nhdfit_candidates (TEST INFRASTRUCTURE, see candidates_twin.cpp and candidates_pick_emul.cpp), built the way
headroom_twin builds its own, and an engine that answers candidates() with the scalar one."""
import ctypes
import os
import subprocess

import numpy as np

from nhd_amd import pack
from tests import harness
from tests.harness import explain_twin, headroom_twin

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "nhd_amd", "csrc")
SRC = os.path.join(HERE, "candidates_twin.cpp")
SO = os.path.join(HERE, "_candidates_twin.so")
PICK_SRC = os.path.join(HERE, "candidates_pick_emul.cpp")
PICK_SO = os.path.join(HERE, "_candidates_pick_emul.so")
PICK_INC = os.path.join(HERE, "_wave_candidates_block.inc")
_FROM, _TO = "// ---- the pick with the wavefront's lanes", "// ---- the launch"
_lib = None
_pick = None


def lib():
    """The scalar twin (hx_candidates) and the group entry's merge of the shards' lists (hx_merge_candidate_lists)."""
    global _lib
    if _lib is None:
        if headroom_twin._stale(SO, [SRC] + headroom_twin._headers()):
            tmp = f"{SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = ctypes.CDLL(SO)
        _lib.hx_candidates.restype = ctypes.c_int
        _lib.hx_merge_candidate_lists.restype = None
    return _lib


def pick_lib():
    """The kernel's pick on emulated lanes (we_cand_pick): the section of candidates_kernel.h between its two headings, cut out
    unmodified, on the wavefront emulation harness.wave_lib() builds its own sections around."""
    global _pick
    if _pick is None:
        harness.wave_lib()                                  # (wave_emul.cpp includes the sections it cuts out: its .inc files)
        kernel = os.path.join(CSRC, "candidates_kernel.h")
        if headroom_twin._stale(PICK_SO, [PICK_SRC, harness.WAVE_SRC, harness.WAVE_SO, kernel] + headroom_twin._headers()):
            harness.cut_section(kernel, _FROM, _TO, "cand_pick_wave", PICK_INC)
            tmp = f"{PICK_SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", PICK_SRC, "-o", tmp])
            os.replace(tmp, PICK_SO)
        _pick = ctypes.CDLL(PICK_SO)
        _pick.we_cand_pick.restype = ctypes.c_int
        _pick.we_cand_rec_words.restype = ctypes.c_uint32
        _pick.we_cand_pref_bit.restype = ctypes.c_uint32
    return _pick


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def candidates(packer, table, wide, reqs, now, k, cand=None, global_base=0):
    """(sums [P] pack.CANDIDATES_SUM, entries [P][k] pack.CANDIDATE) of the scalar host build for the planes of `table`; candidates
    among the wide records `wide` are counted, not listed."""
    u32 = ctypes.c_uint32
    reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    P, n = len(reqs), table.n
    sums, entries = np.zeros(P, pack.CANDIDATES_SUM), np.zeros((P, int(k)), pack.CANDIDATE)
    caps, sig_off, pool_off, glimit, cc, ncls, nsig, npools, ncc = packer.dictionary_arrays()
    gs = packer.group_set_array()
    planes = [np.ascontiguousarray(getattr(table, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
    cand = None if cand is None else np.ascontiguousarray(cand, dtype=np.uint64)
    rc = lib().hx_candidates(*[_p(x) for x in planes], u32(n), ctypes.c_uint64(global_base), _p(wide) if len(wide) else None, u32(len(wide)),
                             _p(reqs), u32(P), ctypes.c_double(now), u32(packer.max_cores_per_numa), u32(packer.max_gpus_per_numa), _p(gs),
                             u32(len(packer.group_sets)), _p(caps), u32(ncls), _p(sig_off), u32(nsig), _p(pool_off), _p(glimit), _p(cc), _p(cand),
                             u32(int(k)), _p(sums), _p(entries))
    assert rc == 0, f"{rc}: the dictionary's stream does not fit"
    return sums, entries


def merge(parts, k):
    """The group entry's merge (candidates_merge.h, as nhdfit_group_candidates runs it shard by shard) over `parts`, a list of
    (sums, entries) per shard: (sums, entries, owner)."""
    P = len(parts[0][0])
    sums, entries, owner = np.zeros(P, pack.CANDIDATES_SUM), np.zeros((P, k), pack.CANDIDATE), np.full((P, k), -1, np.int32)
    for shard, (s, e) in enumerate(parts):
        lib().hx_merge_candidate_lists(_p(sums), _p(entries), _p(owner), _p(np.ascontiguousarray(s)), _p(np.ascontiguousarray(e)),
                                       ctypes.c_uint32(P), ctypes.c_uint32(k), ctypes.c_int32(shard))
    return sums, entries, owner


def pick(block_records, k):
    """cand_pick_wave on emulated lanes over the blocks' records - per block (fits entries, preferred entries) as the scan posts
    them (local index | preferred bit; plain indices): the list of local index | preferred bit."""
    L = pick_lib()
    words = int(L.we_cand_rec_words(ctypes.c_uint32(k)))
    recs = np.zeros((len(block_records), words), np.uint32)
    for b, (fits, pref) in enumerate(block_records):
        recs[b, 0], recs[b, 1] = len(fits), len(pref)
        recs[b, 4:4 + len(fits)] = fits
        recs[b, 4 + k:4 + k + len(pref)] = pref
    out = np.full(64, 0xFFFFFFFF, np.uint32)
    n = L.we_cand_pick(_p(recs), ctypes.c_uint32(len(block_records)), ctypes.c_uint32(k), _p(out))
    assert n >= 0, "the emulated lanes disagreed"
    assert (out[n:] == 0xFFFFFFFF).all(), "the pick stored beyond its count"
    return out[:n]


class CandidatesHarnessEngine(explain_twin.ExplainHarnessEngine):
    """ExplainHarnessEngine (HipMatcher's composed form asks explain()) plus candidates(), as nhd_amd.engine.Engine.candidates
    answers it."""

    def candidates(self, reqs, now, k, cand=None):
        return candidates(self.packer, self.table, self._wide_records(), reqs, now, k, cand=cand, global_base=self.global_base)
