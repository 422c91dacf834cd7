"""Host builds of nhdfit_candidates_big (TEST INFRASTRUCTURE, see candidates_big_twin.cpp and big_candidates_scan_emul.cpp), built the
way candidates_twin.py builds its own, and an engine that answers candidates_big() with the scalar one."""
import ctypes
import os
import subprocess

import numpy as np

from nhd_amd import pack
from nhd_amd._lib import NhdFitError
from tests import harness
from tests.harness import candidates_general_twin as cgt
from tests.harness import candidates_twin as ct
from tests.harness import headroom_twin

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "candidates_big_twin.cpp")
SO = os.path.join(HERE, "_candidates_big_twin.so")
SCAN_SRC = os.path.join(HERE, "big_candidates_scan_emul.cpp")
SCAN_SO = os.path.join(HERE, "_big_candidates_scan_emul.so")
SCAN_INC = os.path.join(HERE, "_wave_big_candidates_block.inc")
_FROM, _TO = "// ---- the scan's records and the two-range pick with the wavefront's lanes", "// ---- the launches"
_lib = None
_scan = None
_p = ct._p


def lib():
    """The scalar twin (hx_candidates_big) and the group entry's merge for the big entry (hx_merge_big_candidate_lists)."""
    global _lib
    if _lib is None:
        if headroom_twin._stale(SO, [SRC] + headroom_twin._headers()):
            tmp = f"{SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = ctypes.CDLL(SO)
        _lib.hx_candidates_big.restype = ctypes.c_int
        _lib.hx_merge_big_candidate_lists.restype = None
    return _lib


def scan_lib():
    """The scan's record logic and the two-range pick on emulated lanes (we_big_cand_scan_pick): the section of
    big_candidates_kernel.h between its two headings, cut out unmodified, behind candidates_kernel.h's pick."""
    global _scan
    if _scan is None:
        ct.pick_lib()                                       # (wave_emul.cpp's own .inc files and candidates_kernel.h's)
        kernel = os.path.join(ct.CSRC, "big_candidates_kernel.h")
        if headroom_twin._stale(SCAN_SO, [SCAN_SRC, harness.WAVE_SRC, harness.WAVE_SO, ct.PICK_SO, kernel] + headroom_twin._headers()):
            harness.cut_section(kernel, _FROM, _TO, "big_cand_pick2", SCAN_INC)
            tmp = f"{SCAN_SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", SCAN_SRC, "-o", tmp])
            os.replace(tmp, SCAN_SO)
        _scan = ctypes.CDLL(SCAN_SO)
        _scan.we_big_cand_scan_pick.restype = ctypes.c_int
        _scan.we_big_cand_rec_words.restype = ctypes.c_uint32
        _scan.we_big_cand_pref_bit.restype = ctypes.c_uint32
    return _scan


def candidates_big(packer, table, wide, share, reqs, now, k, cand=None, global_base=0, budget=0):
    """(sums [P] pack.CANDIDATES_SUM, entries [P][k] pack.BIG_CANDIDATE) of the scalar host build for the planes of `table` and the
    wide records `wide` (`share`: None, or their nhdfit_wide_share records in the same order).  budget: 0, or the NIC search steps a
    (pod, node) pair may take.  Raises what the library's entry returns: NhdFitError(-6)."""
    u32 = ctypes.c_uint32
    reqs = np.ascontiguousarray(reqs, dtype=pack.BIG_REQ)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    if share is not None:
        share = np.ascontiguousarray(share, dtype=pack.WIDE_SHARE).reshape(-1)
        assert len(share) == len(wide)
    P, n = len(reqs), table.n
    sums, entries = np.zeros(P, pack.CANDIDATES_SUM), np.zeros((P, int(k)), pack.BIG_CANDIDATE)
    caps = harness._caps(packer)
    planes = [np.ascontiguousarray(getattr(table, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
    cand = None if cand is None else np.ascontiguousarray(cand, dtype=np.uint64)
    rc = lib().hx_candidates_big(*[_p(x) for x in planes], u32(n), ctypes.c_uint64(global_base), _p(wide) if len(wide) else None, u32(len(wide)),
                                 _p(share), _p(reqs), u32(P), ctypes.c_double(now), _p(caps), _p(cand), u32(int(k)), u32(int(budget)), _p(sums),
                                 _p(entries))
    if rc == -3:
        raise NhdFitError(-6, "a big request's NIC stage ran out of search budget on some node")
    if rc:
        raise NhdFitError(-6, "the set model of a big request's mapping outgrew its table")
    return sums, entries


def merge(parts, k):
    """The group entry's merge (candidates_merge.h, as nhdfit_group_candidates_big runs it shard by shard) over `parts`, a list of
    (sums, entries) per shard: (sums, entries, owner)."""
    P = len(parts[0][0])
    sums, entries, owner = np.zeros(P, pack.CANDIDATES_SUM), np.zeros((P, k), pack.BIG_CANDIDATE), np.full((P, k), -1, np.int32)
    for shard, (s, e) in enumerate(parts):
        lib().hx_merge_big_candidate_lists(_p(sums), _p(entries), _p(owner), _p(np.ascontiguousarray(s)), _p(np.ascontiguousarray(e)),
                                           ctypes.c_uint32(P), ctypes.c_uint32(k), ctypes.c_int32(shard))
    return sums, entries, owner


def scan_pick(planes, wide, nb_planes, nb_wide, k, global_base=0):
    """k_big_cand_scan's record logic and k_big_cand_pick's two-range pick on emulated lanes.  `planes`, `wide`: per unit of either
    range (ok, preferred, node index), in unit order; nb_planes / nb_wide blocks share out each range's 64-unit chunks.
    Returns (list of index | preferred bit, feasible, preferred, records [blocks][words])."""
    L = scan_lib()
    words = int(L.we_big_cand_rec_words(ctypes.c_uint32(k)))
    cols = []
    for units in (planes, wide):
        cols.append((np.ascontiguousarray([u[0] for u in units], dtype=np.uint8), np.ascontiguousarray([u[1] for u in units], dtype=np.uint8),
                     np.ascontiguousarray([u[2] for u in units], dtype=np.uint32)))
    ptrs = lambda j: (ctypes.c_void_p * 2)(*[c[j].ctypes.data if len(c[j]) else None for c in cols])      # noqa: E731
    units = (ctypes.c_uint32 * 2)(len(planes), len(wide))
    nb = (ctypes.c_uint32 * 2)(nb_planes, nb_wide)
    recs = np.zeros((nb_planes + nb_wide, words), np.uint32)
    out = np.full(64, 0xFFFFFFFF, np.uint32)
    sums = np.zeros(2, np.uint32)
    n = L.we_big_cand_scan_pick(ptrs(0), ptrs(1), ptrs(2), units, nb, ctypes.c_uint32(k), ctypes.c_uint64(global_base), _p(recs), _p(out), _p(sums))
    assert n >= 0, "the emulated lanes disagreed"
    assert (out[n:] == 0xFFFFFFFF).all(), "the pick stored beyond its count"
    return out[:n], int(sums[0]), int(sums[1]), recs


class CandidatesBigHarnessEngine(cgt.CandidatesGeneralHarnessEngine):
    """CandidatesGeneralHarnessEngine plus candidates_big(), as nhd_amd.engine.Engine.candidates_big answers it.  `nic_budget` (an
    attribute, as HarnessEngine.big_find reads it): the NIC search steps a (pod, node) pair may take."""

    def candidates_big(self, reqs, now, k, cand=None):
        return candidates_big(self.packer, self.table, self._wide_records(), self._share_records(), reqs, now, k, cand=cand,
                              global_base=self.global_base, budget=getattr(self, "nic_budget", 0))
