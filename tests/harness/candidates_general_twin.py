"""Host builds of nhdfit_candidates_general (TEST INFRASTRUCTURE, see candidates_general_twin.cpp and
wide_candidates_wave_emul.cpp), built the way candidates_twin.py builds its own, and an engine that answers
candidates(general=True) with the scalar one."""
import ctypes
import os
import subprocess

import numpy as np

from nhd_amd import pack
from tests import harness
from tests.harness import candidates_twin as ct
from tests.harness import headroom_general_twin as hg
from tests.harness import headroom_twin

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "candidates_general_twin.cpp")
SO = os.path.join(HERE, "_candidates_general_twin.so")
WAVE_SRC = os.path.join(HERE, "wide_candidates_wave_emul.cpp")
WAVE_SO = os.path.join(HERE, "_wide_candidates_wave_emul.so")
WAVE_INC = os.path.join(HERE, "_wave_wide_candidates_block.inc")
_FROM, _TO = "// ---- one wide record's mapping with the wavefront's lanes", "// ---- the launches"
_lib = None
_wave = None
_p = ct._p


def lib():
    """The scalar twin (hx_candidates_general) and the merge rule k_wide_cand_map's blocks run (hx_cand_merged_entry)."""
    global _lib
    if _lib is None:
        if headroom_twin._stale(SO, [SRC, ct.SRC] + headroom_twin._headers()):
            tmp = f"{SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = ctypes.CDLL(SO)
        _lib.hx_candidates_general.restype = ctypes.c_int
        _lib.hx_cand_merged_entry.restype = ctypes.c_int
    return _lib


def wave_lib():
    """The kernel's mapping routine on emulated lanes (we_wide_cand_map): the section of wide_candidates_kernel.h between its two
    headings, cut out unmodified, behind the section of wide_room_kernel.h headroom_general_twin.wave_lib() cuts out."""
    global _wave
    if _wave is None:
        hg.wave_lib()                                       # (wave_emul.cpp's own .inc files and wide_room_kernel.h's)
        kernel = os.path.join(ct.CSRC, "wide_candidates_kernel.h")
        room = os.path.join(ct.CSRC, "wide_room_kernel.h")
        if headroom_twin._stale(WAVE_SO, [WAVE_SRC, harness.WAVE_SRC, harness.WAVE_SO, hg.WAVE_SO, kernel, room] + headroom_twin._headers()):
            harness.cut_section(kernel, _FROM, _TO, "wide_map_on_state_wave", WAVE_INC)
            tmp = f"{WAVE_SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", WAVE_SRC, "-o", tmp])
            os.replace(tmp, WAVE_SO)
        _wave = ctypes.CDLL(WAVE_SO)
        _wave.we_wide_cand_map.restype = ctypes.c_int
    return _wave


def candidates_general(packer, table, wide, share, reqs, now, k, cand=None, global_base=0):
    """(sums [P] pack.CANDIDATES_SUM, entries [P][k] pack.CANDIDATE) of the scalar host build for the planes of `table` and the wide
    records `wide` (`share`: None, or their nhdfit_wide_share records in the same order)."""
    u32 = ctypes.c_uint32
    reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    if share is not None:
        share = np.ascontiguousarray(share, dtype=pack.WIDE_SHARE).reshape(-1)
        assert len(share) == len(wide)
    P, n = len(reqs), table.n
    sums, entries = np.zeros(P, pack.CANDIDATES_SUM), np.zeros((P, int(k)), pack.CANDIDATE)
    caps, sig_off, pool_off, glimit, cc, ncls, nsig, npools, ncc = packer.dictionary_arrays()
    gs = packer.group_set_array()
    planes = [np.ascontiguousarray(getattr(table, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
    cand = None if cand is None else np.ascontiguousarray(cand, dtype=np.uint64)
    rc = lib().hx_candidates_general(*[_p(x) for x in planes], u32(n), ctypes.c_uint64(global_base), _p(wide) if len(wide) else None,
                                     u32(len(wide)), _p(share), _p(reqs), u32(P), ctypes.c_double(now), u32(packer.max_cores_per_numa),
                                     u32(packer.max_gpus_per_numa), _p(gs), u32(len(packer.group_sets)), _p(caps), u32(ncls), _p(sig_off),
                                     u32(nsig), _p(pool_off), _p(glimit), _p(cc), _p(cand), u32(int(k)), _p(sums), _p(entries))
    assert rc == 0, f"{rc}: the dictionary's stream does not fit (-1) / a set of the model outgrew its table (-2)"
    return sums, entries


def merged_entry(a, b, j):
    """candidates_merge.h cand_merged_entry over two descending lists of score words: (from_b, pos), or None past the merged list."""
    a, b = np.ascontiguousarray(a, dtype=np.uint64), np.ascontiguousarray(b, dtype=np.uint64)
    from_b, pos = ctypes.c_int32(0), ctypes.c_uint32(0)
    rc = lib().hx_cand_merged_entry(_p(a), ctypes.c_uint32(len(a)), _p(b), ctypes.c_uint32(len(b)), ctypes.c_uint32(j), ctypes.byref(from_b),
                                    ctypes.byref(pos))
    return None if rc else (bool(from_b.value), int(pos.value))


def wide_map_wave(packer, wide, share, reqs, fits):
    """wide_map_on_state_wave on emulated lanes and the scalar wide_map for every (pod, wide record) with fits[p][w]:
    (wave mappings [P][W] pack.MAPPING, wave codes [P][W], scalar mappings, scalar codes)."""
    reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    if share is not None:
        share = np.ascontiguousarray(share, dtype=pack.WIDE_SHARE).reshape(-1)
        assert len(share) == len(wide)
    fits = np.ascontiguousarray(fits, dtype=np.uint8)
    assert fits.shape == (len(reqs), len(wide))
    mw, ms = np.zeros(fits.shape, pack.MAPPING), np.zeros(fits.shape, pack.MAPPING)
    rw, rs = np.zeros(fits.shape, np.int32), np.zeros(fits.shape, np.int32)
    caps = packer.dictionary_arrays()[0]
    ncls = packer.dictionary_arrays()[5]
    rc = wave_lib().we_wide_cand_map(_p(wide), _p(share), ctypes.c_uint32(len(wide)), _p(reqs), ctypes.c_uint32(len(reqs)), _p(caps),
                                     ctypes.c_uint32(ncls), _p(fits), _p(mw), _p(rw), _p(ms), _p(rs))
    assert rc == 0, f"{rc}: the emulated lanes disagreed (-100)"
    return mw, rw, ms, rs


class CandidatesGeneralHarnessEngine(ct.CandidatesHarnessEngine):
    """candidates_twin.CandidatesHarnessEngine plus candidates(general=True), as nhd_amd.engine.Engine.candidates answers it."""

    def candidates(self, reqs, now, k, cand=None, general=False):
        if not general:
            return super().candidates(reqs, now, k, cand=cand)
        return candidates_general(self.packer, self.table, self._wide_records(), self._share_records(), reqs, now, k, cand=cand,
                                  global_base=self.global_base)
