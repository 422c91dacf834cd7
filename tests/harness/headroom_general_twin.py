"""Host builds of nhdfit_headroom_general (TEST INFRASTRUCTURE, see headroom_general_twin.cpp and wide_room_wave_emul.cpp), built the
way headroom_twin.py builds its twins, and an engine that answers headroom_general() with them."""
import ctypes
import os
import subprocess

import numpy as np

from nhd_amd import pack
from tests import harness
from tests.harness import headroom_twin as ht
from tests.harness.headroom_limit_twin import HeadroomLimitHarnessEngine

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "headroom_general_twin.cpp")
SO = os.path.join(HERE, "_headroom_general_twin.so")
WAVE_SRC = os.path.join(HERE, "wide_room_wave_emul.cpp")
WAVE_SO = os.path.join(HERE, "_wide_room_wave_emul.so")
WAVE_INC = os.path.join(HERE, "_wave_wide_room_block.inc")
_FROM, _TO = "// ---- one wide record's run with the wavefront's lanes", "// ---- the launch"
_lib = None
_wave = None
_p = ht._p


def lib():
    """The scalar twin (hx_headroom_general)."""
    global _lib
    if _lib is None:
        if ht._stale(SO, [SRC] + ht._headers()):
            tmp = f"{SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = ctypes.CDLL(SO)
        _lib.hx_headroom_general.restype = ctypes.c_int
    return _lib


def wave_lib():
    """The kernel's per-record loop on emulated lanes (we_wide_room): the section of wide_room_kernel.h between its two headings, cut
    out unmodified, beside the sections harness.wave_lib() cuts out of the other kernels' headers."""
    global _wave
    if _wave is None:
        harness.wave_lib()                                  # (wave_emul.cpp's own .inc files)
        kernel = os.path.join(ht.CSRC, "wide_room_kernel.h")
        if ht._stale(WAVE_SO, [WAVE_SRC, harness.WAVE_SRC, harness.WAVE_SO, kernel] + ht._headers()):
            harness.cut_section(kernel, _FROM, _TO, "wide_room_run_wave", WAVE_INC)
            tmp = f"{WAVE_SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", WAVE_SRC, "-o", tmp])
            os.replace(tmp, WAVE_SO)
        _wave = ctypes.CDLL(WAVE_SO)
        _wave.we_wide_room.restype = ctypes.c_int
    return _wave


def headroom_general(packer, table, wide, share, reqs, cand=None, max_per_node=512, per_node=True):
    """(sums [P] pack.HEADROOM_SUM, entries [P][n] uint16 or None) of the scalar twin for the planes of `table` and the wide records
    `wide` (`share`: None, or their nhdfit_wide_share records in the same order)."""
    rc, out = ht.run(lib().hx_headroom_general, packer, table, wide, reqs, cand, max_per_node, per_node, share=share)
    assert rc == 0, f"{rc}: the dictionary's stream does not fit (-1) / a set of the model outgrew its table (-2)"
    return out


def wide_room_wave(packer, wide, share, reqs, max_per_node=512):
    """[P][len(wide)] uint16: the kernel's own per-record loop on emulated lanes, every record a candidate."""
    reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    if share is not None:
        share = np.ascontiguousarray(share, dtype=pack.WIDE_SHARE).reshape(-1)
        assert len(share) == len(wide)
    out = np.zeros((len(reqs), len(wide)), np.uint16)
    if not len(wide) or not len(reqs):
        return out
    caps = packer.dictionary_arrays()[0]
    ncls = packer.dictionary_arrays()[5]
    rc = wave_lib().we_wide_room(_p(wide), _p(share), ctypes.c_uint32(len(wide)), _p(reqs), ctypes.c_uint32(len(reqs)), _p(caps),
                                 ctypes.c_uint32(ncls), ctypes.c_uint32(int(max_per_node)), _p(out))
    assert rc == 0, f"{rc}: a set of the model outgrew its table (-2) / the emulated lanes disagreed (-100)"
    return out


class HeadroomGeneralHarnessEngine(HeadroomLimitHarnessEngine):
    """headroom_limit_twin.HeadroomLimitHarnessEngine plus headroom_general(), as nhd_amd.engine.Engine.headroom_general answers it."""

    def headroom_general(self, reqs, cand=None, max_per_node=512, per_node=False):
        return headroom_general(self.packer, self.table, self._wide_records(), self._share_records(), reqs, cand=cand,
                                max_per_node=max_per_node, per_node=per_node)
