"""Host builds of nhdfit_headroom (TEST INFRASTRUCTURE, see headroom_twin.cpp and headroom_wave_emul.cpp), built the way the
package's __init__ builds the kernels' other host twins, and an engine that answers headroom() with them."""
import ctypes
import os
import subprocess

import numpy as np

from nhd_amd import pack
from tests import harness

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "..", "nhd_amd", "csrc")
SRC = os.path.join(HERE, "headroom_twin.cpp")
SO = os.path.join(HERE, "_headroom_twin.so")
WAVE_SRC = os.path.join(HERE, "headroom_wave_emul.cpp")
WAVE_SO = os.path.join(HERE, "_headroom_wave_emul.so")
WAVE_INC = os.path.join(HERE, "_wave_headroom_block.inc")
_FROM, _TO = "// ---- one node's run with the wavefront's lanes", "// ---- the launch"
_lib = None
_wave = None


def _headers():
    return [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")] + [os.path.join(HERE, "..", "..", "include", "nhdfit.h"),
                                                                                    os.path.join(HERE, "headroom_host.h")]


def _stale(so, deps):
    return not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps)


def lib():
    """The scalar twin (hx_headroom)."""
    global _lib
    if _lib is None:
        if _stale(SO, [SRC] + _headers()):
            tmp = f"{SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = ctypes.CDLL(SO)
        _lib.hx_headroom.restype = ctypes.c_int
    return _lib


def wave_lib():
    """The kernel's per-node loop on emulated lanes (we_headroom): the section of headroom_kernel.h between its two headings, cut
    out unmodified, beside the sections harness.wave_lib() cuts out of the sequential kernels' headers."""
    global _wave
    if _wave is None:
        harness.wave_lib()                                  # (the mapping's and the commit step's wavefront forms: its .inc files)
        kernel = os.path.join(CSRC, "headroom_kernel.h")
        if _stale(WAVE_SO, [WAVE_SRC, harness.WAVE_SRC, harness.WAVE_SO, kernel] + _headers()):
            lines = open(kernel).read().split("\n")
            a = next(i for i, ln in enumerate(lines) if ln.startswith(_FROM))
            b = next(i for i, ln in enumerate(lines) if ln.startswith(_TO))
            assert a < b and any("headroom_run_wave" in ln for ln in lines[a:b])
            with open(WAVE_INC, "w") as f:
                f.write("\n".join(lines[a:b]) + "\n")
            tmp = f"{WAVE_SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", WAVE_SRC, "-o", tmp])
            os.replace(tmp, WAVE_SO)
        _wave = ctypes.CDLL(WAVE_SO)
        _wave.we_headroom.restype = ctypes.c_int
    return _wave


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def headroom(packer, table, wide, reqs, cand=None, max_per_node=512, per_node=True, wave=False):
    """(sums [P] pack.HEADROOM_SUM, entries [P][n] uint16 or None) of a host build for the planes of `table`; the nodes of the wide
    records `wide` are not evaluated.  wave=True: the kernel's own loop on emulated lanes instead of the scalar forms."""
    reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    P, n = len(reqs), table.n
    sums = np.zeros(P, pack.HEADROOM_SUM)
    counts = np.zeros((P, n), np.uint16) if per_node else None
    planes = [np.ascontiguousarray(getattr(table, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
    caps, sig_off, pool_off, glimit, cc, ncls, nsig, npools, ncc = packer.dictionary_arrays()
    gs = packer.group_set_array()
    if cand is not None:
        cand = np.ascontiguousarray(cand, dtype=np.uint64)
    fn = wave_lib().we_headroom if wave else lib().hx_headroom
    rc = fn(*[_p(x) for x in planes], ctypes.c_uint32(n), _p(wide) if len(wide) else None, ctypes.c_uint32(len(wide)), _p(reqs), ctypes.c_uint32(P),
            ctypes.c_uint32(packer.max_cores_per_numa), ctypes.c_uint32(packer.max_gpus_per_numa), _p(gs), ctypes.c_uint32(len(packer.group_sets)),
            _p(caps), ctypes.c_uint32(ncls), _p(sig_off), ctypes.c_uint32(nsig), _p(pool_off), _p(glimit), _p(cc), _p(cand),
            ctypes.c_uint32(int(max_per_node)), _p(sums), _p(counts))
    assert rc == 0, f"{rc}: the dictionary's stream does not fit (-1) / the emulated lanes disagreed (-100)"
    return sums, counts


class HeadroomHarnessEngine(harness.HarnessEngine):
    """harness.HarnessEngine plus headroom(), as nhd_amd.engine.Engine.headroom answers it."""
    wave = False

    def headroom(self, reqs, cand=None, max_per_node=512, per_node=False):
        return headroom(self.packer, self.table, self._wide_records(), reqs, cand=cand, max_per_node=max_per_node, per_node=per_node, wave=self.wave)


class HeadroomWaveEngine(HeadroomHarnessEngine):
    wave = True
