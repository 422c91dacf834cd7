"""Host builds of nhdfit_headroom (TEST INFRASTRUCTURE, see headroom_twin.cpp and headroom_wave_emul.cpp), built the way the
package's __init__ builds the kernels' other host twins, and an engine that answers headroom() with them."""
import ctypes
import os
import subprocess

import numpy as np

from nhd_amd import pack
from nhd_amd.engine import STAGES
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
    """The scalar twin (hx_headroom), and the group entries' merge of summary records (hx_merge_headroom_sums)."""
    global _lib
    if _lib is None:
        if _stale(SO, [SRC] + _headers()):
            tmp = f"{SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = ctypes.CDLL(SO)
        _lib.hx_headroom.restype = ctypes.c_int
        _lib.hx_merge_headroom_sums.restype = None
    return _lib


def wave_lib():
    """The kernel's per-node loop on emulated lanes (we_headroom): the section of headroom_kernel.h between its two headings, cut
    out unmodified, beside the sections harness.wave_lib() cuts out of the sequential kernels' headers."""
    global _wave
    if _wave is None:
        harness.wave_lib()                                  # (the mapping's and the commit step's wavefront forms: its .inc files)
        kernel = os.path.join(CSRC, "headroom_kernel.h")
        if _stale(WAVE_SO, [WAVE_SRC, harness.WAVE_SRC, harness.WAVE_SO, kernel] + _headers()):
            harness.cut_section(kernel, _FROM, _TO, "headroom_run_wave", WAVE_INC)
            tmp = f"{WAVE_SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++20", "-ffp-contract=off", "-shared", "-fPIC", "-pthread", WAVE_SRC, "-o", tmp])
            os.replace(tmp, WAVE_SO)
        _wave = ctypes.CDLL(WAVE_SO)
        _wave.we_headroom.restype = ctypes.c_int
    return _wave


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def run(fn, packer, table, wide, reqs, cand, max_per_node, per_node, limits=False, share=...):
    """Calls an entry of the host builds - hx_headroom, we_headroom, hx_headroom_limits (`limits`: histogram and stage matrix behind
    sums and entries), hx_headroom_general (`share`: the wide records' nhdfit_wide_share records or None - an argument this entry
    alone has) - with the planes of `table`, the wide records, the requests, the dictionary, the mask and the bound.  Returns
    (the entry's return code, (sums [P] pack.HEADROOM_SUM, entries [P][n] uint16 or None[, limits [P][STAGES] uint32, stages [P][n]
    uint8 or None]))."""
    u32 = ctypes.c_uint32
    reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    P, n = len(reqs), table.n
    outs = [np.zeros(P, pack.HEADROOM_SUM), np.zeros((P, n), np.uint16) if per_node else None]
    if limits:
        outs += [np.zeros((P, STAGES), np.uint32), np.zeros((P, n), np.uint8) if per_node else None]
    caps, sig_off, pool_off, glimit, cc, ncls, nsig, npools, ncc = packer.dictionary_arrays()
    gs = packer.group_set_array()
    args = [_p(np.ascontiguousarray(getattr(table, f))) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
    args += [u32(n), _p(wide) if len(wide) else None, u32(len(wide))]
    if share is not ...:
        if share is not None:
            share = np.ascontiguousarray(share, dtype=pack.WIDE_SHARE).reshape(-1)
            assert len(share) == len(wide)
        args.append(_p(share) if len(wide) else None)
    args += [_p(reqs), u32(P), u32(packer.max_cores_per_numa), u32(packer.max_gpus_per_numa), _p(gs), u32(len(packer.group_sets)), _p(caps),
             u32(ncls), _p(sig_off), u32(nsig), _p(pool_off), _p(glimit), _p(cc),
             _p(None if cand is None else np.ascontiguousarray(cand, dtype=np.uint64)), u32(int(max_per_node))]
    return fn(*args, *[_p(o) for o in outs]), tuple(outs)


def headroom(packer, table, wide, reqs, cand=None, max_per_node=512, per_node=True, wave=False):
    """(sums [P] pack.HEADROOM_SUM, entries [P][n] uint16 or None) of a host build for the planes of `table`; the nodes of the wide
    records `wide` are not evaluated.  wave=True: the kernel's own loop on emulated lanes instead of the scalar forms."""
    rc, out = run(wave_lib().we_headroom if wave else lib().hx_headroom, packer, table, wide, reqs, cand, max_per_node, per_node)
    assert rc == 0, f"{rc}: the dictionary's stream does not fit (-1) / the emulated lanes disagreed (-100)"
    return out


class HeadroomHarnessEngine(harness.HarnessEngine):
    """harness.HarnessEngine plus headroom(), as nhd_amd.engine.Engine.headroom answers it."""
    wave = False

    def headroom(self, reqs, cand=None, max_per_node=512, per_node=False):
        return headroom(self.packer, self.table, self._wide_records(), reqs, cand=cand, max_per_node=max_per_node, per_node=per_node, wave=self.wave)


class HeadroomWaveEngine(HeadroomHarnessEngine):
    wave = True
