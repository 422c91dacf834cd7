"""The host build of nhdfit_headroom_limits (TEST INFRASTRUCTURE, see headroom_limit_twin.cpp), built the way headroom_twin.py builds
its twins, and an engine that answers headroom_limits() with it."""
import ctypes
import os
import subprocess

import numpy as np

from nhd_amd import pack
from nhd_amd.engine import STAGES
from tests.harness import headroom_twin as ht

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "headroom_limit_twin.cpp")
SO = os.path.join(HERE, "_headroom_limit_twin.so")
_lib = None
_p = ht._p


def lib():
    """The scalar twin (hx_headroom_limits)."""
    global _lib
    if _lib is None:
        if ht._stale(SO, [SRC] + ht._headers()):
            tmp = f"{SO}.{os.getpid()}.tmp"
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", tmp])
            os.replace(tmp, SO)
        _lib = ctypes.CDLL(SO)
        _lib.hx_headroom_limits.restype = ctypes.c_int
    return _lib


def headroom_limits(packer, table, wide, reqs, cand=None, max_per_node=512, per_node=True):
    """(sums [P] pack.HEADROOM_SUM, entries [P][n] uint16 or None, limits [P][STAGES] uint32, stages [P][n] uint8 or None) of the host
    build for the planes of `table`; the nodes of the wide records `wide` are not evaluated."""
    reqs = np.ascontiguousarray(reqs, dtype=pack.REQ)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    P, n = len(reqs), table.n
    sums = np.zeros(P, pack.HEADROOM_SUM)
    counts = np.zeros((P, n), np.uint16) if per_node else None
    hist = np.zeros((P, STAGES), np.uint32)
    stages = np.zeros((P, n), np.uint8) if per_node else None
    planes = [np.ascontiguousarray(getattr(table, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
    caps, sig_off, pool_off, glimit, cc, ncls, nsig, npools, ncc = packer.dictionary_arrays()
    gs = packer.group_set_array()
    if cand is not None:
        cand = np.ascontiguousarray(cand, dtype=np.uint64)
    rc = lib().hx_headroom_limits(*[_p(x) for x in planes], ctypes.c_uint32(n), _p(wide) if len(wide) else None, ctypes.c_uint32(len(wide)), _p(reqs),
                                  ctypes.c_uint32(P), ctypes.c_uint32(packer.max_cores_per_numa), ctypes.c_uint32(packer.max_gpus_per_numa), _p(gs),
                                  ctypes.c_uint32(len(packer.group_sets)), _p(caps), ctypes.c_uint32(ncls), _p(sig_off), ctypes.c_uint32(nsig),
                                  _p(pool_off), _p(glimit), _p(cc), _p(cand), ctypes.c_uint32(int(max_per_node)), _p(sums), _p(counts), _p(hist),
                                  _p(stages))
    assert rc == 0, f"{rc}: the dictionary's stream does not fit"
    return sums, counts, hist, stages


class HeadroomLimitHarnessEngine(ht.HeadroomHarnessEngine):
    """headroom_twin.HeadroomHarnessEngine plus headroom_limits(), as nhd_amd.engine.Engine.headroom_limits answers it."""

    def headroom_limits(self, reqs, cand=None, max_per_node=512, per_node=False, _slab_bytes=None):
        return headroom_limits(self.packer, self.table, self._wide_records(), reqs, cand=cand, max_per_node=max_per_node, per_node=per_node)
