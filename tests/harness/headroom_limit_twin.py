"""The host build of nhdfit_headroom_limits (TEST INFRASTRUCTURE, see headroom_limit_twin.cpp), built the way headroom_twin.py builds
its twins, and an engine that answers headroom_limits() with it."""
import ctypes
import os
import subprocess

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
    rc, out = ht.run(lib().hx_headroom_limits, packer, table, wide, reqs, cand, max_per_node, per_node, limits=True)
    assert rc == 0, f"{rc}: the dictionary's stream does not fit"
    return out


class HeadroomLimitHarnessEngine(ht.HeadroomHarnessEngine):
    """headroom_twin.HeadroomHarnessEngine plus headroom_limits(), as nhd_amd.engine.Engine.headroom_limits answers it."""

    def headroom_limits(self, reqs, cand=None, max_per_node=512, per_node=False, _slab_bytes=None):
        return headroom_limits(self.packer, self.table, self._wide_records(), reqs, cand=cand, max_per_node=max_per_node, per_node=per_node)
