"""Host build of nhdfit_explain's stage function (TEST INFRASTRUCTURE, see explain_twin.cpp), built the way the
package's __init__ builds the kernels' other host twin, and an engine that answers explain() with it."""
import ctypes
import os
import subprocess

import numpy as np

from nhd_amd import pack
from tests import harness

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "explain_twin.cpp")
SO = os.path.join(HERE, "_explain_twin.so")
STAGES = 10
_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    csrc = os.path.join(HERE, "..", "..", "nhd_amd", "csrc")
    deps = [SRC] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith(".h")] + [os.path.join(HERE, "..", "..", "include", "nhdfit.h")]
    if not os.path.exists(SO) or any(os.path.getmtime(d) > os.path.getmtime(SO) for d in deps):
        tmp = f"{SO}.{os.getpid()}.tmp"
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", tmp])
        os.replace(tmp, SO)
    _lib = ctypes.CDLL(SO)
    _lib.hx_explain.restype = ctypes.c_int
    _lib.hx_explain_big.restype = ctypes.c_int
    return _lib


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def explain(packer, table, wide, reqs, now, cand=None, share=None, per_node=True):
    """(counts [P][10], stages [P][n] or None) of the host build for the planes of `table` and the wide records `wide`
    (sorted by index); big requests (pack.BIG_REQ) take hx_explain_big."""
    big = reqs.dtype == pack.BIG_REQ
    reqs = np.ascontiguousarray(reqs)
    wide = np.ascontiguousarray(wide, dtype=pack.WIDE)
    P, n = len(reqs), table.n
    counts = np.zeros((P, STAGES), np.uint32)
    stages = np.zeros((P, n), np.uint8) if per_node else None
    planes = [np.ascontiguousarray(getattr(table, f)) for f in ("p0", "p1", "p2", "p3", "p4", "detail")]
    sh = None if share is None else np.ascontiguousarray(share, dtype=pack.WIDE_SHARE)
    fn = lib().hx_explain_big if big else lib().hx_explain
    bad = fn(*[_p(x) for x in planes], ctypes.c_uint32(n), _p(wide) if len(wide) else None, ctypes.c_uint32(len(wide)), _p(reqs),
             ctypes.c_uint32(P), ctypes.c_double(now), _p(harness._caps(packer)), _p(cand), _p(sh), _p(counts), _p(stages))
    if bad:
        from nhd_amd._lib import NhdFitError
        raise NhdFitError(-6, "a big request's NIC stage ran out of search budget on some node")
    return counts, stages


class ExplainHarnessEngine(harness.HarnessEngine):
    """harness.HarnessEngine plus explain(), as nhd_amd.engine.Engine.explain answers it."""

    def explain(self, reqs, now, cand=None, per_node=False):
        return explain(self.packer, self.table, self._wide_records(), reqs, now, cand=cand, share=self._share_records(), per_node=per_node)
