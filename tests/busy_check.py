"""Shared by the CPU and GPU tests of the busy window: Node.IsBusy (nhd/Node.py:847-850) in Python's own binary64 arithmetic and
the smallest stamp it calls busy at a given clock, found by bisection over the doubles - computed by nothing under test (no
import from nhd_amd, the harness or the oracles).  Clocks are finite; non-finite ones are not part of this."""
import math
import struct

MIN_BUSY_SECS = 30.0            # nhd/Node.py:107

# the clocks of the boundary tests, one test id each: the interval in which `now - 30.0` is exact and tiny from both sides (30.0 and
# its neighbourhood, 30.2 / 29.8 near its ends), a negative threshold (12.5), ordinary small clocks (31.0, 64.0), the suite's own
# clock, a wall-clock magnitude, 2^53 (`now - 30` exact at an ulp of 2) and a clock whose ulp (16) is coarser than half the window
CLOCKS = [30.0, 30.001, 29.999, 30.2, 29.8, 12.5, 31.0, 64.0, 1.0e6, 1.7e9, 2.0 ** 53, 1.0e17]
CLOCK_IDS = ["30", "30.001", "29.999", "30.2", "29.8", "12.5", "31", "64", "1e6", "1.7e9", "2^53", "1e17"]

_SIGN = 1 << 63
_MASK = (1 << 64) - 1
_DBL_MAX = 1.7976931348623157e308


def is_busy(now: float, t: float) -> bool:
    """Node.IsBusy at clock `now` of a node stamped `t`."""
    return (now - t) < MIN_BUSY_SECS


def _key(x: float) -> int:
    """The doubles in numeric order as unsigned integers (-0.0 right below +0.0)."""
    b = struct.unpack("<Q", struct.pack("<d", x))[0]
    return (~b & _MASK) if b & _SIGN else b | _SIGN


def _at(k: int) -> float:
    b = k ^ _SIGN if k & _SIGN else ~k & _MASK
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def least_busy(now: float) -> float:
    """The smallest double t with is_busy(now, t).  fl(now - t) never increases with t, so the predicate is monotone over the
    ordered doubles: a bisection between -DBL_MAX (not busy) and DBL_MAX (busy), at most 64 evaluations."""
    lo, hi = _key(-_DBL_MAX), _key(_DBL_MAX)
    assert not is_busy(now, _at(lo)) and is_busy(now, _at(hi)), now
    steps = 0
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if is_busy(now, _at(mid)):
            hi = mid
        else:
            lo = mid
        steps += 1
    assert steps <= 64
    return _at(hi)


def self_check(now: float) -> float:
    """least_busy(now), after checking that it is busy and the double below it is not."""
    t = least_busy(now)
    assert is_busy(now, t) and not is_busy(now, math.nextafter(t, -math.inf)), (now, t)
    return t


def stamps(now: float, n: int = 130, below: int = 64):
    """`n` stamps, consecutive doubles: `below` of them under least_busy(now), then least_busy(now) itself and the doubles above."""
    t = self_check(now)
    down = [t]
    for _ in range(below):
        down.append(math.nextafter(down[-1], -math.inf))
    up = [t]
    for _ in range(n - below - 1):
        up.append(math.nextafter(up[-1], math.inf))
    out = down[:0:-1] + up
    assert len(out) == n and out[below] == t and all(a < b for a, b in zip(out, out[1:]))
    return out
