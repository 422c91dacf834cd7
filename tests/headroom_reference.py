"""Headroom as the UNMODIFIED reference defines it (include/nhdfit.h, nhdfit_headroom): the number of times the scheduler's own per-pod
sequence succeeds back to back on a private copy of a node with the busy window out of the way -

    Matcher().FindNode({name: node}, a fresh top)                      nhd/NHDScheduler.py:277
    node.SetPhysicalIdsFromMapping(mapping, top)                        :292   (it raises or returns None: the run stops, flagged, not counted)
    node.ClaimPodNICResources(list({x[0] for x in nic_list}))           :302-304

The reference's Node holds a threading lock and cannot be deep-copied: the private copy is built again from the fixture's
description, and the topology afresh per replica (SetPhysicalIdsFromMapping writes into it, as the scheduler parses a fresh config
per pod).  SetBusy is never called and busy_time is put long ago before every match: capacity, not rate.

`independent_headroom` is the same loop on the independent oracle (oracle/nhd_oracle.py: find_node on the one node + commit), which
travels where the reference does not."""
import contextlib
import io

from oracle import nhd_oracle as O

LONG_AGO = -1.0e9


def reference_headroom(ref, build_node, make_top, max_per_node):
    """(replicas, stopped) for the node `build_node()` returns (a fresh reference Node) and the template `make_top()` (a fresh
    reference topology per call)."""
    n = build_node()
    m = ref.Matcher()
    k, stopped = 0, False
    while k < max_per_node:
        n.busy_time = LONG_AGO                               # IsBusy() false; SetBusy is never called
        top = make_top()
        with contextlib.redirect_stdout(io.StringIO()):
            match = m.FindNode({n.name: n}, top)
        if match[0] is None:
            break
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                nic_list = n.SetPhysicalIdsFromMapping(match[1], top)
        except (IndexError, TypeError):                      # (TypeError: the unwind path in front of `return None` is itself broken,
            nic_list = None                                  #  nhd/Node.py:826-841 - the reference fails on the placement either way)
        if nic_list is None:
            stopped = True
            break
        n.ClaimPodNICResources(list({x[0] for x in nic_list}))
        k += 1
    return k, stopped


def independent_headroom(build_node, make_top, max_per_node, now=1.0e6):
    """(replicas, stopped) by the independent oracle: find_node on the one node, commit with a commit time long ago."""
    n = build_node()
    k, stopped = 0, False
    while k < max_per_node:
        n.busy_time = LONG_AGO
        top = make_top()
        match = O.find_node({n.name: n}, top, now)
        if match[0] is None:
            break
        try:
            O.commit(n, top, match[1], LONG_AGO)
        except O.CommitFailure:
            stopped = True
            break
        k += 1
    return k, stopped
