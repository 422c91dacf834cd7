// headroom_merge.h - how a shard's headroom summary records go into the group's.  Host code: libnhdfit.so's group entries
// (nhdfit_group_headroom, _general, _limits) and the host twin (tests/harness/headroom_twin.cpp exports it) read the rule here;
// nhd_amd/engine.py states it once more for groups of harness engines, and tests/test_headroom_merge.py holds the two to each other.
#pragma once
#include <stdint.h>
#include <algorithm>
#include "../../include/nhdfit.h"

namespace nhdfit {

// Counts add; max_on_one_node and the planes' instantiation (form & 3) take the larger; the wide launch's bit: whether any shard ran it.
inline void merge_headroom_sums(nhdfit_headroom_sum* sum_out, const nhdfit_headroom_sum* part, uint32_t P) {
    for (uint32_t p = 0; p < P; ++p) {
        nhdfit_headroom_sum& s = sum_out[p];
        s.replicas += part[p].replicas; s.nodes_with_room += part[p].nodes_with_room; s.saturated += part[p].saturated;
        s.stopped += part[p].stopped; s.not_evaluated += part[p].not_evaluated;
        s.max_on_one_node = std::max(s.max_on_one_node, part[p].max_on_one_node);
        s.form = std::max(s.form & 3u, part[p].form & 3u) | ((s.form | part[p].form) & NHDFIT_HEADROOM_FORM_WIDE);
    }
}

}  // namespace nhdfit
