// candidates_merge.h - how a shard's candidate lists go into the group's.  Host code: libnhdfit.so's group entry
// (nhdfit_group_candidates) and the host twin (tests/harness/candidates_twin.cpp exports it) read the rule here;
// nhd_amd/sharding.py states it once more for one process per GPU (merge_candidates), and tests/test_candidates_host_logic.py holds
// the two to each other.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include "fit_core.h"

namespace nhdfit {

// The merge rule, once - for the shards' lists below and for the planes' list against the wide records' (wide_candidates_kernel.h
// cand_merged_entry, which the host twin tests/harness/candidates_general_twin.cpp reads too): of two lists in descending score the
// first one's head goes next unless the second one's is larger; a list that has run out passes.
NHD_HD bool merge_takes_first(bool has_a, uint64_t score_a, bool has_b, uint64_t score_b) { return !has_b || (has_a && score_a > score_b); }
// Entry j of lists a [na] and b [nb] (score words, each descending) merged by that rule: true and `from_b` / `pos` (where it stands
// in its own list), or false when the merged list has no entry j.  At most j + 1 turns.
NHD_HD bool cand_merged_entry(const uint64_t* a, uint32_t na, const uint64_t* b, uint32_t nb, uint32_t j, bool& from_b, uint32_t& pos) {
    uint32_t i = 0, k = 0;
    for (uint32_t t = 0; t <= j; ++t) {
        if (i >= na && k >= nb) return false;
        from_b = !merge_takes_first(i < na, i < na ? a[i] : 0ull, k < nb, k < nb ? b[k] : 0ull);
        pos = from_b ? k++ : i++;
    }
    return true;
}

// One more shard (`shard`, its sums `part` [P] and lists `part_list` [P][K]) into the group's answer so far.  Per pod: the two lists
// - each in descending score, the selection order (fit_core.h score_of: preferred nodes first, then ascending global index) - are
// merged by descending score and cut at K; a score names one node of one shard, so no two entries tie.  Counts add; `returned` is
// min(K, feasible) of the sum; the instantiation (`form`) takes the larger.  owner (optional, [P][K]): the shard of each entry, -1
// past `returned`.  The caller starts from all-zero sums and lists (owner: -1).
// Entry: nhdfit_candidate or nhdfit_big_candidate - only the score words are compared, an entry moves as a whole.
template <class Entry>
inline void merge_candidate_lists(nhdfit_candidates_sum* sum, Entry* list, int32_t* owner, const nhdfit_candidates_sum* part,
                                  const Entry* part_list, uint32_t P, uint32_t K, int32_t shard) {
    Entry row[NHDFIT_CANDIDATES_MAX_K];
    int32_t own[NHDFIT_CANDIDATES_MAX_K];
    for (uint32_t p = 0; p < P; ++p) {
        nhdfit_candidates_sum& s = sum[p];
        Entry* a = list + (size_t)p * K;
        const Entry* b = part_list + (size_t)p * K;
        int32_t* o = owner ? owner + (size_t)p * K : nullptr;
        const uint32_t na = s.returned, nb = part[p].returned;
        uint32_t i = 0, j = 0, k = 0;
        while (k < K && (i < na || j < nb)) {
            const bool take_a = merge_takes_first(i < na, i < na ? a[i].score : 0ull, j < nb, j < nb ? b[j].score : 0ull);
            own[k] = take_a ? (o ? o[i] : -1) : shard;
            row[k++] = take_a ? a[i++] : b[j++];
        }
        memcpy(a, row, (size_t)k * sizeof *a);
        if (o) memcpy(o, own, (size_t)k * sizeof *o);
        s.feasible += part[p].feasible; s.preferred += part[p].preferred; s.not_evaluated += part[p].not_evaluated;
        s.returned = std::min(K, s.feasible);
        s.form = std::max(s.form, part[p].form);
    }
}

}  // namespace nhdfit
