// candidates_big_twin.cpp - TEST INFRASTRUCTURE.  The host build of nhdfit_candidates_big: what k_big_cand_scan / _pick / _map
// (nhd_amd/csrc/big_candidates_kernel.h) answer, written as the definition reads over wide_core.h's SCALAR forms - every unit of the
// mirror (a node of the planes through wide_view, a wide record as it is), the candidate bit at its index, wide_fits with the busy
// flag under the pair's NIC search budget; the feasible nodes ranked by descending score word (one sort: no blocks, no ranges), cut at
// K; each entry mapped by one-thread wide_map on tables sized for its own node.  The group entry's merge of the shards' lists is
// candidates_merge.h's, instantiated for the big entry.  It is NOT part of libnhdfit.so and nothing in nhd_amd/ loads it.
// (The kernel's own record logic and two-range pick run on emulated lanes in big_candidates_scan_emul.cpp.)
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../nhd_amd/csrc/seq_core.h"
#include "../../nhd_amd/csrc/wide_core.h"
#include "../../nhd_amd/csrc/candidates_merge.h"

using namespace nhdfit;

// share: NULL, or one record per wide record (ENABLE_SHARING).  budget: 0 - NHDFIT_BIG_NIC_BUDGET - or the search steps a (pod, node)
// pair may take.  Returns 0, -2 (a set of the model outgrew its table) or -3 (a pair ran out of search budget): sums and out all zero.
extern "C" int hx_candidates_big(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3,
                                 const nhdfit_plane4* p4, const nhdfit_detail* det, uint32_t n, uint64_t global_base, const nhdfit_wide_node* wide,
                                 uint32_t n_wide, const nhdfit_wide_share* share, const nhdfit_big_req* reqs, uint32_t P, double now,
                                 const double* caps, const uint64_t* cand, uint32_t K, uint32_t budget, nhdfit_candidates_sum* sums,
                                 nhdfit_big_candidate* out) {
    const double busy_from = busy_threshold(now);
    const uint32_t steps = budget ? budget : NHDFIT_BIG_NIC_BUDGET;
    std::memset(sums, 0, (size_t)P * sizeof *sums);
    std::memset(out, 0, (size_t)P * K * sizeof *out);
    if (!n) return 0;
    int bad = 0;
    struct Hit { uint64_t score; uint32_t unit; };
    for (uint32_t p = 0; p < P && !bad; ++p) {
        const nhdfit_big_req& r = reqs[p];
        uint32_t want = 0;
        for (uint32_t g = 0; g < r.n_groups && g < (uint32_t)NHDFIT_BIG_MAX_GROUPS; ++g) want += r.gpus[g];
        nhdfit_candidates_sum& s = sums[p];
        std::vector<Hit> hits;
        for (uint32_t v = 0; v < n + n_wide; ++v) {
            nhdfit_wide_node view;
            if (v < n) wide_view(p0[v], p1[v], p2[v], p3[v], p4[v], det[v], v, view);
            else view = wide[v - n];
            if (view.index >= n || (cand && !(cand[view.index >> 6] >> (view.index & 63) & 1ull)) || !view.numa_nodes) continue;
            NicSearch ns{steps, false};
            const bool ok = wide_fits(view, r, view.busy_time >= busy_from, WideCaps(caps, share && v >= n ? share + (v - n) : nullptr), &ns);
            if (ns.exhausted) bad = -3;
            if (!ok) continue;
            const bool pref = want == 0 && view.n_gpus == 0;
            s.feasible++;
            if (pref) s.preferred++;
            hits.push_back(Hit{score_of(pref, global_base + view.index), v});
        }
        std::sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.score > b.score; });
        s.returned = std::min(K, s.feasible);
        s.form = NHDFIT_CANDIDATES_FORM_BIG;
        for (uint32_t k = 0; k < s.returned && !bad; ++k) {
            const uint32_t v = hits[k].unit;
            nhdfit_wide_node view;
            if (v < n) wide_view(p0[v], p1[v], p2[v], p3[v], p4[v], det[v], v, view);
            else view = wide[v - n];
            const uint32_t U = view.numa_nodes, G = std::min<uint32_t>(r.n_groups, NHDFIT_BIG_MAX_GROUPS);
            std::vector<int32_t> scratch(big_scratch_words(U, G));       // (any size >= the need gives the same answer)
            nhdfit_big_candidate& e = out[(size_t)p * K + k];
            e.score = hits[k].score;
            const int rc = wide_map(view, r, WideCaps(caps, share && v >= n ? share + (v - n) : nullptr), scratch.data(), e.map,
                                    (int32_t)wide_table_slots(wide_ipow(U, G)), (int32_t)wide_table_slots(wide_ipow(U, G + 1)));
            if (rc < 0) bad = rc == -2 ? -3 : -2;
        }
    }
    if (bad) {                                                           // no half-answered list goes out
        std::memset(sums, 0, (size_t)P * sizeof *sums);
        std::memset(out, 0, (size_t)P * K * sizeof *out);
    }
    return bad;
}

// the statement libnhdfit.so's group entry runs per shard, for the big entry
extern "C" void hx_merge_big_candidate_lists(nhdfit_candidates_sum* sum, nhdfit_big_candidate* list, int32_t* owner, const nhdfit_candidates_sum* part,
                                             const nhdfit_big_candidate* part_list, uint32_t P, uint32_t K, int32_t shard) {
    merge_candidate_lists(sum, list, owner, part, part_list, P, K, shard);
}
