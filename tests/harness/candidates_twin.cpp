// candidates_twin.cpp - TEST INFRASTRUCTURE.  The host build of nhdfit_candidates: what k_cand_list (nhd_amd/csrc/candidates_kernel.h)
// answers, written as the definition reads - every node of the planes in index order through the shared headers' SCALAR forms
// (node_index / lone_pod_fits, fit_core.h; lone_nic_bits -> map_on_state, seq_core.h), the preferred nodes first, cut at K - and the
// group entry's merge of the shards' lists (candidates_merge.h).  It is NOT part of libnhdfit.so and nothing in nhd_amd/ loads it.
// (The kernel's own pick runs on emulated lanes in candidates_pick_emul.cpp.)
#include "headroom_host.h"
#include "../../nhd_amd/csrc/candidates_merge.h"

using namespace nhdfit;

extern "C" int hx_candidates(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3, const nhdfit_plane4* p4,
                             const nhdfit_detail* det, uint32_t n, uint64_t global_base, const nhdfit_wide_node* wide, uint32_t n_wide,
                             const nhdfit_req* reqs, uint32_t P, double now, uint32_t fcmax, uint32_t fgmax, const uint64_t* gs, uint32_t ngs,
                             const double* caps, uint32_t ncls, const uint32_t* sig_off, uint32_t nsig, const uint32_t* pool_off,
                             const uint8_t* pool_glimit, const nhdfit_cc* cc, const uint64_t* cand, uint32_t K, nhdfit_candidates_sum* sums,
                             nhdfit_candidate* out) {
    const hrh::Dictionary d = hrh::make_dictionary(fcmax, fgmax, gs, ngs, caps, ncls, sig_off, nsig, pool_off, pool_glimit, cc);
    if (!d.ok) return -1;
    const double busy_from = busy_threshold(now);
    const MapTables mt{nullptr, nullptr, SetStates{nullptr, nullptr, nullptr, 0}};
    std::memset(sums, 0, (size_t)P * sizeof *sums);
    std::memset(out, 0, (size_t)P * K * sizeof *out);
    for (uint32_t p = 0; p < P; ++p) {
        const nhdfit_req& r = reqs[p];
        const hrh::Masks m = hrh::make_masks(r, d);
        const LoneMasks t = m.view();
        const bool needs_gpu = (m.h.flags & kPodNeedGpu) != 0;
        nhdfit_candidates_sum& s = sums[p];
        s.form = n ? (req_valid(r) && r.n_groups > 3 ? NHDFIT_CANDIDATES_FORM_GENERIC : NHDFIT_CANDIDATES_FORM_WAVE) : 0u;
        std::vector<uint32_t> order[2];                                  // [0] the preferred nodes, [1] the rest: each in index order
        for (uint32_t v = 0; v < n; ++v) {
            if (cand && !(cand[v >> 6] >> (v & 63) & 1ull)) continue;
            if (hrh::is_wide(wide, n_wide, v)) { s.not_evaluated++; continue; }
            const NodeIdx ni = node_index(p0[v], p1[v], p2[v], p4[v], d.fc_dim, d.fg_dim, d.ngs);
            if (!lone_pod_fits(t, m.h, ni, p3[v], p4[v].busy_time >= busy_from, d.gs)) continue;
            const bool pref = !needs_gpu && ni.nogpu;
            s.feasible++;
            if (pref) s.preferred++;
            order[pref ? 0 : 1].push_back(v);
        }
        s.returned = std::min(K, s.feasible);
        uint32_t k = 0;
        for (int kind = 0; kind < 2; ++kind)
            for (size_t q = 0; q < order[kind].size() && k < K; ++q, ++k) {
                const uint32_t v = order[kind][q];
                nhdfit_candidate& e = out[(size_t)p * K + k];
                e.score = score_of(kind == 0, global_base + v);
                const NodeState st{p0[v], p1[v], p2[v], p3[v], p4[v]};
                nhdfit_mapping mp;
                std::memset(&mp, 0, sizeof mp);
                if (!map_on_state(r, st, det[v], d.caps, lone_nic_bits(t, r.map_type == NHDFIT_MAP_PCI, p3[v]), mt, mp)) std::memset(&mp, 0, sizeof mp);
                e.map = mp;
            }
    }
    return 0;
}

// the statement libnhdfit.so's group entry runs per shard
extern "C" void hx_merge_candidate_lists(nhdfit_candidates_sum* sum, nhdfit_candidate* list, int32_t* owner, const nhdfit_candidates_sum* part,
                                         const nhdfit_candidate* part_list, uint32_t P, uint32_t K, int32_t shard) {
    merge_candidate_lists(sum, list, owner, part, part_list, P, K, shard);
}
