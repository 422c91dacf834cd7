// candidates_general_twin.cpp - TEST INFRASTRUCTURE.  The host build of nhdfit_candidates_general: candidates_twin.cpp's list of the
// nodes of the planes, and for every candidate held as a wide record what k_wide_cand_scan / k_wide_cand_map
// (nhd_amd/csrc/wide_candidates_kernel.h) answer, written over wide_core.h's SCALAR forms - wide_fits with the busy flag, wide_map (one
// thread, tables in scratch, hashes recomputed per probe) - the records in index order, the preferred ones first, cut at K; the two lists
// merged by the rule of candidates_merge.h.  It is NOT part of libnhdfit.so and nothing in nhd_amd/ loads it.  (The kernel's own
// mapping routine runs on emulated lanes in wide_candidates_wave_emul.cpp; tests/test_candidates_general_core.py holds the two to
// each other.)
#include "candidates_twin.cpp"
#include "../../nhd_amd/csrc/wide_core.h"

// arguments as hx_candidates (candidates_twin.cpp) and `share`: NULL, or one record per wide record (ENABLE_SHARING).
// Returns 0, -1 (the dictionary's stream does not fit), -2 (a set of the model outgrew its table: sums and out all zero)
extern "C" int hx_candidates_general(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3,
                                     const nhdfit_plane4* p4, const nhdfit_detail* det, uint32_t n, uint64_t global_base,
                                     const nhdfit_wide_node* wide, uint32_t n_wide, const nhdfit_wide_share* share, const nhdfit_req* reqs,
                                     uint32_t P, double now, uint32_t fcmax, uint32_t fgmax, const uint64_t* gs, uint32_t ngs, const double* caps,
                                     uint32_t ncls, const uint32_t* sig_off, uint32_t nsig, const uint32_t* pool_off, const uint8_t* pool_glimit,
                                     const nhdfit_cc* cc, const uint64_t* cand, uint32_t K, nhdfit_candidates_sum* sums, nhdfit_candidate* out) {
    const int rc = hx_candidates(p0, p1, p2, p3, p4, det, n, global_base, wide, n_wide, reqs, P, now, fcmax, fgmax, gs, ngs, caps, ncls, sig_off,
                                 nsig, pool_off, pool_glimit, cc, cand, K, sums, out);
    if (rc || !n || !n_wide) return rc;                                  // (no wide records: nhdfit_candidates, byte for byte)
    const double busy_from = busy_threshold(now);
    std::vector<int16_t> scratch(kWideScratchWords);
    std::vector<nhdfit_candidates_sum> part(P);
    std::vector<nhdfit_candidate> part_list((size_t)P * K);
    std::memset(part.data(), 0, P * sizeof part[0]);
    std::memset(part_list.data(), 0, part_list.size() * sizeof part_list[0]);
    std::vector<uint32_t> evaluated(P, 0);
    bool overflow = false;
    for (uint32_t p = 0; p < P; ++p) {
        const nhdfit_req& r = reqs[p];
        uint32_t want = 0;
        for (uint32_t g = 0; g < r.n_groups && g < (uint32_t)kMaxG; ++g) want += r.gpus[g];
        std::vector<uint32_t> order[2];                                  // [0] the preferred records, [1] the rest: slots, each in index order
        for (uint32_t w = 0; w < n_wide; ++w) {
            const nhdfit_wide_node& nd = wide[w];
            if (nd.index >= n || (cand && !(cand[nd.index >> 6] >> (nd.index & 63) & 1ull))) continue;
            evaluated[p]++;
            if (!wide_fits(nd, r, nd.busy_time >= busy_from, WideCaps(caps, share ? share + w : nullptr))) continue;
            const bool pref = want == 0 && nd.n_gpus == 0;
            part[p].feasible++;
            if (pref) part[p].preferred++;
            order[pref ? 0 : 1].push_back(w);
        }
        part[p].returned = std::min(K, part[p].feasible);
        uint32_t k = 0;
        for (int kind = 0; kind < 2; ++kind)
            for (size_t q = 0; q < order[kind].size() && k < K; ++q, ++k) {
                const uint32_t w = order[kind][q];
                nhdfit_candidate& e = part_list[(size_t)p * K + k];
                e.score = score_of(kind == 0, global_base + wide[w].index);
                nhdfit_mapping mp;
                if (wide_map(wide[w], r, WideCaps(caps, share ? share + w : nullptr), scratch.data(), mp) < 0) { mp.valid = 0; overflow = true; }
                e.map = mp;
            }
    }
    if (overflow) {
        std::memset(sums, 0, (size_t)P * sizeof *sums);
        std::memset(out, 0, (size_t)P * K * sizeof *out);
        return -2;
    }
    merge_candidate_lists(sums, out, nullptr, part.data(), part_list.data(), P, K, 0);
    for (uint32_t p = 0; p < P; ++p) {
        sums[p].not_evaluated -= evaluated[p];
        sums[p].form |= NHDFIT_CANDIDATES_FORM_WIDE;
    }
    return 0;
}

// entry j of two descending lists of score words merged (candidates_merge.h cand_merged_entry, what k_wide_cand_map's blocks run):
// 0 and *from_b / *pos, or -1 when the merged list has no entry j
extern "C" int hx_cand_merged_entry(const uint64_t* a, uint32_t na, const uint64_t* b, uint32_t nb, uint32_t j, int32_t* from_b, uint32_t* pos) {
    bool fb = false;
    uint32_t at = 0;
    if (!cand_merged_entry(a, na, b, nb, j, fb, at)) return -1;
    *from_b = fb ? 1 : 0; *pos = at;
    return 0;
}
