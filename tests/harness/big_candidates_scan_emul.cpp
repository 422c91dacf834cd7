// big_candidates_scan_emul.cpp - TEST INFRASTRUCTURE.  Runs DEVICE SOURCE TEXT on the host: the record logic of k_big_cand_scan and the
// two-range pick of k_big_cand_pick (nhd_amd/csrc/big_candidates_kernel.h, "the scan's records and the two-range pick with the
// wavefront's lanes": big_cand_keep, big_cand_post, big_cand_pick2) are cut out of the kernel header at build time
// (tests/harness/candidates_big_twin.py, unmodified), behind the pick of candidates_kernel.h (cand_pick_wave), and compiled here on the
// 64-thread wavefront emulation of wave_emul.cpp.  The verdicts per unit come from the caller: what is run here is how blocks of
// contiguous chunk ranges - the planes' range and the wide records' range apart - turn them into records, and the records into a list.
// tests/test_candidates_big_core.py holds the result to a scalar statement of the selection order.
// NOT part of libnhdfit.so; nothing in nhd_amd/ loads it.
#include "wave_emul.cpp"
#include "../../nhd_amd/csrc/candidates_merge.h"

#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))

namespace {
#include "_wave_candidates_block.inc"      // candidates_kernel.h: "the pick with the wavefront's lanes"
#include "_wave_big_candidates_block.inc"  // big_candidates_kernel.h: "the scan's records and the two-range pick with the wavefront's lanes"
}

// Per unit of either range (index order within a range): ok, pref (a preferred node; only read where ok), index.  units[2], nb[2]: the
// planes' range, then the wide records' (nb[1] == 0 with no wide record).  recs: [nb[0] + nb[1]][cand_rec_words(K)], zeroed by the
// caller; list: [64] out; sums: feasible, preferred as the blocks count them.  Returns the count every lane agreed on, -100 if they did not.
extern "C" int we_big_cand_scan_pick(const uint8_t* const ok[2], const uint8_t* const pref[2], const uint32_t* const index[2], const uint32_t units[2],
                                     const uint32_t nb[2], uint32_t K, uint64_t global_base, uint32_t* recs, uint32_t* list, uint32_t* sums) {
    static uint32_t first[2 * 64], plist[64], wlist[64];
    static uint64_t pscore[64], wscore[64];
    uint32_t count[emu::kLanes];
    uint32_t feasible = 0, preferred = 0;
    emu::acc[0] = emu::acc[1] = 0;
    std::vector<std::thread> lanes;
    for (int i = 0; i < emu::kLanes; ++i)
        lanes.emplace_back([&, i] {
            const uint32_t lane = (uint32_t)i;
            emu::t_lane = lane; emu::t_count = 0;
            for (uint32_t range = 0; range < 2; ++range) {
                const uint32_t total = (units[range] + 63u) / 64u;
                for (uint32_t b = 0; b < nb[range]; ++b) {               // a block: its contiguous chunk range, as the kernel cuts it
                    const uint32_t c_lo = (uint32_t)((uint64_t)total * b / nb[range]), c_hi = (uint32_t)((uint64_t)total * (b + 1) / nb[range]);
                    uint32_t n_any = 0, n_pref = 0;
                    for (uint32_t c = c_lo; c < c_hi; ++c) {
                        const uint32_t u = c * 64u + lane;
                        const bool in = u < units[range];
                        big_cand_keep(in && ok[range][u], in && pref[range][u], in ? index[range][u] : 0u, K, lane, first, n_any, n_pref);
                    }
                    big_cand_post(recs + (size_t)((range ? nb[0] : 0u) + b) * cand_rec_words(K), first, n_any, n_pref, K, lane);
                    if (lane == 0u) { feasible += n_any; preferred += n_pref; }
                    emu::wave_barrier();                                  // (`first` is the next block's)
                }
            }
            emu::wave_barrier();
            count[i] = big_cand_pick2(recs, nb[0], nb[1], K, global_base, plist, wlist, pscore, wscore, list, lane);
        });
    for (auto& t : lanes) t.join();
    sums[0] = feasible; sums[1] = preferred;
    for (int j = 1; j < emu::kLanes; ++j)
        if (count[j] != count[0]) return -100;
    return (int)count[0];
}
extern "C" uint32_t we_big_cand_rec_words(uint32_t K) { return cand_rec_words(K); }
extern "C" uint32_t we_big_cand_pref_bit() { return kCandPref; }
