// candidates_pick_emul.cpp - TEST INFRASTRUCTURE.  Runs DEVICE SOURCE TEXT on the host: the pick of k_cand_list
// (nhd_amd/csrc/candidates_kernel.h, "the pick with the wavefront's lanes": cand_pick_wave - the per-block firsts merged in block
// order, preferred nodes first, then the rest without them) is cut out of the kernel header at build time
// (tests/harness/candidates_twin.py, unmodified) and compiled here on the 64-thread wavefront emulation of wave_emul.cpp.  The
// agent-scope loads of the records are plain loads here: one process, nothing else writes them.
// tests/test_candidates_core.py holds the result to a scalar statement of the selection order.
// NOT part of libnhdfit.so; nothing in nhd_amd/ loads it.
#include "wave_emul.cpp"

#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_load(p, order, scope) (*(p))

namespace {
#include "_wave_candidates_block.inc"  // candidates_kernel.h: "the pick with the wavefront's lanes"
}

// records: [nb][cand_rec_words(K)] as the blocks post them; list: [64] out.  Returns the count every lane agreed on, -100 if they did not.
extern "C" int we_cand_pick(const uint32_t* recs, uint32_t nb, uint32_t K, uint32_t* list) {
    uint32_t count[emu::kLanes];
    emu::acc[0] = emu::acc[1] = 0;
    std::vector<std::thread> lanes;
    for (int i = 0; i < emu::kLanes; ++i)
        lanes.emplace_back([&, i] {
            emu::t_lane = (uint32_t)i; emu::t_count = 0;
            count[i] = cand_pick_wave(recs, nb, K, list, (uint32_t)i);
        });
    for (auto& t : lanes) t.join();
    for (int j = 1; j < emu::kLanes; ++j)
        if (count[j] != count[0]) return -100;
    return (int)count[0];
}
extern "C" uint32_t we_cand_rec_words(uint32_t K) { return cand_rec_words(K); }
extern "C" uint32_t we_cand_pref_bit() { return kCandPref; }
