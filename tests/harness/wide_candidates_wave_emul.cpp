// wide_candidates_wave_emul.cpp - TEST INFRASTRUCTURE.  Runs DEVICE SOURCE TEXT on the host: the mapping routine of k_wide_cand_map
// (nhd_amd/csrc/wide_candidates_kernel.h, "one wide record's mapping with the wavefront's lanes": wide_map_on_state_wave - the stages
// with lane = tuple, the set model on the first lane) is cut out of the kernel header at build time
// (tests/harness/candidates_general_twin.py, unmodified) and compiled here on the 64-thread wavefront emulation of wave_emul.cpp, behind
// the section of wide_room_kernel.h whose LDS layout it reuses.  tests/test_candidates_general_core.py holds the result to the scalar
// wide_map (wide_core.h) bit for bit.  NOT part of libnhdfit.so; nothing in nhd_amd/ loads it.
#include "wave_emul.cpp"

namespace {
#include "_wave_wide_room_block.inc"        // wide_room_kernel.h: WideRoomLds, WideRoomStages (and wide_room_run_wave, not run here)
#include "_wave_wide_candidates_block.inc"  // wide_candidates_kernel.h: "one wide record's mapping with the wavefront's lanes"
WideRoomLds g_lds;                          // the wavefront's LDS
}

// Per (pod, wide record) with fits[p][w] != 0: the routine's mapping into wave[p][w] and its code into rc_wave[p][w]; the scalar
// wide_map's into scalar / rc_scalar.  `share`: NULL, or one record per wide record.  Returns 0, -100 (the lanes disagreed)
extern "C" int we_wide_cand_map(const nhdfit_wide_node* wide, const nhdfit_wide_share* share, uint32_t n_wide, const nhdfit_req* reqs, uint32_t P,
                                const double* caps, uint32_t ncls, const uint8_t* fits, nhdfit_mapping* wave, int32_t* rc_wave,
                                nhdfit_mapping* scalar, int32_t* rc_scalar) {
    double l_caps[NHDFIT_MAX_CLASSES] = {0};
    for (uint32_t c = 0; c < ncls && c < (uint32_t)NHDFIT_MAX_CLASSES; ++c) l_caps[c] = caps[c];
    int code[emu::kLanes];
    bool disagree = false;
    emu::acc[0] = emu::acc[1] = 0;
    std::vector<int16_t> scratch(kWideScratchWords);
    std::vector<std::thread> lanes;
    for (int i = 0; i < emu::kLanes; ++i)
        lanes.emplace_back([&, i] {
            emu::t_lane = (uint32_t)i; emu::t_count = 0;
            const uint32_t lane = (uint32_t)i;
            for (uint32_t p = 0; p < P; ++p)
                for (uint32_t w = 0; w < n_wide; ++w) {
                    const size_t at = (size_t)p * n_wide + w;
                    if (!fits[at]) continue;
                    if (lane == 0) {
                        std::memset(&g_lds, 0xA5, sizeof g_lds);
                        g_lds.node = wide[w];
                        if (share) g_lds.share = share[w];
                    }
                    emu::wave_barrier();
                    code[lane] = share ? wide_map_on_state_wave<true>(g_lds, reqs[p], l_caps, lane) : wide_map_on_state_wave<false>(g_lds, reqs[p], l_caps, lane);
                    emu::wave_barrier();
                    if (lane == 0) {
                        for (int j = 1; j < emu::kLanes; ++j) disagree |= code[j] != code[0];
                        wave[at] = g_lds.mp; rc_wave[at] = code[0];
                        rc_scalar[at] = wide_map(wide[w], reqs[p], WideCaps(caps, share ? share + w : nullptr), scratch.data(), scalar[at]);
                    }
                    emu::wave_barrier();
                }
        });
    for (auto& t : lanes) t.join();
    return disagree ? -100 : 0;
}
