// wide_room_wave_emul.cpp - TEST INFRASTRUCTURE.  Runs DEVICE SOURCE TEXT on the host: the per-record loop of k_wide_room
// (nhd_amd/csrc/wide_room_kernel.h, "one wide record's run with the wavefront's lanes": wide_room_run_wave - the stages with lane = tuple,
// the set model and the commit step on the first lane, to exhaustion) is cut out of the kernel header at build time
// (tests/harness/headroom_general_twin.py, unmodified) and compiled here on the 64-thread wavefront emulation of wave_emul.cpp.
// Phase A (lane = wide slot) is wide_fits either way and is run as such.  tests/test_headroom_general_core.py holds the result to the
// scalar twin (headroom_general_twin.cpp) entry by entry.  NOT part of libnhdfit.so; nothing in nhd_amd/ loads it.
#include "wave_emul.cpp"

namespace {
#include "_wave_wide_room_block.inc"  // wide_room_kernel.h: "one wide record's run with the wavefront's lanes"
WideRoomLds g_lds;                    // the wavefront's LDS
}

// out [P][n_wide]: the entry of every (template, wide record) - 0 where the template does not fit the record.  `share`: NULL, or one
// record per wide record.  Returns 0, -2 (a set of the model outgrew its table), -100 (the lanes disagreed)
extern "C" int we_wide_room(const nhdfit_wide_node* wide, const nhdfit_wide_share* share, uint32_t n_wide, const nhdfit_req* reqs, uint32_t P,
                            const double* caps, uint32_t ncls, uint32_t cap, uint16_t* out) {
    double l_caps[NHDFIT_MAX_CLASSES] = {0};
    for (uint32_t c = 0; c < ncls && c < (uint32_t)NHDFIT_MAX_CLASSES; ++c) l_caps[c] = caps[c];
    uint32_t entry[emu::kLanes];
    bool disagree = false, failed = false;
    emu::acc[0] = emu::acc[1] = 0;
    std::vector<std::thread> lanes;
    for (int i = 0; i < emu::kLanes; ++i)
        lanes.emplace_back([&, i] {
            emu::t_lane = (uint32_t)i; emu::t_count = 0;
            const uint32_t lane = (uint32_t)i;
            for (uint32_t p = 0; p < P; ++p)
                for (uint32_t w = 0; w < n_wide; ++w) {
                    // phase A (every lane: the same answer)
                    const bool ok = wide_fits(wide[w], reqs[p], false, WideCaps(caps, share ? share + w : nullptr));
                    uint32_t e = 0;
                    if (ok) {                                        // phase B
                        if (lane == 0) {
                            std::memset(&g_lds, 0xA5, sizeof g_lds);
                            g_lds.node = wide[w];
                            if (share) g_lds.share = share[w];
                        }
                        emu::wave_barrier();
                        int err = 0;
                        e = wide_room_run_wave(g_lds, share != nullptr, reqs[p], l_caps, cap, lane, err);
                        entry[lane] = e;
                        emu::wave_barrier();
                        if (lane == 0) {
                            for (int j = 1; j < emu::kLanes; ++j) disagree |= entry[j] != entry[0];
                            failed |= err < 0;
                        }
                        emu::wave_barrier();
                    }
                    if (lane == 0) out[(size_t)p * n_wide + w] = (uint16_t)e;
                }
        });
    for (auto& t : lanes) t.join();
    return disagree ? -100 : failed ? -2 : 0;
}
