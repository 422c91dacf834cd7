// headroom_wave_emul.cpp - TEST INFRASTRUCTURE.  Runs DEVICE SOURCE TEXT on the host: the per-node loop of k_headroom
// (nhd_amd/csrc/headroom_kernel.h, "one node's run with the wavefront's lanes": headroom_run_wave - lone_nic_bits ->
// map_on_state_wave -> commit_node_wave -> node_index / lone_pod_fits, to exhaustion) is cut out of the kernel header at build time
// (tests/harness/headroom_twin.py, unmodified) and compiled here on the 64-thread wavefront emulation of wave_emul.cpp, with the
// wavefront forms of the mapping and of the commit step that file cuts out of seq_kernel.h / seq2_kernel.h and the mapping tables
// as the device builds them.  Phase A (lane = node) is the scalar arithmetic of fit_core.h either way and is run as such.
// tests/test_headroom_core.py holds the result to the scalar twin (headroom_twin.cpp) entry by entry.
// NOT part of libnhdfit.so; nothing in nhd_amd/ loads it.
#include "wave_emul.cpp"
#include "headroom_host.h"

namespace {
#include "_wave_headroom_block.inc"  // headroom_kernel.h: "one node's run with the wavefront's lanes"
}

// arguments as hx_headroom (headroom_twin.cpp); returns 0, -1 (the dictionary's stream does not fit), -100 (the lanes disagreed)
extern "C" int we_headroom(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3, const nhdfit_plane4* p4,
                           const nhdfit_detail* det, uint32_t n, const nhdfit_wide_node* wide, uint32_t n_wide, const nhdfit_req* reqs, uint32_t P,
                           uint32_t fcmax, uint32_t fgmax, const uint64_t* gs, uint32_t ngs, const double* caps, uint32_t ncls,
                           const uint32_t* sig_off, uint32_t nsig, const uint32_t* pool_off, const uint8_t* pool_glimit, const nhdfit_cc* cc,
                           const uint64_t* cand, uint32_t cap, hrh::Sum* sums, uint16_t* counts) {
    const hrh::Dictionary d = hrh::make_dictionary(fcmax, fgmax, gs, ngs, caps, ncls, sig_off, nsig, pool_off, pool_glimit, cc);
    if (!d.ok) return -1;
    std::vector<hrh::Masks> masks;
    for (uint32_t p = 0; p < P; ++p) masks.push_back(hrh::make_masks(reqs[p], d));
    const MapTables mt{asc_table(), choose_table(), set_states()};
    double l_caps[NHDFIT_MAX_CLASSES] = {0};
    for (uint32_t c = 0; c < ncls && c < (uint32_t)NHDFIT_MAX_CLASSES; ++c) l_caps[c] = caps[c];
    NodeState st;                                                    // the wavefront's LDS slice
    alignas(16) nhdfit_detail dd;
    nhdfit_placement pl;
    uint32_t entry[emu::kLanes];
    bool disagree = false;
    for (uint32_t p = 0; p < P; ++p) {
        std::memset(&sums[p], 0, sizeof sums[p]);
        sums[p].form = hrh::form_of(reqs[p]);
    }
    emu::acc[0] = emu::acc[1] = 0;
    std::vector<std::thread> lanes;
    for (int i = 0; i < emu::kLanes; ++i)
        lanes.emplace_back([&, i] {
            emu::t_lane = (uint32_t)i; emu::t_count = 0;
            const uint32_t lane = (uint32_t)i;
            for (uint32_t p = 0; p < P; ++p) {
                const nhdfit_req& r = reqs[p];
                HeadroomCtx x;
                x.t = masks[p].view(); x.h = masks[p].h;
                x.group_sets = gs; x.caps = l_caps; x.mt = mt; x.sigs = d.sigs();
                x.ncls = ncls; x.fc_dim = d.fc_dim; x.fg_dim = d.fg_dim; x.ngs = d.ngs; x.cap = cap;
                const bool g4 = hrh::form_of(r) == NHDFIT_HEADROOM_FORM_GENERIC;
                for (uint32_t v = 0; v < n; ++v) {
                    // phase A (every lane: the same answer)
                    uint32_t e = 0;
                    bool ok = false;
                    if (!cand || (cand[v >> 6] >> (v & 63) & 1ull)) {
                        if (hrh::is_wide(wide, n_wide, v)) e = NHDFIT_HEADROOM_NOT_EVALUATED;
                        else ok = lone_pod_fits(x.t, x.h, node_index(p0[v], p1[v], p2[v], p4[v], x.fc_dim, x.fg_dim, x.ngs), p3[v], false, gs);
                    }
                    if (ok) {                                        // phase B
                        if (lane == 0) { st = NodeState{p0[v], p1[v], p2[v], p3[v], p4[v]}; dd = det[v]; std::memset(&pl, 0xA5, sizeof pl); }
                        emu::wave_barrier();
                        e = g4 ? headroom_run_wave<true>(st, dd, pl, r, x, lane) : headroom_run_wave<false>(st, dd, pl, r, x, lane);
                        entry[lane] = e;
                        emu::wave_barrier();
                        if (lane == 0)
                            for (int j = 1; j < emu::kLanes; ++j) disagree |= entry[j] != entry[0];
                        emu::wave_barrier();
                    }
                    if (lane == 0) {
                        hrh::account(sums[p], e, cap);
                        if (counts) counts[(size_t)p * n + v] = (uint16_t)e;
                    }
                }
            }
        });
    for (auto& t : lanes) t.join();
    return disagree ? -100 : 0;
}
