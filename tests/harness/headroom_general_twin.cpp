// headroom_general_twin.cpp - TEST INFRASTRUCTURE.  The host build of nhdfit_headroom_general: headroom_twin.cpp's scalar run of every
// node of the planes, and for every candidate held as a wide record the loop k_wide_room (nhd_amd/csrc/wide_room_kernel.h) runs, written
// over wide_core.h's SCALAR forms - wide_fits, wide_map (one thread, tables in scratch, hashes recomputed per probe), wide_commit - on a
// private copy of the record and, under ENABLE_SHARING, of its nhdfit_wide_share record.  It is NOT part of libnhdfit.so and nothing in
// nhd_amd/ loads it.  (The kernel's own per-node loop runs on emulated lanes in wide_room_wave_emul.cpp;
// tests/test_headroom_general_core.py holds the two to each other.)
#include "headroom_host.h"
#include "../../nhd_amd/csrc/wide_core.h"

using namespace nhdfit;

// one wide record's run; returns the entry, or -1 where wide_map reports a negative code
static int64_t wide_run(const nhdfit_wide_node& rec, const nhdfit_wide_share* share, const nhdfit_req& r, const double* caps, uint32_t cap,
                        std::vector<int16_t>& scratch) {
    nhdfit_wide_node copy = rec;
    nhdfit_wide_share sh;
    if (share) sh = *share;
    nhdfit_wide_share* shp = share ? &sh : nullptr;
    uint32_t k = 0;
    while (k < cap) {
        const WideCaps wc(caps, shp);
        if (!wide_fits(copy, r, /*busy=*/false, wc)) break;
        nhdfit_mapping m;
        const int rc = wide_map(copy, r, wc, scratch.data(), m);
        if (rc < 0) return -1;
        if (rc == 0) break;
        nhdfit_wide_placement pl;
        if (wide_commit(copy, r, m, 0.0, pl, shp) != kCommitOk) return (int64_t)(k | NHDFIT_HEADROOM_STOPPED);
        ++k;
    }
    return (int64_t)k;
}

// arguments as hx_headroom (headroom_twin.cpp) and `share`: NULL, or one record per wide record (ENABLE_SHARING).
// Returns 0, -1 (the dictionary's stream does not fit), -2 (a set of the model outgrew its table)
extern "C" int hx_headroom_general(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3,
                                   const nhdfit_plane4* p4, const nhdfit_detail* det, uint32_t n, const nhdfit_wide_node* wide, uint32_t n_wide,
                                   const nhdfit_wide_share* share, const nhdfit_req* reqs, uint32_t P, uint32_t fcmax, uint32_t fgmax,
                                   const uint64_t* gs, uint32_t ngs, const double* caps, uint32_t ncls, const uint32_t* sig_off, uint32_t nsig,
                                   const uint32_t* pool_off, const uint8_t* pool_glimit, const nhdfit_cc* cc, const uint64_t* cand, uint32_t cap,
                                   hrh::Sum* sums, uint16_t* counts) {
    const hrh::Dictionary d = hrh::make_dictionary(fcmax, fgmax, gs, ngs, caps, ncls, sig_off, nsig, pool_off, pool_glimit, cc);
    if (!d.ok) return -1;
    std::vector<int16_t> scratch(kWideScratchWords);
    std::vector<int32_t> slot(n, -1);
    for (uint32_t w = 0; w < n_wide; ++w)
        if (wide[w].index < n) slot[wide[w].index] = (int32_t)w;
    for (uint32_t p = 0; p < P; ++p) {
        const nhdfit_req& r = reqs[p];
        const hrh::Masks m = hrh::make_masks(r, d);
        hrh::Sum s;
        std::memset(&s, 0, sizeof s);
        s.form = hrh::form_of(r) | (n_wide ? NHDFIT_HEADROOM_FORM_WIDE : 0u);
        for (uint32_t v = 0; v < n; ++v) {
            uint32_t e = 0;
            const bool listed = !cand || (cand[v >> 6] >> (v & 63) & 1ull);
            if (listed && slot[v] >= 0) {
                const int64_t we = wide_run(wide[slot[v]], share ? share + slot[v] : nullptr, r, caps, cap, scratch);
                if (we < 0) return -2;
                e = (uint32_t)we;
            } else if (listed) {                                        // (headroom_twin.cpp's loop)
                NodeState st{p0[v], p1[v], p2[v], p3[v], p4[v]};
                nhdfit_detail dd = det[v];
                e = hrh::plane_run(st, dd, r, m, d, cap);
            }
            hrh::account(s, e, cap);
            if (counts) counts[(size_t)p * n + v] = (uint16_t)e;
        }
        sums[p] = s;
    }
    return 0;
}
