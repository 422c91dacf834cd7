// headroom_twin.cpp - TEST INFRASTRUCTURE.  The host build of nhdfit_headroom: the loop k_headroom (nhd_amd/csrc/headroom_kernel.h)
// runs per node, written over the shared headers' SCALAR forms (hrh::plane_run, headroom_host.h) on a private copy of every node,
// and the group entries' merge of the shards' summary records (headroom_merge.h).  It is NOT part of libnhdfit.so and
// nothing in nhd_amd/ loads it.  (The kernel's own per-node loop, with the wavefront forms, runs on emulated lanes in
// headroom_wave_emul.cpp; tests/test_headroom_core.py holds the two to each other.)
#include "headroom_host.h"
#include "../../nhd_amd/csrc/headroom_merge.h"

using namespace nhdfit;

extern "C" int hx_headroom(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3, const nhdfit_plane4* p4,
                           const nhdfit_detail* det, uint32_t n, const nhdfit_wide_node* wide, uint32_t n_wide, const nhdfit_req* reqs, uint32_t P,
                           uint32_t fcmax, uint32_t fgmax, const uint64_t* gs, uint32_t ngs, const double* caps, uint32_t ncls,
                           const uint32_t* sig_off, uint32_t nsig, const uint32_t* pool_off, const uint8_t* pool_glimit, const nhdfit_cc* cc,
                           const uint64_t* cand, uint32_t cap, hrh::Sum* sums, uint16_t* counts) {
    const hrh::Dictionary d = hrh::make_dictionary(fcmax, fgmax, gs, ngs, caps, ncls, sig_off, nsig, pool_off, pool_glimit, cc);
    if (!d.ok) return -1;
    for (uint32_t p = 0; p < P; ++p) {
        const nhdfit_req& r = reqs[p];
        const hrh::Masks m = hrh::make_masks(r, d);
        hrh::Sum s;
        std::memset(&s, 0, sizeof s);
        s.form = hrh::form_of(r);
        for (uint32_t v = 0; v < n; ++v) {
            uint32_t e = 0;
            const bool listed = !cand || (cand[v >> 6] >> (v & 63) & 1ull);
            if (listed && hrh::is_wide(wide, n_wide, v)) e = NHDFIT_HEADROOM_NOT_EVALUATED;
            else if (listed) {
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

// the statement libnhdfit.so's group entries run per shard (tests/test_headroom_merge.py holds engine._add_headroom_sums to it)
extern "C" void hx_merge_headroom_sums(nhdfit_headroom_sum* sums, const nhdfit_headroom_sum* part, uint32_t P) {
    merge_headroom_sums(sums, part, P);
}
