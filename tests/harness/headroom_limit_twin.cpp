// headroom_limit_twin.cpp - TEST INFRASTRUCTURE.  The host build of nhdfit_headroom_limits: headroom_twin.cpp's scalar run of every
// node (hrh::plane_run on a private copy), and then - what k_limit_stage
// (nhd_amd/csrc/limit_kernel.h) does on the device - wide_view of the copy as the run left it and explain_stage (explain_core.h)
// with nothing busy.  It is NOT part of libnhdfit.so and nothing in nhd_amd/ loads it.
#include "headroom_host.h"
#include "../../nhd_amd/csrc/explain_core.h"

using namespace nhdfit;

extern "C" int hx_headroom_limits(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3,
                                  const nhdfit_plane4* p4, const nhdfit_detail* det, uint32_t n, const nhdfit_wide_node* wide, uint32_t n_wide,
                                  const nhdfit_req* reqs, uint32_t P, uint32_t fcmax, uint32_t fgmax, const uint64_t* gs, uint32_t ngs,
                                  const double* caps, uint32_t ncls, const uint32_t* sig_off, uint32_t nsig, const uint32_t* pool_off,
                                  const uint8_t* pool_glimit, const nhdfit_cc* cc, const uint64_t* cand, uint32_t cap, hrh::Sum* sums,
                                  uint16_t* counts, uint32_t* hist, uint8_t* stage) {
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
            NodeState st{p0[v], p1[v], p2[v], p3[v], p4[v]};               // the private copy: the mirror's state until a commit succeeds
            nhdfit_detail dd = det[v];
            if (listed && hrh::is_wide(wide, n_wide, v)) e = NHDFIT_HEADROOM_NOT_EVALUATED;
            else if (listed) {
                e = hrh::plane_run(st, dd, r, m, d, cap);
            }
            hrh::account(s, e, cap);
            if (counts) counts[(size_t)p * n + v] = (uint16_t)e;
            uint32_t lim = NHDFIT_LIMIT_NONE;
            if (!(e & (NHDFIT_HEADROOM_STOPPED | NHDFIT_HEADROOM_NOT_EVALUATED))) {
                nhdfit_wide_node view;
                wide_view(st.p0, st.p1, st.p2, st.p3, st.p4, dd, v, view);
                lim = explain_stage(view, r, listed, /*busy=*/false, WideCaps(caps), 0u, nullptr);
                hist[(size_t)p * NHDFIT_STAGES + lim]++;
            }
            if (stage) stage[(size_t)p * n + v] = (uint8_t)lim;
        }
        sums[p] = s;
    }
    return 0;
}
