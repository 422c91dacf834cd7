// explain_twin.cpp - TEST INFRASTRUCTURE.  The host build of the stage function behind nhdfit_explain
// (nhd_amd/csrc/explain_core.h), walked over the nodes the way k_explain walks them: a node of the planes read through
// wide_view, a node whose entry is a placeholder answered by its wide record.  It is NOT part of libnhdfit.so and
// nothing in nhd_amd/ loads it.
#include <cstdint>
#include "../../nhd_amd/csrc/explain_core.h"

using namespace nhdfit;

namespace {
template <class R>
int explain(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3, const nhdfit_plane4* p4,
            const nhdfit_detail* det, uint32_t n, const nhdfit_wide_node* wide, uint32_t n_wide, const R* reqs, uint32_t P, double now,
            const double* caps, const uint64_t* cand, const nhdfit_wide_share* share, uint32_t budget, uint32_t* counts, uint8_t* stage) {
    const double busy_from = busy_threshold(now);
    int exhausted = 0;
    for (uint32_t v = 0; v < n; ++v) {
        int s = -1;
        for (uint32_t w = 0; w < n_wide; ++w)
            if (wide[w].index == v) s = (int)w;
        nhdfit_wide_node view;
        if (s < 0) wide_view(p0[v], p1[v], p2[v], p3[v], p4[v], det[v], v, view);
        const nhdfit_wide_node& node = s >= 0 ? wide[s] : view;
        const bool listed = !cand || (cand[v >> 6] >> (v & 63) & 1ull);
        const bool busy = node.busy_time >= busy_from;
        for (uint32_t i = 0; i < P; ++i) {
            bool out = false;
            const uint32_t st = explain_stage(node, reqs[i], listed, busy, WideCaps(caps, share && s >= 0 ? share + s : nullptr), budget, &out);
            exhausted |= out;
            counts[(size_t)i * NHDFIT_STAGES + st]++;
            if (stage) stage[(size_t)i * n + v] = (uint8_t)st;
        }
    }
    return exhausted;
}
}  // namespace

extern "C" int hx_explain(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3,
                          const nhdfit_plane4* p4, const nhdfit_detail* det, uint32_t n, const nhdfit_wide_node* wide, uint32_t n_wide,
                          const nhdfit_req* reqs, uint32_t P, double now, const double* caps, const uint64_t* cand,
                          const nhdfit_wide_share* share, uint32_t* counts, uint8_t* stage) {
    return explain(p0, p1, p2, p3, p4, det, n, wide, n_wide, reqs, P, now, caps, cand, share, 0u, counts, stage);
}
extern "C" int hx_explain_big(const nhdfit_plane0* p0, const nhdfit_plane1* p1, const nhdfit_plane2* p2, const nhdfit_plane3* p3,
                              const nhdfit_plane4* p4, const nhdfit_detail* det, uint32_t n, const nhdfit_wide_node* wide, uint32_t n_wide,
                              const nhdfit_big_req* reqs, uint32_t P, double now, const double* caps, const uint64_t* cand,
                              const nhdfit_wide_share* share, uint32_t* counts, uint8_t* stage) {
    return explain(p0, p1, p2, p3, p4, det, n, wide, n_wide, reqs, P, now, caps, cand, share, (uint32_t)NHDFIT_BIG_NIC_BUDGET, counts, stage);
}
