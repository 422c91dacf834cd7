// limit_kernel.h - nhdfit_headroom_limits on the device: the stage that ends each node's headroom run (k_limit_stage).
// Device code of libnhdfit.so; included by nhdfit.hip inside its anonymous namespace, behind explain_kernel.h and
// headroom_kernel.h.  gfx950 only.
//
// limit(node, template) = explain_stage (explain_core.h) of the template on the node in the state in which its run ended,
// nothing busy.  k_headroom leaves that state behind where a run placed at least one replica (HeadroomArgs::final: planes 0-4
// and the detail record as the last commit left them); a node whose run placed nothing ended in the mirror's own state.
//
//   grid = (nodes / kLimitThreads, templates of the slab), lane = node.  A lane reads its node's headroom entry; a node flagged
//   STOPPED or NOT_EVALUATED has no stage (NHDFIT_LIMIT_NONE, in no histogram bin: the reference leaves a half-committed node
//   behind where it raises, and a wide record's run was never made).  Every other lane builds the general path's view of its
//   state (wide_view) and asks explain_stage with busy = false and the run's own candidate bit.  A wide node outside `cand` reads
//   as its placeholder in the planes - no shape the general path holds - and is NOT_CANDIDATE like every other node outside it.
//   The view is 640 bytes and differs per (template, node), so it cannot be prepared once per call as k_explain_views does: it
//   lives in LDS, a slot per lane, padded to 648 bytes (162 dwords: the lanes' equal fields fall into different banks) - 41 KB
//   per 64-lane block, three blocks per CU.  Nothing of it is in private memory.
//   Counting is k_explain's (stage_histogram, explain_kernel.h): one atomicAdd per (block, template, stage).
//   The stage matrix is written only when the caller asked for it.
// The loops are explain_stage's (bounded by U^G assignments and the NIC odometer); no spin wait, no hand-off between blocks.
constexpr size_t kHeadroomSlabBytes = 64u << 20;  // device memory for the final states of one slab of templates (208 bytes per pair:
                                                  // four templates at 65 536 nodes, 78 at 4 096; one where a single one needs more)
constexpr uint32_t kLimitThreads = 64;            // nodes per block: 64 views of 648 bytes
struct LimitView { nhdfit_wide_node n; uint64_t pad; };
static_assert(sizeof(LimitView) == 648 && kLimitThreads * sizeof(LimitView) <= 48 * 1024, "three blocks' views in a CU's 160 KB of LDS");

struct LimitArgs {
    const nhdfit_plane0* p0; const nhdfit_plane1* p1; const nhdfit_plane2* p2; const nhdfit_plane3* p3; const nhdfit_plane4* p4;
    const nhdfit_detail* det; uint32_t n;
    const nhdfit_req* reqs;                        // [P]
    const double* caps;
    const uint64_t* cand;                          // optional [chunks]: the run's candidate mask
    const uint16_t* counts; size_t pitch;          // [P][pitch] headroom entries (k_headroom's rows: pitch = chunks * 64)
    const HeadroomFinal* final;                    // [slab][pitch]: written where an entry's count is non-zero
    uint32_t tpl0;                                 // the slab's first template: blockIdx.y counts from it
    uint32_t* hist;                                // [P][NHDFIT_STAGES], zeroed by the caller
    uint8_t* stage;                                // optional [P][n]
};
__global__ __launch_bounds__(kLimitThreads) void k_limit_stage(LimitArgs a) {
    __shared__ LimitView s_view[kLimitThreads];
    __shared__ uint32_t s_cnt[kLimitThreads / 64][NHDFIT_STAGES];
    __shared__ nhdfit_req s_req;                                       // (its fields reach the lanes as VGPRs, as in k_explain)
    const uint32_t tid = threadIdx.x;
    const uint32_t v = blockIdx.x * kLimitThreads + tid;
    const uint32_t tpl = a.tpl0 + blockIdx.y;                          // rows of reqs / counts / hist / stage; final is the slab's
    const bool live = v < a.n;
    static_assert(sizeof(nhdfit_req) % 4 == 0 && sizeof(nhdfit_req) / 4 <= kLimitThreads, "one dword of the record per thread");
    if (tid < sizeof(nhdfit_req) / 4) reinterpret_cast<uint32_t*>(&s_req)[tid] = reinterpret_cast<const uint32_t*>(a.reqs + tpl)[tid];
    __syncthreads();
    uint32_t st = NHDFIT_STAGES;                                       // (a lane past the end counts nowhere)
    if (live) {
        const uint32_t e = a.counts[(size_t)tpl * a.pitch + v];
        if (e & (NHDFIT_HEADROOM_STOPPED | NHDFIT_HEADROOM_NOT_EVALUATED)) st = NHDFIT_LIMIT_NONE;
        else {
            nhdfit_wide_node& w = s_view[tid].n;
            if (e & NHDFIT_HEADROOM_COUNT_MASK) {
                const HeadroomFinal& f = a.final[(size_t)blockIdx.y * a.pitch + v];
                wide_view(f.st.p0, f.st.p1, f.st.p2, f.st.p3, f.st.p4, f.dd, v, w);
            } else wide_view(a.p0[v], a.p1[v], a.p2[v], a.p3[v], a.p4[v], a.det[v], v, w);
            const bool listed = !a.cand || (a.cand[v >> 6] >> (v & 63u) & 1ull);
            st = explain_stage(w, s_req, listed, /*busy=*/false, WideCaps(a.caps), 0u, nullptr);
        }
        if (a.stage) a.stage[(size_t)tpl * a.n + v] = (uint8_t)st;
    }
    stage_histogram<kLimitThreads / 64>(s_cnt, st, a.hist, tpl, tid);
}
