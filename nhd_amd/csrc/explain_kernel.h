// explain_kernel.h - nhdfit_explain on the device: for every (pod, node) pair the first stage of the reference's filter that
// drops the node (explain_core.h), counted per pod and stage.  Device code of libnhdfit.so; included by nhdfit.hip inside its
// anonymous namespace.  gfx950 only.
//
// k_explain_views writes every node of the planes once per call as the general path reads it (wide_view, straight into
// global memory: no 640-byte record in private memory) and, for a node whose entry is a placeholder, the slot of its wide
// record.  k_explain then runs lane = node, grid.y = a run of kExplainPods pods: a block's 256 nodes are read from L2 / L1
// once per pod of the run, not once per pair.  Per pod, every wavefront ballots each stage, the four wavefronts' counts
// meet in LDS, and one thread per stage posts ONE atomicAdd per (block, pod, stage) - never one per pair.  The stage
// matrix [P][n] is written only when the caller asked for it.
constexpr uint32_t kExplainThreads = 256;         // nodes per block (four wavefronts)
constexpr uint32_t kExplainPods = 16;             // pods per block: each lane's node record is reused across them

struct ExplainViewArgs {
    const nhdfit_plane0* p0; const nhdfit_plane1* p1; const nhdfit_plane2* p2; const nhdfit_plane3* p3; const nhdfit_plane4* p4;
    const nhdfit_detail* det; uint32_t n;
    const nhdfit_wide_node* wide; uint32_t n_wide;
    nhdfit_wide_node* views;                       // [n]: the node through wide_view (not written where a wide record answers)
    int32_t* slot;                                 // [n]: the node's wide record, or -1
};
__global__ __launch_bounds__(kExplainThreads) void k_explain_views(ExplainViewArgs a) {
    const uint32_t v = blockIdx.x * kExplainThreads + threadIdx.x;
    if (v >= a.n) return;
    const int s = a.n_wide ? wide_slot_of(a.wide, a.n_wide, v) : -1;
    a.slot[v] = s;
    if (s < 0) wide_view(a.p0[v], a.p1[v], a.p2[v], a.p3[v], a.p4[v], a.det[v], v, a.views[v]);
}

// The stage histogram of one (block, pod): every wavefront ballots each stage, the wavefronts' counts meet in LDS (`cnt`), and one
// thread per stage posts ONE atomicAdd into row `pod` of `hist`.  `st`: the lane's stage (NHDFIT_STAGES and beyond: counted nowhere).
// Ends with `cnt` still being read: the caller puts a barrier in front of its next use.  (k_explain; k_limit_stage, limit_kernel.h.)
template <uint32_t kWaves>
__device__ __forceinline__ void stage_histogram(uint32_t (*cnt)[NHDFIT_STAGES], uint32_t st, uint32_t* hist, uint32_t pod, uint32_t tid) {
    for (uint32_t k = 0; k < NHDFIT_STAGES; ++k) {
        const uint64_t m = __ballot(st == k);
        if ((tid & 63u) == 0) cnt[tid >> 6][k] = (uint32_t)popc64(m);
    }
    __syncthreads();
    if (tid < NHDFIT_STAGES) {
        uint32_t sum = 0;
        for (uint32_t w = 0; w < kWaves; ++w) sum += cnt[w][tid];
        if (sum) atomicAdd(&hist[(size_t)pod * NHDFIT_STAGES + tid], sum);
    }
}

template <class R> struct ExplainArgs {
    const nhdfit_wide_node* views; const int32_t* slot; uint32_t n;
    const nhdfit_wide_node* wide;
    const nhdfit_wide_share* share;                // optional [n_wide]: ENABLE_SHARING arithmetic
    const R* reqs; uint32_t P;
    const double* caps; double busy_from;
    const uint64_t* cand;                          // optional [chunks]
    uint32_t budget;                               // NIC search steps per pair and NIC question (big requests only)
    uint32_t* counts;                              // [P][NHDFIT_STAGES], zeroed by the caller
    uint8_t* stage;                                // optional [P][n]
    uint32_t* flags;                               // [0]: some pair ran out of NIC search budget
};
template <class R> __global__ __launch_bounds__(kExplainThreads) void k_explain(ExplainArgs<R> a) {
    __shared__ uint32_t s_cnt[kExplainThreads / 64][NHDFIT_STAGES];
    __shared__ R s_req;                                                // the pod's record: its fields reach the lanes as VGPRs (read
                                                                       // from the kernel argument's pointer they would be held in SGPRs)
    const uint32_t tid = threadIdx.x;
    const uint32_t v = blockIdx.x * kExplainThreads + tid;
    const bool live = v < a.n;
    const int s = live ? a.slot[v] : -1;
    const nhdfit_wide_node& node = s >= 0 ? a.wide[s] : a.views[live ? v : 0];
    const WideCaps caps(a.caps, a.share && s >= 0 ? a.share + s : nullptr);
    const bool listed = live && (!a.cand || (a.cand[v >> 6] >> (v & 63) & 1ull));
    const bool busy = live && node.busy_time >= a.busy_from;         // IsBusy, as the fit role asks it (fit_core.h busy_threshold)
    const uint32_t i0 = blockIdx.y * kExplainPods, i1 = min(a.P, i0 + kExplainPods);
    static_assert(sizeof(R) % 4 == 0 && sizeof(R) / 4 <= kExplainThreads, "one dword of the record per thread");
    for (uint32_t i = i0; i < i1; ++i) {
        if (tid < sizeof(R) / 4) reinterpret_cast<uint32_t*>(&s_req)[tid] = reinterpret_cast<const uint32_t*>(a.reqs + i)[tid];
        __syncthreads();
        uint32_t st = NHDFIT_STAGES;                                   // (a lane past the end counts nowhere)
        if (live) {
            bool out = false;                                          // (ordinary requests search without a budget, as k_wide_eval)
            st = explain_stage(node, s_req, listed, busy, caps, req_traits<R>::kBig ? a.budget : 0u, &out);
            if (out) atomicOr(&a.flags[0], 1u);
            if (a.stage) a.stage[(size_t)i * a.n + v] = (uint8_t)st;
        }
        stage_histogram<kExplainThreads / 64>(s_cnt, st, a.counts, i, tid);
        __syncthreads();                                               // (s_cnt and s_req are the next pod's)
    }
}
