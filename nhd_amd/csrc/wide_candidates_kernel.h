// wide_candidates_kernel.h - nhdfit_candidates_general on the device: the candidates the mirror holds as WIDE records join the list
// k_cand_list left (k_wide_cand_scan, k_wide_cand_map).  Device code of libnhdfit.so; included by nhdfit.hip inside its anonymous
// namespace, behind candidates_kernel.h (cand_pick_wave, the records' layout, CandSum) and wide_room_kernel.h (WideRoomLds,
// WideRoomStages).  gfx950 only.
//
// k_cand_list (candidates_kernel.h) lists the nodes of the planes and counts a candidate held as a wide record - 3 or 4 sockets, 65..128
// cores per socket, every node of an ENABLE_SHARING mirror - in not_evaluated.  These two kernels run behind it on the same stream;
// stream order is every hand-off there is.
//
//   k_wide_cand_scan, grid = (blocks, pods), a block is ONE wavefront, lane = wide slot.  A block takes a contiguous range of 64-slot
//     chunks of the wide records - they are sorted by index, so block order is index order.  Per lane the candidate bit of the
//     record's node, then wide_fits with the busy flag (nhdfit_find's verdict through k_wide_eval, wide_kernel.h); two ballots per
//     chunk, "fits" and "fits and preferred" (the pod requests no GPU and the node has none: k_wide_eval's expression).  The block keeps
//     its first K of each kind and its counts, posts them as a record of cand_rec_words(K) words - the record's node INDEX, not its slot
//     - and adds its counts to the pod's summary record, one atomic per non-zero field: feasible, preferred, and the candidates
//     evaluated here off not_evaluated.
//   k_wide_cand_map, grid = (K, pods), a block is ONE wavefront with WideRoomLds (41 KB, three blocks to a CU).  Block (j, pod) picks the
//     wide firsts in block order (cand_pick_wave), merges their score words with those of the planes' list by the rule of
//     candidates_merge.h, cut at K, and answers entry j: a planes entry is copied; for a wide record the 640-byte record (and the
//     1 024-byte share record) go into LDS with 16-byte loads and wide_map_on_state_wave maps it.  The merged list is a buffer of its
//     own: blocks of one pod read the planes' list while others write.  `returned` of the summary record stays the planes' count on
//     the device (every block of the pod reads it); the host sets min(K, feasible).
// Every loop has a bound known before it starts: the chunk range, the block count, K, U^(G+1) <= 1 024 (tuples).  No spin wait, no
// block waits for another.  Nothing but the call's own buffers is written.

// ---- one wide record's mapping with the wavefront's lanes ----------------------------------------------------------------------------
// One turn of wide_room_run_wave (wide_room_kernel.h) with no commit - its lines, COPIED here so that k_wide_room's code stays as it is:
// lane = tuple answers the GPU / NIC / CPU stage questions into bit rows, every tuple's hash is computed once; lane 0 runs
// wide_map_model over the rows, its set tables in LDS.  `t.node` (and, under Sharing, `t.share`) are in place and visible to every lane.
// Every lane returns wide_map's code (wide_core.h: 1 mapped, 0 the node does not take the pod, < 0 a set outgrew its table); t.mp is
// wide_map's mapping, bit for bit (tests/harness/wide_candidates_wave_emul.cpp runs this text on emulated lanes).
// Sharing: `t.share` prices the NICs (ENABLE_SHARING).  The routine and the two kernels below are templates over it: the mirror's kind
// is known at the launch, and as templates - the routine inlined into its one caller - they are emitted behind every function the
// file already had: within the code object's text k_step and the others keep the offsets they have without this header.
template <bool Sharing>
__device__ __forceinline__ int wide_map_on_state_wave(WideRoomLds& t, const nhdfit_req& r, const double* caps, uint32_t lane) {
    const nhdfit_wide_node& n = t.node;
    const nhdfit_wide_share* sh = Sharing ? &t.share : nullptr;
    const WideCaps wc(caps, sh);
    const bool shaped = req_valid(r) && wide_shape_ok(n);                // (wide_map's own guards; wide_fits admits no other pair)
    const uint32_t G = shaped ? r.n_groups : 0u, U = shaped ? n.numa_nodes : 1u, nG = wide_ipow(U, G), nC = nG * U;
    const bool fits_rows = shaped && nC <= kRoomTuplesC;
    if (lane == 0u) { wide_map_clear(t.mp, kMaxG); t.rc = !shaped ? 0 : fits_rows ? 1 : -1; }
    if (fits_rows) {                                                     // (wavefront-uniform)
        for (uint32_t code = lane; code < nG; code += 64u) t.hash_g[code] = wide_tuple_hash(code, G, U);
        for (uint32_t code = lane; code < nC; code += 64u) t.hash_c[code] = wide_tuple_hash(code, G + 1, U);
        const WideFree f = wide_free(n);
        for (uint32_t base = 0; base < nG; base += 64u) {                // the stages, lane = tuple
            const uint32_t code = base + lane;
            bool g = false, q = false;
            if (code < nG) {
                int8_t idx[kMaxG];
                g = wide_gpu_ok(r, f, code);
                q = wide_nic_choice(n, r, wc, code, idx);
            }
            const uint64_t mg = __ballot(g), mq = __ballot(q);
            if (lane == 0u) { t.bit_g[base >> 6] = mg; t.bit_n[base >> 6] = mq; }
        }
        for (uint32_t base = 0; base < nC; base += 64u) {
            const uint32_t code = base + lane;
            const uint64_t mc = __ballot(code < nC && wide_cpu_ok(r, f, code));
            if (lane == 0u) t.bit_c[base >> 6] = mc;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (lane == 0u) {                                                // the serial part: CPython's sets
            WideRoomStages rows{t};
            t.rc = wide_map_model(n, r, wc, f, t.tables, t.mp, kWideSetSlotsG, kWideSetSlotsC, rows);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return t.rc;
}

// ---- the launches -----------------------------------------------------------------------------------------------------------------
struct WideCandArgs {
    const nhdfit_wide_node* wide; uint32_t n_wide;
    const nhdfit_wide_share* share;                  // [n_wide] under Sharing: ENABLE_SHARING arithmetic
    const nhdfit_req* reqs;                          // [gridDim.y] pods
    const double* caps; uint32_t ncls;
    double busy_from;
    const uint64_t* cand;                            // optional [chunks of the planes' nodes]
    uint32_t n, wchunks, K, nb;                      // nodes of the mirror; 64-slot chunks of the wide records; blocks per pod of the scan
    uint64_t global_base;
    CandSum* sum;                                    // [pods]: k_cand_list's records
    uint32_t* recs;                                  // [pods][nb][cand_rec_words(K)], zeroed by the caller
    const nhdfit_candidate* planes;                  // [pods][K]: k_cand_list's lists
    nhdfit_candidate* out;                           // [pods][K], zeroed by the caller: the merged lists
    uint32_t* flags;                                 // [0] a set of the model outgrew its table (never expected)
};
constexpr uint32_t kWideCandBlock = 64;

// the pod requests no GPU (k_wide_eval's `want == 0`)
__device__ __forceinline__ bool wide_cand_gpuless(const nhdfit_req& r) {
    uint32_t want = 0;
    for (uint32_t g = 0; g < r.n_groups && g < (uint32_t)kMaxG; ++g) want += r.gpus[g];
    return want == 0u;
}

template <bool Sharing>
__global__ __launch_bounds__(kWideCandBlock) void k_wide_cand_scan(WideCandArgs a) {
    __shared__ double s_caps[NHDFIT_MAX_CLASSES];
    __shared__ uint32_t s_first[2 * 64];                                 // the block's firsts: "fits", preferred
    const uint32_t pod = blockIdx.y, lane = threadIdx.x, K = a.K, nb = gridDim.x;
    const nhdfit_req r = a.reqs[pod];
    if (lane < (uint32_t)NHDFIT_MAX_CLASSES) s_caps[lane] = lane < a.ncls ? a.caps[lane] : 0.0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const bool gpuless = wide_cand_gpuless(r);
    const uint32_t c_lo = (uint32_t)((uint64_t)a.wchunks * blockIdx.x / nb), c_hi = (uint32_t)((uint64_t)a.wchunks * (blockIdx.x + 1) / nb);
    const uint64_t below = (1ull << lane) - 1ull;
    uint32_t n_any = 0, n_pref = 0, n_seen = 0;                          // (wavefront-uniform)
    for (uint32_t c = c_lo; c < c_hi; ++c) {
        const uint32_t w = c * 64u + lane;
        bool listed = false, ok = false, nogpu = false;
        uint32_t index = 0;
        if (w < a.n_wide) {
            const nhdfit_wide_node& n = a.wide[w];
            index = n.index;
            listed = index < a.n && (!a.cand || (a.cand[index >> 6] >> (index & 63u) & 1ull));
            if (listed) {
                ok = wide_fits(n, r, n.busy_time >= a.busy_from, WideCaps(s_caps, Sharing ? a.share + w : nullptr));
                nogpu = n.n_gpus == 0;
            }
        }
        const uint64_t word = __ballot(ok), pref = gpuless ? __ballot(ok && nogpu) : 0ull;
        const bool mine = (pref >> lane & 1ull) != 0;
        if (ok) {
            const uint32_t pos = n_any + (uint32_t)popc64(word & below);
            if (pos < K) s_first[pos] = index | (mine ? kCandPref : 0u);
        }
        if (mine) {
            const uint32_t pos = n_pref + (uint32_t)popc64(pref & below);
            if (pos < K) s_first[64u + pos] = index;
        }
        n_any += (uint32_t)popc64(word); n_pref += (uint32_t)popc64(pref);
        n_seen += (uint32_t)popc64(__ballot(listed));
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    uint32_t* rec = a.recs + ((size_t)pod * nb + blockIdx.x) * cand_rec_words(K);
    const uint32_t na = n_any < K ? n_any : K, np = n_pref < K ? n_pref : K;
    if (lane == 0u) { rec[0] = na; rec[1] = np; }
    if (lane < na) rec[4u + lane] = s_first[lane];
    if (lane < np) rec[4u + K + lane] = s_first[64u + lane];
    CandSum* q = a.sum + pod;
    const uint32_t mine = lane == 0u ? n_any : lane == 1u ? n_pref : 0u - n_seen;   // (the candidates evaluated here leave not_evaluated)
    if (lane < 3u && mine) {                                             // one atomic per (block, pod, field)
        uint32_t* f = lane == 0u ? &q->feasible : lane == 1u ? &q->preferred : &q->not_evaluated;
        (void)__hip_atomic_fetch_add(f, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool Sharing>
__global__ __launch_bounds__(kWideCandBlock) void k_wide_cand_map(WideCandArgs a) {
    __shared__ __align__(16) WideRoomLds s_t;
    __shared__ double s_caps[NHDFIT_MAX_CLASSES];
    __shared__ uint32_t s_list[64];                                      // the wide firsts in selection order: index | kCandPref
    __shared__ uint64_t s_pscore[64], s_wscore[64];                      // the two lists' score words
    const uint32_t j = blockIdx.x, pod = blockIdx.y, lane = threadIdx.x, K = a.K;
    const nhdfit_req r = a.reqs[pod];
    if (lane < (uint32_t)NHDFIT_MAX_CLASSES) s_caps[lane] = lane < a.ncls ? a.caps[lane] : 0.0;
    const nhdfit_candidate* planes = a.planes + (size_t)pod * K;
    uint32_t n_planes = a.sum[pod].returned;                             // (k_cand_list's count: nobody writes it here)
    n_planes = n_planes < K ? n_planes : K;
    s_pscore[lane] = lane < n_planes ? planes[lane].score : 0ull;
    const uint32_t n_wide = cand_pick_wave(a.recs + (size_t)pod * a.nb * cand_rec_words(K), a.nb, K, s_list, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    s_wscore[lane] = lane < n_wide ? score_of((s_list[lane] & kCandPref) != 0u, a.global_base + (s_list[lane] & ~kCandPref)) : 0ull;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    bool from_wide = false;
    uint32_t pos = 0;
    if (!cand_merged_entry(s_pscore, n_planes, s_wscore, n_wide, j, from_wide, pos)) return;   // (wavefront-uniform) the list ends before entry j
    nhdfit_candidate* o = a.out + (size_t)pod * K + j;
    if (!from_wide) {                                                    // a planes entry: two 16-byte loads
        if (lane < sizeof(nhdfit_candidate) / 16) reinterpret_cast<uint4*>(o)[lane] = reinterpret_cast<const uint4*>(planes + pos)[lane];
        return;
    }
    const int slot = wide_slot_of(a.wide, a.n_wide, s_list[pos] & ~kCandPref);
    if (slot < 0) return;                                                // (the scan posted the record's own index)
    if (lane < sizeof(nhdfit_wide_node) / 16) {                          // forty 16-byte loads
        const uint4 q = reinterpret_cast<const uint4*>(a.wide + slot)[lane];
        uint32_t* d = reinterpret_cast<uint32_t*>(&s_t.node) + lane * 4u;
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    }
    if (Sharing) {                                                       // sixty-four
        static_assert(sizeof(nhdfit_wide_share) == 64 * 16, "a 16-byte load per lane");
        const uint4 q = reinterpret_cast<const uint4*>(a.share + slot)[lane];
        uint32_t* d = reinterpret_cast<uint32_t*>(&s_t.share) + lane * 4u;
        d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const int rc = wide_map_on_state_wave<Sharing>(s_t, r, s_caps, lane);
    if (lane == 0u) {
        nhdfit_mapping mp = s_t.mp;
        if (rc < 0) { mp.valid = 0; atomicOr(&a.flags[0], 1u); }          // as k_wide_map reports it
        o->score = s_wscore[pos];
        o->map = mp;
    }
}
