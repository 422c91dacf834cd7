// candidates_kernel.h - nhdfit_candidates on the device: the first K nodes FindNode would pick, in the order it would get there,
// each with its mapping (k_cand_list).  Device code of libnhdfit.so; included by nhdfit.hip inside its anonymous namespace, behind
// headroom_kernel.h (the lone-pod masks of step_kernel.h, the wavefront form of the mapping - seq_kernel.h - wide_slot_of and the
// LDS slices of a node's private copy as k_headroom lays them out).  gfx950 only.
//
// The selection order is one word (fit_core.h score_of): a pod without GPUs takes the feasible nodes without GPUs in index order, then
// the other feasible nodes in index order; a pod that requests GPUs takes the feasible nodes in index order (nhd/Matcher.py:393-421).
//
//   grid = (blocks, pods).  A block derives its pod's masks in LDS (NHDFIT_LONE_POD_MASKS_OF, step_kernel.h: k_find1's own text).
//   Scan, lane = node: the block's contiguous chunk range is cut four ways, a wavefront per piece - node_index + lone_pod_fits with
//     the busy window, the candidate mask applied (bits beyond n ignored), a candidate held as a wide record counted instead; one
//     ballot for "fits", one for "fits and has no GPU".  A wavefront keeps its first K of each kind (all a list of K can need from
//     it) and its popcounts; wavefront 0 strings the four together and posts the block's record - two counts, at most K "fits"
//     entries (bit 31: the node is a preferred one), at most K preferred entries - and one atomic per summary field.
//   Pick and map, in the block that takes the pod's last ticket (find1_launch's pattern: plain stores, ONE agent-scope release by one
//     lane behind the block's barrier, a relaxed agent-scope fetch-add; the last block acquires once and reads the records with
//     agent-scope loads): cand_pick_wave below merges the per-block firsts in block order - preferred nodes, then the rest without
//     them.  Then wavefront = entry: planes 0-4 and the detail record into the wavefront's LDS slice, lone_nic_bits ->
//     map_on_state_wave, the 32-byte entry stored.  k_headroom's phase B with no commit.
// Every loop has a bound known before it starts: the chunk range, the block count, K.  No spin wait, no block waits for another.
// Nothing but the call's own buffers is written.
//
// G4 as k_headroom: false - pods of one to three processing groups, neither set model compiled in, no private segment; true - four
// groups, and every pod where a tuning aid switched a mapping table off.  Each instantiation answers its own pods of a call.

// ---- the pick with the wavefront's lanes ----------------------------------------------------------------------------------------------
constexpr uint32_t kCandPref = 0x80000000u;          // bit 31 of an entry: the node has no GPU and the pod requests none
// a block's record, in 32-bit words: [0] "fits" entries, [1] preferred entries (each min(count, K)), [2..3] unused, [4, 4 + K) the first
// "fits" nodes by local index | kCandPref, [4 + K, 4 + 2K) the first preferred nodes by local index
constexpr uint32_t cand_rec_words(uint32_t K) { return 4u + 2u * K; }
// `recs`: the records of the pod's `nb` blocks in block order, which is index order (each block scans one contiguous chunk range).
// Stores the first K nodes in selection order into `list` (local index | kCandPref) and returns how many; every lane returns the same.
// A "fits" entry that is preferred is always one of its block's first K preferred ones (the preferred nodes are a subsequence of
// the "fits" nodes), so either the first pass listed it or the first pass filled the list: the second pass skips it by its flag.
// (tests/harness/candidates_pick_emul.cpp runs this text on emulated lanes.)
__device__ __forceinline__ uint32_t cand_pick_wave(const uint32_t* recs, uint32_t nb, uint32_t K, uint32_t* list, uint32_t lane) {
    const uint32_t stride = cand_rec_words(K);
    uint32_t n = 0;
    for (uint32_t b = 0; b < nb && n < K; ++b) {                         // the preferred nodes
        const uint32_t* rec = recs + (size_t)b * stride;
        const uint32_t np = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        if (lane < np && n + lane < K) list[n + lane] = __hip_atomic_load(rec + 4u + K + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) | kCandPref;
        n += np;
    }
    n = n < K ? n : K;
    for (uint32_t b = 0; b < nb && n < K; ++b) {                         // then the rest, without them
        const uint32_t* rec = recs + (size_t)b * stride;
        const uint32_t na = (uint32_t)__builtin_amdgcn_readfirstlane((int)__hip_atomic_load(rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        const uint32_t v = lane < na ? __hip_atomic_load(rec + 4u + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : kCandPref;
        const bool keep = !(v & kCandPref);
        const uint64_t m = __ballot(keep);
        const uint32_t pos = n + (uint32_t)popc64(m & ((1ull << lane) - 1ull));
        if (keep && pos < K) list[pos] = v;
        n += (uint32_t)popc64(m);
    }
    return n < K ? n : K;
}

// ---- the launch -------------------------------------------------------------------------------------------------------------------
struct CandSum { uint32_t feasible, preferred, returned, not_evaluated, form, reserved[3]; };
static_assert(sizeof(CandSum) == sizeof(nhdfit_candidates_sum) && sizeof(CandSum) == 32, "the summary record of include/nhdfit.h");
static_assert(sizeof(nhdfit_candidate) == 32 && offsetof(nhdfit_candidate, map) == 8, "the entry of include/nhdfit.h");

struct CandArgs {
    const nhdfit_plane0* p0; const nhdfit_plane1* p1; const nhdfit_plane2* p2; const nhdfit_plane3* p3; const nhdfit_plane4* p4;
    const nhdfit_detail* det; uint32_t n;
    uint64_t global_base;
    const nhdfit_wide_node* wide; uint32_t n_wide;
    const nhdfit_req* reqs;                          // [gridDim.y] pods
    DictView d; uint32_t nsig, fc_dim, fg_dim, ngs;
    MapTables mt; uint32_t ncls;
    double busy_from;
    const uint64_t* cand;                            // optional [chunks]
    uint32_t chunks, K;
    uint32_t all_generic;                            // the mapping tables are incomplete (tuning aids): every pod takes k_cand_list<true>
    uint32_t* tickets;                               // [pods], zeroed by the caller
    CandSum* sum;                                    // [pods], zeroed by the caller
    uint32_t* recs;                                  // [pods][gridDim.x][cand_rec_words(K)], zeroed by the caller
    nhdfit_candidate* out;                           // [pods][K], zeroed by the caller
};
constexpr uint32_t kCandBlock = 256, kCandWaves = kCandBlock / 64;
constexpr size_t kCandLds = kLoneLds + lds_slice(kCandWaves * sizeof(NodeState)) + lds_slice(kCandWaves * sizeof(nhdfit_detail)) +
                            lds_slice(NHDFIT_MAX_CLASSES * sizeof(double)) + lds_slice(kCandWaves * 2 * 64 * sizeof(uint32_t)) +
                            lds_slice(kCandWaves * 4 * sizeof(uint32_t)) + lds_slice(2 * 64 * sizeof(uint32_t)) + lds_slice(64 * sizeof(uint32_t)) +
                            lds_slice(4 * sizeof(uint32_t));

template <bool G4>
__global__ __launch_bounds__(kCandBlock) void k_cand_list(CandArgs a) {
    const uint32_t pod = blockIdx.y;
    {   // (block-uniform) the other instantiation answers this pod
        const uint32_t ng = a.reqs[pod].n_groups, mt = a.reqs[pod].map_type;
        const bool four = (mt == NHDFIT_MAP_NUMA || mt == NHDFIT_MAP_PCI) && ng > 3u && ng <= (uint32_t)kMaxG;
        if ((four || a.all_generic) != G4) return;
    }
    extern __shared__ __align__(16) uint8_t lds_all[];
    uint8_t* lds = lds_all;
    NHDFIT_LONE_LDS(lds)
    (void)s_best;
    NodeState* s_st = carve<NodeState>(lds, kCandWaves);
    nhdfit_detail* s_dd = carve<nhdfit_detail>(lds, kCandWaves);
    double* s_caps = carve<double>(lds, NHDFIT_MAX_CLASSES);
    uint32_t* s_wfirst = carve<uint32_t>(lds, kCandWaves * 2 * 64);      // [wavefront][fits, preferred][K]: a wavefront's firsts
    uint32_t* s_wcnt = carve<uint32_t>(lds, kCandWaves * 4);             // [wavefront]: fits, preferred, wide candidates
    uint32_t* s_first = carve<uint32_t>(lds, 2 * 64);                    // the block's firsts
    uint32_t* s_list = carve<uint32_t>(lds, 64);                         // the pod's list (last block)
    uint32_t* s_word = carve<uint32_t>(lds, 4);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const uint32_t K = a.K, nb = gridDim.x;

    // (a dictionary stream beyond the LDS slice is read where it lies, once per block, as k_headroom does)
    NHDFIT_LONE_POD_MASKS_OF(kCandBlock, tid, a.reqs + pod, a.d, a.nsig, a.fc_dim, a.fg_dim, a.d.flat_words <= kDictLdsWords)
    (void)W; (void)G;
    if (tid < (uint32_t)NHDFIT_MAX_CLASSES) s_caps[tid] = tid < a.ncls ? a.d.caps[tid] : 0.0;
    const LoneMasks t{s_a0, s_a1, s_w0, s_w1, s_r0, s_r1};
    const PodHeader h = *s_hdr;
    const bool needs_gpu = (h.flags & kPodNeedGpu) != 0;

    // ---- scan: lane = node, a contiguous piece of the block's chunk range per wavefront
    {
        const uint32_t c_lo = (uint32_t)((uint64_t)a.chunks * blockIdx.x / nb), c_hi = (uint32_t)((uint64_t)a.chunks * (blockIdx.x + 1) / nb);
        const uint32_t w_lo = c_lo + (uint32_t)((uint64_t)(c_hi - c_lo) * wave / kCandWaves), w_hi = c_lo + (uint32_t)((uint64_t)(c_hi - c_lo) * (wave + 1) / kCandWaves);
        uint32_t* wf_any = s_wfirst + wave * 128u;
        uint32_t* wf_pref = wf_any + 64u;
        uint32_t n_any = 0, n_pref = 0, n_off = 0;                       // (wavefront-uniform)
        const uint64_t below = (1ull << lane) - 1ull;
        for (uint32_t c = w_lo; c < w_hi; ++c) {
            const uint32_t i = c * 64u + lane;
            bool ok = false, nogpu = false, off = false;
            if (i < a.n && (!a.cand || (a.cand[c] >> lane & 1ull))) {
                if (a.n_wide && wide_slot_of(a.wide, a.n_wide, i) >= 0) off = true;          // answered by its wide record: counted, not listed
                else {
                    const NodeIdx ni = node_index(a.p0[i], a.p1[i], a.p2[i], a.p4[i], a.fc_dim, a.fg_dim, a.ngs);
                    nogpu = ni.nogpu != 0;
                    ok = lone_pod_fits(t, h, ni, a.p3[i], a.p4[i].busy_time >= a.busy_from, a.d.group_sets);
                }
            }
            const uint64_t word = __ballot(ok), pref = needs_gpu ? 0ull : __ballot(ok && nogpu);
            const bool mine = (pref >> lane & 1ull) != 0;
            if (ok) {
                const uint32_t pos = n_any + (uint32_t)popc64(word & below);
                if (pos < K) wf_any[pos] = i | (mine ? kCandPref : 0u);
            }
            if (mine) {
                const uint32_t pos = n_pref + (uint32_t)popc64(pref & below);
                if (pos < K) wf_pref[pos] = i;
            }
            n_any += (uint32_t)popc64(word); n_pref += (uint32_t)popc64(pref);
            if (a.n_wide) n_off += (uint32_t)popc64(__ballot(off));
        }
        if (lane == 0u) { s_wcnt[wave * 4u] = n_any; s_wcnt[wave * 4u + 1u] = n_pref; s_wcnt[wave * 4u + 2u] = n_off; }
    }
    __syncthreads();
    // ---- the block's record, by wavefront 0: the wavefronts' firsts in order, cut at K
    uint32_t* recs = a.recs + (size_t)pod * nb * cand_rec_words(K);
    if (wave == 0u) {
        uint32_t tot_any = 0, tot_pref = 0, tot_off = 0, base_any = 0, base_pref = 0;
        for (uint32_t w = 0; w < kCandWaves; ++w) {
            const uint32_t wa = s_wcnt[w * 4u], wp = s_wcnt[w * 4u + 1u];
            const uint32_t ca = wa < K ? wa : K, cp = wp < K ? wp : K;
            if (lane < ca && base_any + lane < K) s_first[base_any + lane] = s_wfirst[w * 128u + lane];
            if (lane < cp && base_pref + lane < K) s_first[64u + base_pref + lane] = s_wfirst[w * 128u + 64u + lane];
            base_any += ca; base_pref += cp;
            tot_any += wa; tot_pref += wp; tot_off += s_wcnt[w * 4u + 2u];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        uint32_t* rec = recs + (size_t)blockIdx.x * cand_rec_words(K);
        const uint32_t na = tot_any < K ? tot_any : K, np = tot_pref < K ? tot_pref : K;
        if (lane == 0u) { rec[0] = na; rec[1] = np; }
        if (lane < na) rec[4u + lane] = s_first[lane];
        if (lane < np) rec[4u + K + lane] = s_first[64u + lane];
        CandSum* q = a.sum + pod;
        const uint32_t mine = lane == 0u ? tot_any : lane == 1u ? tot_pref : tot_off;
        if (lane < 3u && mine) {                                         // one atomic per (block, pod, field)
            uint32_t* f = lane == 0u ? &q->feasible : lane == 1u ? &q->preferred : &q->not_evaluated;
            (void)__hip_atomic_fetch_add(f, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    // ---- the ticket behind the block's stores; the last block goes on
    const uint32_t ticket = publish_and_count(&a.tickets[pod], true);
    if (tid == 0u) {
        if (ticket == nb - 1u) { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); NHDFIT_DRAIN_VMEM(); }    // every block's record
        s_word[0] = ticket;
    }
    __syncthreads();
    if (s_word[0] != nb - 1u) return;                                    // (block-uniform)

    // ---- pick
    if (wave == 0u) {
        const uint32_t cnt = cand_pick_wave(recs, nb, K, s_list, lane);
        if (lane == 0u) { s_word[1] = cnt; a.sum[pod].returned = cnt; }
    }
    __syncthreads();
    const uint32_t count = s_word[1];
    // ---- map: wavefront = entry
    NodeState& st = s_st[wave];
    nhdfit_detail& dd = s_dd[wave];
    const bool pci = r.map_type == NHDFIT_MAP_PCI;
    for (uint32_t j = wave; j < count; j += kCandWaves) {                 // (at most K / 4 turns)
        const uint32_t e = s_list[j], v = e & ~kCandPref;
        uint32_t* sw = reinterpret_cast<uint32_t*>(&st);
        if (lane < 5u) {                                                 // the node's planes: a 16-byte load per lane
            const uint4 q = lane == 0u ? *reinterpret_cast<const uint4*>(a.p0 + v) : lane == 1u ? *reinterpret_cast<const uint4*>(a.p1 + v) :
                            lane == 2u ? *reinterpret_cast<const uint4*>(a.p2 + v) : lane == 3u ? *reinterpret_cast<const uint4*>(a.p3 + v) :
                                         *reinterpret_cast<const uint4*>(a.p4 + v);
            sw[lane * 4 + 0] = q.x; sw[lane * 4 + 1] = q.y; sw[lane * 4 + 2] = q.z; sw[lane * 4 + 3] = q.w;
        }
        if (lane >= 8u && lane < 8u + sizeof(nhdfit_detail) / 16) {
            const uint4 q = reinterpret_cast<const uint4*>(a.det + v)[lane - 8u];
            uint32_t* dw = reinterpret_cast<uint32_t*>(&dd) + (lane - 8u) * 4u;
            dw[0] = q.x; dw[1] = q.y; dw[2] = q.z; dw[3] = q.w;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        nhdfit_mapping mp;
        (void)map_on_state_wave<G4, G4>(r, st, dd, s_caps, lone_nic_bits(t, pci, st.p3), a.mt, lane, mp);   // every lane: the same mapping (zeros when nothing maps)
        if (lane == 0u) {
            nhdfit_candidate* o = a.out + (size_t)pod * K + j;
            o->score = score_of((e & kCandPref) != 0u, a.global_base + v);
            o->map = mp;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();                                 // (the slice is the next entry's)
    }
}
