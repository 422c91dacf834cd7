// big_candidates_kernel.h - nhdfit_candidates_big on the device: the first K nodes FindNode would pick for a BIG request (a pod of
// 5..8 processing groups, nhdfit_big_req), each with its mapping (k_big_cand_scan, k_big_cand_pick, k_big_cand_map).  Device code of
// libnhdfit.so; included by nhdfit.hip inside its anonymous namespace, behind big_kernel.h (BigWaveLds, WideStagesLds) and
// candidates_kernel.h (cand_pick_wave, the records' layout, CandSum, kCandPref).  gfx950 only.
//
// A big request is answered the way k_big_eval answers it: every node through the general path's eyes - an ordinary node through
// wide_view, a wide node from its record - with wide_fits under the (pod, node) pair's NIC search budget.  Three launches on one
// stream (four where the mirror has nodes for either form of the mapping); stream order is every hand-off there is.
//
//   k_big_cand_scan, grid = (blocks, pods), a block is ONE wavefront, lane = node.  The first `nb_planes` blocks share out the 64-node
//     chunks of the planes' nodes, the others the 64-slot chunks of the wide records: no block has units of both, each block takes a
//     contiguous chunk range, and within either range unit order is index order (the records are sorted by index) - across them it is
//     not.  Per lane k_big_eval's verdict: the candidate bit at view.index, view.numa_nodes != 0 (a placeholder of the planes has none:
//     its record answers, in the other range), wide_fits with the busy flag; two ballots per chunk, "fits" and "fits and preferred"
//     (the pod requests no GPU and the node has none).  The block keeps its first K of each kind by prefix popcount and posts them as
//     a record of cand_rec_words(K) words holding node INDEXES, and adds its counts to the pod's summary record, one atomic per
//     non-zero field.  A pair that runs out of search budget raises flags[1], as in k_big_eval.  A block evaluates its whole range:
//     `feasible` is a count.
//   k_big_cand_pick, grid = pods, ONE wavefront: cand_pick_wave over the planes' blocks and again over the wide blocks, the two lists'
//     score words merged by the rule of candidates_merge.h and cut at K.  Lane j settles entry j: its node (index | kCandPref, or
//     kBigCandNone past the list's end), the map launch's work item (node, wide slot or -1, pod) and the entry's score word.
//   k_big_cand_map, grid = workers: a worker loop over the (pod, entry) pairs as k_big_map loops over pods - the same text per pair:
//     the node's view and the request into LDS, wide_map_wave where the set tables fit LDS and the node has at most two NUMA nodes,
//     one-thread wide_map on the worker's scratch otherwise; lane 0 stores the entry's mapping.  The two forms are two
//     instantiations of the kernel, each taking its own pairs (see the kernel).
// Every loop has a bound known before it starts: the chunk range, the block counts, K, pods x K pairs, U^(G+1) tuples.  No spin wait,
// no block waits for another.  Nothing but the call's own buffers is written.
//
// The kernels are templates over the mirror's kind (Sharing: the wide records' NICs are priced by their share records), so they are
// emitted behind every function the code object already had (wide_candidates_kernel.h has the reason).

// ---- the scan's records and the two-range pick with the wavefront's lanes -----------------------------------------------------------
// (tests/harness/big_candidates_scan_emul.cpp runs this text on emulated lanes against a scalar statement of the selection order.)
// One chunk of a block's range: `ok` - the lane's unit fits -, `pref_node` - and is a preferred one -, `index` its node.  The block's
// first K of each kind go into `first` ([0, 64) "fits" by index | kCandPref, [64, 128) preferred), the counts go up; every lane calls.
__device__ __forceinline__ void big_cand_keep(bool ok, bool pref_node, uint32_t index, uint32_t K, uint32_t lane, uint32_t* first, uint32_t& n_any,
                                              uint32_t& n_pref) {
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t word = __ballot(ok), pref = __ballot(ok && pref_node);
    const bool mine = (pref >> lane & 1ull) != 0;
    if (ok) {
        const uint32_t pos = n_any + (uint32_t)popc64(word & below);
        if (pos < K) first[pos] = index | (mine ? kCandPref : 0u);
    }
    if (mine) {
        const uint32_t pos = n_pref + (uint32_t)popc64(pref & below);
        if (pos < K) first[64u + pos] = index;
    }
    n_any += (uint32_t)popc64(word); n_pref += (uint32_t)popc64(pref);
}
// The block's record (cand_rec_words(K) words, candidates_kernel.h) from its firsts and counts.
__device__ __forceinline__ void big_cand_post(uint32_t* rec, const uint32_t* first, uint32_t n_any, uint32_t n_pref, uint32_t K, uint32_t lane) {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const uint32_t na = n_any < K ? n_any : K, np = n_pref < K ? n_pref : K;
    if (lane == 0u) { rec[0] = na; rec[1] = np; }
    if (lane < na) rec[4u + lane] = first[lane];
    if (lane < np) rec[4u + K + lane] = first[64u + lane];
}
// A pod's list from its blocks' records - `nb_planes` blocks of the planes' nodes, then `nb_wide` of the wide records, each range in
// index order: cand_pick_wave over either, the two lists' score words merged by the rule of candidates_merge.h and cut at K.  Lane j
// below K stores entry j (index | kCandPref) into `list`, or kBigCandNone past the list's end; every lane returns the count.  plist, wlist,
// pscore, wscore: 64 words of LDS each.
constexpr uint32_t kBigCandNone = 0xFFFFFFFFu;      // no entry: as a node index it is beyond any mirror
__device__ __forceinline__ uint32_t big_cand_pick2(const uint32_t* recs, uint32_t nb_planes, uint32_t nb_wide, uint32_t K, uint64_t global_base,
                                                   uint32_t* plist, uint32_t* wlist, uint64_t* pscore, uint64_t* wscore, uint32_t* list, uint32_t lane) {
    const uint32_t n_planes = cand_pick_wave(recs, nb_planes, K, plist, lane);
    const uint32_t n_wide = cand_pick_wave(recs + (size_t)nb_planes * cand_rec_words(K), nb_wide, K, wlist, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    pscore[lane] = lane < n_planes ? score_of((plist[lane] & kCandPref) != 0u, global_base + (plist[lane] & ~kCandPref)) : 0ull;
    wscore[lane] = lane < n_wide ? score_of((wlist[lane] & kCandPref) != 0u, global_base + (wlist[lane] & ~kCandPref)) : 0ull;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    bool from_wide = false;
    uint32_t pos = 0;
    if (lane < K) {                                                       // lane = entry: at most lane + 1 turns
        const bool has = cand_merged_entry(pscore, n_planes, wscore, n_wide, lane, from_wide, pos);
        list[lane] = !has ? kBigCandNone : from_wide ? wlist[pos] : plist[pos];
    }
    return n_planes + n_wide < K ? n_planes + n_wide : K;
}

// ---- the launches -----------------------------------------------------------------------------------------------------------------
struct BigCandArgs {
    const nhdfit_plane0* p0; const nhdfit_plane1* p1; const nhdfit_plane2* p2; const nhdfit_plane3* p3; const nhdfit_plane4* p4;
    const nhdfit_detail* det; uint32_t n;
    const nhdfit_wide_node* wide; uint32_t n_wide;
    const nhdfit_wide_share* share;                  // [n_wide] under Sharing
    const nhdfit_big_req* reqs; uint32_t P;          // [P] pods
    const double* caps; double busy_from;
    const uint64_t* cand;                            // optional [chunks of the planes' nodes]
    uint32_t chunks, wchunks, nb_planes, nb_wide, K; // 64-unit chunks and blocks per pod of either range
    uint64_t global_base;
    CandSum* sum;                                    // [P], zeroed by the caller
    uint32_t* recs;                                  // [P][nb_planes + nb_wide][cand_rec_words(K)], zeroed by the caller
    uint32_t* list;                                  // [P][K] the picked nodes in selection order: index | kCandPref, kBigCandNone past the end
    uint4* items;                                    // [P][K] k_big_cand_map's work: (node index or kBigCandNone, wide slot or -1, pod, the node's NUMA nodes)
    nhdfit_big_candidate* out;                       // [P][K], zeroed by the caller; k_big_cand_pick stores the score words
    uint32_t* flags;                                 // [0] a set of the model outgrew its table, [1] a (pod, node) pair ran out of NIC search budget
};
// k_big_cand_map's: BigMapArgs with the picked pairs in the scores' place (what names a pair's node was settled by k_big_cand_pick)
struct BigCandMapArgs {
    const nhdfit_plane0* p0; const nhdfit_plane1* p1; const nhdfit_plane2* p2; const nhdfit_plane3* p3; const nhdfit_plane4* p4;
    const nhdfit_detail* det;
    const nhdfit_wide_node* wide;
    const nhdfit_big_req* reqs; uint32_t pairs;      // pairs = pods x K <= 65 535 x 64
    const double* caps;
    const uint4* items;                              // [pairs]
    nhdfit_big_candidate* out;                       // [pairs]
    int32_t* scratch;                                // [workers][stride]: the set tables of one mapping each (wide_core.h big_scratch_words)
    size_t stride; int32_t slots_g, slots_c; uint32_t workers;
    uint32_t lds_tables;                             // the set tables of a mapping fit the block's LDS (launched with stride * 4 bytes of it)
    uint32_t* flags;
    const nhdfit_wide_share* share;                  // [n_wide] under Sharing
};
static_assert(sizeof(nhdfit_big_candidate) == 48 && offsetof(nhdfit_big_candidate, map) == 8, "the entry of include/nhdfit.h");
constexpr uint32_t kBigCandBlock = 64;

template <bool Sharing>
__global__ __launch_bounds__(kBigCandBlock) void k_big_cand_scan(BigCandArgs a) {
    __shared__ uint32_t s_first[2 * 64];                                 // the block's firsts: "fits", preferred
    const uint32_t pod = blockIdx.y, lane = threadIdx.x, K = a.K, nb = a.nb_planes + a.nb_wide;
    const nhdfit_big_req& r = a.reqs[pod];
    uint32_t want = 0;
    for (uint32_t g = 0; g < r.n_groups && g < (uint32_t)NHDFIT_BIG_MAX_GROUPS; ++g) want += r.gpus[g];
    const bool gpuless = want == 0u;
    // (block-uniform) the block's range: chunks of the planes' nodes, or of the wide records
    const bool of_wide = blockIdx.x >= a.nb_planes;
    const uint32_t b = of_wide ? blockIdx.x - a.nb_planes : blockIdx.x, parts = of_wide ? a.nb_wide : a.nb_planes;
    const uint32_t total = of_wide ? a.wchunks : a.chunks, units = of_wide ? a.n_wide : a.n;
    const uint32_t c_lo = (uint32_t)((uint64_t)total * b / parts), c_hi = (uint32_t)((uint64_t)total * (b + 1) / parts);
    uint32_t n_any = 0, n_pref = 0;                                      // (wavefront-uniform)
    for (uint32_t c = c_lo; c < c_hi; ++c) {
        const uint32_t u = c * 64u + lane;
        bool ok = false, nogpu = false;
        uint32_t index = 0;
        if (u < units) {
            nhdfit_wide_node view;
            if (of_wide) view = a.wide[u];
            else wide_view(a.p0[u], a.p1[u], a.p2[u], a.p3[u], a.p4[u], a.det[u], u, view);
            index = view.index;
            const bool listed = index < a.n && (!a.cand || (a.cand[index >> 6] >> (index & 63u) & 1ull));
            if (listed && view.numa_nodes) {
                NicSearch ns{NHDFIT_BIG_NIC_BUDGET, false};
                ok = wide_fits(view, r, view.busy_time >= a.busy_from, WideCaps(a.caps, Sharing && of_wide ? a.share + u : nullptr), &ns);
                if (ns.exhausted) atomicOr(&a.flags[1], 1u);
                nogpu = view.n_gpus == 0;
            }
        }
        big_cand_keep(ok, gpuless && nogpu, index, K, lane, s_first, n_any, n_pref);
    }
    big_cand_post(a.recs + ((size_t)pod * nb + blockIdx.x) * cand_rec_words(K), s_first, n_any, n_pref, K, lane);
    CandSum* q = a.sum + pod;
    const uint32_t mine = lane == 0u ? n_any : n_pref;
    if (lane < 2u && mine) {                                             // one atomic per (block, pod, field)
        uint32_t* f = lane == 0u ? &q->feasible : &q->preferred;
        (void)__hip_atomic_fetch_add(f, mine, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <bool Sharing>
__global__ __launch_bounds__(kBigCandBlock) void k_big_cand_pick(BigCandArgs a) {
    __shared__ uint32_t s_plist[64], s_wlist[64];                        // either range's firsts in selection order: index | kCandPref
    __shared__ uint64_t s_pscore[64], s_wscore[64];                      // their score words
    const uint32_t pod = blockIdx.x, lane = threadIdx.x, K = a.K, nb = a.nb_planes + a.nb_wide;
    uint32_t* list = a.list + (size_t)pod * K;
    (void)big_cand_pick2(a.recs + (size_t)pod * nb * cand_rec_words(K), a.nb_planes, a.nb_wide, K, a.global_base, s_plist, s_wlist, s_pscore, s_wscore,
                         list, lane);
    if (lane < K) {                                                      // lane = entry (its own store of `list`): the map launch's work item
        const uint32_t e = list[lane], v = e & ~kCandPref;
        const bool has = e != kBigCandNone && v < a.n;                   // (the scan posted indexes of the mirror)
        const int slot = has && a.n_wide ? wide_slot_of(a.wide, a.n_wide, v) : -1;
        const uint32_t numa = slot >= 0 ? a.wide[slot].numa_nodes : (uint32_t)NHDFIT_MAX_NUMA;     // (a node of the planes has at most two)
        a.items[(size_t)pod * K + lane] = make_uint4(has ? v : kBigCandNone, (uint32_t)slot, pod, numa);
        if (has) a.out[(size_t)pod * K + lane].score = score_of((e & kCandPref) != 0u, a.global_base + v);
    }
}

// wide_map_wave (big_kernel.h) - its lines, COPIED here as a template inlined into its one caller, so that wide_map_wave keeps its one
// call site and k_big_map and it compile to the parent's code (a second caller changed both).  Same stages with lane = tuple, same
// model on the first lane: the mapping is wide_map's, bit for bit (tests/test_candidates_big_gpu.py holds every entry to nhdfit_big_find's).
template <bool Sharing>
__device__ __forceinline__ int big_cand_map_wave(BigWaveLds& t, const WideCaps& caps, int32_t* tables, nhdfit_big_mapping& out, int32_t slots_g, int32_t slots_c, uint32_t lane) {
    const nhdfit_wide_node& n = t.view;
    const nhdfit_big_req& r = t.req;
    wide_map_clear(out, NHDFIT_BIG_MAX_GROUPS);
    if (!req_valid(r) || !wide_shape_ok(n)) return 0;
    const WideFree f = wide_free(n);
    const uint32_t G = r.n_groups, U = f.U, nG = wide_ipow(U, G), nC = nG * U;
    const bool separable = nic_separable(n, r);
    NicSearch ns{8u * NHDFIT_BIG_NIC_BUDGET, false};              // (a lane that alone outruns the call's budget has outrun it)
    for (uint32_t base = 0; base < nG; base += 64) {
        const uint32_t code = base + lane;
        bool g = false, k = false;
        if (code < nG) {
            g = wide_gpu_ok(r, f, code);
            k = nic_stage_ok_plain(separable, n, r, caps, code, &ns);
            t.hash_g[code] = wide_tuple_hash(code, G, U);
        }
        const uint64_t mg = __ballot(g), mk = __ballot(k);
        if (lane == 0) { t.bit_g[base >> 6] = mg; t.bit_n[base >> 6] = mk; }
    }
    for (uint32_t base = 0; base < nC; base += 64) {
        const uint32_t code = base + lane;
        bool ok = false;
        if (code < nC) {
            ok = wide_cpu_ok(r, f, code);
            t.hash_c[code] = wide_tuple_hash(code, G + 1, U);
        }
        const uint64_t mc = __ballot(ok);
        if (lane == 0) t.bit_c[base >> 6] = mc;
    }
    t.steps[lane] = 8u * NHDFIT_BIG_NIC_BUDGET - ns.left;
    const bool any_out = __ballot(ns.exhausted) != 0ull;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    if (lane == 0) {
        uint64_t total = 0;
        for (int l = 0; l < 64; ++l) total += t.steps[l];
        int rc = -2;                                              // the budget of the call's searches, summed over the tuples as one thread spends it
        if (!any_out && total <= (uint64_t)(8u * NHDFIT_BIG_NIC_BUDGET)) {
            WideStagesLds st{t};
            rc = wide_map_model(n, r, caps, f, tables, out, slots_g, slots_c, st);
        }
        t.rc = rc;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    return t.rc;
}

// Wave: true - the pairs whose tables fit LDS on a node of at most two NUMA nodes, mapped by wide_map_wave's lines (lane = tuple); false -
// the others, mapped by one thread (wide_map on LDS tables or on the worker's scratch).  Each instantiation takes its own pairs of
// the call and skips the other's; the host launches the one-thread form only where the mirror can have such a pair.  Two kernels and
// not k_big_map's one: with both forms in one frame the general set model's registers push the loop's scalars out on the wavefront
// path as well (profiles/r18/README.md), and a device function of its own for either form would be emitted in FRONT of the existing
// kernels and move them (wide_candidates_kernel.h has what that did to the step kernel's timing) - kernel templates come last.
template <bool Sharing, bool Wave>
__global__ __launch_bounds__(kBigCandBlock) void k_big_cand_map(BigCandMapArgs a) {
    extern __shared__ __align__(16) int32_t s_tables[];
    __shared__ BigWaveLds s_wave;
    const uint32_t tid = blockIdx.x, lane = threadIdx.x;                 // one mapping per wavefront at a time
    if (tid >= a.workers) return;
    int32_t* scratch = a.lds_tables ? s_tables : a.scratch + (size_t)tid * a.stride;   // (k_big_map's choice)
    for (uint32_t i = tid; i < a.pairs; i += a.workers) {                // pair i: entry i % K of pod i / K
        const uint4 w = a.items[i];                                      // (node, wide slot or -1, pod, the node's NUMA nodes)
        const uint32_t v = w.x;
        if (v == kBigCandNone) continue;                                 // (wavefront-uniform) the list ends before this entry: it stays zero
        if ((a.lds_tables && w.w <= 2u) != Wave) continue;               // (wavefront-uniform) the other instantiation's pair
        const int slot = (int)w.y;
        nhdfit_big_mapping m;
        wide_map_clear(m, NHDFIT_BIG_MAX_GROUPS);
        if (lane == 0) {
            if (slot >= 0) s_wave.view = a.wide[slot];
            else wide_view(a.p0[v], a.p1[v], a.p2[v], a.p3[v], a.p4[v], a.det[v], v, s_wave.view);
        }
        reinterpret_cast<uint32_t*>(&s_wave.req)[lane] = reinterpret_cast<const uint32_t*>(&a.reqs[w.z])[lane];     // (256 bytes: a dword per lane)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const WideCaps caps(a.caps, Sharing && slot >= 0 ? a.share + slot : nullptr);
        int rc = 0;
        if (Wave) rc = big_cand_map_wave<Sharing>(s_wave, caps, scratch, m, a.slots_g, a.slots_c, lane);
        else if (lane == 0) rc = wide_map(s_wave.view, s_wave.req, caps, scratch, m, a.slots_g, a.slots_c);
        if (lane == 0) {
            if (rc < 0) { m.valid = 0; atomicOr(&a.flags[rc == -2 ? 1 : 0], 1u); }
            a.out[i].map = m;                                            // (the score word is in place)
        }
        __builtin_amdgcn_wave_barrier();                                  // (the LDS record is the next mapping's)
    }
}
