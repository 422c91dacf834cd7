// headroom_kernel.h - nhdfit_headroom on the device: how many more replicas of a pod template each node can take (k_headroom).
// Device code of libnhdfit.so; included by nhdfit.hip inside its anonymous namespace, behind find1_commit.h (the lone-pod masks of
// step_kernel.h, the wavefront forms of the mapping and of the commit step - seq_kernel.h, seq2_kernel.h) and wide_kernel.h
// (wide_slot_of).  gfx950 only.
//
// headroom(node, template) = the number of times FindNode -> SetPhysicalIdsFromMapping -> ClaimPodNICResources
// (nhd/NHDScheduler.py:277-304) succeeds back to back on a private copy of the node with IsBusy() false (include/nhdfit.h).  The
// question is parallel over the nodes - a commit only ever changes its own node - and the pieces exist: find1_commit.h chains
// find -> map -> commit once, for one node; this kernel runs that chain to exhaustion on a private copy of every node at once.
//
//   grid = (blocks, templates).  A block derives its template's masks in LDS (NHDFIT_LONE_POD_MASKS_OF, step_kernel.h: k_find1's own text)
//   and then takes 64-node chunks off the template's ticket counter until the tickets run out - nodes differ by orders of
//   magnitude in work (0 replicas against hundreds), a fixed split would leave the chip waiting for one block.  The counter is a
//   relaxed agent-scope fetch-add: it hands out work, it publishes nothing, no fence.  Per chunk:
//   Phase A, lane = node (every wavefront of the block, the same answer): node_index + lone_pod_fits with "not busy", the
//     candidate mask applied, one ballot.  A candidate the mirror holds as a wide record is flagged NOT_EVALUATED instead.  In a
//     full cluster most nodes end here with 0 and cost what a k_find1 sweep costs.
//   Phase B, wavefront = node: the chunk's set bits are dealt round robin to the block's wavefronts.  Planes 0-4 and the detail
//     record go into the wavefront's own LDS slice (464 bytes with the placement record the commit writes), then
//     lone_nic_bits -> map_on_state_wave -> commit_node_wave on the LDS copy -> node_index / lone_pod_fits on the new state, until
//     it no longer fits, the cap is reached, or the commit reports kCommitWouldRaise / kCommitNewSig (stop, flag, do not count).
//     Nothing is written back.  Where the caller asks for it (HeadroomArgs::final, nhdfit_headroom_limits) the copy a run of at
//     least one replica ended in is stored - planes 0-4 and the detail record, 208 bytes - for k_limit_stage (limit_kernel.h).
//   Results: wavefront 0 stores the chunk's 64 entries as one coalesced 128-byte row of uint16 and adds the chunk to the block's
//   partial sums in LDS; at the end one atomic per (block, template, field) into the summary record.
// Every loop has a bound known before it starts: the chunk count (tickets), 64 (set bits), max_per_node (replicas).  No spin wait,
// no hand-off between blocks.
//
// G4 = false: the wavefront form proper - templates of one to three processing groups, every shape answered from the mapping tables
// (map_on_state_wave<false, false>: neither the generic set model nor the insertion-by-insertion model is compiled in), no private
// segment at all.  G4 = true: the same kernel with both models compiled in (scratch arrays, 10 KB per lane, as k_decide<true>) for
// templates of four groups, and for every template where a tuning aid switched a table off - same answers, slower.  Each
// instantiation answers its own templates of a call and leaves the others' blocks at once.

// ---- one node's run with the wavefront's lanes --------------------------------------------------------------------------------
// `st` / `dd` / `pl`: the wavefront's LDS copies (modified); every lane returns the same entry: replicas | NHDFIT_HEADROOM_STOPPED.
// The caller knows that the template fits the state it hands in.  (tests/harness/headroom_wave_emul.cpp runs this text on emulated lanes.)
struct HeadroomCtx {                                 // what a node's run reads besides the node: the template's masks and the dictionary
    LoneMasks t; PodHeader h;
    const uint64_t* group_sets; const double* caps;
    MapTables mt; SigTable sigs;
    uint32_t ncls, fc_dim, fg_dim, ngs, cap;
};
template <bool G4>
__device__ __forceinline__ uint32_t headroom_run_wave(NodeState& st, nhdfit_detail& dd, nhdfit_placement& pl, const nhdfit_req& r, const HeadroomCtx& x,
                                                      uint32_t lane) {
    const bool pci = r.map_type == NHDFIT_MAP_PCI;
    const int G = (int)r.n_groups;
    uint32_t k = 0;
    while (k < x.cap) {
        const uint32_t bits = lone_nic_bits(x.t, pci, st.p3);
        nhdfit_mapping mp;
        if (!map_on_state_wave<G4, G4>(r, st, dd, x.caps, bits, x.mt, lane, mp)) break;       // FindNode returns (None,): the run ends, nothing to flag
        bool nic_missing = false;                                        // GetNicObjFromIndex returns None -> IndexError (nhd/Node.py:700-704; k_commit's guard)
#pragma unroll
        for (int g = 0; g < kMaxG; ++g)
            if (g < G) nic_missing |= (uint32_t)mp.nic_idx[g] >= dd.nic_cnt[mp.nic_numa[g] & 1];
        if (nic_missing) return k | NHDFIT_HEADROOM_STOPPED;
        const int status = commit_node_wave(st, dd, r, mp, 0.0, x.sigs, x.ncls, pl, lane);
        if (status != kCommitOk) return k | NHDFIT_HEADROOM_STOPPED;     // the reference raises / a NIC state without a signature: not counted
        ++k;
        const NodeIdx ni = node_index(st.p0, st.p1, st.p2, st.p4, x.fc_dim, x.fg_dim, x.ngs);
        if (!lone_pod_fits(x.t, x.h, ni, st.p3, false, x.group_sets)) break;
    }
    return k;
}

// ---- the launch -------------------------------------------------------------------------------------------------------------------
struct HeadroomFinal { NodeState st; nhdfit_detail dd; };   // a node's private copy as its run left it (nhdfit_headroom_limits)
static_assert(sizeof(HeadroomFinal) == 208 && sizeof(HeadroomFinal) % 16 == 0, "planes 0-4 and the detail record, thirteen 16-byte stores");
struct HeadroomSum { unsigned long long replicas; uint32_t nodes_with_room, max_on_one_node, saturated, stopped, not_evaluated, form; };
static_assert(sizeof(HeadroomSum) == sizeof(nhdfit_headroom_sum) && sizeof(HeadroomSum) == 32, "the summary record of include/nhdfit.h");

// A block's partial sums of one template, in LDS (eight words, zeroed by the block): [0] replicas [1] nodes with room [2] max
// [3] saturated [4] stopped [5] the launch's own count - nodes k_headroom leaves not evaluated, nodes k_wide_room evaluates after all.
// (The host twin's statement of the tally: hrh::account, tests/harness/headroom_host.h.)
struct HeadroomTally {
    unsigned long long* tot;
    // one chunk: every lane of ONE wavefront brings its node's entry `e`; `sixth`: the chunk's nodes that count in slot 5 (wavefront-uniform)
    __device__ __forceinline__ void chunk(uint32_t e, uint32_t cap, uint64_t sixth, uint32_t lane) const {
        const uint32_t k = e & NHDFIT_HEADROOM_COUNT_MASK;
        if (k) { atomicAdd(&tot[0], (unsigned long long)k); atomicMax(&tot[2], (unsigned long long)k); }
        const uint64_t room = __ballot(k != 0u), sat = __ballot(k != 0u && k >= cap), stp = __ballot((e & NHDFIT_HEADROOM_STOPPED) != 0u);
        if (lane == 0u) {
            tot[1] += (unsigned long long)popc64(room); tot[3] += (unsigned long long)popc64(sat);
            tot[4] += (unsigned long long)popc64(stp); tot[5] += (unsigned long long)popc64(sixth);
        }
    }
    // the end of the block, behind its barrier, threads 0..5: one atomic per (block, template, field).  kTakeBack: slot 5 is taken out of
    // not_evaluated (k_headroom counted those nodes; they have a figure now) instead of added to it
    template <bool kTakeBack>
    __device__ __forceinline__ void flush(HeadroomSum* q, uint32_t t) const {
        if (t >= 6u || !tot[t]) return;
        const unsigned long long v = tot[t];
        if (t == 0u) atomicAdd(&q->replicas, v);
        else if (t == 1u) atomicAdd(&q->nodes_with_room, (uint32_t)v);
        else if (t == 2u) atomicMax(&q->max_on_one_node, (uint32_t)v);
        else if (t == 3u) atomicAdd(&q->saturated, (uint32_t)v);
        else if (t == 4u) atomicAdd(&q->stopped, (uint32_t)v);
        else if (kTakeBack) atomicSub(&q->not_evaluated, (uint32_t)v);
        else atomicAdd(&q->not_evaluated, (uint32_t)v);
    }
};

struct HeadroomArgs {
    const nhdfit_plane0* p0; const nhdfit_plane1* p1; const nhdfit_plane2* p2; const nhdfit_plane3* p3; const nhdfit_plane4* p4;
    const nhdfit_detail* det; uint32_t n;
    const nhdfit_wide_node* wide; uint32_t n_wide;
    const nhdfit_req* reqs;                          // [gridDim.y] templates
    DictView d; uint32_t nsig, fc_dim, fg_dim, ngs;
    MapTables mt; SigTable sigs; uint32_t ncls;
    const uint64_t* cand;                            // optional [chunks]
    uint32_t chunks, cap;
    uint32_t all_generic;                            // the mapping tables are incomplete (tuning aids): every template takes k_headroom<true>
    uint32_t* tickets;                               // [templates], zeroed by the caller
    uint16_t* counts;                                // [templates][chunks * 64]
    HeadroomSum* sum;                                // [templates], zeroed by the caller
    HeadroomFinal* final;                            // optional [templates][chunks * 64]: the state each run of >= 1 replica ended in (limit_kernel.h)
};
constexpr uint32_t kHeadroomBlock = 256, kHeadroomWaves = kHeadroomBlock / 64;
constexpr size_t kHeadroomLds = kLoneLds + lds_slice(kHeadroomWaves * sizeof(NodeState)) + lds_slice(kHeadroomWaves * sizeof(nhdfit_detail)) +
                                lds_slice(kHeadroomWaves * sizeof(nhdfit_placement)) + lds_slice(NHDFIT_MAX_CLASSES * sizeof(double)) +
                                lds_slice(64 * sizeof(uint32_t)) + lds_slice(4 * sizeof(uint32_t)) + lds_slice(8 * sizeof(unsigned long long));
static_assert(sizeof(NodeState) % 16 == 0 && sizeof(nhdfit_detail) % 16 == 0, "the wavefronts' slices keep the sixteen-byte alignment of the loads");

template <bool G4>
__global__ __launch_bounds__(kHeadroomBlock) void k_headroom(HeadroomArgs a) {
    const uint32_t tpl = blockIdx.y;
    {   // (block-uniform) the other instantiation answers this template
        const uint32_t ng = a.reqs[tpl].n_groups, mt = a.reqs[tpl].map_type;
        const bool four = (mt == NHDFIT_MAP_NUMA || mt == NHDFIT_MAP_PCI) && ng > 3u && ng <= (uint32_t)kMaxG;
        if ((four || a.all_generic) != G4) return;
    }
    extern __shared__ __align__(16) uint8_t lds_all[];
    uint8_t* lds = lds_all;
    NHDFIT_LONE_LDS(lds)
    (void)s_best;
    NodeState* s_st = carve<NodeState>(lds, kHeadroomWaves);
    nhdfit_detail* s_dd = carve<nhdfit_detail>(lds, kHeadroomWaves);
    nhdfit_placement* s_pl = carve<nhdfit_placement>(lds, kHeadroomWaves);
    double* s_caps = carve<double>(lds, NHDFIT_MAX_CLASSES);
    uint32_t* s_cnt = carve<uint32_t>(lds, 64);                          // the chunk's entries
    uint32_t* s_tick = carve<uint32_t>(lds, 4);
    unsigned long long* s_tot = carve<unsigned long long>(lds, 8);       // the block's partial sums (HeadroomTally)
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));

    // (a dictionary of many NIC signatures - nodes with a dozen NICs of several speeds, every state a commit can produce interned - has
    // a stream beyond the LDS slice: the masks are then derived off global memory, once per block; nothing below reads the stream again)
    NHDFIT_LONE_POD_MASKS_OF(kHeadroomBlock, tid, a.reqs + tpl, a.d, a.nsig, a.fc_dim, a.fg_dim, a.d.flat_words <= kDictLdsWords)
    if (tid < (uint32_t)NHDFIT_MAX_CLASSES) s_caps[tid] = tid < a.ncls ? a.d.caps[tid] : 0.0;
    if (tid < 8u) s_tot[tid] = 0ull;
    HeadroomCtx x;
    x.t = LoneMasks{s_a0, s_a1, s_w0, s_w1, s_r0, s_r1};
    x.h = *s_hdr;
    x.group_sets = a.d.group_sets; x.caps = s_caps; x.mt = a.mt; x.sigs = a.sigs;
    x.ncls = a.ncls; x.fc_dim = a.fc_dim; x.fg_dim = a.fg_dim; x.ngs = a.ngs; x.cap = a.cap;
    NodeState& st = s_st[wave];
    nhdfit_detail& dd = s_dd[wave];
    nhdfit_placement& pl = s_pl[wave];
    uint16_t* out = a.counts + (size_t)tpl * a.chunks * 64u;

    for (uint32_t turn = 0; turn < a.chunks; ++turn) {                   // (a block takes at most every chunk)
        if (tid == 0) s_tick[0] = __hip_atomic_fetch_add(&a.tickets[tpl], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (tid < 64u) s_cnt[tid] = 0u;
        __syncthreads();
        const uint32_t c = s_tick[0];
        if (c >= a.chunks) break;                                        // (block-uniform)
        // ---- phase A: lane = node
        const uint32_t i = c * 64u + lane;
        bool ok = false, off = false;
        if (i < a.n && (!a.cand || (a.cand[c] >> lane & 1ull))) {
            if (a.n_wide && wide_slot_of(a.wide, a.n_wide, i) >= 0) off = true;          // answered by its wide record: not in this launch
            else {
                const NodeIdx ni = node_index(a.p0[i], a.p1[i], a.p2[i], a.p4[i], a.fc_dim, a.fg_dim, a.ngs);
                ok = lone_pod_fits(x.t, x.h, ni, a.p3[i], false, a.d.group_sets);
            }
        }
        const uint64_t word = __ballot(ok), off_word = __ballot(off);
        // ---- phase B: wavefront = node
        uint32_t rank = 0;
        for (uint64_t w = word; w; w &= w - 1ull, ++rank) {              // (at most 64 turns)
            if ((rank & (kHeadroomWaves - 1u)) != wave) continue;
            const uint32_t b = (uint32_t)__builtin_ctzll(w), v = c * 64u + b;
            uint32_t* sw = reinterpret_cast<uint32_t*>(&st);
            if (lane < 5u) {                                             // the node's planes: a 16-byte load per lane
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
            const uint32_t e = headroom_run_wave<G4>(st, dd, pl, r, x, lane);
            if (lane == 0u) s_cnt[b] = e;
            if (a.final && (e & NHDFIT_HEADROOM_COUNT_MASK)) {           // (block-uniform pointer, wavefront-uniform entry) the copy as the last commit
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // left it, by the lanes that loaded it: thirteen 16-byte stores
                __builtin_amdgcn_wave_barrier();
                uint4* f = reinterpret_cast<uint4*>(a.final + ((size_t)tpl * a.chunks * 64u + v));
                if (lane < 5u) f[lane] = uint4{sw[lane * 4 + 0], sw[lane * 4 + 1], sw[lane * 4 + 2], sw[lane * 4 + 3]};
                if (lane >= 8u && lane < 8u + sizeof(nhdfit_detail) / 16) {
                    const uint32_t* dw = reinterpret_cast<const uint32_t*>(&dd) + (lane - 8u) * 4u;
                    f[5u + lane - 8u] = uint4{dw[0], dw[1], dw[2], dw[3]};
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();                             // (the slice is the next node's)
        }
        __syncthreads();
        if (wave == 0u) {
            const uint32_t e = s_cnt[lane] | ((off_word >> lane & 1ull) ? NHDFIT_HEADROOM_NOT_EVALUATED : 0u);
            out[c * 64u + lane] = (uint16_t)e;                           // one 128-byte row
            HeadroomTally{s_tot}.chunk(e, a.cap, off_word, lane);
        }
        __syncthreads();                                                 // (everybody has read the ticket; the entries are wavefront 0's to clear)
    }
    __syncthreads();
    HeadroomTally{s_tot}.flush<false>(a.sum + tpl, tid);
}
