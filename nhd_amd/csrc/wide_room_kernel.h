// wide_room_kernel.h - nhdfit_headroom_general on the device: how many more replicas of a pod template every WIDE record can take
// (k_wide_room).  Device code of libnhdfit.so; included by nhdfit.hip inside its anonymous namespace, behind wide_kernel.h and
// headroom_kernel.h (HeadroomSum, HeadroomTally).  gfx950 only.
//
// k_headroom (headroom_kernel.h) answers for the planes and flags a candidate the mirror holds as a wide record - 3 or 4 sockets, 65..128
// cores per socket, every node of an ENABLE_SHARING mirror - NOT_EVALUATED.  This kernel runs behind it on the same stream and answers
// for those: per (template, wide record) the number of times wide_fits -> wide_map -> wide_commit (wide_core.h: FindNode ->
// SetPhysicalIdsFromMapping -> ClaimPodNICResources, nhd/NHDScheduler.py:277-304) succeeds back to back on a private copy of the
// record - and, under ENABLE_SHARING, of its nhdfit_wide_share record: the commit adds each group's rx / tx to it (nhd/Node.py:754), so
// a later replica is priced against what the earlier ones use - with IsBusy() false.
//
//   grid = (blocks, templates), a block is ONE wavefront: the private copy, the stage rows, the tuple hashes and the set tables of one
//   run take 41 KB of LDS, three blocks to a CU.  A block takes 64-slot chunks of the wide records off the template's ticket counter (a
//   relaxed agent-scope fetch-add: it hands out work, it publishes nothing) until the tickets run out.  Per chunk:
//   Phase A, lane = wide slot: the candidate bit of the record's node and wide_fits with "not busy", one ballot.  Most records end here.
//   Phase B, wavefront = node, the chunk's set bits one after the other: the 640-byte record (and the 1 024-byte share record) go into
//     LDS with 16-byte loads; wide_room_run_wave runs the node to exhaustion.
//   Results: the entries overwrite k_headroom's flags (uint16, scattered by record.index), the partial sums are kept in LDS; at the end
//   one atomic per (block, template, field) into the summary record - the nodes evaluated here are taken back out of not_evaluated.
// Every loop has a bound known before it starts: the chunk count (tickets), 64 (set bits), max_per_node (replicas), U^(G+1) <= 1 024
// (tuples).  No spin wait, no hand-off between blocks.  Nothing is written back to the mirror.

// ---- one wide record's run with the wavefront's lanes --------------------------------------------------------------------------------
// As wide_map_wave (big_kernel.h) does it for a big request: per replica, lane = tuple answers the GPU / NIC / CPU stage questions into
// bit rows (U^G <= 256 G-tuples, U^(G+1) <= 1 024 (G+1)-tuples for U <= 4, G <= 4; every tuple's hash is computed once per run - it
// depends on U and G alone); "does it still fit" (wide_fits: some G-tuple passes all three stages) is read off the rows with one
// ballot per 64 tuples; lane 0 runs the serial part - wide_map_model over the rows, its set tables in LDS, then wide_commit on the LDS
// copy - and the wavefront goes round again.  Same stages, same model, same commit: the count is the scalar loop's
// (tests/harness/headroom_general_twin.cpp), bit for bit (tests/harness/wide_room_wave_emul.cpp runs this text on emulated lanes).
constexpr uint32_t kRoomTuplesG = 256, kRoomTuplesC = 1024;
struct WideRoomLds {
    nhdfit_wide_node node;                                        // the private copy (modified)
    nhdfit_wide_share share;                                      // ... of the NICs' speed_used (ENABLE_SHARING)
    nhdfit_wide_placement pl;                                     // what the commit step writes
    uint64_t hash_g[kRoomTuplesG], hash_c[kRoomTuplesC];          // tuplehash of every G- / (G+1)-tuple
    uint64_t bit_g[kRoomTuplesG / 64], bit_n[kRoomTuplesG / 64], bit_c[kRoomTuplesC / 64];   // the stages' answers, bit = tuple
    nhdfit_mapping mp;
    int32_t rc, status;
    int16_t tables[kWideScratchWords];                            // the set model's tables (wide_core.h), 28 KB
};
static_assert(offsetof(WideRoomLds, node) == 0 && offsetof(WideRoomLds, share) % 16 == 0, "the copies keep the sixteen-byte alignment of the loads");
static_assert(sizeof(WideRoomLds) <= 42 * 1024, "three blocks to a CU's 160 KB");
struct WideRoomStages {
    const WideRoomLds& t;
    NHD_HD bool gpu(uint32_t code) const { return t.bit_g[code >> 6] >> (code & 63) & 1ull; }
    NHD_HD bool nic(uint32_t code) const { return t.bit_n[code >> 6] >> (code & 63) & 1ull; }
    NHD_HD bool cpu(uint32_t code) const { return t.bit_c[code >> 6] >> (code & 63) & 1ull; }
    NHD_HD bool exhausted() const { return false; }               // (an ordinary request's NIC search has no budget)
    NHD_HD const uint64_t* hash_g() const { return t.hash_g; }
    NHD_HD const uint64_t* hash_c() const { return t.hash_c; }
};
// `t.node` (and, `sharing`, `t.share`) are in place and visible to every lane; the caller knows that the template fits the record
// (wide_fits).  Every lane returns the same entry: replicas | NHDFIT_HEADROOM_STOPPED.  `err`: 0, or wide_map's negative code (a set of the
// model outgrew its table: never expected, reported by the caller as the find path reports it) - the run ends there.
__device__ __noinline__ uint32_t wide_room_run_wave(WideRoomLds& t, bool sharing, const nhdfit_req& r, const double* caps, uint32_t cap, uint32_t lane,
                                                    int& err) {
    nhdfit_wide_node& n = t.node;
    nhdfit_wide_share* sh = sharing ? &t.share : nullptr;
    const WideCaps wc(caps, sh);
    const uint32_t G = r.n_groups, U = n.numa_nodes, nG = wide_ipow(U, G), nC = nG * U;
    err = 0;
    if (nC > kRoomTuplesC) { err = -1; return 0u; }                // (wide_map's own guard; wide_fits admits no such pair)
    for (uint32_t code = lane; code < nG; code += 64u) t.hash_g[code] = wide_tuple_hash(code, G, U);
    for (uint32_t code = lane; code < nC; code += 64u) t.hash_c[code] = wide_tuple_hash(code, G + 1, U);
    uint32_t k = 0;
    while (k < cap) {
        // wide_fits on the copy as the last commit left it: the scalar predicates (hugepages go down with every replica) ...
        if (!wide_scalar_ok(n, r, false)) break;
        const WideFree f = wide_free(n);
        for (uint32_t base = 0; base < nG; base += 64u) {         // ... and the stages, lane = tuple
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
        const WideRoomStages st{t};
        bool any = false;                                         // some assignment passes all three stages (Matcher.py:346 is non-empty)
        for (uint32_t base = 0; base < nG; base += 64u) {
            const uint32_t code = base + lane;
            bool ok = code < nG && st.gpu(code) && st.nic(code);
            if (ok) {
                bool cpu = false;
                for (uint32_t m = 0; m < U; ++m) cpu = cpu || st.cpu(code * U + m);
                ok = cpu;
            }
            any = (__ballot(ok) != 0ull) || any;
        }
        if (!any) break;                                          // FindNode returns (None,): the run ends, nothing to flag
        if (lane == 0u) {                                         // the serial part: CPython's sets, then the commit step
            WideRoomStages rows{t};
            wide_map_clear(t.mp, kMaxG);
            const int rc = wide_map_model(n, r, wc, f, t.tables, t.mp, kWideSetSlotsG, kWideSetSlotsC, rows);
            t.rc = rc;
            t.status = rc == 1 ? wide_commit(n, r, t.mp, 0.0, t.pl, sh) : kCommitOk;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        const int rc = t.rc, status = t.status;
        __builtin_amdgcn_wave_barrier();                          // (everybody has read the verdict; the next turn's is lane 0's to write)
        if (rc < 0) { err = rc; break; }
        if (rc == 0) break;
        if (status != kCommitOk) return k | NHDFIT_HEADROOM_STOPPED;   // the reference raises (nhd/Node.py:686): not counted
        ++k;
    }
    return k;
}

// ---- the launch -------------------------------------------------------------------------------------------------------------------
struct WideRoomArgs {
    const nhdfit_wide_node* wide; uint32_t n_wide;
    const nhdfit_wide_share* share;                  // optional [n_wide]: ENABLE_SHARING arithmetic
    const nhdfit_req* reqs;                          // [gridDim.y] templates
    const double* caps; uint32_t ncls;
    const uint64_t* cand;                            // optional [chunks of the planes' nodes]
    uint32_t n, wchunks, cap;                        // nodes of the mirror; 64-slot chunks of the wide records
    size_t pitch;                                    // entries per template row of `counts`
    uint32_t* tickets;                               // [templates], zeroed by the caller
    uint16_t* counts;                                // [templates][pitch]: k_headroom's rows
    HeadroomSum* sum;                                // [templates]: k_headroom's records
    uint32_t* flags;                                 // [0] a set of the model outgrew its table (never expected)
};
constexpr uint32_t kWideRoomBlock = 64;

__global__ __launch_bounds__(kWideRoomBlock) void k_wide_room(WideRoomArgs a) {
    __shared__ __align__(16) WideRoomLds s_t;
    __shared__ double s_caps[NHDFIT_MAX_CLASSES];
    __shared__ uint32_t s_cnt[64];
    __shared__ unsigned long long s_tot[8];                              // the block's partial sums (HeadroomTally)
    const uint32_t tpl = blockIdx.y, lane = threadIdx.x;
    const nhdfit_req r = a.reqs[tpl];
    if (lane < (uint32_t)NHDFIT_MAX_CLASSES) s_caps[lane] = lane < a.ncls ? a.caps[lane] : 0.0;
    if (lane < 8u) s_tot[lane] = 0ull;
    const bool sharing = a.share != nullptr;
    uint16_t* out = a.counts + (size_t)tpl * a.pitch;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();

    for (uint32_t turn = 0; turn < a.wchunks; ++turn) {                  // (a block takes at most every chunk)
        uint32_t c = 0;
        if (lane == 0u) c = __hip_atomic_fetch_add(&a.tickets[tpl], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        c = (uint32_t)__builtin_amdgcn_readfirstlane((int)c);
        if (c >= a.wchunks) break;                                       // (wavefront-uniform)
        // ---- phase A: lane = wide slot
        const uint32_t w = c * 64u + lane;
        bool listed = false, ok = false;
        uint32_t index = 0;
        if (w < a.n_wide) {
            const nhdfit_wide_node& n = a.wide[w];
            index = n.index;
            listed = index < a.n && (!a.cand || (a.cand[index >> 6] >> (index & 63u) & 1ull));
            if (listed) ok = wide_fits(n, r, false, WideCaps(s_caps, sharing ? a.share + w : nullptr));
        }
        const uint64_t word = __ballot(ok), listed_word = __ballot(listed);
        s_cnt[lane] = 0u;
        // ---- phase B: wavefront = node
        for (uint64_t m = word; m; m &= m - 1ull) {                      // (at most 64 turns)
            const uint32_t b = (uint32_t)__builtin_ctzll(m), v = c * 64u + b;
            if (lane < sizeof(nhdfit_wide_node) / 16) {                  // forty 16-byte loads
                const uint4 q = reinterpret_cast<const uint4*>(a.wide + v)[lane];
                uint32_t* d = reinterpret_cast<uint32_t*>(&s_t.node) + lane * 4u;
                d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
            }
            if (sharing) {                                               // sixty-four
                static_assert(sizeof(nhdfit_wide_share) == 64 * 16, "a 16-byte load per lane");
                const uint4 q = reinterpret_cast<const uint4*>(a.share + v)[lane];
                uint32_t* d = reinterpret_cast<uint32_t*>(&s_t.share) + lane * 4u;
                d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            int err = 0;
            const uint32_t e = wide_room_run_wave(s_t, sharing, r, s_caps, a.cap, lane, err);
            if (lane == 0u) {
                s_cnt[b] = e;
                if (err < 0) atomicOr(&a.flags[0], 1u);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();                             // (the copy is the next node's)
        }
        const uint32_t e = s_cnt[lane];
        if (listed_word >> lane & 1ull) out[index] = (uint16_t)e;        // over k_headroom's NOT_EVALUATED
        HeadroomTally{s_tot}.chunk(e, a.cap, listed_word, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();                                 // (the entries are read; the next chunk clears them)
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    HeadroomTally{s_tot}.flush<true>(a.sum + tpl, lane);                 // (slot 5: the nodes evaluated here leave not_evaluated)
}
