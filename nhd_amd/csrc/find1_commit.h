// find1_commit.h - FindNode for ONE pod and the commit step on its winner in ONE launch (nhdfit_find_commit; k_find1_commit).
// Device code of libnhdfit.so, included by nhdfit.hip behind seq2_kernel.h (the wavefront form of the commit step, commit_node_wave,
// is defined there - which is why this launch is not in step_kernel.h beside k_find1).
//
// The scheduler places pods one at a time: FindNode, then SetBusy / SetPhysicalIdsFromMapping / ClaimPodNICResources on the winner
// (nhd/NHDScheduler.py:277-304), then the next pod.  As two calls that is two launches, two polled words and two trips through the
// binding per pod (k_find1 + k_commit).  Here the block of k_find1 that holds the last ticket - it has the winner, the winner's
// planes 0-3 and detail record in LDS, and the mapping - goes on with the commit:
//   * digest, sweep, ticket and mapping are k_find1's own code (find1_launch, step_kernel.h), instantiated with this file's tail;
//   * wavefront 0 then loads plane 4 beside the state the mapping staged, makes k_commit's check that every NIC ordinal of the
//     mapping exists on the node, and runs commit_node_wave on the LDS copy with the caller's busy time;
//   * status OK / NEW_SIG: the same lanes write planes and detail back (sixteen-byte stores, a lane per plane) and the placement record
//     goes to the host block as 64 four-byte stores; host word `committed` = 1;
//   * a NIC that is missing, or status WOULD_RAISE: nothing is written back - the wavefront form worked on the LDS copy - and the
//     launch reports "found, not committed": the host finishes with k_commit, whose scalar form leaves the documented partial state.
//     (The scalar commit_node is NOT inlined here: its local structs would give every launch of the hot form a private segment.)
// Ordering inside the launch: every other block took its ticket behind its last read of the planes, and this block runs behind the
// last ticket, so nobody reads what the commit writes; the next launch on the stream sees the new state at the kernel boundary,
// exactly as it does behind k_commit.  Publishing is k_find1's: score, mapping, placement and `committed` are stored, every wave
// drains its vector stores, block barrier, then one lane stores the sequence number with system-scope release.  No new spin wait.
//
// The busy-time correction.  The reference stamps busy_time inside SetBusy, AFTER the match, so the time a fused call commits and
// the time the scheduler's SetBusy writes a few microseconds later differ; sent as a SET_BUSY delta that would be a blocking call per
// pod.  The call therefore takes `prev_node` / `prev_busy_time`: "as if a SET_BUSY delta for that node had been applied first".
// Shipped in the in-kernel form: a sweeping lane whose node is prev_node reads prev_busy_time in place of p4[i].busy_time (one
// compare and one select per node, the values are kernel arguments in scalar registers), and the committing wavefront stores
// prev_busy_time to p4[prev_node] before it loads the winner's plane 4 (same lane: the winner may be that very node).  The composed
// form of the call (nhdfit.hip) applies the same correction with a stream-ordered launch of k_set_busy in front of its find.
struct Find1CommitArgs {
    Find1Args f;                                     // (f.m's planes are the same arrays as below, read-only there)
    nhdfit_plane0* p0; nhdfit_plane1* p1; nhdfit_plane2* p2; nhdfit_plane3* p3; nhdfit_plane4* p4; nhdfit_detail* det;
    SigTable sigs;
    uint32_t ncls;                                   // capacity classes of the dictionary (the wavefront form's signature keys)
    uint32_t prev_node;                              // local index, kNoPrevNode: no correction
    double busy_time, prev_busy_time;
};
constexpr uint32_t kNoPrevNode = 0xFFFFFFFFu;
constexpr int kClockCommitTail = 5;                  // slot of the tail in the tuning build's role clock (NHDFIT_ROLE_TIMES), behind the five roles

struct Find1CommitTail {
    static constexpr bool kCommits = true;
    const Find1CommitArgs& c;
    __device__ __forceinline__ double busy_time(uint32_t i, double stored) const { return i == c.prev_node ? c.prev_busy_time : stored; }
    // (behind the mapping's staging area; run() below carves the same way)
    __device__ __forceinline__ nhdfit_mapping* kept_mapping(uint8_t* lds) const { (void)lone_map_lds(lds); return carve<nhdfit_mapping>(lds, 1); }
    // every thread of the block with the last ticket calls it behind map_lone_pod_wave's barrier
    __device__ __forceinline__ void run(const Find1Args& a, const nhdfit_req& r, uint8_t* lds) const {
        const uint32_t tid = threadIdx.x, lane = tid & 63u;
        if (tid >= 64u) return;                                          // wavefront 0; the others wait at the launch's publishing barrier
        const unsigned long long t0 = a.role_clock ? (unsigned long long)wall_clock64() : 0ull;
        const LoneMapLds l = lone_map_lds(lds);
        const nhdfit_mapping* s_map = carve<nhdfit_mapping>(lds, 1);
        nhdfit_placement* s_pl = carve<nhdfit_placement>(lds, 1);
        uint32_t* sw = reinterpret_cast<uint32_t*>(l.st);
        // the correction reaches the mirror whatever becomes of the pod (lane 4: the lane that loads and stores plane 4 below)
        if (lane == 4u && c.prev_node != kNoPrevNode) c.p4[c.prev_node].busy_time = c.prev_busy_time;
        uint32_t committed = 0u;
        const unsigned long long s = __hip_atomic_load(a.m.score, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint64_t gi = s ? NHDFIT_SCORE_INDEX(s) : ~0ull;
        if (s && s_map->valid && gi >= a.m.global_base && gi < a.m.global_base + a.m.n) {     // (wave-uniform) a winner of this mirror, mapped
            const uint32_t i = (uint32_t)(gi - a.m.global_base);
            if (lane == 4u) {                                            // planes 0-3 and the detail record are where the mapping staged them
                const uint4 q = *reinterpret_cast<const uint4*>(c.p4 + i);
                sw[16] = q.x; sw[17] = q.y; sw[18] = q.z; sw[19] = q.w;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            // k_commit's guard: GetNicObjFromIndex returns None -> IndexError before anything is touched (nhd/Node.py:700-704).  A mapping
            // that comes out of the find names NICs of the node it was made on, so this branch is not reachable through the ABI.
            bool nic_missing = false;
            for (uint32_t g = 0; g < r.n_groups; ++g) nic_missing |= (uint32_t)s_map->nic_idx[g] >= l.dd->nic_cnt[s_map->nic_numa[g] & 1];
            if (!nic_missing) {
                const int status = commit_node_wave(*l.st, *l.dd, r, *s_map, c.busy_time, c.sigs, c.ncls, *s_pl, lane);
                if (status != kCommitWouldRaise) {                       // (every lane holds the same status)
                    if (lane < 5u) {
                        const uint4 q = make_uint4(sw[lane * 4], sw[lane * 4 + 1], sw[lane * 4 + 2], sw[lane * 4 + 3]);
                        if (lane == 0u) *reinterpret_cast<uint4*>(c.p0 + i) = q;
                        else if (lane == 1u) *reinterpret_cast<uint4*>(c.p1 + i) = q;
                        else if (lane == 2u) *reinterpret_cast<uint4*>(c.p2 + i) = q;
                        else if (lane == 3u) *reinterpret_cast<uint4*>(c.p3 + i) = q;
                        else *reinterpret_cast<uint4*>(c.p4 + i) = q;
                    }
                    if (lane >= 8u && lane < 8u + sizeof(nhdfit_detail) / 16) {
                        const uint32_t* dw = reinterpret_cast<const uint32_t*>(l.dd) + (lane - 8u) * 4u;
                        reinterpret_cast<uint4*>(c.det + i)[lane - 8u] = make_uint4(dw[0], dw[1], dw[2], dw[3]);
                    }
                    if (lane < sizeof(nhdfit_placement) / 4) reinterpret_cast<uint32_t*>(&a.host->place)[lane] = reinterpret_cast<const uint32_t*>(s_pl)[lane];
                    committed = 1u;
                }
            }
        }
        if (lane == 0u) a.host->committed = committed;
        stamp(a.role_clock, kClockCommitTail, t0);
    }
};
static_assert(sizeof(NodeState) == 80 && sizeof(nhdfit_detail) == 128 && sizeof(nhdfit_placement) == 256, "the tail's lanes are dealt out by these sizes");
static_assert(lds_slice(sizeof(NodeState)) + lds_slice(sizeof(nhdfit_detail)) + lds_slice(NHDFIT_MAX_CLASSES * sizeof(double)) +
              lds_slice(sizeof(nhdfit_mapping)) + lds_slice(sizeof(nhdfit_placement)) <= map_tile_lds_bytes<256>(),
              "the tail's slices fit the staging area the launch is given behind kLoneLds");

template <int BLOCK>
__global__ __launch_bounds__(BLOCK) void k_find1_commit(Find1CommitArgs a) { find1_launch<BLOCK>(a.f, Find1CommitTail{a}); }

// SET_BUSY for one node, stream-ordered (the composed form of nhdfit_find_commit: its correction in front of the find)
__global__ __launch_bounds__(64) void k_set_busy(nhdfit_plane4* p4, uint32_t node, double busy_time) {
    if (threadIdx.x == 0) p4[node].busy_time = busy_time;
}
