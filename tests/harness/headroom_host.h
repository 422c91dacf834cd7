// headroom_host.h - TEST INFRASTRUCTURE.  What the two host builds of nhdfit_headroom (headroom_twin.cpp: the shared headers' scalar
// forms; headroom_wave_emul.cpp: the kernel's own per-node loop on emulated lanes) have in common: the dictionary as
// nhdfit_set_dictionary derives it (16-bit signature stream, signature key table), one template's masks as NHDFIT_LONE_POD_MASKS
// (nhd_amd/csrc/step_kernel.h) derives them, and the bookkeeping of entries and sums.  NOT part of libnhdfit.so.
#pragma once
#include <algorithm>
#include <cstring>
#include <vector>
#include "../../nhd_amd/csrc/seq_core.h"

namespace hrh {
using namespace nhdfit;

struct Sum { uint64_t replicas; uint32_t nodes_with_room, max_on_one_node, saturated, stopped, not_evaluated, form; };
static_assert(sizeof(Sum) == sizeof(nhdfit_headroom_sum), "the summary record of include/nhdfit.h");

struct Dictionary {
    uint32_t fc_dim, fg_dim, ngs, ncls, nsig;
    const uint64_t* gs; const double* caps;
    std::vector<uint16_t> flat;
    std::vector<uint64_t> skeys; std::vector<uint32_t> sids;
    bool ok = true;
    SigTable sigs() const { return SigTable{skeys.data(), sids.data(), (uint32_t)skeys.size() - 1}; }
};
inline Dictionary make_dictionary(uint32_t fcmax, uint32_t fgmax, const uint64_t* gs, uint32_t ngs, const double* caps, uint32_t ncls,
                                  const uint32_t* sig_off, uint32_t nsig, const uint32_t* pool_off, const uint8_t* pool_glimit, const nhdfit_cc* cc) {
    Dictionary d;
    d.fc_dim = fcmax + 1; d.fg_dim = fgmax + 1; d.ngs = ngs; d.ncls = ncls; d.nsig = nsig; d.gs = gs; d.caps = caps;
    d.flat.assign(nsig + 1, 0);
    for (uint32_t sg = 0; sg < nsig; ++sg) {
        const size_t at = d.flat.size() - (nsig + 1);
        if (at > 0xFFFFu) { d.ok = false; return d; }
        d.flat[sg] = (uint16_t)at;
        d.flat.push_back((uint16_t)(sig_off[sg + 1] - sig_off[sg]));
        for (uint32_t pl = sig_off[sg]; pl < sig_off[sg + 1]; ++pl) {
            const uint32_t ncc_pl = pool_off[pl + 1] - pool_off[pl];
            if (ncc_pl > 255u) { d.ok = false; return d; }
            d.flat.push_back((uint16_t)(pool_glimit[pl] << 8 | ncc_pl));
            for (uint32_t k = pool_off[pl]; k < pool_off[pl + 1]; ++k) d.flat.push_back((uint16_t)((cc[k].cls & 0xFFu) << 8 | cc[k].cnt));
        }
    }
    uint32_t slots = 64;
    while (slots < 4 * nsig) slots <<= 1;
    d.skeys.assign(slots, 0);
    d.sids.assign(slots, 0);
    for (uint32_t sg = 1; sg < nsig; ++sg) {
        uint64_t key = 0;
        for (uint32_t pl = sig_off[sg]; pl < sig_off[sg + 1]; ++pl) {
            uint8_t cnt[NHDFIT_MAX_CLASSES] = {0};
            for (uint32_t k = pool_off[pl]; k < pool_off[pl + 1]; ++k) cnt[cc[k].cls & 15u] = cc[k].cnt;
            key = sig_key_add(key, pool_key(pool_glimit[pl], cnt));
        }
        if (!key) continue;
        uint32_t sl = (uint32_t)mix64(key) & (slots - 1);
        while (d.skeys[sl] != 0 && d.skeys[sl] != key) sl = (sl + 1) & (slots - 1);
        d.skeys[sl] = key; d.sids[sl] = sg;
    }
    return d;
}

struct Masks {
    std::vector<uint16_t> a0, a1, w0, w1, r0, r1;
    PodHeader h;
    LoneMasks view() const { return LoneMasks{a0.data(), a1.data(), w0.data(), w1.data(), r0.data(), r1.data()}; }
};
inline Masks make_masks(const nhdfit_req& r, const Dictionary& d) {
    Masks m;
    m.h = pod_header(r);
    m.a0.assign(d.fg_dim, 0); m.a1.assign(d.fg_dim, 0);
    m.w0.assign(2 * d.fc_dim * 2, 0); m.w1.assign(2 * d.fc_dim * 2, 0);
    m.r0.assign(d.nsig, 0); m.r1.assign(d.nsig, 0);
    if (!(m.h.flags & kPodValid)) return m;
    PodSums s;
    pod_sums(r, s);
    std::vector<uint16_t> cover(d.ncls * (kMaxG + 1));
    for (uint32_t c = 0; c < d.ncls; ++c) class_cover(r, d.caps[c], s.W, s.G, &cover[c * (kMaxG + 1)]);
    for (uint32_t f = 0; f < d.fg_dim; ++f) { m.a0[f] = (uint16_t)entry_a(s, 0, f); m.a1[f] = (uint16_t)entry_a(s, 1, f); }
    for (uint32_t smt = 0; smt < 2; ++smt)
        for (uint32_t c = 0; c < d.fc_dim; ++c)
            for (uint32_t k = 0; k < 2; ++k) {
                m.w0[(smt * d.fc_dim + c) * 2 + k] = (uint16_t)entry_w(s, 0, smt, c, k);
                m.w1[(smt * d.fc_dim + c) * 2 + k] = (uint16_t)entry_w(s, 1, smt, c, k);
            }
    for (uint32_t sig = 0; sig < d.nsig; ++sig) {
        const uint32_t reach = sig_reach_flat(d.flat.data(), d.nsig, sig, cover.data(), s.W);
        m.r0[sig] = (uint16_t)entry_r(reach, s.W, 0);
        m.r1[sig] = (uint16_t)entry_r(reach, s.W, 1);
    }
    return m;
}

inline bool is_wide(const nhdfit_wide_node* wide, uint32_t n_wide, uint32_t v) {
    for (uint32_t w = 0; w < n_wide; ++w)
        if (wide[w].index == v) return true;
    return false;
}
// one node's entry into the template's sum (what wavefront 0 of k_headroom adds per chunk)
inline void account(Sum& s, uint32_t e, uint32_t cap) {
    const uint32_t k = e & NHDFIT_HEADROOM_COUNT_MASK;
    s.replicas += k;
    if (k) s.nodes_with_room++;
    s.max_on_one_node = std::max(s.max_on_one_node, k);
    if (k && k >= cap) s.saturated++;
    if (e & NHDFIT_HEADROOM_STOPPED) s.stopped++;
    if (e & NHDFIT_HEADROOM_NOT_EVALUATED) s.not_evaluated++;
}
// One node of the planes run to exhaustion over the shared headers' SCALAR forms - node_index / lone_pod_fits (fit_core.h),
// lone_nic_bits, map_on_state (seq_core.h), commit_node (commit_core.h) - on the private copy `st` / `dd`, which is left as the run
// ended (the mirror's state until a commit succeeds).  IsBusy() false: the busy window is not a resource.  Returns the node's entry:
// replicas | NHDFIT_HEADROOM_STOPPED.
inline uint32_t plane_run(NodeState& st, nhdfit_detail& dd, const nhdfit_req& r, const Masks& m, const Dictionary& d, uint32_t cap) {
    const LoneMasks t = m.view();
    const SigTable sigs = d.sigs();
    const MapTables mt{nullptr, nullptr, SetStates{nullptr, nullptr, nullptr, 0}};
    const bool pci = r.map_type == NHDFIT_MAP_PCI;
    uint32_t k = 0;
    for (;;) {
        const NodeIdx ni = node_index(st.p0, st.p1, st.p2, st.p4, d.fc_dim, d.fg_dim, d.ngs);
        if (!lone_pod_fits(t, m.h, ni, st.p3, false, d.gs)) break;
        if (k >= cap) break;
        nhdfit_mapping mp;
        std::memset(&mp, 0, sizeof mp);
        if (!map_on_state(r, st, dd, d.caps, lone_nic_bits(t, pci, st.p3), mt, mp)) break;
        bool nic_missing = false;
        for (uint32_t g = 0; g < r.n_groups; ++g) nic_missing |= (uint32_t)mp.nic_idx[g] >= dd.nic_cnt[mp.nic_numa[g] & 1];
        nhdfit_placement pl;
        if (nic_missing || commit_node(st, dd, r, mp, 0.0, sigs, pl) != kCommitOk) return k | NHDFIT_HEADROOM_STOPPED;
        ++k;
    }
    return k;
}
inline uint32_t form_of(const nhdfit_req& r) { return req_valid(r) && r.n_groups > 3 ? NHDFIT_HEADROOM_FORM_GENERIC : NHDFIT_HEADROOM_FORM_WAVE; }
}  // namespace hrh
