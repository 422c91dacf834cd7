// explain_core.h - why a node turned a pod away: the first stage of the reference's filter that drops the node
// (include/nhdfit.h NHDFIT_STAGE_*).  Written once for the gfx950 kernel (explain_kernel.h) and the host twin of the tests.
//
// The stages are the reference's, in its order, each asked the way the fit path asks it (wide_core.h), so every quirk of
// the fit path (DESIGN Q1-Q7) is inherited rather than restated:
//
//   NOT_CANDIDATE  not in `cand`, or InitialNodeFilter drops it                        nhd/NHDScheduler.py:235-247
//   MAINTENANCE    Node.maintenance                                                    nhd/Matcher.py:72
//   HUGEPAGES      top.hugepages_gb > free 1 GB hugepages                              nhd/Matcher.py:77
//   BUSY           a GPU pod and a node deployed to within the last few seconds       nhd/Matcher.py:104
//   GPU            no assignment of the groups to NUMA nodes has the GPUs              nhd/Matcher.py:112-134
//   CPU            no (G+1)-tuple (groups + misc cores) has the cores                  nhd/Matcher.py:169-216
//   NIC            no assignment has a NIC choice that passes the bandwidth test       nhd/Matcher.py:228-272
//   PCI            PCI mode: every such NIC choice is removed by the switch pruning    nhd/Matcher.py:294-335
//   NUMA           no assignment passes the GPU, CPU and NIC stages at once            nhd/Matcher.py:337-358
//   FITS           the node survives: the verdict bit of nhdfit_find / nhdfit_big_find
//
// A request the device cannot evaluate at all (a map type other than NUMA / PCI, no processing groups - the reference
// returns before it filters anything, Matcher.py:45-47) and a record of no shape the general path holds are charged
// NOT_CANDIDATE.  FITS is wide_fits exactly: the NUMA stage asks the same per-assignment question in the same order.
//
// The arithmetic is wide_core.h's (wide_free, wide_gpu_ok, wide_cpu_ok, wide_nic_choice) restated for one purpose: every value the
// kernel keeps per pair lives in registers.  Per-NUMA-node totals are four scalars selected by index (Quad), and the NIC search's
// per-group state - the group's NUMA node (2 bits), its NIC (4 bits) and the search order (3 bits) - is packed into integers, so
// nothing is indexed dynamically in private memory (k_explain has no private segment; tests/test_explain_gpu.py asserts it).
// The search is wide_nic_choice step for step: the same enumeration order, the same f64 subtractions in the same order, the
// same prefix pruning and (big requests) the same skipping of interchangeable NICs and the same step accounting against a budget.
#pragma once
#include "commit_core.h"                 // (wide_core.h's commit step names its status codes)
#include "wide_core.h"

namespace nhdfit {

// four per-NUMA-node counters as scalars (u < 4 = NHDFIT_WIDE_MAX_NUMA)
struct Quad {
    uint32_t v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    NHD_HD uint32_t get(uint32_t u) const { return u == 0 ? v0 : u == 1 ? v1 : u == 2 ? v2 : v3; }
    NHD_HD void add(uint32_t u, uint32_t x) { v0 += u == 0 ? x : 0u; v1 += u == 1 ? x : 0u; v2 += u == 2 ? x : 0u; v3 += u == 3 ? x : 0u; }
};
struct ExFree { uint32_t U; bool smt; Quad c, g; };

// GetFreeCpuCores / GetFreeNumaGPUs (wide_free)
NHD_HD ExFree explain_free(const nhdfit_wide_node& n) {
    ExFree f;
    f.U = n.numa_nodes;
    f.smt = (n.flags & NHDFIT_NF_SMT) != 0;
    const uint32_t cpp = n.cores_per_proc;
    for (uint32_t u = 0; u < f.U; ++u) {
        const uint32_t lo = u * cpp, hi = lo + cpp;
        uint32_t k = 0;
        for (uint32_t w = lo >> 6; w < (uint32_t)NHDFIT_WIDE_CORE_WORDS && w * 64u < hi; ++w) {
            uint64_t m = n.t0[w] & n.t1[w];
            const uint32_t s = w * 64u;
            if (lo > s) m &= ~0ull << (lo - s);
            if (hi < s + 64u) m &= ~0ull >> (s + 64u - hi);
            k += (uint32_t)popc64(m);
        }
        f.c.add(u, k);
    }
    for (uint32_t x = 0; x < n.n_gpus; ++x)
        if ((n.gpu_free >> x & 1u) && n.gpu_numa[x] < f.U) f.g.add(n.gpu_numa[x], 1u);
    return f;
}
// GPU stage, one assignment (wide_gpu_ok, Matcher.py:120-131)
template <class R> NHD_HD bool explain_gpu_ok(const R& r, const ExFree& f, uint32_t code) {
    Quad t;
    for (int g = (int)r.n_groups - 1; g >= 0; --g) { t.add(code % f.U, r.gpus[g]); code /= f.U; }
    for (uint32_t u = 0; u < f.U; ++u)
        if (t.get(u) > f.g.get(u)) return false;
    return true;
}
// CPU stage, one (G+1)-tuple: the last element places the misc cores (wide_cpu_ok, Matcher.py:206-216)
template <class R> NHD_HD bool explain_cpu_ok(const R& r, const ExFree& f, uint32_t code) {
    Quad t;
    for (int g = (int)r.n_groups; g >= 0; --g) {
        const uint32_t d = g < (int)r.n_groups ? (f.smt ? r.cpu_smt[g] : r.cpu_nosmt[g]) : (f.smt ? r.misc_smt : r.misc_nosmt);
        t.add(code % f.U, d);
        code /= f.U;
    }
    for (uint32_t u = 0; u < f.U; ++u)
        if (t.get(u) > f.c.get(u)) return false;
    return true;
}

// does assignment `gcode` have a NIC choice (wide_nic_choice's search; `switch_test`: PCI pods' switch test as well)?
template <class R>
NHD_HD bool explain_nic_ok(const nhdfit_wide_node& n, const R& r, const WideCaps& caps, uint32_t gcode, bool switch_test, bool bounded,
                           NicSearch& ns) {
    const uint32_t G = r.n_groups, U = n.numa_nodes;
    const bool pci = switch_test && r.map_type == NHDFIT_MAP_PCI;
    uint32_t numa = 0, pick = 0, order = 0;                   // 2 / 4 / 3 bits per group (or per search position)
    auto numa_of = [&](uint32_t g) { return numa >> (2 * g) & 3u; };
    auto pick_of = [&](uint32_t g) { return pick >> (4 * g) & 15u; };
    auto set_pick = [&](uint32_t g, uint32_t k) { pick = (pick & ~(15u << (4 * g))) | (k << (4 * g)); };
    auto order_at = [&](uint32_t q) { return order >> (3 * q) & 7u; };
    for (int g = (int)G - 1, c = (int)gcode; g >= 0; --g) { numa |= (uint32_t)(c % (int)U) << (2 * g); c /= (int)U; }
    uint32_t cnt = 0;
    for (uint32_t u = 0; u < U; ++u)
        for (uint32_t g = 0; g < G; ++g)
            if (numa_of(g) == u) order |= g << (3 * cnt++);
    for (uint32_t g = 0; g < G; ++g)
        if (n.nic_cnt[numa_of(g)] == 0) return false;          // a NUMA node without NICs hosts no group (quirk Q3)
    bool prune = true;
    for (uint32_t g = 0; g < G; ++g)
        if (!(r.rx[g] >= 0) || !(r.tx[g] >= 0)) prune = false;
    if (caps.sh && prune)
        for (uint32_t u = 0; u < U; ++u)
            for (uint32_t k = 0; k < n.nic_cnt[u]; ++k)
                if (caps.free_of(n, u, k, 0) < 0 || caps.free_of(n, u, k, 1) < 0) return false;
    auto nic_holds = [&](uint32_t upto, uint32_t u, uint32_t k) {
        double rx = caps.free_of(n, u, k, 0), tx = caps.free_of(n, u, k, 1);
        for (uint32_t q = 0; q <= upto; ++q) {
            const uint32_t h = order_at(q);
            if (numa_of(h) == u && pick_of(h) == k) { rx = rx - r.rx[h]; tx = tx - r.tx[h]; }
        }
        return !(rx < 0) && !(tx < 0);                         // Matcher.py:267
    };
    auto switch_holds = [&](uint32_t upto, uint32_t sw) {
        uint32_t c = 0;
        for (uint32_t q = 0; q <= upto; ++q) {
            const uint32_t h = order_at(q);
            if (n.nic_sw[numa_of(h)][pick_of(h)] == sw) ++c;
        }
        return c <= wide_sw_free(n, sw);                       // Matcher.py:318-322
    };
    auto twin_skipped = [&](int pos, uint32_t u, uint32_t k) {
        for (int q = 0; q < pos; ++q)
            if (numa_of(order_at(q)) == u && pick_of(order_at(q)) == k) return false;
        for (uint32_t k2 = 0; k2 < k; ++k2) {
            if (!caps.same_price(n, u, k, k2) || n.nic_sw[u][k2] != n.nic_sw[u][k]) continue;
            bool used = false;
            for (int q = 0; q < pos && !used; ++q) used = numa_of(order_at(q)) == u && pick_of(order_at(q)) == k2;
            if (!used) return true;
        }
        return false;
    };
    auto spend = [&]() {
        if (!bounded) return true;
        if (ns.left == 0) { ns.exhausted = true; return false; }
        ns.left--;
        return true;
    };
    if (prune) {
        int pos = 0;
        for (;;) {
            const uint32_t g = order_at((uint32_t)pos), u = numa_of(g), k = pick_of(g);
            if (!spend()) return false;
            const bool ok = !(req_traits<R>::kBig && twin_skipped(pos, u, k)) && nic_holds((uint32_t)pos, u, k) &&
                            (!pci || switch_holds((uint32_t)pos, n.nic_sw[u][k]));
            if (ok) {
                if (pos == (int)G - 1) return true;
                ++pos;
                continue;
            }
            for (;;) {
                const uint32_t h = order_at((uint32_t)pos);
                if (pick_of(h) + 1 < n.nic_cnt[numa_of(h)]) { set_pick(h, pick_of(h) + 1); break; }
                set_pick(h, 0);
                if (--pos < 0) return false;
            }
        }
    }
    for (;;) {
        if (!spend()) return false;
        bool ok = true;
        for (uint32_t q = 0; q < G && ok; ++q) {
            const uint32_t g = order_at(q);
            ok = nic_holds(G - 1, numa_of(g), pick_of(g)) && (!pci || switch_holds(G - 1, n.nic_sw[numa_of(g)][pick_of(g)]));
        }
        if (caps.sh)
            for (uint32_t u = 0; u < U && ok; ++u)
                for (uint32_t k = 0; k < n.nic_cnt[u] && ok; ++k) ok = nic_holds(G - 1, u, k);
        if (ok) return true;
        int pos = (int)G - 1;
        while (pos >= 0) {
            const uint32_t h = order_at((uint32_t)pos);
            if (pick_of(h) + 1 < n.nic_cnt[numa_of(h)]) { set_pick(h, pick_of(h) + 1); break; }
            set_pick(h, 0);
            --pos;
        }
        if (pos < 0) return false;
    }
}

// The stage of one pair.  `budget`: NIC search steps per question (0: unbounded); a question that runs out sets *exhausted and
// the pair has no answer (NOT_CANDIDATE is returned; the caller reports the call as failed).
template <class R>
NHD_HD uint32_t explain_stage(const nhdfit_wide_node& n, const R& r, bool listed, bool busy, const WideCaps& caps, uint32_t budget = 0,
                              bool* exhausted = nullptr) {
    if (!listed || !req_valid(r) || !wide_shape_ok(n)) return NHDFIT_STAGE_NOT_CANDIDATE;
    if (r.flags & NHDFIT_RF_INITIAL_FILTER)
        if (!(n.flags & NHDFIT_NF_ACTIVE) || !(n.groups & r.groups)) return NHDFIT_STAGE_NOT_CANDIDATE;
    if (n.flags & NHDFIT_NF_MAINTENANCE) return NHDFIT_STAGE_MAINTENANCE;
    if (r.hugepages_gb > n.hp_free) return NHDFIT_STAGE_HUGEPAGES;
    uint32_t want = 0;
    for (uint32_t g = 0; g < r.n_groups; ++g) want += r.gpus[g];
    if (busy && want) return NHDFIT_STAGE_BUSY;
    const ExFree f = explain_free(n);
    const uint32_t nG = wide_ipow(f.U, r.n_groups);
    bool any = false;
    for (uint32_t code = 0; code < nG && !any; ++code) any = explain_gpu_ok(r, f, code);
    if (!any) return NHDFIT_STAGE_GPU;
    any = false;
    for (uint32_t code = 0; code < nG * f.U && !any; ++code) any = explain_cpu_ok(r, f, code);
    if (!any) return NHDFIT_STAGE_CPU;
    // The NIC stage, the PCI pruning and the intersection, each "is there an assignment ...", each with a budget of its own
    const bool pci = r.map_type == NHDFIT_MAP_PCI;
    for (uint32_t q = 0; q < 3u; ++q) {                      // q = 0: the bandwidth test alone; 1: and the switch test (PCI pods: the
        if (q == 1 && !pci) continue;                         // PCI pruning); 2: every stage at once (the intersection, wide_fits' walk)
        NicSearch ns{budget, false};
        any = false;
        for (uint32_t code = 0; code < nG && !any; ++code) {
            if (q == 2) {
                if (!explain_gpu_ok(r, f, code)) continue;
                bool cpu = false;
                for (uint32_t m = 0; m < f.U && !cpu; ++m) cpu = explain_cpu_ok(r, f, code * f.U + m);
                if (!cpu) continue;
            }
            any = explain_nic_ok(n, r, caps, code, q >= 1, budget != 0, ns);
            if (ns.exhausted) {
                if (exhausted) *exhausted = true;
                return NHDFIT_STAGE_NOT_CANDIDATE;
            }
        }
        if (!any) return q == 0 ? NHDFIT_STAGE_NIC : q == 1 ? NHDFIT_STAGE_PCI : NHDFIT_STAGE_NUMA;
    }
    return NHDFIT_STAGE_FITS;
}

}  // namespace nhdfit
