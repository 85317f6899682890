// dccl_amd/csrc/routing.hpp — where the operands of a k-way or chain combine lie, and which launch takes them.
// Host-only C++ (no HIP header): tests/test_routing.py compiles it with g++ and checks route() over an exhaustive
// grid of placements against the rules restated in the test.  local_reduce.hip switches on route()'s result;
// chain_forms.hpp (the pre-multiplied and wide chains) uses the same classifier.
#pragma once

#include <cstddef>
#include <cstdint>

#include "caps.hpp"

namespace dccl_amd {

struct SendList { const unsigned char* p[8]; };
// p[k]: 16-B phase of source k's body; p[nsend]: of own's (chain).
struct PhaseList { unsigned p[9]; };

inline SendList send_list(const void* const* sends, int nsend) {
    SendList sl{};
    for (int k = 0; k < nsend; ++k) sl.p[k] = static_cast<const unsigned char*>(sends[k]);
    return sl;
}

struct Split {
    size_t head, nvec, tail;
};

// head scalars bring recv to an `align`-byte boundary (16 or more, a power of two).  Aligning recv to
// its 128-B lines keeps every tile's recv loads and stores whole-line: a recv that straddles lines
// costs 10-15 % (phase_probe.py@4f20423, profiles/r1_s3_phase_probe.json).  head < align / esz; esz: bytes per
// element.
inline Split split_for_vectors(uintptr_t recv, size_t count, size_t esz, size_t align) {
    const size_t V = 16 / esz;
    size_t head = ((align - (recv & (align - 1))) & (align - 1)) / esz;
    if (head > count) head = count;
    const size_t rest = count - head;
    const size_t nvec = rest / V;
    return Split{head, nvec, rest - nvec * V};
}

// One block per `tile` vectors; a split with no whole vector still needs block 0 for its head / tail elements.
inline size_t grid_for(Split sp, size_t tile) {
    const size_t grid = (sp.nvec + tile - 1) / tile;
    return grid == 0 && sp.head + sp.tail > 0 ? 1 : grid;
}

// 16-B phase of an operand whose body starts `off` bytes in (see PhaseList).
inline unsigned phase_word(const void* base, size_t off) {
    return unsigned((reinterpret_cast<uintptr_t>(base) + off) & 15);
}

// Where the operands lie against the destination (own = dst for the k-way combine).
struct Placement {
    bool dst_elem;  // the destination element-aligned
    bool elem_ok;   // every operand element-aligned (the destination, own and the sources)
    bool src_off;   // some source at another 16-B phase than the destination
    bool own_off;   // own at another 16-B phase than the destination
    bool in_phase() const { return !src_off && !own_off; }
};
inline Placement classify(const void* const* sends, int nsend, const void* own, const void* dst, size_t esz) {
    const uintptr_t ad = reinterpret_cast<uintptr_t>(dst), ao = reinterpret_cast<uintptr_t>(own);
    Placement c{ad % esz == 0, ad % esz == 0 && ao % esz == 0, false, ((ad ^ ao) & 15) != 0};
    for (int k = 0; k < nsend; ++k) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(sends[k]);
        if (a % esz) c.elem_ok = false;
        if ((a ^ ad) & 15) c.src_off = true;
    }
    return c;
}

// The launches of a k-way (recv = op(...op(recv, s0)..., s{k-1}); own = dst = recv) or chain combine.
enum Route : int {
    kRoutePair = 0,        // one source (chain: in place): the pairwise combine's own dispatch
    kRouteWindowsDstOff,   // destination off element alignment: the windows kernels, operands at any phase
    kRouteWindowsViaCaps,  // element-aligned destination, operands off phase, where caps::phased_via_windows says so
    kRoutePhased,          // element-aligned destination, operands at other 16-B (or byte) phases
    kRouteStraddle,        // in phase, some source off the destination's 128-B line grid (loaded through the caches)
    kRouteInPhase,         // in phase and on the line grid: the vector kernels
};
struct Routed {
    Route route;
    Split sp;      // phased, straddle, in phase: the destination's split (head up to `align`)
    PhaseList ph;  // windows: phases of the operands themselves; phased: of their bodies past the head
};

// esz: bytes per element; align: the destination alignment the head scalars reach; scaled_bytes: bytes per operand
// as the size-selected forms see them (dispatch.hpp caps_bytes).  count > 0, 1 <= nsend <= 8.
inline Routed route(bool chain, int nsend, size_t esz, const void* const* sends, const void* own, const void* dst,
                    size_t count, size_t align, size_t scaled_bytes) {
    Routed r{kRouteInPhase, {0, 0, 0}, {}};
    // One source is the pairwise combine itself: take its tuned dispatch (every alignment class).  The
    // k-way kernel at k = 1 ran at 78.7 % of peak at 1 GiB against 85 % for the pairwise kernel
    // (profiles/r2_kway_pmc.json, traffic exactly 3N in both).  Chain: dst = op(own, s0) is that combine only in
    // place (recv = own = dst).
    if (nsend == 1 && (!chain || own == dst)) {
        r.route = kRoutePair;
        return r;
    }
    const Placement c = classify(sends, nsend, own, dst, esz);
    const uintptr_t ad = reinterpret_cast<uintptr_t>(dst);
    const auto phases = [&](size_t off) {
        for (int k = 0; k < nsend; ++k) r.ph.p[k] = phase_word(sends[k], off);
        if (chain) r.ph.p[nsend] = phase_word(own, off);
    };
    if (!c.dst_elem) {  // 16-B accesses at the destination's own address, operands at any phase
        r.route = kRouteWindowsDstOff;
        phases(0);
        return r;
    }
    if (!c.in_phase()) {
        // The windows kernel's off-phase forms were measured with sources off phase, not with `own` alone off
        // phase: that chain launch keeps the phased kernels.  A one-byte element has no windows kernel.
        const bool measured = chain ? c.src_off : true;
        if (esz > 1 && measured && caps::phased_via_windows(chain, nsend, scaled_bytes, (ad & 15) == 0)) {
            r.route = kRouteWindowsViaCaps;
            phases(0);
            return r;
        }
        r.route = kRoutePhased;
        r.sp = split_for_vectors(ad, count, esz, align);
        phases(r.sp.head * esz);
        return r;
    }
    r.sp = split_for_vectors(ad, count, esz, align);
    // In-phase sources off recv's 128-B line grid (recv is line-aligned past the head): their loads go
    // through the caches, so the line two neighbouring tiles share is fetched once (StraddleCfg's rule).
    // 1 GiB-class A/B on one MI355X (profiles/r1_s5_kway_straddle_ab.json): k = 1 76.7 -> 85.6 %,
    // k = 2 75.5 -> 78.0 %, k = 4 74.4 -> 78.4 %, k = 7 72.3 -> 77.5 % of HBM peak.
    for (int k = 0; k < nsend; ++k)
        if ((reinterpret_cast<uintptr_t>(sends[k]) + r.sp.head * esz) & 127) r.route = kRouteStraddle;
    return r;
}

}  // namespace dccl_amd
