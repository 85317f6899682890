// dccl_amd/csrc/group_plan.hpp — what ncclGroupEnd does with the calls queued since ncclGroupStart: which
// stretches of reductions are folded into one collective, and the layout of the buffer they are packed into.
// No HIP include: dccl_api.cpp uses it, tests/test_group_plan.py compiles it with g++.
//
// Slot-major packing.  Every algorithm here combines an element's W contributions in an order that depends only
// on the slot of its buffer the element lies in, a slot being one of the P equal parts the algorithm cuts the
// buffer into (P = W for the ring, direct and grouped forms, 2^floor(log2 W) for Rabenseifner).  The packed
// buffer's slot k is the concatenation of slot k of every tensor of the run (padded to a line), so one
// collective on it takes every element through the combine order it would have had alone: the results are the
// per-tensor collectives' bits.
//
// Every criterion below is something all ranks agree on by NCCL's contract (api, count, dtype, op, root,
// placement, the two environment limits).  Streams, pointer values and alignment never enter: a plan that
// differed between ranks would pair different collectives.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace dccl_amd {
namespace group {

enum Api : int { kAllReduce = 0, kReduceScatter = 1, kReduce = 2, kAllGather = 3, kBroadcast = 4 };

constexpr size_t kMaxRun = 32;        // tensors per coalesced run (dccl_copy_rows_multi's segment limit)
constexpr size_t kSlotAlign = 128;    // kDeviceCachelineSize: every packed slot starts on a line
// Tensors of this many bytes or more are never packed: the largest of 4 KiB, 64 KiB, 1 MiB, 16 MiB and 64 MiB at
// which a coalesced group of 16 was still at least 10 % faster than its plain calls (5.5 x at 1 MiB, 0.85 x at
// 16 MiB; one MI355X, thread ranks, W = 4).  It serves widened runs too, compared against their
// 16-bit bytes: packing them was still 1.5 x faster at 4 MiB, the largest of 4 KiB .. 16 MiB with a gain of 10 % or
// more, so they need no lower limit of their own (§7.11).
constexpr size_t kDefaultMaxBytes = size_t(1) << 20;

// What the plan may look at of one queued call.  `count` is the element count of the whole reduced buffer
// (recvcount * W for a reduce-scatter); `op` the op value as the caller passed it (a pre-multiplied-sum handle
// included); `comm` only tells communicators apart.
struct Call {
    int api = 0;
    const void* comm = nullptr;
    size_t count = 0;
    size_t esz = 0;
    int dtype = 0;
    int op = 0;
    int root = 0;
    bool device = false;
    uint32_t world = 1;
    // Set: the call runs alone, in issue order, whatever else holds.
    bool never_packed = false;
    // Element size of the call's OUTPUT where it differs from `esz` (a widened sum: 16-bit sendbuff, fp32 recvbuff:
    // 4); 0: the same as `esz`.  Calls of one run agree on it: the op value decides it, and same_run compares that.
    size_t out_esz = 0;
};

struct Run {
    size_t first = 0, n = 0;
    bool packed = false;  // false: every call of the run (there is one) executes as the plain call
};

inline bool packable(const Call& c, size_t max_bytes) {
    return max_bytes > 0 && !c.never_packed && c.api <= kReduce && c.device && c.world > 1 && c.count > 0 &&
           c.count * c.esz < max_bytes;
}

inline bool same_run(const Call& a, const Call& b) {
    return a.api == b.api && a.comm == b.comm && a.dtype == b.dtype && a.op == b.op && a.device == b.device &&
           (a.api != kReduce || a.root == b.root);
}

// Cuts the queue into runs, in issue order.  max_bytes 0 turns packing off.
inline std::vector<Run> plan_runs(const Call* calls, size_t n, size_t max_bytes) {
    std::vector<Run> runs;
    for (size_t i = 0; i < n;) {
        size_t m = 1;
        if (packable(calls[i], max_bytes))
            while (i + m < n && m < kMaxRun && packable(calls[i + m], max_bytes) && same_run(calls[i], calls[i + m])) ++m;
        runs.push_back(Run{i, m, m > 1});
        i += m;
    }
    return runs;
}

// Packed layout of a run of n <= kMaxRun tensors cut into P slots: tensor i's slot k lies at byte
// k * S + off[i] of the packed buffer, slot[i] bytes long; pad bytes sit at the end of each packed slot only.
//
// The collective's result lies in an output region of its own elements, out_esz bytes each (esz unless the run's
// calls say otherwise): element j of the packed input is element j of the output, so tensor i's slot k lies at
// byte k * S_out + out_off[i] of the region, out_slot[i] bytes long, each the input's number times out_esz / esz.
// With equal sizes the two layouts are one.  16-bit in, fp32 out: every output offset is a multiple of 4 and every
// output slot k * S_out starts on a 256-B boundary of the region.
struct Layout {
    size_t slot[kMaxRun], off[kMaxRun];
    size_t out_slot[kMaxRun], out_off[kMaxRun];
    size_t S = 0;      // bytes of one packed slot, a multiple of kSlotAlign
    size_t S_out = 0;  // bytes of one slot of the output region
    size_t count = 0;  // elements of the packed buffer: P * S / esz
};

inline Layout pack_layout(const Call* calls, size_t n, size_t P) {
    Layout L;
    size_t sum = 0;
    for (size_t i = 0; i < n; ++i) {
        L.slot[i] = calls[i].count / P * calls[i].esz;
        L.off[i] = sum;
        sum += L.slot[i];
    }
    L.S = (sum + kSlotAlign - 1) / kSlotAlign * kSlotAlign;
    L.count = P * L.S / calls[0].esz;
    const size_t esz = calls[0].esz, out_esz = calls[0].out_esz != 0 ? calls[0].out_esz : esz;
    for (size_t i = 0; i < n; ++i) {
        L.out_slot[i] = L.slot[i] / esz * out_esz;
        L.out_off[i] = L.off[i] / esz * out_esz;
    }
    L.S_out = L.S / esz * out_esz;
    return L;
}

// Slots an algorithm cuts its buffer into.
inline size_t slots_of(uint32_t world, bool rabenseifner) {
    if (!rabenseifner) return world;
    size_t p = 1;
    while (p * 2 <= world) p *= 2;
    return p;
}

}  // namespace group
}  // namespace dccl_amd
