// dccl_amd/csrc/select.hpp — which algorithm runs a collective: the one place that decides it.
// Host-only C++ (no HIP header, and it reads no environment): dccl_api.cpp reads DCCL_ALLREDUCE_ALGORITHM once per
// call, when the call is validated, and switches on select()'s answer when the call runs; tests/test_select.py
// compiles this file with g++ and checks select() over the whole grid against the rules restated in the test.
#pragma once

#include <cstddef>
#include <cstdint>

#include "group_plan.hpp"

namespace dccl_amd {

constexpr uint32_t kDirectMaxWorld = 8;  // one 8-GPU node; <= 8 copy pairs / chain sends per launch

// Which sum a reduction computes (comm.hpp SumForm carries it with its scalar).  New kinds are appended: the values
// are what tests/test_select.py and the selector's callers pass.
enum SumKind : int { kBuiltin = 0, kPremulSum, kWideSum, kWideScaledSum, kWidenedSum };

// DCCL_ALLREDUCE_ALGORITHM (the reference's DCCL/allreduce_algorithm key, dccl.hpp:38-46, whose values are "ring"
// and "rabenseifner": DCCL_ALLREDUCE_RING / DCCL_ALLREDUCE_RABENSEIFNER of include/dccl/dccl.hpp).  Unset, "" and
// "auto" leave the choice to select().  The reference defaults to ring and silently skips the reduction for any
// other value (dccl.cpp:412-501); here kUnknown is ncclInvalidUsage for ncclAllReduce.
enum class AlgoName { kAuto, kRing, kRabenseifner, kDirect, kGrouped, kUnknown };

constexpr bool same_text(const char* a, const char* b) {
    while (*a != 0 && *a == *b) ++a, ++b;
    return *a == *b;
}

constexpr AlgoName parse_algo(const char* s) {
    if (s == nullptr || *s == 0 || same_text(s, "auto")) return AlgoName::kAuto;
    if (same_text(s, "ring")) return AlgoName::kRing;
    if (same_text(s, "rabenseifner")) return AlgoName::kRabenseifner;
    if (same_text(s, "direct")) return AlgoName::kDirect;
    if (same_text(s, "grouped")) return AlgoName::kGrouped;
    return AlgoName::kUnknown;
}

// How the communicator's ranks reach each other: threads of one process (comm.hpp), processes on the IPC
// peer-read transport (direct.hpp), RCCL, or a plugged-in point-to-point transport.
enum class Transport { kThreads, kIpc, kRccl, kP2p };

// Everything a collective's run function can do.
enum class Path {
    kLocal,         // W == 1: dst = src (times the scalar of a pre-multiplied sum)
    kDirect,        // direct.hpp: every rank reads its peers' device buffers
    kHostDirect,    // the same choreography on host buffers of an in-process group
    kWideStaged,    // a wide sum off the direct path: widened, run as an fp32 collective, rounded once (a widened
                    // sum: not rounded)
    kGrouped,       // algorithms.hpp: grouped exchanges on RCCL
    kRabenseifner,  // ncclAllReduce only
    kRing,          // the ring; for ncclReduce the ring and its gather, for ncclBroadcast the root's fan-out
};

// The peer-read forms are faster than the ring at every size measured and give its bits, so they
// come first: always on IPC (it has no other), on threads unless the name asks for another algorithm; never on
// RCCL or a plugged-in transport, where "direct" runs the ring.  "grouped" is not the default on RCCL yet (§7.2).
inline Path select(int api, Transport t, uint32_t world, bool device, SumKind kind, AlgoName name) {
    const bool reduces = api <= group::kReduce;
    // a widened sum (fp32 recvbuff) goes where the wide sums go: direct, else staged through fp32
    const bool wide = reduces && (kind == kWideSum || kind == kWideScaledSum || kind == kWidenedSum);
    if (world == 1) return wide ? Path::kWideStaged : Path::kLocal;
    const bool peer_read = t == Transport::kThreads && world <= kDirectMaxWorld &&
                           (name == AlgoName::kAuto || name == AlgoName::kDirect);
    if (device && (t == Transport::kIpc || peer_read)) return Path::kDirect;
    if (!reduces) return Path::kRing;
    const bool scatters = api != group::kReduce;  // ncclReduce has neither a host-direct nor a grouped form
    if (scatters && !device && peer_read) return Path::kHostDirect;
    if (wide) return Path::kWideStaged;
    if (scatters && kind == kBuiltin && device && t == Transport::kRccl && name == AlgoName::kGrouped)
        return Path::kGrouped;
    if (api == group::kAllReduce && name == AlgoName::kRabenseifner) return Path::kRabenseifner;
    return Path::kRing;
}

// Slots the algorithm of `p` cuts its buffer into (group_plan.hpp): what a packed group is laid out by.
inline size_t slots(Path p, uint32_t world) { return group::slots_of(world, p == Path::kRabenseifner); }

}  // namespace dccl_amd
