// dccl_amd/csrc/phased_launch.hpp — the phased and the line-straddle launches of the k-way (CHAIN false) and chain
// (CHAIN true) combines, stated once.  Included by phased_multi.hip and phased_chain.hip only: each instantiates
// its own flag for every (T, OP), so the build compiles the two halves side by side.  own = d for the k-way.
#pragma once

#include "dispatch.hpp"
#include "reduce_kernels.hpp"

namespace dccl_amd {

template <typename T, int OP, int K, bool CHAIN>
int launch_phased(SendList sl, PhaseList ph, const unsigned char* own, unsigned char* d, Split sp,
                  hipStream_t stream) {
    constexpr caps::Kernel kFirst = CHAIN ? caps::kChainPhasedFirst : caps::kMultiPhasedFirst;
    constexpr bool first = caps::phased_loads_first(CHAIN, K);
    const size_t grid = grid_for(sp, 64);
    // the per-operand form uncapped (with the XCD order up to kPhasedXcdMaxK), or the loads-first form under
    // its own cap and in its own tile-run order (caps::kMultiPhasedFirst / kChainPhasedFirst, caps.hpp)
    constexpr bool xcd = !first && K <= kPhasedXcdMaxK;
    constexpr int run = first ? caps::tile_run(kFirst, K) : 1;
    const size_t lds = first ? caps::lds(kFirst, K, caps_bytes(sp.nvec * 16)) : 0;
    if constexpr (CHAIN) {
        void* args[] = {&sl, &ph, &own, &d, &sp.head, &sp.nvec, &sp.tail};
        return launch(reinterpret_cast<const void*>(&reduce_chain_phased_kernel<T, OP, K, xcd, first, run>), grid, args,
                      stream, 64, lds);
    } else {
        void* args[] = {&sl, &ph, &d, &sp.head, &sp.nvec, &sp.tail};
        return launch(reinterpret_cast<const void*>(&reduce_multi_phased_kernel<T, OP, K, xcd, first, run>), grid, args,
                      stream, 64, lds);
    }
}

template <typename T, int OP, int K, bool CHAIN>
int launch_straddle(SendList sl, const unsigned char* own, unsigned char* d, Split sp, hipStream_t stream) {
    // sources through the caches, in the tile-run order of caps::kRun, under the line-straddle caps by operand
    // size (caps::kMultiStraddle / kChainStraddle, caps.hpp)
    constexpr caps::Kernel kStraddle = CHAIN ? caps::kChainStraddle : caps::kMultiStraddle;
    using C = VecCfg<64, 1, kNtRecv | kNtStore, false, 0, caps::tile_run(kStraddle, K)>;
    const size_t grid = grid_for(sp, 64), lds = caps::lds(kStraddle, K, caps_bytes(sp.nvec * 16));
    if constexpr (CHAIN) {
        void* args[] = {&sl, &own, &d, &sp.head, &sp.nvec, &sp.tail};
        return launch(reinterpret_cast<const void*>(&reduce_chain_vec_kernel<T, OP, K, C>), grid, args, stream, 64, lds);
    } else {
        void* args[] = {&sl, &d, &sp.head, &sp.nvec, &sp.tail};
        return launch(reinterpret_cast<const void*>(&reduce_multi_vec_kernel<T, OP, K, C>), grid, args, stream, 64, lds);
    }
}

// The k-way combine has 2..8 sources (one source is the pairwise combine), the chain 1..8.
template <typename T, int OP, bool CHAIN>
int phased_typed(SendList sl, PhaseList ph, int nsend, const unsigned char* own, unsigned char* d, Split sp,
                 hipStream_t stream) {
    return with_k<(CHAIN ? 1 : 2), 8>(
        nsend, [&](auto K) { return launch_phased<T, OP, K.value, CHAIN>(sl, ph, own, d, sp, stream); });
}

template <typename T, int OP, bool CHAIN>
int straddle_typed(SendList sl, int nsend, const unsigned char* own, unsigned char* d, Split sp, hipStream_t stream) {
    return with_k<(CHAIN ? 1 : 2), 8>(
        nsend, [&](auto K) { return launch_straddle<T, OP, K.value, CHAIN>(sl, own, d, sp, stream); });
}

#define DCCL_PHASED_INST_OP(T, OP, CHAIN)                                                                          \
    template int straddle_typed<T, OP, CHAIN>(SendList, int, const unsigned char*, unsigned char*, Split, hipStream_t); \
    template int phased_typed<T, OP, CHAIN>(SendList, PhaseList, int, const unsigned char*, unsigned char*, Split,  \
                                            hipStream_t);
#define DCCL_PHASED_INST(T, CHAIN)        \
    DCCL_PHASED_INST_OP(T, kSum, CHAIN)   \
    DCCL_PHASED_INST_OP(T, kProd, CHAIN)  \
    DCCL_PHASED_INST_OP(T, kMax, CHAIN)   \
    DCCL_PHASED_INST_OP(T, kMin, CHAIN)
#define DCCL_PHASED_INST_ALL(CHAIN)     \
    DCCL_PHASED_INST(int8_t, CHAIN)     \
    DCCL_PHASED_INST(uint8_t, CHAIN)    \
    DCCL_PHASED_INST(int32_t, CHAIN)    \
    DCCL_PHASED_INST(uint32_t, CHAIN)   \
    DCCL_PHASED_INST(int64_t, CHAIN)    \
    DCCL_PHASED_INST(uint64_t, CHAIN)   \
    DCCL_PHASED_INST(f16_bits, CHAIN)   \
    DCCL_PHASED_INST(float, CHAIN)      \
    DCCL_PHASED_INST(double, CHAIN)     \
    DCCL_PHASED_INST(bf16_bits, CHAIN)

}  // namespace dccl_amd
