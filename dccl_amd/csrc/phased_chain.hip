// dccl_amd/csrc/phased_chain.hip — the chain combine dst = op(own, op(s{K-1}, ... op(s1, s0))) (the ring order,
// DESIGN.md §7.3) for element-aligned operands whose 16-B phases differ from the destination's
// (reduce_chain_phased_kernel in reduce_kernels.hpp) or whose sources straddle its lines; the launches are
// phased_launch.hpp's with CHAIN true.  Instantiated for every (T, OP) here, in a translation unit of its own, so
// the build compiles it beside local_reduce.hip and phased_multi.hip.
#include <hip/hip_runtime.h>

#include "phased_launch.hpp"

namespace dccl_amd {
DCCL_PHASED_INST_ALL(true)
}  // namespace dccl_amd
