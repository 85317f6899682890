// dccl_amd/csrc/phased_multi.hip — the k-way combine recv = op(...op(recv, s0)..., s{K-1}) for element-aligned
// operands whose 16-B phases differ from the destination's (reduce_multi_phased_kernel in
// reduce_kernels.hpp) or whose sources straddle its lines; the launches are phased_launch.hpp's with CHAIN false.
// Instantiated for every (T, OP) here, in a translation unit of its own, so the build compiles it beside
// local_reduce.hip and phased_chain.hip.
#include <hip/hip_runtime.h>

#include "phased_launch.hpp"

namespace dccl_amd {
DCCL_PHASED_INST_ALL(false)
}  // namespace dccl_amd
