// dccl_amd/csrc/checked_entry.hpp — the checked widened sum's two device entry points (include/dccl/dccl_reduce.h,
// DESIGN.md §7.12) as the collectives' host code refers to them: weakly.  wide.hip defines them in the library.
// tests/native/fake_hip.cpp, the recording runtime that tests/test_stream_order.py links this host code against,
// defines the kernel entry points the harness reaches and not these two (it never creates a checked op); a weak
// reference leaves that link whole.  A caller asks checked_entries_linked() first.
#pragma once

#include "dccl/dccl_reduce.h"

extern "C" {
__attribute__((weak)) int dccl_local_reduce_chain_widen_checked(const void* const* sends, int nsend, const void* own,
                                                                void* dst, int dtype, size_t count, int accumulate,
                                                                uint32_t* flag, void* stream);
__attribute__((weak)) int dccl_local_nonfinite_f32(const void* src, size_t count, uint32_t* flag, void* stream);
}

namespace dccl_amd {

inline bool checked_entries_linked() {
    return &dccl_local_reduce_chain_widen_checked != nullptr && &dccl_local_nonfinite_f32 != nullptr;
}

}  // namespace dccl_amd
