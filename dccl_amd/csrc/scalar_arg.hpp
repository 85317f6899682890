// dccl_amd/csrc/scalar_arg.hpp — how a scalar reaches the kernels of the pre-multiplied sums (premul.hip) and the
// scaled wide sums (wide.hip).  It travels as a kernel argument {bits, dev_ptr}: with dev_ptr set every wave loads
// it from device memory when it runs (stream-ordered, so a captured graph replays with the value of the moment);
// otherwise `bits` holds the value the host read at the call.
#pragma once

#include <cstdint>
#include <cstring>

#include "reduce_kernels.hpp"

namespace dccl_amd {

struct ScalarArg {
    uint64_t bits;        // the scalar's bytes (host-immediate residence)
    const void* dev_ptr;  // non-null: read the scalar here when the kernel runs (device residence)
};

template <typename T>
__device__ __forceinline__ T load_scalar(const ScalarArg& a) {
    if (a.dev_ptr != nullptr) return ld_elem<T, false>(static_cast<const unsigned char*>(a.dev_ptr), 0);
    T s;
    __builtin_memcpy(&s, &a.bits, sizeof(T));
    return s;
}

inline bool scalar_ok(const void* scalar, int residence) {
    return scalar != nullptr && (residence == 0 || residence == 1);
}

// residence 0: the device address itself; 1: the host value of `bytes` bytes, read now
inline ScalarArg make_scalar(const void* scalar, int residence, size_t bytes) {
    ScalarArg sa{0, nullptr};
    if (residence == 0) sa.dev_ptr = scalar;
    else std::memcpy(&sa.bits, scalar, bytes);
    return sa;
}

}  // namespace dccl_amd
