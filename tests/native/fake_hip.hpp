// tests/native/fake_hip.hpp — what the stream-order harness asks of the recording fake runtime (fake_hip.cpp).
#pragma once

#include <hip/hip_runtime_api.h>

#include <vector>

#include "hb_check.hpp"

namespace fake {

// The call site the calling thread's next records carry.
void set_site(int rank, int call);
// A new scenario: the trace, every allocation, stream and event are forgotten.  No rank thread may be running.
void reset();
// The records since reset(), in host order.
hb::Trace trace();
hipStream_t new_stream();
// A synthetic operation of the user (producer / consumer / clobber) enqueued on `st`.
void user_op(hipStream_t st, const char* what, std::vector<hb::Range> ranges);

inline hb::Range reads(const void* p, size_t bytes) {
    return hb::Range{reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes, false};
}
inline hb::Range writes(const void* p, size_t bytes) {
    return hb::Range{reinterpret_cast<uintptr_t>(p), reinterpret_cast<uintptr_t>(p) + bytes, true};
}

}  // namespace fake
