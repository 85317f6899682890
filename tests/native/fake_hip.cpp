// tests/native/fake_hip.cpp — a HIP runtime, and the kernel entry points of include/dccl/dccl_reduce.h, that execute
// nothing and record everything.  The host code of the collectives (comm.cpp, algorithms.cpp,
// grouped.cpp, bootstrap.cpp, dccl_api.cpp, direct.cpp, rccl_transport.cpp) links against this file instead of the
// HIP runtime and the .hip translation units; tests/native/stream_order_harness.cpp drives it.
//
// Every call appends one record to a global trace under a mutex, which gives the total host order hb_check.hpp
// works from.
//   Memory    hipMalloc / hipHostMalloc hand out addresses from a bump allocator inside one PROT_NONE reservation:
//             nothing is ever backed (a communicator's 64 MiB scratchpads cost address space only), and a host
//             dereference of "device" memory by product code ends the process at once, which is a finding.
//             hipPointerGetAttributes and hipMemGetAddressRange answer from the allocation table: hipMalloc ranges
//             are device memory, hipHostMalloc ranges host memory, anything else is unknown to the runtime (the
//             product takes that for host memory).
//   Streams   and events are opaque ids.  hipEventRecord / hipStreamWaitEvent become records; the checker binds a
//             wait to the latest earlier record of its event, HIP's rule.
//   Enqueued  operations (hipMemcpyAsync, hipMemsetAsync, every kernel entry point) declare the byte ranges they
//             read and write, taken from the entry point's contract in dccl_reduce.h.  A destination that is also
//             read (a combine's recv, an accumulate) is a write: for ordering a write conflicts with everything.
//             A scalar in device memory is a read of its 4 or 8 bytes; a host-immediate scalar is read here, on the
//             host, as the contract says ("read before the call returns").
//   Syncs     hipStreamSynchronize, hipEventSynchronize, hipDeviceSynchronize, the blocking hipMemcpy and hipFree
//             (device-wide, as comm.cpp's grow() assumes) are host synchronisations: what they cover happens before
//             everything issued later in host order by ANY thread.  That is deliberately generous across threads
//             (hb_check.hpp): it cannot report a false hazard in the barrier-synchronised direct collectives and can
//             miss a real one there.  The two *_host entry points are host-synchronous operations.
//   Not here  RCCL (never loaded: the harness uses the thread transport only) and the IPC calls (they fail).
#include "fake_hip.hpp"

#include <sys/mman.h>

#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>

#include "dccl/dccl_reduce.h"

namespace dccl_amd {
int copy_rows_launch(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, hipStream_t stream);
int add_rows_launch(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, hipStream_t stream);
}  // namespace dccl_amd

namespace {

constexpr size_t kReserve = size_t(1) << 37;  // 128 GiB of addresses, none of it backed
constexpr size_t kPage = 4096;
constexpr uintptr_t kStreamBase = 0x1000, kEventBase = 0x100000;
constexpr uint64_t kHostStreamBase = uint64_t(1) << 40;  // pseudo-streams of the host-synchronous entry points

struct Alloc {
    size_t bytes = 0;
    bool device = false;
};

struct State {
    std::mutex mu;
    hb::Trace trace;
    unsigned char* base = nullptr;
    size_t used = 0;
    std::map<uintptr_t, Alloc> allocs;
    uintptr_t streams = 0, events = 0;
};

State& S() {
    static State s;
    return s;
}

thread_local int tl_rank = -1, tl_call = -1;

uint64_t id_of(const void* handle) { return reinterpret_cast<uintptr_t>(handle); }

// Appends under the mutex; `user` marks the harness's own operations.
void append(hb::Kind kind, const char* fn, uint64_t stream, uint64_t event, std::vector<hb::Range> ranges,
            hb::Covers covers = hb::Covers::kStream, bool user = false) {
    hb::Rec r;
    r.kind = kind;
    r.fn = fn;
    r.stream = stream;
    r.event = event;
    r.covers = covers;
    r.ranges = std::move(ranges);
    r.rank = tl_rank;
    r.call = tl_call;
    r.user = user;
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    s.trace.push_back(std::move(r));
}

void op(const char* fn, const void* stream, std::vector<hb::Range> ranges) {
    append(hb::Kind::kOp, fn, id_of(stream), 0, std::move(ranges));
}

hipError_t allocate(void** out, size_t bytes, bool device) {
    if (out == nullptr) return hipErrorInvalidValue;
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    if (s.base == nullptr) {
        void* p = mmap(nullptr, kReserve, PROT_NONE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) {
            std::perror("fake_hip: mmap");
            std::abort();
        }
        s.base = static_cast<unsigned char*>(p);
    }
    const size_t span = (bytes + kPage - 1) / kPage * kPage + kPage;  // one guard page of distance
    if (s.used + span > kReserve) return hipErrorOutOfMemory;
    unsigned char* p = s.base + s.used;
    s.used += span;
    s.allocs[reinterpret_cast<uintptr_t>(p)] = Alloc{bytes, device};
    *out = p;
    return hipSuccess;
}

// The allocation that holds `p`, or null.
const std::pair<const uintptr_t, Alloc>* find_alloc(State& s, const void* p) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(p);
    auto it = s.allocs.upper_bound(x);
    if (it == s.allocs.begin()) return nullptr;
    --it;
    return x < it->first + it->second.bytes ? &*it : nullptr;
}

size_t esz_of(int dtype) {
    switch (dtype) {
    case 0: case 1: return 1;
    case 6: case 9: return 2;
    case 2: case 3: case 7: return 4;
    case 4: case 5: case 8: return 8;
    default: return 0;
    }
}

// A scalar argument: device memory is read by the kernel (a range), host memory is read now.
bool scalar_arg(const void* scalar, int residence, size_t bytes, std::vector<hb::Range>* ranges) {
    if (scalar == nullptr || (residence != 0 && residence != 1)) return false;
    if (residence == 0) {
        ranges->push_back(fake::reads(scalar, bytes));
    } else {
        volatile unsigned char sink = 0;
        for (size_t i = 0; i < bytes; ++i) sink = sink ^ static_cast<const volatile unsigned char*>(scalar)[i];
    }
    return true;
}

// The chain entry points' ranges: sends[j] and own are read, dst is written (`dst_esz` bytes per element).
int chain_op(const char* fn, const void* const* sends, int nsend, const void* own, void* dst, int dtype, size_t count,
             size_t dst_esz, std::vector<hb::Range> ranges, void* stream) {
    const size_t esz = esz_of(dtype);
    if (esz == 0 || nsend < 1 || nsend > 8 || sends == nullptr) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (own == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    for (int j = 0; j < nsend; ++j) {
        if (sends[j] == nullptr) return DCCL_INVALID_ARGUMENT;
        ranges.push_back(fake::reads(sends[j], count * esz));
    }
    ranges.push_back(fake::reads(own, count * esz));
    ranges.push_back(fake::writes(dst, count * dst_esz));
    op(fn, stream, std::move(ranges));
    return DCCL_SUCCESS;
}

int rows_op(const char* fn, const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, hipStream_t stream) {
    std::vector<hb::Range> ranges;
    for (int i = 0; i < nsegs; ++i)
        for (uint32_t r = 0; r < rows && segs[i].row_bytes > 0; ++r) {
            ranges.push_back(fake::reads(static_cast<const unsigned char*>(segs[i].src) + r * segs[i].src_stride,
                                         segs[i].row_bytes));
            ranges.push_back(fake::writes(static_cast<unsigned char*>(segs[i].dst) + r * segs[i].dst_stride,
                                          segs[i].row_bytes));
        }
    if (!ranges.empty()) op(fn, stream, std::move(ranges));
    return DCCL_SUCCESS;
}

// A host-synchronous entry point: the device is idle before it (it stages through the GPU and waits), it runs on a
// pseudo-stream of the calling thread, and it is complete on return.
void host_op(const char* fn, std::vector<hb::Range> ranges) {
    const uint64_t pseudo = kHostStreamBase + uint64_t(tl_rank + 1);
    append(hb::Kind::kSync, fn, 0, 0, {}, hb::Covers::kDevice);
    append(hb::Kind::kOp, fn, pseudo, 0, std::move(ranges));
    append(hb::Kind::kSync, fn, pseudo, 0, {}, hb::Covers::kStream);
}

}  // namespace

namespace fake {

void set_site(int rank, int call) {
    tl_rank = rank;
    tl_call = call;
}

void reset() {
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    s.trace.clear();
    s.allocs.clear();
    s.used = 0;
    s.streams = s.events = 0;
}

hb::Trace trace() {
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    return s.trace;
}

hipStream_t new_stream() {
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    return reinterpret_cast<hipStream_t>(kStreamBase + ++s.streams);
}

void user_op(hipStream_t st, const char* what, std::vector<hb::Range> ranges) {
    append(hb::Kind::kOp, what, id_of(st), 0, std::move(ranges), hb::Covers::kStream, true);
}

}  // namespace fake

// ------------------------------------------------------------------------------------------- the HIP runtime
extern "C" {

hipError_t hipGetDevice(int* device) {
    if (device == nullptr) return hipErrorInvalidValue;
    *device = 0;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
hipError_t hipDeviceCanAccessPeer(int* can, int, int) {
    if (can != nullptr) *can = 1;
    return hipSuccess;
}
hipError_t hipDeviceEnablePeerAccess(int, unsigned int) { return hipSuccess; }

hipError_t hipMalloc(void** ptr, size_t size) { return allocate(ptr, size, true); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) { return allocate(ptr, size, false); }
hipError_t hipFree(void* ptr) {  // synchronises the device
    append(hb::Kind::kSync, "hipFree", 0, 0, {}, hb::Covers::kDevice);
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    return ptr == nullptr || s.allocs.erase(reinterpret_cast<uintptr_t>(ptr)) == 1 ? hipSuccess : hipErrorInvalidValue;
}
hipError_t hipHostFree(void* ptr) { return hipFree(ptr); }
hipError_t hipHostRegister(void*, size_t, unsigned int) { return hipSuccess; }
hipError_t hipHostUnregister(void*) { return hipSuccess; }

hipError_t hipPointerGetAttributes(hipPointerAttribute_t* a, const void* ptr) {
    if (a == nullptr) return hipErrorInvalidValue;
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    const auto* al = find_alloc(s, ptr);
    if (al == nullptr) return hipErrorInvalidValue;  // not the runtime's: the product takes it for host memory
    *a = hipPointerAttribute_t{};
    a->type = al->second.device ? hipMemoryTypeDevice : hipMemoryTypeHost;
    a->device = 0;
    a->devicePointer = const_cast<void*>(ptr);
    a->hostPointer = al->second.device ? nullptr : const_cast<void*>(ptr);
    return hipSuccess;
}
hipError_t hipPointerGetAttribute(void*, hipPointer_attribute, hipDeviceptr_t) { return hipErrorNotSupported; }
hipError_t hipMemGetAddressRange(hipDeviceptr_t* base, size_t* size, hipDeviceptr_t ptr) {
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    const auto* al = find_alloc(s, ptr);
    if (al == nullptr) return hipErrorInvalidValue;
    if (base != nullptr) *base = reinterpret_cast<hipDeviceptr_t>(al->first);
    if (size != nullptr) *size = al->second.bytes;
    return hipSuccess;
}

hipError_t hipIpcGetMemHandle(hipIpcMemHandle_t*, void*) { return hipErrorNotSupported; }
hipError_t hipIpcOpenMemHandle(void**, hipIpcMemHandle_t, unsigned int) { return hipErrorNotSupported; }
hipError_t hipIpcCloseMemHandle(void*) { return hipErrorNotSupported; }

hipError_t hipStreamCreateWithFlags(hipStream_t* stream, unsigned int) {
    if (stream == nullptr) return hipErrorInvalidValue;
    *stream = fake::new_stream();
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* event, unsigned) {
    if (event == nullptr) return hipErrorInvalidValue;
    State& s = S();
    std::lock_guard<std::mutex> lk(s.mu);
    *event = reinterpret_cast<hipEvent_t>(kEventBase + ++s.events);
    return hipSuccess;
}
hipError_t hipEventDestroy(hipEvent_t event) { return event != nullptr ? hipSuccess : hipErrorInvalidValue; }

hipError_t hipEventRecord(hipEvent_t event, hipStream_t stream) {
    if (event == nullptr) return hipErrorInvalidValue;
    append(hb::Kind::kRecord, "hipEventRecord", id_of(stream), id_of(event), {});
    return hipSuccess;
}
hipError_t hipStreamWaitEvent(hipStream_t stream, hipEvent_t event, unsigned int) {
    if (event == nullptr) return hipErrorInvalidValue;
    append(hb::Kind::kWait, "hipStreamWaitEvent", id_of(stream), id_of(event), {});
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t stream) {
    append(hb::Kind::kSync, "hipStreamSynchronize", id_of(stream), 0, {}, hb::Covers::kStream);
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t event) {
    append(hb::Kind::kSync, "hipEventSynchronize", 0, id_of(event), {}, hb::Covers::kEvent);
    return hipSuccess;
}
hipError_t hipDeviceSynchronize(void) {
    append(hb::Kind::kSync, "hipDeviceSynchronize", 0, 0, {}, hb::Covers::kDevice);
    return hipSuccess;
}

hipError_t hipMemcpyAsync(void* dst, const void* src, size_t bytes, hipMemcpyKind, hipStream_t stream) {
    if (bytes == 0) return hipSuccess;
    if (dst == nullptr || src == nullptr) return hipErrorInvalidValue;
    op("hipMemcpyAsync", stream, {fake::reads(src, bytes), fake::writes(dst, bytes)});
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* dst, int, size_t bytes, hipStream_t stream) {
    if (bytes == 0) return hipSuccess;
    if (dst == nullptr) return hipErrorInvalidValue;
    op("hipMemsetAsync", stream, {fake::writes(dst, bytes)});
    return hipSuccess;
}
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {  // blocking: a host sync
    if (bytes != 0 && (dst == nullptr || src == nullptr)) return hipErrorInvalidValue;
    host_op("hipMemcpy", {fake::reads(src, bytes), fake::writes(dst, bytes)});
    return hipSuccess;
}

// ------------------------------------------------------------------------------- include/dccl/dccl_reduce.h
int dccl_local_reduce(const void* send, void* recv, int dtype, size_t count, int, void* stream) {
    const size_t esz = esz_of(dtype);
    if (esz == 0) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (send == nullptr || recv == nullptr) return DCCL_INVALID_ARGUMENT;
    op("dccl_local_reduce", stream, {fake::reads(send, count * esz), fake::writes(recv, count * esz)});
    return DCCL_SUCCESS;
}

int dccl_local_reduce_chain(const void* const* sends, int nsend, const void* own, void* dst, int dtype, size_t count,
                            int, void* stream) {
    return chain_op("dccl_local_reduce_chain", sends, nsend, own, dst, dtype, count, esz_of(dtype), {}, stream);
}

int dccl_local_reduce_chain_premul(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                   size_t count, const void* scalar, int residence, void* stream) {
    std::vector<hb::Range> ranges;
    if (!scalar_arg(scalar, residence, esz_of(dtype), &ranges)) return DCCL_INVALID_ARGUMENT;
    return chain_op("dccl_local_reduce_chain_premul", sends, nsend, own, dst, dtype, count, esz_of(dtype),
                    std::move(ranges), stream);
}

int dccl_local_reduce_chain_wide(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                 size_t count, void* stream) {
    if (dtype != 6 && dtype != 9) return DCCL_INVALID_ARGUMENT;
    return chain_op("dccl_local_reduce_chain_wide", sends, nsend, own, dst, dtype, count, 2, {}, stream);
}

int dccl_local_reduce_chain_wide_scaled(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                        size_t count, const void* scalar, int residence, void* stream) {
    std::vector<hb::Range> ranges;
    if ((dtype != 6 && dtype != 9) || !scalar_arg(scalar, residence, sizeof(float), &ranges))
        return DCCL_INVALID_ARGUMENT;
    return chain_op("dccl_local_reduce_chain_wide_scaled", sends, nsend, own, dst, dtype, count, 2, std::move(ranges),
                    stream);
}

// accumulate == 1 also reads dst; dst is a write either way (see the file comment)
int dccl_local_reduce_chain_widen(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                  size_t count, int accumulate, void* stream) {
    if ((dtype != 6 && dtype != 9) || (accumulate != 0 && accumulate != 1)) return DCCL_INVALID_ARGUMENT;
    return chain_op("dccl_local_reduce_chain_widen", sends, nsend, own, dst, dtype, count, sizeof(float), {}, stream);
}

int dccl_local_convert(const void* src, int src_dtype, void* dst, int dst_dtype, size_t count, void* stream) {
    const bool widen = (src_dtype == 6 || src_dtype == 9) && dst_dtype == 7;
    const bool narrow = src_dtype == 7 && (dst_dtype == 6 || dst_dtype == 9);
    if (!widen && !narrow) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (src == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    op("dccl_local_convert", stream,
       {fake::reads(src, count * esz_of(src_dtype)), fake::writes(dst, count * esz_of(dst_dtype))});
    return DCCL_SUCCESS;
}

int dccl_local_convert_scaled(const void* src, int src_dtype, void* dst, int dst_dtype, size_t count,
                              const void* scalar, int residence, void* stream) {
    const bool narrow = src_dtype == 7 && (dst_dtype == 6 || dst_dtype == 9);
    const bool same = (src_dtype == 6 || src_dtype == 9) && dst_dtype == src_dtype;
    std::vector<hb::Range> ranges;
    if ((!narrow && !same) || !scalar_arg(scalar, residence, sizeof(float), &ranges)) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (src == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    ranges.push_back(fake::reads(src, count * esz_of(src_dtype)));
    ranges.push_back(fake::writes(dst, count * esz_of(dst_dtype)));
    op("dccl_local_convert_scaled", stream, std::move(ranges));
    return DCCL_SUCCESS;
}

int dccl_local_scale(const void* src, void* dst, int dtype, size_t count, const void* scalar, int residence,
                     void* stream) {
    const size_t esz = esz_of(dtype);
    std::vector<hb::Range> ranges;
    if (esz == 0 || !scalar_arg(scalar, residence, esz, &ranges)) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (src == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    ranges.push_back(fake::reads(src, count * esz));
    ranges.push_back(fake::writes(dst, count * esz));
    op("dccl_local_scale", stream, std::move(ranges));
    return DCCL_SUCCESS;
}

int dccl_copy_multi(const void* const* srcs, void* const* dsts, int npairs, size_t bytes, void* stream) {
    if (npairs < 0 || npairs > 8 || (npairs > 0 && (srcs == nullptr || dsts == nullptr))) return DCCL_INVALID_ARGUMENT;
    std::vector<hb::Range> ranges;
    for (int y = 0; y < npairs && bytes > 0; ++y) {
        if (srcs[y] == nullptr || dsts[y] == nullptr) return DCCL_INVALID_ARGUMENT;
        ranges.push_back(fake::reads(srcs[y], bytes));
        ranges.push_back(fake::writes(dsts[y], bytes));
    }
    if (!ranges.empty()) op("dccl_copy_multi", stream, std::move(ranges));
    return DCCL_SUCCESS;
}

int dccl_local_reduce_host(const void* send, void* recv, int dtype, size_t count, int) {
    const size_t esz = esz_of(dtype);
    if (esz == 0) return DCCL_INVALID_ARGUMENT;
    if (count != 0) host_op("dccl_local_reduce_host", {fake::reads(send, count * esz), fake::writes(recv, count * esz)});
    return DCCL_SUCCESS;
}

int dccl_local_reduce_chain_host(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                 size_t count, int) {
    const size_t esz = esz_of(dtype);
    if (esz == 0 || nsend < 1 || nsend > 8 || sends == nullptr) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    std::vector<hb::Range> ranges{fake::reads(own, count * esz), fake::writes(dst, count * esz)};
    for (int j = 0; j < nsend; ++j) ranges.push_back(fake::reads(sends[j], count * esz));
    host_op("dccl_local_reduce_chain_host", std::move(ranges));
    return DCCL_SUCCESS;
}

}  // extern "C"

namespace dccl_amd {
int copy_rows_launch(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, hipStream_t stream) {
    return rows_op("copy_rows_launch", segs, nsegs, rows, stream);
}
int add_rows_launch(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, hipStream_t stream) {
    return rows_op("add_rows_launch", segs, nsegs, rows, stream);  // dst is read and written: a write
}
}  // namespace dccl_amd
