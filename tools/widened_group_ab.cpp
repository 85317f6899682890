// tools/widened_group_ab.cpp — groups of widened reduce-scatters, timed on the public API (a driver, not a test;
// DESIGN.md §7.11, profiles/widened_group_ab.json).  The source uses nothing newer than dcclRedOpCreateWidenedSum and
// ncclGroupStart / ncclGroupEnd, so the same file links against the library of this tree (arm A: same-handle widened
// calls of a group are coalesced) and against the library of the commit before it (arm B: they run one by one at
// ncclGroupEnd); tools/widened_group_ab.py alternates the two binaries and folds their lines into the profile.
//
// W = 4 thread ranks on one GPU, the default (direct) path, bf16: 16 ncclReduceScatter calls with one widened handle
// per group, per-tensor 16-bit payload (count * 2 bytes of the whole reduced buffer) 4 KiB .. 16 MiB, accumulate 0 and
// 1.  DCCL_GROUP_COALESCE_MAX_BYTES is set to 1 GiB so that every size is packed where the library packs widened calls
// at all; DCCL_GROUP_COALESCE=0 in the environment still turns packing off (arm A-off).  Per case: warm-up groups,
// then timed groups; a group's time is the slowest rank's wall time from a barrier ahead of ncclGroupStart to the
// return of hipStreamSynchronize after ncclGroupEnd.  One JSON line per case: median, min and max us per group and a
// hash of every rank's outputs of one more group run on zeroed recvbuffs (the arms must agree on it).
//
// The kernel (report only): dccl_add_rows_f32_multi over 16 segments of one 1 MiB row against dccl_local_reduce fp32
// Sum on one 16 MiB pair, the same 3 N bytes, alternated, device events.  The entry point is looked up at run time:
// arm B's library has none and prints no kernel line.
//   hipcc -std=c++17 -O2 -I include tools/widened_group_ab.cpp -o BIN -L LIBDIR -ldccl_amd -Wl,-rpath,LIBDIR -pthread -ldl
#include <dlfcn.h>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "dccl/dccl.hpp"
#include "dccl/dccl_reduce.h"

#define CK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed line %d\n", #x, __LINE__); exit(1); } } while (0)
#define NK(x) do { if ((x) != dccl::ncclSuccess) { fprintf(stderr, "%s failed line %d\n", #x, __LINE__); exit(1); } } while (0)

namespace {
using namespace dccl;
constexpr int kW = 4, kTensors = 16;

struct Stat { double med, lo, hi; };
Stat stat(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return {v[v.size() / 2], v.front(), v.back()};
}

// A sense-reversing spin barrier of the kW rank threads.
struct Barrier {
    std::atomic<int> count{0}, gen{0};
    void wait() {
        const int g = gen.load();
        if (count.fetch_add(1) + 1 == kW) {
            count.store(0);
            gen.fetch_add(1);
        } else {
            while (gen.load() == g) std::this_thread::yield();
        }
    }
};

uint64_t fnv(uint64_t h, const unsigned char* p, size_t n) {
    for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 1099511628211ull;
    return h;
}

struct Case { size_t payload; int acc, warm, iters; };

Barrier g_bar;
std::vector<double> g_times[kW];
uint64_t g_hash[kW];

void rank_main(int r, const std::vector<Case>* cases) {
    CK(hipSetDevice(0));
    ncclComm_t comm = nullptr;
    NK(dcclCommInitRank(&comm, kW, r));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    for (size_t ci = 0; ci < cases->size(); ++ci) {
        const Case& c = (*cases)[ci];
        const size_t count = c.payload / 2, recvcount = count / kW;
        ncclRedOp_t op;
        NK(dcclRedOpCreateWidenedSum(&op, ncclBfloat16, c.acc, comm));
        unsigned char *send = nullptr, *recv = nullptr;
        CK(hipMalloc(reinterpret_cast<void**>(&send), kTensors * c.payload));
        CK(hipMalloc(reinterpret_cast<void**>(&recv), kTensors * recvcount * 4));
        {  // bf16 values in [2^-7, 2^-5): finite sums however often they accumulate here
            std::vector<uint16_t> h(kTensors * count);
            uint32_t x = 12345u + 977u * r + 31u * uint32_t(ci);
            for (auto& v : h) x = x * 1664525u + 1013904223u, v = uint16_t(0x3C00u + ((x >> 12) & 0x0FFu));
            CK(hipMemcpy(send, h.data(), h.size() * 2, hipMemcpyHostToDevice));
        }
        CK(hipMemset(recv, 0, kTensors * recvcount * 4));
        CK(hipDeviceSynchronize());
        auto group = [&] {
            NK(ncclGroupStart());
            for (int t = 0; t < kTensors; ++t)
                NK(ncclReduceScatter(send + t * c.payload, recv + t * recvcount * 4, recvcount, ncclBfloat16, op, comm, st));
            NK(ncclGroupEnd());
            CK(hipStreamSynchronize(st));
        };
        g_times[r].clear();
        for (int i = 0; i < c.warm + c.iters; ++i) {
            g_bar.wait();
            const auto t0 = std::chrono::steady_clock::now();
            group();
            const auto t1 = std::chrono::steady_clock::now();
            if (i >= c.warm) g_times[r].push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
        }
        CK(hipMemset(recv, 0, kTensors * recvcount * 4));
        CK(hipDeviceSynchronize());
        g_bar.wait();
        group();
        std::vector<unsigned char> out(kTensors * recvcount * 4);
        CK(hipMemcpy(out.data(), recv, out.size(), hipMemcpyDeviceToHost));
        g_hash[r] = fnv(1469598103934665603ull, out.data(), out.size());
        g_bar.wait();
        if (r == 0) {
            std::vector<double> slowest(c.iters, 0.0);
            uint64_t h = 1469598103934665603ull;
            for (int q = 0; q < kW; ++q) {
                for (int i = 0; i < c.iters; ++i) slowest[i] = std::max(slowest[i], g_times[q][i]);
                h = fnv(h, reinterpret_cast<const unsigned char*>(&g_hash[q]), 8);
            }
            const Stat s = stat(slowest);
            printf("{\"case\": \"group\", \"payload_bytes\": %zu, \"accumulate\": %d, \"groups_timed\": %d, "
                   "\"us\": %.1f, \"us_min\": %.1f, \"us_max\": %.1f, \"hash\": \"%016llx\"}\n",
                   c.payload, c.acc, c.iters, s.med, s.lo, s.hi, static_cast<unsigned long long>(h));
            fflush(stdout);
        }
        g_bar.wait();
        CK(hipFree(send));
        CK(hipFree(recv));
        NK(ncclRedOpDestroy(op, comm));
    }
    CK(hipStreamDestroy(st));
    NK(ncclCommFinalize(comm));
}

void kernel_ab() {
    typedef int (*add_rows_fn)(const dccl_copy_rows_t*, int, uint32_t, void*);
    const auto add_rows = reinterpret_cast<add_rows_fn>(dlsym(RTLD_DEFAULT, "dccl_add_rows_f32_multi"));
    if (add_rows == nullptr) return;
    constexpr size_t kSeg = size_t(1) << 20, kAll = 16 * kSeg;
    constexpr int kRounds = 12, kPer = 20, kWarm = 10;
    hipStream_t st;
    CK(hipStreamCreate(&st));
    unsigned char *src = nullptr, *dst = nullptr;
    CK(hipMalloc(reinterpret_cast<void**>(&src), kAll));
    CK(hipMalloc(reinterpret_cast<void**>(&dst), kAll));
    CK(hipMemset(src, 0, kAll));  // 0.0f + 0.0f: finite for any number of repetitions
    CK(hipMemset(dst, 0, kAll));
    dccl_copy_rows_t segs[16];
    for (int i = 0; i < 16; ++i) segs[i] = {src + i * kSeg, dst + i * kSeg, kSeg, kSeg, kSeg};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto batch = [&](bool rows, int n) {
        CK(hipEventRecord(e0, st));
        for (int i = 0; i < n; ++i)
            if ((rows ? add_rows(segs, 16, 1, st) : dccl_local_reduce(src, dst, 7, kAll / 4, 0, st)) != 0) exit(2);
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        return double(ms) * 1e3 / n;
    };
    batch(true, kWarm), batch(false, kWarm);
    std::vector<double> a, b;
    for (int r = 0; r < kRounds; ++r) a.push_back(batch(true, kPer)), b.push_back(batch(false, kPer));
    const Stat sa = stat(a), sb = stat(b);
    const double gb = 3.0 * kAll / 1e9;
    printf("{\"case\": \"kernel\", \"bytes_moved\": %zu, \"add_rows_us\": %.1f, \"add_rows_us_min\": %.1f, "
           "\"add_rows_us_max\": %.1f, \"add_rows_gb_s\": %.0f, \"local_reduce_us\": %.1f, \"local_reduce_us_min\": %.1f, "
           "\"local_reduce_us_max\": %.1f, \"local_reduce_gb_s\": %.0f}\n",
           3 * kAll, sa.med, sa.lo, sa.hi, gb / (sa.med * 1e-6), sb.med, sb.lo, sb.hi, gb / (sb.med * 1e-6));
    fflush(stdout);
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    CK(hipFree(src));
    CK(hipFree(dst));
    CK(hipStreamDestroy(st));
}
}  // namespace

int main() {
    setenv("DCCL_GROUP_COALESCE_MAX_BYTES", "1073741824", 1);
    std::vector<Case> cases;
    for (size_t kib : {4, 64, 256, 1024, 4096, 16384})
        for (int acc : {0, 1}) cases.push_back({kib << 10, acc, 5, kib >= 4096 ? 15 : 40});
    std::vector<std::thread> th;
    for (int r = 0; r < kW; ++r) th.emplace_back(rank_main, r, &cases);
    for (auto& t : th) t.join();
    kernel_ab();
    return 0;
}
