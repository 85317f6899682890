// tools/widen_checked_ab.cpp — what the non-finite flag of the checked widened sum costs (a driver, not a test;
// DESIGN.md §7.12, profiles/widen_checked_ab.json).
//
// Chain (default): tools/widen_ab.cpp's sizes and protocol.  Three arms alternate in one process on the same buffers:
// k = 1, 3 and 7 sources, bf16 and fp16, accumulate 0 and 1, 64 MiB of 16-bit elements per operand (N = 32 Mi):
//   A  unchecked   dccl_local_reduce_chain_widen, whose kernels are the parent commit's;
//   B  checked     dccl_local_reduce_chain_widen_checked: the same launch, the same bytes, the flag from registers;
//   C  two passes  A followed by dccl_local_nonfinite_f32 over dst (4N more bytes read): the only way to the flag
//                  before B existed.
// Every case: warm-up, then ROUNDS rounds of [PER A | PER B | PER C], each batch between two device events.  One JSON
// line per case: each arm's median round with its spread over the rounds (min, max); b_over_a with `margin`, twice the
// larger of the two arms' own (max - min) / median, and `b_within_margin`; c_over_b (reported, not judged).  The
// inputs are finite, so no arm ever stores to the flag; it is read back at the end and must still be 0.
//
// Group (`widen_checked_ab group`): tools/widened_group_ab.cpp's method.  W = 4 thread ranks on one GPU, the direct
// path, bf16, groups of 16 ncclReduceScatter calls with one handle, recvcounts of payload / 8 + 3 elements so that
// every packed slot ends in pad bytes; the unchecked and the checked handle alternate group by group.  A group's time
// is the slowest rank's wall time from a barrier ahead of ncclGroupStart to the return of hipStreamSynchronize.  The
// difference is the checked run's W pad memsets plus the check inside the chain.
//   hipcc -std=c++17 -O2 -I include tools/widen_checked_ab.cpp -o tools/bin/widen_checked_ab -L dccl_amd/lib \
//         -ldccl_amd -Wl,-rpath,$PWD/dccl_amd/lib -pthread
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#include "dccl/dccl.hpp"
#include "dccl/dccl_reduce.h"

#define CK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed line %d\n", #x, __LINE__); exit(1); } } while (0)
#define NK(x) do { if ((x) != dccl::ncclSuccess) { fprintf(stderr, "%s failed line %d\n", #x, __LINE__); exit(1); } } while (0)

namespace {
constexpr size_t kBytes = size_t(64) << 20;  // of 16-bit elements per operand
constexpr int kRounds = 12, kPer = 20, kWarm = 10;
constexpr int kArms = 3;

struct Stat { double med, lo, hi; };

Stat stat(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return {v[v.size() / 2], v.front(), v.back()};
}

double spread(const Stat& s) { return (s.hi - s.lo) / s.med; }

// us per repetition of each arm, alternated round by round
void abc(hipStream_t st, const std::function<int()> (&arm)[kArms], Stat (&out)[kArms]) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    auto batch = [&](const std::function<int()>& f, int n) {
        CK(hipEventRecord(e0, st));
        for (int i = 0; i < n; ++i)
            if (f() != 0) { fprintf(stderr, "launch failed\n"); exit(2); }
        CK(hipEventRecord(e1, st));
        CK(hipEventSynchronize(e1));
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        return double(ms) * 1e3 / n;
    };
    for (const auto& f : arm) batch(f, kWarm);
    std::vector<double> t[kArms];
    for (int r = 0; r < kRounds; ++r)
        for (int a = 0; a < kArms; ++a) t[a].push_back(batch(arm[a], kPer));
    for (int a = 0; a < kArms; ++a) out[a] = stat(t[a]);
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
}

int chain_main() {
    hipStream_t st;
    CK(hipStreamCreate(&st));
    unsigned char *half = nullptr, *full = nullptr;
    uint32_t* flag = nullptr;
    CK(hipMalloc(reinterpret_cast<void**>(&half), 8 * kBytes));
    CK(hipMalloc(reinterpret_cast<void**>(&full), 2 * kBytes));
    CK(hipMalloc(reinterpret_cast<void**>(&flag), 256));
    CK(hipMemset(half, 0x3c, 8 * kBytes));  // bf16 0x3c3c about 0.0115, fp16 0x3c3c about 1.06: finite sums
    CK(hipMemset(full, 0, 2 * kBytes));     // dst starts at 0.0f and stays finite under accumulate
    CK(hipMemset(flag, 0, 256));
    CK(hipDeviceSynchronize());
    const size_t n = kBytes / 2;
    auto h = [&](int i) { return half + size_t(i) * kBytes; };
    struct { int dtype; const char* name; } types[] = {{9, "bf16"}, {6, "fp16"}};
    for (const auto& t : types)
        for (int k : {1, 3, 7})
            for (int acc : {0, 1}) {
                const void* sends[8];
                for (int j = 0; j < k; ++j) sends[j] = h(j);
                const void* own = h(7);
                void* dst = full;
                const std::function<int()> arm[kArms] = {
                    [&] { return dccl_local_reduce_chain_widen(sends, k, own, dst, t.dtype, n, acc, st); },
                    [&] { return dccl_local_reduce_chain_widen_checked(sends, k, own, dst, t.dtype, n, acc, flag, st); },
                    [&] {
                        const int rc = dccl_local_reduce_chain_widen(sends, k, own, dst, t.dtype, n, acc, st);
                        return rc != 0 ? rc : dccl_local_nonfinite_f32(dst, n, flag, st);
                    },
                };
                Stat s[kArms];
                abc(st, arm, s);
                const double gb = (double(k + 1) * 2 + (acc ? 8 : 4)) * n / 1e9;
                const double margin = 2 * std::max(spread(s[0]), spread(s[1]));
                const double b_over_a = s[1].med / s[0].med;
                printf("{\"case\": \"chain\", \"dtype\": \"%s\", \"k\": %d, \"accumulate\": %d, \"elements\": %zu, "
                       "\"a_us\": %.1f, \"a_us_min\": %.1f, \"a_us_max\": %.1f, \"a_gb_s\": %.0f, "
                       "\"b_us\": %.1f, \"b_us_min\": %.1f, \"b_us_max\": %.1f, \"b_gb_s\": %.0f, "
                       "\"c_us\": %.1f, \"c_us_min\": %.1f, \"c_us_max\": %.1f, "
                       "\"b_over_a\": %.4f, \"margin\": %.4f, \"b_within_margin\": %s, \"c_over_b\": %.3f}\n",
                       t.name, k, acc, n, s[0].med, s[0].lo, s[0].hi, gb / (s[0].med * 1e-6), s[1].med, s[1].lo,
                       s[1].hi, gb / (s[1].med * 1e-6), s[2].med, s[2].lo, s[2].hi, b_over_a, margin,
                       b_over_a <= 1 + margin ? "true" : "false", s[2].med / s[1].med);
                fflush(stdout);
            }
    uint32_t seen = 7;
    CK(hipMemcpy(&seen, flag, 4, hipMemcpyDeviceToHost));
    printf("{\"case\": \"flag\", \"value_after_all_arms\": %u}\n", seen);
    CK(hipFree(half));
    CK(hipFree(full));
    CK(hipFree(flag));
    return seen == 0 ? 0 : 3;
}

// ---- groups ----
using namespace dccl;
constexpr int kW = 4, kTensors = 16;

struct Barrier {  // sense-reversing, of the kW rank threads
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

struct Case { size_t payload; int acc, warm, iters; };

Barrier g_bar;
std::vector<double> g_times[2][kW];  // [unchecked, checked][rank]
uint32_t g_flag[kW];

void rank_main(int r, const std::vector<Case>* cases) {
    CK(hipSetDevice(0));
    ncclComm_t comm = nullptr;
    NK(dcclCommInitRank(&comm, kW, r));
    hipStream_t st;
    CK(hipStreamCreate(&st));
    uint32_t* flag = nullptr;
    CK(hipMalloc(reinterpret_cast<void**>(&flag), 256));
    CK(hipMemset(flag, 0, 256));
    for (size_t ci = 0; ci < cases->size(); ++ci) {
        const Case& c = (*cases)[ci];
        const size_t recvcount = c.payload / 2 / kW + 3, count = recvcount * kW;  // 2 (recvcount) bytes: no 128 multiple
        ncclRedOp_t ops[2];
        NK(dcclRedOpCreateWidenedSum(&ops[0], ncclBfloat16, c.acc, comm));
        NK(dcclRedOpCreateWidenedSumChecked(&ops[1], ncclBfloat16, c.acc, flag, comm));
        unsigned char *send = nullptr, *recv = nullptr;
        CK(hipMalloc(reinterpret_cast<void**>(&send), kTensors * count * 2));
        CK(hipMalloc(reinterpret_cast<void**>(&recv), kTensors * recvcount * 4));
        {  // bf16 values in [2^-7, 2^-5): finite sums however often they accumulate here
            std::vector<uint16_t> h(kTensors * count);
            uint32_t x = 12345u + 977u * r + 31u * uint32_t(ci);
            for (auto& v : h) x = x * 1664525u + 1013904223u, v = uint16_t(0x3C00u + ((x >> 12) & 0x0FFu));
            CK(hipMemcpy(send, h.data(), h.size() * 2, hipMemcpyHostToDevice));
        }
        CK(hipMemset(recv, 0, kTensors * recvcount * 4));
        CK(hipDeviceSynchronize());
        auto group = [&](ncclRedOp_t op) {
            NK(ncclGroupStart());
            for (int t = 0; t < kTensors; ++t)
                NK(ncclReduceScatter(send + t * count * 2, recv + t * recvcount * 4, recvcount, ncclBfloat16, op, comm, st));
            NK(ncclGroupEnd());
            CK(hipStreamSynchronize(st));
        };
        for (int a = 0; a < 2; ++a) g_times[a][r].clear();
        for (int i = 0; i < c.warm + c.iters; ++i)
            for (int a = 0; a < 2; ++a) {
                g_bar.wait();
                const auto t0 = std::chrono::steady_clock::now();
                group(ops[a]);
                const auto t1 = std::chrono::steady_clock::now();
                if (i >= c.warm) g_times[a][r].push_back(std::chrono::duration<double, std::micro>(t1 - t0).count());
            }
        CK(hipMemcpy(&g_flag[r], flag, 4, hipMemcpyDeviceToHost));
        g_bar.wait();
        if (r == 0) {
            Stat s[2];
            for (int a = 0; a < 2; ++a) {
                std::vector<double> slowest(c.iters, 0.0);
                for (int q = 0; q < kW; ++q)
                    for (int i = 0; i < c.iters; ++i) slowest[i] = std::max(slowest[i], g_times[a][q][i]);
                s[a] = stat(slowest);
            }
            uint32_t any = 0;
            for (int q = 0; q < kW; ++q) any |= g_flag[q];
            printf("{\"case\": \"group\", \"tensors\": %d, \"recvcount\": %zu, \"payload_bytes\": %zu, \"accumulate\": %d, "
                   "\"groups_timed\": %d, \"unchecked_us\": %.1f, \"unchecked_us_min\": %.1f, \"unchecked_us_max\": %.1f, "
                   "\"checked_us\": %.1f, \"checked_us_min\": %.1f, \"checked_us_max\": %.1f, "
                   "\"checked_minus_unchecked_us\": %.1f, \"flags\": %u}\n",
                   kTensors, recvcount, count * 2, c.acc, c.iters, s[0].med, s[0].lo, s[0].hi, s[1].med, s[1].lo, s[1].hi,
                   s[1].med - s[0].med, any);
            fflush(stdout);
        }
        g_bar.wait();
        CK(hipFree(send));
        CK(hipFree(recv));
        NK(ncclRedOpDestroy(ops[0], comm));
        NK(ncclRedOpDestroy(ops[1], comm));
    }
    CK(hipFree(flag));
    CK(hipStreamDestroy(st));
    NK(ncclCommFinalize(comm));
}

int group_main() {
    setenv("DCCL_GROUP_COALESCE_MAX_BYTES", "1073741824", 1);
    std::vector<Case> cases;
    for (size_t kib : {4, 64, 1024})
        for (int acc : {0, 1}) cases.push_back({kib << 10, acc, 5, 40});
    std::vector<std::thread> th;
    for (int r = 0; r < kW; ++r) th.emplace_back(rank_main, r, &cases);
    for (auto& t : th) t.join();
    return 0;
}
}  // namespace

int main(int argc, char** argv) {
    return argc > 1 && std::strcmp(argv[1], "group") == 0 ? group_main() : chain_main();
}
