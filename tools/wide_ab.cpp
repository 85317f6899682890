// tools/wide_ab.cpp — A/B of the wide-sum kernels against what they stand next to (a driver, not a test;
// DESIGN.md §7.7, profiles/wide_ab.json):
//   chain    dccl_local_reduce_chain (Sum, the unchanged baseline: rounds after every add) and
//            dccl_local_reduce_chain_wide alternate in one process on the same buffers: k = 1, 3 and 7 sources,
//            bf16 and fp16, 64 MiB per operand, a separate dst, so both move (k + 2) N bytes;
//   convert  hipMemcpyAsync device-to-device of the same total bytes (64 MiB read and 64 MiB written) and
//            dccl_local_convert alternate: widening reads 64 MiB / 1.5 of 16-bit elements and writes twice that,
//            narrowing the mirror image, so each side moves 128 MiB.  Reported only.
// Every case: warm-up, then ROUNDS rounds of [PER baseline launches | PER new launches], each batch between two
// device events (ROUNDS * PER = 240 timed launches per side).  One JSON line per case: the median round of each
// side with its spread over the rounds (min, max); the baseline's spread is the noise a difference must exceed.
//   hipcc -std=c++17 -O2 -I include tools/wide_ab.cpp -o tools/bin/wide_ab -L dccl_amd/lib -ldccl_amd \
//         -Wl,-rpath,$PWD/dccl_amd/lib
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <vector>

#include "dccl/dccl_reduce.h"

#define CK(x) do { if ((x) != hipSuccess) { fprintf(stderr, "%s failed line %d\n", #x, __LINE__); exit(1); } } while (0)

namespace {
constexpr size_t kBytes = size_t(64) << 20;
constexpr int kRounds = 12, kPer = 20, kWarm = 10;

struct Stat { double med, lo, hi; };

Stat stat(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return {v[v.size() / 2], v.front(), v.back()};
}

// us per launch of `a` and `b`, alternated round by round
void ab(hipStream_t st, const std::function<int()>& a, const std::function<int()>& b, Stat* sa, Stat* sb) {
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
    batch(a, kWarm);
    batch(b, kWarm);
    std::vector<double> ta, tb;
    for (int r = 0; r < kRounds; ++r) {
        ta.push_back(batch(a, kPer));
        tb.push_back(batch(b, kPer));
    }
    *sa = stat(ta);
    *sb = stat(tb);
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
}
}  // namespace

int main() {
    hipStream_t st;
    CK(hipStreamCreate(&st));
    unsigned char* buf[10];  // 8 sources / own, dst, and one more (the conversion's fp32 side spans buf 8 and 9)
    unsigned char* all = nullptr;
    CK(hipMalloc(reinterpret_cast<void**>(&all), 10 * kBytes));
    CK(hipMemset(all, 0x3c, 10 * kBytes));  // bf16 0x3c3c about 0.0115, fp16 0x3c3c about 1.06, fp32 0.0115: finite sums
    for (int i = 0; i < 10; ++i) buf[i] = all + size_t(i) * kBytes;
    CK(hipDeviceSynchronize());
    struct { int dtype; const char* name; } types[] = {{9, "bf16"}, {6, "fp16"}};
    for (const auto& t : types) {
        const size_t n = kBytes / 2;
        for (int k : {1, 3, 7}) {
            const void* sends[8];
            for (int j = 0; j < k; ++j) sends[j] = buf[j];
            const void* own = buf[7];
            void* dst = buf[8];
            Stat plain, wide;
            ab(st, [&] { return dccl_local_reduce_chain(sends, k, own, dst, t.dtype, n, 0, st); },
               [&] { return dccl_local_reduce_chain_wide(sends, k, own, dst, t.dtype, n, st); }, &plain, &wide);
            const double gb = double(k + 2) * kBytes / 1e9;
            printf("{\"case\": \"chain\", \"dtype\": \"%s\", \"k\": %d, \"bytes_per_operand\": %zu, "
                   "\"plain_us\": %.1f, \"plain_us_min\": %.1f, \"plain_us_max\": %.1f, \"plain_gb_s\": %.0f, "
                   "\"wide_us\": %.1f, \"wide_us_min\": %.1f, \"wide_us_max\": %.1f, \"wide_gb_s\": %.0f}\n",
                   t.name, k, kBytes, plain.med, plain.lo, plain.hi, gb / (plain.med * 1e-6), wide.med, wide.lo, wide.hi,
                   gb / (wide.med * 1e-6));
            fflush(stdout);
        }
        // 16-bit side in buf[0] (two thirds of 64 MiB), fp32 side in buf[8..9]: 128 MiB moved, as the copy's 2 x 64 MiB
        const size_t nc = kBytes * 2 / 3 / 2 / 8 * 8;
        for (int widen : {1, 0}) {
            Stat cp, cv;
            ab(st, [&] { return hipMemcpyAsync(buf[8], buf[7], kBytes, hipMemcpyDeviceToDevice, st) == hipSuccess ? 0 : 1; },
               [&] {
                   return widen ? dccl_local_convert(buf[0], t.dtype, buf[8], 7, nc, st)
                                : dccl_local_convert(buf[8], 7, buf[0], t.dtype, nc, st);
               },
               &cp, &cv);
            const double gb = 2.0 * kBytes / 1e9, gbc = 6.0 * nc / 1e9;
            printf("{\"case\": \"convert\", \"dtype\": \"%s\", \"direction\": \"%s\", \"elements\": %zu, "
                   "\"memcpy_us\": %.1f, \"memcpy_us_min\": %.1f, \"memcpy_us_max\": %.1f, \"memcpy_gb_s\": %.0f, "
                   "\"convert_us\": %.1f, \"convert_us_min\": %.1f, \"convert_us_max\": %.1f, \"convert_gb_s\": %.0f}\n",
                   t.name, widen ? "widen" : "narrow", nc, cp.med, cp.lo, cp.hi, gb / (cp.med * 1e-6), cv.med, cv.lo,
                   cv.hi, gbc / (cv.med * 1e-6));
            fflush(stdout);
        }
    }
    return 0;
}
