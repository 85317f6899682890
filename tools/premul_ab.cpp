// tools/premul_ab.cpp — A/B of the pre-multiplied-sum kernels against what they replace (a driver, not a test;
// DESIGN.md §7.5, profiles/premul_ab.json):
//   chain  dccl_local_reduce_chain (Sum, the unchanged baseline) and dccl_local_reduce_chain_premul alternate in
//          one process on the same buffers: k = 1 and 7 sources, fp32 and bf16, 64 MiB per operand, a separate
//          dst, so both move (k + 2) N bytes;
//   scale  hipMemcpyAsync device-to-device (the baseline: the copy the ring paths replace) and dccl_local_scale
//          out of place alternate at the same size (2 N bytes).
// Every case: warm-up, then ROUNDS rounds of [PER baseline launches | PER new launches], each batch between two
// device events (ROUNDS * PER = 240 timed launches per side).  One JSON line per case: the median round of each
// side, and the baseline's own spread over its rounds (min, max), which is the noise a difference must exceed.
//   hipcc -std=c++17 -O2 -I include tools/premul_ab.cpp -o tools/bin/premul_ab -L dccl_amd/lib -ldccl_amd \
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
    unsigned char* buf[10];  // 8 sources / own, dst, and one more for the scale's source
    for (auto& b : buf) {
        CK(hipMalloc(reinterpret_cast<void**>(&b), kBytes));
        CK(hipMemset(b, 0x3c, kBytes));  // fp32 0x3c3c3c3c and bf16 0x3c3c: about 0.0115, finite sums
    }
    CK(hipDeviceSynchronize());
    const float s32 = 0.5f;
    const uint16_t sbf = 0x3f00;  // bf16 0.5
    struct { int dtype; const char* name; size_t esz; const void* scalar; } types[] = {
        {7, "fp32", 4, &s32}, {9, "bf16", 2, &sbf}};
    for (const auto& t : types) {
        const size_t n = kBytes / t.esz;
        for (int k : {1, 7}) {
            const void* sends[8];
            for (int j = 0; j < k; ++j) sends[j] = buf[j];
            const void* own = buf[7];
            void* dst = buf[8];
            Stat plain, pre;
            ab(st, [&] { return dccl_local_reduce_chain(sends, k, own, dst, t.dtype, n, 0, st); },
               [&] { return dccl_local_reduce_chain_premul(sends, k, own, dst, t.dtype, n, t.scalar, 1, st); }, &plain,
               &pre);
            const double gb = double(k + 2) * kBytes / 1e9;
            printf("{\"case\": \"chain\", \"dtype\": \"%s\", \"k\": %d, \"bytes_per_operand\": %zu, "
                   "\"plain_us\": %.1f, \"plain_us_min\": %.1f, \"plain_us_max\": %.1f, \"plain_gb_s\": %.0f, "
                   "\"premul_us\": %.1f, \"premul_us_min\": %.1f, \"premul_us_max\": %.1f, \"premul_gb_s\": %.0f}\n",
                   t.name, k, kBytes, plain.med, plain.lo, plain.hi, gb / (plain.med * 1e-6), pre.med, pre.lo, pre.hi,
                   gb / (pre.med * 1e-6));
            fflush(stdout);
        }
        Stat cp, sc;
        ab(st, [&] { return hipMemcpyAsync(buf[8], buf[9], kBytes, hipMemcpyDeviceToDevice, st) == hipSuccess ? 0 : 1; },
           [&] { return dccl_local_scale(buf[9], buf[8], t.dtype, n, t.scalar, 1, st); }, &cp, &sc);
        const double gb = 2.0 * kBytes / 1e9;
        printf("{\"case\": \"scale\", \"dtype\": \"%s\", \"bytes_per_operand\": %zu, "
               "\"memcpy_us\": %.1f, \"memcpy_us_min\": %.1f, \"memcpy_us_max\": %.1f, \"memcpy_gb_s\": %.0f, "
               "\"scale_us\": %.1f, \"scale_us_min\": %.1f, \"scale_us_max\": %.1f, \"scale_gb_s\": %.0f}\n",
               t.name, kBytes, cp.med, cp.lo, cp.hi, gb / (cp.med * 1e-6), sc.med, sc.lo, sc.hi, gb / (sc.med * 1e-6));
        fflush(stdout);
    }
    return 0;
}
