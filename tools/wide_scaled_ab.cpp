// tools/wide_scaled_ab.cpp — A/B of the scaled wide-sum kernels against the wide-sum kernels they extend (a driver,
// not a test; DESIGN.md §7.8, profiles/wide_scaled_ab.json), with tools/wide_ab.cpp's method:
//   chain    dccl_local_reduce_chain_wide (unchanged code: the yardstick) and dccl_local_reduce_chain_wide_scaled
//            alternate in one process on the same buffers: k = 1, 3 and 7 sources, bf16 and fp16, 64 MiB per operand,
//            a separate dst, the scalar host-immediate; bf16 k = 7 once more with the scalar in device memory.  Both
//            sides move (k + 2) N bytes; the scaled side adds four packed multiplies per lane and tile.
//   narrow   dccl_local_convert (fp32 -> 16 bits) and dccl_local_convert_scaled on §7.7's shape: 128 MiB moved
//            (two thirds read as fp32, one third written).
// Every case: warm-up, then ROUNDS rounds of [PER baseline launches | PER new launches], each batch between two
// device events (ROUNDS * PER = 240 timed launches per side).  One JSON line per case: the median round of each
// side with its spread over the rounds (min, max), and whether the new side's median lies inside the baseline's
// [min, max] band widened by 2 %.
//   hipcc -std=c++17 -O2 -I include tools/wide_scaled_ab.cpp -o tools/bin/wide_scaled_ab -L dccl_amd/lib \
//         -ldccl_amd -Wl,-rpath,$PWD/dccl_amd/lib
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

bool in_band(const Stat& base, const Stat& mine) { return mine.med >= base.lo * 0.98 && mine.med <= base.hi * 1.02; }
}  // namespace

int main() {
    hipStream_t st;
    CK(hipStreamCreate(&st));
    unsigned char* buf[10];  // 8 sources / own, dst, and one more (the conversion's fp32 side spans buf 8 and 9)
    unsigned char* all = nullptr;
    CK(hipMalloc(reinterpret_cast<void**>(&all), 10 * kBytes));
    CK(hipMemset(all, 0x3c, 10 * kBytes));  // bf16 0x3c3c about 0.0115, fp16 0x3c3c about 1.06, fp32 0.0115: finite sums
    for (int i = 0; i < 10; ++i) buf[i] = all + size_t(i) * kBytes;
    const float s = 0.3f;
    float* dev_s = nullptr;
    CK(hipMalloc(reinterpret_cast<void**>(&dev_s), sizeof(float)));
    CK(hipMemcpy(dev_s, &s, sizeof(float), hipMemcpyHostToDevice));
    CK(hipDeviceSynchronize());
    struct { int dtype; const char* name; } types[] = {{9, "bf16"}, {6, "fp16"}};
    struct { int k; int residence; } chains[] = {{1, 1}, {3, 1}, {7, 1}, {7, 0}};
    for (const auto& t : types) {
        const size_t n = kBytes / 2;
        for (const auto& c : chains) {
            if (c.residence == 0 && t.dtype != 9) continue;
            const int k = c.k;
            const void* sends[8];
            for (int j = 0; j < k; ++j) sends[j] = buf[j];
            const void* own = buf[7];
            void* dst = buf[8];
            const void* scalar = c.residence == 0 ? static_cast<const void*>(dev_s) : &s;
            Stat wide, scaled;
            ab(st, [&] { return dccl_local_reduce_chain_wide(sends, k, own, dst, t.dtype, n, st); },
               [&] {
                   return dccl_local_reduce_chain_wide_scaled(sends, k, own, dst, t.dtype, n, scalar, c.residence, st);
               },
               &wide, &scaled);
            const double gb = double(k + 2) * kBytes / 1e9;
            printf("{\"case\": \"chain\", \"dtype\": \"%s\", \"k\": %d, \"scalar\": \"%s\", "
                   "\"bytes_per_operand\": %zu, "
                   "\"wide_us\": %.1f, \"wide_us_min\": %.1f, \"wide_us_max\": %.1f, \"wide_gb_s\": %.0f, "
                   "\"scaled_us\": %.1f, \"scaled_us_min\": %.1f, \"scaled_us_max\": %.1f, \"scaled_gb_s\": %.0f, "
                   "\"scaled_median_in_wide_band_2pct\": %s}\n",
                   t.name, k, c.residence == 0 ? "device" : "host", kBytes, wide.med, wide.lo, wide.hi,
                   gb / (wide.med * 1e-6), scaled.med, scaled.lo, scaled.hi, gb / (scaled.med * 1e-6),
                   in_band(wide, scaled) ? "true" : "false");
            fflush(stdout);
        }
        // 16-bit side in buf[0] (two thirds of 64 MiB), fp32 side in buf[8..9]: 128 MiB moved
        const size_t nc = kBytes * 2 / 3 / 2 / 8 * 8;
        Stat cv, cs;
        ab(st, [&] { return dccl_local_convert(buf[8], 7, buf[0], t.dtype, nc, st); },
           [&] { return dccl_local_convert_scaled(buf[8], 7, buf[0], t.dtype, nc, &s, 1, st); }, &cv, &cs);
        const double gbc = 6.0 * nc / 1e9;
        printf("{\"case\": \"narrow\", \"dtype\": \"%s\", \"elements\": %zu, "
               "\"convert_us\": %.1f, \"convert_us_min\": %.1f, \"convert_us_max\": %.1f, \"convert_gb_s\": %.0f, "
               "\"scaled_us\": %.1f, \"scaled_us_min\": %.1f, \"scaled_us_max\": %.1f, \"scaled_gb_s\": %.0f, "
               "\"scaled_median_in_convert_band_2pct\": %s}\n",
               t.name, nc, cv.med, cv.lo, cv.hi, gbc / (cv.med * 1e-6), cs.med, cs.lo, cs.hi, gbc / (cs.med * 1e-6),
               in_band(cv, cs) ? "true" : "false");
        fflush(stdout);
    }
    return 0;
}
