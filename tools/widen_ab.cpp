// tools/widen_ab.cpp — A/B of the widened chain against the only other route to its bits (a driver, not a test;
// DESIGN.md §7.10, profiles/widen_ab.json).  Three arms alternate in one process on the same buffers: k = 1, 3 and 7
// sources, bf16 and fp16, accumulate 0 and 1, 64 MiB of 16-bit elements per operand (N = 32 Mi elements):
//   fused   dccl_local_reduce_chain_widen: one launch, (k + 1) 2N bytes read and 4N written (8N moved on the
//           destination side with accumulate);
//   routeb  what gave the same bits before that entry point existed: dccl_local_convert of each of the k + 1 operands
//           to fp32, then dccl_local_reduce_chain (fp32, Sum) over the widened operands, and with accumulate that
//           chain into a temporary and dccl_local_reduce (fp32, Sum) of it into dst: k + 2 or k + 3 launches,
//           (k + 1) 6N + (k + 2) 4N bytes (+ 12N with accumulate);
//   wide    dccl_local_reduce_chain_wide on the same operands (16 bits out, (k + 2) 2N bytes), for scale.
// Every case: warm-up, then ROUNDS rounds of [PER fused | PER routeb | PER wide], each batch between two device events
// (ROUNDS * PER = 240 timed repetitions per arm).  One JSON line per case on stdout: each arm's median round with its
// spread over the rounds (min, max), the fused and wide arms' rates against their own algorithmic bytes, and
// routeb_over_fused with the worst-case ratio over the rounds (routeb's fastest round over fused's slowest).
//   hipcc -std=c++17 -O2 -I include tools/widen_ab.cpp -o tools/bin/widen_ab -L dccl_amd/lib -ldccl_amd \
//         -Wl,-rpath,$PWD/dccl_amd/lib && tools/bin/widen_ab > profiles/widen_ab.json
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
constexpr size_t kBytes = size_t(64) << 20;  // of 16-bit elements per operand
constexpr int kRounds = 12, kPer = 20, kWarm = 10;
constexpr int kArms = 3;

struct Stat { double med, lo, hi; };

Stat stat(std::vector<double> v) {
    std::sort(v.begin(), v.end());
    return {v[v.size() / 2], v.front(), v.back()};
}

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
}  // namespace

int main() {
    hipStream_t st;
    CK(hipStreamCreate(&st));
    // 8 operands of 16-bit elements, their 8 fp32 copies (route B), the fp32 dst, route B's temporary, the wide
    // arm's 16-bit dst
    unsigned char *half = nullptr, *full = nullptr;
    CK(hipMalloc(reinterpret_cast<void**>(&half), 9 * kBytes));
    CK(hipMalloc(reinterpret_cast<void**>(&full), 10 * 2 * kBytes));
    CK(hipMemset(half, 0x3c, 9 * kBytes));  // bf16 0x3c3c about 0.0115, fp16 0x3c3c about 1.06: finite sums
    CK(hipMemset(full, 0, 10 * 2 * kBytes));  // dst starts at 0.0f and stays finite under accumulate
    CK(hipDeviceSynchronize());
    const size_t n = kBytes / 2;
    auto h = [&](int i) { return half + size_t(i) * kBytes; };
    auto f = [&](int i) { return full + size_t(i) * 2 * kBytes; };
    struct { int dtype; const char* name; } types[] = {{9, "bf16"}, {6, "fp16"}};
    for (const auto& t : types)
        for (int k : {1, 3, 7})
            for (int acc : {0, 1}) {
                const void *sends[8], *wsends[8];
                for (int j = 0; j < k; ++j) sends[j] = h(j), wsends[j] = f(j);
                const void* own = h(7);
                void *wown = f(7), *dst = f(8), *tmp = f(9), *dst16 = h(8);
                const std::function<int()> arm[kArms] = {
                    [&] { return dccl_local_reduce_chain_widen(sends, k, own, dst, t.dtype, n, acc, st); },
                    [&] {
                        int rc = 0;
                        for (int j = 0; j < k && rc == 0; ++j) rc = dccl_local_convert(h(j), t.dtype, f(j), 7, n, st);
                        if (rc == 0) rc = dccl_local_convert(own, t.dtype, wown, 7, n, st);
                        if (rc == 0) rc = dccl_local_reduce_chain(wsends, k, wown, acc ? tmp : dst, 7, n, 0, st);
                        if (rc == 0 && acc) rc = dccl_local_reduce(tmp, dst, 7, n, 0, st);
                        return rc;
                    },
                    [&] { return dccl_local_reduce_chain_wide(sends, k, own, dst16, t.dtype, n, st); },
                };
                Stat s[kArms];
                abc(st, arm, s);
                const double fused_gb = (double(k + 1) * 2 + (acc ? 8 : 4)) * n / 1e9;
                const double routeb_gb = (double(k + 1) * 6 + double(k + 2) * 4 + (acc ? 12 : 0)) * n / 1e9;
                const double wide_gb = double(k + 2) * 2 * n / 1e9;
                printf("{\"case\": \"widen\", \"dtype\": \"%s\", \"k\": %d, \"accumulate\": %d, \"elements\": %zu, "
                       "\"fused_us\": %.1f, \"fused_us_min\": %.1f, \"fused_us_max\": %.1f, \"fused_gb\": %.3f, "
                       "\"fused_gb_s\": %.0f, "
                       "\"routeb_us\": %.1f, \"routeb_us_min\": %.1f, \"routeb_us_max\": %.1f, \"routeb_gb\": %.3f, "
                       "\"routeb_over_fused\": %.2f, \"routeb_over_fused_worst\": %.2f, "
                       "\"wide_us\": %.1f, \"wide_us_min\": %.1f, \"wide_us_max\": %.1f, \"wide_gb_s\": %.0f}\n",
                       t.name, k, acc, n, s[0].med, s[0].lo, s[0].hi, fused_gb, fused_gb / (s[0].med * 1e-6), s[1].med,
                       s[1].lo, s[1].hi, routeb_gb, s[1].med / s[0].med, s[1].lo / s[0].hi, s[2].med, s[2].lo, s[2].hi,
                       wide_gb / (s[2].med * 1e-6));
                fflush(stdout);
            }
    CK(hipFree(half));
    CK(hipFree(full));
    return 0;
}
