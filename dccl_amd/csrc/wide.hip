// dccl_amd/csrc/wide.hip — wide sum (dcclRedOpCreateWideSum): fp16 / bf16 contributions accumulated in fp32 and
// rounded to 16 bits once.
//
//   dccl_local_reduce_chain_wide   acc = widen(sends[0][i]); acc = widen(sends[j][i]) + acc, j = 1..k-1;
//                                  acc = widen(own[i]) + acc;  dst[i] = round16(acc)
//   dccl_local_convert             dst[i] = widen(src[i]) (fp16 / bf16 -> fp32, exact) or round16(src[i])
//                                  (fp32 -> fp16 / bf16, nearest-even)
//
// widen and round16 are combine.hpp's f16_to_f32 / bf16_to_f32 / f32_to_f16 / f32_to_bf16, the conversions the Sum
// combine itself applies, and every add is one IEEE fp32 add in dccl_local_reduce_chain's order (sends[0] first,
// own last).  The chain therefore gives the bits of "widen every operand, run the fp32 Sum chain, round once";
// with one source it gives the plain 16-bit chain's bits (one add, one rounding).  It reads and writes what the
// plain chain does: 16-bit operands in, 16 bits out.  There is no pre-multiplied form.  Every store is an
// ordinary vector store.
//
// Forms: operands that are element-aligned and share the destination's 16-B phase take the vector kernel (head
// scalars | 16-B non-temporal vectors, eight fp32 accumulators per lane | tail scalars, under local_reduce.hip's
// chain caps).  The conversion's vector kernel needs the 16-bit side's 16-B vectors and the fp32 side to line up:
// 16 B of 16-bit elements against 2 x 16 B of fp32.  Any other placement (another phase, operands off element
// alignment) takes one coalesced element-wise kernel: that fallback is for correctness only, nobody has tuned it.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dccl/dccl_reduce.h"
#include "dispatch.hpp"
#include "reduce_kernels.hpp"

namespace dccl_amd {
namespace {

// local_reduce.hip's shipped shape: one-wave blocks, one 16-B vector per lane and operand, all non-temporal
using DefaultCfg = VecCfg<64, 1, kNtSend | kNtRecv | kNtStore, false>;
// the head scalars bring the destination to its 128-B lines (local_reduce.hip's default recv_align)
constexpr size_t kDstAlign = 128;
constexpr int kLanes16 = 8;  // 16-bit elements of one 16-B vector

template <typename T> struct Wide;
template <> struct Wide<f16_bits> {
    __device__ __forceinline__ static float widen(f16_bits x) { return f16_to_f32(x.v); }
    __device__ __forceinline__ static f16_bits narrow(float f) { return f16_bits{f32_to_f16(f)}; }
};
template <> struct Wide<bf16_bits> {
    __device__ __forceinline__ static float widen(bf16_bits x) { return bf16_to_f32(x.v); }
    __device__ __forceinline__ static bf16_bits narrow(float f) { return bf16_bits{f32_to_bf16(f)}; }
};

struct F32x8 { float f[kLanes16]; };
struct U32x4x2 { u32x4 v[2]; };  // the same eight fp32 as two 16-B vectors (whole-object bit casts only)

template <typename T>
__device__ __forceinline__ F32x8 widen16(u32x4 v) {
    const Pack<T> p = __builtin_bit_cast(Pack<T>, v);
    F32x8 w;
#pragma unroll
    for (int i = 0; i < kLanes16; ++i) w.f[i] = Wide<T>::widen(p.e[i]);
    return w;
}

template <typename T>
__device__ __forceinline__ u32x4 narrow16(const F32x8& w) {
    Pack<T> p;
#pragma unroll
    for (int i = 0; i < kLanes16; ++i) p.e[i] = Wide<T>::narrow(w.f[i]);
    return __builtin_bit_cast(u32x4, p);
}

// acc = widen(v) + acc, lane by lane
template <typename T>
__device__ __forceinline__ void add16(F32x8& acc, u32x4 v) {
    const F32x8 w = widen16<T>(v);
#pragma unroll
    for (int i = 0; i < kLanes16; ++i) acc.f[i] = w.f[i] + acc.f[i];
}

// index of block 0's j-th scalar element: head [0, head), then the tail past the vector body
__device__ __forceinline__ size_t edge_index(size_t j, size_t head, size_t nvec) {
    return j < head ? j : head + nvec * kLanes16 + (j - head);
}

// ---- chain: reduce_chain_vec_kernel's roles and order, one fp32 accumulator per element ----
template <typename T, int K, typename C>
__global__ __launch_bounds__(C::BLOCK) void wide_chain_vec_kernel(SendList sends, const unsigned char* own,
                                                                  unsigned char* dst, size_t head, size_t nvec,
                                                                  size_t tail) {
    static_assert(C::UNROLL == 1, "one vector per lane");
    const size_t off = head * sizeof(T);
    const u32x4* vo = reinterpret_cast<const u32x4*>(own + off);
    u32x4* vd = reinterpret_cast<u32x4*>(dst + off);
    const size_t ntiles = (nvec + C::TILE - 1) / C::TILE;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t i = t * C::TILE + threadIdx.x;
        if (i < nvec) {
            u32x4 s[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                s[k] = ld16<(C::POLICY & kNtSend) != 0>(reinterpret_cast<const u32x4*>(sends.p[k] + off) + i);
            const u32x4 o = ld16<true>(vo + i);
            F32x8 acc = widen16<T>(s[0]);
#pragma unroll
            for (int k = 1; k < K; ++k) add16<T>(acc, s[k]);
            add16<T>(acc, o);
            __builtin_nontemporal_store(narrow16<T>(acc), vd + i);
        }
    }
    if (blockIdx.x == 0)
        for (size_t j = threadIdx.x; j < head + tail; j += blockDim.x) {
            const size_t i = edge_index(j, head, nvec);
            float acc = Wide<T>::widen(ld_elem<T, true>(sends.p[0], i));
#pragma unroll
            for (int k = 1; k < K; ++k) acc = Wide<T>::widen(ld_elem<T, true>(sends.p[k], i)) + acc;
            acc = Wide<T>::widen(ld_elem<T, true>(own, i)) + acc;
            st_elem<T, true>(dst, i, Wide<T>::narrow(acc));
        }
}

// Any placement, one element per thread and step (correctness only).
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void wide_chain_elem_kernel(SendList sends, int nsend, const unsigned char* own,
                                                                 unsigned char* dst, size_t count) {
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += size_t(gridDim.x) * kBlock) {
        float acc = Wide<T>::widen(ld_elem<T, ALIGNED>(sends.p[0], i));
        for (int k = 1; k < nsend; ++k) acc = Wide<T>::widen(ld_elem<T, ALIGNED>(sends.p[k], i)) + acc;
        acc = Wide<T>::widen(ld_elem<T, ALIGNED>(own, i)) + acc;
        st_elem<T, ALIGNED>(dst, i, Wide<T>::narrow(acc));
    }
}

// ---- convert: `half` is the 16-bit side, `full` the fp32 side; WIDEN: half -> full, else full -> half ----
template <typename T, bool WIDEN>
__global__ __launch_bounds__(64) void convert_vec_kernel(const unsigned char* src, unsigned char* dst, size_t head,
                                                         size_t nvec, size_t tail) {
    const size_t ntiles = (nvec + 63) / 64;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t i = t * 64 + threadIdx.x;
        if (i >= nvec) continue;
        if constexpr (WIDEN) {
            const u32x4* vs = reinterpret_cast<const u32x4*>(src + head * sizeof(T));
            u32x4* vd = reinterpret_cast<u32x4*>(dst + head * sizeof(float));
            const U32x4x2 w = __builtin_bit_cast(U32x4x2, widen16<T>(ld16<true>(vs + i)));
            __builtin_nontemporal_store(w.v[0], vd + 2 * i);
            __builtin_nontemporal_store(w.v[1], vd + 2 * i + 1);
        } else {
            const u32x4* vs = reinterpret_cast<const u32x4*>(src + head * sizeof(float));
            u32x4* vd = reinterpret_cast<u32x4*>(dst + head * sizeof(T));
            const U32x4x2 w{{ld16<true>(vs + 2 * i), ld16<true>(vs + 2 * i + 1)}};
            __builtin_nontemporal_store(narrow16<T>(__builtin_bit_cast(F32x8, w)), vd + i);
        }
    }
    if (blockIdx.x == 0)
        for (size_t j = threadIdx.x; j < head + tail; j += blockDim.x) {
            const size_t i = edge_index(j, head, nvec);
            if constexpr (WIDEN) st_elem<float, true>(dst, i, Wide<T>::widen(ld_elem<T, true>(src, i)));
            else st_elem<T, true>(dst, i, Wide<T>::narrow(ld_elem<float, true>(src, i)));
        }
}

template <typename T, bool WIDEN, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void convert_elem_kernel(const unsigned char* src, unsigned char* dst,
                                                              size_t count) {
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += size_t(gridDim.x) * kBlock) {
        if constexpr (WIDEN) st_elem<float, ALIGNED>(dst, i, Wide<T>::widen(ld_elem<T, ALIGNED>(src, i)));
        else st_elem<T, ALIGNED>(dst, i, Wide<T>::narrow(ld_elem<float, ALIGNED>(src, i)));
    }
}

// ---- launches ----
template <typename T, int K>
int launch_wide_chain_vec(SendList sl, const unsigned char* own, unsigned char* d, Split sp, hipStream_t stream) {
    using C = DefaultCfg;
    size_t grid = ceil_div(sp.nvec, C::TILE);
    if (grid == 0 && (sp.head + sp.tail) > 0) grid = 1;
    void* args[] = {&sl, &own, &d, &sp.head, &sp.nvec, &sp.tail};
    // the plain chain's caps (launch_chain_vec): not measured for this kernel's register use
    return launch(reinterpret_cast<const void*>(&wide_chain_vec_kernel<T, K, C>), grid, args, stream, C::BLOCK,
                  caps::lds(caps::kChain, K, caps_bytes(sp.nvec * 16)));
}

template <typename T>
int wide_chain_typed(const void* const* sends, int nsend, const void* own, void* dst, size_t count,
                     hipStream_t stream) {
    SendList sl{};
    const uintptr_t ad = reinterpret_cast<uintptr_t>(dst), ao = reinterpret_cast<uintptr_t>(own);
    bool elem_ok = ad % sizeof(T) == 0 && ao % sizeof(T) == 0, in_phase = ((ad ^ ao) & 15) == 0;
    for (int k = 0; k < nsend; ++k) {
        sl.p[k] = static_cast<const unsigned char*>(sends[k]);
        const uintptr_t a = reinterpret_cast<uintptr_t>(sends[k]);
        if (a % sizeof(T)) elem_ok = false;
        if ((a ^ ad) & 15) in_phase = false;
    }
    auto o = static_cast<const unsigned char*>(own);
    auto d = static_cast<unsigned char*>(dst);
    if (!elem_ok || !in_phase) {
        void* args[] = {&sl, &nsend, &o, &d, &count};
        const void* fn = elem_ok ? reinterpret_cast<const void*>(&wide_chain_elem_kernel<T, true>)
                                 : reinterpret_cast<const void*>(&wide_chain_elem_kernel<T, false>);
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    const Split sp = split_for_vectors<T>(ad, count, kDstAlign);
    return with_k<1, 8>(nsend, [&](auto K) { return launch_wide_chain_vec<T, K.value>(sl, o, d, sp, stream); });
}

template <typename T, bool WIDEN>
int convert_typed(const void* src, void* dst, size_t count, hipStream_t stream) {
    auto s = static_cast<const unsigned char*>(src);
    auto d = static_cast<unsigned char*>(dst);
    const uintptr_t as = reinterpret_cast<uintptr_t>(src), ad = reinterpret_cast<uintptr_t>(dst);
    const uintptr_t half = WIDEN ? as : ad, full = WIDEN ? ad : as;
    const bool elem_ok = half % sizeof(T) == 0 && full % sizeof(float) == 0;
    // head elements bring the 16-bit side to a 16-B boundary; the fp32 side must be on one there too
    size_t head = elem_ok ? ((16 - (half & 15)) & 15) / sizeof(T) : 0;
    if (!elem_ok || ((full + head * sizeof(float)) & 15)) {
        void* args[] = {&s, &d, &count};
        const void* fn = elem_ok ? reinterpret_cast<const void*>(&convert_elem_kernel<T, WIDEN, true>)
                                 : reinterpret_cast<const void*>(&convert_elem_kernel<T, WIDEN, false>);
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    if (head > count) head = count;
    size_t nvec = (count - head) / kLanes16, tail = count - head - nvec * kLanes16;
    size_t grid = ceil_div(nvec, size_t(64));
    if (grid == 0 && (head + tail) > 0) grid = 1;
    void* args[] = {&s, &d, &head, &nvec, &tail};
    return launch(reinterpret_cast<const void*>(&convert_vec_kernel<T, WIDEN>), grid, args, stream, 64);
}

bool is_16bit_float(int dtype) { return dtype == kFloat16 || dtype == kBfloat16; }

// [a, a + na) and [b, b + nb) share a byte
bool ranges_intersect(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x < na : x - y < nb;
}

}  // namespace
}  // namespace dccl_amd

using namespace dccl_amd;

extern "C" int dccl_local_reduce_chain_wide(const void* const* sends, int nsend, const void* own, void* dst,
                                            int dtype, size_t count, void* stream) {
    if (!is_16bit_float(dtype)) return DCCL_INVALID_ARGUMENT;
    if (nsend < 1 || nsend > 8 || sends == nullptr) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (own == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    for (int k = 0; k < nsend; ++k)
        if (sends[k] == nullptr) return DCCL_INVALID_ARGUMENT;
    if (sources_overlap_destination(sends, nsend, own, dst, count * size_of_dtype(dtype)))
        return DCCL_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == kFloat16 ? wide_chain_typed<f16_bits>(sends, nsend, own, dst, count, st)
                             : wide_chain_typed<bf16_bits>(sends, nsend, own, dst, count, st);
}

extern "C" int dccl_local_convert(const void* src, int src_dtype, void* dst, int dst_dtype, size_t count,
                                  void* stream) {
    const bool widen = is_16bit_float(src_dtype) && dst_dtype == kFloat32;
    const bool narrow = src_dtype == kFloat32 && is_16bit_float(dst_dtype);
    if (!widen && !narrow) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (src == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    if (ranges_intersect(src, count * size_of_dtype(src_dtype), dst, count * size_of_dtype(dst_dtype)))
        return DCCL_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (widen)
        return src_dtype == kFloat16 ? convert_typed<f16_bits, true>(src, dst, count, st)
                                     : convert_typed<bf16_bits, true>(src, dst, count, st);
    return dst_dtype == kFloat16 ? convert_typed<f16_bits, false>(src, dst, count, st)
                                 : convert_typed<bf16_bits, false>(src, dst, count, st);
}
