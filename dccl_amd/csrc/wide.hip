// dccl_amd/csrc/wide.hip — wide sum (dcclRedOpCreateWideSum): fp16 / bf16 contributions accumulated in fp32 and
// rounded to 16 bits once, and its scaled form (dcclRedOpCreateWideScaledSum, §7.8): the finished
// fp32 accumulator times one fp32 scalar s, then the one rounding.
//
//   dccl_local_reduce_chain_wide          acc = widen(sends[0][i]); acc = widen(sends[j][i]) + acc, j = 1..k-1;
//                                         acc = widen(own[i]) + acc;  dst[i] = round16(acc)
//   dccl_local_reduce_chain_wide_scaled   the same acc;  dst[i] = round16(acc * s)
//   dccl_local_reduce_chain_widen         the same acc;  dst (fp32)[i] = acc, or dst[i] + acc
//   dccl_local_reduce_chain_widen_checked the same, and *flag = 1 when some acc is +-inf or NaN
//   dccl_local_nonfinite_f32              *flag = 1 when some src (fp32)[i] is +-inf or NaN; reads only
//   dccl_local_convert                    dst[i] = widen(src[i]) (fp16 / bf16 -> fp32, exact) or round16(src[i])
//                                         (fp32 -> fp16 / bf16, nearest-even)
//   dccl_local_convert_scaled             dst[i] = round16(as_fp32(src[i]) * s), src fp32 or dst's own 16-bit type
//
// widen and round16 are combine.hpp's f16_to_f32 / bf16_to_f32 / f32_to_f16 / f32_to_bf16, the conversions the Sum
// combine itself applies, and every add is one IEEE fp32 add in dccl_local_reduce_chain's order (sends[0] first,
// own last).  The chain therefore gives the bits of "widen every operand, run the fp32 Sum chain, round once";
// with one source it gives the plain 16-bit chain's bits (one add, one rounding).  It reads and writes what the
// plain chain does: 16-bit operands in, 16 bits out.  The scaled form multiplies AFTER the sum (one IEEE fp32
// multiply per element, never fused with an add; a wide sum of pre-multiplied contributions does not exist); its
// scalar travels as scalar_arg.hpp's ScalarArg.  Every store is an ordinary vector store.
//
// The chain kernels are reduce_kernels.hpp's chain bodies (the plain chain's tile loop, loads, ring order and edge
// elements) with the WideChain policy below, eight fp32 accumulators per lane; their placement rule and launch are
// chain_forms.hpp's.  The conversion has a body of its own: its vector kernel needs the 16-bit side's 16-B vectors
// and the fp32 side to line up (16 B of 16-bit elements against 2 x 16 B of fp32), and any other placement takes one
// coalesced element-wise kernel (correctness only, nobody has tuned it).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#include "chain_forms.hpp"
#include "dccl/dccl_reduce.h"
#include "scalar_arg.hpp"

namespace dccl_amd {
namespace {

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

// widen(v) + acc, lane by lane
template <typename T>
__device__ __forceinline__ F32x8 add16(u32x4 v, F32x8 acc) {
    const F32x8 w = widen16<T>(v);
#pragma unroll
    for (int i = 0; i < kLanes16; ++i) acc.f[i] = w.f[i] + acc.f[i];
    return acc;
}

// acc * s on its way to the 16-bit rounding of ONE element (edge elements, element-wise kernels): one IEEE fp32
// multiply, rounded to fp32 (no contraction: nothing may fuse it with an add of the chain).  For fp16 the product
// then passes an identity lane move (every lane reads itself).  Without it hipcc selects v_fma_mixlo_f16 /
// v_fma_mixhi_f16 for "fp32 multiply, convert to fp16", one instruction for both steps, wherever a conversion is not
// half of a packed pair.  On gfx950 its results are not those of the fp32 rounding followed by the fp16 rounding
// that the contract states: they differ where the exact product rounds differently in one step than in two, about
// 1 % of elements with s = 0.3.  No pragma or flag reaches that selection; the move keeps
// v_mul_f32 and v_cvt_f16_f32 two instructions.  bf16 has no such instruction.
template <typename T>
__device__ __forceinline__ float scale1(float acc, float s) {
#pragma clang fp contract(off)
    const float p = acc * s;
    if constexpr (std::is_same_v<T, f16_bits>)  // quad_perm [0, 1, 2, 3], every row and bank: the identity
        return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, p), 0xE4, 0xF, 0xF, true));
    else return p;
}
// Eight products, rounded: bf16 lane by lane; fp16 as four explicit pairs, a 2-vector multiply and a 2-vector
// conversion (v_pk_mul_f32, v_cvt_pk_f16_f32), which the compiler keeps two instructions: no lane moves in the
// vector loops, and no lane left for the fused instruction above.
template <typename T>
__device__ __forceinline__ u32x4 narrow_scaled16(const F32x8& acc, float s) {
    if constexpr (std::is_same_v<T, f16_bits>) {
#pragma clang fp contract(off)
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
        struct { f16x2 h[kLanes16 / 2]; } p;
#pragma unroll
        for (int i = 0; i < kLanes16 / 2; ++i)
            p.h[i] = __builtin_convertvector(f32x2{acc.f[2 * i], acc.f[2 * i + 1]} * s, f16x2);
        return __builtin_bit_cast(u32x4, p);
    } else {
        Pack<T> p;
#pragma unroll
        for (int i = 0; i < kLanes16; ++i) p.e[i] = Wide<T>::narrow(scale1<T>(acc.f[i], s));
        return __builtin_bit_cast(u32x4, p);
    }
}

// How the finished fp32 accumulators become 16 bits: rounded as they are, or multiplied by the fp32 scalar s first.
struct NoScale {
    template <typename T>
    __device__ __forceinline__ u32x4 finish16(const F32x8& acc) const { return narrow16<T>(acc); }
    template <typename T>
    __device__ __forceinline__ T finish(float acc) const { return Wide<T>::narrow(acc); }
};
struct ScaleBy {
    float s;
    template <typename T>
    __device__ __forceinline__ u32x4 finish16(const F32x8& acc) const { return narrow_scaled16<T>(acc, s); }
    template <typename T>
    __device__ __forceinline__ T finish(float acc) const { return Wide<T>::narrow(scale1<T>(acc, s)); }
};

// The chain policy (reduce_kernels.hpp chain_vec_body): fp32 accumulators, rounded to 16 bits once, at the store.
template <typename T, typename Scale = NoScale>
struct WideChain {
    using Elem = T;
    Scale scale;
    __device__ __forceinline__ F32x8 first16(u32x4 v) const { return widen16<T>(v); }
    __device__ __forceinline__ F32x8 fold16(u32x4 v, F32x8 acc) const { return add16<T>(v, acc); }
    __device__ __forceinline__ u32x4 finish16(const F32x8& acc) const { return scale.template finish16<T>(acc); }
    __device__ __forceinline__ float first(T x) const { return Wide<T>::widen(x); }
    __device__ __forceinline__ float fold(T x, float acc) const { return Wide<T>::widen(x) + acc; }
    __device__ __forceinline__ T finish(float acc) const { return scale.template finish<T>(acc); }
};
template <typename T>
using WideScaledChain = WideChain<T, ScaleBy>;

// ---- chain: reduce_chain_vec_kernel's roles and order, one fp32 accumulator per element ----
template <typename T, int K, typename C>
__global__ __launch_bounds__(C::BLOCK) void wide_chain_vec_kernel(SendList sends, const unsigned char* own,
                                                                  unsigned char* dst, size_t head, size_t nvec,
                                                                  size_t tail) {
    chain_vec_body<WideChain<T>, K, C>(sends, own, dst, head, nvec, tail, WideChain<T>{});
}

// Any placement, one element per thread and step (correctness only).
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void wide_chain_elem_kernel(SendList sends, int nsend, const unsigned char* own,
                                                                 unsigned char* dst, size_t count) {
    chain_elem_body<WideChain<T>, ALIGNED>(sends, nsend, own, dst, count, WideChain<T>{});
}

template <typename T, int K, typename C>
__global__ __launch_bounds__(C::BLOCK) void wide_scaled_chain_vec_kernel(SendList sends, const unsigned char* own,
                                                                         unsigned char* dst, size_t head, size_t nvec,
                                                                         size_t tail, ScalarArg sa) {
    chain_vec_body<WideScaledChain<T>, K, C>(sends, own, dst, head, nvec, tail,
                                             WideScaledChain<T>{{load_scalar<float>(sa)}});
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void wide_scaled_chain_elem_kernel(SendList sends, int nsend,
                                                                        const unsigned char* own, unsigned char* dst,
                                                                        size_t count, ScalarArg sa) {
    chain_elem_body<WideScaledChain<T>, ALIGNED>(sends, nsend, own, dst, count,
                                                 WideScaledChain<T>{{load_scalar<float>(sa)}});
}

// ---- widened chain (dccl_local_reduce_chain_widen): the wide chain's accumulator stored as fp32,
// ACC: added to what dst holds by one more fp32 add after the chain (prior + acc; two adds, nothing to contract).
// A sibling of chain_vec_body, whose loads, order and edge elements it follows: the 16-bit operands are walked in
// 16-B vectors, dst in the 2 x 16 B that hold the same eight elements (convert_vec_kernel<T, true>'s stores).
// `head` elements bring the 16-bit operands to their 16-B boundary; dst is on one there too (widen_typed). ----
//
// CHECK (dccl_local_reduce_chain_widen_checked): every finished accumulator, before ACC's add, passes
// an integer test of its exponent field, ORed into one register of the thread over all of its tiles and edge
// elements; a thread that saw a non-finite one stores 1 to `flag` after its loops.  Every writer stores the same
// word, so there is no atomic, no LDS and no cross-lane step, and nothing is stored when every accumulator is finite.

// Bit 31 of the result is set exactly when acc's exponent field is all ones (+-inf or a NaN): the field plus one
// carries into it, any other field does not.  Integer arithmetic on the bits: nothing a float comparison could fold.
__device__ __forceinline__ uint32_t nonfinite_bit(float acc) {
    return (__builtin_bit_cast(uint32_t, acc) & 0x7f800000u) + 0x00800000u;
}
__device__ __forceinline__ void raise_if(uint32_t bad, uint32_t* flag) {
    if (bad >> 31) *flag = 1u;
}
// The kernels' last argument: the flag's address, or nothing at all for the unchecked instances, whose code is the
// one they had before CHECK existed ("Build facts").
template <bool CHECK> struct FlagArg { uint32_t* p; };
template <> struct FlagArg<false> {};

template <typename T, int K, bool ACC, typename C, bool CHECK = false>
__global__ __launch_bounds__(C::BLOCK) void widen_chain_vec_kernel(SendList sends, const unsigned char* own,
                                                                   unsigned char* dst, size_t head, size_t nvec,
                                                                   size_t tail, FlagArg<CHECK> flag) {
    static_assert(C::UNROLL == 1, "one vector per lane");
    [[maybe_unused]] uint32_t bad = 0;
    const size_t off = head * sizeof(T);
    const u32x4* vo = reinterpret_cast<const u32x4*>(own + off);
    u32x4* vd = reinterpret_cast<u32x4*>(dst + head * sizeof(float));
    const size_t ntiles = (nvec + C::TILE - 1) / C::TILE;
    for (size_t t = C::XCD ? xcd_remap(blockIdx.x, gridDim.x) : run_tile<C::RUN>(blockIdx.x, gridDim.x); t < ntiles;
         t += gridDim.x) {
        const size_t i = t * C::TILE + threadIdx.x;
        if (i < nvec) {
            U32x4x2 prior{};
            if constexpr (ACC) prior = U32x4x2{{ld16<true>(vd + 2 * i), ld16<true>(vd + 2 * i + 1)}};
            u32x4 s[K];
#pragma unroll
            for (int k = 0; k < K; ++k)
                s[k] = ld16<(C::POLICY & kNtSend) != 0>(reinterpret_cast<const u32x4*>(sends.p[k] + off) + i);
            const u32x4 o = ld16<true>(vo + i);
            F32x8 acc = widen16<T>(s[0]);
#pragma unroll
            for (int k = 1; k < K; ++k) acc = add16<T>(s[k], acc);
            acc = add16<T>(o, acc);
            if constexpr (CHECK) {
#pragma unroll
                for (int l = 0; l < kLanes16; ++l) bad |= nonfinite_bit(acc.f[l]);
                // ACC false: the test ends here.  Left to itself the scheduler puts it between the two stores below,
                // the two halves of each lane's 32 B, and this kernel, which only writes dst, then ran 10 % (k = 3)
                // to 33 % (k = 1) longer at 32 Mi elements than its unchecked twin, whose stores are back to back
                // (DESIGN.md §7.12 "The scheduling barrier"; both runs: profiles/widen_checked_ab.json).  With ACC
                // the scheduler's own order measured equal, and stays.
                if constexpr (!ACC) __builtin_amdgcn_sched_barrier(0);
            }
            if constexpr (ACC) {
                const F32x8 was = __builtin_bit_cast(F32x8, prior);
#pragma unroll
                for (int l = 0; l < kLanes16; ++l) acc.f[l] = was.f[l] + acc.f[l];
            }
            const U32x4x2 w = __builtin_bit_cast(U32x4x2, acc);
            __builtin_nontemporal_store(w.v[0], vd + 2 * i);
            __builtin_nontemporal_store(w.v[1], vd + 2 * i + 1);
        }
    }
    if (blockIdx.x == 0) {
        for (size_t j = threadIdx.x; j < head + tail; j += blockDim.x) {
            const size_t i = edge_index<T>(j, head, nvec);
            float acc = Wide<T>::widen(ld_elem<T, true>(sends.p[0], i));
#pragma unroll
            for (int k = 1; k < K; ++k) acc = Wide<T>::widen(ld_elem<T, true>(sends.p[k], i)) + acc;
            acc = Wide<T>::widen(ld_elem<T, true>(own, i)) + acc;
            if constexpr (CHECK) bad |= nonfinite_bit(acc);
            if constexpr (ACC) acc = ld_elem<float, true>(dst, i) + acc;
            st_elem<float, true>(dst, i, acc);
        }
    }
    if constexpr (CHECK) raise_if(bad, flag.p);
}

// Any placement, one element per thread and step (correctness only).  ALIGNED: the 16-bit operands on 2-byte and
// dst on 4-byte boundaries; else byte loads and stores on every side.
template <typename T, bool ACC, bool ALIGNED, bool CHECK = false>
__global__ __launch_bounds__(kBlock) void widen_chain_elem_kernel(SendList sends, int nsend, const unsigned char* own,
                                                                  unsigned char* dst, size_t count,
                                                                  FlagArg<CHECK> flag) {
    [[maybe_unused]] uint32_t bad = 0;
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += size_t(gridDim.x) * kBlock) {
        float acc = Wide<T>::widen(ld_elem<T, ALIGNED>(sends.p[0], i));
        for (int k = 1; k < nsend; ++k) acc = Wide<T>::widen(ld_elem<T, ALIGNED>(sends.p[k], i)) + acc;
        acc = Wide<T>::widen(ld_elem<T, ALIGNED>(own, i)) + acc;
        if constexpr (CHECK) bad |= nonfinite_bit(acc);
        if constexpr (ACC) acc = ld_elem<float, ALIGNED>(dst, i) + acc;
        st_elem<float, ALIGNED>(dst, i, acc);
    }
    if constexpr (CHECK) raise_if(bad, flag.p);
}

// ---- dccl_local_nonfinite_f32: the same flag from a read-only pass over fp32 (the staged routes' sums).  One-wave
// blocks, 16-B non-temporal loads of the aligned body, at most three head and three tail elements in block 0. ----
__global__ __launch_bounds__(64) void nonfinite_f32_kernel(const unsigned char* src, size_t head, size_t nvec,
                                                           size_t tail, uint32_t* flag) {
    const u32x4* vs = reinterpret_cast<const u32x4*>(src + head * sizeof(float));
    const size_t ntiles = (nvec + 63) / 64;
    uint32_t bad = 0;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t i = t * 64 + threadIdx.x;
        if (i >= nvec) continue;
        const u32x4 v = ld16<true>(vs + i);
#pragma unroll
        for (int l = 0; l < 4; ++l) bad |= (v[l] & 0x7f800000u) + 0x00800000u;
    }
    if (blockIdx.x == 0)
        for (size_t j = threadIdx.x; j < head + tail; j += blockDim.x)
            bad |= nonfinite_bit(ld_elem<float, true>(src, edge_index<float>(j, head, nvec)));
    raise_if(bad, flag);
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
            const size_t i = edge_index<T>(j, head, nvec);
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

// ---- scaled convert: dst (T) = round16(as_fp32(src) * s); S is float (the staged route's narrowing pass) or T
// (its W = 1 case: 16 B against 16 B, src may be dst) ----
template <typename T, typename S, bool ALIGNED>
__device__ __forceinline__ float ld_as_f32(const unsigned char* src, size_t i) {
    if constexpr (sizeof(S) == sizeof(float)) return ld_elem<float, ALIGNED>(src, i);
    else return Wide<T>::widen(ld_elem<T, ALIGNED>(src, i));
}

template <typename T, typename S>
__global__ __launch_bounds__(64) void convert_scaled_vec_kernel(const unsigned char* src, unsigned char* dst,
                                                                size_t head, size_t nvec, size_t tail, ScalarArg sa) {
    const float s = load_scalar<float>(sa);
    const u32x4* vs = reinterpret_cast<const u32x4*>(src + head * sizeof(S));
    u32x4* vd = reinterpret_cast<u32x4*>(dst + head * sizeof(T));
    const size_t ntiles = (nvec + 63) / 64;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t i = t * 64 + threadIdx.x;
        if (i >= nvec) continue;
        F32x8 w;
        if constexpr (sizeof(S) == sizeof(float)) {
            const U32x4x2 v{{ld16<true>(vs + 2 * i), ld16<true>(vs + 2 * i + 1)}};
            w = __builtin_bit_cast(F32x8, v);
        } else {
            w = widen16<T>(ld16<true>(vs + i));
        }
        __builtin_nontemporal_store(narrow_scaled16<T>(w, s), vd + i);
    }
    if (blockIdx.x == 0)
        for (size_t j = threadIdx.x; j < head + tail; j += blockDim.x) {
            const size_t i = edge_index<T>(j, head, nvec);
            st_elem<T, true>(dst, i, Wide<T>::narrow(scale1<T>(ld_as_f32<T, S, true>(src, i), s)));
        }
}

template <typename T, typename S, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void convert_scaled_elem_kernel(const unsigned char* src, unsigned char* dst,
                                                                     size_t count, ScalarArg sa) {
    const float s = load_scalar<float>(sa);
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += size_t(gridDim.x) * kBlock)
        st_elem<T, ALIGNED>(dst, i, Wide<T>::narrow(scale1<T>(ld_as_f32<T, S, ALIGNED>(src, i), s)));
}

// ---- launches ----
struct WideChainKernels {  // chain_forms.hpp launch_chain_form
    template <typename T, int K>
    static const void* vec() { return reinterpret_cast<const void*>(&wide_chain_vec_kernel<T, K, DefaultCfg>); }
    template <typename T, bool ALIGNED>
    static const void* elem() { return reinterpret_cast<const void*>(&wide_chain_elem_kernel<T, ALIGNED>); }
};

struct WideScaledChainKernels {
    template <typename T, int K>
    static const void* vec() {
        return reinterpret_cast<const void*>(&wide_scaled_chain_vec_kernel<T, K, DefaultCfg>);
    }
    template <typename T, bool ALIGNED>
    static const void* elem() { return reinterpret_cast<const void*>(&wide_scaled_chain_elem_kernel<T, ALIGNED>); }
};

template <typename T, bool WIDEN>
int convert_typed(const void* src, void* dst, size_t count, hipStream_t stream) {
    auto s = static_cast<const unsigned char*>(src);
    auto d = static_cast<unsigned char*>(dst);
    const uintptr_t as = reinterpret_cast<uintptr_t>(src), ad = reinterpret_cast<uintptr_t>(dst);
    // chain_forms.hpp place_pass: the 16-bit side leads, the fp32 side must meet its 16-B vectors
    PassPlacement p = WIDEN ? place_pass(as, sizeof(T), ad, sizeof(float), count)
                            : place_pass(ad, sizeof(T), as, sizeof(float), count);
    if (!p.vec_ok) {
        void* args[] = {&s, &d, &count};
        const void* fn = p.elem_ok ? reinterpret_cast<const void*>(&convert_elem_kernel<T, WIDEN, true>)
                                   : reinterpret_cast<const void*>(&convert_elem_kernel<T, WIDEN, false>);
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    Split& sp = p.sp;
    void* args[] = {&s, &d, &sp.head, &sp.nvec, &sp.tail};
    return launch(reinterpret_cast<const void*>(&convert_vec_kernel<T, WIDEN>), grid_for(sp, 64), args, stream, 64);
}

// place_pass with dst as the 16-bit side; src is fp32, or 16 bits wide like dst.
template <typename T, typename S>
int convert_scaled_typed(const void* src, void* dst, size_t count, ScalarArg sa, hipStream_t stream) {
    auto s = static_cast<const unsigned char*>(src);
    auto d = static_cast<unsigned char*>(dst);
    PassPlacement p =
        place_pass(reinterpret_cast<uintptr_t>(dst), sizeof(T), reinterpret_cast<uintptr_t>(src), sizeof(S), count);
    if (!p.vec_ok) {
        void* args[] = {&s, &d, &count, &sa};
        const void* fn = p.elem_ok ? reinterpret_cast<const void*>(&convert_scaled_elem_kernel<T, S, true>)
                                   : reinterpret_cast<const void*>(&convert_scaled_elem_kernel<T, S, false>);
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    Split& sp = p.sp;
    void* args[] = {&s, &d, &sp.head, &sp.nvec, &sp.tail, &sa};
    return launch(reinterpret_cast<const void*>(&convert_scaled_vec_kernel<T, S>), grid_for(sp, 64), args, stream, 64);
}

// The widened chain's placement rule and launch.  The vector kernel needs every 16-bit operand element-aligned and
// at one 16-B phase, dst on a 4-byte boundary, and dst on a 16-B boundary past the head elements that bring the
// 16-bit operands to theirs (place_pass, `own` leading; no further head elements towards dst's 128-B lines).  It
// launches like launch_chain_form, under the plain chain's caps selected by the fp32 bytes written, which nobody
// has measured for this kernel (more registers per lane, 4 or 8 more bytes per element on the destination side).
// Any other placement takes the element-wise kernel: correctness only, nobody has tuned it.
// CHECK: the kernels' checked instances, with `flag` as their last argument; the rule, the launch and the caps are
// the same.
template <typename T, bool ACC, bool CHECK = false>
int widen_typed(const void* const* sends, int nsend, const void* own, void* dst, size_t count, hipStream_t stream,
                FlagArg<CHECK> flag = {}) {
    const uintptr_t ao = reinterpret_cast<uintptr_t>(own), ad = reinterpret_cast<uintptr_t>(dst);
    bool elem_ok = ao % sizeof(T) == 0 && ad % sizeof(float) == 0, in_phase = true;
    for (int k = 0; k < nsend; ++k) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(sends[k]);
        if (a % sizeof(T)) elem_ok = false;
        if ((a ^ ao) & 15) in_phase = false;
    }
    SendList sl = send_list(sends, nsend);
    auto o = static_cast<const unsigned char*>(own);
    auto d = static_cast<unsigned char*>(dst);
    PassPlacement p{false, false, {0, 0, 0}};
    if (elem_ok && in_phase) p = place_pass(ao, sizeof(T), ad, sizeof(float), count);
    if (!p.vec_ok) {
        void* args[] = {&sl, &nsend, &o, &d, &count, &flag};
        const void* fn = elem_ok ? reinterpret_cast<const void*>(&widen_chain_elem_kernel<T, ACC, true, CHECK>)
                                 : reinterpret_cast<const void*>(&widen_chain_elem_kernel<T, ACC, false, CHECK>);
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    Split& sp = p.sp;
    void* args[] = {&sl, &o, &d, &sp.head, &sp.nvec, &sp.tail, &flag};
    return with_k<1, 8>(nsend, [&](auto K) {
        return launch(reinterpret_cast<const void*>(&widen_chain_vec_kernel<T, K.value, ACC, DefaultCfg, CHECK>),
                      grid_for(sp, DefaultCfg::TILE), args, stream, DefaultCfg::BLOCK,
                      caps::lds(caps::kChain, K.value, caps_bytes(count * sizeof(float))));
    });
}

bool is_16bit_float(int dtype) { return dtype == kFloat16 || dtype == kBfloat16; }

// [a, a + na) and [b, b + nb) share a byte
bool ranges_intersect(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x < na : x - y < nb;
}

// a non-finite flag: one uint32_t on its 4-byte boundary
bool flag_ok(const uint32_t* flag) { return flag != nullptr && reinterpret_cast<uintptr_t>(flag) % 4 == 0; }

// The validation rows dccl_local_reduce_chain_widen and its checked form share, in their order; `flag` is looked at
// only when `checked`.  *run: validation passed and there is something to launch.
int check_widen_args(const void* const* sends, int nsend, const void* own, const void* dst, int dtype, size_t count,
                     int accumulate, bool checked, const uint32_t* flag, bool* run) {
    *run = false;
    if (!is_16bit_float(dtype)) return DCCL_INVALID_ARGUMENT;
    if (accumulate != 0 && accumulate != 1) return DCCL_INVALID_ARGUMENT;
    if (nsend < 1 || nsend > 8 || sends == nullptr) return DCCL_INVALID_ARGUMENT;
    if (checked && !flag_ok(flag)) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (own == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    for (int k = 0; k < nsend; ++k)
        if (sends[k] == nullptr) return DCCL_INVALID_ARGUMENT;
    // no shared byte with the fp32 destination (dccl_local_convert's rule: the element sizes differ)
    const size_t in_bytes = count * size_of_dtype(dtype), out_bytes = count * sizeof(float);
    for (int k = 0; k < nsend; ++k)
        if (ranges_intersect(sends[k], in_bytes, dst, out_bytes)) return DCCL_INVALID_ARGUMENT;
    if (ranges_intersect(own, in_bytes, dst, out_bytes)) return DCCL_INVALID_ARGUMENT;
    if (checked && ranges_intersect(flag, sizeof(uint32_t), dst, out_bytes)) return DCCL_INVALID_ARGUMENT;
    *run = true;
    return DCCL_SUCCESS;
}

}  // namespace
}  // namespace dccl_amd

using namespace dccl_amd;

extern "C" int dccl_local_reduce_chain_wide(const void* const* sends, int nsend, const void* own, void* dst,
                                            int dtype, size_t count, void* stream) {
    if (!is_16bit_float(dtype)) return DCCL_INVALID_ARGUMENT;
    const int rc = check_chain_args(sends, nsend, own, dst, count * size_of_dtype(dtype));
    if (rc != DCCL_SUCCESS || count == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    return dtype == kFloat16 ? launch_chain_form<WideChainKernels, f16_bits>(sends, nsend, own, dst, count, st)
                             : launch_chain_form<WideChainKernels, bf16_bits>(sends, nsend, own, dst, count, st);
}

extern "C" int dccl_local_reduce_chain_widen(const void* const* sends, int nsend, const void* own, void* dst,
                                             int dtype, size_t count, int accumulate, void* stream) {
    bool run;
    const int rc = check_widen_args(sends, nsend, own, dst, dtype, count, accumulate, false, nullptr, &run);
    if (!run) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == kFloat16)
        return accumulate ? widen_typed<f16_bits, true>(sends, nsend, own, dst, count, st)
                          : widen_typed<f16_bits, false>(sends, nsend, own, dst, count, st);
    return accumulate ? widen_typed<bf16_bits, true>(sends, nsend, own, dst, count, st)
                      : widen_typed<bf16_bits, false>(sends, nsend, own, dst, count, st);
}

extern "C" int dccl_local_reduce_chain_widen_checked(const void* const* sends, int nsend, const void* own, void* dst,
                                                     int dtype, size_t count, int accumulate, uint32_t* flag,
                                                     void* stream) {
    bool run;
    const int rc = check_widen_args(sends, nsend, own, dst, dtype, count, accumulate, true, flag, &run);
    if (!run) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (dtype == kFloat16)
        return accumulate ? widen_typed<f16_bits, true, true>(sends, nsend, own, dst, count, st, {flag})
                          : widen_typed<f16_bits, false, true>(sends, nsend, own, dst, count, st, {flag});
    return accumulate ? widen_typed<bf16_bits, true, true>(sends, nsend, own, dst, count, st, {flag})
                      : widen_typed<bf16_bits, false, true>(sends, nsend, own, dst, count, st, {flag});
}

extern "C" int dccl_local_nonfinite_f32(const void* src, size_t count, uint32_t* flag, void* stream) {
    if (!flag_ok(flag)) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (src == nullptr || reinterpret_cast<uintptr_t>(src) % sizeof(float)) return DCCL_INVALID_ARGUMENT;
    if (ranges_intersect(flag, sizeof(uint32_t), src, count * sizeof(float))) return DCCL_INVALID_ARGUMENT;
    auto s = static_cast<const unsigned char*>(src);
    Split sp = split_for_vectors(reinterpret_cast<uintptr_t>(src), count, sizeof(float), 16);
    void* args[] = {&s, &sp.head, &sp.nvec, &sp.tail, &flag};
    return launch(reinterpret_cast<const void*>(&nonfinite_f32_kernel), grid_for(sp, 64), args,
                  static_cast<hipStream_t>(stream), 64);
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

extern "C" int dccl_local_reduce_chain_wide_scaled(const void* const* sends, int nsend, const void* own, void* dst,
                                                   int dtype, size_t count, const void* scalar, int residence,
                                                   void* stream) {
    if (!is_16bit_float(dtype)) return DCCL_INVALID_ARGUMENT;
    if (!scalar_ok(scalar, residence)) return DCCL_INVALID_ARGUMENT;  // where dccl_local_reduce_chain_premul has it
    const int rc = check_chain_args(sends, nsend, own, dst, count * size_of_dtype(dtype));
    if (rc != DCCL_SUCCESS || count == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ScalarArg sa = make_scalar(scalar, residence, sizeof(float));
    return dtype == kFloat16
               ? launch_chain_form<WideScaledChainKernels, f16_bits>(sends, nsend, own, dst, count, st, sa)
               : launch_chain_form<WideScaledChainKernels, bf16_bits>(sends, nsend, own, dst, count, st, sa);
}

extern "C" int dccl_local_convert_scaled(const void* src, int src_dtype, void* dst, int dst_dtype, size_t count,
                                         const void* scalar, int residence, void* stream) {
    const bool from32 = src_dtype == kFloat32 && is_16bit_float(dst_dtype);
    const bool same16 = src_dtype == dst_dtype && is_16bit_float(dst_dtype);
    if (!from32 && !same16) return DCCL_INVALID_ARGUMENT;
    if (!scalar_ok(scalar, residence)) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (src == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    // fp32 source: no shared byte (dccl_local_convert's rule); 16-bit source: src == dst or no shared byte
    if (from32 ? ranges_intersect(src, count * sizeof(float), dst, count * size_of_dtype(dst_dtype))
               : partial_overlap(src, dst, count * size_of_dtype(dst_dtype)))
        return DCCL_INVALID_ARGUMENT;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const ScalarArg sa = make_scalar(scalar, residence, sizeof(float));
    if (from32)
        return dst_dtype == kFloat16 ? convert_scaled_typed<f16_bits, float>(src, dst, count, sa, st)
                                     : convert_scaled_typed<bf16_bits, float>(src, dst, count, sa, st);
    return dst_dtype == kFloat16 ? convert_scaled_typed<f16_bits, f16_bits>(src, dst, count, sa, st)
                                 : convert_scaled_typed<bf16_bits, bf16_bits>(src, dst, count, sa, st);
}
