// dccl_amd/csrc/premul.hip — pre-multiplied sum (ncclRedOpCreatePreMulSum): every contribution is multiplied
// by one scalar s of the operands' dtype before the Sum collective adds it.
//
//   dccl_local_scale                  dst[i] = PreMul(src[i], s)
//   dccl_local_reduce_chain_premul    dst[i] = Sum(PreMul(own[i]), Sum(PreMul(sends[k-1][i]), ...
//                                              Sum(PreMul(sends[1][i]), PreMul(sends[0][i]))))
//
// PreMul is combine.hpp's Prod element multiply and Sum its Sum, each rounded on its own, so both entry
// points give the bits of "multiply every rank's input with today's Prod, then run today's Sum collective":
//   * fp32 / fp64: one IEEE multiply, then one IEEE add.  hipcc contracts a * s + b into one fused
//     multiply-add (a single rounding) by default, also through __fmul_rn and across inlined functions;
//     PreMul<float / double>::apply switches contraction off for its multiply, which keeps v_mul + v_add.
//   * fp16 / bf16: widen to fp32, multiply, ROUND BACK to 16 bits; the Sum widens again.  (fp16 needs the
//     contraction switch as well: see PreMul<f16_bits>.)
//   * integers wrap (8-bit types truncate).
// The scalar travels as scalar_arg.hpp's ScalarArg (read by the host at the call, or by every wave from device
// memory when it runs).  Every store is an ordinary vector store.
//
// The chain kernels are reduce_kernels.hpp's chain bodies (the plain chain's tile loop, loads, ring order and edge
// elements) with the PremulChain policy below; their placement rule and launch are chain_forms.hpp's.  The scale
// follows the same rule with a body of its own: element-aligned operands in one 16-B phase take the vector kernel,
// any other placement one coalesced element-wise kernel (correctness only, nobody has tuned it).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "chain_forms.hpp"
#include "dccl/dccl_reduce.h"
#include "scalar_arg.hpp"

namespace dccl_amd {
namespace {

// x * s with Prod's element semantics; 16-bit floats come back rounded to 16 bits.
template <typename T> struct PreMul {
    __device__ __forceinline__ static T apply(T x, T s) { return Combine<T, kProd>::apply(x, s); }
};
template <> struct PreMul<float> {
    __device__ __forceinline__ static float apply(float x, float s) {
#pragma clang fp contract(off)
        return x * s;
    }
};
template <> struct PreMul<double> {
    __device__ __forceinline__ static double apply(double x, double s) {
#pragma clang fp contract(off)
        return x * s;
    }
};

// The 16-bit floats need the switch too: the compiler narrows widen-multiply-round to one f16 multiply (the
// same bits), does the same to the Sum, and then contracts the pair into v_fma_f16 / v_pk_fma_f16.
template <> struct PreMul<f16_bits> {
    __device__ __forceinline__ static f16_bits apply(f16_bits x, f16_bits s) {
#pragma clang fp contract(off)
        return f16_bits{f32_to_f16(f16_to_f32(x.v) * f16_to_f32(s.v))};
    }
};
template <> struct PreMul<bf16_bits> {
    __device__ __forceinline__ static bf16_bits apply(bf16_bits x, bf16_bits s) {
#pragma clang fp contract(off)
        return bf16_bits{f32_to_bf16(bf16_to_f32(x.v) * bf16_to_f32(s.v))};
    }
};

template <typename T>
__device__ __forceinline__ u32x4 premul16(u32x4 v, T s) {
    Pack<T> p = __builtin_bit_cast(Pack<T>, v);
#pragma unroll
    for (int i = 0; i < Pack<T>::N; ++i) p.e[i] = PreMul<T>::apply(p.e[i], s);
    return __builtin_bit_cast(u32x4, p);
}

// The chain policy (reduce_kernels.hpp chain_vec_body): every operand is multiplied by s as it enters the Sum.
template <typename T>
struct PremulChain {
    using Elem = T;
    T s;
    __device__ __forceinline__ u32x4 first16(u32x4 v) const { return premul16<T>(v, s); }
    __device__ __forceinline__ u32x4 fold16(u32x4 v, u32x4 acc) const {
        return combine16<T, kSum>(premul16<T>(v, s), acc);
    }
    __device__ __forceinline__ u32x4 finish16(u32x4 acc) const { return acc; }
    __device__ __forceinline__ T first(T x) const { return PreMul<T>::apply(x, s); }
    __device__ __forceinline__ T fold(T x, T acc) const { return Combine<T, kSum>::apply(PreMul<T>::apply(x, s), acc); }
    __device__ __forceinline__ T finish(T acc) const { return acc; }
};

// ---- scale ----
template <typename T>
__global__ __launch_bounds__(64) void scale_vec_kernel(const unsigned char* src, unsigned char* dst, size_t head,
                                                       size_t nvec, size_t tail, ScalarArg sa) {
    const T s = load_scalar<T>(sa);
    const u32x4* vs = reinterpret_cast<const u32x4*>(src + head * sizeof(T));
    u32x4* vd = reinterpret_cast<u32x4*>(dst + head * sizeof(T));
    const size_t ntiles = (nvec + 63) / 64;
    for (size_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const size_t i = t * 64 + threadIdx.x;
        if (i < nvec) __builtin_nontemporal_store(premul16<T>(ld16<true>(vs + i), s), vd + i);
    }
    if (blockIdx.x == 0)
        for (size_t j = threadIdx.x; j < head + tail; j += blockDim.x) {
            const size_t i = edge_index<T>(j, head, nvec);
            st_elem<T, true>(dst, i, PreMul<T>::apply(ld_elem<T, true>(src, i), s));
        }
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void scale_elem_kernel(const unsigned char* src, unsigned char* dst, size_t count,
                                                            ScalarArg sa) {
    const T s = load_scalar<T>(sa);
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += size_t(gridDim.x) * kBlock)
        st_elem<T, ALIGNED>(dst, i, PreMul<T>::apply(ld_elem<T, ALIGNED>(src, i), s));
}

// ---- fused chain: reduce_chain_vec_kernel's roles and order, every operand pre-multiplied ----
template <typename T, int K, typename C>
__global__ __launch_bounds__(C::BLOCK) void premul_chain_vec_kernel(SendList sends, const unsigned char* own,
                                                                    unsigned char* dst, size_t head, size_t nvec,
                                                                    size_t tail, ScalarArg sa) {
    chain_vec_body<PremulChain<T>, K, C>(sends, own, dst, head, nvec, tail, PremulChain<T>{load_scalar<T>(sa)});
}

// Any placement, one element per thread and step (correctness only).
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void premul_chain_elem_kernel(SendList sends, int nsend, const unsigned char* own,
                                                                   unsigned char* dst, size_t count, ScalarArg sa) {
    chain_elem_body<PremulChain<T>, ALIGNED>(sends, nsend, own, dst, count, PremulChain<T>{load_scalar<T>(sa)});
}

// ---- launches ----
template <typename T>
int scale_typed(const void* src, void* dst, size_t count, ScalarArg sa, hipStream_t stream) {
    auto s = static_cast<const unsigned char*>(src);
    auto d = static_cast<unsigned char*>(dst);
    // chain_forms.hpp place_pass: dst leads, to its 128-B lines; src (same element size) must share its 16-B phase
    PassPlacement p = place_pass(reinterpret_cast<uintptr_t>(dst), sizeof(T), reinterpret_cast<uintptr_t>(src),
                                 sizeof(T), count, kDstAlign);
    if (!p.vec_ok) {
        void* args[] = {&s, &d, &count, &sa};
        const void* fn = !p.elem_ok ? reinterpret_cast<const void*>(&scale_elem_kernel<T, false>)
                                    : reinterpret_cast<const void*>(&scale_elem_kernel<T, true>);
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    Split& sp = p.sp;
    void* args[] = {&s, &d, &sp.head, &sp.nvec, &sp.tail, &sa};
    return launch(reinterpret_cast<const void*>(&scale_vec_kernel<T>), grid_for(sp, 64), args, stream, 64);
}

struct PremulChainKernels {  // chain_forms.hpp launch_chain_form
    template <typename T, int K>
    static const void* vec() { return reinterpret_cast<const void*>(&premul_chain_vec_kernel<T, K, DefaultCfg>); }
    template <typename T, bool ALIGNED>
    static const void* elem() { return reinterpret_cast<const void*>(&premul_chain_elem_kernel<T, ALIGNED>); }
};

// dispatch.hpp's dtype switch (its op parameter is unused here: callers pass kSum)
struct ScaleFn {
    template <typename T, int OP>
    static int run(const void* src, void* dst, size_t count, ScalarArg sa, hipStream_t stream) {
        return scale_typed<T>(src, dst, count, sa, stream);
    }
};
struct PremulChainFn {
    template <typename T, int OP>
    static int run(const void* const* sends, int nsend, const void* own, void* dst, size_t count, ScalarArg sa,
                   hipStream_t stream) {
        return launch_chain_form<PremulChainKernels, T>(sends, nsend, own, dst, count, stream, sa);
    }
};

}  // namespace
}  // namespace dccl_amd

using namespace dccl_amd;

extern "C" int dccl_local_scale(const void* src, void* dst, int dtype, size_t count, const void* scalar, int residence,
                                void* stream) {
    if (size_of_dtype(dtype) == 0) return DCCL_INVALID_ARGUMENT;
    if (!scalar_ok(scalar, residence)) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (src == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    if (partial_overlap(src, dst, count * size_of_dtype(dtype))) return DCCL_INVALID_ARGUMENT;
    return dispatch<ScaleFn>(dtype, kSum, src, dst, count, make_scalar(scalar, residence, size_of_dtype(dtype)),
                             static_cast<hipStream_t>(stream));
}

extern "C" int dccl_local_reduce_chain_premul(const void* const* sends, int nsend, const void* own, void* dst,
                                              int dtype, size_t count, const void* scalar, int residence,
                                              void* stream) {
    if (size_of_dtype(dtype) == 0) return DCCL_INVALID_ARGUMENT;
    if (!scalar_ok(scalar, residence)) return DCCL_INVALID_ARGUMENT;  // the same code as a bad nsend, before count == 0
    const int rc = check_chain_args(sends, nsend, own, dst, count * size_of_dtype(dtype));
    if (rc != DCCL_SUCCESS || count == 0) return rc;
    return dispatch<PremulChainFn>(dtype, kSum, sends, nsend, own, dst, count,
                                   make_scalar(scalar, residence, size_of_dtype(dtype)),
                                   static_cast<hipStream_t>(stream));
}
