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
// The scalar travels as a kernel argument {bits, dev_ptr}: with dev_ptr set every wave loads it from device
// memory when it runs (stream-ordered, so a captured graph replays with the value of the moment); otherwise
// `bits` holds the value the host read at the call.  Every store is an ordinary vector store.
//
// Forms: operands that are element-aligned and share the destination's 16-B phase take the vector kernels
// (head scalars | 16-B non-temporal vectors | tail scalars; the chain under local_reduce.hip's chain caps).
// Any other placement (another phase, operands off element alignment) takes one coalesced element-wise
// kernel: that fallback is for correctness only, nobody has tuned it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "dccl/dccl_reduce.h"
#include "dispatch.hpp"
#include "reduce_kernels.hpp"

namespace dccl_amd {
namespace {

// local_reduce.hip's shipped shape: one-wave blocks, one 16-B vector per lane and operand, all non-temporal
using DefaultCfg = VecCfg<64, 1, kNtSend | kNtRecv | kNtStore, false>;
// the head scalars bring the destination to its 128-B lines (local_reduce.hip's default recv_align)
constexpr size_t kDstAlign = 128;

struct ScalarArg {
    uint64_t bits;        // the scalar's bytes (host-immediate residence)
    const void* dev_ptr;  // non-null: read the scalar here when the kernel runs (device residence)
};

template <typename T>
__device__ __forceinline__ T load_scalar(const ScalarArg& a) {
    if (a.dev_ptr != nullptr) return ld_elem<T, false>(static_cast<const unsigned char*>(a.dev_ptr), 0);
    T s;
    __builtin_memcpy(&s, &a.bits, sizeof(T));
    return s;
}

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

// index of block 0's j-th scalar element: head [0, head), then the tail past the vector body
template <typename T>
__device__ __forceinline__ size_t edge_index(size_t j, size_t head, size_t nvec) {
    return j < head ? j : head + nvec * Pack<T>::N + (j - head);
}

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
    static_assert(C::UNROLL == 1, "one vector per lane");
    const T sc = load_scalar<T>(sa);
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
            u32x4 acc = premul16<T>(s[0], sc);
#pragma unroll
            for (int k = 1; k < K; ++k) acc = combine16<T, kSum>(premul16<T>(s[k], sc), acc);
            __builtin_nontemporal_store(combine16<T, kSum>(premul16<T>(o, sc), acc), vd + i);
        }
    }
    if (blockIdx.x == 0)
        for (size_t j = threadIdx.x; j < head + tail; j += blockDim.x) {
            const size_t i = edge_index<T>(j, head, nvec);
            T acc = PreMul<T>::apply(ld_elem<T, true>(sends.p[0], i), sc);
#pragma unroll
            for (int k = 1; k < K; ++k)
                acc = Combine<T, kSum>::apply(PreMul<T>::apply(ld_elem<T, true>(sends.p[k], i), sc), acc);
            st_elem<T, true>(dst, i, Combine<T, kSum>::apply(PreMul<T>::apply(ld_elem<T, true>(own, i), sc), acc));
        }
}

// Any placement, one element per thread and step (correctness only).
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kBlock) void premul_chain_elem_kernel(SendList sends, int nsend, const unsigned char* own,
                                                                   unsigned char* dst, size_t count, ScalarArg sa) {
    const T sc = load_scalar<T>(sa);
    for (size_t i = size_t(blockIdx.x) * kBlock + threadIdx.x; i < count; i += size_t(gridDim.x) * kBlock) {
        T acc = PreMul<T>::apply(ld_elem<T, ALIGNED>(sends.p[0], i), sc);
        for (int k = 1; k < nsend; ++k)
            acc = Combine<T, kSum>::apply(PreMul<T>::apply(ld_elem<T, ALIGNED>(sends.p[k], i), sc), acc);
        st_elem<T, ALIGNED>(dst, i, Combine<T, kSum>::apply(PreMul<T>::apply(ld_elem<T, ALIGNED>(own, i), sc), acc));
    }
}

// ---- launches ----
template <typename T>
int scale_typed(const void* src, void* dst, size_t count, ScalarArg sa, hipStream_t stream) {
    auto s = static_cast<const unsigned char*>(src);
    auto d = static_cast<unsigned char*>(dst);
    const uintptr_t as = reinterpret_cast<uintptr_t>(src), ad = reinterpret_cast<uintptr_t>(dst);
    if (as % sizeof(T) || ad % sizeof(T) || ((as ^ ad) & 15)) {
        void* args[] = {&s, &d, &count, &sa};
        const void* fn = (as % sizeof(T) || ad % sizeof(T))
                             ? reinterpret_cast<const void*>(&scale_elem_kernel<T, false>)
                             : reinterpret_cast<const void*>(&scale_elem_kernel<T, true>);
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    Split sp = split_for_vectors<T>(ad, count, kDstAlign);
    size_t grid = ceil_div(sp.nvec, size_t(64));
    if (grid == 0 && (sp.head + sp.tail) > 0) grid = 1;
    void* args[] = {&s, &d, &sp.head, &sp.nvec, &sp.tail, &sa};
    return launch(reinterpret_cast<const void*>(&scale_vec_kernel<T>), grid, args, stream, 64);
}

template <typename T, int K>
int launch_premul_chain_vec(SendList sl, const unsigned char* own, unsigned char* d, Split sp, ScalarArg sa,
                            hipStream_t stream) {
    using C = DefaultCfg;
    size_t grid = ceil_div(sp.nvec, C::TILE);
    if (grid == 0 && (sp.head + sp.tail) > 0) grid = 1;
    void* args[] = {&sl, &own, &d, &sp.head, &sp.nvec, &sp.tail, &sa};
    // the plain chain's caps (launch_chain_vec): not measured for this kernel's heavier arithmetic
    return launch(reinterpret_cast<const void*>(&premul_chain_vec_kernel<T, K, C>), grid, args, stream, C::BLOCK,
                  caps::lds(caps::kChain, K, caps_bytes(sp.nvec * 16)));
}

template <typename T>
int premul_chain_typed(const void* const* sends, int nsend, const void* own, void* dst, size_t count, ScalarArg sa,
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
        void* args[] = {&sl, &nsend, &o, &d, &count, &sa};
        const void* fn = elem_ok ? reinterpret_cast<const void*>(&premul_chain_elem_kernel<T, true>)
                                 : reinterpret_cast<const void*>(&premul_chain_elem_kernel<T, false>);
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    const Split sp = split_for_vectors<T>(ad, count, kDstAlign);
    return with_k<1, 8>(nsend, [&](auto K) { return launch_premul_chain_vec<T, K.value>(sl, o, d, sp, sa, stream); });
}

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
        return premul_chain_typed<T>(sends, nsend, own, dst, count, sa, stream);
    }
};

bool scalar_ok(const void* scalar, int residence) { return scalar != nullptr && (residence == 0 || residence == 1); }

// residence 0: the device address itself; 1: the host value, read now
ScalarArg make_scalar(const void* scalar, int residence, int dtype) {
    ScalarArg sa{0, nullptr};
    if (residence == 0) sa.dev_ptr = scalar;
    else std::memcpy(&sa.bits, scalar, size_of_dtype(dtype));
    return sa;
}

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
    return dispatch<ScaleFn>(dtype, kSum, src, dst, count, make_scalar(scalar, residence, dtype),
                             static_cast<hipStream_t>(stream));
}

extern "C" int dccl_local_reduce_chain_premul(const void* const* sends, int nsend, const void* own, void* dst,
                                              int dtype, size_t count, const void* scalar, int residence,
                                              void* stream) {
    if (size_of_dtype(dtype) == 0) return DCCL_INVALID_ARGUMENT;
    if (nsend < 1 || nsend > 8 || sends == nullptr) return DCCL_INVALID_ARGUMENT;
    if (!scalar_ok(scalar, residence)) return DCCL_INVALID_ARGUMENT;
    if (count == 0) return DCCL_SUCCESS;
    if (own == nullptr || dst == nullptr) return DCCL_INVALID_ARGUMENT;
    for (int k = 0; k < nsend; ++k)
        if (sends[k] == nullptr) return DCCL_INVALID_ARGUMENT;
    if (sources_overlap_destination(sends, nsend, own, dst, count * size_of_dtype(dtype)))
        return DCCL_INVALID_ARGUMENT;
    return dispatch<PremulChainFn>(dtype, kSum, sends, nsend, own, dst, count, make_scalar(scalar, residence, dtype),
                                   static_cast<hipStream_t>(stream));
}
