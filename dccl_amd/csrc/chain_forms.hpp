// dccl_amd/csrc/chain_forms.hpp — the host side of the extended chains (premul.hip, wide.hip): where the operands
// lie, and the one launch both take.  Operands that are element-aligned and share the destination's 16-B phase
// take the chain's vector kernel (head scalars | 16-B non-temporal vectors | tail scalars) under local_reduce.hip's
// chain caps, which nobody has measured for these kernels' heavier arithmetic and register use.  Any other placement
// (another phase, operands off element alignment) takes one coalesced element-wise kernel: that fallback is for
// correctness only, nobody has tuned it.
#pragma once

#include "dispatch.hpp"
#include "reduce_kernels.hpp"

namespace dccl_amd {

// KN names the kernels: KN::template vec<T, K>() and KN::template elem<T, ALIGNED>() give their addresses;
// `extra` is what they take after the chain's own arguments (the pre-multiplied chain's scalar).  Where the
// operands lie: classify (routing.hpp), the plain chain's classifier.
template <typename KN, typename T, typename... Extra>
int launch_chain_form(const void* const* sends, int nsend, const void* own, void* dst, size_t count,
                      hipStream_t stream, Extra... extra) {
    const Placement c = classify(sends, nsend, own, dst, sizeof(T));
    SendList sl = send_list(sends, nsend);
    auto o = static_cast<const unsigned char*>(own);
    auto d = static_cast<unsigned char*>(dst);
    if (!c.elem_ok || !c.in_phase()) {
        void* args[] = {&sl, &nsend, &o, &d, &count, &extra...};
        const void* fn = c.elem_ok ? KN::template elem<T, true>() : KN::template elem<T, false>();
        return launch(fn, ceil_div(count, size_t(kBlock)), args, stream, kBlock);
    }
    Split sp = split_for_vectors<T>(reinterpret_cast<uintptr_t>(dst), count, kDstAlign);
    void* args[] = {&sl, &o, &d, &sp.head, &sp.nvec, &sp.tail, &extra...};
    return with_k<1, 8>(nsend, [&](auto K) {
        return launch(KN::template vec<T, K.value>(), grid_for(sp, DefaultCfg::TILE), args, stream, DefaultCfg::BLOCK,
                      caps::lds(caps::kChain, K.value, caps_bytes(sp.nvec * 16)));
    });
}

// The placement rule of the one-source passes (premul.hip's scale, wide.hip's conversions).  `lead` is the side whose
// 16-B vectors the vector kernel walks (elements of `lead_size` bytes: the destination of a scale, the 16-bit side of
// a conversion), `other` the side it meets with elements of `other_size` bytes.  Head elements bring `lead` to an
// `align`-byte boundary (16 or more, a power of two); `other` must be on a 16-B boundary there too (vec_ok), else the
// element-wise kernel applies, ALIGNED when both sides are element-aligned (elem_ok).  `sp` counts in elements,
// 16 / lead_size of them per vector; it is meaningful when vec_ok.
struct PassPlacement {
    bool elem_ok, vec_ok;
    Split sp;
};
inline PassPlacement place_pass(uintptr_t lead, size_t lead_size, uintptr_t other, size_t other_size, size_t count,
                                size_t align = 16) {
    PassPlacement p{lead % lead_size == 0 && other % other_size == 0, false, {0, 0, 0}};
    if (!p.elem_ok) return p;
    size_t head = ((align - (lead & (align - 1))) & (align - 1)) / lead_size;
    p.vec_ok = ((other + head * other_size) & 15) == 0;
    if (head > count) head = count;
    const size_t nvec = (count - head) / (16 / lead_size);
    p.sp = Split{head, nvec, count - head - nvec * (16 / lead_size)};
    return p;
}

}  // namespace dccl_amd
