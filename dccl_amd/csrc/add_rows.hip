// dccl_amd/csrc/add_rows.hip — the batched strided fp32 row accumulate of gfx950 (dccl_add_rows_f32_multi,
// include/dccl/dccl_reduce.h): the unpack of a coalesced run of widened sums with accumulate = 1, one launch for
// every tensor of the run.
//
// Segment i adds `rows` rows of row_bytes[i] / 4 fp32 elements, row r of src[i] + r * src_stride[i] into row r of
// dst[i] + r * dst_stride[i]: dst = dst + src, one IEEE fp32 add per element (round to nearest even, denormals kept),
// the add dccl_local_reduce_chain_widen applies for accumulate == 1.  The kernel is copy_rows_kernel's (copy_rows.hip)
// with a read of the destination and four adds in front of the store: one-wave blocks over rows_map.hpp's tiles, each
// destination row walked in aligned 16-B vectors, a source at another 16-B phase read with ld_phased, head and tail
// ELEMENTS of a row done by the row's first tile, non-temporal loads and stores.  A row whose destination is not
// 4-byte aligned has no aligned fp32 to walk: it takes the element-wise path, which assembles every fp32 from bytes
// (correctness only).  No LDS, no atomics.  Roofline: HBM, 12 bytes moved per element.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dccl/dccl_reduce.h"
#include "reduce_kernels.hpp"
#include "rows_map.hpp"

namespace dccl_amd {
namespace {

// copy_rows.hip's segment table: a plain struct kernel argument (1.5 KiB of the 4 KiB limit).
struct AddRowsList {
    const unsigned char* src[kRowsMaxSegs];
    unsigned char* dst[kRowsMaxSegs];
    size_t row_bytes[kRowsMaxSegs], src_stride[kRowsMaxSegs], dst_stride[kRowsMaxSegs];
    size_t pre[kRowsMaxSegs + 1];  // tile prefix sums (rows_map.hpp)
};

// dst[e] += src[e] for one element; the source at any byte address, the destination 4-byte aligned or (DA false) not.
template <bool DA>
__device__ __forceinline__ void add_elem(unsigned char* d, const unsigned char* s, size_t e) {
    st_elem<float, DA>(d, e, ld_elem<float, DA>(d, e) + ld_elem<float, false>(s, e));
}

// A tile is 64 aligned 16-B vectors of one destination row (rows_locate, uniform for the wave, so every lane
// reaches ld_phased's lane exchange).  rows_tiles_per_row bounds the vector count for every alignment, and four
// times it the element count, which is what the element-wise path cuts its tiles by.
__global__ __launch_bounds__(64) void add_rows_kernel(AddRowsList rl, int nsegs) {
    const size_t total = rl.pre[nsegs];
    for (size_t t = blockIdx.x; t < total; t += gridDim.x) {  // uniform per wave
        const RowTile rt = rows_locate(rl.pre, rl.row_bytes, nsegs, t);
        const size_t bytes = rl.row_bytes[rt.seg];
        const unsigned char* s = rl.src[rt.seg] + rt.row * rl.src_stride[rt.seg];
        unsigned char* d = rl.dst[rt.seg] + rt.row * rl.dst_stride[rt.seg];
        if ((reinterpret_cast<uintptr_t>(d) & 3) != 0) {  // uniform: this row's fp32 are assembled from bytes
            const size_t n = bytes / 4, end = (rt.tile + 1) * kRowsTileVecs * 4;
            for (size_t e = rt.tile * kRowsTileVecs * 4 + threadIdx.x; e < (end < n ? end : n); e += 64)
                add_elem<false>(d, s, e);
            continue;
        }
        size_t head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;  // 0, 4, 8 or 12
        if (head > bytes) head = bytes;
        const size_t nvec = (bytes - head) / 16;
        if (rt.tile * kRowsTileVecs < nvec) {  // uniform
            const unsigned p = unsigned((reinterpret_cast<uintptr_t>(s) + head) & 15);
            const size_t v = rt.tile * kRowsTileVecs + threadIdx.x;
            u32x4* vd = reinterpret_cast<u32x4*>(d + head);
            u32x4 acc = {0u, 0u, 0u, 0u};
            if (v < nvec) acc = ld16<true>(vd + v);
            const u32x4 val = ld_phased(s + head, p, v, nvec);
            if (v < nvec) __builtin_nontemporal_store(combine16<float, kSum>(acc, val), vd + v);
        }
        if (rt.tile == 0) {  // at most 3 head and 3 tail elements
            const size_t he = head / 4, te = (head + nvec * 16) / 4, n = bytes / 4;
            if (threadIdx.x < he) add_elem<true>(d, s, threadIdx.x);
            if (te + threadIdx.x < n) add_elem<true>(d, s, te + threadIdx.x);
        }
    }
}

}  // namespace

// dccl_add_rows_f32_multi's launch without its validation: the coalesced widened runs of dccl_api.cpp, whose plans
// are disjoint by construction (group_plan.hpp).  1 <= nsegs <= 32, rows >= 1, every row_bytes a multiple of 4.
// Hidden: not part of the ABI.  The grid cap is copy_rows_launch's.
__attribute__((visibility("hidden"))) int add_rows_launch(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows,
                                                          hipStream_t stream) {
    AddRowsList rl{};
    for (int i = 0; i < nsegs; ++i) {
        rl.src[i] = static_cast<const unsigned char*>(segs[i].src);
        rl.dst[i] = static_cast<unsigned char*>(segs[i].dst);
        rl.row_bytes[i] = segs[i].row_bytes;
        rl.src_stride[i] = segs[i].src_stride;
        rl.dst_stride[i] = segs[i].dst_stride;
    }
    size_t grid = rows_prefix(rl.row_bytes, nsegs, rows, rl.pre);
    if (grid == 0) return DCCL_SUCCESS;  // nothing but empty rows
    const size_t cap = max_grid() < (size_t(1) << 20) ? max_grid() : size_t(1) << 20;
    if (grid > cap) grid = cap;  // the blocks stride
    void* args[] = {&rl, &nsegs};
    return hipLaunchKernel(reinterpret_cast<const void*>(&add_rows_kernel), dim3(unsigned(grid)), dim3(64), args, 0,
                           stream) == hipSuccess
               ? DCCL_SUCCESS
               : DCCL_UNHANDLED_DEVICE_ERROR;
}

}  // namespace dccl_amd

using namespace dccl_amd;

extern "C" int dccl_add_rows_f32_multi(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, void* stream) {
    const int v = dccl_copy_rows_check(segs, nsegs, rows);
    if (v != DCCL_SUCCESS || nsegs == 0) return v;
    for (int i = 0; i < nsegs; ++i)
        if (segs[i].row_bytes % 4 != 0) return DCCL_INVALID_ARGUMENT;
    return add_rows_launch(segs, nsegs, rows, static_cast<hipStream_t>(stream));
}
