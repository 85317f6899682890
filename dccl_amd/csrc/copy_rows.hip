// dccl_amd/csrc/copy_rows.hip — the batched strided row copy of gfx950 (dccl_copy_rows_multi,
// include/dccl/dccl_reduce.h): the pack and the unpack of a coalesced group, one launch each.
//
// Segment i copies `rows` rows of row_bytes[i] bytes, row r from src[i] + r * src_stride[i] to
// dst[i] + r * dst_stride[i]; every segment in one launch.  Any byte alignment of either side.  The kernel is
// copy_multi_kernel's (local_reduce.hip) over a table of strided segments: one-wave blocks, each destination row
// walked in aligned 16-B vectors, a source at another 16-B phase read with the phased kernels' cross-lane funnel
// shift (ld_phased), head and tail bytes of a row written bytewise by the row's first tile, non-temporal loads
// and stores.  No LDS.  Roofline: HBM, 2 bytes moved per byte copied.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dccl/dccl_reduce.h"
#include "reduce_kernels.hpp"
#include "rows_map.hpp"

namespace dccl_amd {
namespace {

// The segment table, a plain struct kernel argument like CopyList / SendList (1.5 KiB of the 4 KiB limit).
struct RowsList {
    const unsigned char* src[kRowsMaxSegs];
    unsigned char* dst[kRowsMaxSegs];
    size_t row_bytes[kRowsMaxSegs], src_stride[kRowsMaxSegs], dst_stride[kRowsMaxSegs];
    size_t pre[kRowsMaxSegs + 1];  // tile prefix sums (rows_map.hpp)
};

// One-wave blocks stride over the batch's tiles; a tile is 64 aligned 16-B vectors of one destination row,
// found by a scan over the prefix sums that is uniform for the wave (rows_locate), so every lane reaches
// ld_phased's lane exchange.
__global__ __launch_bounds__(64) void copy_rows_kernel(RowsList rl, int nsegs) {
    const size_t total = rl.pre[nsegs];
    for (size_t t = blockIdx.x; t < total; t += gridDim.x) {  // uniform per wave
        const RowTile rt = rows_locate(rl.pre, rl.row_bytes, nsegs, t);
        const size_t bytes = rl.row_bytes[rt.seg];
        const unsigned char* s = rl.src[rt.seg] + rt.row * rl.src_stride[rt.seg];
        unsigned char* d = rl.dst[rt.seg] + rt.row * rl.dst_stride[rt.seg];
        size_t head = (16 - (reinterpret_cast<uintptr_t>(d) & 15)) & 15;
        if (head > bytes) head = bytes;
        const size_t nvec = (bytes - head) / 16;
        if (rt.tile * kRowsTileVecs < nvec) {  // uniform: rows_tiles_per_row bounds nvec for every alignment
            const unsigned p = unsigned((reinterpret_cast<uintptr_t>(s) + head) & 15);
            const size_t v = rt.tile * kRowsTileVecs + threadIdx.x;
            const u32x4 val = ld_phased(s + head, p, v, nvec);
            if (v < nvec) __builtin_nontemporal_store(val, reinterpret_cast<u32x4*>(d + head) + v);
        }
        if (rt.tile == 0) {
            for (size_t b = threadIdx.x; b < head; b += 64) d[b] = s[b];
            for (size_t b = head + nvec * 16 + threadIdx.x; b < bytes; b += 64) d[b] = s[b];
        }
    }
}

}  // namespace

// dccl_copy_rows_multi's launch without its validation: the coalesced groups of dccl_api.cpp, whose plans are
// disjoint by construction (group_plan.hpp).  1 <= nsegs <= 32, rows >= 1.  Hidden: not part of the ABI.
__attribute__((visibility("hidden"))) int copy_rows_launch(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows,
                                                           hipStream_t stream) {
    RowsList rl{};
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
    if (grid > cap) grid = cap;  // copy_multi_kernel's cap; the blocks stride
    void* args[] = {&rl, &nsegs};
    return hipLaunchKernel(reinterpret_cast<const void*>(&copy_rows_kernel), dim3(unsigned(grid)), dim3(64), args, 0,
                           stream) == hipSuccess
               ? DCCL_SUCCESS
               : DCCL_UNHANDLED_DEVICE_ERROR;
}

}  // namespace dccl_amd

using namespace dccl_amd;

extern "C" int dccl_copy_rows_check(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows) {
    if (nsegs < 0 || nsegs > kRowsMaxSegs || (nsegs > 0 && segs == nullptr) || rows == 0) return DCCL_INVALID_ARGUMENT;
    if (nsegs == 0) return DCCL_SUCCESS;
    for (int i = 0; i < nsegs; ++i)
        if (segs[i].row_bytes > 0 && (segs[i].src == nullptr || segs[i].dst == nullptr)) return DCCL_INVALID_ARGUMENT;
    if (rows > 1)
        for (int i = 0; i < nsegs; ++i)
            if (segs[i].src_stride < segs[i].row_bytes || segs[i].dst_stride < segs[i].row_bytes)
                return DCCL_INVALID_ARGUMENT;
    // no destination byte is a source byte or another destination's byte (exact: a pack's destinations interleave)
    for (int i = 0; i < nsegs; ++i) {
        const RowSet d{reinterpret_cast<uintptr_t>(segs[i].dst), segs[i].row_bytes, segs[i].dst_stride, rows};
        for (int j = 0; j < nsegs; ++j) {
            const RowSet s{reinterpret_cast<uintptr_t>(segs[j].src), segs[j].row_bytes, segs[j].src_stride, rows};
            if (rows_share_byte(d, s)) return DCCL_INVALID_ARGUMENT;
            if (j <= i) continue;
            const RowSet e{reinterpret_cast<uintptr_t>(segs[j].dst), segs[j].row_bytes, segs[j].dst_stride, rows};
            if (rows_share_byte(d, e)) return DCCL_INVALID_ARGUMENT;
        }
    }
    return DCCL_SUCCESS;
}

extern "C" int dccl_copy_rows_multi(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, void* stream) {
    const int v = dccl_copy_rows_check(segs, nsegs, rows);
    if (v != DCCL_SUCCESS || nsegs == 0) return v;
    return copy_rows_launch(segs, nsegs, rows, static_cast<hipStream_t>(stream));
}
