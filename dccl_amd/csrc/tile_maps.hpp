// dccl_amd/csrc/tile_maps.hpp — the block -> tile maps of the combine kernels and the grids they need.
// No HIP include: reduce_kernels.hpp includes it for the kernels, tests/test_tile_maps.py compiles it with g++
// and checks every map exhaustively (bijections, strided coverage, tile_order against first_tile).
#pragma once

#include <cstddef>
#include <cstdlib>

#if defined(__HIPCC__)
#define DCCL_TILE_FN __host__ __device__ __forceinline__
#else
#define DCCL_TILE_FN inline
#endif

namespace dccl_amd {

constexpr size_t kMaxGrid = size_t(1) << 24;  // grid-stride beyond this (2^24 x 64 threads)

// DCCL_MAX_GRID_TEST as a grid clamp: a decimal integer that is a multiple of 8 from 8 to kMaxGrid, nothing after
// it; anything else (null, empty, trailing characters, 0, 4, 12, 100, kMaxGrid + 8) is kMaxGrid.
inline size_t parse_max_grid(const char* e) {
    if (e == nullptr || *e < '0' || *e > '9') return kMaxGrid;
    char* end = nullptr;
    const unsigned long long x = std::strtoull(e, &end, 10);
    return (*end == '\0' && x >= 8 && x <= kMaxGrid && x % 8 == 0) ? size_t(x) : kMaxGrid;
}
// Test-only clamp of every combine and copy launch: DCCL_MAX_GRID_TEST = G, read once per process, makes launch()
// (reduce_kernels.hpp) clamp its grid at G blocks instead of kMaxGrid, and dccl_copy_multi / copy_rows_launch at
// min(2^20, G), so tests/test_gpu_grid_stride_small.py runs every kernel's second and later grid-stride passes
// with operands of about 312 KiB instead of 16 GiB.  Unset, max_grid() is kMaxGrid.
inline size_t max_grid() {
    static const size_t g = parse_max_grid(std::getenv("DCCL_MAX_GRID_TEST"));
    return g;
}

// Bijective XCD-aware remap (cdna_hip_programming.md, "XCD swizzle must be bijective"):
// blocks b and b+8 share an XCD, so give each group {b : b % 8 == x} one contiguous range.
DCCL_TILE_FN size_t xcd_remap(size_t b, size_t nb) {
    const size_t q = nb / 8, r = nb % 8, x = b % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// Tile-run order: in every full group of 8 RUN blocks, block 8 RUN q + r (XCD r % 8 under the round-robin
// dispatch) takes tile 8 RUN q + RUN (r % 8) + r / 8, so each XCD walks RUN consecutive tiles of the group
// while the groups sweep the range in order: a line two neighbouring tiles share is fetched by one L2 in
// RUN - 1 of RUN cases.  RUN 1 is block order, RUN 8 the group-interleaved order (xcd_group_tile).  A partial
// last group keeps the identity.  Bijective on [0, nb).
template <int RUN>
DCCL_TILE_FN size_t run_tile(size_t b, size_t nb) {
    if constexpr (RUN == 1) return b;
    constexpr size_t span = size_t(8) * RUN;
    const size_t q = b / span, r = b % span;
    return (q + 1) * span > nb ? b : q * span + (r % 8) * RUN + r / 8;
}
DCCL_TILE_FN size_t xcd_group_tile(size_t b, size_t nb) { return run_tile<8>(b, nb); }

// First tile of block b of a g-block grid (g a multiple of 8) for the misaligned-destination kernels, by a
// uniform runtime `order`: kOrderXcd gives each XCD one contiguous range (consecutive tiles on one XCD: the
// line two tiles share meets in one L2), kOrderBlock is block order, kOrderGroup the group-interleaved order
// above (one front for the chip, 7 of 8 tile boundaries inside one XCD).  Computed once per block.
enum : int { kOrderXcd = 0, kOrderBlock = 1, kOrderGroup = 2, kOrderRun4 = 3, kOrderRun2 = 4 };
DCCL_TILE_FN size_t tile_order(int order, size_t b, size_t g) {
    return order == kOrderXcd     ? (b % 8) * (g / 8) + b / 8
           : order == kOrderBlock ? b
           : order == kOrderRun4  ? run_tile<4>(b, g)
           : order == kOrderRun2  ? run_tile<2>(b, g)
                                  : xcd_group_tile(b, g);
}

// The same map with the order as a template parameter (reduce_windows_kernel).
template <int ORDER>
DCCL_TILE_FN size_t first_tile(size_t b, size_t g) {
    if constexpr (ORDER == kOrderXcd) return (b % 8) * (g / 8) + b / 8;
    else if constexpr (ORDER == kOrderBlock) return b;
    else if constexpr (ORDER == kOrderRun4) return run_tile<4>(b, g);
    else if constexpr (ORDER == kOrderRun2) return run_tile<2>(b, g);
    else return xcd_group_tile(b, g);
}

// One-wave blocks for nvec 16-B vectors, rounded up to a multiple of 8 and at least 8 (the XCD / group tile
// maps above need one); max_grid(), where launch() clamps it, is a multiple of 8 too (kMaxGrid, or the test clamp).
inline size_t unaligned_grid(size_t nvec) {
    const size_t g = ((nvec + 63) / 64 + 7) / 8 * 8;
    return g == 0 ? 8 : g;
}

}  // namespace dccl_amd
