// dccl_amd/csrc/rows_map.hpp — the tile -> (segment, row, tile-in-row) map of the batched strided row copy
// (copy_rows_kernel, copy_rows.hip; dccl_copy_rows_multi) and the exact overlap test of its validation.
// No HIP include, like tile_maps.hpp: the kernel and its launcher include it, tests/test_group_plan.py compiles
// it with g++ and checks the map exhaustively.
//
// A segment is `rows` rows of row_bytes bytes.  A row is cut into tiles of 64 16-B vectors of the DESTINATION's
// aligned body; where that body starts depends on the row's address, so the tile count per row is the bound
// that holds for every alignment: row_bytes / 16 + 1 vectors (at least one tile for a non-empty row: tile 0 also
// writes the row's head and tail bytes).  Segment i owns the tile indices [pre[i], pre[i + 1]), row-major.
#pragma once

#include <cstddef>
#include <cstdint>

#include "tile_maps.hpp"

namespace dccl_amd {

constexpr int kRowsMaxSegs = 32;
constexpr size_t kRowsTileVecs = 64;  // one wave, one 16-B vector per lane

DCCL_TILE_FN size_t rows_tiles_per_row(size_t row_bytes) {
    return row_bytes == 0 ? 0 : (row_bytes / 16 + 1 + kRowsTileVecs - 1) / kRowsTileVecs;
}

struct RowTile {
    int seg;
    size_t row, tile;
};

// Tile t < pre[nsegs] of a batch whose segment i has rows * rows_tiles_per_row(row_bytes[i]) tiles.  A scan over
// at most 32 prefix sums, uniform for a wave when t is; segments without tiles are passed over.
DCCL_TILE_FN RowTile rows_locate(const size_t* pre, const size_t* row_bytes, int nsegs, size_t t) {
    int i = 0;
    while (i + 1 < nsegs && t >= pre[i + 1]) ++i;
    const size_t local = t - pre[i], tpr = rows_tiles_per_row(row_bytes[i]);
    return RowTile{i, local / tpr, local % tpr};
}

// Fills pre[0..nsegs] and returns the batch's tile count.
inline size_t rows_prefix(const size_t* row_bytes, int nsegs, size_t rows, size_t* pre) {
    pre[0] = 0;
    for (int i = 0; i < nsegs; ++i) pre[i + 1] = pre[i] + rows * rows_tiles_per_row(row_bytes[i]);
    return pre[nsegs];
}

// The byte set of one side of a segment: rows intervals [base + r * stride, + len), r < rows.
struct RowSet {
    uintptr_t base;
    size_t len, stride, rows;
};

// True when the two sets share a byte.  Exact, not by bounding box: the destinations of a pack interleave by
// design.  Sets of one row, or of equal strides, are decided in closed form; two multi-row sets of different
// strides whose bounding boxes meet are swept row by row over the set with fewer rows inside the other's box.
inline bool rows_share_byte(const RowSet& a, const RowSet& b) {
    typedef __int128 I;
    if (a.len == 0 || b.len == 0 || a.rows == 0 || b.rows == 0) return false;
    const I a0 = I(a.base), b0 = I(b.base);
    const I a1 = a0 + I(a.rows - 1) * I(a.stride) + I(a.len), b1 = b0 + I(b.rows - 1) * I(b.stride) + I(b.len);
    if (a1 <= b0 || b1 <= a0) return false;  // the boxes are apart
    auto floor_div = [](I x, I y) { return x / y - ((x % y != 0 && (x < 0) != (y < 0)) ? 1 : 0); };
    // does one interval [x, x + len) meet a row of set s?
    auto meets = [&](I x, I len, const RowSet& s) {
        const I s0 = I(s.base);
        if (s.rows == 1 || s.stride == 0) return x < s0 + I(s.len) && s0 < x + len;
        // the last row that starts below x + len: every earlier row also ends earlier, so it alone decides
        I r = floor_div(x + len - 1 - s0, I(s.stride));
        if (r < 0) return false;
        if (r > I(s.rows - 1)) r = I(s.rows - 1);
        return x < s0 + r * I(s.stride) + I(s.len);
    };
    if (a.rows == 1) return meets(a0, I(a.len), b);
    if (b.rows == 1) return meets(b0, I(b.len), a);
    if (a.stride == b.stride && a.stride > 0) {
        // rows ra, rb meet iff -a.len < (a0 - b0) - k * stride < b.len with k = rb - ra, |k| < rows
        const I s = I(a.stride), d = a0 - b0;
        // k in ((d - b.len) / s, (d + a.len) / s), open
        I lo = floor_div(d - I(b.len), s) + 1, hi = floor_div(d + I(a.len) - 1, s);
        const I kmin = -I(a.rows - 1), kmax = I(b.rows - 1);
        if (lo < kmin) lo = kmin;
        if (hi > kmax) hi = kmax;
        return lo <= hi;
    }
    // different strides: sweep the rows of one set that lie inside the other's box, whichever are fewer (the
    // cost of the test is that count; packs and unpacks never come here)
    auto in_box = [&](const RowSet& x, I x0, I y0, I y1, I* r0, I* r1) {
        *r0 = x.stride ? floor_div(y0 - x0 - I(x.len) + 1, I(x.stride)) : 0;
        *r1 = x.stride ? floor_div(y1 - 1 - x0, I(x.stride)) : 0;
        if (*r0 < 0) *r0 = 0;
        if (*r1 > I(x.rows - 1)) *r1 = I(x.rows - 1);
    };
    I ra0, ra1, rb0, rb1;
    in_box(a, a0, b0, b1, &ra0, &ra1);
    in_box(b, b0, a0, a1, &rb0, &rb1);
    if (ra1 - ra0 <= rb1 - rb0) {
        for (I r = ra0; r <= ra1; ++r)
            if (meets(a0 + r * I(a.stride), I(a.len), b)) return true;
    } else {
        for (I r = rb0; r <= rb1; ++r)
            if (meets(b0 + r * I(b.stride), I(b.len), a)) return true;
    }
    return false;
}

}  // namespace dccl_amd
