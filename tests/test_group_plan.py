"""The plan of a coalesced group (dccl_amd/csrc/group_plan.hpp) and the tile map of its pack / unpack kernel
(dccl_amd/csrc/rows_map.hpp), on the CPU: both headers have no HIP include, so g++ compiles them into one harness
(as tests/test_tile_maps.py does for the combine kernels' maps).  Then the layout itself, in numpy: packing
slot-major, running ONE simulated collective and unpacking gives the per-tensor collectives' bytes for the ring,
the reduce-scatter ring and Rabenseifner, with the oracle as the combine."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
from tests import rabsim, ringsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dccl_amd", "csrc")

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "group_plan.hpp"
#include "rows_map.hpp"
using namespace dccl_amd;

// runs: stdin holds "max_bytes n" and n lines "api comm count esz dtype op root device world"
static int do_runs() {
    unsigned long long max_bytes, n;
    if (std::scanf("%llu %llu", &max_bytes, &n) != 2) return 2;
    std::vector<group::Call> calls(n);
    for (auto& c : calls) {
        unsigned long long comm, count, esz;
        int dev;
        unsigned world;
        if (std::scanf("%d %llu %llu %llu %d %d %d %d %u", &c.api, &comm, &count, &esz, &c.dtype, &c.op, &c.root, &dev,
                       &world) != 9)
            return 2;
        c.comm = reinterpret_cast<const void*>(uintptr_t(comm));
        c.count = count, c.esz = esz, c.device = dev != 0, c.world = world;
    }
    const auto runs = group::plan_runs(calls.data(), calls.size(), max_bytes);
    std::printf("[");
    for (size_t i = 0; i < runs.size(); ++i)
        std::printf("%s[%zu, %zu, %d]", i ? ", " : "", runs[i].first, runs[i].n, int(runs[i].packed));
    std::printf("]\n");
    return 0;
}

// layout W P esz: the issue's five tensors; prints the layout and checks (tensor, slot) -> bytes is injective
static int do_layout(size_t W, size_t P, size_t esz) {
    const size_t mult[] = {1, 5, 77, 1000, 4099};
    group::Call calls[5];
    for (int i = 0; i < 5; ++i) calls[i].count = P * mult[i], calls[i].esz = esz, calls[i].world = uint32_t(W);
    const group::Layout L = group::pack_layout(calls, 5, P);
    std::vector<unsigned char> seen(P * L.S, 0);
    bool injective = true, inside = true;
    for (int i = 0; i < 5; ++i)
        for (size_t k = 0; k < P; ++k)
            for (size_t b = 0; b < L.slot[i]; ++b) {
                const size_t at = k * L.S + L.off[i] + b;
                if (at >= seen.size()) { inside = false; continue; }
                if (seen[at]) injective = false;
                seen[at] = 1;
            }
    std::printf("{\"S\": %zu, \"count\": %zu, \"slots_ring\": %zu, \"slots_rab\": %zu, \"injective\": %s, \"inside\": %s, "
                "\"slot\": [%zu, %zu, %zu, %zu, %zu], \"off\": [%zu, %zu, %zu, %zu, %zu]}\n",
                L.S, L.count, group::slots_of(uint32_t(W), false), group::slots_of(uint32_t(W), true),
                injective ? "true" : "false", inside ? "true" : "false", L.slot[0], L.slot[1], L.slot[2], L.slot[3],
                L.slot[4], L.off[0], L.off[1], L.off[2], L.off[3], L.off[4]);
    return 0;
}

// the kernel's walk over one batch: every (segment, row, tile) exactly once at several grids, and every byte of a
// row exactly once at every destination alignment
static std::string check_batch(const std::vector<size_t>& row_bytes, size_t rows) {
    const int nsegs = int(row_bytes.size());
    size_t pre[kRowsMaxSegs + 1];
    const size_t total = rows_prefix(row_bytes.data(), nsegs, rows, pre);
    size_t want = 0;
    for (size_t b : row_bytes) want += rows * rows_tiles_per_row(b);
    if (total != want) return "total";
    for (size_t grid : {size_t(1), size_t(7), total, total + 5}) {
        if (grid == 0) continue;
        std::vector<std::vector<unsigned char>> seen(nsegs);
        for (int i = 0; i < nsegs; ++i) seen[i].assign(rows * rows_tiles_per_row(row_bytes[i]), 0);
        size_t visits = 0;
        for (size_t b = 0; b < grid; ++b)
            for (size_t t = b; t < total; t += grid) {
                const RowTile rt = rows_locate(pre, row_bytes.data(), nsegs, t);
                if (rt.seg < 0 || rt.seg >= nsegs) return "seg";
                const size_t tpr = rows_tiles_per_row(row_bytes[rt.seg]);
                if (tpr == 0 || rt.row >= rows || rt.tile >= tpr) return "range";
                unsigned char& s = seen[rt.seg][rt.row * tpr + rt.tile];
                if (s) return "twice";
                s = 1;
                ++visits;
            }
        if (visits != total) return "visits";
    }
    for (size_t bytes : row_bytes)
        for (size_t a = 0; a < 16; ++a) {  // the destination row's address modulo 16
            std::vector<int> hit(bytes, 0);
            size_t head = (16 - a) & 15;
            if (head > bytes) head = bytes;
            const size_t nvec = (bytes - head) / 16;
            for (size_t tile = 0; tile < rows_tiles_per_row(bytes); ++tile) {
                for (size_t v = tile * kRowsTileVecs; v < (tile + 1) * kRowsTileVecs && v < nvec; ++v)
                    for (size_t b = 0; b < 16; ++b) ++hit[head + v * 16 + b];
                if (tile == 0) {
                    for (size_t b = 0; b < head; ++b) ++hit[b];
                    for (size_t b = head + nvec * 16; b < bytes; ++b) ++hit[b];
                }
            }
            for (int h : hit)
                if (h != 1) return "bytes";
        }
    return "";
}

static int do_map() {
    const size_t sizes[] = {0, 1, 15, 16, 17, 1023, 1024, 1025, 64 * 16 + 1, 64 * 16 * 3, 2 * 4099};
    long n = 0;
    std::string fail;
    for (size_t rows : {size_t(1), size_t(3), size_t(8)}) {
        std::vector<std::vector<size_t>> batches;
        for (size_t s : sizes) batches.push_back({s});
        batches.push_back(std::vector<size_t>(sizes, sizes + sizeof sizes / sizeof sizes[0]));
        std::vector<size_t> full;
        for (int i = 0; i < kRowsMaxSegs; ++i) full.push_back(sizes[(i * 7 + 3) % (sizeof sizes / sizeof sizes[0])]);
        batches.push_back(full);
        batches.push_back({0, 0, 17, 0});
        batches.push_back({17, 0, 0});
        for (const auto& b : batches) {
            const std::string f = check_batch(b, rows);
            ++n;
            if (!f.empty() && fail.empty()) fail = f + " rows=" + std::to_string(rows) + " nsegs=" + std::to_string(b.size());
        }
    }
    std::printf("{\"ok\": %s, \"n\": %ld, \"fail\": \"%s\"}\n", fail.empty() ? "true" : "false", n, fail.c_str());
    return 0;
}

// rows_share_byte against a byte map, on small random sets
static int do_overlap() {
    unsigned long long x = 88172645463325252ull;
    auto rnd = [&](unsigned m) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return unsigned(x % m); };
    long n = 0, shared = 0;
    std::string fail;
    for (int trial = 0; trial < 200000 && fail.empty(); ++trial) {
        RowSet s[2];
        const bool same_stride = rnd(3) == 0;
        const size_t st = rnd(70);
        for (RowSet& r : s) {
            r.base = 1000 + rnd(300);
            r.len = rnd(40);
            r.rows = 1 + rnd(6);
            r.stride = same_stride ? st : rnd(70);
        }
        std::vector<unsigned char> map(4096, 0);
        for (size_t r = 0; r < s[0].rows; ++r)
            for (size_t b = 0; b < s[0].len; ++b) map[s[0].base + r * s[0].stride + b] = 1;
        bool want = false;
        for (size_t r = 0; r < s[1].rows; ++r)
            for (size_t b = 0; b < s[1].len; ++b) want = want || map[s[1].base + r * s[1].stride + b];
        ++n;
        shared += want;
        if (rows_share_byte(s[0], s[1]) != want || rows_share_byte(s[1], s[0]) != want) {
            char buf[256];
            std::snprintf(buf, sizeof buf, "a=(%zu,%zu,%zu,%zu) b=(%zu,%zu,%zu,%zu) want %d", size_t(s[0].base), s[0].len,
                          s[0].stride, s[0].rows, size_t(s[1].base), s[1].len, s[1].stride, s[1].rows, int(want));
            fail = buf;
        }
    }
    // far ends of the address space and 2^32 rows answer at once, without overflow
    const RowSet big{uintptr_t(1) << 62, 4096, 8192, size_t(1) << 32}, inter{(uintptr_t(1) << 62) + 4096, 4096, 8192, size_t(1) << 32};
    if (fail.empty() && rows_share_byte(big, inter)) fail = "interleaved 2^32 rows";
    const RowSet touch{(uintptr_t(1) << 62) + 4095, 4096, 8192, size_t(1) << 32};
    if (fail.empty() && !rows_share_byte(big, touch)) fail = "one shared byte, 2^32 rows";
    std::printf("{\"ok\": %s, \"n\": %ld, \"shared\": %ld, \"fail\": \"%s\"}\n", fail.empty() ? "true" : "false", n, shared,
                fail.c_str());
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    const std::string mode = argv[1];
    if (mode == "runs") return do_runs();
    if (mode == "layout" && argc == 5) return do_layout(std::atol(argv[2]), std::atol(argv[3]), std::atol(argv[4]));
    if (mode == "map") return do_map();
    if (mode == "overlap") return do_overlap();
    return 2;
}
"""

AR, RS, RED, AG, BC = 0, 1, 2, 3, 4
MIB = 1 << 20


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("group_plan")
    src, exe = d / "harness.cpp", d / "harness"
    src.write_text(HARNESS)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)], check=True)
    return str(exe)


def call(api=AR, count=4096, esz=4, dtype=7, op=0, root=0, device=1, world=4, comm=1):
    return (api, comm, count, esz, dtype, op, root, device, world)


def runs(harness, calls, max_bytes=MIB):
    text = f"{max_bytes} {len(calls)}\n" + "".join(" ".join(str(v) for v in c) + "\n" for c in calls)
    p = subprocess.run([harness, "runs"], input=text, capture_output=True, text=True, check=True, timeout=60)
    return [tuple(r) for r in json.loads(p.stdout)]


def test_runs_are_cut_where_the_key_changes(harness):
    assert runs(harness, [call()] * 5) == [(0, 5, 1)]
    assert runs(harness, [call()]) == [(0, 1, 0)]  # a one-tensor run is plain
    assert runs(harness, [call(), call(), call(api=RS), call(api=RS)]) == [(0, 2, 1), (2, 2, 1)]
    assert runs(harness, [call(), call(), call(dtype=9, esz=2), call()]) == [(0, 2, 1), (2, 1, 0), (3, 1, 0)]
    assert runs(harness, [call(), call(op=2), call(op=2), call(op=5)]) == [(0, 1, 0), (1, 2, 1), (3, 1, 0)]
    assert runs(harness, [call(), call(), call(device=0), call(device=0), call()]) == \
        [(0, 2, 1), (2, 1, 0), (3, 1, 0), (4, 1, 0)]  # host buffers are never packed
    assert runs(harness, [call(api=RED, root=0), call(api=RED, root=0), call(api=RED, root=1)]) == [(0, 2, 1), (2, 1, 0)]
    assert runs(harness, [call(root=0), call(root=3)]) == [(0, 2, 1)]  # the root only matters to ncclReduce
    assert runs(harness, [call(comm=1), call(comm=2), call(comm=2)]) == [(0, 1, 0), (1, 2, 1)]
    assert runs(harness, [call(api=AG)] * 3 + [call(api=BC)] * 2) == [(i, 1, 0) for i in range(5)]
    assert runs(harness, [call(world=1)] * 3) == [(i, 1, 0) for i in range(3)]  # W = 1 is a plain copy


def test_runs_are_cut_after_32_tensors_and_at_the_size_limit(harness):
    assert runs(harness, [call()] * 40) == [(0, 32, 1), (32, 8, 1)]
    assert runs(harness, [call()] * 33) == [(0, 32, 1), (32, 1, 0)]
    assert runs(harness, [call()] * 64) == [(0, 32, 1), (32, 32, 1)]
    big, edge, under = call(count=MIB), call(count=MIB // 4), call(count=MIB // 4 - 1)
    assert runs(harness, [call(), call(), big, call()]) == [(0, 2, 1), (2, 1, 0), (3, 1, 0)]
    assert runs(harness, [call(), edge, call(), under]) == [(0, 1, 0), (1, 1, 0), (2, 2, 1)]  # at the limit: never packed
    assert runs(harness, [call()] * 4, max_bytes=0) == [(i, 1, 0) for i in range(4)]  # DCCL_GROUP_COALESCE=0
    assert runs(harness, [call()] * 4, max_bytes=4096 * 4) == [(i, 1, 0) for i in range(4)]
    assert runs(harness, [call()] * 4, max_bytes=4096 * 4 + 1) == [(0, 4, 1)]


@pytest.mark.parametrize("W", [2, 3, 5, 8])
@pytest.mark.parametrize("esz", [4, 2])
def test_layout(harness, W, esz):
    pow2 = 1 << (W.bit_length() - 1)
    for P in {W, pow2}:
        p = subprocess.run([harness, "layout", str(W), str(P), str(esz)], capture_output=True, text=True, check=True,
                           timeout=60)
        L = json.loads(p.stdout)
        assert L["slots_ring"] == W and L["slots_rab"] == pow2
        assert L["slot"] == [m * esz for m in (1, 5, 77, 1000, 4099)]
        assert L["off"] == [sum(L["slot"][:i]) for i in range(5)]  # prefix sums
        assert L["S"] % 128 == 0 and 0 <= L["S"] - sum(L["slot"]) < 128
        assert L["count"] * esz == P * L["S"]
        assert L["injective"] and L["inside"]


def test_tile_map_covers_every_tile_and_byte_once(harness):
    p = subprocess.run([harness, "map"], capture_output=True, text=True, check=True, timeout=300)
    r = json.loads(p.stdout)
    assert r["ok"] and r["n"] > 30, r


def test_overlap_test_is_exact(harness):
    p = subprocess.run([harness, "overlap"], capture_output=True, text=True, check=True, timeout=300)
    r = json.loads(p.stdout)
    assert r["ok"], r
    assert 0.1 < r["shared"] / r["n"] < 0.9, r  # both answers are exercised


# ------------------------------------------------------------------------------------------------------------------
# Bit-identity of the layout, in numpy
# ------------------------------------------------------------------------------------------------------------------
MULTS = (1, 5, 77, 1000, 4099)


def make_inputs(W, P, dt, seed):
    """inputs[rank][tensor]: P * MULTS[tensor] elements."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(W):
        row = []
        for m in MULTS:
            x = rng.standard_normal(P * m).astype(np.float32)
            if dt == 9:  # bf16 travels as its bit pattern: the high half of a float32
                x = (x.view(np.uint32) >> 16).astype(np.uint16)
            row.append(x)
        out.append(row)
    return out


def plan_layout(harness, W, P, esz):
    """group_plan.hpp's pack_layout for the five tensors, from the compiled header: (slot, off, S) in ELEMENTS."""
    p = subprocess.run([harness, "layout", str(W), str(P), str(esz)], capture_output=True, text=True, check=True,
                       timeout=60)
    L = json.loads(p.stdout)
    assert all(v % esz == 0 for v in L["slot"] + L["off"] + [L["S"]])
    return [v // esz for v in L["slot"]], [v // esz for v in L["off"]], L["S"] // esz


def pack_by_plan(tensors, P, layout):
    """Pack as the plan says: tensor i's slot k goes to element k * S + off[i] of the packed buffer."""
    slot, off, S = layout
    packed = np.zeros(P * S, tensors[0].dtype)
    for t, n, o in zip(tensors, slot, off):
        assert t.size == P * n
        for k in range(P):
            packed[k * S + o:k * S + o + n] = t[k * n:(k + 1) * n]
    return packed


def unpack_by_plan(packed, P, layout):
    slot, off, S = layout
    return [np.concatenate([packed[k * S + o:k * S + o + n] for k in range(P)]) for n, o in zip(slot, off)]


def tensors_changed_by_concatenation(sim, inputs, alone, W):
    """How many of the five tensors plain concatenation (no slot-major order) changes on some rank."""
    cat = sim([np.concatenate(inputs[r]) for r in range(W)])
    changed, at = 0, 0
    for i in range(len(MULTS)):
        n = inputs[0][i].size
        changed += any(cat[r][at:at + n].tobytes() != alone[i][r].tobytes() for r in range(W))
        at += n
    return changed


def oracle_combine(dt, op=0):
    def combine(s, r):
        assert oracle.expected_reduce(np.ascontiguousarray(s), r, dt, op) == 0
    return combine


def copy(d, s):
    d[:] = s


@pytest.mark.parametrize("W", [3, 4, 8])
@pytest.mark.parametrize("dt", [7, 9])
def test_packed_ring_allreduce_is_bit_identical(harness, W, dt):
    esz = 4 if dt == 7 else 2
    layout = plan_layout(harness, W, W, esz)
    inputs = make_inputs(W, W, dt, 100 * W + dt)

    def sim(bufs):
        return ringsim.ring_allreduce(bufs, oracle_combine(dt), copy)

    alone = [sim([inputs[r][i].copy() for r in range(W)]) for i in range(len(MULTS))]
    bufs = sim([pack_by_plan(inputs[r], W, layout) for r in range(W)])
    for r in range(W):
        got = unpack_by_plan(bufs[r], W, layout)
        for i in range(len(MULTS)):
            assert got[i].tobytes() == alone[i][r].tobytes(), (r, i)
    if dt == 7:  # what the slot-major order is for: plain concatenation changes 4 to 5 of the 5 tensors (W >= 3)
        assert tensors_changed_by_concatenation(sim, inputs, alone, W) >= 4


@pytest.mark.parametrize("W", [3, 4, 8])
@pytest.mark.parametrize("dt", [7, 9])
def test_packed_reduce_scatter_ring_is_bit_identical(harness, W, dt):
    esz = 4 if dt == 7 else 2
    slot, off, S = layout = plan_layout(harness, W, W, esz)
    inputs = make_inputs(W, W, dt, 200 * W + dt)
    alone = [ringsim.reduce_scatter_ring([inputs[r][i].copy() for r in range(W)], oracle_combine(dt), *ringsim.rs_maps())
             for i in range(len(MULTS))]
    bufs = ringsim.reduce_scatter_ring([pack_by_plan(inputs[r], W, layout) for r in range(W)], oracle_combine(dt),
                                       *ringsim.rs_maps())
    for r in range(W):  # rank r ends with slot r of every tensor: its packed slot r, unpacked with rows = 1
        for i, (n, o) in enumerate(zip(slot, off)):
            got = bufs[r][r * S + o:r * S + o + n]
            assert got.tobytes() == alone[i][r][r * n:(r + 1) * n].tobytes(), (r, i)


@pytest.mark.parametrize("W", [3, 4, 8])
@pytest.mark.parametrize("dt", [7, 9])
def test_packed_rabenseifner_is_bit_identical(harness, W, dt):
    esz = 4 if dt == 7 else 2
    P = 1 << (W.bit_length() - 1)
    layout = plan_layout(harness, W, P, esz)
    inputs = make_inputs(W, P, dt, 300 * W + dt)

    def sim(bufs):
        return rabsim.rabenseifner_allreduce(bufs, oracle_combine(dt))

    alone = [sim([inputs[r][i].copy() for r in range(W)]) for i in range(len(MULTS))]
    bufs = sim([pack_by_plan(inputs[r], P, layout) for r in range(W)])
    for r in range(W):
        got = unpack_by_plan(bufs[r], P, layout)
        for i in range(len(MULTS)):
            assert got[i].tobytes() == alone[i][r].tobytes(), (r, i)
    # no concatenation check here: Rabenseifner pairs the same ranks in the same tree wherever an element lies, and
    # only the operand order of each combine depends on its position, which a commutative Sum does not show
