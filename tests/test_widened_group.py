"""Widened sums coalesced in groups: runs of same-handle dcclRedOpCreateWidenedSum reduce-scatters
and reduces inside ncclGroupStart / ncclGroupEnd are packed into one collective, and the batched fp32 row accumulate
(dccl_add_rows_f32_multi, include/dccl/dccl_reduce.h) unpacks a run whose handle accumulates.

Every comparison is on bits (0 ULP); no input holds a NaN, so NaN payloads never enter.

CPU: the planner with `out_esz` (g++ on group_plan.hpp), the two-element-size layout carried through the ring and
Rabenseifner simulations, the argument checks of dccl_add_rows_f32_multi, and the premise of the kernel test (the
expected sums differ from both operands).
GPU: the kernel against numpy over every row size / phase class with guard bytes, its grid-stride passes in a child
process, grouped against separate collectives on thread ranks (direct and ring), a mixed queue with and without
DCCL_GROUP_COALESCE=0, and one group across two IPC processes.
"""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rabsim, ringsim, xproc
from tests.test_caps import CSRC
from tests.test_group import run_ranks, stats_delta
from tests.test_wide_sum import BF16, DTS, ROOT, SEED, SUM, collective_inputs, widen
from tests.test_widened_sum import (_f32_add_into, assert_f32_bits, expected_slots, f32_add, plain_slots, prior_recv)

COUNTS = (1, 2, 3, 257, 515, 1031, 64)  # per-slot elements; fp32 output offsets mod 16: 0, 4, 12, 8, 12, 8, 4
RS, REDUCE = 1, 2                       # group::Api
WOP = 7                                 # a user-op handle


def _gxx(tmp_path, name, text):
    src, exe = tmp_path / f"{name}.cpp", tmp_path / name
    src.write_text(text)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True)
    return exe


# ------------------------------------------------------------------------------------------------------ CPU: the plan
PLAN_HARNESS = r"""
#include <cstdio>
#include <vector>
#include "group_plan.hpp"
using namespace dccl_amd;
int main() {
    unsigned long long max_bytes, n;
    if (std::scanf("%llu %llu", &max_bytes, &n) != 2) return 2;
    std::vector<group::Call> calls(n);
    static int comm;
    for (auto& c : calls) {
        unsigned long long count, out_esz;
        int never;
        if (std::scanf("%d %llu %d %d %llu", &c.api, &count, &c.op, &never, &out_esz) != 5) return 2;
        c.comm = &comm, c.count = count, c.esz = 2, c.dtype = 9, c.device = true, c.world = 4;
        c.never_packed = never != 0;
        c.out_esz = out_esz;
    }
    for (const group::Run& r : group::plan_runs(calls.data(), calls.size(), max_bytes))
        std::printf("%zu %zu %d\n", r.first, r.n, int(r.packed));
}
"""


def test_group_plan_packs_same_handle_widened_calls_cpu(tmp_path):
    """Same-handle widened reduce-scatters (never_packed false, out_esz 4) form one packed run; two op values form
    two; a widened and a plain call of one dtype never share a run; the packing limit is on the 16-bit bytes; with
    never_packed set the answers of tests/test_widened_sum.py come back."""
    exe = _gxx(tmp_path, "plan", PLAN_HARNESS)

    def runs(queue, max_bytes=1 << 20):
        text = f"{max_bytes} {len(queue)}\n" + "\n".join(" ".join(map(str, map(int, q))) for q in queue)
        out = subprocess.run([str(exe)], input=text + "\n", check=True, capture_output=True, text=True).stdout
        return [tuple(map(int, l.split())) for l in out.splitlines()]

    plain, wid, other = (RS, 4096, SUM, 0, 0), (RS, 4096, WOP, 0, 4), (RS, 4096, WOP + 1, 0, 4)
    never = (RS, 4096, WOP, 1, 4)
    assert runs([wid] * 3) == [(0, 3, 1)]
    assert runs([wid, wid, other, other, other]) == [(0, 2, 1), (2, 3, 1)]
    assert runs([wid, other, wid]) == [(0, 1, 0), (1, 1, 0), (2, 1, 0)]
    assert runs([wid, plain]) == [(0, 1, 0), (1, 1, 0)]
    assert runs([plain, plain, wid, wid, plain]) == [(0, 2, 1), (2, 2, 1), (4, 1, 0)]
    # the mixed queue of the GPU test: [acc0, acc0, acc1, acc1, SUM, SUM, acc0]
    assert runs([wid, wid, other, other, plain, plain, wid]) == [(0, 2, 1), (2, 2, 1), (4, 2, 1), (6, 1, 0)]
    # a reduce and a reduce-scatter of one handle, and reduces to two roots, stay apart (same_run, unchanged)
    assert runs([wid, (REDUCE, 4096, WOP, 0, 4), (REDUCE, 4096, WOP, 0, 4)]) == [(0, 1, 0), (1, 2, 1)]
    # the limit compares count * esz, the 16-bit bytes: 2 * 262144 = 512 KiB passes a 1 MiB limit, 524288 does not
    assert runs([(RS, 262144, WOP, 0, 4)] * 2) == [(0, 2, 1)]
    assert runs([(RS, 524288, WOP, 0, 4)] * 2) == [(0, 1, 0), (1, 1, 0)]
    assert runs([wid] * 3, 0) == [(0, 1, 0), (1, 1, 0), (2, 1, 0)]
    assert runs([wid] * 40) == [(0, 32, 1), (32, 8, 1)]
    # never_packed wins as before
    assert runs([never] * 3) == [(0, 1, 0), (1, 1, 0), (2, 1, 0)]
    assert runs([plain, plain, never, never, plain, plain, plain, never]) == [(0, 2, 1), (2, 1, 0), (3, 1, 0),
                                                                              (4, 3, 1), (7, 1, 0)]
    assert runs([wid, never, wid, wid]) == [(0, 1, 0), (1, 1, 0), (2, 2, 1)]


# ---------------------------------------------------------------------------------------------------- CPU: the layout
LAYOUT_HARNESS = r"""
#include <cstdio>
#include <vector>
#include "group_plan.hpp"
using namespace dccl_amd;
int main() {
    unsigned long long P, n, esz, out_esz;
    if (std::scanf("%llu %llu %llu %llu", &P, &n, &esz, &out_esz) != 4 || n > group::kMaxRun) return 2;
    std::vector<group::Call> calls(n);
    for (auto& c : calls) {
        unsigned long long count;
        if (std::scanf("%llu", &count) != 1) return 2;
        c.count = count, c.esz = esz, c.out_esz = out_esz;
    }
    const group::Layout L = group::pack_layout(calls.data(), n, P);
    std::printf("%zu %zu %zu\n", L.S, L.S_out, L.count);
    for (size_t i = 0; i < n; ++i) std::printf("%zu %zu %zu %zu\n", L.off[i], L.slot[i], L.out_off[i], L.out_slot[i]);
}
"""


def _layout(exe, P, counts, esz, out_esz):
    text = f"{P} {len(counts)} {esz} {out_esz}\n" + " ".join(str(c) for c in counts) + "\n"
    rows = [tuple(map(int, l.split())) for l in
            subprocess.run([str(exe)], input=text, check=True, capture_output=True, text=True).stdout.splitlines()]
    return rows[0], rows[1:]


def test_layout_with_two_element_sizes_keeps_every_tensors_bits_cpu(tmp_path):
    """bf16 inputs packed by the header's input numbers and widened, the fp32 ring reduce-scatter (P = W = 3, 4, 8)
    and the Rabenseifner all-reduce (P = 2, 4, 8) simulated on the packed array, the result unpacked by the header's
    OUTPUT numbers: every tensor's bits are those of its own simulation, on every rank.  The output slots are
    disjoint, inside the region, at multiples of 4, on all four 16-B phases."""
    exe = _gxx(tmp_path, "layout", LAYOUT_HARNESS)
    # equal element sizes (out_esz 0 or esz): the two layouts are one, which is what every plain run relies on
    for oe in (0, 2):
        (S, S_out, _), rows = _layout(exe, 4, [4 * c for c in COUNTS], 2, oe)
        assert S == S_out and all(r[0] == r[2] and r[1] == r[3] for r in rows)
    for P in (2, 3, 4, 8):
        (S, S_out, count), rows = _layout(exe, P, [P * c for c in COUNTS], 2, 4)
        assert S % 128 == 0 and S_out == 2 * S and S_out % 256 == 0 and count == P * S // 2
        assert [r[1] for r in rows] == [2 * c for c in COUNTS] and [r[3] for r in rows] == [4 * c for c in COUNTS]
        assert [r[2] % 16 for r in rows] == [0, 4, 12, 8, 12, 8, 4]
        assert all(r[2] == 2 * r[0] and r[2] % 4 == 0 for r in rows)
        ends = [(r[2], r[2] + r[3]) for r in rows]
        assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:])) and ends[-1][1] <= S_out  # disjoint, inside a slot
        data = [collective_inputs(70 + i, P, BF16, P * c) for i, c in enumerate(COUNTS)]  # [tensor][rank]
        packed = [np.zeros(P * S // 2, np.uint16) for _ in range(P)]
        for r in range(P):
            for (off, slot, _, _), xs, c in zip(rows, data, COUNTS):
                for k in range(P):
                    packed[r][(k * S + off) // 2:(k * S + off + slot) // 2] = xs[r][k * c:(k + 1) * c]
        if P != 2:  # the ring's slot counts: P = W
            bufs = [widen(p, BF16) for p in packed]
            ringsim.reduce_scatter_ring(bufs, _f32_add_into, *ringsim.rs_maps())
            for (_, _, o_off, o_slot), xs in zip(rows, data):
                own = expected_slots(xs, BF16)
                for r in range(P):
                    got = bufs[r][(r * S_out + o_off) // 4:(r * S_out + o_off + o_slot) // 4]
                    assert got.tobytes() == own[r].tobytes(), (P, r, o_off)
        if P & (P - 1) == 0:  # Rabenseifner's slot counts
            bufs = [widen(p, BF16) for p in packed]
            rabsim.rabenseifner_allreduce(bufs, _f32_add_into)
            for (_, _, o_off, o_slot), xs, c in zip(rows, data, COUNTS):
                own = [widen(x, BF16) for x in xs]
                rabsim.rabenseifner_allreduce(own, _f32_add_into)
                for r in range(P):
                    got = np.concatenate([bufs[r][(k * S_out + o_off) // 4:(k * S_out + o_off + o_slot) // 4]
                                          for k in range(P)])
                    assert got.tobytes() == own[r].tobytes(), (P, r, o_off)


# ------------------------------------------------------------------------------------------- CPU: the argument checks
BASE = 1 << 44  # never dereferenced: validation is pointer arithmetic ahead of any HIP call


def test_add_rows_argument_checks_cpu():
    import dccl_amd as d
    assert "dccl_add_rows_f32_multi" in d.EXPORTED_SYMBOLS
    out = subprocess.run(["nm", "-D", "--defined-only", d.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "dccl_add_rows_f32_multi" in {line.split()[-1] for line in out.splitlines() if line.strip()}
    add = d.add_rows_f32_multi
    far = BASE + (1 << 30)
    seg = (BASE, far, 64, 64, 64)
    assert add([(BASE, far, 6, 8, 8)], 1) == 4                    # row_bytes not a multiple of 4
    assert add([seg, (BASE + 4096, far + 4096, 1022, 1024, 1024)], 3) == 4
    assert add([seg] * 33, 1) == 4                                # nsegs
    assert d.lib.dccl_add_rows_f32_multi(None, -1, 1, None) == 4
    assert d.lib.dccl_add_rows_f32_multi(None, 1, 1, None) == 4   # NULL segs with nsegs > 0
    assert add([seg], 0) == 4                                     # rows == 0
    assert add([], 0) == 4                                        # ... ahead of nsegs == 0
    assert add([(0, far, 64, 64, 64)], 1) == 4                    # NULL src / dst of a segment with bytes
    assert add([(BASE, 0, 64, 64, 64)], 1) == 4
    assert add([(BASE, far, 64, 60, 64)], 2) == 4                 # a stride below row_bytes with rows > 1
    assert add([(BASE, far, 64, 64, 60)], 2) == 4
    assert add([(BASE, BASE + 60, 64, 64, 64)], 1) == 4           # a dst row sharing a byte with a src row
    assert add([(BASE, BASE, 64, 64, 64)], 1) == 4                # no in-place form
    assert add([(BASE, BASE + 128 + 60, 64, 128, 128)], 3) == 4   # dst row 0 meets src row 1
    assert add([seg, (BASE + 4096, far + 60, 64, 64, 64)], 1) == 4  # ... or with another dst
    assert add([seg, (far + 60, BASE + 4096, 64, 64, 64)], 1) == 4  # ... or another segment's src
    # the overlap rules come before the multiple-of-4 rule, in copy_rows_check's order
    assert add([(BASE, far, 6, 2, 8)], 2) == 4
    assert add([], 3) == 0                                        # nsegs == 0 succeeds
    assert d.lib.dccl_add_rows_f32_multi(None, 0, 3, None) == 0
    assert add([(0, 0, 0, 0, 0)], 2) == 0                         # nothing but empty rows: nothing to launch
    import torch
    if not torch.cuda.is_available():  # accepted arguments reach the launch, which fails where no GPU exists
        assert add([seg], 1) == 1
        assert add([(BASE, BASE + 64, 64, 128, 128)], 3) == 1     # src and dst rows interleave: accepted


# ------------------------------------------------------------------------------------------ the kernel's cases (numpy)
ROW_BYTES = (4, 12, 16, 1020, 1024, 1028, 2060)  # below a vector, one tile exactly, a tile + an element, two tiles + tail
DST_PHASES = (0, 4, 8, 12, 2, 1)                 # the last two: the element-wise path
SRC_PHASES = (0, 4, 8, 12)
GUARD = 0xA5
ADD_CASES = [(1, rows, seed) for rows in (1, 3) for seed in range(len(ROW_BYTES) * len(DST_PHASES))] + \
            [(n, rows, seed) for n in (5, 32) for rows in (1, 3) for seed in (0, 3)]


def add_case(nsegs, rows, seed):
    """Segments (src offset, dst offset, row_bytes, src_stride, dst_stride) in one source and one destination arena.
    Segment i of seed s takes row size (i + s) % 7, destination phase (i + s // 7) % 6 and source phase (i + s) % 4:
    the one-segment seeds 0..41 walk every (row size, destination phase) pair.  Strides exceed row_bytes by a
    multiple of 4, so the rows of a segment fall on different 16-B phases but keep their 4-byte class."""
    rng = np.random.default_rng([SEED, 11, nsegs, rows, seed])
    segs, s_at, d_at = [], 64, 64
    for i in range(nsegs):
        n = ROW_BYTES[(i + seed) % len(ROW_BYTES)]
        ss, ds = n + 4 * int(rng.integers(1, 10)), n + 64 + 4 * int(rng.integers(0, 10))
        s_off = (s_at + 255) // 256 * 256 + SRC_PHASES[(i + seed) % 4]
        d_off = (d_at + 255) // 256 * 256 + DST_PHASES[(i + seed // len(ROW_BYTES)) % len(DST_PHASES)]
        segs.append((s_off, d_off, n, ss, ds))
        s_at, d_at = s_off + rows * ss + 64, d_off + rows * ds + 64
    return segs, s_at + 256, d_at + 256


def add_arenas(nsegs, rows, seed):
    """(segs, source arena, destination arena, expected destination arena): fp32 standard normals in the rows of both
    arenas, the guard pattern everywhere else; the expectation is numpy's prior + src in np.float32, rows only.
    Returns also the share of row elements whose sum differs from the prior and from the source."""
    segs, s_len, d_len = add_case(nsegs, rows, seed)
    rng = np.random.default_rng([SEED, 12, nsegs, rows, seed])
    src, dst = np.full(s_len, GUARD, np.uint8), np.full(d_len, GUARD, np.uint8)
    parts = []
    for (s_off, d_off, n, ss, ds) in segs:
        for r in range(rows):
            a, b = rng.standard_normal(n // 4).astype(np.float32), rng.standard_normal(n // 4).astype(np.float32)
            src[s_off + r * ss:s_off + r * ss + n] = a.view(np.uint8)
            dst[d_off + r * ds:d_off + r * ds + n] = b.view(np.uint8)
            parts.append((d_off + r * ds, a, b))
    want = dst.copy()
    differ, total = 0, 0
    for at, a, b in parts:
        sum_ = f32_add(b, a)
        want[at:at + sum_.nbytes] = sum_.view(np.uint8)
        differ += int(np.count_nonzero((sum_.view(np.uint32) != a.view(np.uint32)) &
                                       (sum_.view(np.uint32) != b.view(np.uint32))))
        total += sum_.size
    return segs, src, dst, want, differ / total


def test_add_rows_cases_are_distinguishable_cpu():
    """The premise of the GPU kernel tests, from numpy alone: in every case at least 99 % of the expected sums differ
    from both the previous destination and the source, so a copy or a no-op cannot pass; and the one-segment seeds
    cover every (row size, destination phase) pair."""
    seen, five = set(), set()
    for nsegs, rows, seed in ADD_CASES:
        segs, _, _, _, share = add_arenas(nsegs, rows, seed)
        assert share >= 0.99, (nsegs, rows, seed, share)
        if nsegs == 1:
            seen.add((segs[0][2], segs[0][1] % 16))
        elif nsegs == 5:
            five |= {s[2] for s in segs}
        else:  # a batch of 32 holds every row size, both 4-byte classes and every source phase
            assert {s[2] for s in segs} == set(ROW_BYTES) and {s[1] % 16 for s in segs} == set(DST_PHASES)
            assert {s[0] % 16 for s in segs} == set(SRC_PHASES)
    assert seen == {(n, p) for n in ROW_BYTES for p in DST_PHASES} and five == set(ROW_BYTES)


def run_add_case(nsegs, rows, seed):
    """One launch on the GPU, compared with numpy over the whole destination arena (guards and stride gaps included)."""
    import torch
    import dccl_amd as d
    segs, src, dst, want, share = add_arenas(nsegs, rows, seed)
    assert share >= 0.99, (nsegs, rows, seed, share)
    t_src, t_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    assert t_src.data_ptr() % 256 == 0 and t_dst.data_ptr() % 256 == 0
    abs_segs = [(t_src.data_ptr() + s, t_dst.data_ptr() + q, n, ss, ds) for (s, q, n, ss, ds) in segs]
    torch.cuda.synchronize()
    assert d.add_rows_f32_multi(abs_segs, rows) == 0
    torch.cuda.synchronize()
    got = t_dst.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (nsegs, rows, seed, bad.size, bad[:8], segs[:3])
    assert t_src.cpu().numpy().tobytes() == src.tobytes()


# ----------------------------------------------------------------------------------------------------- GPU: the kernel
@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 3])
@pytest.mark.parametrize("nsegs", [1, 5, 32])
def test_add_rows_against_numpy(gpu, nsegs, rows):
    """dccl_add_rows_f32_multi against prior + src in np.float32, bit for bit: every row size at every destination
    phase (one segment), and batches of 5 and 32 segments; every byte outside the rows keeps the guard pattern."""
    cases = [c for c in ADD_CASES if c[0] == nsegs and c[1] == rows]
    assert len(cases) == (42 if nsegs == 1 else 2)
    for c in cases:
        run_add_case(*c)


STRIDE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import dccl_amd
assert dccl_amd.lib.dccl_max_grid_test() == 8, "the grid clamp is not live in this process"
from tests import test_widened_group as wg
ran = 0
for case in wg.ADD_CASES:
    if case[0] == 32:
        wg.run_add_case(*case)
        ran += 1
print("RAN", ran)
"""


@pytest.mark.gpu
def test_add_rows_grid_stride(gpu):
    """The 32-segment batches in a fresh child under DCCL_MAX_GRID_TEST=8 (tests/test_gpu_grid_stride_small.py's
    mechanism): 50 to 150 tiles over 8 blocks, so most tiles are second and later passes."""
    for c in ADD_CASES:
        if c[0] == 32:
            tiles = c[1] * sum(-(-(s[2] // 16 + 1) // 64) for s in add_case(*c)[0])
            assert tiles >= 5 * 8, (c, tiles)
    env = {**os.environ, "DCCL_MAX_GRID_TEST": "8", "PYTHONPATH": ROOT}
    env.pop("DCCL_CAPS_TEST_SHIFT", None)
    p = subprocess.run([sys.executable, "-c", STRIDE_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "RAN 4" in p.stdout.splitlines(), p.stdout[-500:]


# ------------------------------------------------------------------------------------- GPU: collectives, thread ranks
RECV_PHASES = (0, 4, 8, 12, 2, 8, 4)  # byte phase of each recvbuff in its arena; the fifth is off 4-byte alignment
ACCS = (0, 1)


def recv_arena(prior_seed, r, sizes):
    """One host arena holding a recvbuff per tensor (sizes in fp32 elements), tensor i at 16-B phase RECV_PHASES[i],
    filled with prior_recv; guard bytes in between.  Returns (arena, byte offsets)."""
    offs, at = [], 64
    for m, ph in zip(sizes, RECV_PHASES):
        o = (at + 15) // 16 * 16 + ph
        offs.append(o)
        at = o + 4 * m + 32
    arena = np.full(at + 64, GUARD, np.uint8)
    for i, (o, m) in enumerate(zip(offs, sizes)):
        arena[o:o + 4 * m] = prior_recv(prior_seed + i, r, m).view(np.uint8)
    return arena, offs


def split_arena(arena, offs, sizes):
    """The tensors of an arena as fp32 arrays, after asserting that every guard byte is still the pattern."""
    mask = np.ones(arena.size, bool)
    for o, m in zip(offs, sizes):
        mask[o:o + 4 * m] = False
    assert (arena[mask] == GUARD).all(), "guard bytes between the recvbuffs changed"
    return [arena[o:o + 4 * m].copy().view(np.float32) for o, m in zip(offs, sizes)]


def _issue(comm, api, sends, recv_ptrs, counts, W, dt, ops, stream, grouped):
    import dccl_amd

    def calls():
        for s, v, c, op in zip(sends, recv_ptrs, counts, ops):
            if api == "reduce_scatter":
                assert comm.reduce_scatter(s.data_ptr(), v, c, dt, op, stream) == 0
            else:
                assert comm.reduce(s.data_ptr(), v, c * W, dt, op, 1, stream) == 0
    if grouped:
        with dccl_amd.group():
            calls()
    else:
        calls()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring"])
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("W", [3, 4])
def test_widened_groups_threads(gpu, monkeypatch, W, dt, algo):
    """Seven same-handle widened reduce-scatters (recvcount COUNTS), and seven reduces to root 1, once inside a group
    and once as separate calls, accumulate 0 and 1; algo "": the direct collectives, "ring": the wide-staged route.
    Grouped and separate results are equal bit for bit, both equal the ring simulation over the widened inputs (plus
    the previous recvbuff with accumulate), a non-root recvbuff of a reduce keeps its bytes, and every grouped pass
    is one coalesced run of seven tensors on every rank.  The recvbuffs are carved from one arena at 16-B phases
    0, 4, 8, 12, 2, 8, 4: the fifth is not 4-byte aligned, which the plain call accepts (its results are checked
    against numpy here like the others')."""
    import torch
    import dccl_amd
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    data = [collective_inputs(80 + i, W, dt, c * W) for i, c in enumerate(COUNTS)]  # [tensor][rank]
    root = 1

    def body(comm, r):
        st = torch.cuda.Stream()
        out = {}
        for acc in ACCS:
            rc, op = comm.red_op_create_widened_sum(dt, acc)
            assert rc == 0
            for api in ("reduce_scatter", "reduce"):
                sizes = [c if api == "reduce_scatter" else c * W for c in COUNTS]
                for grouped in (False, True):
                    sends = [torch.from_numpy(xs[r].view(np.uint8).copy()).cuda() for xs in data]
                    arena, offs = recv_arena(90, r, sizes)
                    t = torch.from_numpy(arena).cuda()
                    assert t.data_ptr() % 16 == 0
                    torch.cuda.synchronize()
                    _issue(comm, api, sends, [t.data_ptr() + o for o in offs], COUNTS, W, dt, [op] * len(COUNTS),
                           st.cuda_stream, grouped)
                    torch.cuda.synchronize()
                    out[(api, acc, grouped)] = split_arena(t.cpu().numpy(), offs, sizes)
                    for s, xs in zip(sends, data):
                        assert s.cpu().numpy().tobytes() == xs[r].view(np.uint8).tobytes(), "sendbuff changed"
            assert comm.red_op_destroy(op) == 0
        return out

    before = dccl_amd.group_stats()
    outs = run_ranks(W, body)
    delta = stats_delta(before)
    # 2 accumulate values x 2 apis grouped passes, each one run of seven tensors on each of the W ranks
    assert (delta["coalesced_runs"], delta["tensors_coalesced"]) == (4 * W, 4 * W * len(COUNTS)), delta
    assert delta["bytes_packed"] == 4 * W * sum(2 * c * W for c in COUNTS), delta  # the 16-bit bytes
    for i, (xs, c) in enumerate(zip(data, COUNTS)):
        slots = expected_slots(xs, dt)
        whole = np.concatenate(slots)
        for acc in ACCS:
            for r in range(W):
                for grouped in (False, True):
                    what = (i, acc, r, "grouped" if grouped else "separate")
                    prior = prior_recv(90 + i, r, c)
                    assert_f32_bits(outs[r][("reduce_scatter", acc, grouped)][i],
                                    f32_add(prior, slots[r]) if acc else slots[r], ("reduce_scatter",) + what)
                    prior = prior_recv(90 + i, r, c * W)
                    got = outs[r][("reduce", acc, grouped)][i]
                    if r == root:
                        assert_f32_bits(got, f32_add(prior, whole) if acc else whole, ("reduce",) + what)
                    else:
                        assert got.tobytes() == prior.tobytes(), ("non-root recvbuff",) + what
                for api in ("reduce_scatter", "reduce"):
                    assert outs[r][(api, acc, True)][i].tobytes() == outs[r][(api, acc, False)][i].tobytes(), (api, i)


# ---------------------------------------------------------------------------------------------- GPU: the mixed queue
MIXED_W, MIXED_DT = 4, BF16
MIXED_QUEUE = ("acc0", "acc0", "acc1", "acc1", "sum", "sum", "acc0")
MIXED_COUNTS = (257, 1031, 515, 3, 64, 257, 2)


def run_mixed_queue():
    """The child's body: MIXED_QUEUE as reduce-scatters on W = 4 thread ranks, separate and grouped.  Returns the
    group-stats delta of the grouped pass and, per mode, a digest of every rank's results; asserts both modes against
    numpy."""
    import torch
    import dccl_amd
    W, dt = MIXED_W, MIXED_DT
    data = [collective_inputs(100 + i, W, dt, c * W) for i, c in enumerate(MIXED_COUNTS)]

    def body(comm, r):
        st = torch.cuda.Stream()
        ops = {"sum": SUM}
        for acc in ACCS:
            rc, ops[f"acc{acc}"] = comm.red_op_create_widened_sum(dt, acc)
            assert rc == 0
        out = {}
        for grouped in (False, True):
            sends = [torch.from_numpy(xs[r].view(np.uint8).copy()).cuda() for xs in data]
            recvs = [torch.from_numpy(prior_recv(110 + i, r, c).copy()).cuda() for i, c in enumerate(MIXED_COUNTS)]
            torch.cuda.synchronize()
            _issue(comm, "reduce_scatter", sends, [v.data_ptr() for v in recvs], MIXED_COUNTS, W, dt,
                   [ops[k] for k in MIXED_QUEUE], st.cuda_stream, grouped)
            torch.cuda.synchronize()
            out[grouped] = [v.cpu().numpy() for v in recvs]
        for k in ("acc0", "acc1"):
            assert comm.red_op_destroy(ops[k]) == 0
        return out

    before = dccl_amd.group_stats()
    outs = run_ranks(W, body)
    delta = stats_delta(before)
    digest = {}
    for grouped in (False, True):
        h = hashlib.sha256()
        for i, (xs, c, kind) in enumerate(zip(data, MIXED_COUNTS, MIXED_QUEUE)):
            slots = expected_slots(xs, dt)
            for r in range(W):
                got, prior = outs[r][grouped][i], prior_recv(110 + i, r, c)
                if kind == "sum":  # bf16 into the first half of the buffer's bytes
                    half = got.view(np.uint16)
                    assert half[:c].tobytes() == plain_slots(xs, dt)[r].tobytes(), (i, r, grouped)
                    assert half[c:].tobytes() == prior.view(np.uint16)[c:].tobytes(), (i, r, grouped)
                else:
                    assert_f32_bits(got, f32_add(prior, slots[r]) if kind == "acc1" else slots[r], (i, r, grouped))
                assert got.tobytes() == outs[r][False][i].tobytes(), (i, r)
                h.update(got.tobytes())
        digest["grouped" if grouped else "separate"] = h.hexdigest()
    return {"runs": delta["coalesced_runs"], "tensors": delta["tensors_coalesced"], "groups": delta["groups"],
            "digest": digest}


MIXED_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from tests import test_widened_group as wg
print("RESULT", json.dumps(wg.run_mixed_queue()))
"""


def _mixed_child(coalesce):
    env = {**os.environ, "PYTHONPATH": ROOT}
    for k in ("DCCL_GROUP_COALESCE", "DCCL_GROUP_COALESCE_MAX_BYTES", "DCCL_ALLREDUCE_ALGORITHM",
              "DCCL_MAX_GRID_TEST", "DCCL_CAPS_TEST_SHIFT"):
        env.pop(k, None)
    if coalesce is not None:
        env["DCCL_GROUP_COALESCE"] = coalesce
    p = subprocess.run([sys.executable, "-c", MIXED_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    line = [l for l in p.stdout.splitlines() if l.startswith("RESULT ")]
    assert len(line) == 1, p.stdout[-500:]
    return json.loads(line[0][len("RESULT "):])


@pytest.mark.gpu
def test_widened_mixed_queue_and_coalesce_off(gpu):
    """[acc0, acc0, acc1, acc1, plain SUM, plain SUM, acc0] in one group, W = 4, bf16: three coalesced runs of six
    tensors on every rank (the last call runs alone), every result the separate call's and numpy's.  With
    DCCL_GROUP_COALESCE=0 the same queue gives the same bits and no coalesced run.  Each setting in its own child:
    the variable is read at every group end and must agree on all ranks."""
    on, off = _mixed_child(None), _mixed_child("0")
    W = MIXED_W
    assert (on["groups"], on["runs"], on["tensors"]) == (W, 3 * W, 6 * W), on
    assert (off["groups"], off["runs"], off["tensors"]) == (W, 0, 0), off
    assert on["digest"]["grouped"] == on["digest"]["separate"] == off["digest"]["grouped"] == off["digest"]["separate"]


# ------------------------------------------------------------------------------------------ GPU: across IPC processes
XP_COUNTS = (257, 3, 1031)
XP_DT = BF16


def _xp_group(comm, r, W, torch):
    import dccl_amd
    rc, op = comm.red_op_create_widened_sum(XP_DT, 1)
    assert rc == 0, rc
    data = [collective_inputs(120 + i, W, XP_DT, c * W) for i, c in enumerate(XP_COUNTS)]
    sends = [torch.from_numpy(xs[r].view(np.uint8).copy()).cuda() for xs in data]
    recvs = [torch.from_numpy(prior_recv(130 + i, r, c).copy()).cuda() for i, c in enumerate(XP_COUNTS)]
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    before = dccl_amd.group_stats()
    _issue(comm, "reduce_scatter", sends, [v.data_ptr() for v in recvs], XP_COUNTS, W, XP_DT, [op] * 3, st.cuda_stream,
           True)
    torch.cuda.synchronize()
    after = dccl_amd.group_stats()
    assert comm.red_op_destroy(op) == 0
    return [v.cpu().numpy() for v in recvs], {k: after[k] - before[k] for k in after}


@pytest.mark.gpu
def test_widened_group_ipc_processes(gpu):
    """One process per rank on the IPC transport, W = 2: three same-handle widened reduce-scatters (accumulate 1) in a
    group are one coalesced run in each process and give the expected bits."""
    W = 2
    results = xproc.run_ipc(W, _xp_group)
    for i, c in enumerate(XP_COUNTS):
        slots = expected_slots(collective_inputs(120 + i, W, XP_DT, c * W), XP_DT)
        for r in range(W):
            (outs, delta), fin = results[r]
            assert fin == 0
            assert (delta["coalesced_runs"], delta["tensors_coalesced"]) == (1, 3), delta
            assert_f32_bits(outs[i].view(np.float32), f32_add(prior_recv(130 + i, r, c), slots[r]), (i, r))
