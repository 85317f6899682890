"""Widened sums (dcclRedOpCreateWidenedSum): fp16 / bf16 contributions accumulated in fp32 and
delivered as fp32, optionally added to what the fp32 destination holds:

    dst32[i] (+)= widen(own[i]) + (widen(sends[k-1][i]) + ... (widen(sends[1][i]) + widen(sends[0][i])))

The contract is bit-exact.  Every expected value is numpy's (tests/test_wide_sum.py's widen / wide_acc: exact
widening, sequential np.float32 adds in the stated order; the ring simulation over the widened inputs; one more
np.float32 add for `accumulate`).  fp32 results are compared as uint32 bits where the expectation is not NaN, and by
NaN-ness where it is.

CPU: the validation tables of dccl_local_reduce_chain_widen and of the op, the op table's lifecycle, the collectives'
errors, the selector over its whole grid (kind 4 next to kinds 0..3), the group planner, and the distinguishability
conditions below.
GPU: the chain against the oracle at nine placements (vector kernel with and without head elements, both element-wise
fallbacks), all 65,536 patterns, the grid-stride passes in a child process, reduce_scatter / reduce on thread ranks
(direct and ring; W = 1; a group), and one IPC and one RCCL reduce-scatter across processes.

Distinguishability, on streams of at least 4096 elements (tests/test_wide_sum.py chain_stream's seeds); each
alternative implementation must differ from the contract in at least the stated share of elements:
  normal                  the result rounded to 16 bits and widened again (the wide sum + convert): >= 0.40 for every
                          nsend >= 1; per-step rounding: >= 0.40
  cancelling              the adds in reversed order, and as a pairwise tree: >= 0.40 each for nsend >= 2
  accumulate, cancelling  the previous dst folded in FIRST instead of last: >= 0.90 for nsend >= 1
  accumulate, both        the previous dst ignored: >= 0.90
The previous dst is fp32 standard normals times the family's SMALL factor.
"""
import ctypes
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ringsim, xproc
from tests import test_select as sel
from tests.test_caps import CSRC
from tests.test_collectives import _expected_allreduce, run_ranks
from tests.test_oracle import fp_equal
from tests.test_wide_sum import (BF16, DTS, F16, F32, FAMILIES, ROOT, SEED, SMALL, SUM, all_patterns, chain_stream,
                                 collective_inputs, expected_collective, family_ops, narrow, stepwise_sum, tree_acc,
                                 wide_acc, widen)

# (nsend, count, dst bytes past a 128-B line, sources' byte phase, own's byte phase, form reached)
CHAIN_CASES = [
    (1, 1, 0, 0, 0, "vector, no head"),
    (2, 17, 0, 0, 0, "vector, no head"),
    (3, 4099, 0, 0, 0, "vector, no head"),
    (8, 1000, 0, 0, 0, "vector, no head"),
    (7, 65537, 8, 4, 4, "vector, head of 6"),
    (4, 3001, 0, 4, 4, "element-aligned fallback: dst misses the 16-B boundary"),
    (5, 777, 0, 1, 1, "bytewise fallback"),
    (2, 515, 2, 0, 0, "bytewise fallback: dst off 4-byte alignment"),
    (3, 2050, 0, 0, 8, "fallback: operands at different phases"),
]
PAD = 256  # every operand lies this far into its allocation: guard bytes on both sides
ACCS = (0, 1)


# ----------------------------------------------------------------------------- the oracle (numpy only)
def prior_dst(dt, family, nsend, count, n):
    """The previous content of dst of a chain case: fp32 standard normals times the family's SMALL factor."""
    rng = np.random.default_rng([SEED, dt, FAMILIES.index(family), nsend, count, 32])
    return (rng.standard_normal(n) * (SMALL[dt] if family == "cancelling" else 1.0)).astype(np.float32)


def f32_add(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, np.float32) + np.asarray(b, np.float32)


def widened_expected(ops, dt, prior=None):
    """The contract: the wide chain's accumulator; with a previous dst, one more fp32 add after the chain."""
    acc = wide_acc(ops, dt)
    return acc if prior is None else f32_add(prior, acc)


def folded_first(ops, dt, prior):
    """The previous dst as the chain's first operand (what the contract forbids)."""
    acc = prior.copy()
    for x in ops:
        acc = f32_add(widen(x, dt), acc)
    return acc


def bits_differ(a, b) -> float:
    return float(np.mean(np.ascontiguousarray(a, np.float32).view(np.uint32) !=
                         np.ascontiguousarray(b, np.float32).view(np.uint32)))


def assert_f32_bits(got, want, what=""):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.flatnonzero(got.view(np.uint32)[~nan] != want.view(np.uint32)[~nan])
    assert bad.size == 0, (what, bad.size, bad[:4], got[~nan][bad[:4]], want[~nan][bad[:4]])
    assert np.isnan(got[nan]).all(), what


def assert_distinguishable(ops, dt, family, nsend, prior):
    want = wide_acc(ops, dt)
    assert np.isfinite(want).all()
    shares = {}
    if family == "normal":
        shares["rounded and widened again"] = (bits_differ(widen(narrow(want, dt), dt), want), 0.40, 1)
        shares["per-step rounding"] = (bits_differ(widen(stepwise_sum(ops, dt), dt), want), 0.40, 1)
    else:
        shares["reversed order"] = (bits_differ(wide_acc(ops[::-1], dt), want), 0.40, 2)
        shares["pairwise tree"] = (bits_differ(tree_acc(ops, dt), want), 0.40, 2)
        shares["prior folded in first"] = (bits_differ(folded_first(ops, dt, prior), f32_add(prior, want)), 0.90, 1)
    shares["prior ignored"] = (bits_differ(want, f32_add(prior, want)), 0.90, 1)
    print(f"dtype {dt} {family} nsend {nsend} n {ops[0].size}: " +
          ", ".join(f"{k} differs in {v[0]:.3f}" for k, v in shares.items()))
    for k, (share, least, from_nsend) in shares.items():
        if nsend >= from_nsend:
            assert share >= least, (dt, family, nsend, k, share)


def stream_and_prior(dt, family, nsend, count):
    ops = chain_stream(dt, family, nsend, count)
    return ops, prior_dst(dt, family, nsend, count, ops[0].size)


# ----------------------------------------------------------------------------- CPU
def test_widen_argument_checks_cpu():
    """Every row of dccl_local_reduce_chain_widen's validation table, in its order; the pointer values are never
    dereferenced (the checks run ahead of any launch)."""
    import dccl_amd as d
    n = 16
    a, b, c = 1 << 40, (1 << 40) + (1 << 20), (1 << 40) + (2 << 20)
    chain = d.local_reduce_chain_widen
    raw = d.lib.dccl_local_reduce_chain_widen
    # 1. dtype not fp16 / bf16 wins over everything after it (a bad accumulate, no sources, NULLs)
    for dt in (0, 2, 7, 8, 10, 11, -1):
        assert chain([a], b, c, dt, n, 0) == 4, dt
        assert chain([], 0, 0, dt, n, 7) == 4, dt
    for dt in DTS:
        # 2. accumulate not 0 / 1, ahead of nsend / sends and of count == 0
        for acc in (2, -1, 256):
            assert chain([a], b, c, dt, n, acc) == 4, acc
            assert chain([a], b, c, dt, 0, acc) == 4, acc
            assert raw(None, 1, b, c, dt, 0, acc, None) == 4, acc
        for acc in ACCS:
            # 3. nsend outside 1..8, NULL sends: also ahead of count == 0
            assert chain([], b, c, dt, n, acc) == 4
            assert chain([a] * 9, b, c, dt, n, acc) == 4
            assert raw(None, 1, b, c, dt, n, acc, None) == 4
            assert raw(None, 1, b, c, dt, 0, acc, None) == 4
            # 4. count == 0 succeeds, ahead of the operand checks
            assert chain([0], 0, 0, dt, 0, acc) == 0
            assert chain([c], c, c, dt, 0, acc) == 0
            # 5. NULL operands
            assert chain([0], b, c, dt, n, acc) == 4
            assert chain([a, 0], b, c, dt, n, acc) == 4
            assert chain([a], 0, c, dt, n, acc) == 4
            assert chain([a], b, 0, dt, n, acc) == 4
            # 6. any byte shared with [dst, dst + 4 n): the same address (no in-place form), one range inside the
            # other, one byte at either end; for a source and for own
            for sh in (0, 2, 4, 4 * n - 1, 4 * n - 2, -2, -(2 * n - 1), -(2 * n - 2), 1):
                assert chain([a, c + sh], b, c, dt, n, acc) == 4, sh
                assert chain([a], c + sh, c, dt, n, acc) == 4, sh
    # 7. launch failure: only where no GPU exists; operands adjacent to dst pass validation and reach the launch
    import torch
    if not torch.cuda.is_available():
        assert chain([a], b, c, BF16, n, 0) == 1
        assert chain([c + 4 * n], c - 2 * n, c, F16, n, 1) == 1


def test_widened_op_lifecycle_and_collective_errors_cpu():
    import dccl_amd as d
    comm = d.Comm.in_process(1, 0)
    try:
        s = np.array([0.25], np.float32)
        h = np.arange(8, dtype=np.uint16)
        y = np.zeros(8, np.float32)
        make = comm.red_op_create_widened_sum
        # creation: NULL op, the datatype (fp16 / bf16 only), accumulate (0 / 1 only)
        assert d.lib.dccl_red_op_create_widened_sum(None, BF16, 0, comm.handle) == 4
        for dt in (0, 2, 7, 8, 10, 11, -1):
            assert make(dt, 0)[0] == 4, dt
        for acc in (2, -1, 256):
            assert make(BF16, acc)[0] == 4, acc
        out = ctypes.c_int(0)
        assert d.lib.dccl_red_op_create_widened_sum(ctypes.byref(out), BF16, 0, None) == 4  # null communicator
        for acc in ACCS:
            rc, op = make(BF16, acc)
            assert rc == 0 and 5 <= op <= 20
            # no widened all-reduce, whatever the buffers
            assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 5
            assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 0, BF16, op) == 5
            # host buffers: the library never combines on the CPU
            assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 5
            assert comm.reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op, 0) == 5
            # sendbuff and recvbuff sharing any byte: the same address, one byte at either end
            base = y.ctypes.data
            for send, recv in ((base, base), (base + 31, base), (base, base + 15), (base + 4, base)):
                assert comm.reduce_scatter(send, recv, 8, BF16, op) == 4, (send - base, recv - base)
                assert comm.reduce(send, recv, 8, BF16, op, 0) == 4, (send - base, recv - base)
            # a live handle with another datatype (the other 16-bit float included)
            for dt in (F16, F32, 2, 10, 11):
                assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 4, dt, op) == 4, dt
                assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 4, dt, op) == 4, dt
                assert comm.reduce(h.ctypes.data, y.ctypes.data, 4, dt, op, 0) == 4, dt
            assert comm.red_op_destroy(op) == 0
            assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 4  # dead
            assert comm.red_op_destroy(op) == 4
        assert not y.any()
        # the 16 slots are shared with the other creators; the 17th live op of any kind is ncclInvalidUsage
        ops = []
        for k in range(16):
            if k % 4 == 0:
                rc, hnd = comm.red_op_create_premul_sum(s.ctypes.data, F32, 1)
            elif k % 4 == 1:
                rc, hnd = comm.red_op_create_wide_sum(BF16)
            elif k % 4 == 2:
                rc, hnd = comm.red_op_create_wide_scaled_sum(s.ctypes.data, F16, 1)
            else:
                rc, hnd = make(F16 if k % 8 == 3 else BF16, (k // 4) % 2)
            assert rc == 0
            ops.append(hnd)
        assert sorted(ops) == list(range(5, 21))
        assert make(BF16, 1)[0] == 5
        assert comm.red_op_create_wide_sum(BF16)[0] == 5
        # destroy, then create again: the slot is reused and carries the new op's kind and datatype
        assert comm.red_op_destroy(ops[1]) == 0  # a bf16 wide sum
        rc, again = make(F16, 1)
        assert rc == 0 and again == ops[1]
        assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 8, BF16, again) == 4  # an fp16 op now
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, F16, again) == 5       # ... and a widened one
        assert comm.red_op_destroy(ops[3]) == 0  # a widened sum
        rc, again = comm.red_op_create_wide_sum(F16)
        assert rc == 0 and again == ops[3]
        assert comm.all_reduce(h.ctypes.data, h.ctypes.data, 8, F16, again) == 5  # a wide sum: only the host buffers
        assert make(BF16, 0)[0] == 5
        # built-in ops answer as before
        x = np.arange(8, dtype=np.float32)
        assert comm.all_reduce(x.ctypes.data, y.ctypes.data, 8, F32, SUM) == 0
        assert y.tobytes() == x.tobytes()
    finally:
        comm.finalize()


WIDENED = 4  # select.hpp SumKind kWidenedSum


@pytest.fixture(scope="module")
def selected(tmp_path_factory):
    """select() over the whole grid with five sum kinds, from tests/test_select.py's harness."""
    d = tmp_path_factory.mktemp("select_widened")
    src, exe = d / "select_dump.cpp", d / "select_dump"
    src.write_text(sel.HARNESS)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True)
    grid = list(itertools.product(range(5), range(4), sel.WORLDS, (0, 1), range(5), sel.NAMES))
    token = {None: "<unset>", "": "<empty>"}
    lines = [" ".join(map(str, [api, t, W, device, kind, token.get(a, a)])) for api, t, W, device, kind, a in grid]
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", check=True, capture_output=True, text=True).stdout
    rows = [tuple(map(int, l.split())) for l in out.splitlines()]
    assert len(rows) == len(grid) == 5 * 4 * 6 * 2 * 5 * 8
    return dict(zip(grid, rows))


def test_select_widened_goes_where_the_wide_sum_goes_cpu(selected):
    checked = 0
    for (api, t, W, device, kind, a), (_, path, slots) in selected.items():
        if kind != WIDENED:
            # kinds 0..3: what tests/test_select.py expects, unchanged
            assert path == sel.parent_path(api, t, W, device, kind, a), (api, t, W, device, kind, a)
            continue
        if api in (sel.REDUCE_SCATTER, sel.REDUCE):
            assert (path, slots) == selected[(api, t, W, device, sel.WIDE, a)][1:], (api, t, W, device, a)
            assert path in (sel.DIRECT, sel.HOST_DIRECT, sel.WIDE_STAGED)
            checked += 1
        elif api in (sel.ALL_GATHER, sel.BROADCAST):  # the form is never looked at
            assert path == selected[(api, t, W, device, sel.BUILTIN, a)][1]
    assert checked == 2 * 4 * 6 * 2 * 8
    assert selected[(sel.REDUCE_SCATTER, sel.THREADS, 8, 1, WIDENED, None)][1] == sel.DIRECT
    assert selected[(sel.REDUCE_SCATTER, sel.THREADS, 8, 1, WIDENED, "ring")][1] == sel.WIDE_STAGED
    assert selected[(sel.REDUCE, sel.IPC, 3, 1, WIDENED, "ring")][1] == sel.DIRECT
    assert selected[(sel.REDUCE, sel.RCCL, 2, 1, WIDENED, None)][1] == sel.WIDE_STAGED
    assert selected[(sel.REDUCE_SCATTER, sel.THREADS, 9, 1, WIDENED, None)][1] == sel.WIDE_STAGED
    assert selected[(sel.REDUCE, sel.THREADS, 1, 1, WIDENED, None)][1] == sel.WIDE_STAGED  # W == 1: the conversion


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
        unsigned long long count;
        int never;
        if (std::scanf("%d %llu %d %d", &c.api, &count, &c.op, &never) != 4) return 2;
        c.comm = &comm, c.count = count, c.esz = 2, c.dtype = 9, c.device = true, c.world = 4;
        c.never_packed = never != 0;
    }
    for (const group::Run& r : group::plan_runs(calls.data(), calls.size(), max_bytes))
        std::printf("%zu %zu %d\n", r.first, r.n, int(r.packed));
}
"""


def test_group_plan_never_packs_a_widened_call_cpu(tmp_path):
    """A queue that mixes packable reductions with widened calls: no run holds a widened call with n > 1, the runs
    cover the queue in issue order, and the packable stretches between them are packed as before."""
    src, exe = tmp_path / "plan.cpp", tmp_path / "plan"
    src.write_text(PLAN_HARNESS)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", f"-I{CSRC}", str(src), "-o", str(exe)],
                   check=True)
    RS, WOP = 1, 7  # reduce-scatter; a user-op handle

    def runs(queue):
        text = f"{1 << 20} {len(queue)}\n" + "\n".join(f"{api} {count} {op} {int(w)}" for api, count, op, w in queue)
        out = subprocess.run([str(exe)], input=text + "\n", check=True, capture_output=True, text=True).stdout
        return [tuple(map(int, l.split())) for l in out.splitlines()]

    plain, wid = (RS, 4096, SUM, False), (RS, 4096, WOP, True)
    assert runs([plain] * 3) == [(0, 3, 1)]
    assert runs([wid] * 3) == [(0, 1, 0), (1, 1, 0), (2, 1, 0)]  # the same key, still never packed
    assert runs([plain, plain, wid, wid, plain, plain, plain, wid]) == [(0, 2, 1), (2, 1, 0), (3, 1, 0), (4, 3, 1),
                                                                        (7, 1, 0)]
    assert runs([wid, plain]) == [(0, 1, 0), (1, 1, 0)]
    rng = np.random.default_rng(SEED)
    for _ in range(20):
        queue = [wid if rng.random() < 0.4 else plain for _ in range(int(rng.integers(1, 40)))]
        got = runs(queue)
        assert [r[0] for r in got] == list(np.cumsum([0] + [r[1] for r in got[:-1]]))
        assert sum(r[1] for r in got) == len(queue)
        for first, n, packed in got:
            assert packed == (n > 1)
            if any(q[3] for q in queue[first:first + n]):
                assert n == 1 and not packed, (first, n)


def test_widened_families_are_distinguishable_cpu():
    """The premise of the GPU chain test, on its own data (module docstring)."""
    checked = 0
    for dt in DTS:
        for family in FAMILIES:
            for nsend, count, *_ in CHAIN_CASES:
                ops, prior = stream_and_prior(dt, family, nsend, count)
                assert ops[0].size >= 4096
                assert_distinguishable(ops, dt, family, nsend, prior)
                checked += 1
    assert checked == 2 * 2 * len(CHAIN_CASES)


# ----------------------------------------------------------------------------- GPU: kernels
def _zero_outside(t, off: int, nbytes: int) -> bool:
    return not t[:off].any() and not t[off + nbytes:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("acc", ACCS, ids=lambda a: f"acc{a}")
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: f"k{c[0]}-n{c[1]}-dst{c[2]}-src{c[3]}-own{c[4]}")
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dt", DTS)
def test_widen_chain_against_oracle(gpu, dt, family, case, acc):
    """dccl_local_reduce_chain_widen, bit for bit against wide_acc (+ the previous dst), at the nine placements of
    CHAIN_CASES.  The family's distinguishability conditions are asserted first, so passing proves the missing
    rounding, the order, and the place of the accumulate add.  Guard bytes around dst and every source stay as they
    were, and so do the sources."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    nsend, n, dst_off, src_ph, own_ph, _ = case
    stream, prior_all = stream_and_prior(dt, family, nsend, n)
    assert_distinguishable(stream, dt, family, nsend, prior_all)
    ops = [np.ascontiguousarray(x[:n]) for x in stream]
    prior = np.ascontiguousarray(prior_all[:n])
    sends, own = ops[:nsend], ops[nsend]
    want = widened_expected(ops, dt, prior if acc else None)
    dev = [dev_bytes(a, PAD + src_ph) for a in sends]
    t_own, p_own = dev_bytes(own, PAD + own_ph)
    t_dst, p_dst = dev_bytes(prior, PAD + dst_off)
    assert p_dst % 128 == dst_off and p_own % 16 == own_ph and all(d[1] % 16 == src_ph for d in dev)
    torch.cuda.synchronize()
    assert dccl_amd.local_reduce_chain_widen([d[1] for d in dev], p_own, p_dst, dt, n, acc) == 0
    torch.cuda.synchronize()
    assert_f32_bits(host_of(t_dst, PAD + dst_off, prior), want, case)
    assert _zero_outside(t_dst, PAD + dst_off, n * 4), case
    for a, (t, _), ph in zip(sends + [own], dev + [(t_own, p_own)], [src_ph] * nsend + [own_ph]):
        assert host_of(t, PAD + ph, a).tobytes() == a.tobytes() and _zero_outside(t, PAD + ph, n * 2), case


@pytest.mark.gpu
@pytest.mark.parametrize("acc", ACCS, ids=lambda a: f"acc{a}")
@pytest.mark.parametrize("dt", DTS)
def test_widen_chain_all_patterns(gpu, dt, acc):
    """All 65,536 patterns as sends[0] against a zero own, nsend = 1: exact bits for non-NaN, NaN stays NaN (fp16
    denormals included).  With accumulate the previous dst holds fp32 denormals and small normals."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    p = all_patterns()
    zeros = np.zeros_like(p)
    rng = np.random.default_rng([SEED, dt, 65536])
    prior = (rng.standard_normal(p.size) * np.float32(2.0 ** -130)).astype(np.float32)
    assert (np.abs(prior[prior != 0]) < np.finfo(np.float32).tiny).mean() > 0.5  # fp32 denormals
    want = widened_expected([p, zeros], dt, prior if acc else None)
    t_src, p_src = dev_bytes(p, PAD)
    t_own, p_own = dev_bytes(zeros, PAD)
    t_dst, p_dst = dev_bytes(prior, PAD)
    torch.cuda.synchronize()
    assert dccl_amd.local_reduce_chain_widen([p_src], p_own, p_dst, dt, p.size, acc) == 0
    torch.cuda.synchronize()
    got = host_of(t_dst, PAD, prior)
    assert_f32_bits(got, want)
    assert not np.isnan(got[~np.isnan(want)]).any()
    assert _zero_outside(t_dst, PAD, p.size * 4) and _zero_outside(t_src, PAD, p.size * 2)
    assert host_of(t_src, PAD, p).tobytes() == p.tobytes()


STRIDE_N = 160000  # 20,000 vectors = 313 one-wave tiles over 8 blocks: 40 grid-stride passes


def run_stride_cases():
    """The child's body: the bf16 widened chain (nsend = 3) at STRIDE_N under a grid of 8 blocks, both accumulates."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    dt, nsend, n = BF16, 3, STRIDE_N
    rng = np.random.default_rng([SEED, 8])
    ops = family_ops(rng, dt, "cancelling", nsend + 1, n)
    prior = (rng.standard_normal(n) * SMALL[dt]).astype(np.float32)
    dev = [dev_bytes(a, 0) for a in ops]
    ran = 0
    for acc in ACCS:
        t_dst, p_dst = dev_bytes(prior, 0)
        torch.cuda.synchronize()
        assert dccl_amd.local_reduce_chain_widen([d[1] for d in dev[:nsend]], dev[nsend][1], p_dst, dt, n, acc) == 0
        torch.cuda.synchronize()
        assert_f32_bits(host_of(t_dst, 0, prior), widened_expected(ops, dt, prior if acc else None), f"acc {acc}")
        assert _zero_outside(t_dst, 0, n * 4)
        ran += 1
    return ran


STRIDE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import dccl_amd
assert dccl_amd.lib.dccl_max_grid_test() == 8, "the grid clamp is not live in this process"
assert dccl_amd.lib.dccl_caps_test_shift() == int(sys.argv[2]), "the size scale is not live in this process"
from tests import test_widened_sum as widened
print("RAN", widened.run_stride_cases())
"""


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 10])
def test_widen_grid_stride(gpu, shift):
    """One fresh child with DCCL_MAX_GRID_TEST=8 (and DCCL_CAPS_TEST_SHIFT unset or 10, so the chain's caps rows for
    large operands are taken too): every block walks about 40 tiles."""
    env = {**os.environ, "DCCL_MAX_GRID_TEST": "8", "PYTHONPATH": ROOT}
    env.pop("DCCL_CAPS_TEST_SHIFT", None)
    if shift:
        env["DCCL_CAPS_TEST_SHIFT"] = str(shift)
    p = subprocess.run([sys.executable, "-c", STRIDE_CHILD, ROOT, str(shift)], env=env, capture_output=True, text=True,
                       timeout=180)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "RAN 2" in p.stdout.splitlines(), p.stdout[-500:]


# ----------------------------------------------------------------------------- GPU: collectives
def _f32_add_into(send, recv):
    with np.errstate(all="ignore"):
        recv += send  # one IEEE fp32 add per element


def expected_slots(inputs, dt):
    """The fp32 Sum ring reduce-scatter (ncclReduceScatter's rank maps) over the widened inputs: slot r of rank r."""
    W = len(inputs)
    bufs = [widen(x, dt) for x in inputs]
    ringsim.reduce_scatter_ring(bufs, _f32_add_into, *ringsim.rs_maps())
    slot = inputs[0].size // W
    return [bufs[r][r * slot:(r + 1) * slot].copy() for r in range(W)]


def plain_slots(inputs, dt):
    """The built-in ncclSum reduce-scatter on the same ring: rounded to 16 bits after every step."""
    W = len(inputs)
    bufs = [x.copy() for x in inputs]

    def combine(send, recv):
        with np.errstate(all="ignore"):
            recv[:] = narrow(widen(send, dt) + widen(recv, dt), dt)

    ringsim.reduce_scatter_ring(bufs, combine, *ringsim.rs_maps())
    slot = inputs[0].size // W
    return [bufs[r][r * slot:(r + 1) * slot].copy() for r in range(W)]


def prior_recv(seed, r, n):
    return np.random.default_rng([SEED, seed, r, n]).standard_normal(n).astype(np.float32)


def _run_widened(comm, r, W, dt, xs, n, ops, stream, torch):
    """reduce_scatter and reduce to root 1 % W with each op of `ops` (accumulate -> handle) on rank r; the recv
    buffers start as prior_recv.  Returns {(api, acc): fp32 recv}."""
    out = {}
    raw = xs[r].view(np.uint8)
    root = 1 % W
    for api in ("reduce_scatter", "reduce"):
        for acc, op in ops.items():
            m = n // W if api == "reduce_scatter" else n
            send = torch.from_numpy(raw.copy()).cuda()
            recv = torch.from_numpy(prior_recv(acc, r, m).copy()).cuda()
            torch.cuda.synchronize()
            if api == "reduce_scatter":
                rc = comm.reduce_scatter(send.data_ptr(), recv.data_ptr(), m, dt, op, stream)
            else:
                rc = comm.reduce(send.data_ptr(), recv.data_ptr(), n, dt, op, root, stream)
            assert rc == 0, (api, acc, rc)
            torch.cuda.synchronize()
            out[(api, acc)] = recv.cpu().numpy()
            assert send.cpu().numpy().tobytes() == raw.tobytes(), (api, "sendbuff changed")
    return out


def _check_widened(outs, xs, W, dt, n, what):
    slots = expected_slots(xs, dt)
    whole = np.concatenate(slots)
    root = 1 % W
    for acc in ACCS:
        for r in range(W):
            prior = prior_recv(acc, r, n // W)
            assert_f32_bits(outs[r][("reduce_scatter", acc)], f32_add(prior, slots[r]) if acc else slots[r],
                            (what, "reduce_scatter", acc, r))
            prior = prior_recv(acc, r, n)
            if r == root:
                assert_f32_bits(outs[r][("reduce", acc)], f32_add(prior, whole) if acc else whole, (what, "reduce", acc))
            else:  # a non-root recvbuff is untouched
                assert outs[r][("reduce", acc)].tobytes() == prior.tobytes(), (what, "non-root recv", acc, r)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring"])
@pytest.mark.parametrize("W,dt", [(4, BF16), (3, F16), (8, BF16), (2, F16)])
def test_widened_collectives_threads(gpu, monkeypatch, W, dt, algo):
    """Thread ranks on one GPU: reduce_scatter, and reduce to root 1 % W, with accumulate 0 and 1, bit for bit against
    the fp32 ring simulation over the widened inputs (plus the previous recvbuff).  algo "": the direct collectives
    (the fused chain kernel writes fp32); "ring": widen, the fp32 ring, and one fp32 add for accumulate.  n = W * 1031:
    odd slots, so head and tail elements exist."""
    import torch
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    n = W * 1031
    data = {family: collective_inputs(30, W, dt, n, family) for family in FAMILIES}

    def body(comm, r):
        st = torch.cuda.Stream()
        ops = {}
        for acc in ACCS:
            rc, ops[acc] = comm.red_op_create_widened_sum(dt, acc)
            assert rc == 0 and ops[acc] >= 5
        out = {family: _run_widened(comm, r, W, dt, xs, n, ops, st.cuda_stream, torch) for family, xs in data.items()}
        for op in ops.values():
            assert comm.red_op_destroy(op) == 0
        return out

    outs = run_ranks(W, body)
    for family, xs in data.items():
        _check_widened([o[family] for o in outs], xs, W, dt, n, (family, algo))


@pytest.mark.gpu
def test_widened_world1(gpu):
    """W = 1: both APIs, both accumulate values: the conversion, or the conversion and one fp32 add."""
    import torch
    import dccl_amd
    dt, n = F16, 4099
    x = all_patterns()[30000:30000 + n].copy()  # NaN patterns included
    comm = dccl_amd.Comm.in_process(1, 0)
    try:
        ops = {}
        for acc in ACCS:
            rc, ops[acc] = comm.red_op_create_widened_sum(dt, acc)
            assert rc == 0
        out = _run_widened(comm, 0, 1, dt, [x], n, ops, 0, torch)
        for api in ("reduce_scatter", "reduce"):
            for acc in ACCS:
                want = widen(x, dt)
                assert_f32_bits(out[(api, acc)], f32_add(prior_recv(acc, 0, n), want) if acc else want, (api, acc))
        for op in ops.values():
            assert comm.red_op_destroy(op) == 0
    finally:
        comm.finalize()


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring"])
def test_widened_group_and_other_sums(gpu, monkeypatch, algo):
    """W = 4, bf16: two widened reduce-scatters (accumulate 0 and 1) next to a plain ncclSum one inside
    ncclGroupStart / ncclGroupEnd give the separate calls' bits (and the oracle's); a plain ncclSum and a wide-sum
    all-reduce on the same communicator afterwards answer as today."""
    import torch
    import dccl_amd
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    W, dt = 4, BF16
    sizes = [W * 1031, W * 257, W * 515]
    data = [collective_inputs(40 + i, W, dt, n, "normal") for i, n in enumerate(sizes)]

    def body(comm, r):
        st = torch.cuda.Stream()
        rc0, op0 = comm.red_op_create_widened_sum(dt, 0)
        rc1, op1 = comm.red_op_create_widened_sum(dt, 1)
        rcw, wide = comm.red_op_create_wide_sum(dt)
        assert (rc0, rc1, rcw) == (0, 0, 0)
        ops = [op0, op1, SUM]
        outs = {}
        for mode in ("separate", "grouped"):
            sends = [torch.from_numpy(xs[r].view(np.uint8).copy()).cuda() for xs in data]
            recvs = [torch.from_numpy(prior_recv(50 + i, r, n // W).copy()).cuda() for i, n in enumerate(sizes)]
            torch.cuda.synchronize()
            if mode == "grouped":
                with dccl_amd.group():
                    for s, v, n, o in zip(sends, recvs, sizes, ops):
                        assert comm.reduce_scatter(s.data_ptr(), v.data_ptr(), n // W, dt, o, st.cuda_stream) == 0
            else:
                for s, v, n, o in zip(sends, recvs, sizes, ops):
                    assert comm.reduce_scatter(s.data_ptr(), v.data_ptr(), n // W, dt, o, st.cuda_stream) == 0
            torch.cuda.synchronize()
            outs[mode] = [v.cpu().numpy() for v in recvs]
        for name, o in (("plain afterwards", SUM), ("wide afterwards", wide)):
            buf = torch.from_numpy(data[0][r].view(np.uint8).copy()).cuda()
            torch.cuda.synchronize()
            assert comm.all_reduce(buf.data_ptr(), buf.data_ptr(), sizes[0], dt, o, st.cuda_stream) == 0
            torch.cuda.synchronize()
            outs[name] = buf.cpu().numpy().view(np.uint16)
        for o in (op0, op1, wide):
            assert comm.red_op_destroy(o) == 0
        return outs

    outs = run_ranks(W, body)
    for i, (xs, n) in enumerate(zip(data, sizes)):
        slots = expected_slots(xs, dt)
        for r in range(W):
            assert outs[r]["grouped"][i].tobytes() == outs[r]["separate"][i].tobytes(), (i, r)
            got = outs[r]["separate"][i]
            prior = prior_recv(50 + i, r, n // W)
            if i == 0:
                assert_f32_bits(got, slots[r], (i, r))
            elif i == 1:
                assert_f32_bits(got, f32_add(prior, slots[r]), (i, r))
            else:  # the plain ncclSum reduce-scatter wrote bf16 into the first half of the buffer's bytes
                want = plain_slots(xs, dt)[r]
                half = got.view(np.uint16)
                assert fp_equal(half[:n // W], want, dt), (i, r)
                assert half[n // W:].tobytes() == prior.view(np.uint16)[n // W:].tobytes(), (i, r)
    plain = _expected_allreduce(data[0], dt, SUM)
    wide = expected_collective("all_reduce", data[0], dt, "ring")
    assert not fp_equal(plain[0], wide[0], dt)
    for r in range(W):
        assert fp_equal(outs[r]["plain afterwards"], plain[r], dt), r
        assert fp_equal(outs[r]["wide afterwards"], wide[r], dt), r


# ----------------------------------------------------------------------------- GPU: across processes
XP_DT = BF16


def _xp_inputs(W):
    return collective_inputs(60, W, XP_DT, W * 1031)


def _xp_reduce_scatter(comm, r, W, torch):
    rc, op = comm.red_op_create_widened_sum(XP_DT, 1)
    assert rc == 0, rc
    x = _xp_inputs(W)[r]
    m = x.size // W
    send = torch.from_numpy(x.view(np.uint8).copy()).cuda()
    recv = torch.from_numpy(prior_recv(61, r, m).copy()).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = comm.reduce_scatter(send.data_ptr(), recv.data_ptr(), m, XP_DT, op, st.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert comm.red_op_destroy(op) == 0
    assert send.cpu().numpy().tobytes() == x.view(np.uint8).tobytes()
    return recv.cpu().numpy()


def _check_xp(results, W):
    slots = expected_slots(_xp_inputs(W), XP_DT)
    for r in range(W):
        out, fin = results[r]
        assert fin == 0
        assert_f32_bits(out.view(np.float32), f32_add(prior_recv(61, r, slots[r].size), slots[r]), r)


@pytest.mark.gpu
def test_widened_ipc_processes(gpu):
    """One process per rank on the IPC transport, W = 3: the fused widened chain reads the peers' scratch copies and
    adds into the caller's fp32 recvbuff."""
    W = 3
    _check_xp(xproc.run_ipc(W, _xp_reduce_scatter), W)


@pytest.mark.gpu
def test_widened_rccl_processes(gpu):
    """The RCCL transport, W = 2: the staged path (widen, the fp32 ring, one fp32 add)."""
    import dccl_amd
    if not dccl_amd.lib.dccl_rccl_available():
        pytest.skip("librccl not loadable")
    W = 2
    _check_xp(xproc.run_rccl(W, _xp_reduce_scatter), W)
