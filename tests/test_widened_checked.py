"""Checked widened sums (dcclRedOpCreateWidenedSumChecked): the widened sum of
tests/test_widened_sum.py, whose reduction also raises a caller-supplied device word when a finished fp32 accumulator
is not finite (exponent field all ones: +-inf or any NaN):

    flag = 1  when  any(~isfinite(wide_acc(ops)));  nothing is stored otherwise, and never another value.

Every expectation is numpy's: the flag from np.isfinite over tests/test_wide_sum.py's wide_acc (or over the fp32 ring
simulation of the widened inputs), the values from tests/test_widened_sum.py's widened_expected / expected_slots, bit
for bit where the expectation is not NaN and by NaN-ness where it is.  The previous content of dst (accumulate) never
enters the flag.  Every flag word sits between two guard words (0xA5A5A5A5) that must survive.

CPU: the validation tables of dccl_local_reduce_chain_widen_checked and dccl_local_nonfinite_f32 row by row on
addresses that are never dereferenced, the op's creation errors, lifecycle and 17th op, the collective-level errors
(the flag inside recvbuff included), and the Python bindings.
GPU: the chain at test_widened_sum.CHAIN_CASES' nine placements (finite; one poisoned element at each of five
positions, four poison kinds), accumulate over a dst that holds inf, every 16-bit pattern classified, the grid-stride
passes in a child process, dccl_local_nonfinite_f32 at every head / tail length, thread ranks (W = 1, 2, 3; direct
and ring), a coalesced group over a dirtied pack, and one IPC and one RCCL two-process reduce-scatter.
"""
import ctypes
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

from tests import xproc
from tests.test_collectives import run_ranks
from tests.test_wide_sum import BF16, DTS, F16, F32, ROOT, SEED, all_patterns, chain_stream, collective_inputs, \
    wide_acc, widen
from tests.test_widened_sum import ACCS, CHAIN_CASES, PAD, assert_f32_bits, expected_slots, f32_add, prior_dst, \
    prior_recv, widened_expected

GUARD = 0xA5A5A5A5
INF16 = {F16: 0x7C00, BF16: 0x7F80}
NINF16 = {F16: 0xFC00, BF16: 0xFF80}
NAN16 = {F16: 0x7E01, BF16: 0x7FC1}


def nonfinite(acc) -> int:
    """The contract's flag for finished accumulators `acc`."""
    return int((~np.isfinite(np.asarray(acc, np.float32))).any())


def exp_all_ones(bits, dt):
    m = 0x7C00 if dt == F16 else 0x7F80
    return (bits & m) == m


# ----------------------------------------------------------------------------- CPU
def test_widen_checked_argument_checks_cpu():
    """dccl_local_reduce_chain_widen's rows in their order, with the flag's two rows where the header puts them."""
    import dccl_amd as d
    n = 16
    a, b, c, f = 1 << 40, (1 << 40) + (1 << 20), (1 << 40) + (2 << 20), (1 << 40) + (3 << 20)
    chain = d.local_reduce_chain_widen_checked
    raw = d.lib.dccl_local_reduce_chain_widen_checked
    # 1. dtype not fp16 / bf16 wins over everything after it
    for dt in (0, 2, 7, 8, 10, 11, -1):
        assert chain([a], b, c, dt, n, 0, f) == 4, dt
        assert chain([], 0, 0, dt, n, 7, 0) == 4, dt
    for dt in DTS:
        # 2. accumulate not 0 / 1: ahead of nsend / sends, the flag and count == 0
        for acc in (2, -1, 256):
            assert chain([a], b, c, dt, n, acc, f) == 4, acc
            assert chain([a], b, c, dt, 0, acc, f) == 4, acc
            assert raw(None, 1, b, c, dt, 0, acc, None, None) == 4, acc
        for acc in ACCS:
            # 3. nsend outside 1..8, NULL sends: ahead of count == 0
            assert chain([], b, c, dt, n, acc, f) == 4
            assert chain([a] * 9, b, c, dt, n, acc, f) == 4
            assert raw(None, 1, b, c, dt, n, acc, f, None) == 4
            assert raw(None, 1, b, c, dt, 0, acc, f, None) == 4
            # 4. NULL or misaligned flag: ahead of count == 0 too
            for bad in (0, f + 1, f + 2, f + 3):
                assert chain([a], b, c, dt, n, acc, bad) == 4, bad - f
                assert chain([a], b, c, dt, 0, acc, bad) == 4, bad - f
                assert chain([0], 0, 0, dt, 0, acc, bad) == 4, bad - f
            # 5. count == 0 succeeds, ahead of the operand checks (the flag may then lie anywhere aligned)
            assert chain([0], 0, 0, dt, 0, acc, f) == 0
            assert chain([c], c, c, dt, 0, acc, c) == 0
            # 6. NULL operands
            assert chain([0], b, c, dt, n, acc, f) == 4
            assert chain([a, 0], b, c, dt, n, acc, f) == 4
            assert chain([a], 0, c, dt, n, acc, f) == 4
            assert chain([a], b, 0, dt, n, acc, f) == 4
            # 7. a source or own sharing any byte with [dst, dst + 4 n)
            for sh in (0, 2, 4, 4 * n - 1, 4 * n - 2, -2, -(2 * n - 1), -(2 * n - 2), 1):
                assert chain([a, c + sh], b, c, dt, n, acc, f) == 4, sh
                assert chain([a], c + sh, c, dt, n, acc, f) == 4, sh
            # 8. [flag, flag + 4) sharing a byte with [dst, dst + 4 n): its first, an inner and its last element
            for j in (0, 1, n // 2, n - 1):
                assert chain([a], b, c, dt, n, acc, c + 4 * j) == 4, j
    # 9. launch failure: only where no GPU exists; a flag adjacent to dst on either side, or inside a SOURCE, passes
    # validation and reaches the launch
    import torch
    if not torch.cuda.is_available():
        assert chain([a], b, c, BF16, n, 0, f) == 1
        assert chain([a], b, c, F16, n, 1, c - 4) == 1
        assert chain([a], b, c, BF16, n, 1, c + 4 * n) == 1
        assert chain([a], b, c, BF16, n, 0, a) == 1


def test_nonfinite_f32_argument_checks_cpu():
    import dccl_amd as d
    scan = d.local_nonfinite_f32
    n = 16
    s, f = 1 << 40, (1 << 40) + (1 << 20)
    # 1. NULL or misaligned flag, ahead of count == 0
    for bad in (0, f + 1, f + 2, f + 3):
        assert scan(s, n, bad) == 4, bad
        assert scan(s, 0, bad) == 4, bad
        assert scan(0, 0, bad) == 4, bad
    # 2. count == 0 succeeds, ahead of the source checks
    assert scan(0, 0, f) == 0
    assert scan(s + 1, 0, f) == 0
    assert scan(f, 0, f) == 0
    # 3. NULL src, src off its 4-byte boundary
    assert scan(0, n, f) == 4
    for off in (1, 2, 3):
        assert scan(s + off, n, f) == 4, off
    # 4. the flag inside [src, src + 4 n)
    for j in (0, 1, n // 2, n - 1):
        assert scan(s, n, s + 4 * j) == 4, j
    # 5. launch failure: only where no GPU exists; the words next to src on either side are fine
    import torch
    if not torch.cuda.is_available():
        assert scan(s, n, f) == 1
        assert scan(s, n, s - 4) == 1
        assert scan(s, n, s + 4 * n) == 1


def test_checked_op_lifecycle_and_collective_errors_cpu():
    import dccl_amd as d
    comm = d.Comm.in_process(1, 0)
    try:
        s = np.array([0.25], np.float32)
        h = np.arange(16, dtype=np.uint16)
        y = np.zeros(8, np.float32)
        word = np.zeros(4, np.uint32)
        f = word.ctypes.data + 4
        make = comm.red_op_create_widened_sum_checked
        raw = d.lib.dccl_red_op_create_widened_sum_checked
        # creation: dcclRedOpCreateWidenedSum's rows, then the flag
        assert raw(None, BF16, 0, f, comm.handle) == 4
        for dt in (0, 2, 7, 8, 10, 11, -1):
            assert make(dt, 0, f)[0] == 4, dt
        for acc in (2, -1, 256):
            assert make(BF16, acc, f)[0] == 4, acc
        for bad in (0, f + 1, f + 2, f + 3):
            assert make(BF16, 0, bad)[0] == 4, bad - f
        out = ctypes.c_int(0)
        assert raw(ctypes.byref(out), BF16, 0, f, None) == 4  # null communicator
        for acc in ACCS:
            rc, op = make(BF16, acc, f)
            assert rc == 0 and 5 <= op <= 20
            # everything the widened sum rejects
            assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 5
            assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 0, BF16, op) == 5
            assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 5  # host buffers
            assert comm.reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op, 0) == 5
            base = y.ctypes.data
            for send, recv in ((base, base), (base + 31, base), (base, base + 15), (base + 4, base)):
                assert comm.reduce_scatter(send, recv, 8, BF16, op) == 4, (send - base, recv - base)
                assert comm.reduce(send, recv, 8, BF16, op, 0) == 4, (send - base, recv - base)
            for dt in (F16, F32, 2, 10, 11):
                assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 4, dt, op) == 4, dt
                assert comm.reduce(h.ctypes.data, y.ctypes.data, 4, dt, op, 0) == 4, dt
            # count == 0 succeeds wherever the flag lies
            assert comm.reduce_scatter(h.ctypes.data, f, 0, BF16, op) == 0
            assert comm.red_op_destroy(op) == 0
            # the flag's 4 bytes inside recvbuff's fp32 range: ncclInvalidArgument, ahead of the placement checks
            for j in (0, 3, 7):
                rc, op = make(BF16, acc, base + 4 * j)
                assert rc == 0
                assert comm.reduce_scatter(h.ctypes.data, base, 8, BF16, op) == 4, j
                assert comm.reduce(h.ctypes.data, base, 8, BF16, op, 0) == 4, j
                # a recvbuff that ends before the flag, or starts after it, gets as far as the host-buffer answer
                if j == 7:
                    assert comm.reduce_scatter(h.ctypes.data, base, 7, BF16, op) == 5
                if j == 0:
                    assert comm.reduce_scatter(h.ctypes.data, base + 4, 7, BF16, op) == 5
                assert comm.red_op_destroy(op) == 0
            assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 4  # dead
            assert comm.red_op_destroy(op) == 4
        assert not y.any() and not word.any()
        # the 16 slots are shared with the other creators; the 17th live op of any kind is ncclInvalidUsage
        ops = []
        for k in range(16):
            if k % 4 == 0:
                rc, hnd = comm.red_op_create_premul_sum(s.ctypes.data, F32, 1)
            elif k % 4 == 1:
                rc, hnd = comm.red_op_create_widened_sum(BF16, k // 4 % 2)
            elif k % 4 == 2:
                rc, hnd = comm.red_op_create_wide_scaled_sum(s.ctypes.data, F16, 1)
            else:
                rc, hnd = make(F16 if k % 8 == 3 else BF16, (k // 4) % 2, f)
            assert rc == 0
            ops.append(hnd)
        assert sorted(ops) == list(range(5, 21))
        assert make(BF16, 1, f)[0] == 5
        assert comm.red_op_create_widened_sum(BF16, 0)[0] == 5
        # destroy, then create again: the slot is reused and carries the new op's kind, datatype and flag
        assert comm.red_op_destroy(ops[3]) == 0  # a checked fp16 op
        rc, again = comm.red_op_create_wide_sum(F16)
        assert rc == 0 and again == ops[3]
        assert comm.all_reduce(h.ctypes.data, h.ctypes.data, 8, F16, again) == 5  # a wide sum: only the host buffers
        assert comm.red_op_destroy(ops[1]) == 0  # an unchecked widened sum
        rc, again = make(BF16, 0, y.ctypes.data)
        assert rc == 0 and again == ops[1]
        assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 8, BF16, again) == 4  # its flag is in recvbuff now
        assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data + 4, 7, BF16, again) == 5
        assert not y.any() and not word.any()
    finally:
        comm.finalize()


def test_checked_bindings_cpu():
    import dccl_amd as d
    for name in ("dccl_local_reduce_chain_widen_checked", "dccl_local_nonfinite_f32",
                 "dccl_red_op_create_widened_sum_checked"):
        assert name in d.EXPORTED_SYMBOLS and hasattr(d.lib, name), name
    assert callable(d.local_reduce_chain_widen_checked) and callable(d.local_nonfinite_f32)
    assert callable(d.Comm.red_op_create_widened_sum_checked)


# ----------------------------------------------------------------------------- GPU: helpers
def flag_block(torch, init=0, n=1):
    """n flag words, each `init`, between guard words: (tensor, address of the first flag)."""
    host = np.full(n + 2, GUARD, np.uint32)
    host[1:-1] = init
    t = torch.from_numpy(host.view(np.int32).copy()).cuda()
    return t, t.data_ptr() + 4


def flags_of(t):
    """The flag words of a flag_block; the guards must be intact."""
    host = t.cpu().numpy().view(np.uint32)
    assert host[0] == GUARD and host[-1] == GUARD, [hex(int(x)) for x in (host[0], host[-1])]
    return host[1:-1].copy()


def _zero_outside(t, off: int, nbytes: int) -> bool:
    return not t[:off].any() and not t[off + nbytes:].any()


def _case_operands(dt, case):
    """Finite operands (the "normal" family of test_widened_sum's streams) and a previous dst for a CHAIN_CASES row."""
    nsend, n = case[0], case[1]
    stream = chain_stream(dt, "normal", nsend, n)
    ops = [np.ascontiguousarray(x[:n]) for x in stream]
    prior = np.ascontiguousarray(prior_dst(dt, "normal", nsend, n, stream[0].size)[:n])
    assert np.isfinite(wide_acc(ops, dt)).all() and np.isfinite(prior).all()
    return ops, prior


def _run_chain(torch, dccl_amd, ops, prior, dt, case, acc, init=0):
    """One checked launch at the case's placement: (fp32 dst, the flag word)."""
    from tests.test_gpu_parity import dev_bytes, host_of
    nsend, n, dst_off, src_ph, own_ph, _ = case
    dev = [dev_bytes(a, PAD + src_ph) for a in ops[:nsend]]
    t_own, p_own = dev_bytes(ops[nsend], PAD + own_ph)
    t_dst, p_dst = dev_bytes(prior, PAD + dst_off)
    t_flag, p_flag = flag_block(torch, init)
    torch.cuda.synchronize()
    rc = dccl_amd.local_reduce_chain_widen_checked([d[1] for d in dev], p_own, p_dst, dt, n, acc, p_flag)
    assert rc == 0, (rc, case)
    torch.cuda.synchronize()
    assert _zero_outside(t_dst, PAD + dst_off, n * 4), case
    for a, (t, _), ph in zip(ops, dev + [(t_own, p_own)], [src_ph] * nsend + [own_ph]):
        assert host_of(t, PAD + ph, a).tobytes() == a.tobytes() and _zero_outside(t, PAD + ph, n * 2), case
    return host_of(t_dst, PAD + dst_off, prior), int(flags_of(t_flag)[0])


CASE_IDS = [f"k{c[0]}-n{c[1]}-dst{c[2]}-src{c[3]}-own{c[4]}" for c in CHAIN_CASES]


# ----------------------------------------------------------------------------- GPU: the chain
@pytest.mark.gpu
@pytest.mark.parametrize("acc", ACCS, ids=lambda a: f"acc{a}")
@pytest.mark.parametrize("case", CHAIN_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dt", DTS)
def test_checked_chain_finite(gpu, dt, case, acc):
    """Finite inputs: the unchecked contract's bits; a zeroed flag stays 0 and a flag preset to 1 stays 1 (nothing is
    stored, nothing is cleared); the guard words around the flag are intact."""
    import torch
    import dccl_amd
    ops, prior = _case_operands(dt, case)
    want = widened_expected(ops, dt, prior if acc else None)
    assert nonfinite(wide_acc(ops, dt)) == 0
    for init in (0, 1):
        got, flag = _run_chain(torch, dccl_amd, ops, prior, dt, case, acc, init)
        assert_f32_bits(got, want, (case, init))
        assert flag == init, (case, init, flag)


def poison_positions(case):
    """Index 0 (a head element where the case has a head), the first vector's first lane, the last lane of the last,
    partial tile, the last index (a tail element) and the middle."""
    _, n, _, _, own_ph, _ = case
    head = min(((16 - own_ph) % 16) // 2, n)
    nvec = (n - head) // 8
    pos = [0, min(head, n - 1), n - 1, n // 2]
    if nvec:
        pos.append(head + nvec * 8 - 1)
    return sorted(set(pos))


def poison_kinds(dt, nops):
    """(name, {operand index: 16-bit pattern})"""
    kinds = [("+inf", {0: INF16[dt]}), ("nan", {nops - 1: NAN16[dt]}), ("+inf and -inf", {0: INF16[dt], nops - 1: NINF16[dt]})]
    if dt == BF16:
        kinds.append(("two of 0x7f7f", {0: 0x7F7F, nops - 1: 0x7F7F}))  # finite, their sum overflows fp32
    return kinds


@pytest.mark.gpu
@pytest.mark.parametrize("acc", ACCS, ids=lambda a: f"acc{a}")
@pytest.mark.parametrize("case", CHAIN_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("dt", DTS)
def test_checked_chain_one_poisoned_element(gpu, dt, case, acc):
    """One poisoned element at a time, at each of poison_positions, for each of poison_kinds: the flag is 1 and the
    values are the contract's (NaN where it says NaN)."""
    import torch
    import dccl_amd
    ops, prior = _case_operands(dt, case)
    ran = 0
    for pos in poison_positions(case):
        for name, patch in poison_kinds(dt, len(ops)):
            bad = [x.copy() for x in ops]
            for k, bits in patch.items():
                bad[k][pos] = bits
            acc32 = wide_acc(bad, dt)
            assert nonfinite(acc32) == 1 and not np.isfinite(acc32[pos]), (name, pos)  # numpy says so
            assert np.isfinite(np.delete(acc32, pos)).all()
            got, flag = _run_chain(torch, dccl_amd, bad, prior, dt, case, acc)
            assert flag == 1, (case, name, pos)
            assert_f32_bits(got, widened_expected(bad, dt, prior if acc else None), (case, name, pos))
            ran += 1
    assert ran == len(poison_positions(case)) * (4 if dt == BF16 else 3) and ran >= 3  # count 1 has one position


@pytest.mark.gpu
@pytest.mark.parametrize("case", [CHAIN_CASES[2], CHAIN_CASES[4], CHAIN_CASES[5], CHAIN_CASES[6]],
                         ids=[CASE_IDS[i] for i in (2, 4, 5, 6)])
@pytest.mark.parametrize("dt", DTS)
def test_checked_chain_prior_inf_does_not_raise(gpu, dt, case):
    """accumulate == 1 over a dst that already holds +-inf and NaN, with finite contributions: the flag stays 0 (it
    reports the contributions); the values are still prior + acc."""
    import torch
    import dccl_amd
    ops, prior = _case_operands(dt, case)
    prior = prior.copy()
    prior[::3] = np.inf
    prior[1::7] = -np.inf
    prior[-1] = np.nan
    prior[0] = np.inf
    got, flag = _run_chain(torch, dccl_amd, ops, prior, dt, case, 1)
    assert flag == 0, case
    assert_f32_bits(got, widened_expected(ops, dt, prior), case)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_checked_chain_classifies_every_pattern(gpu, dt):
    """k = 1, own = the pattern, sends[0] = 0.  One launch over all finite patterns leaves the flag 0; one tiny launch
    per non-finite pattern (2048 for fp16, 256 for bf16), each with its own flag word, sets every word."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    p = all_patterns()
    bad = exp_all_ones(p, dt)
    assert int(bad.sum()) == (2048 if dt == F16 else 256)
    assert (~np.isfinite(widen(p, dt)) == bad).all()  # numpy's classification is the exponent test
    fin, non = np.ascontiguousarray(p[~bad]), np.ascontiguousarray(p[bad])
    zeros = np.zeros_like(p)
    t_zero, p_zero = dev_bytes(zeros, PAD)
    t_fin, p_fin = dev_bytes(fin, PAD)
    t_non, p_non = dev_bytes(non, PAD)
    t_dst, p_dst = dev_bytes(np.zeros(p.size, np.float32), PAD)
    t_flag, p_flag = flag_block(torch, 0)
    t_each, p_each = flag_block(torch, 0, non.size)
    torch.cuda.synchronize()
    assert dccl_amd.local_reduce_chain_widen_checked([p_zero], p_fin, p_dst, dt, fin.size, 0, p_flag) == 0
    torch.cuda.synchronize()
    assert int(flags_of(t_flag)[0]) == 0
    assert_f32_bits(host_of(t_dst, PAD, np.zeros(fin.size, np.float32)), wide_acc([zeros[:fin.size], fin], dt))
    for i in range(non.size):
        rc = dccl_amd.local_reduce_chain_widen_checked([p_zero], p_non + 2 * i, p_dst + 4 * i, dt, 1, 0, p_each + 4 * i)
        assert rc == 0, i
    torch.cuda.synchronize()
    each = flags_of(t_each)
    assert (each == 1).all(), np.flatnonzero(each != 1)[:8]
    assert int(flags_of(t_flag)[0]) == 0


# ----------------------------------------------------------------------------- GPU: dccl_local_nonfinite_f32
SCAN_COUNTS = (1, 3, 4, 5, 1027, 4099)
SCAN_OFFSETS = (0, 4, 8, 12)


def scan_data(n, off):
    """Finite fp32, the largest finite value and denormals among them."""
    rng = np.random.default_rng([SEED, 120, n, off])
    x = rng.standard_normal(n).astype(np.float32)
    u = x.view(np.uint32)
    u[::5] = 0x7F7FFFFF
    u[1::5] = 0x00000001
    u[2::5] = 0x807FFFFF
    assert np.isfinite(x).all()
    return x


def _scan(torch, dccl_amd, x, off, init=0):
    from tests.test_gpu_parity import dev_bytes, host_of
    t_src, p_src = dev_bytes(x, PAD + off)
    assert p_src % 16 == off
    t_flag, p_flag = flag_block(torch, init)
    torch.cuda.synchronize()
    assert dccl_amd.local_nonfinite_f32(p_src, x.size, p_flag) == 0
    torch.cuda.synchronize()
    assert host_of(t_src, PAD + off, x).tobytes() == x.tobytes() and _zero_outside(t_src, PAD + off, x.size * 4)
    return int(flags_of(t_flag)[0])


@pytest.mark.gpu
@pytest.mark.parametrize("off", SCAN_OFFSETS)
@pytest.mark.parametrize("n", SCAN_COUNTS)
def test_nonfinite_f32_head_body_tail(gpu, n, off):
    """Every head length (source 0 / 4 / 8 / 12 bytes past a 16-B boundary) against counts with no, one and many
    whole vectors: finite data leaves the flag as it was (0 or 1); +inf at the first, a middle and the last element
    raises it; the source is only read."""
    import torch
    import dccl_amd
    x = scan_data(n, off)
    assert _scan(torch, dccl_amd, x, off, 0) == nonfinite(x) == 0
    assert _scan(torch, dccl_amd, x, off, 1) == 1
    for pos in sorted({0, n // 2, n - 1, min(3, n - 1), max(0, n - 4)}):
        y = x.copy()
        y[pos] = np.inf
        assert _scan(torch, dccl_amd, y, off) == nonfinite(y) == 1, pos


@pytest.mark.gpu
def test_nonfinite_f32_special_values(gpu):
    import torch
    import dccl_amd
    raises = (0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF)
    quiet = (0x7F7FFFFF, 0xFF7FFFFF, 0x00000001, 0x807FFFFF, 0x00800000, 0x00000000, 0x80000000, 0x3F800000)
    for n, off, pos in ((5, 4, 0), (5, 4, 4), (1027, 8, 513)):
        for bits in raises + quiet:
            x = np.zeros(n, np.float32)
            x.view(np.uint32)[pos] = bits
            want = nonfinite(x)
            assert want == int(bits in raises)
            assert _scan(torch, dccl_amd, x, off) == want, (hex(bits), n, pos)


# ----------------------------------------------------------------------------- GPU: the grid-stride passes
STRIDE_N = 3 * 8 * 512 + 5  # under a grid of 8 one-wave blocks: three passes of the chain's 512-element tiles and a tail


def run_stride_cases():
    """The child's body (DCCL_MAX_GRID_TEST=8): poison only in a block's third pass, and no poison, for the checked
    chain (bf16, nsend = 2, both accumulates) and for dccl_local_nonfinite_f32 (tiles of 256 elements)."""
    import torch
    import dccl_amd
    dt, nsend, n = BF16, 2, STRIDE_N
    case = (nsend, n, 0, 0, 0, "vector, no head")
    rng = np.random.default_rng([SEED, 121])
    ops = [(rng.standard_normal(n).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16) for _ in range(nsend + 1)]
    prior = rng.standard_normal(n).astype(np.float32)
    assert nonfinite(wide_acc(ops, dt)) == 0
    ran = 0
    for acc in ACCS:
        for pos in (None, 2 * 8 * 512 + 100, 3 * 8 * 512 - 1):  # the third pass of blocks 0 and 7
            bad = [x.copy() for x in ops]
            if pos is not None:
                bad[1][pos] = INF16[dt]
            got, flag = _run_chain(torch, dccl_amd, bad, prior, dt, case, acc)
            assert flag == nonfinite(wide_acc(bad, dt)) == int(pos is not None), (acc, pos)
            assert_f32_bits(got, widened_expected(bad, dt, prior if acc else None), (acc, pos))
            ran += 1
    x = scan_data(n, 0)
    for pos in (None, 2 * 8 * 256 + 100, 3 * 8 * 256 - 1):
        y = x.copy()
        if pos is not None:
            y[pos] = -np.inf
        assert _scan(torch, dccl_amd, y, 0) == nonfinite(y) == int(pos is not None), pos
        ran += 1
    return ran


STRIDE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import dccl_amd
assert dccl_amd.lib.dccl_max_grid_test() == 8, "the grid clamp is not live in this process"
from tests import test_widened_checked as checked
print("RAN", checked.run_stride_cases())
"""


@pytest.mark.gpu
def test_checked_grid_stride(gpu):
    env = {**os.environ, "DCCL_MAX_GRID_TEST": "8", "PYTHONPATH": ROOT}
    env.pop("DCCL_CAPS_TEST_SHIFT", None)
    p = subprocess.run([sys.executable, "-c", STRIDE_CHILD, ROOT], env=env, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "RAN 9" in p.stdout.splitlines(), p.stdout[-500:]


# ----------------------------------------------------------------------------- GPU: collectives
def _poisoned(xs, dt, rank, index):
    out = [x.copy() for x in xs]
    out[rank][index] = INF16[dt]
    return out


def _run_checked(comm, r, W, dt, xs, n, stream, torch):
    """reduce_scatter and reduce to root 1 % W on rank r with a checked op per accumulate value, each call with a
    flag block of its own.  Returns {(api, acc): (fp32 recv, flag)}."""
    out = {}
    raw = xs[r].view(np.uint8)
    root = 1 % W
    for acc in ACCS:
        for api in ("reduce_scatter", "reduce"):
            t_flag, p_flag = flag_block(torch, 0)
            rc, op = comm.red_op_create_widened_sum_checked(dt, acc, p_flag)
            assert rc == 0 and op >= 5
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
            out[(api, acc)] = (recv.cpu().numpy(), int(flags_of(t_flag)[0]))
            assert send.cpu().numpy().tobytes() == raw.tobytes(), (api, "sendbuff changed")
            assert comm.red_op_destroy(op) == 0
    return out


def _check_checked(outs, xs, W, dt, n, what):
    slots = expected_slots(xs, dt)
    whole = np.concatenate(slots)
    root = 1 % W
    for acc in ACCS:
        for r in range(W):
            got, flag = outs[r][("reduce_scatter", acc)]
            prior = prior_recv(acc, r, n // W)
            assert_f32_bits(got, f32_add(prior, slots[r]) if acc else slots[r], (what, "reduce_scatter", acc, r))
            assert flag == nonfinite(slots[r]), (what, "reduce_scatter", acc, r, flag)
            got, flag = outs[r][("reduce", acc)]
            prior = prior_recv(acc, r, n)
            if r == root:
                assert_f32_bits(got, f32_add(prior, whole) if acc else whole, (what, "reduce", acc))
                assert flag == nonfinite(whole), (what, "reduce", acc, flag)
            else:  # a non-root recvbuff and a non-root flag are untouched
                assert got.tobytes() == prior.tobytes(), (what, "non-root recv", acc, r)
                assert flag == 0, (what, "non-root flag", acc, r)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring"])
@pytest.mark.parametrize("W,dt", [(2, F16), (3, BF16)])
def test_checked_collectives_threads(gpu, monkeypatch, W, dt, algo):
    """Thread ranks on one GPU, direct (algo "") and staged ("ring"), accumulate 0 and 1.  Finite inputs: no flag.
    One +inf in one rank's input: reduce_scatter raises exactly the flag of the rank that owns the element's slot,
    reduce raises the root's alone; the values are the unchecked contract's."""
    import torch
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    n = W * 1031
    clean = collective_inputs(130, W, dt, n, "normal")
    owner = W - 1
    data = {"finite": clean, "poisoned": _poisoned(clean, dt, 0, owner * 1031 + 517)}
    want = [nonfinite(s) for s in expected_slots(data["poisoned"], dt)]
    assert want == [int(r == owner) for r in range(W)]
    assert not any(nonfinite(s) for s in expected_slots(clean, dt))

    def body(comm, r):
        st = torch.cuda.Stream()
        return {k: _run_checked(comm, r, W, dt, xs, n, st.cuda_stream, torch) for k, xs in data.items()}

    outs = run_ranks(W, body)
    for k, xs in data.items():
        _check_checked([o[k] for o in outs], xs, W, dt, n, (k, algo))


@pytest.mark.gpu
def test_checked_world1(gpu):
    """W = 1, both APIs, both accumulate values: the conversion (and one fp32 add), scanned before that add: a finite
    input over a recvbuff that holds inf raises nothing, an input with NaN patterns raises the flag."""
    import torch
    import dccl_amd
    dt, n = F16, 4099
    inputs = {"finite": all_patterns()[20000:20000 + n].copy(), "nan": all_patterns()[30000:30000 + n].copy()}
    assert nonfinite(widen(inputs["finite"], dt)) == 0 and nonfinite(widen(inputs["nan"], dt)) == 1
    comm = dccl_amd.Comm.in_process(1, 0)
    try:
        for name, x in inputs.items():
            for acc in ACCS:
                for api in ("reduce_scatter", "reduce"):
                    t_flag, p_flag = flag_block(torch, 0)
                    rc, op = comm.red_op_create_widened_sum_checked(dt, acc, p_flag)
                    assert rc == 0
                    prior = prior_recv(acc, 0, n)
                    prior[::2] = np.inf
                    send = torch.from_numpy(x.view(np.uint8).copy()).cuda()
                    recv = torch.from_numpy(prior.copy()).cuda()
                    torch.cuda.synchronize()
                    if api == "reduce_scatter":
                        assert comm.reduce_scatter(send.data_ptr(), recv.data_ptr(), n, dt, op, 0) == 0
                    else:
                        assert comm.reduce(send.data_ptr(), recv.data_ptr(), n, dt, op, 0, 0) == 0
                    torch.cuda.synchronize()
                    want = widen(x, dt)
                    assert_f32_bits(recv.cpu().numpy(), f32_add(prior, want) if acc else want, (name, api, acc))
                    assert int(flags_of(t_flag)[0]) == nonfinite(want), (name, api, acc)
                    assert comm.red_op_destroy(op) == 0
    finally:
        comm.finalize()


GROUP_COUNTS = (257, 33, 515, 7, 101)  # recvcounts: 16-bit slots of 514, 66, 1030, 14 and 202 bytes, 94 pad bytes
DIRTY_COUNT = 1000


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring"])
def test_checked_group_over_a_dirty_pack(gpu, monkeypatch, algo):
    """W = 3, bf16.  A larger unchecked widened group of all-NaN tensors leaves NaN patterns where the next run's pad
    bytes lie.  Then five checked reduce-scatters with one handle and one flag, in a group: one coalesced run of five
    on every rank (the group_stats delta), the flag stays 0 for finite tensors (it would not if the pads were read as
    they are), one poisoned tensor raises the owning rank's flag alone, and the values are the separate calls'."""
    import torch
    import dccl_amd
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    W, dt = 3, BF16
    assert all((2 * c) % 128 for c in GROUP_COUNTS) and sum(2 * c for c in GROUP_COUNTS) % 128
    clean = [collective_inputs(140 + i, W, dt, c * W, "normal") for i, c in enumerate(GROUP_COUNTS)]
    owner = 2
    poisoned = [xs if i != 2 else _poisoned(xs, dt, 1, owner * GROUP_COUNTS[2] + 300) for i, xs in enumerate(clean)]
    barrier = threading.Barrier(W, timeout=120)  # a rank that failed earlier breaks it: nobody waits for ever
    stats = {}

    def issue(comm, r, data, op, st, grouped):
        sends = [torch.from_numpy(xs[r].view(np.uint8).copy()).cuda() for xs in data]
        recvs = [torch.from_numpy(prior_recv(150 + i, r, c).copy()).cuda() for i, c in enumerate(GROUP_COUNTS)]
        torch.cuda.synchronize()
        if grouped:
            with dccl_amd.group():
                for s, v, c in zip(sends, recvs, GROUP_COUNTS):
                    assert comm.reduce_scatter(s.data_ptr(), v.data_ptr(), c, dt, op, st.cuda_stream) == 0
        else:
            for s, v, c in zip(sends, recvs, GROUP_COUNTS):
                assert comm.reduce_scatter(s.data_ptr(), v.data_ptr(), c, dt, op, st.cuda_stream) == 0
        torch.cuda.synchronize()
        return [v.cpu().numpy() for v in recvs]

    def body(comm, r):
        st = torch.cuda.Stream()
        rc, plain = comm.red_op_create_widened_sum(dt, 0)
        assert rc == 0
        nan = torch.full((2, DIRTY_COUNT * W), 0x7FC0, dtype=torch.int16).cuda()
        sink = torch.zeros((2, DIRTY_COUNT), dtype=torch.float32).cuda()
        torch.cuda.synchronize()
        with dccl_amd.group():
            for i in range(2):
                assert comm.reduce_scatter(nan[i].data_ptr(), sink[i].data_ptr(), DIRTY_COUNT, dt, plain,
                                           st.cuda_stream) == 0
        torch.cuda.synchronize()
        assert torch.isnan(sink).all()
        out = {}
        for acc in ACCS:
            for name, data in (("finite", clean), ("poisoned", poisoned)):
                for grouped in (True, False):
                    t_flag, p_flag = flag_block(torch, 0)
                    rc, op = comm.red_op_create_widened_sum_checked(dt, acc, p_flag)
                    assert rc == 0
                    first = acc == 0 and name == "finite" and grouped
                    if first:
                        barrier.wait()
                        if r == 0:
                            stats["before"] = dccl_amd.group_stats()
                        barrier.wait()
                    vals = issue(comm, r, data, op, st, grouped)
                    if first:
                        barrier.wait()
                        if r == 0:
                            stats["after"] = dccl_amd.group_stats()
                        barrier.wait()
                    out[(acc, name, grouped)] = (vals, int(flags_of(t_flag)[0]))
                    assert comm.red_op_destroy(op) == 0
        assert comm.red_op_destroy(plain) == 0
        return out

    outs = run_ranks(W, body)
    delta = {k: stats["after"][k] - stats["before"][k] for k in stats["after"]}
    assert (delta["coalesced_runs"], delta["tensors_coalesced"]) == (W, W * len(GROUP_COUNTS)), delta
    for acc in ACCS:
        for name, data in (("finite", clean), ("poisoned", poisoned)):
            slots = [expected_slots(xs, dt) for xs in data]
            for r in range(W):
                want_flag = int(any(nonfinite(s[r]) for s in slots))
                assert want_flag == int(name == "poisoned" and r == owner)
                for grouped in (True, False):
                    vals, flag = outs[r][(acc, name, grouped)]
                    assert flag == want_flag, (acc, name, r, grouped, flag)
                    for i, c in enumerate(GROUP_COUNTS):
                        prior = prior_recv(150 + i, r, c)
                        assert_f32_bits(vals[i], f32_add(prior, slots[i][r]) if acc else slots[i][r],
                                        (acc, name, r, grouped, i))
                        assert vals[i].tobytes() == outs[r][(acc, name, False)][0][i].tobytes(), (acc, name, r, i)


# ----------------------------------------------------------------------------- GPU: across processes
XP_DT, XP_W, XP_COUNT = BF16, 2, 1031
XP_POISON = (1, 0 * XP_COUNT + 700)  # in rank 1's input, in the slot rank 0 owns: rank 0 sees it in its peer's data


def _xp_inputs():
    xs = collective_inputs(160, XP_W, XP_DT, XP_W * XP_COUNT, "normal")
    return _poisoned(xs, XP_DT, *XP_POISON)


def _xp_reduce_scatter(comm, r, W, torch):
    t_flag, p_flag = flag_block(torch, 0)
    rc, op = comm.red_op_create_widened_sum_checked(XP_DT, 1, p_flag)
    assert rc == 0, rc
    x = _xp_inputs()[r]
    send = torch.from_numpy(x.view(np.uint8).copy()).cuda()
    recv = torch.from_numpy(prior_recv(161, r, XP_COUNT).copy()).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = comm.reduce_scatter(send.data_ptr(), recv.data_ptr(), XP_COUNT, XP_DT, op, st.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert comm.red_op_destroy(op) == 0
    assert send.cpu().numpy().tobytes() == x.view(np.uint8).tobytes()
    return recv.cpu().numpy(), int(flags_of(t_flag)[0])


def _check_xp(results):
    slots = expected_slots(_xp_inputs(), XP_DT)
    assert [nonfinite(s) for s in slots] == [1, 0]
    for r in range(XP_W):
        (out, flag), fin = results[r]
        assert fin == 0
        assert_f32_bits(out.view(np.float32), f32_add(prior_recv(161, r, XP_COUNT), slots[r]), r)
        assert flag == nonfinite(slots[r]), (r, flag)


@pytest.mark.gpu
def test_checked_ipc_processes(gpu):
    """One process per rank on the IPC transport: the checked chain reads the peer's scratch copy."""
    _check_xp(xproc.run_ipc(XP_W, _xp_reduce_scatter))


@pytest.mark.gpu
def test_checked_rccl_processes(gpu):
    """The RCCL transport: the staged path (widen, the fp32 ring, the scan, one fp32 add)."""
    import dccl_amd
    if not dccl_amd.lib.dccl_rccl_available():
        pytest.skip("librccl not loadable")
    _check_xp(xproc.run_rccl(XP_W, _xp_reduce_scatter))
