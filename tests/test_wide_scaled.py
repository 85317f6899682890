"""Scaled wide sums (dcclRedOpCreateWideScaledSum): fp16 / bf16 contributions accumulated in fp32,
the finished accumulator multiplied by ONE fp32 scalar, rounded to 16 bits once.

The contract is bit-exact: acc = widen(x_first); acc = fp32_add(widen(x_next), acc) per contribution in the order the
algorithm combines them; result = round16(fp32_mul(acc, s)).  Every expected value here is numpy's:
narrow(wide_acc(ops) * np.float32(s)) for the chain, the ring and Rabenseifner simulations on the widened fp32 inputs
(multiplied and rounded once at the end) for the collectives.  Nothing expected comes from the code under test.

CPU: the argument tables of dccl_local_reduce_chain_wide_scaled / dccl_local_convert_scaled / the op creation, the op
table's lifecycle (shared with the pre-multiplied and the wide sums), the distinguishability conditions of the three
input families, and the scaled narrowing oracle against an independent float64 computation.
GPU: the chain and the scaled conversion against the oracle (vector and element-wise forms, guard bytes, both scalar
residences), their grid-stride passes in a child process, the collectives on thread ranks (direct, ring,
Rabenseifner; a mixed group; W = 1) and one IPC and one RCCL all-reduce across processes.

Distinguishability (s = 0.3 as fp32; asserted on streams of at least 4096 elements before any GPU comparison):
  normal           a kernel that rounds the scalar to 16 bits first differs in >= 15 % of elements, one that rounds
                   the accumulator to 16 bits, scales and rounds again in >= 15 %, the unscaled wide sum in >= 90 %.
  cancelling       (test_wide_sum's family, with the scale) for nsend >= 2 the reversed order and the pairwise tree
                   each differ in >= 40 %.  For fp16 about a third of the expected results are fp16 subnormals: they
                   pin the denormal behaviour of the narrowing.
  near-cancelling  standard normals rounded to the dtype; per element two distinct operands are +B and -B (B = 2^12
                   for fp16, 2^14 for bf16).  For nsend >= 2 a kernel that multiplies every contribution by s before
                   adding differs in >= 5 % (plain normals separate that variant in under 1 %).
s = 1 / (nsend + 1) runs as well but nothing relies on it: for a power-of-two divisor every variant above but the
unscaled one coincides with the contract.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import rabsim, ringsim, xproc
from tests.test_collectives import run_ranks
from tests.test_oracle import fp_equal
from tests.test_wide_sum import (BF16, CHAIN_CASES, CONVERT_PLACES, DST_OFF, DTS, F16, F32, GUARD_ELEMS, SEED, STRIDE_N,
                                 SUM, _call, _copy, _f32_add, _zero_outside, all_patterns, chain_stream,
                                 collective_inputs, expected_collective, family_ops, is_nan16, narrow, narrow_inputs,
                                 share_differs, to_bits, tree_acc, wide_acc, wide_sum, widen)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = np.float32(0.3)
FAMILIES3 = ("normal", "cancelling", "near-cancelling")
NEAR_BIG = {F16: 2.0 ** 12, BF16: 2.0 ** 14}
HOST, DEVICE = 1, 0  # ncclScalarHostImmediate, ncclScalarDevice


# ----------------------------------------------------------------------------- the oracle (numpy only)
def scaled_narrow(acc: np.ndarray, s, dt: int) -> np.ndarray:
    """round16(fp32_mul(acc, s)): one IEEE fp32 multiply, one nearest-even rounding."""
    with np.errstate(all="ignore"):
        return narrow(np.ascontiguousarray(acc, np.float32) * np.float32(s), dt)


def scaled_sum(ops, dt: int, s) -> np.ndarray:
    """The contract: operands in the algorithm's order (chain: sends[0] first, own last)."""
    return scaled_narrow(wide_acc(ops, dt), s, dt)


def mean_scalar(nops: int) -> np.float32:
    return np.float32(1.0) / np.float32(nops)


def near_cancelling_ops(rng, dt: int, nops: int, n: int):
    ops = [to_bits(rng.standard_normal(n), dt) for _ in range(nops)]
    if nops > 1:
        i = rng.integers(0, nops, n)
        j = (i + rng.integers(1, nops, n)) % nops
        idx = np.arange(n)
        stack = np.stack(ops)
        stack[i, idx] = to_bits([NEAR_BIG[dt]], dt)[0]
        stack[j, idx] = to_bits([-NEAR_BIG[dt]], dt)[0]
        ops = [np.ascontiguousarray(row) for row in stack]
    return ops


def scaled_stream(dt: int, family: str, nsend: int, count: int):
    """The stream of a chain case: nsend + 1 operands (sends, then own) of max(count, GUARD_ELEMS) elements."""
    if family != "near-cancelling":
        return chain_stream(dt, family, nsend, count)
    rng = np.random.default_rng([SEED, dt, 2, nsend, count])
    return near_cancelling_ops(rng, dt, nsend + 1, max(count, GUARD_ELEMS))


# the wrong kernels a test must tell from the contract
def scalar16_sum(ops, dt, s):
    """The scalar rounded to 16 bits first."""
    return scaled_narrow(wide_acc(ops, dt), widen(narrow(np.array([s], np.float32), dt), dt)[0], dt)


def twice_rounded_sum(ops, dt, s):
    """The accumulator rounded to 16 bits, scaled, rounded again."""
    return scaled_narrow(widen(wide_sum(ops, dt), dt), s, dt)


def premultiplied_sum(ops, dt, s):
    """Every contribution multiplied by s (in fp32) before it is added."""
    s = np.float32(s)
    with np.errstate(all="ignore"):
        acc = widen(ops[0], dt) * s
        for x in ops[1:]:
            acc = widen(x, dt) * s + acc
    return narrow(acc, dt)


def scaled_guard_shares(ops, dt: int, family: str, s=S):
    want = scaled_sum(ops, dt, s)
    if family == "normal":
        return {"scalar rounded to 16 bits": share_differs(scalar16_sum(ops, dt, s), want),
                "accumulator rounded twice": share_differs(twice_rounded_sum(ops, dt, s), want),
                "unscaled": share_differs(wide_sum(ops, dt), want)}
    if family == "cancelling":
        return {"reversed order": share_differs(scaled_sum(ops[::-1], dt, s), want),
                "pairwise tree": share_differs(scaled_narrow(tree_acc(ops, dt), s, dt), want)}
    return {"scaled before adding": share_differs(premultiplied_sum(ops, dt, s), want)}


def assert_scaled_distinguishable(ops, dt: int, family: str, nsend: int):
    assert ops[0].size >= GUARD_ELEMS
    shares = scaled_guard_shares(ops, dt, family)
    print(f"dtype {dt} {family} nsend {nsend} n {ops[0].size}: " +
          ", ".join(f"{k} differs in {v:.3f}" for k, v in shares.items()))
    if family == "normal":
        assert shares["scalar rounded to 16 bits"] >= 0.15, (dt, nsend, shares)
        assert shares["accumulator rounded twice"] >= 0.15, (dt, nsend, shares)
        assert shares["unscaled"] >= 0.90, (dt, nsend, shares)
    elif family == "cancelling":
        if nsend >= 2:
            assert shares["reversed order"] >= 0.40 and shares["pairwise tree"] >= 0.40, (dt, nsend, shares)
    elif nsend >= 2:
        assert shares["scaled before adding"] >= 0.05, (dt, nsend, shares)
    assert np.isfinite(widen(scaled_sum(ops, dt, S), dt)).all()
    assert np.isfinite(widen(scaled_sum(ops, dt, mean_scalar(nsend + 1)), dt)).all()


def round16_f64(v: np.ndarray, dt: int) -> np.ndarray:
    """float64 values -> 16-bit patterns with one nearest-even rounding, in float64 arithmetic alone: the value is
    divided by the spacing of the dtype at its magnitude (a power of two, so exact), np.rint rounds half to even."""
    mant, emin, emax = (10, -14, 15) if dt == F16 else (7, -126, 127)
    v = np.asarray(v, np.float64)
    with np.errstate(all="ignore"):
        _, e = np.frexp(v)  # v = m * 2^e, 0.5 <= |m| < 1
        q = np.ldexp(1.0, np.maximum(e - 1, emin) - mant)
        r = np.rint(v / q) * q
        r = np.where(np.abs(r) >= np.ldexp(1.0, emax + 1), np.copysign(np.inf, v), r)
        r = np.where(np.isfinite(v), r, v)
        return narrow(r.astype(np.float32), dt)  # r is a value of the dtype (or inf / nan): encoding only


# ----------------------------------------------------------------------------- CPU
def test_wide_scaled_argument_checks_cpu():
    """Every row of the validation tables of dccl_local_reduce_chain_wide_scaled and dccl_local_convert_scaled, in
    their order; the operand pointers are never dereferenced (the checks run ahead of any launch)."""
    import dccl_amd as d
    n, esz = 16, 2
    a, b, c = 1 << 40, (1 << 40) + (1 << 20), (1 << 40) + (2 << 20)
    s = np.array([0.3], np.float32)
    sp = s.ctypes.data
    chain = d.local_reduce_chain_wide_scaled
    # dtype not fp16 / bf16 wins over everything after it
    for dt in (0, 2, 7, 8, 10, 11, -1):
        assert chain([a], b, c, dt, n, sp, HOST) == 4, dt
        assert chain([], 0, 0, dt, n, 0, 7) == 4, dt
    for dt in DTS:
        # the scalar: NULL or a residence other than 0 / 1, ahead of count == 0
        assert chain([a], b, c, dt, n, 0, HOST) == 4
        assert chain([a], b, c, dt, 0, 0, DEVICE) == 4
        for res in (2, -1, 7):
            assert chain([a], b, c, dt, n, sp, res) == 4
            assert chain([a], b, c, dt, 0, sp, res) == 4
        # nsend outside 1..8, NULL sends
        assert chain([], b, c, dt, n, sp, HOST) == 4
        assert chain([a] * 9, b, c, dt, n, sp, HOST) == 4
        assert d.lib.dccl_local_reduce_chain_wide_scaled(None, 1, b, c, dt, n, sp, HOST, None) == 4
        assert d.lib.dccl_local_reduce_chain_wide_scaled(None, 1, b, c, dt, 0, sp, HOST, None) == 4
        # count == 0 succeeds, ahead of the operand checks; a device scalar's address is not read by the host
        assert chain([0], 0, 0, dt, 0, sp, HOST) == 0
        assert chain([c + esz], b, c, dt, 0, a, DEVICE) == 0
        # NULL operands
        assert chain([0], b, c, dt, n, sp, HOST) == 4
        assert chain([a, 0], b, c, dt, n, sp, HOST) == 4
        assert chain([a], 0, c, dt, n, sp, HOST) == 4
        assert chain([a], b, 0, dt, n, sp, HOST) == 4
        # partial overlap with dst, for a source and for own
        for sh in (esz, -esz, (n - 1) * esz, -(n - 1) * esz, 1):
            assert chain([a, c + sh], b, c, dt, n, sp, HOST) == 4, sh
            assert chain([a], c + sh, c, dt, n, sp, HOST) == 4, sh
    # scaled conversion: exactly the pairs 7 -> 6, 7 -> 9, 6 -> 6, 9 -> 9
    conv = d.local_convert_scaled
    pairs = {(7, 6), (7, 9), (6, 6), (9, 9)}
    for sd in range(-1, 12):
        for td in range(-1, 12):
            if (sd, td) not in pairs:
                assert conv(a, sd, b, td, n, sp, HOST) == 4, (sd, td)
                assert conv(0, sd, 0, td, 0, 0, 5) == 4, (sd, td)
    for sd, td in pairs:
        ssz = 4 if sd == 7 else 2
        assert conv(a, sd, b, td, n, 0, HOST) == 4  # NULL scalar
        assert conv(a, sd, b, td, 0, sp, 2) == 4    # residence, ahead of count == 0
        assert conv(0, sd, 0, td, 0, sp, HOST) == 0
        assert conv(c, sd, c + 1, td, 0, a, DEVICE) == 0
        assert conv(0, sd, b, td, n, sp, HOST) == 4
        assert conv(a, sd, 0, td, n, sp, HOST) == 4
        if sd == 7:  # any shared byte: the same address, one range inside the other, one byte at either end
            places = ((c, c), (c + ssz, c), (c, c + 2), (c + n * 2 - 1, c), (c, c + n * ssz - 1),
                      (c - n * ssz + 1, c), (c, c - n * 2 + 1))
        else:        # src == dst is the in-place form; every partial overlap is rejected
            places = ((c + 2, c), (c - 2, c), (c + (n - 1) * 2, c), (c - (n - 1) * 2, c), (c + 1, c))
        for src, dst in places:
            assert conv(src, sd, dst, td, n, sp, HOST) == 4, (sd, td, src - c, dst - c)
    # op creation with a NULL communicator
    out = ctypes.c_int(0)
    assert d.lib.dccl_red_op_create_wide_scaled_sum(ctypes.byref(out), sp, BF16, HOST, None) == 4
    # launch failure: only where no GPU exists; adjacent ranges, own == dst and src == dst (16 -> 16) reach the launch
    import torch
    if not torch.cuda.is_available():
        assert chain([a], c, c, BF16, n, sp, HOST) == 1
        assert chain([c + n * esz], c - n * esz, c, F16, n, sp, HOST) == 1
        assert conv(c - n * 4, F32, c, F16, n, sp, HOST) == 1
        assert conv(c + n * 2, F32, c, BF16, n, sp, HOST) == 1
        assert conv(c, BF16, c, BF16, n, sp, HOST) == 1
        assert conv(c + n * 2, F16, c, F16, n, sp, HOST) == 1


def test_wide_scaled_op_lifecycle_cpu():
    import dccl_amd as d
    comm = d.Comm.in_process(1, 0)
    try:
        s = np.array([0.25], np.float32)
        sp = s.ctypes.data
        h = np.arange(8, dtype=np.uint16)
        y = np.zeros(8, np.uint16)
        xf = np.arange(8, dtype=np.float32)
        yf = np.zeros(8, np.float32)
        make = comm.red_op_create_wide_scaled_sum
        # creation: NULL op, NULL scalar, the residence, the datatype (fp16 / bf16 only)
        assert d.lib.dccl_red_op_create_wide_scaled_sum(None, sp, BF16, HOST, comm.handle) == 4
        assert make(0, BF16, HOST)[0] == 4
        for res in (2, -1, 9):
            assert make(sp, BF16, res)[0] == 4, res
        for dt in (0, 2, 7, 8, 10, 11, -1):
            assert make(sp, dt, HOST)[0] == 4, dt
        rc, op = make(sp, BF16, HOST)
        assert rc == 0 and 5 <= op <= 20
        # host buffers: the library never combines on the CPU
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 5
        assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 5
        assert comm.reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op, 0) == 5
        assert not y.any()
        # a live handle with another datatype (the other 16-bit float, and fp32 although the scalar is one)
        for dt in (F16, F32, 2, 10, 11):
            assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 4, dt, op) == 4, dt
            assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 4, dt, op) == 4, dt
            assert comm.reduce(h.ctypes.data, y.ctypes.data, 4, dt, op, 0) == 4, dt
        # destroy: ncclRedOpDestroy as for every user op
        assert comm.red_op_destroy(op) == 0
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 4
        assert comm.red_op_destroy(op) == 4
        # ncclSum and ncclAvg are answered as before
        assert comm.all_reduce(xf.ctypes.data, yf.ctypes.data, 8, F32, SUM) == 0
        assert yf.tobytes() == xf.tobytes()
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, 4) == 5
        # the 16 slots are shared by the three kinds; the 17th live op of any kind is ncclInvalidUsage
        ops = []
        for k in range(16):
            if k % 3 == 0:
                rc, hnd = make(sp, F16 if k % 2 else BF16, HOST)
            elif k % 3 == 1:
                rc, hnd = comm.red_op_create_premul_sum(sp, F32, 1)
            else:
                rc, hnd = comm.red_op_create_wide_sum(BF16)
            assert rc == 0
            ops.append(hnd)
        assert sorted(ops) == list(range(5, 21))
        assert make(sp, BF16, HOST)[0] == 5
        assert comm.red_op_create_wide_sum(BF16)[0] == 5
        assert comm.red_op_create_premul_sum(sp, F32, 1)[0] == 5
        # a destroyed slot is reused, by any kind, and carries the new op's kind and datatype
        assert comm.red_op_destroy(ops[1]) == 0  # a pre-multiplied fp32 sum
        rc, again = make(sp, F16, HOST)
        assert rc == 0 and again == ops[1]
        assert comm.all_reduce(xf.ctypes.data, yf.ctypes.data, 8, F32, again) == 4  # it is an fp16 op now
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, F16, again) == 5   # ... and host buffers
        assert comm.red_op_destroy(ops[0]) == 0  # a scaled wide sum (bf16)
        rc, again = comm.red_op_create_premul_sum(sp, F32, 1)
        assert rc == 0 and again == ops[0]
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, again) == 4  # an fp32 pre-multiplied sum now
        assert comm.red_op_destroy(ops[2]) == 0  # a wide sum
        rc, again = make(sp, BF16, DEVICE)  # a device scalar's address is only kept
        assert rc == 0 and again == ops[2]
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, again) == 5
        assert make(sp, BF16, HOST)[0] == 5
        assert not y.any()
        # inside a group the call is validated at once, as outside
        assert d.group_start() == 0
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, again) == 5
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, F16, again) == 4
        assert d.group_end() == 0
    finally:
        comm.finalize()


def test_wide_scaled_families_are_distinguishable_cpu():
    """The premise of the GPU chain test, on its own data (module docstring)."""
    checked = 0
    for dt in DTS:
        for family in FAMILIES3:
            for nsend, count, _, _ in CHAIN_CASES:
                ops = scaled_stream(dt, family, nsend, count)
                assert_scaled_distinguishable(ops, dt, family, nsend)
                checked += 1
    assert checked == 2 * 3 * len(CHAIN_CASES)
    # fp16 cancelling: the subnormal results that pin the narrowing's denormal behaviour are there
    ops = scaled_stream(F16, "cancelling", 3, 4099)
    want = scaled_sum(ops, F16, S)
    sub = ((want & 0x7C00) == 0) & ((want & 0x03FF) != 0)
    print(f"fp16 cancelling: {sub.mean():.3f} of the expected results are subnormal")
    assert sub.mean() >= 0.15


@pytest.mark.parametrize("dt", DTS)
def test_scaled_narrow_oracle_agrees_with_float64_cpu(dt):
    """scaled_narrow against float64: the product of two fp32 values is exact in float64 (48 significant bits) while
    it stays in float64's normal range, so rounding it to fp32 is fp32_mul's one rounding, and round16_f64 rounds
    that fp32 value to 16 bits in float64 arithmetic alone.  With s = 1.0 the oracle is test_wide_sum's narrow()."""
    x = narrow_inputs(dt)
    assert fp_equal(scaled_narrow(x, 1.0, dt), narrow(x, dt), dt)
    fin = x[np.isfinite(x)]
    for s in (S, mean_scalar(3), np.float32(1.0), np.float32(-7.25)):
        with np.errstate(all="ignore"):
            p64 = fin.astype(np.float64) * np.float64(s)
            exact = (p64 == 0) | (np.abs(p64) >= 2.0 ** -1000)  # float64 normal range: the product is exact
            p32 = p64.astype(np.float32)
            mul32 = fin * np.float32(s)  # numpy's fp32 multiply
        assert exact.all()
        assert np.array_equal(p32.view(np.uint32), mul32.view(np.uint32))
        assert fp_equal(scaled_narrow(fin, s, dt), round16_f64(p32.astype(np.float64), dt), dt), float(s)


# ----------------------------------------------------------------------------- GPU: kernels
def _dev_f32(torch, value):
    return torch.from_numpy(np.array([value], np.float32)).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: f"k{c[0]}-n{c[1]}-off{c[2]}")
@pytest.mark.parametrize("family", FAMILIES3)
@pytest.mark.parametrize("dt", DTS)
def test_wide_scaled_chain_against_oracle(gpu, dt, family, case):
    """dccl_local_reduce_chain_wide_scaled, bit for bit, at test_wide_sum's placements: dst 6 bytes past a 128-B
    line, sources and own at dst's 16-B phase (vector kernel), 4 bytes off it (element-aligned fallback) or 1 byte
    off it (unaligned fallback).  The family's distinguishability condition is asserted first.  Host-immediate
    scalar: s = 0.3 and s = 1 / (nsend + 1).  Device scalar: the same two values, the second written between the
    two launches on one stream: each launch sees the value of its moment.  s = 1.0 gives
    dccl_local_reduce_chain_wide's bits.  Guard bytes around dst and every source stay as they were."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    nsend, n, shift, _ = case
    stream = scaled_stream(dt, family, nsend, n)
    assert_scaled_distinguishable(stream, dt, family, nsend)
    ops = [np.ascontiguousarray(x[:n]) for x in stream]
    sends, own = ops[:nsend], ops[nsend]
    scalars = [S, mean_scalar(nsend + 1)]
    wants = [scaled_sum(ops, dt, s) for s in scalars]
    soff = DST_OFF + shift
    dev = [dev_bytes(a, soff) for a in sends]
    t_own, p_own = dev_bytes(own, soff)
    ptrs = [d[1] for d in dev]
    nb = n * 2

    def fresh_dst():
        t, p = dev_bytes(np.zeros_like(own), DST_OFF)
        assert p % 128 == DST_OFF and (p_own - p) % 16 == shift
        return t, p

    def check(t_dst, want, what):
        got = host_of(t_dst, DST_OFF, own)
        bad = np.nonzero(got != want)[0]
        if bad.size:  # NaN payloads aside (fp_equal below), these are the elements that miss
            print(f"{case} {what}: {bad.size} of {n} differ, first at {bad[:8]}: got {got[bad[:8]]}, "
                  f"want {want[bad[:8]]}")
        assert fp_equal(got, want, dt), (case, what)
        assert _zero_outside(t_dst, DST_OFF, nb), (case, what)

    # host-immediate scalar
    for s, want in zip(scalars, wants):
        t_dst, p_dst = fresh_dst()
        hs = np.array([s], np.float32)
        torch.cuda.synchronize()
        assert dccl_amd.local_reduce_chain_wide_scaled(ptrs, p_own, p_dst, dt, n, hs.ctypes.data, HOST) == 0
        hs[0] = np.nan  # read before the call returned
        torch.cuda.synchronize()
        check(t_dst, want, ("host", float(s)))
    # device scalar, changed between two launches on one stream
    st = torch.cuda.Stream()
    vals = [_dev_f32(torch, s) for s in scalars]
    dev_s = _dev_f32(torch, np.nan)
    dsts = [fresh_dst(), fresh_dst()]
    torch.cuda.synchronize()
    with torch.cuda.stream(st):
        for v, (_, p_dst) in zip(vals, dsts):
            dev_s.copy_(v, non_blocking=True)
            assert dccl_amd.local_reduce_chain_wide_scaled(ptrs, p_own, p_dst, dt, n, dev_s.data_ptr(), DEVICE,
                                                           st.cuda_stream) == 0
    torch.cuda.synchronize()
    for s, want, (t_dst, _) in zip(scalars, wants, dsts):
        check(t_dst, want, ("device", float(s)))
    # s = 1.0: the wide sum's bits
    t_one, p_one = fresh_dst()
    t_wide, p_wide = fresh_dst()
    one = np.array([1.0], np.float32)
    assert dccl_amd.local_reduce_chain_wide_scaled(ptrs, p_own, p_one, dt, n, one.ctypes.data, HOST) == 0
    assert dccl_amd.local_reduce_chain_wide(ptrs, p_own, p_wide, dt, n) == 0
    torch.cuda.synchronize()
    assert host_of(t_one, DST_OFF, own).tobytes() == host_of(t_wide, DST_OFF, own).tobytes(), case
    check(t_one, wide_sum(ops, dt), "s = 1")
    for a, (t, _) in zip(sends + [own], dev + [(t_own, p_own)]):
        assert host_of(t, soff, a).tobytes() == a.tobytes() and _zero_outside(t, soff, nb), case
    if (nsend, n) == (3, 4099):  # own == dst, in dst's place
        t_io, p_io = dev_bytes(own, DST_OFF)
        dev2 = [dev_bytes(a, DST_OFF) for a in sends]
        hs = np.array([S], np.float32)
        torch.cuda.synchronize()
        assert dccl_amd.local_reduce_chain_wide_scaled([d[1] for d in dev2], p_io, p_io, dt, n, hs.ctypes.data,
                                                       HOST) == 0
        torch.cuda.synchronize()
        check(t_io, wants[0], "own == dst")


@pytest.mark.gpu
@pytest.mark.parametrize("place", CONVERT_PLACES, ids=lambda p: f"half{p[0]}-full{p[1]}")
@pytest.mark.parametrize("dt", DTS)
def test_convert_scaled_against_oracle(gpu, dt, place):
    """dccl_local_convert_scaled at test_wide_sum's placements (dst is the 16-bit side).  fp32 -> 16 bits over
    narrow_inputs with s = 1 (narrow()'s bits) and s = 0.3; 16 -> 16 bits over all 65,536 patterns (NaN stays NaN),
    out of place and in place, host and device scalar.  Sources and guard bytes unchanged."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    hoff, foff = place
    dev_s = _dev_f32(torch, S)
    x = narrow_inputs(dt)
    for s in (np.float32(1.0), S):
        hs = np.array([s], np.float32)
        t_src, p_src = dev_bytes(x, foff)
        t_dst, p_dst = dev_bytes(np.zeros(x.size, np.uint16), hoff)
        torch.cuda.synchronize()
        assert dccl_amd.local_convert_scaled(p_src, F32, p_dst, dt, x.size, hs.ctypes.data, HOST) == 0
        torch.cuda.synchronize()
        got = host_of(t_dst, hoff, np.zeros(x.size, np.uint16))
        assert fp_equal(got, scaled_narrow(x, s, dt), dt), float(s)
        if s == 1.0:
            assert fp_equal(got, narrow(x, dt), dt)
        assert _zero_outside(t_dst, hoff, x.size * 2) and _zero_outside(t_src, foff, x.size * 4)
        assert host_of(t_src, foff, x).view(np.uint32).tobytes() == x.view(np.uint32).tobytes()
    p = all_patterns()
    want = scaled_narrow(widen(p, dt), S, dt)
    nan = is_nan16(p, dt)
    assert np.array_equal(is_nan16(want, dt), nan)
    hs = np.array([S], np.float32)
    for residence, sptr in ((HOST, hs.ctypes.data), (DEVICE, dev_s.data_ptr())):
        t_src, p_src = dev_bytes(p, foff)  # the source takes the fp32 side's offset: 0 / 16 / 0
        t_dst, p_dst = dev_bytes(np.zeros(p.size, np.uint16), hoff)
        torch.cuda.synchronize()
        assert dccl_amd.local_convert_scaled(p_src, dt, p_dst, dt, p.size, sptr, residence) == 0
        torch.cuda.synchronize()
        assert fp_equal(host_of(t_dst, hoff, p), want, dt), residence
        assert _zero_outside(t_dst, hoff, p.size * 2) and _zero_outside(t_src, foff, p.size * 2)
        assert host_of(t_src, foff, p).tobytes() == p.tobytes()
    # in place, at the 16-bit side's offset (0, 8 and 2 bytes past a 16-B boundary: head elements exist)
    t_io, p_io = dev_bytes(p[:65531], hoff)
    torch.cuda.synchronize()
    assert dccl_amd.local_convert_scaled(p_io, dt, p_io, dt, 65531, hs.ctypes.data, HOST) == 0
    torch.cuda.synchronize()
    assert fp_equal(host_of(t_io, hoff, p[:65531]), want[:65531], dt)
    assert _zero_outside(t_io, hoff, 65531 * 2)


def run_scaled_stride_cases():
    """The child's body: the scaled bf16 chain (nsend = 3) and both scaled conversions at STRIDE_N under a grid of
    8 blocks."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    dt, nsend, n = BF16, 3, STRIDE_N
    rng = np.random.default_rng([SEED, 8])
    ops = family_ops(rng, dt, "cancelling", nsend + 1, n)
    hs = np.array([S], np.float32)
    dev = [dev_bytes(a, 0) for a in ops]
    t_dst, p_dst = dev_bytes(np.zeros(n, np.uint16), 0)
    torch.cuda.synchronize()
    assert dccl_amd.local_reduce_chain_wide_scaled([d[1] for d in dev[:nsend]], dev[nsend][1], p_dst, dt, n,
                                                   hs.ctypes.data, HOST) == 0
    torch.cuda.synchronize()
    assert fp_equal(host_of(t_dst, 0, ops[0]), scaled_sum(ops, dt, S), dt), "chain"
    assert _zero_outside(t_dst, 0, n * 2)
    ran = 1
    x = wide_acc(ops, dt)  # fp32 values with low bits set
    t_f, p_f = dev_bytes(x, 0)
    t_h, p_h = dev_bytes(np.zeros(n, np.uint16), 0)
    assert dccl_amd.local_convert_scaled(p_f, F32, p_h, dt, n, hs.ctypes.data, HOST) == 0
    torch.cuda.synchronize()
    assert fp_equal(host_of(t_h, 0, ops[0]), scaled_narrow(x, S, dt), dt), "narrow"
    assert _zero_outside(t_h, 0, n * 2)
    ran += 1
    t_o, p_o = dev_bytes(np.zeros(n, np.uint16), 0)
    assert dccl_amd.local_convert_scaled(dev[2][1], dt, p_o, dt, n, hs.ctypes.data, HOST) == 0
    torch.cuda.synchronize()
    assert fp_equal(host_of(t_o, 0, ops[0]), scaled_narrow(widen(ops[2], dt), S, dt), dt), "16 -> 16"
    assert _zero_outside(t_o, 0, n * 2)
    return ran + 1


STRIDE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import dccl_amd
assert dccl_amd.lib.dccl_max_grid_test() == 8, "the grid clamp is not live in this process"
assert dccl_amd.lib.dccl_caps_test_shift() == int(sys.argv[2]), "the size scale is not live in this process"
from tests import test_wide_scaled as scaled
print("RAN", scaled.run_scaled_stride_cases())
"""


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 10])
def test_wide_scaled_grid_stride(gpu, shift):
    """One fresh child with DCCL_MAX_GRID_TEST=8 (and DCCL_CAPS_TEST_SHIFT unset or 10, so the chain's caps rows for
    large operands are taken too), exactly as test_wide_grid_stride: every block walks about 40 tiles."""
    env = {**os.environ, "DCCL_MAX_GRID_TEST": "8", "PYTHONPATH": ROOT}
    env.pop("DCCL_CAPS_TEST_SHIFT", None)
    if shift:
        env["DCCL_CAPS_TEST_SHIFT"] = str(shift)
    p = subprocess.run([sys.executable, "-c", STRIDE_CHILD, ROOT, str(shift)], env=env, capture_output=True, text=True,
                       timeout=180)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "RAN 3" in p.stdout.splitlines(), p.stdout[-500:]


# ----------------------------------------------------------------------------- GPU: collectives
def expected_scaled_collective(api, inputs, dt, algo, s):
    """The fp32 Sum collective's simulation over the widened inputs, multiplied by s in fp32 and rounded once."""
    W = len(inputs)
    bufs = [widen(x, dt) for x in inputs]
    if api == "all_reduce":
        if algo == "rabenseifner":
            rabsim.rabenseifner_allreduce(bufs, _f32_add)
        else:
            ringsim.ring_allreduce(bufs, _f32_add, _copy)
        return [scaled_narrow(b, s, dt) for b in bufs]
    ringsim.reduce_scatter_ring(bufs, _f32_add, *ringsim.rs_maps())
    slot = inputs[0].size // W
    slots = [scaled_narrow(bufs[r][r * slot:(r + 1) * slot], s, dt) for r in range(W)]
    return slots if api == "reduce_scatter" else np.concatenate(slots)


def assert_scaling_shows(unscaled: np.ndarray, want: np.ndarray):
    """The premise of a collective test on the normal family: a missing multiply would be seen.  (Many sums of the
    cancelling family are exactly zero, at W = 2 all of them: no scalar shows there, that family pins the order.)"""
    assert share_differs(unscaled, want) >= 0.90


def _run_scaled_apis(comm, r, W, dt, apis, xs, n, op_of, stream, torch):
    out = {}
    raw = xs[r].view(np.uint8)
    for api in apis:
        send = torch.from_numpy(raw.copy()).cuda()
        nbytes = {"all_reduce_inplace": 0, "reduce_scatter": n // W * 2}.get(api, n * 2)
        recv = torch.zeros(nbytes, dtype=torch.uint8, device="cuda") if nbytes else send
        torch.cuda.synchronize()
        rc = _call(comm, api, send, recv, n, W, dt, op_of[api], stream)
        assert rc == 0, (api, n, rc)
        torch.cuda.synchronize()
        out[api] = recv.cpu().numpy().view(np.uint16)
        if recv is not send:
            assert send.cpu().numpy().tobytes() == raw.tobytes(), (api, "sendbuff changed")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring", "rabenseifner"])
@pytest.mark.parametrize("W,dt", [(4, BF16), (3, F16), (8, BF16), (2, F16)])
def test_wide_scaled_collectives_threads(gpu, monkeypatch, W, dt, algo):
    """Thread ranks on one GPU: all_reduce in and out of place, reduce_scatter and reduce to root 1 with a scaled
    wide sum, s = 1 / W as fp32, bit for bit against the fp32 simulations over the widened inputs, multiplied and
    rounded once.  algo "": the direct collectives (the fused scaled chain kernel); "ring": widen, fp32 ring,
    scaled narrowing; "rabenseifner": the same around Rabenseifner (all_reduce only).  The out-of-place all_reduce
    uses an op whose scalar lives in device memory, the others a host-immediate one.  Counts as
    test_wide_collectives_threads: W * 1031, for Rabenseifner 2^floor(log2 W) * 1031."""
    import torch
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    sub = 1 << (W.bit_length() - 1)
    n = (sub if algo == "rabenseifner" else W) * 1031
    s = mean_scalar(W)
    families = ("cancelling", "normal")
    data = {family: collective_inputs(1, W, dt, n, family) for family in families}
    apis = ["all_reduce_inplace", "all_reduce"] + ([] if algo == "rabenseifner" else ["reduce_scatter", "reduce"])

    def body(comm, r):
        st = torch.cuda.Stream()
        hs = np.array([s], np.float32)
        ds = _dev_f32(torch, s)
        torch.cuda.synchronize()
        rc, op_h = comm.red_op_create_wide_scaled_sum(hs.ctypes.data, dt, HOST)
        assert rc == 0 and op_h >= 5
        hs[0] = np.nan  # read at creation
        rc, op_d = comm.red_op_create_wide_scaled_sum(ds.data_ptr(), dt, DEVICE)
        assert rc == 0 and op_d >= 5 and op_d != op_h
        op_of = {api: op_h for api in apis}
        op_of["all_reduce"] = op_d
        out = {family: _run_scaled_apis(comm, r, W, dt, apis, xs, n, op_of, st.cuda_stream, torch)
               for family, xs in data.items()}
        assert comm.red_op_destroy(op_h) == 0 and comm.red_op_destroy(op_d) == 0
        return out

    outs = run_ranks(W, body)
    for family, xs in data.items():
        want = expected_scaled_collective("all_reduce", xs, dt, algo, s)
        unscaled = expected_collective("all_reduce", xs, dt, algo)
        if family == "normal":
            assert_scaling_shows(unscaled[0], want[0])
        for r in range(W):
            for api in ("all_reduce_inplace", "all_reduce"):
                assert fp_equal(outs[r][family][api], want[r], dt), (family, api, r)
        if algo == "rabenseifner":
            continue
        want = expected_scaled_collective("reduce_scatter", xs, dt, algo, s)
        for r in range(W):
            assert fp_equal(outs[r][family]["reduce_scatter"], want[r], dt), (family, r)
        assert fp_equal(outs[1 % W][family]["reduce"], expected_scaled_collective("reduce", xs, dt, algo, s),
                        dt), family


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring", "rabenseifner"])
def test_wide_scaled_group_mixed(gpu, monkeypatch, algo):
    """W = 4, bf16: a group of two scaled-wide all-reduces (s = 0.3, not a power of two), two wide ones and two
    plain ncclSum ones gives the separate calls' bits (and the oracle's), and each pair ran as one coalesced
    collective (dccl_group_stats)."""
    import torch
    import dccl_amd
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    W, dt = 4, BF16
    sizes = [W * 1031, W * 257, W * 515, W * 64, W * 129, W * 300]
    data = [collective_inputs(30 + i, W, dt, n, "normal") for i, n in enumerate(sizes)]

    def body(comm, r):
        st = torch.cuda.Stream()
        hs = np.array([S], np.float32)
        rc, scaled = comm.red_op_create_wide_scaled_sum(hs.ctypes.data, dt, HOST)
        assert rc == 0
        rc, wide = comm.red_op_create_wide_sum(dt)
        assert rc == 0
        ops = [scaled, scaled, wide, wide, SUM, SUM]
        outs = {}
        for mode in ("separate", "grouped"):
            bufs = [torch.from_numpy(xs[r].view(np.uint8).copy()).cuda() for xs in data]
            torch.cuda.synchronize()
            if mode == "grouped":
                with dccl_amd.group():
                    for b, n, o in zip(bufs, sizes, ops):
                        assert comm.all_reduce(b.data_ptr(), b.data_ptr(), n, dt, o, st.cuda_stream) == 0
            else:
                for b, n, o in zip(bufs, sizes, ops):
                    assert comm.all_reduce(b.data_ptr(), b.data_ptr(), n, dt, o, st.cuda_stream) == 0
            torch.cuda.synchronize()
            outs[mode] = [b.cpu().numpy().view(np.uint16) for b in bufs]
        assert comm.red_op_destroy(scaled) == 0 and comm.red_op_destroy(wide) == 0
        return outs

    before = dccl_amd.group_stats()
    outs = run_ranks(W, body)
    after = dccl_amd.group_stats()
    delta = {k: after[k] - before[k] for k in after}
    assert delta["groups"] == W and delta["calls_queued"] == 6 * W, delta
    assert delta["coalesced_runs"] == 3 * W and delta["tensors_coalesced"] == 6 * W, delta
    assert delta["collectives_issued"] == 3 * W, delta
    for i, xs in enumerate(data):
        if i < 2:
            want = expected_scaled_collective("all_reduce", xs, dt, algo, S)
            assert_scaling_shows(expected_collective("all_reduce", xs, dt, algo)[0], want[0])
        elif i < 4:
            want = expected_collective("all_reduce", xs, dt, algo)
        else:
            want = None  # plain ncclSum: the separate call is the reference
        for r in range(W):
            assert outs[r]["grouped"][i].tobytes() == outs[r]["separate"][i].tobytes(), (i, r)
            if want is not None:
                assert fp_equal(outs[r]["separate"][i], want[r], dt), (i, r)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", DTS)
def test_wide_scaled_world1(gpu, dt):
    """W = 1 is no byte copy: every API returns round16(widen(x) * s), in place and out of place."""
    import torch
    import dccl_amd
    n = 4099
    x = all_patterns()[30000:30000 + n].copy()  # NaN patterns included
    want = scaled_narrow(widen(x, dt), S, dt)
    fin = np.isfinite(widen(x, dt)) & ((x & 0x7FFF) != 0)  # infinities, NaNs and zeros stay what they are
    assert fin.sum() >= 2000 and share_differs(want[fin], x[fin]) >= 0.90
    comm = dccl_amd.Comm.in_process(1, 0)
    try:
        hs = np.array([S], np.float32)
        rc, op = comm.red_op_create_wide_scaled_sum(hs.ctypes.data, dt, HOST)
        assert rc == 0
        for api in ("all_reduce", "reduce_scatter", "reduce"):
            send = torch.from_numpy(x.view(np.uint8).copy()).cuda()
            io = send.clone()
            recv = torch.zeros_like(send)
            torch.cuda.synchronize()
            assert _call(comm, api, send, recv, n, 1, dt, op, 0) == 0
            assert _call(comm, api, io, io, n, 1, dt, op, 0) == 0
            torch.cuda.synchronize()
            assert fp_equal(recv.cpu().numpy().view(np.uint16), want, dt), api
            assert fp_equal(io.cpu().numpy().view(np.uint16), want, dt), api
            assert send.cpu().numpy().tobytes() == x.tobytes(), api
        assert comm.red_op_destroy(op) == 0
    finally:
        comm.finalize()


# ----------------------------------------------------------------------------- GPU: across processes
XP_DT = BF16


def _xp_inputs(W):
    return collective_inputs(40, W, XP_DT, W * 1031, "normal")  # at W = 2 every cancelling sum is zero


def _xp_all_reduce(comm, r, W, torch):
    hs = np.array([mean_scalar(W)], np.float32)
    rc, op = comm.red_op_create_wide_scaled_sum(hs.ctypes.data, XP_DT, HOST)
    assert rc == 0, rc
    x = _xp_inputs(W)[r]
    buf = torch.from_numpy(x.view(np.uint8).copy()).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = comm.all_reduce(buf.data_ptr(), buf.data_ptr(), x.size, XP_DT, op, st.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert comm.red_op_destroy(op) == 0
    return buf.cpu().numpy()


def _check_xp(results, W):
    xs = _xp_inputs(W)
    want = expected_scaled_collective("all_reduce", xs, XP_DT, "ring", mean_scalar(W))
    assert_scaling_shows(expected_collective("all_reduce", xs, XP_DT, "ring")[0], want[0])
    for r in range(W):
        out, fin = results[r]
        assert fin == 0
        assert fp_equal(out.view(np.uint16), want[r], XP_DT), r


@pytest.mark.gpu
def test_wide_scaled_ipc_processes(gpu):
    """One process per rank on the IPC transport, W = 3: the fused scaled chain reads the peers' scratch copies."""
    W = 3
    _check_xp(xproc.run_ipc(W, _xp_all_reduce), W)


@pytest.mark.gpu
def test_wide_scaled_rccl_processes(gpu):
    """The RCCL transport, W = 2: the staged path (widen, the fp32 ring, the scaled narrowing)."""
    import dccl_amd
    if not dccl_amd.lib.dccl_rccl_available():
        pytest.skip("librccl not loadable")
    W = 2
    _check_xp(xproc.run_rccl(W, _xp_all_reduce), W)
