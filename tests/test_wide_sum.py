"""Wide sums (dcclRedOpCreateWideSum): fp16 / bf16 contributions accumulated in fp32, rounded once.

The contract is bit-exact: widen every contribution to fp32 (exact), add with one IEEE fp32 add per contribution in
the order the algorithm combines them, round to nearest-even once.  Every expected value here is numpy's: bf16 by
bit shifts, fp16 by np.float16, sequential np.float32 adds in the stated order, one rounding; the ring and
Rabenseifner simulations run on the widened fp32 inputs.  Nothing expected comes from the code under test.

CPU: argument checks of dccl_local_reduce_chain_wide / dccl_local_convert / the op creation, the op table's
lifecycle (shared with the pre-multiplied sums), the distinguishability conditions of the two input families and
the narrowing oracle against oracle.combine.
GPU: the chain and the conversions against the oracle (vector and element-wise forms, guard bytes), their
grid-stride passes in a child process, the collectives on thread ranks (direct, ring, Rabenseifner; groups; W = 1)
and one IPC and one RCCL all-reduce across processes.

Distinguishability.  The chain test's operands are the first `count` elements of a stream of at least
GUARD_ELEMS elements per (dtype, family, nsend), and the shares below are asserted on the whole stream: at 17
elements a share of 22 % has a standard deviation of 10 points, so a condition on 17 elements would be a coin
toss, while on 4096 it is 0.7 points.
  normal      standard-normal values rounded to the dtype.  Today's per-step-rounded chain differs from the wide
              sum in at least 15 % of elements for nsend >= 2 (measured 21.9 % at nsend = 2 to 54 % at 8) and in
              none at nsend = 1: a kernel that rounds per step cannot pass.
  cancelling  per element two operands hold +B and -B (B = 2^30 for bf16, 2^15 for fp16), the others normals
              times s (1 for bf16, 2^-12 for fp16).  The wide sum in reversed order (own first) and as a pairwise
              tree each differ from the ring order in at least 40 % of elements for nsend >= 2: a kernel that
              adds in another order cannot pass.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from tests import rabsim, ringsim, xproc
from tests.test_collectives import _expected_allreduce, run_ranks
from tests.test_direct import chain_expected
from tests.test_oracle import fp_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0xDCC1
SUM = 0
F16, F32, BF16 = 6, 7, 9
DTS = (F16, BF16)
FAMILIES = ("normal", "cancelling")
GUARD_ELEMS = 4096
BIG = {BF16: 2.0 ** 30, F16: 2.0 ** 15}
SMALL = {BF16: 1.0, F16: 2.0 ** -12}
# (nsend, count, byte offset of the sources and own from dst's 16-B phase, form reached)
CHAIN_CASES = [(1, 1, 0, "vector"), (2, 17, 0, "vector"), (3, 4099, 0, "vector"), (7, 65537, 0, "vector"),
               (8, 1000, 0, "vector"), (4, 3001, 4, "element-aligned fallback"), (5, 777, 1, "unaligned fallback")]
DST_OFF = 6  # dst lies 6 bytes past a 128-B line: head and tail scalars exist


# ----------------------------------------------------------------------------- the oracle (numpy only)
def widen(bits: np.ndarray, dt: int) -> np.ndarray:
    """16-bit patterns -> float32, exact."""
    bits = np.ascontiguousarray(bits, np.uint16)
    if dt == F16:
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << 16).view(np.float32)


def narrow(f: np.ndarray, dt: int) -> np.ndarray:
    """float32 -> 16-bit patterns, round to nearest-even; overflow goes to infinity, NaN stays NaN."""
    f = np.ascontiguousarray(f, np.float32)
    if dt == F16:
        with np.errstate(all="ignore"):
            return f.astype(np.float16).view(np.uint16)
    b = f.view(np.uint32).astype(np.uint64)
    out = ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)
    out[np.isnan(f)] = 0x7FC0
    return out


def to_bits(values, dt: int) -> np.ndarray:
    return narrow(np.asarray(values, np.float64).astype(np.float32), dt)


def wide_acc(ops, dt: int) -> np.ndarray:
    """fp32 accumulator after adding the operands in the given order: acc = widen(next) + acc."""
    with np.errstate(all="ignore"):
        acc = widen(ops[0], dt)
        for x in ops[1:]:
            acc = widen(x, dt) + acc
    return acc


def wide_sum(ops, dt: int) -> np.ndarray:
    """The contract: operands in the algorithm's order (chain: sends[0] first, own last), one rounding."""
    return narrow(wide_acc(ops, dt), dt)


def stepwise_sum(ops, dt: int) -> np.ndarray:
    """Today's chain: rounded to 16 bits after every add."""
    acc = np.ascontiguousarray(ops[0], np.uint16)
    with np.errstate(all="ignore"):
        for x in ops[1:]:
            acc = narrow(widen(x, dt) + widen(acc, dt), dt)
    return acc


def tree_acc(ops, dt: int) -> np.ndarray:
    """Pairwise tree in fp32: the smaller half first, so three operands give x0 + (x1 + x2)."""
    if len(ops) == 1:
        return widen(ops[0], dt)
    h = len(ops) // 2
    with np.errstate(all="ignore"):
        return tree_acc(ops[:h], dt) + tree_acc(ops[h:], dt)


def share_differs(a: np.ndarray, b: np.ndarray) -> float:
    return float(np.mean(a != b))


def family_ops(rng, dt: int, family: str, nops: int, n: int):
    """nops operands of n elements of one input family, as 16-bit patterns."""
    ops = [to_bits(rng.standard_normal(n) * (SMALL[dt] if family == "cancelling" else 1.0), dt) for _ in range(nops)]
    if family == "cancelling":
        i = rng.integers(0, nops, n)
        j = (i + rng.integers(1, nops, n)) % nops if nops > 1 else i
        idx = np.arange(n)
        stack = np.stack(ops)
        stack[i, idx] = to_bits([BIG[dt]], dt)[0]
        if nops > 1:
            stack[j, idx] = to_bits([-BIG[dt]], dt)[0]
        ops = [np.ascontiguousarray(row) for row in stack]
    return ops


def chain_stream(dt: int, family: str, nsend: int, count: int):
    """The stream of a chain case: nsend + 1 operands (sends, then own) of max(count, GUARD_ELEMS) elements."""
    rng = np.random.default_rng([SEED, dt, FAMILIES.index(family), nsend, count])
    return family_ops(rng, dt, family, nsend + 1, max(count, GUARD_ELEMS))


def guard_shares(ops, dt: int, family: str):
    """The shares the family's condition speaks of, on the whole stream."""
    want = wide_sum(ops, dt)
    if family == "normal":
        return {"per-step rounding": share_differs(stepwise_sum(ops, dt), want)}
    return {"reversed order": share_differs(wide_sum(ops[::-1], dt), want),
            "pairwise tree": share_differs(narrow(tree_acc(ops, dt), dt), want)}


def assert_distinguishable(ops, dt: int, family: str, nsend: int):
    shares = guard_shares(ops, dt, family)
    print(f"dtype {dt} {family} nsend {nsend} n {ops[0].size}: " +
          ", ".join(f"{k} differs in {v:.3f}" for k, v in shares.items()))
    if family == "normal":
        if nsend == 1:
            assert shares["per-step rounding"] == 0.0, (dt, nsend, shares)
        else:
            assert shares["per-step rounding"] >= 0.15, (dt, nsend, shares)
    elif nsend >= 2:
        assert shares["reversed order"] >= 0.40 and shares["pairwise tree"] >= 0.40, (dt, nsend, shares)
    assert np.isfinite(widen(wide_sum(ops, dt), dt)).all()


def all_patterns() -> np.ndarray:
    return np.arange(1 << 16, dtype=np.uint32).astype(np.uint16)


def is_nan16(bits: np.ndarray, dt: int) -> np.ndarray:
    exp, mask = (0x7C00, 0x03FF) if dt == F16 else (0x7F80, 0x007F)
    return ((bits & exp) == exp) & ((bits & mask) != 0)


def narrow_inputs(dt: int) -> np.ndarray:
    """fp32 inputs of the narrowing test: for every finite 16-bit pattern p the value of p itself, the midpoint to
    the next pattern of the same sign (the tie goes to even; past the largest finite it is the overflow threshold),
    the midpoint -+ 1 fp32 ulp; then values past the largest finite, infinities and a NaN."""
    p = all_patterns()
    exp = 0x7C00 if dt == F16 else 0x7F80
    p = p[(p & exp) != exp]
    if dt == BF16:
        exact = p.astype(np.uint32) << 16
        mid = exact + 0x8000
        parts = [exact, mid, mid - 1, mid + 1]
        past = np.array([0x7F7F8000, 0x7F7F7FFF, 0x7F7FFFFF, 0x7F800000, 0xFF7F8000, 0xFF7FFFFF, 0xFF800000,
                         0x7FC00000], np.uint32)
        return np.concatenate(parts + [past]).view(np.float32)
    w = widen(p, dt).astype(np.float64)
    nxt = np.where((p & 0x7FFF) == 0x7BFF, np.copysign(65536.0, w), widen(p + np.uint16(1), dt).astype(np.float64))
    mid = ((w + nxt) / 2).astype(np.float32)
    assert np.array_equal(mid.astype(np.float64), (w + nxt) / 2)  # a midpoint has 12 significant bits: exact
    away = np.copysign(np.float32(np.inf), mid)
    parts = [w.astype(np.float32), mid, np.nextafter(mid, away), np.nextafter(mid, -away)]
    past = np.array([65520.0, 65536.0, 1e10, 3e38, np.inf, -65520.0, -65536.0, -3e38, -np.inf, np.nan], np.float32)
    return np.concatenate(parts + [past])


# ----------------------------------------------------------------------------- CPU
def test_wide_argument_checks_cpu():
    """Every row of the validation tables of dccl_local_reduce_chain_wide and dccl_local_convert, in their order;
    the pointer values are never dereferenced (the checks run ahead of any launch)."""
    import dccl_amd as d
    n, esz = 16, 2
    a, b, c = 1 << 40, (1 << 40) + (1 << 20), (1 << 40) + (2 << 20)
    # dtype not fp16 / bf16 wins over everything after it
    for dt in (0, 2, 7, 8, 10, 11, -1):
        assert d.local_reduce_chain_wide([a], b, c, dt, n) == 4, dt
        assert d.local_reduce_chain_wide([], 0, 0, dt, n) == 4, dt
    # nsend outside 1..8, NULL sends
    for dt in DTS:
        assert d.local_reduce_chain_wide([], b, c, dt, n) == 4
        assert d.local_reduce_chain_wide([a] * 9, b, c, dt, n) == 4
        assert d.lib.dccl_local_reduce_chain_wide(None, 1, b, c, dt, n, None) == 4
        assert d.lib.dccl_local_reduce_chain_wide(None, 1, b, c, dt, 0, None) == 4  # also ahead of count == 0
        # count == 0 succeeds, ahead of the operand checks
        assert d.local_reduce_chain_wide([0], 0, 0, dt, 0) == 0
        assert d.local_reduce_chain_wide([c + esz], b, c, dt, 0) == 0
        # NULL operands
        assert d.local_reduce_chain_wide([0], b, c, dt, n) == 4
        assert d.local_reduce_chain_wide([a, 0], b, c, dt, n) == 4
        assert d.local_reduce_chain_wide([a], 0, c, dt, n) == 4
        assert d.local_reduce_chain_wide([a], b, 0, dt, n) == 4
        # partial overlap with dst: by one element and by all but one, both directions, for a source and for own
        for sh in (esz, -esz, (n - 1) * esz, -(n - 1) * esz, 1):
            assert d.local_reduce_chain_wide([a, c + sh], b, c, dt, n) == 4, sh
            assert d.local_reduce_chain_wide([a], c + sh, c, dt, n) == 4, sh
    # conversion: exactly the pairs 6 -> 7, 9 -> 7, 7 -> 6, 7 -> 9
    pairs = {(6, 7), (9, 7), (7, 6), (7, 9)}
    for s in range(-1, 12):
        for t in range(-1, 12):
            if (s, t) not in pairs:
                assert d.local_convert(a, s, b, t, n) == 4, (s, t)
                assert d.local_convert(0, s, 0, t, 0) == 4, (s, t)  # ahead of count == 0 and NULL
    for s, t in pairs:
        ssz, tsz = (2, 4) if t == 7 else (4, 2)
        assert d.local_convert(0, s, 0, t, 0) == 0
        assert d.local_convert(c, s, c, t, 0) == 0
        assert d.local_convert(0, s, b, t, n) == 4
        assert d.local_convert(a, s, 0, t, n) == 4
        # any shared byte: the same address, one range inside the other, one byte at either end
        for src, dst in ((c, c), (c + ssz, c), (c, c + tsz), (c + n * tsz - 1, c), (c, c + n * ssz - 1),
                         (c - n * ssz + 1, c), (c, c - n * tsz + 1)):
            assert d.local_convert(src, s, dst, t, n) == 4, (s, t, src - c, dst - c)
    # launch failure: only where no GPU exists (there a launch cannot run anything); adjacent ranges and
    # own == dst / a source == dst pass validation and reach the launch
    import torch
    if not torch.cuda.is_available():
        assert d.local_reduce_chain_wide([a], c, c, BF16, n) == 1
        assert d.local_reduce_chain_wide([c], b, c, F16, n) == 1
        assert d.local_reduce_chain_wide([c + n * esz], c - n * esz, c, F16, n) == 1
        assert d.local_convert(c + n * 4, BF16, c, F32, n) == 1
        assert d.local_convert(c - n * 4, F32, c, F16, n) == 1


def test_wide_op_lifecycle_cpu():
    import dccl_amd as d
    comm = d.Comm.in_process(1, 0)
    try:
        s = np.array([0.25], np.float32)
        h = np.arange(8, dtype=np.uint16)
        y = np.zeros(8, np.uint16)
        xf = np.arange(8, dtype=np.float32)
        yf = np.zeros(8, np.float32)
        # creation: NULL op, then the datatype (fp16 / bf16 only), then a handle >= ncclNumOps
        assert d.lib.dccl_red_op_create_wide_sum(None, BF16, comm.handle) == 4
        for dt in (0, 2, 7, 8, 10, 11, -1):
            assert comm.red_op_create_wide_sum(dt)[0] == 4, dt
        rc, op = comm.red_op_create_wide_sum(BF16)
        assert rc == 0 and 5 <= op <= 20
        # host buffers: the library never combines on the CPU
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 5
        assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 5
        assert comm.reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op, 0) == 5
        assert not y.any()
        # a live handle with another datatype (the other 16-bit float included)
        for dt in (F16, F32, 2, 10, 11):
            assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 4, dt, op) == 4, dt
            assert comm.reduce_scatter(h.ctypes.data, y.ctypes.data, 4, dt, op) == 4, dt
            assert comm.reduce(h.ctypes.data, y.ctypes.data, 4, dt, op, 0) == 4, dt
        # destroy: the handle is dead afterwards, for the collectives and for a second destroy
        assert comm.red_op_destroy(op) == 0
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, op) == 4
        assert comm.red_op_destroy(op) == 4
        # ncclSum, ncclAvg and dtype 10 are answered as before
        assert comm.all_reduce(xf.ctypes.data, yf.ctypes.data, 8, F32, SUM) == 0
        assert yf.tobytes() == xf.tobytes()
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, SUM) == 0
        assert y.tobytes() == h.tobytes()
        y[:] = 0
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, 4) == 5
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, 10, SUM) == 4
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, 10, 4) == 4
        for never in (5, 7, 20, 21, 1000, -1):
            assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, never) == 4, never
            assert comm.red_op_destroy(never) == 4, never
        for builtin in range(5):
            assert comm.red_op_destroy(builtin) == 4
        # another communicator's handle is not live here
        other = d.Comm.in_process(1, 0)
        try:
            rc, foreign = other.red_op_create_wide_sum(BF16)
            assert rc == 0
            assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, foreign) == 4
        finally:
            other.finalize()
        # the 16 slots are shared with the pre-multiplied sums; the 17th live op of either kind is ncclInvalidUsage
        ops = []
        for k in range(16):
            if k % 2:
                rc, hnd = comm.red_op_create_premul_sum(s.ctypes.data, F32, 1)
            else:
                rc, hnd = comm.red_op_create_wide_sum(F16 if k % 4 else BF16)
            assert rc == 0
            ops.append(hnd)
        assert sorted(ops) == list(range(5, 21))
        assert comm.red_op_create_wide_sum(BF16)[0] == 5
        assert comm.red_op_create_premul_sum(s.ctypes.data, F32, 1)[0] == 5
        # a destroyed slot is reused, by either kind, and carries the new op's kind and datatype
        assert comm.red_op_destroy(ops[3]) == 0  # a pre-multiplied fp32 sum
        rc, again = comm.red_op_create_wide_sum(F16)
        assert rc == 0 and again == ops[3]
        assert comm.all_reduce(xf.ctypes.data, yf.ctypes.data, 8, F32, again) == 4  # it is an fp16 op now
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, F16, again) == 5   # ... and host buffers
        assert comm.red_op_destroy(ops[4]) == 0  # a wide sum
        rc, again = comm.red_op_create_premul_sum(s.ctypes.data, F32, 1)
        assert rc == 0 and again == ops[4]
        assert comm.all_reduce(h.ctypes.data, y.ctypes.data, 8, BF16, again) == 4  # an fp32 pre-multiplied sum now
        assert comm.red_op_create_wide_sum(BF16)[0] == 5
        assert not y.any()
        # null communicator
        out = ctypes.c_int(0)
        assert d.lib.dccl_red_op_create_wide_sum(ctypes.byref(out), BF16, None) == 4
    finally:
        comm.finalize()


def test_wide_families_are_distinguishable_cpu():
    """The premise of the GPU chain test, on its own data: per-step rounding (normal family) and another order of
    the fp32 adds (cancelling family) each change a large share of the results (module docstring)."""
    checked = 0
    for dt in DTS:
        for family in FAMILIES:
            for nsend, count, _, _ in CHAIN_CASES:
                assert_distinguishable(chain_stream(dt, family, nsend, count), dt, family, nsend)
                checked += 1
    assert checked == 2 * 2 * len(CHAIN_CASES)


@pytest.mark.parametrize("dt", DTS)
def test_narrow_oracle_agrees_with_combine_cpu(dt):
    """narrow() against oracle.combine's rounding: Sum of every pattern against a buffer of zeros (widen, + 0,
    round: every pattern comes back), and Sum of every finite pattern against half its own ulp where that is a
    value of the dtype (the midpoints of the narrowing test: ties go to even)."""
    p = all_patterns()
    zeros = np.zeros_like(p)
    with np.errstate(all="ignore"):
        mine = narrow(widen(p, dt) + widen(zeros, dt), dt)
    assert fp_equal(mine, oracle.combine(p, zeros, dt, SUM), dt)
    ok = ~is_nan16(p, dt)
    assert np.array_equal(narrow(widen(p, dt), dt)[ok], p[ok])  # the "fp32 exactly p" expectations
    exp = 0x7C00 if dt == F16 else 0x7F80
    fin = p[(p & exp) != exp]
    w = widen(fin, dt).astype(np.float64)
    nxt = widen(fin + np.uint16(1), dt).astype(np.float64)
    half = ((nxt - w) / 2).astype(np.float32)
    rep = np.isfinite(nxt) & (widen(narrow(half, dt), dt) == half)  # half an ulp is a value of the dtype
    assert rep.sum() > 50000
    a, b = fin[rep], narrow(half, dt)[rep]
    with np.errstate(all="ignore"):
        mine = narrow(widen(a, dt) + widen(b, dt), dt)
    assert np.array_equal(mine, oracle.combine(b, a, dt, SUM))
    assert np.array_equal(mine & 1, np.zeros_like(mine))  # every one of them is a tie, and went to even


# ----------------------------------------------------------------------------- GPU: kernels
def _zero_outside(t, off: int, nbytes: int) -> bool:
    return not t[:off].any() and not t[off + nbytes:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CHAIN_CASES, ids=lambda c: f"k{c[0]}-n{c[1]}-off{c[2]}")
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("dt", DTS)
def test_wide_chain_against_oracle(gpu, dt, family, case):
    """dccl_local_reduce_chain_wide, bit for bit: dst 6 bytes past a 128-B line, the sources and own at dst's
    16-B phase (vector kernel), 4 bytes off it (element-aligned fallback) or 1 byte off it (unaligned
    fallback).  The family's distinguishability condition is asserted first, so passing proves the single
    rounding and the order.  Guard bytes around dst and every source stay as they were; nsend = 1 equals the
    plain chain; own == dst once."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    nsend, n, shift, _ = case
    stream = chain_stream(dt, family, nsend, n)
    assert_distinguishable(stream, dt, family, nsend)
    ops = [np.ascontiguousarray(x[:n]) for x in stream]
    sends, own = ops[:nsend], ops[nsend]
    want = wide_sum(ops, dt)
    soff = DST_OFF + shift
    dev = [dev_bytes(a, soff) for a in sends]
    t_own, p_own = dev_bytes(own, soff)
    t_dst, p_dst = dev_bytes(np.zeros_like(own), DST_OFF)
    assert p_dst % 128 == DST_OFF and (p_own - p_dst) % 16 == shift
    torch.cuda.synchronize()
    ptrs = [d[1] for d in dev]
    assert dccl_amd.local_reduce_chain_wide(ptrs, p_own, p_dst, dt, n) == 0
    torch.cuda.synchronize()
    nb = n * 2
    assert fp_equal(host_of(t_dst, DST_OFF, own), want, dt), case
    assert _zero_outside(t_dst, DST_OFF, nb), case
    for a, (t, _) in zip(sends + [own], dev + [(t_own, p_own)]):
        assert host_of(t, soff, a).tobytes() == a.tobytes() and _zero_outside(t, soff, nb), case
    if nsend == 1:
        t_plain, p_plain = dev_bytes(np.zeros_like(own), DST_OFF)
        assert dccl_amd.local_reduce_chain(ptrs, p_own, p_plain, dt, n, SUM) == 0
        torch.cuda.synchronize()
        assert host_of(t_plain, DST_OFF, own).tobytes() == host_of(t_dst, DST_OFF, own).tobytes()
        assert fp_equal(chain_expected(sends, own, dt, SUM), want, dt)
    if (nsend, n) == (3, 4099):  # own == dst, in dst's place
        t_io, p_io = dev_bytes(own, DST_OFF)
        dev2 = [dev_bytes(a, DST_OFF) for a in sends]
        torch.cuda.synchronize()
        assert dccl_amd.local_reduce_chain_wide([d[1] for d in dev2], p_io, p_io, dt, n) == 0
        torch.cuda.synchronize()
        assert fp_equal(host_of(t_io, DST_OFF, own), want, dt), "own == dst"
        assert _zero_outside(t_io, DST_OFF, nb)


# (16-bit side's byte offset, fp32 side's byte offset): both on 16-B boundaries; the 16-bit side 8 bytes in and the
# fp32 side 16 (four head scalars line them up: still the vector kernel); the 16-bit side at a 2-byte phase (seven
# head scalars would leave the fp32 side 12 bytes off: the element-wise kernel)
CONVERT_PLACES = [(0, 0), (8, 16), (2, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("place", CONVERT_PLACES, ids=lambda p: f"half{p[0]}-full{p[1]}")
@pytest.mark.parametrize("dt", DTS)
def test_convert_against_oracle(gpu, dt, place):
    """dccl_local_convert.  Widening: all 65,536 patterns, exact bits for non-NaN, NaN stays NaN.  Narrowing:
    narrow_inputs (every pattern's value, the midpoint to the next one, the midpoint -+ 1 fp32 ulp, values past
    the largest finite) against numpy's round-to-nearest-even.  Sources and guard bytes unchanged."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    hoff, foff = place
    p = all_patterns()
    t_src, p_src = dev_bytes(p, hoff)
    t_dst, p_dst = dev_bytes(np.zeros(p.size, np.float32), foff)
    torch.cuda.synchronize()
    assert dccl_amd.local_convert(p_src, dt, p_dst, F32, p.size) == 0
    torch.cuda.synchronize()
    got, want = host_of(t_dst, foff, np.zeros(p.size, np.float32)), widen(p, dt)
    nan = is_nan16(p, dt)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    assert np.isnan(got[nan]).all() and not np.isnan(got[~nan]).any()
    assert _zero_outside(t_dst, foff, p.size * 4) and _zero_outside(t_src, hoff, p.size * 2)
    assert host_of(t_src, hoff, p).tobytes() == p.tobytes()

    x = narrow_inputs(dt)
    t_src, p_src = dev_bytes(x, foff)
    t_dst, p_dst = dev_bytes(np.zeros(x.size, np.uint16), hoff)
    torch.cuda.synchronize()
    assert dccl_amd.local_convert(p_src, F32, p_dst, dt, x.size) == 0
    torch.cuda.synchronize()
    got = host_of(t_dst, hoff, np.zeros(x.size, np.uint16))
    assert fp_equal(got, narrow(x, dt), dt)
    assert _zero_outside(t_dst, hoff, x.size * 2) and _zero_outside(t_src, foff, x.size * 4)
    assert host_of(t_src, foff, x).view(np.uint32).tobytes() == x.view(np.uint32).tobytes()


STRIDE_N = 160000  # 20,000 vectors = 313 one-wave tiles over 8 blocks: 40 grid-stride passes


def run_stride_cases():
    """The child's body: the bf16 chain (nsend = 3) and both conversions at STRIDE_N under a grid of 8 blocks."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    dt, nsend, n = BF16, 3, STRIDE_N
    rng = np.random.default_rng([SEED, 7])
    ops = family_ops(rng, dt, "cancelling", nsend + 1, n)
    dev = [dev_bytes(a, 0) for a in ops]
    t_dst, p_dst = dev_bytes(np.zeros(n, np.uint16), 0)
    torch.cuda.synchronize()
    assert dccl_amd.local_reduce_chain_wide([d[1] for d in dev[:nsend]], dev[nsend][1], p_dst, dt, n) == 0
    torch.cuda.synchronize()
    assert fp_equal(host_of(t_dst, 0, ops[0]), wide_sum(ops, dt), dt), "chain"
    assert _zero_outside(t_dst, 0, n * 2)
    ran = 1
    x = wide_acc(ops, dt)  # fp32 values with low bits set
    t_f, p_f = dev_bytes(x, 0)
    t_h, p_h = dev_bytes(np.zeros(n, np.uint16), 0)
    assert dccl_amd.local_convert(p_f, F32, p_h, dt, n) == 0
    torch.cuda.synchronize()
    assert fp_equal(host_of(t_h, 0, ops[0]), narrow(x, dt), dt), "narrow"
    assert _zero_outside(t_h, 0, n * 2)
    ran += 1
    t_w, p_w = dev_bytes(np.zeros(n, np.float32), 0)
    assert dccl_amd.local_convert(dev[0][1], dt, p_w, F32, n) == 0
    torch.cuda.synchronize()
    assert host_of(t_w, 0, x).view(np.uint32).tobytes() == widen(ops[0], dt).view(np.uint32).tobytes(), "widen"
    assert _zero_outside(t_w, 0, n * 4)
    return ran + 1


STRIDE_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import dccl_amd
assert dccl_amd.lib.dccl_max_grid_test() == 8, "the grid clamp is not live in this process"
assert dccl_amd.lib.dccl_caps_test_shift() == int(sys.argv[2]), "the size scale is not live in this process"
from tests import test_wide_sum as wide
print("RAN", wide.run_stride_cases())
"""


@pytest.mark.gpu
@pytest.mark.parametrize("shift", [0, 10])
def test_wide_grid_stride(gpu, shift):
    """One fresh child with DCCL_MAX_GRID_TEST=8 (and DCCL_CAPS_TEST_SHIFT unset or 10, so the chain's caps rows for
    large operands are taken too): every block walks about 40 tiles."""
    env = {**os.environ, "DCCL_MAX_GRID_TEST": "8", "PYTHONPATH": ROOT}
    env.pop("DCCL_CAPS_TEST_SHIFT", None)
    if shift:
        env["DCCL_CAPS_TEST_SHIFT"] = str(shift)
    p = subprocess.run([sys.executable, "-c", STRIDE_CHILD, ROOT, str(shift)], env=env, capture_output=True, text=True,
                       timeout=180)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    assert "RAN 3" in p.stdout.splitlines(), p.stdout[-500:]


# ----------------------------------------------------------------------------- GPU: collectives
def _f32_add(send, recv):
    with np.errstate(all="ignore"):
        recv += send  # one IEEE fp32 add per element


def _copy(dst, src):
    dst[:] = src


def expected_collective(api, inputs, dt, algo):
    """The fp32 Sum collective's simulation over the widened inputs, rounded once: per rank for all_reduce /
    reduce_scatter, the root's buffer for reduce."""
    W = len(inputs)
    bufs = [widen(x, dt) for x in inputs]
    if api == "all_reduce":
        if algo == "rabenseifner":
            rabsim.rabenseifner_allreduce(bufs, _f32_add)
        else:
            ringsim.ring_allreduce(bufs, _f32_add, _copy)
        return [narrow(b, dt) for b in bufs]
    ringsim.reduce_scatter_ring(bufs, _f32_add, *ringsim.rs_maps())
    slot = inputs[0].size // W
    slots = [narrow(bufs[r][r * slot:(r + 1) * slot], dt) for r in range(W)]
    return slots if api == "reduce_scatter" else np.concatenate(slots)


def collective_inputs(seed, W, dt, n, family="cancelling"):
    rng = np.random.default_rng([SEED, seed, W, dt, n, FAMILIES.index(family)])
    return family_ops(rng, dt, family, W, n)


def _call(comm, api, send, recv, n, W, dt, op, stream):
    if api.startswith("all_reduce"):
        return comm.all_reduce(send.data_ptr(), recv.data_ptr(), n, dt, op, stream)
    if api == "reduce_scatter":
        return comm.reduce_scatter(send.data_ptr(), recv.data_ptr(), n // W, dt, op, stream)
    return comm.reduce(send.data_ptr(), recv.data_ptr(), n, dt, op, 1 % W, stream)


def _run_apis(comm, r, W, dt, apis, xs, n, op, stream, torch):
    out = {}
    raw = xs[r].view(np.uint8)
    for api in apis:
        send = torch.from_numpy(raw.copy()).cuda()
        nbytes = {"all_reduce_inplace": 0, "reduce_scatter": n // W * 2}.get(api, n * 2)
        recv = torch.zeros(nbytes, dtype=torch.uint8, device="cuda") if nbytes else send
        torch.cuda.synchronize()
        rc = _call(comm, api, send, recv, n, W, dt, op, stream)
        assert rc == 0, (api, n, rc)
        torch.cuda.synchronize()
        out[api] = recv.cpu().numpy().view(np.uint16)
        if recv is not send:
            assert send.cpu().numpy().tobytes() == raw.tobytes(), (api, "sendbuff changed")
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring", "rabenseifner"])
@pytest.mark.parametrize("W,dt", [(4, BF16), (3, F16), (8, BF16), (2, F16)])
def test_wide_collectives_threads(gpu, monkeypatch, W, dt, algo):
    """Thread ranks on one GPU: all_reduce in and out of place, reduce_scatter and reduce to root 1 with a wide
    sum, bit for bit against the fp32 simulations over the widened inputs, rounded once.  algo "": the direct
    collectives (the fused chain kernel); "ring": widen, fp32 ring, narrow; "rabenseifner": the same around
    Rabenseifner (all_reduce only).  Cancelling inputs: another order of the adds would show; with at most two
    small operands next to +-B they do not tell per-step rounding apart, so the normal family runs as well.  The
    count is W * 1031 (odd slots: head and tail scalars), for Rabenseifner 2^floor(log2 W) * 1031."""
    import torch
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    sub = 1 << (W.bit_length() - 1)
    n = (sub if algo == "rabenseifner" else W) * 1031
    data = {family: collective_inputs(1, W, dt, n, family) for family in FAMILIES}
    apis = ["all_reduce_inplace", "all_reduce"] + ([] if algo == "rabenseifner" else ["reduce_scatter", "reduce"])

    def body(comm, r):
        st = torch.cuda.Stream()
        rc, op = comm.red_op_create_wide_sum(dt)
        assert rc == 0 and op >= 5
        out = {family: _run_apis(comm, r, W, dt, apis, xs, n, op, st.cuda_stream, torch) for family, xs in data.items()}
        assert comm.red_op_destroy(op) == 0
        return out

    outs = run_ranks(W, body)
    for family, xs in data.items():
        want = expected_collective("all_reduce", xs, dt, algo)
        if family == "normal" and W > 2 and algo != "rabenseifner":  # the premise: per-step rounding would be seen
            assert share_differs(_expected_allreduce(xs, dt, SUM)[0], want[0]) >= 0.15
        for r in range(W):
            for api in ("all_reduce_inplace", "all_reduce"):
                assert fp_equal(outs[r][family][api], want[r], dt), (family, api, r)
        if algo == "rabenseifner":
            continue
        want = expected_collective("reduce_scatter", xs, dt, algo)
        for r in range(W):
            assert fp_equal(outs[r][family]["reduce_scatter"], want[r], dt), (family, r)
        assert fp_equal(outs[1 % W][family]["reduce"], expected_collective("reduce", xs, dt, algo), dt), family


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring", "rabenseifner"])
def test_wide_group_and_plain_sum(gpu, monkeypatch, algo):
    """W = 4, bf16: two small wide-sum all-reduces next to a plain ncclSum one inside ncclGroupStart / ncclGroupEnd
    give the separate calls' bits (and the oracle's); a plain ncclSum all-reduce on the same communicator
    afterwards still rounds per step, as today."""
    import torch
    import dccl_amd
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    W, dt = 4, BF16
    sizes = [W * 1031, W * 257, W * 515]
    # the normal family: it tells the wide sum from the per-step-rounded one (asserted below)
    data = [collective_inputs(10 + i, W, dt, n, "normal") for i, n in enumerate(sizes)]

    def body(comm, r):
        st = torch.cuda.Stream()
        rc, op = comm.red_op_create_wide_sum(dt)
        assert rc == 0
        ops = [op, op, SUM]
        outs = {}
        for mode in ("separate", "grouped", "plain afterwards"):
            bufs = [torch.from_numpy(xs[r].view(np.uint8).copy()).cuda() for xs in data]
            torch.cuda.synchronize()
            if mode == "grouped":
                with dccl_amd.group():
                    for b, n, o in zip(bufs, sizes, ops):
                        assert comm.all_reduce(b.data_ptr(), b.data_ptr(), n, dt, o, st.cuda_stream) == 0
            else:
                for b, n, o in zip(bufs, sizes, ops if mode == "separate" else [SUM] * 3):
                    assert comm.all_reduce(b.data_ptr(), b.data_ptr(), n, dt, o, st.cuda_stream) == 0
            torch.cuda.synchronize()
            outs[mode] = [b.cpu().numpy().view(np.uint16) for b in bufs]
        assert comm.red_op_destroy(op) == 0
        return outs

    outs = run_ranks(W, body)
    for i, xs in enumerate(data):
        wide = expected_collective("all_reduce", xs, dt, algo)
        if algo == "rabenseifner":
            plain = rabsim.rabenseifner_allreduce(
                [x.copy() for x in xs], lambda s, rv: oracle.expected_reduce(np.ascontiguousarray(s), rv, dt, SUM))
        else:
            plain = _expected_allreduce(xs, dt, SUM)
        assert not fp_equal(plain[0], wide[0], dt)
        for r in range(W):
            assert outs[r]["grouped"][i].tobytes() == outs[r]["separate"][i].tobytes(), (i, r)
            assert fp_equal(outs[r]["separate"][i], plain[r] if i == 2 else wide[r], dt), (i, r)
            assert fp_equal(outs[r]["plain afterwards"][i], plain[r], dt), (i, r)


@pytest.mark.gpu
def test_wide_world1(gpu):
    """W = 1: every API returns the input's bytes, in place and out of place."""
    import torch
    import dccl_amd
    dt, n = F16, 4099
    x = all_patterns()[30000:30000 + n].copy()  # NaN patterns included: a byte copy keeps them
    comm = dccl_amd.Comm.in_process(1, 0)
    try:
        rc, op = comm.red_op_create_wide_sum(dt)
        assert rc == 0
        send = torch.from_numpy(x.view(np.uint8).copy()).cuda()
        for api in ("all_reduce", "reduce_scatter", "reduce"):
            recv = torch.zeros_like(send)
            torch.cuda.synchronize()
            assert _call(comm, api, send, recv, n, 1, dt, op, 0) == 0
            assert _call(comm, api, send, send, n, 1, dt, op, 0) == 0
            torch.cuda.synchronize()
            assert recv.cpu().numpy().tobytes() == x.tobytes(), api
            assert send.cpu().numpy().tobytes() == x.tobytes(), api
        assert comm.red_op_destroy(op) == 0
    finally:
        comm.finalize()


# ----------------------------------------------------------------------------- GPU: across processes
XP_DT = BF16


def _xp_inputs(W):
    return collective_inputs(20, W, XP_DT, W * 1031)


def _xp_all_reduce(comm, r, W, torch):
    rc, op = comm.red_op_create_wide_sum(XP_DT)
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
    want = expected_collective("all_reduce", _xp_inputs(W), XP_DT, "ring")
    for r in range(W):
        out, fin = results[r]
        assert fin == 0
        assert fp_equal(out.view(np.uint16), want[r], XP_DT), r


@pytest.mark.gpu
def test_wide_ipc_processes(gpu):
    """One process per rank on the IPC transport, W = 3: the fused wide chain reads the peers' scratch copies."""
    W = 3
    _check_xp(xproc.run_ipc(W, _xp_all_reduce), W)


@pytest.mark.gpu
def test_wide_rccl_processes(gpu):
    """The RCCL transport, W = 2: the staged path (widen, the fp32 ring, narrow)."""
    import dccl_amd
    if not dccl_amd.lib.dccl_rccl_available():
        pytest.skip("librccl not loadable")
    W = 2
    _check_xp(xproc.run_rccl(W, _xp_all_reduce), W)
