"""Pre-multiplied sum reductions (ncclRedOpCreatePreMulSum).

The contract is bit-exact: scaled_r = Prod(x_r, s) with the oracle's Prod element semantics (16-bit floats
rounded back to 16 bits), then the existing Sum collective over scaled_0 .. scaled_{W-1}.  So every expected
value here is oracle.combine(..., Prod) against a buffer filled with s, followed by the existing chain order
(chain_expected) or the ring / Rabenseifner simulations with op Sum.

CPU: argument checks of dccl_local_scale / dccl_local_reduce_chain_premul and the op table's lifecycle.
GPU: the scale and fused chain kernels against the oracle for every dtype and placement, the collectives on
thread ranks (direct, ring, Rabenseifner), HIP-graph replay with a device-resident scalar, and one IPC and one
RCCL all-reduce across processes.
"""
import ctypes
import fractions

import numpy as np
import pytest

import oracle
from tests import rabsim, ringsim, xproc
from tests.test_collectives import _expected_allreduce, run_ranks
from tests.test_direct import chain_expected
from tests.test_oracle import fp_equal

SEED = 0xDCC1
SUM, PROD = 0, 1
DEVICE, HOST = 0, 1  # ncclScalarResidence_t
FLOATS = (6, 7, 8, 9)


# ----------------------------------------------------------------------------- helpers
def f32_to_bf16_bits(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bit patterns, round-to-nearest-even (finite inputs)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b: np.ndarray) -> np.ndarray:
    return (b.astype(np.uint32) << 16).view(np.float32)


def to_dtype(values, dt: int) -> np.ndarray:
    """Real values in the wire format of dtype `dt` (fp16 / bf16 as uint16 bit patterns)."""
    v = np.asarray(values, np.float64)
    if dt == 6:
        return v.astype(np.float16).view(np.uint16)
    if dt == 9:
        return f32_to_bf16_bits(v.astype(np.float32))
    if dt in (7, 8):
        return v.astype(oracle.NP_DTYPES[dt])
    return v.astype(np.int64).astype(oracle.NP_DTYPES[dt])  # integers wrap into the type


def scalars_of(dt: int):
    """Two scalars per dtype: 1/3 and -0.75 for floats; 3 and -7 (249 unsigned) for integers, so 8-bit wraps."""
    if dt in FLOATS:
        return [to_dtype([1.0 / 3.0], dt), to_dtype([-0.75], dt)]
    return [to_dtype([3], dt), to_dtype([-7], dt)]  # -7 wraps to 249 / 2^32 - 7 / 2^64 - 7 when unsigned


def premul(x: np.ndarray, s: np.ndarray, dt: int) -> np.ndarray:
    """Prod(x, s): the oracle's element multiply of x against a buffer filled with the scalar."""
    return oracle.combine(np.full(x.shape, s[0], dtype=x.dtype), x, dt, PROD)


def normal_inputs(rng, dt: int, n: int) -> np.ndarray:
    if dt in FLOATS:
        return to_dtype(rng.standard_normal(n), dt)
    return rng.integers(-1000, 1000, n).astype(oracle.NP_DTYPES[dt])


def chain_inputs(rng, dt: int, n: int) -> np.ndarray:
    """rand_inputs' raw bit patterns (denormals, infinities, NaNs); from n = 4099, three quarters of a float
    operand are standard-normal values, so most sums are finite and the discrimination guard has material."""
    from tests.test_gpu_parity import rand_inputs
    x = rand_inputs(rng, dt, n)[0]
    if dt in FLOATS and n >= 4099:
        tame = rng.random(n) < 0.75
        x[tame] = normal_inputs(rng, dt, int(tame.sum()))
    return x


class Scalar:
    """One scalar in host memory and, on demand, in device memory."""

    def __init__(self, s: np.ndarray, residence: int):
        self.host = np.ascontiguousarray(s)
        self.residence = residence
        self.dev = None
        if residence == DEVICE:
            import torch
            self.dev = torch.from_numpy(self.host.view(np.uint8).copy()).cuda()
            torch.cuda.synchronize()

    @property
    def ptr(self) -> int:
        return self.dev.data_ptr() if self.residence == DEVICE else self.host.ctypes.data


def wrong_variants(sends, own, s, dt):
    """What a kernel that skips one of the contract's roundings would give, as arrays comparable to the expected
    result (fp64: the first 256 elements).  fp32 / fp64: every multiply-add fused (one rounding); fp16 / bf16:
    the product not rounded to 16 bits before the fp32 add."""
    ops = list(sends) + [own]
    if dt == 7:
        sc = np.float64(s[0])
        with np.errstate(all="ignore"):
            acc = (ops[0].astype(np.float64) * sc).astype(np.float32)
            for x in ops[1:]:
                acc = (x.astype(np.float64) * sc + acc.astype(np.float64)).astype(np.float32)
        return acc
    if dt == 8:
        m = min(256, own.size)
        out = np.empty(m, np.float64)
        sc = float(s[0])
        for i in range(m):
            vals = [float(x[i]) for x in ops]
            if not all(np.isfinite(vals)):
                out[i] = np.nan
                continue
            acc = vals[0] * sc
            try:
                for v in vals[1:]:
                    if not np.isfinite(acc):
                        break
                    acc = float(fractions.Fraction(v) * fractions.Fraction(sc) + fractions.Fraction(acc))
            except OverflowError:
                acc = np.nan
            out[i] = acc
        return out
    widen = (lambda b: b.view(np.float16).astype(np.float32)) if dt == 6 else bf16_bits_to_f32
    narrow = (lambda f: f.astype(np.float16).view(np.uint16)) if dt == 6 else f32_to_bf16_bits
    sc = widen(s)[0]
    with np.errstate(all="ignore"):
        acc = narrow(widen(ops[0]) * sc)
        for x in ops[1:]:
            acc = narrow(widen(x) * sc + widen(acc))  # the product stays in fp32
    return acc


def finite_mask(a: np.ndarray, dt: int) -> np.ndarray:
    if dt == 6:
        return (a & 0x7C00) != 0x7C00
    if dt == 9:
        return (a & 0x7F80) != 0x7F80
    return np.isfinite(a)


def fraction_distinguished(wrong: np.ndarray, want: np.ndarray, dt: int) -> float:
    """Share of elements (of those the wrong variant covers) where it and the expected result are both finite
    and differ."""
    want = want[:wrong.size]
    both = finite_mask(wrong, dt) & finite_mask(want, dt)
    return float(np.mean(both & (wrong != want)))


CHAIN_CASES = [(1, 1, 0), (2, 17, 0), (3, 4099, 0), (7, 65537, 0), (8, 1000, 0), (4, 3001, 4), (5, 777, None)]


def chain_cases(dt: int, esz: int):
    """(k, n, byte offsets of the sends, own and dst, operands, scalar, residence) of the fused chain test: the
    in-phase cases (offsets 0, 4 and 2 elements, shared by every operand), one mixed-phase case and one off
    element alignment.  Seeded per dtype, so the CPU guard test sees the GPU test's data."""
    rng = np.random.default_rng(7000 + dt)
    cases = [(k, n, [2 * esz if off is None else off] * (k + 2)) for k, n, off in CHAIN_CASES]
    cases.append((3, 4099, [0, esz, 16, 0, 3 * esz]))
    if esz > 1:
        cases.append((2, 1000, [1, 0, esz + 1, 1]))
    for idx, (k, n, offs) in enumerate(cases):
        arrs = [chain_inputs(rng, dt, n) for _ in range(k + 1)]
        yield k, n, offs, arrs, scalars_of(dt)[idx % 2], (idx // 2) % 2


# ----------------------------------------------------------------------------- CPU
def test_premul_argument_checks_cpu():
    """Every row of the validation tables of dccl_local_scale and dccl_local_reduce_chain_premul, in their order;
    the pointer values are never dereferenced (the checks run ahead of any launch)."""
    import dccl_amd as d
    s = np.array([0.5], np.float32)
    sp = s.ctypes.data
    n, esz = 16, 4
    a, b, c = 1 << 40, (1 << 40) + (1 << 20), (1 << 40) + (2 << 20)
    # unknown dtype wins over everything after it
    assert d.local_scale(a, b, 11, n, sp, HOST) == 4
    assert d.local_scale(0, 0, -1, n, 0, 7) == 4
    assert d.local_reduce_chain_premul([a], b, c, 11, n, sp, HOST) == 4
    assert d.local_reduce_chain_premul([], 0, 0, 10, n, 0, 7) == 4
    # nsend outside 1..8, NULL sends
    assert d.local_reduce_chain_premul([], b, c, 7, n, sp, HOST) == 4
    assert d.local_reduce_chain_premul([a] * 9, b, c, 7, n, sp, HOST) == 4
    assert d.lib.dccl_local_reduce_chain_premul(None, 1, b, c, 7, n, sp, HOST, None) == 4
    # residence not 0 / 1, NULL scalar
    for res in (2, -1):
        assert d.local_scale(a, b, 7, n, sp, res) == 4
        assert d.local_reduce_chain_premul([a], b, c, 7, n, sp, res) == 4
    for res in (DEVICE, HOST):
        assert d.local_scale(a, b, 7, n, 0, res) == 4
        assert d.local_reduce_chain_premul([a], b, c, 7, n, 0, res) == 4
        assert d.local_scale(a, b, 7, 0, 0, res) == 4  # also ahead of count == 0
    # count == 0 succeeds, ahead of the operand checks
    assert d.local_scale(0, 0, 7, 0, sp, HOST) == 0
    assert d.local_scale(a, a + esz, 7, 0, sp, DEVICE) == 0
    assert d.local_reduce_chain_premul([0], 0, 0, 7, 0, sp, HOST) == 0
    assert d.local_reduce_chain_premul([c + esz], b, c, 7, 0, sp, DEVICE) == 0
    # NULL operands
    assert d.local_scale(0, b, 7, n, sp, HOST) == 4
    assert d.local_scale(a, 0, 7, n, sp, HOST) == 4
    assert d.local_reduce_chain_premul([0], b, c, 7, n, sp, HOST) == 4
    assert d.local_reduce_chain_premul([a, 0], b, c, 7, n, sp, HOST) == 4
    assert d.local_reduce_chain_premul([a], 0, c, 7, n, sp, HOST) == 4
    assert d.local_reduce_chain_premul([a], b, 0, 7, n, sp, HOST) == 4
    # partial overlap with dst: by one element and by all but one, both directions, for a source and for own
    for sh in (esz, -esz, (n - 1) * esz, -(n - 1) * esz):
        assert d.local_scale(c + sh, c, 7, n, sp, HOST) == 4, sh
        assert d.local_reduce_chain_premul([a, c + sh], b, c, 7, n, sp, HOST) == 4, sh
        assert d.local_reduce_chain_premul([a], c + sh, c, 7, n, sp, DEVICE) == 4, sh
    # launch failure: only where no GPU exists (there a launch cannot run anything); adjacent ranges and
    # src == dst / own == dst pass validation and reach the launch
    import torch
    if not torch.cuda.is_available():
        assert d.local_scale(c + n * esz, c, 7, n, sp, HOST) == 1
        assert d.local_scale(c, c, 7, n, sp, HOST) == 1
        assert d.local_reduce_chain_premul([a], c, c, 7, n, sp, HOST) == 1


def test_premul_op_lifecycle_cpu():
    import dccl_amd as d
    comm = d.Comm.in_process(1, 0)
    try:
        s = np.array([0.25], np.float32)
        x = np.arange(8, dtype=np.float32)
        y = np.zeros(8, np.float32)
        xi = np.arange(8, dtype=np.int32)
        # creation: argument checks, then a handle >= ncclNumOps
        assert d.lib.dccl_red_op_create_premul_sum(None, s.ctypes.data, 7, HOST, comm.handle) == 4
        assert comm.red_op_create_premul_sum(0, 7, HOST)[0] == 4
        assert comm.red_op_create_premul_sum(s.ctypes.data, 10, HOST)[0] == 4
        assert comm.red_op_create_premul_sum(s.ctypes.data, 7, 2)[0] == 4
        assert comm.red_op_create_premul_sum(s.ctypes.data, 7, -1)[0] == 4
        rc, op = comm.red_op_create_premul_sum(s.ctypes.data, 7, HOST)
        assert rc == 0 and 5 <= op <= 20
        # host buffers: the library never combines on the CPU
        assert comm.all_reduce(x.ctypes.data, y.ctypes.data, 8, 7, op) == 5
        assert comm.reduce_scatter(x.ctypes.data, y.ctypes.data, 8, 7, op) == 5
        assert comm.reduce(x.ctypes.data, y.ctypes.data, 8, 7, op, 0) == 5
        assert not y.any()
        # a live handle with another datatype
        assert comm.all_reduce(xi.ctypes.data, xi.ctypes.data, 8, 2, op) == 4
        assert comm.reduce_scatter(xi.ctypes.data, xi.ctypes.data, 8, 2, op) == 4
        assert comm.reduce(xi.ctypes.data, xi.ctypes.data, 8, 2, op, 0) == 4
        assert comm.all_reduce(x.ctypes.data, y.ctypes.data, 8, 11, op) == 4
        # destroy: the handle is dead afterwards, for the collectives and for a second destroy
        assert comm.red_op_destroy(op) == 0
        assert comm.all_reduce(x.ctypes.data, y.ctypes.data, 8, 7, op) == 4
        assert comm.red_op_destroy(op) == 4
        # never-created handles, ncclAvg and the built-in ops keep today's answers
        for never in (5, 7, 20, 21, 1000, -1):
            assert comm.all_reduce(x.ctypes.data, y.ctypes.data, 8, 7, never) == 4, never
            assert comm.red_op_destroy(never) == 4, never
        assert comm.all_reduce(x.ctypes.data, y.ctypes.data, 8, 7, 4) == 5
        for builtin in range(5):
            assert comm.red_op_destroy(builtin) == 4
        # another communicator's handle is not live here
        other = d.Comm.in_process(1, 0)
        try:
            rc, foreign = other.red_op_create_premul_sum(s.ctypes.data, 7, HOST)
            assert rc == 0
            assert comm.all_reduce(x.ctypes.data, y.ctypes.data, 8, 7, foreign) == 4
        finally:
            other.finalize()
        # 16 live ops; the 17th is ncclInvalidUsage; a destroyed slot is reused
        ops = []
        for _ in range(16):
            rc, h = comm.red_op_create_premul_sum(s.ctypes.data, 7, HOST)
            assert rc == 0
            ops.append(h)
        assert sorted(ops) == list(range(5, 21))
        assert comm.red_op_create_premul_sum(s.ctypes.data, 7, HOST)[0] == 5
        assert comm.red_op_destroy(ops[3]) == 0
        rc, again = comm.red_op_create_premul_sum(s.ctypes.data, 9, HOST)
        assert rc == 0 and again == ops[3]
        assert comm.all_reduce(x.ctypes.data, y.ctypes.data, 8, 7, again) == 4  # it is a bf16 op now
        # null communicator
        assert d.lib.dccl_red_op_destroy(5, None) == 4
        out = ctypes.c_int(0)
        assert d.lib.dccl_red_op_create_premul_sum(ctypes.byref(out), s.ctypes.data, 7, HOST, None) == 4
    finally:
        comm.finalize()


def test_wrong_variants_are_distinguishable_cpu():
    """The discrimination guard's premise, on the CPU and on the GPU chain test's own data: at n >= 4099 a
    fused multiply-add (fp32, fp64) or a product kept in fp32 (fp16, bf16) changes at least 1 % of the results."""
    checked = 0
    for dt in FLOATS:
        for k, n, _, arrs, s, _ in chain_cases(dt, np.dtype(oracle.NP_DTYPES[dt]).itemsize):
            if n < 4099:
                continue
            want = chain_expected([premul(a, s, dt) for a in arrs[:k]], premul(arrs[k], s, dt), dt, SUM)
            frac = fraction_distinguished(wrong_variants(arrs[:k], arrs[k], s, dt), want, dt)
            print(f"dtype {dt} k {k} n {n} scalar {s}: {frac:.3f} of elements distinguish the wrong variant")
            assert frac >= 0.01, (dt, k, n, frac)
            checked += 1
    assert checked == 3 * len(FLOATS)


# ----------------------------------------------------------------------------- GPU: kernels
@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(range(10)))
def test_scale_against_oracle(gpu, dt):
    """dccl_local_scale: in place; out of place at the same 16-B phase (4 bytes in); one element apart (another
    phase: the element-wise kernel); destination 1 byte off element alignment.  Both residences, two scalars,
    n = 1, 17, 4099 (head, vector body and tail).  Bit-exact against the oracle's Prod; src untouched."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of, rand_inputs
    rng = np.random.default_rng(9000 + dt)
    esz = dccl_amd.size_of_type(dt)
    places = [("in place", 0, None), ("same phase", 4, 4), ("same phase, 3 elements in", 3 * esz, 3 * esz + 16),
              ("other phase", 0, esz)]
    if esz > 1:
        places.append(("unaligned dst", 0, 1))
    for n in (1, 17, 4099):
        x = rand_inputs(rng, dt, n)[0]
        for s in scalars_of(dt):
            want = premul(x, s, dt)
            for residence in (DEVICE, HOST):
                sc = Scalar(s, residence)
                for what, soff, doff in places:
                    t_src, p_src = dev_bytes(x, soff)
                    t_dst, p_dst = (t_src, p_src) if doff is None else dev_bytes(np.zeros_like(x), doff)
                    torch.cuda.synchronize()
                    assert dccl_amd.local_scale(p_src, p_dst, dt, n, sc.ptr, residence) == 0
                    torch.cuda.synchronize()
                    got = host_of(t_dst, soff if doff is None else doff, x)
                    assert fp_equal(got, want, dt), (what, n, s, residence)
                    if doff is not None:
                        assert host_of(t_src, soff, x).tobytes() == x.tobytes(), (what, n)
                        nb = n * esz
                        assert not t_dst[:doff].any() and not t_dst[doff + nb:].any(), (what, n)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", list(range(10)))
def test_premul_chain_against_oracle(gpu, dt):
    """dccl_local_reduce_chain_premul against chain_expected over pre-multiplied operands: the in-phase vector
    kernel, one mixed-phase case and one case off element alignment (the element-wise kernel); a separate dst
    (own, the sends and the bytes around dst untouched) and own == dst.  For float dtypes at n >= 4099 the
    variants that skip one of the contract's roundings must differ from the expected bits in at least 1 % of
    elements, so a kernel that computed them could not pass."""
    import torch
    import dccl_amd
    from tests.test_gpu_parity import dev_bytes, host_of
    esz = dccl_amd.size_of_type(dt)
    for k, n, offs, arrs, s, residence in chain_cases(dt, esz):
        sends, own = arrs[:k], arrs[k]
        sc = Scalar(s, residence)
        want = chain_expected([premul(a, s, dt) for a in sends], premul(own, s, dt), dt, SUM)
        if dt in FLOATS and n >= 4099:
            frac = fraction_distinguished(wrong_variants(sends, own, s, dt), want, dt)
            assert frac >= 0.01, ("the wrong variant is indistinguishable", dt, k, n, frac)
        dev = [dev_bytes(a, o) for a, o in zip(sends, offs)]
        t_own, p_own = dev_bytes(own, offs[k])
        t_dst, p_dst = dev_bytes(np.zeros_like(own), offs[k + 1])
        torch.cuda.synchronize()
        ptrs = [d[1] for d in dev]
        assert dccl_amd.local_reduce_chain_premul(ptrs, p_own, p_dst, dt, n, sc.ptr, residence) == 0
        torch.cuda.synchronize()
        got = host_of(t_dst, offs[k + 1], own)
        assert fp_equal(got, want, dt), (k, n, offs, "separate dst")
        assert host_of(t_own, offs[k], own).tobytes() == own.tobytes(), (k, n, offs)
        nb = n * esz
        assert not t_dst[:offs[k + 1]].any() and not t_dst[offs[k + 1] + nb:].any(), (k, n, offs)
        for a, (t, _), o in zip(sends, dev, offs):
            assert host_of(t, o, a).tobytes() == a.tobytes()
        # own == dst
        assert dccl_amd.local_reduce_chain_premul(ptrs, p_own, p_own, dt, n, sc.ptr, residence) == 0
        torch.cuda.synchronize()
        assert fp_equal(host_of(t_own, offs[k], own), want, dt), (k, n, offs, "own == dst")


@pytest.mark.gpu
def test_premul_graph_replay_device_scalar(gpu):
    """dccl_local_scale then dccl_local_reduce_chain_premul (k = 2, fp32, n = 4099) captured once on one stream
    with a device-resident scalar: each replay reads the scalar's value of that moment."""
    import torch
    import dccl_amd
    dt, n, k = 7, 4099, 2
    rng = np.random.default_rng(4242)
    x = rng.standard_normal(n).astype(np.float32)
    arrs = [rng.standard_normal(n).astype(np.float32) for _ in range(k + 1)]
    t_x = torch.from_numpy(x).cuda()
    t_scaled = torch.zeros(n, device="cuda")
    t_ops = [torch.from_numpy(a).cuda() for a in arrs]
    t_out = torch.zeros(n, device="cuda")
    t_s = torch.zeros(1, device="cuda")
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            assert dccl_amd.local_scale(t_x.data_ptr(), t_scaled.data_ptr(), dt, n, t_s.data_ptr(), DEVICE,
                                        st.cuda_stream) == 0
            assert dccl_amd.local_reduce_chain_premul([t.data_ptr() for t in t_ops[:k]], t_ops[k].data_ptr(),
                                                      t_out.data_ptr(), dt, n, t_s.data_ptr(), DEVICE,
                                                      st.cuda_stream) == 0
    torch.cuda.synchronize()
    assert not t_out.any() and not t_scaled.any()  # capture does not execute
    for value in (1.0 / 3.0, -0.75):
        s = np.array([value], np.float32)
        t_s.copy_(torch.from_numpy(s))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert t_scaled.cpu().numpy().tobytes() == premul(x, s, dt).tobytes(), value
        want = chain_expected([premul(a, s, dt) for a in arrs[:k]], premul(arrs[k], s, dt), dt, SUM)
        assert t_out.cpu().numpy().tobytes() == want.tobytes(), value


# ----------------------------------------------------------------------------- GPU: collectives
def _sum_combine(dt):
    def combine(send, recv):
        assert oracle.expected_reduce(np.ascontiguousarray(send), recv, dt, SUM) == 0
    return combine


def _expected(api, scaled, dt, algo):
    """The Sum collective's simulation over the pre-multiplied inputs: per rank for all_reduce /
    reduce_scatter, the root's buffer for reduce."""
    W = len(scaled)
    if api == "all_reduce":
        if algo == "rabenseifner":
            return rabsim.rabenseifner_allreduce([x.copy() for x in scaled], _sum_combine(dt))
        return _expected_allreduce(scaled, dt, SUM)
    bufs = [x.copy() for x in scaled]
    ringsim.reduce_scatter_ring(bufs, _sum_combine(dt), *ringsim.rs_maps())
    slot = scaled[0].size // W
    slots = [bufs[r][r * slot:(r + 1) * slot] for r in range(W)]
    return slots if api == "reduce_scatter" else np.concatenate(slots)


def _run_collectives(comm, r, W, dt, algo, inputs, s, residence, stream, torch):
    """One rank: every API at every n with one op; returns {(api, n): host bytes of the output}."""
    sc = Scalar(s, residence)
    rc, op = comm.red_op_create_premul_sum(sc.ptr, dt, residence)
    assert rc == 0 and op >= 5
    out = {}
    for n, xs in inputs.items():
        raw = xs[r].view(np.uint8)
        esz = xs[r].itemsize
        apis = ["all_reduce_inplace", "all_reduce"]
        if algo != "rabenseifner":
            apis += ["reduce_scatter", "reduce"]
        for api in apis:
            send = torch.from_numpy(raw.copy()).cuda()
            nbytes = {"all_reduce_inplace": 0, "reduce_scatter": n // W * esz}.get(api, n * esz)
            recv = torch.zeros(nbytes, dtype=torch.uint8, device="cuda") if nbytes else send
            torch.cuda.synchronize()
            if api.startswith("all_reduce"):
                rc = comm.all_reduce(send.data_ptr(), recv.data_ptr(), n, dt, op, stream)
            elif api == "reduce_scatter":
                rc = comm.reduce_scatter(send.data_ptr(), recv.data_ptr(), n // W, dt, op, stream)
            else:
                rc = comm.reduce(send.data_ptr(), recv.data_ptr(), n, dt, op, 1 % W, stream)
            assert rc == 0, (api, n, rc)
            torch.cuda.synchronize()
            out[(api, n)] = recv.cpu().numpy()
            if recv is not send:
                assert send.cpu().numpy().tobytes() == raw.tobytes(), (api, n, "sendbuff changed")
    assert comm.red_op_destroy(op) == 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring", "rabenseifner"])
@pytest.mark.parametrize("W,dt", [(4, 7), (3, 9), (2, 6), (5, 8), (4, 2)])
def test_premul_collectives_threads(gpu, monkeypatch, W, dt, algo):
    """Thread ranks on one GPU: all_reduce in and out of place, reduce_scatter and reduce to root 1 with a
    pre-multiplied sum, bit-exact against the Sum simulations over pre-multiplied inputs.  algo "": the direct
    collectives (fused chain kernel); "ring": scale, then the ring; "rabenseifner": scale, then Rabenseifner
    (all_reduce only, and only counts divisible by 2^floor(log2 W)).  n = W * 4099: every slot starts off a
    16-B boundary (head and tail scalars live); n = W * 4096: aligned slots.  (4, 7) under "" reads its scalar
    from device memory."""
    import torch
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    rng = np.random.default_rng(100 * W + dt)
    sub = 1 << (W.bit_length() - 1)
    sizes = [n for n in (W * 4099, W * 4096) if algo != "rabenseifner" or n % sub == 0]
    assert sizes
    inputs = {n: [normal_inputs(rng, dt, n) for _ in range(W)] for n in sizes}
    s = scalars_of(dt)[0]
    residence = DEVICE if (W, dt, algo) == (4, 7, "") else HOST

    def body(comm, r):
        st = torch.cuda.Stream()
        return _run_collectives(comm, r, W, dt, algo, inputs, s, residence, st.cuda_stream, torch)

    outs = run_ranks(W, body)
    npd = oracle.NP_DTYPES[dt]
    for n, xs in inputs.items():
        scaled = [premul(x, s, dt) for x in xs]
        want = _expected("all_reduce", scaled, dt, algo)
        for r in range(W):
            for api in ("all_reduce_inplace", "all_reduce"):
                assert outs[r][(api, n)].view(npd).tobytes() == want[r].tobytes(), (api, n, r)
        if algo == "rabenseifner":
            continue
        want = _expected("reduce_scatter", scaled, dt, algo)
        for r in range(W):
            assert outs[r][("reduce_scatter", n)].view(npd).tobytes() == want[r].tobytes(), (n, r)
        want = _expected("reduce", scaled, dt, algo)
        assert outs[1 % W][("reduce", n)].view(npd).tobytes() == want.tobytes(), n


@pytest.mark.gpu
@pytest.mark.parametrize("residence", [DEVICE, HOST])
def test_premul_all_reduce_world1(gpu, residence):
    """W = 1: the result is the scaled input, in place and out of place."""
    import torch
    import dccl_amd
    dt, n = 9, 4099
    rng = np.random.default_rng(11)
    x = normal_inputs(rng, dt, n)
    s = scalars_of(dt)[0]
    want = premul(x, s, dt)
    comm = dccl_amd.Comm.in_process(1, 0)
    try:
        sc = Scalar(s, residence)
        rc, op = comm.red_op_create_premul_sum(sc.ptr, dt, residence)
        assert rc == 0
        send = torch.from_numpy(x.view(np.uint8).copy()).cuda()
        recv = torch.zeros_like(send)
        torch.cuda.synchronize()
        assert comm.all_reduce(send.data_ptr(), recv.data_ptr(), n, dt, op) == 0
        torch.cuda.synchronize()
        assert recv.cpu().numpy().tobytes() == want.tobytes()
        assert send.cpu().numpy().tobytes() == x.tobytes()
        assert comm.all_reduce(send.data_ptr(), send.data_ptr(), n, dt, op) == 0
        assert comm.reduce_scatter(recv.data_ptr(), recv.data_ptr(), n, dt, op) == 0  # scaled twice
        torch.cuda.synchronize()
        assert send.cpu().numpy().tobytes() == want.tobytes()
        assert recv.cpu().numpy().view(np.uint16).tobytes() == premul(want, s, dt).tobytes()
    finally:
        comm.finalize()


# ----------------------------------------------------------------------------- GPU: across processes
XP_DT, XP_N, XP_W = 9, 2 * 4099, 2


def _xp_scalar():
    return to_dtype([0.5], XP_DT)


def _xp_all_reduce(comm, r, W, torch):
    s = _xp_scalar()
    rc, op = comm.red_op_create_premul_sum(s.ctypes.data, XP_DT, HOST)
    assert rc == 0, rc
    x = oracle.synth(XP_N, XP_DT, SUM, SEED, r)
    buf = torch.from_numpy(x.view(np.uint8).copy()).cuda()
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    rc = comm.all_reduce(buf.data_ptr(), buf.data_ptr(), XP_N, XP_DT, op, st.cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert comm.red_op_destroy(op) == 0
    return buf.cpu().numpy()


def _check_xp(results):
    s = _xp_scalar()
    scaled = [premul(oracle.synth(XP_N, XP_DT, SUM, SEED, r), s, XP_DT) for r in range(XP_W)]
    want = _expected_allreduce(scaled, XP_DT, SUM)
    for r in range(XP_W):
        out, fin = results[r]
        assert fin == 0
        assert out.view(np.uint16).tobytes() == want[r].tobytes(), r


@pytest.mark.gpu
def test_premul_ipc_processes(gpu):
    """One process per rank on the IPC transport: the fused chain reads the peers' scratch copies."""
    _check_xp(xproc.run_ipc(XP_W, _xp_all_reduce))


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["ring", "grouped"])
def test_premul_rccl_processes(gpu, algo):
    """The RCCL transport: scale, then the ring ("grouped" takes the ring too for a pre-multiplied sum)."""
    import dccl_amd
    if not dccl_amd.lib.dccl_rccl_available():
        pytest.skip("librccl not loadable")
    _check_xp(xproc.run_rccl(XP_W, _xp_all_reduce, algo))
