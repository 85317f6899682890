"""ncclGroupStart / ncclGroupEnd (include/dccl/dccl.hpp, dccl_group_* of include/dccl/dccl_comm.h) and the batched
strided row copy behind a coalesced group (dccl_copy_rows_multi, include/dccl/dccl_reduce.h).

CPU: group semantics, deferral of host collectives, validation inside a group, and every validation case of the row
copy on never-dereferenced addresses.  GPU: the row copy against numpy (and against dccl_copy_multi, and under graph
capture), and coalesced groups of reductions, bit for bit against the same calls issued one by one AND against the
ring / Rabenseifner simulations with the oracle as the combine.  Ranks are threads on one device,
as in tests/test_collectives.py; every rank issues the identical call sequence."""
import ctypes
import json
import multiprocessing as mp
import os
import subprocess
import threading
import uuid

import numpy as np
import pytest

import oracle
from tests import rabsim, ringsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "dccl_amd", "bin", "dccl_cli")
SUM, PROD, MAX = 0, 1, 2
MULTS = (1, 5, 77, 1000, 4099)


def run_ranks(W, body):
    import dccl_amd
    errs, out = [], [None] * W

    def worker(r):
        try:
            comm = dccl_amd.Comm.in_process(W, r)
            try:
                out[r] = body(comm, r)
            finally:
                comm.finalize()
        except Exception as e:  # pragma: no cover - reported below
            errs.append((r, repr(e)))

    ts = [threading.Thread(target=worker, args=(r,)) for r in range(W)]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "a rank did not return"
    assert not errs, errs
    return out


def stats_delta(before):
    import dccl_amd
    after = dccl_amd.group_stats()
    return {k: after[k] - before[k] for k in after}


# ------------------------------------------------------------------------------------------------------------- CPU
def test_group_depth_and_symbols_cpu():
    import dccl_amd as d
    assert d.group_end() == 5  # ncclInvalidUsage: no group is open
    before = d.group_stats()
    assert d.group_start() == 0 and d.group_start() == 0
    assert d.group_end() == 0  # inner: nothing executes
    assert stats_delta(before)["groups"] == 0
    assert d.group_end() == 0
    assert stats_delta(before) == {"groups": 1, "calls_queued": 0, "collectives_issued": 0, "coalesced_runs": 0,
                                   "tensors_coalesced": 0, "bytes_packed": 0}
    assert d.group_end() == 5
    with d.group():
        pass
    assert stats_delta(before)["groups"] == 2
    out = subprocess.run(["nm", "-D", "-C", "--defined-only", d.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    assert "dccl::ncclGroupStart()" in out and "dccl::ncclGroupEnd()" in out


def test_group_defers_host_collectives_world1_cpu():
    """W = 1: a host all_reduce (a plain copy) and a host all_gather inside a group leave recv untouched until the
    outermost group_end; invalid calls inside a group answer at once and are not queued."""
    import dccl_amd as d
    comm = d.Comm.in_process(1, 0)
    try:
        a = np.arange(100, dtype=np.float32)
        ra = np.full(100, -1, np.float32)
        g = np.arange(7, dtype=np.int64) + 5
        rg = np.full(7, -1, np.int64)
        before = d.group_stats()
        assert d.group_start() == 0
        assert d.group_start() == 0
        assert comm.all_reduce(a.ctypes.data, ra.ctypes.data, 100, 7, SUM) == 0
        assert d.group_end() == 0  # the inner end executes nothing
        assert comm.all_gather(g.ctypes.data, rg.ctypes.data, 7, 4) == 0
        assert comm.all_reduce(a.ctypes.data, ra.ctypes.data, 0, 7, SUM) == 0       # count 0: valid, queues nothing
        assert comm.all_reduce(a.ctypes.data, ra.ctypes.data, 100, 10, SUM) == 4    # unknown dtype
        assert comm.all_reduce(a.ctypes.data, ra.ctypes.data, 100, 7, 4) == 5       # ncclAvg
        assert comm.all_reduce(0, ra.ctypes.data, 100, 7, SUM) == 4                 # NULL send
        assert comm.reduce(a.ctypes.data, ra.ctypes.data, 100, 7, SUM, 1) == 4      # root outside the group
        assert (ra == -1).all() and (rg == -1).all()
        assert stats_delta(before)["calls_queued"] == 2
        assert d.group_end() == 0
        assert np.array_equal(ra, a) and np.array_equal(rg, g)
        assert stats_delta(before) == {"groups": 1, "calls_queued": 2, "collectives_issued": 2, "coalesced_runs": 0,
                                       "tensors_coalesced": 0, "bytes_packed": 0}
    finally:
        assert comm.finalize() == 0


def test_group_threads_host_cpu():
    """W = 3 thread ranks: three host all_gathers and a broadcast in one group give the ungrouped results; a count
    that W does not divide is rejected at once inside the group, on every rank."""
    import dccl_amd as d
    W, slot = 3, 1001
    data = [[(np.arange(slot, dtype=np.int64) + 1) * (100 * j + r + 1) for j in range(3)] for r in range(W)]
    bsrc = np.arange(257, dtype=np.float32) * 0.5

    def body(comm, r):
        def issue():
            recvs = [np.zeros(W * slot, np.int64) for _ in range(3)]
            for j in range(3):
                assert comm.all_gather(data[r][j].ctypes.data, recvs[j].ctypes.data, slot, 4) == 0
            b = bsrc.copy() if r == 2 else np.zeros_like(bsrc)
            assert comm.broadcast(b.ctypes.data, b.ctypes.data, b.size, 7, 2) == 0
            return recvs + [b]
        plain = issue()
        assert d.group_start() == 0
        bad = np.zeros(W + 1, np.float32)
        assert comm.all_reduce(bad.ctypes.data, bad.ctypes.data, W + 1, 7, SUM) == 4  # count % W, at once
        grouped = issue()
        assert all(not x.any() for x in grouped[:3])  # nothing ran yet
        assert d.group_end() == 0
        return plain, grouped

    out = run_ranks(W, body)
    for r in range(W):
        plain, grouped = out[r]
        for j in range(3):
            want = np.concatenate([data[q][j] for q in range(W)])
            assert np.array_equal(plain[j], want) and np.array_equal(grouped[j], want)
        assert np.array_equal(plain[3], bsrc) and np.array_equal(grouped[3], bsrc)


def test_point_to_point_inside_a_group_is_invalid_usage_cpu():
    """ncclSend / ncclRecv inside a group return ncclInvalidUsage (5), with W = 3 thread ranks: through dccl_cli,
    the C++ API's caller (its ranks 0 and 1 address each other, rank 2 issues nothing)."""
    assert os.path.exists(CLI), "dccl_cli is built by build()"
    for api in ("send", "recv"):
        p = subprocess.run([CLI, "-a", api, "-n", "3", "-c", "16", "-r", "1", "-G", "1"], capture_output=True,
                           text=True, timeout=120)
        rows = sorted((json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")),
                      key=lambda row: row["rank"])
        assert [row["rc"] for row in rows] == [5, 5, 0], p.stdout + p.stderr


BASE = 1 << 44  # never dereferenced: validation is pointer arithmetic ahead of any HIP call


def test_copy_rows_validation_without_gpu():
    import dccl_amd as d
    seg = (BASE, BASE + (1 << 30), 100, 100, 256)
    # 1. nsegs outside 0..32, NULL segs, rows == 0
    assert d.copy_rows_multi([seg] * 33, 4) == 4
    assert d.lib.dccl_copy_rows_multi(None, 1, 4, None) == 4
    assert d.lib.dccl_copy_rows_multi(None, -1, 4, None) == 4
    assert d.copy_rows_multi([seg], 0) == 4
    assert d.copy_rows_multi([], 0) == 4           # rows == 0 comes before nsegs == 0
    # 2. nsegs == 0
    assert d.copy_rows_multi([], 3) == 0
    assert d.lib.dccl_copy_rows_multi(None, 0, 3, None) == 0
    # 3. NULL src / dst of a segment with bytes; an empty segment may be NULL
    assert d.copy_rows_multi([(0, BASE, 8, 8, 8)], 2) == 4
    assert d.copy_rows_multi([(BASE, 0, 8, 8, 8)], 2) == 4
    assert d.copy_rows_check([(0, 0, 0, 0, 0)], 2) == 0
    assert d.copy_rows_multi([(0, 0, 0, 0, 0)], 2) == 0  # nothing to launch
    # 4. a stride below row_bytes with rows > 1; rows == 1 does not look at strides
    assert d.copy_rows_multi([(BASE, BASE + 4096, 100, 99, 256)], 2) == 4
    assert d.copy_rows_multi([(BASE, BASE + 4096, 100, 256, 99)], 2) == 4
    assert d.copy_rows_check([(BASE, BASE + 4096, 100, 0, 0)], 1) == 0
    # 5. overlap, exactly.  A pack: destinations interleave row by row without sharing a byte ...
    S, far = 256, BASE + (1 << 30)
    pack = [(BASE, far, 100, 100, S), (BASE + 4096, far + 100, 28, 28, S), (BASE + 8192, far + 128, 128, 128, S)]
    assert d.copy_rows_check(pack, 8) == 0
    unpack = [(dst, src, n, ds, ss) for (src, dst, n, ss, ds) in pack]
    assert d.copy_rows_check(unpack, 8) == 0
    # ... and one shared byte is rejected: between two destinations, in any row
    assert d.copy_rows_multi([pack[0], (BASE + 4096, far + 99, 28, 28, S)], 8) == 4
    assert d.copy_rows_multi([pack[0], (BASE + 4096, far + S - 27, 28, 28, S)], 8) == 4   # wraps into the next row
    assert d.copy_rows_check([pack[0], (BASE + 4096, far + S - 28, 28, 28, S)], 8) == 0
    assert d.copy_rows_multi([pack[0], (BASE + 4096, far + 7 * S + 99, 28, 28, S)], 8) == 4  # only its row 0 meets row 7
    # a destination against a source: another segment's, and its own (src == dst included)
    assert d.copy_rows_multi([pack[0], (far + 99, BASE + 4096, 8, 8, 8)], 2) == 4
    assert d.copy_rows_multi([(BASE, BASE + 99, 100, 100, 256)], 1) == 4
    assert d.copy_rows_multi([(BASE, BASE, 100, 100, 100)], 3) == 4
    assert d.copy_rows_check([(BASE, BASE + 100, 100, 256, 256)], 3) == 0   # src and dst interleave: accepted
    # different strides whose boxes meet are swept: rows of 8 at 0, 24, 48 against rows of 8 at 8, 40, 72
    assert d.copy_rows_check([(BASE, far, 8, 8, 24), (BASE + 64, far + 8, 8, 8, 32)], 3) == 0
    assert d.copy_rows_multi([(BASE, far, 8, 8, 24), (BASE + 64, far + 9, 8, 8, 32)], 3) == 4   # 41..48 meets 48..55
    # validation order: rows == 0 beats a NULL pointer, a NULL pointer beats a stride, a stride beats overlap
    assert d.copy_rows_multi([(0, BASE, 8, 8, 8)], 0) == 4
    assert d.copy_rows_check([(BASE, BASE, 100, 50, 50)], 2) == 4


# ------------------------------------------------------------------------------------------------------------- GPU
ROW_BYTES = (1, 15, 16, 17, 1023, 1025, 2 * 4099)


def rows_case(nsegs, rows, seed):
    """Segments laid out in one source and one destination arena: each row sits at its own byte offset (0..15 on
    either side, independently), strides exceed row_bytes by a few bytes, 64-byte guard bands around every row."""
    rng = np.random.default_rng(seed)
    segs, s_at, d_at = [], 64, 64
    for i in range(nsegs):
        n = ROW_BYTES[(i + seed) % len(ROW_BYTES)]
        ss, ds = n + int(rng.integers(0, 40)), n + 64 + int(rng.integers(0, 40))
        s_off = (s_at + 255) // 256 * 256 + int(rng.integers(0, 16))
        d_off = (d_at + 255) // 256 * 256 + int(rng.integers(0, 16))
        segs.append((s_off, d_off, n, ss, ds))
        s_at, d_at = s_off + rows * ss + 64, d_off + rows * ds + 64
    return segs, s_at + 256, d_at + 256


def rows_expected(segs, rows, src, dst):
    want = dst.copy()
    for (s_off, d_off, n, ss, ds) in segs:
        for r in range(rows):
            want[d_off + r * ds:d_off + r * ds + n] = src[s_off + r * ss:s_off + r * ss + n]
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("nsegs", [1, 32])
def test_copy_rows_multi_against_numpy(gpu, nsegs, rows):
    import torch
    import dccl_amd as d
    for seed in range(len(ROW_BYTES) if nsegs == 1 else 2):  # one segment: every row size in turn
        segs, s_len, d_len = rows_case(nsegs, rows, seed)
        rng = np.random.default_rng(1000 + seed)
        src = rng.integers(0, 256, s_len, dtype=np.uint8)
        dst = rng.integers(0, 256, d_len, dtype=np.uint8)
        t_src, t_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
        assert t_src.data_ptr() % 256 == 0 and t_dst.data_ptr() % 256 == 0
        abs_segs = [(t_src.data_ptr() + s, t_dst.data_ptr() + q, n, ss, ds) for (s, q, n, ss, ds) in segs]
        torch.cuda.synchronize()
        assert d.copy_rows_multi(abs_segs, rows) == 0
        torch.cuda.synchronize()
        want = rows_expected(segs, rows, src, dst)
        assert t_dst.cpu().numpy().tobytes() == want.tobytes(), (nsegs, rows, seed)  # guard bands included
        assert t_src.cpu().numpy().tobytes() == src.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("P", [3, 8])
def test_copy_rows_pack_shape_against_copy_multi(gpu, P):
    """The pack of a group (slot-major, group_plan.hpp's layout) in one launch, against dccl_copy_multi per tensor;
    then the unpack restores the tensors."""
    import torch
    import dccl_amd as d
    rng = np.random.default_rng(P)
    slots = [m * 4 for m in MULTS]
    S = (sum(slots) + 127) // 128 * 128
    tensors = [torch.from_numpy(rng.integers(0, 256, P * n, dtype=np.uint8)).cuda() for n in slots]
    pack_a = torch.full((P * S,), 0x5A, dtype=torch.uint8, device="cuda")
    pack_b = pack_a.clone()
    offs = [sum(slots[:i]) for i in range(len(slots))]
    torch.cuda.synchronize()
    assert d.copy_rows_multi([(t.data_ptr(), pack_a.data_ptr() + o, n, n, S) for t, o, n in zip(tensors, offs, slots)],
                             P) == 0
    for t, o, n in zip(tensors, offs, slots):
        assert d.copy_multi([t.data_ptr() + k * n for k in range(P)], [pack_b.data_ptr() + k * S + o for k in range(P)],
                            n) == 0
    torch.cuda.synchronize()
    a = pack_a.cpu().numpy()
    assert a.tobytes() == pack_b.cpu().numpy().tobytes()
    assert (a.reshape(P, S)[:, sum(slots):] == 0x5A).all()  # pad bytes are not written
    back = [torch.zeros_like(t) for t in tensors]
    assert d.copy_rows_multi([(pack_a.data_ptr() + o, b.data_ptr(), n, S, n) for b, o, n in zip(back, offs, slots)],
                             P) == 0
    torch.cuda.synchronize()
    for t, b in zip(tensors, back):
        assert torch.equal(t, b)


def _hip():
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    pytest.skip("the HIP runtime is not loaded")


@pytest.mark.gpu
def test_copy_rows_multi_graph_capture(gpu):
    """One launch captured on a non-default stream (torch.cuda.graph) and replayed; a raw capture of the same call
    holds exactly one node."""
    import torch
    import dccl_amd as d
    rows = 3
    segs, s_len, d_len = rows_case(32, rows, 5)
    rng = np.random.default_rng(55)
    src = rng.integers(0, 256, s_len, dtype=np.uint8)
    dst = rng.integers(0, 256, d_len, dtype=np.uint8)
    t_src, t_dst = torch.from_numpy(src).cuda(), torch.from_numpy(dst).cuda()
    abs_segs = [(t_src.data_ptr() + s, t_dst.data_ptr() + q, n, ss, ds) for (s, q, n, ss, ds) in segs]
    g = torch.cuda.CUDAGraph()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=st):
            assert d.copy_rows_multi(abs_segs, rows, st.cuda_stream) == 0
    torch.cuda.synchronize()
    assert t_dst.cpu().numpy().tobytes() == dst.tobytes()  # capture does not execute
    for _ in range(2):
        src = rng.integers(0, 256, s_len, dtype=np.uint8)
        t_src.copy_(torch.from_numpy(src))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert t_dst.cpu().numpy().tobytes() == rows_expected(segs, rows, src, dst).tobytes()
    hip = _hip()
    graph, n = ctypes.c_void_p(), ctypes.c_size_t(0)
    stream = ctypes.c_void_p(st.cuda_stream)
    assert hip.hipStreamBeginCapture(stream, 1) == 0  # hipStreamCaptureModeThreadLocal
    rc = d.copy_rows_multi(abs_segs, rows, st.cuda_stream)
    assert hip.hipStreamEndCapture(stream, ctypes.byref(graph)) == 0
    assert rc == 0
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    assert hip.hipGraphDestroy(graph) == 0
    assert n.value == 1


# dtype / op sets of the coalesced groups: (name, dtype, op, premul scalar)
COMBOS = [("fp32_sum", 7, SUM, None), ("bf16_sum", 9, SUM, None), ("fp64_prod", 8, PROD, None),
          ("int8_max", 0, MAX, None), ("fp32_premul", 7, SUM, 0.3)]


def make_tensor(rng, n, dt, op):
    if dt == 7:
        return rng.standard_normal(n).astype(np.float32)
    if dt == 9:
        return (rng.standard_normal(n).astype(np.float32).view(np.uint32) >> 16).astype(np.uint16)
    if dt == 8:
        return rng.uniform(0.5, 1.5, n)
    return rng.integers(-128, 128, n).astype(np.int8)


def combine_of(dt, op):
    def combine(s, r):
        assert oracle.expected_reduce(np.ascontiguousarray(s), r, dt, op) == 0
    return combine


def copy(dst, src):
    dst[:] = src


def scaled(x, dt, scalar):
    if scalar is None:
        return x.copy()
    return oracle.combine(np.full(x.size, scalar, x.dtype), x, dt, PROD)


def simulate(api, algo, per_rank, dt, op, scalar, W, root=1):
    """per_rank[r]: one tensor per rank -> what every rank must hold afterwards (None: nothing is defined)."""
    bufs = [scaled(x, dt, scalar) for x in per_rank]
    if api == "all_reduce":
        if algo == "rabenseifner":
            return rabsim.rabenseifner_allreduce(bufs, combine_of(dt, op))
        return ringsim.ring_allreduce(bufs, combine_of(dt, op), copy)
    ringsim.reduce_scatter_ring(bufs, combine_of(dt, op), *ringsim.rs_maps())
    slot = bufs[0].size // W
    if api == "reduce_scatter":
        return [bufs[r][r * slot:(r + 1) * slot] for r in range(W)]
    whole = np.concatenate([bufs[o][o * slot:(o + 1) * slot] for o in range(W)])  # the root gathers every slot
    return [whole if r == root else None for r in range(W)]


def issue(comm, r, api, W, dt, op, sends, st, root=1):
    """One call per tensor; even tensors in place where the api allows it.  Returns the receive buffers."""
    import torch
    if api == "reduce_scatter":
        outs = [torch.zeros(t.numel() // W, dtype=t.dtype, device="cuda") for t in sends]
    else:
        outs = [t if i % 2 == 0 else torch.zeros_like(t) for i, t in enumerate(sends)]
    torch.cuda.synchronize()  # the fills above ran on torch's stream, the collectives run on `st`
    for t, recv in zip(sends, outs):
        n = t.numel()
        if api == "all_reduce":
            assert comm.all_reduce(t.data_ptr(), recv.data_ptr(), n, dt, op, st) == 0
        elif api == "reduce_scatter":
            assert comm.reduce_scatter(t.data_ptr(), recv.data_ptr(), n // W, dt, op, st) == 0
        else:
            assert comm.reduce(t.data_ptr(), recv.data_ptr(), n, dt, op, root, st) == 0
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("W,algo", [(3, ""), (4, ""), (8, ""), (4, "ring"), (4, "rabenseifner"), (5, "rabenseifner")])
def test_coalesced_reductions_bit_for_bit(gpu, W, algo, monkeypatch):
    """Groups of five reductions of P * {1, 5, 77, 1000, 4099} elements: every output equals the same calls issued
    one by one AND the simulation with the oracle; each group is one coalesced run of five tensors that issued
    one collective."""
    import torch
    import dccl_amd as d
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    monkeypatch.delenv("DCCL_GROUP_COALESCE", raising=False)
    monkeypatch.delenv("DCCL_GROUP_COALESCE_MAX_BYTES", raising=False)
    P = 1 << (W.bit_length() - 1) if algo == "rabenseifner" else W
    apis = ["all_reduce"] if algo == "rabenseifner" else ["all_reduce", "reduce_scatter", "reduce"]
    rng = np.random.default_rng(7 * W + len(algo))
    cases = []  # (api, name, dt, op, scalar, inputs[r][i], want[i][r])
    for api in apis:
        for name, dt, op, scalar in COMBOS:
            inputs = [[make_tensor(rng, P * m, dt, op) for m in MULTS] for _ in range(W)]
            want = [simulate(api, algo, [inputs[r][i] for r in range(W)], dt, op, scalar, W) for i in range(len(MULTS))]
            cases.append((api, name, dt, op, scalar, inputs, want))

    def body(comm, r):
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        got = []
        for api, name, dt, op, scalar, inputs, _ in cases:
            use_op = op
            if scalar is not None:
                s = np.array([scalar], np.float32)
                rc, use_op = comm.red_op_create_premul_sum(s.ctypes.data, dt, 1)
                assert rc == 0
            pair = []
            for grouped in (False, True):
                sends = [torch.from_numpy(x.view(np.uint8).copy()).cuda().view(torch.uint8) for x in inputs[r]]
                sends = [t.view({1: torch.int8, 2: torch.int16, 4: torch.float32, 8: torch.float64}[x.itemsize])
                         for t, x in zip(sends, inputs[r])]
                torch.cuda.synchronize()
                if grouped:
                    assert d.group_start() == 0
                outs = issue(comm, r, api, W, dt, use_op, sends, st)
                if grouped:
                    assert d.group_end() == 0
                stream.synchronize()
                pair.append([o.cpu().numpy().tobytes() for o in outs])
            if scalar is not None:
                assert comm.red_op_destroy(use_op) == 0
            got.append(pair)
        return got

    before = d.group_stats()
    out = run_ranks(W, body)
    delta = stats_delta(before)
    n = len(cases)
    assert delta["groups"] == W * n and delta["calls_queued"] == W * n * 5
    assert delta["coalesced_runs"] == W * n and delta["tensors_coalesced"] == W * n * 5
    assert delta["collectives_issued"] == W * n  # one collective per group, not five
    for c, (api, name, dt, op, scalar, inputs, want) in enumerate(cases):
        for r in range(W):
            plain, grouped = out[r][c]
            for i in range(len(MULTS)):
                if want[i][r] is None:  # ncclReduce away from the root defines no output
                    continue
                assert plain[i] == want[i][r].tobytes(), ("plain", api, name, r, i)
                assert grouped[i] == want[i][r].tobytes(), ("grouped", api, name, r, i)


def _small_inputs(W, counts, seed):
    rng = np.random.default_rng(seed)
    return [[rng.standard_normal(n).astype(np.float32) for n in counts] for _ in range(W)]


def _ring_want(inputs, W, i, dt=7):
    return ringsim.ring_allreduce([inputs[r][i].copy() for r in range(W)], combine_of(dt, SUM), copy)


@pytest.mark.gpu
def test_mixed_group(gpu, monkeypatch):
    """W = 4: fp32, fp32, bf16, fp32, a host-buffer all-reduce, an all-gather and one tensor at the coalescing
    limit (64 KiB here).  Only the first two coalesce; everything is correct."""
    import torch
    import dccl_amd as d
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", "")
    monkeypatch.delenv("DCCL_GROUP_COALESCE", raising=False)
    monkeypatch.setenv("DCCL_GROUP_COALESCE_MAX_BYTES", str(64 << 10))
    W = 4
    counts = [W * 77, W * 1000, W * 5, W * 4099, W * 33, W * 9, 16384]  # the last: 64 KiB of fp32, at the limit
    inputs = _small_inputs(W, counts, 11)
    bf = [(inputs[r][2].view(np.uint32) >> 16).astype(np.uint16) for r in range(W)]
    want = {i: _ring_want(inputs, W, i) for i in (0, 1, 3, 4, 6)}
    want_bf = ringsim.ring_allreduce([x.copy() for x in bf], combine_of(9, SUM), copy)
    want_ag = np.concatenate([inputs[q][5] for q in range(W)])

    def body(comm, r):
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        dev = {i: torch.from_numpy(inputs[r][i].copy()).cuda() for i in (0, 1, 3, 5, 6)}
        t_bf = torch.from_numpy(bf[r].view(np.int16).copy()).cuda()
        host = inputs[r][4].copy()
        ag = torch.zeros(W * counts[5], device="cuda")
        torch.cuda.synchronize()
        with d.group():
            assert comm.all_reduce(dev[0].data_ptr(), dev[0].data_ptr(), counts[0], 7, SUM, st) == 0
            assert comm.all_reduce(dev[1].data_ptr(), dev[1].data_ptr(), counts[1], 7, SUM, st) == 0
            assert comm.all_reduce(t_bf.data_ptr(), t_bf.data_ptr(), counts[2], 9, SUM, st) == 0
            assert comm.all_reduce(dev[3].data_ptr(), dev[3].data_ptr(), counts[3], 7, SUM, st) == 0
            assert comm.all_reduce(host.ctypes.data, host.ctypes.data, counts[4], 7, SUM) == 0
            assert comm.all_gather(dev[5].data_ptr(), ag.data_ptr(), counts[5], 7, st) == 0
            assert comm.all_reduce(dev[6].data_ptr(), dev[6].data_ptr(), counts[6], 7, SUM, st) == 0
        stream.synchronize()
        return ({i: dev[i].cpu().numpy() for i in (0, 1, 3, 6)}, t_bf.cpu().numpy().view(np.uint16), host,
                ag.cpu().numpy())

    before = d.group_stats()
    out = run_ranks(W, body)
    assert stats_delta(before) == {"groups": W, "calls_queued": 7 * W, "collectives_issued": 6 * W,
                                   "coalesced_runs": W, "tensors_coalesced": 2 * W,
                                   "bytes_packed": W * 4 * (counts[0] + counts[1])}
    for r in range(W):
        dev, t_bf, host, ag = out[r]
        for i in (0, 1, 3, 6):
            assert dev[i].tobytes() == want[i][r].tobytes(), (r, i)
        assert t_bf.tobytes() == want_bf[r].tobytes(), r
        assert host.tobytes() == want[4][r].tobytes(), r
        assert ag.tobytes() == want_ag.tobytes(), r


@pytest.mark.gpu
def test_forty_small_tensors_are_two_runs(gpu, monkeypatch):
    import torch
    import dccl_amd as d
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", "")
    monkeypatch.delenv("DCCL_GROUP_COALESCE", raising=False)
    monkeypatch.delenv("DCCL_GROUP_COALESCE_MAX_BYTES", raising=False)
    W = 3
    counts = [W * (1 + (7 * i) % 13) for i in range(40)]
    inputs = _small_inputs(W, counts, 40)
    want = [_ring_want(inputs, W, i) for i in range(40)]

    def body(comm, r):
        stream = torch.cuda.Stream()
        ts = [torch.from_numpy(x.copy()).cuda() for x in inputs[r]]
        torch.cuda.synchronize()
        with d.group():
            for t, n in zip(ts, counts):
                assert comm.all_reduce(t.data_ptr(), t.data_ptr(), n, 7, SUM, stream.cuda_stream) == 0
        stream.synchronize()
        return [t.cpu().numpy() for t in ts]

    before = d.group_stats()
    out = run_ranks(W, body)
    delta = stats_delta(before)
    assert delta["coalesced_runs"] == 2 * W and delta["tensors_coalesced"] == 40 * W  # 32 + 8
    assert delta["collectives_issued"] == 2 * W and delta["calls_queued"] == 40 * W
    for r in range(W):
        for i in range(40):
            assert out[r][i].tobytes() == want[i][r].tobytes(), (r, i)


@pytest.mark.gpu
def test_two_streams_in_one_run(gpu, monkeypatch):
    """The second tensor of the run is produced on stream B (behind a long-running kernel) and consumed on stream B
    after group_end, with no host synchronisation in between: the run's stream waits for B, and B for the unpack."""
    import torch
    import dccl_amd as d
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", "")
    monkeypatch.delenv("DCCL_GROUP_COALESCE", raising=False)
    monkeypatch.delenv("DCCL_GROUP_COALESCE_MAX_BYTES", raising=False)
    W = 3
    counts = [W * 1000, W * 4099]
    inputs = _small_inputs(W, counts, 2)
    want = [_ring_want(inputs, W, i) for i in range(2)]

    def body(comm, r):
        a, b = torch.cuda.Stream(), torch.cuda.Stream()
        t0 = torch.from_numpy(inputs[r][0].copy()).cuda()
        staged = torch.from_numpy(inputs[r][1].copy()).cuda()
        t1 = torch.zeros_like(staged)
        torch.cuda.synchronize()
        with torch.cuda.stream(b):  # the producer: late on purpose
            torch.cuda._sleep(20_000_000)
            t1.copy_(staged, non_blocking=True)
        with d.group():
            assert comm.all_reduce(t0.data_ptr(), t0.data_ptr(), counts[0], 7, SUM, a.cuda_stream) == 0
            assert comm.all_reduce(t1.data_ptr(), t1.data_ptr(), counts[1], 7, SUM, b.cuda_stream) == 0
        with torch.cuda.stream(b):  # the consumer: ordered behind the unpack by the library's event
            seen = t1 * 1.0
        b.synchronize()
        a.synchronize()
        return t0.cpu().numpy(), seen.cpu().numpy()

    before = d.group_stats()
    out = run_ranks(W, body)
    assert stats_delta(before)["coalesced_runs"] == W
    for r in range(W):
        assert out[r][0].tobytes() == want[0][r].tobytes(), r
        assert out[r][1].tobytes() == want[1][r].tobytes(), r


@pytest.mark.gpu
def test_coalescing_turned_off(gpu, monkeypatch):
    """DCCL_GROUP_COALESCE=0: the same outputs, every call runs as the plain call at group_end."""
    import torch
    import dccl_amd as d
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", "")
    monkeypatch.delenv("DCCL_GROUP_COALESCE_MAX_BYTES", raising=False)
    W = 4
    counts = [W * m for m in MULTS]
    inputs = _small_inputs(W, counts, 5)
    want = [_ring_want(inputs, W, i) for i in range(len(counts))]

    def body(comm, r):
        stream = torch.cuda.Stream()
        ts = [torch.from_numpy(x.copy()).cuda() for x in inputs[r]]
        torch.cuda.synchronize()
        with d.group():
            for t, n in zip(ts, counts):
                assert comm.all_reduce(t.data_ptr(), t.data_ptr(), n, 7, SUM, stream.cuda_stream) == 0
        stream.synchronize()
        return [t.cpu().numpy() for t in ts]

    for off in (True, False):
        if off:
            monkeypatch.setenv("DCCL_GROUP_COALESCE", "0")
        else:
            monkeypatch.delenv("DCCL_GROUP_COALESCE")
        before = d.group_stats()
        out = run_ranks(W, body)
        delta = stats_delta(before)
        assert delta["coalesced_runs"] == (0 if off else W) and delta["tensors_coalesced"] == (0 if off else 5 * W)
        assert delta["collectives_issued"] == (5 * W if off else W) and delta["calls_queued"] == 5 * W
        for r in range(W):
            for i in range(len(counts)):
                assert out[r][i].tobytes() == want[i][r].tobytes(), (off, r, i)


# A queued call owns its scalar: the op may be destroyed, and its slot taken by another scalar, before group_end.
FIRST_S, SECOND_S = np.float32(0.5), np.float32(3.0)
SLOT_N = 1031


def _unit_interval_inputs(seed, dt, n):
    """Inputs in [1, 2): x * 0.5 and x * 3.0 differ for every one of them."""
    x = np.random.default_rng(seed).uniform(1.0, 2.0, n).astype(np.float32)
    return x if dt == 7 else (x.view(np.uint32) >> 16).astype(np.uint16)


def _create_scaling_op(comm, kind, dt, s):
    hs = np.array([s], np.float32)  # fp32 is the operands' dtype for the pre-multiplied sum, and the wide scalar's
    create = comm.red_op_create_premul_sum if kind == "premul" else comm.red_op_create_wide_scaled_sum
    rc, op = create(hs.ctypes.data, dt, 1)
    assert rc == 0, rc
    return op


def _assert_differ_everywhere(a, b):
    assert a.shape == b.shape and np.all(a != b)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,dt", [("premul", 7), ("wide_scaled", 9)])
def test_queued_call_keeps_its_scalar_world1(gpu, kind, dt):
    """W = 1: an all-reduce queued with a host-immediate scalar of 0.5, then the op destroyed and one with 3.0 created
    in the same slot, then group_end.  The result is the 0.5 one, bit for bit."""
    import torch
    import dccl_amd as d
    from tests.test_wide_scaled import scaled_sum
    x = _unit_interval_inputs(61, dt, SLOT_N)
    if kind == "premul":
        want, other = scaled(x, dt, FIRST_S), scaled(x, dt, SECOND_S)
    else:
        want, other = scaled_sum([x], dt, FIRST_S), scaled_sum([x], dt, SECOND_S)
    _assert_differ_everywhere(want, other)

    def body(comm, r):
        stream = torch.cuda.Stream()
        send = torch.from_numpy(x.view(np.uint8).copy()).cuda()
        recv = torch.zeros_like(send)
        torch.cuda.synchronize()
        op = _create_scaling_op(comm, kind, dt, FIRST_S)
        assert d.group_start() == 0
        assert comm.all_reduce(send.data_ptr(), recv.data_ptr(), SLOT_N, dt, op, stream.cuda_stream) == 0
        assert comm.red_op_destroy(op) == 0
        again = _create_scaling_op(comm, kind, dt, SECOND_S)
        assert again == op  # the same slot: whoever still looked there would find 3.0
        assert d.group_end() == 0
        stream.synchronize()
        assert comm.red_op_destroy(again) == 0
        return recv.cpu().numpy()

    out = run_ranks(1, body)
    assert out[0].tobytes() == want.tobytes()


@pytest.mark.gpu
def test_packed_run_keeps_its_scalar(gpu, monkeypatch):
    """W = 2 thread ranks: two small all-reduces with one host-immediate pre-multiplied sum (0.5) make one packed run;
    the op is destroyed and recreated with 3.0 before group_end.  Both results are the 0.5 ones, bit for bit.  Each
    tensor has W * 1,031 elements: an all-reduce's count is a multiple of W."""
    import torch
    import dccl_amd as d
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", "")
    monkeypatch.delenv("DCCL_GROUP_COALESCE", raising=False)
    monkeypatch.delenv("DCCL_GROUP_COALESCE_MAX_BYTES", raising=False)
    W, n, dt = 2, 2 * SLOT_N, 7
    inputs = [[_unit_interval_inputs(70 + 2 * r + i, dt, n) for i in range(2)] for r in range(W)]
    want = [simulate("all_reduce", "", [inputs[r][i] for r in range(W)], dt, SUM, FIRST_S, W) for i in range(2)]
    other = [simulate("all_reduce", "", [inputs[r][i] for r in range(W)], dt, SUM, SECOND_S, W) for i in range(2)]
    for i in range(2):
        for r in range(W):
            _assert_differ_everywhere(want[i][r], other[i][r])

    def body(comm, r):
        stream = torch.cuda.Stream()
        ts = [torch.from_numpy(x.copy()).cuda() for x in inputs[r]]
        torch.cuda.synchronize()
        op = _create_scaling_op(comm, "premul", dt, FIRST_S)
        assert d.group_start() == 0
        for t in ts:
            assert comm.all_reduce(t.data_ptr(), t.data_ptr(), n, dt, op, stream.cuda_stream) == 0
        assert comm.red_op_destroy(op) == 0
        again = _create_scaling_op(comm, "premul", dt, SECOND_S)
        assert again == op
        assert d.group_end() == 0
        stream.synchronize()
        assert comm.red_op_destroy(again) == 0
        return [t.cpu().numpy() for t in ts]

    before = d.group_stats()
    out = run_ranks(W, body)
    delta = stats_delta(before)
    assert delta["coalesced_runs"] == W and delta["tensors_coalesced"] == 2 * W
    for r in range(W):
        for i in range(2):
            assert out[r][i].tobytes() == want[i][r].tobytes(), (r, i)


@pytest.mark.gpu
def test_queued_call_runs_by_the_name_it_was_validated_under(gpu, monkeypatch):
    """W = 3 thread ranks queue one fp32 Sum all-reduce of 4 elements under DCCL_ALLREDUCE_ALGORITHM=rabenseifner:
    4 is a multiple of 2^floor(log2 3) = 2, the count that name is checked for, and not of W.  Once every rank has
    queued it, one rank sets the variable to "" and only then does any rank reach group_end.  The call runs the
    algorithm it was validated under: every rank holds the Rabenseifner result, bit for bit, not a direct all-reduce
    with slots of 4 / 3 = 1 element."""
    import torch
    import dccl_amd as d
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", "rabenseifner")
    W, n = 3, 4
    inputs = [np.random.default_rng(90 + r).standard_normal(n).astype(np.float32) for r in range(W)]
    want = rabsim.rabenseifner_allreduce([x.copy() for x in inputs], combine_of(7, SUM))
    meet = threading.Barrier(W)

    def body(comm, r):
        stream = torch.cuda.Stream()
        t = torch.from_numpy(inputs[r].copy()).cuda()
        torch.cuda.synchronize()
        assert d.group_start() == 0
        assert comm.all_reduce(t.data_ptr(), t.data_ptr(), n, 7, SUM, stream.cuda_stream) == 0
        meet.wait(timeout=60)
        if r == 0:
            os.environ["DCCL_ALLREDUCE_ALGORITHM"] = ""
        meet.wait(timeout=60)
        assert d.group_end() == 0
        stream.synchronize()
        return t.cpu().numpy()

    out = run_ranks(W, body)
    for r in range(W):
        assert out[r].tobytes() == want[r].tobytes(), (r, out[r], want[r])


def _ipc_group_rank(r, W, counts, tag, q):
    os.environ["DCCL_BOOTSTRAP_TAG"] = tag
    os.environ.setdefault("DCCL_IPC_TIMEOUT_S", "60")
    try:
        import torch
        import dccl_amd
        torch.cuda.set_device(0)
        inputs = _small_inputs(W, counts, 77)
        comm = dccl_amd.Comm.ipc(W, r)
        res = {}
        try:
            st = torch.cuda.Stream()
            for grouped in (False, True):
                ts = [torch.from_numpy(x.copy()).cuda() for x in inputs[r]]
                torch.cuda.synchronize()
                before = dccl_amd.group_stats()
                if grouped:
                    assert dccl_amd.group_start() == 0
                for t, n in zip(ts, counts):
                    assert comm.all_reduce(t.data_ptr(), t.data_ptr(), n, 7, SUM, st.cuda_stream) == 0
                if grouped:
                    assert dccl_amd.group_end() == 0
                st.synchronize()
                after = dccl_amd.group_stats()
                res[grouped] = ([t.cpu().numpy().tobytes() for t in ts], after["coalesced_runs"] - before["coalesced_runs"])
        finally:
            res["finalize"] = comm.finalize()
        q.put((r, res, None))
    except Exception as e:  # pragma: no cover - reported by the parent
        q.put((r, None, repr(e)))


@pytest.mark.gpu
def test_ipc_group_of_three_all_reduces(gpu):
    """W = 2 processes on the IPC transport: a group of three all-reduces is one coalesced run whose outputs are
    the ungrouped calls' bytes."""
    W, counts = 2, [2 * 77, 2 * 4099, 2 * 1000]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    tag = "test_" + uuid.uuid4().hex[:12]
    ps = [ctx.Process(target=_ipc_group_rank, args=(r, W, counts, tag, q)) for r in range(W)]
    for p in ps:
        p.start()
    results = {}
    try:
        for _ in range(W):
            r, res, err = q.get(timeout=240)
            assert err is None, (r, err)
            results[r] = res
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    inputs = _small_inputs(W, counts, 77)
    want = [_ring_want(inputs, W, i) for i in range(len(counts))]
    for r in range(W):
        plain, runs_plain = results[r][False]
        grouped, runs_grouped = results[r][True]
        assert runs_plain == 0 and runs_grouped == 1
        assert results[r]["finalize"] == 0
        for i in range(len(counts)):
            assert plain[i] == want[i][r].tobytes() and grouped[i] == plain[i], (r, i)


def _ipc_rab_name_rank(r, W, slots, tag, q):
    os.environ["DCCL_BOOTSTRAP_TAG"] = tag
    os.environ["DCCL_ALLREDUCE_ALGORITHM"] = "rabenseifner"
    os.environ.setdefault("DCCL_IPC_TIMEOUT_S", "60")
    try:
        import torch
        import dccl_amd
        torch.cuda.set_device(0)
        inputs = _small_inputs(W, [W * n for n in slots], 78)
        comm = dccl_amd.Comm.ipc(W, r)
        res = {}
        try:
            st = torch.cuda.Stream()
            probe = torch.zeros(W * 4, device="cuda")
            torch.cuda.synchronize()
            res["ar_plain"] = comm.all_reduce(probe.data_ptr(), probe.data_ptr(), W * 4, 7, SUM, st.cuda_stream)
            assert dccl_amd.group_start() == 0
            res["ar_grouped"] = comm.all_reduce(probe.data_ptr(), probe.data_ptr(), W * 4, 7, SUM, st.cuda_stream)
            assert dccl_amd.group_end() == 0  # nothing was queued
            for grouped in (False, True):
                ts = [torch.from_numpy(x.copy()).cuda() for x in inputs[r]]
                outs = [torch.zeros(n, device="cuda") for n in slots]
                torch.cuda.synchronize()
                before = dccl_amd.group_stats()
                if grouped:
                    assert dccl_amd.group_start() == 0
                for t, o, n in zip(ts, outs, slots):
                    assert comm.reduce_scatter(t.data_ptr(), o.data_ptr(), n, 7, SUM, st.cuda_stream) == 0
                if grouped:
                    assert dccl_amd.group_end() == 0
                st.synchronize()
                after = dccl_amd.group_stats()
                res[grouped] = ([o.cpu().numpy().tobytes() for o in outs],
                                after["coalesced_runs"] - before["coalesced_runs"])
        finally:
            res["finalize"] = comm.finalize()
        q.put((r, res, None))
    except Exception as e:  # pragma: no cover - reported by the parent
        q.put((r, None, repr(e)))


@pytest.mark.gpu
def test_ipc_world3_with_the_rabenseifner_name(gpu):
    """W = 3 processes on the IPC transport with DCCL_ALLREDUCE_ALGORITHM=rabenseifner (a non-power-of-two world,
    where Rabenseifner's slot count differs from W): the IPC transport always runs the direct forms, so an
    all-reduce under that name is ncclInvalidUsage inside a group exactly as outside it, and is not queued; a group
    of reduce-scatters is packed into W slots and gives the ungrouped calls' bytes."""
    W, slots = 3, [77, 4099, 1000]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    tag = "test_" + uuid.uuid4().hex[:12]
    ps = [ctx.Process(target=_ipc_rab_name_rank, args=(r, W, slots, tag, q)) for r in range(W)]
    for p in ps:
        p.start()
    results = {}
    try:
        for _ in range(W):
            r, res, err = q.get(timeout=240)
            assert err is None, (r, err)
            results[r] = res
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    inputs = _small_inputs(W, [W * n for n in slots], 78)
    for i, n in enumerate(slots):
        work = [inputs[r][i].copy() for r in range(W)]
        ringsim.reduce_scatter_ring(work, combine_of(7, SUM), *ringsim.rs_maps())
        for r in range(W):
            plain, runs_plain = results[r][False]
            grouped, runs_grouped = results[r][True]
            assert runs_plain == 0 and runs_grouped == 1
            assert plain[i] == work[r][r * n:(r + 1) * n].tobytes() and grouped[i] == plain[i], (r, i)
    for r in range(W):
        assert results[r]["ar_plain"] == 5 and results[r]["ar_grouped"] == 5
        assert results[r]["finalize"] == 0


@pytest.mark.gpu
def test_cli_group_flag(gpu):
    """dccl_cli -G: the same hashes with coalescing on and off."""
    assert os.path.exists(CLI), "dccl_cli is built by build()"
    rows = {}
    for off in ("1", "0"):
        env = {**os.environ, "DCCL_GROUP_COALESCE": off, "DCCL_ALLREDUCE_ALGORITHM": ""}
        env.pop("DCCL_GROUP_COALESCE_MAX_BYTES", None)
        p = subprocess.run([CLI, "-a", "all_reduce", "-G", "4", "-n", "4", "-c", "1024", "-g", "0"], env=env,
                           capture_output=True, text=True, timeout=240)
        assert p.returncode == 0, p.stdout + p.stderr
        rows[off] = sorted((json.loads(line) for line in p.stdout.splitlines() if line.startswith("{")),
                           key=lambda row: row["rank"])
        assert len(rows[off]) == 4 and all(row["rc"] == 0 and row["group"] == 4 for row in rows[off])
        assert all(row["us_per_group"] > 0 for row in rows[off])
    assert [row["fnv1a"] for row in rows["1"]] == [row["fnv1a"] for row in rows["0"]]
    assert len({row["fnv1a"] for row in rows["1"]}) == 1  # an all-reduce: every rank holds the same bytes
