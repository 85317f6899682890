"""The collectives' stream ordering.

CPU: tests/native/stream_order_harness.cpp links the collectives' host code against a recording fake HIP runtime
(tests/native/fake_hip.cpp) and runs every API on every path of the thread transport, alone, three times back to back,
in pairs on two streams and in groups; tests/native/hb_check.hpp builds the happens-before relation HIP guarantees
(stream order, event edges, host synchronisations) and reports every pair of conflicting accesses it leaves unordered.
The tests below build that harness with ROCm's clang++ under ASan + UBSan and assert on its JSON: no hazard, no cycle,
the library wrote exactly recvbuff, every rank returned 0; the checker's answers on hand-written traces; and the waits
that must be load-bearing (ignored alone, a hazard appears) are.  There is no allow-list.

GPU: two tests on thread ranks that never synchronise between the steps of a round.  They can fail only when ordering
is broken; they cannot prove it (at these sizes a missing wait would rarely show): the proof is the CPU part.
"""
import functools
import json
import math
import os
import shutil
import subprocess
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from tests import ringsim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dccl_amd", "csrc")
NATIVE = os.path.join(ROOT, "tests", "native")
PRODUCT = ("comm", "algorithms", "grouped", "bootstrap", "dccl_api", "direct", "rccl_transport")
HARNESS = ("fake_hip", "stream_order_harness")


def rocm_clang():
    """ROCm's clang++ next to hipcc, and ROCm's include directory; None where there is no ROCm compiler."""
    hipcc = shutil.which("hipcc")
    roots = [os.path.dirname(os.path.dirname(os.path.realpath(hipcc)))] if hipcc else []
    roots += [os.environ.get("ROCM_PATH", ""), "/opt/rocm"]
    for root in roots:
        for rel in ("llvm/bin/clang++", "lib/llvm/bin/clang++"):
            cxx = os.path.join(root, rel)
            if root and os.path.isfile(cxx) and os.access(cxx, os.X_OK):
                return cxx, os.path.join(root, "include")
    return None


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    """The harness's JSON lines: {"selftests": {name: line}, "scenarios": {name: line}, "summary": line}."""
    found = rocm_clang()
    if found is None:
        pytest.skip("no ROCm compiler")
    cxx, rocm_include = found
    out = tmp_path_factory.mktemp("stream_order")
    flags = ["-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all", "-D__HIP_PLATFORM_AMD__", f"-I{rocm_include}",
             f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}", f"-I{NATIVE}"]
    units = [(os.path.join(CSRC, f"{n}.cpp"), str(out / f"{n}.o")) for n in PRODUCT] + \
            [(os.path.join(NATIVE, f"{n}.cpp"), str(out / f"{n}.o")) for n in HARNESS]

    def compile_one(unit):
        return subprocess.run([cxx, *flags, "-c", unit[0], "-o", unit[1]], capture_output=True, text=True, timeout=300)

    with ThreadPoolExecutor(max_workers=min(len(units), os.cpu_count() or 1, 16)) as pool:
        for unit, done in zip(units, pool.map(compile_one, units)):
            assert done.returncode == 0, (unit[0], done.stderr[-3000:])
    exe = str(out / "stream_order_harness")
    link = subprocess.run([cxx, *flags, *[u[1] for u in units], "-o", exe, "-lpthread", "-ldl"], capture_output=True,
                          text=True, timeout=300)
    assert link.returncode == 0, link.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("DCCL_")}
    t0 = time.perf_counter()
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    seconds = time.perf_counter() - t0
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-3000:])
    lines = [json.loads(line) for line in run.stdout.splitlines()]
    rep = {"selftests": {x["selftest"]: x for x in lines if "selftest" in x},
           "scenarios": {x["scenario"]: x for x in lines if "scenario" in x},
           "summary": [x for x in lines if "summary" in x][0]}
    print(f"stream_order_harness: {len(rep['scenarios'])} scenarios in {seconds:.1f} s")
    assert len(rep["scenarios"]) == rep["summary"]["scenarios"] == sum("scenario" in x for x in lines)
    return rep


def test_checker_on_hand_written_traces(report):
    """(a) of the self-check: the exact reports (trace indices) for a ring step with and without the acknowledgement
    wait, a two-stream scratch reuse with and without an event, a wait that precedes its record in host order (a
    no-op under HIP's rule: the hazard stays and the wait is reported unbound), the cycle such waits would close
    under late binding, and a host synchronisation that covers one of two writes."""
    st = report["selftests"]

    def got(name):
        x = st[name]
        return x["hazards"], x["unbound_waits"], x["cycles"], x["load_bearing"]

    assert got("ring_step") == ([], [], [], [2, 5])  # both the wait on `ready` and the acknowledgement carry weight
    assert got("ring_step_without_ack") == ([[3, 5]], [], [], [2])  # the peer's read against the clobber
    assert got("scratch_two_streams") == ([], [], [], [3])
    assert got("scratch_two_streams_without_event") == ([[0, 2], [1, 2]], [], [], [])
    assert got("wait_before_record") == ([[1, 3]], [0], [], [])
    assert got("late_binding_cycle") == ([], [0], [[0, 1, 2, 3]], [])
    assert got("host_sync") == ([[2, 3]], [], [], [])
    assert len(st) == 7


def test_no_hazard_in_any_scenario(report):
    """Every scenario: return code 0 on every rank, no unordered conflicting pair, no cycle, no unbound wait, the
    library wrote exactly recvbuff and read user memory only inside the call's buffers."""
    bad = {}
    for name, x in report["scenarios"].items():
        if any(x["rc"]) or x["n_hazards"] or x["cycles"] or x["unbound_waits"] or x["bytes_errors"]:
            bad[name] = (x["rc"], x["n_hazards"], x["hazards"][:2], x["cycles"], x["unbound_waits"], x["bytes_errors"])
    assert not bad, json.dumps(bad, indent=1)[:6000]
    assert report["summary"]["failed"] == 0


def test_scenarios_cover_the_paths(report):
    """The harness ran what the suite relies on it for: each API on each path, the user ops on their staged routes,
    the back-to-back runs, a two-stream pair per library buffer, and the groups."""
    names = set(report["scenarios"])
    assert len(names) >= 400

    def has(*parts):
        return any(all(p in n for p in parts) for n in names)

    for mode in ("single/", "thrice/"):
        for W in (2, 3, 4):
            assert has(mode, "all_reduce/ring/", f"/W{W}/sum/", "/in_place") and \
                has(mode, "all_reduce/ring/", f"/W{W}/sum/", "/out_of_place")
        for W in (4, 5):
            assert has(mode, "all_reduce/rabenseifner/", f"/W{W}/")
        for api, paths in (("all_reduce", ("direct", "ring_scratchpad")),
                           ("reduce_scatter", ("ring", "ring_scratchpad", "direct")),
                           ("reduce", ("ring_gather", "direct")), ("all_gather", ("ring", "direct")),
                           ("broadcast", ("fan_out", "direct"))):
            for path in paths:
                assert has(mode, f"{api}/{path}/W3/"), (mode, api, path)
        for root in (0, 1):
            assert has(mode, "reduce/ring_gather/", f"/root{root}/") and has(mode, "broadcast/fan_out/", f"/root{root}/")
        assert has(mode, "/W9/")
        for W in (1, 3):
            for op in ("premul_host", "premul_dev"):
                assert has(mode, "all_reduce/ring/", f"/W{W}/{op}/") and has(mode, "all_reduce/rabenseifner/", f"/W{W}/{op}/")
            for op in ("wide", "scaled_host", "scaled_dev"):
                for api in ("all_reduce", "reduce_scatter", "reduce"):
                    assert has(mode, f"{api}/wide_staged_ring/", f"/W{W}/{op}/")
                assert has(mode, "all_reduce/wide_staged_rabenseifner/", f"/W{W}/{op}/")
            for op in ("widened_acc0", "widened_acc1"):
                for api in ("reduce_scatter", "reduce"):
                    assert has(mode, f"{api}/wide_staged_ring/", f"/W{W}/{op}/")
        assert has(mode, "/n3093/") and has(mode, "/n24/")
    for buffer in ("dev_work", "dev_scratch", "dev_wide"):
        assert has("two_streams/", buffer)
    for group in ("three_streams", "two_groups_two_streams", "widened_acc1", "mixed_queue/ring/coalesce_on",
                  "mixed_queue/ring/coalesce_off"):
        assert has("group/", group)


def test_named_waits_are_load_bearing(report):
    """(b) of the self-check: each wait of a product trace is ignored alone and the trace analysed again; a wait is
    load-bearing when a hazard appears.  The waits the comments rest the design on must be: the ring's
    acknowledgement waits (xport_wait_send on `done`) against the clobber of an in-place call and, back to back,
    against the next call; the receive's wait on `ready`; dev_pack_done between two groups on two streams; both
    directions of stream_join in the three-stream run; the library-scratch event between two calls on two streams
    (as a class where the peers' own waits cover a single one).  Every W > 1 event-ordered scenario has at least one
    load-bearing wait, so no such trace passes because the checker is blind to it."""
    sc = report["scenarios"]

    def lb(x, cls):
        return x["load_bearing"].get(cls, [0, 0])[0]

    blind = [n for n, x in sc.items() if x["event_ordered"] and x["W"] > 1 and x["load_bearing_total"] == 0]
    assert not blind, blind
    ring = [x for n, x in sc.items() if n.startswith(("single/", "thrice/")) and "/direct/" not in n]
    assert len(ring) > 200
    for x in ring:
        if x["W"] == 1:
            continue
        assert lb(x, "ready") > 0, x["scenario"]
        if x["scenario"].startswith("thrice/"):  # the next call's producer and staging against the peers' reads
            assert lb(x, "done") > 0, x["scenario"]
        if x["scenario"].startswith("single/all_reduce/ring/") and x["scenario"].endswith("/in_place"):
            assert lb(x, "done") > 0, x["scenario"]  # the clobber against the peers' in-place reads
    two = sc["group/two_groups_two_streams/ring"]
    assert lb(two, "pack_done") > 0 and lb(sc["group/two_groups_two_streams/direct"], "pack_done") > 0
    for path in ("ring", "direct"):
        three = sc[f"group/three_streams/{path}"]
        assert lb(three, "join_in") > 0 and lb(three, "join_out") > 0, three["load_bearing"]
    pairs = [x for n, x in sc.items() if n.startswith("two_streams/dev_")]
    assert len(pairs) >= 9
    for x in pairs:
        assert x["hazards_without_class"]["scratch_done"] > 0, x["scenario"]
    for n in ("two_streams/dev_work/reduce_scatter+reduce_scatter/W3", "two_streams/dev_wide/wide_all_reduce+wide_all_reduce/W3",
              "two_streams/dev_wide/widened_acc1+widened_acc0/W3", "two_streams/dev_wide/widened_w1/W1"):
        assert lb(sc[n], "scratch_done") > 0, n


# ------------------------------------------------------------------------------------------------------------- GPU
W = 3
N = W * 1031
ROUNDS = 3
F32, BF16, SUM = 7, 9, 0
POISON32, POISON16 = 3.0e38, 0x7F7F  # a huge finite fp32 / bf16: one poisoned element changes its whole sum


@functools.lru_cache(maxsize=None)
def reference():
    """Inputs and expected results, computed once: per round an fp32 Sum all-reduce, an fp32 Sum reduce-scatter and a
    bf16 widened accumulate = 1 reduce-scatter (the ring simulation with the oracle as the combine; the accumulating
    sum adds each round's result to what recvbuff held, one fp32 add)."""
    from tests.test_group import combine_of, copy
    from tests.test_wide_sum import collective_inputs
    from tests.test_widened_sum import expected_slots, f32_add, prior_recv
    ref = {"in32": [], "in16": [], "all_reduce": [], "reduce_scatter": [], "slots16": [], "prior": [], "widened": []}
    for k in range(2 * ROUNDS):  # the two-stream test uses inputs ROUNDS .. 2 * ROUNDS - 1
        rng = np.random.default_rng([0xDCC1, 77, k])
        xs = [rng.standard_normal(N).astype(np.float32) for _ in range(W)]
        ref["in32"].append(xs)
        ref["all_reduce"].append(ringsim.ring_allreduce([x.copy() for x in xs], combine_of(F32, SUM), copy))
        bufs = ringsim.reduce_scatter_ring([x.copy() for x in xs], combine_of(F32, SUM), *ringsim.rs_maps())
        ref["reduce_scatter"].append([bufs[r][r * 1031:(r + 1) * 1031].copy() for r in range(W)])
        bits = collective_inputs(200 + k, W, BF16, N)
        ref["in16"].append(bits)
        ref["slots16"].append(expected_slots(bits, BF16))
    ref["prior"] = [prior_recv(300, r, N // W) for r in range(W)]
    for r in range(W):  # recvbuff after each round: the previous content plus the round's sum
        acc, rounds = ref["prior"][r], []
        for k in range(ROUNDS):
            acc = f32_add(acc, ref["slots16"][k][r])
            rounds.append(acc)
        ref["widened"].append(rounds)
    ref["f32_add"] = f32_add
    return ref


def _pinned(torch, array):
    return torch.from_numpy(np.ascontiguousarray(array).view(np.uint8).copy()).pin_memory()


def _delay_op_seconds(torch, stream, scratch):
    """One elementwise pass over `scratch` on `stream`, timed on the GPU."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        scratch.mul_(1.0)
        a.record()
        for _ in range(4):
            scratch.mul_(1.0)
        b.record()
    b.synchronize()
    return a.elapsed_time(b) / 4 / 1e3


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring"])
def test_collectives_follow_their_stream(gpu, monkeypatch, algo):
    """Three rounds per rank on a non-default stream with no synchronisation after setup: sendbuff holds poison; a
    delay (elementwise passes over a scratch tensor) goes on the stream; the round's input is copied from pinned
    memory, non-blocking; the collective is called; recvbuff is copied out on the stream; sendbuff is poisoned again
    on the stream.  One stream synchronisation at the end.  Every round of the fp32 Sum all-reduce and of the bf16
    widened accumulate = 1 reduce-scatter equals the ring simulation with the oracle bit for bit: a collective that
    read its input early, wrote its output late, or let a peer read sendbuff after the call would have seen poison
    or the previous round.  Premise, asserted for "ring" (the direct path synchronises the host by design): the stream
    is still busy when each call returns, i.e. the calls really were enqueued behind unfinished work.  The delay is
    sized on the GPU to about ten times the measured call-return time.
    Measured on one MI355X, three thread ranks, "ring": a call returns in 0.25-0.41 ms (the mean of the two warm-up
    calls on each rank), the delay that rank then enqueues lasts 2.8-4.2 ms per round.  ("": 15.9 ms, the first
    direct call of the process included, and 159 ms.)"""
    import torch
    ref = reference()
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    monkeypatch.delenv("DCCL_RS_SCRATCH", raising=False)
    from tests.test_group import run_ranks

    def body(comm, r):
        stream = torch.cuda.Stream()
        st = stream.cuda_stream
        rc, wop = comm.red_op_create_widened_sum(BF16, 1)
        assert rc == 0
        pin32 = [_pinned(torch, ref["in32"][k][r]) for k in range(ROUNDS)]
        pin16 = [_pinned(torch, ref["in16"][k][r]) for k in range(ROUNDS)]
        send32 = torch.full((N,), POISON32, dtype=torch.float32, device="cuda")
        send16 = torch.full((N,), POISON16, dtype=torch.int16, device="cuda")
        recv32 = torch.zeros(N, dtype=torch.float32, device="cuda")
        recvw = torch.from_numpy(ref["prior"][r].copy()).cuda()
        warm = torch.zeros(N // W, dtype=torch.float32, device="cuda")
        out32 = torch.zeros((ROUNDS, N), dtype=torch.float32, device="cuda")
        outw = torch.zeros((ROUNDS, N // W), dtype=torch.float32, device="cuda")
        scratch = torch.ones(1 << 26, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        # setup: one warm-up of each collective (library buffers and events exist afterwards), timed on the host
        t0 = time.perf_counter()
        assert comm.all_reduce(send32.data_ptr(), recv32.data_ptr(), N, F32, SUM, st) == 0
        assert comm.reduce_scatter(send16.data_ptr(), warm.data_ptr(), N // W, BF16, wop, st) == 0
        call_s = (time.perf_counter() - t0) / 2
        stream.synchronize()
        op_s = _delay_op_seconds(torch, stream, scratch)
        passes = max(8, min(4000, math.ceil(10 * call_s / op_s)))
        torch.cuda.synchronize()  # the last synchronisation before the final one
        busy = []
        with torch.cuda.stream(stream):
            for k in range(ROUNDS):
                for _ in range(passes):
                    scratch.mul_(1.0)
                send32.view(torch.uint8).copy_(pin32[k], non_blocking=True)
                send16.view(torch.uint8).copy_(pin16[k], non_blocking=True)
                assert comm.all_reduce(send32.data_ptr(), recv32.data_ptr(), N, F32, SUM, st) == 0
                busy.append(not stream.query())
                assert comm.reduce_scatter(send16.data_ptr(), recvw.data_ptr(), N // W, BF16, wop, st) == 0
                busy.append(not stream.query())
                out32[k].copy_(recv32)
                outw[k].copy_(recvw)
                send32.fill_(POISON32)
                send16.fill_(POISON16)
        stream.synchronize()
        assert comm.red_op_destroy(wop) == 0
        return out32.cpu().numpy(), outw.cpu().numpy(), busy, call_s, passes * op_s

    outs = run_ranks(W, body)
    print("call return, delay (ms) per rank:", [(round(o[3] * 1e3, 3), round(o[4] * 1e3, 3)) for o in outs])
    for r, (got32, gotw, busy, _, _) in enumerate(outs):
        if algo == "ring":
            assert all(busy), (r, busy)
        for k in range(ROUNDS):
            assert got32[k].tobytes() == ref["all_reduce"][k][r].tobytes(), ("all_reduce", algo, r, k)
            assert gotw[k].tobytes() == ref["widened"][r][k].tobytes(), ("widened reduce_scatter", algo, r, k)


def _two_stream_pairs(comm, r, torch, ref, scratchpad):
    """The pairs of the CPU harness's two-stream scenarios, one per library buffer: on stream A a delay and call 1,
    on stream B call 2 at once, no synchronisation in between.  Without an order between the two calls' use of the
    communicator's buffers, call 2 stages its input while call 1 has not yet read its own."""
    import dccl_amd
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    rc, wop = comm.red_op_create_widened_sum(BF16, 1)
    assert rc == 0
    scratch = torch.ones(1 << 26, dtype=torch.float32, device="cuda")
    k1, k2 = ROUNDS, ROUNDS + 1
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).copy()).cuda()  # noqa: E731
    s32 = [dev(ref["in32"][k][r]) for k in (k1, k2)]
    s16 = [dev(ref["in16"][k][r]) for k in (k1, k2)]
    out = {}
    new32 = lambda n: torch.zeros(n, dtype=torch.float32, device="cuda")  # noqa: E731

    def pair(name, call):
        recvs = [new32(N) if name == "all_reduce" else torch.from_numpy(ref["prior"][r].copy()).cuda() for _ in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(a):
            for _ in range(40):
                scratch.mul_(1.0)
        call(0, recvs[0], a)
        call(1, recvs[1], b)
        a.synchronize()
        b.synchronize()
        out[name] = [v.cpu().numpy() for v in recvs]

    if scratchpad:  # dev_scratch: the ring all-reduce with the reference's scratchpad
        pair("all_reduce", lambda i, v, s: _ok(comm.all_reduce(s32[i].data_ptr(), v.data_ptr(), N, F32, SUM, s.cuda_stream)))
    else:
        # dev_work: two fp32 reduce-scatters; dev_wide: two widened accumulate = 1 reduce-scatters
        pair("reduce_scatter",
             lambda i, v, s: _ok(comm.reduce_scatter(s32[i].data_ptr(), v.data_ptr(), N // W, F32, SUM, s.cuda_stream)))
        pair("widened",
             lambda i, v, s: _ok(comm.reduce_scatter(s16[i].data_ptr(), v.data_ptr(), N // W, BF16, wop, s.cuda_stream)))

        def grouped(i, v, s):  # dev_pack: a coalesced group of two reduce-scatters per stream
            with dccl_amd.group():
                for half in (0, 1):
                    _ok(comm.reduce_scatter(s32[(i + half) % 2].data_ptr(), v[half].data_ptr(), N // W, F32, SUM, s.cuda_stream))

        recvs = [[new32(N // W), new32(N // W)] for _ in range(2)]
        torch.cuda.synchronize()
        with torch.cuda.stream(a):
            for _ in range(40):
                scratch.mul_(1.0)
        grouped(0, recvs[0], a)
        grouped(1, recvs[1], b)
        a.synchronize()
        b.synchronize()
        out["grouped"] = [[h.cpu().numpy() for h in v] for v in recvs]
    assert comm.red_op_destroy(wop) == 0
    return out


def _ok(rc):
    assert rc == 0, rc


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["", "ring"])
def test_two_streams_one_communicator(gpu, monkeypatch, algo):
    """Two calls of one communicator on two streams with nothing between them, for each library buffer (dev_work,
    dev_wide, dev_pack, and with "ring" dev_scratch under DCCL_RS_SCRATCH=1); stream A carries a delay first, so call 2
    would overtake call 1 if only the streams ordered them.  Both results are exact.  This test can only fail when
    ordering is broken; it cannot prove ordering: the proof is the happens-before check on the CPU above.  (Against
    a library built without the communicator's scratch event the "ring" case did fail on an MI355X, at the second
    reduce-scatter's result: the hazard the CPU check reports is not only a theoretical one.)"""
    import torch
    ref = reference()
    from tests.test_group import run_ranks
    monkeypatch.setenv("DCCL_ALLREDUCE_ALGORITHM", algo)
    monkeypatch.delenv("DCCL_GROUP_COALESCE", raising=False)
    monkeypatch.delenv("DCCL_GROUP_COALESCE_MAX_BYTES", raising=False)
    k = (ROUNDS, ROUNDS + 1)
    for scratchpad in ((False, True) if algo == "ring" else (False,)):
        if scratchpad:
            monkeypatch.setenv("DCCL_RS_SCRATCH", "1")
        else:
            monkeypatch.delenv("DCCL_RS_SCRATCH", raising=False)
        outs = run_ranks(W, lambda comm, r: _two_stream_pairs(comm, r, torch, ref, scratchpad))
        for r, out in enumerate(outs):
            for i in (0, 1):
                what = (algo, scratchpad, r, i)
                if scratchpad:
                    assert out["all_reduce"][i].tobytes() == ref["all_reduce"][k[i]][r].tobytes(), what
                    continue
                assert out["reduce_scatter"][i].tobytes() == ref["reduce_scatter"][k[i]][r].tobytes(), what
                want = ref["f32_add"](ref["prior"][r], ref["slots16"][k[i]][r])
                assert out["widened"][i].tobytes() == want.tobytes(), what
                for half in (0, 1):
                    assert out["grouped"][i][half].tobytes() == ref["reduce_scatter"][k[(i + half) % 2]][r].tobytes(), what
