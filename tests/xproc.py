"""One process per rank on one GPU: the scaffolding of the user-op tests that cross process boundaries.

``run_ipc`` / ``run_rccl`` spawn W children, each of which joins a communicator on its transport, calls
``body(comm, r, W, torch)`` and finalizes; they return {rank: (body's result, finalize's return code)}.  ``body`` is a
module-level function of the calling test file: a spawned child imports it by name.
"""
import multiprocessing as mp
import os
import uuid


def _report(r, q, make_comm, body, W):
    try:
        import torch
        import dccl_amd
        torch.cuda.set_device(0)
        comm = make_comm(dccl_amd)
        try:
            out = body(comm, r, W, torch)
        finally:
            fin = comm.finalize()
        q.put((r, (out, fin), None))
    except Exception as e:  # pragma: no cover - reported by the parent
        q.put((r, None, repr(e)))


def _ipc_rank(r, W, tag, body, q):
    os.environ["DCCL_BOOTSTRAP_TAG"] = tag
    os.environ.setdefault("DCCL_IPC_TIMEOUT_S", "60")

    def make_comm(dccl_amd):
        return dccl_amd.Comm.ipc(W, r)

    _report(r, q, make_comm, body, W)


def _rccl_rank(r, W, hostid, conn, algo, body, q):
    os.environ.update({"NCCL_HOSTID": f"{hostid}-{r}", "NCCL_SOCKET_IFNAME": "lo", "NCCL_IB_DISABLE": "1",
                       "DCCL_ALLREDUCE_ALGORITHM": algo})

    def make_comm(dccl_amd):
        if r == 0:
            uid = dccl_amd.Comm.unique_id()
            conn.send(uid)
        else:
            uid = conn.recv()
        return dccl_amd.Comm.rccl(W, r, uid)

    _report(r, q, make_comm, body, W)


def collect(ps, q):
    for p in ps:
        p.start()
    results = {}
    try:
        for _ in range(len(ps)):
            r, res, err = q.get(timeout=240)
            assert err is None, (r, err)
            results[r] = res
    finally:
        for p in ps:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    return results


def run_ipc(W, body):
    """The IPC transport, under a bootstrap tag of this call's own."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    tag = "test_" + uuid.uuid4().hex[:12]
    return collect([ctx.Process(target=_ipc_rank, args=(r, W, tag, body, q)) for r in range(W)], q)


def run_rccl(W, body, algo="ring"):
    """The RCCL transport over loopback sockets; rank 0 hands its unique id to the others through a pipe."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    a, b = ctx.Pipe()
    hostid = "dccl-test-" + uuid.uuid4().hex[:10]
    return collect([ctx.Process(target=_rccl_rank, args=(r, W, hostid, a if r == 0 else b, algo, body, q))
                    for r in range(W)], q)
