// dccl_amd/csrc/dccl_api.cpp — the namespace-dccl API (include/dccl/dccl.hpp) of the MI355X build.
//
// Entry glue mirrors /root/reference/src/core/dccl.cpp:
//   ncclAllReduce      :344-501  host/device decision by pointer attributes, in-place copy,
//                                scratchpad sizing (total/W), ring algorithm
//   ncclReduceScatter  :551-698  full-size copy of sendbuff, ring RS with rank maps
//                                (orank+W-1)%W / (nrank+1)%W, copy slot `rank` out
//   ncclReduce         :745-846  ring RS with the same maps, then gather slots at root
//   ncclAllGather      :849-862  copy into own slot, ring AG
//   ncclSend/Recv      :865-911  one transfer, waited
//   ncclBroadcast/Bcast:701-743  root -> every rank
// ncclGroupStart / ncclGroupEnd (the reference has neither) queue these calls per thread and run them at the
// outermost end; consecutive small reductions are packed and run as one collective (group_plan.hpp).
// Deliberate differences: op/dtype are validated before any buffer is touched
// (ncclAvg -> ncclInvalidUsage even at W = 1; unknown dtype -> ncclInvalidArgument), a null comm
// throws std::runtime_error for every call (the reference's VALIDATE_COMM, dccl.cpp:32-36),
// device paths are stream-ordered (no per-step stream sync), and every API supports device
// buffers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "algorithms.hpp"
#include "bootstrap.hpp"
#include "checked_entry.hpp"
#include "comm.hpp"
#include "direct.hpp"
#include "group_plan.hpp"
#include "rccl_transport.hpp"
#include "dccl/dccl.hpp"
#include "dccl/dccl_comm.h"
#include "dccl/dccl_reduce.h"

using dccl::dcclComm;
using dccl::ncclResult_t;
using namespace dccl_amd;

namespace {

// Process-wide rendezvous: the group currently being formed.
struct Registry {
    std::mutex mu;
    std::condition_variable cv;
    std::shared_ptr<Group> forming;
};
Registry& registry() {
    static Registry r;
    return r;
}

void validate_comm(const dcclComm* c, const char* fn) {
    if (c == nullptr) throw std::runtime_error(std::string(fn) + ": invalid (null) DCCL communicator");
}

bool is_device_ptr(const void* p) {
    if (p == nullptr) return false;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

ncclResult_t check_op_dtype(int dtype, int op) {
    return static_cast<ncclResult_t>(validate(dtype, op));
}

ncclResult_t copy_bytes(void* dst, const void* src, size_t bytes, bool device, hipStream_t st) {
    if (dst == src || bytes == 0) return dccl::ncclSuccess;
    if (device)
        return hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st) == hipSuccess
                   ? dccl::ncclSuccess
                   : dccl::ncclUnhandledCudaError;
    std::memmove(dst, src, bytes);
    return dccl::ncclSuccess;
}

// A user-op handle that is live on `c` becomes (ncclSum, a copy of its form); every other op value keeps today's
// answer (built-in ops with the kBuiltin form, ncclAvg -> ncclInvalidUsage, anything else -> ncclInvalidArgument).
ncclResult_t resolve_op(const dcclComm* c, int dtype, int* op, SumForm* form) {
    const int slot = *op - int(dccl::ncclNumOps);
    if (slot < 0 || slot >= kMaxUserOps || !c->user_ops[slot].live) return check_op_dtype(dtype, *op);
    const UserOp& u = c->user_ops[slot];
    if (u.dtype != dtype) return dccl::ncclInvalidArgument;
    *op = dccl::ncclSum;
    *form = u.form;
    return dccl::ncclSuccess;
}

// The collectives' first step outside the direct paths: dst = src, or dst = src * scalar for a pre-multiplied sum
// (in place when src == dst), after which the algorithm runs with ncclSum.  A wide form never comes here (wide_staged
// takes it first): its scalar is an fp32 that multiplies the finished sum, not an element of `dtype`.
ncclResult_t stage_input(void* dst, const void* src, size_t count, int dtype, const SumForm& form, bool device,
                         hipStream_t st) {
    switch (form.kind) {
    case kBuiltin: return copy_bytes(dst, src, count * size_of_dtype(dtype), device, st);
    case kPremulSum:
        return static_cast<ncclResult_t>(dccl_local_scale(src, dst, dtype, count, form.scalar(), form.residence(), st));
    case kWideSum:
    case kWideScaledSum:
    case kWidenedSum: break;
    }
    return dccl::ncclInternalError;
}

// [a, a + na) and [b, b + nb) share a byte: a widened sum's sendbuff (16-bit elements) against its fp32 recvbuff,
// which have no in-place form.
bool ranges_share_a_byte(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y ? y - x < na : x - y < nb;
}

// A checked widened sum's flag word (comm.hpp SumForm::nonfinite) shares a byte with recvbuff's `count` fp32.
bool flag_in_recv(const SumForm& form, const void* recv, size_t count) {
    const uint32_t* flag = form.nonfinite();
    return flag != nullptr && ranges_share_a_byte(flag, sizeof(uint32_t), recv, count * sizeof(float));
}

ncclResult_t placement(const void* send, const void* recv, bool* device) {
    const bool sd = is_device_ptr(send), rd = is_device_ptr(recv);
    if (send != nullptr && recv != nullptr && sd != rd) return dccl::ncclInvalidArgument;  // dccl.cpp:358-366
    *device = rd || sd;
    return dccl::ncclSuccess;
}

// nullptr selects the fused receive+combine ring step; DCCL_RS_SCRATCH=1 the reference's scratchpad
bool use_scratch() {
    const char* e = std::getenv("DCCL_RS_SCRATCH");
    return e != nullptr && e[0] == '1';
}

ncclResult_t ring_scratch(dcclComm* c, size_t bytes, bool dev, void** out) {
    *out = nullptr;
    if (!use_scratch()) return dccl::ncclSuccess;
    const ncclResult_t rc = ensure_scratch(c, bytes, dev);
    if (rc == dccl::ncclSuccess) *out = dev ? c->dev_scratch : c->host_scratch;
    return rc;
}

void destroy_events(dcclComm* c) {
    for (hipEvent_t& e : c->ready_events)
        if (e) (void)hipEventDestroy(e), e = nullptr;
    for (hipEvent_t& e : c->done_events)
        if (e) (void)hipEventDestroy(e), e = nullptr;
}

// In-process group formation.  Once a rank is counted into the group it always reaches both of the
// group's agreeing barriers, so a failure on any rank (event creation, peer access) comes back as an
// error on every rank instead of a peer blocked forever; a failed group is discarded by all.
ncclResult_t join(dcclComm** out, uint32_t world, int64_t want_rank) {
    if (world == 0) return dccl::ncclInvalidArgument;
    if (want_rank >= int64_t(world)) return dccl::ncclInvalidArgument;
    auto c = std::make_unique<dcclComm>();
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess) {
        (void)hipGetLastError();
        dev = -1;
    }
    c->device = dev;
    std::shared_ptr<Group> g;
    {
        Registry& R = registry();
        std::unique_lock<std::mutex> lk(R.mu);
        if (!R.forming || R.forming->world() != world) R.forming = std::make_shared<Group>(world);
        g = R.forming;
        uint32_t rank;
        if (want_rank >= 0) {
            if (g->taken[want_rank]) return dccl::ncclInvalidUsage;
            rank = static_cast<uint32_t>(want_rank);
        } else {
            rank = 0;
            while (rank < world && g->taken[rank]) ++rank;
        }
        g->taken[rank] = true;
        g->devices[rank] = dev;
        c->rank = rank;
        if (++g->joined == world) R.forming.reset();  // group complete: the next init starts a new one
    }
    c->group = g;
    c->world = world;
    c->event_ring = world > 2 ? world - 1 : 1;
    c->ready_events.assign(size_t(world) * c->event_ring, nullptr);
    c->done_events.assign(size_t(world) * c->event_ring, nullptr);
    c->sent.assign(world, 0);
    c->received.assign(world, 0);
    ncclResult_t rc = dccl::ncclSuccess;
    if (fault_injected("join_events", c->rank)) rc = dccl::ncclUnhandledCudaError;
    if (dev >= 0) {
        for (size_t i = 0; i < c->ready_events.size() && rc == dccl::ncclSuccess; ++i) {
            if (hipEventCreateWithFlags(&c->ready_events[i], hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&c->done_events[i], hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                rc = dccl::ncclUnhandledCudaError;
            }
        }
    }
    // like Derecho's group formation: returns once every member joined (and agrees on success)
    if (!g->barrier(rc == dccl::ncclSuccess)) {
        destroy_events(c.get());
        return rc != dccl::ncclSuccess ? rc : dccl::ncclRemoteError;
    }
    // Ranks on other GPUs: let this device's kernels and copies read their memory over xGMI.
    if (dev >= 0) {
        for (uint32_t p = 0; p < world && rc == dccl::ncclSuccess; ++p) {
            const int pd = g->devices[p];
            if (pd < 0 || pd == dev) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, dev, pd) == hipSuccess && can) {
                const hipError_t e = hipDeviceEnablePeerAccess(pd, 0);
                if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) rc = dccl::ncclUnhandledCudaError;
                (void)hipGetLastError();
            }
        }
    }
    if (!g->barrier(rc == dccl::ncclSuccess)) {
        destroy_events(c.get());
        return rc != dccl::ncclSuccess ? rc : dccl::ncclRemoteError;
    }
    *out = c.release();
    return dccl::ncclSuccess;
}

int rccl_p2p(void* ctx, const void* sendbuf, size_t send_bytes, uint32_t to, void* recvbuf, size_t recv_bytes,
             uint32_t from, void* stream) {
    return rccl_exchange(ctx, sendbuf, send_bytes, to, recvbuf, recv_bytes, from, static_cast<hipStream_t>(stream));
}

// Cross-process communicator on the RCCL transport; the current HIP device is this rank's GPU.
ncclResult_t join_rccl(dcclComm** out, uint32_t world, uint32_t rank, const void* id128) {
    if (world == 0 || rank >= world || id128 == nullptr) return dccl::ncclInvalidArgument;
    auto c = std::make_unique<dcclComm>();
    if (hipGetDevice(&c->device) != hipSuccess) return dccl::ncclUnhandledCudaError;
    c->rank = rank;
    c->world = world;
    const int rc = rccl_comm_init(&c->rccl, world, rank, id128);
    if (rc != 0) return static_cast<ncclResult_t>(rc);
    c->p2p = &rccl_p2p;  // RCCL moves device memory only
    c->p2p_ctx = c->rccl;
    *out = c.release();
    return dccl::ncclSuccess;
}

// A plugged-in point-to-point transport (P2PExchangeFn, comm.hpp): `memory` bit 0 = it moves host
// buffers, bit 1 = device buffers.
ncclResult_t join_p2p(dcclComm** out, uint32_t world, uint32_t rank, P2PExchangeFn fn, void* ctx, int memory) {
    if (world == 0 || rank >= world || fn == nullptr || memory < 1 || memory > 3) return dccl::ncclInvalidArgument;
    auto c = std::make_unique<dcclComm>();
    if (hipGetDevice(&c->device) != hipSuccess) {
        (void)hipGetLastError();
        c->device = -1;
    }
    c->rank = rank;
    c->world = world;
    c->p2p = fn;
    c->p2p_ctx = ctx;
    c->p2p_host = (memory & 1) != 0;
    c->p2p_device = (memory & 2) != 0;
    *out = c.release();
    return dccl::ncclSuccess;
}

// Single-node bootstrap of the RCCL unique id through a rendezvous file (bootstrap.hpp): rank 0
// publishes it stamped with its pid, start time and the world size; the others take it only from a live
// publisher, so a file an earlier job left behind with the same tag is never used.
ncclResult_t bootstrap_unique_id(uint32_t rank, uint32_t world, unsigned char* id) {
    const std::string path = rdv_path("dccl_rccl_uid_");
    if (rank == 0) {
        const int rc = rccl_get_unique_id(id);
        if (rc != 0) return static_cast<ncclResult_t>(rc);
        return rdv_publish(path, world, std::string(reinterpret_cast<const char*>(id), kRcclUniqueIdBytes));
    }
    std::string payload;
    const ncclResult_t rc = rdv_read(path, world, rank, rdv_timeout_s(), &payload);
    if (rc != dccl::ncclSuccess) return rc;
    if (payload.size() != kRcclUniqueIdBytes) return dccl::ncclSystemError;
    std::memcpy(id, payload.data(), kRcclUniqueIdBytes);
    return dccl::ncclSuccess;
}

long env_long(const char* a, const char* b, long dflt) {
    const char* v = std::getenv(a);
    if (!v && b) v = std::getenv(b);
    return v ? std::strtol(v, nullptr, 10) : dflt;
}

// The one read of DCCL_ALLREDUCE_ALGORITHM: every validator keeps the name in its Call, and the call runs by it.
static_assert(parse_algo(DCCL_ALLREDUCE_RING) == AlgoName::kRing &&
              parse_algo(DCCL_ALLREDUCE_RABENSEIFNER) == AlgoName::kRabenseifner, "select.hpp spells the names");
AlgoName algo_name() { return parse_algo(std::getenv(DCCL_ALLREDUCE_ALGORITHM_CONFSTR)); }

Transport transport_of(const dcclComm* c) {
    if (c->ipc != nullptr) return Transport::kIpc;
    if (c->rccl != nullptr) return Transport::kRccl;
    return c->p2p != nullptr ? Transport::kP2p : Transport::kThreads;
}

// Which buffers the communicator's transport can move: the in-process channels both; the IPC transport
// and RCCL device memory only; a plugged-in p2p transport what it declared at init.
bool transport_accepts(const dcclComm* c, bool device) {
    if (c->ipc != nullptr) return device;
    if (c->p2p != nullptr) return device ? c->p2p_device : c->p2p_host;
    return true;
}

}  // namespace

namespace dccl {

ncclResult_t ncclCommInit(ncclComm_t* comm) {
    if (comm == nullptr) return ncclInvalidArgument;
    const char* t = std::getenv("DCCL_TRANSPORT");
    const bool ipc = t != nullptr && std::string(t) == "ipc", rccl = t != nullptr && std::string(t) == "rccl";
    const long w = env_long("DCCL_WORLD_SIZE", (rccl || ipc) ? "WORLD_SIZE" : nullptr, 1);
    if (w <= 0) return ncclInvalidArgument;
    if (rccl || ipc) {  // one process per GPU: rank / world from the launcher's environment
        const long r = env_long("DCCL_RANK", "RANK", 0);
        if (r < 0 || r >= w) return ncclInvalidArgument;
        if (ipc) return dcclCommInitIpc(comm, static_cast<uint32_t>(w), static_cast<uint32_t>(r));
        unsigned char id[kRcclUniqueIdBytes];
        ncclResult_t rc = bootstrap_unique_id(static_cast<uint32_t>(r), static_cast<uint32_t>(w), id);
        if (rc != ncclSuccess) return rc;
        rc = join_rccl(comm, static_cast<uint32_t>(w), static_cast<uint32_t>(r), id);
        // ncclCommInitRank returns on rank 0 once every rank connected, i.e. read the file
        if (r == 0) rdv_remove(rdv_path("dccl_rccl_uid_"));
        return rc;
    }
    return join(comm, static_cast<uint32_t>(w), -1);
}

ncclResult_t dcclGetUniqueId(void* id128) {
    if (id128 == nullptr) return ncclInvalidArgument;
    return static_cast<ncclResult_t>(rccl_get_unique_id(id128));
}

ncclResult_t dcclCommInitRccl(ncclComm_t* comm, uint32_t world_size, uint32_t rank, const void* id128) {
    if (comm == nullptr) return ncclInvalidArgument;
    return join_rccl(comm, world_size, rank, id128);
}

ncclResult_t dcclCommInitIpc(ncclComm_t* comm, uint32_t world_size, uint32_t rank) {
    if (comm == nullptr) return ncclInvalidArgument;
    auto c = std::make_unique<dcclComm>();
    const ncclResult_t rc = ipc_join(c.get(), world_size, rank);
    if (rc != ncclSuccess) {
        if (c->ipc) (void)ipc_leave(c.get());
        return rc;
    }
    *comm = c.release();
    return ncclSuccess;
}

ncclResult_t dcclCommInitRank(ncclComm_t* comm, uint32_t world_size, uint32_t rank) {
    if (comm == nullptr) return ncclInvalidArgument;
    return join(comm, world_size, rank);
}

ncclResult_t ncclCommFinalize(ncclComm_t comm) {
    validate_comm(comm, __func__);
    ncclResult_t rc = ncclSuccess;
    // A C caller without the HIP headers has no other way to wait for the device: tools/c_abi_check.c relies on
    // this synchronisation before it reads what dccl_copy_rows_multi wrote.
    if (comm->device >= 0 && hipDeviceSynchronize() != hipSuccess) rc = ncclUnhandledCudaError;
    if (comm->rccl != nullptr) {
        const int r = rccl_comm_destroy(comm->rccl);
        if (rc == ncclSuccess) rc = static_cast<ncclResult_t>(r);
    } else if (comm->ipc != nullptr) {
        const ncclResult_t r = ipc_leave(comm);
        if (rc == ncclSuccess) rc = r;
    } else if (comm->group != nullptr) {
        comm->group->barrier();  // no peer may still be reading our buffers
    }  // a plugged-in p2p transport belongs to the caller
    destroy_events(comm);
    if (comm->dev_scratch) (void)hipFree(comm->dev_scratch);
    if (comm->dev_work) (void)hipFree(comm->dev_work);
    if (comm->dev_pack) (void)hipFree(comm->dev_pack);
    if (comm->dev_wide) (void)hipFree(comm->dev_wide);
    if (comm->dev_pack_done) (void)hipEventDestroy(comm->dev_pack_done);
    if (comm->dev_scratch_done) (void)hipEventDestroy(comm->dev_scratch_done);
    if (comm->dev_pack_join) (void)hipEventDestroy(comm->dev_pack_join);
    for (void* h : {comm->host_scratch, comm->host_work}) {
        if (h) {
            (void)hipHostUnregister(h);
            std::free(h);
        }
    }
    delete comm;
    return rc;
}

uint32_t dcclGetWorldSize(ncclComm_t comm) {
    validate_comm(comm, __func__);
    return comm->world;
}

uint32_t dcclGetMyRank(ncclComm_t comm) {
    validate_comm(comm, __func__);
    return comm->rank;
}

ncclResult_t dcclRegisterCacheMemory(ncclComm_t comm, void* buffer, size_t size) {
    validate_comm(comm, __func__);
    if (buffer == nullptr || reinterpret_cast<uintptr_t>(buffer) % kCachelineSize || size % kCachelineSize)
        return ncclInvalidArgument;  // dccl.cpp:506-514
    if (is_device_ptr(buffer)) return comm->ipc != nullptr ? ipc_register(buffer, size) : ncclSuccess;
    if (hipHostRegister(buffer, size, hipHostRegisterDefault) != hipSuccess) {
        (void)hipGetLastError();  // already registered / pinned: nothing to do
    }
    return ncclSuccess;
}

ncclResult_t dcclDeregisterCacheMemory(ncclComm_t comm, void* buffer, size_t) {
    validate_comm(comm, __func__);
    if (buffer == nullptr) return ncclInvalidArgument;
    if (is_device_ptr(buffer)) return comm->ipc != nullptr ? ipc_deregister(buffer) : ncclSuccess;
    if (hipHostUnregister(buffer) != hipSuccess) (void)hipGetLastError();
    return ncclSuccess;
}

}  // namespace dccl

namespace {
using namespace dccl;

// One validated collective call: what "validate" leaves for "run", and what a group queues.
struct Call {
    int api = 0;               // group::Api
    dcclComm* comm = nullptr;
    const void* send = nullptr;
    void* recv = nullptr;
    size_t count = 0;          // as the call counts: recvcount for a reduce-scatter, sendcount for an all-gather
    int dtype = 0;
    int user_op = 0;           // the op value as passed (a user-op handle included): the run key
    int op = 0;                // resolved: a built-in op
    SumForm form;              // resolved: which sum, with its scalar by value (comm.hpp)
    int root = 0;
    bool dev = false;
    AlgoName algo = AlgoName::kAuto;  // DCCL_ALLREDUCE_ALGORITHM when the call was validated: the call runs by it
    hipStream_t stream = nullptr;
};

// What the call does when it runs (select.hpp).  By value from the Call alone: a queued call takes at ncclGroupEnd
// the path its count was checked for, whatever the environment says by then.
Path path_of(const Call& c) {
    return select(c.api, transport_of(c.comm), c.comm->world, c.dev, c.form.kind, c.algo);
}

// The buffer checks every validator shares: the two buffers' one placement, a user op on device buffers only (its
// scaling / widening kernels run on the GPU), and a transport that moves such buffers.
ncclResult_t check_buffers(const dcclComm* comm, const void* a, const void* b, const SumForm& form, bool* dev) {
    const ncclResult_t rc = placement(a, b, dev);
    if (rc != ncclSuccess) return rc;
    if (form.kind != kBuiltin && !*dev) return ncclInvalidUsage;
    return transport_accepts(comm, *dev) ? ncclSuccess : ncclInvalidUsage;  // e.g. host buffers on RCCL / IPC
}

// The fields every collective has, by name; the validators write the rest where they learn it (user_op / op / form
// from resolve_op, dev from check_buffers, root).  Their `c` comes in default-constructed, and only a call with
// something to do gets here: a Call whose comm is still null has nothing to run.
void set_call(Call* c, int api, ncclComm_t comm, const void* send, void* recv, size_t count, int dtype,
              AlgoName algo = algo_name()) {
    c->algo = algo;
    c->api = api;
    c->comm = comm;
    c->send = send;
    c->recv = recv;
    c->count = count;
    c->dtype = dtype;
}

// ------------------------------------------------------------------------------------------
// Every collective is "validate" (its checks, in their order, with their return values, unchanged; it leaves a
// Call) and "run" (the collective's body on a Call).  Outside a group a call is validate + run; inside one it is
// validate + queue, and the outermost ncclGroupEnd runs the queue (below).
// ------------------------------------------------------------------------------------------
ncclResult_t ar_validate(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                         ncclRedOp_t user_op, ncclComm_t comm, Call* c) {
    validate_comm(comm, "ncclAllReduce");
    c->user_op = c->op = user_op;
    ncclResult_t rc = resolve_op(comm, datatype, &c->op, &c->form);
    if (rc != ncclSuccess) return rc;
    // no widened all-reduce: its all-gather half would move fp32 whatever the first half does
    if (c->form.widened()) return ncclInvalidUsage;
    if (count == 0) return ncclSuccess;
    if (sendbuff == nullptr || recvbuff == nullptr) return ncclInvalidArgument;
    if ((rc = check_buffers(comm, sendbuff, recvbuff, c->form, &c->dev)) != ncclSuccess) return rc;
    const uint32_t W = comm->world;
    const AlgoName algo = algo_name();  // dccl.cpp:412-413,454
    const bool rab = algo == AlgoName::kRabenseifner;
    if (algo == AlgoName::kUnknown) return ncclInvalidUsage;
    if (rab && comm->ipc != nullptr) return ncclInvalidUsage;
    if (W > 1 && rab && count % slots(Path::kRabenseifner, W))
        return ncclInvalidArgument;  // all_reduce_recursive_halving_and_doubling.cpp:50-54
    if (W > 1 && !rab && (count < W || count % W)) return ncclInvalidArgument;
    set_call(c, group::kAllReduce, comm, sendbuff, recvbuff, count, datatype, algo);
    return ncclSuccess;
}

ncclResult_t wide_staged(const Call& c);  // below: a wide sum outside the direct paths

ncclResult_t ar_run(const Call& c) {
    dcclComm* comm = c.comm;
    const Path path = path_of(c);
    switch (path) {
    case Path::kDirect:
        return direct_all_reduce(comm, c.send, c.recv, c.count, c.dtype, c.op, c.stream, c.form);
    case Path::kHostDirect: return direct_all_reduce_host(comm, c.send, c.recv, c.count, c.dtype, c.op);
    case Path::kWideStaged: return wide_staged(c);
    case Path::kGrouped: return all_reduce_grouped(comm, c.send, c.recv, c.count, c.dtype, c.op, c.stream);
    case Path::kLocal:
    case Path::kRabenseifner:
    case Path::kRing: break;
    }
    ncclResult_t rc = stage_input(c.recv, c.send, c.count, c.dtype, c.form, c.dev, c.stream);  // dccl.cpp:393-408
    if (rc != ncclSuccess || path == Path::kLocal) return rc;
    // scratchpad: half the buffer for Rabenseifner (dccl.cpp:458-466), one slot for the ring
    const bool rab = path == Path::kRabenseifner;
    const size_t total = c.count * size_of_dtype(c.dtype);
    void* scratch = nullptr;
    if ((rc = ring_scratch(comm, rab ? total / 2 : total / comm->world, c.dev, &scratch)) != ncclSuccess) return rc;
    return rab ? all_reduce_rabenseifner(comm, c.recv, scratch, c.count, c.dtype, c.op, c.dev, c.stream)
               : all_reduce_ring(comm, c.recv, scratch, c.count, c.dtype, c.op, c.dev, c.stream);
}

ncclResult_t rs_validate(const void* sendbuff, void* recvbuff, size_t recvcount, ncclDataType_t datatype,
                         ncclRedOp_t user_op, ncclComm_t comm, Call* c) {
    validate_comm(comm, "ncclReduceScatter");
    c->user_op = c->op = user_op;
    ncclResult_t rc = resolve_op(comm, datatype, &c->op, &c->form);
    if (rc != ncclSuccess) return rc;
    if (recvcount == 0) return ncclSuccess;
    if (sendbuff == nullptr || recvbuff == nullptr) return ncclInvalidArgument;
    if (c->form.widened() && ranges_share_a_byte(sendbuff, recvcount * comm->world * size_of_dtype(datatype), recvbuff,
                                                 recvcount * sizeof(float)))
        return ncclInvalidArgument;  // recvbuff holds fp32: no in-place form
    if (flag_in_recv(c->form, recvbuff, recvcount)) return ncclInvalidArgument;
    if ((rc = check_buffers(comm, sendbuff, recvbuff, c->form, &c->dev)) != ncclSuccess) return rc;
    set_call(c, group::kReduceScatter, comm, sendbuff, recvbuff, recvcount, datatype);
    return ncclSuccess;
}

// The ring reduce-scatter of ncclReduceScatter and ncclReduce on `buf` (`count` elements, already staged), with the
// reference's rank maps (dccl.cpp:551-698): slot o ends up reduced on rank o.
ncclResult_t ring_to_own_slot(const Call& c, void* buf, size_t count) {
    const uint32_t W = c.comm->world;
    void* scratch = nullptr;
    const ncclResult_t rc = ring_scratch(c.comm, count / W * size_of_dtype(c.dtype), c.dev, &scratch);
    if (rc != ncclSuccess) return rc;
    return reduce_scatter_ring(c.comm, buf, scratch, count, c.dtype, c.op, c.dev, c.stream,
                               [W](uint32_t o) { return (o + W - 1) % W; }, [W](uint32_t n) { return (n + 1) % W; });
}

ncclResult_t rs_run(const Call& c) {
    dcclComm* comm = c.comm;
    const uint32_t W = comm->world;
    switch (path_of(c)) {
    case Path::kLocal: return stage_input(c.recv, c.send, c.count, c.dtype, c.form, c.dev, c.stream);
    case Path::kDirect:
        return direct_reduce_scatter(comm, c.send, c.recv, c.count, c.dtype, c.op, c.stream, c.form);
    case Path::kHostDirect: return direct_reduce_scatter_host(comm, c.send, c.recv, c.count, c.dtype, c.op);
    case Path::kWideStaged: return wide_staged(c);
    case Path::kGrouped:  // slot r, reduced straight from sendbuff: no work copy
        return reduce_scatter_grouped(comm, c.send, c.recv, c.count * W, c.dtype, c.op, c.stream, 0);
    case Path::kRabenseifner:
    case Path::kRing: break;
    }
    const size_t slot = c.count * size_of_dtype(c.dtype);
    ncclResult_t rc = ensure_work(comm, slot * W, c.dev);
    if (rc != ncclSuccess) return rc;
    void* work = c.dev ? comm->dev_work : comm->host_work;
    rc = stage_input(work, c.send, c.count * W, c.dtype, c.form, c.dev, c.stream);  // dccl.cpp:585-609
    if (rc == ncclSuccess) rc = ring_to_own_slot(c, work, c.count * W);
    if (rc != ncclSuccess) return rc;
    return copy_bytes(c.recv, static_cast<unsigned char*>(work) + size_t(comm->rank) * slot, slot, c.dev, c.stream);
}

ncclResult_t reduce_validate(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                             ncclRedOp_t user_op, int root, ncclComm_t comm, Call* c) {
    validate_comm(comm, "ncclReduce");
    c->user_op = c->op = user_op;
    ncclResult_t rc = resolve_op(comm, datatype, &c->op, &c->form);
    if (rc != ncclSuccess) return rc;
    const uint32_t W = comm->world, r = comm->rank;
    if (root < 0 || uint32_t(root) >= W) return ncclInvalidArgument;
    if (count == 0) return ncclSuccess;
    if (count % W) return ncclInvalidArgument;  // dccl.cpp:762-767
    const bool iamroot = r == uint32_t(root);
    if (sendbuff == nullptr || (iamroot && recvbuff == nullptr)) return ncclInvalidArgument;
    if (c->form.widened() && iamroot &&
        ranges_share_a_byte(sendbuff, count * size_of_dtype(datatype), recvbuff, count * sizeof(float)))
        return ncclInvalidArgument;  // the root's recvbuff holds fp32: no in-place form
    if (iamroot && flag_in_recv(c->form, recvbuff, count)) return ncclInvalidArgument;
    if ((rc = check_buffers(comm, sendbuff, iamroot ? recvbuff : sendbuff, c->form, &c->dev)) != ncclSuccess) return rc;
    set_call(c, group::kReduce, comm, sendbuff, recvbuff, count, datatype);
    c->root = root;
    return ncclSuccess;
}

ncclResult_t reduce_run(const Call& c) {
    dcclComm* comm = c.comm;
    const uint32_t W = comm->world, r = comm->rank, root = uint32_t(c.root);
    const bool iamroot = r == root, dev = c.dev;
    hipStream_t stream = c.stream;
    switch (path_of(c)) {
    case Path::kLocal: return stage_input(c.recv, c.send, c.count, c.dtype, c.form, dev, stream);
    case Path::kDirect:
        return direct_reduce(comm, c.send, c.recv, c.count, c.dtype, c.op, root, stream, c.form);
    case Path::kWideStaged: return wide_staged(c);
    default: break;  // the ring, then the gather
    }
    ncclResult_t rc;
    const size_t total = c.count * size_of_dtype(c.dtype), slot = total / W;
    void* rbuf = c.recv;
    if (!iamroot) {
        if ((rc = ensure_work(comm, total, dev)) != ncclSuccess) return rc;
        rbuf = dev ? comm->dev_work : comm->host_work;
    }
    if ((rc = stage_input(rbuf, c.send, c.count, c.dtype, c.form, dev, stream)) != ncclSuccess) return rc;
    if ((rc = ring_to_own_slot(c, rbuf, c.count)) != ncclSuccess) return rc;
    auto at = [&](uint32_t i) { return static_cast<unsigned char*>(rbuf) + size_t(i) * slot; };
    if (comm->rccl != nullptr && iamroot) {  // gather to the root (dccl.cpp:803-840): one RCCL group
        std::vector<void*> bufs(W);
        for (uint32_t p = 0; p < W; ++p) bufs[p] = at(p);
        return static_cast<ncclResult_t>(rccl_fan(comm->rccl, false, bufs.data(), slot, W, r, stream));
    }
    if (comm->p2p != nullptr) {  // gather to the root (dccl.cpp:803-840), one exchange per peer
        for (uint32_t p = 0; p < W && rc == ncclSuccess; ++p) {
            if (p == root || (!iamroot && p != r)) continue;
            rc = iamroot ? p2p_exchange(comm, nullptr, 0, 0, at(p), slot, p, stream)
                         : p2p_exchange(comm, at(r), slot, root, nullptr, 0, 0, stream);
        }
        return rc;
    }
    if (iamroot) {
        for (uint32_t p = 0; p < W; ++p)
            if (p != r && (rc = xport_recv(comm, p, at(p), slot, dev, stream)) != ncclSuccess) return rc;
        return ncclSuccess;
    }
    if ((rc = xport_send(comm, root, at(r), slot, dev, stream)) != ncclSuccess) return rc;
    return xport_wait_send(comm, root, dev, stream);
}

ncclResult_t ag_validate(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype,
                         ncclComm_t comm, Call* c) {
    validate_comm(comm, "ncclAllGather");
    const size_t esz = size_of_dtype(datatype);
    if (esz == 0) return ncclInvalidArgument;
    if (sendcount == 0) return ncclSuccess;
    if (sendbuff == nullptr || recvbuff == nullptr) return ncclInvalidArgument;
    const ncclResult_t rc = check_buffers(comm, sendbuff, recvbuff, c->form, &c->dev);
    if (rc != ncclSuccess) return rc;
    set_call(c, group::kAllGather, comm, sendbuff, recvbuff, sendcount, datatype);
    return ncclSuccess;
}

ncclResult_t ag_run(const Call& c) {
    dcclComm* comm = c.comm;
    const size_t bytes = c.count * size_of_dtype(c.dtype);
    switch (path_of(c)) {
    case Path::kLocal: return copy_bytes(c.recv, c.send, bytes, c.dev, c.stream);
    case Path::kDirect: return direct_all_gather(comm, c.send, c.recv, c.count, c.dtype, c.stream);
    default: break;  // the ring
    }
    void* slot = static_cast<unsigned char*>(c.recv) + bytes * comm->rank;
    const ncclResult_t rc = copy_bytes(slot, c.send, bytes, c.dev, c.stream);
    if (rc != ncclSuccess) return rc;
    const RankMap id = [](uint32_t x) { return x; };
    return all_gather_ring(comm, c.recv, c.count, c.dtype, c.dev, c.stream, id, id);
}

ncclResult_t bcast_validate(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root,
                            ncclComm_t comm, Call* c) {
    validate_comm(comm, "ncclBroadcast");
    const size_t esz = size_of_dtype(datatype);
    const uint32_t W = comm->world, r = comm->rank;
    if (esz == 0 || root < 0 || uint32_t(root) >= W) return ncclInvalidArgument;
    if (count == 0) return ncclSuccess;
    const ncclResult_t rc = check_buffers(comm, r == uint32_t(root) ? sendbuff : recvbuff, recvbuff, c->form, &c->dev);
    if (rc != ncclSuccess) return rc;
    set_call(c, group::kBroadcast, comm, sendbuff, recvbuff, count, datatype);
    c->root = root;
    return ncclSuccess;
}

ncclResult_t bcast_run(const Call& c) {
    dcclComm* comm = c.comm;
    const uint32_t W = comm->world, r = comm->rank, root = uint32_t(c.root);
    const bool dev = c.dev;
    hipStream_t stream = c.stream;
    const size_t bytes = c.count * size_of_dtype(c.dtype);
    switch (path_of(c)) {
    case Path::kLocal: return copy_bytes(c.recv, c.send, bytes, dev, stream);
    case Path::kDirect: return direct_broadcast(comm, c.send, c.recv, c.count, c.dtype, root, stream);
    default: break;  // the root's fan-out
    }
    ncclResult_t rc = ncclSuccess;
    if (comm->p2p != nullptr) {  // root -> every rank, one exchange per peer (RCCL: one group)
        if (r != root) return p2p_exchange(comm, nullptr, 0, 0, c.recv, bytes, root, stream);
        if (comm->rccl != nullptr) {
            std::vector<void*> bufs(W, const_cast<void*>(c.send));
            rc = static_cast<ncclResult_t>(rccl_fan(comm->rccl, true, bufs.data(), bytes, W, r, stream));
            return rc == ncclSuccess ? copy_bytes(c.recv, c.send, bytes, dev, stream) : rc;
        }
        for (uint32_t p = 0; p < W && rc == ncclSuccess; ++p)
            if (p != r) rc = p2p_exchange(comm, c.send, bytes, p, nullptr, 0, 0, stream);
        return rc == ncclSuccess ? copy_bytes(c.recv, c.send, bytes, dev, stream) : rc;
    }
    if (r == root) {
        for (uint32_t p = 0; p < W; ++p)
            if (p != r && (rc = xport_send(comm, p, c.send, bytes, dev, stream)) != ncclSuccess) return rc;
        if ((rc = copy_bytes(c.recv, c.send, bytes, dev, stream)) != ncclSuccess) return rc;
        for (uint32_t p = 0; p < W; ++p)
            if (p != r && (rc = xport_wait_send(comm, p, dev, stream)) != ncclSuccess) return rc;
        return ncclSuccess;
    }
    return xport_recv(comm, root, c.recv, bytes, dev, stream);
}

ncclResult_t run_plain(const Call& c) {
    switch (c.api) {
    case group::kAllReduce: return ar_run(c);
    case group::kReduceScatter: return rs_run(c);
    case group::kReduce: return reduce_run(c);
    case group::kAllGather: return ag_run(c);
    default: return bcast_run(c);
    }
}

// A widened sum (dcclRedOpCreateWidenedSum) on every path but the direct ones, ncclReduceScatter and
// ncclReduce only: recvbuff holds fp32.  The input is widened into the fp32 staging buffer and the ncclFloat32 /
// ncclSum collective these settings select runs on it, as for a wide sum; nothing is rounded.  Without `accumulate`
// that collective writes recvbuff itself (the root's, for ncclReduce: it is the buffer the fp32 ring then runs in).
// With it the result stays in staging (a reduce-scatter's behind the widened input) and one fp32 Sum combine adds it
// to recvbuff.  W == 1: the conversion alone, or the conversion into staging and the same add.
// A checked sum (SumForm::nonfinite): on the ranks that have output, one read-only pass over the
// fp32 sum this rank received raises the caller's flag, ahead of the accumulate add (the flag reports the
// contributions, as the direct chain's does).
ncclResult_t widened_staged(const Call& c) {
    hipStream_t stream = c.stream;
    dcclComm* comm = c.comm;
    const uint32_t W = comm->world;
    const bool rs = c.api == group::kReduceScatter, acc = c.form.accumulate();
    const size_t in_count = rs ? c.count * W : c.count, out_count = c.count;
    const bool has_out = rs || comm->rank == uint32_t(c.root);
    uint32_t* const flag = c.form.nonfinite();
    if (W == 1 && !acc) {
        const int rc = dccl_local_convert(c.send, c.dtype, c.recv, ncclFloat32, out_count, stream);
        if (rc != DCCL_SUCCESS || flag == nullptr) return static_cast<ncclResult_t>(rc);
        return static_cast<ncclResult_t>(dccl_local_nonfinite_f32(c.recv, out_count, flag, stream));
    }
    ncclResult_t rc = ensure_wide(comm, (in_count + (rs && acc ? out_count : 0)) * sizeof(float));
    if (rc != ncclSuccess) return rc;
    float* wide = static_cast<float*>(comm->dev_wide);
    rc = static_cast<ncclResult_t>(dccl_local_convert(c.send, c.dtype, wide, ncclFloat32, in_count, stream));
    if (rc != ncclSuccess) return rc;
    const float* sum = wide;  // W == 1: the widened input is the sum
    if (W > 1) {
        Call f = c;
        f.send = wide;
        f.recv = acc ? (rs ? wide + in_count : wide) : (has_out ? c.recv : static_cast<void*>(wide));
        f.dtype = ncclFloat32;
        f.op = ncclSum;
        f.form = SumForm{};  // the builtin kind: path_of(f) is the fp32 collective these settings select
        rc = run_plain(f);
        sum = static_cast<const float*>(f.recv);
    }
    if (rc != ncclSuccess || !has_out) return rc;
    if (flag != nullptr) rc = static_cast<ncclResult_t>(dccl_local_nonfinite_f32(sum, out_count, flag, stream));
    if (rc != ncclSuccess || !acc) return rc;
    return static_cast<ncclResult_t>(dccl_local_reduce(sum, c.recv, ncclFloat32, out_count, ncclSum, stream));
}

// A wide sum (dcclRedOpCreateWideSum) on every path but the direct ones: widen the input into the communicator's
// fp32 staging buffer, run the ncclFloat32 / ncclSum collective these settings select on it (ring, Rabenseifner,
// p2p, RCCL ring or grouped), and round its result once into recvbuff (ncclReduce: on the root only).  A
// reduce-scatter's fp32 result lies behind the widened input.  The staging buffer is not dev_work: rs_run and
// reduce_run grow that one underneath.  W == 1: the input's bytes.  A scaled wide sum (kWideScaledSum, one fp32)
// takes the same route with dccl_local_convert_scaled as the narrowing pass, which multiplies as it rounds; the
// fp32 collective in the middle never sees the scalar.  Its W == 1 is that pass from 16 bits to 16 bits.
ncclResult_t wide_staged(const Call& c) {
    hipStream_t stream = c.stream;
    dcclComm* comm = c.comm;
    const uint32_t W = comm->world;
    const bool rs = c.api == group::kReduceScatter;
    const size_t in_count = rs ? c.count * W : c.count, out_count = c.count;
    const bool has_out = c.api != group::kReduce || comm->rank == uint32_t(c.root);
    const SumForm& form = c.form;  // kWideSum, kWideScaledSum or kWidenedSum: what select() sends here
    const bool scaled = form.kind == kWideScaledSum;
    if (form.widened()) return widened_staged(c);
    if (W == 1 && scaled)
        return static_cast<ncclResult_t>(dccl_local_convert_scaled(c.send, c.dtype, c.recv, c.dtype, out_count,
                                                                   form.scalar(), form.residence(), stream));
    if (W == 1) return copy_bytes(c.recv, c.send, out_count * size_of_dtype(c.dtype), true, stream);
    ncclResult_t rc = ensure_wide(comm, (in_count + (rs ? out_count : 0)) * sizeof(float));
    if (rc != ncclSuccess) return rc;
    float* wide = static_cast<float*>(comm->dev_wide);
    rc = static_cast<ncclResult_t>(dccl_local_convert(c.send, c.dtype, wide, ncclFloat32, in_count, stream));
    if (rc != ncclSuccess) return rc;
    Call f = c;
    f.send = wide;
    f.recv = rs ? wide + in_count : wide;
    f.dtype = ncclFloat32;
    f.op = ncclSum;
    f.form = SumForm{};  // the builtin kind: path_of(f) is the fp32 collective these settings select
    rc = run_plain(f);
    if (rc != ncclSuccess || !has_out) return rc;
    if (scaled)
        return static_cast<ncclResult_t>(dccl_local_convert_scaled(f.recv, ncclFloat32, c.recv, c.dtype, out_count,
                                                                   form.scalar(), form.residence(), stream));
    return static_cast<ncclResult_t>(dccl_local_convert(f.recv, ncclFloat32, c.recv, c.dtype, out_count, stream));
}

// ------------------------------------------------------------------------------------------
// Group state (per thread) and execution.
// ------------------------------------------------------------------------------------------
thread_local int tl_depth = 0;
thread_local std::vector<Call> tl_queue;

// groups ended, calls queued, collectives issued, coalesced runs, tensors coalesced, bytes packed
std::atomic<uint64_t> g_group_stats[6];

// DCCL_GROUP_COALESCE=0: no packing; DCCL_GROUP_COALESCE_MAX_BYTES: tensors of that many bytes or more are never
// packed.  Read at every ncclGroupEnd; the same on every rank (the plan depends on them).
size_t coalesce_max_bytes() {
    const char* off = std::getenv("DCCL_GROUP_COALESCE");
    if (off != nullptr && off[0] == '0' && off[1] == '\0') return 0;
    const char* e = std::getenv("DCCL_GROUP_COALESCE_MAX_BYTES");
    if (e != nullptr && *e != '\0') {
        char* end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (*end == '\0') return static_cast<size_t>(v);
    }
    return group::kDefaultMaxBytes;
}

ncclResult_t hip_rc(hipError_t e) {
    if (e == hipSuccess) return ncclSuccess;
    (void)hipGetLastError();
    return ncclUnhandledCudaError;
}

inline void keep_first(ncclResult_t* first, ncclResult_t rc) {
    if (*first == ncclSuccess) *first = rc;
}

// The call stages through dev_work, dev_scratch or dev_wide: buffers of the communicator that the next such call
// writes again, maybe on another stream.  (dev_pack has its own guard, dev_pack_done in run_packed.)
bool uses_library_scratch(const Call& c) {
    if (!c.dev) return false;
    switch (path_of(c)) {
    case Path::kWideStaged:  // dev_wide, and whatever the fp32 collective inside it takes
    case Path::kGrouped: return true;  // dev_scratch
    case Path::kRabenseifner: return use_scratch();
    case Path::kRing:  // ncclReduceScatter and a non-root ncclReduce run in dev_work; the scratchpad is an option
        return c.api == group::kReduceScatter || c.api == group::kReduce || (c.api == group::kAllReduce && use_scratch());
    case Path::kLocal:
    case Path::kDirect:
    case Path::kHostDirect: break;
    }
    return false;
}

// A collective as ncclGroupEnd or a plain call issues it.  Calls of one communicator may come on different streams
// (INTEGRATION.md), and nothing else orders the library's own buffers between two of them: a call that uses them
// waits, before its first write, for the event recorded behind the last call that did, and records it behind itself.
// One stream: the wait is on an event of the same stream, and adds nothing to the order.  The collective runs
// whatever the wait or the record answer: the peers are in it.
ncclResult_t run_call(const Call& c) {
    if (!uses_library_scratch(c)) return run_plain(c);
    dcclComm* comm = c.comm;
    ncclResult_t first = ncclSuccess;
    if (comm->dev_scratch_done != nullptr)
        keep_first(&first, hip_rc(hipStreamWaitEvent(c.stream, comm->dev_scratch_done, 0)));
    else
        keep_first(&first, hip_rc(hipEventCreateWithFlags(&comm->dev_scratch_done, hipEventDisableTiming)));
    keep_first(&first, run_plain(c));
    if (comm->dev_scratch_done != nullptr) keep_first(&first, hip_rc(hipEventRecord(comm->dev_scratch_done, c.stream)));
    return first;
}

// What every public collective does with its validator's answer: nothing more for an error or an empty call; else
// the call runs, or inside a group joins the queue.  Its SumForm holds a host-immediate scalar by value, so nothing
// refers to the op's slot later: the op may be destroyed, and its slot taken again, before the group ends.
ncclResult_t submit(ncclResult_t rc, Call& c, hipStream_t stream) {
    if (rc != ncclSuccess || c.comm == nullptr) return rc;
    c.stream = stream;
    if (tl_depth == 0) return run_call(c);
    tl_queue.push_back(c);
    g_group_stats[1].fetch_add(1, std::memory_order_relaxed);
    return ncclSuccess;
}

// `to` waits for everything enqueued on `from` so far.  One event of the communicator serves every join: a wait
// refers to the record that precedes it, and the communicator's thread issues them one after the other.
ncclResult_t stream_join(dcclComm* comm, hipStream_t from, hipStream_t to) {
    if (comm->dev_pack_join == nullptr) {
        const ncclResult_t rc = hip_rc(hipEventCreateWithFlags(&comm->dev_pack_join, hipEventDisableTiming));
        if (rc != ncclSuccess) return rc;
    }
    const ncclResult_t rc = hip_rc(hipEventRecord(comm->dev_pack_join, from));
    return rc == ncclSuccess ? hip_rc(hipStreamWaitEvent(to, comm->dev_pack_join, 0)) : rc;
}

// One coalesced run (group_plan.hpp): pack -> the ordinary collective on the packed buffer -> unpack, on the
// stream of the run's first call.  The collective always runs, whatever failed before it on this rank: the
// peers are in it.
ncclResult_t run_packed(const Call* calls, const group::Call* plan, size_t n) {
    const Call& c0 = calls[0];
    dcclComm* comm = c0.comm;
    const uint32_t W = comm->world;
    const size_t esz = size_of_dtype(c0.dtype);
    // The slots of the algorithm that runs, asked of the selector; a wide run is cut like the fp32 collective that
    // wide_staged runs inside it.
    Call inner = c0;
    inner.form = SumForm{};
    const Path path = path_of(c0);
    const size_t P = slots(path == Path::kWideStaged ? path_of(inner) : path, W);
    const group::Layout L = group::pack_layout(plan, n, P);
    const bool rs = c0.api == group::kReduceScatter;
    // A widened run (16-bit in, fp32 out) is the widened collective on library-owned buffers: its
    // fp32 result goes to an output region behind the packed input, one slot of it for a reduce-scatter, all P for a
    // reduce.  A plain reduce-scatter has such a region already; a plain reduce runs in place.
    const bool widened = c0.form.widened();
    const size_t out_at = rs || widened ? P * L.S : 0;
    const size_t bytes = P * L.S + (rs ? L.S_out : widened ? P * L.S_out : 0);
    hipStream_t st = c0.stream;
    const size_t had = comm->dev_pack_bytes;
    ncclResult_t rc = ensure_pack(comm, bytes);
    // Known limit: without the buffer there is nothing to run the collective on, so a rank whose allocation fails
    // returns here while its peers enter the collective and wait for it, exactly as a plain ncclReduceScatter or
    // non-root ncclReduce whose ensure_work fails does today ("Known limit").
    if (rc != ncclSuccess) return rc;
    ncclResult_t first = ncclSuccess;
    if (comm->dev_pack_bytes != had)  // new or grown (hipFree drained the device): no pad byte is read uninitialised
        keep_first(&first, hip_rc(hipMemsetAsync(comm->dev_pack, 0, comm->dev_pack_bytes, st)));
    else if (comm->dev_pack_done != nullptr)  // the last run's unpack, maybe on another stream, still reads the buffer
        keep_first(&first, hip_rc(hipStreamWaitEvent(st, comm->dev_pack_done, 0)));
    unsigned char* pack = static_cast<unsigned char*>(comm->dev_pack);
    std::vector<hipStream_t> others;
    for (size_t i = 1; i < n; ++i)
        if (calls[i].stream != st && std::find(others.begin(), others.end(), calls[i].stream) == others.end())
            others.push_back(calls[i].stream);
    for (hipStream_t o : others) keep_first(&first, stream_join(comm, o, st));
    dccl_copy_rows_t segs[group::kMaxRun];
    for (size_t i = 0; i < n; ++i) segs[i] = {calls[i].send, pack + L.off[i], L.slot[i], L.slot[i], L.S};
    keep_first(&first, static_cast<ncclResult_t>(copy_rows_launch(segs, int(n), uint32_t(P), st)));
    // A checked run: the collective tests every element of the packed slots, the pad bytes at their
    // ends included, and those hold whatever an earlier, larger run packed there.  This rank zeroes its own pack's
    // pads (zeros add nothing non-finite); the peers, in the same run, zero theirs.  Unchecked runs never look.
    if (const size_t used = L.off[n - 1] + L.slot[n - 1]; c0.form.nonfinite() != nullptr && used < L.S)
        for (size_t k = 0; k < P; ++k)
            keep_first(&first, hip_rc(hipMemsetAsync(pack + k * L.S + used, 0, L.S - used, st)));
    Call pc = c0;
    pc.send = pack;
    pc.recv = pack + out_at;
    pc.count = rs ? L.S / esz : L.count;
    if (widened) pc.form.bits = 0;  // accumulate cleared: the region receives the accumulator itself, the unpack adds
    const ncclResult_t crc = run_call(pc);  // a ring reduce-scatter or a wide run stages through other buffers
    keep_first(&first, crc);
    g_group_stats[2].fetch_add(1, std::memory_order_relaxed);
    g_group_stats[3].fetch_add(1, std::memory_order_relaxed);
    g_group_stats[4].fetch_add(n, std::memory_order_relaxed);
    size_t packed = 0;
    for (size_t i = 0; i < n; ++i) packed += P * L.slot[i];
    g_group_stats[5].fetch_add(packed, std::memory_order_relaxed);
    if (crc == ncclSuccess && (c0.api != group::kReduce || comm->rank == uint32_t(c0.root))) {
        for (size_t i = 0; i < n; ++i) {
            if (rs) segs[i] = {pack + out_at + L.out_off[i], calls[i].recv, L.out_slot[i], 0, 0};
            else segs[i] = {pack + out_at + L.out_off[i], calls[i].recv, L.out_slot[i], L.S_out, L.out_slot[i]};
        }
        const auto unpack = c0.form.accumulate() ? add_rows_launch : copy_rows_launch;  // recvbuff += or = the result
        keep_first(&first, static_cast<ncclResult_t>(unpack(segs, int(n), rs ? 1u : uint32_t(P), st)));
    }
    for (hipStream_t o : others) keep_first(&first, stream_join(comm, st, o));
    if (comm->dev_pack_done == nullptr)
        keep_first(&first, hip_rc(hipEventCreateWithFlags(&comm->dev_pack_done, hipEventDisableTiming)));
    if (comm->dev_pack_done != nullptr) keep_first(&first, hip_rc(hipEventRecord(comm->dev_pack_done, st)));
    return first;
}

// The outermost ncclGroupEnd: every queued item executes, in issue order, even after an error (a collective
// never leaves a peer waiting); the first error is returned.
ncclResult_t run_queue(const std::vector<Call>& q) {
    std::vector<group::Call> plan(q.size());
    for (size_t i = 0; i < q.size(); ++i) {
        const Call& c = q[i];
        const uint32_t W = c.comm->world;
        plan[i].api = c.api;
        plan[i].comm = c.comm;
        plan[i].esz = size_of_dtype(c.dtype);
        plan[i].count = c.api == group::kReduceScatter ? c.count * W : c.count;
        plan[i].dtype = c.dtype;
        plan[i].op = c.user_op;
        plan[i].root = c.root;
        plan[i].device = c.dev;
        plan[i].world = W;
        if (c.form.widened()) plan[i].out_esz = sizeof(float);  // 16-bit sendbuff, fp32 recvbuff
    }
    ncclResult_t first = ncclSuccess;
    for (const group::Run& r : group::plan_runs(plan.data(), plan.size(), coalesce_max_bytes())) {
        if (r.packed) {
            keep_first(&first, run_packed(&q[r.first], &plan[r.first], r.n));
            continue;
        }
        for (size_t i = r.first; i < r.first + r.n; ++i) {
            keep_first(&first, run_call(q[i]));
            g_group_stats[2].fetch_add(1, std::memory_order_relaxed);
        }
    }
    return first;
}

// The first free slot of the communicator's op table becomes a `kind` op of `datatype`; its scalar (`scalar_bytes`
// of it, none for 0) is read now from the host or kept as a device address.  The public create functions check
// their own arguments first.
ncclResult_t create_user_op(ncclComm_t comm, SumKind kind, int datatype, const void* scalar, int residence,
                            size_t scalar_bytes, ncclRedOp_t* out) {
    for (int slot = 0; slot < kMaxUserOps; ++slot) {
        UserOp& u = comm->user_ops[slot];
        if (u.live) continue;
        u = UserOp{};
        u.live = true;
        u.dtype = datatype;
        u.form.kind = kind;
        if (scalar_bytes != 0 && residence == ncclScalarDevice) u.form.dev_ptr = scalar;
        else if (scalar_bytes != 0) std::memcpy(&u.form.bits, scalar, scalar_bytes);
        *out = static_cast<ncclRedOp_t>(int(ncclNumOps) + slot);
        return ncclSuccess;
    }
    return ncclInvalidUsage;  // kMaxUserOps live ops already
}

}  // namespace

namespace dccl {

ncclResult_t ncclGroupStart() {
    ++tl_depth;
    return ncclSuccess;
}

ncclResult_t ncclGroupEnd() {
    if (tl_depth == 0) return ncclInvalidUsage;
    if (--tl_depth > 0) return ncclSuccess;
    std::vector<Call> q;
    q.swap(tl_queue);  // the queue and the depth are clear whatever happens below
    g_group_stats[0].fetch_add(1, std::memory_order_relaxed);
    return run_queue(q);
}

ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                           ncclRedOp_t user_op, ncclComm_t comm, hipStream_t stream) {
    Call c;
    const ncclResult_t rc = ar_validate(sendbuff, recvbuff, count, datatype, user_op, comm, &c);
    return submit(rc, c, stream);
}

ncclResult_t ncclReduceScatter(const void* sendbuff, void* recvbuff, size_t recvcount, ncclDataType_t datatype,
                               ncclRedOp_t user_op, ncclComm_t comm, hipStream_t stream) {
    Call c;
    const ncclResult_t rc = rs_validate(sendbuff, recvbuff, recvcount, datatype, user_op, comm, &c);
    return submit(rc, c, stream);
}

ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                        ncclRedOp_t user_op, int root, ncclComm_t comm, hipStream_t stream) {
    Call c;
    const ncclResult_t rc = reduce_validate(sendbuff, recvbuff, count, datatype, user_op, root, comm, &c);
    return submit(rc, c, stream);
}

ncclResult_t ncclRedOpCreatePreMulSum(ncclRedOp_t* op, void* scalar, ncclDataType_t datatype,
                                      ncclScalarResidence_t residence, ncclComm_t comm) {
    validate_comm(comm, __func__);
    const size_t esz = size_of_dtype(datatype);
    if (op == nullptr || scalar == nullptr || esz == 0) return ncclInvalidArgument;
    if (residence != ncclScalarDevice && residence != ncclScalarHostImmediate) return ncclInvalidArgument;
    return create_user_op(comm, kPremulSum, datatype, scalar, residence, esz, op);
}

ncclResult_t dcclRedOpCreateWideSum(ncclRedOp_t* op, ncclDataType_t datatype, ncclComm_t comm) {
    validate_comm(comm, __func__);
    if (op == nullptr) return ncclInvalidArgument;
    if (datatype != ncclFloat16 && datatype != ncclBfloat16) return ncclInvalidArgument;
    return create_user_op(comm, kWideSum, datatype, nullptr, ncclScalarHostImmediate, 0, op);
}

ncclResult_t dcclRedOpCreateWideScaledSum(ncclRedOp_t* op, const void* scalar, ncclDataType_t datatype,
                                          ncclScalarResidence_t residence, ncclComm_t comm) {
    validate_comm(comm, __func__);
    if (op == nullptr || scalar == nullptr) return ncclInvalidArgument;
    if (residence != ncclScalarDevice && residence != ncclScalarHostImmediate) return ncclInvalidArgument;
    if (datatype != ncclFloat16 && datatype != ncclBfloat16) return ncclInvalidArgument;
    // always one fp32, whatever the datatype
    return create_user_op(comm, kWideScaledSum, datatype, scalar, residence, sizeof(float), op);
}

ncclResult_t dcclRedOpCreateWidenedSum(ncclRedOp_t* op, ncclDataType_t datatype, int accumulate, ncclComm_t comm) {
    validate_comm(comm, __func__);
    if (op == nullptr) return ncclInvalidArgument;
    if (datatype != ncclFloat16 && datatype != ncclBfloat16) return ncclInvalidArgument;
    if (accumulate != 0 && accumulate != 1) return ncclInvalidArgument;
    // no scalar: the form's `bits` carry the flag (comm.hpp SumForm::accumulate)
    const uint64_t flag = uint64_t(accumulate);
    return create_user_op(comm, kWidenedSum, datatype, &flag, ncclScalarHostImmediate, sizeof(flag), op);
}

ncclResult_t dcclRedOpCreateWidenedSumChecked(ncclRedOp_t* op, ncclDataType_t datatype, int accumulate,
                                              uint32_t* nonfinite, ncclComm_t comm) {
    validate_comm(comm, __func__);
    if (op == nullptr) return ncclInvalidArgument;
    if (datatype != ncclFloat16 && datatype != ncclBfloat16) return ncclInvalidArgument;
    if (accumulate != 0 && accumulate != 1) return ncclInvalidArgument;
    if (nonfinite == nullptr || reinterpret_cast<uintptr_t>(nonfinite) % sizeof(uint32_t)) return ncclInvalidArgument;
    if (!checked_entries_linked()) return ncclInternalError;  // a build without wide.hip's checked entry points
    ncclRedOp_t h;
    const uint64_t acc = uint64_t(accumulate);
    const ncclResult_t rc = create_user_op(comm, kWidenedSum, datatype, &acc, ncclScalarHostImmediate, sizeof(acc), &h);
    if (rc != ncclSuccess) return rc;
    comm->user_ops[int(h) - int(ncclNumOps)].form.dev_ptr = nonfinite;  // SumForm::nonfinite()
    *op = h;
    return ncclSuccess;
}

ncclResult_t ncclRedOpDestroy(ncclRedOp_t op, ncclComm_t comm) {
    validate_comm(comm, __func__);
    const int slot = int(op) - int(ncclNumOps);
    if (slot < 0 || slot >= kMaxUserOps || !comm->user_ops[slot].live) return ncclInvalidArgument;
    comm->user_ops[slot] = UserOp{};
    return ncclSuccess;
}

ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype,
                           ncclComm_t comm, hipStream_t stream) {
    Call c;
    const ncclResult_t rc = ag_validate(sendbuff, recvbuff, sendcount, datatype, comm, &c);
    return submit(rc, c, stream);
}

ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root,
                           ncclComm_t comm, hipStream_t stream) {
    Call c;
    const ncclResult_t rc = bcast_validate(sendbuff, recvbuff, count, datatype, root, comm, &c);
    return submit(rc, c, stream);
}

ncclResult_t ncclBcast(void* buff, size_t count, ncclDataType_t datatype, int root, ncclComm_t comm,
                       hipStream_t stream) {
    return ncclBroadcast(buff, buff, count, datatype, root, comm, stream);
}

ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream) {
    validate_comm(comm, __func__);
    if (tl_depth > 0) return ncclInvalidUsage;  // no grouped point-to-point (include/dccl/dccl.hpp)
    const size_t esz = size_of_dtype(datatype);
    if (esz == 0 || peer < 0 || uint32_t(peer) >= comm->world || uint32_t(peer) == comm->rank)
        return ncclInvalidArgument;  // dccl.cpp:869-872
    const bool dev = is_device_ptr(sendbuff);
    if (comm->ipc != nullptr) return ncclInvalidUsage;  // the IPC transport has no point-to-point verbs
    if (!transport_accepts(comm, dev)) return ncclInvalidUsage;
    if (comm->p2p != nullptr) return p2p_exchange(comm, sendbuff, count * esz, uint32_t(peer), nullptr, 0, 0, stream);
    ncclResult_t rc = xport_send(comm, uint32_t(peer), sendbuff, count * esz, dev, stream);
    if (rc != ncclSuccess) return rc;
    return xport_wait_send(comm, uint32_t(peer), dev, stream);
}

ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream) {
    validate_comm(comm, __func__);
    if (tl_depth > 0) return ncclInvalidUsage;  // no grouped point-to-point (include/dccl/dccl.hpp)
    const size_t esz = size_of_dtype(datatype);
    if (esz == 0 || peer < 0 || uint32_t(peer) >= comm->world || uint32_t(peer) == comm->rank)
        return ncclInvalidArgument;  // dccl.cpp:893-896
    const bool dev = is_device_ptr(recvbuff);
    if (comm->ipc != nullptr) return ncclInvalidUsage;
    if (!transport_accepts(comm, dev)) return ncclInvalidUsage;
    if (comm->p2p != nullptr) return p2p_exchange(comm, nullptr, 0, 0, recvbuff, count * esz, uint32_t(peer), stream);
    return xport_recv(comm, uint32_t(peer), recvbuff, count * esz, dev, stream);
}

}  // namespace dccl

// ------------------------------------------------------------------------------------------
// C-ABI of the collectives (include/dccl/dccl_comm.h): plain pointers for FFI callers.
// ------------------------------------------------------------------------------------------
namespace {
template <typename F>
int guarded(F&& f) {
    try {
        return static_cast<int>(f());
    } catch (const std::exception&) {
        return DCCL_INVALID_ARGUMENT;  // null / invalid communicator (VALIDATE_COMM)
    }
}
}  // namespace

extern "C" int dccl_comm_init_rank(void** comm, uint32_t world, uint32_t rank) {
    if (comm == nullptr) return DCCL_INVALID_ARGUMENT;
    return guarded([&] { return dccl::dcclCommInitRank(reinterpret_cast<dccl::ncclComm_t*>(comm), world, rank); });
}

extern "C" int dccl_get_unique_id(void* id128) {
    return guarded([&] { return dccl::dcclGetUniqueId(id128); });
}

extern "C" int dccl_comm_init_rccl(void** comm, uint32_t world, uint32_t rank, const void* id128) {
    if (comm == nullptr) return DCCL_INVALID_ARGUMENT;
    return guarded([&] {
        return dccl::dcclCommInitRccl(reinterpret_cast<dccl::ncclComm_t*>(comm), world, rank, id128);
    });
}

extern "C" int dccl_comm_init_p2p(void** comm, uint32_t world, uint32_t rank, dccl_p2p_exchange_fn exchange,
                                  void* ctx, int memory) {
    if (comm == nullptr) return DCCL_INVALID_ARGUMENT;
    return guarded([&] {
        return join_p2p(reinterpret_cast<dccl::ncclComm_t*>(comm), world, rank, exchange, ctx, memory);
    });
}

extern "C" int dccl_comm_init_ipc(void** comm, uint32_t world, uint32_t rank) {
    if (comm == nullptr) return DCCL_INVALID_ARGUMENT;
    return guarded([&] { return dccl::dcclCommInitIpc(reinterpret_cast<dccl::ncclComm_t*>(comm), world, rank); });
}

extern "C" int dccl_comm_finalize(void* comm) {
    return guarded([&] { return dccl::ncclCommFinalize(static_cast<dccl::ncclComm_t>(comm)); });
}

extern "C" int dccl_all_reduce(const void* send, void* recv, size_t count, int dtype, int op, void* comm,
                               void* stream) {
    return guarded([&] {
        return dccl::ncclAllReduce(send, recv, count, static_cast<dccl::ncclDataType_t>(dtype),
                                   static_cast<dccl::ncclRedOp_t>(op), static_cast<dccl::ncclComm_t>(comm),
                                   static_cast<hipStream_t>(stream));
    });
}

extern "C" int dccl_reduce_scatter(const void* send, void* recv, size_t recvcount, int dtype, int op, void* comm,
                                   void* stream) {
    return guarded([&] {
        return dccl::ncclReduceScatter(send, recv, recvcount, static_cast<dccl::ncclDataType_t>(dtype),
                                       static_cast<dccl::ncclRedOp_t>(op), static_cast<dccl::ncclComm_t>(comm),
                                       static_cast<hipStream_t>(stream));
    });
}

extern "C" int dccl_all_gather(const void* send, void* recv, size_t sendcount, int dtype, void* comm,
                               void* stream) {
    return guarded([&] {
        return dccl::ncclAllGather(send, recv, sendcount, static_cast<dccl::ncclDataType_t>(dtype),
                                   static_cast<dccl::ncclComm_t>(comm), static_cast<hipStream_t>(stream));
    });
}

extern "C" int dccl_reduce(const void* send, void* recv, size_t count, int dtype, int op, int root, void* comm,
                           void* stream) {
    return guarded([&] {
        return dccl::ncclReduce(send, recv, count, static_cast<dccl::ncclDataType_t>(dtype),
                                static_cast<dccl::ncclRedOp_t>(op), root, static_cast<dccl::ncclComm_t>(comm),
                                static_cast<hipStream_t>(stream));
    });
}

extern "C" int dccl_broadcast(const void* send, void* recv, size_t count, int dtype, int root, void* comm,
                              void* stream) {
    return guarded([&] {
        return dccl::ncclBroadcast(send, recv, count, static_cast<dccl::ncclDataType_t>(dtype), root,
                                   static_cast<dccl::ncclComm_t>(comm), static_cast<hipStream_t>(stream));
    });
}

namespace {
// The create functions' handle out-parameter for a C caller: `create` gets a ncclRedOp_t* (null when `op` is), and
// *op is written on success only.
template <typename F>
int create_handle(int* op, F&& create) {
    return guarded([&] {
        dccl::ncclRedOp_t h = dccl::ncclSum;
        const ncclResult_t rc = create(op != nullptr ? &h : nullptr);
        if (rc == dccl::ncclSuccess) *op = int(h);
        return rc;
    });
}
}  // namespace

extern "C" int dccl_red_op_create_premul_sum(int* op, const void* scalar, int dtype, int residence, void* comm) {
    if (residence != 0 && residence != 1) return DCCL_INVALID_ARGUMENT;  // before the cast to the two-value enum
    return create_handle(op, [&](dccl::ncclRedOp_t* h) {
        return dccl::ncclRedOpCreatePreMulSum(h, const_cast<void*>(scalar), static_cast<dccl::ncclDataType_t>(dtype),
                                              static_cast<dccl::ncclScalarResidence_t>(residence),
                                              static_cast<dccl::ncclComm_t>(comm));
    });
}

extern "C" int dccl_red_op_create_wide_sum(int* op, int dtype, void* comm) {
    return create_handle(op, [&](dccl::ncclRedOp_t* h) {
        return dccl::dcclRedOpCreateWideSum(h, static_cast<dccl::ncclDataType_t>(dtype),
                                            static_cast<dccl::ncclComm_t>(comm));
    });
}

extern "C" int dccl_red_op_create_wide_scaled_sum(int* op, const void* scalar, int dtype, int residence, void* comm) {
    if (residence != 0 && residence != 1) return DCCL_INVALID_ARGUMENT;  // before the cast to the two-value enum
    return create_handle(op, [&](dccl::ncclRedOp_t* h) {
        return dccl::dcclRedOpCreateWideScaledSum(h, scalar, static_cast<dccl::ncclDataType_t>(dtype),
                                                  static_cast<dccl::ncclScalarResidence_t>(residence),
                                                  static_cast<dccl::ncclComm_t>(comm));
    });
}

extern "C" int dccl_red_op_create_widened_sum(int* op, int dtype, int accumulate, void* comm) {
    return create_handle(op, [&](dccl::ncclRedOp_t* h) {
        return dccl::dcclRedOpCreateWidenedSum(h, static_cast<dccl::ncclDataType_t>(dtype), accumulate,
                                               static_cast<dccl::ncclComm_t>(comm));
    });
}

extern "C" int dccl_red_op_create_widened_sum_checked(int* op, int dtype, int accumulate, void* flag, void* comm) {
    return create_handle(op, [&](dccl::ncclRedOp_t* h) {
        return dccl::dcclRedOpCreateWidenedSumChecked(h, static_cast<dccl::ncclDataType_t>(dtype), accumulate,
                                                      static_cast<uint32_t*>(flag),
                                                      static_cast<dccl::ncclComm_t>(comm));
    });
}

extern "C" int dccl_red_op_destroy(int op, void* comm) {
    return guarded([&] {
        return dccl::ncclRedOpDestroy(static_cast<dccl::ncclRedOp_t>(op), static_cast<dccl::ncclComm_t>(comm));
    });
}

extern "C" int dccl_rccl_available(void) { return rccl_available(); }

extern "C" int dccl_comm_register(void* comm, void* buffer, size_t size) {
    return guarded([&] { return dccl::dcclRegisterCacheMemory(static_cast<dccl::ncclComm_t>(comm), buffer, size); });
}

extern "C" int dccl_comm_deregister(void* comm, void* buffer) {
    return guarded([&] { return dccl::dcclDeregisterCacheMemory(static_cast<dccl::ncclComm_t>(comm), buffer, 0); });
}

extern "C" int dccl_ipc_stats(uint64_t* out, int n) {
    if (out == nullptr && n > 0) return -1;
    return ipc_stats(out, n);
}

extern "C" int dccl_group_start(void) {
    return guarded([&] { return dccl::ncclGroupStart(); });
}

extern "C" int dccl_group_end(void) {
    return guarded([&] { return dccl::ncclGroupEnd(); });
}

extern "C" int dccl_group_stats(uint64_t* out, int n) {
    if (out == nullptr && n > 0) return -1;
    const int count = int(sizeof(g_group_stats) / sizeof(g_group_stats[0]));
    for (int i = 0; i < n && i < count; ++i) out[i] = g_group_stats[i].load(std::memory_order_relaxed);
    return count;
}

extern "C" int dccl_bootstrap_unique_id(uint32_t rank, uint32_t world, void* id128) {
    if (id128 == nullptr || world == 0 || rank >= world) return DCCL_INVALID_ARGUMENT;
    return guarded([&] { return bootstrap_unique_id(rank, world, static_cast<unsigned char*>(id128)); });
}

extern "C" int dccl_bootstrap_done(uint32_t rank, uint32_t world) {
    if (world == 0 || rank >= world) return DCCL_INVALID_ARGUMENT;
    if (rank == 0) rdv_remove(rdv_path("dccl_rccl_uid_"));  // as ncclCommInit does once the group formed
    return DCCL_SUCCESS;
}
