// include/dccl/dccl.hpp — NCCL-compatible DCCL surface of the MI355X build.
//
// Source-compatible with the reference's public header (/root/reference/include/dccl/dccl.hpp):
// same namespace (dccl), C++ linkage, same enum names and values (results 0-8, dtypes 0-9,
// ops 0-5; :59-112) and the same function names and argument meaning.  Differences, all
// deliberate and documented in INTEGRATION.md:
//   * the stream parameter is a hipStream_t (the reference's is cudaStream_t, :11-22);
//     nullptr still means "host buffers" (:188-201);
//   * ncclBfloat16 = 9 is always present (the reference gates it on CUDA bf16, :81-86);
//   * ncclCommInit joins an in-process group (one communicator per thread, rank = join
//     order, world size from DCCL_WORLD_SIZE) instead of a Derecho subgroup; the transport
//     between ranks is host memcpy / device-to-device (xGMI peer) copies, stream-ordered.
//     dcclCommInitRank() picks the rank explicitly.
// The element-wise combine behind ncclAllReduce / ncclReduceScatter is the gfx950 HIP kernel
// of include/dccl/dccl_reduce.h.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <cstdint>

/** Option key (environment variable here, derecho.cfg in the reference, dccl.hpp:38). */
#define DCCL_ALLREDUCE_ALGORITHM_CONFSTR "DCCL_ALLREDUCE_ALGORITHM"
#define DCCL_ALLREDUCE_RING "ring"
#define DCCL_ALLREDUCE_RABENSEIFNER "rabenseifner"

namespace dccl {

typedef enum {
    ncclSuccess = 0,
    ncclUnhandledCudaError = 1,  // a HIP runtime failure on this build
    ncclSystemError = 2,
    ncclInternalError = 3,
    ncclInvalidArgument = 4,
    ncclInvalidUsage = 5,
    ncclRemoteError = 6,
    ncclInProgress = 7,
    ncclNumResults = 8
} ncclResult_t;

typedef enum {
    ncclInt8 = 0, ncclChar = 0,
    ncclUint8 = 1,
    ncclInt32 = 2, ncclInt = 2,
    ncclUint32 = 3,
    ncclInt64 = 4,
    ncclUint64 = 5,
    ncclFloat16 = 6, ncclHalf = 6,
    ncclFloat32 = 7, ncclFloat = 7,
    ncclFloat64 = 8, ncclDouble = 8,
    ncclBfloat16 = 9,
    ncclNumTypes = 10
} ncclDataType_t;

typedef enum { ncclNumOps_dummy = 5 } ncclRedOp_dummy_t;

typedef enum {
    ncclSum = 0,
    ncclProd = 1,
    ncclMax = 2,
    ncclMin = 3,
    ncclAvg = 4,
    ncclNumOps = 5,
    ncclMaxRedOp = 0x7fffffff >> (32 - 8 * sizeof(ncclRedOp_dummy_t))
} ncclRedOp_t;

struct dcclComm;
typedef struct dcclComm* ncclComm_t;

/** Join the process's DCCL group; blocks until DCCL_WORLD_SIZE (default 1) ranks joined. */
ncclResult_t ncclCommInit(ncclComm_t* comm);
/** MI355X-build extension: join the process's group at an explicit rank. */
ncclResult_t dcclCommInitRank(ncclComm_t* comm, uint32_t world_size, uint32_t rank);
/** MI355X-build extension: cross-process communicator on the RCCL (xGMI) transport, one process
 *  per GPU (the current HIP device).  `unique_id` is 128 bytes from dcclGetUniqueId on one rank.
 *  ncclCommInit selects this transport itself when DCCL_TRANSPORT=rccl (rank/world from
 *  RANK/WORLD_SIZE, id exchanged through a file in DCCL_BOOTSTRAP_DIR). Device buffers only. */
ncclResult_t dcclGetUniqueId(void* unique_id);
ncclResult_t dcclCommInitRccl(ncclComm_t* comm, uint32_t world_size, uint32_t rank, const void* unique_id);
/** MI355X-build extension: cross-process communicator on the IPC peer-read transport, one process
 *  per GPU of one node (the current HIP device).  Collectives read peers' buffers directly over
 *  xGMI.  ncclCommInit selects it when DCCL_TRANSPORT=ipc (rank/world from
 *  RANK/WORLD_SIZE, rendezvous through DCCL_BOOTSTRAP_DIR).  Device buffers only, world <= 8
 *  for the collectives, no ncclSend/ncclRecv. */
ncclResult_t dcclCommInitIpc(ncclComm_t* comm, uint32_t world_size, uint32_t rank);
ncclResult_t ncclCommFinalize(ncclComm_t comm);

/** Page-lock host memory for direct DMA.  Device memory: validated (on an IPC communicator: a device
 *  allocation of this process, the range inside it) and tracked; peers read every input through the
 *  communicator's scratch, never user memory. */
ncclResult_t dcclRegisterCacheMemory(ncclComm_t comm, void* buffer, size_t size);
ncclResult_t dcclDeregisterCacheMemory(ncclComm_t comm, void* buffer, size_t size = 0UL);

/** Pre-multiplied sum (NCCL 2.11): `*op` becomes a handle (ncclNumOps + slot, up to 16 live per communicator)
 *  that ncclAllReduce / ncclReduceScatter / ncclReduce accept on `comm` with `datatype` and device buffers:
 *  every rank's input is multiplied by `scalar` (one element of `datatype`; with 16-bit floats the product is
 *  rounded to 16 bits) and the products are summed, bit-identical to ncclProd against the scalar followed by the
 *  ncclSum collective.  ncclScalarDevice: `scalar` is device memory, read by each collective's kernels when
 *  they run; ncclScalarHostImmediate: host memory, read before this call returns.  Every rank must pass the
 *  same value (differing scalars are undefined behaviour).  Host buffers: ncclInvalidUsage; ncclAvg stays
 *  ncclInvalidUsage too. */
typedef enum { ncclScalarDevice = 0, ncclScalarHostImmediate = 1 } ncclScalarResidence_t;
ncclResult_t ncclRedOpCreatePreMulSum(ncclRedOp_t* op, void* scalar, ncclDataType_t datatype,
                                      ncclScalarResidence_t residence, ncclComm_t comm);
ncclResult_t ncclRedOpDestroy(ncclRedOp_t op, ncclComm_t comm);

/** Wide sum (no NCCL counterpart as an op; NCCL's peer-memory kernels accumulate this way): `*op` becomes a handle
 *  from the same table as the pre-multiplied sums (ncclNumOps + slot, 16 live ops per communicator together;
 *  ncclRedOpDestroy releases it) that ncclAllReduce / ncclReduceScatter / ncclReduce accept on `comm` with
 *  `datatype` (ncclFloat16 or ncclBfloat16 only) and device buffers.  Every element's W contributions are widened
 *  to fp32, added in fp32 in the order the algorithm combines them, and rounded to 16 bits ONCE; the results are
 *  the bits of widening every rank's input to fp32, running the ncclFloat32 / ncclSum collective this communicator
 *  and these settings would run, and rounding its result to nearest-even.  ncclSum on these datatypes is
 *  unchanged (it rounds after every combine step).  The direct collectives move the 16-bit bytes they move for
 *  ncclSum; every other path stages through an fp32 buffer of the communicator.  NULL `op` or
 *  another datatype: ncclInvalidArgument; a 17th live op: ncclInvalidUsage; host buffers: ncclInvalidUsage.
 *  A wide sum cannot be combined with a pre-multiplied scalar (one applied to every contribution); for a scalar
 *  applied to the finished sum see dcclRedOpCreateWideScaledSum. */
ncclResult_t dcclRedOpCreateWideSum(ncclRedOp_t* op, ncclDataType_t datatype, ncclComm_t comm);

/** Scaled wide sum: the wide sum above whose finished fp32 accumulator is multiplied by `scalar` before the one
 *  rounding: result = round16(fp32_mul(fp32 sum of the widened contributions, s)), e.g. s = 1.0f / W for the mean
 *  of 16-bit gradients.  `scalar` is ALWAYS one fp32, whatever `datatype` (ncclFloat16 or ncclBfloat16 only), so
 *  1/3 is the fp32 1/3.  ncclScalarDevice: a device float, read by each collective's kernels when they run;
 *  ncclScalarHostImmediate: host memory, read before this call returns.  Every rank must pass the same value.
 *  The results are the bits of running the ncclFloat32 / ncclSum collective of the wide sum, multiplying its result
 *  by s in fp32 and rounding to nearest-even; with s = 1.0f they are the wide sum's.  W = 1 gives
 *  round16(widen(x) * s), not a byte copy.  The handle comes from the same table (ncclNumOps + slot, 16 live ops
 *  per communicator together; ncclRedOpDestroy releases it).  The direct collectives fuse the multiply into their
 *  chain launch, every other path into the narrowing pass it already runs: no extra pass over memory.  NULL `op`
 *  or `scalar`, a bad residence or another datatype: ncclInvalidArgument; a 17th live op: ncclInvalidUsage; host
 *  buffers: ncclInvalidUsage; another datatype at the collective: ncclInvalidArgument. */
ncclResult_t dcclRedOpCreateWideScaledSum(ncclRedOp_t* op, const void* scalar, ncclDataType_t datatype,
                                          ncclScalarResidence_t residence, ncclComm_t comm);

/** Widened sum: the wide sum's fp32 accumulator is not rounded but delivered as fp32, for the caller that keeps an
 *  fp32 gradient shard: main_grad32[i] (+)= sum over ranks of widen(grad16_r[i]).  ncclReduceScatter and ncclReduce
 *  accept the handle on `comm` with `datatype` (ncclFloat16 or ncclBfloat16 only) and device buffers: `sendbuff`
 *  holds `datatype` elements, `recvbuff` holds FP32 elements (`recvcount` / `count` of them; ncclReduce: on the root
 *  only).  The result is the bits of widening every rank's input to fp32, running the ncclFloat32 / ncclSum
 *  collective this communicator and these settings would run and, with `accumulate` == 1, adding that result to the
 *  previous content of `recvbuff` with one fp32 add (`accumulate` == 0: it replaces the content).  The handle comes
 *  from the same table as the other user ops (ncclNumOps + slot, 16 live ops per communicator together;
 *  ncclRedOpDestroy releases it).  The direct collectives fuse everything into their one chain launch and read
 *  16-bit bytes from the peers; every other path stages through an fp32 buffer of the communicator.  Inside
 *  ncclGroupStart / ncclGroupEnd consecutive calls with the SAME handle are coalesced like other reductions (below;
 *  the limit is on the 16-bit payload), with the separate calls' bits; calls with different handles, or a widened
 *  and a plain or wide call, never share a run.  NULL `op`, another datatype
 *  or an `accumulate` other than 0 / 1: ncclInvalidArgument; a 17th live op: ncclInvalidUsage.  At the collective:
 *  ncclAllReduce with the handle: ncclInvalidUsage (there is no widened all-reduce); another datatype:
 *  ncclInvalidArgument; host buffers: ncclInvalidUsage; `sendbuff` and `recvbuff` sharing any byte:
 *  ncclInvalidArgument (the element sizes differ: no in-place form).  There is no scalar: an fp32 consumer applies
 *  1/W itself. */
ncclResult_t dcclRedOpCreateWidenedSum(ncclRedOp_t* op, ncclDataType_t datatype, int accumulate, ncclComm_t comm);

/** Checked widened sum: the widened sum above, whose reduction also answers "did any reduced gradient come out inf or
 *  NaN?" (the question a loss scaler asks before the optimizer step) without a second pass over the fp32 shard.
 *  `nonfinite` is one uint32_t in device memory of the calling rank's device, on a 4-byte boundary.  The library
 *  stores the value 1 to it when at least one element of the fp32 Sum collective's result DELIVERED TO THIS RANK is
 *  not finite (fp32 exponent field all ones: +inf, -inf or any NaN), and stores nothing otherwise.  It never reads
 *  the word, never clears it and never stores another value: the caller zeroes it, and it stays raised over as many
 *  calls (and ops, and streams) as the caller likes.  The store is ordered on the collective's stream like
 *  `recvbuff`'s.  ncclReduceScatter: each rank's flag covers its own shard (all-reduce the flags for a global
 *  answer).  ncclReduce: only the root's flag can be raised; the other ranks' flags are never written.
 *  The flag reports the contributions, not the caller's running buffer: with `accumulate` == 1 the previous content
 *  of `recvbuff` does not enter the test (a `recvbuff` that already holds inf leaves the flag alone when the
 *  contributions are finite), and a finite previous value plus a finite sum that overflows in that last add does
 *  NOT raise it.  The reduced values are exactly the unchecked widened sum's bits, on every path.  Every rank of the
 *  communicator creates the op as a checked one (each with its own flag), as every rank passes the same op to a
 *  collective.  The direct collectives test the accumulators their chain launch already holds; every other path
 *  reads this rank's fp32 result once more before it is delivered; coalesced groups (same handle) keep coalescing
 *  and additionally clear the pad bytes of their packed slots.  Errors: dcclRedOpCreateWidenedSum's, and a NULL or
 *  misaligned `nonfinite`: ncclInvalidArgument.  At the collective: the widened sum's, and the flag's 4 bytes sharing
 *  a byte with `recvbuff`'s fp32 range (on a rank that has output): ncclInvalidArgument.  The flag must not lie
 *  inside `sendbuff` either (not checked).  A coalesced run of same-handle calls takes the flag, like `accumulate`,
 *  from the run's first call: an op destroyed and another created in its slot between two calls of one group makes
 *  them one run with the first call's flag.  There is no checked
 *  all-reduce, and no flag for the wide or scaled wide sums. */
ncclResult_t dcclRedOpCreateWidenedSumChecked(ncclRedOp_t* op, ncclDataType_t datatype, int accumulate,
                                              uint32_t* nonfinite, ncclComm_t comm);

ncclResult_t ncclAllReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                           ncclRedOp_t op, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclReduceScatter(const void* sendbuff, void* recvbuff, size_t recvcount,
                               ncclDataType_t datatype, ncclRedOp_t op, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclBroadcast(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype, int root,
                           ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclBcast(void* buff, size_t count, ncclDataType_t datatype, int root, ncclComm_t comm,
                       hipStream_t stream);
ncclResult_t ncclReduce(const void* sendbuff, void* recvbuff, size_t count, ncclDataType_t datatype,
                        ncclRedOp_t op, int root, ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t datatype,
                           ncclComm_t comm, hipStream_t stream);
ncclResult_t ncclSend(const void* sendbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream);
ncclResult_t ncclRecv(void* recvbuff, size_t count, ncclDataType_t datatype, int peer, ncclComm_t comm,
                      hipStream_t stream);

/** Group calls (NCCL's): between ncclGroupStart and the matching outermost ncclGroupEnd, ncclAllReduce,
 *  ncclReduceScatter, ncclReduce, ncclAllGather, ncclBroadcast and ncclBcast on the calling thread are validated
 *  as always (an invalid call returns its error at once and is not queued), queued, and return ncclSuccess; the
 *  outermost ncclGroupEnd executes the queue in issue order, every item even after an error, and returns the
 *  first error.  Nesting is counted per thread; ncclGroupEnd without a start is ncclInvalidUsage.  Buffers must
 *  stay valid until the outermost ncclGroupEnd returns, and a pre-multiplied-sum op must not be destroyed before it
 *  (its host scalar was read when it was created; the handle is resolved when the call is queued).
 *  Coalescing: consecutive reductions of device buffers with the same api, communicator, datatype, op (and root)
 *  whose payloads are each below DCCL_GROUP_COALESCE_MAX_BYTES are packed, at most 32 at a time, into one
 *  library-owned buffer and run as ONE collective on the stream of the first call (streams of later calls are
 *  joined by events); results are the separate calls' bits.  DCCL_GROUP_COALESCE=0 turns packing
 *  off.  Both variables must have the same value on every rank: the plan must be the same everywhere.
 *  ncclSend / ncclRecv inside a group return ncclInvalidUsage: the in-process transport keeps one outstanding
 *  device message per peer at W <= 2, so a deadlock-free grouped point-to-point needs transport work. */
ncclResult_t ncclGroupStart();
ncclResult_t ncclGroupEnd();

uint32_t dcclGetWorldSize(ncclComm_t comm);
uint32_t dcclGetMyRank(ncclComm_t comm);

/** Host cache line used for the alignment advisories (CACHELINE_SIZE of the reference). */
constexpr size_t kCachelineSize = 64;
/** GPU line size for the device-side alignment advisories. */
constexpr size_t kDeviceCachelineSize = 128;

}  // namespace dccl
