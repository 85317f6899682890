/*
 * include/dccl/dccl_comm.h — C-ABI of the collectives built around the combine, for FFI callers
 * (the C++ surface is include/dccl/dccl.hpp).  Communicators are opaque `void*`; integer enums
 * and results are the ncclDataType_t / ncclRedOp_t / ncclResult_t values.
 *
 *   dccl_comm_init_rank   in-process group: one communicator per thread, blocks until all
 *                         `world` ranks joined (dcclCommInitRank)
 *   dccl_get_unique_id /  cross-process group over the RCCL (xGMI) transport, one process per
 *   dccl_comm_init_rccl   GPU; the 128-byte id travels out of band (dcclCommInitRccl)
 *   dccl_comm_init_p2p    a group over a point-to-point transport the caller plugs in: one exchange
 *                         call sends one buffer to a rank and receives one from a rank (either side may
 *                         be skipped with NULL), complete on return for host buffers and ordered on
 *                         `stream` for device buffers; `memory` = 1 host buffers, 2 device buffers,
 *                         3 both.  This is where the reference's own transport plugs in: Derecho's OOB
 *                         send / recv / wait (/root/reference/src/core/internal_common.hpp:698-792)
 *                         wrapped as one exchange.  The ring collectives
 *                         (reduce_scatter_ring.cpp:73-101, all_gather_ring.cpp:44-64) then run on it,
 *                         with the gfx950 combine after every receive.
 *   dccl_comm_init_ipc    cross-process group over the IPC peer-read transport (one process per GPU
 *                         on one node; rendezvous through DCCL_BOOTSTRAP_DIR, dcclCommInitIpc).  A failed
 *                         collective aborts the group, like an aborted NCCL communicator: every later
 *                         collective returns ncclRemoteError (6) until dccl_comm_finalize, which still
 *                         returns and releases the shared segment and the peers' mappings.  (The
 *                         in-process transport agrees per collective and stays usable after a failure.)
 *                         Inputs are first copied (on the collective's stream) into the communicator's
 *                         scratch, one library-owned allocation exported once, whose token every peer
 *                         checks through its new mapping; peers never read user memory.  A peer whose
 *                         process dies ends every other rank's wait with ncclRemoteError within ~0.1 s; a
 *                         live peer may take any time between collectives (no limit unless
 *                         DCCL_IPC_TIMEOUT_S sets one; 300 s when peers' processes are not visible, e.g.
 *                         another pid namespace, which turns the liveness check off).  Communicators of one
 *                         process share one mapping cache under one mutex: collectives driven from several
 *                         threads at once serialise while they map peer buffers (a failing open retries
 *                         for up to ~0.5 s under it); a collective releases its mappings once its stream
 *                         has drained, before its last barrier.
 *   dccl_comm_register /  dcclRegisterCacheMemory / dcclDeregisterCacheMemory (/root/reference/src/core/
 *   dccl_comm_deregister  dccl.cpp:503-549): 64-byte aligned address and size.  Host memory is page-locked.
 *                         Device memory: validated (an IPC communicator checks it is a device allocation
 *                         of this process and the range lies inside it) and tracked, nothing exported
 *                         (registering a start address again counts; deregister as often).
 *   dccl_ipc_stats        the process's IPC transport counters, in this order: exports made, exports
 *                         retired, (0), scratch copies, scratch bytes copied, scratch grows, (0),
 *                         mappings opened, mappings reused, mappings closed on retirement, retirement-log
 *                         overflows, mappings trimmed, alias evictions, alias errors, open retries, size
 *                         mismatches, mappings open, bytes mapped, exports with recycled handle bytes (never
 *                         published), (0), new scratch mappings whose token did not read back.  The (0)
 *                         slots counted the registered in-place path removed in round 5.  Fills min(n,
 *                         count) values; returns count.
 *   dccl_bootstrap_unique_id  single-node exchange of the RCCL id through DCCL_BOOTSTRAP_DIR: rank 0
 *                         creates and publishes it, the others wait (DCCL_BOOTSTRAP_TIMEOUT_S, default
 *                         120 s) for a file published by a LIVE rank 0 of the same world size, so a
 *                         file an earlier job left behind is never taken (what ncclCommInit does
 *                         with DCCL_TRANSPORT=rccl).  A second call under the same tag waits for a new
 *                         publication: a rank never takes the id it already took, and the file is removed
 *                         as soon as every reader rank took it, so a process started later never takes a
 *                         formed group's id (even without dccl_bootstrap_done)
 *   dccl_bootstrap_done   rank 0 removes the published id once dccl_comm_init_rccl returned (every rank
 *                         has read it then), as ncclCommInit does; other ranks: no-op
 *   dccl_all_reduce       ncclAllReduce       (/root/reference/include/dccl/dccl.hpp:206-207)
 *   dccl_reduce_scatter   ncclReduceScatter   (/root/reference/include/dccl/dccl.hpp:243-244)
 *   dccl_all_gather       ncclAllGather       (/root/reference/include/dccl/dccl.hpp:392-393)
 *   dccl_reduce           ncclReduce          (/root/reference/include/dccl/dccl.hpp:346-347)
 *   dccl_broadcast        ncclBroadcast       (/root/reference/include/dccl/dccl.hpp:289-290)
 *   dccl_red_op_create_premul_sum /  ncclRedOpCreatePreMulSum / ncclRedOpDestroy (NCCL 2.11): a reduction op
 *   dccl_red_op_destroy   that multiplies every rank's input by `scalar` (one element of `dtype`) and sums
 *                         the products, e.g. 1/W for a mean (ncclAvg itself stays ncclInvalidUsage).
 *                         `residence` 0: the scalar lives in device memory and is read by each collective's
 *                         kernels when they run; 1: host memory, read at creation.  The handle (5..20: up to
 *                         16 live ops per communicator, a destroyed slot is reused) is valid in
 *                         dccl_all_reduce / dccl_reduce_scatter / dccl_reduce on that communicator with the
 *                         same dtype and DEVICE buffers; host buffers return ncclInvalidUsage (5) (the
 *                         library never combines on the CPU), another dtype or a handle that is not live
 *                         ncclInvalidArgument (4).  Every rank must pass the SAME scalar value: the direct
 *                         collectives multiply every rank's contribution by the calling rank's scalar, so
 *                         differing values are undefined behaviour, not an error.  Results are bit-identical
 *                         to multiplying each input with op Prod and running the Sum collective.  Create: NULL
 *                         op or scalar, unknown dtype or residence -> 4; a 17th live op -> 5.  Destroy: a
 *                         built-in op (0-4) or a handle that is not live -> 4.
 *   dccl_group_start /    ncclGroupStart / ncclGroupEnd (include/dccl/dccl.hpp): between them, on the calling thread,
 *   dccl_group_end        dccl_all_reduce / dccl_reduce_scatter / dccl_reduce / dccl_all_gather / dccl_broadcast are
 *                         validated as always (an invalid call returns its usual code at once and is not queued),
 *                         then queued, and return 0; the outermost dccl_group_end executes the queue in issue order
 *                         and returns the first error after executing everything.  dccl_group_end without a start
 *                         -> 5.  Buffers stay valid until the outermost end returns.  Consecutive reductions of
 *                         device buffers with the same communicator, dtype, op (and root) and fewer than
 *                         DCCL_GROUP_COALESCE_MAX_BYTES bytes each are packed and run as ONE collective, at most 32
 *                         tensors at a time, with the bits of the separate calls;
 *                         DCCL_GROUP_COALESCE=0 turns the packing off.  Both variables must be the same on every
 *                         rank.  Point-to-point calls inside a group return 5: a deadlock-free grouped send/recv
 *                         needs more than the one outstanding device message per peer the in-process transport has.
 *   dccl_group_stats      process-wide counters, in this order: outermost groups ended, calls queued, collectives
 *                         actually issued by group ends, coalesced runs, tensors coalesced, bytes packed.  Fills
 *                         min(n, count) values; returns count.
 *   dccl_red_op_create_wide_sum  dcclRedOpCreateWideSum: a reduction op for dtype 6 (fp16) or 9 (bf16) that widens
 *                         every contribution to fp32, adds in fp32 in the algorithm's order and rounds to 16 bits
 *                         once (the built-in Sum rounds after every combine step and is unchanged).  Results are
 *                         bit-identical to widening each rank's input, running the fp32 Sum collective of this
 *                         communicator and these settings, and rounding its result to nearest-even.  The handle
 *                         comes from the same table as the pre-multiplied sums (5..20, 16 live ops together) and
 *                         follows their rules: valid in dccl_all_reduce / dccl_reduce_scatter / dccl_reduce on
 *                         that communicator with the same dtype and DEVICE buffers (host buffers 5, another dtype
 *                         or a dead handle 4), released by dccl_red_op_destroy.  Create: NULL op 4; a dtype
 *                         other than 6 / 9 4; a 17th live op 5.  The direct collectives (in-process default,
 *                         IPC) fuse it into their one chain launch and move the 16-bit bytes; ring,
 *                         Rabenseifner, plugged-in p2p and RCCL paths widen into an fp32 buffer of the
 *                         communicator, run the fp32 Sum collective there and narrow into recv.  There is no
 *                         combination with a pre-multiplied scalar (one applied to every contribution).
 *   dccl_red_op_create_wide_scaled_sum  dcclRedOpCreateWideScaledSum: the wide sum whose finished fp32 accumulator
 *                         is multiplied by `scalar` (ONE fp32 whatever the dtype; `residence` as above) before the
 *                         one rounding, e.g. 1.0f / W for a mean.  Same table, handles and rules as the wide sum;
 *                         the same scalar on every rank.  Create: NULL op or scalar, a residence other than 0 / 1
 *                         or a dtype other than 6 / 9 -> 4; a 17th live op -> 5.  The direct collectives fuse the
 *                         multiply into their chain launch, the staged paths into their narrowing pass.
 *   dccl_red_op_create_widened_sum  dcclRedOpCreateWidenedSum: the wide sum's fp32 accumulator delivered as fp32
 *                         instead of rounded.  dccl_reduce_scatter and dccl_reduce only (dccl_all_reduce 5): `send`
 *                         holds dtype 6 / 9 elements, `recv` holds FP32 (recvcount / count of them, on the root only
 *                         for dccl_reduce); accumulate 1 adds the sum to recv's previous content with one fp32 add,
 *                         0 replaces it.  Same table and handles as the other ops.  Create: NULL op, a dtype other
 *                         than 6 / 9 or an accumulate other than 0 / 1 -> 4; a 17th live op -> 5.  At the
 *                         collective: another dtype 4; send and recv sharing any byte 4; host buffers 5.  Inside a
 *                         group consecutive calls with the same handle are coalesced like other reductions (the
 *                         limit is on the 16-bit payload; an accumulate handle's run is unpacked by
 *                         dccl_add_rows_f32_multi); calls with different handles, or a widened and a plain or wide
 *                         call, never share a run.
 *   dccl_red_op_create_widened_sum_checked  dcclRedOpCreateWidenedSumChecked: the widened sum, which also stores 1 to
 *                         `flag` (one uint32_t of device memory on a 4-byte boundary) when an element of the fp32
 *                         sum delivered to this rank is +-inf or a NaN, and nothing otherwise.  The library never
 *                         reads, clears or otherwise writes the word: zero it, and it stays raised over as many
 *                         calls as you like.  dccl_reduce_scatter: each rank's flag covers its shard; dccl_reduce:
 *                         only the root's flag can be raised.  The previous content of recv (accumulate 1) does not
 *                         enter the test, and finite + finite overflowing in that last add does not raise the flag.
 *                         The values are the unchecked op's bits.  Create: dccl_red_op_create_widened_sum's rows,
 *                         and a NULL or misaligned flag -> 4.  At the collective: its rows, and the flag's 4 bytes
 *                         sharing a byte with recv's fp32 range -> 4.  Same-handle calls in a group still coalesce.
 * A null / finalized communicator returns ncclInvalidArgument (4) instead of throwing.
 */
#ifndef DCCL_COMM_H_
#define DCCL_COMM_H_
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* returns 0 on success, else an ncclResult_t value (the collective returns it) */
typedef int (*dccl_p2p_exchange_fn)(void* ctx, const void* sendbuf, size_t send_bytes, uint32_t to, void* recvbuf,
                                    size_t recv_bytes, uint32_t from, void* stream);
int dccl_comm_init_rank(void** comm, uint32_t world, uint32_t rank);
int dccl_get_unique_id(void* unique_id_128);
int dccl_comm_init_rccl(void** comm, uint32_t world, uint32_t rank, const void* unique_id_128);
int dccl_comm_init_ipc(void** comm, uint32_t world, uint32_t rank);
int dccl_comm_init_p2p(void** comm, uint32_t world, uint32_t rank, dccl_p2p_exchange_fn exchange, void* ctx,
                       int memory);
int dccl_bootstrap_unique_id(uint32_t rank, uint32_t world, void* unique_id_128);
int dccl_bootstrap_done(uint32_t rank, uint32_t world);
int dccl_comm_finalize(void* comm);
int dccl_all_reduce(const void* send, void* recv, size_t count, int dtype, int op, void* comm, void* stream);
int dccl_reduce_scatter(const void* send, void* recv, size_t recvcount, int dtype, int op, void* comm,
                        void* stream);
int dccl_all_gather(const void* send, void* recv, size_t sendcount, int dtype, void* comm, void* stream);
int dccl_reduce(const void* send, void* recv, size_t count, int dtype, int op, int root, void* comm,
                void* stream);
int dccl_broadcast(const void* send, void* recv, size_t count, int dtype, int root, void* comm, void* stream);
int dccl_red_op_create_premul_sum(int* op, const void* scalar, int dtype, int residence, void* comm);
int dccl_red_op_destroy(int op, void* comm);
int dccl_red_op_create_wide_sum(int* op, int dtype, void* comm);
int dccl_red_op_create_wide_scaled_sum(int* op, const void* scalar, int dtype, int residence, void* comm);
int dccl_red_op_create_widened_sum(int* op, int dtype, int accumulate, void* comm);
int dccl_red_op_create_widened_sum_checked(int* op, int dtype, int accumulate, void* flag, void* comm);
int dccl_rccl_available(void);
int dccl_comm_register(void* comm, void* buffer, size_t size);
int dccl_comm_deregister(void* comm, void* buffer);
int dccl_ipc_stats(uint64_t* out, int n);
int dccl_group_start(void);
int dccl_group_end(void);
int dccl_group_stats(uint64_t* out, int n);
#ifdef __cplusplus
}
#endif
#endif
