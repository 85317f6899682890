/*
 * include/dccl/dccl_reduce.h — the C-ABI drop-in boundary of the DCCL local
 * bucket-reduction combine on MI355X (gfx950).
 *
 * Every entry point is `extern "C"`, takes plain pointers, sizes and integer
 * enum values (numerically identical to dccl::ncclDataType_t / ncclRedOp_t /
 * ncclResult_t of include/dccl/dccl.hpp and of the reference's
 * /root/reference/include/dccl/dccl.hpp:59-112), and never throws.
 *
 * Semantics: recv[i] = op(recv[i], send[i]) for
 * i in [0, count).  Sum/Prod wrap for integers, Max/Min are compare-and-select
 * (`if (r < s) r = s` / `if (r > s) r = s`: NaN or +-0 ties keep recv),
 * fp16/bf16 widen to fp32 and round back to nearest-even.  Avg returns
 * ncclInvalidUsage (5), any other op or an unknown dtype ncclInvalidArgument (4),
 * a HIP failure ncclUnhandledCudaError (1).  count == 0 is a successful no-op.
 *
 * Aliasing (SURVEY.md §8(b) "Ownership"), the same rule at every combine entry point below:
 *   - an operand may BE the destination (send == recv; a k-way source == recv; a chain source or
 *     own == dst): every combine is element-wise, so each output depends only on its own index;
 *   - an operand whose count*sizeof(dtype) bytes PARTIALLY overlap the destination's (shared bytes,
 *     different start) returns ncclInvalidArgument (4) before anything is launched.  The reference's
 *     one-thread ascending loop (/root/reference/src/core/internal_common.hpp:550-560) gives such a call
 *     an order-dependent answer that no parallel kernel reproduces.
 *   Sources may overlap each other freely (they are only read).  dccl_copy_multi: a pair's dst may equal
 *   its own src; no dst may share a byte with another pair's src or dst.
 */
#ifndef DCCL_REDUCE_H_
#define DCCL_REDUCE_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Result codes (ncclResult_t values). */
#define DCCL_SUCCESS 0
#define DCCL_UNHANDLED_DEVICE_ERROR 1
#define DCCL_SYSTEM_ERROR 2
#define DCCL_INTERNAL_ERROR 3
#define DCCL_INVALID_ARGUMENT 4
#define DCCL_INVALID_USAGE 5

/*
 * Device combine, asynchronous and stream-ordered.
 *
 * Replaces the reference's GPU boundary
 *   dccl::do_device_reduce(const void*, void*, ncclDataType_t, size_t,
 *                          ncclRedOp_t, cudaStream_t)
 *   (/root/reference/src/core/internal_common.hpp:613-618, definition
 *    /root/reference/src/core/reduce.cu:40-100)
 * and its template shim do_device_reduce<DT>
 *   (/root/reference/src/core/internal_common.hpp:644-691).
 *
 * `send` and `recv` are device pointers of the device that owns `stream`
 * (a hipStream_t; NULL = that device's null stream).  Returns after the kernel
 * is enqueued; errors of the launch itself are reported, not asynchronous faults.
 */
int dccl_local_reduce(const void* send, void* recv, int dtype, size_t count, int op, void* stream);

/*
 * k-way device combine: recv[i] = op(...op(op(recv[i], sends[0][i]), sends[1][i])..., sends[k-1][i]),
 * applied in that order, one read of recv and one write.  Bit-identical to k
 * successive dccl_local_reduce calls (same association order).  1 <= nsend <= 8.
 * Serves the multi-arrival callers: recursive halving
 *   (/root/reference/src/core/reduce_scatter_recursive_halving.cpp:66-111) and the
 * Rabenseifner fold (/root/reference/src/core/all_reduce_recursive_halving_and_doubling.cpp:72-151).
 */
int dccl_local_reduce_multi(const void* const* sends, int nsend, void* recv, int dtype, size_t count,
                            int op, void* stream);

/*
 * Chain combine: the whole combine sequence of the ring reduce-scatter for one chunk, in one pass:
 *   dst[i] = op(own[i], op(sends[k-1][i], ... op(sends[1][i], sends[0][i])))
 * Each step is op(recv = next rank's data, send = partial so far), exactly as the ring applies it
 * (/root/reference/src/core/reduce_scatter_ring.cpp:73-101: rank c+j combines its own chunk c with
 * the partial received from rank c+j-1), so the result is bit-identical to W-1 ring steps when
 * sends[j] is rank c+j's chunk and `own` is the last rank's.  `own` may equal `dst`.
 * 1 <= nsend <= 8.  Used by the direct (xGMI peer-read) collectives, DESIGN.md §7.3.
 */
int dccl_local_reduce_chain(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                            size_t count, int op, void* stream);

/*
 * Pre-multiplied sum (the device half of ncclRedOpCreatePreMulSum, include/dccl/dccl.hpp): every contribution
 * is multiplied by one scalar s of the operands' dtype, then summed.
 *   dccl_local_scale                 dst[i] = Prod(src[i], s); src == dst scales in place
 *   dccl_local_reduce_chain_premul   dccl_local_reduce_chain with op Sum over Prod(sends[j][i], s) and
 *                                    Prod(own[i], s), in the same order and roles, in one pass
 * Prod and Sum are the element semantics above, each rounded on its own: integers wrap, fp32 / fp64 take one
 * IEEE multiply and then one IEEE add (never a fused multiply-add), fp16 / bf16 products are rounded to
 * 16 bits before they enter the sum.  The results are therefore bit-identical to dccl_local_reduce with
 * op Prod against a buffer filled with s, followed by the Sum combine (NaN payloads unpinned, as everywhere).
 * `scalar` points to one element of `dtype`; `residence` 0: device memory, read by the kernel when it runs
 * (stream-ordered: a captured graph replays with the value the memory holds then); 1: host memory, read
 * before the call returns.  Validation, in this order: unknown dtype 4; nsend outside 1..8 or NULL sends 4;
 * residence not 0 / 1 or NULL scalar 4; count == 0 succeeds; NULL operand 4; an operand partially
 * overlapping dst 4 (src == dst, own == dst and a source == dst are allowed); launch failure 1.
 * Operands that are element-aligned and share dst's 16-byte phase take 16-byte vector kernels; any other
 * placement (operands off element alignment included) takes an element-wise kernel kept for correctness.
 */
int dccl_local_scale(const void* src, void* dst, int dtype, size_t count, const void* scalar, int residence,
                     void* stream);
int dccl_local_reduce_chain_premul(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                   size_t count, const void* scalar, int residence, void* stream);

/*
 * Wide sum (the device half of dcclRedOpCreateWideSum, include/dccl/dccl.hpp): fp16 (6) / bf16 (9) contributions
 * accumulated in fp32 and rounded to 16 bits once, instead of once per combine step.
 *   dccl_local_reduce_chain_wide   dccl_local_reduce_chain's roles, limits (1 <= nsend <= 8) and aliasing rule:
 *                                  acc = widen(sends[0][i]); acc = widen(sends[j][i]) + acc for j = 1..nsend-1;
 *                                  acc = widen(own[i]) + acc; dst[i] = round16(acc).  widen is exact, every add
 *                                  one IEEE fp32 add, round16 the nearest-even rounding of the Sum combine: the
 *                                  bits of widening every operand, running the fp32 Sum chain and rounding
 *                                  once.  With nsend == 1 that equals dccl_local_reduce_chain with op Sum.
 *   dccl_local_convert             dst[i] = widen(src[i]) for (src_dtype, dst_dtype) = (6, 7) or (9, 7),
 *                                  dst[i] = round16(src[i]) for (7, 6) or (7, 9); any other pair 4.
 * NaN payloads are unpinned, as everywhere.  The wide sum has no pre-multiplied form (a scalar applied to every
 * contribution); its scaled form, one multiply of the finished sum, follows below.
 * Validation, in this order: dtype not 6 / 9 (convert: an unsupported pair) 4, unknown dtypes included; nsend
 * outside 1..8 or NULL sends 4; count == 0 succeeds; NULL operand 4; chain: an operand partially overlapping dst
 * 4 (own == dst and a source == dst are allowed); convert: src and dst sharing ANY byte 4 (their element sizes
 * differ, so there is no in-place form); launch failure 1.
 * Chain operands that are element-aligned and share dst's 16-byte phase take a 16-byte vector kernel under
 * the plain chain's caps; the conversion takes its vector kernel (16 B of 16-bit elements against 2 x 16 B of
 * fp32) when the 16-bit side's vectors and the fp32 side line up on 16-byte boundaries.  Any other placement
 * (operands off element alignment included) takes an element-wise kernel kept for correctness.
 */
int dccl_local_reduce_chain_wide(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                 size_t count, void* stream);
int dccl_local_convert(const void* src, int src_dtype, void* dst, int dst_dtype, size_t count, void* stream);

/*
 * Scaled wide sum (the device half of dcclRedOpCreateWideScaledSum, include/dccl/dccl.hpp): the wide sum's finished
 * fp32 accumulator is multiplied by one fp32 scalar s and rounded to 16 bits once, e.g. s = 1/W for a mean.
 *   dccl_local_reduce_chain_wide_scaled   dccl_local_reduce_chain_wide's accumulator, roles, limits and aliasing
 *                                         rule; dst[i] = round16(acc * s): one IEEE fp32 multiply (never fused
 *                                         with an add), then the one nearest-even rounding.  With s = 1.0f the
 *                                         bits of dccl_local_reduce_chain_wide.
 *   dccl_local_convert_scaled             dst[i] = round16(as_fp32(src[i]) * s) for (src_dtype, dst_dtype) =
 *                                         (7, 6), (7, 9), (6, 6) or (9, 9); any other pair 4.  It is the narrowing
 *                                         pass of the staged collectives; the 16 -> 16 pairs are their W = 1 case.
 * `scalar` points to ONE fp32 whatever the operands' dtype; `residence` as for the pre-multiplied sums: 0 device
 * memory, read by the kernel when it runs (stream-ordered); 1 host memory, read before the call returns.
 * fp32 and fp16 denormals are kept; NaN payloads are unpinned.
 * Validation, in this order: dtype not 6 / 9 (convert: an unsupported pair) 4; residence not 0 / 1 or NULL scalar
 * 4; nsend outside 1..8 or NULL sends 4; count == 0 succeeds; NULL operand 4; chain: an operand partially
 * overlapping dst 4 (own == dst and a source == dst are allowed); convert from fp32: src and dst sharing ANY byte
 * 4; convert 16 -> 16: src == dst is allowed (in place), a partial overlap 4; launch failure 1.
 * Placement as for the wide sum: the chain's 16-byte vector kernel for element-aligned operands in dst's 16-byte
 * phase; the conversion's vector kernel when dst's 16-byte vectors and the source line up on 16-byte boundaries;
 * any other placement takes an element-wise kernel kept for correctness.
 */
int dccl_local_reduce_chain_wide_scaled(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                        size_t count, const void* scalar, int residence, void* stream);
int dccl_local_convert_scaled(const void* src, int src_dtype, void* dst, int dst_dtype, size_t count,
                              const void* scalar, int residence, void* stream);

/*
 * Widened sum (the device half of dcclRedOpCreateWidenedSum, include/dccl/dccl.hpp): the wide sum's fp32 accumulator
 * is not rounded at all but stored as fp32, optionally added to what dst holds.
 *   dccl_local_reduce_chain_widen   sends[j] and own hold `count` elements of dtype 6 (fp16) or 9 (bf16), dst holds
 *                                   `count` fp32.  acc is dccl_local_reduce_chain_wide's, unchanged: acc =
 *                                   widen(sends[0][i]); acc = widen(sends[j][i]) + acc for j = 1..nsend-1; acc =
 *                                   widen(own[i]) + acc.  accumulate == 0: dst[i] = acc.  accumulate == 1: dst[i] =
 *                                   dst[i] + acc, one more IEEE fp32 add applied after the chain (never folded into
 *                                   the chain as a first operand, never contracted).
 * fp32 and fp16 denormals are kept; NaN payloads are unpinned.
 * Validation, in this order: dtype not 6 / 9 4, unknown dtypes included; accumulate not 0 / 1 4; nsend outside 1..8
 * or NULL sends 4; count == 0 succeeds; NULL operand 4; a source or own sharing ANY byte with [dst, dst + 4 count)
 * 4 (the element sizes differ, so there is no in-place form: dccl_local_convert's rule); launch failure 1.
 * The 16-byte vector kernel runs when every 16-bit operand is 2-byte aligned, all of them share one 16-byte phase
 * p, dst is 4-byte aligned and dst + 4 h is on a 16-byte boundary, h = ((16 - p) % 16) / 2 being the head elements
 * that bring the 16-bit operands to theirs.  Any other placement takes an element-wise kernel kept for correctness.
 */
int dccl_local_reduce_chain_widen(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                  size_t count, int accumulate, void* stream);

/*
 * Checked widened sum (the device half of dcclRedOpCreateWidenedSumChecked): the widened sum above, which also tells
 * whether a reduced value came out non-finite, from the registers the chain already holds.
 *   dccl_local_reduce_chain_widen_checked  dccl_local_reduce_chain_widen, bit for bit (the check changes no stored
 *                                   value), and: when acc of at least one element i is not finite (fp32 exponent
 *                                   field all ones: +inf, -inf or any NaN), the value 1 is stored to *flag.  acc is
 *                                   the accumulator after widen(own[i]) + acc, BEFORE accumulate's add.
 *   dccl_local_nonfinite_f32        the same rule over `count` fp32 at src, which is only read: *flag = 1 when some
 *                                   src[i] is +-inf or a NaN.  It serves the staged collectives, and any caller.
 * `flag` is one uint32_t in device memory, on a 4-byte boundary.  Nothing else is ever stored to it: it is not read,
 * not cleared and never given another value, so the caller zeroes it and it stays raised over as many calls as the
 * caller likes (several calls may share one flag, on one stream or many).  When every acc is finite nothing is
 * stored.  The flag reports the CONTRIBUTIONS, not the caller's running buffer: with accumulate == 1 the previous
 * content of dst does not enter the test (a dst that already holds inf, with finite contributions, leaves the flag
 * alone), and a finite dst[i] + finite acc that overflows in that last add does NOT raise it.  The store is ordered
 * on `stream` like dst's.  The flag must not lie inside sends[j] or own either: that is the caller's to see to (no
 * validation row; a kernel would store to a word that other lanes read as an operand).
 * Validation of dccl_local_reduce_chain_widen_checked: dccl_local_reduce_chain_widen's rows in their order, with two
 * more: directly after the nsend / sends row (so ahead of count == 0), NULL flag or flag off its 4-byte boundary 4;
 * after the operand-overlap rows, [flag, flag + 4) sharing a byte with [dst, dst + 4 count) 4.  count == 0 succeeds
 * and touches nothing.  Same placement rule, kernels' shape, launch and caps as dccl_local_reduce_chain_widen.
 * Validation of dccl_local_nonfinite_f32, in this order: NULL or misaligned flag 4; count == 0 succeeds; NULL src or
 * src off its 4-byte boundary 4; flag inside [src, src + 4 count) 4; launch failure 1.  One-wave blocks read the
 * 16-byte-aligned body in 16-byte vectors; at most three head and three tail elements are read one by one.
 */
int dccl_local_reduce_chain_widen_checked(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                          size_t count, int accumulate, uint32_t* flag, void* stream);
int dccl_local_nonfinite_f32(const void* src, size_t count, uint32_t* flag, void* stream);

/*
 * Multi-source device copy: dsts[y][0..bytes) = srcs[y][0..bytes) for y < npairs (<= 8), in one
 * launch, so the reads of several peers' chunks use several xGMI links at once (the all-gather
 * half of the direct collectives; replaces W-1 ring all-gather steps,
 * /root/reference/src/core/all_gather_ring.cpp:44-64).
 */
int dccl_copy_multi(const void* const* srcs, void* const* dsts, int npairs, size_t bytes, void* stream);

/*
 * Batched strided row copy, one launch: for every segment i < nsegs (<= 32), every row r < rows and every byte
 * b < row_bytes,  dst[r * dst_stride + b] = src[r * src_stride + b].  It is the pack and unpack of a coalesced
 * group (ncclGroupStart / ncclGroupEnd): packing tensor i of a group into slot-major order is
 * {send_i, pack + off_i, slot_i, slot_i, S} with rows = the slot count, unpacking is the mirror image.  Any byte
 * alignment of either side; every destination row is written in aligned 16-byte vectors with bytewise head and
 * tail.  Validation, in this order and before any HIP call: nsegs outside 0..32, NULL segs with nsegs > 0 or
 * rows == 0 -> 4; nsegs == 0 succeeds; a NULL src or dst of a segment with row_bytes > 0 -> 4; a stride below
 * row_bytes with rows > 1 -> 4; a destination byte that is also a source byte (its own segment's included) or
 * another destination's byte -> 4 (an exact test: destinations that interleave without sharing a byte, as a
 * pack's do, are accepted); launch failure 1.  The overlap test is closed-form for one-row sets and for equal
 * strides (every pack and unpack); segments of different strides whose bounding boxes meet are swept row by row
 * over the side with fewer rows inside the other's box, which costs host time in proportion to that count.
 * dccl_copy_rows_check answers the validation alone (0 or 4) and launches nothing.  It is not one of NCCL's or
 * the reference's entry points: it exists so that a caller, and this project's tests, can tell "accepted" from
 * "rejected" on addresses that must not be dereferenced, which dccl_copy_rows_multi cannot show without launching.
 */
typedef struct {
    const void* src;
    void* dst;
    size_t row_bytes;
    size_t src_stride;
    size_t dst_stride;
} dccl_copy_rows_t;
int dccl_copy_rows_multi(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, void* stream);
int dccl_copy_rows_check(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows);

/*
 * Batched strided fp32 row accumulate, one launch: for every segment i < nsegs (<= 32), every row r < rows and
 * every element e < row_bytes / 4,
 *     dst[r * dst_stride + 4 e] = dst[r * dst_stride + 4 e] + src[r * src_stride + 4 e]      (fp32)
 * one IEEE fp32 add per element, round to nearest even, denormals kept; the payload of a NaN result is not pinned.
 * It is the add dccl_local_reduce_chain_widen applies for accumulate == 1, and the unpack of a coalesced run of
 * widened sums created with accumulate = 1: the segments are the ones dccl_copy_rows_multi would
 * unpack by.  Bytes of dst between its rows are not touched; src is only read.  Either side may lie at any byte
 * address: destination rows on a 4-byte boundary are walked in aligned 16-byte vectors with at most three head and
 * three tail elements, a destination row off that boundary is combined element by element (correct, not fast).
 * Validation, before any HIP call: dccl_copy_rows_check's rules in their order (dst is read as well as written,
 * which "no destination byte is a source byte or another destination's byte" already covers; nsegs == 0
 * succeeds), then a row_bytes that is not a multiple of 4 -> 4; launch failure 1.
 */
int dccl_add_rows_f32_multi(const dccl_copy_rows_t* segs, int nsegs, uint32_t rows, void* stream);

/*
 * Host combine, synchronous: `send` and `recv` are host pointers (the RDMA
 * receive buffers of the reference's host path).  Replaces the reference's CPU
 * boundary do_host_reduce<DT>
 *   (/root/reference/src/core/internal_common.hpp:496-586),
 * called by the ring reduce-scatter at /root/reference/src/core/reduce_scatter_ring.cpp:91-94.
 * The combine runs on the calling thread's current HIP device: chunks are staged
 * through pinned buffers in a copy/compute pipeline (H2D || combine || D2H).
 * Pointers registered with dccl_register_host_memory() are DMA'd directly.
 */
int dccl_local_reduce_host(const void* send, void* recv, int dtype, size_t count, int op);

/*
 * Host chain combine, synchronous: dccl_local_reduce_chain on host pointers (the direct all_reduce of
 * in-process ranks on host buffers).  Operands are staged through pinned memory and
 * combined by zero-copy kernels on the calling thread's current HIP device, in pieces whose staging
 * overlaps the previous piece's kernel; registered operands are read in place.
 */
int dccl_local_reduce_chain_host(const void* const* sends, int nsend, const void* own, void* dst, int dtype,
                                 size_t count, int op);

/*
 * Routing hint for host-resident chunks: the payload size (bytes per operand) from which
 * dccl_local_reduce_host beats the reference's own one-thread CPU loop do_host_reduce<DT>
 * (/root/reference/src/core/internal_common.hpp:496-586) on MI355X, measured by bench.py's
 * `host_crossover` leg on buffers registered with dccl_register_host_memory against one core on the
 * buffers' NUMA node.  A caller keeps do_host_reduce below it; pageable
 * chunks never beat that loop.  0 for dtypes the reference's host loop cannot combine (bf16; fp16 has host
 * operators only in CUDA builds), an unknown dtype included: the GPU path is then the only one.
 * DCCL_HOST_GPU_MIN_BYTES overrides the measured value for every dtype the reference's loop supports.  This
 * is advice for the caller: the library itself never combines on the CPU.
 */
size_t dccl_host_reduce_gpu_min_bytes(int dtype);

/* Page-lock a host range for direct DMA by dccl_local_reduce_host
 * (the role of dcclRegisterCacheMemory, /root/reference/src/core/dccl.cpp:503-549). */
int dccl_register_host_memory(void* buffer, size_t size);
int dccl_deregister_host_memory(void* buffer);

/* Size in bytes of a dtype, 0 if unknown (size_of_type, internal_common.hpp:314-335,
 * with bf16 always present). */
size_t dccl_size_of_type(int dtype);

/* Human-readable result string. */
const char* dccl_result_string(int result);

/* Library version, major*10000 + minor*100 + patch. */
int dccl_version(void);

#ifdef __cplusplus
}
#endif

#endif /* DCCL_REDUCE_H_ */
