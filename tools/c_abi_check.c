/* tools/c_abi_check.c — a plain C11 consumer of the C-ABI headers (no C++, no HIP headers): proves
 * that the include/dccl headers are valid C and that libdccl_amd.so links from C, as a DCCL-side FFI caller
 * would use it.  Without arguments it runs the checks that need no GPU; with "gpu" it also runs the
 * host-pointer combine (staged through the current GPU) against a plain C loop.
 *
 *   gcc -std=c11 -Wall -Wextra -pedantic -Werror -I include tools/c_abi_check.c \
 *       -L dccl_amd/lib -ldccl_amd -Wl,-rpath,dccl_amd/lib -o dccl_amd/bin/c_abi_check
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dccl/dccl_comm.h"
#include "dccl/dccl_reduce.h"
#include "dccl/dccl_synth.h"

static int failures = 0;

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            fprintf(stderr, "c_abi_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            failures++;                                                  \
        }                                                                \
    } while (0)

static void cpu_checks(void) {
    static const size_t sizes[10] = {1, 1, 4, 4, 8, 8, 2, 4, 8, 2};
    for (int t = 0; t < 10; ++t) CHECK(dccl_size_of_type(t) == sizes[t]);
    CHECK(dccl_size_of_type(10) == 0);
    CHECK(dccl_version() > 0);
    CHECK(strlen(dccl_result_string(DCCL_SUCCESS)) > 0);
    float a[4] = {0}, b[4] = {0};
    /* argument validation happens before any device work */
    CHECK(dccl_local_reduce(a, b, 7, 4, 4, NULL) == DCCL_INVALID_USAGE);    /* ncclAvg */
    CHECK(dccl_local_reduce(a, b, 7, 4, 9, NULL) == DCCL_INVALID_ARGUMENT); /* bad op */
    CHECK(dccl_local_reduce(a, b, 11, 4, 0, NULL) == DCCL_INVALID_ARGUMENT); /* bad dtype */
    CHECK(dccl_local_reduce(a, b, 7, 0, 0, NULL) == DCCL_SUCCESS);          /* count 0 */
    CHECK(dccl_local_reduce_host(a, b, 7, 4, 4) == DCCL_INVALID_USAGE);
    const void* sends[1] = {a};
    CHECK(dccl_local_reduce_multi(sends, 0, b, 7, 4, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain(sends, 9, a, b, 7, 4, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_host(sends, 0, a, b, 7, 4, 0) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_synth_fill(NULL, 7, 16, 0, 1, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_copy_multi(NULL, NULL, 0, 16, NULL) == DCCL_SUCCESS);
    CHECK(dccl_all_reduce(a, b, 4, 7, 0, NULL, NULL) == DCCL_INVALID_ARGUMENT); /* null communicator */
    /* partial overlap with the destination (one element apart) is rejected before any device work */
    float c[8] = {0};
    CHECK(dccl_local_reduce(c + 1, c, 7, 4, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_host(c, c + 1, 7, 4, 0) == DCCL_INVALID_ARGUMENT);
    const void* ov[1] = {c + 1};
    CHECK(dccl_local_reduce_multi(ov, 1, c, 7, 4, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain(sends, 1, c + 3, c, 7, 4, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_host(ov, 1, a, c, 7, 4, 0) == DCCL_INVALID_ARGUMENT);
    /* pre-multiplied sum: dtype, nsend, scalar / residence, count 0, NULL operands, overlap, in that order */
    const float half = 0.5f;
    CHECK(dccl_local_scale(a, b, 11, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_scale(a, b, 7, 4, &half, 2, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_scale(a, b, 7, 4, NULL, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_scale(NULL, NULL, 7, 0, &half, 1, NULL) == DCCL_SUCCESS);
    CHECK(dccl_local_scale(NULL, b, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_scale(c + 1, c, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_premul(sends, 1, a, b, 11, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_premul(sends, 9, a, b, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_premul(sends, 1, a, b, 7, 4, &half, -1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_premul(sends, 1, a, b, 7, 0, &half, 0, NULL) == DCCL_SUCCESS);
    CHECK(dccl_local_reduce_chain_premul(sends, 1, NULL, b, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_premul(ov, 1, a, c, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_premul(sends, 1, c + 3, c, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    int premul_op = 0;
    CHECK(dccl_red_op_create_premul_sum(&premul_op, &half, 7, 1, NULL) == DCCL_INVALID_ARGUMENT); /* null comm */
    CHECK(dccl_red_op_destroy(5, NULL) == DCCL_INVALID_ARGUMENT);
    /* wide sum: dtype (fp16 / bf16 only), nsend, count 0, NULL operands, overlap, in that order */
    CHECK(dccl_local_reduce_chain_wide(sends, 1, a, b, 7, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide(sends, 1, a, b, 10, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide(sends, 9, a, b, 9, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide(NULL, 1, a, b, 6, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide(sends, 1, NULL, NULL, 9, 0, NULL) == DCCL_SUCCESS);
    CHECK(dccl_local_reduce_chain_wide(sends, 1, NULL, b, 9, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide(ov, 1, a, c, 9, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide(sends, 1, c + 1, c, 6, 4, NULL) == DCCL_INVALID_ARGUMENT);
    /* conversion: the four pairs only, count 0, NULL operands, any shared byte */
    CHECK(dccl_local_convert(a, 7, b, 7, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert(a, 6, b, 9, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert(a, 8, b, 7, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert(a, 10, b, 7, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert(NULL, 9, NULL, 7, 0, NULL) == DCCL_SUCCESS);
    CHECK(dccl_local_convert(NULL, 7, b, 6, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert(a, 7, NULL, 9, 4, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert(c, 9, c, 7, 4, NULL) == DCCL_INVALID_ARGUMENT);     /* no in-place form */
    CHECK(dccl_local_convert(c + 1, 7, c, 6, 4, NULL) == DCCL_INVALID_ARGUMENT); /* dst's second half in src */
    int wide_op = 0;
    CHECK(dccl_red_op_create_wide_sum(&wide_op, 9, NULL) == DCCL_INVALID_ARGUMENT); /* null communicator */
    /* scaled wide sum: dtype, scalar / residence, nsend, count 0, NULL operands, overlap, in that order; the scalar
     * is one float whatever the dtype */
    CHECK(dccl_local_reduce_chain_wide_scaled(sends, 1, a, b, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide_scaled(sends, 1, a, b, 10, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide_scaled(sends, 1, a, b, 9, 0, NULL, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide_scaled(sends, 1, a, b, 9, 0, &half, 2, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide_scaled(sends, 9, a, b, 9, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide_scaled(NULL, 1, a, b, 6, 4, &half, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide_scaled(sends, 1, NULL, NULL, 9, 0, &half, 0, NULL) == DCCL_SUCCESS);
    CHECK(dccl_local_reduce_chain_wide_scaled(sends, 1, NULL, b, 9, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide_scaled(ov, 1, a, c, 9, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_wide_scaled(sends, 1, c + 1, c, 6, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    /* scaled conversion: 7 -> 6, 7 -> 9, 6 -> 6, 9 -> 9 only, scalar / residence, count 0, NULL operands, overlap */
    CHECK(dccl_local_convert_scaled(a, 9, b, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert_scaled(a, 6, b, 9, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert_scaled(a, 7, b, 7, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert_scaled(a, 7, b, 9, 0, NULL, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert_scaled(a, 9, b, 9, 0, &half, -1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert_scaled(NULL, 7, NULL, 6, 0, &half, 1, NULL) == DCCL_SUCCESS);
    CHECK(dccl_local_convert_scaled(NULL, 7, b, 6, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert_scaled(a, 6, NULL, 6, 4, &half, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_convert_scaled(c, 7, c, 9, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT);     /* no in-place */
    CHECK(dccl_local_convert_scaled(c + 1, 9, c, 9, 4, &half, 1, NULL) == DCCL_INVALID_ARGUMENT); /* partial overlap */
    CHECK(dccl_red_op_create_wide_scaled_sum(&wide_op, &half, 9, 1, NULL) == DCCL_INVALID_ARGUMENT); /* null comm */
    CHECK(dccl_red_op_create_wide_scaled_sum(&wide_op, &half, 9, 2, NULL) == DCCL_INVALID_ARGUMENT);
    /* widened sum: dtype, accumulate, nsend, count 0, NULL operands, any shared byte with the fp32 dst, in that order */
    CHECK(dccl_local_reduce_chain_widen(sends, 1, a, b, 7, 4, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_widen(sends, 1, a, b, 10, 4, 2, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_widen(sends, 1, a, b, 9, 0, 2, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_widen(sends, 9, a, b, 9, 4, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_widen(NULL, 1, a, b, 6, 0, 0, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_widen(sends, 1, NULL, NULL, 9, 0, 1, NULL) == DCCL_SUCCESS);
    CHECK(dccl_local_reduce_chain_widen(sends, 1, NULL, b, 9, 4, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_local_reduce_chain_widen(sends, 1, c, c, 9, 4, 0, NULL) == DCCL_INVALID_ARGUMENT); /* no in-place form */
    /* a source 4 bytes past dst: behind the end of two 16-bit elements, inside two fp32 ones */
    CHECK(dccl_local_reduce_chain_widen(ov, 1, a, c, 6, 2, 1, NULL) == DCCL_INVALID_ARGUMENT);
    CHECK(dccl_red_op_create_widened_sum(&wide_op, 9, 1, NULL) == DCCL_INVALID_ARGUMENT); /* null communicator */
    /* batched row copy: every validation case answers before any device work (never-dereferenced addresses) */
    {
        char* const base = (char*)(uintptr_t)0x100000000000ull;
        dccl_copy_rows_t seg[2] = {{base, base + 4096, 100, 100, 256}, {base + 1024, base + 4096 + 100, 28, 28, 256}};
        CHECK(dccl_copy_rows_multi(seg, -1, 4, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_copy_rows_multi(seg, 33, 4, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_copy_rows_multi(NULL, 1, 4, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_copy_rows_multi(seg, 2, 0, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_copy_rows_multi(NULL, 0, 4, NULL) == DCCL_SUCCESS);
        CHECK(dccl_copy_rows_check(seg, 2, 4) == DCCL_SUCCESS); /* a pack: the destinations interleave */
        seg[1].dst = base + 4096 + 99;                          /* one shared byte */
        CHECK(dccl_copy_rows_multi(seg, 2, 4, NULL) == DCCL_INVALID_ARGUMENT);
        seg[1].dst = base + 4096 + 100;
        seg[1].dst_stride = 27; /* a stride below row_bytes */
        CHECK(dccl_copy_rows_multi(seg, 2, 4, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_copy_rows_check(seg, 2, 1) == DCCL_SUCCESS); /* one row: strides are not looked at */
        seg[0].src = NULL;
        CHECK(dccl_copy_rows_multi(seg, 2, 1, NULL) == DCCL_INVALID_ARGUMENT);
    }
    /* batched fp32 row accumulate: the row copy's rules, then row_bytes % 4 */
    {
        char* const base = (char*)(uintptr_t)0x100000000000ull;
        dccl_copy_rows_t seg[2] = {{base, base + 4096, 100, 100, 256}, {base + 1024, base + 4096 + 100, 30, 32, 256}};
        CHECK(dccl_add_rows_f32_multi(seg, 33, 4, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_add_rows_f32_multi(NULL, 1, 4, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_add_rows_f32_multi(seg, 2, 0, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_add_rows_f32_multi(NULL, 0, 4, NULL) == DCCL_SUCCESS);
        CHECK(dccl_copy_rows_check(seg, 2, 4) == DCCL_SUCCESS);
        CHECK(dccl_add_rows_f32_multi(seg, 2, 4, NULL) == DCCL_INVALID_ARGUMENT); /* 30 bytes: no whole fp32 */
        seg[1].row_bytes = 28;
        seg[1].dst = base + 4096 + 99; /* one shared byte */
        CHECK(dccl_add_rows_f32_multi(seg, 2, 4, NULL) == DCCL_INVALID_ARGUMENT);
    }
    /* group calls: depth per thread, an invalid call inside a group answers at once */
    {
        uint64_t st0[6] = {0}, st1[6] = {0};
        CHECK(dccl_group_stats(st0, 6) == 6);
        CHECK(dccl_group_end() == DCCL_INVALID_USAGE);
        CHECK(dccl_group_start() == DCCL_SUCCESS && dccl_group_start() == DCCL_SUCCESS);
        CHECK(dccl_all_reduce(a, b, 4, 7, 0, NULL, NULL) == DCCL_INVALID_ARGUMENT);
        CHECK(dccl_group_end() == DCCL_SUCCESS && dccl_group_end() == DCCL_SUCCESS);
        CHECK(dccl_group_end() == DCCL_INVALID_USAGE);
        CHECK(dccl_group_stats(st1, 6) == 6 && st1[0] == st0[0] + 1 && st1[1] == st0[1]);
    }
    /* routing hint: the reference has no host loop for bf16 / fp16 */
    CHECK(dccl_host_reduce_gpu_min_bytes(9) == 0 && dccl_host_reduce_gpu_min_bytes(6) == 0);
}

static void gpu_checks(void) {
    enum { N = 100003 };
    float* s = malloc(N * sizeof(float));
    float* r = malloc(N * sizeof(float));
    float* want = malloc(N * sizeof(float));
    int8_t* si = malloc(N);
    int8_t* ri = malloc(N);
    int8_t* wanti = malloc(N);
    if (!s || !r || !want || !si || !ri || !wanti) {
        failures++;
        return;
    }
    for (int i = 0; i < N; ++i) {
        s[i] = (float)(i % 977) * 0.25f - 100.0f;
        r[i] = (float)(i % 131) * 0.5f;
        want[i] = r[i] + s[i];
        si[i] = (int8_t)(i * 7);
        ri[i] = (int8_t)(i * 13 + 1);
        wanti[i] = (int8_t)(ri[i] * si[i]); /* wraps, like the reference's int8 r *= s */
    }
    CHECK(dccl_local_reduce_host(s, r, 7, N, 0) == DCCL_SUCCESS);
    CHECK(memcmp(r, want, N * sizeof(float)) == 0);
    CHECK(dccl_local_reduce_host(si, ri, 0, N, 1) == DCCL_SUCCESS);
    CHECK(memcmp(ri, wanti, N) == 0);
    free(s), free(r), free(want), free(si), free(ri), free(wanti);
    /* one small batched row copy on page-locked host memory (the kernel reads and writes it in place); finalizing a
     * communicator waits for the device */
    enum { ROWS = 3, PAGE = 4096 };
    unsigned char* m = aligned_alloc(PAGE, 2 * PAGE);
    void* comm = NULL;
    if (!m) {
        failures++;
        return;
    }
    for (int i = 0; i < 2 * PAGE; ++i) m[i] = (unsigned char)(i < PAGE ? i * 31 + 7 : 0xee);
    CHECK(dccl_register_host_memory(m, 2 * PAGE) == DCCL_SUCCESS);
    CHECK(dccl_comm_init_rank(&comm, 1, 0) == DCCL_SUCCESS);
    const dccl_copy_rows_t seg[2] = {{m + 3, m + PAGE + 5, 37, 37, 128}, {m + 200, m + PAGE + 5 + 37, 17, 17, 128}};
    CHECK(dccl_copy_rows_multi(seg, 2, ROWS, NULL) == DCCL_SUCCESS);
    /* the only device synchronisation a C caller has: ncclCommFinalize waits for the device (dccl_api.cpp says so
     * at that call); without it the comparison below would race the kernel */
    CHECK(dccl_comm_finalize(comm) == DCCL_SUCCESS);
    for (int i = 0; i < PAGE; ++i) {
        unsigned char want_b = 0xee;
        const int row = (i - 5) / 128, b = (i - 5) % 128;
        if (i >= 5 && row < ROWS && b < 37) want_b = m[3 + row * 37 + b];
        else if (i >= 5 && row < ROWS && b < 37 + 17) want_b = m[200 + row * 17 + (b - 37)];
        CHECK(m[PAGE + i] == want_b);
    }
    CHECK(dccl_deregister_host_memory(m) == DCCL_SUCCESS);
    free(m);
}

int main(int argc, char** argv) {
    cpu_checks();
    if (argc > 1 && strcmp(argv[1], "gpu") == 0) gpu_checks();
    printf("c_abi_check: %s\n", failures ? "FAILED" : "ok");
    return failures ? 1 : 0;
}
