// prims.h -- scan_exclusive (scan.h) and sort_pairs (sort.h) called on their own, exactly as the product calls them:
// the bodies of shp_prim_scan / shp_prim_sort.  No product path goes through here; the two entry points exist so
// that tests/test_gpu_primitives.py can reach the primitives at the sizes, alignments and flag combinations at which
// their kernels change path (tests/prim_cases.py), which whole workloads only meet by chance.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"

struct PlainArrFn {     // ArrFn without get4: scan_block takes its four 4-byte loads
    const uint32_t *a;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return a[i]; }
};

#define PRIM_POISON 0xA5A5A5A5u     // what both totals hold before the scan: a total the scan never stored shows

// flags bit 0: PlainArrFn in place of ArrFn; bit 1: lazy add-back (out stays without the block offsets, which go to
// d_boff_out, *nboff_out of them: 0 when the scan handed back nullptr)
static int run_prim_scan(shp_ctx *ctx, const uint32_t *d_in, uint32_t n, uint32_t *d_out, int flags,
                         uint32_t *total_dev_out, uint32_t *total_mirror_out, uint32_t *d_boff_out, uint32_t *nboff_out)
{
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(n)));
    CHK(buf_ensure(ctx, ctx->small, 4096));
    uint32_t *tot = bp<uint32_t>(ctx->small);
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_PRIM;
    HIPCHK(ctx, hipMemsetAsync(tot, (int)(PRIM_POISON & 255u), 4, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *(volatile uint32_t *)mir = PRIM_POISON;
    const uint32_t *boff = nullptr;
    const uint32_t **lazy = (flags & 2) ? &boff : nullptr;
    if (flags & 1) {
        PlainArrFn f{d_in};
        CHK(scan_exclusive(ctx, f, n, d_out, tot, bp<uint32_t>(ctx->scan_tmp), lazy, mir));
    } else {
        ArrFn f{d_in};
        CHK(scan_exclusive(ctx, f, n, d_out, tot, bp<uint32_t>(ctx->scan_tmp), lazy, mir));
    }
    uint32_t nboff = 0;
    if (boff) {
        nboff = (n + SCAN_ITEMS - 1) / SCAN_ITEMS;
        HIPCHK(ctx, hipMemcpyAsync(d_boff_out, boff, (size_t)nboff * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, tot, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *total_dev_out = ctx->h_pinned[0];
    *total_mirror_out = *(volatile uint32_t *)mir;
    if (nboff_out) *nboff_out = nboff;
    return 0;
}

// the 257 digit starts of a one-pass sort, read the way fit_elkan.h's sums kernels read them
__global__ __launch_bounds__(64) void k_prim_digit_starts(const uint32_t *hscan, const uint32_t *boff, uint32_t nblk,
                                                          uint32_t n, uint32_t *out)
{
    for (uint32_t d = threadIdx.x; d <= 256u; d += 64u) out[d] = sort_digit_start(hscan, boff, nblk, d, n);
}

// flags bit 0: the staged scatter.  d_keys_out == nullptr: sort_pairs is told that the keys are not wanted.
// digit_starts (host, 257 words, may be nullptr): filled when the sort took one pass, all zero for n == 0 (no pass
// ran: there is no histogram), left alone otherwise
static int run_prim_sort(shp_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, uint32_t n, int bits, int flags,
                         uint32_t *d_keys_out, uint32_t *d_vals_out, uint32_t *digit_starts)
{
    uint32_t *ks = nullptr, *vs = nullptr;
    SortDigits sd;
    CHK(sort_pairs(ctx, d_keys, d_vals, n, bits, d_keys_out ? &ks : nullptr, &vs, (flags & 1) != 0, &sd));
    if (n) {
        if (d_keys_out) HIPCHK(ctx, hipMemcpyAsync(d_keys_out, ks, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(d_vals_out, vs, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if (digit_starts && n == 0) memset(digit_starts, 0, 257 * 4);
    if (digit_starts && n && sd.passes == 1) {
        CHK(buf_ensure(ctx, ctx->small, 4096));
        uint32_t *d_st = bp<uint32_t>(ctx->small);
        hipLaunchKernelGGL(k_prim_digit_starts, dim3(1), dim3(64), 0, ctx->stream, sd.hscan, sd.boff, sd.nblk, n, d_st);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, d_st, 257 * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        memcpy(digit_starts, ctx->h_pinned, 257 * 4);
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
