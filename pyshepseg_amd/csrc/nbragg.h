// nbragg.h -- per-segment columns carried to the groups of a merge (neighbours.aggregateToGroups), and the groups'
// member list.
//
// recode[i] is the group of old id i (0: none), M the number of groups (nbrmerge.h).  The MEMBER LIST is the CSR of
// the groups over their members: offsets over the new ids 0 .. M (row 0 is empty), and the old ids of every group in
// ascending order.  It is a pure function of recode:
//   sizes     the groups' sizes: those of the merge, or counted from an uploaded recode (k_agg_count, integer atomics);
//   offsets   their exclusive scan (scan.h), widened to the int64 offsets the reduction kernels read;
//   members   the ids 0 .. S sorted by their new id with the stable radix sort of sort.h (value = index): within a
//             group the ids stay ascending; the ids that recode to 0 come first and are left out.
// It is built once per merge result and kept, with the list of its long rows (shp_ctx::agg_longs, an NbrLongList
// under the member list's serial), until the next merge.
//
// THE AGGREGATION runs the reduction kernels of nbrreduce.h over that CSR: a group is a "row", its members are the
// "neighbour ids" and the weight of a member is the "border length" (k_agg_weights lays the weights out by entry).
// The order of the float sums is therefore the one nbrreduce.h states for a row, as a function of the group's
// size alone: member order up to NBRR_LONG members, chunks of NBRR_CHUNK by position above that.  count, weight, min,
// max, the float sum, mean and weightedmean come from those kernels (count, border, min, max, NBRR_SUM, mean,
// bordermean).  The sum of an INTEGER column is exact int64 and wraps: k_agg_isum adds every id's value to its
// group by 64-bit integer atomics, the lanes of a wavefront that hold the first lane's group as one add (mrg_count).
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"
#include "nbrreduce.h"
#include "nbrmerge.h"

// bits of the aggregation's mask, and the slot of a statistic's output
enum { AGG_COUNT = 0, AGG_WEIGHT = 1, AGG_MIN = 2, AGG_MAX = 3, AGG_SUM = 4, AGG_MEAN = 5, AGG_WEIGHTEDMEAN = 6,
       AGG_NSTATS = 7 };

// gsize[recode[i]] += 1 for every id with a group; *bad: the largest recode above M (such an id is not counted)
__global__ __launch_bounds__(256) void k_agg_count(const uint32_t *__restrict__ recode, uint32_t ns, uint32_t M,
                                                   unsigned long long *gsize, unsigned long long *bad)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t g = i < ns ? recode[i] : 0u;
    if (g > M) { atomicMax(bad, (unsigned long long)g); g = 0u; }
    if (i == 0u && g != 0u) { atomicMax(bad, 0xffffffffull); g = 0u; }      // (id 0 is in no group)
    mrg_count(gsize, g, 1ull, g != 0u);
}

struct AggSizeFn {              // the size of group i; the item behind the last group is 0 (its scan is the total)
    const unsigned long long *gsize;
    uint32_t nm;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return i < nm ? (uint32_t)gsize[i] : 0u; }
};

__global__ __launch_bounds__(256) void k_agg_offsets(const uint32_t *__restrict__ scanned, uint32_t n, long long *__restrict__ offs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) offs[i] = (long long)scanned[i];
}

// w[e] = the weight of member e (1 without a weight column)
__global__ __launch_bounds__(256) void k_agg_weights(const uint32_t *__restrict__ mem, size_t nmem,
                                                     const long long *__restrict__ wcol, long long *__restrict__ w)
{
    for (size_t e = (size_t)blockIdx.x * 256u + threadIdx.x; e < nmem; e += (size_t)gridDim.x * 256u)
        w[e] = wcol ? wcol[mem[e]] : 1ll;
}

// isum[recode[i]] += col[i] (wrapping) over the ids whose value, widened, is not ignored
__global__ __launch_bounds__(256) void k_agg_isum(const long long *__restrict__ col, const uint32_t *__restrict__ recode,
                                                  uint32_t ns, int has_ign, double ign, unsigned long long *isum)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    uint32_t g = 0u;
    long long v = 0;
    if (i < ns) {
        g = recode[i];
        v = col[i];
        if (nbrr_ignored((double)v, has_ign, ign)) g = 0u;
    }
    mrg_count(isum, g, (unsigned long long)v, g != 0u);
}

// ---- host side --------------------------------------------------------------------------------------------
// The member list of the resident groups (h_recode == NULL: S, M and the serial are theirs) or of a recode from the
// host (S + 1 uint32, M groups: a serial of its own).
static int run_agg_build(shp_ctx *ctx, const uint32_t *h_recode, uint32_t S, uint32_t M)
{
    AggState &a = ctx->agg;
    hipStream_t st = ctx->stream;
    a = AggState{};
    const size_t ns = (size_t)S + 1, nm = (size_t)M + 1;
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_NBR;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    const uint32_t *d_recode = bp<uint32_t>(ctx->mrg_recode);
    const unsigned long long *d_gsize = (const unsigned long long *)ctx->mrg_gsize.p;
    CHK(buf_ensure(ctx, ctx->agg_scan, (nm + 1) * 4));
    CHK(buf_ensure(ctx, ctx->agg_offs, (nm + 1) * 8));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(nm + 1)));
    if (h_recode) {
        CHK(buf_ensure(ctx, ctx->agg_recode, ns * 4));
        CHK(buf_ensure(ctx, ctx->agg_gsize, nm * 8));
        CHK(buf_ensure(ctx, ctx->agg_ctr, 8));
        HIPCHK(ctx, hipMemcpyAsync(ctx->agg_recode.p, h_recode, ns * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemsetAsync(ctx->agg_gsize.p, 0, nm * 8, st));
        HIPCHK(ctx, hipMemsetAsync(ctx->agg_ctr.p, 0, 8, st));
        d_recode = bp<uint32_t>(ctx->agg_recode);
        d_gsize = (const unsigned long long *)ctx->agg_gsize.p;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (h_recode) {
        hipLaunchKernelGGL(k_agg_count, dim3(grid_for(ns, 256)), dim3(256), 0, st, d_recode, (uint32_t)ns, M,
                           (unsigned long long *)ctx->agg_gsize.p, (unsigned long long *)ctx->agg_ctr.p);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(pin, ctx->agg_ctr.p, 8, hipMemcpyDeviceToHost, st));
    }
    AggSizeFn sf{d_gsize, (uint32_t)nm};
    uint32_t *scanned = bp<uint32_t>(ctx->agg_scan);
    CHK(scan_exclusive(ctx, sf, (uint32_t)(nm + 1), scanned, nullptr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir));
    hipLaunchKernelGGL(k_agg_offsets, dim3(grid_for(nm + 1, 256)), dim3(256), 0, st, (const uint32_t *)scanned,
                       (uint32_t)(nm + 1), bp<long long>(ctx->agg_offs));
    KCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (h_recode && pin[0])
        SHP_FAIL(ctx, SHP_ERR_ARG, "recode is no recode of %u groups: %s", M,
                 pin[0] == 0xffffffffull ? "id 0 has a group" : "an id's group lies above them");
    const size_t nmem = *(volatile uint32_t *)mir;
    if (nmem > (size_t)S) SHP_FAIL(ctx, SHP_ERR_STATE, "%zu members of %u ids", nmem, S);
    uint32_t *sorted = nullptr;
    CHK(sort_pairs(ctx, d_recode, nullptr, (uint32_t)ns, bits_for(M), nullptr, &sorted));
    CHK(buf_ensure(ctx, ctx->agg_mem, nmem * 4));
    if (nmem) HIPCHK(ctx, hipMemcpyAsync(ctx->agg_mem.p, sorted + (ns - nmem), nmem * 4, hipMemcpyDeviceToDevice, st));
    const unsigned long long serial = h_recode ? nbr_next_serial() : ctx->mrg.serial;
    CHK(nbrr_long_ensure(ctx, ctx->agg_longs, (const long long *)ctx->agg_offs.p, (uint32_t)nm, serial));
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    a.dev_ms = ms;
    a.S = S;
    a.M = M;
    a.nmem = nmem;
    a.recode = d_recode;
    a.serial = serial;
    a.stage = 1;
    return 0;
}

static int run_agg_download(shp_ctx *ctx, int64_t *offsets, uint32_t *members)
{
    const AggState &a = ctx->agg;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(offsets, ctx->agg_offs.p, ((size_t)a.M + 2) * 8, hipMemcpyDeviceToHost, st));
    if (a.nmem) HIPCHK(ctx, hipMemcpyAsync(members, ctx->agg_mem.p, (size_t)a.nmem * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// One column of the old ids over the member list.  weights: host, S + 1 int64 of 0 or more, or NULL (every weight 1).
// outs[i]: host memory of M + 1 rows for statistic i of the mask.
static int run_agg(shp_ctx *ctx, const void *col, int ctype, const int64_t *weights, int has_ign, double ign, double missing,
                   uint32_t mask, void *const *outs, double *dev_ms_out)
{
    const AggState &a = ctx->agg;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)a.S + 1, nm = (size_t)a.M + 1;
    const bool isum = ctype == COL_I64 && ((mask >> AGG_SUM) & 1u);
    static const int slot_of[AGG_NSTATS] = {NBRR_COUNT, NBRR_BORDER, NBRR_MIN, NBRR_MAX, NBRR_SUM, NBRR_MEAN, NBRR_BORDERMEAN};
    int nsel = 0;
    for (int i = 0; i < AGG_NSTATS; i++) nsel += (mask >> i) & 1u;
    CHK(buf_ensure(ctx, ctx->nbrr_out, (size_t)nsel * nm * 8));
    CHK(buf_ensure(ctx, ctx->agg_w, (size_t)a.nmem * 8));
    const long long *d_wcol = nullptr;
    if (weights) {
        CHK(buf_ensure(ctx, ctx->agg_wcol, ns * 8));
        HIPCHK(ctx, hipMemcpyAsync(ctx->agg_wcol.p, weights, ns * 8, hipMemcpyHostToDevice, st));
        d_wcol = (const long long *)ctx->agg_wcol.p;
    }
    const void *d_raw = nullptr;
    CHK(nbrr_stage_column(ctx, col, ctype, ns, &d_raw));
    hipLaunchKernelGGL(k_agg_weights, dim3(grid_for(a.nmem, 256, 2048u)), dim3(256), 0, st, (const uint32_t *)ctx->agg_mem.p,
                       (size_t)a.nmem, d_wcol, bp<long long>(ctx->agg_w));
    KCHK(ctx);
    NbrrParams p = nbrr_params(ctx, ctx->agg_offs.p, ctx->agg_mem.p, ctx->agg_w.p, (uint32_t)nm, 0u, has_ign, ign, missing);
    void *d_out[AGG_NSTATS];
    int slot = 0;
    bool any = false;
    for (int i = 0; i < AGG_NSTATS; i++) {
        d_out[i] = ((mask >> i) & 1u) ? (void *)((char *)ctx->nbrr_out.p + (size_t)(slot++) * nm * 8) : nullptr;
        if (d_out[i] && !(i == AGG_SUM && isum)) { p.out[slot_of[i]] = d_out[i]; any = true; }
    }
    if (any) CHK(nbrr_launch(ctx, p, ctx->agg_longs));
    if (isum) {
        HIPCHK(ctx, hipMemsetAsync(d_out[AGG_SUM], 0, nm * 8, st));
        hipLaunchKernelGGL(k_agg_isum, dim3(grid_for(ns, 256)), dim3(256), 0, st, (const long long *)d_raw, a.recode,
                           (uint32_t)ns, has_ign, ign, (unsigned long long *)d_out[AGG_SUM]);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    for (int i = 0; i < AGG_NSTATS; i++)
        if (d_out[i]) HIPCHK(ctx, hipMemcpyAsync(outs[i], d_out[i], nm * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return nbrr_dev_ms(ctx, dev_ms_out);
}
