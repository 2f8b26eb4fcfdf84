// dneighbours.h -- the segment-neighbour table (neighbours.h) of a label raster that is sharded by rows over the
// ranks, and the reduction of columns over it (nbrreduce.h), without gathering the labels
// (distributed.findSegmentNeighboursDistributed / reduceOverNeighboursDistributed).
//
// The distributed table is sharded by ID, not by image rows: rank r ends up with the finished CSR rows of the ids of
// its share [id_lo, id_hi) (distributed.idRange, where the statistics reduce their straddlers) -- whole rows, every
// neighbour, final lengths, which is what the float sums of nbrreduce.h need (they run over the complete row in
// entry order).  Everything up to there is integer work, so no order of records or atomics can change a result.
//
//  1. run_dnbr_local.  The rank's rows go through k_nbr_patch as they are (only pairs whose UPPER pixel lies in a
//     block count): rows 0 .. h - 2 in place, each with the row after it, then a two-row scratch block -- the last
//     own row and the halo row, the first row of the next rank that holds rows, which does not follow in memory.
//     The records are sorted by (a, b) and run-length reduced (nbr_sort_reduce of neighbours.h, reading 64-bit
//     counts), so AT MOST ONE RECORD PER DISTINCT PAIR of a rank exists from here on.  dnbr_pack: k_dnbr_pack writes
//     them as 16-byte records in the patch kernel's layout (b, a, count low word, count high word) into two sets,
//     split by ballot and one atomic per wavefront and set: HOME (both ids in the rank's own share: nobody else
//     needs them) and TRAVELLING (everything else).
//  2. The caller all-gathers the travelling records, slot = the largest count over the ranks.
//  3. run_dnbr_merge.  k_dnbr_pick takes from the gathered blocks (every rank's valid count, not the slot) the
//     records with a or b in the share, behind a copy of the home records; they are sorted and reduced again (a pair
//     seen by several ranks adds up) and the CSR of the share is built by the routine that builds the whole table
//     (nbr_build_csr of neighbours.h, over the rows [id_lo, id_hi)):
//     entry (a, b) goes to row a if a is in the share (its larger neighbours, in the reduced order) and to row b if
//     b is (its smaller neighbours, in the stable order by b); a row holds the smaller neighbours first.  The reduced
//     entries with a in the share are one run of the (a, b) order, those with b in the share one run of the order by
//     b: k_dnbr_bounds finds where the runs start.  k_dnbr_columns writes the rows' lengths and sums into two
//     full-length int64 columns that are 0 outside the share, so one integer all-reduce completes them.
//  4. run_dnbr_reduce: k_nbrr_short / k_nbrr_long / k_nbrr_long_combine over the share table with the row base
//     NbrrParams::row0 = id_lo: row i is id id_lo + i.  The gathered values come from the full column every rank
//     passes; the outputs are full-length device columns, 0 outside the share, for one all-reduce of bit patterns.
//     The summation order of a row is that of nbrreduce.h, so the results are those of the one-GPU reduction.
//
// The share table is an NbrTable of its own (shp_ctx::dnbr_tab: buffers, serial, list of long rows): it is not the
// context's "finished table" of shp_nbr_reduce (shp_ctx::nbr_tab), and neither displaces the other; download, the
// copy half of an upload and the reduction's host routines are those of the one-GPU table.  DNbrState holds only the
// exchange between the local step and the merge.  The local step does use the one-GPU accumulation (shp_nbr_begin's
// state), so it ends any one-GPU table of the context.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"
#include "neighbours.h"
#include "nbrreduce.h"

// where the lanes of a wavefront that hold `take` put their items: a ballot, one atomic add of the wavefront's
// count by its first lane; returns the lane's place (meaningless where !take)
__device__ __forceinline__ unsigned long long dnbr_place(bool take, unsigned long long *ctr)
{
    const unsigned lane = lane_id();
    const unsigned long long m = __ballot(take);
    unsigned long long base = 0ull;
    if (lane == 0u && m) base = atomicAdd(ctr, (unsigned long long)__popcll(m));
    const uint32_t blo = __shfl((uint32_t)base, 0, 64), bhi = __shfl((uint32_t)(base >> 32), 0, 64);
    return (((unsigned long long)bhi << 32) | blo) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
}

// the reduced pairs as records (b, a, count low, count high): ctr[0] counts the home records (both ids in [lo, hi)),
// ctr[1] the travelling ones.  Each set has room for all U.
__global__ __launch_bounds__(256) void k_dnbr_pack(const uint32_t *__restrict__ ua, const uint32_t *__restrict__ ub,
                                                   const unsigned long long *__restrict__ ucnt, uint32_t U, uint32_t lo,
                                                   uint32_t hi, uint4 *__restrict__ home, uint4 *__restrict__ trav,
                                                   unsigned long long *__restrict__ ctr)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const bool in = j < U;
    const uint32_t a = in ? ua[j] : 0u, b = in ? ub[j] : 0u;
    const unsigned long long c = in ? ucnt[j] : 0ull;
    const bool ishome = in && a >= lo && a < hi && b >= lo && b < hi;
    const bool istrav = in && !ishome;
    const unsigned long long ph = dnbr_place(ishome, &ctr[0]), pt = dnbr_place(istrav, &ctr[1]);
    const uint4 r = make_uint4(b, a, (uint32_t)c, (uint32_t)(c >> 32));
    if (ishome && ph < (unsigned long long)U) home[ph] = r;
    if (istrav && pt < (unsigned long long)U) trav[pt] = r;
}

// from `world` gathered blocks of `slot` records, block r holding counts[r] valid ones: those with an id in [lo, hi),
// appended to out at ctr[0] (which starts at the number of records out holds already); room for `cap` records
__global__ __launch_bounds__(256) void k_dnbr_pick(const uint4 *__restrict__ all, unsigned long long slot,
                                                   unsigned long long total, const uint32_t *__restrict__ counts,
                                                   uint32_t lo, uint32_t hi, uint4 *__restrict__ out,
                                                   unsigned long long cap, unsigned long long *__restrict__ ctr)
{
    const unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x;
    bool take = false;
    uint4 r = make_uint4(0u, 0u, 0u, 0u);
    if (i < total) {
        const unsigned long long blk = i / slot, j = i - blk * slot;
        if (j < (unsigned long long)counts[blk]) {
            r = all[i];
            take = (r.y >= lo && r.y < hi) || (r.x >= lo && r.x < hi);
        }
    }
    const unsigned long long p = dnbr_place(take, &ctr[0]);
    if (take && p < cap) out[p] = r;
}

// numNeighbours and borderLength of the share's rows into the full-length columns num / bor.  A thread per row sums a
// row of up to NBRR_LONG entries; the longer rows of a workgroup are then summed by all of its threads together
// (integer sums: any order).
__global__ __launch_bounds__(256) void k_dnbr_columns(const long long *__restrict__ offs, const long long *__restrict__ lens,
                                                      uint32_t nrows, uint32_t lo, long long *__restrict__ num,
                                                      long long *__restrict__ bor)
{
    __shared__ long long s_a[256], s_b[256];
    __shared__ unsigned long long s_sum;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    long long a = 0, b = 0;
    if (i < nrows) {
        a = offs[i];
        b = offs[i + 1u];
        num[(size_t)lo + i] = b - a;
        if (b - a <= (long long)NBRR_LONG) {
            long long sum = 0;
            for (long long e = a; e < b; e++) sum += lens[e];
            bor[(size_t)lo + i] = sum;
        }
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    __syncthreads();
    for (uint32_t t = 0; t < 256u; t++) {
        const long long ta = s_a[t], tb = s_b[t];
        if (tb - ta <= (long long)NBRR_LONG) continue;          // (uniform in the workgroup)
        if (threadIdx.x == 0u) s_sum = 0ull;
        __syncthreads();
        unsigned long long part = 0ull;
        for (long long e = ta + threadIdx.x; e < tb; e += 256) part += (unsigned long long)lens[e];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t plo = __shfl_xor((uint32_t)part, d, 64), phi = __shfl_xor((uint32_t)(part >> 32), d, 64);
            part += ((unsigned long long)phi << 32) | plo;
        }
        if (lane_id() == 0u) atomicAdd(&s_sum, part);
        __syncthreads();
        if (threadIdx.x == 0u) bor[(size_t)lo + blockIdx.x * 256u + t] = (long long)s_sum;
        __syncthreads();
    }
}

// ---- host side --------------------------------------------------------------------------------------------
// The U reduced pairs (nbr_ua / nbr_ub / nbr_ucnt) as home and travelling records against the share [lo, hi), in
// dnbr_home / dnbr_trav.  ev[1] is recorded behind the pack and the stream synchronised; the two counts must add up to U.
static int dnbr_pack(shp_ctx *ctx, uint32_t U, uint32_t lo, uint32_t hi, unsigned long long *nhome_out,
                     unsigned long long *ntrav_out)
{
    hipStream_t st = ctx->stream;
    unsigned long long *ctr = (unsigned long long *)ctx->nbr_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    pin[0] = pin[1] = 0ull;
    if (U) {
        CHK(buf_ensure(ctx, ctx->dnbr_home, (size_t)U * 16));
        CHK(buf_ensure(ctx, ctx->dnbr_trav, (size_t)U * 16));
        HIPCHK(ctx, hipMemsetAsync(ctr, 0, 16, st));
        hipLaunchKernelGGL(k_dnbr_pack, dim3(grid_for(U, 256)), dim3(256), 0, st, (const uint32_t *)ctx->nbr_ua.p,
                           (const uint32_t *)ctx->nbr_ub.p, (const unsigned long long *)ctx->nbr_ucnt.p, U, lo, hi,
                           (uint4 *)ctx->dnbr_home.p, (uint4 *)ctx->dnbr_trav.p, ctr);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(pin, ctr, 16, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (pin[0] + pin[1] != (unsigned long long)U)
        SHP_FAIL(ctx, SHP_ERR_STATE, "%llu home and %llu travelling records for %u pairs", pin[0], pin[1], U);
    *nhome_out = pin[0];
    *ntrav_out = pin[1];
    return 0;
}

// a share table is begun: the share of the ids 0 .. S waits in the context's share table, which gets a new serial
static void dnbr_begin_share(shp_ctx *ctx, uint32_t S, uint32_t id_lo, uint32_t id_hi)
{
    NbrTable &t = ctx->dnbr_tab;
    nbr_table_end(t);
    t.serial = nbr_next_serial();
    t.S = S;
    t.row0 = id_lo;
    t.nrows = id_hi - id_lo;
}

// Step 1.  d_seg: the rank's nrows rows; d_halo: the row after them (nullptr: the raster ends with them).
// *max_label_out: the largest label of the rows (the halo row included); above S nothing further is done.
// counts_out[3]: distinct pairs of the rank, home records, travelling records (*trav_out, in dnbr_trav).
static int run_dnbr_local(shp_ctx *ctx, const uint32_t *d_seg, uint32_t nrows, uint32_t ncols, const uint32_t *d_halo,
                          uint32_t S, int four_connected, uint32_t id_lo, uint32_t id_hi, uint32_t *max_label_out,
                          int64_t *counts_out, void **trav_out)
{
    DNbrState &d = ctx->dnbr;
    hipStream_t st = ctx->stream;
    d = DNbrState{};
    dnbr_begin_share(ctx, S, id_lo, id_hi);
    counts_out[0] = counts_out[1] = counts_out[2] = 0;
    *trav_out = nullptr;
    CHK(run_nbr_begin(ctx, (int64_t)S, four_connected));
    if (nrows >= 2u) CHK(run_nbr_accumulate(ctx, d_seg, nrows - 1u, ncols, 1));
    if (nrows >= 1u && ncols > 0u) {
        // the last own row and the halo row, which lies elsewhere: one row block of two rows in memory
        CHK(buf_ensure(ctx, ctx->dnbr_blk, (size_t)2 * ncols * 4));
        uint32_t *blk = bp<uint32_t>(ctx->dnbr_blk);
        HIPCHK(ctx, hipMemcpyAsync(blk, d_seg + (size_t)(nrows - 1u) * ncols, (size_t)ncols * 4, hipMemcpyDeviceToDevice, st));
        if (d_halo) HIPCHK(ctx, hipMemcpyAsync(blk + ncols, d_halo, (size_t)ncols * 4, hipMemcpyDeviceToDevice, st));
        CHK(run_nbr_accumulate(ctx, blk, 1u, ncols, d_halo ? 1 : 0));
    }
    NbrState &s = ctx->nbr;
    s.open = false;                             // (neither accumulating nor a finished one-GPU table)
    *max_label_out = s.max_label;
    d.dev_ms = s.dev_ms;
    if (s.max_label > S) return 0;
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    uint32_t U = 0;
    CHK(nbr_sort_reduce<unsigned long long>(ctx, (const uint4 *)ctx->nbr_rec.p, (uint32_t)s.used, bits_for(S), &U));
    CHK(dnbr_pack(ctx, U, id_lo, id_hi, &d.nhome, &d.ntrav));
    nbr_ms(ctx);
    d.dev_ms = s.dev_ms;
    d.nlocal = U;
    d.stage = 1;
    counts_out[0] = (int64_t)d.nlocal;
    counts_out[1] = (int64_t)d.nhome;
    counts_out[2] = (int64_t)d.ntrav;
    *trav_out = d.ntrav ? ctx->dnbr_trav.p : nullptr;
    return 0;
}

// Step 3.  d_all: `world` blocks of `slot` records, counts[r] valid in block r (host).  d_cols: 2 (S + 1) int64 in
// device memory, numNeighbours then borderLength: zeroed here, the share's rows filled.
static int run_dnbr_merge(shp_ctx *ctx, const uint4 *d_all, unsigned long long slot, uint32_t world, const uint32_t *counts,
                          long long *d_cols, int64_t *picked_out, int64_t *nent_out)
{
    DNbrState &d = ctx->dnbr;
    NbrTable &t = ctx->dnbr_tab;
    hipStream_t st = ctx->stream;
    const uint32_t lo = t.row0, hi = lo + t.nrows;
    const size_t ns = (size_t)t.S + 1;
    const int bits = bits_for(t.S);
    unsigned long long valid = 0;
    for (uint32_t r = 0; r < world; r++) {
        if ((unsigned long long)counts[r] > slot) SHP_FAIL(ctx, SHP_ERR_ARG, "rank %u: %u records in a slot of %llu", r, counts[r], slot);
        valid += counts[r];
    }
    const unsigned long long cap = d.nhome + valid, total = slot * world;
    if (cap > NBR_MAX_REC || total > NBR_MAX_REC)
        SHP_FAIL(ctx, SHP_ERR_NOMEM, "%llu neighbour records: more than the sort indexes", cap > total ? cap : total);
    unsigned long long *ctr = (unsigned long long *)ctx->nbr_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    CHK(buf_ensure(ctx, ctx->dnbr_mrg, (size_t)cap * 16));
    uint4 *mrg = (uint4 *)ctx->dnbr_mrg.p;
    if (d.nhome)
        HIPCHK(ctx, hipMemcpyAsync(mrg, ctx->dnbr_home.p, (size_t)d.nhome * 16, hipMemcpyDeviceToDevice, st));
    unsigned long long n64 = d.nhome;
    if (valid) {
        CHK(buf_ensure(ctx, ctx->dnbr_rcnt, (size_t)world * 4));
        HIPCHK(ctx, hipMemcpyAsync(ctx->dnbr_rcnt.p, counts, (size_t)world * 4, hipMemcpyHostToDevice, st));
        pin[0] = d.nhome;
        HIPCHK(ctx, hipMemcpyAsync(ctr, pin, 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_dnbr_pick, dim3(grid_for(total, 256)), dim3(256), 0, st, d_all, slot, total,
                           (const uint32_t *)ctx->dnbr_rcnt.p, lo, hi, mrg, cap, ctr);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(pin, ctr, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        n64 = pin[0];
        if (n64 < d.nhome || n64 > cap) SHP_FAIL(ctx, SHP_ERR_STATE, "%llu records picked into room for %llu", n64, cap);
    }
    *picked_out = (int64_t)(n64 - d.nhome);
    uint32_t U = 0;
    CHK(nbr_sort_reduce<unsigned long long>(ctx, mrg, (uint32_t)n64, bits, &U));
    CHK(nbr_build_csr<true>(ctx, t, U, bits));
    HIPCHK(ctx, hipMemsetAsync(d_cols, 0, 2 * ns * 8, st));
    if (t.nrows) {
        hipLaunchKernelGGL(k_dnbr_columns, dim3(grid_for(t.nrows, 256)), dim3(256), 0, st, (const long long *)t.offs.p,
                           (const long long *)t.lens.p, t.nrows, lo, d_cols, d_cols + ns);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) d.dev_ms += ms;
    d.stage = 0;
    t.finished = true;
    *nent_out = (int64_t)t.nent;
    return 0;
}

// a share table from the host (the caller has checked it) becomes the context's share table, with a new serial
static int run_dnbr_upload(shp_ctx *ctx, const int64_t *offsets, const uint32_t *nbrs, const int64_t *lens, uint32_t S,
                           uint32_t id_lo, uint32_t id_hi, unsigned long long nent)
{
    NbrTable &t = ctx->dnbr_tab;
    ctx->dnbr = DNbrState{};
    nbr_table_end(t);
    t.row0 = id_lo;
    t.nrows = id_hi - id_lo;
    CHK(nbr_table_upload_arrays(ctx, t, offsets, nbrs, lens, nent));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    t.serial = nbr_next_serial();
    t.S = S;
    t.nent = nent;
    t.finished = true;
    return 0;
}

// Step 4: one column (host memory, S + 1 values) over the share table.  d_out: nsel (S + 1) 8-byte values in device
// memory, the selected statistics in the order of their bits: zeroed here, the share's rows written.
static int run_dnbr_reduce(shp_ctx *ctx, const void *col, int ctype, int has_ign, double ign, double missing,
                           uint32_t mask, void *d_out, double *dev_ms_out)
{
    NbrTable &t = ctx->dnbr_tab;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)t.S + 1;
    CHK(nbrr_stage_column(ctx, col, ctype, ns, nullptr));
    CHK(nbrr_long_ensure(ctx, t.longs, (const long long *)t.offs.p, t.nrows, t.serial));
    HIPCHK(ctx, hipMemsetAsync(d_out, 0, (size_t)nbrr_mask_count(mask) * ns * 8, st));
    if (t.nrows) CHK(nbrr_launch(ctx, nbrr_table_params(ctx, t, has_ign, ign, missing, d_out, mask), t.longs));
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return nbrr_dev_ms(ctx, dev_ms_out);
}
