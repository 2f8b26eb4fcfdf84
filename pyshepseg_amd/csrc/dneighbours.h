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
//     The records are sorted by (a, b) and run-length reduced (dnbr_sort_reduce: the steps of run_nbr_finish with
//     64-bit counts), so AT MOST ONE RECORD PER DISTINCT PAIR of a rank exists from here on.  k_dnbr_pack writes
//     them as 16-byte records in the patch kernel's layout (b, a, count low word, count high word) into two sets,
//     split by ballot and one atomic per wavefront and set: HOME (both ids in the rank's own share: nobody else
//     needs them) and TRAVELLING (everything else).
//  2. The caller all-gathers the travelling records, slot = the largest count over the ranks.
//  3. run_dnbr_merge.  k_dnbr_pick takes from the gathered blocks (every rank's valid count, not the slot) the
//     records with a or b in the share, behind a copy of the home records; they are sorted and reduced again (a pair
//     seen by several ranks adds up) and the CSR of the share is built as run_nbr_finish builds the whole table:
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
// The share table has buffers (dnbr_offs / dnbr_ids / dnbr_lens), a serial and a list of long rows of its own: it is
// not the context's "finished table" of shp_nbr_reduce, and neither displaces the other.  The local step does use the
// one-GPU accumulation (shp_nbr_begin's state), so it ends any one-GPU table of the context.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"
#include "neighbours.h"
#include "nbrreduce.h"

// b and the 64-bit count of every record in sorted order
__global__ __launch_bounds__(256) void k_dnbr_gather(const uint4 *__restrict__ rec, uint32_t n,
                                                     const uint32_t *__restrict__ idx, uint32_t *__restrict__ sb,
                                                     unsigned long long *__restrict__ sc)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint4 r = rec[idx[j]];
    sb[j] = r.x;
    sc[j] = ((unsigned long long)r.w << 32) | r.z;
}

// k_nbr_reduce with 64-bit counts: entry e = (heads before j) + head(j) - 1 gets (a, b) from its head and the sum
// of its records' counts; the records of an entry that share a wavefront add once
__global__ __launch_bounds__(256) void k_dnbr_reduce(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
                                                     const unsigned long long *__restrict__ sc,
                                                     const uint32_t *__restrict__ uidx, uint32_t n,
                                                     uint32_t *__restrict__ ua, uint32_t *__restrict__ ub,
                                                     unsigned long long *__restrict__ ucnt)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = lane_id();
    const bool in = j < n;
    const NbrHeadFn hf{sa, sb};
    const bool head = in && hf(j) != 0u;
    const uint32_t e = in ? uidx[j] + (head ? 1u : 0u) - 1u : 0u;
    unsigned long long incl = in ? sc[j] : 0ull;
    const unsigned long long own = incl;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)incl, d, 64), hi = __shfl_up((uint32_t)(incl >> 32), d, 64);
        if ((int)lane >= d) incl += ((unsigned long long)hi << 32) | lo;
    }
    const bool bd = lane == 0u || head || !in;
    const unsigned long long bound = __ballot(bd);
    const unsigned long long rest = lane == 63u ? 0ull : (bound >> (lane + 1u));
    const unsigned last = rest ? lane + (unsigned)__builtin_ctzll(rest) : 63u;
    const uint32_t llo = __shfl((uint32_t)incl, (int)last, 64), lhi = __shfl((uint32_t)(incl >> 32), (int)last, 64);
    if (!in) return;
    if (head) { ua[e] = sa[j]; ub[e] = sb[j]; }
    if (bd) atomicAdd(&ucnt[e], (((unsigned long long)lhi << 32) | llo) - (incl - own));
}

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

// cnt[key - lo] += how often key occurs in the SORTED keys, for the keys in [lo, hi): a run inside a wavefront adds once
__global__ __launch_bounds__(256) void k_dnbr_degree(const uint32_t *__restrict__ keys, uint32_t n, uint32_t lo,
                                                     uint32_t hi, uint32_t *__restrict__ cnt)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = lane_id();
    const bool in = j < n;
    const uint32_t k = in ? keys[j] : 0xffffffffu;
    const uint32_t pk = __shfl_up(k, 1, 64);
    const bool bd = lane == 0u || k != pk;
    const unsigned long long bound = __ballot(bd);
    if (!in || !bd || k < lo || k >= hi) return;
    const unsigned long long rest = lane == 63u ? 0ull : (bound >> (lane + 1u));
    atomicAdd(&cnt[k - lo], rest ? (uint32_t)__builtin_ctzll(rest) + 1u : 64u - lane);
}

// first[0] / first[1]: how many of the sorted keys ka / kb (n each) are below lo
__global__ void k_dnbr_bounds(const uint32_t *__restrict__ ka, const uint32_t *__restrict__ kb, uint32_t n, uint32_t lo,
                              uint32_t *__restrict__ first)
{
    if (blockIdx.x != 0u || threadIdx.x >= 2u) return;
    const uint32_t *k = threadIdx.x == 0u ? ka : kb;
    uint32_t a = 0u, b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2u;
        if (k[mid] < lo) a = mid + 1u; else b = mid;
    }
    first[threadIdx.x] = a;
}

// Rows are the ids lo + i.  Row i starts at hoff[i] + loff[i] and holds its lcnt[i] smaller neighbours first.  The
// reduced entries with a in the share start at first[0], so entry j = (a, b) is the (j - first[0] - hoff[i])-th larger
// neighbour of row i = a - lo: place hoff[i] + loff[i] + lcnt[i] + j - first[0] - hoff[i] = loff[i + 1] + j - first[0].
__global__ __launch_bounds__(256) void k_dnbr_fill_high(const uint32_t *__restrict__ ua, const uint32_t *__restrict__ ub,
                                                        const unsigned long long *__restrict__ ucnt, uint32_t U,
                                                        uint32_t lo, uint32_t hi, const uint32_t *__restrict__ first,
                                                        const uint32_t *__restrict__ loff, uint32_t *__restrict__ nbrs,
                                                        long long *__restrict__ lens)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= U) return;
    const uint32_t a = ua[j];
    if (a < lo || a >= hi) return;
    const size_t p = (size_t)loff[a - lo + 1u] + (j - first[0]);
    nbrs[p] = ub[j];
    lens[p] = (long long)ucnt[j];
}

// The q-th entry in the stable order by b (entry order[q], its b = skb[q]); those with b in the share start at
// first[1], so it is the (q - first[1] - loff[i])-th smaller neighbour of row i = b - lo: place hoff[i] + q - first[1].
__global__ __launch_bounds__(256) void k_dnbr_fill_low(const uint32_t *__restrict__ skb, const uint32_t *__restrict__ order,
                                                       const uint32_t *__restrict__ ua,
                                                       const unsigned long long *__restrict__ ucnt, uint32_t U,
                                                       uint32_t lo, uint32_t hi, const uint32_t *__restrict__ first,
                                                       const uint32_t *__restrict__ hoff, uint32_t *__restrict__ nbrs,
                                                       long long *__restrict__ lens)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= U) return;
    const uint32_t b = skb[q];
    if (b < lo || b >= hi) return;
    const uint32_t j = order[q];
    const size_t p = (size_t)hoff[b - lo] + (q - first[1]);
    nbrs[p] = ua[j];
    lens[p] = (long long)ucnt[j];
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
// n records (b, a, count low, count high) sorted by (a, b) and run-length reduced with 64-bit sums: *U_out distinct
// pairs in nbr_ua / nbr_ub / nbr_ucnt.  The steps of run_nbr_finish up to k_nbr_reduce.
static int dnbr_sort_reduce(shp_ctx *ctx, const uint4 *rec, uint32_t n, int bits, uint32_t *U_out)
{
    hipStream_t st = ctx->stream;
    *U_out = 0u;
    if (n == 0u) return 0;
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_NBR;
    CHK(buf_ensure(ctx, ctx->nbr_key, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->nbr_val, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->nbr_uidx, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->dnbr_cnt, (size_t)n * 8));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(n)));
    uint32_t *key = bp<uint32_t>(ctx->nbr_key), *val = bp<uint32_t>(ctx->nbr_val), *uidx = bp<uint32_t>(ctx->nbr_uidx);
    unsigned long long *sc = (unsigned long long *)ctx->dnbr_cnt.p;
    const unsigned gn = grid_for(n, 256);
    uint32_t *ord = nullptr, *sa = nullptr;
    hipLaunchKernelGGL(k_nbr_field, dim3(gn), dim3(256), 0, st, rec, n, 0, (const uint32_t *)nullptr, key, (uint32_t *)nullptr);
    KCHK(ctx);
    CHK(sort_pairs(ctx, key, nullptr, n, bits, nullptr, &ord, true));
    hipLaunchKernelGGL(k_nbr_field, dim3(gn), dim3(256), 0, st, rec, n, 1, (const uint32_t *)ord, key, val);
    KCHK(ctx);
    CHK(sort_pairs(ctx, key, val, n, bits, &sa, &ord, true));
    uint32_t *sb = key;                         // (the sort has read it)
    hipLaunchKernelGGL(k_dnbr_gather, dim3(gn), dim3(256), 0, st, rec, n, (const uint32_t *)ord, sb, sc);
    KCHK(ctx);
    NbrHeadFn hf{sa, sb};
    CHK(scan_exclusive(ctx, hf, n, uidx, nullptr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t U = *(volatile uint32_t *)mir;
    if (U < 1u || U > n) SHP_FAIL(ctx, SHP_ERR_STATE, "%u distinct pairs out of %u records", U, n);
    CHK(buf_ensure(ctx, ctx->nbr_ua, (size_t)U * 4));
    CHK(buf_ensure(ctx, ctx->nbr_ub, (size_t)U * 4));
    CHK(buf_ensure(ctx, ctx->nbr_ucnt, (size_t)U * 8));
    HIPCHK(ctx, hipMemsetAsync(ctx->nbr_ucnt.p, 0, (size_t)U * 8, st));
    hipLaunchKernelGGL(k_dnbr_reduce, dim3(gn), dim3(256), 0, st, (const uint32_t *)sa, (const uint32_t *)sb,
                       (const unsigned long long *)sc, (const uint32_t *)uidx, n, bp<uint32_t>(ctx->nbr_ua),
                       bp<uint32_t>(ctx->nbr_ub), (unsigned long long *)ctx->nbr_ucnt.p);
    KCHK(ctx);
    *U_out = U;
    return 0;
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
    const unsigned long long list_serial = d.list_serial;
    d = DNbrState{};
    d.list_serial = list_serial;                // (of a table that is gone: no serial to come equals it)
    counts_out[0] = counts_out[1] = counts_out[2] = 0;
    *trav_out = nullptr;
    CHK(run_nbr_begin(ctx, (int64_t)S, four_connected));
    d.serial = nbr_next_serial();
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
    s.stage = 0;                                // (neither accumulating nor a finished one-GPU table)
    *max_label_out = s.max_label;
    d.dev_ms = s.dev_ms;
    if (s.max_label > S) return 0;
    const uint32_t n = (uint32_t)s.used;
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    uint32_t U = 0;
    CHK(dnbr_sort_reduce(ctx, (const uint4 *)ctx->nbr_rec.p, n, bits_for(S), &U));
    unsigned long long *ctr = (unsigned long long *)ctx->nbr_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    pin[0] = pin[1] = 0ull;
    if (U) {
        CHK(buf_ensure(ctx, ctx->dnbr_home, (size_t)U * 16));
        CHK(buf_ensure(ctx, ctx->dnbr_trav, (size_t)U * 16));
        HIPCHK(ctx, hipMemsetAsync(ctr, 0, 16, st));
        hipLaunchKernelGGL(k_dnbr_pack, dim3(grid_for(U, 256)), dim3(256), 0, st, (const uint32_t *)ctx->nbr_ua.p,
                           (const uint32_t *)ctx->nbr_ub.p, (const unsigned long long *)ctx->nbr_ucnt.p, U, id_lo, id_hi,
                           (uint4 *)ctx->dnbr_home.p, (uint4 *)ctx->dnbr_trav.p, ctr);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(pin, ctr, 16, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    nbr_ms(ctx);
    d.dev_ms = s.dev_ms;
    if (pin[0] + pin[1] != (unsigned long long)U)
        SHP_FAIL(ctx, SHP_ERR_STATE, "%llu home and %llu travelling records for %u pairs", pin[0], pin[1], U);
    d.S = S;
    d.id_lo = id_lo;
    d.id_hi = id_hi;
    d.nlocal = U;
    d.nhome = pin[0];
    d.ntrav = pin[1];
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
    hipStream_t st = ctx->stream;
    const uint32_t S = d.S, lo = d.id_lo, hi = d.id_hi, nsh = hi - lo;
    const size_t ns = (size_t)S + 1;
    const int bits = bits_for(S);
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
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_NBR;
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
    CHK(dnbr_sort_reduce(ctx, mrg, (uint32_t)n64, bits, &U));
    const uint32_t *ua = bp<uint32_t>(ctx->nbr_ua), *ub = bp<uint32_t>(ctx->nbr_ub);
    const unsigned long long *ucnt = (const unsigned long long *)ctx->nbr_ucnt.p;
    // degrees of the share's rows at both ends, their scans, the two fills
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes((size_t)nsh + 1)));
    CHK(buf_ensure(ctx, ctx->nbr_deg, (size_t)2 * nsh * 4));
    CHK(buf_ensure(ctx, ctx->nbr_hoff, ((size_t)nsh + 1) * 4));
    CHK(buf_ensure(ctx, ctx->nbr_loff, ((size_t)nsh + 1) * 4));
    CHK(buf_ensure(ctx, ctx->dnbr_offs, ((size_t)nsh + 1) * 8));
    uint32_t *hcnt = bp<uint32_t>(ctx->nbr_deg), *lcnt = hcnt + nsh;
    uint32_t *hoff = bp<uint32_t>(ctx->nbr_hoff), *loff = bp<uint32_t>(ctx->nbr_loff);
    uint32_t *first = (uint32_t *)(ctr + 2);
    if (nsh) HIPCHK(ctx, hipMemsetAsync(hcnt, 0, (size_t)2 * nsh * 4, st));
    uint32_t *skb = nullptr, *ordb = nullptr;
    const unsigned gu = grid_for(U, 256);
    if (U && nsh) {
        hipLaunchKernelGGL(k_dnbr_degree, dim3(gu), dim3(256), 0, st, ua, U, lo, hi, hcnt);
        KCHK(ctx);
        CHK(sort_pairs(ctx, ub, nullptr, U, bits, &skb, &ordb, true));
        hipLaunchKernelGGL(k_dnbr_degree, dim3(gu), dim3(256), 0, st, (const uint32_t *)skb, U, lo, hi, lcnt);
        KCHK(ctx);
        hipLaunchKernelGGL(k_dnbr_bounds, dim3(1), dim3(64), 0, st, ua, (const uint32_t *)skb, U, lo, first);
        KCHK(ctx);
    }
    ArrFn fh{hcnt}, fl{lcnt};
    CHK(scan_exclusive(ctx, fh, nsh, hoff, hoff + nsh, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 1));
    CHK(scan_exclusive(ctx, fl, nsh, loff, loff + nsh, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 2));
    hipLaunchKernelGGL(k_nbr_offsets, dim3(grid_for((size_t)nsh + 1, 256)), dim3(256), 0, st, (const uint32_t *)hoff,
                       (const uint32_t *)loff, nsh + 1u, (long long *)ctx->dnbr_offs.p);
    KCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t th = *(volatile uint32_t *)(mir + 1), tl = *(volatile uint32_t *)(mir + 2);
    if (th > U || tl > U) SHP_FAIL(ctx, SHP_ERR_STATE, "degrees sum to %u and %u for %u pairs", th, tl, U);
    const unsigned long long nent = (unsigned long long)th + tl;
    CHK(buf_ensure(ctx, ctx->dnbr_ids, (size_t)nent * 4));
    CHK(buf_ensure(ctx, ctx->dnbr_lens, (size_t)nent * 8));
    if (nent) {
        hipLaunchKernelGGL(k_dnbr_fill_high, dim3(gu), dim3(256), 0, st, ua, ub, ucnt, U, lo, hi, (const uint32_t *)first,
                           (const uint32_t *)loff, bp<uint32_t>(ctx->dnbr_ids), (long long *)ctx->dnbr_lens.p);
        KCHK(ctx);
        hipLaunchKernelGGL(k_dnbr_fill_low, dim3(gu), dim3(256), 0, st, (const uint32_t *)skb, (const uint32_t *)ordb, ua,
                           ucnt, U, lo, hi, (const uint32_t *)first, (const uint32_t *)hoff, bp<uint32_t>(ctx->dnbr_ids),
                           (long long *)ctx->dnbr_lens.p);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipMemsetAsync(d_cols, 0, 2 * ns * 8, st));
    if (nsh) {
        hipLaunchKernelGGL(k_dnbr_columns, dim3(grid_for(nsh, 256)), dim3(256), 0, st, (const long long *)ctx->dnbr_offs.p,
                           (const long long *)ctx->dnbr_lens.p, nsh, lo, d_cols, d_cols + ns);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) d.dev_ms += ms;
    d.nent = nent;
    d.stage = 2;
    *nent_out = (int64_t)nent;
    return 0;
}

static int run_dnbr_download(shp_ctx *ctx, int64_t *offsets, uint32_t *nbrs, int64_t *lens)
{
    const DNbrState &d = ctx->dnbr;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(offsets, ctx->dnbr_offs.p, ((size_t)(d.id_hi - d.id_lo) + 1) * 8, hipMemcpyDeviceToHost, st));
    if (d.nent) {
        HIPCHK(ctx, hipMemcpyAsync(nbrs, ctx->dnbr_ids.p, (size_t)d.nent * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(lens, ctx->dnbr_lens.p, (size_t)d.nent * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// a share table from the host (the caller has checked it) becomes the context's share table, with a new serial
static int run_dnbr_upload(shp_ctx *ctx, const int64_t *offsets, const uint32_t *nbrs, const int64_t *lens, uint32_t S,
                           uint32_t id_lo, uint32_t id_hi, unsigned long long nent)
{
    DNbrState &d = ctx->dnbr;
    hipStream_t st = ctx->stream;
    const unsigned long long list_serial = d.list_serial;
    d = DNbrState{};
    d.list_serial = list_serial;
    const size_t nsh = (size_t)(id_hi - id_lo);
    CHK(buf_ensure(ctx, ctx->dnbr_offs, (nsh + 1) * 8));
    CHK(buf_ensure(ctx, ctx->dnbr_ids, (size_t)nent * 4));
    CHK(buf_ensure(ctx, ctx->dnbr_lens, (size_t)nent * 8));
    HIPCHK(ctx, hipMemcpyAsync(ctx->dnbr_offs.p, offsets, (nsh + 1) * 8, hipMemcpyHostToDevice, st));
    if (nent) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->dnbr_ids.p, nbrs, (size_t)nent * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->dnbr_lens.p, lens, (size_t)nent * 8, hipMemcpyHostToDevice, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    d.serial = nbr_next_serial();
    d.S = S;
    d.id_lo = id_lo;
    d.id_hi = id_hi;
    d.nent = nent;
    d.stage = 2;
    return 0;
}

// Step 4: one column (host memory, S + 1 values) over the share table.  d_out: nsel (S + 1) 8-byte values in device
// memory, the selected statistics in the order of their bits: zeroed here, the share's rows written.
static int run_dnbr_reduce(shp_ctx *ctx, const void *col, int ctype, int has_ign, double ign, double missing,
                           uint32_t mask, void *d_out, double *dev_ms_out)
{
    DNbrState &d = ctx->dnbr;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)d.S + 1;
    const uint32_t nsh = d.id_hi - d.id_lo;
    int nsel = 0;
    for (int i = 0; i < NBRR_NSTATS; i++) nsel += (mask >> i) & 1u;
    CHK(buf_ensure(ctx, ctx->nbrr_col, ns * 8));
    double *d_col = bp<double>(ctx->nbrr_col);
    const void *d_raw = nullptr;
    if (ctype == COL_F64) {
        HIPCHK(ctx, hipMemcpyAsync(d_col, col, ns * 8, hipMemcpyHostToDevice, st));
    } else {
        const size_t bytes = ns * (ctype == COL_F32 ? 4 : 8);
        CHK(buf_ensure(ctx, ctx->img, bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->img.p, col, bytes, hipMemcpyHostToDevice, st));
        d_raw = ctx->img.p;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (d.list_serial != d.serial) {
        CHK(nbrr_long_list_of(ctx, (const long long *)ctx->dnbr_offs.p, nsh, ctx->dnbr_lrow, ctx->dnbr_lcoff, &d.nlong,
                              &d.nchunks));
        d.list_serial = d.serial;
    }
    if (ctype == COL_F32) {
        hipLaunchKernelGGL(k_col_from_f32, dim3(colour_grid(ns, 256)), dim3(256), 0, st, (const float *)d_raw, ns, d_col);
        KCHK(ctx);
    } else if (ctype == COL_I64) {
        hipLaunchKernelGGL(k_nbrr_from_i64, dim3(colour_grid(ns, 256)), dim3(256), 0, st, (const long long *)d_raw, ns, d_col);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipMemsetAsync(d_out, 0, (size_t)nsel * ns * 8, st));
    NbrrParams p;
    p.offs = (const long long *)ctx->dnbr_offs.p;
    p.ids = (const uint32_t *)ctx->dnbr_ids.p;
    p.lens = (const long long *)ctx->dnbr_lens.p;
    p.col = d_col;
    p.ns = nsh;
    p.row0 = d.id_lo;
    p.has_ign = has_ign;
    p.ign = ign;
    p.missing = missing;
    int slot = 0;
    for (int i = 0; i < NBRR_NSTATS; i++)
        p.out[i] = ((mask >> i) & 1u) ? (void *)((char *)d_out + (size_t)(slot++) * ns * 8) : nullptr;
    if (nsh) CHK(nbrr_launch(ctx, p, bp<uint32_t>(ctx->dnbr_lrow), bp<uint32_t>(ctx->dnbr_lcoff), d.nlong, d.nchunks));
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (dev_ms_out) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        *dev_ms_out = ms;
    }
    return 0;
}
