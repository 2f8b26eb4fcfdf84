// dsegshape.h -- the shape table (segshape.h) of a label raster that lies sharded by rows over the ranks
// (dist_shapes.deviceShapes).  Every rank accumulates its own rows into a table of all ids, with the raster's row
// above and below them from the halo gather (shp_shape_accumulate_halo_dev); what this file adds are the two steps
// around the exchange.  All of it is integer add / min / max, so neither the order of the records nor the number of
// ranks can change a bit.
//
//  1. k_dshape_count, k_dshape_pack (shp_dshape_local_dev): over the ids 1 .. S with the raster's histogram, l the
//     id's area in this rank's table:
//       l == hist[id]       the id is whole here, its row stays;
//       0 < l < hist[id]    a straddler: its row leaves as a record of DSHAPE_REC_WORDS 64-bit words (the id, then the
//                           row's eleven words: 96 bytes, so records stay 16-byte aligned) and becomes empty;
//       l > hist[id]        the histogram does not belong to these labels: counted, reported by the host.
//     The count runs first so that the record buffer is sized to the straddlers, not to S.  A wavefront takes its
//     record slots with ONE atomic for its ballot (and one for the ids above their histogram), not one per id.
//  2. k_dshape_fold (shp_dshape_merge_dev): over the gathered records of all ranks (slot records per rank, the first
//     counts[r] of rank r valid), a group of 16 lanes per record and a lane per word, as k_shape_patch's flush (whose
//     measurement of that form against a thread per row is in segshape.h's header).  A record whose id lies in this
//     rank's id share [lo, hi) is folded into the id's row -- empty here whether or not this rank sent a record of
//     it -- with 64-bit atomic adds for the nine sums and counts and 32-bit atomic min / max for the four extents.
//     The first record of an id finds the area 0, which counts the share's distinct straddlers.
//     Then k_shape_finish (extents of empty rows become 0) and k_dshape_check: an id of the share whose area is
//     neither 0 nor hist[id] is counted -- the histogram is not that of the raster.
// After step 2 an id's row is non-zero on at most one rank: one integer all-reduce of the (S + 1) x 11 words completes
// the table on every rank, the packed extent words included.
#pragma once
#include "segshape.h"

#define DSHAPE_REC_WORDS 12u    // 64-bit words of a record: the id, then SHAPE_WORDS of its row
static_assert(DSHAPE_REC_WORDS == SHAPE_WORDS + 1u && (DSHAPE_REC_WORDS * 8u) % 16u == 0u, "a record is the id and the row");

// counters of a call: DSHAPE_NREC records (counted, then the slots handed out), DSHAPE_OVER ids above their histogram,
// DSHAPE_PICKED records folded, DSHAPE_IDS distinct ids folded, DSHAPE_WRONG ids of the share with another area
enum { DSHAPE_NREC = 0, DSHAPE_OVER = 1, DSHAPE_PICKED = 2, DSHAPE_IDS = 3, DSHAPE_WRONG = 4, DSHAPE_SLOTS = 5, DSHAPE_NCTR = 6 };

// ctr[DSHAPE_NREC] += straddlers, ctr[DSHAPE_OVER] += ids with more pixels here than the histogram gives them
__global__ __launch_bounds__(256) void k_dshape_count(const unsigned long long *__restrict__ tab, const uint32_t *__restrict__ hist,
                                                      size_t nids, unsigned long long *__restrict__ ctr)
{
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x + 1u;
    unsigned long long l = 0ull, h = 0ull;
    if (id < nids) { l = tab[id * SHAPE_WORDS + SHAPE_AREA]; h = hist[id]; }
    const unsigned long long strad = __ballot(l > 0ull && l < h), over = __ballot(l > h);
    if (lane_id() == 0u) {
        if (strad) atomicAdd(&ctr[DSHAPE_NREC], (unsigned long long)__popcll(strad));
        if (over) atomicAdd(&ctr[DSHAPE_OVER], (unsigned long long)__popcll(over));
    }
}

// the straddlers' rows into rec (room for cap records), the rows emptied; ctr[DSHAPE_SLOTS]: slots handed out
__global__ __launch_bounds__(256) void k_dshape_pack(unsigned long long *__restrict__ tab, const uint32_t *__restrict__ hist,
                                                     size_t nids, unsigned long long *__restrict__ rec, unsigned long long cap,
                                                     unsigned long long *__restrict__ ctr)
{
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x + 1u;
    unsigned long long l = 0ull, h = 0ull;
    if (id < nids) { l = tab[id * SHAPE_WORDS + SHAPE_AREA]; h = hist[id]; }
    const bool strad = l > 0ull && l < h;
    const unsigned long long b = __ballot(strad);
    if (b == 0ull) return;                              // (uniform in the wavefront)
    const unsigned lane = lane_id();
    unsigned long long base = 0ull;
    if (lane == 0u) base = atomicAdd(&ctr[DSHAPE_SLOTS], (unsigned long long)__popcll(b));
    base = __shfl(base, 0, 64);
    if (!strad) return;
    const unsigned long long at = base + (unsigned long long)__popcll(b & ((1ull << lane) - 1ull));
    if (at >= cap) return;                              // (the table changed since the count: the host compares the two)
    unsigned long long *row = tab + id * SHAPE_WORDS;
    unsigned long long *out = rec + at * DSHAPE_REC_WORDS;
    out[0] = (unsigned long long)id;
#pragma unroll
    for (unsigned k = 0; k < SHAPE_WORDS; k++) {
        out[1u + k] = row[k];
        row[k] = k >= SHAPE_ROWEXT ? 0xffffffffull : 0ull;
    }
}

// all: world blocks of slot records, the first counts[r] of block r valid; total = slot * world
__global__ __launch_bounds__(256) void k_dshape_fold(const unsigned long long *__restrict__ all, unsigned long long slot,
                                                     unsigned long long total, const uint32_t *__restrict__ counts, uint32_t lo,
                                                     uint32_t hi, uint32_t S, unsigned long long *__restrict__ tab,
                                                     unsigned long long *__restrict__ ctr)
{
    const unsigned long long q = ((unsigned long long)blockIdx.x * 256u + threadIdx.x) >> 4;
    const uint32_t f = threadIdx.x & 15u;
    bool mine = false, first = false;
    if (q < total) {
        const unsigned long long r = q / slot, i = q - r * slot;
        if (i < (unsigned long long)counts[r]) {
            const unsigned long long *rec = all + q * DSHAPE_REC_WORDS;
            const unsigned long long id = rec[0];
            // (an id outside 1 .. S is no record of this library's: never an index)
            if (id >= 1ull && id <= (unsigned long long)S && id >= (unsigned long long)lo && id < (unsigned long long)hi) {
                unsigned long long *row = tab + (size_t)id * SHAPE_WORDS;
                mine = f == 0u;
                if (f < SHAPE_ROWEXT) {
                    const unsigned long long v = rec[1u + f];
                    if (v) {
                        const unsigned long long old = atomicAdd(row + f, v);
                        first = f == SHAPE_AREA && old == 0ull;
                    }
                } else if (f < SHAPE_ROWEXT + 4u) {
                    const uint32_t e = f - SHAPE_ROWEXT;            // rowMin, rowMax, colMin, colMax
                    const uint32_t v = (uint32_t)(rec[1u + SHAPE_ROWEXT + (e >> 1)] >> (32u * (e & 1u)));
                    uint32_t *ext = (uint32_t *)(row + SHAPE_ROWEXT) + e;
                    if (e & 1u) atomicMax(ext, v); else atomicMin(ext, v);
                }
            }
        }
    }
    const unsigned long long bm = __ballot(mine), bf = __ballot(first);
    if (lane_id() == 0u) {
        if (bm) atomicAdd(&ctr[DSHAPE_PICKED], (unsigned long long)__popcll(bm));
        if (bf) atomicAdd(&ctr[DSHAPE_IDS], (unsigned long long)__popcll(bf));
    }
}

// ctr[DSHAPE_WRONG] += ids of [lo, hi) (lo >= 1) whose area is neither 0 nor the histogram's
__global__ __launch_bounds__(256) void k_dshape_check(const unsigned long long *__restrict__ tab, const uint32_t *__restrict__ hist,
                                                      size_t lo, size_t hi, unsigned long long *__restrict__ ctr)
{
    const size_t id = lo + (size_t)blockIdx.x * 256u + threadIdx.x;
    bool wrong = false;
    if (id < hi) {
        const unsigned long long a = tab[id * SHAPE_WORDS + SHAPE_AREA];
        wrong = a != 0ull && a != (unsigned long long)hist[id];
    }
    const unsigned long long b = __ballot(wrong);
    if (b && lane_id() == 0u) atomicAdd(&ctr[DSHAPE_WRONG], (unsigned long long)__popcll(b));
}

// ---- host side --------------------------------------------------------------------------------------------
// *max_label_out: the largest label above S in this rank's rows, 0 when there is none -- then counts_out[0] records
// lie at *d_records_out, and counts_out[1] ids have more pixels here than d_hist gives them
static int run_dshape_local(shp_ctx *ctx, const uint32_t *d_hist, uint32_t *max_label_out, int64_t *counts_out,
                            void **d_records_out)
{
    ShapeState &s = ctx->shape;
    hipStream_t st = ctx->stream;
    const size_t nids = (size_t)s.S + 1;
    counts_out[0] = counts_out[1] = 0;
    *d_records_out = nullptr;
    CHK(buf_ensure(ctx, ctx->dshape_ctr, DSHAPE_NCTR * 8));
    unsigned long long *ctr = (unsigned long long *)ctx->dshape_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctx->shape_ctr.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    *max_label_out = *(volatile uint32_t *)ctx->h_pinned;
    s.nrec = 0;
    if (*max_label_out) {               // (such labels were never looked up: there is no table to classify)
        s.stage = 0;
        return 0;
    }
    HIPCHK(ctx, hipMemsetAsync(ctr, 0, DSHAPE_NCTR * 8, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (s.S) {
        hipLaunchKernelGGL(k_dshape_count, dim3(grid_for(s.S, 256)), dim3(256), 0, st, (const unsigned long long *)ctx->shape_tab.p,
                           d_hist, nids, ctr);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(pin, ctr, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    shape_ms(ctx);
    const unsigned long long nrec = pin[DSHAPE_NREC], over = pin[DSHAPE_OVER];
    if (nrec > (unsigned long long)s.S) SHP_FAIL(ctx, SHP_ERR_STATE, "%llu straddlers among %u ids", nrec, s.S);
    if (nrec) {
        CHK(buf_ensure(ctx, ctx->dshape_rec, (size_t)nrec * DSHAPE_REC_WORDS * 8));
        HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
        hipLaunchKernelGGL(k_dshape_pack, dim3(grid_for(s.S, 256)), dim3(256), 0, st, (unsigned long long *)ctx->shape_tab.p, d_hist,
                           nids, (unsigned long long *)ctx->dshape_rec.p, nrec, ctr);
        KCHK(ctx);
        HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
        HIPCHK(ctx, hipMemcpyAsync(pin, ctr + DSHAPE_SLOTS, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        shape_ms(ctx);
        if (pin[0] != nrec) SHP_FAIL(ctx, SHP_ERR_STATE, "%llu records packed, %llu counted", pin[0], nrec);
        *d_records_out = ctx->dshape_rec.p;
    }
    s.nrec = nrec;
    s.stage = 3;
    counts_out[0] = (int64_t)nrec;
    counts_out[1] = (int64_t)over;
    return 0;
}

// counts_out: records folded, distinct ids folded, ids of the share whose area is not the histogram's; the table is
// finished (shp_shape_download) and lies at *d_table_out, (S + 1) x SHAPE_WORDS words
static int run_dshape_merge(shp_ctx *ctx, const unsigned long long *d_all, unsigned long long slot, uint32_t world,
                            const uint32_t *counts, const uint32_t *d_hist, uint32_t lo, uint32_t hi, int64_t *counts_out,
                            void **d_table_out)
{
    ShapeState &s = ctx->shape;
    hipStream_t st = ctx->stream;
    const size_t nids = (size_t)s.S + 1;
    unsigned long long *ctr = (unsigned long long *)ctx->dshape_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    unsigned long long *tab = (unsigned long long *)ctx->shape_tab.p;
    unsigned long long valid = 0;
    for (uint32_t r = 0; r < world; r++) {
        if ((unsigned long long)counts[r] > slot) SHP_FAIL(ctx, SHP_ERR_ARG, "rank %u: %u records in a slot of %llu", r, counts[r], slot);
        valid += counts[r];
    }
    const unsigned long long total = slot * world;
    // (k_dshape_fold: a workgroup per 16 records, no grid stride)
    if (total > 0x7fffffffull * 16ull) SHP_FAIL(ctx, SHP_ERR_ARG, "%llu gathered records", total);
    if (valid) {
        CHK(buf_ensure(ctx, ctx->dshape_rcnt, (size_t)world * 4));
        HIPCHK(ctx, hipMemcpyAsync(ctx->dshape_rcnt.p, counts, (size_t)world * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (valid) {
        hipLaunchKernelGGL(k_dshape_fold, dim3(grid_for(total * 16ull, 256)), dim3(256), 0, st, d_all, slot, total,
                           (const uint32_t *)ctx->dshape_rcnt.p, lo, hi, s.S, tab, ctr);
        KCHK(ctx);
    }
    hipLaunchKernelGGL(k_shape_finish, dim3(grid_for(nids, 256, 16384u)), dim3(256), 0, st, tab, nids);
    KCHK(ctx);
    const size_t clo = lo < 1u ? 1u : lo;
    if ((size_t)hi > clo) {
        hipLaunchKernelGGL(k_dshape_check, dim3(grid_for((size_t)hi - clo, 256)), dim3(256), 0, st, (const unsigned long long *)tab,
                           d_hist, clo, (size_t)hi, ctr);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(pin, ctr, DSHAPE_NCTR * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    shape_ms(ctx);
    counts_out[0] = (int64_t)pin[DSHAPE_PICKED];
    counts_out[1] = (int64_t)pin[DSHAPE_IDS];
    counts_out[2] = (int64_t)pin[DSHAPE_WRONG];
    *d_table_out = tab;
    s.stage = 2;
    return 0;
}
