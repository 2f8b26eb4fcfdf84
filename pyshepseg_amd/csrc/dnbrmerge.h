// dnbrmerge.h -- the merges of nbrmerge.h (neighbours.mergeSegments / mergeSimilarSegments) over the neighbour table
// that dneighbours.h left sharded by id over the ranks (distributed.mergeSegmentsDistributed /
// mergeSimilarSegmentsDistributed): the groups on every rank, the contracted table sharded by the new ids.
//
// Links, groups, numbering, recode and the contracted table are those of nbrmerge.h.  All of it is integer work
// except d2 of the similarity rule, which is a function of the two ids' records alone; so nothing depends on which
// rank holds an entry, or on the order of the atomics.
//
//  1. run_dmrg_begin / run_dmrg_hook.  Row i of the share table is id id_lo + i (NbrTable::row0; mrg_table of
//     nbrmerge.h makes the kernels' view of either table), so the entries
//     a < b of a rank's rows are owned by that rank alone and every such entry of the whole table has one owner.
//     k_mrg_hook and k_mrgs_best run over them as they run over the one-GPU table, into a parent array of ALL ids
//     (S + 1) from the full key / size / distance columns.  The mutual rule needs best[b] of ids of other shares:
//     k_dmrg_pack_best writes best + 1 of the share's rows into an int64 column that is 0 elsewhere, one integer
//     all-reduce (the caller's) completes it and k_dmrg_unpack_best turns it back into the uint32 best before the
//     hook.  d2(a, b) and d2(b, a) have the same bits, so the two owners of a pair's rows see the same candidates.
//  2. The forest exchange.  After the local flatten k_dmrg_pairs compacts one 8-byte pair (i, root[i]) for every id
//     with root[i] != i: ballots and one atomic per wavefront of 1024 ids, first counted, then written into a buffer
//     of that size.  Their number is a function of the rank's links alone (the ids that are not the smallest of
//     their local component); their order is not, and does not matter.  The caller all-gathers them, slot = the
//     largest count.  k_dmrg_hook_pairs hooks the OTHER ranks' valid pairs into the rank's own parent array with
//     mrg_union (agent-scope loads and atomics only, as nbrmerge.h explains), a workgroup per MRG_PIECE pairs.
//     The union of all ranks' forests has the components of all links, so after mrg_number's flatten root[i] is
//     the smallest id of i's global component on every rank.
//  3. run_dmrg_number: mrg_number unchanged, redundantly on every rank; the groups lie where shp_nbr_merge leaves
//     them (ctx->mrg, mrg_recode / mrg_rep / mrg_gsize / mrg_hist), so the calls that read them serve as they are.
//  4. run_dmrg_records: k_mrg_records over the share's entries a < b; the records are sorted and reduced to distinct
//     pairs (nbr_sort_reduce) and split into home and travelling records against the NEW share of the ids 0 .. M
//     (dnbr_pack), the two routines of run_dnbr_local.  That is the state run_dnbr_local leaves (DNbrState stage 1,
//     the new share waiting in shp_ctx::dnbr_tab), so the caller's all-gather and run_dnbr_merge build the new share
//     table and its two columns as they build the first one.
#pragma once
#include "common.h"
#include "nbrmerge.h"
#include "dneighbours.h"

// more device words of a merge (ctx->mrg_ctr, behind MRG_C_BAD): forest pairs counted, forest pairs placed, gathered
// pairs that name an id outside 1 .. S
enum { DMRG_C_NPAIR = 5, DMRG_C_PLACE = 6, DMRG_C_BADPAIR = 7 };
static_assert(DMRG_C_BADPAIR < MRG_C_WORDS, "the merge's counters hold the forest exchange's");

// b64[lo + i] = best[lo + i] + 1 for the n rows of the share (b64 is zero elsewhere)
__global__ __launch_bounds__(256) void k_dmrg_pack_best(const uint32_t *__restrict__ best, uint32_t lo, uint32_t n,
                                                        long long *__restrict__ b64)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) b64[(size_t)lo + i] = (long long)best[(size_t)lo + i] + 1;
}

// best[i] = b64[i] - 1 (an id no rank wrote: none)
__global__ __launch_bounds__(256) void k_dmrg_unpack_best(const long long *__restrict__ b64, uint32_t ns,
                                                          uint32_t *__restrict__ best)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= ns) return;
    const long long v = b64[i];
    best[i] = (v >= 1 && v <= 0x100000000ll) ? (uint32_t)(v - 1) : 0xffffffffu;
}

// the ids that are not the root of their component, as pairs (i, root[i]).  A wavefront takes DMRG_WAVE_IDS
// consecutive ids, 64 at a time, and makes ONE atomic for all of them (a wavefront per 64 ids would queue a sixteenth
// of a million adds on one word per million ids).  WRITE false: counted into ctr[NPAIR]; WRITE true: the wavefront
// counts its pairs, reserves them at ctr[PLACE] and goes over its ids again to place them; room for cap pairs.
#define DMRG_WAVE_IDS 1024u
template <bool WRITE>
__global__ __launch_bounds__(256) void k_dmrg_pairs(const uint32_t *__restrict__ root, uint32_t ns, uint2 *__restrict__ out,
                                                    unsigned long long cap, unsigned long long *__restrict__ ctr)
{
    const unsigned lane = lane_id();
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * 4ull + threadIdx.x / 64u) * DMRG_WAVE_IDS;
    uint32_t n = 0u;
    for (uint32_t k = 0; k < DMRG_WAVE_IDS; k += 64u) {                     // (uniform in the wavefront)
        const unsigned long long i = i0 + k + lane;
        const bool take = i < ns && root[i] != (uint32_t)i;
        n += (uint32_t)__popcll(__ballot(take));
    }
    if (n == 0u) return;
    if (!WRITE) {
        if (lane == 0u) atomicAdd(&ctr[DMRG_C_NPAIR], (unsigned long long)n);
        return;
    }
    unsigned long long base = 0ull;
    if (lane == 0u) base = atomicAdd(&ctr[DMRG_C_PLACE], (unsigned long long)n);
    base = (unsigned long long)__shfl((long long)base, 0, 64);
    for (uint32_t k = 0; k < DMRG_WAVE_IDS; k += 64u) {
        const unsigned long long i = i0 + k + lane;
        const uint32_t r = i < ns ? root[i] : 0u;
        const bool take = i < ns && r != (uint32_t)i;
        const unsigned long long m = __ballot(take);
        const unsigned long long p = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (take && p < cap) out[p] = make_uint2((uint32_t)i, r);
        base += (unsigned long long)__popcll(m);
    }
}

// `world` gathered blocks of `slot` pairs, block r holding counts[r] valid ones: those of the blocks other than
// `skip` are hooked into par (ns ids).  A pair that names id 0 or an id past the table is counted, not hooked.
__global__ __launch_bounds__(256) void k_dmrg_hook_pairs(const uint2 *__restrict__ all, unsigned long long slot,
                                                         unsigned long long total, const uint32_t *__restrict__ counts,
                                                         uint32_t skip, uint32_t ns, uint32_t *par, unsigned long long *ctr)
{
    const unsigned long long i0 = (unsigned long long)blockIdx.x * MRG_PIECE;
    for (uint32_t k = 0; k < MRG_PIECE / 256u; k++) {
        const unsigned long long i = i0 + (k * 256u + threadIdx.x);
        if (i >= total) break;
        const unsigned long long blk = i / slot, j = i - blk * slot;
        if (blk == (unsigned long long)skip || j >= (unsigned long long)counts[blk]) continue;
        const uint2 p = all[i];
        if (p.x == 0u || p.y == 0u || p.x >= ns || p.y >= ns) { atomicAdd(&ctr[DMRG_C_BADPAIR], 1ull); continue; }
        mrg_union(par, p.x, p.y);
    }
}

// ---- host side --------------------------------------------------------------------------------------------
static inline MrgSimRule dmrg_sim_rule(shp_ctx *ctx, const uint32_t *best)
{
    const DMrgState &m = ctx->dmrg;
    return MrgSimRule{bp<double>(ctx->mrg_rec), m.ncol, m.has_key ? bp<long long>(ctx->mrg_key) : nullptr,
                      m.has_size ? bp<long long>(ctx->mrg_size) : nullptr, m.has_ign, m.ign, m.minb, m.has_thr, m.thr2, best};
}

// Step 1, up to the mutual rule's exchange.  The share table must be the context's finished one.  ncol 0: the
// key rule (keys given).  *d_best_out: with `mutual` the int64 column of S + 1 values for the all-reduce (context
// memory), otherwise NULL.  ms_out[2]: device time of the records' kernels, of the best passes.
static int run_dmrg_begin(shp_ctx *ctx, const double *const *cols, int ncol, int has_ignv, double ignv, int has_thr,
                          double thr2, int mutual, const int64_t *keys, int has_ignk, int64_t ignk, int64_t min_border,
                          const int64_t *seg_size, void **d_best_out, double *ms_out)
{
    const NbrTable &d = ctx->dnbr_tab;
    hipStream_t st = ctx->stream;
    const uint32_t S = d.S, nsh = d.nrows;
    const size_t ns = (size_t)S + 1;
    ctx->dmrg = DMrgState{};
    *d_best_out = nullptr;
    double msr = 0.0;
    if (ncol) CHK(mrgs_place_columns(ctx, cols, ncol, ns, has_ignv, ignv, mutual, &msr));
    CHK(mrg_begin(ctx, S, d.nent, keys, seg_size));
    DMrgState &m = ctx->dmrg;
    m.similar = ncol ? 1 : 0;
    m.ncol = ncol;
    m.has_key = keys ? 1 : 0;
    m.has_size = seg_size ? 1 : 0;
    m.has_ign = has_ignk;
    m.ign = (long long)ignk;
    m.minb = (long long)min_border;
    m.has_thr = has_thr;
    m.thr2 = thr2;
    m.mutual = ncol ? mutual : 0;
    m.table_serial = d.serial;
    m.ms_records = msr;
    float ms = 0.f;
    if (m.mutual) {
        CHK(buf_ensure(ctx, ctx->dmrg_b64, ns * 8));
        unsigned long long *bestd = (unsigned long long *)ctx->mrg_bestd.p;
        uint32_t *best = bp<uint32_t>(ctx->mrg_best);
        long long *b64 = bp<long long>(ctx->dmrg_b64);
        HIPCHK(ctx, hipEventRecord(ctx->ev[7], st));
        HIPCHK(ctx, hipMemsetAsync(bestd, 0xff, ns * 8, st));
        HIPCHK(ctx, hipMemsetAsync(best, 0xff, ns * 4, st));
        HIPCHK(ctx, hipMemsetAsync(b64, 0, ns * 8, st));
        if (d.nent) {
            const MrgSimRule q = dmrg_sim_rule(ctx, nullptr);
            const dim3 grid(mrg_pieces(d.nent));
            hipLaunchKernelGGL(k_mrgs_best<0>, grid, dim3(256), 0, st, mrg_table(d), q, bestd, best);
            KCHK(ctx);
            hipLaunchKernelGGL(k_mrgs_best<1>, grid, dim3(256), 0, st, mrg_table(d), q, bestd, best);
            KCHK(ctx);
        }
        if (nsh) {
            hipLaunchKernelGGL(k_dmrg_pack_best, dim3(grid_for(nsh, 256)), dim3(256), 0, st, (const uint32_t *)best, d.row0,
                               nsh, b64);
            KCHK(ctx);
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev[8], st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[7], ctx->ev[8]));
        *d_best_out = b64;
    } else {
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    if (ms_out) { ms_out[0] = msr; ms_out[1] = ms; }
    m.stage = 1;
    return 0;
}

// Step 1, the hook, and the rank's forest pairs.  counts_out[3]: links, entries a < b, forest pairs (at *d_pairs_out,
// context memory).  ms_out[2]: device time of the hook, of the flatten and the pairs' compaction.
static int run_dmrg_hook(shp_ctx *ctx, int64_t *counts_out, void **d_pairs_out, double *ms_out)
{
    const NbrTable &d = ctx->dnbr_tab;
    DMrgState &m = ctx->dmrg;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)d.S + 1;
    uint32_t *par = bp<uint32_t>(ctx->mrg_par), *root = bp<uint32_t>(ctx->mrg_root);
    unsigned long long *ctr = (unsigned long long *)ctx->mrg_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    const unsigned gs = grid_for(ns, 256);
    *d_pairs_out = nullptr;
    HIPCHK(ctx, hipEventRecord(ctx->ev[7], st));
    if (m.mutual) {
        hipLaunchKernelGGL(k_dmrg_unpack_best, dim3(gs), dim3(256), 0, st, (const long long *)ctx->dmrg_b64.p, (uint32_t)ns,
                           bp<uint32_t>(ctx->mrg_best));
        KCHK(ctx);
    }
    if (d.nent) {
        const dim3 grid(mrg_pieces(d.nent));
        if (m.similar) {
            const MrgSimRule q = dmrg_sim_rule(ctx, m.mutual ? bp<uint32_t>(ctx->mrg_best) : nullptr);
            hipLaunchKernelGGL(k_mrg_hook<MrgSimRule>, grid, dim3(256), 0, st, mrg_table(d), q, par, ctr);
        } else {
            const MrgLinkRule q{bp<long long>(ctx->mrg_key), m.has_size ? bp<long long>(ctx->mrg_size) : nullptr, m.has_ign,
                                m.ign, m.minb};
            hipLaunchKernelGGL(k_mrg_hook<MrgLinkRule>, grid, dim3(256), 0, st, mrg_table(d), q, par, ctr);
        }
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[8], st));
    hipLaunchKernelGGL(k_mrg_flatten, dim3(gs), dim3(256), 0, st, (const uint32_t *)par, (uint32_t)ns, root);
    KCHK(ctx);
    const unsigned gp = grid_for(ns, 4u * DMRG_WAVE_IDS);                  // (four wavefronts a workgroup)
    hipLaunchKernelGGL(k_dmrg_pairs<false>, dim3(gp), dim3(256), 0, st, (const uint32_t *)root, (uint32_t)ns, (uint2 *)nullptr,
                       0ull, ctr);
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(pin, ctr, MRG_C_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const unsigned long long np = pin[DMRG_C_NPAIR], links = pin[MRG_C_LINKS], half = pin[MRG_C_HALF];
    if (np > links || np >= ns) SHP_FAIL(ctx, SHP_ERR_STATE, "%llu forest pairs of %llu links", np, links);
    CHK(buf_ensure(ctx, ctx->dmrg_pairs, (size_t)(np ? np : 1) * 8));
    if (np) {
        hipLaunchKernelGGL(k_dmrg_pairs<true>, dim3(gp), dim3(256), 0, st, (const uint32_t *)root, (uint32_t)ns,
                           (uint2 *)ctx->dmrg_pairs.p, np, ctr);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[9], st));
    HIPCHK(ctx, hipMemcpyAsync(pin, &ctr[DMRG_C_PLACE], 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (pin[0] != np) SHP_FAIL(ctx, SHP_ERR_STATE, "%llu forest pairs placed, %llu counted", pin[0], np);
    float ms0 = 0.f, ms1 = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms0, ctx->ev[7], ctx->ev[8]));
    HIPCHK(ctx, hipEventElapsedTime(&ms1, ctx->ev[8], ctx->ev[9]));
    if (ms_out) { ms_out[0] = ms0; ms_out[1] = ms1; }
    m.npairs = np;
    m.stage = 2;
    counts_out[0] = (int64_t)links;
    counts_out[1] = (int64_t)half;
    counts_out[2] = (int64_t)np;
    *d_pairs_out = np ? ctx->dmrg_pairs.p : nullptr;
    return 0;
}

// Steps 2 and 3.  d_all: `world` blocks of `slot` pairs, counts[r] (host) valid in block r; the block `rank` is the
// rank's own and is not hooked again.  The groups are then the context's, as after shp_nbr_merge.  *d_hist_out: the
// groups' histogram (M + 1 int64, context memory).  ms_out[2]: device time of the pairs' hook, of the renumbering.
static int run_dmrg_number(shp_ctx *ctx, const uint2 *d_all, unsigned long long slot, uint32_t world, const uint32_t *counts,
                           uint32_t rank, uint32_t *M_out, void **d_hist_out, double *ms_out)
{
    const NbrTable &d = ctx->dnbr_tab;
    DMrgState &m = ctx->dmrg;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)d.S + 1;
    const unsigned long long total = slot * world;
    if (total > (unsigned long long)MRG_PIECE * 0x7fffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "%llu gathered pairs: too many", total);
    for (uint32_t r = 0; r < world; r++)
        if ((unsigned long long)counts[r] > slot) SHP_FAIL(ctx, SHP_ERR_ARG, "rank %u: %u pairs in a slot of %llu", r, counts[r], slot);
    if (total) {
        CHK(buf_ensure(ctx, ctx->dmrg_pcnt, (size_t)world * 4));
        HIPCHK(ctx, hipMemcpyAsync(ctx->dmrg_pcnt.p, counts, (size_t)world * 4, hipMemcpyHostToDevice, st));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));            // (mrg_number takes the hook's time from here)
    if (total && world > 1u) {
        hipLaunchKernelGGL(k_dmrg_hook_pairs, dim3(mrg_pieces(total)), dim3(256), 0, st, d_all, slot, total,
                           (const uint32_t *)ctx->dmrg_pcnt.p, rank, (uint32_t)ns, bp<uint32_t>(ctx->mrg_par),
                           (unsigned long long *)ctx->mrg_ctr.p);
        KCHK(ctx);
    }
    CHK(mrg_number(ctx, d.S, m.has_size != 0, M_out, nullptr, ms_out));
    const unsigned long long *pin = (const unsigned long long *)ctx->h_pinned;     // (mrg_number has fetched the counters)
    if (pin[DMRG_C_BADPAIR]) {
        ctx->mrg.stage = 0;
        SHP_FAIL(ctx, SHP_ERR_ARG, "%llu gathered pairs name an id outside 1..%u", pin[DMRG_C_BADPAIR], d.S);
    }
    ctx->mrg.table_serial = 0;                              // (no one-GPU table: shp_nbr_merge_contract refuses these groups)
    *d_hist_out = ctx->mrg_hist.p;
    m.stage = 3;
    return 0;
}

// Step 4.  [new_lo, new_hi): the rank's share of the new ids 0 .. M.  counts_out[5]: records (entries a < b between two
// groups), distinct pairs among them, home records, travelling records (at *d_trav_out), border lengths outside
// 1 .. 2^32 - 1.  With such a length nothing else is done and the old share table stays; otherwise the old share
// table ends here and shp_dnbr_merge_dev builds the new one.
static int run_dmrg_records(shp_ctx *ctx, uint32_t new_lo, uint32_t new_hi, int64_t *counts_out, void **d_trav_out,
                            double *ms_out)
{
    DNbrState &x = ctx->dnbr;
    const NbrTable &d = ctx->dnbr_tab;
    DMrgState &m = ctx->dmrg;
    MrgState &g = ctx->mrg;
    hipStream_t st = ctx->stream;
    unsigned long long *ctr = (unsigned long long *)ctx->mrg_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    for (int i = 0; i < 5; i++) counts_out[i] = 0;
    *d_trav_out = nullptr;
    m.stage = 0;
    if (g.half > NBR_MAX_REC) SHP_FAIL(ctx, SHP_ERR_NOMEM, "%llu neighbour records: more than the sort indexes", g.half);
    ctx->nbr.open = false;                                  // (the record buffer is the one-GPU accumulation's)
    CHK(buf_ensure(ctx, ctx->nbr_rec, (size_t)(g.half ? g.half : 1) * 16));
    CHK(buf_ensure(ctx, ctx->nbr_ctr, NBR_C_WORDS * 8));
    const unsigned long long cap = ctx->nbr_rec.cap / 16;
    HIPCHK(ctx, hipMemsetAsync(&ctr[MRG_C_REC], 0, 16, st));        // (MRG_C_REC and MRG_C_WIDE)
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (d.nent) {
        hipLaunchKernelGGL(k_mrg_records, dim3(mrg_pieces(d.nent)), dim3(256), 0, st, mrg_table(d),
                           (const uint32_t *)ctx->mrg_recode.p, (uint4 *)ctx->nbr_rec.p, cap, ctr);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipMemcpyAsync(pin, ctr, MRG_C_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const unsigned long long n = pin[MRG_C_REC], wide = pin[MRG_C_WIDE];
    if (n > g.half || n > cap) SHP_FAIL(ctx, SHP_ERR_STATE, "%llu records of %llu entries", n, g.half);
    counts_out[0] = (int64_t)n;
    counts_out[4] = (int64_t)wide;
    if (wide) return 0;
    // from here on the share table the groups were found in is gone: the share of the new ids waits in its place
    const uint32_t M = g.M;
    x = DNbrState{};
    dnbr_begin_share(ctx, M, new_lo, new_hi);
    uint32_t U = 0;
    CHK(nbr_sort_reduce<unsigned long long>(ctx, (const uint4 *)ctx->nbr_rec.p, (uint32_t)n, bits_for(M), &U));
    CHK(dnbr_pack(ctx, U, new_lo, new_hi, &x.nhome, &x.ntrav));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    x.nlocal = U;
    x.dev_ms = ms;
    x.stage = 1;
    g.contracted = true;
    counts_out[1] = (int64_t)U;
    counts_out[2] = (int64_t)x.nhome;
    counts_out[3] = (int64_t)x.ntrav;
    *d_trav_out = x.ntrav ? ctx->dnbr_trav.p : nullptr;
    if (ms_out) *ms_out = ms;
    return 0;
}
