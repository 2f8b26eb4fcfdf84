// nbrreduce.h -- per-segment columns reduced over the rows of the neighbour table (neighbours.reduceOverNeighbours),
// and the upload of a host table into the context (shp_nbr_upload).
//
// Row r of the CSR table (neighbours.h) has entries j = 0 .. deg - 1 with neighbour id n_j and border length w_j;
// v is the column widened to float64.  A value is IGNORED when it is NaN or equals the ignore value; C(r) is the
// set of entries whose v[n_j] is not ignored.  One pass over the row gives all nine statistics:
//   count |C|, border sum w, min / max of v[n], mean = (sum v[n]) / |C|, bordermean = (sum w v[n]) / sum w,
//   and with the row's own value v[r] (none of the three when v[r] is ignored): meanabsdiff = (sum w |v[n] - v[r]|)
//   / sum w, bordertohigher = sum of w over v[n] > v[r], nearest = the id with the smallest |v[n] - v[r]| (ties: the
//   smallest id).
// The integer sums are int64, min / max / nearest are comparisons: exact in any order.
//
// THE ORDER OF THE THREE FLOAT SUMS (sum v, sum w v, sum w |v - v[r]|) is a function of the row's length alone; a
// row-sharded form of this reduction has to reproduce it.  Every term is one float64 (a product is rounded once,
// the library is built with -ffp-contract=off), a sum starts at +0.0, an ignored entry adds nothing:
//   deg <= NBRR_LONG   one accumulator per sum, the entries added in entry order j = 0, 1, 2, ...
//   deg >  NBRR_LONG   the row is cut into chunks of NBRR_CHUNK entries by POSITION in the row (chunk c holds the
//                      entries c * NBRR_CHUNK .. ).  In a chunk, lane l of 64 adds the chunk's entries l, l + 64,
//                      l + 128, ... in that order into its own accumulator; the 64 accumulators are then combined
//                      by a butterfly: for d = 32, 16, 8, 4, 2, 1: acc[l] = acc[l] + acc[l ^ d] (IEEE addition
//                      commutes, so all lanes hold the same value; lanes past the chunk's end hold +0.0).  The
//                      chunks' sums are added in chunk order into an accumulator that starts at +0.0.
// Neither depends on the launch, on the rows that share a workgroup, or on where the table came from; there are no
// floating-point atomics.
//
// Kernels:
//  k_nbrr_short: a workgroup takes NBRR_ROWS consecutive rows, a thread per row.  The rows' entries are one span of
//     the arrays; it goes through LDS in pieces of NBRR_PIECE entries (id, border length and the gathered v[id],
//     20 bytes each: 20 KiB per workgroup, so seven workgroups -- 28 wavefronts -- fit the 160 KiB of a CU), loaded
//     coalesced, and every thread walks the part of its row that lies in the piece, its accumulators in registers
//     across pieces.  The gather v[n_j] is the only random access.  A piece that holds entries of long rows only is
//     skipped after one barrier.  LDS reads of the walk are 8 bytes at a stride of the rows' lengths: bank
//     conflicts there are left as they fall.
//  k_nbrr_long: a wavefront per chunk of a long row, partial results to a record per chunk; k_nbrr_long_combine: a
//     thread per long row adds the chunks' records in chunk order.  The long rows and their chunks are listed once
//     per table (a flag scan, a fill, a scan of the chunk counts: scan.h) and kept while the table is resident:
//     NbrLongList (common.h) and nbrr_long_ensure, for the one-GPU table, a rank's share table and the member list of
//     nbragg.h alike.
//  k_nbrr_validate: the rules of an uploaded table (below), one launch.
// The three reduction kernels take a row base (NbrrParams::row0): the table's row i is id row0 + i.  The one-GPU
// table has row0 = 0; the share table of a row-sharded raster (dneighbours.h) holds the whole rows of the ids
// row0 .. row0 + ns - 1, and since a row's order above depends on nothing but the row, its results are the same bits.
// Host side, shared by the three reductions (run_nbr_reduce here, run_dnbr_reduce, run_agg): nbrr_stage_column puts
// the host column on the device, nbrr_params / nbrr_table_params fill the kernels' parameters, nbrr_launch runs them.
#pragma once
#include "common.h"
#include "scan.h"
#include "colour.h"
#include "neighbours.h"
#include <math.h>

#define NBRR_ROWS 256u          // rows per workgroup of k_nbrr_short (a thread each)
#ifndef NBRR_PIECE
#define NBRR_PIECE 1024u        // entries per LDS piece
#endif
#ifndef NBRR_LONG
#define NBRR_LONG 256u          // rows with more entries go to k_nbrr_long
#endif
#ifndef NBRR_CHUNK
#define NBRR_CHUNK 4096u        // entries per chunk of a long row: part of the summation order
#endif
static_assert(NBRR_PIECE >= 256u && NBRR_PIECE * 20u <= 160u * 1024u, "NBRR_PIECE: 20 bytes of LDS per entry");
static_assert(NBRR_CHUNK >= 64u && NBRR_CHUNK % 64u == 0u && NBRR_LONG >= 1u, "NBRR_CHUNK is a multiple of the wavefront");

// bits of the statistics mask, and the slot of a statistic's output
enum { NBRR_COUNT = 0, NBRR_BORDER = 1, NBRR_MIN = 2, NBRR_MAX = 3, NBRR_MEAN = 4, NBRR_BORDERMEAN = 5,
       NBRR_MEANABSDIFF = 6, NBRR_BORDERTOHIGHER = 7, NBRR_NEAREST = 8, NBRR_NPUBLIC = 9,
       NBRR_SUM = 9, NBRR_NSTATS = 10 };
// (NBRR_NPUBLIC: the statistics shp_nbr_reduce / shp_dnbr_reduce_dev offer.  NBRR_SUM, sum v itself, is the
//  aggregation's: nbragg.h runs these kernels over the member lists of a merge's groups)

struct NbrrParams {
    const long long *offs;
    const uint32_t *ids;
    const long long *lens;
    const double *col;
    uint32_t ns;                // rows of the table: max_seg_id + 1, or the rows of an id share (dneighbours.h)
    uint32_t row0;              // the id of the table's row 0: 0, or the share's first id.  Row i is id row0 + i: its own
                                // value is col[row0 + i], its results go to out[..][row0 + i]; col and out span all ids
    int has_ign;
    double ign, missing;
    void *out[NBRR_NSTATS];     // device columns of ns rows (8 bytes each), nullptr where not asked for
};

struct NbrrAcc {
    double sv, swv, swd;        // the three float sums
    long long cnt, bor, bth;
    double mn, mx, nd;          // nd: the smallest distance so far
    uint32_t nid;               // its id (0xffffffff: none yet)
};

__device__ __forceinline__ void nbrr_init(NbrrAcc &a)
{
    a.sv = 0.0; a.swv = 0.0; a.swd = 0.0;
    a.cnt = 0; a.bor = 0; a.bth = 0;
    a.mn = INFINITY; a.mx = -INFINITY; a.nd = INFINITY;
    a.nid = 0xffffffffu;
}

__device__ __forceinline__ bool nbrr_ignored(double x, int has_ign, double ign)
{
    return x != x || (has_ign && x == ign);
}

// one entry of a row: neighbour id, border length w, gathered value x; own: the row's value, used when own_ok
__device__ __forceinline__ void nbrr_add(NbrrAcc &a, uint32_t id, long long w, double x, double own, bool own_ok,
                                         int has_ign, double ign)
{
    if (nbrr_ignored(x, has_ign, ign)) return;
    const double wd = (double)w;
    a.cnt += 1;
    a.bor += w;
    a.sv = a.sv + x;
    a.swv = a.swv + wd * x;
    a.mn = x < a.mn ? x : a.mn;
    a.mx = x > a.mx ? x : a.mx;
    if (own_ok) {
        const double d = fabs(x - own);
        a.swd = a.swd + wd * d;
        if (x > own) a.bth += w;
        if (d < a.nd || (d == a.nd && id < a.nid)) { a.nd = d; a.nid = id; }
    }
}

// a = a (+) b: the sums as a + b, the rest exact
__device__ __forceinline__ void nbrr_merge(NbrrAcc &a, const NbrrAcc &b)
{
    a.sv = a.sv + b.sv;
    a.swv = a.swv + b.swv;
    a.swd = a.swd + b.swd;
    a.cnt += b.cnt; a.bor += b.bor; a.bth += b.bth;
    a.mn = b.mn < a.mn ? b.mn : a.mn;
    a.mx = b.mx > a.mx ? b.mx : a.mx;
    if (b.nd < a.nd || (b.nd == a.nd && b.nid < a.nid)) { a.nd = b.nd; a.nid = b.nid; }
}

__device__ __forceinline__ void nbrr_store(const NbrrParams &p, uint32_t r, const NbrrAcc &a, bool own_ok)
{
    const bool any = a.cnt > 0;
    r += p.row0;
    if (p.out[NBRR_COUNT]) ((long long *)p.out[NBRR_COUNT])[r] = a.cnt;
    if (p.out[NBRR_BORDER]) ((long long *)p.out[NBRR_BORDER])[r] = a.bor;
    if (p.out[NBRR_MIN]) ((double *)p.out[NBRR_MIN])[r] = any ? a.mn : p.missing;
    if (p.out[NBRR_MAX]) ((double *)p.out[NBRR_MAX])[r] = any ? a.mx : p.missing;
    if (p.out[NBRR_MEAN]) ((double *)p.out[NBRR_MEAN])[r] = any ? a.sv / (double)a.cnt : p.missing;
    // (a table's border lengths are 1 or more; the weights of nbragg.h may all be 0)
    if (p.out[NBRR_BORDERMEAN]) ((double *)p.out[NBRR_BORDERMEAN])[r] = (any && a.bor != 0) ? a.swv / (double)a.bor : p.missing;
    if (p.out[NBRR_SUM]) ((double *)p.out[NBRR_SUM])[r] = any ? a.sv : p.missing;
    if (p.out[NBRR_MEANABSDIFF])
        ((double *)p.out[NBRR_MEANABSDIFF])[r] = (any && own_ok) ? a.swd / (double)a.bor : p.missing;
    if (p.out[NBRR_BORDERTOHIGHER]) ((long long *)p.out[NBRR_BORDERTOHIGHER])[r] = (any && own_ok) ? a.bth : 0;
    if (p.out[NBRR_NEAREST])
        ((long long *)p.out[NBRR_NEAREST])[r] = (any && own_ok && a.nid != 0xffffffffu) ? (long long)a.nid : 0;
}

__global__ __launch_bounds__(256) void k_nbrr_short(NbrrParams p)
{
    __shared__ double s_x[NBRR_PIECE];
    __shared__ long long s_w[NBRR_PIECE];
    __shared__ uint32_t s_id[NBRR_PIECE];
    const uint32_t r0 = blockIdx.x * NBRR_ROWS, r = r0 + threadIdx.x;
    const uint32_t rend = r0 + NBRR_ROWS < p.ns ? r0 + NBRR_ROWS : p.ns;
    const long long s0 = p.offs[r0], s1 = p.offs[rend];
    const bool in = r < p.ns;
    const long long a = in ? p.offs[r] : s1, b = in ? p.offs[r + 1u] : s1;
    const bool mine = in && b - a <= (long long)NBRR_LONG;         // (a long row is written by k_nbrr_long_combine)
    const double own = in ? p.col[p.row0 + r] : 0.0;
    const bool own_ok = !nbrr_ignored(own, p.has_ign, p.ign);
    NbrrAcc acc;
    nbrr_init(acc);
    for (long long p0 = s0; p0 < s1; p0 += (long long)NBRR_PIECE) {
        const long long p1 = p0 + (long long)NBRR_PIECE < s1 ? p0 + (long long)NBRR_PIECE : s1;
        const long long lo = a > p0 ? a : p0, hi = b < p1 ? b : p1;
        const bool need = mine && lo < hi;
        // (a barrier as well: the walk of the last piece is over before this one is loaded)
        if (!__syncthreads_or(need ? 1 : 0)) continue;
        const uint32_t len = (uint32_t)(p1 - p0);
        for (uint32_t i = threadIdx.x; i < len; i += 256u) {
            const uint32_t id = p.ids[p0 + i];
            s_id[i] = id;
            s_w[i] = p.lens[p0 + i];
            s_x[i] = p.col[id];
        }
        __syncthreads();
        if (need) {
            const uint32_t e1 = (uint32_t)(hi - p0);
            for (uint32_t e = (uint32_t)(lo - p0); e < e1; e++)
                nbrr_add(acc, s_id[e], s_w[e], s_x[e], own, own_ok, p.has_ign, p.ign);
        }
    }
    if (mine) nbrr_store(p, r, acc, own_ok);
}

// what a chunk of a long row leaves for k_nbrr_long_combine
struct NbrrPart {
    double sv, swv, swd, mn, mx, nd;
    long long cnt, bor, bth;
    unsigned long long nid;
};

// lrow[k]: the k-th long row; lcoff[k]: the chunks of the long rows before it (nlong + 1 words).  A wavefront per chunk.
__global__ __launch_bounds__(256) void k_nbrr_long(NbrrParams p, const uint32_t *__restrict__ lrow,
                                                   const uint32_t *__restrict__ lcoff, uint32_t nlong, uint32_t nchunks,
                                                   NbrrPart *__restrict__ part)
{
    const uint32_t item = blockIdx.x * 4u + (threadIdx.x >> 6);
    const unsigned lane = lane_id();
    if (item >= nchunks) return;                // (uniform in the wavefront)
    // the last k with lcoff[k] <= item
    uint32_t lo = 0u, hi = nlong;
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (lcoff[mid] <= item) lo = mid; else hi = mid;
    }
    const uint32_t r = lrow[lo], c = item - lcoff[lo];
    const long long a = p.offs[r] + (long long)c * (long long)NBRR_CHUNK, rowend = p.offs[r + 1u];
    const long long b = a + (long long)NBRR_CHUNK < rowend ? a + (long long)NBRR_CHUNK : rowend;
    const double own = p.col[p.row0 + r];
    const bool own_ok = !nbrr_ignored(own, p.has_ign, p.ign);
    NbrrAcc acc;
    nbrr_init(acc);
    for (long long e = a + lane; e < b; e += 64) {
        const uint32_t id = p.ids[e];
        nbrr_add(acc, id, p.lens[e], p.col[id], own, own_ok, p.has_ign, p.ign);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        NbrrAcc o;
        o.sv = __shfl_xor(acc.sv, d, 64); o.swv = __shfl_xor(acc.swv, d, 64); o.swd = __shfl_xor(acc.swd, d, 64);
        o.cnt = __shfl_xor(acc.cnt, d, 64); o.bor = __shfl_xor(acc.bor, d, 64); o.bth = __shfl_xor(acc.bth, d, 64);
        o.mn = __shfl_xor(acc.mn, d, 64); o.mx = __shfl_xor(acc.mx, d, 64); o.nd = __shfl_xor(acc.nd, d, 64);
        o.nid = (uint32_t)__shfl_xor((int)acc.nid, d, 64);
        nbrr_merge(acc, o);
    }
    if (lane == 0u) {
        NbrrPart q;
        q.sv = acc.sv; q.swv = acc.swv; q.swd = acc.swd; q.mn = acc.mn; q.mx = acc.mx; q.nd = acc.nd;
        q.cnt = acc.cnt; q.bor = acc.bor; q.bth = acc.bth; q.nid = acc.nid;
        part[item] = q;
    }
}

__global__ __launch_bounds__(256) void k_nbrr_long_combine(NbrrParams p, const uint32_t *__restrict__ lrow,
                                                           const uint32_t *__restrict__ lcoff, uint32_t nlong,
                                                           const NbrrPart *__restrict__ part)
{
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k >= nlong) return;
    const uint32_t r = lrow[k];
    const bool own_ok = !nbrr_ignored(p.col[p.row0 + r], p.has_ign, p.ign);
    NbrrAcc acc;
    nbrr_init(acc);
    for (uint32_t i = lcoff[k]; i < lcoff[k + 1u]; i++) {
        const NbrrPart q = part[i];
        NbrrAcc o;
        o.sv = q.sv; o.swv = q.swv; o.swd = q.swd; o.mn = q.mn; o.mx = q.mx; o.nd = q.nd;
        o.cnt = q.cnt; o.bor = q.bor; o.bth = q.bth; o.nid = (uint32_t)q.nid;
        nbrr_merge(acc, o);
    }
    nbrr_store(p, r, acc, own_ok);
}

// ---- the list of long rows ----------------------------------------------------------------------------------
struct NbrrLongFn {             // 1 where row i is long
    const long long *offs;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        return offs[i + 1u] - offs[i] > (long long)NBRR_LONG ? 1u : 0u;
    }
};
struct NbrrChunksFn {           // chunks of the k-th long row
    const long long *offs;
    const uint32_t *lrow;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const
    {
        const uint32_t r = lrow[k];
        return (uint32_t)((offs[r + 1u] - offs[r] + (long long)NBRR_CHUNK - 1) / (long long)NBRR_CHUNK);
    }
};
__global__ __launch_bounds__(256) void k_nbrr_long_fill(const long long *__restrict__ offs, uint32_t ns,
                                                        const uint32_t *__restrict__ lidx, uint32_t *__restrict__ lrow)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r < ns && offs[r + 1u] - offs[r] > (long long)NBRR_LONG) lrow[lidx[r]] = r;
}

__global__ __launch_bounds__(256) void k_nbrr_from_i64(const long long *__restrict__ in, size_t n, double *__restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) out[i] = (double)in[i];
}

// ---- an uploaded table's rules --------------------------------------------------------------------------------
// The first violation is the smallest key: offsets before entries, then the position, then the rule.
enum { NBRR_V_FIRST = 1, NBRR_V_DECREASING = 2, NBRR_V_END = 3, NBRR_V_RANGE = 4, NBRR_V_SELF = 5, NBRR_V_ORDER = 6,
       NBRR_V_LENGTH = 7 };
__device__ __forceinline__ void nbrr_violation(unsigned long long *first, int entry, long long pos, int rule)
{
    atomicMin(first, ((unsigned long long)entry << 60) | ((unsigned long long)pos << 4) | (unsigned long long)rule);
}
__device__ __forceinline__ void nbrr_check_entry(const uint32_t *ids, const long long *lens, long long e, long long a,
                                                 uint32_t r, uint32_t S, unsigned long long *first)
{
    const uint32_t id = ids[e];
    if (id < 1u || id > S) nbrr_violation(first, 1, e, NBRR_V_RANGE);
    else if (id == r) nbrr_violation(first, 1, e, NBRR_V_SELF);
    if (e > a && ids[e - 1] >= id) nbrr_violation(first, 1, e, NBRR_V_ORDER);
    if (lens[e] < 1) nbrr_violation(first, 1, e, NBRR_V_LENGTH);
}
// A thread per row checks the row's offsets and, if they lie in the arrays, a short row's entries; the long rows of
// a workgroup are then checked by all of its threads together.
__global__ __launch_bounds__(256) void k_nbrr_validate(const long long *__restrict__ offs, const uint32_t *__restrict__ ids,
                                                       const long long *__restrict__ lens, uint32_t ns, long long nent,
                                                       unsigned long long *first)
{
    __shared__ long long s_a[256], s_b[256];
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const uint32_t S = ns - 1u;
    long long a = 0, b = 0;
    if (r < ns) {
        a = offs[r];
        b = offs[r + 1u];
        if (r == 0u && (a != 0 || b != 0)) nbrr_violation(first, 0, a != 0 ? 0 : 1, NBRR_V_FIRST);
        if (b < a) nbrr_violation(first, 0, (long long)r + 1, NBRR_V_DECREASING);
        if (r == S && b != nent) nbrr_violation(first, 0, (long long)r + 1, NBRR_V_END);
        if (a < 0 || b < a || b > nent) a = b = 0;             // nothing of this row can be read
    }
    s_a[threadIdx.x] = a;
    s_b[threadIdx.x] = b;
    if (b - a <= (long long)NBRR_LONG)
        for (long long e = a; e < b; e++) nbrr_check_entry(ids, lens, e, a, r, S, first);
    __syncthreads();
    for (uint32_t t = 0; t < 256u; t++) {
        const long long ta = s_a[t], tb = s_b[t];
        if (tb - ta <= (long long)NBRR_LONG) continue;          // (uniform)
        for (long long e = ta + threadIdx.x; e < tb; e += 256) nbrr_check_entry(ids, lens, e, ta, blockIdx.x * 256u + t, S, first);
    }
}

// ---- host side --------------------------------------------------------------------------------------------
static const char *nbrr_rule_text(int rule)
{
    switch (rule) {
    case NBRR_V_FIRST: return "offsets[0] and offsets[1] must be 0";
    case NBRR_V_DECREASING: return "the offsets must not decrease";
    case NBRR_V_END: return "the last offset must be the number of entries";
    case NBRR_V_RANGE: return "a neighbour id outside 1..max_seg_id";
    case NBRR_V_SELF: return "a row names itself";
    case NBRR_V_ORDER: return "the ids of a row must ascend strictly";
    default: return "a border length below 1";
    }
}

// A host table into the context's one-GPU table.  A table that breaks a rule leaves no finished table.
static int run_nbr_upload(shp_ctx *ctx, const int64_t *offsets, const uint32_t *nbrs, const int64_t *lens, uint32_t S,
                          long long nent, double *dev_ms_out)
{
    NbrState &s = ctx->nbr;
    NbrTable &t = ctx->nbr_tab;
    hipStream_t st = ctx->stream;
    s = NbrState{};
    nbr_table_end(t);
    t.serial = nbr_next_serial();
    t.S = S;
    t.nrows = S + 1u;
    CHK(buf_ensure(ctx, ctx->nbr_ctr, NBR_C_WORDS * 8));
    unsigned long long *first = (unsigned long long *)ctx->nbr_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    CHK(nbr_table_upload_arrays(ctx, t, offsets, nbrs, lens, (unsigned long long)nent));
    HIPCHK(ctx, hipMemsetAsync(first, 0xff, 8, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_nbrr_validate, dim3(grid_for(t.nrows, 256)), dim3(256), 0, st, (const long long *)t.offs.p,
                       (const uint32_t *)t.ids.p, (const long long *)t.lens.p, t.nrows, nent, first);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(pin, first, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    nbr_ms(ctx);
    if (dev_ms_out) *dev_ms_out = s.dev_ms;
    const unsigned long long key = pin[0];
    if (key != ~0ull) {
        const int rule = (int)(key & 15ull);
        const long long pos = (long long)((key >> 4) & ((1ull << 56) - 1ull));
        SHP_FAIL(ctx, SHP_ERR_ARG, "not a neighbour table: %s %lld: %s", (key >> 60) ? "entry" : "offset", pos,
                 nbrr_rule_text(rule));
    }
    t.nent = (unsigned long long)nent;
    t.finished = true;
    return 0;
}

// The long rows of a CSR of nrows rows (offsets offs) and their chunks into `list`, unless it holds those of `serial`
// already: once per table or member list, whichever of them the list belongs to.
static int nbrr_long_ensure(shp_ctx *ctx, NbrLongList &list, const long long *offs, uint32_t nrows, unsigned long long serial)
{
    if (list.serial == serial) return 0;
    hipStream_t st = ctx->stream;
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_NBR;
    list.serial = 0;
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(nrows)));
    CHK(buf_ensure(ctx, ctx->nbr_deg, (size_t)nrows * 4));
    uint32_t *lidx = bp<uint32_t>(ctx->nbr_deg);
    NbrrLongFn lf{offs};
    CHK(scan_exclusive(ctx, lf, nrows, lidx, nullptr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nlong = *(volatile uint32_t *)mir;
    uint32_t nchunks = 0;
    if (nlong) {
        CHK(buf_ensure(ctx, list.lrow, (size_t)nlong * 4));
        CHK(buf_ensure(ctx, list.lcoff, ((size_t)nlong + 1) * 4));
        hipLaunchKernelGGL(k_nbrr_long_fill, dim3(grid_for(nrows, 256)), dim3(256), 0, st, offs, nrows, (const uint32_t *)lidx,
                           bp<uint32_t>(list.lrow));
        KCHK(ctx);
        NbrrChunksFn cf{offs, bp<uint32_t>(list.lrow)};
        uint32_t *lcoff = bp<uint32_t>(list.lcoff);
        CHK(scan_exclusive(ctx, cf, nlong, lcoff, lcoff + nlong, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 1));
        HIPCHK(ctx, hipStreamSynchronize(st));
        nchunks = *(volatile uint32_t *)(mir + 1);
        if (nchunks < nlong) SHP_FAIL(ctx, SHP_ERR_STATE, "%u chunks for %u long rows", nchunks, nlong);
    }
    list.nlong = nlong;
    list.nchunks = nchunks;
    list.serial = serial;
    return 0;
}

// the reduction's kernels over the CSR of p, its long rows listed in `list`
static int nbrr_launch(shp_ctx *ctx, const NbrrParams &p, const NbrLongList &list)
{
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_nbrr_short, dim3(grid_for(p.ns, NBRR_ROWS)), dim3(256), 0, st, p);
    KCHK(ctx);
    if (list.nlong) {
        const uint32_t *lrow = (const uint32_t *)list.lrow.p, *lcoff = (const uint32_t *)list.lcoff.p;
        CHK(buf_ensure(ctx, ctx->nbrr_part, (size_t)list.nchunks * sizeof(NbrrPart)));
        hipLaunchKernelGGL(k_nbrr_long, dim3(grid_for(list.nchunks, 4)), dim3(256), 0, st, p, lrow, lcoff, list.nlong,
                           list.nchunks, (NbrrPart *)ctx->nbrr_part.p);
        KCHK(ctx);
        hipLaunchKernelGGL(k_nbrr_long_combine, dim3(grid_for(list.nlong, 256)), dim3(256), 0, st, p, lrow, lcoff, list.nlong,
                           (const NbrrPart *)ctx->nbrr_part.p);
        KCHK(ctx);
    }
    return 0;
}

// One host column of ns values (ctype: COL_F64 / COL_F32 / COL_I64) as float64 in nbrr_col: float64 is copied there,
// float32 and int64 go to ctx->img and through a conversion kernel.  ev[0] is recorded between the copy and the
// conversion: the caller's device time starts there.  *raw_out: the column as the host gave it, on the device.
static int nbrr_stage_column(shp_ctx *ctx, const void *col, int ctype, size_t ns, const void **raw_out)
{
    hipStream_t st = ctx->stream;
    CHK(buf_ensure(ctx, ctx->nbrr_col, ns * 8));
    double *d_col = bp<double>(ctx->nbrr_col);
    const void *d_raw = d_col;
    if (ctype != COL_F64) {
        CHK(buf_ensure(ctx, ctx->img, ns * (ctype == COL_F32 ? 4 : 8)));
        d_raw = ctx->img.p;
    }
    HIPCHK(ctx, hipMemcpyAsync((void *)d_raw, col, ns * (ctype == COL_F32 ? 4 : 8), hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (ctype == COL_F32) {
        hipLaunchKernelGGL(k_col_from_f32, dim3(colour_grid(ns, 256)), dim3(256), 0, st, (const float *)d_raw, ns, d_col);
        KCHK(ctx);
    } else if (ctype == COL_I64) {
        hipLaunchKernelGGL(k_nbrr_from_i64, dim3(colour_grid(ns, 256)), dim3(256), 0, st, (const long long *)d_raw, ns, d_col);
        KCHK(ctx);
    }
    if (raw_out) *raw_out = d_raw;
    return 0;
}

// the kernels' parameters over a CSR of nrows rows whose row 0 is id row0, the column staged in nbrr_col; no outputs yet
static NbrrParams nbrr_params(shp_ctx *ctx, const void *offs, const void *ids, const void *lens, uint32_t nrows, uint32_t row0,
                              int has_ign, double ign, double missing)
{
    NbrrParams p;
    p.offs = (const long long *)offs;
    p.ids = (const uint32_t *)ids;
    p.lens = (const long long *)lens;
    p.col = bp<double>(ctx->nbrr_col);
    p.ns = nrows;
    p.row0 = row0;
    p.has_ign = has_ign;
    p.ign = ign;
    p.missing = missing;
    for (int i = 0; i < NBRR_NSTATS; i++) p.out[i] = nullptr;
    return p;
}

// ... over a table, the statistics of `mask` written to consecutive columns of S + 1 rows from d_out, in the order of
// their bits
static NbrrParams nbrr_table_params(shp_ctx *ctx, const NbrTable &t, int has_ign, double ign, double missing, void *d_out,
                                    uint32_t mask)
{
    NbrrParams p = nbrr_params(ctx, t.offs.p, t.ids.p, t.lens.p, t.nrows, t.row0, has_ign, ign, missing);
    int slot = 0;
    for (int i = 0; i < NBRR_NSTATS; i++)
        if ((mask >> i) & 1u) p.out[i] = (char *)d_out + (size_t)(slot++) * ((size_t)t.S + 1) * 8;
    return p;
}

static int nbrr_mask_count(uint32_t mask)
{
    int nsel = 0;
    for (int i = 0; i < NBRR_NSTATS; i++) nsel += (mask >> i) & 1u;
    return nsel;
}

// device time between ev[0] and ev[1] (the stream is synchronised)
static int nbrr_dev_ms(shp_ctx *ctx, double *dev_ms_out)
{
    if (dev_ms_out) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        *dev_ms_out = ms;
    }
    return 0;
}

// One column over the one-GPU table.  outs[i]: host memory of S + 1 rows for statistic i of the mask.
static int run_nbr_reduce(shp_ctx *ctx, const void *col, int ctype, int has_ign, double ign, double missing,
                          uint32_t mask, void *const *outs, double *dev_ms_out)
{
    NbrTable &t = ctx->nbr_tab;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)t.S + 1;
    CHK(buf_ensure(ctx, ctx->nbrr_out, (size_t)nbrr_mask_count(mask) * ns * 8));
    CHK(nbrr_stage_column(ctx, col, ctype, ns, nullptr));
    CHK(nbrr_long_ensure(ctx, t.longs, (const long long *)t.offs.p, t.nrows, t.serial));
    const NbrrParams p = nbrr_table_params(ctx, t, has_ign, ign, missing, ctx->nbrr_out.p, mask);
    CHK(nbrr_launch(ctx, p, t.longs));
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    for (int i = 0; i < NBRR_NSTATS; i++)
        if (p.out[i]) HIPCHK(ctx, hipMemcpyAsync(outs[i], p.out[i], ns * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return nbrr_dev_ms(ctx, dev_ms_out);
}
