// nbrmerge.h -- touching segments of one class become one object (neighbours.mergeSegments): the groups of the
// neighbour table under a key column, their numbering, the contracted table and the recoded label raster.
//
// key[i] is the class of id i (int64).  Entry (a, b, w) of the finished table (neighbours.h: row a names b with
// border length w) is a LINK when key[a] == key[b], key[a] is not the ignored key, w >= min_border and -- with
// sizes given -- both ids have pixels.  A GROUP is a connected component of the links over the ids 1 .. S (with
// sizes: over those that have pixels; the others recode to 0).  Groups are numbered 1 .. M in ascending order of
// their smallest member.  Every table of this library names a pair from both sides, so only the entries with
// a < b are read, here and in the contraction.  All of it is integer work: no result depends on the order in which
// the atomics below arrive.
//
// neighbours.mergeSimilarSegments is the same merge under another link rule (MrgSimRule below: a distance between
// per-segment columns, by threshold or by mutually nearest neighbours); only k_mrg_hook's predicate and what feeds it
// differ, everything after the links is shared (mrg_begin / mrg_number).
//
// Kernels:
//  k_mrg_hook: a template over the link rule.  The entries are cut into pieces of MRG_PIECE consecutive entries, a workgroup each, whatever rows they
//     belong to: a row of 20 000 entries is ten pieces, 500 rows of four entries are one.  Two threads find the
//     rows of the piece's first and last entry in the offsets (a search over all rows), every thread then finds the row
//     of each of its entries between those two.  A link is hooked into a uint32 parent array as the pixel CCL hooks
//     (clump.h, uf_merge): the larger root under the smaller by atomicMin, again from the returned value when the
//     root had been hooked meanwhile.  A parent only ever decreases, so the smallest member ends as the root.  The
//     parent array is read with agent-scope loads only: they are answered where the atomics land, never by a line
//     of the CU's L1 or of another XCD's L2.  After a find the entry's own id is pointed at the root it found
//     (atomicMin again), which keeps the paths of a long chain of hooks short.
//  k_mrgs_place / k_mrgs_mark: the distance columns as one record per id; k_mrgs_best: the mutual rule's per-row best,
//     two passes over the hook's pieces (at MrgSimRule and the kernels).
//  k_mrg_flatten: root[i] of every id, in a launch of its own (nothing hooks any more: plain loads).
//  MrgRootFn + scan.h: 1 at every root that is a vertex; its exclusive scan is the root's new id - 1.
//  k_mrg_write: recode, representative, and by 64-bit atomics the group sizes and (with sizes) the new histogram;
//     the lanes of a wavefront that hold the first lane's group add once (one group of everything: one atomic per
//     wavefront, not 64 on one word).
//  k_mrg_records: the entries a < b whose ends recode to different non-zero ids, as the 16-byte records of
//     neighbours.h (larger new id, smaller new id, w); nbr_build_table sorts and reduces them into the context's
//     finished table.  A record carries a 32-bit count: a border length of 2^32 or more is refused.
//  k_mrg_recode: out[p] = recode[seg[p]], four labels a lane as k_colour_lookup streams them; a label above S is not
//     looked up, the largest one is kept.  COUNT: the new ids are counted into the 64-bit histogram in the same pass, a
//     lane's equal labels next to each other as one add, and the lanes that hold the first lane's id as one atomic.
#pragma once
#include "common.h"
#include "scan.h"
#include "neighbours.h"

#ifndef MRG_PIECE
#define MRG_PIECE 2048u         // entries per workgroup of k_mrg_hook / k_mrg_records (8 per thread)
#endif
static_assert(MRG_PIECE % 256u == 0u, "MRG_PIECE is a multiple of the workgroup");

// device words of a merge (ctx->mrg_ctr): [0] links, [1] entries with a < b, [2] records reserved,
// [3] records whose border length does not fit 32 bits, [4] largest label above S met by k_mrg_recode
enum { MRG_C_LINKS = 0, MRG_C_HALF = 1, MRG_C_REC = 2, MRG_C_WIDE = 3, MRG_C_BAD = 4, MRG_C_WORDS = 8 };

// What the merge's kernels read of an NbrTable (mrg_table): the one-GPU table (rows 0 .. S) or the rows of a rank's id
// share (dnbrmerge.h); row i is id row0 + i.
struct MrgTable {
    const long long *offs;
    const uint32_t *ids;
    const long long *lens;
    uint32_t ns;                // ids: S + 1
    long long nent;
    uint32_t nrows;             // rows of offs: S + 1, or those of the share
    uint32_t row0;              // id of row 0: 0, or the share's first id
};

// A link rule answers link(a, b, w) for an entry with a < b, both ids inside the table.
struct MrgLinkRule {
    const long long *key;
    const long long *size;      // nullptr: every id 1 .. S is a vertex
    int has_ign;
    long long ign, minb;
    __device__ __forceinline__ bool link(uint32_t a, uint32_t b, long long w) const
    {
        if (w < minb) return false;
        const long long ka = key[a];
        if (ka != key[b] || (has_ign && ka == ign)) return false;
        if (size && (size[a] <= 0 || size[b] <= 0)) return false;
        return true;
    }
};

// The rule of neighbours.mergeSimilarSegments.  rec: one record of ncol float64 per id, the id's values in the order
// of the columns (k_mrgs_place), its first value NaN when any of them is ignored (k_mrgs_mark): d2 of such an id is
// NaN against everybody, and a d2 that is not finite is no candidate anyway.  A record and not ncol planes: the two
// gathers of an entry are the only random accesses of the hook, and a record of up to 64 bytes lies in one or two
// 128-byte lines where planes would touch ncol of them per end.
// d2(a, b) = sum over the columns, in their order, of t * t with t = x[a] - x[b], from +0.0; every operation rounded
// once (the library is built with -ffp-contract=off); t * t has the bits of (-t) * (-t), so d2(a, b) == d2(b, a).
// An entry is a CANDIDATE when w >= minb, both ids have pixels (with sizes), the keys agree and are not the ignored
// one (with keys) and d2 is finite.  best == nullptr: a candidate is a link when d2 <= thr2.  Otherwise best[i] is
// the candidate neighbour of row i with the smallest d2, the smallest id among equals (0xffffffff: none), and a
// candidate is a link when its ends name each other and (with has_thr) d2 <= thr2.
#define MRGS_MAX_COLS 8
struct MrgSimRule {
    const double *rec;
    int ncol;
    const long long *key;       // nullptr: no key rule
    const long long *size;      // nullptr: every id 1 .. S is a vertex
    int has_ign;
    long long ign, minb;
    int has_thr;
    double thr2;
    const uint32_t *best;
    __device__ __forceinline__ bool candidate(uint32_t a, uint32_t b, long long w, double &d) const
    {
        if (w < minb) return false;
        if (size && (size[a] <= 0 || size[b] <= 0)) return false;
        if (key) {
            const long long ka = key[a];
            if (ka != key[b] || (has_ign && ka == ign)) return false;
        }
        const double *xa = rec + (size_t)a * (size_t)ncol, *xb = rec + (size_t)b * (size_t)ncol;
        double s = 0.0;
        for (int c = 0; c < ncol; c++) {
            const double t = xa[c] - xb[c];
            s = s + t * t;
        }
        d = s;
        return s < INFINITY;                                    // (false for NaN as well)
    }
    __device__ __forceinline__ bool link(uint32_t a, uint32_t b, long long w) const
    {
        double d;
        if (!candidate(a, b, w, d)) return false;
        if (best && (best[a] != b || best[b] != a)) return false;
        return !has_thr || d <= thr2;
    }
};

// the last row r of lo .. hi with offs[r] <= e (it is the row of entry e: offs[r + 1] > e)
__device__ __forceinline__ uint32_t mrg_row_of(const long long *__restrict__ offs, uint32_t lo, uint32_t hi, long long e)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1u) / 2u;
        if (offs[mid] <= e) lo = mid; else hi = mid - 1u;
    }
    return lo;
}

// the rows of the first and the last entry of the workgroup's piece, into s_r[0] and s_r[1]
__device__ __forceinline__ void mrg_piece_rows(const MrgTable &t, long long e0, long long e1, uint32_t *s_r)
{
    if (threadIdx.x < 2u) s_r[threadIdx.x] = mrg_row_of(t.offs, 0u, t.nrows - 1u, threadIdx.x == 0u ? e0 : e1 - 1);
    __syncthreads();
}

__device__ __forceinline__ uint32_t mrg_find(uint32_t *par, uint32_t x)
{
    uint32_t p = L2LOAD(&par[x]);
    while (p != x) { x = p; p = L2LOAD(&par[x]); }
    return x;
}

__device__ __forceinline__ void mrg_union(uint32_t *par, uint32_t a, uint32_t b)
{
    uint32_t ra = mrg_find(par, a), rb = mrg_find(par, b);
    // (a and b point at what was found: a root, or an id that leads to today's root)
    if (ra != a) atomicMin(&par[a], ra);
    if (rb != b) atomicMin(&par[b], rb);
    while (ra != rb) {
        if (ra < rb) { const uint32_t x = ra; ra = rb; rb = x; }       // ra > rb: hook ra under rb
        const uint32_t old = atomicMin(&par[ra], rb);
        if (old == ra) break;                                           // ra was a root: done
        ra = mrg_find(par, old);                                        // ra had been hooked meanwhile: join its parent with rb
        rb = mrg_find(par, rb);
    }
}

__global__ __launch_bounds__(256) void k_mrg_init(uint32_t *__restrict__ par, uint32_t ns)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < ns) par[i] = i;
}

__device__ __forceinline__ uint32_t mrg_wave_sum(uint32_t v)
{
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
    return v;
}

template <class Rule>
__global__ __launch_bounds__(256) void k_mrg_hook(MrgTable t, Rule q, uint32_t *par, unsigned long long *ctr)
{
    __shared__ uint32_t s_r[2];
    const long long e0 = (long long)blockIdx.x * (long long)MRG_PIECE;
    const long long e1 = e0 + (long long)MRG_PIECE < t.nent ? e0 + (long long)MRG_PIECE : t.nent;
    mrg_piece_rows(t, e0, e1, s_r);
    const uint32_t rlo = s_r[0], rhi = s_r[1];
    uint32_t nhalf = 0u, nlink = 0u;
    for (uint32_t k = 0; k < MRG_PIECE / 256u; k++) {
        const long long e = e0 + (long long)(k * 256u + threadIdx.x);
        if (e >= e1) break;
        const uint32_t b = t.ids[e];
        const uint32_t a = t.row0 + mrg_row_of(t.offs, rlo, rhi, e);
        // (row 0 has no entries and no id lies past the table in a checked table: neither is relied on here)
        if (a == 0u || a >= b || b >= t.ns) continue;
        nhalf++;
        if (!q.link(a, b, t.lens[e])) continue;
        nlink++;
        mrg_union(par, a, b);
    }
    nhalf = mrg_wave_sum(nhalf);
    nlink = mrg_wave_sum(nlink);
    if (lane_id() == 0u) {
        if (nhalf) atomicAdd(&ctr[MRG_C_HALF], (unsigned long long)nhalf);
        if (nlink) atomicAdd(&ctr[MRG_C_LINKS], (unsigned long long)nlink);
    }
}

// ---- the similarity rule's columns and per-row best -------------------------------------------------------------
// column c of ncol into the records
__global__ __launch_bounds__(256) void k_mrgs_place(const double *__restrict__ col, size_t ns, int c, int ncol,
                                                    double *__restrict__ rec)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < ns; i += (size_t)gridDim.x * 256u)
        rec[i * (size_t)ncol + (size_t)c] = col[i];
}

// an id with an ignored value (NaN, or the ignore value) in any column: its record's first value becomes NaN
__global__ __launch_bounds__(256) void k_mrgs_mark(double *__restrict__ rec, size_t ns, int ncol, int has_ign, double ign)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < ns; i += (size_t)gridDim.x * 256u) {
        bool bad = false;
        for (int c = 0; c < ncol; c++) {
            const double x = rec[i * (size_t)ncol + (size_t)c];
            bad = bad || x != x || (has_ign && x == ign);
        }
        if (bad) rec[i * (size_t)ncol] = NAN;
    }
}

// The per-row best of the mutual rule, over the pieces of the hook and EVERY entry (a row is read from its own
// side).  PASS 0: bestd[a] = the smallest d2 of row a's candidates, by a 64-bit atomicMin on its bit pattern (d2 is
// +0.0 or above: such doubles order as unsigned integers).  PASS 1, a launch later: best[a] = the smallest id among
// the candidates at that minimum.  Both arrays start at all ones.  A value already at or below what the entry
// brings needs no atomic (it only decreases), which spares a row of thousands of entries thousands of atomics on
// one word; the look goes to the L2, where the atomics land.
template <int PASS>
__global__ __launch_bounds__(256) void k_mrgs_best(MrgTable t, MrgSimRule q, unsigned long long *bestd, uint32_t *best)
{
    __shared__ uint32_t s_r[2];
    const long long e0 = (long long)blockIdx.x * (long long)MRG_PIECE;
    const long long e1 = e0 + (long long)MRG_PIECE < t.nent ? e0 + (long long)MRG_PIECE : t.nent;
    mrg_piece_rows(t, e0, e1, s_r);
    const uint32_t rlo = s_r[0], rhi = s_r[1];
    for (uint32_t k = 0; k < MRG_PIECE / 256u; k++) {
        const long long e = e0 + (long long)(k * 256u + threadIdx.x);
        if (e >= e1) break;
        const uint32_t b = t.ids[e];
        const uint32_t a = t.row0 + mrg_row_of(t.offs, rlo, rhi, e);
        if (a == 0u || a == b || b == 0u || b >= t.ns) continue;
        double d;
        if (!q.candidate(a, b, t.lens[e], d)) continue;
        const unsigned long long bits = (unsigned long long)__double_as_longlong(d);
        if (PASS == 0) {
            if (L2LOAD(&bestd[a]) > bits) atomicMin(&bestd[a], bits);
        } else {
            if (bestd[a] == bits && L2LOAD(&best[a]) > b) atomicMin(&best[a], b);
        }
    }
}

__global__ __launch_bounds__(256) void k_mrg_flatten(const uint32_t *__restrict__ par, uint32_t ns, uint32_t *__restrict__ root)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= ns) return;
    uint32_t x = i, p = par[x];
    while (p != x) { x = p; p = par[x]; }
    root[i] = x;
}

struct MrgRootFn {              // 1 where id i is the root of a group
    const uint32_t *root;
    const long long *size;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        return (i != 0u && root[i] == i && (!size || size[i] > 0)) ? 1u : 0u;
    }
};

// hist[id] += cnt of every lane with `valid`; the lanes that hold the first valid lane's id add once.  Every lane of
// the wavefront must call it.
__device__ __forceinline__ void mrg_count(unsigned long long *hist, uint32_t id, unsigned long long cnt, bool valid)
{
    const unsigned long long m = __ballot(valid);
    if (m == 0ull) return;
    const int leader = __ffsll((long long)m) - 1;
    const uint32_t id0 = (uint32_t)__shfl((int)id, leader, 64);
    const bool same = valid && id == id0;
    unsigned long long c = same ? cnt : 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) c += (unsigned long long)__shfl_xor((long long)c, d, 64);
    if ((int)lane_id() == leader) atomicAdd(&hist[id0], c);
    else if (valid && !same) atomicAdd(&hist[id], cnt);
}

// idx: the exclusive scan of MrgRootFn.  rep / gsize / hist have M + 1 rows and are zero on entry; row 0 of gsize stays
// 0, row 0 of hist receives the pixels of the ids that recode to 0.
__global__ __launch_bounds__(256) void k_mrg_write(const uint32_t *__restrict__ root, const uint32_t *__restrict__ idx,
                                                   const long long *__restrict__ size, uint32_t ns,
                                                   uint32_t *__restrict__ recode, uint32_t *__restrict__ rep,
                                                   unsigned long long *gsize, unsigned long long *hist)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool in = i < ns;
    uint32_t nid = 0u;
    long long sz = 0;
    if (in) {
        const uint32_t r = root[i];
        sz = size ? size[i] : 1;
        if (i != 0u && sz > 0) {
            nid = idx[r] + 1u;
            if (r == i) rep[nid] = i;
        }
        recode[i] = nid;
    }
    mrg_count(gsize, nid, 1ull, in && nid != 0u);
    if (size) mrg_count(hist, nid, (unsigned long long)(sz > 0 ? sz : 0), in && sz > 0);
}

__global__ __launch_bounds__(256) void k_mrg_records(MrgTable t, const uint32_t *__restrict__ recode, uint4 *__restrict__ rec,
                                                     unsigned long long cap, unsigned long long *ctr)
{
    __shared__ uint32_t s_r[2];
    const long long e0 = (long long)blockIdx.x * (long long)MRG_PIECE;
    const long long e1 = e0 + (long long)MRG_PIECE < t.nent ? e0 + (long long)MRG_PIECE : t.nent;
    mrg_piece_rows(t, e0, e1, s_r);
    const uint32_t rlo = s_r[0], rhi = s_r[1];
    const unsigned lane = lane_id();
    for (uint32_t k = 0; k < MRG_PIECE / 256u; k++) {
        const long long e = e0 + (long long)(k * 256u + threadIdx.x);      // (e0 + k * 256 is uniform: so is the loop)
        if (e0 + (long long)(k * 256u) >= e1) break;
        bool emit = false;
        uint32_t lo = 0u, hi = 0u;
        long long w = 0;
        if (e < e1) {
            const uint32_t b = t.ids[e];
            const uint32_t a = t.row0 + mrg_row_of(t.offs, rlo, rhi, e);
            if (a != 0u && a < b && b < t.ns) {
                const uint32_t ra = recode[a], rb = recode[b];
                if (ra != 0u && rb != 0u && ra != rb) {
                    emit = true;
                    lo = ra < rb ? ra : rb;
                    hi = ra < rb ? rb : ra;
                    w = t.lens[e];
                }
            }
        }
        // the wavefront reserves its records with one atomic
        const unsigned long long m = __ballot(emit);
        if (m == 0ull) continue;                                            // (uniform in the wavefront)
        const int first = __ffsll((long long)m) - 1;
        unsigned long long base = 0ull;
        if ((int)lane == first) base = atomicAdd(&ctr[MRG_C_REC], (unsigned long long)__popcll(m));
        base = (unsigned long long)__shfl((long long)base, first, 64);
        if (emit) {
            if (w < 1 || w > 0xffffffffll) { atomicAdd(&ctr[MRG_C_WIDE], 1ull); w = 0; }
            const unsigned long long p = base + (unsigned long long)__popcll(m & lanemask_lt());
            if (p < cap) rec[p] = make_uint4(hi, lo, (uint32_t)w, 0u);
        }
    }
}

__device__ __forceinline__ uint32_t mrg_new_id(const uint32_t *__restrict__ recode, uint32_t ns, uint32_t s, unsigned long long *bad)
{
    if (s < ns) return recode[s];
    atomicMax(bad, (unsigned long long)s);
    return 0u;
}

// the labels before the first 16-byte boundary of seg and behind the last whole group of four go one by one (`head`
// of them in front), as in k_colour_lookup
template <bool COUNT>
__global__ __launch_bounds__(256) void k_mrg_recode(const uint32_t *__restrict__ seg, size_t n, size_t head, int vec_out,
                                                    const uint32_t *__restrict__ recode, uint32_t ns,
                                                    uint32_t *__restrict__ out, unsigned long long *hist,
                                                    unsigned long long *bad)
{
    const size_t ngroups = (n - head) / 4u, tail = head + ngroups * 4u;
    const size_t t0 = (size_t)blockIdx.x * 256u + threadIdx.x, step = (size_t)gridDim.x * 256u;
    for (size_t qb = (size_t)blockIdx.x * 256u; qb < ngroups; qb += step) {       // (uniform in the workgroup)
        const size_t q = qb + threadIdx.x;
        const bool live = q < ngroups;
        uint32_t c[4] = {0u, 0u, 0u, 0u};
        if (live) {
            const size_t i = head + q * 4u;
            const uint4 s = *reinterpret_cast<const uint4 *>(seg + i);
            c[0] = mrg_new_id(recode, ns, s.x, bad);
            c[1] = mrg_new_id(recode, ns, s.y, bad);
            c[2] = mrg_new_id(recode, ns, s.z, bad);
            c[3] = mrg_new_id(recode, ns, s.w, bad);
            if (vec_out) {
                *reinterpret_cast<uint4 *>(out + i) = make_uint4(c[0], c[1], c[2], c[3]);
            } else {
                out[i] = c[0]; out[i + 1] = c[1]; out[i + 2] = c[2]; out[i + 3] = c[3];
            }
        }
        if (COUNT) {
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const bool first = live && (k == 0 || c[k] != c[k > 0 ? k - 1 : 0]);
                uint32_t len = 1u;
#pragma unroll
                for (int j = k + 1; j < 4; j++) {
                    if (c[j] != c[k]) break;
                    len++;
                }
                mrg_count(hist, c[k], (unsigned long long)len, first);
            }
        }
    }
    // (head < 4 and n - tail < 4)
    if (t0 < head) {
        const uint32_t v = mrg_new_id(recode, ns, seg[t0], bad);
        out[t0] = v;
        if (COUNT) atomicAdd(&hist[v], 1ull);
    }
    if (t0 < n - tail) {
        const uint32_t v = mrg_new_id(recode, ns, seg[tail + t0], bad);
        out[tail + t0] = v;
        if (COUNT) atomicAdd(&hist[v], 1ull);
    }
}

// ---- host side --------------------------------------------------------------------------------------------
static inline MrgTable mrg_table(const NbrTable &t)
{
    return MrgTable{(const long long *)t.offs.p, (const uint32_t *)t.ids.p, (const long long *)t.lens.p, t.S + 1u,
                    (long long)t.nent, t.nrows, t.row0};
}

static inline unsigned mrg_pieces(unsigned long long nent)
{
    return (unsigned)((nent + MRG_PIECE - 1u) / MRG_PIECE);
}

// S, nent: the table's last id and its entries (the context's finished table, or a rank's share table).
// The buffers of a merge, its host columns on the device (either may be NULL), zeroed counters and the parent array
// with every id its own root: what comes before the hook of either link rule.  ev[0] is recorded in front of the
// parent array's launch.  The groups of the merge before, and their member list (nbragg.h), end here.
static int mrg_begin(shp_ctx *ctx, uint32_t S, unsigned long long nent, const int64_t *keys, const int64_t *seg_size)
{
    hipStream_t st = ctx->stream;
    ctx->mrg = MrgState{};
    ctx->agg = AggState{};
    const size_t ns = (size_t)S + 1;
    if (nent > (unsigned long long)MRG_PIECE * 0x7fffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "%llu entries: too many", nent);
    if (keys) CHK(buf_ensure(ctx, ctx->mrg_key, ns * 8));
    if (seg_size) CHK(buf_ensure(ctx, ctx->mrg_size, ns * 8));
    CHK(buf_ensure(ctx, ctx->mrg_par, ns * 4));
    CHK(buf_ensure(ctx, ctx->mrg_root, ns * 4));
    CHK(buf_ensure(ctx, ctx->mrg_idx, ns * 4));
    CHK(buf_ensure(ctx, ctx->mrg_recode, ns * 4));
    CHK(buf_ensure(ctx, ctx->mrg_ctr, MRG_C_WORDS * 8));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(ns)));
    if (keys) HIPCHK(ctx, hipMemcpyAsync(ctx->mrg_key.p, keys, ns * 8, hipMemcpyHostToDevice, st));
    if (seg_size) HIPCHK(ctx, hipMemcpyAsync(ctx->mrg_size.p, seg_size, ns * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->mrg_ctr.p, 0, MRG_C_WORDS * 8, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_mrg_init, dim3(grid_for(ns, 256)), dim3(256), 0, st, bp<uint32_t>(ctx->mrg_par), (uint32_t)ns);
    KCHK(ctx);
    return 0;
}

// What follows the hook of either link rule: the roots flagged, scanned and numbered, the groups written.  ms_out[2]:
// device time since ev[0] (the hook), of the renumbering.
static int mrg_number(shp_ctx *ctx, uint32_t S, bool has_size, uint32_t *M_out, int64_t *counters_out, double *ms_out)
{
    MrgState &g = ctx->mrg;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    long long *d_size = has_size ? bp<long long>(ctx->mrg_size) : nullptr;
    uint32_t *par = bp<uint32_t>(ctx->mrg_par), *root = bp<uint32_t>(ctx->mrg_root), *idx = bp<uint32_t>(ctx->mrg_idx);
    unsigned long long *ctr = (unsigned long long *)ctx->mrg_ctr.p;
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_NBR;
    const unsigned gs = grid_for(ns, 256);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    hipLaunchKernelGGL(k_mrg_flatten, dim3(gs), dim3(256), 0, st, (const uint32_t *)par, (uint32_t)ns, root);
    KCHK(ctx);
    MrgRootFn rf{root, d_size};
    CHK(scan_exclusive(ctx, rf, (uint32_t)ns, idx, nullptr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir));
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t M = *(volatile uint32_t *)mir;
    if (M > S) SHP_FAIL(ctx, SHP_ERR_STATE, "%u groups of %u ids", M, S);
    const size_t nm = (size_t)M + 1;
    CHK(buf_ensure(ctx, ctx->mrg_rep, nm * 4));
    CHK(buf_ensure(ctx, ctx->mrg_gsize, nm * 8));
    CHK(buf_ensure(ctx, ctx->mrg_hist, nm * 8));
    HIPCHK(ctx, hipEventRecord(ctx->ev[3], st));         // (the host's read of M and the allocations are not device time)
    HIPCHK(ctx, hipMemsetAsync(ctx->mrg_rep.p, 0, nm * 4, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->mrg_gsize.p, 0, nm * 8, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->mrg_hist.p, 0, nm * 8, st));
    hipLaunchKernelGGL(k_mrg_write, dim3(gs), dim3(256), 0, st, (const uint32_t *)root, (const uint32_t *)idx,
                       (const long long *)d_size, (uint32_t)ns, bp<uint32_t>(ctx->mrg_recode), bp<uint32_t>(ctx->mrg_rep),
                       (unsigned long long *)ctx->mrg_gsize.p, (unsigned long long *)ctx->mrg_hist.p);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[4], st));
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    HIPCHK(ctx, hipMemcpyAsync(pin, ctr, MRG_C_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    if (ms_out) ms_out[0] = ms;
    float ms2 = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2]));
    HIPCHK(ctx, hipEventElapsedTime(&ms2, ctx->ev[3], ctx->ev[4]));
    if (ms_out) ms_out[1] = (double)ms + (double)ms2;
    g.S = S;
    g.M = M;
    g.links = pin[MRG_C_LINKS];
    g.half = pin[MRG_C_HALF];
    g.has_size = has_size;
    g.table_serial = ctx->nbr_tab.serial;
    g.serial = nbr_next_serial();
    g.stage = 1;
    *M_out = M;
    if (counters_out) {
        counters_out[0] = (int64_t)g.links;
        counters_out[1] = (int64_t)g.half;
    }
    return 0;
}

// The groups of the finished table under the key rule.  keys / seg_size: host, S + 1 int64 (seg_size may be NULL).
// ms_out[2]: device time of the hook, of the renumbering.
static int run_nbr_merge(shp_ctx *ctx, const int64_t *keys, int has_ign, int64_t ign, int64_t min_border,
                         const int64_t *seg_size, uint32_t *M_out, int64_t *counters_out, double *ms_out)
{
    const NbrTable &t = ctx->nbr_tab;
    const unsigned long long nent = t.nent;
    CHK(mrg_begin(ctx, t.S, nent, keys, seg_size));
    if (nent) {
        const MrgLinkRule q{bp<long long>(ctx->mrg_key), seg_size ? bp<long long>(ctx->mrg_size) : nullptr, has_ign,
                            (long long)ign, (long long)min_border};
        hipLaunchKernelGGL(k_mrg_hook<MrgLinkRule>, dim3(mrg_pieces(nent)), dim3(256), 0, ctx->stream, mrg_table(t), q,
                           bp<uint32_t>(ctx->mrg_par), (unsigned long long *)ctx->mrg_ctr.p);
        KCHK(ctx);
    }
    return mrg_number(ctx, t.S, seg_size != nullptr, M_out, counters_out, ms_out);
}

// The distance columns (ncol host columns of ns float64) through one staging plane into the records of MrgSimRule,
// ignored values marked; the mutual rule's two arrays are sized.  *ms_out: device time of the records' kernels.
static int mrgs_place_columns(shp_ctx *ctx, const double *const *cols, int ncol, size_t ns, int has_ignv, double ignv,
                              int mutual, double *ms_out)
{
    hipStream_t st = ctx->stream;
    CHK(buf_ensure(ctx, ctx->mrg_rec, ns * (size_t)ncol * 8));
    CHK(buf_ensure(ctx, ctx->img, ns * 8));
    if (mutual) {
        CHK(buf_ensure(ctx, ctx->mrg_bestd, ns * 8));
        CHK(buf_ensure(ctx, ctx->mrg_best, ns * 4));
    }
    double *rec = bp<double>(ctx->mrg_rec);
    const unsigned gc = grid_for(ns, 256, 2048u);
    float msr = 0.f, ms1 = 0.f;
    for (int c = 0; c < ncol; c++) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->img.p, cols[c], ns * 8, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipEventRecord(ctx->ev[5], st));
        hipLaunchKernelGGL(k_mrgs_place, dim3(gc), dim3(256), 0, st, (const double *)ctx->img.p, ns, c, ncol, rec);
        KCHK(ctx);
        if (c == ncol - 1) {
            hipLaunchKernelGGL(k_mrgs_mark, dim3(gc), dim3(256), 0, st, rec, ns, ncol, has_ignv, ignv);
            KCHK(ctx);
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev[6], st));
        HIPCHK(ctx, hipStreamSynchronize(st));                  // (the staging plane is free again)
        HIPCHK(ctx, hipEventElapsedTime(&ms1, ctx->ev[5], ctx->ev[6]));
        msr += ms1;
    }
    *ms_out = msr;
    return 0;
}

// The groups of the finished table under the similarity rule (MrgSimRule).  cols: ncol host columns of S + 1 float64;
// keys and seg_size may be NULL.  The columns go through one staging plane into the records, in front of ev[0].
// ms_out[3]: device time of the hook (with the two best passes of the mutual rule), of the renumbering, of the
// records' kernels.
static int run_nbr_merge_similar(shp_ctx *ctx, const double *const *cols, int ncol, int has_ignv, double ignv, int has_thr,
                                 double thr2, int mutual, const int64_t *keys, int has_ignk, int64_t ignk, int64_t min_border,
                                 const int64_t *seg_size, uint32_t *M_out, int64_t *counters_out, double *ms_out)
{
    hipStream_t st = ctx->stream;
    const NbrTable &t = ctx->nbr_tab;
    const size_t ns = (size_t)t.S + 1;
    const unsigned long long nent = t.nent;
    double msr = 0.0;
    CHK(mrgs_place_columns(ctx, cols, ncol, ns, has_ignv, ignv, mutual, &msr));
    double *rec = bp<double>(ctx->mrg_rec);
    CHK(mrg_begin(ctx, t.S, nent, keys, seg_size));
    if (nent) {
        MrgSimRule q{rec, ncol, keys ? bp<long long>(ctx->mrg_key) : nullptr, seg_size ? bp<long long>(ctx->mrg_size) : nullptr,
                     has_ignk, (long long)ignk, (long long)min_border, has_thr, thr2, nullptr};
        const dim3 grid(mrg_pieces(nent));
        if (mutual) {
            unsigned long long *bestd = (unsigned long long *)ctx->mrg_bestd.p;
            uint32_t *best = bp<uint32_t>(ctx->mrg_best);
            HIPCHK(ctx, hipMemsetAsync(bestd, 0xff, ns * 8, st));
            HIPCHK(ctx, hipMemsetAsync(best, 0xff, ns * 4, st));
            hipLaunchKernelGGL(k_mrgs_best<0>, grid, dim3(256), 0, st, mrg_table(t), q, bestd, best);
            KCHK(ctx);
            hipLaunchKernelGGL(k_mrgs_best<1>, grid, dim3(256), 0, st, mrg_table(t), q, bestd, best);
            KCHK(ctx);
            q.best = best;
        }
        hipLaunchKernelGGL(k_mrg_hook<MrgSimRule>, grid, dim3(256), 0, st, mrg_table(t), q, bp<uint32_t>(ctx->mrg_par),
                           (unsigned long long *)ctx->mrg_ctr.p);
        KCHK(ctx);
    }
    CHK(mrg_number(ctx, t.S, seg_size != nullptr, M_out, counters_out, ms_out));
    if (ms_out) ms_out[2] = msr;
    return 0;
}

// the groups to host memory; a NULL pointer skips its array
static int run_nbr_merge_groups(shp_ctx *ctx, uint32_t *recode, uint32_t *rep, int64_t *gsize, int64_t *hist)
{
    const MrgState &g = ctx->mrg;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)g.S + 1, nm = (size_t)g.M + 1;
    if (recode) HIPCHK(ctx, hipMemcpyAsync(recode, ctx->mrg_recode.p, ns * 4, hipMemcpyDeviceToHost, st));
    if (rep) HIPCHK(ctx, hipMemcpyAsync(rep, ctx->mrg_rep.p, nm * 4, hipMemcpyDeviceToHost, st));
    if (gsize) HIPCHK(ctx, hipMemcpyAsync(gsize, ctx->mrg_gsize.p, nm * 8, hipMemcpyDeviceToHost, st));
    if (hist) HIPCHK(ctx, hipMemcpyAsync(hist, ctx->mrg_hist.p, nm * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// The table of the groups replaces the table they were found in: the context's finished table, with a new serial.
// The record buffer is sized for every entry a < b, which is what the hook counted: a conservative bound (an entry
// inside a group yields no record), so a table with more than NBR_MAX_REC such entries is refused even where few
// records would come of it.  dev_ms_out: the record kernel plus nbr_build_table's interval, which like
// shp_nbr_finish's holds the host's read of the distinct-pair count.
static int run_nbr_merge_contract(shp_ctx *ctx, int64_t *nent_out, int64_t *records_out, double *dev_ms_out)
{
    MrgState &g = ctx->mrg;
    hipStream_t st = ctx->stream;
    const unsigned long long nent = ctx->nbr_tab.nent;
    unsigned long long *ctr = (unsigned long long *)ctx->mrg_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    if (g.half > NBR_MAX_REC) SHP_FAIL(ctx, SHP_ERR_NOMEM, "%llu neighbour records: more than the sort indexes", g.half);
    CHK(buf_ensure(ctx, ctx->nbr_rec, (size_t)g.half * 16));
    const unsigned long long cap = ctx->nbr_rec.cap / 16;
    float ms = 0.f;
    if (nent) {
        HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
        hipLaunchKernelGGL(k_mrg_records, dim3(mrg_pieces(nent)), dim3(256), 0, st, mrg_table(ctx->nbr_tab),
                           (const uint32_t *)ctx->mrg_recode.p, (uint4 *)ctx->nbr_rec.p, cap, ctr);
        KCHK(ctx);
        HIPCHK(ctx, hipEventRecord(ctx->ev[3], st));
    }
    HIPCHK(ctx, hipMemcpyAsync(pin, ctr, MRG_C_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (nent) HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3]));
    const unsigned long long n = pin[MRG_C_REC];
    if (pin[MRG_C_WIDE]) SHP_FAIL(ctx, SHP_ERR_ARG, "%llu border lengths outside 1 .. 2^32 - 1", pin[MRG_C_WIDE]);
    if (n > g.half || n > cap) SHP_FAIL(ctx, SHP_ERR_STATE, "%llu records of %llu entries", n, g.half);
    // from here on the table the groups were found in is gone
    ctx->nbr = NbrState{};
    nbr_table_end(ctx->nbr_tab);
    ctx->nbr_tab.serial = nbr_next_serial();
    ctx->nbr.cap = cap;
    ctx->nbr.used = n;
    g.contracted = true;
    CHK(nbr_build_table(ctx, g.M, (uint32_t)n));
    *nent_out = (int64_t)ctx->nbr_tab.nent;
    *records_out = (int64_t)n;
    if (dev_ms_out) *dev_ms_out = (double)ms + ctx->nbr.dev_ms;
    return 0;
}

// d_out[p] = recode[d_seg[p]] for npix labels; *bad_out: 0, or the largest label above S among them (their pixels
// become 0).  count: the new ids are added to the groups' histogram.
static int run_nbr_merge_recode(shp_ctx *ctx, const uint32_t *d_seg, size_t n, uint32_t *d_out, int count, uint32_t *bad_out,
                                double *dev_ms_out)
{
    const MrgState &g = ctx->mrg;
    hipStream_t st = ctx->stream;
    *bad_out = 0u;
    if (dev_ms_out) *dev_ms_out = 0.0;
    if (n == 0) return 0;
    unsigned long long *ctr = (unsigned long long *)ctx->mrg_ctr.p;
    unsigned long long *pin = (unsigned long long *)ctx->h_pinned;
    HIPCHK(ctx, hipMemsetAsync(&ctr[MRG_C_BAD], 0, 8, st));
    size_t head = ((16u - ((uintptr_t)d_seg & 15u)) & 15u) / 4u;
    if (head > n) head = n;
    const int vec_out = ((uintptr_t)(d_out + head) & 15u) == 0;
    const unsigned grid = grid_for((n - head) / 4u + 1u, 256, 2048u);
    const uint32_t ns = g.S + 1u;
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (count)
        hipLaunchKernelGGL(k_mrg_recode<true>, dim3(grid), dim3(256), 0, st, d_seg, n, head, vec_out,
                           (const uint32_t *)ctx->mrg_recode.p, ns, d_out, (unsigned long long *)ctx->mrg_hist.p,
                           &ctr[MRG_C_BAD]);
    else
        hipLaunchKernelGGL(k_mrg_recode<false>, dim3(grid), dim3(256), 0, st, d_seg, n, head, vec_out,
                           (const uint32_t *)ctx->mrg_recode.p, ns, d_out, (unsigned long long *)nullptr, &ctr[MRG_C_BAD]);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(pin, &ctr[MRG_C_BAD], 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    *bad_out = (uint32_t)pin[0];
    if (dev_ms_out) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        *dev_ms_out = ms;
    }
    return 0;
}
