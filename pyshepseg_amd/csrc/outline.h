// outline.h -- the outline of every segment as rings of vertices, traced from the label raster
// (outlines.traceSegmentOutlines).  segshape.h counts the boundary sides; this puts them in order.  Integer work
// throughout: no launch geometry, atomic order or round count can change a bit of the result.
//
// Pixel (y, x) covers [y, y + 1] x [x, x + 1], corners are (row, col) pairs, label 0 is no segment.  A side of a pixel
// of id A is an EDGE of A when the label across it is not A (another id, 0, outside the raster).  Edges are directed
// with A's pixel on the right: side 0 (N) (y, x) -> (y, x + 1), 1 (E) (y, x + 1) -> (y + 1, x + 1), 2 (S) (y + 1, x + 1)
// -> (y + 1, x), 3 (W) (y + 1, x) -> (y, x).  Its key is (y, x, side).  At its end corner, with R / L = the pixel
// right-ahead / left-ahead is A: not R turns right (next side of the same pixel), R and not L goes straight (same side
// of the pixel right-ahead), R and L turns left (side - 1 of the pixel left-ahead); the saddle (not R, L) turns right
// for four-connected segments and left for eight-connected ones.  Every edge has one successor and one predecessor, so
// the successor map is a permutation and its cycles are the rings.  A TURN EDGE is an edge whose predecessor has
// another side; its start corner is a vertex.  A ring starts at its turn edge of the smallest key, its LEADER.
//
// The whole raster is in device memory.  Steps (all workgroups OL_BLOCK = 256 threads, a thread per pixel, edge, ring,
// vertex or id; no LDS tiles):
//  1. k_ol_mask: a byte per pixel, bit s = side s is an edge (0 for label 0 and for labels above max_seg_id, the
//     largest of which goes to a device word); at most OL_MASK_GRID = 4096 workgroups, which stride over the raster
//     and add their edges to a 64-bit count (the scan's total is 32 bits and would wrap unseen).  scan.h over the bytes' population counts gives every pixel the index of
//     its first edge: edge indices are compact, below 2^32, and ascend with the key, so "smallest key" is "smallest
//     index".  k_ol_link: per edge its successor's index, from the 3 x 3 labels round its pixel and the successor
//     pixel's offset and byte; whether it is a turn edge, from the two pixels behind its start corner (the predecessor
//     went straight if and only if the pixel right-behind is A and the pixel left-behind is not); its pixel and side.
//  2., 3. k_ol_round, pointer doubling, leader and rank in one state of 16 bytes per edge: for the window of 2^k edges
//     that starts at e, (j, m, c, t) = the edge after the window, the smallest turn edge in it (OL_NONE: none), the turn
//     edges before that one, the turn edges in the window (modulo 2^32).  A round joins the window at e with the window
//     at j: t adds, and the second window's minimum wins only if smaller (m is then its m, c the first window's t plus
//     its c).  A round READS one buffer and WRITES the other: a round that jumped in place would read states other
//     lanes are replacing.  The host launches round after round and reads a device word a round sets when a window
//     minimum changed.  While a ring is longer than the window, the window that ends just before the leader changes;
//     so a round without a change proves that every m is its ring's leader, and c the turn edges from e up to the
//     leader.  That takes ceil(log2(longest ring)) + 1 rounds; more than ceil(log2(edges)) + 2 is an error, never a
//     loop.  No kernel waits for another workgroup.
//  4. The leaders (m == own index) are counted by a scan and numbered in key order; k_ol_turns counts every ring's
//     turn edges T (atomic adds, a wavefront's lanes of one ring together); sort.h's stable sort_pairs by id puts the
//     rings in (id, leader key) order; a scan of T in that order gives the vertex offsets; k_ol_emit writes the start
//     corner of turn edge e to place offset + (c ? T - c : 0), origin added; k_ol_area adds every vertex's term
//     c_i r_(i+1) - c_(i+1) r_i (raster coordinates, below 2^32 in magnitude) to its ring's int64 (integer atomics, a
//     wavefront's lanes of one ring together); k_ol_ring_offsets finds every id's first ring in the sorted ids.
//
// Device memory beside the labels (4 bytes a pixel): 5 bytes a pixel (byte, offset); 37 bytes an edge (pixel 4, side
// and turn flag 1, the two state buffers 16 each; the ring number of an edge lives in the state buffer that is free
// after the last round); 16 bytes a vertex; 36 bytes a ring plus the sort's 16; 8 bytes an id.
//
// The junction switch (shp_outline_junctions, set between the edges and the trace, gone with the next edges): the
// edges whose start corner is a junction -- three or four of the four neighbouring pairs of the pixels round it differ
// -- are vertex edges like the turn edges, so a ring gets a collinear vertex where it runs straight through such a
// corner, and a flag byte per vertex (ol_jflag) says which vertices lie on junctions.  simplify.h cuts the rings there.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"

#define OL_BLOCK 256u               // threads per workgroup of every kernel here
#define OL_NONE 0xFFFFFFFFu
#define OL_MAX_ITEMS 0xFFFFE000u    // pixels, and edges: scan.h indexes a block's SCAN_ITEMS items past n with 32 bits
#define OL_MAX_ROUNDS 40

// device words of ol_ctr: [0] largest label above S, [2..3] edges (64 bits), [8 + r] round r changed a minimum
#define OL_CTR_WORDS (8u + OL_MAX_ROUNDS)

struct OlGeom {
    const uint32_t *seg;
    uint32_t nrows, ncols, npix, S;
};

// a workgroup takes every gridDim.x-th block of OL_BLOCK pixels, so that the grid's wavefronts, not the raster's, each
// add their edges to the one 64-bit count (OL_MASK_GRID workgroups at most: an atomic per wavefront of the raster
// took 50 ms of the 16384^2 mosaic's 77)
#define OL_MASK_GRID 4096u
__global__ __launch_bounds__(256) void k_ol_mask(OlGeom g, uint8_t *__restrict__ mask, uint32_t *__restrict__ ctr)
{
    uint32_t n = 0u, bad = 0u;
    for (size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x; i < g.npix; i += (size_t)gridDim.x * OL_BLOCK) {
        const uint32_t p = (uint32_t)i, y = p / g.ncols, x = p - y * g.ncols;
        const uint32_t a = g.seg[p];
        uint32_t m = 0u;
        if (a > g.S) bad = max(bad, a);
        else if (a != 0u) {
            if (y == 0u || g.seg[p - g.ncols] != a) m |= 1u;
            if (x + 1u == g.ncols || g.seg[p + 1u] != a) m |= 2u;
            if (y + 1u == g.nrows || g.seg[(size_t)p + g.ncols] != a) m |= 4u;
            if (x == 0u || g.seg[p - 1u] != a) m |= 8u;
        }
        mask[p] = (uint8_t)m;
        n += __popc(m);
    }
    // (a thread counts at most 4 edges for each of its 2^32 / (OL_MASK_GRID * OL_BLOCK) pixels)
    unsigned long long nn = n;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        nn += (unsigned long long)__shfl_xor(nn, d, 64);
        bad = max(bad, (uint32_t)__shfl_xor(bad, d, 64));
    }
    if (lane_id() == 0u) {
        if (nn) atomicAdd((unsigned long long *)(ctr + 2), nn);
        if (bad && bad > L2LOAD(&ctr[0])) atomicMax(&ctr[0], bad);
    }
}

struct OlCountFn {          // edges of pixel i
    const uint8_t *m;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return __popc((uint32_t)m[i]); }
    __device__ __forceinline__ bool get4(uint32_t base, uint32_t v[4]) const
    {
        if (((uintptr_t)m & 3u) != 0u) return false;
        const uint32_t w = *(const uint32_t *)(m + base);
        v[0] = __popc(w & 0xffu); v[1] = __popc(w & 0xff00u); v[2] = __popc(w & 0xff0000u); v[3] = __popc(w & 0xff000000u);
        return true;
    }
};

// st[e] = (successor, e if a vertex edge else OL_NONE, 0, 1 if a vertex edge else 0); epix[e], eside[e] = side | vertex
// << 2 | junction << 3.  A vertex edge is a turn edge; with JUNC (the junction switch, shp_outline_junctions) also an
// edge whose start corner is a JUNCTION: of the four pixels round the corner, labels outside the raster read as 0, at
// least three of the four neighbouring pairs differ.  Those four are this pixel, the pixel across the side and the two
// behind the corner, all among the 3 x 3; the plain instance keeps no labels and is the kernel it always was.
template <bool JUNC>
__global__ __launch_bounds__(256) void k_ol_link(OlGeom g, int eight, const uint8_t *__restrict__ mask,
                                                 const uint32_t *__restrict__ off, uint32_t n, uint4 *__restrict__ st,
                                                 uint32_t *__restrict__ epix, uint8_t *__restrict__ eside)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= g.npix) return;
    const uint32_t p = (uint32_t)i;
    const uint32_t m = mask[p];
    if (m == 0u) return;
    const int y = (int)(p / g.ncols), x = (int)(p - (uint32_t)y * g.ncols);
    const uint32_t a = g.seg[p];
    // eq bit (dy + 1) * 3 + (dx + 1): the pixel at (y + dy, x + dx) is A
    uint32_t eq = 0u;
    uint32_t lab[9];
#pragma unroll
    for (int dy = -1; dy <= 1; dy++)
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int yy = y + dy, xx = x + dx;
            if constexpr (JUNC) {
                const uint32_t v = (yy >= 0 && yy < (int)g.nrows && xx >= 0 && xx < (int)g.ncols)
                                       ? g.seg[(size_t)yy * g.ncols + (size_t)xx] : 0u;
                lab[(dy + 1) * 3 + (dx + 1)] = v;
                if (v == a) eq |= 1u << ((dy + 1) * 3 + (dx + 1));
            } else {
                if (yy >= 0 && yy < (int)g.nrows && xx >= 0 && xx < (int)g.ncols &&
                    g.seg[(size_t)yy * g.ncols + (size_t)xx] == a)
                    eq |= 1u << ((dy + 1) * 3 + (dx + 1));
            }
        }
    const uint32_t e0 = off[p];
    constexpr int DY[4] = {0, 1, 0, -1}, DX[4] = {1, 0, -1, 0};
#pragma unroll
    for (int s = 0; s < 4; s++) {
        if (!(m & (1u << s))) continue;
        const uint32_t e = e0 + __popc(m & ((1u << s) - 1u));
        const int dy = DY[s], dx = DX[s], ay = DY[(s + 3) & 3], ax = DX[(s + 3) & 3];
        const bool R = (eq >> ((dy + 1) * 3 + (dx + 1))) & 1u;
        const bool L = (eq >> ((dy + ay + 1) * 3 + (dx + ax + 1))) & 1u;
        const bool RB = (eq >> ((1 - dy) * 3 + (1 - dx))) & 1u;
        const bool LB = (eq >> ((1 - dy + ay) * 3 + (1 - dx + ax))) & 1u;
        uint32_t succ;
        if (R && !L) {                              // straight: the same side of the pixel right-ahead
            const uint32_t q = (uint32_t)((long long)p + (long long)dy * (long long)g.ncols + dx);
            succ = off[q] + __popc((uint32_t)mask[q] & ((1u << s) - 1u));
        } else if (L && (R || eight)) {             // left: side - 1 of the pixel left-ahead
            const uint32_t q = (uint32_t)((long long)p + (long long)(dy + ay) * (long long)g.ncols + (dx + ax));
            const int t = (s + 3) & 3;
            succ = off[q] + __popc((uint32_t)mask[q] & ((1u << t) - 1u));
        } else {                                    // right: the next side of this pixel
            const int t = (s + 1) & 3;
            succ = e0 + __popc(m & ((1u << t) - 1u));
        }
        bool turn = !(RB && !LB);
        uint32_t junc = 0u;
        if constexpr (JUNC) {
            // round the start corner: this pixel, the pixel across the side, the pixel left-behind, the pixel right-behind
            const uint32_t across = lab[(ay + 1) * 3 + (ax + 1)], lb = lab[(1 - dy + ay) * 3 + (1 - dx + ax)];
            const uint32_t rb = lab[(1 - dy) * 3 + (1 - dx)];
            const uint32_t degree = (a != across ? 1u : 0u) + (across != lb ? 1u : 0u) + (lb != rb ? 1u : 0u) + (rb != a ? 1u : 0u);
            junc = degree >= 3u ? 8u : 0u;
            turn = turn || junc != 0u;
        }
        if (e >= n) continue;                       // (cannot happen: off[] and mask[] count the same sides)
        if (succ >= n) succ = e;
        st[e] = make_uint4(succ, turn ? e : OL_NONE, 0u, turn ? 1u : 0u);
        epix[e] = p;
        eside[e] = (uint8_t)((uint32_t)s | (turn ? 4u : 0u) | junc);
    }
}

// one doubling round: out[e] = in[e] joined with in[in[e].x]; *flag is set when a window minimum changed
__global__ __launch_bounds__(256) void k_ol_round(const uint4 *__restrict__ in, uint4 *__restrict__ out, uint32_t n,
                                                  uint32_t *__restrict__ flag)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    bool changed = false;
    if (i < n) {
        const uint4 a = in[i];
        const uint4 b = in[a.x];
        uint4 o = make_uint4(b.x, a.y, a.z, a.w + b.w);
        if (b.y < a.y) { o.y = b.y; o.z = a.w + b.z; changed = true; }
        out[i] = o;
    }
    if (__ballot(changed) != 0ull && lane_id() == 0u && L2LOAD(flag) == 0u) atomicOr(flag, 1u);
}

struct OlLeaderFn {         // edge i is its ring's leader
    const uint4 *st;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return st[i].y == i ? 1u : 0u; }
};

// ring r (leaders in key order): its leader edge and its id
__global__ __launch_bounds__(256) void k_ol_rings(OlGeom g, const uint4 *__restrict__ st, const uint32_t *__restrict__ lnum,
                                                  const uint32_t *__restrict__ epix, uint32_t n,
                                                  uint32_t *__restrict__ ring_id)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= n || st[i].y != (uint32_t)i) return;
    ring_id[lnum[i]] = g.seg[epix[i]];
}

// adds v to acc[key] for every lane with key != OL_NONE; the lanes that share the first lane's key add once
template <class T>
__device__ __forceinline__ void ol_wave_add(T *acc, uint32_t key, T v)
{
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
    const bool same = key == k0;
    T s = same ? v : (T)0;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += (T)__shfl_xor(s, d, 64);
    if (k0 != OL_NONE && lane_id() == (unsigned)__builtin_ctzll(__ballot(true)) && s != (T)0) atomicAdd(&acc[k0], s);
    if (!same && key != OL_NONE && v != (T)0) atomicAdd(&acc[key], v);
}

// T[r] = turn edges of ring r
__global__ __launch_bounds__(256) void k_ol_turns(const uint4 *__restrict__ st, const uint32_t *__restrict__ lnum,
                                                  const uint8_t *__restrict__ eside, uint32_t n, uint32_t *__restrict__ T)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    uint32_t key = OL_NONE;
    if (i < n && (eside[i] & 4u)) {
        const uint32_t lead = st[i].y;
        if (lead < n) key = lnum[lead];
    }
    ol_wave_add<uint32_t>(T, key, key != OL_NONE ? 1u : 0u);
}

// place k of the sorted order holds ring order[k]: pos[ring] = k, Ts[k] = its turn edges
__global__ __launch_bounds__(256) void k_ol_place(const uint32_t *__restrict__ order, const uint32_t *__restrict__ T, uint32_t n,
                                                  uint32_t *__restrict__ pos, uint32_t *__restrict__ Ts)
{
    const size_t k = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (k >= n) return;
    const uint32_t r = order[k];
    pos[r] = (uint32_t)k;
    Ts[k] = T[r];
}

__global__ __launch_bounds__(256) void k_ol_emit(OlGeom g, const uint4 *__restrict__ st, const uint32_t *__restrict__ lnum,
                                                 const uint32_t *__restrict__ epix, const uint8_t *__restrict__ eside, uint32_t n,
                                                 const uint32_t *__restrict__ pos, const uint32_t *__restrict__ T,
                                                 const uint32_t *__restrict__ voff, uint32_t nverts, long long row0,
                                                 long long col0, longlong2 *__restrict__ vtx, uint8_t *__restrict__ jflag)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t sd = eside[i];
    if (!(sd & 4u)) return;
    const uint4 a = st[i];
    if (a.y >= n) return;
    const uint32_t r = lnum[a.y];
    const uint32_t at = voff[pos[r]] + (a.z ? T[r] - a.z : 0u);
    const uint32_t p = epix[i], y = p / g.ncols, x = p - y * g.ncols, s = sd & 3u;
    // start corner: N (y, x), E (y, x + 1), S (y + 1, x + 1), W (y + 1, x)
    if (at >= nverts) return;                       // (cannot happen: c < T for every turn edge of a ring)
    vtx[at] = make_longlong2(row0 + (long long)y + (s >= 2u ? 1 : 0), col0 + (long long)x + ((s == 1u || s == 2u) ? 1 : 0));
    if (jflag) jflag[at] = (uint8_t)((sd >> 3) & 1u);       // (only with the junction switch)
}

// the ring of vertex v: the last k with voff[k] <= v
__device__ __forceinline__ uint32_t ol_ring_of(const uint32_t *__restrict__ voff, uint32_t nrings, uint32_t v)
{
    uint32_t lo = 0u, hi = nrings;          // voff[lo] <= v < voff[hi] (voff[nrings] = the vertices)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (voff[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(256) void k_ol_area(const longlong2 *__restrict__ vtx, const uint32_t *__restrict__ voff,
                                                 uint32_t nrings, uint32_t nverts, long long row0, long long col0,
                                                 unsigned long long *__restrict__ area2)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    uint32_t key = OL_NONE;
    unsigned long long term = 0ull;
    if (i < nverts) {
        const uint32_t v = (uint32_t)i, k = ol_ring_of(voff, nrings, v);
        const uint32_t end = k + 1u < nrings ? voff[k + 1u] : nverts;
        const uint32_t nx = v + 1u == end ? voff[k] : v + 1u;
        const longlong2 a = vtx[v], b = vtx[nx];
        const long long ra = a.x - row0, ca = a.y - col0, rb = b.x - row0, cb = b.y - col0;
        term = (unsigned long long)(ca * rb - cb * ra);
        key = k;
    }
    ol_wave_add<unsigned long long>(area2, key, term);
}

// roff[i] = rings of the ids below i (i = 0 .. S + 1): the first place of the sorted ids that holds i or more
__global__ __launch_bounds__(256) void k_ol_ring_offsets(const uint32_t *__restrict__ ids, uint32_t nrings, size_t n,
                                                         long long *__restrict__ roff)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= n) return;
    uint32_t lo = 0u, hi = nrings;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((size_t)ids[mid] < i) lo = mid + 1u; else hi = mid;
    }
    roff[i] = (long long)lo;
}

// voff64[k] = voff[k] for k < nrings, the vertices for k = nrings
__global__ __launch_bounds__(256) void k_ol_widen(const uint32_t *__restrict__ voff, uint32_t nrings, uint32_t nverts,
                                                  long long *__restrict__ voff64)
{
    const size_t k = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (k <= nrings) voff64[k] = k < nrings ? (long long)voff[k] : (long long)nverts;
}

// ---- host side --------------------------------------------------------------------------------------------
static inline size_t ol_grown(const DevBuf &b, size_t bytes)       // what buf_ensure would allocate
{
    if (bytes == 0) bytes = 16;
    return b.cap >= bytes ? 0 : bytes + bytes / 8 + 256;
}
// bytes of a ring's rows in ol_ring: leader id, T, pos, Ts and the vertex offset (4 each), area2 (8), offset as int64 (8)
#define OL_RING_BYTES 36u

// the device memory the buffers still have to grow by: for the pixels' step (edges < 0) or for the edges' steps,
// where vertices (at most the edges) and rings (at most a quarter of them) are not known yet
static int run_outline_need(shp_ctx *ctx, unsigned long long npix, long long edges, long long *need_out, long long *free_out)
{
    size_t need = 0;
    if (edges < 0) {
        need += ol_grown(ctx->ol_mask, npix) + ol_grown(ctx->ol_off, npix * 4) + ol_grown(ctx->ol_ctr, OL_CTR_WORDS * 4);
        need += ol_grown(ctx->scan_tmp, scan_tmp_bytes(npix));
    } else {
        const size_t n = (size_t)edges, nr = n / 4 + 1;
        need += ol_grown(ctx->ol_epix, n * 4) + ol_grown(ctx->ol_eside, n) + ol_grown(ctx->ol_a, n * 16) + ol_grown(ctx->ol_b, n * 16);
        need += ol_grown(ctx->ol_vtx, n * 16) + ol_grown(ctx->ol_ring, (nr + 2) * OL_RING_BYTES);
        need += ol_grown(ctx->sort_k0, nr * 4) + ol_grown(ctx->sort_k1, nr * 4) + ol_grown(ctx->sort_v1, nr * 4) + ol_grown(ctx->pix, nr * 4);
        need += ol_grown(ctx->scan_tmp, scan_tmp_bytes(n));
        if (ctx->outline.stage == 1 && ctx->outline.junctions) need += ol_grown(ctx->ol_jflag, n);
    }
    size_t fr = 0, tot = 0;
    HIPCHK(ctx, hipMemGetInfo(&fr, &tot));
    *need_out = (long long)need;
    *free_out = (long long)fr;
    return 0;
}

static inline double ol_elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}

// step 1, first half: the sides that are edges and every pixel's first edge index
static int run_outline_edges(shp_ctx *ctx, const uint32_t *d_seg, uint32_t nrows, uint32_t ncols, uint32_t S, int eight,
                             long long *edges_out, uint32_t *bad_out)
{
    OutlineState &o = ctx->outline;
    hipStream_t st = ctx->stream;
    o = OutlineState{};
    o.serial = ctx->outline_calls;
    const uint32_t npix = nrows * ncols;
    CHK(buf_ensure(ctx, ctx->ol_ctr, OL_CTR_WORDS * 4));
    CHK(buf_ensure(ctx, ctx->ol_mask, npix));
    CHK(buf_ensure(ctx, ctx->ol_off, (size_t)npix * 4));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(npix)));
    uint32_t *ctr = bp<uint32_t>(ctx->ol_ctr);
    HIPCHK(ctx, hipMemsetAsync(ctr, 0, OL_CTR_WORDS * 4, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    const OlGeom g{d_seg, nrows, ncols, npix, S};
    if (npix) {
        hipLaunchKernelGGL(k_ol_mask, dim3(grid_for(npix, OL_BLOCK, OL_MASK_GRID)), dim3(OL_BLOCK), 0, st, g, bp<uint8_t>(ctx->ol_mask), ctr);
        KCHK(ctx);
        OlCountFn f{bp<uint8_t>(ctx->ol_mask)};
        CHK(scan_exclusive(ctx, f, npix, bp<uint32_t>(ctx->ol_off), nullptr, bp<uint32_t>(ctx->scan_tmp)));
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    o.ms[0] = ol_elapsed(ctx->ev[0], ctx->ev[1]);
    const volatile uint32_t *h = (const volatile uint32_t *)ctx->h_pinned;
    const unsigned long long edges = (unsigned long long)h[2] | ((unsigned long long)h[3] << 32);
    *bad_out = h[0];
    *edges_out = (long long)edges;
    if (h[0] || edges > OL_MAX_ITEMS) return 0;         // nothing to trace: the caller reports it
    o.seg = d_seg; o.nrows = nrows; o.ncols = ncols; o.S = S; o.eight = eight;
    o.edges = (uint32_t)edges;
    o.stage = 1;
    return 0;
}

static int run_outline_trace(shp_ctx *ctx, long long row0, long long col0)
{
    OutlineState &o = ctx->outline;
    hipStream_t st = ctx->stream;
    const uint32_t n = o.edges, npix = o.nrows * o.ncols;
    const OlGeom g{o.seg, o.nrows, o.ncols, npix, o.S};
    uint32_t *ctr = bp<uint32_t>(ctx->ol_ctr);
    volatile uint32_t *h = (volatile uint32_t *)ctx->h_pinned;
    o.stage = 0;
    o.rings = o.verts = o.rounds = 0u;
    o.has_flags = false;
    CHK(buf_ensure(ctx, ctx->ol_roff, ((size_t)o.S + 2) * 8));
    long long *roff = bp<long long>(ctx->ol_roff);
    if (n == 0u) {                                      // no edges: no rings
        HIPCHK(ctx, hipMemsetAsync(roff, 0, ((size_t)o.S + 2) * 8, st));
        CHK(buf_ensure(ctx, ctx->ol_ring, OL_RING_BYTES * 2));
        HIPCHK(ctx, hipMemsetAsync(ctx->ol_ring.p, 0, OL_RING_BYTES * 2, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        o.voff64_at = 0;
        o.area_at = 16;
        o.has_flags = o.junctions != 0;
        o.stage = 2;
        return 0;
    }
    CHK(buf_ensure(ctx, ctx->ol_epix, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->ol_eside, n));
    CHK(buf_ensure(ctx, ctx->ol_a, (size_t)n * 16));
    CHK(buf_ensure(ctx, ctx->ol_b, (size_t)n * 16));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(n)));
    uint32_t *epix = bp<uint32_t>(ctx->ol_epix);
    uint8_t *eside = bp<uint8_t>(ctx->ol_eside);
    uint4 *buf[2] = {bp<uint4>(ctx->ol_a), bp<uint4>(ctx->ol_b)};
    const unsigned egrid = grid_for(n, OL_BLOCK);
    // ---- step 1, second half: successors, turn edges
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (o.junctions)
        hipLaunchKernelGGL(k_ol_link<true>, dim3(grid_for(npix, OL_BLOCK)), dim3(OL_BLOCK), 0, st, g, o.eight,
                           bp<uint8_t>(ctx->ol_mask), bp<uint32_t>(ctx->ol_off), n, buf[0], epix, eside);
    else
        hipLaunchKernelGGL(k_ol_link<false>, dim3(grid_for(npix, OL_BLOCK)), dim3(OL_BLOCK), 0, st, g, o.eight,
                           bp<uint8_t>(ctx->ol_mask), bp<uint32_t>(ctx->ol_off), n, buf[0], epix, eside);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    // ---- steps 2 and 3: doubling rounds until one changes no minimum
    uint32_t max_rounds = 2u;
    while ((1ull << (max_rounds - 2u)) < (unsigned long long)n) max_rounds++;       // ceil(log2(n)) + 2
    int cur = 0;
    bool settled = false;
    for (uint32_t r = 0; r < max_rounds && !settled; r++) {
        hipLaunchKernelGGL(k_ol_round, dim3(egrid), dim3(OL_BLOCK), 0, st, (const uint4 *)buf[cur], buf[cur ^ 1], n, ctr + 8 + r);
        KCHK(ctx);
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr + 8 + r, 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        cur ^= 1;
        o.rounds = r + 1u;
        settled = h[0] == 0u;
    }
    if (!settled)
        SHP_FAIL(ctx, SHP_ERR_STATE, "outline: the window minima still change after %u doubling rounds over %u edges", o.rounds, n);
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    // ---- step 4: number the leaders, order the rings, emit
    const uint4 *fin = buf[cur];
    uint32_t *lnum = (uint32_t *)buf[cur ^ 1];          // (that buffer is free now: 4 of its 16 bytes an edge)
    OlLeaderFn lf{fin};
    CHK(scan_exclusive(ctx, lf, n, lnum, ctr + 4, bp<uint32_t>(ctx->scan_tmp)));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr + 4, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nr = h[0];
    if (nr == 0u || nr > n / 4u) SHP_FAIL(ctx, SHP_ERR_STATE, "outline: %u rings over %u edges", nr, n);
    // ol_ring: ring_id, T, pos, Ts, voff (nr uint32 each, 16-byte aligned starts), then voff64 (nr + 1) and area2 (nr)
    const size_t q = ((size_t)nr + 3) & ~(size_t)3;
    CHK(buf_ensure(ctx, ctx->ol_ring, q * 20 + ((size_t)nr + 2) * 8 + (size_t)nr * 8));
    uint32_t *ring_id = bp<uint32_t>(ctx->ol_ring), *T = ring_id + q, *pos = T + q, *Ts = pos + q, *voff = Ts + q;
    long long *voff64 = (long long *)(voff + q);
    unsigned long long *area2 = (unsigned long long *)(voff64 + nr + 2);
    HIPCHK(ctx, hipMemsetAsync(T, 0, (size_t)nr * 4, st));
    HIPCHK(ctx, hipMemsetAsync(area2, 0, (size_t)nr * 8, st));
    hipLaunchKernelGGL(k_ol_rings, dim3(egrid), dim3(OL_BLOCK), 0, st, g, fin, (const uint32_t *)lnum, (const uint32_t *)epix, n, ring_id);
    KCHK(ctx);
    hipLaunchKernelGGL(k_ol_turns, dim3(egrid), dim3(OL_BLOCK), 0, st, fin, (const uint32_t *)lnum, (const uint8_t *)eside, n, T);
    KCHK(ctx);
    uint32_t *ids_sorted = nullptr, *order = nullptr;
    CHK(sort_pairs(ctx, ring_id, nullptr, nr, bits_for(o.S), &ids_sorted, &order));
    hipLaunchKernelGGL(k_ol_place, dim3(grid_for(nr, OL_BLOCK)), dim3(OL_BLOCK), 0, st, (const uint32_t *)order, (const uint32_t *)T, nr, pos, Ts);
    KCHK(ctx);
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(nr)));
    ArrFn tf{Ts};
    CHK(scan_exclusive(ctx, tf, nr, voff, ctr + 5, bp<uint32_t>(ctx->scan_tmp)));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr + 5, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nv = h[0];
    if (nv < 4u * nr || nv > n) SHP_FAIL(ctx, SHP_ERR_STATE, "outline: %u vertices in %u rings over %u edges", nv, nr, n);
    CHK(buf_ensure(ctx, ctx->ol_vtx, (size_t)nv * 16));
    longlong2 *vtx = bp<longlong2>(ctx->ol_vtx);
    uint8_t *jflag = nullptr;
    if (o.junctions) {
        CHK(buf_ensure(ctx, ctx->ol_jflag, nv));
        jflag = bp<uint8_t>(ctx->ol_jflag);
    }
    hipLaunchKernelGGL(k_ol_emit, dim3(egrid), dim3(OL_BLOCK), 0, st, g, fin, (const uint32_t *)lnum, (const uint32_t *)epix,
                       (const uint8_t *)eside, n, (const uint32_t *)pos, (const uint32_t *)T, (const uint32_t *)voff, nv, row0, col0, vtx,
                       jflag);
    KCHK(ctx);
    hipLaunchKernelGGL(k_ol_area, dim3(grid_for(nv, OL_BLOCK)), dim3(OL_BLOCK), 0, st, (const longlong2 *)vtx, (const uint32_t *)voff,
                       nr, nv, row0, col0, area2);
    KCHK(ctx);
    hipLaunchKernelGGL(k_ol_ring_offsets, dim3(grid_for((size_t)o.S + 2, OL_BLOCK)), dim3(OL_BLOCK), 0, st,
                       (const uint32_t *)ids_sorted, nr, (size_t)o.S + 2, roff);
    KCHK(ctx);
    hipLaunchKernelGGL(k_ol_widen, dim3(grid_for((size_t)nr + 1, OL_BLOCK)), dim3(OL_BLOCK), 0, st, (const uint32_t *)voff, nr, nv, voff64);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[3], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    o.ms[1] = ol_elapsed(ctx->ev[0], ctx->ev[1]);
    o.ms[2] = ol_elapsed(ctx->ev[1], ctx->ev[2]);
    o.ms[3] = ol_elapsed(ctx->ev[2], ctx->ev[3]);
    o.rings = nr;
    o.verts = nv;
    o.voff64_at = (size_t)((char *)voff64 - (char *)ctx->ol_ring.p);
    o.area_at = (size_t)((char *)area2 - (char *)ctx->ol_ring.p);
    o.has_flags = o.junctions != 0;
    o.stage = 2;
    return 0;
}

static int run_outline_download(shp_ctx *ctx, int64_t *ring_offsets, int64_t *vertex_offsets, int64_t *vertices, int64_t *ring_area2)
{
    const OutlineState &o = ctx->outline;
    hipStream_t st = ctx->stream;
    const char *ring = (const char *)ctx->ol_ring.p;
    HIPCHK(ctx, hipMemcpyAsync(ring_offsets, ctx->ol_roff.p, ((size_t)o.S + 2) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(vertex_offsets, ring + o.voff64_at, ((size_t)o.rings + 1) * 8, hipMemcpyDeviceToHost, st));
    if (o.rings) HIPCHK(ctx, hipMemcpyAsync(ring_area2, ring + o.area_at, (size_t)o.rings * 8, hipMemcpyDeviceToHost, st));
    if (o.verts) HIPCHK(ctx, hipMemcpyAsync(vertices, ctx->ol_vtx.p, (size_t)o.verts * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

static int run_outline_download_junction(shp_ctx *ctx, uint8_t *junction)
{
    const OutlineState &o = ctx->outline;
    if (o.verts) HIPCHK(ctx, hipMemcpyAsync(junction, ctx->ol_jflag.p, o.verts, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
