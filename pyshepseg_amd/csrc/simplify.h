// simplify.h -- topology-aware Douglas-Peucker simplification of the outline rings (outlines.simplifySegmentOutlines).
// Integer work throughout: no launch geometry, atomic order, size class or round count can change a bit of the result.
//
// Input: rings as outline.h leaves them with the junction switch on (vertices as (row, col) int64 pairs, int64 vertex
// offsets per ring, int64 ring offsets per id, ringArea2, a junction flag per vertex), still in the context's outline
// buffers (read in place) or uploaded into buffers of this file's own (sp_vtx, sp_voff, sp_roff, sp_area, sp_jflag):
// rings.h decides and makes the view.  (r0, c0) = the smallest row and column of all
// vertices; the host has checked that the spans H and W satisfy H W <= 2^32 and max(H, W) < 2^31, so coordinates
// relative to (r0, c0) fit 31 bits, every cross product stays within 2^33 and every squared distance fits int64.
//
// Definitions.  A ring's ANCHORS are its flagged vertices; a ring without any takes its vertex of the smallest (row,
// col) (of the smallest index among equal ones) as its one anchor.  An ARC is the vertex sequence from one anchor to the
// next in ring order, cyclically, both anchors included: it may wrap round the end of the ring's vertex list, and with
// one anchor it is closed (both ends the same vertex).  Both ends of an arc are kept.  For an open interval with kept
// ends a, b and points between them: m(q) = |(b - a) x (q - a)| if a != b, |q - a|^2 if a = b; the CANDIDATE is the
// point of the largest m, ties to the smallest (row, col), then to the first in arc order (only rings built by hand
// repeat a point); it EXCEEDS when m^2 65536 > T |b - a|^2 (a != b), m 65536 > T (a = b), in 128-bit integers, T =
// floor(tolerance^2 65536) from the host.  A candidate that exceeds is kept and both halves are treated the same way;
// otherwise nothing between a and b is kept.  Everything is symmetric in the direction of travel, so the two rings that
// share a border keep the same corners of it.
//
// Steps (workgroups of OL_BLOCK = 256 threads unless said; scan.h as outline.h uses it):
//  1. Anchors and arcs.  k_sp_ringof: every vertex's ring.  k_sp_flagged / k_sp_minkey / k_sp_minidx: which rings have a
//     flagged vertex, and for the others the smallest packed (row, col) and the first vertex that has it (integer
//     atomics).  A scan of the anchor flags numbers the arcs in vertex order, so a ring's arcs are consecutive;
//     k_sp_arc_start / k_sp_arc_make give every arc its start vertex, its point count and its size class.
//  2. Douglas-Peucker, level-synchronous: in one ROUND every open interval finds its candidate, and splits if that
//     exceeds.  Intervals are independent, so rounds until no interval splits give exactly the recursive result, and
//     the rounds that split number the recursion's depth.  Every point holds the positions of the kept points to its
//     left and right (left = right = own position: kept).  A round is four phases with the interval's slot at its left
//     end: atomic max of m; atomic min of the packed (row, col) among the points of that m; atomic min of the position
//     among those; then every point of the interval tests the winner's m itself and, if it exceeds, takes the winner
//     as its new right or left end.  Three size classes by the arc's point count:
//       short  (<= SP_SHORT_MAX = 64):   k_sp_local<64, 1>, a workgroup of one wavefront per arc, points and slots in
//                                        LDS (36 bytes a point), the round loop inside the kernel;
//       group  (<= SP_GROUP_MAX = 1024): k_sp_local<256, 4>, a workgroup per arc, the same code, 36 KiB of LDS;
//       global (longer):                 the points of all such arcs side by side in global arrays (40 bytes a point),
//                                        a thread per point, the four phases as four launches per round from the host,
//                                        which reads a "split happened" word as outline.h's doubling rounds do.
//     The rounds of an arc are bounded by its points; beyond the longest arc's points the call fails with
//     SHP_ERR_STATE and never loops.  No kernel waits for another workgroup.  The path selector (the `path` of
//     simplifySegmentOutlines) forces one class for all arcs that fit it: 1 short arcs short and the others as auto, 2 everything up to
//     SP_GROUP_MAX points in the group class, 3 everything global.
//  3. Areas and the drop rule.  A scan of the kept flags numbers the kept vertices; k_sp_area adds every kept vertex's
//     term c_i r_(i+1) - c_(i+1) r_i over the kept vertices of its ring (k_ol_area's pattern); k_sp_alive drops a ring
//     with fewer than three kept vertices, or whose new area is 0 or differs in sign from its source ring's.
//  4. Emission.  Scans of the surviving rings and of their kept counts give the new ring numbers and vertex offsets;
//     k_sp_emit_v / _r / _id write vertices, kept source indices, areas, source ring numbers and the offsets per ring
//     and per id, all as int64.  All global stores are ordinary vector stores from plain C++.
//
// Device memory, bounds from the counts the host has (run_simplify_need): 13 bytes a vertex (ring number 4, arc then
// kept number 4, kept list 4, kept flag 1), 24 bytes an arc at the bound arcs <= vertices, 40 bytes a point of the global
// class at the bound points <= vertices + arcs, 40 bytes a ring; the result 24 bytes a vertex, 24 a ring, 8 an id; when
// the rings are uploaded 17 a vertex, 16 a ring and 8 an id more.
#pragma once
#include "common.h"
#include "scan.h"
#include "outline.h"
#include "rings.h"

#define SP_SHORT_MAX 64u            // points of an arc up to which one wavefront takes it
#define SP_GROUP_MAX 1024u          // points of an arc up to which one workgroup takes it in LDS
#define SP_MAX_VERTS 0x7FFFE000u    // vertices one call can take: points of the global class <= 2 vertices, in 32 bits
// device words of sp_ctr
enum { SPC_ARCS = 0, SPC_NSHORT, SPC_NGROUP, SPC_NPTS, SPC_LONGEST, SPC_ROUNDS, SPC_KEPT, SPC_RINGS, SPC_VERTS, SPC_FLAG, SPC_WORDS = 16 };

struct SpSrc : RingView {           // (with the flags)
    long long r0, c0;
};

__device__ __forceinline__ unsigned long long sp_key(const SpSrc &s, uint32_t v)
{
    const longlong2 p = s.vtx[v];
    return ((unsigned long long)(p.x - s.r0) << 32) | (unsigned long long)(uint32_t)(p.y - s.c0);
}

// m(q) for the kept ends a, b (coordinates relative to (r0, c0), below 2^31)
__device__ __forceinline__ unsigned long long sp_measure(uint32_t ar, uint32_t ac, uint32_t br, uint32_t bc, uint32_t qr, uint32_t qc)
{
    const long long dr = (long long)qr - (long long)ar, dc = (long long)qc - (long long)ac;
    if (ar == br && ac == bc) return (unsigned long long)(dr * dr + dc * dc);
    const long long x = ((long long)br - (long long)ar) * dc - ((long long)bc - (long long)ac) * dr;
    return (unsigned long long)(x < 0 ? -x : x);
}

__device__ __forceinline__ bool sp_exceeds(unsigned long long m, uint32_t ar, uint32_t ac, uint32_t br, uint32_t bc, unsigned long long T)
{
    if (ar == br && ac == bc) return ((unsigned __int128)m << 16) > (unsigned __int128)T;
    const long long er = (long long)br - (long long)ar, ec = (long long)bc - (long long)ac;
    const unsigned long long len2 = (unsigned long long)(er * er + ec * ec);
    return (((unsigned __int128)m * (unsigned __int128)m) << 16) > (unsigned __int128)T * (unsigned __int128)len2;
}

__global__ __launch_bounds__(256) void k_sp_ringof(SpSrc s, uint32_t *__restrict__ vring)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i < s.nv) vring[i] = ring_last_le(s.voff, s.nr, (long long)i);
}

__global__ __launch_bounds__(256) void k_sp_flagged(SpSrc s, const uint32_t *__restrict__ vring, uint32_t *__restrict__ hasj)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i < s.nv && s.jflag[i] != 0u && L2LOAD(&hasj[vring[i]]) == 0u) atomicOr(&hasj[vring[i]], 1u);
}

__global__ __launch_bounds__(256) void k_sp_minkey(SpSrc s, const uint32_t *__restrict__ vring, const uint32_t *__restrict__ hasj,
                                                   unsigned long long *__restrict__ minkey)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= s.nv) return;
    const uint32_t k = vring[i];
    if (hasj[k] != 0u) return;
    const unsigned long long key = sp_key(s, (uint32_t)i);
    if (key < L2LOAD(&minkey[k])) atomicMin(&minkey[k], key);
}

__global__ __launch_bounds__(256) void k_sp_minidx(SpSrc s, const uint32_t *__restrict__ vring, const uint32_t *__restrict__ hasj,
                                                   const unsigned long long *__restrict__ minkey, uint32_t *__restrict__ minidx)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= s.nv) return;
    const uint32_t k = vring[i];
    if (hasj[k] == 0u && sp_key(s, (uint32_t)i) == minkey[k]) atomicMin(&minidx[k], (uint32_t)i);
}

struct SpAnchorFn {         // vertex v is an anchor
    const uint8_t *jflag;
    const uint32_t *vring, *hasj, *minidx;
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const
    {
        if (jflag[v] != 0u) return 1u;
        const uint32_t k = vring[v];
        return (hasj[k] == 0u && minidx[k] == v) ? 1u : 0u;
    }
};

struct SpByteFn {           // a flag byte per item
    const uint8_t *a;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const { return a[i] != 0u ? 1u : 0u; }
};

__global__ __launch_bounds__(256) void k_sp_arc_start(SpAnchorFn f, const uint32_t *__restrict__ apos, uint32_t nv, uint32_t narcs,
                                                      uint32_t *__restrict__ avtx, uint8_t *__restrict__ keep)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= nv) return;
    const uint32_t on = f((uint32_t)i);
    keep[i] = (uint8_t)on;
    if (on && apos[i] < narcs) avtx[apos[i]] = (uint32_t)i;
}

// the place of every lane with `on` in a list that grows by *ctr: one atomic add per wavefront (a word takes about 88
// atomics a microsecond, and there are millions of arcs)
__device__ __forceinline__ uint32_t sp_wave_append(uint32_t *ctr, bool on)
{
    const unsigned long long m = __ballot(on);
    if (m == 0ull) return 0u;
    const int lead = __builtin_ctzll(m);
    uint32_t base = 0u;
    if ((int)lane_id() == lead) base = atomicAdd(ctr, (uint32_t)__popcll(m));
    base = (uint32_t)__shfl((int)base, lead, 64);
    return base + (uint32_t)__popcll(m & lanemask_lt());
}

// arc a: its point count and class; the short and the group arcs go to their lists, the others count their points
__global__ __launch_bounds__(256) void k_sp_arc_make(SpSrc s, const uint32_t *__restrict__ vring, const uint32_t *__restrict__ apos,
                                                     const uint32_t *__restrict__ avtx, uint32_t narcs, int path,
                                                     uint32_t *__restrict__ acnt, uint32_t *__restrict__ gcnt, uint32_t *__restrict__ slist,
                                                     uint32_t *__restrict__ glist, uint32_t *__restrict__ ctr)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    const bool on = i < narcs;
    const uint32_t a = (uint32_t)i;
    uint32_t cnt = 0u;
    int cls = -1;                                       // 0 short, 1 group, 2 global
    if (on) {
        const uint32_t v = avtx[a], k = vring[v];
        const uint32_t b = (uint32_t)s.voff[k], e = (uint32_t)s.voff[k + 1u], len = e - b;
        const uint32_t a0 = apos[b], a1 = e < s.nv ? apos[e] : narcs;
        const uint32_t nxt = a + 1u < a1 ? avtx[a + 1u] : avtx[a0];
        const uint32_t steps = nxt > v ? nxt - v : nxt + len - v;
        cnt = steps + 1u;
        acnt[a] = cnt;
        if (path == 3) cls = 2;
        else if (path == 2) cls = cnt <= SP_GROUP_MAX ? 1 : 2;
        else cls = cnt <= SP_SHORT_MAX ? 0 : (cnt <= SP_GROUP_MAX ? 1 : 2);
        gcnt[a] = cls == 2 ? cnt : 0u;
    }
    const uint32_t at0 = sp_wave_append(&ctr[SPC_NSHORT], cls == 0), at1 = sp_wave_append(&ctr[SPC_NGROUP], cls == 1);
    if (cls == 0 && at0 < narcs) slist[at0] = a;
    if (cls == 1 && at1 < narcs) glist[at1] = a;
    uint32_t longest = cnt;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) longest = max(longest, (uint32_t)__shfl_xor((int)longest, d, 64));
    if (lane_id() == 0u && longest > L2LOAD(&ctr[SPC_LONGEST])) atomicMax(&ctr[SPC_LONGEST], longest);
}

// the short and the group class: a workgroup per arc of the list, BLOCK * ITEMS points at most, all in LDS
template <uint32_t BLOCK, uint32_t ITEMS>
__global__ __launch_bounds__(BLOCK) void k_sp_local(SpSrc s, const uint32_t *__restrict__ list, uint32_t nlist,
                                                    const uint32_t *__restrict__ avtx, const uint32_t *__restrict__ acnt,
                                                    const uint32_t *__restrict__ vring, unsigned long long T,
                                                    uint8_t *__restrict__ keep, uint32_t *__restrict__ ctr)
{
    constexpr uint32_t CAP = BLOCK * ITEMS;
    __shared__ unsigned long long s_bm[CAP], s_brc[CAP];
    __shared__ uint32_t s_r[CAP], s_c[CAP], s_left[CAP], s_right[CAP], s_bidx[CAP];
    if (blockIdx.x >= nlist) return;
    const uint32_t a = list[blockIdx.x], v0 = avtx[a], cnt = acnt[a];
    if (cnt > CAP || cnt < 2u) return;                  // (cannot happen: the list holds the arcs of this class)
    const uint32_t k = vring[v0], b = (uint32_t)s.voff[k], len = (uint32_t)s.voff[k + 1u] - b;
#pragma unroll
    for (uint32_t it = 0; it < ITEMS; it++) {
        const uint32_t i = threadIdx.x + it * BLOCK;
        if (i < cnt) {
            const uint32_t j = (uint32_t)(((unsigned long long)(v0 - b) + i) % len);
            const longlong2 p = s.vtx[b + j];
            const bool end = i == 0u || i + 1u == cnt;
            s_r[i] = (uint32_t)(p.x - s.r0);
            s_c[i] = (uint32_t)(p.y - s.c0);
            s_left[i] = end ? i : 0u;
            s_right[i] = end ? i : cnt - 1u;
        }
    }
    __syncthreads();
    uint32_t rounds = 0u;
    for (uint32_t round = 0u; round < cnt; round++) {
#pragma unroll
        for (uint32_t it = 0; it < ITEMS; it++) {
            const uint32_t i = threadIdx.x + it * BLOCK;
            if (i < cnt) { s_bm[i] = 0ull; s_brc[i] = ~0ull; s_bidx[i] = OL_NONE; }
        }
        __syncthreads();
        unsigned long long m[ITEMS], rc[ITEMS];
        bool open[ITEMS];
#pragma unroll
        for (uint32_t it = 0; it < ITEMS; it++) {
            const uint32_t i = threadIdx.x + it * BLOCK;
            open[it] = i < cnt && s_left[i] != i;
            m[it] = rc[it] = 0ull;
            if (open[it]) {
                const uint32_t L = s_left[i], R = s_right[i];
                m[it] = sp_measure(s_r[L], s_c[L], s_r[R], s_c[R], s_r[i], s_c[i]);
                rc[it] = ((unsigned long long)s_r[i] << 32) | (unsigned long long)s_c[i];
                atomicMax(&s_bm[L], m[it]);
            }
        }
        __syncthreads();
#pragma unroll
        for (uint32_t it = 0; it < ITEMS; it++) {
            const uint32_t i = threadIdx.x + it * BLOCK;
            if (open[it] && m[it] == s_bm[s_left[i]]) atomicMin(&s_brc[s_left[i]], rc[it]);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t it = 0; it < ITEMS; it++) {
            const uint32_t i = threadIdx.x + it * BLOCK;
            if (open[it] && m[it] == s_bm[s_left[i]] && rc[it] == s_brc[s_left[i]]) atomicMin(&s_bidx[s_left[i]], i);
        }
        __syncthreads();
        int any = 0;
#pragma unroll
        for (uint32_t it = 0; it < ITEMS; it++) {
            const uint32_t i = threadIdx.x + it * BLOCK;
            if (!open[it]) continue;
            const uint32_t L = s_left[i], R = s_right[i], w = s_bidx[L];
            if (w < cnt && sp_exceeds(s_bm[L], s_r[L], s_c[L], s_r[R], s_c[R], T)) {
                any = 1;                                // (only a point writes its own ends: nobody reads them in this phase)
                if (i < w) s_right[i] = w;
                else if (i > w) s_left[i] = w;
                else s_left[i] = s_right[i] = i;
            }
        }
        if (!__syncthreads_or(any)) break;
        rounds++;
    }
#pragma unroll
    for (uint32_t it = 0; it < ITEMS; it++) {
        const uint32_t i = threadIdx.x + it * BLOCK;
        if (i > 0u && i + 1u < cnt && s_left[i] == i) keep[b + (uint32_t)(((unsigned long long)(v0 - b) + i) % len)] = (uint8_t)1;
    }
    if (threadIdx.x == 0u && rounds > L2LOAD(&ctr[SPC_ROUNDS])) atomicMax(&ctr[SPC_ROUNDS], rounds);
}

// ---- the global class: the points of its arcs side by side ------------------------------------------------------
struct SpPts {
    uint32_t *r, *c, *left, *right, *bidx, *vtx;
    unsigned long long *bm, *brc;
    uint32_t n;
};

__global__ __launch_bounds__(256) void k_sp_g_fill(SpSrc s, SpPts g, const uint32_t *__restrict__ gpoff, const uint32_t *__restrict__ avtx,
                                                   const uint32_t *__restrict__ acnt, const uint32_t *__restrict__ vring, uint32_t narcs)
{
    const size_t t = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (t >= g.n) return;
    const uint32_t p = (uint32_t)t;
    uint32_t lo = 0u, hi = narcs;                       // the last arc whose points begin at or before p
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (gpoff[mid] <= p) lo = mid; else hi = mid;
    }
    const uint32_t a = lo, p0 = gpoff[a], cnt = acnt[a], i = p - p0;
    if (i >= cnt) return;                               // (cannot happen: arcs of other classes have no points here)
    const uint32_t v0 = avtx[a], k = vring[v0], b = (uint32_t)s.voff[k], len = (uint32_t)s.voff[k + 1u] - b;
    const uint32_t v = b + (uint32_t)(((unsigned long long)(v0 - b) + i) % len);
    const longlong2 q = s.vtx[v];
    const bool end = i == 0u || i + 1u == cnt;
    g.r[p] = (uint32_t)(q.x - s.r0);
    g.c[p] = (uint32_t)(q.y - s.c0);
    g.vtx[p] = v;
    g.left[p] = end ? p : p0;
    g.right[p] = end ? p : p0 + cnt - 1u;
}

// phase 0: the largest m of every interval; 1: the smallest (row, col) among its points of that m; 2: the first of those
template <int PHASE>
__global__ __launch_bounds__(256) void k_sp_g_phase(SpPts g)
{
    const size_t t = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (t >= g.n) return;
    const uint32_t p = (uint32_t)t, L = g.left[p];
    if (L == p) return;
    const uint32_t R = g.right[p];
    const unsigned long long m = sp_measure(g.r[L], g.c[L], g.r[R], g.c[R], g.r[p], g.c[p]);
    if (PHASE == 0) { atomicMax(&g.bm[L], m); return; }
    if (m != g.bm[L]) return;
    const unsigned long long rc = ((unsigned long long)g.r[p] << 32) | (unsigned long long)g.c[p];
    if (PHASE == 1) { atomicMin(&g.brc[L], rc); return; }
    if (rc == g.brc[L]) atomicMin(&g.bidx[L], p);
}

// phase 3: the intervals whose candidate exceeds split; a point writes its own ends only, and reads those of no other
__global__ __launch_bounds__(256) void k_sp_g_split(SpPts g, unsigned long long T, uint32_t *__restrict__ flag)
{
    const size_t t = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    bool split = false;
    if (t < g.n) {
        const uint32_t p = (uint32_t)t, L = g.left[p];
        if (L != p) {
            const uint32_t R = g.right[p], w = g.bidx[L];
            if (w < g.n && sp_exceeds(g.bm[L], g.r[L], g.c[L], g.r[R], g.c[R], T)) {
                split = true;
                if (p < w) g.right[p] = w;
                else if (p > w) g.left[p] = w;
                else g.left[p] = g.right[p] = p;
            }
        }
    }
    if (__ballot(split) != 0ull && lane_id() == 0u && L2LOAD(flag) == 0u) atomicOr(flag, 1u);
}

__global__ __launch_bounds__(256) void k_sp_g_keep(SpPts g, uint8_t *__restrict__ keep, uint32_t nv)
{
    const size_t t = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (t >= g.n) return;
    const uint32_t p = (uint32_t)t, v = g.vtx[p];
    if (g.left[p] == p && v < nv) keep[v] = (uint8_t)1;
}

// ---- kept vertices, areas, the drop rule, emission ---------------------------------------------------------------
__global__ __launch_bounds__(256) void k_sp_kv(const uint8_t *__restrict__ keep, const uint32_t *__restrict__ kpos, uint32_t nv, uint32_t nk,
                                               uint32_t *__restrict__ kv)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i < nv && keep[i] != 0u && kpos[i] < nk) kv[kpos[i]] = (uint32_t)i;
}

// the kept vertices of ring k are kv[ks .. ke)
__device__ __forceinline__ void sp_kept_range(const SpSrc &s, const uint32_t *__restrict__ kpos, uint32_t nk, uint32_t k, uint32_t *ks, uint32_t *ke)
{
    const uint32_t b = (uint32_t)s.voff[k], e = (uint32_t)s.voff[k + 1u];
    *ks = b < s.nv ? kpos[b] : nk;
    *ke = e < s.nv ? kpos[e] : nk;
}

__global__ __launch_bounds__(256) void k_sp_area(SpSrc s, const uint32_t *__restrict__ vring, const uint32_t *__restrict__ kpos,
                                                 const uint32_t *__restrict__ kv, uint32_t nk, unsigned long long *__restrict__ narea)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    uint32_t key = OL_NONE;
    unsigned long long term = 0ull;
    if (i < nk) {
        const uint32_t j = (uint32_t)i, v = kv[j], k = vring[v];
        uint32_t ks, ke;
        sp_kept_range(s, kpos, nk, k, &ks, &ke);
        const uint32_t nx = j + 1u < ke ? j + 1u : ks;
        const longlong2 a = s.vtx[v], b = s.vtx[kv[nx]];
        const long long ra = a.x - s.r0, ca = a.y - s.c0, rb = b.x - s.r0, cb = b.y - s.c0;
        term = (unsigned long long)(ca * rb - cb * ra);
        key = k;
    }
    ol_wave_add<unsigned long long>(narea, key, term);
}

__global__ __launch_bounds__(256) void k_sp_alive(SpSrc s, const uint32_t *__restrict__ kpos, uint32_t nk,
                                                  const unsigned long long *__restrict__ narea, uint32_t *__restrict__ alive,
                                                  uint32_t *__restrict__ kcnt)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= s.nr) return;
    const uint32_t k = (uint32_t)i;
    uint32_t ks, ke;
    sp_kept_range(s, kpos, nk, k, &ks, &ke);
    const long long now = (long long)narea[k], was = s.area2[k];
    const bool on = ke - ks >= 3u && now != 0 && (now > 0) == (was > 0) && was != 0;
    alive[k] = on ? 1u : 0u;
    kcnt[k] = on ? ke - ks : 0u;
}

__global__ __launch_bounds__(256) void k_sp_emit_v(SpSrc s, const uint32_t *__restrict__ vring, const uint32_t *__restrict__ kpos,
                                                   const uint32_t *__restrict__ kv, uint32_t nk, const uint32_t *__restrict__ alive,
                                                   const uint32_t *__restrict__ vo2, uint32_t nv2, longlong2 *__restrict__ verts,
                                                   long long *__restrict__ kept_vertex)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= nk) return;
    const uint32_t j = (uint32_t)i, v = kv[j], k = vring[v];
    if (!alive[k]) return;
    uint32_t ks, ke;
    sp_kept_range(s, kpos, nk, k, &ks, &ke);
    const uint32_t at = vo2[k] + (j - ks);
    if (at >= nv2) return;                              // (cannot happen: vo2 counts the same vertices)
    verts[at] = s.vtx[v];
    kept_vertex[at] = (long long)v;
}

__global__ __launch_bounds__(256) void k_sp_emit_r(uint32_t nr, const uint32_t *__restrict__ alive, const uint32_t *__restrict__ rpos,
                                                   const uint32_t *__restrict__ vo2, const unsigned long long *__restrict__ narea,
                                                   uint32_t nr2, uint32_t nv2, long long *__restrict__ voff_out,
                                                   long long *__restrict__ area_out, long long *__restrict__ source_ring)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i > nr) return;
    if (i == nr) { voff_out[nr2] = (long long)nv2; return; }
    if (!alive[i]) return;
    const uint32_t at = rpos[i];
    if (at >= nr2) return;                              // (cannot happen)
    voff_out[at] = (long long)vo2[i];
    area_out[at] = (long long)narea[i];
    source_ring[at] = (long long)i;
}

__global__ __launch_bounds__(256) void k_sp_emit_id(SpSrc s, const uint32_t *__restrict__ rpos, uint32_t nr2, long long *__restrict__ roff_out)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= (size_t)s.S + 2) return;
    const long long k = s.roff[i];
    roff_out[i] = k >= 0 && k < (long long)s.nr ? (long long)rpos[k] : (k < 0 ? 0ll : (long long)nr2);
}

// ---- host side --------------------------------------------------------------------------------------------
// the buffers uploaded rings and flags go into
static inline RingBufs sp_ring_bufs(shp_ctx *ctx) { return RingBufs{ctx->sp_vtx, ctx->sp_voff, ctx->sp_roff, ctx->sp_area, &ctx->sp_jflag}; }

// bytes of a ring's rows in sp_ring: minkey, narea (8 each), hasj, minidx, alive, kcnt, rpos, vo2 (4 each)
#define SP_RING_BYTES 40u
#define SP_ARC_BYTES 24u            // avtx, acnt, gcnt, gpoff, slist, glist
#define SP_PT_BYTES 40u

static inline size_t sp_out_bytes(size_t nv2, size_t nr2, size_t S)
{
    return nv2 * 16 + nv2 * 8 + (nr2 + 1) * 8 + nr2 * 16 + (S + 2) * 8 + 64;
}

// the device memory the buffers still have to grow by for nv vertices in nr rings of the ids 0 .. S, at the bounds arcs
// <= nv, points of the global class <= 2 nv, kept vertices <= nv; upload: the rings go into buffers of this file's own
static int run_simplify_need(shp_ctx *ctx, size_t nv, size_t nr, size_t S, int upload, long long *need_out, long long *free_out)
{
    size_t need = upload ? ring_upload_need(sp_ring_bufs(ctx), nv, nr, S) : 0;
    need += ol_grown(ctx->sp_ctr, SPC_WORDS * 4) + ol_grown(ctx->sp_keep, nv) + ol_grown(ctx->sp_pos, (nv + 4) * 8);
    need += ol_grown(ctx->sp_ring, (nr + 4) * SP_RING_BYTES) + ol_grown(ctx->sp_arc, (nv + 4) * SP_ARC_BYTES);
    need += ol_grown(ctx->sp_pt, (2 * nv + 4) * SP_PT_BYTES) + ol_grown(ctx->sp_kv, nv * 4);
    need += ol_grown(ctx->sp_out, sp_out_bytes(nv, nr, S));
    need += ol_grown(ctx->scan_tmp, scan_tmp_bytes(nv > nr ? nv : nr));
    size_t fr = 0, tot = 0;
    HIPCHK(ctx, hipMemGetInfo(&fr, &tot));
    *need_out = (long long)need;
    *free_out = (long long)fr;
    return 0;
}

// the rings to simplify: the context's traced outlines in place (all arrays NULL), or host arrays uploaded
static int run_simplify_source(shp_ctx *ctx, const int64_t *ring_offsets, const int64_t *vertex_offsets, const int64_t *vertices,
                               const int64_t *ring_area2, const uint8_t *junction, uint32_t S, uint32_t nr, uint32_t nv,
                               double *upload_ms_out)
{
    SimplifyState &z = ctx->simplify;
    z = SimplifyState{};
    CHK(ring_source_take(ctx, z.src, sp_ring_bufs(ctx), ring_offsets, vertex_offsets, vertices, ring_area2, junction, S, nr, nv, upload_ms_out));
    z.stage = 1;
    return 0;
}

static int run_simplify_build(shp_ctx *ctx, unsigned long long T, int path, long long r0, long long c0)
{
    SimplifyState &z = ctx->simplify;
    hipStream_t st = ctx->stream;
    z.stage = 0;
    z.narcs = z.longest = z.rounds = z.nshort = z.ngroup = z.nglobal = z.kept = z.rings = z.verts = 0u;
    for (int i = 0; i < 4; i++) z.ms[i] = 0.0;
    const uint32_t nv = z.src.nv, nr = z.src.nr, S = z.src.S;
    const SpSrc src{ring_view(ctx, z.src, sp_ring_bufs(ctx)), r0, c0};
    CHK(buf_ensure(ctx, ctx->sp_ctr, SPC_WORDS * 4));
    uint32_t *ctr = bp<uint32_t>(ctx->sp_ctr);
    volatile uint32_t *hp = (volatile uint32_t *)ctx->h_pinned;
    HIPCHK(ctx, hipMemsetAsync(ctr, 0, SPC_WORDS * 4, st));
    // sp_out: vertices (16-byte aligned), kept vertices, vertex offsets, areas, source rings, ring offsets
    auto lay_out = [&](size_t nv2, size_t nr2) {
        z.off[2] = 0;
        z.off[5] = nv2 * 16;
        z.off[1] = z.off[5] + nv2 * 8;
        z.off[3] = z.off[1] + (nr2 + 1) * 8;
        z.off[4] = z.off[3] + nr2 * 8;
        z.off[0] = z.off[4] + nr2 * 8;
    };
    if (nv == 0u || nr == 0u) {                         // nothing to keep: no rings
        lay_out(0, 0);
        CHK(buf_ensure(ctx, ctx->sp_out, sp_out_bytes(0, 0, S)));
        HIPCHK(ctx, hipMemsetAsync(ctx->sp_out.p, 0, sp_out_bytes(0, 0, S), st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        z.stage = 2;
        return 0;
    }
    // ---- step 1: anchors and arcs
    const size_t qv = ((size_t)nv + 4) & ~(size_t)3, qr = ((size_t)nr + 4) & ~(size_t)3;
    CHK(buf_ensure(ctx, ctx->sp_pos, qv * 8));
    CHK(buf_ensure(ctx, ctx->sp_keep, nv));
    CHK(buf_ensure(ctx, ctx->sp_ring, qr * SP_RING_BYTES));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(nv > nr ? nv : nr)));
    uint32_t *apos = bp<uint32_t>(ctx->sp_pos), *vring = apos + qv;
    uint8_t *keep = bp<uint8_t>(ctx->sp_keep);
    unsigned long long *minkey = bp<unsigned long long>(ctx->sp_ring), *narea = minkey + qr;
    uint32_t *hasj = (uint32_t *)(narea + qr), *minidx = hasj + qr, *alive = minidx + qr, *kcnt = alive + qr, *rpos = kcnt + qr,
             *vo2 = rpos + qr;
    uint32_t *tmp = bp<uint32_t>(ctx->scan_tmp);
    const unsigned vgrid = grid_for(nv, OL_BLOCK), rgrid = grid_for(nr, OL_BLOCK);
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    HIPCHK(ctx, hipMemsetAsync(minkey, 0xff, qr * 8, st));
    HIPCHK(ctx, hipMemsetAsync(narea, 0, qr * 8, st));
    HIPCHK(ctx, hipMemsetAsync(hasj, 0, qr * 4, st));
    HIPCHK(ctx, hipMemsetAsync(minidx, 0xff, qr * 4, st));
    hipLaunchKernelGGL(k_sp_ringof, dim3(vgrid), dim3(OL_BLOCK), 0, st, src, vring);
    KCHK(ctx);
    hipLaunchKernelGGL(k_sp_flagged, dim3(vgrid), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)vring, hasj);
    KCHK(ctx);
    hipLaunchKernelGGL(k_sp_minkey, dim3(vgrid), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)vring, (const uint32_t *)hasj, minkey);
    KCHK(ctx);
    hipLaunchKernelGGL(k_sp_minidx, dim3(vgrid), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)vring, (const uint32_t *)hasj,
                       (const unsigned long long *)minkey, minidx);
    KCHK(ctx);
    SpAnchorFn af{src.jflag, vring, hasj, minidx};
    CHK(scan_exclusive(ctx, af, nv, apos, ctr + SPC_ARCS, tmp));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr + SPC_ARCS, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t narcs = hp[0];
    if (narcs == 0u || narcs > nv) SHP_FAIL(ctx, SHP_ERR_STATE, "simplify: %u arcs over %u vertices", narcs, nv);
    const size_t qa = ((size_t)narcs + 4) & ~(size_t)3;
    CHK(buf_ensure(ctx, ctx->sp_arc, qa * SP_ARC_BYTES));
    uint32_t *avtx = bp<uint32_t>(ctx->sp_arc), *acnt = avtx + qa, *gcnt = acnt + qa, *gpoff = gcnt + qa, *slist = gpoff + qa,
             *glist = slist + qa;
    const unsigned agrid = grid_for(narcs, OL_BLOCK);
    hipLaunchKernelGGL(k_sp_arc_start, dim3(vgrid), dim3(OL_BLOCK), 0, st, af, (const uint32_t *)apos, nv, narcs, avtx, keep);
    KCHK(ctx);
    hipLaunchKernelGGL(k_sp_arc_make, dim3(agrid), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)vring, (const uint32_t *)apos,
                       (const uint32_t *)avtx, narcs, path, acnt, gcnt, slist, glist, ctr);
    KCHK(ctx);
    ArrFn gf{gcnt};
    CHK(scan_exclusive(ctx, gf, narcs, gpoff, ctr + SPC_NPTS, tmp));
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr, SPC_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nshort = hp[SPC_NSHORT], ngroup = hp[SPC_NGROUP], npts = hp[SPC_NPTS], longest = hp[SPC_LONGEST];
    if ((size_t)nshort + ngroup > narcs || (unsigned long long)npts > 2ull * nv || longest < 2u || longest > nv + 1u)
        SHP_FAIL(ctx, SHP_ERR_STATE, "simplify: %u short and %u group arcs of %u, %u points, the longest arc %u", nshort, ngroup, narcs,
                 npts, longest);
    z.narcs = narcs; z.longest = longest; z.nshort = nshort; z.ngroup = ngroup;
    // ---- step 2: the rounds, class by class
    if (nshort) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sp_local<64u, 1u>), dim3(nshort), dim3(64), 0, st, src, (const uint32_t *)slist, nshort,
                           (const uint32_t *)avtx, (const uint32_t *)acnt, (const uint32_t *)vring, T, keep, ctr);
        KCHK(ctx);
    }
    if (ngroup) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_sp_local<256u, 4u>), dim3(ngroup), dim3(256), 0, st, src, (const uint32_t *)glist, ngroup,
                           (const uint32_t *)avtx, (const uint32_t *)acnt, (const uint32_t *)vring, T, keep, ctr);
        KCHK(ctx);
    }
    uint32_t grounds = 0u;
    if (npts) {
        const size_t qp = ((size_t)npts + 4) & ~(size_t)3;
        CHK(buf_ensure(ctx, ctx->sp_pt, qp * SP_PT_BYTES));
        SpPts g;
        g.bm = bp<unsigned long long>(ctx->sp_pt); g.brc = g.bm + qp;
        g.r = (uint32_t *)(g.brc + qp); g.c = g.r + qp; g.left = g.c + qp; g.right = g.left + qp; g.bidx = g.right + qp; g.vtx = g.bidx + qp;
        g.n = npts;
        const unsigned pgrid = grid_for(npts, OL_BLOCK);
        hipLaunchKernelGGL(k_sp_g_fill, dim3(pgrid), dim3(OL_BLOCK), 0, st, src, g, (const uint32_t *)gpoff, (const uint32_t *)avtx,
                           (const uint32_t *)acnt, (const uint32_t *)vring, narcs);
        KCHK(ctx);
        bool settled = false;
        for (uint32_t r = 0; r <= longest && !settled; r++) {
            HIPCHK(ctx, hipMemsetAsync(g.bm, 0, qp * 8, st));
            HIPCHK(ctx, hipMemsetAsync(g.brc, 0xff, qp * 8, st));
            HIPCHK(ctx, hipMemsetAsync(g.bidx, 0xff, qp * 4, st));
            HIPCHK(ctx, hipMemsetAsync(ctr + SPC_FLAG, 0, 4, st));
            hipLaunchKernelGGL(k_sp_g_phase<0>, dim3(pgrid), dim3(OL_BLOCK), 0, st, g);
            KCHK(ctx);
            hipLaunchKernelGGL(k_sp_g_phase<1>, dim3(pgrid), dim3(OL_BLOCK), 0, st, g);
            KCHK(ctx);
            hipLaunchKernelGGL(k_sp_g_phase<2>, dim3(pgrid), dim3(OL_BLOCK), 0, st, g);
            KCHK(ctx);
            hipLaunchKernelGGL(k_sp_g_split, dim3(pgrid), dim3(OL_BLOCK), 0, st, g, T, ctr + SPC_FLAG);
            KCHK(ctx);
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr + SPC_FLAG, 4, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipStreamSynchronize(st));
            settled = hp[0] == 0u;
            if (!settled) grounds++;
        }
        if (!settled) SHP_FAIL(ctx, SHP_ERR_STATE, "simplify: intervals still split after %u rounds, the longest arc has %u points", grounds, longest);
        hipLaunchKernelGGL(k_sp_g_keep, dim3(pgrid), dim3(OL_BLOCK), 0, st, g, keep, nv);
        KCHK(ctx);
        z.nglobal = narcs - nshort - ngroup;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    // ---- step 3: the kept vertices, the areas over them, the drop rule
    uint32_t *kpos = apos;                              // (the arcs are done with their numbers)
    SpByteFn kf{keep};
    CHK(scan_exclusive(ctx, kf, nv, kpos, ctr + SPC_KEPT, tmp));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr, SPC_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nk = hp[SPC_KEPT], lrounds = hp[SPC_ROUNDS];
    if (nk < narcs || nk > nv) SHP_FAIL(ctx, SHP_ERR_STATE, "simplify: %u vertices kept of %u, %u anchors", nk, nv, narcs);
    z.rounds = lrounds > grounds ? lrounds : grounds;
    z.kept = nk;
    CHK(buf_ensure(ctx, ctx->sp_kv, (size_t)nk * 4));
    uint32_t *kv = bp<uint32_t>(ctx->sp_kv);
    const unsigned kgrid = grid_for(nk, OL_BLOCK);
    hipLaunchKernelGGL(k_sp_kv, dim3(vgrid), dim3(OL_BLOCK), 0, st, (const uint8_t *)keep, (const uint32_t *)kpos, nv, nk, kv);
    KCHK(ctx);
    hipLaunchKernelGGL(k_sp_area, dim3(kgrid), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)vring, (const uint32_t *)kpos,
                       (const uint32_t *)kv, nk, narea);
    KCHK(ctx);
    hipLaunchKernelGGL(k_sp_alive, dim3(rgrid), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)kpos, nk, (const unsigned long long *)narea,
                       alive, kcnt);
    KCHK(ctx);
    ArrFn lf{alive}, cf{kcnt};
    CHK(scan_exclusive(ctx, lf, nr, rpos, ctr + SPC_RINGS, tmp));
    CHK(scan_exclusive(ctx, cf, nr, vo2, ctr + SPC_VERTS, tmp));
    HIPCHK(ctx, hipEventRecord(ctx->ev[3], st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr, SPC_WORDS * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nr2 = hp[SPC_RINGS], nv2 = hp[SPC_VERTS];
    if (nr2 > nr || nv2 > nk || nv2 < 3ull * nr2) SHP_FAIL(ctx, SHP_ERR_STATE, "simplify: %u vertices in %u rings of %u kept", nv2, nr2, nk);
    // ---- step 4: emission
    lay_out(nv2, nr2);
    CHK(buf_ensure(ctx, ctx->sp_out, sp_out_bytes(nv2, nr2, S)));
    char *out = (char *)ctx->sp_out.p;
    hipLaunchKernelGGL(k_sp_emit_v, dim3(kgrid), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)vring, (const uint32_t *)kpos,
                       (const uint32_t *)kv, nk, (const uint32_t *)alive, (const uint32_t *)vo2, nv2, (longlong2 *)(out + z.off[2]),
                       (long long *)(out + z.off[5]));
    KCHK(ctx);
    hipLaunchKernelGGL(k_sp_emit_r, dim3(grid_for((size_t)nr + 1, OL_BLOCK)), dim3(OL_BLOCK), 0, st, nr, (const uint32_t *)alive,
                       (const uint32_t *)rpos, (const uint32_t *)vo2, (const unsigned long long *)narea, nr2, nv2,
                       (long long *)(out + z.off[1]), (long long *)(out + z.off[3]), (long long *)(out + z.off[4]));
    KCHK(ctx);
    hipLaunchKernelGGL(k_sp_emit_id, dim3(grid_for((size_t)S + 2, OL_BLOCK)), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)rpos, nr2,
                       (long long *)(out + z.off[0]));
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[4], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < 4; i++) z.ms[i] = ol_elapsed(ctx->ev[i], ctx->ev[i + 1]);
    z.rings = nr2;
    z.verts = nv2;
    z.stage = 2;
    return 0;
}

static int run_simplify_download(shp_ctx *ctx, int64_t *ring_offsets, int64_t *vertex_offsets, int64_t *vertices, int64_t *ring_area2,
                                 int64_t *source_ring, int64_t *kept_vertex)
{
    const SimplifyState &z = ctx->simplify;
    hipStream_t st = ctx->stream;
    const char *out = (const char *)ctx->sp_out.p;
    HIPCHK(ctx, hipMemcpyAsync(ring_offsets, out + z.off[0], ((size_t)z.src.S + 2) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(vertex_offsets, out + z.off[1], ((size_t)z.rings + 1) * 8, hipMemcpyDeviceToHost, st));
    if (z.rings) {
        HIPCHK(ctx, hipMemcpyAsync(ring_area2, out + z.off[3], (size_t)z.rings * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(source_ring, out + z.off[4], (size_t)z.rings * 8, hipMemcpyDeviceToHost, st));
    }
    if (z.verts) {
        HIPCHK(ctx, hipMemcpyAsync(vertices, out + z.off[2], (size_t)z.verts * 16, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(kept_vertex, out + z.off[5], (size_t)z.verts * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}
