// hull.h -- the strict convex hull of every segment's outline rings, with the per-edge reach and the squared
// diameter that the Feret diameters come from (outlines.calcSegmentHulls).  Integer work throughout: no launch
// geometry, atomic order or size threshold can change a bit of the result.
//
// Input: the rings as outline.h leaves them (vertices as (row, col) int64 pairs, int64 vertex offsets per ring, int64
// ring offsets per id, ringArea2), either still in the context's outline buffers (read in place) or uploaded into
// buffers of this file's own (hl_vtx, hl_voff, hl_roff, hl_area): rings.h decides and makes the view.  (r0, c0) = the smallest row and column of all vertices; the host has checked that the
// spans H and W satisfy H W <= 2^32 and max(H, W) < 2^31, so coordinates relative to (r0, c0) fit 31 bits, every cross
// product stays within 2^33 and every squared distance fits int64.  With x = col and y = row a positive ringArea2 is a
// counter-clockwise polygon, cross(a, b, c) = (b.x - a.x)(c.y - a.y) - (b.y - a.y)(c.x - a.x) > 0 a left turn.
//
// Steps (workgroups of OL_BLOCK = 256 threads; scan.h and sort.h as outline.h uses them):
//  1. Candidates (k_hl_cand): every vertex; for traced rings (convex_only, set by the resident path and for outlines
//     the trace made) only the left-turn vertices of rings with ringArea2 > 0, since a hull vertex is a convex corner
//     of an outer ring.  Compacted with a scan: id, relative col and row, 4 bytes each.
//  2. Order: three stable sort_pairs (row, then col, then id) with a gather between them put the candidates in (id,
//     col, row) order.  k_hl_compact keeps of each (id, col) run the first and the last point: an id's list is then
//     at most 2 (its column span + 1) points long, whatever its pixel count.  k_hl_idoff finds every id's range.
//  3. Chains (k_hl_chain), a wavefront per id.  An id of at most HL_WAVE_MAX = 64 kept points has a point per lane:
//     adjacent equal points are dropped, then rounds remove at once every live point that is no strict left turn
//     between its live neighbours (such a point lies on or inside a segment between two other points of the set, so
//     it is no hull vertex; the fixed point is the strict chain), the live set a 64-bit ballot, for the lower chain
//     (ascending) and the upper chain (descending).  A longer list is walked by lane 0 with Andrew's stack (upper
//     chain into a stack of its own, lower chain in place), which is linear in the list whatever the pops.  Both
//     write the hull counter-clockwise from the smallest (col, row) into the id's own range, with its length and the
//     place of its smallest (row, col) point.  The only size threshold of this file is HL_WAVE_MAX
//     (tests/test_gpu_hulls.py: test_pop_cascade has ids of 62, 63, 64, 65 and 66 kept points at n = 28, 29, 30).
//  4. Emit: a scan of the lengths gives the offsets; k_hl_emit writes the points rotated to start at the smallest
//     (row, col), (r0, c0) added back.
//  5. Reach and diameter (k_hl_reach), a thread per hull edge a -> b: along the hull the cross product with the edge
//     rises and falls, so the first following edge that does not turn further from the line is found by bisection in
//     O(log h); its start q is the farthest point (reach = cross(a, b, q)), and when that edge is parallel its end
//     counts too.  The squared diameter is the largest |a q|^2, |b q|^2 over the edges (the antipodal pairs); it and
//     the area terms go to the id's int64 with integer atomics, a wavefront's lanes of one id together.
// No kernel waits for another workgroup.
//
// Device memory, bounds from the counts the host has (run_hull_need): 40 bytes a vertex at the bound candidates <=
// vertices (place 4; id, col, row 12; the gather's keys and values 8; the sort's own 16), 24 a vertex for the hull
// points and their reach at the bound hull points <= vertices; 40 bytes an id; when the rings are uploaded 16 a vertex,
// 16 a ring and 8 an id more.  Nothing is sized by a bounding box.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"
#include "outline.h"
#include "rings.h"

#define HL_WAVE_MAX 64u             // kept points of an id up to which its chains are built in registers
#define HL_CTR_WORDS 8u             // device words of hl_ctr: [0] candidates, [1] kept points, [2] hull points

struct HlSrc : RingView {           // (no flags: jflag is NULL)
    long long r0, c0;
    int convex_only;
};

__device__ __forceinline__ long long hl_cross(long long ax, long long ay, long long bx, long long by, long long cx, long long cy)
{
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// vertex v is a candidate; *ring_out its ring
__device__ __forceinline__ bool hl_is_cand(const HlSrc &s, uint32_t v, uint32_t *ring_out)
{
    const uint32_t k = ring_last_le(s.voff, s.nr, (long long)v);
    *ring_out = k;
    if (!s.convex_only) return true;
    if (s.area2[k] <= 0) return false;
    const long long b = s.voff[k], e = s.voff[k + 1u];
    if (b < 0 || e > (long long)s.nv || e - b < 3 || (long long)v >= e) return false;
    const uint32_t pv = (long long)v == b ? (uint32_t)(e - 1) : v - 1u, nx = (long long)v + 1 == e ? (uint32_t)b : v + 1u;
    const longlong2 p = s.vtx[pv], c = s.vtx[v], n = s.vtx[nx];
    return hl_cross(p.y - s.c0, p.x - s.r0, c.y - s.c0, c.x - s.r0, n.y - s.c0, n.x - s.r0) > 0;
}

struct HlCandFn {
    HlSrc s;
    __device__ __forceinline__ uint32_t operator()(uint32_t v) const
    {
        uint32_t k;
        return hl_is_cand(s, v, &k) ? 1u : 0u;
    }
};

__global__ __launch_bounds__(256) void k_hl_cand(HlSrc s, const uint32_t *__restrict__ pos, uint32_t ncand,
                                                 uint32_t *__restrict__ cid, uint32_t *__restrict__ ccol, uint32_t *__restrict__ crow)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= s.nv) return;
    const uint32_t v = (uint32_t)i;
    uint32_t k;
    if (!hl_is_cand(s, v, &k)) return;
    const uint32_t at = pos[v];
    if (at >= ncand) return;                            // (cannot happen: pos counts the same flags)
    const longlong2 p = s.vtx[v];
    cid[at] = ring_last_le(s.roff, s.S + 1u, (long long)k);
    ccol[at] = (uint32_t)(p.y - s.c0);
    crow[at] = (uint32_t)(p.x - s.r0);
}

// keys[j] = src[order[j]], vals[j] = order[j]
__global__ __launch_bounds__(256) void k_hl_gather(const uint32_t *__restrict__ order, const uint32_t *__restrict__ src, uint32_t n,
                                                   uint32_t *__restrict__ keys, uint32_t *__restrict__ vals)
{
    const size_t j = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (j >= n) return;
    const uint32_t o = order[j];
    if (o >= n) return;                                 // (cannot happen: a permutation)
    keys[j] = src[o];
    if (vals) vals[j] = o;
}

struct HlKeepFn {           // place k of the (id, col, row) order is the first or the last of its (id, col) run
    const uint32_t *sid, *scol;
    uint32_t n;
    __device__ __forceinline__ uint32_t operator()(uint32_t k) const
    {
        const uint32_t i = sid[k], c = scol[k];
        const bool first = k == 0u || sid[k - 1u] != i || scol[k - 1u] != c;
        const bool last = k + 1u == n || sid[k + 1u] != i || scol[k + 1u] != c;
        return (first || last) ? 1u : 0u;
    }
};

__global__ __launch_bounds__(256) void k_hl_compact(HlKeepFn f, const uint32_t *__restrict__ srow, const uint32_t *__restrict__ pos,
                                                    uint32_t nkept, uint32_t *__restrict__ pid, uint32_t *__restrict__ pcol,
                                                    uint32_t *__restrict__ prow)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= f.n) return;
    const uint32_t k = (uint32_t)i;
    if (!f(k)) return;
    const uint32_t at = pos[k];
    if (at >= nkept) return;                            // (cannot happen)
    pid[at] = f.sid[k];
    pcol[at] = f.scol[k];
    prow[at] = srow[k];
}

// poff[i] = kept points of the ids below i (i = 0 .. S + 1)
__global__ __launch_bounds__(256) void k_hl_idoff(const uint32_t *__restrict__ pid, uint32_t n, size_t nid, uint32_t *__restrict__ poff)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i >= nid) return;
    uint32_t lo = 0u, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if ((size_t)pid[mid] < i) lo = mid + 1u; else hi = mid;
    }
    poff[i] = lo;
}

// one chain of a list held a point per lane: the live lanes that remain when no live point is left that is not a
// strict left turn between its live neighbours (upper: taken in descending order)
__device__ __forceinline__ unsigned long long hl_wave_chain(unsigned long long live, bool upper, long long x, long long y)
{
    const unsigned lane = lane_id();
    const unsigned long long lt = lanemask_lt(), gt = lane == 63u ? 0ull : ~((2ull << lane) - 1ull);
    const bool mine = (live >> lane) & 1ull;
    for (int round = 0; round < 64; round++) {
        const unsigned long long lo = live & lt, hi = live & gt;
        const bool inner = mine && ((live >> lane) & 1ull) && lo != 0ull && hi != 0ull;
        const int pv = lo ? 63 - __builtin_clzll(lo) : (int)lane, nx = hi ? __builtin_ctzll(hi) : (int)lane;
        const int ia = upper ? nx : pv, ib = upper ? pv : nx;
        const long long ax = __shfl(x, ia, 64), ay = __shfl(y, ia, 64), bx = __shfl(x, ib, 64), by = __shfl(y, ib, 64);
        const bool drop = inner && hl_cross(ax, ay, x, y, bx, by) <= 0;
        const unsigned long long next = live & ~__ballot(drop);
        if (next == live) break;
        live = next;
    }
    return live;
}

// a wavefront per id: the hull of its kept points, counter-clockwise from the smallest (col, row), written over the
// head of the id's own range pcol / prow[poff[i] ..]; hcnt[i] its points, hstart[i] the place of the smallest (row,
// col).  stk_c / stk_r: as long as pcol, the upper chain's stack of the ids walked by one lane.
__global__ __launch_bounds__(256) void k_hl_chain(const uint32_t *__restrict__ poff, uint32_t nid, uint32_t nkept, uint32_t *pcol,
                                                  uint32_t *prow, uint32_t *stk_c, uint32_t *stk_r, uint32_t *__restrict__ hcnt,
                                                  uint32_t *__restrict__ hstart)
{
    const size_t w = ((size_t)blockIdx.x * OL_BLOCK + threadIdx.x) >> 6;
    if (w >= nid) return;                               // (whole wavefronts)
    const uint32_t i = (uint32_t)w, b = poff[i], e = poff[i + 1u];
    const unsigned lane = lane_id();
    if (e <= b || e > nkept) {
        if (lane == 0u) { hcnt[i] = 0u; hstart[i] = 0u; }
        return;
    }
    const uint32_t m = e - b;
    if (m <= HL_WAVE_MAX) {
        const bool valid = lane < m;
        const long long x = valid ? (long long)pcol[b + lane] : 0, y = valid ? (long long)prow[b + lane] : 0;
        const long long px = __shfl_up(x, 1, 64), py = __shfl_up(y, 1, 64);
        const unsigned long long live0 = __ballot(valid && !(lane > 0u && px == x && py == y));
        const unsigned long long L = hl_wave_chain(live0, false, x, y), U = hl_wave_chain(live0, true, x, y);
        const unsigned first = (unsigned)__builtin_ctzll(live0), last = 63u - (unsigned)__builtin_clzll(live0);
        const unsigned long long lt = lanemask_lt(), gt = lane == 63u ? 0ull : ~((2ull << lane) - 1ull);
        const uint32_t nl = (uint32_t)__popcll(L), nu = (uint32_t)__popcll(U);
        const uint32_t h = first == last ? 1u : nl + nu - 2u;
        const bool inL = ((L >> lane) & 1ull) && (lane != last || first == last), inU = ((U >> lane) & 1ull) && lane != first;
        const bool on = inL || (inU && first != last);
        const uint32_t at = inL ? (uint32_t)__popcll(L & lt) : nl - 1u + (uint32_t)__popcll(U & gt);
        unsigned long long key = on ? ((unsigned long long)y << 32) | (unsigned long long)x : ~0ull, best = key;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = (unsigned long long)__shfl_xor(best, d, 64);
            best = o < best ? o : best;
        }
        const unsigned long long who = __ballot(on && key == best);
        const uint32_t s = (uint32_t)__shfl((int)at, who ? __builtin_ctzll(who) : 0, 64);
        if (on && at < m) { pcol[b + at] = (uint32_t)x; prow[b + at] = (uint32_t)y; }
        if (lane == 0u) { hcnt[i] = h <= m ? h : 0u; hstart[i] = s < h ? s : 0u; }
        return;
    }
    if (lane != 0u) return;
    // Andrew's stack on one lane.  The upper chain first, in descending order, into the stack of its own ...
    uint32_t nu = 0u;
    for (uint32_t k = m; k-- > 0u;) {
        const long long x = pcol[b + k], y = prow[b + k];
        if (nu && (long long)stk_c[b + nu - 1u] == x && (long long)stk_r[b + nu - 1u] == y) continue;
        while (nu >= 2u && hl_cross(stk_c[b + nu - 2u], stk_r[b + nu - 2u], stk_c[b + nu - 1u], stk_r[b + nu - 1u], x, y) <= 0) nu--;
        stk_c[b + nu] = (uint32_t)x; stk_r[b + nu] = (uint32_t)y;
        nu++;
    }
    // ... then the lower chain in place: the stack never reaches the point that is read
    uint32_t nl = 0u;
    for (uint32_t k = 0u; k < m; k++) {
        const long long x = pcol[b + k], y = prow[b + k];
        if (nl && (long long)pcol[b + nl - 1u] == x && (long long)prow[b + nl - 1u] == y) continue;
        while (nl >= 2u && hl_cross(pcol[b + nl - 2u], prow[b + nl - 2u], pcol[b + nl - 1u], prow[b + nl - 1u], x, y) <= 0) nl--;
        pcol[b + nl] = (uint32_t)x; prow[b + nl] = (uint32_t)y;
        nl++;
    }
    uint32_t h = nl <= 1u ? 1u : nl + nu - 2u;
    if (h > m) h = 0u;                                  // (cannot happen: the chains share their two ends only)
    for (uint32_t j = 0u; nl > 1u && j + 1u < nu && nl - 1u + j < m; j++) {
        pcol[b + nl - 1u + j] = stk_c[b + j];
        prow[b + nl - 1u + j] = stk_r[b + j];
    }
    uint32_t s = 0u;
    unsigned long long best = ~0ull;
    for (uint32_t j = 0u; j < h; j++) {
        const unsigned long long key = ((unsigned long long)prow[b + j] << 32) | (unsigned long long)pcol[b + j];
        if (key < best) { best = key; s = j; }
    }
    hcnt[i] = h;
    hstart[i] = s;
}

__global__ __launch_bounds__(256) void k_hl_emit(const uint32_t *__restrict__ pid, const uint32_t *__restrict__ pcol,
                                                 const uint32_t *__restrict__ prow, uint32_t nkept, const uint32_t *__restrict__ poff,
                                                 const uint32_t *__restrict__ hcnt, const uint32_t *__restrict__ hstart,
                                                 const uint32_t *__restrict__ hoff, uint32_t nid, uint32_t nh, long long r0, long long c0,
                                                 longlong2 *__restrict__ pts)
{
    const size_t t = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (t >= nkept) return;
    const uint32_t k = (uint32_t)t, i = pid[k];
    if (i >= nid || k < poff[i]) return;
    const uint32_t j = k - poff[i], h = hcnt[i];
    if (j >= h) return;
    const uint32_t s = hstart[i], at = hoff[i] + (j >= s ? j - s : j + h - s);
    if (at >= nh) return;                               // (cannot happen)
    pts[at] = make_longlong2(r0 + (long long)prow[k], c0 + (long long)pcol[k]);
}

// hoff64[i] = hoff[i] for i <= S, the hull points for i = S + 1
__global__ __launch_bounds__(256) void k_hl_widen(const uint32_t *__restrict__ hoff, uint32_t nid, uint32_t nh, long long *__restrict__ hoff64)
{
    const size_t i = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    if (i <= nid) hoff64[i] = i < nid ? (long long)hoff[i] : (long long)nh;
}

// the largest v of the lanes with the same key goes to acc[key]; the lanes that share the first lane's key together
__device__ __forceinline__ void hl_wave_max(unsigned long long *acc, uint32_t key, unsigned long long v)
{
    const uint32_t k0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)key);
    const bool same = key == k0;
    unsigned long long s = same ? v : 0ull;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const unsigned long long o = (unsigned long long)__shfl_xor(s, d, 64);
        s = o > s ? o : s;
    }
    if (k0 != OL_NONE && lane_id() == (unsigned)__builtin_ctzll(__ballot(true)) && s != 0ull) atomicMax(&acc[k0], s);
    if (!same && key != OL_NONE && v != 0ull) atomicMax(&acc[key], v);
}

__global__ __launch_bounds__(256) void k_hl_reach(const longlong2 *__restrict__ pts, const uint32_t *__restrict__ hoff,
                                                  const uint32_t *__restrict__ hcnt, uint32_t nid, uint32_t nh, long long r0,
                                                  long long c0, long long *__restrict__ reach, unsigned long long *__restrict__ area2,
                                                  unsigned long long *__restrict__ feret2)
{
    const size_t t = (size_t)blockIdx.x * OL_BLOCK + threadIdx.x;
    uint32_t key = OL_NONE;
    unsigned long long term = 0ull, d2 = 0ull;
    if (t < nh) {
        // the id of hull point t: the last i with hoff[i] <= t
        uint32_t lo = 0u, hi = nid;
        while (hi - lo > 1u) {
            const uint32_t mid = lo + (hi - lo) / 2u;
            if (hoff[mid] <= (uint32_t)t) lo = mid; else hi = mid;
        }
        const uint32_t i = lo, b0 = hoff[i], h = hcnt[i], j0 = (uint32_t)t - b0;
        long long rch = 0;
        if (j0 < h && b0 + h <= nh) {
            key = i;
            const longlong2 A = pts[t], B = pts[b0 + (j0 + 1u == h ? 0u : j0 + 1u)];
            const long long ax = A.y - c0, ay = A.x - r0, bx = B.y - c0, by = B.x - r0;
            term = (unsigned long long)(ax * by - bx * ay);
            if (h == 2u) d2 = (unsigned long long)((bx - ax) * (bx - ax) + (by - ay) * (by - ay));
            if (h >= 3u) {
                // point j of the walk from b: j = 0 is b, j = h - 1 is a.  turn(j) = the edge from point j to point
                // j + 1 still leads away from the line a b; true at 0, false at h - 2, and never true after false
                auto P = [&](uint32_t j) { uint32_t q = j0 + 1u + j; q = q >= h ? q - h : q; return pts[b0 + (q >= h ? q - h : q)]; };
                auto turn = [&](uint32_t j) {
                    const longlong2 p = P(j), q = P(j + 1u);
                    return (bx - ax) * (q.x - p.x) - (by - ay) * (q.y - p.y) > 0;
                };
                uint32_t l = 0u, r = h - 2u;
                while (r - l > 1u) {
                    const uint32_t mid = l + (r - l) / 2u;
                    if (turn(mid)) l = mid; else r = mid;
                }
                if (h == 3u) r = 1u;
                const longlong2 Q = P(r), Q2 = P(r + 1u);
                const long long qx = Q.y - c0, qy = Q.x - r0, sx = Q2.y - c0, sy = Q2.x - r0;
                rch = hl_cross(ax, ay, bx, by, qx, qy);
                auto dist2 = [](long long ux, long long uy, long long vx, long long vy) {
                    return (unsigned long long)((ux - vx) * (ux - vx) + (uy - vy) * (uy - vy));
                };
                d2 = max(dist2(ax, ay, qx, qy), dist2(bx, by, qx, qy));
                if (hl_cross(ax, ay, bx, by, sx, sy) == rch) d2 = max(d2, max(dist2(ax, ay, sx, sy), dist2(bx, by, sx, sy)));
                d2 = max(d2, dist2(ax, ay, bx, by));
            }
            reach[t] = rch;
        }
    }
    ol_wave_add<unsigned long long>(area2, key, term);
    hl_wave_max(feret2, key, d2);
}

// ---- host side --------------------------------------------------------------------------------------------
// the buffers uploaded rings go into
static inline RingBufs hl_ring_bufs(shp_ctx *ctx) { return RingBufs{ctx->hl_vtx, ctx->hl_voff, ctx->hl_roff, ctx->hl_area, nullptr}; }

// bytes of an id's rows in hl_id: poff, hcnt, hstart, hoff (4 each, S + 2 rows), hoff64, area2, feret2 (8 each)
#define HL_ID_BYTES 40u

// the device memory the buffers still have to grow by for nv vertices in nr rings of the ids 0 .. S, at the bounds
// candidates <= nv and hull points <= nv; upload: the rings go into buffers of this file's own
static int run_hull_need(shp_ctx *ctx, size_t nv, size_t nr, size_t S, int upload, long long *need_out, long long *free_out)
{
    size_t need = upload ? ring_upload_need(hl_ring_bufs(ctx), nv, nr, S) : 0;
    need += ol_grown(ctx->hl_pos, nv * 4) + ol_grown(ctx->hl_cid, nv * 4) + ol_grown(ctx->hl_ccol, nv * 4) + ol_grown(ctx->hl_crow, nv * 4);
    need += ol_grown(ctx->hl_k, nv * 4) + ol_grown(ctx->hl_v, nv * 4);
    need += ol_grown(ctx->sort_k0, nv * 4) + ol_grown(ctx->sort_k1, nv * 4) + ol_grown(ctx->sort_v1, nv * 4) + ol_grown(ctx->pix, nv * 4);
    const size_t nh = (size_t)256 * ((nv + SORT_TILE - 1) / SORT_TILE + 1);
    need += ol_grown(ctx->sort_hist, 2 * nh * 4);
    const size_t nscan = nv > nh ? (nv > S + 2 ? nv : S + 2) : (nh > S + 2 ? nh : S + 2);
    need += ol_grown(ctx->scan_tmp, scan_tmp_bytes(nscan));
    need += ol_grown(ctx->hl_id, (S + 2) * HL_ID_BYTES + 64) + ol_grown(ctx->hl_pts, nv * 16) + ol_grown(ctx->hl_reach, nv * 8);
    need += ol_grown(ctx->hl_ctr, HL_CTR_WORDS * 4);
    size_t fr = 0, tot = 0;
    HIPCHK(ctx, hipMemGetInfo(&fr, &tot));
    *need_out = (long long)need;
    *free_out = (long long)fr;
    return 0;
}

// the rings to hull: the context's traced outlines in place (all arrays NULL), or host arrays uploaded
static int run_hull_source(shp_ctx *ctx, const int64_t *ring_offsets, const int64_t *vertex_offsets, const int64_t *vertices,
                           const int64_t *ring_area2, uint32_t S, uint32_t nr, uint32_t nv, double *upload_ms_out)
{
    HullState &h = ctx->hull;
    h = HullState{};
    CHK(ring_source_take(ctx, h.src, hl_ring_bufs(ctx), ring_offsets, vertex_offsets, vertices, ring_area2, nullptr, S, nr, nv, upload_ms_out));
    h.stage = 1;
    return 0;
}

static int run_hull_build(shp_ctx *ctx, long long r0, long long c0, uint32_t row_span, uint32_t col_span, int convex_only)
{
    HullState &h = ctx->hull;
    hipStream_t st = ctx->stream;
    h.stage = 0;
    h.nh = h.ncand = h.nkept = 0u;
    for (int i = 0; i < 5; i++) h.ms[i] = 0.0;
    const uint32_t nv = h.src.nv, nr = h.src.nr, S = h.src.S, nid = S + 1u;
    const HlSrc src{ring_view(ctx, h.src, hl_ring_bufs(ctx)), r0, c0, convex_only};
    // hl_id: poff, hcnt, hstart, hoff (S + 2 uint32 each, 16-byte aligned starts), then hoff64 (S + 2), area2, feret2 (S + 1)
    const size_t q = ((size_t)S + 2 + 3) & ~(size_t)3;
    CHK(buf_ensure(ctx, ctx->hl_id, q * 16 + ((size_t)S + 2) * 24));
    CHK(buf_ensure(ctx, ctx->hl_ctr, HL_CTR_WORDS * 4));
    uint32_t *poff = bp<uint32_t>(ctx->hl_id), *hcnt = poff + q, *hstart = hcnt + q, *hoff = hstart + q;
    long long *hoff64 = (long long *)(hoff + q);
    unsigned long long *area2 = (unsigned long long *)(hoff64 + S + 2), *feret2 = area2 + S + 2;
    uint32_t *ctr = bp<uint32_t>(ctx->hl_ctr);
    volatile uint32_t *hp = (volatile uint32_t *)ctx->h_pinned;
    h.hoff64_at = (size_t)((char *)hoff64 - (char *)ctx->hl_id.p);
    h.area_at = (size_t)((char *)area2 - (char *)ctx->hl_id.p);
    h.feret_at = (size_t)((char *)feret2 - (char *)ctx->hl_id.p);
    HIPCHK(ctx, hipMemsetAsync(ctx->hl_id.p, 0, q * 16 + ((size_t)S + 2) * 24, st));
    HIPCHK(ctx, hipMemsetAsync(ctr, 0, HL_CTR_WORDS * 4, st));
    if (nv == 0u || nr == 0u) {
        HIPCHK(ctx, hipStreamSynchronize(st));
        h.stage = 2;
        return 0;
    }
    // ---- step 1: candidates
    CHK(buf_ensure(ctx, ctx->hl_pos, (size_t)nv * 4));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(nv)));
    uint32_t *pos = bp<uint32_t>(ctx->hl_pos);
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    HlCandFn cf{src};
    CHK(scan_exclusive(ctx, cf, nv, pos, ctr + 0, bp<uint32_t>(ctx->scan_tmp)));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nc = hp[0];
    if (nc > nv) SHP_FAIL(ctx, SHP_ERR_STATE, "hull: %u candidates of %u vertices", nc, nv);
    h.ncand = nc;
    if (nc == 0u) {                                     // (rings without an outer ring: no hulls)
        h.stage = 2;
        return 0;
    }
    CHK(buf_ensure(ctx, ctx->hl_cid, (size_t)nc * 4));
    CHK(buf_ensure(ctx, ctx->hl_ccol, (size_t)nc * 4));
    CHK(buf_ensure(ctx, ctx->hl_crow, (size_t)nc * 4));
    CHK(buf_ensure(ctx, ctx->hl_k, (size_t)nc * 4));
    CHK(buf_ensure(ctx, ctx->hl_v, (size_t)nc * 4));
    uint32_t *cid = bp<uint32_t>(ctx->hl_cid), *ccol = bp<uint32_t>(ctx->hl_ccol), *crow = bp<uint32_t>(ctx->hl_crow);
    uint32_t *hk = bp<uint32_t>(ctx->hl_k), *hv = bp<uint32_t>(ctx->hl_v);
    const unsigned cgrid = grid_for(nc, OL_BLOCK);
    hipLaunchKernelGGL(k_hl_cand, dim3(grid_for(nv, OL_BLOCK)), dim3(OL_BLOCK), 0, st, src, (const uint32_t *)pos, nc, cid, ccol, crow);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    // ---- step 2: (id, col, row) order, the ends of every (id, col) run, the ids' ranges
    uint32_t *ks = nullptr, *vs = nullptr;
    CHK(sort_pairs(ctx, crow, nullptr, nc, bits_for(row_span), nullptr, &vs));
    hipLaunchKernelGGL(k_hl_gather, dim3(cgrid), dim3(OL_BLOCK), 0, st, (const uint32_t *)vs, (const uint32_t *)ccol, nc, hk, hv);
    KCHK(ctx);
    CHK(sort_pairs(ctx, hk, hv, nc, bits_for(col_span), nullptr, &vs));
    hipLaunchKernelGGL(k_hl_gather, dim3(cgrid), dim3(OL_BLOCK), 0, st, (const uint32_t *)vs, (const uint32_t *)cid, nc, hk, hv);
    KCHK(ctx);
    CHK(sort_pairs(ctx, hk, hv, nc, bits_for(S), &ks, &vs));
    hipLaunchKernelGGL(k_hl_gather, dim3(cgrid), dim3(OL_BLOCK), 0, st, (const uint32_t *)vs, (const uint32_t *)ccol, nc, hk, (uint32_t *)nullptr);
    KCHK(ctx);
    hipLaunchKernelGGL(k_hl_gather, dim3(cgrid), dim3(OL_BLOCK), 0, st, (const uint32_t *)vs, (const uint32_t *)crow, nc, hv, (uint32_t *)nullptr);
    KCHK(ctx);
    HlKeepFn kf{ks, hk, nc};
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(nc > nid ? nc : nid)));
    CHK(scan_exclusive(ctx, kf, nc, pos, ctr + 1, bp<uint32_t>(ctx->scan_tmp)));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr + 1, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nk = hp[0];
    if (nk == 0u || nk > nc) SHP_FAIL(ctx, SHP_ERR_STATE, "hull: %u points kept of %u candidates", nk, nc);
    h.nkept = nk;
    hipLaunchKernelGGL(k_hl_compact, dim3(cgrid), dim3(OL_BLOCK), 0, st, kf, (const uint32_t *)hv, (const uint32_t *)pos, nk, cid, ccol, crow);
    KCHK(ctx);
    hipLaunchKernelGGL(k_hl_idoff, dim3(grid_for((size_t)S + 2, OL_BLOCK)), dim3(OL_BLOCK), 0, st, (const uint32_t *)cid, nk, (size_t)S + 2, poff);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
    // ---- step 3: chains (hk / hv are free: the stack of the ids walked by one lane)
    hipLaunchKernelGGL(k_hl_chain, dim3(grid_for((size_t)nid * 64, OL_BLOCK)), dim3(OL_BLOCK), 0, st, (const uint32_t *)poff, nid, nk, ccol,
                       crow, hk, hv, hcnt, hstart);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[3], st));
    // ---- step 4: offsets and points
    ArrFn hf{hcnt};
    CHK(scan_exclusive(ctx, hf, nid, hoff, ctr + 2, bp<uint32_t>(ctx->scan_tmp)));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr + 2, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nh = hp[0];
    if (nh == 0u || nh > nk) SHP_FAIL(ctx, SHP_ERR_STATE, "hull: %u hull points of %u kept points", nh, nk);
    CHK(buf_ensure(ctx, ctx->hl_pts, (size_t)nh * 16));
    CHK(buf_ensure(ctx, ctx->hl_reach, (size_t)nh * 8));
    longlong2 *pts = bp<longlong2>(ctx->hl_pts);
    long long *reach = bp<long long>(ctx->hl_reach);
    HIPCHK(ctx, hipMemsetAsync(reach, 0, (size_t)nh * 8, st));
    hipLaunchKernelGGL(k_hl_emit, dim3(grid_for(nk, OL_BLOCK)), dim3(OL_BLOCK), 0, st, (const uint32_t *)cid, (const uint32_t *)ccol,
                       (const uint32_t *)crow, nk, (const uint32_t *)poff, (const uint32_t *)hcnt, (const uint32_t *)hstart,
                       (const uint32_t *)hoff, nid, nh, r0, c0, pts);
    KCHK(ctx);
    hipLaunchKernelGGL(k_hl_widen, dim3(grid_for((size_t)nid + 1, OL_BLOCK)), dim3(OL_BLOCK), 0, st, (const uint32_t *)hoff, nid, nh, hoff64);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[4], st));
    // ---- step 5: reach, diameter, area
    hipLaunchKernelGGL(k_hl_reach, dim3(grid_for(nh, OL_BLOCK)), dim3(OL_BLOCK), 0, st, (const longlong2 *)pts, (const uint32_t *)hoff,
                       (const uint32_t *)hcnt, nid, nh, r0, c0, reach, area2, feret2);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[5], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int i = 0; i < 5; i++) h.ms[i] = ol_elapsed(ctx->ev[i], ctx->ev[i + 1]);
    h.nh = nh;
    h.stage = 2;
    return 0;
}

static int run_hull_download(shp_ctx *ctx, int64_t *hull_offsets, int64_t *hull_points, int64_t *hull_reach, int64_t *hull_area2,
                             int64_t *feret_max2)
{
    const HullState &h = ctx->hull;
    hipStream_t st = ctx->stream;
    const char *id = (const char *)ctx->hl_id.p;
    HIPCHK(ctx, hipMemcpyAsync(hull_offsets, id + h.hoff64_at, ((size_t)h.src.S + 2) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hull_area2, id + h.area_at, ((size_t)h.src.S + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(feret_max2, id + h.feret_at, ((size_t)h.src.S + 1) * 8, hipMemcpyDeviceToHost, st));
    if (h.nh) {
        HIPCHK(ctx, hipMemcpyAsync(hull_points, ctx->hl_pts.p, (size_t)h.nh * 16, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(hull_reach, ctx->hl_reach.p, (size_t)h.nh * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}
