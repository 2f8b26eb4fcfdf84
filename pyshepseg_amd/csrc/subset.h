// subset.h -- subset.subsetImage's recode on the device.
//
// Replaces the tile loop of subset.subsetImage (subset.py:124-166) and its njit kernel
// processSubsetTile (subset.py:366-425): the window is visited tile by tile (tile rows outer,
// tile columns inner, raster order inside a tile) and an id gets the next new number the first
// time it is seen.  "First seen" is a minimum: every window pixel has a position in that visiting
// order (subset_key), first[id] = min key over the id's unmasked pixels (only pixels that have
// no unmasked same-id neighbour to the left or above inside their tile can hold it), and the new
// id is the rank of first[id] among the ids present -- one radix sort of (key, id) pairs.
// HBM-bound: 4 B (+1 B mask) in twice, 4 B out per pixel.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"
#include "clump.h"      // k_run_count
#include "elim_small.h" // bits_for

// The kernels work on a slice of the window: window rows [r0, r0 + nr), of which the label rows
// from image row base_row on are at seg (a rank's rows of a row-sharded raster; the one-GPU recode
// is the slice base_row = 0, r0 = 0, nr = ys).  Keys stay in the whole window's visiting order.
struct SubsetGeom {
    const uint32_t *seg;        // label rows from image row base_row on, row pitch img_cols
    const uint8_t *mask;        // xs bytes per held window row (row r0 first), or nullptr
    uint32_t img_cols, tlx, tly, xs, ys, T;
    uint32_t base_row, r0, nr;
};

__device__ __forceinline__ uint32_t subset_key(const SubsetGeom &g, uint32_t r, uint32_t c)
{
    const uint32_t tr = r / g.T, tc = c / g.T;
    const uint32_t th = g.ys - tr * g.T < g.T ? g.ys - tr * g.T : g.T;
    const uint32_t tw = g.xs - tc * g.T < g.T ? g.xs - tc * g.T : g.T;
    return tr * g.T * g.xs + tc * g.T * th + (r - tr * g.T) * tw + (c - tc * g.T);
}

// r: window row, r0 <= r < r0 + nr
__device__ __forceinline__ uint32_t subset_id(const SubsetGeom &g, uint32_t r, uint32_t c)
{
    if (g.mask && g.mask[(size_t)(r - g.r0) * g.xs + c] == 0) return 0u;
    return g.seg[((size_t)g.tly + r - g.base_row) * g.img_cols + (g.tlx + c)];
}

__global__ __launch_bounds__(256) void k_subset_first(SubsetGeom g, uint32_t max_id, uint32_t *first,
                                                      uint32_t *bad)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= g.xs * g.nr) return;
    const uint32_t q = p / g.xs, c = p - q * g.xs, r = g.r0 + q;
    const uint32_t s = subset_id(g, r, c);
    if (s == 0u) return;
    if (s > max_id) { *bad = 1u; return; }
    // a same-id pixel to the left / above in the same tile comes earlier in the visiting order (the
    // row above the slice's first is not held: without the test the min is still right)
    if (c % g.T != 0u && subset_id(g, r, c - 1) == s) return;
    if (r % g.T != 0u && r > g.r0 && subset_id(g, r - 1, c) == s) return;
    const uint32_t key = subset_key(g, r, c);
    if (key < first[s]) atomicMin(&first[s], key);
}

struct PresentFn {
    const uint32_t *first;
    __device__ __forceinline__ uint32_t operator()(uint32_t s) const
    {
        return (s != 0u && first[s] != 0xFFFFFFFFu) ? 1u : 0u;
    }
};

__global__ __launch_bounds__(256) void k_subset_list(const uint32_t *__restrict__ first,
                                                     const uint32_t *__restrict__ slot, uint32_t max_id,
                                                     uint32_t *__restrict__ keys, uint32_t *__restrict__ ids)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s == 0u || s > max_id) return;
    const uint32_t f = first[s];
    if (f == 0xFFFFFFFFu) return;
    keys[slot[s]] = f;
    ids[slot[s]] = s;
}

// sorted ids -> lut[old] = rank + 1, orig[rank + 1] = old
__global__ __launch_bounds__(256) void k_subset_lut(const uint32_t *__restrict__ ids, uint32_t m,
                                                    uint32_t *__restrict__ lut, uint32_t *__restrict__ orig)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= m) return;
    const uint32_t s = ids[i];
    lut[s] = i + 1u;
    orig[i + 1u] = s;
}

__global__ __launch_bounds__(256) void k_subset_apply(SubsetGeom g, const uint32_t *__restrict__ lut,
                                                      uint32_t *__restrict__ out)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= g.xs * g.nr) return;
    const uint32_t q = p / g.xs, c = p - q * g.xs;
    const uint32_t s = subset_id(g, g.r0 + q, c);
    out[p] = s ? lut[s] : 0u;
}

// The all-gathered pairs of shp_dsubset_merge_dev: `world` slots of 2 * slot words, slot r holds
// counts[r] keys, then their counts[r] ids; first[id] = min key over all of them.
__global__ __launch_bounds__(256) void k_subset_scatter(const uint32_t *__restrict__ pairs, uint32_t slot,
                                                        uint32_t world, const uint32_t *__restrict__ counts,
                                                        uint32_t max_id, uint32_t *first)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= slot * world) return;
    const uint32_t r = i / slot, j = i - r * slot, n = counts[r];
    if (j >= n) return;                                   // slot padding
    const uint32_t *base = pairs + (size_t)r * 2u * slot;
    const uint32_t key = base[j], s = base[n + j];
    if (s == 0u || s > max_id) return;
    if (key < first[s]) atomicMin(&first[s], key);
}

// the workspace of a recode of ids 0..max_id
struct SubsetWs {
    uint32_t *first, *slot, *lut, *keys, *ids, *orig, *scal, *scan;
};

static int subset_ws(shp_ctx *ctx, size_t ns, SubsetWs *w)
{
    CHK(buf_ensure(ctx, ctx->segsz, (ns + 1) * 4));           // first[]
    CHK(buf_ensure(ctx, ctx->off, (ns + 1) * 4 + 16));          // compaction slots
    CHK(buf_ensure(ctx, ctx->origsz, (ns + 1) * 4));            // lut
    CHK(buf_ensure(ctx, ctx->tlist, (ns + 1) * 4));             // keys
    CHK(buf_ensure(ctx, ctx->tsorted, (ns + 1) * 4));           // ids
    CHK(buf_ensure(ctx, ctx->mergeto, (ns + 1) * 4));           // orig
    CHK(buf_ensure(ctx, ctx->small, 64));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(ns)));
    *w = SubsetWs{bp<uint32_t>(ctx->segsz), bp<uint32_t>(ctx->off), bp<uint32_t>(ctx->origsz),
                  bp<uint32_t>(ctx->tlist), bp<uint32_t>(ctx->tsorted), bp<uint32_t>(ctx->mergeto),
                  bp<uint32_t>(ctx->small), bp<uint32_t>(ctx->scan_tmp)};
    HIPCHK(ctx, hipMemsetAsync(w->first, 0xff, ns * 4, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(w->scal, 0, 16, ctx->stream));
    return 0;
}

// first[] over the slice's pixels; scal[1] = 1 if one of them holds an id above max_id
static int subset_first(shp_ctx *ctx, const SubsetGeom &g, uint32_t max_id, const SubsetWs &w)
{
    const uint32_t n = g.xs * g.nr;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_subset_first, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream, g, max_id, w.first,
                       w.scal + 1);
    KCHK(ctx);
    return 0;
}

// the ids present in first[]: their slots, *m of them, *bad the flag of subset_first
static int subset_present(shp_ctx *ctx, const SubsetWs &w, size_t ns, uint32_t *m, uint32_t *bad)
{
    PresentFn pf{w.first};
    CHK(scan_exclusive(ctx, pf, (uint32_t)ns, w.slot, w.scal, w.scan));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, w.scal, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *m = ctx->h_pinned[0];
    *bad = ctx->h_pinned[1];
    return 0;
}

// the m ids present, numbered in first-seen order of a window of n_win pixels: lut[old] = new,
// orig[new] = old (orig[0] = 0)
static int subset_number(shp_ctx *ctx, const SubsetWs &w, uint32_t max_id, uint32_t m, uint32_t n_win)
{
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_subset_list, dim3(grid_for((size_t)max_id + 1, 256)), dim3(256), 0, st, w.first, w.slot,
                       max_id, w.keys, w.ids);
    KCHK(ctx);
    uint32_t *ksorted = nullptr, *isorted = nullptr;
    CHK(sort_pairs(ctx, w.keys, w.ids, m, bits_for(n_win - 1u), &ksorted, &isorted));
    HIPCHK(ctx, hipMemsetAsync(w.orig, 0, 4, st));
    if (m) {
        hipLaunchKernelGGL(k_subset_lut, dim3(grid_for(m, 256)), dim3(256), 0, st, isorted, m, w.lut, w.orig);
        KCHK(ctx);
    }
    return 0;
}

// the slice recoded into out (xs * nr labels), its new ids counted into hist (zeroed by the caller)
static int subset_apply(shp_ctx *ctx, const SubsetGeom &g, const SubsetWs &w, uint32_t *out, uint32_t *hist)
{
    const uint32_t n = g.xs * g.nr;
    if (n == 0) return 0;
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_subset_apply, dim3(grid_for(n, 256)), dim3(256), 0, st, g, w.lut, out); KCHK(ctx);
    hipLaunchKernelGGL(k_run_count, dim3(grid_for(n, 256)), dim3(256), 0, st, out, n, hist, 0u, 1); KCHK(ctx);
    return 0;
}

// d_seg: device label raster (img_rows x img_cols); d_mask: device xs*ys bytes or nullptr;
// d_out: device xs*ys labels.  orig_out / hist_out: HOST arrays of cap entries.
static int run_subset_recode(shp_ctx *ctx, const uint32_t *d_seg, uint32_t img_cols, uint32_t tlx,
                             uint32_t tly, uint32_t xs, uint32_t ys, const uint8_t *d_mask,
                             uint32_t tile_size, uint32_t max_id, uint32_t *d_out, uint32_t *orig_out,
                             uint32_t *hist_out, int64_t cap, uint32_t *n_new_out)
{
    hipStream_t st = ctx->stream;
    const uint32_t n = xs * ys;
    const size_t ns = (size_t)max_id + 1;
    *n_new_out = 0;
    if (n == 0) return 0;
    SubsetWs w;
    CHK(subset_ws(ctx, ns, &w));
    CHK(buf_ensure(ctx, ctx->tcount, (ns + 1) * 4));            // hist
    uint32_t *hist = bp<uint32_t>(ctx->tcount);
    const SubsetGeom g{d_seg, d_mask, img_cols, tlx, tly, xs, ys, tile_size, 0u, 0u, ys};
    CHK(subset_first(ctx, g, max_id, w));
    uint32_t m = 0, bad = 0;
    CHK(subset_present(ctx, w, ns, &m, &bad));
    if (bad) SHP_FAIL(ctx, SHP_ERR_ARG, "segment id above max_seg_id (%u) in the subset", max_id);
    if ((int64_t)m + 1 > cap)
        SHP_FAIL(ctx, SHP_ERR_ARG, "subset holds %u segments, output arrays hold %lld rows", m, (long long)cap);
    CHK(subset_number(ctx, w, max_id, m, n));
    HIPCHK(ctx, hipMemsetAsync(hist, 0, ((size_t)m + 1) * 4, st));
    CHK(subset_apply(ctx, g, w, d_out, hist));
    HIPCHK(ctx, hipMemcpyAsync(orig_out, w.orig, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(hist_out, hist, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    *n_new_out = m;
    return 0;
}

// ---- the recode of a row-sharded window (shp_dsubset_local_dev / shp_dsubset_merge_dev) ----
// A rank holds window rows [g.r0, g.r0 + g.nr).  Local: first[] over them, the ids present packed as
// m keys then m ids at *d_pairs_out (the context's workspace, valid until its next call).
static int run_dsubset_local(shp_ctx *ctx, const SubsetGeom &g, uint32_t max_id, void **d_pairs_out,
                             int64_t *n_pairs_out, int *bad_out)
{
    const size_t ns = (size_t)max_id + 1;
    SubsetWs w;
    CHK(subset_ws(ctx, ns, &w));
    CHK(buf_ensure(ctx, ctx->toff, (2 * ns + 2) * 4));
    uint32_t *pairs = bp<uint32_t>(ctx->toff);
    CHK(subset_first(ctx, g, max_id, w));
    uint32_t m = 0, bad = 0;
    CHK(subset_present(ctx, w, ns, &m, &bad));
    if (m) {
        hipLaunchKernelGGL(k_subset_list, dim3(grid_for(ns, 256)), dim3(256), 0, ctx->stream, w.first, w.slot,
                           max_id, pairs, pairs + m);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *d_pairs_out = pairs;
    *n_pairs_out = m;
    *bad_out = bad ? 1 : 0;
    return 0;
}

// Merge, on every rank: the all-gathered pairs (k_subset_scatter) -> the same numbering everywhere;
// the held rows recoded into d_out (xs * nr), their new ids counted into d_hist (cap words, zeroed
// here); orig_out (host, cap words) = old id per new id, *n_new_out = m.
static int run_dsubset_merge(shp_ctx *ctx, const uint32_t *d_pairs, uint32_t slot, uint32_t world,
                             const uint32_t *counts, const SubsetGeom &g, uint32_t max_id, uint32_t *d_out,
                             uint32_t *d_hist, uint32_t *orig_out, int64_t cap, uint32_t *n_new_out)
{
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)max_id + 1;
    *n_new_out = 0;
    SubsetWs w;
    CHK(subset_ws(ctx, ns, &w));
    if (slot > 0) {
        CHK(buf_ensure(ctx, ctx->tfill, (size_t)world * 4));
        uint32_t *d_counts = bp<uint32_t>(ctx->tfill);
        HIPCHK(ctx, hipMemcpyAsync(d_counts, counts, (size_t)world * 4, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_subset_scatter, dim3(grid_for((size_t)slot * world, 256)), dim3(256), 0, st, d_pairs,
                           slot, world, d_counts, max_id, w.first);
        KCHK(ctx);
    }
    uint32_t m = 0, bad = 0;
    CHK(subset_present(ctx, w, ns, &m, &bad));
    if ((int64_t)m + 1 > cap)
        SHP_FAIL(ctx, SHP_ERR_ARG, "subset holds %u segments, output arrays hold %lld rows", m, (long long)cap);
    CHK(subset_number(ctx, w, max_id, m, g.xs * g.ys));
    HIPCHK(ctx, hipMemsetAsync(d_hist, 0, (size_t)cap * 4, st));
    CHK(subset_apply(ctx, g, w, d_out, d_hist));
    HIPCHK(ctx, hipMemcpyAsync(orig_out, w.orig, ((size_t)m + 1) * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    *n_new_out = m;
    return 0;
}
