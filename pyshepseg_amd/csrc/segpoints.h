// segpoints.h -- every segment's non-nodata pixels as (x, y, value) points, in the reference's visit order,
// for user-defined spatial statistics (tilingstats.iterSegmentPoints / calcPerSegmentSpatialStats with any
// userFunc).
//
// Replaces the point accumulation of calcPerSegmentSpatialStatsTiled (tilingstats.py:1262-1390):
// accumulateSegSpatial (:1652-1699) walks the raster in tileSize x tileSize tiles, tiles in row-major order and
// pixels row-major inside a tile, and appends SegPoint(x, y, value) to its segment's list for every pixel whose
// label is not 0 and whose value is not the nodata value.  The lists here are the same: a stable sort by id of
// all valid pixels taken in that VISIT ORDER.  As in csr.h the sort moves runs, not pixels: a run is a maximal
// sequence of consecutive visit indices with one id, cut at the end of a tile row (where the visit jumps to the
// tile's next row) and at multiples of 64 (a wavefront sees whole runs); runs come out in ascending visit index,
// so the stable sort of the runs by id keeps every segment's runs in visit order.  A run covers consecutive
// pixels of one image row, so a run table entry is its raster position (32 bits: n < 2^32) and its length, and
// the sort's payload is the index of that entry.
//
// Two steps: run_segpoints_build does the sort once (for the whole raster; the result stays in the context's
// workspace), run_segpoints_emit expands the runs of an id range [lo, hi) into 16-byte records
// {uint32 x; uint32 y; int64 val} (the reference's SegPoint with val widened to numbaTypeForImageType, int64) and
// downloads them with the per-id offsets -- a batch at a time, so that the points of a raster need not fit in
// host memory at once.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"
#include "spatial.h"

#define PTS_TILE 4096u          // visit indices per workgroup: 4 wavefronts x 16 rows of 64
#define PTS_ROWS 16u

// The rows seg / band hold: nrows x ncols pixels, the whole raster or a slice of it (dsegpoints.h: a rank's rows
// [row0, row0 + nrows) of a taller raster).  Tile rows (bands) are th rows of the WHOLE raster, so a slice's first
// band may be cut short: it holds h0 rows (th for the whole raster), every later band th rows but the last.
struct PtsGeom {
    const uint32_t *seg;
    const void *band;
    int dtype;
    uint32_t nrows, ncols, S;
    uint32_t th, tw;            // tile height / width: min(tileSize, raster rows), min(tileSize, ncols)
    long long null_val;
    uint32_t h0;                // rows of the first band
};

// visit index i (< nrows * ncols) -> raster position; *row_start: i is the first pixel of a tile row.  Tile rows
// (bands of th image rows; the first of h0) are visited one after the other; inside a band the tiles (all tw wide
// but the last), inside a tile its rows.  Every earlier band is full, and so is every earlier tile of a band.  The
// order is the raster's visit order restricted to the rows held.
__device__ __forceinline__ uint32_t pts_visit_pos(const PtsGeom &g, uint32_t i, bool *row_start)
{
    const uint32_t first = g.h0 * g.ncols;
    uint32_t rem, y0, h;
    if (i < first) {
        rem = i;
        y0 = 0u;
        h = g.h0;
    } else {
        const uint32_t bandsz = g.th * g.ncols;
        const uint32_t tr = (i - first) / bandsz;
        rem = i - first - tr * bandsz;
        y0 = g.h0 + tr * g.th;
        h = min(g.th, g.nrows - y0);
    }
    const uint32_t tilesz = h * g.tw;
    const uint32_t tc = rem / tilesz;
    rem -= tc * tilesz;
    const uint32_t x0 = tc * g.tw;
    const uint32_t w = min(g.tw, g.ncols - x0);
    const uint32_t rr = rem / w, cc = rem - rr * w;
    *row_start = cc == 0u;
    return (y0 + rr) * g.ncols + x0 + cc;
}

// One row of 64 visit indices of a wavefront: the id of this lane's pixel when it is a point (0 otherwise), its
// raster position, and the wavefront's masks of run boundaries (every lane where a run may not continue from
// the lane before) and of run heads (boundaries that start a run of points).
__device__ __forceinline__ uint32_t pts_row(const PtsGeom &g, unsigned long long i, uint32_t n, uint32_t *pos,
                                            unsigned long long *bound, unsigned long long *heads)
{
    bool rs = false;
    uint32_t key = 0u, p = 0u;
    if (i < n) {
        p = pts_visit_pos(g, (uint32_t)i, &rs);
        const uint32_t s = g.seg[p];
        if (s != 0u && s <= g.S && ld_px(g.band, g.dtype, p) != g.null_val) key = s;
    }
    const uint32_t prev = __shfl_up(key, 1, 64);
    const bool b = lane_id() == 0u || key != prev || rs;
    *bound = __ballot(b);
    *heads = __ballot(b && key != 0u);
    *pos = p;
    return key;
}

__global__ __launch_bounds__(256) void k_pts_run_count(PtsGeom g, uint32_t n, uint32_t *__restrict__ bcount)
{
    __shared__ uint32_t wc[4];
    const unsigned w = threadIdx.x >> 6, lane = lane_id();
    const unsigned long long base = (unsigned long long)blockIdx.x * PTS_TILE + w * (PTS_ROWS * 64u) + lane;
    uint32_t cnt = 0;
    for (unsigned r = 0; r < PTS_ROWS; r++) {
        uint32_t p;
        unsigned long long bd, hd;
        (void)pts_row(g, base + r * 64u, n, &p, &bd, &hd);
        cnt += (uint32_t)__popcll(hd);
    }
    if (lane == 0) wc[w] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) bcount[blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

// rkeys[j] = the run's id, rtab[j] = raster position | (length - 1) << 32, j in visit order
__global__ __launch_bounds__(256) void k_pts_run_emit(PtsGeom g, uint32_t n, const uint32_t *__restrict__ boff,
                                                      uint32_t *__restrict__ rkeys,
                                                      unsigned long long *__restrict__ rtab)
{
    __shared__ uint32_t wc[4];
    const unsigned w = threadIdx.x >> 6, lane = lane_id();
    const unsigned long long base = (unsigned long long)blockIdx.x * PTS_TILE + w * (PTS_ROWS * 64u) + lane;
    uint32_t key[PTS_ROWS], pos[PTS_ROWS];
    unsigned long long bd[PTS_ROWS], hd[PTS_ROWS];
    uint32_t cnt = 0;
#pragma unroll
    for (unsigned r = 0; r < PTS_ROWS; r++) {
        key[r] = pts_row(g, base + r * 64u, n, &pos[r], &bd[r], &hd[r]);
        cnt += (uint32_t)__popcll(hd[r]);
    }
    if (lane == 0) wc[w] = cnt;
    __syncthreads();
    uint32_t j0 = boff[blockIdx.x];
    for (unsigned q = 0; q < w; q++) j0 += wc[q];
    const unsigned long long lt = lanemask_lt();
#pragma unroll
    for (unsigned r = 0; r < PTS_ROWS; r++) {
        if ((hd[r] >> lane) & 1ull) {
            // the run ends at the next boundary: a lane past the raster's end has key 0, so is one
            const unsigned long long rest = lane == 63u ? 0ull : (bd[r] >> (lane + 1u));
            const uint32_t len = rest ? (uint32_t)__builtin_ctzll(rest) + 1u : 64u - lane;
            const uint32_t j = j0 + (uint32_t)__popcll(hd[r] & lt);
            rkeys[j] = key[r];
            rtab[j] = (unsigned long long)pos[r] | ((unsigned long long)(len - 1u) << 32);
        }
        j0 += (uint32_t)__popcll(hd[r]);
    }
}

// length of sorted run j (its run table entry is rtab[order[j]])
struct PtsLenFn {
    const uint32_t *order;
    const unsigned long long *rtab;
    __device__ __forceinline__ uint32_t operator()(uint32_t j) const { return (uint32_t)(rtab[order[j]] >> 32) + 1u; }
};

// the sorted runs of ids [lo, hi): res = {first run, end run, first point, points}; offs[k] (k = 0 .. hi - lo) =
// first point of id lo + k relative to the batch's first point (poff: exclusive scan of the per-id counts)
__global__ __launch_bounds__(256) void k_pts_range(const uint32_t *__restrict__ skeys, uint32_t m,
                                                   const uint32_t *__restrict__ poff, uint32_t lo, uint32_t hi,
                                                   uint32_t *__restrict__ res, long long *__restrict__ offs)
{
    const uint32_t base = poff[lo];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k <= hi - lo) offs[k] = (long long)(poff[lo + k] - base);
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    uint32_t b[2];
    const uint32_t want[2] = {lo, hi};
    for (int q = 0; q < 2; q++) {               // lower bound of want[q] in the sorted keys
        uint32_t a = 0, e = m;
        while (a < e) {
            const uint32_t mid = a + (e - a) / 2u;
            if (skeys[mid] < want[q]) a = mid + 1u;
            else e = mid;
        }
        b[q] = a;
    }
    res[0] = b[0];
    res[1] = b[1];
    res[2] = base;
    res[3] = poff[hi] - base;
}

// The records of sorted runs [rlo, rhi): one run per lane first, then output record t of the wavefront's runs is
// written by lane t % 64 (as csr.h's k_run_expand), so that a wavefront stores 64 consecutive 16-byte records
// per instruction.  roff: first point of every sorted run (global); base: first point of the batch.
template <int DT>
__global__ __launch_bounds__(256) void k_pts_expand(const uint32_t *__restrict__ order,
                                                    const unsigned long long *__restrict__ rtab,
                                                    const uint32_t *__restrict__ roff, uint32_t rlo, uint32_t rhi,
                                                    uint32_t base, uint32_t npts, const void *__restrict__ band,
                                                    uint32_t ncols, uint4 *__restrict__ out)
{
    __shared__ uint32_t s_pre[4][64], s_pos[4][64], s_o[4][64];
    const unsigned long long j = (unsigned long long)rlo + blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = lane_id(), wv = threadIdx.x >> 6;
    uint32_t len = 0, pos = 0, o = 0;
    if (j < rhi) {
        const unsigned long long e = rtab[order[j]];
        pos = (uint32_t)e;
        len = (uint32_t)(e >> 32) + 1u;
        o = roff[j] - base;
    }
    uint32_t incl = len;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += t;
    }
    s_pre[wv][lane] = incl - len;
    s_pos[wv][lane] = pos;
    s_o[wv][lane] = o;
    const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    __builtin_amdgcn_wave_barrier();
    for (uint32_t t = lane; t < T; t += 64u) {
        uint32_t q = 0;                         // the last run whose prefix is <= t
#pragma unroll
        for (uint32_t step = 32u; step >= 1u; step >>= 1)
            if (q + step < 64u && s_pre[wv][q + step] <= t) q += step;
        const uint32_t k = t - s_pre[wv][q];
        const uint32_t p = s_pos[wv][q] + k, r = s_o[wv][q] + k;
        if (r < npts) {
            const uint32_t y = p / ncols;
            const long long v = ld_t<DT>(band, p);
            out[r] = make_uint4(p - y * ncols, y, (uint32_t)(unsigned long long)v,
                                (uint32_t)((unsigned long long)v >> 32));
        }
    }
}

static inline PtsGeom pts_geom(const uint32_t *d_seg, const void *d_band, int dtype, uint32_t nrows, uint32_t ncols,
                               uint32_t S, int64_t null_val, uint32_t tile_size)
{
    const uint32_t th = tile_size < nrows ? tile_size : nrows;
    return PtsGeom{d_seg, d_band, dtype, nrows, ncols, S, th, tile_size < ncols ? tile_size : ncols,
                   (long long)null_val, th};
}

// rows [row0, row0 + nrows) of an img_rows-row raster: the bands stay those of the whole raster
static inline PtsGeom pts_geom_slice(const uint32_t *d_seg, const void *d_band, int dtype, uint32_t row0,
                                     uint32_t nrows, uint32_t img_rows, uint32_t ncols, uint32_t S, int64_t null_val,
                                     uint32_t tile_size)
{
    PtsGeom g = pts_geom(d_seg, d_band, dtype, img_rows, ncols, S, null_val, tile_size);
    g.nrows = nrows;
    const uint32_t left = g.th ? g.th - row0 % g.th : 0u;     // rows of row0's band from row0 on
    g.h0 = left < nrows ? left : nrows;
    return g;
}

// counts_out (host, S + 1 entries): valid points per id (k_spatial_sums without the coordinate sums)
static int run_segpoints_count(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, uint32_t nrows,
                               uint32_t ncols, uint32_t S, int64_t null_val, uint32_t *counts_out)
{
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    const uint32_t n = nrows * ncols;
    CHK(buf_ensure(ctx, ctx->segsz, ns * 4));
    uint32_t *cnt = bp<uint32_t>(ctx->segsz);
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, ns * 4, st));
    SpatialGeom g{d_seg, d_band, dtype, nrows, ncols, S, (long long)null_val};
    if (n) hipLaunchKernelGGL(k_spatial_sums, dim3(grid_for(n, 256)), dim3(256), 0, st, g, cnt,
                              (unsigned long long *)nullptr, (unsigned long long *)nullptr);
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(counts_out, cnt, ns * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// The sorted runs of the whole raster, left in the context for run_segpoints_emit: run table in ctx->pts_runs,
// sorted run order in ctx->pix, sorted ids in sort_k0 / sort_k1, first point of every sorted run in ctx->sort_v1,
// per-id first points (S + 2) in ctx->pts_off.  The band stays where the caller keeps it (emit reads it).
// run_segpoints_build_geom: the same for the rows of any geometry (a slice: pts_geom_slice; the points' runs then
// come in the whole raster's visit order restricted to the slice).
static int run_segpoints_build_geom(shp_ctx *ctx, const PtsGeom &g, int64_t null_val, int64_t *npts_out)
{
    hipStream_t st = ctx->stream;
    const uint32_t *d_seg = g.seg;
    const void *d_band = g.band;
    const int dtype = g.dtype;
    const uint32_t nrows = g.nrows, ncols = g.ncols, S = g.S;
    const uint32_t n = nrows * ncols;
    const size_t ns = (size_t)S + 1;
    SegPointsState &ps = ctx->pts;
    ps = SegPointsState{};
    // per-id counts and their scan: where every id's points start
    CHK(buf_ensure(ctx, ctx->segsz, ns * 4));
    CHK(buf_ensure(ctx, ctx->pts_off, (ns + 1) * 4));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(ns + 1 > n ? ns + 1 : n)));
    uint32_t *cnt = bp<uint32_t>(ctx->segsz), *poff = bp<uint32_t>(ctx->pts_off);
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, ns * 4, st));
    SpatialGeom sg{d_seg, d_band, dtype, nrows, ncols, S, (long long)null_val};
    if (n) hipLaunchKernelGGL(k_spatial_sums, dim3(grid_for(n, 256)), dim3(256), 0, st, sg, cnt,
                              (unsigned long long *)nullptr, (unsigned long long *)nullptr);
    KCHK(ctx);
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_PTS;       // [0] runs, [1] points by id, [2] points by run
    ArrFn cf{cnt};
    CHK(scan_exclusive(ctx, cf, (uint32_t)ns, poff, poff + ns, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 1));
    // the runs in visit order
    const uint32_t nblk = (n + PTS_TILE - 1) / PTS_TILE;
    uint32_t m = 0;
    if (n) {
        CHK(buf_ensure(ctx, ctx->sort_hist, ((size_t)2 * nblk + 16) * 4));
        uint32_t *bcount = bp<uint32_t>(ctx->sort_hist), *boff = bcount + nblk, *tot = boff + nblk;
        hipLaunchKernelGGL(k_pts_run_count, dim3(nblk), dim3(256), 0, st, g, n, bcount); KCHK(ctx);
        ArrFn bf{bcount};
        CHK(scan_exclusive(ctx, bf, nblk, boff, tot, bp<uint32_t>(ctx->scan_tmp), nullptr, mir));
        HIPCHK(ctx, hipStreamSynchronize(st));
        m = *(volatile uint32_t *)mir;
        if (m > n) SHP_FAIL(ctx, SHP_ERR_STATE, "run count %u out of range (n = %u)", m, n);
        if (m) {
            CHK(buf_ensure(ctx, ctx->aux, (size_t)m * 4));
            CHK(buf_ensure(ctx, ctx->pts_runs, (size_t)m * 8));
            hipLaunchKernelGGL(k_pts_run_emit, dim3(nblk), dim3(256), 0, st, g, n, boff, bp<uint32_t>(ctx->aux),
                               (unsigned long long *)ctx->pts_runs.p);
            KCHK(ctx);
        }
    } else {
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    const uint32_t npts = *(volatile uint32_t *)(mir + 1);
    uint32_t *skeys = nullptr, *order = nullptr;
    if (m) {
        CHK(sort_pairs(ctx, bp<uint32_t>(ctx->aux), nullptr, m, bits_for(S), &skeys, &order));
        // (the values end in ctx->pix: sort_v1 is free now)
        uint32_t *roff = bp<uint32_t>(ctx->sort_v1);
        PtsLenFn lf{order, (const unsigned long long *)ctx->pts_runs.p};
        CHK(scan_exclusive(ctx, lf, m, roff, nullptr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 2));
        HIPCHK(ctx, hipStreamSynchronize(st));
        const uint32_t byrun = *(volatile uint32_t *)(mir + 2);
        if (byrun != npts) SHP_FAIL(ctx, SHP_ERR_STATE, "runs hold %u points, the per-id counts %u", byrun, npts);
    }
    ps.skeys = skeys;
    ps.order = order;
    ps.roff = bp<uint32_t>(ctx->sort_v1);
    ps.band = d_band;
    ps.dtype = dtype;
    ps.ncols = ncols;
    ps.S = S;
    ps.m = m;
    ps.npts = npts;
    ps.valid = true;
    *npts_out = npts;
    return 0;
}

static int run_segpoints_build(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, uint32_t nrows,
                               uint32_t ncols, uint32_t S, int64_t null_val, uint32_t tile_size, int64_t *npts_out)
{
    return run_segpoints_build_geom(ctx, pts_geom(d_seg, d_band, dtype, nrows, ncols, S, null_val, tile_size),
                                    null_val, npts_out);
}

// ids [lo, hi) of the last build: offs_out (host, hi - lo + 1 int64) and the records (host, at most cap of them)
static int run_segpoints_emit(shp_ctx *ctx, uint32_t lo, uint32_t hi, int64_t *offs_out, void *pts_out,
                              int64_t cap, int64_t *npts_out)
{
    hipStream_t st = ctx->stream;
    const SegPointsState &ps = ctx->pts;
    const size_t nid = (size_t)hi - lo;
    CHK(buf_ensure(ctx, ctx->pts_offs, (nid + 1) * 8 + 64));
    uint32_t *res = bp<uint32_t>(ctx->pts_offs);
    long long *d_offs = (long long *)(res + 16);
    hipLaunchKernelGGL(k_pts_range, dim3(grid_for(nid + 1, 256)), dim3(256), 0, st, ps.skeys, ps.m,
                       bp<uint32_t>(ctx->pts_off), lo, hi, res, d_offs);
    KCHK(ctx);
    uint32_t *pin = ctx->h_pinned + PIN_MIRROR + MIR_PTS + 4;
    HIPCHK(ctx, hipMemcpyAsync(pin, res, 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(offs_out, d_offs, (nid + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t rlo = pin[0], rhi = pin[1], base = pin[2], npts = pin[3];
    if (rlo > rhi || rhi > ps.m) SHP_FAIL(ctx, SHP_ERR_STATE, "run range %u..%u of %u", rlo, rhi, ps.m);
    *npts_out = npts;
    if ((int64_t)npts > cap) SHP_FAIL(ctx, SHP_ERR_ARG, "ids %u..%u hold %u points, the output %lld", lo, hi, npts,
                                      (long long)cap);
    if (npts == 0) return 0;
    CHK(buf_ensure(ctx, ctx->pts_stage, (size_t)npts * 16));
    uint4 *d_out = (uint4 *)ctx->pts_stage.p;
    const uint32_t nr = rhi - rlo;
    DISPATCH_DTYPE(ps.dtype,
        hipLaunchKernelGGL(k_pts_expand<DT>, dim3(grid_for(nr, 256)), dim3(256), 0, st, ps.order,
                           (const unsigned long long *)ctx->pts_runs.p, ps.roff, rlo, rhi, base, npts, ps.band,
                           ps.ncols, d_out));
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(pts_out, d_out, (size_t)npts * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}
