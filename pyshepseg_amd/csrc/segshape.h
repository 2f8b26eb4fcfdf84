// segshape.h -- what shape every segment has: area, extent, perimeter and the coordinate moments of the label raster
// (shapes.calcSegmentShapes).  All of it is integer work over the labels alone, so neither the atomics nor the row
// blocks can change a bit of a result.
//
// Per id (label 0 is no segment), with r, c the pixel's coordinates from the caller's origin (row0, col0):
//   area; sum r, sum c, sum r^2, sum c^2, sum r c (modulo 2^64); min and max of r and of c;
//   perimeter: the sides (N, S, W, E) of the id's pixels whose other side is another label, label 0 or outside the
//   raster; outer border: those whose other side is label 0 or outside; edge pixels: pixels with at least one such side.
//
// The labels come in row blocks, top to bottom, each with the row above and the row below it where the raster has
// them: a side belongs to the block of its own pixel and looks at the neighbouring block's row without counting it.
// The two rows are given by pointers of their own (ShapeGeom::rowAbove, rowBelow; null where the raster ends): next to
// the block in memory for the one-GPU calls, in the halo gather's buffer for a rank's rows of a sharded raster
// (dsegshape.h), whose gigabytes of labels are then not copied to stand between their halo rows.
//  1. k_shape_patch: one workgroup per 32 x 64 patch (k_nbr_patch's patches) plus a one-pixel rim on all four sides,
//     a wavefront per image row.  Lanes that hold one label side by side form a run and the run's first lane acts for
//     it (nbr_rows' ballot and count-trailing-zeros idiom): its length is the area, the column sums are closed forms of
//     its first lane and length, and the sides are population counts of the four ballots under the run's lane mask.  A
//     label that fills a patch then costs one LDS update per row, not 64 on one address.
//     Runs go into an LDS table keyed by label (open addressing, home slot shape_hash) of PATCH-RELATIVE 32-bit
//     accumulators, ten words a slot:
//       area | edge pixels << 16 (each at most 2048), perimeter | outer border << 16 (each at most 8192),
//       sum dr (<= 2048 * 31), sum dc (<= 2048 * 63), sum dr^2 (<= 2048 * 31^2), sum dc^2 (<= 2048 * 63^2),
//       sum dr dc (<= 2048 * 31 * 63), the rows met (a bit each) and the columns met (two words): the extent is the
//       lowest and highest bit, taken with one atomic OR each where four byte-wide min / max would need four.
//     At the flush the occupied slots are listed and a group of 16 lanes takes each, a lane per word of the id's row
//     of the device table.  The lanes turn the slot into absolute 64-bit terms, with (R0, C0) the patch's origin:
//     sum r = n R0 + sum dr, sum r^2 = n R0^2 + 2 R0 sum dr + sum dr^2, sum r c = n R0 C0 + R0 sum dc + C0 sum dr +
//     sum dr dc, ... and add them: six 64-bit atomic adds, up to three more for perimeter, outer border and edge
//     pixels where they are not 0, and a 32-bit atomic min / max for each of the four extents.  One set per (patch,
//     label), none per pixel.  A wavefront's atomic instruction then covers 72 contiguous bytes of each of four rows;
//     with a thread per slot (8 bytes of each of 64 rows) the 40000^2 raster of 4 x 8 blocks took 30.6 ms instead of
//     18.7, the 8192^2 segmentation 0.41 either way.
//     LDS: the tile 34 x 66 x 4 = 8976 bytes, the table SHAPE_SLOTS x 44 = 22528 bytes at 512 slots: 31.5 KB a
//     workgroup, five workgroups (20 wavefronts, 5 a SIMD) per CU of 160 KiB.
//     OVERFLOW ROUTE: the table has SHAPE_SLOTS = 512 slots, fewer than a patch has pixels.  An insertion gives up
//     after one trip round the table, which happens if and only if the patch holds more than SHAPE_SLOTS distinct
//     labels (whatever the order of arrival); the patch then leaves the table unused and every run adds its own
//     absolute terms to the device table.  With ~32-pixel segments a patch holds ~100 labels.
//  2. k_shape_finish: the extents of ids without pixels become 0.  Labels above max_seg_id are never looked up: the
//     patch kernel keeps the largest of them in a device word, which shp_shape_finish reports.
//
// Device memory: SHAPE_WORDS x 8 = 88 bytes per id, the rows of one id next to each other so that a flush touches one
// or two cache lines of it.
#pragma once
#include "common.h"

#define SHAPE_PH 32u            // patch rows (8 per wavefront)
#define SHAPE_PW 64u            // patch columns: a wavefront per image row
#ifndef SHAPE_SLOTS
#define SHAPE_SLOTS 512u        // table slots per patch (a power of two): 22 KiB of LDS
#endif
#define SHAPE_TW 66u            // tile columns: the patch and a rim column on either side
#define SHAPE_HW 10             // 32-bit accumulators per slot
#define SHAPE_WORDS 11u         // 64-bit words per id of the device table

static_assert((SHAPE_SLOTS & (SHAPE_SLOTS - 1u)) == 0u && SHAPE_SLOTS >= 64u && SHAPE_SLOTS <= 2048u,
              "SHAPE_SLOTS must be a power of two");

// words of an id's row: six sums, three counts, then (rowMin | rowMax << 32) and (colMin | colMax << 32)
enum { SHAPE_AREA = 0, SHAPE_SR = 1, SHAPE_SC = 2, SHAPE_SRR = 3, SHAPE_SCC = 4, SHAPE_SRC = 5, SHAPE_PERIM = 6,
       SHAPE_OUTER = 7, SHAPE_EDGE = 8, SHAPE_ROWEXT = 9, SHAPE_COLEXT = 10 };

struct ShapeGeom {
    const uint32_t *seg;        // the block's first row
    uint32_t nrows, ncols;      // of the block
    uint32_t pcols;             // patches per patch row
    const uint32_t *rowAbove, *rowBelow;    // the raster's row before the block / after its last row; null: the raster ends
    uint32_t S;                 // the table's last row
    unsigned long long R0, C0;  // coordinates of the block's first pixel
};

__device__ __forceinline__ uint32_t shape_hash(uint32_t label)
{
    return ((label * 0x9E3779B1u) >> 16) & (SHAPE_SLOTS - 1u);
}

// sum of k^2 for k = 0 .. m
__device__ __forceinline__ uint32_t shape_sq_to(uint32_t m) { return m * (m + 1u) * (2u * m + 1u) / 6u; }

// patch-relative terms of one label (of a slot, or of one run) added to its row; (R0, C0): the patch's origin
__device__ __forceinline__ void shape_emit(unsigned long long *__restrict__ tab, unsigned long long R0, unsigned long long C0,
                                           uint32_t label, uint32_t n, uint32_t edge, uint32_t per, uint32_t outer,
                                           uint32_t sdr, uint32_t sdc, uint32_t sdr2, uint32_t sdc2, uint32_t sdrc,
                                           uint32_t rmin, uint32_t rmax, uint32_t cmin, uint32_t cmax)
{
    unsigned long long *row = tab + (size_t)label * SHAPE_WORDS;
    const unsigned long long N = n;
    atomicAdd(row + SHAPE_AREA, N);
    atomicAdd(row + SHAPE_SR, N * R0 + sdr);
    atomicAdd(row + SHAPE_SC, N * C0 + sdc);
    atomicAdd(row + SHAPE_SRR, N * R0 * R0 + 2ull * R0 * sdr + sdr2);
    atomicAdd(row + SHAPE_SCC, N * C0 * C0 + 2ull * C0 * sdc + sdc2);
    atomicAdd(row + SHAPE_SRC, N * R0 * C0 + R0 * sdc + C0 * sdr + sdrc);
    if (per) atomicAdd(row + SHAPE_PERIM, (unsigned long long)per);
    if (outer) atomicAdd(row + SHAPE_OUTER, (unsigned long long)outer);
    if (edge) atomicAdd(row + SHAPE_EDGE, (unsigned long long)edge);
    uint32_t *ext = (uint32_t *)(row + SHAPE_ROWEXT);
    atomicMin(ext + 0, (uint32_t)(R0 + rmin));
    atomicMax(ext + 1, (uint32_t)(R0 + rmax));
    atomicMin(ext + 2, (uint32_t)(C0 + cmin));
    atomicMax(ext + 3, (uint32_t)(C0 + cmax));
}

// The runs of the patch's rows, a wavefront row at a time.  DIRECT = false adds a run to the LDS table (*over is set
// when a label found no slot), DIRECT = true adds it to the device table.
template <bool DIRECT>
__device__ __forceinline__ void shape_rows(const ShapeGeom &g, uint32_t y0, const uint32_t (*tile)[SHAPE_TW], uint32_t *hkey,
                                           uint32_t (*hw)[SHAPE_SLOTS], volatile uint32_t *over,
                                           unsigned long long *__restrict__ tab, unsigned long long R0, unsigned long long C0)
{
    const unsigned w = threadIdx.x >> 6, lane = lane_id();
    for (unsigned rr = 0; rr < SHAPE_PH / 4u; rr++) {
        const unsigned r = w * (SHAPE_PH / 4u) + rr;
        if (y0 + r >= g.nrows) break;                   // (uniform in the wavefront)
        const uint32_t c0 = tile[r + 1u][lane + 1u];
        const uint32_t cn = tile[r][lane + 1u], cs = tile[r + 2u][lane + 1u];
        const uint32_t cw = tile[r + 1u][lane], ce = tile[r + 1u][lane + 2u];
        const bool valid = c0 != 0u && c0 <= g.S;
        const unsigned long long bn = __ballot(valid && cn != c0), bs = __ballot(valid && cs != c0);
        const unsigned long long bw = __ballot(valid && cw != c0), be = __ballot(valid && ce != c0);
        const unsigned long long on = __ballot(valid && cn == 0u), os = __ballot(valid && cs == 0u);
        const unsigned long long ow = __ballot(valid && cw == 0u), oe = __ballot(valid && ce == 0u);
        const uint32_t pc = __shfl_up(c0, 1, 64);
        const bool bd = lane == 0u || c0 != pc;
        const unsigned long long bound = __ballot(bd);
        if (bd && valid) {
            const unsigned long long rest = lane == 63u ? 0ull : (bound >> (lane + 1u));
            const uint32_t len = rest ? (uint32_t)__builtin_ctzll(rest) + 1u : 64u - lane;
            const unsigned long long rm = (len == 64u ? ~0ull : ((1ull << len) - 1ull)) << lane;
            const uint32_t per = (uint32_t)(__popcll(bn & rm) + __popcll(bs & rm) + __popcll(bw & rm) + __popcll(be & rm));
            const uint32_t outer = (uint32_t)(__popcll(on & rm) + __popcll(os & rm) + __popcll(ow & rm) + __popcll(oe & rm));
            const uint32_t edge = (uint32_t)__popcll((bn | bs | bw | be) & rm);
            const uint32_t last = lane + len - 1u;
            const uint32_t sdc = len * lane + len * (len - 1u) / 2u;
            const uint32_t sdc2 = shape_sq_to(last) - (lane ? shape_sq_to(lane - 1u) : 0u);
            if (DIRECT) {
                shape_emit(tab, R0, C0, c0, len, edge, per, outer, len * r, sdc, len * r * r, sdc2, r * sdc, r, r, lane, last);
            } else if (!*over) {
                uint32_t h = shape_hash(c0);
                bool done = false;
                for (uint32_t probe = 0; probe < SHAPE_SLOTS; probe++) {
                    const uint32_t old = atomicCAS(&hkey[h], 0u, c0);
                    if (old == 0u || old == c0) { done = true; break; }
                    h = (h + 1u) & (SHAPE_SLOTS - 1u);
                }
                if (!done) {
                    *over = 1u;
                } else {
                    atomicAdd(&hw[0][h], len | (edge << 16));
                    if (per) atomicAdd(&hw[1][h], per | (outer << 16));
                    if (r) atomicAdd(&hw[2][h], len * r);
                    atomicAdd(&hw[3][h], sdc);
                    if (r) atomicAdd(&hw[4][h], len * r * r);
                    atomicAdd(&hw[5][h], sdc2);
                    if (r) atomicAdd(&hw[6][h], r * sdc);
                    atomicOr(&hw[7][h], 1u << r);
                    if ((uint32_t)rm) atomicOr(&hw[8][h], (uint32_t)rm);
                    if ((uint32_t)(rm >> 32)) atomicOr(&hw[9][h], (uint32_t)(rm >> 32));
                }
            }
        }
    }
}

// ctr[0]: the largest label above g.S met so far
__global__ __launch_bounds__(256) void k_shape_patch(ShapeGeom g, unsigned long long *__restrict__ tab,
                                                     uint32_t *__restrict__ ctr)
{
    __shared__ uint32_t tile[SHAPE_PH + 2u][SHAPE_TW];
    __shared__ uint32_t hkey[SHAPE_SLOTS];
    __shared__ uint32_t hw[SHAPE_HW][SHAPE_SLOTS];
    __shared__ uint32_t s_over, s_nlist;
    const uint32_t py = blockIdx.x / g.pcols, px = blockIdx.x - py * g.pcols;
    const uint32_t y0 = py * SHAPE_PH, x0 = px * SHAPE_PW;
    for (uint32_t i = threadIdx.x; i < SHAPE_SLOTS; i += 256u) {
        hkey[i] = 0u;
#pragma unroll
        for (int k = 0; k < SHAPE_HW; k++) hw[k][i] = 0u;
    }
    if (threadIdx.x == 0) { s_over = 0u; s_nlist = 0u; }
    // the patch and its rim; 0 (no segment) wherever the raster, or what may be read of it, ends
    uint32_t mx = 0u;
    for (uint32_t i = threadIdx.x; i < (SHAPE_PH + 2u) * SHAPE_TW; i += 256u) {
        const uint32_t r = i / SHAPE_TW, c = i - r * SHAPE_TW;
        const long long gy = (long long)y0 + r - 1, gx = (long long)x0 + c - 1;
        uint32_t v = 0u;
        if (gx >= 0 && gx < (long long)g.ncols) {
            if (gy >= 0 && gy < (long long)g.nrows) v = g.seg[gy * (long long)g.ncols + gx];
            else if (gy == -1) v = g.rowAbove ? g.rowAbove[gx] : 0u;
            else if (gy == (long long)g.nrows) v = g.rowBelow ? g.rowBelow[gx] : 0u;
        }
        tile[r][c] = v;
        mx = max(mx, v);
    }
    __syncthreads();
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    // (a label above S is an error of the caller's: look before the atomic, one address for the whole grid)
    if (lane_id() == 0u && mx > g.S && mx > L2LOAD(&ctr[0])) atomicMax(&ctr[0], mx);
    const unsigned long long R0 = g.R0 + y0, C0 = g.C0 + x0;
    shape_rows<false>(g, y0, tile, hkey, hw, &s_over, tab, R0, C0);
    __syncthreads();
    if (s_over == 0u) {
        // a group of 16 lanes per occupied slot, a lane per word of the id's row: a wavefront's atomic instruction
        // then covers 72 contiguous bytes of each of four rows, not 8 bytes of 64
        uint32_t *list = &tile[0][0];               // (the tile has been read)
        for (uint32_t i = threadIdx.x; i < SHAPE_SLOTS; i += 256u)
            if (hkey[i] != 0u) list[atomicAdd(&s_nlist, 1u)] = i;
        __syncthreads();
        const uint32_t nlist = s_nlist, f = threadIdx.x & 15u;
        for (uint32_t q = threadIdx.x >> 4; q < nlist; q += 16u) {
            const uint32_t i = list[q], key = hkey[i];
            const uint32_t w0 = hw[0][i], w1 = hw[1][i], rows = hw[7][i];
            const unsigned long long cols = ((unsigned long long)hw[9][i] << 32) | hw[8][i];
            const unsigned long long N = w0 & 0xffffu, sdr = hw[2][i], sdc = hw[3][i];
            unsigned long long *row = tab + (size_t)key * SHAPE_WORDS;
            if (f < SHAPE_ROWEXT) {
                unsigned long long v;
                switch (f) {
                case SHAPE_AREA: v = N; break;
                case SHAPE_SR: v = N * R0 + sdr; break;
                case SHAPE_SC: v = N * C0 + sdc; break;
                case SHAPE_SRR: v = N * R0 * R0 + 2ull * R0 * sdr + hw[4][i]; break;
                case SHAPE_SCC: v = N * C0 * C0 + 2ull * C0 * sdc + hw[5][i]; break;
                case SHAPE_SRC: v = N * R0 * C0 + R0 * sdc + C0 * sdr + hw[6][i]; break;
                case SHAPE_PERIM: v = w1 & 0xffffu; break;
                case SHAPE_OUTER: v = w1 >> 16; break;
                default: v = w0 >> 16; break;
                }
                if (v) atomicAdd(row + f, v);
            } else if (f < SHAPE_ROWEXT + 4u) {
                uint32_t *ext = (uint32_t *)(row + SHAPE_ROWEXT) + (f - SHAPE_ROWEXT);
                if (f == SHAPE_ROWEXT) atomicMin(ext, (uint32_t)(R0 + (uint32_t)__builtin_ctz(rows)));
                else if (f == SHAPE_ROWEXT + 1u) atomicMax(ext, (uint32_t)(R0 + 31u - (uint32_t)__builtin_clz(rows)));
                else if (f == SHAPE_ROWEXT + 2u) atomicMin(ext, (uint32_t)(C0 + (uint32_t)__builtin_ctzll(cols)));
                else atomicMax(ext, (uint32_t)(C0 + 63u - (uint32_t)__builtin_clzll(cols)));
            }
        }
    } else {
        shape_rows<true>(g, y0, tile, hkey, hw, &s_over, tab, R0, C0);
    }
}

// an empty table: sums and counts 0, minima 2^32 - 1, maxima 0
__global__ __launch_bounds__(256) void k_shape_init(unsigned long long *__restrict__ tab, size_t nwords)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256u)
        tab[i] = i % SHAPE_WORDS >= SHAPE_ROWEXT ? 0xffffffffull : 0ull;
}

__global__ __launch_bounds__(256) void k_shape_finish(unsigned long long *__restrict__ tab, size_t nids)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < nids; i += (size_t)gridDim.x * 256u) {
        unsigned long long *row = tab + i * SHAPE_WORDS;
        if (row[SHAPE_AREA] == 0ull) { row[SHAPE_ROWEXT] = 0ull; row[SHAPE_COLEXT] = 0ull; }
    }
}

// out[0] = max(out[0], the largest of n labels)
__global__ __launch_bounds__(256) void k_shape_label_max(const uint32_t *__restrict__ seg, size_t n, uint32_t *__restrict__ out)
{
    uint32_t mx = 0u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) mx = max(mx, seg[i]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    if (lane_id() == 0u && mx) atomicMax(out, mx);
}

// ---- host side --------------------------------------------------------------------------------------------
static int shape_ms(shp_ctx *ctx)       // device time between ev[0] and ev[1] (the stream is synchronised)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) ctx->shape.dev_ms += ms;
    return 0;
}

static int run_shape_label_max(shp_ctx *ctx, const uint32_t *d_seg, size_t npix, uint32_t *max_out, double *dev_ms_out)
{
    hipStream_t st = ctx->stream;
    CHK(buf_ensure(ctx, ctx->shape_ctr, 16));
    uint32_t *ctr = bp<uint32_t>(ctx->shape_ctr);
    HIPCHK(ctx, hipMemsetAsync(ctr + 2, 0, 4, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (npix) {
        hipLaunchKernelGGL(k_shape_label_max, dim3(grid_for(npix, 256 * 16, 16384u)), dim3(256), 0, st, d_seg, npix, ctr + 2);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr + 2, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    *max_out = *(volatile uint32_t *)ctx->h_pinned;
    if (dev_ms_out) {
        float ms = 0.f;
        *dev_ms_out = hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess ? (double)ms : 0.0;
    }
    return 0;
}

static int run_shape_begin(shp_ctx *ctx, uint32_t S, unsigned long long row0, unsigned long long col0)
{
    ShapeState &s = ctx->shape;
    hipStream_t st = ctx->stream;
    s = ShapeState{};
    const size_t nwords = ((size_t)S + 1) * SHAPE_WORDS;
    CHK(buf_ensure(ctx, ctx->shape_tab, nwords * 8));
    CHK(buf_ensure(ctx, ctx->shape_ctr, 16));
    HIPCHK(ctx, hipMemsetAsync(ctx->shape_ctr.p, 0, 16, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_shape_init, dim3(grid_for(nwords, 256, 16384u)), dim3(256), 0, st,
                       (unsigned long long *)ctx->shape_tab.p, nwords);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    shape_ms(ctx);
    s.S = S;
    s.row0 = row0;
    s.col0 = col0;
    s.stage = 1;
    return 0;
}

// d_seg: the block's first row; d_above / d_below: the raster's row before / after the block, null where it ends
static int run_shape_accumulate(shp_ctx *ctx, const uint32_t *d_seg, uint32_t nrows, uint32_t ncols, const uint32_t *d_above,
                                const uint32_t *d_below)
{
    ShapeState &s = ctx->shape;
    hipStream_t st = ctx->stream;
    if (nrows == 0 || ncols == 0) return 0;
    if (s.row0 + s.rows_done + nrows > (1ull << 32) || s.col0 + ncols > (1ull << 32))
        SHP_FAIL(ctx, SHP_ERR_ARG, "coordinates of 2^32 and more");
    const uint32_t pcols = (ncols + SHAPE_PW - 1u) / SHAPE_PW, prows = (nrows + SHAPE_PH - 1u) / SHAPE_PH;
    if ((unsigned long long)pcols * prows > 0x7fffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "row block too large");
    ShapeGeom g{d_seg, nrows, ncols, pcols, d_above, d_below, s.S, s.row0 + s.rows_done, s.col0};
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_shape_patch, dim3(pcols * prows), dim3(256), 0, st, g, (unsigned long long *)ctx->shape_tab.p,
                       bp<uint32_t>(ctx->shape_ctr));
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    shape_ms(ctx);
    s.rows_done += nrows;
    return 0;
}

// *bad_out: 0, or the largest label above max_seg_id (then there is nothing to download)
static int run_shape_finish(shp_ctx *ctx, uint32_t *S_out, uint32_t *bad_out)
{
    ShapeState &s = ctx->shape;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_shape_finish, dim3(grid_for((size_t)s.S + 1, 256, 16384u)), dim3(256), 0, st,
                       (unsigned long long *)ctx->shape_tab.p, (size_t)s.S + 1);
    KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctx->shape_ctr.p, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    shape_ms(ctx);
    *S_out = s.S;
    *bad_out = *(volatile uint32_t *)ctx->h_pinned;
    s.stage = *bad_out ? 0 : 2;
    return 0;
}

static int run_shape_download(shp_ctx *ctx, uint64_t *rows)
{
    const ShapeState &s = ctx->shape;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(rows, ctx->shape_tab.p, ((size_t)s.S + 1) * SHAPE_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}
