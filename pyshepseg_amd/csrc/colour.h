// colour.h -- colour tables from per-segment columns, and the RGBA rendering through the labels.
//
// Replaces the numpy expression of utils.writeColorTableFromRatColumns (utils.py:216-221): two
// numpy.percentile calls (a partition of the whole float64 column each) and a stretch to 0..255.
// numpy's linear percentile needs only the elements of ranks floor((n-1)q) and that rank + 1, so
// the column is not sorted: every double maps to a 64-bit key of the same order, and the four ranks
// (two per percentile) are found together by a most-significant-digit radix selection -- per 8-bit
// digit one read of the column into LDS digit histograms of the prefixes still followed (at most
// four, usually one or two), then one small kernel that steps each rank into its digit's bucket.
// Eight passes of 8 B per row; from the second pass on nearly all rows fail the prefix test and
// touch no histogram.  The interpolation between the two elements is numpy's, on the host.
// The renderer is a gather: 4 B label in, 4 B packed (R, G, B, A) entry gathered, 4 B out.
#pragma once
#include <chrono>
#include "common.h"

#define SEL_RANKS 4
#define SEL_BINS 256u
#define SEL_PASSES 8
enum { COL_F64 = 0, COL_F32 = 1, COL_I64 = 2 };
enum { COL_BAD_NONFINITE = 1u, COL_BAD_WIDE_INT = 2u };

struct SelState {
    unsigned long long prefix[SEL_RANKS];    // the digits found so far of rank r's key (all 64 bits after the last pass)
    unsigned long long rank[SEL_RANKS];      // rank r among the rows whose key starts with prefix[r]
    unsigned long long uprefix[SEL_RANKS];   // the distinct prefixes
    uint32_t slot[SEL_RANKS];                // prefix[r] == uprefix[slot[r]]: its histogram is hist[slot[r]]
    uint32_t nuniq;
    uint32_t bad;                            // COL_BAD_* bits
    uint32_t hist[SEL_RANKS][SEL_BINS];      // zero between passes
    uint32_t nbad[2];                        // row-sharded columns only: the ranks whose share is non-finite / too wide
};
// what the ranks of a row-sharded column sum per pass: the histograms as int64 words of two uint32 lanes (hist is
// 8-byte aligned and no count reaches 2^32), and in the first pass the word of nbad behind them
#define SEL_HIST_WORDS (SEL_RANKS * SEL_BINS / 2u)
static_assert(offsetof(SelState, hist) % 8 == 0 && offsetof(SelState, nbad) == offsetof(SelState, hist) + SEL_HIST_WORDS * 8,
              "SelState: the exchanged block is int64 words");

// float64 -> a key whose unsigned order is the numeric order (-0.0 sorts just below 0.0)
__device__ __forceinline__ unsigned long long sel_key(double v)
{
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
static inline double sel_unkey(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &u, 8);
    return v;
}

// One count into an LDS histogram per lane with `valid`.  The lanes whose bin is the first valid
// lane's are counted with one atomic: in the first passes whole wavefronts fall into one bin (the
// sign and exponent digits of a column of means), and 64 atomics on one LDS word serialise.
// Every lane of the wavefront must call it.
__device__ __forceinline__ void sel_count(uint32_t *hist, uint32_t bin, bool valid)
{
    const unsigned long long m = __ballot(valid);
    if (m == 0ull) return;
    const int leader = __ffsll((long long)m) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)bin, leader);
    const unsigned long long same = __ballot(valid && bin == b0);
    if ((int)lane_id() == leader) atomicAdd(&hist[b0], (uint32_t)__popcll(same));
    else if (valid && bin != b0) atomicAdd(&hist[bin], 1u);
}

// pass p looks at key bits [56 - 8p, 64 - 8p); a workgroup takes 512 consecutive rows per step, a lane two
// of them with one 16-byte load
__global__ __launch_bounds__(256) void k_sel_hist(const double *__restrict__ col, size_t n, int pass, SelState *st)
{
    __shared__ uint32_t h[SEL_RANKS * SEL_BINS];
    for (uint32_t i = threadIdx.x; i < SEL_RANKS * SEL_BINS; i += 256u) h[i] = 0u;
    const uint32_t nu = pass == 0 ? 1u : st->nuniq;
    unsigned long long up[SEL_RANKS];
    for (int u = 0; u < SEL_RANKS; u++) up[u] = pass == 0 ? 0ull : st->uprefix[u];
    const int shift = 56 - 8 * pass;
    uint32_t bad = 0u;
    __syncthreads();
    for (size_t base = (size_t)blockIdx.x * 512u; base < n; base += (size_t)gridDim.x * 512u) {
        const size_t i0 = base + 2u * threadIdx.x;
        double v[2] = {0.0, 0.0};
        if (i0 + 1 < n) {
            const double2 w = *reinterpret_cast<const double2 *>(col + i0);
            v[0] = w.x; v[1] = w.y;
        } else if (i0 < n) {
            v[0] = col[i0];
        }
#pragma unroll
        for (int e = 0; e < 2; e++) {
            const bool live = i0 + e < n;
            const unsigned long long u = (unsigned long long)__double_as_longlong(v[e]);
            if (pass == 0 && live && (u & 0x7ff0000000000000ull) == 0x7ff0000000000000ull) bad = COL_BAD_NONFINITE;
            const unsigned long long key = sel_key(v[e]);
            const unsigned long long hi = pass == 0 ? 0ull : key >> (shift + 8);
            uint32_t s = SEL_RANKS;
#pragma unroll
            for (uint32_t q = 0; q < SEL_RANKS; q++)
                if (q < nu && hi == up[q]) s = q;
            const bool hit = live && s < SEL_RANKS;
            sel_count(h, (hit ? s : 0u) * SEL_BINS + (uint32_t)((key >> shift) & 0xffull), hit);
        }
    }
    if (bad) atomicOr(&st->bad, bad);
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < nu * SEL_BINS; i += 256u)
        if (h[i]) atomicAdd(&st->hist[0][0] + i, h[i]);
}

// one workgroup: every rank steps into the digit whose bucket holds it; the histograms are zeroed for the next pass
__global__ __launch_bounds__(256) void k_sel_pick(SelState *st, int pass)
{
    if (threadIdx.x == 0) {
        for (int r = 0; r < SEL_RANKS; r++) {
            const uint32_t *h = st->hist[pass == 0 ? 0u : st->slot[r]];
            const unsigned long long rank = st->rank[r];
            unsigned long long cum = 0ull;
            uint32_t d = 0u;
            // (the last digit is taken when the counts fall short of the rank: they cannot, the ranks are below n)
            for (; d + 1u < SEL_BINS; d++) {
                if (rank < cum + h[d]) break;
                cum += h[d];
            }
            st->prefix[r] = (pass == 0 ? 0ull : st->prefix[r] << 8) | d;
            st->rank[r] = rank - cum;
        }
        uint32_t nu = 0u;
        for (int r = 0; r < SEL_RANKS; r++) {
            int q = 0;
            while (q < r && st->prefix[q] != st->prefix[r]) q++;
            if (q < r) { st->slot[r] = st->slot[q]; continue; }
            st->slot[r] = nu;
            st->uprefix[nu++] = st->prefix[r];
        }
        st->nuniq = nu;
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < SEL_RANKS * SEL_BINS; i += 256u) (&st->hist[0][0])[i] = 0u;
}

// the statistics' other column types as float64 (float32: exact; int64: exact below 2^53, anything wider is flagged)
__global__ __launch_bounds__(256) void k_col_from_f32(const float *__restrict__ in, size_t n, double *__restrict__ out)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) out[i] = (double)in[i];
}
__global__ __launch_bounds__(256) void k_col_from_i64(const long long *__restrict__ in, size_t n, double *__restrict__ out,
                                                      SelState *st)
{
    uint32_t bad = 0u;
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u) {
        const long long v = in[i];
        if (v >= (1ll << 53) || v <= -(1ll << 53)) bad = COL_BAD_WIDE_INT;
        out[i] = (double)v;
    }
    if (bad) atomicOr(&st->bad, bad);
}

// utils.py:218 and :221 in float64, in that order: 255 * clip((v - lo) / (hi - lo), 0, 1), truncated to uint8.
// hi == lo divides by zero there: +inf clips to 1, -inf to 0, and the NaN of v == lo becomes 0 in numpy's cast on
// x86-64; `!(t > 0)` gives all three without producing a NaN here.
__device__ __forceinline__ uint32_t stretch_byte(double v, double lo, double hi)
{
    double t = (v - lo) / (hi - lo);
    t = !(t > 0.0) ? 0.0 : (t > 1.0 ? 1.0 : t);
    return (uint32_t)(255.0 * t);
}
// a lane takes four rows: two 16-byte loads, one 4-byte store (out is 4-byte aligned)
__global__ __launch_bounds__(256) void k_colour_stretch(const double *__restrict__ col, size_t n, double lo, double hi,
                                                        uint8_t *__restrict__ out)
{
    for (size_t i = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u; i < n; i += (size_t)gridDim.x * 1024u) {
        if (i + 3 < n) {
            const double2 a = *reinterpret_cast<const double2 *>(col + i);
            const double2 b = *reinterpret_cast<const double2 *>(col + i + 2);
            *reinterpret_cast<uint32_t *>(out + i) = stretch_byte(a.x, lo, hi) | stretch_byte(a.y, lo, hi) << 8 |
                                                     stretch_byte(b.x, lo, hi) << 16 | stretch_byte(b.y, lo, hi) << 24;
        } else {
            for (size_t j = i; j < n; j++) out[j] = (uint8_t)stretch_byte(col[j], lo, hi);
        }
    }
}

// four byte columns (each 4-byte aligned) -> one little-endian (R, G, B, A) word per row
__global__ __launch_bounds__(256) void k_colour_pack(const uint8_t *__restrict__ r, const uint8_t *__restrict__ g,
                                                     const uint8_t *__restrict__ b, const uint8_t *__restrict__ a,
                                                     size_t n, uint32_t *__restrict__ table)
{
    for (size_t i = ((size_t)blockIdx.x * 256u + threadIdx.x) * 4u; i < n; i += (size_t)gridDim.x * 1024u) {
        if (i + 3 < n) {
            const uint32_t wr = *reinterpret_cast<const uint32_t *>(r + i), wg = *reinterpret_cast<const uint32_t *>(g + i);
            const uint32_t wb = *reinterpret_cast<const uint32_t *>(b + i), wa = *reinterpret_cast<const uint32_t *>(a + i);
            for (uint32_t k = 0; k < 4u; k++)
                table[i + k] = ((wr >> (8u * k)) & 0xffu) | ((wg >> (8u * k)) & 0xffu) << 8 |
                               ((wb >> (8u * k)) & 0xffu) << 16 | ((wa >> (8u * k)) & 0xffu) << 24;
        } else {
            for (size_t j = i; j < n; j++)
                table[j] = (uint32_t)r[j] | (uint32_t)g[j] << 8 | (uint32_t)b[j] << 16 | (uint32_t)a[j] << 24;
        }
    }
}

// out[p] = table[seg[p]].  The labels before the first 16-byte boundary of seg and behind the last whole group of
// four go one by one (`head` of them in front); a lane takes four labels in between with one 16-byte load and
// stores its four entries with one 16-byte store where out + head is aligned as well (vec_out), else one by one.
// A label that is not below nrows is not looked up: bad[0] is set and bad[1] keeps the smallest such label.
__device__ __forceinline__ uint32_t colour_of(const uint32_t *__restrict__ table, uint32_t nrows, uint32_t s, uint32_t *bad)
{
    if (s < nrows) return table[s];
    bad[0] = 1u;
    atomicMin(&bad[1], s);
    return 0u;
}
__global__ __launch_bounds__(256) void k_colour_lookup(const uint32_t *__restrict__ seg, size_t n, size_t head, int vec_out,
                                                       const uint32_t *__restrict__ table, uint32_t nrows,
                                                       uint32_t *__restrict__ out, uint32_t *bad)
{
    const size_t ngroups = (n - head) / 4u, tail = head + ngroups * 4u;
    const size_t t0 = (size_t)blockIdx.x * 256u + threadIdx.x, step = (size_t)gridDim.x * 256u;
    for (size_t q = t0; q < ngroups; q += step) {
        const size_t i = head + q * 4u;
        const uint4 s = *reinterpret_cast<const uint4 *>(seg + i);
        uint4 c;
        c.x = colour_of(table, nrows, s.x, bad);
        c.y = colour_of(table, nrows, s.y, bad);
        c.z = colour_of(table, nrows, s.z, bad);
        c.w = colour_of(table, nrows, s.w, bad);
        if (vec_out) {
            *reinterpret_cast<uint4 *>(out + i) = c;
        } else {
            out[i] = c.x; out[i + 1] = c.y; out[i + 2] = c.z; out[i + 3] = c.w;
        }
    }
    // (head < 4 and n - tail < 4)
    if (t0 < head) out[t0] = colour_of(table, nrows, seg[t0], bad);
    if (t0 < n - tail) out[tail + t0] = colour_of(table, nrows, seg[tail + t0], bad);
}

// the COL_BAD_* bits of this rank's share as counts of ranks, one uint32 lane each, so that the sum over the ranks
// keeps them apart (one thread)
__global__ void k_sel_bad_lanes(SelState *st)
{
    st->nbad[0] = (st->bad & COL_BAD_NONFINITE) ? 1u : 0u;
    st->nbad[1] = (st->bad & COL_BAD_WIDE_INT) ? 1u : 0u;
}

// k_overview_rects (stitch.h) with the table lookup fused in: packed[i] = table[label sampled for packed pixel i].
// The rectangle table is the label layers' (checked on the host against the raster); a label without a row is
// handled as in k_colour_lookup.
__global__ __launch_bounds__(256) void k_colour_overview_rects(const uint32_t *__restrict__ ras,
                                                               const int64_t *__restrict__ rects, uint32_t nrects,
                                                               uint64_t npacked, const uint32_t *__restrict__ table,
                                                               uint32_t nrows, uint32_t *__restrict__ packed, uint32_t *bad)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= npacked) return;
    uint32_t lo = 0u, hi = nrects;                  // rects[lo].dst0 <= i < rects[hi].dst0 (npacked for nrects)
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) / 2u;
        if ((uint64_t)rects[6 * (size_t)mid + 5] <= i) lo = mid; else hi = mid;
    }
    const int64_t *q = rects + 6 * (size_t)lo;
    const uint64_t k = i - (uint64_t)q[5];
    const uint64_t r = k / (uint64_t)q[4], c = k - r * (uint64_t)q[4];
    packed[i] = colour_of(table, nrows, ras[(uint64_t)q[0] + r * (uint64_t)q[1] + c * (uint64_t)q[2]], bad);
}

// numpy.percentile(col, q), method 'linear' (numpy >= 1.22: _quantile and _lerp of numpy/lib/function_base.py), from
// the elements a and b of ranks floor((n-1)q/100) and that + 1 of the sorted column
static inline void percentile_ranks(size_t n, double q, size_t *prev, size_t *next, double *gamma)
{
    const double vidx = (double)(n - 1) * (q / 100.0);
    const double f = (double)(size_t)vidx;          // floor: vidx >= 0
    *gamma = vidx - f;
    *prev = (size_t)f;
    *next = *prev + 1 < n ? *prev + 1 : n - 1;
    if (*prev > n - 1) *prev = n - 1;
}
static inline double percentile_lerp(double a, double b, double g)
{
    const double d = b - a;
    return g >= 0.5 ? b - d * (1.0 - g) : a + d * g;
}

static inline unsigned colour_grid(size_t n, unsigned per_block)
{
    return grid_for(n, per_block, 2048u);       // 8 workgroups per CU; the kernels stride over the rest
}

// host column (n rows of ctype) -> out (host, n bytes) and stretch_out = (lo, hi); dev_ms_out: the device time between
// the end of the upload and the start of the download
static int run_colour_stretch(shp_ctx *ctx, const void *col, int ctype, size_t n, uint8_t *out, double *stretch_out,
                              double *dev_ms_out)
{
    hipStream_t st = ctx->stream;
    CHK(buf_ensure(ctx, ctx->pix, n * 8));
    CHK(buf_ensure(ctx, ctx->clus, n + 16));
    CHK(buf_ensure(ctx, ctx->small, sizeof(SelState)));
    double *d_col = bp<double>(ctx->pix);
    uint8_t *d_out = bp<uint8_t>(ctx->clus);
    SelState *d_st = bp<SelState>(ctx->small);
    size_t prev[2], next[2];
    double gamma[2];
    percentile_ranks(n, 5.0, &prev[0], &next[0], &gamma[0]);
    percentile_ranks(n, 95.0, &prev[1], &next[1], &gamma[1]);
    unsigned long long *h_rank = (unsigned long long *)ctx->h_pinned;
    h_rank[0] = prev[0]; h_rank[1] = next[0]; h_rank[2] = prev[1]; h_rank[3] = next[1];
    HIPCHK(ctx, hipMemsetAsync(d_st, 0, sizeof(SelState), st));
    HIPCHK(ctx, hipMemcpyAsync(d_st->rank, h_rank, sizeof(d_st->rank), hipMemcpyHostToDevice, st));
    const void *d_raw = nullptr;
    if (ctype == COL_F64) {
        HIPCHK(ctx, hipMemcpyAsync(d_col, col, n * 8, hipMemcpyHostToDevice, st));
    } else {
        const size_t bytes = n * (ctype == COL_F32 ? 4 : 8);
        CHK(buf_ensure(ctx, ctx->img, bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->img.p, col, bytes, hipMemcpyHostToDevice, st));
        d_raw = ctx->img.p;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (ctype == COL_F32) {
        hipLaunchKernelGGL(k_col_from_f32, dim3(colour_grid(n, 256)), dim3(256), 0, st, (const float *)d_raw, n, d_col);
        KCHK(ctx);
    } else if (ctype == COL_I64) {
        hipLaunchKernelGGL(k_col_from_i64, dim3(colour_grid(n, 256)), dim3(256), 0, st, (const long long *)d_raw, n, d_col,
                           d_st);
        KCHK(ctx);
    }
    for (int pass = 0; pass < SEL_PASSES; pass++) {
        hipLaunchKernelGGL(k_sel_hist, dim3(colour_grid(n, 512)), dim3(256), 0, st, d_col, n, pass, d_st); KCHK(ctx);
        hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(256), 0, st, d_st, pass); KCHK(ctx);
    }
    // (the ranks have been uploaded by now: the staging block is free again)
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, d_st, offsetof(SelState, hist), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const SelState *h_st = (const SelState *)ctx->h_pinned;
    if (h_st->bad & COL_BAD_WIDE_INT)
        SHP_FAIL(ctx, SHP_ERR_ARG, "integer column holds a magnitude of 2^53 or more: not exact in float64");
    if (h_st->bad & COL_BAD_NONFINITE) SHP_FAIL(ctx, SHP_ERR_ARG, "column holds a NaN or an infinity");
    double e[SEL_RANKS];
    for (int r = 0; r < SEL_RANKS; r++) e[r] = sel_unkey(h_st->prefix[r]);
    const double lo = percentile_lerp(e[0], e[1], gamma[0]), hi = percentile_lerp(e[2], e[3], gamma[1]);
    hipLaunchKernelGGL(k_colour_stretch, dim3(colour_grid(n, 1024)), dim3(256), 0, st, d_col, n, lo, hi, d_out); KCHK(ctx);
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(out, d_out, n, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    stretch_out[0] = lo;
    stretch_out[1] = hi;
    if (dev_ms_out) {
        float ms = 0.f;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
        *dev_ms_out = ms;
    }
    return 0;
}

// four host byte columns of n rows -> d_table (device, n words)
static int run_colour_pack(shp_ctx *ctx, const uint8_t *const cols[4], size_t n, uint32_t *d_table)
{
    hipStream_t st = ctx->stream;
    const size_t pitch = (n + 15) & ~(size_t)15;
    CHK(buf_ensure(ctx, ctx->clus, 4 * pitch));
    uint8_t *d = bp<uint8_t>(ctx->clus);
    for (int k = 0; k < 4; k++) HIPCHK(ctx, hipMemcpyAsync(d + k * pitch, cols[k], n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_colour_pack, dim3(colour_grid(n, 1024)), dim3(256), 0, st, d, d + pitch, d + 2 * pitch,
                       d + 3 * pitch, n, d_table);
    KCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

static int run_colour_lookup(shp_ctx *ctx, const uint32_t *d_seg, size_t n, const uint32_t *d_table, uint32_t nrows,
                             uint32_t *d_out)
{
    hipStream_t st = ctx->stream;
    if (n == 0) return 0;
    CHK(buf_ensure(ctx, ctx->small, sizeof(SelState)));
    uint32_t *bad = bp<uint32_t>(ctx->small);
    ctx->h_pinned[0] = 0u;
    ctx->h_pinned[1] = 0xffffffffu;
    HIPCHK(ctx, hipMemcpyAsync(bad, ctx->h_pinned, 8, hipMemcpyHostToDevice, st));
    size_t head = ((16u - ((uintptr_t)d_seg & 15u)) & 15u) / 4u;
    if (head > n) head = n;
    const int vec_out = ((uintptr_t)(d_out + head) & 15u) == 0;
    hipLaunchKernelGGL(k_colour_lookup, dim3(colour_grid((n - head) / 4u + 1u, 256)), dim3(256), 0, st, d_seg, n, head,
                       vec_out, d_table, nrows, d_out, bad);
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, bad, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (ctx->h_pinned[0])
        SHP_FAIL(ctx, SHP_ERR_ARG, "segment id %u is not in the colour table (%u rows)", ctx->h_pinned[1], nrows);
    return 0;
}

// ---- a column shared by rows over the ranks ---------------------------------------------------------------------
// run_colour_stretch in steps the host puts a collective between: every rank holds m rows of a column of n, the
// ranks are those of the whole column, and between a histogram pass and its pick the ranks sum the block at
// *d_block_out (SEL_HIST_WORDS int64 words, one more in pass 0: nbad), after which every rank picks alike.
// Every step is synchronous (the collective runs on another stream) and adds its device time to dcol.dev_ms.
static int dcolour_timed_end(shp_ctx *ctx)
{
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    float ms = 0.f;
    HIPCHK(ctx, hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
    ctx->dcol.dev_ms += ms;
    return 0;
}

static int run_dcolour_begin(shp_ctx *ctx, const void *col, int ctype, size_t m, size_t n, void **d_block_out)
{
    hipStream_t st = ctx->stream;
    ctx->dcol = DColourState();
    CHK(buf_ensure(ctx, ctx->pix, m * 8));
    CHK(buf_ensure(ctx, ctx->small, sizeof(SelState)));
    double *d_col = bp<double>(ctx->pix);
    SelState *d_st = bp<SelState>(ctx->small);
    size_t prev[2], next[2];
    percentile_ranks(n, 5.0, &prev[0], &next[0], &ctx->dcol.gamma[0]);
    percentile_ranks(n, 95.0, &prev[1], &next[1], &ctx->dcol.gamma[1]);
    unsigned long long *h_rank = (unsigned long long *)ctx->h_pinned;
    h_rank[0] = prev[0]; h_rank[1] = next[0]; h_rank[2] = prev[1]; h_rank[3] = next[1];
    HIPCHK(ctx, hipMemsetAsync(d_st, 0, sizeof(SelState), st));
    HIPCHK(ctx, hipMemcpyAsync(d_st->rank, h_rank, sizeof(d_st->rank), hipMemcpyHostToDevice, st));
    const void *d_raw = nullptr;
    if (m && ctype == COL_F64) {
        HIPCHK(ctx, hipMemcpyAsync(d_col, col, m * 8, hipMemcpyHostToDevice, st));
    } else if (m) {
        const size_t bytes = m * (ctype == COL_F32 ? 4 : 8);
        CHK(buf_ensure(ctx, ctx->img, bytes));
        HIPCHK(ctx, hipMemcpyAsync(ctx->img.p, col, bytes, hipMemcpyHostToDevice, st));
        d_raw = ctx->img.p;
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    if (m && ctype == COL_F32) {
        hipLaunchKernelGGL(k_col_from_f32, dim3(colour_grid(m, 256)), dim3(256), 0, st, (const float *)d_raw, m, d_col);
        KCHK(ctx);
    } else if (m && ctype == COL_I64) {
        hipLaunchKernelGGL(k_col_from_i64, dim3(colour_grid(m, 256)), dim3(256), 0, st, (const long long *)d_raw, m, d_col,
                           d_st);
        KCHK(ctx);
    }
    CHK(dcolour_timed_end(ctx));
    ctx->dcol.stage = 1;
    ctx->dcol.m = m;
    ctx->dcol.n = n;
    *d_block_out = &d_st->hist[0][0];
    return 0;
}

static int run_dcolour_hist(shp_ctx *ctx, int pass)
{
    hipStream_t st = ctx->stream;
    DColourState &dc = ctx->dcol;
    if (dc.stage != 1 || !dc.picked || pass != dc.pass) SHP_FAIL(ctx, SHP_ERR_ARG, "histogram pass %d is out of turn", pass);
    SelState *d_st = bp<SelState>(ctx->small);
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    hipLaunchKernelGGL(k_sel_hist, dim3(colour_grid(dc.m, 512)), dim3(256), 0, st, bp<double>(ctx->pix), dc.m, pass, d_st);
    KCHK(ctx);
    if (pass == 0) {
        hipLaunchKernelGGL(k_sel_bad_lanes, dim3(1), dim3(1), 0, st, d_st);
        KCHK(ctx);
    }
    CHK(dcolour_timed_end(ctx));
    dc.picked = 0;
    return 0;
}

static int run_dcolour_pick(shp_ctx *ctx, int pass)
{
    DColourState &dc = ctx->dcol;
    if (dc.stage != 1 || dc.picked || pass != dc.pass) SHP_FAIL(ctx, SHP_ERR_ARG, "pick of pass %d is out of turn", pass);
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_sel_pick, dim3(1), dim3(256), 0, ctx->stream, bp<SelState>(ctx->small), pass);
    KCHK(ctx);
    CHK(dcolour_timed_end(ctx));
    dc.picked = 1;
    dc.pass = pass + 1;
    return 0;
}

// stretch_out = (lo, hi), the same on every rank; *bad_out = COL_BAD_* bits of ANY rank's share (then lo and hi mean nothing)
static int run_dcolour_finish(shp_ctx *ctx, double *stretch_out, int *bad_out)
{
    hipStream_t st = ctx->stream;
    DColourState &dc = ctx->dcol;
    if (dc.stage != 1 || !dc.picked || dc.pass != SEL_PASSES) SHP_FAIL(ctx, SHP_ERR_ARG, "the selection is not finished");
    SelState *d_st = bp<SelState>(ctx->small);
    const size_t head = offsetof(SelState, hist);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, d_st, head, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync((char *)ctx->h_pinned + head, d_st->nbad, sizeof(d_st->nbad), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const SelState *h_st = (const SelState *)ctx->h_pinned;
    const uint32_t *nbad = (const uint32_t *)((const char *)ctx->h_pinned + head);
    *bad_out = (nbad[0] ? (int)COL_BAD_NONFINITE : 0) | (nbad[1] ? (int)COL_BAD_WIDE_INT : 0);
    double e[SEL_RANKS];
    for (int r = 0; r < SEL_RANKS; r++) e[r] = sel_unkey(h_st->prefix[r]);
    dc.lo = percentile_lerp(e[0], e[1], dc.gamma[0]);
    dc.hi = percentile_lerp(e[2], e[3], dc.gamma[1]);
    stretch_out[0] = dc.lo;
    stretch_out[1] = dc.hi;
    dc.stage = *bad_out ? 0 : 2;
    return 0;
}

// the share's bytes -> d_out (device, 4-byte aligned, m bytes); *dev_ms_out: the device time of all steps of the column
static int run_dcolour_stretch(shp_ctx *ctx, uint8_t *d_out, double *dev_ms_out)
{
    DColourState &dc = ctx->dcol;
    if (dc.stage != 2) SHP_FAIL(ctx, SHP_ERR_ARG, "no finished selection to stretch by");
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_colour_stretch, dim3(colour_grid(dc.m, 1024)), dim3(256), 0, ctx->stream, bp<double>(ctx->pix),
                       dc.m, dc.lo, dc.hi, d_out);
    KCHK(ctx);
    CHK(dcolour_timed_end(ctx));
    if (dev_ms_out) *dev_ms_out = dc.dev_ms;
    dc.stage = 0;
    return 0;
}

// run_colour_pack from byte columns that are on the device already (each 4-byte aligned)
static int run_colour_pack_dev(shp_ctx *ctx, const uint8_t *const d_cols[4], size_t n, uint32_t *d_table)
{
    hipLaunchKernelGGL(k_colour_pack, dim3(colour_grid(n, 1024)), dim3(256), 0, ctx->stream, d_cols[0], d_cols[1], d_cols[2],
                       d_cols[3], n, d_table);
    KCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- the rows of a rank, painted and brought to the host ------------------------------------------------------------
// n labels at d_seg -> h_dst (pinned, n words) in blocks of `block` labels: block i is looked up on the context's
// stream into one of two device buffers and downloaded on the side stream, while block i + 1 is looked up into the
// other.  A buffer is written again only after the host has seen its download end (events 4-7 of the context), which
// is also when that block's lookup and download times are read.  bad_out[2]: k_colour_lookup's (flag, smallest label
// without a row) -- reported, not raised: the caller's ranks compare theirs.  ms_out[3]: the sum of the lookups'
// device times, of the downloads', and the wall time of the whole call.
static int run_colour_render_rows(shp_ctx *ctx, const uint32_t *d_seg, size_t n, size_t block, const uint32_t *d_table,
                                  uint32_t nrows, uint32_t *h_dst, uint32_t *bad_out, double *ms_out)
{
    hipStream_t st = ctx->stream;
    bad_out[0] = 0u;
    bad_out[1] = 0xffffffffu;
    ms_out[0] = ms_out[1] = ms_out[2] = 0.0;
    if (n == 0) return 0;
    if (block > n) block = n;
    CHK(ensure_stream2(ctx));
    hipStream_t cp = ctx->stream2;
    CHK(buf_ensure(ctx, ctx->small, sizeof(SelState)));
    CHK(buf_ensure(ctx, ctx->aux, block * 4 + 16));
    CHK(buf_ensure(ctx, ctx->aux2, block * 4 + 16));
    uint32_t *dbuf[2] = {bp<uint32_t>(ctx->aux), bp<uint32_t>(ctx->aux2)};
    uint32_t *bad = bp<uint32_t>(ctx->small);
    hipEvent_t *ev = ctx->ev;           // [b] lookup begins, [2 + b] lookup ends, [4 + b] download begins, [6 + b] download ends
    ctx->h_pinned[0] = 0u;
    ctx->h_pinned[1] = 0xffffffffu;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(ctx, hipMemcpyAsync(bad, ctx->h_pinned, 8, hipMemcpyHostToDevice, st));
    const size_t nblocks = (n + block - 1) / block;
    auto account = [&](int b) -> int {
        float ms = 0.f;
        HIPCHK(ctx, hipEventSynchronize(ev[6 + b]));
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev[b], ev[2 + b]));
        ms_out[0] += ms;
        HIPCHK(ctx, hipEventElapsedTime(&ms, ev[4 + b], ev[6 + b]));
        ms_out[1] += ms;
        return 0;
    };
    for (size_t i = 0; i < nblocks; i++) {
        const int b = (int)(i & 1u);
        const size_t p0 = i * block, np = n - p0 < block ? n - p0 : block;
        if (i >= 2) CHK(account(b));            // (block i - 2 has left this buffer)
        const uint32_t *seg = d_seg + p0;
        // (the output starts at the labels' offset from a 16-byte boundary: the kernel then stores whole vectors)
        uint32_t *out = dbuf[b] + ((uintptr_t)seg & 15u) / 4u;
        size_t head = ((16u - ((uintptr_t)seg & 15u)) & 15u) / 4u;
        if (head > np) head = np;
        const int vec_out = ((uintptr_t)(out + head) & 15u) == 0;
        HIPCHK(ctx, hipEventRecord(ev[b], st));
        hipLaunchKernelGGL(k_colour_lookup, dim3(colour_grid((np - head) / 4u + 1u, 256)), dim3(256), 0, st, seg, np, head,
                           vec_out, d_table, nrows, out, bad);
        KCHK(ctx);
        HIPCHK(ctx, hipEventRecord(ev[2 + b], st));
        HIPCHK(ctx, hipStreamWaitEvent(cp, ev[2 + b], 0));
        HIPCHK(ctx, hipEventRecord(ev[4 + b], cp));
        HIPCHK(ctx, hipMemcpyAsync(h_dst + p0, out, np * 4, hipMemcpyDeviceToHost, cp));
        HIPCHK(ctx, hipEventRecord(ev[6 + b], cp));
    }
    if (nblocks >= 2) CHK(account((int)(nblocks & 1u)));
    CHK(account((int)((nblocks - 1) & 1u)));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, bad, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipStreamSynchronize(cp));
    ms_out[2] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    bad_out[0] = ctx->h_pinned[0];
    bad_out[1] = ctx->h_pinned[1];
    return 0;
}

// the colours of the overview rectangles of a row-sharded raster (the table of shp_overview_rects_dev, checked by the
// caller as there) -> d_packed; bad_out as in run_colour_render_rows
static int run_colour_overview_rects(shp_ctx *ctx, const uint32_t *d_raster, const int64_t *rects, int nrects,
                                     const uint32_t *d_table, uint32_t nrows, uint32_t *d_packed, size_t npacked,
                                     uint32_t *bad_out)
{
    hipStream_t st = ctx->stream;
    CHK(buf_ensure(ctx, ctx->small, sizeof(SelState)));
    CHK(buf_ensure(ctx, ctx->tlist, (size_t)nrects * 48));
    uint32_t *bad = bp<uint32_t>(ctx->small);
    ctx->h_pinned[0] = 0u;
    ctx->h_pinned[1] = 0xffffffffu;
    HIPCHK(ctx, hipMemcpyAsync(bad, ctx->h_pinned, 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->tlist.p, rects, (size_t)nrects * 48, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_colour_overview_rects, dim3(grid_for(npacked, 256)), dim3(256), 0, st, d_raster,
                       bp<int64_t>(ctx->tlist), (uint32_t)nrects, (uint64_t)npacked, d_table, nrows, d_packed, bad);
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, bad, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    bad_out[0] = ctx->h_pinned[0];
    bad_out[1] = ctx->h_pinned[1];
    return 0;
}
