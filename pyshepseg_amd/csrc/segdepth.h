// segdepth.h -- how deep every segment is: the exact squared Euclidean distance from each pixel to the nearest pixel
// that is not of its segment, and per id the deepest pixel, the sum of the depths and the core areas
// (depths.calcSegmentDepths).  All of it is integer work over the labels alone, so neither the atomics nor the tiling
// can change a bit of a result.
//
// A position q is foreign to a pixel p of label L != 0 when q lies outside the raster or label(q) != L (another id and
// label 0 alike).  depth2(p) = min over foreign q of |p - q|^2, and 0 where the label is 0.  The transform separates:
//  1. COLUMN STEP.  g(y, x) = min(y - top + 1, bottom - y + 1) with top .. bottom the vertical run of (y, x)'s label in
//     its column, stored saturated at 65535 in 16 bits: a depth is at most 32768, so a saturated term is never the
//     minimum, and 65535^2 + DEPTH_HALO^2 still fits 32 bits (static_assert below).
//     k_depth_band_sum: a thread per column and band of DEPTH_BAND rows (loads coalesced across the columns) notes the
//     band's first and last label and the lengths of the runs that touch the band's edges.  k_depth_band_carry: a
//     thread per column walks the bands down and up and leaves, per band, how many pixels of the first (last) row's
//     label stand directly above (below) the band.  k_depth_col: a thread per column and band again, the band's labels
//     in registers, one sweep down and one up, one 16-bit store per pixel.  A thread per column over the whole raster
//     would be too few wavefronts on narrow rasters.
//  2. ROW STEP.  With l .. r the horizontal run of (y, x)'s label in its row,
//       depth2(y, x) = min((x - l + 1)^2, (r + 1 - x)^2, min over x' in l .. r of (x - x')^2 + g(y, x')^2),
//     and an x' whose offset squared is not below the best so far cannot win.
//     WINDOW, k_depth_window: a workgroup stages DEPTH_TH rows of DEPTH_TW columns in LDS, labels and g, with
//     DEPTH_HALO columns on either side; a wavefront per row.  A pixel starts from g^2 and scans the offsets d = 1, 2,
//     ... both ways at once: d^2 >= best ends the scan, a foreign label or the raster's edge at offset d makes d^2 the
//     answer.  A pixel that has looked at all DEPTH_HALO offsets without either is deferred: it writes DEPTH_DEFER
//     and is counted.  So a pixel never looks farther than min(depth, DEPTH_HALO), whatever the run's length.
//     ENVELOPE.  A row run that holds a deferred pixel is marked: it goes into the run list and takes its room in the
//     scratch with one atomic add of its length.  Such a run has at least 2 DEPTH_HALO + 1 pixels, so it crosses a
//     multiple of DEPTH_TW columns: k_depth_pieces sums up every piece of DEPTH_TW columns of a row with ballots (its
//     first and last run, whether they hold a deferred pixel, whether the last goes on), and k_depth_long walks a long
//     run a piece a step, not a pixel a step.  With all = 1 (path 'envelope') the window is skipped and every run is
//     marked.  k_depth_envelope: a thread per marked run
//     solves it whole by the lower envelope of the parabolas (x - x')^2 + g(x')^2 (Meijster, Roerdink and Hesselink
//     2000), the two ends of the run being sites of height 0 one pixel outside it: O(run length), in 64-bit
//     integers, the intersection abscissae by floor division of non-negative integers.  Scratch: two 32-bit words per
//     pixel of the marked runs (and their two outer sites), in global memory.
//  3. REDUCTION, k_depth_reduce: k_shape_patch's patches (DEPTH_PH x 64, a wavefront per image row) and an LDS table
//     keyed by label: pixels, the sum of depth2 (64 bits), the 64-bit key (depth2 << 32) | (0xFFFFFFFF - linear index),
//     whose maximum is the deepest pixel and of several the first in row-major order, and up to DEPTH_CORES counts of
//     depth2 > Q.  A wavefront whose 64 pixels hold one label reduces them with shuffles and lane 0 alone updates the
//     slot; otherwise every labelled lane does (runs are then shorter than 64).  The flush is one set of device
//     atomics per (patch, label).  OVERFLOW ROUTE: a patch with more than DEPTH_SLOTS labels leaves the table unused and
//     its pixels (or uniform wavefronts) update the device table directly.
//
// Device memory: 2 (g) + 4 (depth2) bytes a pixel, 20 bytes per column and band (0.625 a pixel), 12 bytes per piece of a
// row (0.19 a pixel), DEPTH_WORDS x 8 = 88 bytes per id, 16 bytes per marked run (room for pixels / (2 DEPTH_HALO + 1) of them, for every pixel with all = 1) and
// 8 bytes per pixel of the marked runs.
#pragma once
#include "common.h"

#define DEPTH_BAND 32u          // rows of a band of the column step
#define DEPTH_HALO 32u          // columns a pixel of the window looks to either side
#define DEPTH_TW 64u            // window tile columns: a wavefront per row
#define DEPTH_TH 16u            // window tile rows (4 per wavefront)
#define DEPTH_PH 32u            // reduction patch rows (8 per wavefront); its columns are DEPTH_TW
#define DEPTH_SLOTS 512u        // table slots per patch (a power of two)
#define DEPTH_CORES 8u          // core areas of one call
#define DEPTH_WORDS 11u         // 64-bit words per id of the device table: pixels, sum, key, DEPTH_CORES counts
#define DEPTH_DEFER 0xFFFFFFFFu // depth2 of a deferred pixel between the window and the envelope
#define DEPTH_GSAT 65535u
#define DEPTH_LW (DEPTH_TW + 2u * DEPTH_HALO)

static_assert((DEPTH_SLOTS & (DEPTH_SLOTS - 1u)) == 0u, "DEPTH_SLOTS must be a power of two");
static_assert((unsigned long long)DEPTH_GSAT * DEPTH_GSAT + (unsigned long long)DEPTH_HALO * DEPTH_HALO < (1ull << 32),
              "a saturated g and a halo offset must fit 32 bits");
static_assert(DEPTH_TW == 64u && DEPTH_TH % 4u == 0u && DEPTH_PH % 4u == 0u, "a wavefront per row, four wavefronts");

enum { DEPTH_AREA = 0, DEPTH_SUM = 1, DEPTH_KEY = 2, DEPTH_CORE0 = 3 };
enum { DEPTH_C_BAD = 0, DEPTH_C_NRUNS = 1, DEPTH_C_DEFER = 2, DEPTH_C_ROOM = 4, DEPTH_CTR_WORDS = 8 };   // (2 and 4: 64 bits)

struct DepthCores {
    uint32_t n;
    uint32_t q[DEPTH_CORES];
};

// ---- 1. column step ----------------------------------------------------------------------------------------------
// per (band, column), block b * cblocks + c taking band b and the columns 256 c ..: the first and last label, and
// lens = (run from the first row) | (run to the last row) << 16
__global__ __launch_bounds__(256) void k_depth_band_sum(const uint32_t *__restrict__ seg, uint32_t nrows, uint32_t ncols, uint32_t cblocks,
                                                        uint32_t *__restrict__ top_lab, uint32_t *__restrict__ bot_lab,
                                                        uint32_t *__restrict__ lens)
{
    const uint32_t b = blockIdx.x / cblocks, x = (blockIdx.x - b * cblocks) * 256u + threadIdx.x;
    if (x >= ncols) return;
    const uint32_t y0 = b * DEPTH_BAND, h = min(DEPTH_BAND, nrows - y0);
    const uint32_t *p = seg + (size_t)y0 * ncols + x;
    const uint32_t first = p[0];
    uint32_t prev = first, ltop = h, run = 0u;
    bool open = true;
    for (uint32_t i = 0; i < h; i++) {
        const uint32_t v = p[(size_t)i * ncols];
        if (v != prev) {
            if (open) { ltop = i; open = false; }
            run = 0u;
            prev = v;
        }
        run++;
    }
    const size_t o = (size_t)b * ncols + x;
    top_lab[o] = first;
    bot_lab[o] = prev;
    lens[o] = ltop | (run << 16);
}

// per column: up[b] = pixels of band b's first label directly above the band, down[b] likewise below its last row
__global__ __launch_bounds__(256) void k_depth_band_carry(uint32_t nrows, uint32_t ncols, uint32_t nbands,
                                                          const uint32_t *__restrict__ top_lab, const uint32_t *__restrict__ bot_lab,
                                                          const uint32_t *__restrict__ lens, uint32_t *__restrict__ up,
                                                          uint32_t *__restrict__ down)
{
    const uint32_t x = blockIdx.x * 256u + threadIdx.x;
    if (x >= ncols) return;
    uint32_t lab = 0u, len = 0u;            // the run that ends at the last row of the bands so far (len 0: none)
    for (uint32_t b = 0; b < nbands; b++) {
        const size_t o = (size_t)b * ncols + x;
        const uint32_t h = min(DEPTH_BAND, nrows - b * DEPTH_BAND);
        const uint32_t tl = top_lab[o], bl = bot_lab[o], ln = lens[o];
        const uint32_t carried = (len != 0u && lab == tl) ? len : 0u;
        up[o] = carried;
        if ((ln & 0xffffu) == h) len = carried + h;     // one label from edge to edge: the run goes on (no wrap: < 2^31 rows)
        else len = ln >> 16;
        lab = bl;
    }
    len = 0u;
    for (uint32_t b = nbands; b-- > 0u;) {
        const size_t o = (size_t)b * ncols + x;
        const uint32_t h = min(DEPTH_BAND, nrows - b * DEPTH_BAND);
        const uint32_t tl = top_lab[o], bl = bot_lab[o], ln = lens[o];
        const uint32_t carried = (len != 0u && lab == bl) ? len : 0u;
        down[o] = carried;
        if ((ln >> 16) == h) len = carried + h;
        else len = ln & 0xffffu;
        lab = tl;
    }
}

__global__ __launch_bounds__(256) void k_depth_col(const uint32_t *__restrict__ seg, uint32_t nrows, uint32_t ncols, uint32_t cblocks,
                                                   const uint32_t *__restrict__ up, const uint32_t *__restrict__ down,
                                                   uint16_t *__restrict__ g)
{
    const uint32_t b = blockIdx.x / cblocks, x = (blockIdx.x - b * cblocks) * 256u + threadIdx.x;
    if (x >= ncols) return;
    const uint32_t y0 = b * DEPTH_BAND, h = min(DEPTH_BAND, nrows - y0);
    const size_t base = (size_t)y0 * ncols + x;
    uint32_t lab[DEPTH_BAND], dt[DEPTH_BAND];
#pragma unroll
    for (uint32_t i = 0; i < DEPTH_BAND; i++) lab[i] = i < h ? seg[base + (size_t)i * ncols] : 0u;
    uint32_t t = up[(size_t)b * ncols + x];
#pragma unroll
    for (uint32_t i = 0; i < DEPTH_BAND; i++) {
        if (i > 0u && lab[i] != lab[i - 1u]) t = 0u;
        t++;
        dt[i] = t;
    }
    t = down[(size_t)b * ncols + x];
#pragma unroll
    for (uint32_t k = 0; k < DEPTH_BAND; k++) {
        const uint32_t i = DEPTH_BAND - 1u - k;
        if (i < h) {                                    // (rows past the raster's end are not part of the band)
            if (i + 1u < h && lab[i] != lab[i + 1u]) t = 0u;
            t++;
            g[base + (size_t)i * ncols] = (uint16_t)min(min(dt[i], t), DEPTH_GSAT);
        }
    }
}

// ---- 2. row step: the window ---------------------------------------------------------------------------------------
// ctr[DEPTH_C_DEFER] (64 bits): deferred pixels
__global__ __launch_bounds__(256) void k_depth_window(const uint32_t *__restrict__ seg, const uint16_t *__restrict__ g,
                                                      uint32_t nrows, uint32_t ncols, uint32_t tcols,
                                                      uint32_t *__restrict__ depth2, uint32_t *__restrict__ ctr)
{
    __shared__ uint32_t s_lab[DEPTH_TH][DEPTH_LW];
    __shared__ uint16_t s_g[DEPTH_TH][DEPTH_LW];
    const uint32_t ty = blockIdx.x / tcols, tx = blockIdx.x - ty * tcols;
    const uint32_t y0 = ty * DEPTH_TH, x0 = tx * DEPTH_TW;
    // columns outside the raster hold label 0 and are never a labelled pixel's own: the raster's edge is foreign
    for (uint32_t i = threadIdx.x; i < DEPTH_TH * DEPTH_LW; i += 256u) {
        const uint32_t r = i / DEPTH_LW, c = i - r * DEPTH_LW;
        const long long gx = (long long)x0 + c - (long long)DEPTH_HALO;
        const uint32_t gy = y0 + r;
        uint32_t v = 0u, gv = 0u;
        if (gy < nrows && gx >= 0 && gx < (long long)ncols) {
            const size_t o = (size_t)gy * ncols + (size_t)gx;
            v = seg[o];
            gv = g[o];
        }
        s_lab[r][c] = v;
        s_g[r][c] = (uint16_t)gv;
    }
    __syncthreads();
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    uint32_t ndefer = 0u;
    for (uint32_t rr = 0; rr < DEPTH_TH / 4u; rr++) {
        const uint32_t r = w * (DEPTH_TH / 4u) + rr;
        const uint32_t y = y0 + r, x = x0 + lane;
        if (y >= nrows) break;                          // (uniform in the wavefront)
        const uint32_t c = lane + DEPTH_HALO;
        const uint32_t own = s_lab[r][c];
        uint32_t best = 0u;
        if (x < ncols && own != 0u) {
            const uint32_t g0 = s_g[r][c];
            best = g0 * g0;
            bool decided = false;
            for (uint32_t d = 1u; d <= DEPTH_HALO; d++) {
                const uint32_t d2 = d * d;
                if (d2 >= best) { decided = true; break; }
                // (a column outside the raster holds 0 != own)
                const uint32_t ll = s_lab[r][c - d], lr = s_lab[r][c + d];
                if (ll != own || lr != own) { best = d2; decided = true; break; }
                const uint32_t gl = s_g[r][c - d], gr = s_g[r][c + d];
                best = min(best, d2 + min(gl * gl, gr * gr));
            }
            if (!decided) { best = DEPTH_DEFER; ndefer++; }
        }
        if (x < ncols) depth2[(size_t)y * ncols + x] = best;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) ndefer += (uint32_t)__shfl_xor(ndefer, d, 64);
    if (lane == 0u && ndefer) atomicAdd((unsigned long long *)(ctr + DEPTH_C_DEFER), (unsigned long long)ndefer);
}

// label 0 is depth 0 (path 'envelope' has no window to write it)
__global__ __launch_bounds__(256) void k_depth_zero(const uint32_t *__restrict__ seg, size_t n, uint32_t *__restrict__ depth2)
{
    for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (size_t)gridDim.x * 256u)
        if (seg[i] == 0u) depth2[i] = 0u;
}

// ---- 2. row step: the marked runs and their envelope -----------------------------------------------------------------
// runs[2k] = the linear index of marked run k's first pixel | its length << 32, runs[2k + 1] = its first scratch position.
// ctr[DEPTH_C_NRUNS]: runs marked; ctr[DEPTH_C_ROOM] (64 bits): scratch positions taken (length + 2 a run).  max_runs:
// room of the list (never reached: a marked run has at least 2 DEPTH_HALO + 1 pixels, or, with all = 1, one).
//
// A row is cut into pieces of DEPTH_TW columns.  k_depth_pieces, a wavefront per piece, notes per piece (three words):
// the first and the last label, and meta = (length of the run from the first column) | (length of the run to the last
// column) << 8 | flags << 16: the last run begins in this piece, it goes on into the next piece, the first run holds a
// deferred pixel, the last run does.  With all = 1 it also lists the runs that begin and end inside the piece (no such
// run is long enough to hold a deferred pixel).  k_depth_long, a thread per piece whose last run begins there and goes
// on, walks the pieces that follow, a step per piece, and lists the run if it holds a deferred pixel (or all = 1).
enum { DEPTH_P_BEGINS = 1, DEPTH_P_GOES_ON = 2, DEPTH_P_DEFER_FIRST = 4, DEPTH_P_DEFER_LAST = 8 };

__device__ __forceinline__ void depth_list_run(unsigned long long *__restrict__ runs, uint32_t max_runs, uint32_t k,
                                               unsigned long long at, size_t first, uint32_t len)
{
    if (k < max_runs) {
        runs[2 * (size_t)k] = (unsigned long long)first | ((unsigned long long)len << 32);
        runs[2 * (size_t)k + 1] = at;
    }
}

__global__ __launch_bounds__(256) void k_depth_pieces(const uint32_t *__restrict__ seg, const uint32_t *__restrict__ depth2,
                                                      uint32_t nrows, uint32_t ncols, uint32_t pcols, int all, uint32_t max_runs,
                                                      uint32_t *__restrict__ pieces, unsigned long long *__restrict__ runs,
                                                      uint32_t *__restrict__ ctr)
{
    const size_t piece = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (piece >= (size_t)nrows * pcols) return;         // (uniform in the wavefront)
    const uint32_t y = (uint32_t)(piece / pcols), x0 = (uint32_t)(piece - (size_t)y * pcols) * DEPTH_TW;
    const uint32_t lane = lane_id(), x = x0 + lane;
    const uint32_t nvalid = min(DEPTH_TW, ncols - x0);
    const size_t row = (size_t)y * ncols;
    const bool in = lane < nvalid;
    const uint32_t lab = in ? seg[row + x] : 0u;
    const bool defer = in && !all && depth2[row + x] == DEPTH_DEFER;
    const uint32_t left = (uint32_t)__shfl_up(lab, 1, 64);
    // the labels beside the piece (the same address in every lane)
    const bool has_before = x0 > 0u, has_after = x0 + DEPTH_TW < ncols;
    const uint32_t before = has_before ? seg[row + x0 - 1u] : 0u, after = has_after ? seg[row + x0 + DEPTH_TW] : 0u;
    const unsigned long long starts = __ballot(in && (lane == 0u || left != lab));      // (bit 0 is set: x0 < ncols)
    const unsigned long long defers = __ballot(defer);
    const unsigned long long rest = starts >> 1;
    const uint32_t len_first = rest ? (uint32_t)__builtin_ctzll(rest) + 1u : nvalid;
    const uint32_t last_at = 63u - (uint32_t)__builtin_clzll(starts);
    const uint32_t len_last = nvalid - last_at;
    const uint32_t lab_first = (uint32_t)__shfl(lab, 0, 64), lab_last = (uint32_t)__shfl(lab, (int)last_at, 64);
    const bool first_begins = !has_before || before != lab_first;       // the run at column x0 begins there
    const bool goes_on = has_after && after == lab_last;
    if (lane == 0u) {
        const unsigned long long first_mask = len_first == 64u ? ~0ull : ((1ull << len_first) - 1ull);
        uint32_t flags = 0u;
        if (last_at > 0u || first_begins) flags |= DEPTH_P_BEGINS;
        if (goes_on) flags |= DEPTH_P_GOES_ON;
        if (defers & first_mask) flags |= DEPTH_P_DEFER_FIRST;
        if (defers >> last_at) flags |= DEPTH_P_DEFER_LAST;
        pieces[3 * piece] = lab_first;
        pieces[3 * piece + 1] = lab_last;
        pieces[3 * piece + 2] = len_first | (len_last << 8) | (flags << 16);
    }
    if (all) {
        // the runs that begin and end in this piece, listed with two atomics a wavefront
        const bool start = in && lab != 0u && (lane == 0u ? first_begins : left != lab);
        const unsigned long long after_me = lane == 63u ? 0ull : (starts >> (lane + 1u));
        const uint32_t len = after_me ? (uint32_t)__builtin_ctzll(after_me) + 1u : nvalid - lane;
        const bool whole = start && (lane + len < nvalid || !goes_on);
        const unsigned long long listed = __ballot(whole);
        if (listed) {                                   // (uniform in the wavefront)
            const uint32_t v = whole ? len + 2u : 0u;
            uint32_t scan = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t o = (uint32_t)__shfl_up(scan, d, 64);
                if (lane >= (uint32_t)d) scan += o;
            }
            const uint32_t total = (uint32_t)__shfl(scan, 63, 64);
            uint32_t k0 = 0u;
            unsigned long long at0 = 0ull;
            if (lane == 0u) {
                k0 = atomicAdd(ctr + DEPTH_C_NRUNS, (uint32_t)__popcll(listed));
                at0 = atomicAdd((unsigned long long *)(ctr + DEPTH_C_ROOM), (unsigned long long)total);
            }
            k0 = (uint32_t)__shfl(k0, 0, 64);
            at0 = (unsigned long long)__shfl((long long)at0, 0, 64);
            if (whole)
                depth_list_run(runs, max_runs, k0 + (uint32_t)__popcll(listed & lanemask_lt()), at0 + scan - v, row + x, len);
        }
    }
}

__global__ __launch_bounds__(256) void k_depth_long(uint32_t nrows, uint32_t ncols, uint32_t pcols, int all, uint32_t max_runs,
                                                    const uint32_t *__restrict__ pieces, unsigned long long *__restrict__ runs,
                                                    uint32_t *__restrict__ ctr)
{
    const size_t npieces = (size_t)nrows * pcols;
    for (size_t p = (size_t)blockIdx.x * 256u + threadIdx.x; p < npieces; p += (size_t)gridDim.x * 256u) {
        const uint32_t meta = pieces[3 * p + 2], flags = meta >> 16;
        if ((flags & (DEPTH_P_BEGINS | DEPTH_P_GOES_ON)) != (DEPTH_P_BEGINS | DEPTH_P_GOES_ON) || pieces[3 * p + 1] == 0u) continue;
        const uint32_t y = (uint32_t)(p / pcols), px = (uint32_t)(p - (size_t)y * pcols);
        uint32_t len = (meta >> 8) & 0xffu;             // (the piece is whole: a run goes on from its last column)
        const size_t first = (size_t)y * ncols + (size_t)px * DEPTH_TW + (DEPTH_TW - len);
        bool defer = (flags & DEPTH_P_DEFER_LAST) != 0u;
        for (size_t j = p + 1;; j++) {                  // (the row's last piece does not go on: j stays in the row)
            const uint32_t mj = pieces[3 * j + 2], lf = mj & 0xffu;
            len += lf;
            defer = defer || ((mj >> 16) & DEPTH_P_DEFER_FIRST) != 0u;
            if (lf != DEPTH_TW || !((mj >> 16) & DEPTH_P_GOES_ON)) break;
        }
        if (!all && !defer) continue;
        const uint32_t k = atomicAdd(ctr + DEPTH_C_NRUNS, 1u);
        const unsigned long long at = atomicAdd((unsigned long long *)(ctr + DEPTH_C_ROOM), (unsigned long long)len + 2ull);
        depth_list_run(runs, max_runs, k, at, first, len);
    }
}

// site u of a run of m - 2 pixels: 0 and m - 1 are the foreign positions at its ends (height 0), 1 .. m - 2 its pixels
__device__ __forceinline__ unsigned long long depth_site(const uint16_t *__restrict__ gr, uint32_t u, uint32_t m)
{
    if (u == 0u || u == m - 1u) return 0ull;
    const unsigned long long v = gr[u - 1u];
    return v * v;
}

__global__ __launch_bounds__(64) void k_depth_envelope(const uint16_t *__restrict__ g, const unsigned long long *__restrict__ runs,
                                                       uint32_t nruns, uint32_t *__restrict__ sbuf, uint32_t *__restrict__ tbuf,
                                                       uint32_t *__restrict__ depth2)
{
    const uint32_t k = blockIdx.x * 64u + threadIdx.x;
    if (k >= nruns) return;
    const unsigned long long w0 = runs[2 * (size_t)k], at = runs[2 * (size_t)k + 1];
    const size_t first = (size_t)(w0 & 0xffffffffull);
    const uint32_t m = (uint32_t)(w0 >> 32) + 2u;       // (a row has fewer than 2^31 pixels)
    const uint16_t *gr = g + first;
    uint32_t *s = sbuf + at, *t = tbuf + at;
    // the stack's top entry stays in registers (site, where it begins to rule, its height): a step that neither pops nor
    // looks below the top then reads nothing but g
    long long q = 0;
    uint32_t top_s = 0u, top_t = 0u;
    unsigned long long top_g = 0ull;
    s[0] = 0u;
    t[0] = 0u;
    for (uint32_t u = 1u; u < m; u++) {
        const unsigned long long gu = depth_site(gr, u, m);
        while (q >= 0) {
            const unsigned long long di = top_t > top_s ? top_t - top_s : top_s - top_t, du = u > top_t ? u - top_t : top_t - u;
            if (di * di + top_g <= du * du + gu) break;
            q--;
            if (q >= 0) { top_s = s[q]; top_t = t[q]; top_g = depth_site(gr, top_s, m); }
        }
        if (q < 0) {
            q = 0;
            top_s = u; top_t = 0u; top_g = gu;
            s[0] = u;
            t[0] = 0u;
        } else {
            // the last x at which site i = s[q] is no worse than u: floor((u^2 - i^2 + G(u) - G(i)) / (2 (u - i))), whose
            // numerator is not negative here, since i is no worse than u at t[q] >= 0
            const unsigned long long num = (unsigned long long)(u - top_s) * ((unsigned long long)u + top_s) + gu - top_g;
            const unsigned long long den = 2ull * (u - top_s);
            const unsigned long long sep = (num | den) >> 32 ? num / den : (unsigned long long)((uint32_t)num / (uint32_t)den);
            if (sep + 1ull < (unsigned long long)m) {
                q++;
                top_s = u; top_t = (uint32_t)(sep + 1ull); top_g = gu;
                s[q] = top_s;
                t[q] = top_t;
            }
        }
    }
    for (uint32_t u = m - 1u;; u--) {
        if (u >= 1u && u <= m - 2u) {
            const unsigned long long d = u > top_s ? u - top_s : top_s - u;
            depth2[first + u - 1u] = (uint32_t)(d * d + top_g);
        }
        if (u == 0u) break;
        if (u == top_t) {                               // (t[0] = 0: the stack is never left empty before u = 0)
            q--;
            top_s = s[q]; top_t = t[q]; top_g = depth_site(gr, top_s, m);
        }
    }
}

// ---- 3. the per-id table -------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t depth_hash(uint32_t label)
{
    return ((label * 0x9E3779B1u) >> 16) & (DEPTH_SLOTS - 1u);
}

__device__ __forceinline__ void depth_emit(unsigned long long *__restrict__ tab, uint32_t label, uint32_t n, unsigned long long sum,
                                           unsigned long long key, const uint32_t *cores, uint32_t ncores)
{
    unsigned long long *row = tab + (size_t)label * DEPTH_WORDS;
    atomicAdd(row + DEPTH_AREA, (unsigned long long)n);
    atomicAdd(row + DEPTH_SUM, sum);
    atomicMax(row + DEPTH_KEY, key);
    for (uint32_t k = 0; k < ncores; k++)
        if (cores[k]) atomicAdd(row + DEPTH_CORE0 + k, (unsigned long long)cores[k]);
}

struct DepthTable {
    uint32_t key[DEPTH_SLOTS];              // 0 = empty
    uint32_t area[DEPTH_SLOTS];
    unsigned long long sum[DEPTH_SLOTS], mx[DEPTH_SLOTS];
    uint32_t core[DEPTH_CORES][DEPTH_SLOTS];
};

// One pass over the patch's rows.  DIRECT = false adds to the LDS table (*over is set when a label found no slot),
// DIRECT = true to the device table.
template <bool DIRECT>
__device__ __forceinline__ void depth_rows(const uint32_t *__restrict__ seg, const uint32_t *__restrict__ depth2, uint32_t nrows,
                                           uint32_t ncols, uint32_t S, uint32_t y0, uint32_t x0, const DepthCores &cq,
                                           DepthTable &tb, volatile uint32_t *over, unsigned long long *__restrict__ tab,
                                           uint32_t *mx_bad)
{
    const uint32_t w = threadIdx.x >> 6, lane = lane_id();
    for (uint32_t rr = 0; rr < DEPTH_PH / 4u; rr++) {
        const uint32_t y = y0 + w * (DEPTH_PH / 4u) + rr, x = x0 + lane;
        if (y >= nrows) break;                          // (uniform in the wavefront)
        const size_t o = (size_t)y * ncols + x;
        uint32_t lab = 0u, d2 = 0u;
        if (x < ncols) { lab = seg[o]; d2 = depth2[o]; }
        if (lab > S) { *mx_bad = max(*mx_bad, lab); lab = 0u; }
        const unsigned long long key = ((unsigned long long)d2 << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)o);
        const uint32_t lab0 = (uint32_t)__shfl(lab, 0, 64);
        const bool uniform = __ballot(lab != lab0) == 0ull;        // (uniform branch round the ballots)
        uint32_t n = 1u, cores[DEPTH_CORES];
        unsigned long long sum = d2, mk = key;
#pragma unroll
        for (uint32_t k = 0; k < DEPTH_CORES; k++) cores[k] = (k < cq.n && d2 > cq.q[k]) ? 1u : 0u;
        if (uniform && lab0 != 0u) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                sum += (unsigned long long)__shfl_xor((long long)sum, d, 64);
                const unsigned long long other = (unsigned long long)__shfl_xor((long long)mk, d, 64);
                mk = other > mk ? other : mk;
            }
#pragma unroll
            for (uint32_t k = 0; k < DEPTH_CORES; k++) cores[k] = (uint32_t)__popcll(__ballot(cores[k] != 0u));
            n = 64u;
        }
        const bool act = lab != 0u && (!uniform || lane == 0u);
        if (!act) {
        } else if (DIRECT) {
            depth_emit(tab, lab, n, sum, mk, cores, cq.n);
        } else if (!*over) {
            uint32_t h = depth_hash(lab);
            bool done = false;
            for (uint32_t probe = 0; probe < DEPTH_SLOTS; probe++) {
                const uint32_t old = atomicCAS(&tb.key[h], 0u, lab);
                if (old == 0u || old == lab) { done = true; break; }
                h = (h + 1u) & (DEPTH_SLOTS - 1u);
            }
            if (!done) {
                *over = 1u;
            } else {
                atomicAdd(&tb.area[h], n);
                atomicAdd(&tb.sum[h], sum);
                atomicMax(&tb.mx[h], mk);
#pragma unroll
                for (uint32_t k = 0; k < DEPTH_CORES; k++)
                    if (cores[k]) atomicAdd(&tb.core[k][h], cores[k]);
            }
        }
    }
}

// ctr[DEPTH_C_BAD]: the largest label above S met so far
__global__ __launch_bounds__(256) void k_depth_reduce(const uint32_t *__restrict__ seg, const uint32_t *__restrict__ depth2,
                                                      uint32_t nrows, uint32_t ncols, uint32_t pcols, uint32_t S, DepthCores cq,
                                                      unsigned long long *__restrict__ tab, uint32_t *__restrict__ ctr)
{
    __shared__ DepthTable tb;
    __shared__ uint32_t s_over;
    const uint32_t py = blockIdx.x / pcols, px = blockIdx.x - py * pcols;
    const uint32_t y0 = py * DEPTH_PH, x0 = px * DEPTH_TW;
    for (uint32_t i = threadIdx.x; i < DEPTH_SLOTS; i += 256u) {
        tb.key[i] = 0u; tb.area[i] = 0u; tb.sum[i] = 0ull; tb.mx[i] = 0ull;
#pragma unroll
        for (uint32_t k = 0; k < DEPTH_CORES; k++) tb.core[k][i] = 0u;
    }
    if (threadIdx.x == 0) s_over = 0u;
    __syncthreads();
    uint32_t mx = 0u;
    depth_rows<false>(seg, depth2, nrows, ncols, S, y0, x0, cq, tb, &s_over, tab, &mx);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    if (lane_id() == 0u && mx > S && mx > L2LOAD(&ctr[DEPTH_C_BAD])) atomicMax(&ctr[DEPTH_C_BAD], mx);
    __syncthreads();
    if (s_over == 0u) {
        for (uint32_t i = threadIdx.x; i < DEPTH_SLOTS; i += 256u) {
            const uint32_t key = tb.key[i];
            if (key == 0u) continue;
            uint32_t cores[DEPTH_CORES];
#pragma unroll
            for (uint32_t k = 0; k < DEPTH_CORES; k++) cores[k] = tb.core[k][i];
            depth_emit(tab, key, tb.area[i], tb.sum[i], tb.mx[i], cores, cq.n);
        }
    } else {
        depth_rows<true>(seg, depth2, nrows, ncols, S, y0, x0, cq, tb, &s_over, tab, &mx);
    }
}

// ---- host side --------------------------------------------------------------------------------------------
static inline size_t depth_grown(const DevBuf &b, size_t bytes)       // what buf_ensure would allocate
{
    if (bytes == 0) bytes = 16;
    return b.cap >= bytes ? 0 : bytes + bytes / 8 + 256;
}
static inline double depth_elapsed(hipEvent_t a, hipEvent_t b)
{
    float ms = 0.f;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? (double)ms : 0.0;
}
static inline size_t depth_bands(size_t nrows) { return (nrows + DEPTH_BAND - 1u) / DEPTH_BAND; }
static inline size_t depth_pieces(size_t nrows, size_t ncols) { return nrows * ((ncols + DEPTH_TW - 1u) / DEPTH_TW); }
static inline size_t depth_max_runs(size_t npix, int all) { return all ? npix : npix / (2u * DEPTH_HALO + 1u) + 1u; }

// The device memory the buffers still have to grow by.  marked < 0: for shp_depth_transform_dev on nrows x ncols pixels
// and the table of the ids 0 .. S; marked >= 0: for shp_depth_envelope on that many scratch positions.
static int run_depth_need(shp_ctx *ctx, size_t nrows, size_t ncols, size_t S, int all, long long marked, long long *need_out,
                          long long *free_out)
{
    size_t need = 0;
    if (marked < 0) {
        const size_t npix = nrows * ncols, nbc = depth_bands(nrows) * ncols;
        need += depth_grown(ctx->dp_g, npix * 2) + depth_grown(ctx->dp_d2, npix * 4) + depth_grown(ctx->dp_band, nbc * 20);
        need += depth_grown(ctx->dp_runs, depth_max_runs(npix, all) * 16) + depth_grown(ctx->dp_tab, (S + 1) * DEPTH_WORDS * 8);
        need += depth_grown(ctx->dp_ctr, DEPTH_CTR_WORDS * 4) + depth_grown(ctx->dp_piece, depth_pieces(nrows, ncols) * 12);
    } else {
        need += depth_grown(ctx->dp_scr, (size_t)marked * 8);
    }
    size_t fr = 0, tot = 0;
    HIPCHK(ctx, hipMemGetInfo(&fr, &tot));
    *need_out = (long long)need;
    *free_out = (long long)fr;
    return 0;
}

// steps 1 and 2 up to the list of marked runs
static int run_depth_transform(shp_ctx *ctx, const uint32_t *d_seg, uint32_t nrows, uint32_t ncols, int all, long long *counts_out)
{
    DepthState &s = ctx->depth;
    hipStream_t st = ctx->stream;
    s = DepthState{};
    const size_t npix = (size_t)nrows * ncols;
    CHK(buf_ensure(ctx, ctx->dp_ctr, DEPTH_CTR_WORDS * 4));
    uint32_t *ctr = bp<uint32_t>(ctx->dp_ctr);
    HIPCHK(ctx, hipMemsetAsync(ctr, 0, DEPTH_CTR_WORDS * 4, st));
    s.seg = d_seg; s.nrows = nrows; s.ncols = ncols; s.all = all;
    if (npix) {
        const size_t nb = depth_bands(nrows), nbc = nb * ncols, max_runs = depth_max_runs(npix, all);
        const uint32_t tcols = (ncols + DEPTH_TW - 1u) / DEPTH_TW, trows = (nrows + DEPTH_TH - 1u) / DEPTH_TH;
        const uint32_t cblocks = (ncols + 255u) / 256u;
        if ((unsigned long long)nb * cblocks > 0x7fffffffull || (unsigned long long)tcols * trows > 0x7fffffffull)
            SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large");
        CHK(buf_ensure(ctx, ctx->dp_g, npix * 2));
        CHK(buf_ensure(ctx, ctx->dp_d2, npix * 4));
        CHK(buf_ensure(ctx, ctx->dp_band, nbc * 20));
        CHK(buf_ensure(ctx, ctx->dp_runs, max_runs * 16));
        CHK(buf_ensure(ctx, ctx->dp_piece, depth_pieces(nrows, ncols) * 12));
        uint16_t *g = bp<uint16_t>(ctx->dp_g);
        uint32_t *d2 = bp<uint32_t>(ctx->dp_d2);
        uint32_t *top = bp<uint32_t>(ctx->dp_band), *bot = top + nbc, *lens = bot + nbc, *up = lens + nbc, *down = up + nbc;
        const dim3 bgrid((unsigned)nb * cblocks);
        HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
        hipLaunchKernelGGL(k_depth_band_sum, bgrid, dim3(256), 0, st, d_seg, nrows, ncols, cblocks, top, bot, lens);
        KCHK(ctx);
        hipLaunchKernelGGL(k_depth_band_carry, dim3(cblocks), dim3(256), 0, st, nrows, ncols, (uint32_t)nb,
                           (const uint32_t *)top, (const uint32_t *)bot, (const uint32_t *)lens, up, down);
        KCHK(ctx);
        hipLaunchKernelGGL(k_depth_col, bgrid, dim3(256), 0, st, d_seg, nrows, ncols, cblocks, (const uint32_t *)up, (const uint32_t *)down, g);
        KCHK(ctx);
        HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
        bool runs = all != 0;
        if (!all) {
            hipLaunchKernelGGL(k_depth_window, dim3(tcols * trows), dim3(256), 0, st, d_seg, (const uint16_t *)g, nrows, ncols, tcols,
                               d2, ctr);
            KCHK(ctx);
        } else {
            hipLaunchKernelGGL(k_depth_zero, dim3(grid_for(npix, 256 * 8, 16384u)), dim3(256), 0, st, d_seg, npix, d2);
            KCHK(ctx);
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev[2], st));
        if (!all) {
            HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr, DEPTH_CTR_WORDS * 4, hipMemcpyDeviceToHost, st));
            HIPCHK(ctx, hipStreamSynchronize(st));
            s.deferred = *(volatile unsigned long long *)(ctx->h_pinned + DEPTH_C_DEFER);
            runs = s.deferred != 0ull;
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev[3], st));
        if (runs) {
            const size_t npieces = depth_pieces(nrows, ncols);
            const uint32_t room = (uint32_t)min(max_runs, (size_t)0xffffffffu);
            uint32_t *pieces = bp<uint32_t>(ctx->dp_piece);
            hipLaunchKernelGGL(k_depth_pieces, dim3((unsigned)((npieces + 3u) / 4u)), dim3(256), 0, st, d_seg, (const uint32_t *)d2,
                               nrows, ncols, tcols, all, room, pieces, bp<unsigned long long>(ctx->dp_runs), ctr);
            KCHK(ctx);
            hipLaunchKernelGGL(k_depth_long, dim3(grid_for(npieces, 256, 16384u)), dim3(256), 0, st, nrows, ncols, tcols, all, room,
                               (const uint32_t *)pieces, bp<unsigned long long>(ctx->dp_runs), ctr);
            KCHK(ctx);
        }
        HIPCHK(ctx, hipEventRecord(ctx->ev[4], st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr, DEPTH_CTR_WORDS * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        s.nruns = ctx->h_pinned[DEPTH_C_NRUNS];
        s.room = *(volatile unsigned long long *)(ctx->h_pinned + DEPTH_C_ROOM);
        if ((size_t)s.nruns > max_runs) SHP_FAIL(ctx, SHP_ERR_STATE, "%u marked runs in a list of %zu", s.nruns, max_runs);
        s.ms[0] = depth_elapsed(ctx->ev[0], ctx->ev[1]);
        s.ms[1] = depth_elapsed(ctx->ev[1], ctx->ev[2]);
        s.ms[2] = depth_elapsed(ctx->ev[3], ctx->ev[4]);
    }
    counts_out[0] = (long long)s.deferred;
    counts_out[1] = (long long)s.nruns;
    counts_out[2] = (long long)s.room;
    s.stage = 1;
    return 0;
}

// step 2, the envelope of the marked runs
static int run_depth_envelope(shp_ctx *ctx)
{
    DepthState &s = ctx->depth;
    hipStream_t st = ctx->stream;
    if (s.nruns) {
        CHK(buf_ensure(ctx, ctx->dp_scr, (size_t)s.room * 8));
        uint32_t *sb = bp<uint32_t>(ctx->dp_scr), *tb = sb + s.room;
        HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
        hipLaunchKernelGGL(k_depth_envelope, dim3((s.nruns + 63u) / 64u), dim3(64), 0, st, (const uint16_t *)ctx->dp_g.p,
                           (const unsigned long long *)ctx->dp_runs.p, s.nruns, sb, tb, bp<uint32_t>(ctx->dp_d2));
        KCHK(ctx);
        HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        s.ms[2] += depth_elapsed(ctx->ev[0], ctx->ev[1]);
    }
    s.stage = 2;
    return 0;
}

// step 3; *bad_out: 0, or the largest label above S (then there is nothing to download)
static int run_depth_reduce(shp_ctx *ctx, uint32_t S, const DepthCores &cq, uint32_t *bad_out)
{
    DepthState &s = ctx->depth;
    hipStream_t st = ctx->stream;
    const size_t nwords = ((size_t)S + 1) * DEPTH_WORDS;
    CHK(buf_ensure(ctx, ctx->dp_tab, nwords * 8));
    uint32_t *ctr = bp<uint32_t>(ctx->dp_ctr);
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    HIPCHK(ctx, hipMemsetAsync(ctx->dp_tab.p, 0, nwords * 8, st));
    if (s.nrows && s.ncols) {
        const uint32_t pcols = (s.ncols + DEPTH_TW - 1u) / DEPTH_TW, prows = (s.nrows + DEPTH_PH - 1u) / DEPTH_PH;
        if ((unsigned long long)pcols * prows > 0x7fffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large");
        hipLaunchKernelGGL(k_depth_reduce, dim3(pcols * prows), dim3(256), 0, st, s.seg, (const uint32_t *)ctx->dp_d2.p, s.nrows,
                           s.ncols, pcols, S, cq, bp<unsigned long long>(ctx->dp_tab), ctr);
        KCHK(ctx);
    }
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, ctr, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    s.ms[3] = depth_elapsed(ctx->ev[0], ctx->ev[1]);
    s.S = S;
    *bad_out = *(volatile uint32_t *)ctx->h_pinned;
    s.stage = *bad_out ? 0 : 3;
    return 0;
}

static int run_depth_download(shp_ctx *ctx, uint64_t *rows, uint32_t *depth2)
{
    const DepthState &s = ctx->depth;
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(rows, ctx->dp_tab.p, ((size_t)s.S + 1) * DEPTH_WORDS * 8, hipMemcpyDeviceToHost, st));
    if (depth2 && s.nrows && s.ncols)
        HIPCHK(ctx, hipMemcpyAsync(depth2, ctx->dp_d2.p, (size_t)s.nrows * s.ncols * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}
