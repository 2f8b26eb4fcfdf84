// segstats.h -- per-segment statistics of one image band (the "tilingstats" reductions).
//
// Replaces tilingstats.accumulateSegDict / checkSegComplete / calcStatsForCompletedSegs /
// SegmentStats / RatPage (tilingstats.py:466-617, :866-1008, :1949-2045).  The reference builds
// a dict-of-dicts histogram per segment tile by tile; here the exact per-segment, value-sorted
// multiset is produced by two stable radix sorts (by value, then by segment id), after which a
// segment's valid pixel values are one contiguous ascending run:
//   pixcount = run length, min / max = ends, percentile p = element ceil(n*p/100)-1 (p = 0 gives
//   the LAST element: the reference's while loop never runs, tilingstats.py:979-986), median =
//   percentile 50, mode = first longest run of equal values, mean = exact int64 sum / n
//   (float64) stored float32, stddev with the reference's mixed float64/float32 evaluation
//   (see oracle/shepseg_oracle.c orc_segstats; pinned against the reference's goldens).
// Nodata pixels and the null segment are keyed to segment 0 before sorting and never counted.
// HBM-bound: 6 B/px in, ~3+3 radix passes of 16 B/px, 4*nCols B per segment out.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"
#include "clump.h"      // k_run_count
#include "elim_small.h"

__global__ __launch_bounds__(256) void k_stats_keys(const uint32_t *__restrict__ seg,
                                                    const void *__restrict__ band, int dtype,
                                                    uint32_t n, uint32_t S, int has_null,
                                                    long long null_val, long long bias,
                                                    uint32_t *__restrict__ kseg,
                                                    uint32_t *__restrict__ kval)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const long long v = ld_px(band, dtype, p);
    uint32_t s = seg[p];
    if (s > S || (has_null && v == null_val)) s = 0;
    kseg[p] = s;
    kval[p] = (uint32_t)(v - bias);
}

// the statistics of one segment into their columns (a: its ascending value run, n values)
__device__ __forceinline__ void seg_stats_emit(uint32_t s, uint32_t n, const uint32_t *a, long long bias,
                                               const uint32_t *__restrict__ sel, int nstats, long long missing,
                                               long long *__restrict__ intcols, float *__restrict__ fltcols,
                                               size_t ns, long long vmin, long long vmax, long long vmode,
                                               float mean, float stddev)
{
    for (int i = 0; i < nstats; i++) {
        const uint32_t stat = sel[i * 5 + 1], ctype = sel[i * 5 + 2], cidx = sel[i * 5 + 3];
        const uint32_t param = sel[i * 5 + 4];
        double val = 0.0;
        if (stat == 4u || stat == 6u) {
            if (n == 0) val = (double)missing;
            else {
                const double pc = (stat == 4u) ? 50.0 : (double)param;
                const double t = (double)n * (pc / 100.0);
                uint32_t idx = n - 1;                            // t == 0: loop never runs
                if (t > 0.0) {
                    double ct = ceil(t);
                    if (ct > (double)n) ct = (double)n;
                    idx = (uint32_t)ct - 1u;
                }
                val = (double)((long long)a[idx] + bias);
            }
        } else if (stat == 0u) val = (double)vmin;
        else if (stat == 1u) val = (double)vmax;
        else if (stat == 2u) val = (double)mean;
        else if (stat == 3u) val = (double)stddev;
        else if (stat == 5u) val = (double)vmode;
        else if (stat == 7u) val = (double)n;
        if (ctype == 0u) intcols[(size_t)cidx * ns + s] = (long long)val;
        else fltcols[(size_t)cidx * ns + s] = (float)val;
    }
}

// the statistics of one segment from its ascending value run (a[0..n), biased values), into their columns
__device__ __forceinline__ void seg_stats_of_run(uint32_t s, uint32_t n, const uint32_t *a, long long bias,
                                                 const uint32_t *__restrict__ sel, int nstats, long long missing,
                                                 long long *__restrict__ intcols, float *__restrict__ fltcols, size_t ns)
{
    long long vmin = missing, vmax = missing, vmode = missing;
    float mean = (float)missing, stddev = (float)missing;
    if (n > 0) {
        vmin = (long long)a[0] + bias;
        vmax = (long long)a[n - 1] + bias;
        long long sum = 0;
        for (uint32_t i = 0; i < n; i++) sum += (long long)a[i] + bias;
        mean = (float)((double)sum / (double)n);
        // one pass, closing a group of equal values at its last member (a nested "while the next one is equal" loop
        // had the lanes of a wavefront -- a segment each -- wait for one another at every group)
        float var = 0.0f;
        uint32_t bestc = 0, c = 0;
        uint32_t x = a[0];
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t nx = i + 1u < n ? a[i + 1u] : ~x;
            c++;
            if (nx != x) {
                const double d = (double)((long long)x + bias) - (double)mean;
                const float term = (float)((double)c * (d * d));
                var = var + term;
                if (c > bestc) { bestc = c; vmode = (long long)x + bias; }
                c = 0;
            }
            x = nx;
        }
        stddev = (float)sqrt((double)var / (double)n);
    }
    seg_stats_emit(s, n, a, bias, sel, nstats, missing, intcols, fltcols, ns, vmin, vmax, vmode, mean, stddev);
}

#define SEGSTATS_BIG 4096u       // segments above this many valid pixels go to k_seg_stats_big
#define SEGSTATS_STAGE 3072u     // values a wavefront stages in LDS (12 KiB; 48 KiB per workgroup)
// one thread per segment over its ascending value run
__global__ __launch_bounds__(256) void k_seg_stats(const uint32_t *__restrict__ vals,
                                                   const uint32_t *__restrict__ off,
                                                   const uint32_t *__restrict__ cnt, uint32_t S,
                                                   long long bias, const uint32_t *__restrict__ sel,
                                                   int nstats, long long missing,
                                                   long long *__restrict__ intcols,
                                                   float *__restrict__ fltcols, uint32_t *biglist,
                                                   const uint8_t *__restrict__ only)
{
    // (only != nullptr: the rows of unflagged segments belong to somebody else -- the patch path below)
    // The 64 segments of a wavefront hold one contiguous span of the value array.  When that span is
    // short (many small segments: 50 M segments of 32 pixels in the C5 workload) the wavefront loads
    // it into LDS with coalesced reads and every thread walks its own run there; a thread reading
    // its 128 bytes straight from memory, twice, moved a cache line per load.
    __shared__ uint32_t stage[4][SEGSTATS_STAGE];
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = lane_id(), wv = threadIdx.x >> 6;
    const uint32_t s_first = s - lane, s_last = s_first + 63u < S ? s_first + 63u : S;
    const uint32_t span0 = s_first <= S ? off[s_first] : 0u;
    const uint32_t span1 = s_first <= S ? off[s_last] + cnt[s_last] : 0u;
    const bool staged = span1 - span0 <= SEGSTATS_STAGE;          // (uniform per wavefront)
    if (staged) {
        for (uint32_t i = lane; i < span1 - span0; i += 64u) stage[wv][i] = vals[span0 + i];
        __builtin_amdgcn_wave_barrier();
    }
    if (s > S) return;
    const size_t ns = (size_t)S + 1;
    if (only && s != 0u && !only[s]) return;
    if (s == 0) {                       // null segment row: zeros (RatPage :1992-1996)
        for (int i = 0; i < nstats; i++) {
            if (sel[i * 5 + 2] == 0) intcols[(size_t)sel[i * 5 + 3] * ns] = 0;
            else fltcols[(size_t)sel[i * 5 + 3] * ns] = 0.0f;
        }
        return;
    }
    const uint32_t n = cnt[s];
    if (n > SEGSTATS_BIG) {             // a long run is a wavefront's work (k_seg_stats_big), not a thread's
        biglist[1u + atomicAdd(&biglist[0], 1u)] = s;
        return;
    }
    const uint32_t *a = staged ? &stage[wv][off[s] - span0] : vals + off[s];
    seg_stats_of_run(s, n, a, bias, sel, nstats, missing, intcols, fltcols, ns);
}

// Segments with long value runs, one wavefront each (a persistent grid over biglist: [0] = count,
// ids from [1]).  The sum is a parallel integer sum; the variance and the mode need the runs of equal
// values IN ORDER (the reference adds one float32 term per distinct value, ascending): the wavefront
// reads 64 values a step, finds the run boundaries with one ballot and closes the runs that end in
// the step one after the other -- at most one per distinct value in all, whatever the pixel count.
__global__ __launch_bounds__(256) void k_seg_stats_big(const uint32_t *__restrict__ vals,
                                                       const uint32_t *__restrict__ off,
                                                       const uint32_t *__restrict__ cnt, uint32_t S,
                                                       long long bias, const uint32_t *__restrict__ sel,
                                                       int nstats, long long missing,
                                                       long long *__restrict__ intcols,
                                                       float *__restrict__ fltcols, const uint32_t *biglist)
{
    const unsigned lane = lane_id();
    const uint32_t nbig = biglist[0];
    const size_t ns = (size_t)S + 1;
    for (uint32_t e = blockIdx.x * 4u + (threadIdx.x >> 6); e < nbig; e += gridDim.x * 4u) {
        const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane((int)biglist[1u + e]);
        const uint32_t n = (uint32_t)__builtin_amdgcn_readfirstlane((int)cnt[s]);
        const uint32_t *a = vals + (uint32_t)__builtin_amdgcn_readfirstlane((int)off[s]);
        long long sum = 0;
        for (uint32_t i = lane; i < n; i += 64u) sum += (long long)a[i] + bias;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
        const float mean = (float)((double)sum / (double)n);
        float var = 0.0f;
        uint32_t bestc = 0, curx = (uint32_t)__builtin_amdgcn_readfirstlane((int)a[0]), curc = 0;
        long long vmode = missing;
        for (uint32_t base = 0; base < n; base += 64u) {
            const uint32_t i = base + lane;
            const bool valid = i < n;
            const uint32_t x = valid ? a[i] : 0u;
            uint32_t prev = __shfl_up(x, 1, 64);
            if (lane == 0) prev = curx;
            unsigned long long heads = __ballot(valid && x != prev);
            const uint32_t nvalid = n - base < 64u ? n - base : 64u;
            uint32_t start = 0;
            while (heads) {
                const uint32_t h = (uint32_t)__builtin_ctzll(heads);
                heads &= heads - 1ull;
                curc += h - start;
                const double dd = (double)((long long)curx + bias) - (double)mean;
                var = var + (float)((double)curc * (dd * dd));
                if (curc > bestc) { bestc = curc; vmode = (long long)curx + bias; }
                curx = (uint32_t)__builtin_amdgcn_readlane((int)x, (int)h);
                curc = 0;
                start = h;
            }
            curc += nvalid - start;
        }
        {
            const double dd = (double)((long long)curx + bias) - (double)mean;
            var = var + (float)((double)curc * (dd * dd));
            if (curc > bestc) { bestc = curc; vmode = (long long)curx + bias; }
        }
        if (lane == 0) {
            const float stddev = (float)sqrt((double)var / (double)n);
            seg_stats_emit(s, n, a, bias, sel, nstats, missing, intcols, fltcols, ns, (long long)a[0] + bias,
                           (long long)a[n - 1] + bias, vmode, mean, stddev);
        }
    }
}

// ---- small segments: statistics patch by patch, without the global sorts -----------------------------
// Where the average segment is a few dozen pixels (the C5 workload: 50 M segments of 4 x 8 pixels) nearly
// every segment lies inside one 32 x 64-pixel patch, and six radix passes over (segment, value) pairs of the
// WHOLE raster -- 16 B per pixel and pass -- sort what is already together.  Here a workgroup takes a patch:
// its pixels stay in registers (eight per thread), the distinct labels get slots in an LDS hash table with
// their pixel counts; a label whose count equals its count in the whole raster (tot[], one histogram pass
// before) is COMPLETE here: its valid values (at most SPP_MAXRUN) are gathered into one LDS run, sorted by
// rank, and reduced with the same code as k_seg_stats.  The pixels of every other label --
// segments that straddle patches or are too long -- are appended to a (segment, value) list that goes through
// the sorts as before; flagged[] tells the two paths' rows apart.  HBM traffic: the rasters twice (histogram,
// patches) + the columns, instead of ~100 B per pixel.
#define SPP_H 32u
#define SPP_W 64u
#define SPP_PPT 8u                  // pixels per thread: SPP_H * SPP_W / 256
#define SPP_SLOTS 1024u
#define SPP_MAXDIST 704u            // distinct labels a patch may hold before it gives up (load factor 0.69)
#define SPP_MAXRUN 64u
#define SPP_EMPTY 0xFFFFFFFFu

// tot[label] = pixels carrying it (labels above S are nobody's), one atomic per run of equal labels per wavefront
__global__ __launch_bounds__(256) void k_label_hist(const uint32_t *__restrict__ seg, uint32_t n, uint32_t S,
                                                    uint32_t *tot)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    const bool inb = p < n;
    const unsigned lane = lane_id();
    const uint32_t v = inb ? seg[p] : 0u;
    const uint32_t pv = __shfl_up(v, 1, 64);
    const bool head = lane == 0 || pv != v || !inb;
    const unsigned long long heads = __ballot(head);
    if (head && inb && v != 0u && v <= S) {
        const unsigned long long nxt = (lane == 63) ? 0ull : (heads & ~((2ull << lane) - 1ull));
        const unsigned nl = nxt ? (unsigned)__builtin_ctzll(nxt) : 64u;
        atomicAdd(&tot[v], nl - lane);
    }
}

// The same over a raster of known shape, a workgroup per 32 x 64-pixel patch (the patches of k_stats_patch): the runs'
// counts are first combined in an LDS hash table, and a label costs ONE global atomic per patch it touches instead of
// one per row run (C5: 4 x 8-pixel blocks, 200 M run heads -> 50 M atomics).  A label that finds no slot (a patch
// with more than 1024 labels) is added directly.
__global__ __launch_bounds__(256) void k_label_hist_patch(const uint32_t *__restrict__ seg, uint32_t nrows, uint32_t ncols,
                                                          uint32_t S, uint32_t *tot)
{
    __shared__ uint32_t key[SPP_SLOTS], cnt[SPP_SLOTS];
    for (uint32_t i = threadIdx.x; i < SPP_SLOTS; i += 256u) { key[i] = SPP_EMPTY; cnt[i] = 0u; }
    __syncthreads();
    const uint32_t x0 = blockIdx.x * SPP_W, y0 = blockIdx.y * SPP_H;
    const unsigned lane = lane_id();
    uint32_t sv[SPP_PPT];
#pragma unroll
    for (uint32_t k = 0; k < SPP_PPT; k++) {          // (a wavefront = one row of the patch)
        const uint32_t pl = k * 256u + threadIdx.x;
        const uint32_t y = y0 + pl / SPP_W, x = x0 + (pl % SPP_W);
        sv[k] = (y < nrows && x < ncols) ? seg[(size_t)y * ncols + x] : 0u;
    }
#pragma unroll
    for (uint32_t k = 0; k < SPP_PPT; k++) {
        const uint32_t v = sv[k];
        const uint32_t pv = __shfl_up(v, 1, 64);
        const bool head = lane == 0 || pv != v;
        const unsigned long long heads = __ballot(head);
        if (!head || v == 0u || v > S) continue;
        const unsigned long long nxt = (lane == 63) ? 0ull : (heads & ~((2ull << lane) - 1ull));
        const uint32_t nl = (nxt ? (unsigned)__builtin_ctzll(nxt) : 64u) - lane;
        uint32_t h = (v * 2654435761u) >> 22;
        bool placed = false;
        for (uint32_t probe = 0; probe < SPP_SLOTS && !placed; probe++) {
            const uint32_t kk = key[h];
            if (kk == v) placed = true;
            else if (kk == SPP_EMPTY) {
                const uint32_t old = atomicCAS(&key[h], SPP_EMPTY, v);
                placed = old == SPP_EMPTY || old == v;
            }
            if (!placed) h = (h + 1u) & (SPP_SLOTS - 1u);
        }
        if (placed) atomicAdd(&cnt[h], nl);
        else atomicAdd(&tot[v], nl);
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < SPP_SLOTS; i += 256u)
        if (key[i] != SPP_EMPTY) atomicAdd(&tot[key[i]], cnt[i]);
}

// every row as for a segment without valid pixels; the paths below overwrite what they compute
__global__ __launch_bounds__(256) void k_stats_prefill(uint32_t S, long long bias, const uint32_t *__restrict__ sel,
                                                       int nstats, long long missing, long long *__restrict__ intcols,
                                                       float *__restrict__ fltcols)
{
    const uint32_t s = blockIdx.x * 256u + threadIdx.x;
    if (s > S) return;
    const size_t ns = (size_t)S + 1;
    if (s == 0) {
        for (int i = 0; i < nstats; i++) {
            if (sel[i * 5 + 2] == 0) intcols[(size_t)sel[i * 5 + 3] * ns] = 0;
            else fltcols[(size_t)sel[i * 5 + 3] * ns] = 0.0f;
        }
        return;
    }
    seg_stats_of_run(s, 0u, nullptr, bias, sel, nstats, missing, intcols, fltcols, ns);
}

// ---- the phases k_stats_patch and k_stats_patch_bands have in common (the LDS arrays are the kernels') ----
// (the slot probe/insert of a label is the same text in both kernels too, and stays there: as a function -- returning
//  the slot, or setting it through a reference -- it compiled to other instructions in all ten instantiations,
//  LABNOTES 2026-10-16)

// offs[slot] = the sum of the run lengths of the slots before it: mine[] are those of this thread's four slots
// (threadIdx.x * 4 ..), msum their sum.  Holds a workgroup barrier; the caller places one before offs[] is read.
__device__ __forceinline__ void spp_scan_offsets(const uint32_t (&mine)[4], uint32_t msum, uint32_t *s_wsum, uint16_t *offs)
{
    uint32_t incl = msum;                                  // inclusive scan over the workgroup's 256 threads
    const unsigned lane = lane_id(), wv = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if ((int)lane >= d) incl += o;
    }
    if (lane == 63) s_wsum[wv] = incl;
    __syncthreads();
    uint32_t base = incl - msum;
    for (unsigned w2 = 0; w2 < wv; w2++) base += s_wsum[w2];
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) { offs[threadIdx.x * 4u + q] = (uint16_t)base; base += mine[q]; }
}

// The rank of value v, stored at place rp of the run q[0..n): how many of the run's values come before it (smaller,
// or equal and stored earlier).
template <bool narrow>
__device__ __forceinline__ uint32_t spp_rank_in_run(const uint32_t *q, uint32_t n, uint32_t v, uint32_t rp)
{
    uint32_t r = 0;
    if (narrow) {
        // 8/16-bit bands: the run holds value << 6 | position (positions < SPP_MAXRUN = 64), and "smaller, or equal
        // and stored earlier" is ONE unsigned compare -- this loop is n iterations for each of the n values, a third
        // of the kernel's instructions: plain offsets from one base, so that a value costs a compare and an add
        const uint32_t me = (v << 6) | rp;
        uint32_t j = 0;
        for (; j + 8u <= n; j += 8u) {
#pragma unroll
            for (uint32_t u = 0; u < 8u; u++) r += q[j + u] < me ? 1u : 0u;
        }
        for (; j < n; j++) r += q[j] < me ? 1u : 0u;
    } else {
        for (uint32_t j = 0; j < n; j++) {
            const uint32_t w = q[j];
            r += (w < v || (w == v && j < rp)) ? 1u : 0u;
        }
    }
    return r;
}

// (eight workgroups per CU -- 64 VGPRs, 20 KiB of LDS -- is worth more here than any unrolling: 23.4 ms at five,
//  21.5 at eight on C5 with the same instructions)
// (DT: the band's pixel type at compile time -- eight loads issued together instead of eight trips through a
//  run-time switch, each with its own wait)
template <int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_stats_patch(const uint32_t *__restrict__ seg, const void *__restrict__ band,
                                                     uint32_t nrows, uint32_t ncols, uint32_t S,
                                                     int has_null, long long null_val, long long bias,
                                                     const uint32_t *__restrict__ tot, const uint32_t *__restrict__ sel,
                                                     int nstats, long long missing, long long *__restrict__ intcols,
                                                     float *__restrict__ fltcols, uint8_t *__restrict__ flagged,
                                                     uint32_t *__restrict__ left_seg, uint32_t *__restrict__ left_val,
                                                     uint32_t *left_count)
{
    // (LDS per workgroup sets how many of them a CU holds, and the kernel lives on that: the fill counters share
    //  cnt[]'s low half once the pixel totals have been compared, the offsets are 16-bit)
    __shared__ uint32_t key[SPP_SLOTS], cnt[SPP_SLOTS];
    __shared__ uint16_t offs[SPP_SLOTS];
    // (runs padded to 16 bytes for four-value LDS reads in the rank loop were tried: 23.6 ms on C5 against 21.5 --
    //  the LDS the padding takes costs more in resident workgroups than the wider reads save)
    // (and one unused entry behind every run: runs of equal length would start at multiples of it, and the labels of
    //  a wavefront read the same few banks all through the rank loop)
    __shared__ uint32_t runs[SPP_H * SPP_W + SPP_MAXDIST];
    __shared__ uint32_t s_ndist, s_left, s_leftbase, s_wsum[4], s_nc;
    __shared__ uint16_t clist[SPP_SLOTS];       // the complete labels' slots, compacted: consecutive threads take them
    for (uint32_t i = threadIdx.x; i < SPP_SLOTS; i += 256u) { key[i] = SPP_EMPTY; cnt[i] = 0u; }
    if (threadIdx.x == 0) { s_ndist = 0u; s_left = 0u; s_nc = 0u; }
    __syncthreads();
    const uint32_t x0 = blockIdx.x * SPP_W, y0 = blockIdx.y * SPP_H;
    constexpr bool narrow = DT != SHP_I32 && DT != SHP_U32;         // biased values below 2^16
    // this thread's pixels: (segment, biased value, slot); the same thread keeps them through every phase
    uint32_t ps[SPP_PPT], pv[SPP_PPT], pslot[SPP_PPT];
    bool pvalid[SPP_PPT];
#pragma unroll
    for (uint32_t k = 0; k < SPP_PPT; k++) {
        const uint32_t pl = k * 256u + threadIdx.x;
        const uint32_t y = y0 + pl / SPP_W, x = x0 + (pl % SPP_W);
        ps[k] = 0u; pv[k] = 0u; pvalid[k] = false;
        if (y < nrows && x < ncols) {
            const size_t p = (size_t)y * ncols + x;
            const uint32_t sg = seg[p];
            const long long v = ld_t<DT>(band, p);
            if (sg != 0u && sg <= S) {
                ps[k] = sg;
                pv[k] = (uint32_t)(v - bias);
                pvalid[k] = !(has_null && v == null_val);
            }
        }
    }
    // ---- slots and counts (all pixels in the low half, valid ones in the high half) ----
#pragma unroll
    for (uint32_t k = 0; k < SPP_PPT; k++) {
        pslot[k] = SPP_SLOTS;
        if (ps[k] == 0u) continue;
        uint32_t h = (ps[k] * 2654435761u) >> 22;
        for (uint32_t probe = 0; probe < SPP_SLOTS; probe++) {
            const uint32_t kk = key[h];
            if (kk == ps[k]) { pslot[k] = h; break; }
            if (kk == SPP_EMPTY) {
                const uint32_t old = atomicCAS(&key[h], SPP_EMPTY, ps[k]);
                if (old == SPP_EMPTY) { atomicAdd(&s_ndist, 1u); pslot[k] = h; break; }
                if (old == ps[k]) { pslot[k] = h; break; }
            }
            h = (h + 1u) & (SPP_SLOTS - 1u);
        }
        if (pslot[k] < SPP_SLOTS) atomicAdd(&cnt[pslot[k]], 1u + (pvalid[k] ? 65536u : 0u));
    }
    __syncthreads();
    const bool crowded = s_ndist > SPP_MAXDIST;          // (a pixel may then have found no slot at all)
    // ---- which labels are complete here; run offsets by a scan of their valid counts ----
    uint32_t mine[4], msum = 0;
#pragma unroll
    for (uint32_t q = 0; q < 4u; q++) {
        const uint32_t sl = threadIdx.x * 4u + q;
        const uint32_t kk = key[sl], c = cnt[sl];
        uint32_t nv = 0;
        if (kk != SPP_EMPTY) {
            const bool complete = !crowded && (c & 0xFFFFu) == tot[kk] && (c >> 16) <= SPP_MAXRUN;
            if (complete) { nv = (c >> 16) + 1u; clist[atomicAdd(&s_nc, 1u)] = (uint16_t)sl; }
            else flagged[kk] = 1;
            // bit 31: complete; the low half (all pixels) has served and becomes the run's fill counter
            cnt[sl] = complete ? ((c & 0x7FFF0000u) | 0x80000000u) : (c & 0x7FFFFFFFu);
        }
        mine[q] = nv;
        msum += nv;
    }
    spp_scan_offsets(mine, msum, s_wsum, offs);
    __syncthreads();
    // ---- values of complete labels into their runs, the rest into the list ----
    // (a run's first lane probing and adding for the run -- one atomic per run instead of one per pixel -- was built
    //  twice, rounds 3 and 4: 27.1 -> 30.7 ms and 15.9 -> 17.9 ms; the masks and shuffles cost more than the
    //  eight-way same-address atomics they save)
    // rpos[k]: the place in the label's run; 0x80000000 | place in the left-over list; 0xFFFFFFFF: neither
    uint32_t rpos[SPP_PPT];
#pragma unroll
    for (uint32_t k = 0; k < SPP_PPT; k++) {
        rpos[k] = 0xFFFFFFFFu;
        if (ps[k] == 0u || !pvalid[k]) continue;           // (nodata pixels count for completeness only)
        const uint32_t sl = pslot[k];
        if (sl < SPP_SLOTS && (cnt[sl] & 0x80000000u)) {
            rpos[k] = atomicAdd(&cnt[sl], 1u) & 0xFFFFu;
            runs[offs[sl] + rpos[k]] = narrow ? (pv[k] << 6) | rpos[k] : pv[k];
        } else rpos[k] = 0x80000000u | atomicAdd(&s_left, 1u);
    }
    if (crowded) {                                          // pixels without a slot: their labels are flagged here
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++)
            if (ps[k] != 0u && pslot[k] >= SPP_SLOTS) flagged[ps[k]] = 1;
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_left) s_leftbase = atomicAdd(left_count, s_left);
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < SPP_PPT; k++)
        if (rpos[k] != 0xFFFFFFFFu && (rpos[k] & 0x80000000u)) {
            const uint32_t li = s_leftbase + (rpos[k] & 0x7FFFFFFFu);
            left_seg[li] = ps[k]; left_val[li] = pv[k];
            rpos[k] = 0xFFFFFFFFu;                           // (not a member of a run)
        }
    // ---- the runs sorted by RANK: every pixel counts the values of its run that come before it (smaller, or equal
    //      and stored earlier) -- all threads busy on independent LDS reads, where a thread per run doing an
    //      insertion sort was a chain of dependent LDS round trips on a quarter of the lanes ----
    // (the rank takes the place of rpos[k] once it is known, and the final place offs + rank the place of that)
#pragma unroll
    for (uint32_t k = 0; k < SPP_PPT; k++) {
        if (rpos[k] == 0xFFFFFFFFu) continue;
        const uint32_t sl = pslot[k];
        const uint32_t n = (cnt[sl] >> 16) & 0x7FFFu, o = offs[sl];
        rpos[k] = o + spp_rank_in_run<narrow>(&runs[o], n, pv[k], rpos[k]);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < SPP_PPT; k++)
        if (rpos[k] != 0xFFFFFFFFu) runs[rpos[k]] = pv[k];
    __syncthreads();
    // ---- a thread per complete label -- consecutive threads take consecutive entries of the compacted list, so
    //      that a wavefront's lanes all work (a thread per SLOT left 4 lanes in 64 busy, four times over) ----
    const size_t ns = (size_t)S + 1;
    for (uint32_t ci = threadIdx.x; ci < s_nc; ci += 256u) {
        const uint32_t sl = clist[ci];
        const uint32_t n = (cnt[sl] >> 16) & 0x7FFFu;
        seg_stats_of_run(key[sl], n, &runs[offs[sl]], bias, sel, nstats, missing, intcols, fltcols, ns);
    }
}

// d_seg / d_band: device rasters of n pixels.  Outputs are HOST arrays.
// nrows x ncols = n when the caller knows the raster's shape (0, 0 otherwise): with small segments the
// statistics are then computed patch by patch (k_stats_patch) and only what is left over is sorted.
// The result columns go to pageable host arrays (the caller's numpy columns): the runtime stages such a copy
// through its own pinned buffers, one pipeline per stream, so the integer and the float columns travel on two
// streams at once (the second waits on an event for the kernels that wrote them).
static int segstats_download(shp_ctx *ctx, void *intcols_out, const void *d_int, size_t int_bytes,
                             void *fltcols_out, const void *d_flt, size_t flt_bytes)
{
    hipStream_t st = ctx->stream;
    if (int_bytes && flt_bytes && int_bytes + flt_bytes > (size_t)(8u << 20)) {
        CHK(ensure_stream2(ctx));
        hipEvent_t ev = nullptr;
        HIPCHK(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        HIPCHK(ctx, hipEventRecord(ev, st));
        HIPCHK(ctx, hipStreamWaitEvent(ctx->stream2, ev, 0));
        HIPCHK(ctx, hipMemcpyAsync(fltcols_out, d_flt, flt_bytes, hipMemcpyDeviceToHost, ctx->stream2));
        HIPCHK(ctx, hipMemcpyAsync(intcols_out, d_int, int_bytes, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream2));
        HIPCHK(ctx, hipEventDestroy(ev));
        return 0;
    }
    if (int_bytes) HIPCHK(ctx, hipMemcpyAsync(intcols_out, d_int, int_bytes, hipMemcpyDeviceToHost, st));
    if (flt_bytes) HIPCHK(ctx, hipMemcpyAsync(fltcols_out, d_flt, flt_bytes, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// The two sorts and the reducers over n (segment key, biased value) pairs in ctx->aux2 / ctx->aux: by value (payload:
// segment key), then stably by segment key (payload: value); then a thread per segment (k_seg_stats), a wavefront per
// long one (k_seg_stats_big).  only != nullptr: only the rows of flagged segments are written.
static int segstats_sort_reduce(shp_ctx *ctx, uint32_t n, uint32_t S, int valbits, long long bias, const uint32_t *d_sel,
                                int nstats, int64_t missing, long long *d_int, float *d_flt, const uint8_t *only)
{
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    uint32_t *kval = bp<uint32_t>(ctx->aux), *kseg = bp<uint32_t>(ctx->aux2);
    uint32_t *cnt = bp<uint32_t>(ctx->segsz), *off = bp<uint32_t>(ctx->off);
    // sort by value (payload: segment key), then stably by segment key (payload: value)
    uint32_t *k1 = nullptr, *v1 = nullptr, *k2 = nullptr, *v2 = nullptr;
    CHK(sort_pairs(ctx, kval, kseg, n, valbits, &k1, &v1, true));            // k1 = values, v1 = seg keys
    // the second sort reads the first one's result where it lies unless its own first pass would
    // write into the same ping-pong buffers (that depends on the two pass counts' parities)
    const uint32_t *in_seg = v1, *in_val = k1;
    {
        const int passes2 = (bits_for(S) + 7) / 8;
        const uint32_t *out_k = bp<uint32_t>(ctx->sort_k0);
        const uint32_t *out_v = (passes2 & 1) ? bp<uint32_t>(ctx->pix) : bp<uint32_t>(ctx->sort_v1);
        if (n && (k1 == out_k || k1 == out_v || v1 == out_k || v1 == out_v)) {
            HIPCHK(ctx, hipMemcpyAsync(kval, k1, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(kseg, v1, (size_t)n * 4, hipMemcpyDeviceToDevice, st));
            in_seg = kseg; in_val = kval;
        }
    }
    CHK(sort_pairs(ctx, in_seg, in_val, n, bits_for(S), &k2, &v2, true));    // k2 = seg keys, v2 = values
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(ns)));
    HIPCHK(ctx, hipMemsetAsync(cnt, 0, ns * 4, st));
    if (n) {
        hipLaunchKernelGGL(k_run_count, dim3(grid_for(n, 256)), dim3(256), 0, st, k2, n, cnt, 0u, 0); KCHK(ctx);
    }
    ArrFn cf{cnt};
    CHK(scan_exclusive(ctx, cf, (uint32_t)ns, off, nullptr, bp<uint32_t>(ctx->scan_tmp)));
    // (the list of long segments: in the first sort's key buffer, free by now)
    uint32_t *biglist = kval;
    HIPCHK(ctx, hipMemsetAsync(biglist, 0, 4, st));
    hipLaunchKernelGGL(k_seg_stats, dim3(grid_for(ns, 256)), dim3(256), 0, st, v2, off, cnt, S, bias, d_sel,
                       nstats, (long long)missing, d_int, d_flt, biglist, only); KCHK(ctx);
    hipLaunchKernelGGL(k_seg_stats_big, dim3(512), dim3(256), 0, st, v2, off, cnt, S, bias, d_sel, nstats,
                       (long long)missing, d_int, d_flt, biglist); KCHK(ctx);      // (only flagged ones got onto the list)
    return 0;
}

// ---- what the drivers below do alike ----
// A selection as the host hands it over, five words per statistic: statistic id and column type are checked, the
// integer and the float columns counted.  index_runs: the column array indices must number the columns of each
// type 0, 1, 2 .. in the order of the entries (the several-band form: its bands' columns lie side by side).
static int stats_sel_check(shp_ctx *ctx, const uint32_t *sel_host, int nstats, int *nint_out = nullptr,
                           int *nflt_out = nullptr, bool index_runs = false)
{
    int nint = 0, nflt = 0;
    for (int i = 0; i < nstats; i++) {
        const uint32_t stat = sel_host[i * 5 + 1], ctype = sel_host[i * 5 + 2];
        if (stat > 7u || ctype > 1u) SHP_FAIL(ctx, SHP_ERR_ARG, "bad statsSelection entry %d", i);
        if (index_runs && sel_host[i * 5 + 3] != (uint32_t)(ctype == 0 ? nint : nflt))
            SHP_FAIL(ctx, SHP_ERR_ARG, "statsSelection entry %d: column array index does not run through the bands", i);
        if (ctype == 0) nint++; else nflt++;
    }
    if (nint_out) *nint_out = nint;
    if (nflt_out) *nflt_out = nflt;
    return 0;
}

// value - bias is the unsigned sort key of a pixel value, valbits wide
static void stats_value_range(int dtype, long long *bias, int *valbits)
{
    *bias = 0;
    *valbits = 32;
    switch (dtype) {
    case SHP_U8: *valbits = 8; break;
    case SHP_U16: *valbits = 16; break;
    case SHP_I16: *valbits = 16; *bias = -32768; break;
    case SHP_I32: *bias = -2147483648ll; break;
    default: break;
    }
}

// Patch by patch, or everything through the sorts?  SHEPSEG_STATS_PATCH=0: never; =1: whenever the raster's shape
// is known; default: when the average segment has at most SPP_MAXRUN pixels.
static bool stats_use_patches(uint32_t n, uint32_t S, bool shape_known)
{
    const int patch_env = getenv("SHEPSEG_STATS_PATCH") ? atoi(getenv("SHEPSEG_STATS_PATCH")) : -1;
    return n && shape_known && patch_env != 0 &&
           (patch_env == 1 || (uint64_t)n <= (uint64_t)SPP_MAXRUN * ((uint64_t)S + 1));
}

// the workspace of a statistics run over n pixels and ns rows: sort keys, run counts and offsets, the small buffer
// (left-over count | selection | what else the caller keeps there), the columns
static int stats_workspace(shp_ctx *ctx, uint32_t n, size_t ns, size_t small_bytes, int nint, int nflt)
{
    CHK(buf_ensure(ctx, ctx->aux, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->aux2, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->segsz, (ns + 1) * 4));
    CHK(buf_ensure(ctx, ctx->off, (ns + 1) * 4 + 16));
    CHK(buf_ensure(ctx, ctx->small, small_bytes));
    CHK(buf_ensure(ctx, ctx->ssum, ((size_t)nint * 8 + (size_t)nflt * 4) * ns + 64));
    return 0;
}

static int run_segstats(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                        uint32_t n, uint32_t S, int has_null, int64_t null_val,
                        const uint32_t *sel_host, int nstats, int64_t missing,
                        int64_t *intcols_out, float *fltcols_out, uint32_t nrows = 0, uint32_t ncols = 0,
                        long long **dev_int = nullptr, float **dev_flt = nullptr)
{
    // (dev_int / dev_flt given: the columns stay in the context's workspace, nothing is copied to the host)
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    int nint = 0, nflt = 0;
    CHK(stats_sel_check(ctx, sel_host, nstats, &nint, &nflt));
    if ((size_t)nstats * 20 + 64 > SHP_PINNED_BYTES) SHP_FAIL(ctx, SHP_ERR_ARG, "too many statistics");
    long long bias;
    int valbits;
    stats_value_range(dtype, &bias, &valbits);
    CHK(stats_workspace(ctx, n, ns, 4096 + (size_t)nstats * 20, nint, nflt));
    uint32_t *kval = bp<uint32_t>(ctx->aux), *kseg = bp<uint32_t>(ctx->aux2);
    uint32_t *d_sel = bp<uint32_t>(ctx->small) + 256;
    long long *d_int = (long long *)ctx->ssum.p;
    float *d_flt = (float *)(d_int + (size_t)nint * ns);
    HIPCHK(ctx, hipStreamSynchronize(st));
    uint32_t *pin = ctx->h_pinned + 16;
    memcpy(pin, sel_host, (size_t)nstats * 20);
    HIPCHK(ctx, hipMemcpyAsync(d_sel, pin, (size_t)nstats * 20, hipMemcpyHostToDevice, st));
    const int ps = prof_begin(ctx, PROF_SEGSTATS);      // device time of the kernels (keys .. statistics)
    const bool patches = stats_use_patches(n, S, nrows && ncols && (uint64_t)nrows * ncols == n);
    const uint8_t *only = nullptr;
    uint32_t nsort = n;                                   // pairs that go through the sorts
    if (patches) {
        CHK(buf_ensure(ctx, ctx->tcount, (ns + 1) * 4));
        CHK(buf_ensure(ctx, ctx->mergeto, ns + 64));
        uint32_t *tot = bp<uint32_t>(ctx->tcount);
        uint8_t *flagged = bp<uint8_t>(ctx->mergeto);
        uint32_t *d_left = bp<uint32_t>(ctx->small);      // (word 0; the selection sits behind word 256)
        HIPCHK(ctx, hipMemsetAsync(tot, 0, ns * 4, st));
        HIPCHK(ctx, hipMemsetAsync(flagged, 0, ns, st));
        HIPCHK(ctx, hipMemsetAsync(d_left, 0, 4, st));
        hipLaunchKernelGGL(k_label_hist_patch, dim3(grid_for(ncols, SPP_W), grid_for(nrows, SPP_H)), dim3(256), 0, st, d_seg,
                           (uint32_t)nrows, (uint32_t)ncols, S, tot); KCHK(ctx);
        hipLaunchKernelGGL(k_stats_prefill, dim3(grid_for(ns, 256)), dim3(256), 0, st, S, bias, d_sel, nstats,
                           (long long)missing, d_int, d_flt); KCHK(ctx);
        DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(k_stats_patch<DT>, dim3(grid_for(ncols, SPP_W), grid_for(nrows, SPP_H)),
                                                 dim3(256), 0, st, d_seg, d_band, (uint32_t)nrows, (uint32_t)ncols, S, has_null,
                                                 (long long)null_val, bias, tot, d_sel, nstats, (long long)missing, d_int,
                                                 d_flt, flagged, kseg, kval, d_left));
        KCHK(ctx);
        CHK(read_u32(ctx, d_left, &nsort));
        only = flagged;
    } else if (n) {
        hipLaunchKernelGGL(k_stats_keys, dim3(grid_for(n, 256)), dim3(256), 0, st, d_seg, d_band, dtype, n,
                           S, has_null, (long long)null_val, bias, kseg, kval); KCHK(ctx);
    }
    if (patches && nsort == 0) {                          // every segment was complete in its patch
        prof_end(ctx, ps);
        if (dev_int) { *dev_int = d_int; *dev_flt = d_flt; return 0; }
        return segstats_download(ctx, intcols_out, d_int, (size_t)nint * ns * 8, fltcols_out, d_flt, (size_t)nflt * ns * 4);
    }
    CHK(segstats_sort_reduce(ctx, nsort, S, valbits, bias, d_sel, nstats, missing, d_int, d_flt, only));
    prof_end(ctx, ps);
    if (dev_int) { *dev_int = d_int; *dev_flt = d_flt; return 0; }
    return segstats_download(ctx, intcols_out, d_int, (size_t)nint * ns * 8, fltcols_out, d_flt, (size_t)nflt * ns * 4);
}

// ---- several bands in one pass over the labels ------------------------------------------------------------------
// The bands of one image share the label raster, and most of the work above depends on the labels alone: the label
// totals (k_label_hist_patch), the slot table of a patch, which labels are complete in it, and which pixels are left
// over for the sorts.  k_stats_patch_bands does that part once per patch and then takes the bands one after the other
// through the same LDS arrays; what is left over is ONE list of (label, pixel position), from which each band
// gathers its values for the two sorts.
// A label is complete in a patch when all its pixels lie there and they are at most SPP_MAXRUN -- ALL pixels, where
// k_stats_patch asks that of the valid ones: the valid count differs from band to band, the pixel count does not,
// and a label's row has the same bits on either path (a run is a run).
struct StatsBand {                  // one entry of the device table, 32 bytes
    const void *band;               // the band's plane of the row block (device memory)
    long long null_val;
    int has_null;
    int sel_first, nstats;          // its rows of the combined selection
    int pad;
};

template <int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(7, 8))) void k_stats_patch_bands(
    const uint32_t *__restrict__ seg, const StatsBand *__restrict__ bands, int nbands, uint32_t nrows, uint32_t ncols,
    uint32_t S, long long bias, const uint32_t *__restrict__ tot, const uint32_t *__restrict__ sel, long long missing,
    long long *__restrict__ intcols, float *__restrict__ fltcols, uint8_t *__restrict__ flagged,
    uint32_t *__restrict__ left_seg, uint32_t *__restrict__ left_pos, uint32_t *left_count)
{
    // (the same LDS as k_stats_patch, byte for byte: the arrays are reused from band to band.  cnt[]: bit 31 = the
    //  label is complete here; the two 15-bit halves below it are the run's fill counter, bands taking them in turn,
    //  so that a band's counter can be cleared while nobody reads it -- during the next band)
    __shared__ uint32_t key[SPP_SLOTS], cnt[SPP_SLOTS];
    __shared__ uint16_t offs[SPP_SLOTS];
    __shared__ uint32_t runs[SPP_H * SPP_W + SPP_MAXDIST];
    __shared__ uint32_t s_ndist, s_left, s_leftbase, s_wsum[4], s_nc;
    __shared__ uint16_t clist[SPP_SLOTS];
    for (uint32_t i = threadIdx.x; i < SPP_SLOTS; i += 256u) { key[i] = SPP_EMPTY; cnt[i] = 0u; }
    if (threadIdx.x == 0) { s_ndist = 0u; s_left = 0u; s_nc = 0u; }
    __syncthreads();
    const uint32_t x0 = blockIdx.x * SPP_W, y0 = blockIdx.y * SPP_H;
    constexpr bool narrow = DT != SHP_I32 && DT != SHP_U32;         // biased values below 2^16
    // this thread's pixels: pixel k is patch pixel k * 256 + threadIdx.x, through every phase and band
    // (a band's values are loaded when its turn comes, not with the labels: holding the first band's through the
    //  label phases, or the next band's through the statistics of the one at hand, takes the kernel past the 72
    //  VGPRs of seven wavefronts per SIMD -- 28 to 36 bytes of scratch per lane in the compiler's report)
    uint32_t pslot[SPP_PPT];
    {
        uint32_t ps[SPP_PPT];
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++) {
            const uint32_t pl = k * 256u + threadIdx.x;
            const uint32_t y = y0 + pl / SPP_W, x = x0 + (pl % SPP_W);
            ps[k] = 0u;
            if (y < nrows && x < ncols) {
                const uint32_t sg = seg[(size_t)y * ncols + x];
                if (sg <= S) ps[k] = sg;
            }
        }
        // ---- slots and pixel counts ----
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++) {
            pslot[k] = SPP_SLOTS;
            if (ps[k] == 0u) continue;
            uint32_t h = (ps[k] * 2654435761u) >> 22;
            for (uint32_t probe = 0; probe < SPP_SLOTS; probe++) {
                const uint32_t kk = key[h];
                if (kk == ps[k]) { pslot[k] = h; break; }
                if (kk == SPP_EMPTY) {
                    const uint32_t old = atomicCAS(&key[h], SPP_EMPTY, ps[k]);
                    if (old == SPP_EMPTY) { atomicAdd(&s_ndist, 1u); pslot[k] = h; break; }
                    if (old == ps[k]) { pslot[k] = h; break; }
                }
                h = (h + 1u) & (SPP_SLOTS - 1u);
            }
            if (pslot[k] < SPP_SLOTS) atomicAdd(&cnt[pslot[k]], 1u);
        }
        __syncthreads();
        const bool crowded = s_ndist > SPP_MAXDIST;          // (a pixel may then have found no slot at all)
        // ---- which labels are complete here; run offsets by a scan of their pixel counts (a band's run is at most
        //      that long, and one unused entry behind every run keeps runs of equal length off the same banks) ----
        uint32_t mine[4], msum = 0;
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) {
            const uint32_t sl = threadIdx.x * 4u + q;
            const uint32_t kk = key[sl], c = cnt[sl];
            uint32_t nv = 0;
            if (kk != SPP_EMPTY) {
                const bool complete = !crowded && c == tot[kk] && c <= SPP_MAXRUN;
                if (complete) { nv = c + 1u; clist[atomicAdd(&s_nc, 1u)] = (uint16_t)sl; }
                else flagged[kk] = 1;
                cnt[sl] = complete ? 0x80000000u : 0u;
            }
            mine[q] = nv;
            msum += nv;
        }
        spp_scan_offsets(mine, msum, s_wsum, offs);
        // ---- the pixels of every other label, nodata or not in whichever band: (label, position) into the list ----
        // (pslot[k] becomes 0x80000000 | the pixel's place among the patch's left-over ones)
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++) {
            if (ps[k] == 0u) continue;
            if (pslot[k] < SPP_SLOTS && (cnt[pslot[k]] & 0x80000000u)) continue;
            if (pslot[k] >= SPP_SLOTS) flagged[ps[k]] = 1;     // (crowded: no slot, so nobody flagged its label above)
            pslot[k] = 0x80000000u | atomicAdd(&s_left, 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0 && s_left) s_leftbase = atomicAdd(left_count, s_left);
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++)
            if (pslot[k] & 0x80000000u) {
                const uint32_t pl = k * 256u + threadIdx.x;
                const uint32_t li = s_leftbase + (pslot[k] & 0x7FFFFFFFu);
                left_seg[li] = ps[k];
                left_pos[li] = (y0 + pl / SPP_W) * ncols + x0 + (pl % SPP_W);
            }
    }
    // from here on pslot[k] < SPP_SLOTS says: a pixel of a label that is complete in this patch
    const size_t ns = (size_t)S + 1;
    const uint32_t nc = s_nc;
    for (int b = 0; b < nbands; b++) {
        const void *__restrict__ band = bands[b].band;
        const bool has_null = bands[b].has_null != 0;
        const long long null_val = bands[b].null_val;
        const uint32_t sh = (b & 1) ? 15u : 0u;                 // this band's half of cnt[]
        // ---- this band's values of complete labels into their runs ----
        // rpos[k]: the place in the label's run; 0xFFFFFFFF: not a member of a run
        uint32_t pv[SPP_PPT], rpos[SPP_PPT];
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++) {
            const uint32_t pl = k * 256u + threadIdx.x;
            rpos[k] = 0xFFFFFFFFu;
            pv[k] = 0u;
            if (pslot[k] < SPP_SLOTS) {                         // (inside the raster, then)
                const size_t p = (size_t)(y0 + pl / SPP_W) * ncols + x0 + (pl % SPP_W);
                const long long v = ld_t<DT>(band, p);
                pv[k] = (uint32_t)(v - bias);
                if (!(has_null && v == null_val)) rpos[k] = 0u;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++) {
            if (rpos[k] == 0xFFFFFFFFu) continue;
            const uint32_t sl = pslot[k];
            rpos[k] = (atomicAdd(&cnt[sl], 1u << sh) >> sh) & 0x7FFFu;
            runs[offs[sl] + rpos[k]] = narrow ? (pv[k] << 6) | rpos[k] : pv[k];
        }
        __syncthreads();
        // (the other half of cnt[] served the band before: nobody reads it now)
#pragma unroll
        for (uint32_t q = 0; q < 4u; q++) atomicAnd(&cnt[threadIdx.x * 4u + q], 0x80000000u | (0x7FFFu << sh));
        // ---- the runs sorted by RANK, as in k_stats_patch ----
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++) {
            if (rpos[k] == 0xFFFFFFFFu) continue;
            const uint32_t sl = pslot[k];
            const uint32_t n = (cnt[sl] >> sh) & 0x7FFFu, o = offs[sl];
            rpos[k] = o + spp_rank_in_run<narrow>(&runs[o], n, pv[k], rpos[k]);
        }
        __syncthreads();
#pragma unroll
        for (uint32_t k = 0; k < SPP_PPT; k++)
            if (rpos[k] != 0xFFFFFFFFu) runs[rpos[k]] = pv[k];
        __syncthreads();
        // ---- a thread per complete label, this band's statistics into this band's columns ----
        const uint32_t *bsel = sel + (size_t)bands[b].sel_first * 5;
        const int bnstats = bands[b].nstats;
        for (uint32_t ci = threadIdx.x; ci < nc; ci += 256u) {
            const uint32_t sl = clist[ci];
            const uint32_t n = (cnt[sl] >> sh) & 0x7FFFu;
            seg_stats_of_run(key[sl], n, &runs[offs[sl]], bias, bsel, bnstats, missing, intcols, fltcols, ns);
        }
        __syncthreads();                                        // (the next band overwrites runs[])
    }
}

// a band's (segment key, biased value) pairs of the left-over pixels; nodata pixels get key 0 as in k_stats_keys
__global__ __launch_bounds__(256) void k_stats_left_keys(const uint32_t *__restrict__ left_seg,
                                                         const uint32_t *__restrict__ left_pos,
                                                         const void *__restrict__ band, int dtype, uint32_t n,
                                                         int has_null, long long null_val, long long bias,
                                                         uint32_t *__restrict__ kseg, uint32_t *__restrict__ kval)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const long long v = ld_px(band, dtype, left_pos[i]);
    kseg[i] = (has_null && v == null_val) ? 0u : left_seg[i];
    kval[i] = (uint32_t)(v - bias);
}

// d_seg, bands_host[b] (device pointers): a row block of nrows x ncols pixels.  sel_host: the combined selection, nstats_per_band[b] consecutive rows for band b, column array indices
// running through all bands; the outputs are HOST arrays of all bands' columns.
// dev_int / dev_flt given: the columns stay in the context's workspace (ctx->ssum), nothing is copied to the host.
// allow_patches false: everything goes through the sorts whatever SHEPSEG_STATS_PATCH says (a 1 x m list of pairs
// has no patches worth the name).
static int run_segstats_bands(shp_ctx *ctx, const uint32_t *d_seg, const void *const *bands_host, int dtype, int nbands,
                              uint32_t nrows, uint32_t ncols, uint32_t S, const int *has_null, const int64_t *null_val,
                              const uint32_t *sel_host, const int *nstats_per_band, int64_t missing,
                              int64_t *intcols_out, float *fltcols_out, long long **dev_int = nullptr,
                              float **dev_flt = nullptr, bool allow_patches = true)
{
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    const uint32_t n = nrows * ncols;
    int nstats = 0;
    for (int b = 0; b < nbands; b++) {
        if (nstats_per_band[b] < 1 || !bands_host[b]) SHP_FAIL(ctx, SHP_ERR_ARG, "band entry %d: no statistics or no band", b);
        nstats += nstats_per_band[b];
    }
    int nint = 0, nflt = 0;
    CHK(stats_sel_check(ctx, sel_host, nstats, &nint, &nflt, true));
    const size_t sel_bytes = ((size_t)nstats * 20 + 31) & ~(size_t)31, tab_bytes = (size_t)nbands * sizeof(StatsBand);
    if (sel_bytes + tab_bytes + 1024 > SHP_PINNED_BYTES) SHP_FAIL(ctx, SHP_ERR_ARG, "too many statistics");
    long long bias;
    int valbits;
    stats_value_range(dtype, &bias, &valbits);
    CHK(stats_workspace(ctx, n, ns, 4096 + sel_bytes + tab_bytes, nint, nflt));
    uint32_t *kval = bp<uint32_t>(ctx->aux), *kseg = bp<uint32_t>(ctx->aux2);
    uint32_t *d_sel = bp<uint32_t>(ctx->small) + 256;
    StatsBand *d_tab = (StatsBand *)(bp<uint8_t>(ctx->small) + 1024 + sel_bytes);
    long long *d_int = (long long *)ctx->ssum.p;
    float *d_flt = (float *)(d_int + (size_t)nint * ns);
    HIPCHK(ctx, hipStreamSynchronize(st));
    uint8_t *pin = (uint8_t *)(ctx->h_pinned + 16);
    memcpy(pin, sel_host, (size_t)nstats * 20);
    StatsBand *tab = (StatsBand *)(pin + sel_bytes);
    for (int b = 0, first = 0; b < nbands; first += nstats_per_band[b], b++)
        tab[b] = StatsBand{bands_host[b], (long long)(has_null[b] ? null_val[b] : 0), has_null[b] ? 1 : 0, first,
                           nstats_per_band[b], 0};
    HIPCHK(ctx, hipMemcpyAsync(d_sel, pin, sel_bytes + tab_bytes, hipMemcpyHostToDevice, st));
    const int ps = prof_begin(ctx, PROF_SEGSTATS);
    const bool patches = stats_use_patches(n, S, allow_patches);
    if (patches) {
        CHK(buf_ensure(ctx, ctx->tcount, (ns + 1) * 4));
        CHK(buf_ensure(ctx, ctx->mergeto, ns + 64));
        CHK(buf_ensure(ctx, ctx->tlist, (size_t)n * 4));
        CHK(buf_ensure(ctx, ctx->tsorted, (size_t)n * 4));
        uint32_t *tot = bp<uint32_t>(ctx->tcount);
        uint8_t *flagged = bp<uint8_t>(ctx->mergeto);
        uint32_t *left_seg = bp<uint32_t>(ctx->tlist), *left_pos = bp<uint32_t>(ctx->tsorted);
        uint32_t *d_left = bp<uint32_t>(ctx->small);      // (word 0; the selection sits behind word 256)
        HIPCHK(ctx, hipMemsetAsync(tot, 0, ns * 4, st));
        HIPCHK(ctx, hipMemsetAsync(flagged, 0, ns, st));
        HIPCHK(ctx, hipMemsetAsync(d_left, 0, 4, st));
        const dim3 grid(grid_for(ncols, SPP_W), grid_for(nrows, SPP_H));
        hipLaunchKernelGGL(k_label_hist_patch, grid, dim3(256), 0, st, d_seg, nrows, ncols, S, tot); KCHK(ctx);
        hipLaunchKernelGGL(k_stats_prefill, dim3(grid_for(ns, 256)), dim3(256), 0, st, S, bias, d_sel, nstats,
                           (long long)missing, d_int, d_flt); KCHK(ctx);
        DISPATCH_DTYPE(dtype, hipLaunchKernelGGL(k_stats_patch_bands<DT>, grid, dim3(256), 0, st, d_seg, d_tab, nbands, nrows,
                                                 ncols, S, bias, tot, d_sel, (long long)missing, d_int, d_flt, flagged,
                                                 left_seg, left_pos, d_left));
        KCHK(ctx);
        uint32_t nleft = 0;
        CHK(read_u32(ctx, d_left, &nleft));
        if (nleft > n) SHP_FAIL(ctx, SHP_ERR_STATE, "%u left-over pixels of %u", nleft, n);
        for (int b = 0, first = 0; nleft && b < nbands; first += nstats_per_band[b], b++) {
            hipLaunchKernelGGL(k_stats_left_keys, dim3(grid_for(nleft, 256)), dim3(256), 0, st, left_seg, left_pos,
                               bands_host[b], dtype, nleft, has_null[b] ? 1 : 0, (long long)(has_null[b] ? null_val[b] : 0), bias, kseg,
                               kval); KCHK(ctx);
            CHK(segstats_sort_reduce(ctx, nleft, S, valbits, bias, d_sel + (size_t)first * 5, nstats_per_band[b], missing,
                                     d_int, d_flt, flagged));
        }
    } else {
        for (int b = 0, first = 0; b < nbands; first += nstats_per_band[b], b++) {
            if (n) {
                hipLaunchKernelGGL(k_stats_keys, dim3(grid_for(n, 256)), dim3(256), 0, st, d_seg, bands_host[b], dtype, n, S,
                                   has_null[b] ? 1 : 0, (long long)(has_null[b] ? null_val[b] : 0), bias, kseg, kval);
                KCHK(ctx);
            }
            CHK(segstats_sort_reduce(ctx, n, S, valbits, bias, d_sel + (size_t)first * 5, nstats_per_band[b], missing,
                                     d_int, d_flt, nullptr));
        }
    }
    prof_end(ctx, ps);
    if (dev_int) { *dev_int = d_int; *dev_flt = d_flt; return 0; }
    return segstats_download(ctx, intcols_out, d_int, (size_t)nint * ns * 8, fltcols_out, d_flt, (size_t)nflt * ns * 4);
}

// ---- multi-GPU split: the pixels of segments that straddle a rank boundary ------------------
// (seg id, band value) of every pixel whose segment is flagged, compacted (any order) with one
// global atomic per 4096 pixels.  count may exceed cap: only the first cap pairs are stored.
// The workgroup's 4096 pixels: the positions of those whose segment is flagged, compacted into s_buf (*s_cnt of them),
// and room for them reserved in the output from *s_base on, with one global atomic.
__device__ __forceinline__ void gather_flagged_positions(const uint32_t *__restrict__ seg, uint32_t n, uint32_t S,
                                                         const uint8_t *__restrict__ flags, uint32_t *count,
                                                         uint32_t *s_buf, uint32_t *s_cnt, uint32_t *s_base)
{
    if (threadIdx.x == 0) *s_cnt = 0;
    __syncthreads();
    const unsigned lane = lane_id();
    for (uint32_t it = 0; it < 16u; it++) {
        const uint32_t p = blockIdx.x * 4096u + it * 256u + threadIdx.x;
        bool take = false;
        if (p < n) {
            const uint32_t sg = seg[p];
            take = sg != 0u && sg <= S && flags[sg] != 0;
        }
        const unsigned long long m = __ballot(take);
        if (m != 0ull) {
            uint32_t wbase = 0;
            if (lane == 0) wbase = atomicAdd(s_cnt, (uint32_t)__popcll(m));
            wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
            if (take) s_buf[wbase + (uint32_t)__popcll(m & lanemask_lt())] = p;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) *s_base = *s_cnt ? atomicAdd(count, *s_cnt) : 0u;
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_gather_flagged(const uint32_t *__restrict__ seg,
                                                        const void *__restrict__ band, int dtype,
                                                        uint32_t n, uint32_t S,
                                                        const uint8_t *__restrict__ flags,
                                                        uint32_t *__restrict__ out_seg,
                                                        long long *__restrict__ out_val,
                                                        uint32_t cap, uint32_t *count)
{
    __shared__ uint32_t s_buf[4096];
    __shared__ uint32_t s_cnt, s_base;
    gather_flagged_positions(seg, n, S, flags, count, s_buf, &s_cnt, &s_base);
    for (uint32_t i = threadIdx.x; i < s_cnt; i += 256u) {
        const uint32_t o = s_base + i;
        if (o < cap) {
            const uint32_t p = s_buf[i];
            out_seg[o] = seg[p];
            out_val[o] = ld_px(band, dtype, p);
        }
    }
}

// The two gather drivers' device side: ctx->small = the count (word 0) | tab_bytes for the caller's band table (from
// byte 64) | the flags, uploaded here; ctx->aux = the ids, ctx->aux2 = val_rows rows of cap values.
static int gather_flagged_begin(shp_ctx *ctx, uint32_t S, const uint8_t *flags_host, uint32_t cap, int val_rows,
                                size_t tab_bytes, uint8_t **d_flags)
{
    const size_t ns = (size_t)S + 1;
    CHK(buf_ensure(ctx, ctx->small, 64 + tab_bytes + ns + 64));
    CHK(buf_ensure(ctx, ctx->aux, (size_t)cap * 4 + 64));
    CHK(buf_ensure(ctx, ctx->aux2, (size_t)cap * 8 * val_rows + 64));
    *d_flags = bp<uint8_t>(ctx->small) + 64 + tab_bytes;
    HIPCHK(ctx, hipMemcpyAsync(*d_flags, flags_host, ns, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->small.p, 0, 4, ctx->stream));
    return 0;
}

// ... and the way back: the count, and the first min(count, cap) pairs (of several rows of values all cap columns
// travel: the rows lie cap apart)
static int gather_flagged_end(shp_ctx *ctx, uint32_t cap, int val_rows, uint32_t *seg_out, int64_t *val_out,
                              int64_t *count_out)
{
    hipStream_t st = ctx->stream;
    uint32_t cnt = 0;
    CHK(read_u32(ctx, bp<uint32_t>(ctx->small), &cnt));
    const uint32_t take = cnt < cap ? cnt : cap;
    if (take) {
        const size_t nval = val_rows == 1 ? (size_t)take : (size_t)cap * val_rows;
        HIPCHK(ctx, hipMemcpyAsync(seg_out, ctx->aux.p, (size_t)take * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(val_out, ctx->aux2.p, nval * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    *count_out = (int64_t)cnt;
    return 0;
}

static int run_gather_flagged(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                              uint32_t n, uint32_t S, const uint8_t *flags_host, uint32_t cap,
                              uint32_t *seg_out, int64_t *val_out, int64_t *count_out)
{
    uint8_t *d_flags = nullptr;
    CHK(gather_flagged_begin(ctx, S, flags_host, cap, 1, 0, &d_flags));
    uint32_t *d_count = bp<uint32_t>(ctx->small);
    if (n) {
        hipLaunchKernelGGL(k_gather_flagged, dim3(grid_for(n, 4096)), dim3(256), 0, ctx->stream, d_seg, d_band, dtype,
                           n, S, d_flags, bp<uint32_t>(ctx->aux), (long long *)ctx->aux2.p, cap, d_count);
        KCHK(ctx);
    }
    return gather_flagged_end(ctx, cap, 1, seg_out, val_out, count_out);
}

// The same for several bands of one image: the ids once, and every band's values in the SAME order (the order itself
// is again arbitrary) -- out_val: nbands rows of cap values.
__global__ __launch_bounds__(256) void k_gather_flagged_bands(const uint32_t *__restrict__ seg,
                                                              const StatsBand *__restrict__ bands, int nbands, int dtype,
                                                              uint32_t n, uint32_t S, const uint8_t *__restrict__ flags,
                                                              uint32_t *__restrict__ out_seg,
                                                              long long *__restrict__ out_val, uint32_t cap,
                                                              uint32_t *count)
{
    __shared__ uint32_t s_buf[4096];
    __shared__ uint32_t s_cnt, s_base;
    gather_flagged_positions(seg, n, S, flags, count, s_buf, &s_cnt, &s_base);
    for (uint32_t i = threadIdx.x; i < s_cnt; i += 256u) {
        const uint32_t o = s_base + i;
        if (o < cap) {
            const uint32_t p = s_buf[i];
            out_seg[o] = seg[p];
            for (int b = 0; b < nbands; b++) out_val[(size_t)b * cap + o] = ld_px(bands[b].band, dtype, p);
        }
    }
}

static int run_gather_flagged_bands(shp_ctx *ctx, const uint32_t *d_seg, const void *const *bands_host, int dtype,
                                    int nbands, uint32_t n, uint32_t S, const uint8_t *flags_host, uint32_t cap,
                                    uint32_t *seg_out, int64_t *val_out, int64_t *count_out)
{
    hipStream_t st = ctx->stream;
    const size_t tab_bytes = (size_t)nbands * sizeof(StatsBand);
    if (tab_bytes + 1024 > SHP_PINNED_BYTES) SHP_FAIL(ctx, SHP_ERR_ARG, "too many bands");
    uint8_t *d_flags = nullptr;
    CHK(gather_flagged_begin(ctx, S, flags_host, cap, nbands, tab_bytes, &d_flags));
    uint32_t *d_count = bp<uint32_t>(ctx->small);
    StatsBand *d_tab = (StatsBand *)(bp<uint8_t>(ctx->small) + 64);
    HIPCHK(ctx, hipStreamSynchronize(st));
    StatsBand *tab = (StatsBand *)(ctx->h_pinned + 16);
    for (int b = 0; b < nbands; b++) {
        if (!bands_host[b]) SHP_FAIL(ctx, SHP_ERR_ARG, "band entry %d: no band", b);
        tab[b] = StatsBand{bands_host[b], 0, 0, 0, 0, 0};
    }
    HIPCHK(ctx, hipMemcpyAsync(d_tab, tab, tab_bytes, hipMemcpyHostToDevice, st));
    if (n) {
        hipLaunchKernelGGL(k_gather_flagged_bands, dim3(grid_for(n, 4096)), dim3(256), 0, st, d_seg, d_tab, nbands, dtype,
                           n, S, d_flags, bp<uint32_t>(ctx->aux), (long long *)ctx->aux2.p, cap, d_count);
        KCHK(ctx);
    }
    return gather_flagged_end(ctx, cap, nbands, seg_out, val_out, count_out);
}

// ---- multi-GPU split, device-resident (distributed.calcPerSegmentStatsDistributedBands) --------
// Rank-local part.  The statistics of this rank's rows are computed as on one GPU; then every id is
// classified against the global histogram (the reference's segSize, tilingstats.py:165): a segment whose
// local pixel count equals it is complete here and its row is final (checkSegComplete, :518-553); a segment
// with fewer is a straddler -- its row is cleared and its pixels are packed, the id and every plane's value, for
// the exchange; ids nobody holds (global count 0, row 0 among them) keep their "missing" row on the rank that is
// told to (keep_unheld), so that the columns of all ranks ADD UP to the single-GPU columns.  An id with MORE
// pixels here than the histogram gives it in the whole raster would count as complete nowhere and straddling
// nowhere, and its row would be cleared silently: the sign of a histogram that belongs to other labels.
// cols: nint int64 columns then nflt float columns of S + 1 rows, in device memory of the caller.
__global__ __launch_bounds__(256) void k_dstats_classify(const uint32_t *__restrict__ lh,
                                                         const uint32_t *__restrict__ gh, uint32_t S,
                                                         int keep_unheld, int nint, int nflt,
                                                         const long long *__restrict__ src_int,
                                                         const float *__restrict__ src_flt,
                                                         long long *__restrict__ dst_int,
                                                         float *__restrict__ dst_flt,
                                                         uint8_t *__restrict__ flags,
                                                         unsigned long long *counters)
{
    const size_t ns = (size_t)S + 1;
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
    bool strad = false, stale = false;
    uint32_t l = 0;
    if (id < ns) {
        l = id == 0 ? 0u : lh[id];
        const uint32_t g = id == 0 ? 0u : gh[id];
        strad = l > 0u && l < g;
        stale = l > g;
        const bool keep = (l > 0u && l == g) || (keep_unheld && g == 0u);
        flags[id] = strad ? 1 : 0;
        for (int c = 0; c < nint; c++) dst_int[(size_t)c * ns + id] = keep ? src_int[(size_t)c * ns + id] : 0ll;
        for (int c = 0; c < nflt; c++) dst_flt[(size_t)c * ns + id] = keep ? src_flt[(size_t)c * ns + id] : 0.0f;
    }
    // counters[0] += pixels of straddlers, counters[1] += straddling segments (one atomic pair per wavefront)
    const unsigned long long m = __ballot(strad);
    if (m != 0ull) {
        unsigned long long px = strad ? (unsigned long long)l : 0ull;
        for (int o = 32; o > 0; o >>= 1) px += __shfl_xor(px, o);
        if (lane_id() == 0) { atomicAdd(&counters[0], px); atomicAdd(&counters[1], (unsigned long long)__popcll(m)); }
    }
    // counters[2] += ids with more pixels here than the histogram gives them
    const unsigned long long ms = __ballot(stale);
    if (ms != 0ull && lane_id() == 0) atomicAdd(&counters[2], (unsigned long long)__popcll(ms));
}

// The rows of the ids that occur among the pairs a rank has reduced (present[id] != 0) go into cols: every rank's
// classify step cleared them.  *n_ids += how many.
__global__ __launch_bounds__(256) void k_dstats_take(const uint32_t *__restrict__ present, uint32_t S, int nint, int nflt,
                                                     const long long *__restrict__ src_int, const float *__restrict__ src_flt,
                                                     long long *__restrict__ dst_int, float *__restrict__ dst_flt,
                                                     uint32_t *n_ids)
{
    const size_t ns = (size_t)S + 1;
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
    const bool here = id != 0 && id < ns && present[id] != 0u;
    const unsigned long long m = __ballot(here);
    if (m != 0ull && lane_id() == 0) atomicAdd(n_ids, (uint32_t)__popcll(m));
    if (!here) return;
    for (int c = 0; c < nint; c++) dst_int[(size_t)c * ns + id] = src_int[(size_t)c * ns + id];
    for (int c = 0; c < nflt; c++) dst_flt[(size_t)c * ns + id] = src_flt[(size_t)c * ns + id];
}

// ---- the split's two drivers, over entries (one entry is no special route: nbands = nplanes = 1) ------------------
// "band" = an entry of the caller's bandSelections (a plane, a null value, some statistics), "plane" = a distinct
// image band; plane_of_band[e] says which plane entry e reads.  Everything that depends on the labels alone -- the
// local label histogram, the classification against the global one, the straddlers' ids on the wire, the pick of
// this rank's id share, the `present` histogram -- is done once whatever the number of entries, and the straddlers'
// values travel in the planes' own pixel type: 4 + nplanes * itemsize bytes per straddler pixel.
// Values travel RAW, nulls included: a null value belongs to an entry, and two entries may read one plane with
// different ones, so it is applied where the statistics are computed (k_stats_keys at the merge).

// rows of values lie this many bytes apart (16-byte aligned, so that every plane's row can be copied and read
// with wide accesses whatever the count)
static inline size_t dstats_row_bytes(size_t count, int dtype) { return (count * dtype_size(dtype) + 15) & ~(size_t)15; }

// k_gather_flagged_bands with the values left in the planes' pixel type T (only its width matters: nothing is
// computed here): the id once, and row b of out_val = plane b's raw values, rows row_bytes apart.
template <typename T>
__global__ __launch_bounds__(256) void k_gather_flagged_planes(const uint32_t *__restrict__ seg,
                                                               const StatsBand *__restrict__ planes, int nplanes,
                                                               uint32_t n, uint32_t S, const uint8_t *__restrict__ flags,
                                                               uint32_t *__restrict__ out_seg,
                                                               uint8_t *__restrict__ out_val, size_t row_bytes,
                                                               uint32_t cap, uint32_t *count)
{
    __shared__ uint32_t s_buf[4096];
    __shared__ uint32_t s_cnt, s_base;
    gather_flagged_positions(seg, n, S, flags, count, s_buf, &s_cnt, &s_base);
    for (uint32_t i = threadIdx.x; i < s_cnt; i += 256u) {
        const uint32_t o = s_base + i;
        if (o < cap) {
            const uint32_t p = s_buf[i];
            out_seg[o] = seg[p];
            for (int b = 0; b < nplanes; b++)
                ((T *)(out_val + (size_t)b * row_bytes))[o] = ((const T *)planes[b].band)[p];
        }
    }
}

// The statistics of the entries over nrows x ncols labels, the columns left in ctx->ssum (*di, *df).  The only place
// in the split that knows "one or several": one entry goes through run_segstats, whose k_stats_patch is faster for
// one band than k_stats_patch_bands (both give a row the same bits), several through run_segstats_bands.
// allow_patches false (the merge's 1 x m list of pairs): everything goes through the sorts, which run_segstats does
// when it is not told the shape.
static int dstats_segstats(shp_ctx *ctx, const uint32_t *d_seg, const void *const *bands_host, int dtype, int nbands,
                           uint32_t nrows, uint32_t ncols, uint32_t S, const int *has_null, const int64_t *null_val,
                           const uint32_t *sel_host, const int *nstats_per_band, int64_t missing, bool allow_patches,
                           long long **di, float **df)
{
    if (nbands != 1)
        return run_segstats_bands(ctx, d_seg, bands_host, dtype, nbands, nrows, ncols, S, has_null, null_val, sel_host,
                                  nstats_per_band, missing, nullptr, nullptr, di, df, allow_patches);
    if (nstats_per_band[0] < 1 || !bands_host[0]) SHP_FAIL(ctx, SHP_ERR_ARG, "band entry 0: no statistics or no band");
    return run_segstats(ctx, d_seg, bands_host[0], dtype, nrows * ncols, S, has_null[0] ? 1 : 0,
                        has_null[0] ? null_val[0] : 0, sel_host, nstats_per_band[0], missing, nullptr, nullptr,
                        allow_patches ? nrows : 0u, allow_patches ? ncols : 0u, di, df);
}

// Local part.  planes_host: nplanes device pointers (this rank's rows of the distinct planes).  The pairs end up in
// ctx->aux (cap ids) and ctx->aux2 (nplanes rows of cap values of the pixel type, dstats_row_bytes(cap) apart): both
// hold the sort keys of the statistics (run_segstats and run_segstats_bands alike: stats_workspace) until those are
// done, so they are sized for the pairs only AFTER the classify kernel has read the columns out of ctx->ssum into
// d_cols (nothing between the statistics and that kernel touches ssum, aux or aux2), and the pairs stay valid until
// the context's next call.
static int run_dstats_local_bands(shp_ctx *ctx, const uint32_t *d_seg, const void *const *planes_host, int nplanes,
                                  const int *plane_of_band, int dtype, int nbands, uint32_t nrows, uint32_t ncols,
                                  uint32_t S, const int *has_null, const int64_t *null_val, const uint32_t *sel_host,
                                  const int *nstats_per_band, int64_t missing, const uint32_t *d_hist, int keep_unheld,
                                  void *d_cols, uint32_t **d_pair_seg, void **d_pair_val, int64_t *pair_row_bytes,
                                  int64_t *n_pairs, int64_t *n_strad)
{
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    const uint32_t n = nrows * ncols;
    int nstats = 0;
    std::vector<const void *> bands((size_t)nbands);
    for (int b = 0; b < nbands; b++) {
        if (plane_of_band[b] < 0 || plane_of_band[b] >= nplanes) SHP_FAIL(ctx, SHP_ERR_ARG, "band entry %d: no such plane", b);
        bands[(size_t)b] = planes_host[plane_of_band[b]];
        nstats += nstats_per_band[b] > 0 ? nstats_per_band[b] : 0;
    }
    const size_t tab_bytes = (size_t)nplanes * sizeof(StatsBand);
    if (tab_bytes + 1024 > SHP_PINNED_BYTES) SHP_FAIL(ctx, SHP_ERR_ARG, "too many bands");
    long long *di = nullptr;
    float *df = nullptr;
    CHK(dstats_segstats(ctx, d_seg, bands.data(), dtype, nbands, nrows, ncols, S, has_null, null_val, sel_host,
                        nstats_per_band, missing, true, &di, &df));
    int nint = 0, nflt = 0;
    CHK(stats_sel_check(ctx, sel_host, nstats, &nint, &nflt, true));
    // the local label histogram (all pixels of a label, valid or not) | counters, the planes' table, flags
    CHK(buf_ensure(ctx, ctx->chnext, ns * 4 + 64));
    CHK(buf_ensure(ctx, ctx->chtail, 64 + tab_bytes + ns + 64));
    uint32_t *lh = bp<uint32_t>(ctx->chnext);
    unsigned long long *ctr = (unsigned long long *)bp<uint8_t>(ctx->chtail);     // [0] pixels [1] segments [2] stale ids
    StatsBand *d_tab = (StatsBand *)(bp<uint8_t>(ctx->chtail) + 64);
    uint8_t *flags = bp<uint8_t>(ctx->chtail) + 64 + tab_bytes;
    HIPCHK(ctx, hipMemsetAsync(lh, 0, ns * 4, st));
    HIPCHK(ctx, hipMemsetAsync(ctr, 0, 64, st));
    if (n) { hipLaunchKernelGGL(k_label_hist, dim3(grid_for(n, 256)), dim3(256), 0, st, d_seg, n, S, lh); KCHK(ctx); }
    hipLaunchKernelGGL(k_dstats_classify, dim3(grid_for(ns, 256)), dim3(256), 0, st, lh, d_hist, S, keep_unheld, nint, nflt,
                       di, df, (long long *)d_cols, (float *)((long long *)d_cols + (size_t)nint * ns), flags, ctr); KCHK(ctx);
    unsigned long long h[3] = {0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h, ctr, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (h[2] != 0ull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "%llu segment ids have more pixels in these rows than the histogram gives them in the "
                 "whole raster: the histogram does not belong to these labels", h[2]);
    if (h[0] >= 0xffffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "too many straddling pixels (%llu)", h[0]);
    const uint32_t cap = (uint32_t)h[0];
    const size_t row_bytes = dstats_row_bytes(cap, dtype);
    // (the statistics are done with aux / aux2, and the columns have left ssum: see above)
    CHK(buf_ensure(ctx, ctx->aux, (size_t)cap * 4 + 64));
    CHK(buf_ensure(ctx, ctx->aux2, (size_t)nplanes * row_bytes + 64));
    uint32_t *d_count = (uint32_t *)(ctr + 4);
    if (n && cap) {
        StatsBand *tab = (StatsBand *)(ctx->h_pinned + 16);
        for (int b = 0; b < nplanes; b++) tab[b] = StatsBand{planes_host[b], 0, 0, 0, 0, 0};
        HIPCHK(ctx, hipMemcpyAsync(d_tab, tab, tab_bytes, hipMemcpyHostToDevice, st));
        uint8_t *out_val = bp<uint8_t>(ctx->aux2);
        const dim3 grid(grid_for(n, 4096));
        switch (dtype_size(dtype)) {
        case 1: hipLaunchKernelGGL(k_gather_flagged_planes<uint8_t>, grid, dim3(256), 0, st, d_seg, d_tab, nplanes, n, S, flags,
                                   bp<uint32_t>(ctx->aux), out_val, row_bytes, cap, d_count); break;
        case 2: hipLaunchKernelGGL(k_gather_flagged_planes<uint16_t>, grid, dim3(256), 0, st, d_seg, d_tab, nplanes, n, S, flags,
                                   bp<uint32_t>(ctx->aux), out_val, row_bytes, cap, d_count); break;
        default: hipLaunchKernelGGL(k_gather_flagged_planes<uint32_t>, grid, dim3(256), 0, st, d_seg, d_tab, nplanes, n, S, flags,
                                    bp<uint32_t>(ctx->aux), out_val, row_bytes, cap, d_count); break;
        }
        KCHK(ctx);
        uint32_t got = 0;
        CHK(read_u32(ctx, d_count, &got));
        if (got != cap) SHP_FAIL(ctx, SHP_ERR_STATE, "straddler gather found %u pixels, the histogram says %u", got, cap);
    }
    *d_pair_seg = bp<uint32_t>(ctx->aux);
    *d_pair_val = ctx->aux2.p;
    *pair_row_bytes = (int64_t)row_bytes;
    *n_pairs = (int64_t)cap;
    *n_strad = (int64_t)h[1];
    return 0;
}

// Merge part.  pseg: `world` slots of `slot` ids; pval: `world` blocks of nplanes rows, rows slot_row_bytes apart
// (the same on every rank), counts[r] pairs valid in slot r.  A pair whose id lies in [id_lo, id_hi) takes ONE
// output position (ballot + one atomic per wavefront) and its id and all planes' values go there, so that the planes
// stay aligned with the ids; out_val: nplanes rows, out_row_bytes apart.
template <typename T>
__global__ __launch_bounds__(256) void k_dstats_pick_planes(const uint32_t *__restrict__ pseg,
                                                            const uint8_t *__restrict__ pval, uint32_t slot,
                                                            uint32_t world, size_t slot_row_bytes, int nplanes,
                                                            const uint32_t *__restrict__ counts, uint32_t id_lo,
                                                            uint32_t id_hi, uint32_t *__restrict__ out_seg,
                                                            uint8_t *__restrict__ out_val, size_t out_row_bytes,
                                                            uint32_t *count)
{
    const size_t q = (size_t)blockIdx.x * 256u + threadIdx.x;
    bool take = false;
    uint32_t sg = 0, r = 0, e = 0;
    if (q < (size_t)slot * world) {
        r = (uint32_t)(q / slot);
        e = (uint32_t)(q - (size_t)r * slot);
        if (e < counts[r]) { sg = pseg[q]; take = sg >= id_lo && sg < id_hi; }
    }
    const unsigned long long m = __ballot(take);
    if (m == 0ull) return;
    uint32_t base = 0;
    if (lane_id() == 0) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    if (take) {
        const uint32_t o = base + (uint32_t)__popcll(m & lanemask_lt());
        out_seg[o] = sg;
        const uint8_t *src = pval + (size_t)r * (size_t)nplanes * slot_row_bytes;
        for (int b = 0; b < nplanes; b++)
            ((T *)(out_val + (size_t)b * out_row_bytes))[o] = ((const T *)(src + (size_t)b * slot_row_bytes))[e];
    }
}

static int run_dstats_merge_bands(shp_ctx *ctx, const uint32_t *d_pseg, const void *d_pval, uint32_t slot,
                                  size_t slot_row_bytes, uint32_t world, const uint32_t *counts_host, int dtype,
                                  int nbands, int nplanes, const int *plane_of_band, uint32_t S, const int *has_null,
                                  const int64_t *null_val, const uint32_t *sel_host, const int *nstats_per_band,
                                  int64_t missing, uint32_t id_lo, uint32_t id_hi, void *d_cols, int64_t *n_merged,
                                  int64_t *n_ids)
{
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    int nstats = 0;
    for (int b = 0; b < nbands; b++) {
        if (plane_of_band[b] < 0 || plane_of_band[b] >= nplanes) SHP_FAIL(ctx, SHP_ERR_ARG, "band entry %d: no such plane", b);
        if (nstats_per_band[b] < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "band entry %d: no statistics", b);
        nstats += nstats_per_band[b];
    }
    int nint = 0, nflt = 0;
    CHK(stats_sel_check(ctx, sel_host, nstats, &nint, &nflt, true));
    *n_merged = 0;
    *n_ids = 0;
    const size_t total = (size_t)slot * world;
    if (total == 0 || id_lo >= id_hi) return 0;
    if (total >= 0xffffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "too many gathered pairs");
    if (slot_row_bytes < (size_t)slot * dtype_size(dtype)) SHP_FAIL(ctx, SHP_ERR_ARG, "the values' rows overlap");
    const size_t out_row_bytes = dstats_row_bytes(total, dtype);
    CHK(buf_ensure(ctx, ctx->lab, total * 4 + 64));
    CHK(buf_ensure(ctx, ctx->img, (size_t)nplanes * out_row_bytes + 64));
    CHK(buf_ensure(ctx, ctx->chtail, (size_t)world * 4 + 128));
    uint32_t *d_counts = bp<uint32_t>(ctx->chtail) + 16, *d_n = bp<uint32_t>(ctx->chtail);
    HIPCHK(ctx, hipStreamSynchronize(st));
    HIPCHK(ctx, hipMemcpyAsync(d_counts, counts_host, (size_t)world * 4, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemsetAsync(d_n, 0, 4, st));
    {
        const dim3 grid(grid_for(total, 256));
        uint32_t *out_seg = bp<uint32_t>(ctx->lab);
        uint8_t *out_val = bp<uint8_t>(ctx->img);
        const uint8_t *pval = (const uint8_t *)d_pval;
        switch (dtype_size(dtype)) {
        case 1: hipLaunchKernelGGL(k_dstats_pick_planes<uint8_t>, grid, dim3(256), 0, st, d_pseg, pval, slot, world,
                                   slot_row_bytes, nplanes, d_counts, id_lo, id_hi, out_seg, out_val, out_row_bytes, d_n); break;
        case 2: hipLaunchKernelGGL(k_dstats_pick_planes<uint16_t>, grid, dim3(256), 0, st, d_pseg, pval, slot, world,
                                   slot_row_bytes, nplanes, d_counts, id_lo, id_hi, out_seg, out_val, out_row_bytes, d_n); break;
        default: hipLaunchKernelGGL(k_dstats_pick_planes<uint32_t>, grid, dim3(256), 0, st, d_pseg, pval, slot, world,
                                    slot_row_bytes, nplanes, d_counts, id_lo, id_hi, out_seg, out_val, out_row_bytes, d_n); break;
        }
        KCHK(ctx);
    }
    uint32_t m = 0;
    CHK(read_u32(ctx, d_n, &m));
    *n_merged = (int64_t)m;
    if (m == 0) return 0;
    if ((size_t)m > total) SHP_FAIL(ctx, SHP_ERR_STATE, "%u pairs picked of %zu", m, total);
    std::vector<const void *> bands((size_t)nbands);
    for (int b = 0; b < nbands; b++) bands[(size_t)b] = bp<uint8_t>(ctx->img) + (size_t)plane_of_band[b] * out_row_bytes;
    long long *di = nullptr;
    float *df = nullptr;
    CHK(dstats_segstats(ctx, bp<uint32_t>(ctx->lab), bands.data(), dtype, nbands, 1u, m, S, has_null, null_val, sel_host,
                        nstats_per_band, missing, false, &di, &df));
    CHK(buf_ensure(ctx, ctx->chnext, ns * 4 + 64));
    uint32_t *present = bp<uint32_t>(ctx->chnext);
    HIPCHK(ctx, hipMemsetAsync(present, 0, ns * 4, st));
    hipLaunchKernelGGL(k_label_hist, dim3(grid_for(m, 256)), dim3(256), 0, st, bp<uint32_t>(ctx->lab), m, S, present); KCHK(ctx);
    HIPCHK(ctx, hipMemsetAsync(d_n, 0, 4, st));
    hipLaunchKernelGGL(k_dstats_take, dim3(grid_for(ns, 256)), dim3(256), 0, st, present, S, nint, nflt, di, df,
                       (long long *)d_cols, (float *)((long long *)d_cols + (size_t)nint * ns), d_n); KCHK(ctx);
    uint32_t ids = 0;
    CHK(read_u32(ctx, d_n, &ids));
    *n_ids = (int64_t)ids;
    return 0;
}
