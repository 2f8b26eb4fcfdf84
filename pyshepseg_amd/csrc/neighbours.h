// neighbours.h -- which segments touch which, and along how many pixel pairs: the CSR segment-adjacency table of a
// label raster (neighbours.findSegmentNeighbours).
//
// Two pixels are adjacent when one is the E or S neighbour of the other (and SE / SW with 8-connectivity); every
// adjacent pair with labels a != b, both non-zero, adds 1 to the border length of (a, b) and of (b, a).  All of it
// is integer work, so neither the atomics nor the order of the records below can change a result.
//
// The labels come in row blocks (a block may be followed by one more row: only pairs whose UPPER pixel lies in the
// block count, so a pair across two blocks counts once).  Three steps:
//  1. k_nbr_patch: one workgroup per 32 x 64 patch (k_stats_patch's patches) plus its one-pixel rim.  A differing
//     pair is canonicalised to (min, max) and counted in an LDS hash table; the patch then appends its DISTINCT pairs
//     with their counts to the record buffer (16 bytes each, one vector store).  With ~32-pixel segments this turns
//     ~1400 differing pairs of a patch into ~300 records.  Lanes of a wavefront that hold the same pair next to each
//     other (a straight border, stripes) add once, with the run's length, so a hot pair costs one LDS atomic per
//     row and not 64 on one address; a hot SEGMENT (a background that is half of every pair) spreads over the table
//     by its partners.  A patch with more distinct pairs than the table has slots takes the overflow route: an
//     insertion gives up after one trip round the table (that happens if and only if the patch holds more than
//     NBR_SLOTS distinct pairs, whatever the order of arrival), and the patch then appends every run as a record of
//     its own, the table unused.
//     The record buffer grows between blocks: every patch reserves its records with one atomic add and stores only
//     what fits; when a block did not fit, the reserved total is exactly what it needs, the buffer is regrown
//     (records of earlier blocks kept) and the block runs again.  Device memory is bounded by records.
//  2. nbr_sort_reduce: the records are sorted by the 64-bit key (a, b) -- two stable passes of sort.h's 32-bit sort,
//     by b then by a, over the significant bits of the largest label -- and run-length reduced with 64-bit sums.  A
//     template over the width of the count a record carries: 32 bits here (what the patch kernel wrote), 64 bits
//     where the records are sums already (dneighbours.h, dnbrmerge.h).
//  3. nbr_build_csr.  Row r holds its neighbours below r (reduced pairs (a, r)), then those above ((r, b)).  The
//     second part lies in the reduced order already; the first is the reduced pairs in a stable sort by b, which keeps
//     the a's ascending.  The degree of both ends is counted (runs of one id add once), scanned, and both parts are
//     filled: every row ascending.  A template over whole table / id share: the share table of dneighbours.h is the
//     same build over the rows [id_lo, id_hi), the one-GPU table is the share [0, S + 1) and reads neither the range
//     nor the shares' entry offsets.
// The table itself is an NbrTable (common.h): shp_ctx::nbr_tab here, shp_ctx::dnbr_tab for a rank's share.  Download
// and the copy half of an upload (nbr_table_download, nbr_table_upload_arrays) serve both.
#pragma once
#include "common.h"
#include "scan.h"
#include "sort.h"
#include <atomic>

#define NBR_PH 32u              // patch rows (8 per wavefront)
#define NBR_PW 64u              // patch columns: a wavefront per image row
#ifndef NBR_SLOTS
#define NBR_SLOTS 1024u         // hash slots per patch (a power of two): 12 KiB of LDS
#endif
#define NBR_TW 66u              // tile columns: the patch and a rim column on either side
#define NBR_MAX_REC 0x7fffffffull

static_assert((NBR_SLOTS & (NBR_SLOTS - 1u)) == 0u && NBR_SLOTS >= 256u, "NBR_SLOTS must be a power of two");

// device words of an accumulation (ctx->nbr_ctr): [0] records reserved, [1] differing pixel pairs met,
// [2] largest label seen (low word), [3] records dropped for want of room (a bug if ever non-zero after a block that fit)
enum { NBR_C_REC = 0, NBR_C_PAIRS = 1, NBR_C_MAXLAB = 2, NBR_C_WORDS = 4 };

struct NbrGeom {
    const uint32_t *seg;
    uint32_t nrows;             // rows of the block
    uint32_t avail;             // rows that may be read: nrows, + 1 when the block is followed by another row
    uint32_t ncols;
    uint32_t pcols;             // patches per patch row
    int eight;
};

__device__ __forceinline__ uint32_t nbr_hash(uint32_t a, uint32_t b)
{
    uint32_t h = a * 0x9E3779B1u ^ b * 0x85EBCA6Bu;
    h ^= h >> 15;
    return (h * 2654435761u) >> 16;
}

// The differing pairs of the patch's rows, a wavefront row and a direction at a time.  Lanes that hold the same
// pair side by side form a run; the run's first lane acts for it: DIRECT = false counts the run in the hash table
// (*over is set when a pair found no slot) and adds the wavefront's runs and pairs to *nrun / *npair, DIRECT = true
// appends the run to the records (at most `room` of them, from rec[base]).
template <bool DIRECT>
__device__ __forceinline__ void nbr_rows(const NbrGeom &g, uint32_t y0, const uint32_t (*tile)[NBR_TW],
                                         unsigned long long *hkey, uint32_t *hcnt, uint32_t *ndist, volatile uint32_t *over,
                                         uint32_t *nrun, uint32_t *npair, uint32_t *spos, uint4 *rec,
                                         unsigned long long base, unsigned long long cap, uint32_t room)
{
    const unsigned w = threadIdx.x >> 6, lane = lane_id();
    const int ndir = g.eight ? 4 : 2;
    uint32_t runs = 0, pairs = 0;
    for (unsigned rr = 0; rr < NBR_PH / 4u; rr++) {
        const unsigned r = w * (NBR_PH / 4u) + rr;
        if (y0 + r >= g.nrows) break;                   // (uniform in the wavefront)
        const uint32_t c0 = tile[r][lane + 1u];
        for (int d = 0; d < ndir; d++) {
            // E, S, SE, SW
            const unsigned dy = d == 0 ? 0u : 1u;
            const unsigned cx = d == 0 || d == 2 ? lane + 2u : d == 1 ? lane + 1u : lane;
            const uint32_t c1 = tile[r + dy][cx];
            const bool valid = c0 != 0u && c1 != 0u && c0 != c1;
            const uint32_t a = valid ? min(c0, c1) : 0u, b = valid ? max(c0, c1) : 0u;
            const uint32_t pa = __shfl_up(a, 1, 64), pb = __shfl_up(b, 1, 64);
            const bool bd = lane == 0u || a != pa || b != pb;
            const unsigned long long bound = __ballot(bd), heads = __ballot(bd && valid);
            const unsigned long long vmask = __ballot(valid);
            runs += (uint32_t)__popcll(heads);          // (every lane counts the same; lane 0 reports)
            pairs += (uint32_t)__popcll(vmask);
            if ((heads >> lane) & 1ull) {
                const unsigned long long rest = lane == 63u ? 0ull : (bound >> (lane + 1u));
                const uint32_t len = rest ? (uint32_t)__builtin_ctzll(rest) + 1u : 64u - lane;
                if (DIRECT) {
                    const uint32_t p = atomicAdd(spos, 1u);
                    if (p < room && base + p < cap) rec[base + p] = make_uint4(b, a, len, 0u);
                } else if (!*over) {
                    const unsigned long long key = ((unsigned long long)a << 32) | b;
                    uint32_t h = nbr_hash(a, b) & (NBR_SLOTS - 1u);
                    bool done = false;
                    for (uint32_t probe = 0; probe < NBR_SLOTS; probe++) {
                        const unsigned long long old = atomicCAS(&hkey[h], 0ull, key);
                        if (old == 0ull) atomicAdd(ndist, 1u);
                        if (old == 0ull || old == key) {
                            atomicAdd(&hcnt[h], len);
                            done = true;
                            break;
                        }
                        h = (h + 1u) & (NBR_SLOTS - 1u);
                    }
                    if (!done) *over = 1u;
                }
            }
        }
    }
    if (!DIRECT && lane == 0u) {
        if (runs) atomicAdd(nrun, runs);
        if (pairs) atomicAdd(npair, pairs);
    }
}

// ctr: the accumulation's device words; rec / cap: the record buffer and its capacity in records
__global__ __launch_bounds__(256) void k_nbr_patch(NbrGeom g, unsigned long long *__restrict__ ctr,
                                                   uint4 *__restrict__ rec, unsigned long long cap)
{
    __shared__ uint32_t tile[NBR_PH + 1u][NBR_TW];
    __shared__ unsigned long long hkey[NBR_SLOTS];
    __shared__ uint32_t hcnt[NBR_SLOTS];
    __shared__ uint32_t s_ndist, s_over, s_nrun, s_npair, s_pos, s_max;
    __shared__ unsigned long long s_base;
    const uint32_t py = blockIdx.x / g.pcols, px = blockIdx.x - py * g.pcols;
    const uint32_t y0 = py * NBR_PH, x0 = px * NBR_PW;
    for (uint32_t i = threadIdx.x; i < NBR_SLOTS; i += 256u) { hkey[i] = 0ull; hcnt[i] = 0u; }
    if (threadIdx.x == 0) { s_ndist = 0u; s_over = 0u; s_nrun = 0u; s_npair = 0u; s_pos = 0u; s_max = 0u; }
    // the patch and its rim; 0 (no segment) wherever the raster, or what may be read of it, ends
    uint32_t mx = 0u;
    for (uint32_t i = threadIdx.x; i < (NBR_PH + 1u) * NBR_TW; i += 256u) {
        const uint32_t r = i / NBR_TW, c = i - r * NBR_TW;
        const uint32_t gy = y0 + r;
        const long long gx = (long long)x0 + c - 1;
        uint32_t v = 0u;
        if (gy < g.avail && gx >= 0 && gx < (long long)g.ncols) v = g.seg[(size_t)gy * g.ncols + (size_t)gx];
        tile[r][c] = v;
        mx = max(mx, v);
    }
    __syncthreads();
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, d, 64));
    if (lane_id() == 0u && mx) atomicMax(&s_max, mx);
    nbr_rows<false>(g, y0, tile, hkey, hcnt, &s_ndist, &s_over, &s_nrun, &s_npair, nullptr, nullptr, 0ull, 0ull, 0u);
    __syncthreads();
    const bool over = s_over != 0u;
    const uint32_t nrec = over ? s_nrun : s_ndist;
    if (threadIdx.x == 0) {
        s_base = nrec ? atomicAdd(&ctr[NBR_C_REC], (unsigned long long)nrec) : 0ull;
        if (s_npair) atomicAdd(&ctr[NBR_C_PAIRS], (unsigned long long)s_npair);
        // (most patches hold no new maximum: look before the atomic, one address for the whole grid)
        if ((unsigned long long)s_max > L2LOAD(&ctr[NBR_C_MAXLAB])) atomicMax(&ctr[NBR_C_MAXLAB], (unsigned long long)s_max);
    }
    __syncthreads();
    if (nrec == 0u) return;
    const unsigned long long base = s_base;
    if (base + nrec > cap) return;              // no room: the host regrows the buffer and runs the block again
    if (!over) {
        for (uint32_t i = threadIdx.x; i < NBR_SLOTS; i += 256u) {
            const unsigned long long key = hkey[i];
            if (key != 0ull) {
                const uint32_t p = atomicAdd(&s_pos, 1u);
                if (p < nrec) rec[base + p] = make_uint4((uint32_t)key, (uint32_t)(key >> 32), hcnt[i], 0u);
            }
        }
    } else {
        nbr_rows<true>(g, y0, tile, hkey, hcnt, nullptr, &s_over, nullptr, nullptr, &s_pos, rec, base, cap, nrec);
    }
}

// one word of every record (which: 0 = b, 1 = a, 2 = count), in the order idx (nullptr: as stored);
// idx_copy (optional) receives idx, which the next sort would overwrite
__global__ __launch_bounds__(256) void k_nbr_field(const uint4 *__restrict__ rec, uint32_t n, int which,
                                                   const uint32_t *__restrict__ idx, uint32_t *__restrict__ out,
                                                   uint32_t *__restrict__ idx_copy)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint32_t i = idx ? idx[j] : j;
    const uint32_t *w = (const uint32_t *)(rec + i);
    out[j] = w[which];
    if (idx_copy) idx_copy[j] = i;
}

// the count of a record as the run-length reduction reads it: the one-GPU finish takes the 32-bit count the patch
// kernel wrote (word 2), the share tables the 64-bit count of a record that is itself a sum (words 2 and 3)
template <typename CNT> __device__ __forceinline__ CNT nbr_rec_count(const uint4 &r);
template <> __device__ __forceinline__ uint32_t nbr_rec_count<uint32_t>(const uint4 &r) { return r.z; }
template <> __device__ __forceinline__ unsigned long long nbr_rec_count<unsigned long long>(const uint4 &r)
{
    return ((unsigned long long)r.w << 32) | r.z;
}

// b and count of every record in sorted order (one 16-byte gather instead of two of 4)
template <typename CNT>
__global__ __launch_bounds__(256) void k_nbr_gather(const uint4 *__restrict__ rec, uint32_t n,
                                                    const uint32_t *__restrict__ idx, uint32_t *__restrict__ sb,
                                                    CNT *__restrict__ sc)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= n) return;
    const uint4 r = rec[idx[j]];
    sb[j] = r.x;
    sc[j] = nbr_rec_count<CNT>(r);
}

// 1 where sorted record j starts a new (a, b)
struct NbrHeadFn {
    const uint32_t *sa, *sb;
    __device__ __forceinline__ uint32_t operator()(uint32_t j) const
    {
        return (j == 0u || sa[j] != sa[j - 1u] || sb[j] != sb[j - 1u]) ? 1u : 0u;
    }
};

// run-length reduction: entry e = (heads before j) + head(j) - 1 gets (a, b) from its head and the 64-bit sum of its
// records' counts (CNT: as read, 32 or 64 bits); the records of an entry that share a wavefront add once
template <typename CNT>
__global__ __launch_bounds__(256) void k_nbr_reduce(const uint32_t *__restrict__ sa, const uint32_t *__restrict__ sb,
                                                    const CNT *__restrict__ sc, const uint32_t *__restrict__ uidx,
                                                    uint32_t n, uint32_t *__restrict__ ua, uint32_t *__restrict__ ub,
                                                    unsigned long long *__restrict__ ucnt)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = lane_id();
    const bool in = j < n;
    const NbrHeadFn hf{sa, sb};
    const bool head = in && hf(j) != 0u;
    const uint32_t e = in ? uidx[j] + (head ? 1u : 0u) - 1u : 0u;
    unsigned long long incl = in ? (unsigned long long)sc[j] : 0ull;
    const unsigned long long own = incl;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = __shfl_up((uint32_t)incl, d, 64), hi = __shfl_up((uint32_t)(incl >> 32), d, 64);
        if ((int)lane >= d) incl += ((unsigned long long)hi << 32) | lo;
    }
    // a run inside the wavefront starts at a head, at lane 0, and ends before the next boundary or lane past n
    const bool bd = lane == 0u || head || !in;
    const unsigned long long bound = __ballot(bd);
    const unsigned long long rest = lane == 63u ? 0ull : (bound >> (lane + 1u));
    const unsigned last = rest ? lane + (unsigned)__builtin_ctzll(rest) : 63u;
    const uint32_t llo = __shfl((uint32_t)incl, (int)last, 64), lhi = __shfl((uint32_t)(incl >> 32), (int)last, 64);
    if (!in) return;
    if (head) { ua[e] = sa[j]; ub[e] = sb[j]; }
    if (bd) atomicAdd(&ucnt[e], (((unsigned long long)lhi << 32) | llo) - (incl - own));
}

// The three CSR kernels run over the rows lo .. hi - 1 (row i is id lo + i).  SHARE = false is the whole table: lo = 0,
// every key has a row and the reduced entries of the rows start at 0, so neither the range nor first[] is read.
// SHARE = true is a rank's id share (dneighbours.h): keys outside [lo, hi) have no row here, and the entries with a in
// the share start at first[0] of the (a, b) order, those with b in the share at first[1] of the order by b.

// cnt[key - lo] += how often key occurs in the SORTED keys: a run inside a wavefront adds once
template <bool SHARE>
__global__ __launch_bounds__(256) void k_nbr_degree(const uint32_t *__restrict__ keys, uint32_t n, uint32_t lo,
                                                    uint32_t hi, uint32_t *__restrict__ cnt)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = lane_id();
    const bool in = j < n;
    const uint32_t k = in ? keys[j] : 0xffffffffu;
    const uint32_t pk = __shfl_up(k, 1, 64);
    const bool bd = lane == 0u || k != pk;
    const unsigned long long bound = __ballot(bd);
    if (!in || !bd || (SHARE && (k < lo || k >= hi))) return;
    const unsigned long long rest = lane == 63u ? 0ull : (bound >> (lane + 1u));
    atomicAdd(&cnt[SHARE ? k - lo : k], rest ? (uint32_t)__builtin_ctzll(rest) + 1u : 64u - lane);
}

// first[0] / first[1]: how many of the sorted keys ka / kb (n each) are below lo (share tables only)
__global__ void k_dnbr_bounds(const uint32_t *__restrict__ ka, const uint32_t *__restrict__ kb, uint32_t n, uint32_t lo,
                              uint32_t *__restrict__ first)
{
    if (blockIdx.x != 0u || threadIdx.x >= 2u) return;
    const uint32_t *k = threadIdx.x == 0u ? ka : kb;
    uint32_t a = 0u, b = n;
    while (a < b) {
        const uint32_t mid = a + (b - a) / 2u;
        if (k[mid] < lo) a = mid + 1u; else b = mid;
    }
    first[threadIdx.x] = a;
}

__global__ __launch_bounds__(256) void k_nbr_offsets(const uint32_t *__restrict__ hoff, const uint32_t *__restrict__ loff,
                                                     uint32_t n, long long *__restrict__ offs)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) offs[i] = (long long)hoff[i] + (long long)loff[i];
}

// Row i starts at hoff[i] + loff[i] (the entries above / below the diagonal of the rows before it) and holds its
// lcnt[i] smaller neighbours first.  Reduced entry j = (a, b), a < b, is the (j - first[0] - hoff[i])-th larger
// neighbour of row i = a - lo: place hoff[i] + loff[i] + lcnt[i] + j - first[0] - hoff[i] = loff[i + 1] + j - first[0].
template <bool SHARE>
__global__ __launch_bounds__(256) void k_nbr_fill_high(const uint32_t *__restrict__ ua, const uint32_t *__restrict__ ub,
                                                       const unsigned long long *__restrict__ ucnt, uint32_t U,
                                                       uint32_t lo, uint32_t hi, const uint32_t *__restrict__ first,
                                                       const uint32_t *__restrict__ loff, uint32_t *__restrict__ nbrs,
                                                       long long *__restrict__ lens)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= U) return;
    const uint32_t a = ua[j];
    if (SHARE && (a < lo || a >= hi)) return;
    const size_t p = SHARE ? (size_t)loff[a - lo + 1u] + (j - first[0]) : (size_t)loff[a + 1u] + j;
    nbrs[p] = ub[j];
    lens[p] = (long long)ucnt[j];
}

// The q-th entry in the stable order by b (entry order[q], its b = skb[q]) is the (q - first[1] - loff[i])-th smaller
// neighbour of row i = b - lo: place hoff[i] + loff[i] + q - first[1] - loff[i] = hoff[i] + q - first[1].
template <bool SHARE>
__global__ __launch_bounds__(256) void k_nbr_fill_low(const uint32_t *__restrict__ skb, const uint32_t *__restrict__ order,
                                                      const uint32_t *__restrict__ ua,
                                                      const unsigned long long *__restrict__ ucnt, uint32_t U,
                                                      uint32_t lo, uint32_t hi, const uint32_t *__restrict__ first,
                                                      const uint32_t *__restrict__ hoff, uint32_t *__restrict__ nbrs,
                                                      long long *__restrict__ lens)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= U) return;
    const uint32_t b = skb[q];
    if (SHARE && (b < lo || b >= hi)) return;
    const uint32_t j = order[q];
    const size_t p = SHARE ? (size_t)hoff[b - lo] + (q - first[1]) : (size_t)hoff[b] + q;
    nbrs[p] = ua[j];
    lens[p] = (long long)ucnt[j];
}

// ---- host side --------------------------------------------------------------------------------------------
// a number for the next table of the process (NbrTable::serial)
static inline unsigned long long nbr_next_serial()
{
    static std::atomic<unsigned long long> serial{0};
    return ++serial;
}

static int nbr_ms(shp_ctx *ctx)         // device time between ev[0] and ev[1] (the stream is synchronised)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]) == hipSuccess) ctx->nbr.dev_ms += ms;
    return 0;
}

// room for `want` records, the first `keep` kept
static int nbr_rec_grow(shp_ctx *ctx, unsigned long long want, unsigned long long keep)
{
    NbrState &s = ctx->nbr;
    if (want <= s.cap) return 0;
    if (want > NBR_MAX_REC) SHP_FAIL(ctx, SHP_ERR_NOMEM, "%llu neighbour records: more than the sort indexes", want);
    DevBuf fresh;
    CHK(buf_ensure(ctx, fresh, (size_t)want * 16));
    if (keep) {
        hipError_t e = hipMemcpyAsync(fresh.p, ctx->nbr_rec.p, (size_t)keep * 16, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            hipFree(fresh.p);
            SHP_FAIL(ctx, SHP_ERR_HIP, "copying the neighbour records: %s", hipGetErrorString(e));
        }
    }
    if (ctx->nbr_rec.p) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipFree(ctx->nbr_rec.p));
    }
    ctx->nbr_rec = fresh;
    s.cap = fresh.cap / 16;
    return 0;
}

static int run_nbr_begin(shp_ctx *ctx, int64_t max_seg_id, int four_connected)
{
    NbrState &s = ctx->nbr;
    s = NbrState{};
    nbr_table_end(ctx->nbr_tab);                // (the table of an earlier serial is gone from here on)
    ctx->nbr_tab.serial = nbr_next_serial();
    CHK(buf_ensure(ctx, ctx->nbr_ctr, NBR_C_WORDS * 8));
    HIPCHK(ctx, hipMemsetAsync(ctx->nbr_ctr.p, 0, NBR_C_WORDS * 8, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    s.cap = ctx->nbr_rec.cap / 16;          // (a buffer of an earlier table is reused)
    s.given = max_seg_id;
    s.eight = four_connected ? 0 : 1;
    s.open = true;
    return 0;
}

static int run_nbr_accumulate(shp_ctx *ctx, const uint32_t *d_seg, uint32_t nrows, uint32_t ncols, int has_next)
{
    NbrState &s = ctx->nbr;
    hipStream_t st = ctx->stream;
    if (nrows == 0 || ncols == 0) return 0;
    const uint32_t pcols = (ncols + NBR_PW - 1u) / NBR_PW, prows = (nrows + NBR_PH - 1u) / NBR_PH;
    if ((unsigned long long)pcols * prows > 0x7fffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "row block too large");
    NbrGeom g{d_seg, nrows, nrows + (has_next ? 1u : 0u), ncols, pcols, s.eight};
    unsigned long long *ctr = (unsigned long long *)ctx->nbr_ctr.p;
    unsigned long long *pin = (unsigned long long *)(ctx->h_pinned);
    // first guess: what the last block took (+ 1/8), or a record per 8 pixels
    unsigned long long guess = s.last_block ? s.last_block + s.last_block / 8u
                                            : ((unsigned long long)nrows * ncols) / 8u + 1024u;
    if (s.used + guess > NBR_MAX_REC) guess = NBR_MAX_REC - s.used;
    CHK(nbr_rec_grow(ctx, s.used + guess, s.used));
    for (int attempt = 0; attempt < 2; attempt++) {
        HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
        hipLaunchKernelGGL(k_nbr_patch, dim3(pcols * prows), dim3(256), 0, st, g, ctr, (uint4 *)ctx->nbr_rec.p, s.cap);
        KCHK(ctx);
        HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
        HIPCHK(ctx, hipMemcpyAsync(pin, ctr, NBR_C_WORDS * 8, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
        nbr_ms(ctx);
        const unsigned long long reserved = pin[NBR_C_REC];
        if (reserved < s.used) SHP_FAIL(ctx, SHP_ERR_STATE, "record counter went back (%llu < %llu)", reserved, s.used);
        if (reserved <= s.cap) {
            s.last_block = reserved - s.used;
            s.used = reserved;
            s.pairs = pin[NBR_C_PAIRS];
            s.max_label = (uint32_t)pin[NBR_C_MAXLAB];
            return 0;
        }
        if (attempt == 1) break;
        // the block needs exactly reserved - used records: make room, put the counters back, run it again
        CHK(nbr_rec_grow(ctx, reserved, s.used));
        s.reruns++;
        pin[NBR_C_REC] = s.used;
        pin[NBR_C_PAIRS] = s.pairs;
        HIPCHK(ctx, hipMemcpyAsync(ctr, pin, 16, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipStreamSynchronize(st));
    }
    SHP_FAIL(ctx, SHP_ERR_STATE, "a row block's records did not fit the buffer sized for them");
}

// n records (b, a, count: CNT as nbr_rec_count reads it) sorted by the 64-bit key (a, b) -- two stable passes of
// sort.h's 32-bit sort, by b then by a, over `bits` significant bits -- and run-length reduced with 64-bit sums:
// *U_out distinct pairs in nbr_ua / nbr_ub / nbr_ucnt.  The host reads the distinct-pair count mid-way (one
// synchronisation).  Step 2 of the header for every table of the library.
template <typename CNT>
static int nbr_sort_reduce(shp_ctx *ctx, const uint4 *rec, uint32_t n, int bits, uint32_t *U_out)
{
    hipStream_t st = ctx->stream;
    *U_out = 0u;
    if (n == 0u) return 0;
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_NBR;
    CHK(buf_ensure(ctx, ctx->nbr_key, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->nbr_val, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->nbr_uidx, (size_t)n * 4));
    if (sizeof(CNT) == 8) CHK(buf_ensure(ctx, ctx->dnbr_cnt, (size_t)n * 8));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(n)));
    uint32_t *key = bp<uint32_t>(ctx->nbr_key), *val = bp<uint32_t>(ctx->nbr_val), *uidx = bp<uint32_t>(ctx->nbr_uidx);
    const unsigned gn = grid_for(n, 256);
    // stable by b, then stable by a: sorted by (a, b)
    uint32_t *ord = nullptr, *sa = nullptr;
    hipLaunchKernelGGL(k_nbr_field, dim3(gn), dim3(256), 0, st, rec, n, 0, (const uint32_t *)nullptr, key, (uint32_t *)nullptr);
    KCHK(ctx);
    CHK(sort_pairs(ctx, key, nullptr, n, bits, nullptr, &ord, true));
    hipLaunchKernelGGL(k_nbr_field, dim3(gn), dim3(256), 0, st, rec, n, 1, (const uint32_t *)ord, key, val);
    KCHK(ctx);
    CHK(sort_pairs(ctx, key, val, n, bits, &sa, &ord, true));
    // (the sort has read key and val: b goes where key was, and a 32-bit count where val was)
    uint32_t *sb = key;
    CNT *sc = sizeof(CNT) == 8 ? (CNT *)ctx->dnbr_cnt.p : (CNT *)val;
    hipLaunchKernelGGL(k_nbr_gather<CNT>, dim3(gn), dim3(256), 0, st, rec, n, (const uint32_t *)ord, sb, sc);
    KCHK(ctx);
    NbrHeadFn hf{sa, sb};
    CHK(scan_exclusive(ctx, hf, n, uidx, nullptr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t U = *(volatile uint32_t *)mir;
    if (U < 1u || U > n) SHP_FAIL(ctx, SHP_ERR_STATE, "%u distinct pairs out of %u records", U, n);
    CHK(buf_ensure(ctx, ctx->nbr_ua, (size_t)U * 4));
    CHK(buf_ensure(ctx, ctx->nbr_ub, (size_t)U * 4));
    CHK(buf_ensure(ctx, ctx->nbr_ucnt, (size_t)U * 8));
    HIPCHK(ctx, hipMemsetAsync(ctx->nbr_ucnt.p, 0, (size_t)U * 8, st));
    hipLaunchKernelGGL(k_nbr_reduce<CNT>, dim3(gn), dim3(256), 0, st, (const uint32_t *)sa, (const uint32_t *)sb,
                       (const CNT *)sc, (const uint32_t *)uidx, n, bp<uint32_t>(ctx->nbr_ua), bp<uint32_t>(ctx->nbr_ub),
                       (unsigned long long *)ctx->nbr_ucnt.p);
    KCHK(ctx);
    *U_out = U;
    return 0;
}

// Step 3 of the header: the CSR of the U reduced pairs (nbr_ua / nbr_ub / nbr_ucnt) over the rows of t (t.row0, t.nrows
// are set) into t.offs / t.ids / t.lens; t.nent is set.  The degrees of both ends are counted, scanned, and both
// parts of every row filled.
//   SHARE = false, the whole table (row0 = 0, nrows = S + 1): every pair has both its rows here, so nent = 2 U is
//     known up front and nothing is read back -- the caller synchronises and checks mir[1] == mir[2] == U.
//   SHARE = true, a rank's id share: k_dnbr_bounds finds where the share's entries start in the two orders, and the
//     host reads the two degree totals (one synchronisation) to size the entries: each is at most U.
template <bool SHARE>
static int nbr_build_csr(shp_ctx *ctx, NbrTable &t, uint32_t U, int bits)
{
    hipStream_t st = ctx->stream;
    const uint32_t lo = t.row0, nr = t.nrows, hi = lo + nr;
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_NBR;
    uint32_t *ua = bp<uint32_t>(ctx->nbr_ua), *ub = bp<uint32_t>(ctx->nbr_ub);
    const unsigned long long *ucnt = (const unsigned long long *)ctx->nbr_ucnt.p;
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes((size_t)nr + 1)));
    CHK(buf_ensure(ctx, ctx->nbr_deg, (size_t)2 * nr * 4));
    CHK(buf_ensure(ctx, ctx->nbr_hoff, ((size_t)nr + 1) * 4));
    CHK(buf_ensure(ctx, ctx->nbr_loff, ((size_t)nr + 1) * 4));
    CHK(buf_ensure(ctx, t.offs, ((size_t)nr + 1) * 8));
    unsigned long long nent = 2ull * U;
    if (!SHARE) {
        CHK(buf_ensure(ctx, t.ids, (size_t)nent * 4));
        CHK(buf_ensure(ctx, t.lens, (size_t)nent * 8));
    }
    uint32_t *hcnt = bp<uint32_t>(ctx->nbr_deg), *lcnt = hcnt + nr;
    uint32_t *hoff = bp<uint32_t>(ctx->nbr_hoff), *loff = bp<uint32_t>(ctx->nbr_loff);
    uint32_t *first = SHARE ? (uint32_t *)((unsigned long long *)ctx->nbr_ctr.p + 2) : nullptr;
    if (nr) HIPCHK(ctx, hipMemsetAsync(hcnt, 0, (size_t)2 * nr * 4, st));
    uint32_t *skb = nullptr, *ordb = nullptr;
    const unsigned gu = grid_for(U, 256);
    if (U && nr) {
        hipLaunchKernelGGL(k_nbr_degree<SHARE>, dim3(gu), dim3(256), 0, st, (const uint32_t *)ua, U, lo, hi, hcnt);
        KCHK(ctx);
        CHK(sort_pairs(ctx, ub, nullptr, U, bits, &skb, &ordb, true));
        hipLaunchKernelGGL(k_nbr_degree<SHARE>, dim3(gu), dim3(256), 0, st, (const uint32_t *)skb, U, lo, hi, lcnt);
        KCHK(ctx);
        if (SHARE) {
            hipLaunchKernelGGL(k_dnbr_bounds, dim3(1), dim3(64), 0, st, (const uint32_t *)ua, (const uint32_t *)skb, U, lo, first);
            KCHK(ctx);
        }
    }
    ArrFn fh{hcnt}, fl{lcnt};
    CHK(scan_exclusive(ctx, fh, nr, hoff, hoff + nr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 1));
    CHK(scan_exclusive(ctx, fl, nr, loff, loff + nr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 2));
    hipLaunchKernelGGL(k_nbr_offsets, dim3(grid_for((size_t)nr + 1, 256)), dim3(256), 0, st, (const uint32_t *)hoff,
                       (const uint32_t *)loff, nr + 1u, (long long *)t.offs.p);
    KCHK(ctx);
    if (SHARE) {
        HIPCHK(ctx, hipStreamSynchronize(st));
        const uint32_t th = *(volatile uint32_t *)(mir + 1), tl = *(volatile uint32_t *)(mir + 2);
        if (th > U || tl > U) SHP_FAIL(ctx, SHP_ERR_STATE, "degrees sum to %u and %u for %u pairs", th, tl, U);
        nent = (unsigned long long)th + tl;
        CHK(buf_ensure(ctx, t.ids, (size_t)nent * 4));
        CHK(buf_ensure(ctx, t.lens, (size_t)nent * 8));
    }
    if (nent) {
        hipLaunchKernelGGL(k_nbr_fill_high<SHARE>, dim3(gu), dim3(256), 0, st, (const uint32_t *)ua, (const uint32_t *)ub, ucnt,
                           U, lo, hi, (const uint32_t *)first, (const uint32_t *)loff, bp<uint32_t>(t.ids), (long long *)t.lens.p);
        KCHK(ctx);
        hipLaunchKernelGGL(k_nbr_fill_low<SHARE>, dim3(gu), dim3(256), 0, st, (const uint32_t *)skb, (const uint32_t *)ordb,
                           (const uint32_t *)ua, ucnt, U, lo, hi, (const uint32_t *)first, (const uint32_t *)hoff,
                           bp<uint32_t>(t.ids), (long long *)t.lens.p);
        KCHK(ctx);
    }
    t.nent = nent;
    return 0;
}

// The table over the ids 0 .. S of the first n records of nbr_rec (ids 1 .. S, a < b, 32-bit counts): steps 2 and 3 of
// the header into the context's one-GPU table, which becomes a finished table.  (nbrmerge.h builds the table of
// merged segments through it.)
static int nbr_build_table(shp_ctx *ctx, uint32_t S, uint32_t n)
{
    NbrTable &t = ctx->nbr_tab;
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    const int bits = bits_for(S);
    const uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_NBR;
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    // (room for the longer of the two halves' scans at once: no buffer grows between them)
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(n > ns + 1 ? n : ns + 1)));
    uint32_t U = 0;
    CHK(nbr_sort_reduce<uint32_t>(ctx, (const uint4 *)ctx->nbr_rec.p, n, bits, &U));
    t.S = S;
    t.row0 = 0u;
    t.nrows = (uint32_t)ns;
    CHK(nbr_build_csr<false>(ctx, t, U, bits));
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    nbr_ms(ctx);
    const uint32_t th = *(volatile const uint32_t *)(mir + 1), tl = *(volatile const uint32_t *)(mir + 2);
    if (th != U || tl != U) SHP_FAIL(ctx, SHP_ERR_STATE, "degrees sum to %u and %u for %u pairs", th, tl, U);
    ctx->nbr.open = false;
    t.finished = true;
    return 0;
}

// The table of everything accumulated, for nbr_table_download.  *bad_out: 0, or the largest label above a given
// max_seg_id (then nothing is built).
static int run_nbr_finish(shp_ctx *ctx, uint32_t *S_out, int64_t *nent_out, uint32_t *bad_out)
{
    NbrState &s = ctx->nbr;
    *bad_out = 0u;
    *nent_out = 0;
    uint32_t S = s.max_label;
    if (s.given >= 0) {
        S = (uint32_t)s.given;
        if (s.max_label > S) { *bad_out = s.max_label; *S_out = S; return 0; }
    }
    if (S >= 0xfffffffeu) SHP_FAIL(ctx, SHP_ERR_ARG, "max_seg_id too large");
    *S_out = S;
    CHK(nbr_build_table(ctx, S, (uint32_t)s.used));
    *nent_out = (int64_t)ctx->nbr_tab.nent;
    return 0;
}

// a finished table (either of the context's two) to host memory
static int nbr_table_download(shp_ctx *ctx, const NbrTable &t, int64_t *offsets, uint32_t *nbrs, int64_t *lens)
{
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemcpyAsync(offsets, t.offs.p, ((size_t)t.nrows + 1) * 8, hipMemcpyDeviceToHost, st));
    if (t.nent) {
        HIPCHK(ctx, hipMemcpyAsync(nbrs, t.ids.p, (size_t)t.nent * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(ctx, hipMemcpyAsync(lens, t.lens.p, (size_t)t.nent * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}

// The arrays of a host table into t's buffers (t.nrows is set; the copies are queued, not awaited).  What makes them
// a table -- the device validation of shp_nbr_upload, the host check of shp_dnbr_upload -- is the caller's.
static int nbr_table_upload_arrays(shp_ctx *ctx, NbrTable &t, const int64_t *offsets, const uint32_t *nbrs, const int64_t *lens,
                                   unsigned long long nent)
{
    hipStream_t st = ctx->stream;
    const size_t nr = t.nrows;
    CHK(buf_ensure(ctx, t.offs, (nr + 1) * 8));
    CHK(buf_ensure(ctx, t.ids, (size_t)nent * 4));
    CHK(buf_ensure(ctx, t.lens, (size_t)nent * 8));
    HIPCHK(ctx, hipMemcpyAsync(t.offs.p, offsets, (nr + 1) * 8, hipMemcpyHostToDevice, st));
    if (nent) {
        HIPCHK(ctx, hipMemcpyAsync(t.ids.p, nbrs, (size_t)nent * 4, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(t.lens.p, lens, (size_t)nent * 8, hipMemcpyHostToDevice, st));
    }
    return 0;
}
