// dsegpoints.h -- the per-segment point lists of segpoints.h when the label raster is split by rows over the
// ranks (distributed.deviceSpatialStats with a user function).
//
// Replaces, for row shards, what segpoints.h replaces for one raster: the point accumulation and the completion
// bookkeeping of calcPerSegmentSpatialStatsTiled (tilingstats.py:1262-1390, :1652-1741).  Three steps per rank:
//   build   the sorted runs of the rank's rows [row0, row0 + nrows), in the WHOLE raster's visit order restricted
//           to those rows (run_segpoints_build_geom with pts_geom_slice), and every id judged against the global
//           histogram: complete here (local label count == hist), straddler (0 < local < hist) or absent.  The
//           straddlers' points are packed into 24-byte records {uint64 visit index; uint32 id, x; uint32 y, val}
//           (val: the pixel's 32 bits; the band types are at most 32 bits wide), placed by a scan over the ids.
//   merge   after the all-gather of the records: those of the rank's id share [id_lo, id_hi) are sorted stably by
//           (id, global visit index) -- LSD passes of sort.h, low word of the visit index, high word (rasters of
//           2^32 pixels and more), id -- and materialised in that order; per-id emission offsets are built over all
//           ids: the points of an id complete here come from the local runs, those of a straddler of the share
//           from the merged records, every other id has none.
//   emit    the points of an id range, both sources, into one host buffer in the layout of segpoints.h.
// The local runs live in the sort buffers of the context; the merge sorts with the context's spare buffers
// (dpts_k0 .. dpts_pix swapped in for the duration), so the local runs survive it.
#pragma once
#include "segstats.h"
#include "segpoints.h"

enum { DPTS_ABSENT = 0, DPTS_COMPLETE = 1, DPTS_STRAD = 2 };

// every id's class; lh = local label count (all labelled pixels, valid or not), gh = the global histogram
__global__ __launch_bounds__(256) void k_dpts_classify(uint32_t S, const uint32_t *__restrict__ lh,
                                                       const uint32_t *__restrict__ gh, uint8_t *__restrict__ cls)
{
    const size_t id = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (id > S) return;
    const uint32_t l = id ? lh[id] : 0u, g = id ? gh[id] : 0u;
    cls[id] = (l > 0u && l == g) ? DPTS_COMPLETE : (l > 0u && l < g) ? DPTS_STRAD : DPTS_ABSENT;
}

// points of id i when it is a straddler (the scan of these places the records)
struct DptsStradFn {
    const uint8_t *cls;
    const uint32_t *poff;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        return cls[i] == DPTS_STRAD ? poff[i + 1] - poff[i] : 0u;
    }
};

// out[i] = a[i + 1] - a[i], i < n (counts from an exclusive scan)
__global__ __launch_bounds__(256) void k_diff_u32(const uint32_t *__restrict__ a, uint32_t n, uint32_t *__restrict__ out)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[i] = a[i + 1] - a[i];
}

// global visit index of pixel (y, x) of the whole raster (img_rows x ncols, th x tw tiles)
__device__ __forceinline__ unsigned long long dpts_visit_index(unsigned long long y, uint32_t x, uint32_t th,
                                                               uint32_t tw, unsigned long long img_rows,
                                                               uint32_t ncols)
{
    const unsigned long long y0 = y - y % th;
    const unsigned long long hb = min((unsigned long long)th, img_rows - y0);
    const uint32_t x0 = x - x % tw;
    const uint32_t w = min(tw, ncols - x0);
    return y0 * ncols + (unsigned long long)x0 * hb + (y - y0) * w + (x - x0);
}

// One lane per sorted run: the runs of straddlers become records, in sorted order (so every id's records are in
// visit order).  spos: first record of every id; poff / roff: first point of every id / sorted run.
__global__ __launch_bounds__(256) void k_dpts_pack(const uint32_t *__restrict__ skeys,
                                                   const uint32_t *__restrict__ order,
                                                   const unsigned long long *__restrict__ rtab,
                                                   const uint32_t *__restrict__ roff,
                                                   const uint32_t *__restrict__ poff,
                                                   const uint32_t *__restrict__ spos,
                                                   const uint8_t *__restrict__ cls, uint32_t m, uint32_t nrec,
                                                   PtsGeom g, unsigned long long row0, unsigned long long img_rows,
                                                   unsigned long long *__restrict__ rec)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j >= m) return;
    const uint32_t id = skeys[j];
    if (cls[id] != DPTS_STRAD) return;
    const unsigned long long e = rtab[order[j]];
    const uint32_t p = (uint32_t)e, len = (uint32_t)(e >> 32) + 1u;
    const uint32_t ly = p / g.ncols, x0 = p - ly * g.ncols;
    const unsigned long long y = row0 + ly;
    const uint32_t r0 = spos[id] + (roff[j] - poff[id]);
    for (uint32_t k = 0; k < len; k++) {
        const uint32_t r = r0 + k;
        if (r >= nrec) break;
        const uint32_t x = x0 + k;
        const uint32_t v = (uint32_t)(unsigned long long)ld_px(g.band, g.dtype, p + k);
        unsigned long long *o = rec + (size_t)r * 3u;
        o[0] = dpts_visit_index(y, x, g.th, g.tw, img_rows, g.ncols);
        o[1] = (unsigned long long)id | ((unsigned long long)x << 32);
        o[2] = (y & 0xffffffffull) | ((unsigned long long)v << 32);
    }
}

// ---- merge ---------------------------------------------------------------------------------------------------
// gathered record q (world slots of `slot`, counts[r] valid in slot r) lies in the share
struct DptsKeepFn {
    const unsigned long long *rec;
    const uint32_t *counts;
    uint32_t slot, id_lo, id_hi;
    __device__ __forceinline__ uint32_t operator()(uint32_t q) const
    {
        const uint32_t r = q / slot, e = q - r * slot;
        if (e >= counts[r]) return 0u;
        const uint32_t id = (uint32_t)rec[(size_t)q * 3u + 1u];
        return (id >= id_lo && id < id_hi) ? 1u : 0u;
    }
};

// the kept records' indices and the first sort key (low word of the visit index)
__global__ __launch_bounds__(256) void k_dpts_keep(DptsKeepFn f, uint32_t n, const uint32_t *__restrict__ pos,
                                                   uint32_t *__restrict__ key, uint32_t *__restrict__ idx)
{
    const uint32_t q = blockIdx.x * 256u + threadIdx.x;
    if (q >= n || !f(q)) return;
    const uint32_t k = pos[q];
    key[k] = (uint32_t)f.rec[(size_t)q * 3u];
    idx[k] = q;
}

// the next pass's key of every record in the current order (what 0: high word of the visit index, 1: id - id_lo),
// and the order itself copied out of the sort's ping-pong buffers
__global__ __launch_bounds__(256) void k_dpts_rekey(const unsigned long long *__restrict__ rec,
                                                    const uint32_t *__restrict__ ord, uint32_t k, int what,
                                                    uint32_t id_lo, uint32_t *__restrict__ key,
                                                    uint32_t *__restrict__ idx)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k) return;
    const uint32_t q = ord[i];
    key[i] = what == 0 ? (uint32_t)(rec[(size_t)q * 3u] >> 32) : (uint32_t)rec[(size_t)q * 3u + 1u] - id_lo;
    idx[i] = q;
}

// the records in (id, visit index) order, and the per-id counts of the share
__global__ __launch_bounds__(256) void k_dpts_gather(const unsigned long long *__restrict__ rec,
                                                     const uint32_t *__restrict__ ord, uint32_t k, uint32_t id_lo,
                                                     unsigned long long *__restrict__ out, uint32_t *__restrict__ mcnt)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= k) return;
    const unsigned long long *s = rec + (size_t)ord[i] * 3u;
    unsigned long long *o = out + (size_t)i * 3u;
    o[0] = s[0];
    o[1] = s[1];
    o[2] = s[2];
    atomicAdd(&mcnt[(uint32_t)s[1] - id_lo], 1u);
}

// points this rank emits for id i: all of them for an id complete here, the merged ones for a straddler of the share
struct DptsEmitCountFn {
    const uint8_t *cls;
    const uint32_t *poff, *moff;
    uint32_t S, id_lo, id_hi;
    __device__ __forceinline__ uint32_t operator()(uint32_t i) const
    {
        if (i > S) return 0u;
        if (cls[i] == DPTS_COMPLETE) return poff[i + 1] - poff[i];
        if (i >= id_lo && i < id_hi) return moff[i - id_lo + 1] - moff[i - id_lo];
        return 0u;
    }
};

// ---- emission ------------------------------------------------------------------------------------------------
// ids [lo, hi): res = {first run, end run, first point, points, first merged record, end merged record};
// offs[k] = first point of id lo + k relative to the batch's first point
__global__ __launch_bounds__(256) void k_dpts_range(const uint32_t *__restrict__ skeys, uint32_t m,
                                                    const uint32_t *__restrict__ eoff,
                                                    const uint32_t *__restrict__ moff, uint32_t id_lo,
                                                    uint32_t id_hi, uint32_t lo, uint32_t hi,
                                                    uint32_t *__restrict__ res, long long *__restrict__ offs)
{
    const uint32_t base = eoff[lo];
    const uint32_t k = blockIdx.x * 256u + threadIdx.x;
    if (k <= hi - lo) offs[k] = (long long)(eoff[lo + k] - base);
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const uint32_t want[2] = {lo, hi};
    for (int q = 0; q < 2; q++) {
        uint32_t a = 0, e = m;
        while (a < e) {
            const uint32_t mid = a + (e - a) / 2u;
            if (skeys[mid] < want[q]) a = mid + 1u;
            else e = mid;
        }
        res[q] = a;
    }
    res[2] = base;
    res[3] = eoff[hi] - base;
    const uint32_t a = max(lo, id_lo), b = min(hi, id_hi);
    res[4] = a < b ? moff[a - id_lo] : 0u;
    res[5] = a < b ? moff[b - id_lo] : 0u;
}

// k_pts_expand for the local runs [rlo, rhi) of ids complete here (other runs have no points to give): output
// record t of the wavefront's runs is written by lane t % 64
template <int DT>
__global__ __launch_bounds__(256) void k_dpts_expand(const uint32_t *__restrict__ skeys,
                                                     const uint32_t *__restrict__ order,
                                                     const unsigned long long *__restrict__ rtab,
                                                     const uint32_t *__restrict__ roff,
                                                     const uint32_t *__restrict__ poff,
                                                     const uint32_t *__restrict__ eoff,
                                                     const uint8_t *__restrict__ cls, uint32_t rlo, uint32_t rhi,
                                                     uint32_t base, uint32_t npts, const void *__restrict__ band,
                                                     uint32_t ncols, uint32_t row0, uint4 *__restrict__ out)
{
    __shared__ uint32_t s_pre[4][64], s_pos[4][64], s_o[4][64];
    const unsigned long long j = (unsigned long long)rlo + blockIdx.x * 256u + threadIdx.x;
    const unsigned lane = lane_id(), wv = threadIdx.x >> 6;
    uint32_t len = 0, pos = 0, o = 0;
    if (j < rhi) {
        const uint32_t id = skeys[j];
        if (cls[id] == DPTS_COMPLETE) {
            const unsigned long long e = rtab[order[j]];
            pos = (uint32_t)e;
            len = (uint32_t)(e >> 32) + 1u;
            o = eoff[id] - base + (roff[j] - poff[id]);
        }
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
        uint32_t q = 0;                         // the last run whose prefix is <= t (it has points)
#pragma unroll
        for (uint32_t step = 32u; step >= 1u; step >>= 1)
            if (q + step < 64u && s_pre[wv][q + step] <= t) q += step;
        const uint32_t k = t - s_pre[wv][q];
        const uint32_t p = s_pos[wv][q] + k, r = s_o[wv][q] + k;
        if (r < npts) {
            const uint32_t y = p / ncols;
            const long long v = ld_t<DT>(band, p);
            out[r] = make_uint4(p - y * ncols, row0 + y, (uint32_t)(unsigned long long)v,
                                (uint32_t)((unsigned long long)v >> 32));
        }
    }
}

// the merged records [mlo, mhi) of the share: one lane per record; val widened as the band type says
__global__ __launch_bounds__(256) void k_dpts_mexpand(const unsigned long long *__restrict__ mrec,
                                                      const uint32_t *__restrict__ moff,
                                                      const uint32_t *__restrict__ eoff, uint32_t id_lo,
                                                      uint32_t mlo, uint32_t mhi, uint32_t base, uint32_t npts,
                                                      int is_signed, uint4 *__restrict__ out)
{
    const uint32_t i = mlo + blockIdx.x * 256u + threadIdx.x;
    if (i >= mhi) return;
    const unsigned long long w1 = mrec[(size_t)i * 3u + 1u], w2 = mrec[(size_t)i * 3u + 2u];
    const uint32_t id = (uint32_t)w1;
    const uint32_t r = eoff[id] - base + (i - moff[id - id_lo]);
    if (r >= npts) return;
    const uint32_t v = (uint32_t)(w2 >> 32);
    const long long val = is_signed ? (long long)(int32_t)v : (long long)v;
    out[r] = make_uint4((uint32_t)(w1 >> 32), (uint32_t)w2, (uint32_t)(unsigned long long)val,
                        (uint32_t)((unsigned long long)val >> 32));
}

// ---- host side -----------------------------------------------------------------------------------------------
// Local part: the slice's sorted runs (left in ctx->pts), classes in ctx->dpts_cls, local label counts and points
// per id downloaded (lh_out, pts_out: S + 1 uint32 each), the straddlers' records at *d_rec (ctx->dpts_rec,
// *n_rec of them, valid until the context's next call but the merge).
static int run_dsegpoints_build(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, uint32_t nrows,
                                uint32_t ncols, uint32_t row0, uint32_t img_rows, uint32_t S, int64_t null_val,
                                uint32_t tile_size, const uint32_t *d_hist, uint32_t *lh_out, uint32_t *pts_out,
                                void **d_rec, int64_t *n_rec)
{
    hipStream_t st = ctx->stream;
    const size_t ns = (size_t)S + 1;
    const uint32_t n = nrows * ncols;
    DSegPointsState &ds = ctx->dpts;
    ds = DSegPointsState{};
    const PtsGeom g = pts_geom_slice(d_seg, d_band, dtype, row0, nrows, img_rows, ncols, S, null_val, tile_size);
    int64_t npts = 0;
    CHK(run_segpoints_build_geom(ctx, g, null_val, &npts));      // (synchronises)
    const SegPointsState &ps = ctx->pts;
    uint32_t *poff = bp<uint32_t>(ctx->pts_off);
    // local label counts, classes
    CHK(buf_ensure(ctx, ctx->dpts_lh, ns * 4));
    CHK(buf_ensure(ctx, ctx->dpts_cls, ns + 16));
    CHK(buf_ensure(ctx, ctx->dpts_spos, (ns + 1) * 4));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(ns)));
    uint32_t *lh = bp<uint32_t>(ctx->dpts_lh), *spos = bp<uint32_t>(ctx->dpts_spos);
    uint8_t *cls = bp<uint8_t>(ctx->dpts_cls);
    HIPCHK(ctx, hipMemsetAsync(lh, 0, ns * 4, st));
    if (n) hipLaunchKernelGGL(k_label_hist, dim3(grid_for(n, 256)), dim3(256), 0, st, d_seg, n, S, lh);
    hipLaunchKernelGGL(k_dpts_classify, dim3(grid_for(ns, 256)), dim3(256), 0, st, S, lh, d_hist, cls);
    KCHK(ctx);
    // the straddlers' records, placed by a scan of their point counts
    // (scan totals land in the pinned mirror words after the build's: [3] records here, [5] / [6] the merge's)
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_PTS;
    DptsStradFn f{cls, poff};
    CHK(scan_exclusive(ctx, f, (uint32_t)ns, spos, spos + ns, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 3));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t nrec = *(volatile uint32_t *)(mir + 3);
    if ((int64_t)nrec > npts) SHP_FAIL(ctx, SHP_ERR_STATE, "%u straddler points of %lld", nrec, (long long)npts);
    CHK(buf_ensure(ctx, ctx->dpts_rec, (size_t)nrec * 24 + 64));
    if (nrec && ps.m)
        hipLaunchKernelGGL(k_dpts_pack, dim3(grid_for(ps.m, 256)), dim3(256), 0, st, ps.skeys, ps.order,
                           (const unsigned long long *)ctx->pts_runs.p, ps.roff, poff, spos, cls, ps.m, nrec, g,
                           (unsigned long long)row0, (unsigned long long)img_rows,
                           (unsigned long long *)ctx->dpts_rec.p);
    KCHK(ctx);
    // points per id = the scan's differences (poff holds S + 2 entries)
    HIPCHK(ctx, hipMemcpyAsync(lh_out, lh, ns * 4, hipMemcpyDeviceToHost, st));
    CHK(buf_ensure(ctx, ctx->pts_offs, ns * 4 + 64));
    hipLaunchKernelGGL(k_diff_u32, dim3(grid_for(ns, 256)), dim3(256), 0, st, poff, (uint32_t)ns,
                       bp<uint32_t>(ctx->pts_offs));
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(pts_out, bp<uint32_t>(ctx->pts_offs), ns * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    ds.row0 = row0;
    ds.max_visit = (unsigned long long)img_rows * ncols - 1ull;
    ds.nrec = nrec;
    ds.npts_local = (uint32_t)npts;
    ds.stage = 1;
    *d_rec = ctx->dpts_rec.p;
    *n_rec = (int64_t)nrec;
    return 0;
}

// Merge part: the share's records sorted by (id, visit index) into ctx->dpts_mrec, moff (share ids + 1) and the
// emission offsets of all ids (eoff, S + 2); merged_out (host, id_hi - id_lo uint32) = records per share id.
static int run_dsegpoints_merge(shp_ctx *ctx, const unsigned long long *d_all, uint32_t slot, uint32_t world,
                                const uint32_t *counts_host, uint32_t id_lo, uint32_t id_hi, uint32_t *merged_out,
                                int64_t *n_merged)
{
    hipStream_t st = ctx->stream;
    DSegPointsState &ds = ctx->dpts;
    const SegPointsState &ps = ctx->pts;
    const uint32_t S = ps.S;
    const size_t ns = (size_t)S + 1;
    const uint32_t nshare = id_hi - id_lo;
    const uint32_t nq = slot * world;
    uint32_t *mir = ctx->h_pinned + PIN_MIRROR + MIR_PTS;
    CHK(buf_ensure(ctx, ctx->dpts_moff, ((size_t)nshare + 1) * 4 + 64));
    CHK(buf_ensure(ctx, ctx->dpts_eoff, (ns + 1) * 4 + 64));
    uint32_t *moff = bp<uint32_t>(ctx->dpts_moff), *eoff = bp<uint32_t>(ctx->dpts_eoff);
    HIPCHK(ctx, hipMemsetAsync(moff, 0, ((size_t)nshare + 1) * 4, st));
    uint32_t k = 0;
    if (nq) {
        CHK(buf_ensure(ctx, ctx->dpts_cnt, (size_t)world * 4 + 64));
        CHK(buf_ensure(ctx, ctx->dpts_kpos, ((size_t)nq + 1) * 4));
        CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(nq)));
        uint32_t *d_counts = bp<uint32_t>(ctx->dpts_cnt), *kpos = bp<uint32_t>(ctx->dpts_kpos);
        HIPCHK(ctx, hipMemcpyAsync(d_counts, counts_host, (size_t)world * 4, hipMemcpyHostToDevice, st));
        DptsKeepFn kf{d_all, d_counts, slot, id_lo, id_hi};
        CHK(scan_exclusive(ctx, kf, nq, kpos, kpos + nq, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 5));
        HIPCHK(ctx, hipStreamSynchronize(st));
        k = *(volatile uint32_t *)(mir + 5);
        if (k > nq) SHP_FAIL(ctx, SHP_ERR_STATE, "%u records kept of %u", k, nq);
    }
    if ((unsigned long long)k + ds.npts_local >= 0xffffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "this rank's points (%u local, %u merged) reach 2^32", ds.npts_local, k);
    CHK(buf_ensure(ctx, ctx->dpts_mrec, (size_t)k * 24 + 64));
    unsigned long long *mrec = (unsigned long long *)ctx->dpts_mrec.p;
    if (k) {
        CHK(buf_ensure(ctx, ctx->dpts_key, (size_t)k * 4));
        CHK(buf_ensure(ctx, ctx->dpts_idx, (size_t)k * 4));
        uint32_t *key = bp<uint32_t>(ctx->dpts_key), *idx = bp<uint32_t>(ctx->dpts_idx);
        DptsKeepFn kf{d_all, bp<uint32_t>(ctx->dpts_cnt), slot, id_lo, id_hi};
        hipLaunchKernelGGL(k_dpts_keep, dim3(grid_for(nq, 256)), dim3(256), 0, st, kf, nq,
                           bp<uint32_t>(ctx->dpts_kpos), key, idx);
        KCHK(ctx);
        // the sorts run in the spare buffers: the local runs stay in the sort buffers for the emission
        std::swap(ctx->sort_k0, ctx->dpts_k0);
        std::swap(ctx->sort_k1, ctx->dpts_k1);
        std::swap(ctx->sort_v1, ctx->dpts_v1);
        std::swap(ctx->pix, ctx->dpts_pix);
        int rc = 0;
        uint32_t *ord = nullptr;
        const unsigned long long max_visit = ds.max_visit;
        const unsigned long long vlo = max_visit > 0xffffffffull ? 0xffffffffull : max_visit;
        const uint32_t gvhi = (uint32_t)(max_visit >> 32);
        // LSD: low word of the visit index, its high word, then the id (each pass stable)
        rc = sort_pairs(ctx, key, idx, k, bits_for((uint32_t)vlo), nullptr, &ord);
        if (!rc && gvhi) {
            hipLaunchKernelGGL(k_dpts_rekey, dim3(grid_for(k, 256)), dim3(256), 0, st, d_all, ord, k, 0, id_lo, key,
                               idx);
            rc = sort_pairs(ctx, key, idx, k, bits_for(gvhi), nullptr, &ord);
        }
        if (!rc && nshare > 1) {
            hipLaunchKernelGGL(k_dpts_rekey, dim3(grid_for(k, 256)), dim3(256), 0, st, d_all, ord, k, 1, id_lo, key,
                               idx);
            rc = sort_pairs(ctx, key, idx, k, bits_for(nshare - 1), nullptr, &ord);
        }
        if (!rc) {
            hipLaunchKernelGGL(k_dpts_gather, dim3(grid_for(k, 256)), dim3(256), 0, st, d_all, ord, k, id_lo, mrec,
                               moff);
            if (hipGetLastError() != hipSuccess) rc = SHP_ERR_HIP;
        }
        std::swap(ctx->sort_k0, ctx->dpts_k0);
        std::swap(ctx->sort_k1, ctx->dpts_k1);
        std::swap(ctx->sort_v1, ctx->dpts_v1);
        std::swap(ctx->pix, ctx->dpts_pix);
        if (rc) return rc;
        KCHK(ctx);
    }
    if (nshare)
        HIPCHK(ctx, hipMemcpyAsync(merged_out, moff, (size_t)nshare * 4, hipMemcpyDeviceToHost, st));
    // counts -> offsets (the scan reads a copy of the counts)
    CHK(buf_ensure(ctx, ctx->dpts_key, ((size_t)nshare + 1) * 4));
    CHK(buf_ensure(ctx, ctx->scan_tmp, scan_tmp_bytes(ns + 1 > nshare + 1 ? ns + 1 : nshare + 1)));
    HIPCHK(ctx, hipMemcpyAsync(bp<uint32_t>(ctx->dpts_key), moff, ((size_t)nshare + 1) * 4, hipMemcpyDeviceToDevice,
                               st));
    ArrFn mf{bp<uint32_t>(ctx->dpts_key)};
    CHK(scan_exclusive(ctx, mf, nshare + 1, moff, nullptr, bp<uint32_t>(ctx->scan_tmp)));
    DptsEmitCountFn ef{bp<uint8_t>(ctx->dpts_cls), bp<uint32_t>(ctx->pts_off), moff, S, id_lo, id_hi};
    CHK(scan_exclusive(ctx, ef, (uint32_t)ns + 1, eoff, nullptr, bp<uint32_t>(ctx->scan_tmp), nullptr, mir + 6));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t total = *(volatile uint32_t *)(mir + 6);
    ds.id_lo = id_lo;
    ds.id_hi = id_hi;
    ds.nmerged = k;
    ds.npts_emit = total;
    ds.stage = 2;
    *n_merged = (int64_t)k;
    return 0;
}

// ids [lo, hi) of the merged lists: offs_out (host, hi - lo + 1 int64) and the records (host, at most cap)
static int run_dsegpoints_emit(shp_ctx *ctx, uint32_t lo, uint32_t hi, int64_t *offs_out, void *pts_out, int64_t cap,
                               int64_t *npts_out)
{
    hipStream_t st = ctx->stream;
    const SegPointsState &ps = ctx->pts;
    const DSegPointsState &ds = ctx->dpts;
    const size_t nid = (size_t)hi - lo;
    CHK(buf_ensure(ctx, ctx->pts_offs, (nid + 1) * 8 + 64));
    uint32_t *res = bp<uint32_t>(ctx->pts_offs);
    long long *d_offs = (long long *)(res + 16);
    hipLaunchKernelGGL(k_dpts_range, dim3(grid_for(nid + 1, 256)), dim3(256), 0, st, ps.skeys, ps.m,
                       bp<uint32_t>(ctx->dpts_eoff), bp<uint32_t>(ctx->dpts_moff), ds.id_lo, ds.id_hi, lo, hi, res,
                       d_offs);
    KCHK(ctx);
    uint32_t h[6] = {0, 0, 0, 0, 0, 0};
    HIPCHK(ctx, hipMemcpyAsync(h, res, 24, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(offs_out, d_offs, (nid + 1) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    const uint32_t rlo = h[0], rhi = h[1], base = h[2], npts = h[3], mlo = h[4], mhi = h[5];
    if (rlo > rhi || rhi > ps.m) SHP_FAIL(ctx, SHP_ERR_STATE, "run range %u..%u of %u", rlo, rhi, ps.m);
    if (mlo > mhi || mhi > ds.nmerged) SHP_FAIL(ctx, SHP_ERR_STATE, "merged range %u..%u of %u", mlo, mhi, ds.nmerged);
    *npts_out = npts;
    if ((int64_t)npts > cap) SHP_FAIL(ctx, SHP_ERR_ARG, "ids %u..%u hold %u points, the output %lld", lo, hi, npts,
                                      (long long)cap);
    if (npts == 0) return 0;
    CHK(buf_ensure(ctx, ctx->pts_stage, (size_t)npts * 16));
    uint4 *d_out = (uint4 *)ctx->pts_stage.p;
    if (rhi > rlo) {
        const uint32_t nr = rhi - rlo;
        DISPATCH_DTYPE(ps.dtype,
            hipLaunchKernelGGL(k_dpts_expand<DT>, dim3(grid_for(nr, 256)), dim3(256), 0, st, ps.skeys, ps.order,
                               (const unsigned long long *)ctx->pts_runs.p, ps.roff, bp<uint32_t>(ctx->pts_off),
                               bp<uint32_t>(ctx->dpts_eoff), bp<uint8_t>(ctx->dpts_cls), rlo, rhi, base, npts,
                               ps.band, ps.ncols, ds.row0, d_out));
    }
    if (mhi > mlo)
        hipLaunchKernelGGL(k_dpts_mexpand, dim3(grid_for(mhi - mlo, 256)), dim3(256), 0, st,
                           (const unsigned long long *)ctx->dpts_mrec.p, bp<uint32_t>(ctx->dpts_moff),
                           bp<uint32_t>(ctx->dpts_eoff), ds.id_lo, mlo, mhi, base, npts,
                           (int)(ps.dtype == SHP_I16 || ps.dtype == SHP_I32), d_out);
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(pts_out, d_out, (size_t)npts * 16, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return 0;
}
