// api.hip -- the extern "C" boundary of libshepseg_hip.so (see include/shepseg_hip.h).
// gfx950 only.  No CPU fallback: without a usable device every call fails.
#include "common.h"
#include <utility>
#include "scan.h"
#include "sort.h"
#include "prims.h"
#include "kmeans.h"
#include "clump.h"
#include "elim_single.h"
#include "elim_small.h"
#include "synth.h"
#include "stitch.h"
static int read_u32(shp_ctx *ctx, const uint32_t *d, uint32_t *h);
#include "segstats.h"
#include "subset.h"
#include "spatial.h"
#include "segpoints.h"
#include "dsegpoints.h"
#include "colour.h"
#include "neighbours.h"
#include "nbrreduce.h"
#include "nbrmerge.h"
#include "nbragg.h"
#include "dneighbours.h"
#include "dnbrmerge.h"
#include "segshape.h"
#include "dsegshape.h"
#include "outline.h"
#include "hull.h"
#include "simplify.h"
#include "segdepth.h"
#include "comm.h"

#define API extern "C" __attribute__((visibility("default")))

static thread_local std::string g_create_err;

API int shp_version(void) { return 100; }

API int shp_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

static int ctx_create(int device, int high_priority, shp_ctx **out, bool shared = false);

API int shp_ctx_create(int device, shp_ctx **out) { return ctx_create(device, 0, out); }

// a worker context of the tiled drivers: device workspace without a stream of its own (see the
// stream pool in common.h); it falls back to an ordinary context on a second device of the process
API int shp_ctx_create_shared(int device, shp_ctx **out) { return ctx_create(device, 0, out, true); }

// a context whose streams are created with the highest stream priority (the tiled drivers use
// one for the sequential stitch chain so that its small kernels are not queued behind the
// worker streams' launches)
API int shp_ctx_create_priority(int device, shp_ctx **out) { return ctx_create(device, 1, out); }

static int ctx_create(int device, int high_priority, shp_ctx **out, bool shared)
{
    if (!out) return SHP_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return SHP_ERR_NO_DEVICE;
    if (device < 0 || device >= n) return SHP_ERR_ARG;
    if (hipSetDevice(device) != hipSuccess) return SHP_ERR_HIP;
    shp_ctx *ctx = new shp_ctx();
    ctx->device = device;
    int prio_lo = 0, prio_hi = 0;
    hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi);      // hi = numerically lowest
    ctx->stream_priority = high_priority ? prio_hi : 0;
    if (shared) {
        std::lock_guard<std::mutex> lk(g_streams.mu);
        if (g_streams.device < 0) {
            if (hipStreamCreateWithPriority(&g_streams.misc, hipStreamNonBlocking, 0) != hipSuccess) {
                delete ctx;
                return SHP_ERR_HIP;
            }
            g_streams.device = device;
        }
        if (g_streams.device == device) {
            ctx->shared = true;
            ctx->stream = g_streams.misc;
        }
    }
    if (!ctx->shared &&
        hipStreamCreateWithPriority(&ctx->stream, hipStreamNonBlocking, ctx->stream_priority) != hipSuccess) {
        delete ctx;
        return SHP_ERR_HIP;
    }
    if (hipHostMalloc((void **)&ctx->h_pinned, SHP_PINNED_BYTES, hipHostMallocDefault) != hipSuccess) {
        if (!ctx->shared) hipStreamDestroy(ctx->stream);
        delete ctx;
        return SHP_ERR_HIP;
    }
    if (hipMalloc((void **)&ctx->scan_ctr, 256) != hipSuccess || hipMemset(ctx->scan_ctr, 0, 256) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {       // (the context's stream does not wait for the null stream)
        hipHostFree(ctx->h_pinned);
        if (!ctx->shared) hipStreamDestroy(ctx->stream);
        delete ctx;
        return SHP_ERR_NOMEM;
    }
    for (int i = 0; i < 16; i++) hipEventCreate(&ctx->ev[i]);
    hipEventCreateWithFlags(&ctx->evfork, hipEventDisableTiming);
    hipEventCreateWithFlags(&ctx->evjoin, hipEventDisableTiming);
    *out = ctx;
    return SHP_OK;
}

API void shp_ctx_destroy(shp_ctx *ctx)
{
    if (!ctx) return;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    for (DevBuf *b : ctx->bufs)
        if (b->p) hipFree(b->p);
    for (int i = 0; i < 16; i++)
        if (ctx->ev[i]) hipEventDestroy(ctx->ev[i]);
    for (int i = 0; i < PROF_POOL; i++)
        for (int j = 0; j < 2; j++)
            if (ctx->prof_ev[i][j]) hipEventDestroy(ctx->prof_ev[i][j]);
    if (ctx->h_pinned) hipHostFree(ctx->h_pinned);
    if (ctx->h_fit) hipHostFree(ctx->h_fit);
    if (ctx->h_jobs) hipHostFree(ctx->h_jobs);
    for (int j = 0; j < 2; j++)
        if (ctx->wb_ev[j]) hipEventDestroy(ctx->wb_ev[j]);
    if (ctx->scan_ctr) hipFree(ctx->scan_ctr);
    if (ctx->stream2) { hipStreamSynchronize(ctx->stream2); hipStreamDestroy(ctx->stream2); }
    if (ctx->evfork) hipEventDestroy(ctx->evfork);
    if (ctx->evjoin) hipEventDestroy(ctx->evjoin);
    if (!ctx->shared) hipStreamDestroy(ctx->stream);
    delete ctx;
}

API const char *shp_last_error(const shp_ctx *ctx) { return ctx ? ctx->err.c_str() : "null ctx"; }

API int shp_last_timings(const shp_ctx *ctx, double *out)
{
    if (!ctx || !out) return SHP_ERR_ARG;
    for (int i = 0; i < 8; i++) out[i] = ctx->timings[i];
    return SHP_OK;
}

static int enter(shp_ctx *ctx)
{
    if (!ctx) return SHP_ERR_ARG;
    ctx->err.clear();
    ctx->pts.valid = false;             // (shp_segpoints_emit keeps it)
    ctx->dpts.stage = 0;                // (shp_dsegpoints_merge_dev / _emit move it on)
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->prof_used) {                       // events of an earlier (synchronised) call
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        prof_collect(ctx);
    }
    return 0;
}

static int check_img_args(shp_ctx *ctx, const void *img, int dtype, int nb, int nr, int nc)
{
    if (!img) SHP_FAIL(ctx, SHP_ERR_ARG, "img is NULL");
    if (dtype_size(dtype) == 0) SHP_FAIL(ctx, SHP_ERR_ARG, "unsupported image dtype %d", dtype);
    if (nb < 1 || nr < 0 || nc < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad image shape (%d,%d,%d)", nb, nr, nc);
    if ((uint64_t)nr * (uint64_t)nc >= 0x7fffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "tile too large: %d x %d", nr, nc);
    return 0;
}

static int upload_img(shp_ctx *ctx, const void *img, int dtype, int nb, size_t npix)
{
    const size_t bytes = (size_t)nb * npix * dtype_size(dtype);
    CHK(buf_ensure(ctx, ctx->img, bytes));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(ctx->img.p, img, bytes, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}

static int read_u32(shp_ctx *ctx, const uint32_t *d, uint32_t *h)
{
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, d, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    *h = ctx->h_pinned[0];
    return 0;
}

static void collect_timings(shp_ctx *ctx);
static float ev_ms(shp_ctx *ctx, int a, int b)
{
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, ctx->ev[a], ctx->ev[b]) != hipSuccess) return 0.f;
    return ms;
}

// ---- k-means --------------------------------------------------------------------------------
API int shp_last_fit_path(const shp_ctx *ctx) { return ctx ? ctx->fit_path : -1; }

// what the four shp_kmeans_fit* entry points check alike (pixels: the sample has a pixel type `dtype`, else it is
// float64; init may be NULL in the planar forms only)
static int check_fit_args(shp_ctx *ctx, const void *xsample, bool pixels, int dtype, const double *init_centres,
                          bool need_init, const double *centres_out)
{
    if (!xsample || (need_init && !init_centres) || !centres_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (pixels && dtype_size(dtype) == 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad pixel type %d", dtype);
    return 0;
}

API int shp_kmeans_fit(shp_ctx *ctx, const double *xsample, int64_t nrows, int nbands, int k,
                       const double *init_centres, int max_iter, double tol_rel,
                       double *centres_out, int32_t *labels_out, int *n_iter_out)
{
    CHK(enter(ctx));
    CHK(check_fit_args(ctx, xsample, false, FIT_DT_F64, init_centres, true, centres_out));
    return run_kmeans_fit(ctx, xsample, FIT_DT_F64, nrows, nbands, k, init_centres, max_iter, tol_rel,
                          centres_out, labels_out, n_iter_out);
}

// the same on rows of the image's own pixel type (no float64 copy of the sample on the host)
API int shp_kmeans_fit_typed(shp_ctx *ctx, const void *xsample, int dtype, int64_t nrows, int nbands,
                             int k, const double *init_centres, int max_iter, double tol_rel,
                             double *centres_out, int32_t *labels_out, int *n_iter_out)
{
    CHK(enter(ctx));
    CHK(check_fit_args(ctx, xsample, true, dtype, init_centres, true, centres_out));
    return run_kmeans_fit(ctx, xsample, dtype, nrows, nbands, k, init_centres, max_iter, tol_rel,
                          centres_out, labels_out, n_iter_out);
}

// The whole-image model of the tiled driver from the sub-sample as it leaves the device: nbands
// planes of npix pixels.  Rows with the null value in any band are dropped, the initial centres are
// diagonalClusterCentres of what is left (init_centres == NULL) or given; *nrows_out = rows fitted
// (labels_out, optional, holds that many).  Same arithmetic as shp_kmeans_fit_typed on the
// transposed rows, prepared by one host thread per band (kmeans.h: fit_prepare).
// cm with more than one rank: the E-step sharded by sample rows over the ranks of the communicator: every rank
// passes the SAME sample and gets the same model (fit_elkan.h: FitShard)
API int shp_kmeans_fit_planar_dist(shp_ctx *ctx, shp_comm *cm, const void *planes, int dtype, int64_t npix, int nbands,
                                   int has_null, int64_t null_val, int k, const double *init_centres,
                                   int max_iter, double tol_rel, double *centres_out, int32_t *labels_out,
                                   int *n_iter_out, int64_t *nrows_out)
{
    CHK(enter(ctx));
    CHK(check_fit_args(ctx, planes, true, dtype, init_centres, false, centres_out));
    if (nrows_out) *nrows_out = 0;
    FitShard sh;
    if (cm && cm->world > 1) {
        if (cm->ctx->device != ctx->device) SHP_FAIL(ctx, SHP_ERR_ARG, "the communicator lives on another device");
        sh.rank = cm->rank; sh.world = cm->world; sh.nc = (void *)cm->nc;
    }
    return run_kmeans_fit(ctx, planes, dtype, npix, nbands, k, init_centres, max_iter, tol_rel, centres_out,
                          labels_out, n_iter_out, true, has_null, (long long)null_val, nrows_out, sh);
}

API int shp_kmeans_fit_planar(shp_ctx *ctx, const void *planes, int dtype, int64_t npix, int nbands,
                              int has_null, int64_t null_val, int k, const double *init_centres,
                              int max_iter, double tol_rel, double *centres_out, int32_t *labels_out,
                              int *n_iter_out, int64_t *nrows_out)
{
    return shp_kmeans_fit_planar_dist(ctx, nullptr, planes, dtype, npix, nbands, has_null, null_val, k, init_centres,
                                      max_iter, tol_rel, centres_out, labels_out, n_iter_out, nrows_out);
}

API int shp_kmeans_assign(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows, int ncols,
                          const double *centres, int k, int has_null, int64_t null_val,
                          int32_t *clusters_out)
{
    CHK(enter(ctx));
    CHK(check_img_args(ctx, img, dtype, nbands, nrows, ncols));
    if (!centres || !clusters_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    const size_t npix = (size_t)nrows * ncols;
    if (npix == 0) return 0;
    CHK(upload_img(ctx, img, dtype, nbands, npix));
    CHK(buf_ensure(ctx, ctx->aux, npix * 4));
    CHK(launch_assign(ctx, ctx->img.p, dtype, nbands, npix, centres, k, has_null, null_val, nullptr,
                      bp<int32_t>(ctx->aux)));
    HIPCHK(ctx, hipMemcpyAsync(clusters_out, ctx->aux.p, npix * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- stages ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_i32_to_u16(const int32_t *__restrict__ in,
                                                    uint16_t *__restrict__ out, uint32_t n,
                                                    uint32_t *bad)
{
    const uint32_t p = blockIdx.x * 256u + threadIdx.x;
    if (p >= n) return;
    const int32_t v = in[p];
    if (v < 0 || v > 65535) atomicAdd(bad, 1u);
    out[p] = (uint16_t)v;
}

API int shp_clump(shp_ctx *ctx, const int32_t *clusters, int nrows, int ncols, int four_connected,
                  uint32_t *seg_out, uint32_t *max_seg_id_out)
{
    CHK(enter(ctx));
    if (!clusters || !seg_out || !max_seg_id_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (nrows < 0 || ncols < 0 || (uint64_t)nrows * (uint64_t)ncols >= 0x7fffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad shape %d x %d", nrows, ncols);
    const uint32_t n = (uint32_t)nrows * (uint32_t)ncols;
    *max_seg_id_out = 0;
    if (n == 0) return 0;
    CHK(buf_ensure(ctx, ctx->aux2, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->clus, (size_t)n * 2));
    CHK(buf_ensure(ctx, ctx->seg, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->small, 4096));
    uint32_t *bad = bp<uint32_t>(ctx->small);
    HIPCHK(ctx, hipMemcpyAsync(ctx->aux2.p, clusters, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(bad, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_i32_to_u16, dim3(grid_for(n, 256)), dim3(256), 0, ctx->stream,
                       bp<int32_t>(ctx->aux2), bp<uint16_t>(ctx->clus), n, bad);
    KCHK(ctx);
    uint32_t nbad = 0;
    CHK(read_u32(ctx, bad, &nbad));
    if (nbad) SHP_FAIL(ctx, SHP_ERR_ARG, "cluster ids must lie in 0..65535 (%u do not)", nbad);
    CHK(run_clump(ctx, bp<uint16_t>(ctx->clus), nrows, ncols, four_connected, bp<uint32_t>(ctx->seg),
                  bad + 1));
    HIPCHK(ctx, hipMemcpyAsync(seg_out, ctx->seg.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    CHK(read_u32(ctx, bad + 1, max_seg_id_out));
    return 0;
}

API int shp_make_seg_size(shp_ctx *ctx, const uint32_t *seg, int64_t npix, uint32_t max_seg_id,
                          uint32_t *seg_size_out)
{
    CHK(enter(ctx));
    if (!seg || !seg_size_out || npix < 0 || npix >= 0x7fffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    const uint32_t n = (uint32_t)npix;
    CHK(buf_ensure(ctx, ctx->seg, (size_t)n * 4));
    CHK(buf_ensure(ctx, ctx->segsz, ((size_t)max_seg_id + 2) * 4));
    if (n) HIPCHK(ctx, hipMemcpyAsync(ctx->seg.p, seg, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    // ids above max_seg_id would index out of bounds: verify on the host copy first
    for (uint32_t i = 0; i < n; i++)
        if (seg[i] > max_seg_id) SHP_FAIL(ctx, SHP_ERR_ARG, "segment id %u > max_seg_id %u", seg[i], max_seg_id);
    CHK(run_seg_size(ctx, bp<uint32_t>(ctx->seg), n, max_seg_id, bp<uint32_t>(ctx->segsz)));
    HIPCHK(ctx, hipMemcpyAsync(seg_size_out, ctx->segsz.p, ((size_t)max_seg_id + 1) * 4,
                               hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

static int check_seg_ids(shp_ctx *ctx, const uint32_t *seg, uint32_t n, uint32_t max_id)
{
    for (uint32_t i = 0; i < n; i++)
        if (seg[i] > max_id) SHP_FAIL(ctx, SHP_ERR_ARG, "segment id %u > max_seg_id %u", seg[i], max_id);
    return 0;
}

API int shp_eliminate_single(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows,
                             int ncols, int four_connected, uint32_t *seg_inout,
                             uint32_t *max_seg_id_inout, uint32_t min_seg_id)
{
    CHK(enter(ctx));
    CHK(check_img_args(ctx, img, dtype, nbands, nrows, ncols));
    if (!seg_inout || !max_seg_id_inout) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (min_seg_id < 1u) SHP_FAIL(ctx, SHP_ERR_ARG, "min_seg_id must be >= 1");
    const uint32_t n = (uint32_t)nrows * (uint32_t)ncols;
    if (n == 0) return 0;
    CHK(check_seg_ids(ctx, seg_inout, n, *max_seg_id_inout));
    CHK(upload_img(ctx, img, dtype, nbands, n));
    CHK(buf_ensure(ctx, ctx->seg, (size_t)n * 4));
    HIPCHK(ctx, hipMemcpyAsync(ctx->seg.p, seg_inout, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    CHK(run_eliminate_single(ctx, ctx->img.p, dtype, nbands, nrows, ncols, four_connected,
                             bp<uint32_t>(ctx->seg), max_seg_id_inout, 0, 0, 0, nullptr, min_seg_id));
    HIPCHK(ctx, hipMemcpyAsync(seg_inout, ctx->seg.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

API int shp_eliminate_small(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows,
                            int ncols, int four_connected, int min_seg_size,
                            double max_spectral_diff, uint32_t *seg_inout,
                            uint32_t *max_seg_id_inout, int64_t *num_elim_out, uint32_t min_seg_id)
{
    CHK(enter(ctx));
    CHK(check_img_args(ctx, img, dtype, nbands, nrows, ncols));
    if (!seg_inout || !max_seg_id_inout) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (min_seg_id < 1u) SHP_FAIL(ctx, SHP_ERR_ARG, "min_seg_id must be >= 1");
    const uint32_t n = (uint32_t)nrows * (uint32_t)ncols;
    if (num_elim_out) *num_elim_out = 0;
    if (n == 0) return 0;
    CHK(check_seg_ids(ctx, seg_inout, n, *max_seg_id_inout));
    CHK(upload_img(ctx, img, dtype, nbands, n));
    CHK(buf_ensure(ctx, ctx->seg, (size_t)n * 4));
    HIPCHK(ctx, hipMemcpyAsync(ctx->seg.p, seg_inout, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    int64_t ne = 0;
    CHK(run_eliminate_small(ctx, ctx->img.p, dtype, nbands, nrows, ncols, four_connected,
                            min_seg_size, max_spectral_diff, bp<uint32_t>(ctx->seg),
                            max_seg_id_inout, &ne, 0, nullptr, min_seg_id));
    if (num_elim_out) *num_elim_out = ne;
    HIPCHK(ctx, hipMemcpyAsync(seg_inout, ctx->seg.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

API int shp_segment_locations(shp_ctx *ctx, const uint32_t *seg, int nrows, int ncols, uint32_t max_seg_id,
                              uint32_t *offsets_out, uint32_t *pix_out)
{
    CHK(enter(ctx));
    if (!seg || !offsets_out || !pix_out || nrows < 0 || ncols < 0 ||
        (uint64_t)nrows * (uint64_t)ncols >= 0x7fffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    const uint32_t n = (uint32_t)nrows * (uint32_t)ncols;
    memset(offsets_out, 0, ((size_t)max_seg_id + 2) * 4);
    if (n == 0) return 0;
    CHK(check_seg_ids(ctx, seg, n, max_seg_id));
    CHK(buf_ensure(ctx, ctx->seg, (size_t)n * 4));
    HIPCHK(ctx, hipMemcpyAsync(ctx->seg.p, seg, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    uint32_t *pix = nullptr;
    CHK(run_segment_tables(ctx, bp<uint32_t>(ctx->seg), n, (uint32_t)ncols, max_seg_id, nullptr, 0, 0, &pix));
    HIPCHK(ctx, hipMemcpyAsync(offsets_out, ctx->off.p, ((size_t)max_seg_id + 2) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(pix_out, pix, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

API int shp_build_segment_spectra(shp_ctx *ctx, const uint32_t *seg, const void *img, int dtype, int nbands,
                                  int nrows, int ncols, uint32_t max_seg_id, float *spect_sum_out)
{
    CHK(enter(ctx));
    CHK(check_img_args(ctx, img, dtype, nbands, nrows, ncols));
    if (!seg || !spect_sum_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    const uint32_t n = (uint32_t)nrows * (uint32_t)ncols;
    const size_t nout = ((size_t)max_seg_id + 1) * nbands;
    memset(spect_sum_out, 0, nout * 4);
    if (n == 0) return 0;
    CHK(check_seg_ids(ctx, seg, n, max_seg_id));
    CHK(upload_img(ctx, img, dtype, nbands, n));
    CHK(buf_ensure(ctx, ctx->seg, (size_t)n * 4));
    HIPCHK(ctx, hipMemcpyAsync(ctx->seg.p, seg, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    uint32_t *pix = nullptr;
    CHK(run_segment_tables(ctx, bp<uint32_t>(ctx->seg), n, (uint32_t)ncols, max_seg_id, ctx->img.p, dtype, nbands, &pix));
    HIPCHK(ctx, hipMemcpyAsync(spect_sum_out, ctx->ssum.p, nout * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// Device-resident fused pipeline on ctx->img -> ctx->seg.  Records stage events 1..5.
static int segment_device(shp_ctx *ctx, const void *d_img, uint32_t *d_seg, int dtype, int nb,
                          uint32_t nrows, uint32_t ncols,
                          const double *centres, int k, int has_null, int64_t null_val, int four,
                          int min_seg_size, double msd, uint32_t *max_seg_id, int64_t *singles,
                          int64_t *small, uint32_t *nclumps_out, const uint16_t *clus_window = nullptr,
                          uint32_t clus_pitch = 0, const ImgGeom *geom = nullptr)
{
    const uint32_t n = nrows * ncols;
    CHK(buf_ensure(ctx, ctx->small, 4096));
    uint32_t *scal = bp<uint32_t>(ctx->small);
    hipEventRecord(ctx->ev[1], ctx->stream);
    const uint16_t *d_clus = clus_window;       // the tile's window of a raster-wide cluster map, read in place
    if (!d_clus) {
        CHK(buf_ensure(ctx, ctx->clus, (size_t)n * 2));
        CHK(launch_assign(ctx, d_img, dtype, nb, n, centres, k, has_null, null_val,
                          bp<uint16_t>(ctx->clus), nullptr));
        d_clus = bp<uint16_t>(ctx->clus);
        clus_pitch = ncols;
    }
    hipEventRecord(ctx->ev[2], ctx->stream);
    CHK(buf_ensure(ctx, ctx->segsz, ((size_t)n + 2) * 4));
    CHK(buf_ensure(ctx, ctx->singles, ((size_t)n + 2) * 4));
    CHK(run_clump(ctx, d_clus, nrows, ncols, four, d_seg, scal + 2, bp<uint32_t>(ctx->segsz),
                  bp<uint32_t>(ctx->singles), scal + 3, clus_pitch));
    // read back: number of clumps, number of one-pixel clumps, null-pixel count (scal[2..4])
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, scal + 2, 12, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t nclumps = ctx->h_pinned[0], nsingles = ctx->h_pinned[1], nnull = ctx->h_pinned[2];
    hipEventRecord(ctx->ev[3], ctx->stream);
    uint32_t max_id = nclumps;
    // (a lone null pixel is itself a size-1 "segment" 0: then fall back to the full scan, N4)
    CHK(run_eliminate_single(ctx, d_img, dtype, nb, nrows, ncols, four, d_seg, &max_id, 1, nnull != 1u,
                             nsingles, geom));
    hipEventRecord(ctx->ev[4], ctx->stream);
    if (singles) *singles = (int64_t)nclumps - (int64_t)max_id;        // shepseg.py:226-227
    int64_t ne = 0;
    CHK(run_eliminate_small(ctx, d_img, dtype, nb, nrows, ncols, four, min_seg_size, msd, d_seg,
                            &max_id, &ne, 1, geom));
    hipEventRecord(ctx->ev[5], ctx->stream);
    if (small) *small = ne;
    if (max_seg_id) *max_seg_id = max_id;
    if (nclumps_out) *nclumps_out = nclumps;
    return 0;
}

API int shp_segment_tile(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows, int ncols,
                         const double *centres, int k, int has_null, int64_t null_val,
                         int four_connected, int min_seg_size, double max_spectral_diff,
                         uint32_t *seg_out, uint32_t *max_seg_id_out, int64_t *singles_elim_out,
                         int64_t *small_elim_out, uint32_t *num_clumps_out)
{
    CHK(enter(ctx));
    CHK(check_img_args(ctx, img, dtype, nbands, nrows, ncols));
    if (!centres || !seg_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    const uint32_t n = (uint32_t)nrows * (uint32_t)ncols;
    if (max_seg_id_out) *max_seg_id_out = 0;
    if (singles_elim_out) *singles_elim_out = 0;
    if (small_elim_out) *small_elim_out = 0;
    if (num_clumps_out) *num_clumps_out = 0;
    if (n == 0) return 0;
    hipEventRecord(ctx->ev[0], ctx->stream);
    CHK(upload_img(ctx, img, dtype, nbands, n));
    CHK(buf_ensure(ctx, ctx->seg, (size_t)n * 4));
    CHK(segment_device(ctx, ctx->img.p, bp<uint32_t>(ctx->seg), dtype, nbands, nrows, ncols, centres, k, has_null, null_val,
                       four_connected, min_seg_size, max_spectral_diff, max_seg_id_out,
                       singles_elim_out, small_elim_out, num_clumps_out));
    HIPCHK(ctx, hipMemcpyAsync(seg_out, ctx->seg.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
    hipEventRecord(ctx->ev[6], ctx->stream);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    collect_timings(ctx);
    return 0;
}

// ---- synthetic imagery ----------------------------------------------------------------------
API int shp_synthimg(shp_ctx *ctx, uint64_t seed, int nbands, int64_t y0, int64_t x0, int nrows,
                     int ncols, uint16_t *out_host)
{
    CHK(enter(ctx));
    if (!out_host || nbands < 1 || nrows < 0 || ncols < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    const size_t total = (size_t)nbands * nrows * ncols;
    if (total == 0) return 0;
    CHK(buf_ensure(ctx, ctx->img, total * 2));
    hipLaunchKernelGGL(k_synthimg, dim3(grid_for(total, 256, 65535u * 8u)), dim3(256), 0, ctx->stream,
                       seed, nbands, y0, x0, (uint32_t)nrows, (uint32_t)ncols, bp<uint16_t>(ctx->img));
    KCHK(ctx);
    HIPCHK(ctx, hipMemcpyAsync(out_host, ctx->img.p, total * 2, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

static void collect_timings(shp_ctx *ctx)
{
    prof_collect(ctx);
    ctx->timings[0] = ev_ms(ctx, 1, 2);
    ctx->timings[1] = ev_ms(ctx, 2, 3);
    ctx->timings[2] = ev_ms(ctx, 3, 4);
    ctx->timings[3] = ev_ms(ctx, 4, 5);
    ctx->timings[4] = ev_ms(ctx, 0, 1);
    ctx->timings[5] = ev_ms(ctx, 5, 6);
    ctx->timings[6] = ev_ms(ctx, 0, 6);
}

// ---- device-resident rasters (tiled driver, benchmark) ----------------------------------------
API int shp_dev_alloc(shp_ctx *ctx, size_t bytes, void **dptr)
{
    CHK(enter(ctx));
    if (!dptr) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    *dptr = nullptr;
    hipError_t e = hipMalloc(dptr, bytes ? bytes : 16);
    if (e != hipSuccess) SHP_FAIL(ctx, SHP_ERR_NOMEM, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return 0;
}

API int shp_dev_free(shp_ctx *ctx, void *dptr)
{
    CHK(enter(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (dptr) HIPCHK(ctx, hipFree(dptr));
    return 0;
}

API int shp_dev_upload(shp_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes)
{
    CHK(enter(ctx));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst_dev, src_host, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

API int shp_dev_download(shp_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes)
{
    CHK(enter(ctx));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst_host, src_dev, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// pinned (page-locked) host memory for the raster I/O pipeline: transfers from / to it run at full
// PCIe rate and asynchronously, pageable memory is staged by the runtime in small synchronous pieces
API int shp_host_alloc(shp_ctx *ctx, size_t bytes, void **hptr)
{
    CHK(enter(ctx));
    if (!hptr) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    *hptr = nullptr;
    hipError_t e = hipHostMalloc(hptr, bytes ? bytes : 16, hipHostMallocDefault);
    if (e != hipSuccess) SHP_FAIL(ctx, SHP_ERR_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return 0;
}

API int shp_host_free(shp_ctx *ctx, void *hptr)
{
    CHK(enter(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (hptr) HIPCHK(ctx, hipHostFree(hptr));
    return 0;
}

API int shp_dev_copy(shp_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes)
{
    CHK(enter(ctx));
    if (bytes) HIPCHK(ctx, hipMemcpyAsync(dst_dev, src_dev, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

API int shp_dev_memset(shp_ctx *ctx, void *dst_dev, int value, size_t bytes)
{
    CHK(enter(ctx));
    if (bytes) HIPCHK(ctx, hipMemsetAsync(dst_dev, value, bytes, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// ---- the shared primitives on their own (prims.h; for the tests) -------------------------------
API int shp_prim_scan(shp_ctx *ctx, const uint32_t *d_in, uint64_t n, uint32_t *d_out, int flags,
                      uint32_t *total_dev_out, uint32_t *total_mirror_out, uint32_t *d_boff_out, uint32_t *nboff_out)
{
    CHK(enter(ctx));
    if (!d_in || !d_out || !total_dev_out || !total_mirror_out || ((flags & 2) && (!d_boff_out || !nboff_out)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (n >= 0x100000000ull || (flags & ~3)) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    return run_prim_scan(ctx, d_in, (uint32_t)n, d_out, flags, total_dev_out, total_mirror_out, d_boff_out, nboff_out);
}

API int shp_prim_sort(shp_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, uint64_t n, int bits, int flags,
                      uint32_t *d_keys_out, uint32_t *d_vals_out, uint32_t *digit_starts_out)
{
    CHK(enter(ctx));
    if (!d_keys || !d_vals_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (n >= 0x100000000ull || bits < 0 || bits > 32 || (flags & ~1)) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    return run_prim_sort(ctx, d_keys, d_vals, (uint32_t)n, bits, flags, d_keys_out, d_vals_out, digit_starts_out);
}

API int shp_dev_synthimg(shp_ctx *ctx, uint64_t seed, int nbands, int64_t y0, int64_t x0, int nrows,
                         int ncols, void *d_out)
{
    CHK(enter(ctx));
    if (!d_out || nbands < 1 || nrows < 0 || ncols < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    const size_t total = (size_t)nbands * nrows * ncols;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_synthimg, dim3(grid_for(total, 256, 65535u * 8u)), dim3(256), 0, ctx->stream,
                       seed, nbands, y0, x0, (uint32_t)nrows, (uint32_t)ncols, (uint16_t *)d_out);
    KCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// synthetic label raster for the statistics benchmark (BASELINE config 5): bh x bw-pixel blocks
// numbered row-major from 1; returns the largest id
__global__ __launch_bounds__(256) void k_block_labels(uint32_t nrows, uint32_t ncols, uint32_t bh, uint32_t bw,
                                                      uint32_t ncb, uint32_t *__restrict__ out)
{
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (size_t)nrows * ncols) return;
    const uint32_t r = (uint32_t)(i / ncols), c = (uint32_t)(i - (size_t)r * ncols);
    out[i] = (r / bh) * ncb + c / bw + 1u;
}

API int shp_dev_block_labels(shp_ctx *ctx, int nrows, int ncols, int block_rows, int block_cols,
                             uint32_t *d_out, uint32_t *max_id_out)
{
    CHK(enter(ctx));
    if (!d_out || nrows < 0 || ncols < 0 || block_rows < 1 || block_cols < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    const uint64_t ncb = ((uint64_t)ncols + block_cols - 1) / block_cols, nrb = ((uint64_t)nrows + block_rows - 1) / block_rows;
    if (ncb * nrb >= 0xffffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "too many blocks");
    if (max_id_out) *max_id_out = (uint32_t)(ncb * nrb);
    const size_t total = (size_t)nrows * ncols;
    if (total == 0) return 0;
    hipLaunchKernelGGL(k_block_labels, dim3(grid_for(total, 256)), dim3(256), 0, ctx->stream, (uint32_t)nrows,
                       (uint32_t)ncols, (uint32_t)block_rows, (uint32_t)block_cols, (uint32_t)ncb, d_out);
    KCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// gather rows y0,y0+ystep.. / cols likewise of every band of a device raster into a host array
__global__ __launch_bounds__(256) void k_subsample(const void *__restrict__ img, int dtype, int nb,
                                                   uint32_t rows, uint32_t cols,
                                                   const uint32_t *__restrict__ ry,
                                                   const uint32_t *__restrict__ rx, uint32_t ny,
                                                   uint32_t nx, void *__restrict__ out)
{
    const size_t total = (size_t)nb * ny * nx;
    const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    const size_t b = i / ((size_t)ny * nx), r = (i / nx) % ny, c = i % nx;
    const size_t src = b * (size_t)rows * cols + (size_t)ry[r] * cols + rx[c];
    switch (dtype) {
    case SHP_U8: ((uint8_t *)out)[i] = ((const uint8_t *)img)[src]; break;
    case SHP_I16: case SHP_U16: ((uint16_t *)out)[i] = ((const uint16_t *)img)[src]; break;
    default: ((uint32_t *)out)[i] = ((const uint32_t *)img)[src]; break;
    }
}

API int shp_dev_subsample(shp_ctx *ctx, const void *d_img, int dtype, int nbands, int nrows, int ncols,
                          const uint32_t *row_idx, int ny, const uint32_t *col_idx, int nx,
                          void *out_host)
{
    CHK(enter(ctx));
    if (!d_img || !row_idx || !col_idx || !out_host || dtype_size(dtype) == 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    const size_t total = (size_t)nbands * ny * nx;
    if (total == 0) return 0;
    CHK(buf_ensure(ctx, ctx->aux, total * dtype_size(dtype)));
    CHK(buf_ensure(ctx, ctx->aux2, ((size_t)ny + nx) * 4));
    uint32_t *ry = bp<uint32_t>(ctx->aux2), *rx = ry + ny;
    HIPCHK(ctx, hipMemcpyAsync(ry, row_idx, (size_t)ny * 4, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(rx, col_idx, (size_t)nx * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_subsample, dim3(grid_for(total, 256)), dim3(256), 0, ctx->stream, d_img, dtype,
                       nbands, (uint32_t)nrows, (uint32_t)ncols, ry, rx, (uint32_t)ny, (uint32_t)nx,
                       ctx->aux.p);
    KCHK(ctx);
    // through the context's pinned staging buffer: a pageable destination makes the runtime stage
    // the copy itself in small synchronous pieces (1-30 ms for 12 MB, erratic)
    const size_t bytes = total * dtype_size(dtype);
    if (ctx->h_fit_cap < bytes) {
        if (ctx->h_fit) hipHostFree(ctx->h_fit);
        ctx->h_fit = nullptr; ctx->h_fit_cap = 0;
        if (hipHostMalloc((void **)&ctx->h_fit, bytes, hipHostMallocDefault) != hipSuccess)
            SHP_FAIL(ctx, SHP_ERR_NOMEM, "hipHostMalloc(%zu) failed", bytes);
        ctx->h_fit_cap = bytes;
    }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_fit, ctx->aux.p, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    memcpy(out_host, ctx->h_fit, bytes);
    return 0;
}

// copy window (x, y, xs, ys) of every band of a device raster into a contiguous tile image:
// blockIdx.x = (band, window row), a thread moves 16 bytes of the row (one vector load / store
// when both ends are 16-byte aligned, element by element otherwise)
__global__ __launch_bounds__(256) void k_window(const uint8_t *__restrict__ img, uint32_t esize,
                                                uint32_t rows, uint32_t cols, uint32_t x, uint32_t y,
                                                uint32_t xs, uint32_t ys, uint8_t *__restrict__ out)
{
    const uint32_t br = blockIdx.x, b = br / ys, r = br - b * ys;
    const size_t rowbytes = (size_t)xs * esize;
    const size_t c0 = ((size_t)blockIdx.y * 256u + threadIdx.x) * 16u;         // byte offset in the row
    if (c0 >= rowbytes) return;
    const uint8_t *src = img + (((size_t)b * rows + (y + r)) * cols + x) * esize + c0;
    uint8_t *dst = out + (size_t)br * rowbytes + c0;
    if (c0 + 16u <= rowbytes && ((((uintptr_t)src) | ((uintptr_t)dst)) & 15u) == 0u) {
        *(uint4 *)dst = *(const uint4 *)src;
    } else {
        const uint32_t nbytes = rowbytes - c0 < 16u ? (uint32_t)(rowbytes - c0) : 16u;
        for (uint32_t i = 0; i < nbytes; i++) dst[i] = src[i];
    }
}

API int shp_segment_window_dev(shp_ctx *ctx, const void *d_img, int dtype, int nbands, int img_rows,
                               int img_cols, int x, int y, int xs, int ys, const double *centres, int k,
                               int has_null, int64_t null_val, int four_connected, int min_seg_size,
                               double max_spectral_diff, uint32_t *d_seg_out, uint32_t *max_seg_id_out,
                               int64_t *singles_elim_out, int64_t *small_elim_out,
                               uint32_t *num_clumps_out, const uint16_t *d_clusmap)
{
    CHK(enter(ctx));
    if (!d_img || !centres || !d_seg_out || dtype_size(dtype) == 0 || nbands < 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (x < 0 || y < 0 || xs < 0 || ys < 0 || (int64_t)x + xs > img_cols || (int64_t)y + ys > img_rows)
        SHP_FAIL(ctx, SHP_ERR_ARG, "window (%d,%d,%d,%d) outside the %d x %d raster", x, y, xs, ys, img_rows, img_cols);
    if ((uint64_t)xs * (uint64_t)ys >= 0x7fffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "tile too large");
    const uint32_t n = (uint32_t)xs * (uint32_t)ys;
    if (max_seg_id_out) *max_seg_id_out = 0;
    if (singles_elim_out) *singles_elim_out = 0;
    if (small_elim_out) *small_elim_out = 0;
    if (num_clumps_out) *num_clumps_out = 0;
    if (n == 0) return 0;
    FillScope fs(ctx, 1);
    fill_acquire(ctx, 0);
    hipEventRecord(ctx->ev[0], ctx->stream);
    // With the cluster map nothing reads the tile as a contiguous image any more: the single-pixel
    // and spectra kernels read the window of the resident raster in place (ImgGeom).  Without it
    // the assign step wants the compact copy.
    const void *tile_img = d_img;
    ImgGeom geom = geom_compact(n, (uint32_t)xs);
    if (d_clusmap) {
        geom.bstride = (size_t)img_rows * (size_t)img_cols;
        geom.origin = (size_t)y * (size_t)img_cols + (size_t)x;
        geom.pitch = (uint32_t)img_cols;
        // (the connected-component kernels read the window of the raster-wide cluster map in place too)
    } else if (!(x == 0 && y == 0 && xs == img_cols && ys == img_rows)) {
        const size_t total = (size_t)nbands * n;
        CHK(buf_ensure(ctx, ctx->img, total * dtype_size(dtype)));
        const size_t rowbytes = (size_t)xs * dtype_size(dtype);
        hipLaunchKernelGGL(k_window, dim3((unsigned)nbands * (unsigned)ys, grid_for((rowbytes + 15) / 16, 256)),
                           dim3(256), 0, ctx->stream, (const uint8_t *)d_img, (uint32_t)dtype_size(dtype),
                           (uint32_t)img_rows, (uint32_t)img_cols, (uint32_t)x, (uint32_t)y, (uint32_t)xs,
                           (uint32_t)ys, (uint8_t *)ctx->img.p);
        KCHK(ctx);
        tile_img = ctx->img.p;
    }
    const uint16_t *clus_window = d_clusmap ? (const uint16_t *)d_clusmap + (size_t)y * (size_t)img_cols + (size_t)x : nullptr;
    CHK(segment_device(ctx, tile_img, d_seg_out, dtype, nbands, ys, xs, centres, k, has_null, null_val,
                       four_connected, min_seg_size, max_spectral_diff, max_seg_id_out,
                       singles_elim_out, small_elim_out, num_clumps_out, clus_window, (uint32_t)img_cols, &geom));
    hipEventRecord(ctx->ev[6], ctx->stream);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    collect_timings(ctx);
    return 0;
}

// Clusters of rectangles of a device raster into a raster-wide cluster map (uint16, the raster's
// geometry): 0 = null pixel, else cluster index + 1, exactly what the per-tile assign step writes.
// rects: nrects x (x, y, xs, ys).  Synchronous.
API int shp_assign_rects_dev(shp_ctx *ctx, const void *d_img, int dtype, int nbands, int img_rows,
                             int img_cols, const int32_t *rects, int nrects, const double *centres,
                             int k, int has_null, int64_t null_val, uint16_t *d_clusmap)
{
    CHK(enter(ctx));
    if (!d_img || !centres || !d_clusmap || dtype_size(dtype) == 0 || nbands < 1 || nrects < 0 ||
        (nrects > 0 && !rects) || img_rows < 0 || img_cols < 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    for (int r = 0; r < nrects; r++) {
        const int32_t *q = rects + 4 * r;
        if (q[0] < 0 || q[1] < 0 || q[2] < 0 || q[3] < 0 || (int64_t)q[0] + q[2] > img_cols ||
            (int64_t)q[1] + q[3] > img_rows)
            SHP_FAIL(ctx, SHP_ERR_ARG, "rectangle (%d,%d,%d,%d) outside the %d x %d raster", q[0], q[1], q[2],
                     q[3], img_rows, img_cols);
    }
    if (nrects == 0) return 0;
    FillScope fs(ctx, 1);
    fill_acquire(ctx, 0);
    CHK(launch_assign(ctx, d_img, dtype, nbands, (size_t)img_rows * (size_t)img_cols, centres, k, has_null,
                      null_val, d_clusmap, nullptr, rects, nrects, (uint32_t)img_cols));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// host tile in, device labels out (file-based tiled driver: read -> H2D -> segment, labels stay in HBM)
API int shp_segment_tile_to_dev(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows,
                                int ncols, const double *centres, int k, int has_null, int64_t null_val,
                                int four_connected, int min_seg_size, double max_spectral_diff,
                                uint32_t *d_seg_out, uint32_t *max_seg_id_out,
                                int64_t *singles_elim_out, int64_t *small_elim_out,
                                uint32_t *num_clumps_out)
{
    CHK(enter(ctx));
    CHK(check_img_args(ctx, img, dtype, nbands, nrows, ncols));
    if (!centres || !d_seg_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    const uint32_t n = (uint32_t)nrows * (uint32_t)ncols;
    if (max_seg_id_out) *max_seg_id_out = 0;
    if (singles_elim_out) *singles_elim_out = 0;
    if (small_elim_out) *small_elim_out = 0;
    if (num_clumps_out) *num_clumps_out = 0;
    if (n == 0) return 0;
    FillScope fs(ctx, 1);
    hipEventRecord(ctx->ev[0], ctx->stream);
    CHK(upload_img(ctx, img, dtype, nbands, n));          // (PCIe: outside the gate)
    if (ctx->shared) HIPCHK(ctx, hipStreamSynchronize(ctx->stream));     // (the phases run on borrowed streams)
    fill_acquire(ctx, 0);
    CHK(segment_device(ctx, ctx->img.p, d_seg_out, dtype, nbands, nrows, ncols, centres, k, has_null,
                       null_val, four_connected, min_seg_size, max_spectral_diff, max_seg_id_out,
                       singles_elim_out, small_elim_out, num_clumps_out));
    hipEventRecord(ctx->ev[6], ctx->stream);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    collect_timings(ctx);
    return 0;
}

API int shp_stitch_tile_dev(shp_ctx *ctx, uint32_t *d_tile, int ys, int xs, int overlap,
                            const uint32_t *d_top_b, int64_t top_pitch, const uint32_t *d_left_b,
                            int64_t left_pitch, uint32_t max_local, int simple_recode,
                            uint32_t *d_max_seg_id, int top, int bottom, int left, int right,
                            uint32_t *d_out, int64_t out_pitch, int xout, int yout)
{
    CHK(enter(ctx));
    if (!d_tile || !d_max_seg_id || !d_out || ys < 0 || xs < 0 || overlap < 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (top < 0 || left < 0 || bottom > ys || right > xs || top > bottom || left > right)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad trimmed window");
    return run_stitch_tile(ctx, d_tile, (uint32_t)ys, (uint32_t)xs, (uint32_t)overlap, d_top_b,
                           (size_t)top_pitch, d_left_b, (size_t)left_pitch, max_local, simple_recode,
                           d_max_seg_id, (uint32_t)top, (uint32_t)bottom, (uint32_t)left,
                           (uint32_t)right, d_out, (size_t)out_pitch, (uint32_t)xout, (uint32_t)yout);
}

API int shp_sync(shp_ctx *ctx)
{
    CHK(enter(ctx));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->stream2) HIPCHK(ctx, hipStreamSynchronize(ctx->stream2));
    return 0;
}

API int shp_stitch_prepare_dev(shp_ctx *ctx, const uint32_t *d_tile, int ys, int xs, int overlap,
                               int has_top, int has_left, uint32_t max_local, int top, int bottom,
                               int left, int right, uint32_t *d_meta, uint32_t *cross_px_out)
{
    CHK(enter(ctx));
    if (!d_tile || !d_meta || ys < 0 || xs < 0 || overlap < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (top < 0 || left < 0 || bottom > ys || right > xs || top > bottom || left > right)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad trimmed window");
    FillScope fs(ctx, 1);
    fill_acquire(ctx, 3);
    uint32_t *d_cross = nullptr;
    if (cross_px_out) {
        CHK(buf_ensure(ctx, ctx->small, 4096));
        d_cross = bp<uint32_t>(ctx->small) + 64;
        HIPCHK(ctx, hipMemsetAsync(d_cross, 0, 8, ctx->stream));
    }
    CHK(run_stitch_prepare(ctx, d_tile, (uint32_t)ys, (uint32_t)xs, (uint32_t)overlap, has_top, has_left,
                           max_local, (uint32_t)top, (uint32_t)bottom, (uint32_t)left, (uint32_t)right,
                           d_meta, d_cross));
    if (cross_px_out) HIPCHK(ctx, hipMemcpyAsync(ctx->h_pinned, d_cross, 8, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (cross_px_out) { cross_px_out[0] = ctx->h_pinned[0]; cross_px_out[1] = ctx->h_pinned[1]; }
    return 0;
}

API int shp_stitch_chain_dev(shp_ctx *ctx, const uint32_t *d_tile, int ys, int xs, int overlap,
                             const uint32_t *d_top_b, int64_t top_pitch, const uint32_t *d_left_b,
                             int64_t left_pitch, uint32_t max_local, int simple_recode,
                             uint32_t *d_max_seg_id, int top, int bottom, int left, int right,
                             uint32_t *d_meta, uint32_t *d_right_out, uint32_t *d_bottom_out,
                             uint32_t *d_out, int64_t out_pitch, int xout, int yout,
                             uint32_t top_cross_px, uint32_t left_cross_px)
{
    CHK(enter(ctx));
    if (!d_tile || !d_max_seg_id || !d_meta || ys < 0 || xs < 0 || overlap < 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (top < 0 || left < 0 || bottom > ys || right > xs || top > bottom || left > right)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad trimmed window");
    CHK(run_stitch_chain(ctx, d_tile, (uint32_t)ys, (uint32_t)xs, (uint32_t)overlap, d_top_b,
                         (size_t)top_pitch, d_left_b, (size_t)left_pitch, max_local, simple_recode,
                         d_max_seg_id, (uint32_t)top, (uint32_t)bottom, (uint32_t)left, (uint32_t)right,
                         d_meta, d_right_out, d_bottom_out, top_cross_px, left_cross_px));
    if (d_out)
        CHK(run_stitch_finish(ctx, d_tile, (uint32_t)ys, (uint32_t)xs, max_local, (uint32_t)top,
                              (uint32_t)bottom, (uint32_t)left, (uint32_t)right, d_meta, d_out,
                              (size_t)out_pitch, (uint32_t)xout, (uint32_t)yout));
    return 0;
}

// one trimmed tile's contribution to one overview layer; runs behind the tile's output write on the
// context's side stream (shp_stitch_chain_dev), so the chain itself is not held up
// Parallel stitch.  After shp_stitch_chain_dev ran with
// *d_max_seg_id = base (the tile's provisional base): d_out2[0] = number of new ids the tile handed
// out, d_out2[1] = the largest of them (minus base) present in its trimmed window.  Asynchronous.
API int shp_stitch_counts_dev(shp_ctx *ctx, const uint32_t *d_meta, uint32_t max_local, uint32_t base,
                              uint32_t *d_out2)
{
    CHK(enter(ctx));
    if (!d_meta || !d_out2) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    const uint32_t nseg = max_local + 1u;
    HIPCHK(ctx, hipMemsetAsync(d_out2, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_lut_counts, dim3(grid_for(nseg, 256)), dim3(256), 0, ctx->stream,
                       d_meta + 3 * (size_t)nseg, d_meta, nseg, base, d_out2);
    KCHK(ctx);
    return 0;
}

// Provisional ids -> final ids over a device raster: id -> new_base[id / stride] + id % stride
// (0 stays 0; new_base: ntiles host values).  Synchronous.
API int shp_renumber_dev(shp_ctx *ctx, uint32_t *d_raster, int64_t npix, uint32_t stride,
                         const uint32_t *new_base, int ntiles)
{
    CHK(enter(ctx));
    if ((!d_raster && npix) || !new_base || ntiles < 1 || stride == 0 || npix < 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (npix == 0) return 0;
    CHK(buf_ensure(ctx, ctx->tlist, (size_t)ntiles * 4));
    HIPCHK(ctx, hipMemcpyAsync(ctx->tlist.p, new_base, (size_t)ntiles * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_renumber, dim3(grid_for((size_t)npix, 256)), dim3(256), 0, ctx->stream, d_raster,
                       (size_t)npix, stride, bp<uint32_t>(ctx->tlist), (uint32_t)ntiles);
    KCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

API int shp_overview_window_dev(shp_ctx *ctx, const uint32_t *d_raster, int64_t pitch, int xout, int yout,
                                int w, int h, int level, uint32_t *d_ov, int ov_w, int ov_h)
{
    CHK(enter(ctx));
    if (!d_raster || !d_ov || pitch < 0 || xout < 0 || yout < 0 || w < 0 || h < 0 || level < 1 || ov_w < 0 || ov_h < 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    const uint32_t o = (uint32_t)level / 2u;
    const uint64_t nsr = (uint32_t)h > o ? ((uint32_t)h - o + level - 1u) / level : 0u;
    const uint64_t nsc = (uint32_t)w > o ? ((uint32_t)w - o + level - 1u) / level : 0u;
    if (nsr * nsc == 0) return 0;
    if (nsr * nsc >= 0x7fffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "window too large");
    CHK(ensure_stream2(ctx));
    hipLaunchKernelGGL(k_overview_window, dim3(grid_for((size_t)(nsr * nsc), 256)), dim3(256), 0, ctx->stream2, d_raster,
                       (size_t)pitch, (uint32_t)xout, (uint32_t)yout, (uint32_t)w, (uint32_t)h, (uint32_t)level, d_ov,
                       (uint32_t)ov_w, (uint32_t)ov_h);
    KCHK(ctx);
    return 0;
}

// a table of overview rectangles against the npix pixels of the raster they sample and the packed buffer they fill
// (shp_overview_rects_dev, shp_colour_overview_rects_dev)
static int overview_rects_check(shp_ctx *ctx, int64_t npix, const int64_t *rects, int nrects, int64_t npacked)
{
    int64_t at = 0;
    for (int k = 0; k < nrects; k++) {
        const int64_t *q = rects + 6 * (size_t)k;
        const int64_t src0 = q[0], rs = q[1], cs = q[2], nr = q[3], nc = q[4];
        if (nr < 1 || nc < 1 || rs < 0 || cs < 0 || src0 < 0 || q[5] != at || nr > npacked || nc > npacked)
            SHP_FAIL(ctx, SHP_ERR_ARG, "overview rectangle %d is malformed", k);
        int64_t room = npix - 1 - src0;             // the last pixel read, src0 + (nr - 1) rs + (nc - 1) cs, < npix
        if (room < 0 || (rs > 0 && nr - 1 > room / rs))
            SHP_FAIL(ctx, SHP_ERR_ARG, "overview rectangle %d reads past the raster", k);
        room -= (nr - 1) * rs;
        if (cs > 0 && nc - 1 > room / cs) SHP_FAIL(ctx, SHP_ERR_ARG, "overview rectangle %d reads past the raster", k);
        if (nr * nc > npacked - at) SHP_FAIL(ctx, SHP_ERR_ARG, "overview rectangles overrun the packed buffer");
        at += nr * nc;
    }
    if (at != npacked) SHP_FAIL(ctx, SHP_ERR_ARG, "overview rectangles fill %lld of %lld packed pixels",
                                (long long)at, (long long)npacked);
    return 0;
}

// overview rectangles of a row-sharded raster, every level in one launch (k_overview_rects); the table is
// checked here, on the host, so that no rectangle reads outside the npix pixels of d_raster.  Synchronous.
API int shp_overview_rects_dev(shp_ctx *ctx, const uint32_t *d_raster, int64_t npix, const int64_t *rects,
                               int nrects, uint32_t *d_packed, int64_t npacked)
{
    CHK(enter(ctx));
    if (npix < 0 || nrects < 0 || npacked < 0 || (nrects > 0 && !rects) || (npacked > 0 && (!d_raster || !d_packed)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    CHK(overview_rects_check(ctx, npix, rects, nrects, npacked));
    if (npacked == 0) return 0;
    CHK(buf_ensure(ctx, ctx->tlist, (size_t)nrects * 48));
    HIPCHK(ctx, hipMemcpyAsync(ctx->tlist.p, rects, (size_t)nrects * 48, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_overview_rects, dim3(grid_for((size_t)npacked, 256)), dim3(256), 0, ctx->stream, d_raster,
                       bp<int64_t>(ctx->tlist), (uint32_t)nrects, (uint64_t)npacked, d_packed);
    KCHK(ctx);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// histogram of a device label raster: hist_out[0..max_seg_id], hist_out[0] = 0 (tiling.py:1915-1963).
// ncols > 0 (npix a multiple of it): the raster's row length, which lets the pixels of a segment
// be combined per 2-D patch before they reach the global counters; 0 = unknown (1-D runs).
// numpy's pairwise float64 sum (DOUBLE_pairwise_sum) of term(i), i in [lo, lo + n), for the host (recursion as numpy's)
template <class Term>
static double hist_pairwise(Term term, size_t lo, size_t n)
{
    if (n <= 128) return np_pairwise_sum_lv<0>(term, lo, n);
    size_t n2 = n / 2;
    n2 -= n2 % 8;
    return hist_pairwise(term, lo, n2) + hist_pairwise(term, lo + n2, n - n2);
}

API int shp_hist_stats(const uint32_t *hist, int64_t n, double *out)
{
    if (!hist || !out || n < 1) return SHP_ERR_ARG;
    // mask = hist > 0; nVals = hist.sum(); min / max = first / last non-zero bin; mode = argmax (first maximum)
    uint64_t nvals = 0, wsum = 0;
    int64_t first = -1, last = -1, mode = 0;
    uint32_t best = hist[0];
    for (int64_t i = 0; i < n; i++) {
        const uint32_t h = hist[i];
        nvals += h;
        wsum += (uint64_t)i * h;                        // (values * hist).sum(): int64, exact
        if (h) { if (first < 0) first = i; last = i; }
        if (h > best) { best = h; mode = i; }
    }
    if (first < 0) { first = 0; last = n - 1; }       // all zero: argmax of an all-False mask is 0 on both sides
    const double nv = (double)nvals;
    const double mean = (double)(int64_t)wsum / nv;
    // (hist * power(values - mean, 2)).sum(): float64 terms, pairwise
    auto term = [hist, mean](size_t i) {
        const double d = (double)(int64_t)i - mean;
        const double d2 = d * d;
        return (double)hist[i] * d2;
    };
    // a .sum() over a long contiguous array reaches the pairwise routine 8192 elements (the ufunc buffer
    // size) at a time, the blocks' sums added one after the other (checked against numpy 2.2 up to 2.5 M bins)
    double ssq = 0.0;
    for (size_t lo = 0; lo < (size_t)n; lo += NP_REDUCE_BLOCK) {
        const size_t m = (size_t)n - lo < NP_REDUCE_BLOCK ? (size_t)n - lo : NP_REDUCE_BLOCK;
        const double part = hist_pairwise(term, lo, m);
        ssq = lo ? ssq + part : part;
    }
    const double sd = __builtin_sqrt(ssq / nv);
    // first bin whose cumulative count reaches hist.sum() / 2 (a float64 comparison)
    const double middle = nv / 2.0;
    uint64_t cum = 0;
    int64_t median = 0;
    bool found = false;
    for (int64_t i = 0; i < n; i++) {
        cum += hist[i];
        if ((double)cum >= middle) { median = i; found = true; break; }
    }
    if (!found) return SHP_ERR_STATE;
    out[0] = (double)first; out[1] = (double)last; out[2] = mean; out[3] = sd; out[4] = (double)mode; out[5] = (double)median;
    return 0;
}

API int shp_histogram_dev(shp_ctx *ctx, const uint32_t *d_raster, int64_t npix, int64_t ncols,
                          uint32_t max_seg_id, uint32_t *hist_out_host)
{
    CHK(enter(ctx));
    if (!d_raster || !hist_out_host || npix < 0 || ncols < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (ncols > 0 && (npix % ncols != 0 || ncols > 0x7fffffffll || npix / ncols > 0x7fffffffll))
        SHP_FAIL(ctx, SHP_ERR_ARG, "npix is not a whole number of rows of %lld pixels", (long long)ncols);
    static const bool io_timing = getenv("SHEPSEG_IO_TIMING") != nullptr;
    const auto tt0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (io_timing) fprintf(stderr, "    [hist] %-18s %.2f ms\n", what,
                               std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tt0).count());
    };
    CHK(buf_ensure(ctx, ctx->segsz, ((size_t)max_seg_id + 2) * 4));
    uint32_t *h = bp<uint32_t>(ctx->segsz);
    const size_t hbytes = ((size_t)max_seg_id + 1) * 4;
    lap("workspace");
    HIPCHK(ctx, hipMemsetAsync(h, 0, hbytes, ctx->stream));
    if (ncols > 0 && npix > 0) {
        const uint32_t nc = (uint32_t)ncols;
        const int64_t nrows = npix / ncols, RCH = 65535ll * AGG_ROWS;      // grid.y limit
        for (int64_t r = 0; r < nrows; r += RCH) {
            const uint32_t nr = (uint32_t)((nrows - r < RCH) ? (nrows - r) : RCH);
            hipLaunchKernelGGL(k_hist_patch, dim3(grid_for(nc, 64), grid_for(nr, AGG_ROWS)), dim3(256), 0,
                               ctx->stream, d_raster + (size_t)r * nc, nr, nc, h);
            KCHK(ctx);
        }
    } else {
        const int64_t CH = 1ll << 30;
        for (int64_t o = 0; o < npix; o += CH) {
            const uint32_t m = (uint32_t)((npix - o < CH) ? (npix - o) : CH);
            hipLaunchKernelGGL(k_run_count, dim3(grid_for(m, 256)), dim3(256), 0, ctx->stream, d_raster + o, m,
                               h, 0u, 1);
            KCHK(ctx);
        }
    }
    // read back through pinned staging (a pageable destination: 1-30 ms for 10 MB, erratic)
    if (ctx->h_fit_cap < hbytes) {
        if (ctx->h_fit) hipHostFree(ctx->h_fit);
        ctx->h_fit = nullptr; ctx->h_fit_cap = 0;
        if (hipHostMalloc((void **)&ctx->h_fit, hbytes + hbytes / 4, hipHostMallocDefault) != hipSuccess)
            SHP_FAIL(ctx, SHP_ERR_NOMEM, "hipHostMalloc(%zu) failed", hbytes);
        ctx->h_fit_cap = hbytes + hbytes / 4;
    }
    lap("launched");
    if (io_timing) { HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); lap("kernel done"); }
    HIPCHK(ctx, hipMemcpyAsync(ctx->h_fit, h, hbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    lap("on the host");
    memcpy(hist_out_host, ctx->h_fit, hbytes);
    lap("copied out");
    hist_out_host[0] = 0;
    return 0;
}

// accumulated device time (ms) and launch count of the instrumented kernels of this context:
// ids: 0 assign, 1 ccl (init+merge+flatten), 2 dfs_split, 3 radix sort, 4 spectra,
//      5 small-segment pass loop, 6 (unused), 7 seed scan + final labels.  reset != 0 clears.
API int shp_prof_get(shp_ctx *ctx, double *ms_out, uint64_t *count_out, int n, int reset)
{
    if (!ctx || !ms_out || !count_out) return SHP_ERR_ARG;
    prof_collect(ctx);
    for (int i = 0; i < n && i < PROF_N; i++) { ms_out[i] = ctx->prof_ms[i]; count_out[i] = ctx->prof_cnt[i]; }
    if (reset) for (int i = 0; i < PROF_N; i++) { ctx->prof_ms[i] = 0; ctx->prof_cnt[i] = 0; }
    return 0;
}

// launches, jobs and largest batch of the replay, then of the pass loop (walkbatch.h); process-wide
API int shp_walk_batch_stats(uint64_t *out, int reset)
{
    if (!out) return SHP_ERR_ARG;
    for (int c = 0; c < walkbatch::NCLS; c++) {
        const walkbatch::Stats s = walk_batcher().stats(c, reset != 0);
        out[3 * c] = s.launches; out[3 * c + 1] = s.jobs; out[3 * c + 2] = s.largest;
    }
    return 0;
}

// workgroups summed over all launches and the most in one launch, of the replay, then of the pass loop
API int shp_walk_batch_blocks(uint64_t *out)
{
    if (!out) return SHP_ERR_ARG;
    for (int c = 0; c < walkbatch::NCLS; c++) {
        const walkbatch::Stats s = walk_batcher().stats(c, false);
        out[2 * c] = s.blocks; out[2 * c + 1] = s.most_blocks;
    }
    return 0;
}

// pass-loop launches per instance of k_small_loop (elim_small.h SMALL_INSTANCES): the generic one, then 6 bands
// 4- and 8-connected, then 10 bands 4- and 8-connected; process-wide
API int shp_small_loop_instances(uint64_t *out, int reset)
{
    if (!out) return SHP_ERR_ARG;
    for (int i = 0; i < SMALL_NINST; i++)
        out[i] = reset ? g_small_inst[i].exchange(0ull, std::memory_order_relaxed) : g_small_inst[i].load(std::memory_order_relaxed);
    return 0;
}

// ---- per-segment statistics (tilingstats) -------------------------------------------------------
API int shp_segstats_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                         int64_t npix, uint32_t max_seg_id, int has_null, int64_t null_val,
                         const uint32_t *stats_sel, int nstats, int64_t missing,
                         int64_t *intcols_out, float *floatcols_out)
{
    CHK(enter(ctx));
    if (!d_seg || !d_band || !stats_sel || nstats < 1 || dtype_size(dtype) == 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (npix < 0 || npix >= 0xffffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large (%lld px)", (long long)npix);
    return run_segstats(ctx, d_seg, d_band, dtype, (uint32_t)npix, max_seg_id, has_null, null_val,
                        stats_sel, nstats, missing, intcols_out, floatcols_out);
}

// the same for a raster whose shape is known (nrows x ncols pixels, row-major): lets the library take the
// patch-by-patch path when the segments are small (segstats.h)
API int shp_segstats2d_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                           int64_t nrows, int64_t ncols, uint32_t max_seg_id, int has_null, int64_t null_val,
                           const uint32_t *stats_sel, int nstats, int64_t missing,
                           int64_t *intcols_out, float *floatcols_out)
{
    CHK(enter(ctx));
    if (!d_seg || !d_band || !stats_sel || nstats < 1 || dtype_size(dtype) == 0 || nrows < 0 || ncols < 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (nrows > 0xffffffffll || ncols > 0xffffffffll || nrows * ncols >= 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large (%lld x %lld px)", (long long)nrows, (long long)ncols);
    return run_segstats(ctx, d_seg, d_band, dtype, (uint32_t)(nrows * ncols), max_seg_id, has_null, null_val,
                        stats_sel, nstats, missing, intcols_out, floatcols_out, (uint32_t)nrows, (uint32_t)ncols);
}

API int shp_segstats(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t npix,
                     uint32_t max_seg_id, int has_null, int64_t null_val, const uint32_t *stats_sel,
                     int nstats, int64_t missing, int64_t *intcols_out, float *floatcols_out)
{
    CHK(enter(ctx));
    if (!seg || !band || !stats_sel || nstats < 1 || dtype_size(dtype) == 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (npix < 0 || npix >= 0xffffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large (%lld px)", (long long)npix);
    CHK(buf_ensure(ctx, ctx->seg, (size_t)npix * 4));
    CHK(buf_ensure(ctx, ctx->img, (size_t)npix * dtype_size(dtype)));
    if (npix) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->seg.p, seg, (size_t)npix * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->img.p, band, (size_t)npix * dtype_size(dtype), hipMemcpyHostToDevice,
                                   ctx->stream));
    }
    return run_segstats(ctx, bp<uint32_t>(ctx->seg), ctx->img.p, dtype, (uint32_t)npix, max_seg_id,
                        has_null, null_val, stats_sel, nstats, missing, intcols_out, floatcols_out);
}

API int shp_gather_flagged_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                               int64_t npix, uint32_t max_seg_id, const uint8_t *flags,
                               int64_t cap, uint32_t *seg_out, int64_t *val_out, int64_t *count_out)
{
    CHK(enter(ctx));
    if (!d_seg || !d_band || !flags || !count_out || dtype_size(dtype) == 0 || cap < 0 ||
        (cap > 0 && (!seg_out || !val_out)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (npix < 0 || npix >= 0xffffffffll || cap >= 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large (%lld px)", (long long)npix);
    return run_gather_flagged(ctx, d_seg, d_band, dtype, (uint32_t)npix, max_seg_id, flags, (uint32_t)cap,
                              seg_out, val_out, count_out);
}

// several bands of one image against the same labels in one pass (segstats.h: run_segstats_bands)
API int shp_segstats2d_bands_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *const *d_bands, int dtype, int nbands,
                                 int64_t nrows, int64_t ncols, uint32_t max_seg_id, const int *has_null,
                                 const int64_t *null_val, const uint32_t *stats_sel, const int *nstats_per_band,
                                 int64_t missing, int64_t *intcols_out, float *floatcols_out)
{
    CHK(enter(ctx));
    if (!d_seg || !d_bands || !has_null || !null_val || !stats_sel || !nstats_per_band || nbands < 1 ||
        dtype_size(dtype) == 0 || nrows < 0 || ncols < 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (nrows > 0xffffffffll || ncols > 0xffffffffll || nrows * ncols >= 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large (%lld x %lld px)", (long long)nrows, (long long)ncols);
    return run_segstats_bands(ctx, d_seg, d_bands, dtype, nbands, (uint32_t)nrows, (uint32_t)ncols, max_seg_id, has_null,
                              null_val, stats_sel, nstats_per_band, missing, intcols_out, floatcols_out);
}

API int shp_gather_flagged_bands_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *const *d_bands, int dtype,
                                     int nbands, int64_t npix, uint32_t max_seg_id, const uint8_t *flags, int64_t cap,
                                     uint32_t *seg_out, int64_t *val_out, int64_t *count_out)
{
    CHK(enter(ctx));
    if (!d_seg || !d_bands || nbands < 1 || !flags || !count_out || dtype_size(dtype) == 0 || cap < 0 ||
        (cap > 0 && (!seg_out || !val_out)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (npix < 0 || npix >= 0xffffffffll || cap >= 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large (%lld px)", (long long)npix);
    return run_gather_flagged_bands(ctx, d_seg, d_bands, dtype, nbands, (uint32_t)npix, max_seg_id, flags, (uint32_t)cap,
                                    seg_out, val_out, count_out);
}

// the multi-GPU split with everything left in device memory, over entries (segstats.h: run_dstats_local_bands /
// run_dstats_merge_bands); a one-band caller passes nbands = nplanes = 1
API int shp_dstats_local_bands_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *const *d_planes, int nplanes,
                                   const int *plane_of_band, int dtype, int nbands, int64_t nrows, int64_t ncols,
                                   uint32_t max_seg_id, const int *has_null, const int64_t *null_val,
                                   const uint32_t *stats_sel, const int *nstats_per_band, int64_t missing,
                                   const uint32_t *d_hist, int keep_unheld, void *d_cols, void **d_pair_seg_out,
                                   void **d_pair_val_out, int64_t *pair_row_bytes_out, int64_t *n_pairs_out,
                                   int64_t *n_straddlers_out)
{
    CHK(enter(ctx));
    if (!d_planes || !plane_of_band || !has_null || !null_val || !stats_sel || !nstats_per_band || !d_hist || !d_cols ||
        !d_pair_seg_out || !d_pair_val_out || !pair_row_bytes_out || !n_pairs_out || !n_straddlers_out || nbands < 1 ||
        nplanes < 1 || nplanes > nbands || dtype_size(dtype) == 0 || nrows < 0 || ncols < 0)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (nrows > 0xffffffffll || ncols > 0xffffffffll || nrows * ncols >= 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large (%lld x %lld px)", (long long)nrows, (long long)ncols);
    if (!d_seg && nrows * ncols > 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    for (int p = 0; p < nplanes; p++) if (!d_planes[p]) SHP_FAIL(ctx, SHP_ERR_ARG, "plane %d: no band", p);
    uint32_t *ps = nullptr;
    void *pv = nullptr;
    CHK(run_dstats_local_bands(ctx, d_seg, d_planes, nplanes, plane_of_band, dtype, nbands, (uint32_t)nrows, (uint32_t)ncols,
                               max_seg_id, has_null, null_val, stats_sel, nstats_per_band, missing, d_hist, keep_unheld,
                               d_cols, &ps, &pv, pair_row_bytes_out, n_pairs_out, n_straddlers_out));
    *d_pair_seg_out = ps;
    *d_pair_val_out = pv;
    return 0;
}

API int shp_dstats_merge_bands_dev(shp_ctx *ctx, const uint32_t *d_pair_seg, const void *d_pair_val, int64_t slot,
                                   int64_t slot_row_bytes, int world, const uint32_t *counts, int dtype, int nbands,
                                   int nplanes, const int *plane_of_band, uint32_t max_seg_id, const int *has_null,
                                   const int64_t *null_val, const uint32_t *stats_sel, const int *nstats_per_band,
                                   int64_t missing, uint32_t id_lo, uint32_t id_hi, void *d_cols, int64_t *n_merged_out,
                                   int64_t *n_ids_out)
{
    CHK(enter(ctx));
    if (!plane_of_band || !has_null || !null_val || !stats_sel || !nstats_per_band || !counts || !d_cols || !n_merged_out ||
        !n_ids_out || nbands < 1 || nplanes < 1 || nplanes > nbands || dtype_size(dtype) == 0 || slot < 0 || world < 1 ||
        slot >= 0xffffffffll || slot_row_bytes < 0 || (slot > 0 && (!d_pair_seg || !d_pair_val)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    for (int r = 0; r < world; r++) if ((int64_t)counts[r] > slot) SHP_FAIL(ctx, SHP_ERR_ARG, "counts[%d] exceeds the slot", r);
    return run_dstats_merge_bands(ctx, d_pair_seg, d_pair_val, (uint32_t)slot, (size_t)slot_row_bytes, (uint32_t)world, counts,
                                  dtype, nbands, nplanes, plane_of_band, max_seg_id, has_null, null_val, stats_sel,
                                  nstats_per_band, missing, id_lo, id_hi, d_cols, n_merged_out, n_ids_out);
}

// ---- subset ---------------------------------------------------------------------
static int subset_check(shp_ctx *ctx, int64_t img_rows, int64_t img_cols, int64_t tlx, int64_t tly,
                        int64_t xs, int64_t ys, int tile_size, uint32_t max_seg_id)
{
    if (img_rows < 0 || img_cols < 0 || tlx < 0 || tly < 0 || xs < 0 || ys < 0 || tile_size < 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (tlx + xs > img_cols || tly + ys > img_rows)
        SHP_FAIL(ctx, SHP_ERR_ARG, "Requested subset is not within input image");      // subset.py:86-88
    if ((uint64_t)xs * (uint64_t)ys >= 0xffffffffull || img_cols >= 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "subset too large");
    // max_seg_id + 1 ids are scanned as a 32-bit count
    if (max_seg_id == 0xffffffffu) SHP_FAIL(ctx, SHP_ERR_ARG, "max_seg_id too large");
    return 0;
}

API int shp_subset_recode_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t img_rows, int64_t img_cols,
                              int64_t tlx, int64_t tly, int64_t xs, int64_t ys, const uint8_t *d_mask,
                              int tile_size, uint32_t max_seg_id, uint32_t *d_out, uint32_t *orig_out,
                              uint32_t *hist_out, int64_t cap, uint32_t *n_new_out)
{
    CHK(enter(ctx));
    if (!d_seg || !d_out || !orig_out || !hist_out || !n_new_out || cap < 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(subset_check(ctx, img_rows, img_cols, tlx, tly, xs, ys, tile_size, max_seg_id));
    return run_subset_recode(ctx, d_seg, (uint32_t)img_cols, (uint32_t)tlx, (uint32_t)tly, (uint32_t)xs,
                             (uint32_t)ys, d_mask, (uint32_t)tile_size, max_seg_id, d_out, orig_out,
                             hist_out, cap, n_new_out);
}

API int shp_subset_recode(shp_ctx *ctx, const uint32_t *seg, int64_t img_rows, int64_t img_cols,
                          int64_t tlx, int64_t tly, int64_t xs, int64_t ys, const uint8_t *mask,
                          int tile_size, uint32_t max_seg_id, uint32_t *out, uint32_t *orig_out,
                          uint32_t *hist_out, int64_t cap, uint32_t *n_new_out)
{
    CHK(enter(ctx));
    if (!seg || !out || !orig_out || !hist_out || !n_new_out || cap < 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(subset_check(ctx, img_rows, img_cols, tlx, tly, xs, ys, tile_size, max_seg_id));
    const size_t n = (size_t)xs * (size_t)ys;
    *n_new_out = 0;
    if (n == 0) return 0;
    // only the window travels: rows of xs labels out of a raster of img_cols
    CHK(buf_ensure(ctx, ctx->seg, n * 4));
    CHK(buf_ensure(ctx, ctx->lab, n * 4));
    HIPCHK(ctx, hipMemcpy2DAsync(ctx->seg.p, (size_t)xs * 4, seg + (size_t)tly * img_cols + tlx,
                                 (size_t)img_cols * 4, (size_t)xs * 4, (size_t)ys, hipMemcpyHostToDevice,
                                 ctx->stream));
    uint8_t *d_mask = nullptr;
    if (mask) {
        CHK(buf_ensure(ctx, ctx->clus, n));
        HIPCHK(ctx, hipMemcpyAsync(ctx->clus.p, mask, n, hipMemcpyHostToDevice, ctx->stream));
        d_mask = (uint8_t *)ctx->clus.p;
    }
    CHK(run_subset_recode(ctx, bp<uint32_t>(ctx->seg), (uint32_t)xs, 0u, 0u, (uint32_t)xs, (uint32_t)ys,
                          d_mask, (uint32_t)tile_size, max_seg_id, bp<uint32_t>(ctx->lab), orig_out, hist_out,
                          cap, n_new_out));
    HIPCHK(ctx, hipMemcpyAsync(out, ctx->lab.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

// the recode of a row-sharded window (subset.h: run_dsubset_local / run_dsubset_merge): this rank's rows
// [row0, row0 + nrows) in place, the window rows they hold and the matching mask rows
static int dsubset_geom(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int64_t row0,
                        uint32_t max_seg_id, int64_t tlx, int64_t tly, int64_t xs, int64_t ys, int tile_size,
                        const uint8_t *d_mask, SubsetGeom *g)
{
    if (nrows < 0 || ncols < 0 || row0 < 0 || tlx < 0 || tly < 0 || xs < 0 || ys < 0 || tile_size < 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (tlx + xs > ncols) SHP_FAIL(ctx, SHP_ERR_ARG, "Requested subset is not within input image");
    if ((uint64_t)xs * (uint64_t)ys >= 0xffffffffull || ncols >= 0xffffffffll || row0 + nrows >= 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "subset too large");
    if ((uint64_t)nrows * (uint64_t)ncols >= 0xffffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "shard too large (%lld x %lld px)", (long long)nrows, (long long)ncols);
    if (max_seg_id == 0xffffffffu) SHP_FAIL(ctx, SHP_ERR_ARG, "max_seg_id too large");
    // window rows held: [a, b) = [max(0, row0 - tly), min(ys, row0 + nrows - tly)), empty if b <= a
    const int64_t a = std::min(std::max<int64_t>(0, row0 - tly), ys);
    const int64_t b = std::max(a, std::min(ys, row0 + nrows - tly));
    if (b > a && !d_seg) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    *g = SubsetGeom{d_seg, d_mask, (uint32_t)ncols, (uint32_t)tlx, (uint32_t)tly, (uint32_t)xs, (uint32_t)ys,
                    (uint32_t)tile_size, (uint32_t)row0, (uint32_t)a, (uint32_t)(b - a)};
    return 0;
}

API int shp_dsubset_local_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int64_t row0,
                              uint32_t max_seg_id, int64_t tlx, int64_t tly, int64_t xs, int64_t ys, int tile_size,
                              const uint8_t *d_mask, void **d_pairs_out, int64_t *n_pairs_out, int *bad_out)
{
    CHK(enter(ctx));
    if (!d_pairs_out || !n_pairs_out || !bad_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    SubsetGeom g;
    CHK(dsubset_geom(ctx, d_seg, nrows, ncols, row0, max_seg_id, tlx, tly, xs, ys, tile_size, d_mask, &g));
    return run_dsubset_local(ctx, g, max_seg_id, d_pairs_out, n_pairs_out, bad_out);
}

API int shp_dsubset_merge_dev(shp_ctx *ctx, const void *d_pairs, int64_t slot, int world, const uint32_t *counts,
                              const uint32_t *d_seg, int64_t nrows, int64_t ncols, int64_t row0, uint32_t max_seg_id,
                              int64_t tlx, int64_t tly, int64_t xs, int64_t ys, int tile_size, const uint8_t *d_mask,
                              uint32_t *d_out, uint32_t *d_hist, uint32_t *orig_out, int64_t cap,
                              uint32_t *n_new_out)
{
    CHK(enter(ctx));
    if (!counts || !d_hist || !orig_out || !n_new_out || cap < 1 || slot < 0 || world < 1 ||
        (slot > 0 && !d_pairs) || (uint64_t)slot * (uint64_t)world >= 0x7fffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    for (int r = 0; r < world; r++) if ((int64_t)counts[r] > slot) SHP_FAIL(ctx, SHP_ERR_ARG, "counts[%d] exceeds the slot", r);
    SubsetGeom g;
    CHK(dsubset_geom(ctx, d_seg, nrows, ncols, row0, max_seg_id, tlx, tly, xs, ys, tile_size, d_mask, &g));
    if (g.nr > 0 && !d_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_dsubset_merge(ctx, (const uint32_t *)d_pairs, (uint32_t)slot, (uint32_t)world, counts, g, max_seg_id,
                             d_out, d_hist, orig_out, cap, n_new_out);
}

// ---- colour tables and their rendering (utils.py:123-230) --------------------------------------------
API int shp_colour_stretch(shp_ctx *ctx, const void *col, int ctype, int64_t n, uint8_t *out, double *stretch_out,
                           double *dev_ms_out)
{
    CHK(enter(ctx));
    if (!col || !out || !stretch_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (ctype != COL_F64 && ctype != COL_F32 && ctype != COL_I64) SHP_FAIL(ctx, SHP_ERR_ARG, "unknown column type %d", ctype);
    if (n < 1 || n > 0xffffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "a column of %lld rows", (long long)n);
    return run_colour_stretch(ctx, col, ctype, (size_t)n, out, stretch_out, dev_ms_out);
}

API int shp_colour_pack(shp_ctx *ctx, const uint8_t *red, const uint8_t *green, const uint8_t *blue, const uint8_t *alpha,
                        int64_t n, uint32_t *d_table)
{
    CHK(enter(ctx));
    if (!red || !green || !blue || !alpha || !d_table) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (n < 1 || n > 0xffffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "a colour table of %lld rows", (long long)n);
    const uint8_t *const cols[4] = {red, green, blue, alpha};
    return run_colour_pack(ctx, cols, (size_t)n, d_table);
}

API int shp_colour_lookup_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t npix, const uint32_t *d_table, int64_t nrows,
                              uint32_t *d_out)
{
    CHK(enter(ctx));
    if (npix < 0 || nrows < 1 || nrows > 0xffffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (npix > 0 && (!d_seg || !d_table || !d_out)) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (((uintptr_t)d_seg & 3u) || ((uintptr_t)d_out & 3u)) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned raster");
    return run_colour_lookup(ctx, d_seg, (size_t)npix, d_table, (uint32_t)nrows, d_out);
}

// ---- argument checks the entry points below share ---------------------------------------------------------------
// a block of label rows in device memory (d_also: a second row pointer that must be aligned as well)
static int chk_row_block(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, const void *d_also = nullptr)
{
    if (nrows < 0 || ncols < 0 || nrows >= 0x7fffffffll || ncols >= 0x7fffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (nrows > 0 && ncols > 0 && !d_seg) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (((uintptr_t)d_seg & 3u) || ((uintptr_t)d_also & 3u)) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned raster");
    return 0;
}

// lowest: -1 where "take the largest label" is an answer, 0 elsewhere
static int chk_max_seg_id(shp_ctx *ctx, int64_t max_seg_id, int64_t lowest = 0)
{
    if (max_seg_id < lowest || max_seg_id >= 0xfffffffell) SHP_FAIL(ctx, SHP_ERR_ARG, "max_seg_id %lld", (long long)max_seg_id);
    return 0;
}

static int chk_id_share(shp_ctx *ctx, int64_t id_lo, int64_t id_hi, int64_t last_id)
{
    if (id_lo < 0 || id_hi < id_lo || id_hi > last_id + 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "id share %lld..%lld of 0..%lld", (long long)id_lo, (long long)id_hi, (long long)last_id);
    return 0;
}

// the three arrays of a table on the host, n_entries long where there are entries
static int chk_table_ptrs(shp_ctx *ctx, const void *offsets, const void *neighbours, const void *border_lengths, int64_t n_entries)
{
    if (!offsets || (n_entries > 0 && (!neighbours || !border_lengths))) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return 0;
}
static int chk_table_arrays(shp_ctx *ctx, const void *offsets, const void *neighbours, const void *border_lengths, int64_t n_entries)
{
    if (n_entries < 0 || n_entries >= (1ll << 40)) SHP_FAIL(ctx, SHP_ERR_ARG, "%lld entries", (long long)n_entries);
    return chk_table_ptrs(ctx, offsets, neighbours, border_lengths, n_entries);
}

// a column of n_rows rows against the ids 0 .. S of a table (or, groups: of a member list)
static int chk_column_rows(shp_ctx *ctx, int64_t n_rows, uint32_t S, bool groups = false)
{
    if (n_rows != (int64_t)S + 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, groups ? "a column of %lld rows for groups of %lld ids" : "a column of %lld rows for a table of %lld",
                 (long long)n_rows, (long long)S + 1);
    return 0;
}

// a column call: its type, its rows, the mask of nstats statistics and (outs given) a host output for every set bit
static int chk_column_call(shp_ctx *ctx, int ctype, int64_t n_rows, uint32_t S, bool groups, uint32_t stat_mask, int nstats,
                           void *const *outs)
{
    if (ctype != COL_F64 && ctype != COL_F32 && ctype != COL_I64) SHP_FAIL(ctx, SHP_ERR_ARG, "unknown column type %d", ctype);
    CHK(chk_column_rows(ctx, n_rows, S, groups));
    if (stat_mask == 0u || stat_mask >= (1u << nstats)) SHP_FAIL(ctx, SHP_ERR_ARG, "statistics mask %#x", stat_mask);
    for (int i = 0; outs && i < nstats; i++)
        if (((stat_mask >> i) & 1u) && !outs[i]) SHP_FAIL(ctx, SHP_ERR_ARG, "no output for statistic %d", i);
    return 0;
}

// `world` gathered blocks of `slot` items with their counts; rank: the caller's own block (0 where it does not matter)
static int chk_gathered(shp_ctx *ctx, const void *d_all, int64_t slot, int world, const uint32_t *counts, int rank = 0)
{
    if (slot < 0 || world < 0 || rank < 0 || (slot > 0 && world > 0 && (!d_all || !counts || rank >= world)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    return 0;
}

// ---- the rings something built on the outlines takes (rings.h) ----
// the vertices and rings one call can take; sized: the refusal names the counts and the limit
static int chk_ring_counts(shp_ctx *ctx, int64_t n_vertices, int64_t n_rings, uint32_t limit, bool sized)
{
    if (n_vertices >= 0 && n_vertices <= (int64_t)limit && n_rings >= 0 && n_rings <= (int64_t)limit) return 0;
    if (!sized) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    SHP_FAIL(ctx, SHP_ERR_ARG, "%lld vertices in %lld rings: more than %u", (long long)n_vertices, (long long)n_rings, limit);
}

// host arrays to upload (the counts are checked): flags: a junction flag per vertex belongs to them
static int chk_ring_arrays(shp_ctx *ctx, const int64_t *ring_offsets, const int64_t *vertex_offsets, const int64_t *vertices,
                           const int64_t *ring_area2, const uint8_t *junction, bool flags, int64_t max_seg_id, int64_t n_rings,
                           int64_t n_vertices)
{
    if (!ring_offsets || !vertex_offsets || (n_rings && !ring_area2) || (n_vertices && (!vertices || (flags && !junction))))
        SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (ring_offsets[0] != 0 || ring_offsets[max_seg_id + 1] != n_rings || vertex_offsets[0] != 0 || vertex_offsets[n_rings] != n_vertices)
        SHP_FAIL(ctx, SHP_ERR_ARG, "the offsets do not span %lld rings and %lld vertices", (long long)n_rings, (long long)n_vertices);
    // (the kernels index the vertices by the vertex offsets and the rings by the ring offsets)
    for (int64_t k = 0; k < n_rings; k++)
        if (vertex_offsets[k] > vertex_offsets[k + 1]) SHP_FAIL(ctx, SHP_ERR_ARG, "the vertex offsets do not ascend at ring %lld", (long long)k);
    for (int64_t i = 0; i <= max_seg_id; i++)
        if (ring_offsets[i] > ring_offsets[i + 1]) SHP_FAIL(ctx, SHP_ERR_ARG, "the ring offsets do not ascend at id %lld", (long long)i);
    return 0;
}

// the smallest row and column of the vertices and their spans H, W: H W <= 2^32 and max(H, W) < 2^31 keep every
// relative coordinate in 31 bits and every cross product within 2^33
static int chk_base_spans(shp_ctx *ctx, int64_t row_base, int64_t col_base, int64_t row_span, int64_t col_span)
{
    if (row_span < 0 || col_span < 0 || row_span > 0x7fffffffll || col_span > 0x7fffffffll ||
        (unsigned long long)row_span * (unsigned long long)col_span > (1ull << 32))
        SHP_FAIL(ctx, SHP_ERR_ARG, "spans (%lld, %lld)", (long long)row_span, (long long)col_span);
    if (row_base < -(1ll << 62) || row_base > (1ll << 62) || col_base < -(1ll << 62) || col_base > (1ll << 62))
        SHP_FAIL(ctx, SHP_ERR_ARG, "base (%lld, %lld)", (long long)row_base, (long long)col_base);
    return 0;
}

// resident rings must still be the ones taken; if not, the holder's stage goes back to "none" and `source` is named
static int chk_rings_current(shp_ctx *ctx, const RingSource &src, int &stage, const char *source)
{
    if (ring_source_current(ctx, src)) return 0;
    stage = 0;
    SHP_FAIL(ctx, SHP_ERR_STATE, "the traced outlines have been replaced: %s must come first", source);
}

static int need_traced(shp_ctx *ctx)
{
    if (ctx->outline.stage != 2) SHP_FAIL(ctx, SHP_ERR_STATE, "no traced outlines: shp_outline_trace must come first");
    return 0;
}

static int need_table(shp_ctx *ctx)
{
    if (!ctx->nbr_tab.finished)
        SHP_FAIL(ctx, SHP_ERR_STATE, "no finished table: shp_nbr_finish or shp_nbr_upload must come first");
    return 0;
}

static int need_share_table(shp_ctx *ctx)
{
    if (!ctx->dnbr_tab.finished)
        SHP_FAIL(ctx, SHP_ERR_STATE, "no share table: shp_dnbr_merge_dev or shp_dnbr_upload must come first");
    return 0;
}

// ---- segment neighbours and border lengths (neighbours.h) -----------------------------------------------
API int shp_nbr_begin(shp_ctx *ctx, int64_t max_seg_id, int four_connected)
{
    CHK(enter(ctx));
    CHK(chk_max_seg_id(ctx, max_seg_id, -1));
    return run_nbr_begin(ctx, max_seg_id, four_connected);
}

API int shp_nbr_accumulate_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int has_next_row)
{
    CHK(enter(ctx));
    if (!ctx->nbr.open) SHP_FAIL(ctx, SHP_ERR_STATE, "no table begun: shp_nbr_begin must come first");
    CHK(chk_row_block(ctx, d_seg, nrows, ncols));
    return run_nbr_accumulate(ctx, d_seg, (uint32_t)nrows, (uint32_t)ncols, has_next_row);
}

API int shp_nbr_finish(shp_ctx *ctx, uint32_t *max_seg_id_out, int64_t *n_entries_out, uint32_t *bad_label_out,
                       int64_t *counters_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (!max_seg_id_out || !n_entries_out || !bad_label_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (!ctx->nbr.open) SHP_FAIL(ctx, SHP_ERR_STATE, "no table begun: shp_nbr_begin must come first");
    CHK(run_nbr_finish(ctx, max_seg_id_out, n_entries_out, bad_label_out));
    if (counters_out) {
        counters_out[0] = (int64_t)ctx->nbr.pairs;
        counters_out[1] = (int64_t)ctx->nbr.used;
        counters_out[2] = (int64_t)ctx->nbr.reruns;
    }
    if (dev_ms_out) *dev_ms_out = ctx->nbr.dev_ms;
    return 0;
}

API int shp_nbr_download(shp_ctx *ctx, int64_t *offsets, uint32_t *neighbours, int64_t *border_lengths)
{
    CHK(enter(ctx));
    if (!ctx->nbr_tab.finished) SHP_FAIL(ctx, SHP_ERR_STATE, "no finished table: shp_nbr_finish must come first");
    CHK(chk_table_ptrs(ctx, offsets, neighbours, border_lengths, (int64_t)ctx->nbr_tab.nent));
    return nbr_table_download(ctx, ctx->nbr_tab, offsets, neighbours, border_lengths);
}

// ---- per-segment shape attributes (segshape.h) ----------------------------------------------------------
API int shp_shape_label_max_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t npix, uint32_t *max_label_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (!max_label_out || npix < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (npix > 0 && !d_seg) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if ((uintptr_t)d_seg & 3u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned raster");
    return run_shape_label_max(ctx, d_seg, (size_t)npix, max_label_out, dev_ms_out);
}

API int shp_shape_begin(shp_ctx *ctx, int64_t max_seg_id, int64_t row0, int64_t col0)
{
    CHK(enter(ctx));
    CHK(chk_max_seg_id(ctx, max_seg_id));
    if (row0 < 0 || col0 < 0 || row0 > 0xffffffffll || col0 > 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "origin (%lld, %lld)", (long long)row0, (long long)col0);
    return run_shape_begin(ctx, (uint32_t)max_seg_id, (unsigned long long)row0, (unsigned long long)col0);
}

API int shp_shape_accumulate_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int has_above,
                                 int has_below)
{
    CHK(enter(ctx));
    if (ctx->shape.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no shapes begun: shp_shape_begin must come first");
    CHK(chk_row_block(ctx, d_seg, nrows, ncols));
    const uint32_t *first = d_seg + (has_above ? (size_t)ncols : 0);
    return run_shape_accumulate(ctx, first, (uint32_t)nrows, (uint32_t)ncols, has_above ? first - ncols : nullptr,
                                has_below ? first + (size_t)nrows * (size_t)ncols : nullptr);
}

API int shp_shape_accumulate_halo_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, const uint32_t *d_above,
                                      const uint32_t *d_below)
{
    CHK(enter(ctx));
    if (ctx->shape.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no shapes begun: shp_shape_begin must come first");
    CHK(chk_row_block(ctx, d_seg, nrows, ncols, d_above));
    if ((uintptr_t)d_below & 3u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned raster");
    return run_shape_accumulate(ctx, d_seg, (uint32_t)nrows, (uint32_t)ncols, d_above, d_below);
}

// ---- the shape table of a row-sharded raster (dsegshape.h) -------------------------------------------------
API int shp_dshape_local_dev(shp_ctx *ctx, const uint32_t *d_hist, int64_t n_hist, uint32_t *max_label_out, int64_t *counts_out,
                             void **d_records_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->shape.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no shapes begun: shp_shape_begin must come first");
    if (!d_hist || !max_label_out || !counts_out || !d_records_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if ((uintptr_t)d_hist & 3u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned histogram");
    if (n_hist != (int64_t)ctx->shape.S + 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "a histogram of %lld rows for a table of %lld", (long long)n_hist, (long long)ctx->shape.S + 1);
    CHK(run_dshape_local(ctx, d_hist, max_label_out, counts_out, d_records_out));
    if (dev_ms_out) *dev_ms_out = ctx->shape.dev_ms;
    return 0;
}

API int shp_dshape_merge_dev(shp_ctx *ctx, const void *d_all, int64_t slot, int world, const uint32_t *counts, const uint32_t *d_hist,
                             int64_t n_hist, int64_t id_lo, int64_t id_hi, int64_t *counts_out, void **d_table_out,
                             double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->shape.stage != 3) SHP_FAIL(ctx, SHP_ERR_STATE, "no local step: shp_dshape_local_dev must come first");
    if (!d_hist || !counts_out || !d_table_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if ((uintptr_t)d_hist & 3u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned histogram");
    if (n_hist != (int64_t)ctx->shape.S + 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "a histogram of %lld rows for a table of %lld", (long long)n_hist, (long long)ctx->shape.S + 1);
    CHK(chk_id_share(ctx, id_lo, id_hi, (int64_t)ctx->shape.S));
    CHK(chk_gathered(ctx, d_all, slot, world, counts));
    if ((uintptr_t)d_all & 15u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned buffer");
    if (slot == 0) world = 0;
    CHK(run_dshape_merge(ctx, (const unsigned long long *)d_all, (unsigned long long)slot, (uint32_t)world, counts, d_hist,
                         (uint32_t)id_lo, (uint32_t)id_hi, counts_out, d_table_out));
    if (dev_ms_out) *dev_ms_out = ctx->shape.dev_ms;
    return 0;
}

API int shp_shape_finish(shp_ctx *ctx, uint32_t *max_seg_id_out, uint32_t *bad_label_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (!max_seg_id_out || !bad_label_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (ctx->shape.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no shapes begun: shp_shape_begin must come first");
    CHK(run_shape_finish(ctx, max_seg_id_out, bad_label_out));
    if (dev_ms_out) *dev_ms_out = ctx->shape.dev_ms;
    return 0;
}

API int shp_shape_download(shp_ctx *ctx, uint64_t *rows)
{
    CHK(enter(ctx));
    if (ctx->shape.stage != 2) SHP_FAIL(ctx, SHP_ERR_STATE, "no finished shapes: shp_shape_finish must come first");
    if (!rows) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_shape_download(ctx, rows);
}

// ---- segment outlines as vertex rings (outline.h) ---------------------------------------------------------
API int shp_outline_need(shp_ctx *ctx, int64_t npix, int64_t edges, int64_t *need_out, int64_t *free_out)
{
    CHK(enter(ctx));
    if (!need_out || !free_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (npix < 0 || npix > (int64_t)OL_MAX_ITEMS || edges > (int64_t)OL_MAX_ITEMS) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    return run_outline_need(ctx, (unsigned long long)npix, (long long)edges, (long long *)need_out, (long long *)free_out);
}

API int shp_outline_edges_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int64_t max_seg_id,
                              int four_connected, int64_t *edges_out, uint32_t *bad_label_out)
{
    if (ctx) ctx->outline_calls++;              // (counted whatever becomes of the call: shp_outline_serial)
    CHK(enter(ctx));
    if (!edges_out || !bad_label_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_max_seg_id(ctx, max_seg_id));
    CHK(chk_row_block(ctx, d_seg, nrows, ncols));
    if (nrows == 0 || ncols == 0) nrows = ncols = 0;
    if (nrows * ncols > (int64_t)OL_MAX_ITEMS)
        SHP_FAIL(ctx, SHP_ERR_ARG, "a raster of %lld pixels: more than %u", (long long)(nrows * ncols), OL_MAX_ITEMS);
    long long edges = 0;
    CHK(run_outline_edges(ctx, d_seg, (uint32_t)nrows, (uint32_t)ncols, (uint32_t)max_seg_id, four_connected ? 0 : 1, &edges,
                          bad_label_out));
    *edges_out = (int64_t)edges;
    return 0;
}

API int shp_outline_trace(shp_ctx *ctx, int64_t row0, int64_t col0, int64_t *counts_out, double *steps_ms_out)
{
    CHK(enter(ctx));
    if (ctx->outline.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no edges counted: shp_outline_edges_dev must come first");
    if (!counts_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (row0 < 0 || col0 < 0 || row0 > 0xffffffffll || col0 > 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "origin (%lld, %lld)", (long long)row0, (long long)col0);
    CHK(run_outline_trace(ctx, (long long)row0, (long long)col0));
    counts_out[0] = (int64_t)ctx->outline.rings;
    counts_out[1] = (int64_t)ctx->outline.verts;
    counts_out[2] = (int64_t)ctx->outline.rounds;
    if (steps_ms_out)
        for (int i = 0; i < 4; i++) steps_ms_out[i] = ctx->outline.ms[i];
    return 0;
}

API int shp_outline_download(shp_ctx *ctx, int64_t *ring_offsets, int64_t *vertex_offsets, int64_t *vertices, int64_t *ring_area2)
{
    CHK(enter(ctx));
    CHK(need_traced(ctx));
    if (!ring_offsets || !vertex_offsets || (ctx->outline.rings && (!vertices || !ring_area2))) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_outline_download(ctx, ring_offsets, vertex_offsets, vertices, ring_area2);
}

API int shp_outline_junctions(shp_ctx *ctx, int on)
{
    CHK(enter(ctx));
    if (ctx->outline.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no edges counted: shp_outline_edges_dev must come first");
    ctx->outline.junctions = on ? 1 : 0;
    return 0;
}

API int shp_outline_download_junction(shp_ctx *ctx, uint8_t *junction)
{
    CHK(enter(ctx));
    CHK(need_traced(ctx));
    if (!ctx->outline.has_flags) SHP_FAIL(ctx, SHP_ERR_STATE, "the outlines were traced without junctions: shp_outline_junctions must come first");
    if (ctx->outline.verts && !junction) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_outline_download_junction(ctx, junction);
}

API int shp_outline_serial(shp_ctx *ctx, uint64_t *calls_out, uint64_t *serial_out)
{
    if (!ctx) return SHP_ERR_ARG;
    ctx->err.clear();
    if (!calls_out || !serial_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    *calls_out = ctx->outline_calls;
    *serial_out = ctx->outline.stage == 2 ? ctx->outline.serial : 0ull;
    return 0;
}

// ---- per-segment depth: the exact distance transform of the labels (segdepth.h) -----------------------------
API int shp_depth_need(shp_ctx *ctx, int64_t nrows, int64_t ncols, int64_t max_seg_id, int all_runs, int64_t marked, int64_t *need_out,
                       int64_t *free_out)
{
    CHK(enter(ctx));
    if (!need_out || !free_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_max_seg_id(ctx, max_seg_id));
    if (nrows < 0 || ncols < 0 || nrows >= 0x7fffffffll || ncols >= 0x7fffffffll || nrows * ncols > (int64_t)OL_MAX_ITEMS ||
        marked > 3 * (int64_t)OL_MAX_ITEMS)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    return run_depth_need(ctx, (size_t)nrows, (size_t)ncols, (size_t)max_seg_id, all_runs ? 1 : 0, (long long)marked,
                          (long long *)need_out, (long long *)free_out);
}

API int shp_depth_transform_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int all_runs, int64_t *counts_out)
{
    CHK(enter(ctx));
    if (!counts_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_row_block(ctx, d_seg, nrows, ncols));
    if (nrows == 0 || ncols == 0) nrows = ncols = 0;
    if (nrows * ncols > (int64_t)OL_MAX_ITEMS)
        SHP_FAIL(ctx, SHP_ERR_ARG, "a raster of %lld pixels: more than %u", (long long)(nrows * ncols), OL_MAX_ITEMS);
    return run_depth_transform(ctx, d_seg, (uint32_t)nrows, (uint32_t)ncols, all_runs ? 1 : 0, (long long *)counts_out);
}

API int shp_depth_envelope(shp_ctx *ctx)
{
    CHK(enter(ctx));
    if (ctx->depth.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no transform: shp_depth_transform_dev must come first");
    return run_depth_envelope(ctx);
}

API int shp_depth_reduce(shp_ctx *ctx, int64_t max_seg_id, int n_cores, const uint32_t *core_q, uint32_t *bad_label_out,
                         double *steps_ms_out)
{
    CHK(enter(ctx));
    if (ctx->depth.stage != 2) SHP_FAIL(ctx, SHP_ERR_STATE, "no envelope: shp_depth_envelope must come first");
    if (!bad_label_out || (n_cores > 0 && !core_q)) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_max_seg_id(ctx, max_seg_id));
    if (n_cores < 0 || n_cores > (int)DEPTH_CORES) SHP_FAIL(ctx, SHP_ERR_ARG, "%d core areas: at most %u", n_cores, DEPTH_CORES);
    DepthCores cq{};
    cq.n = (uint32_t)n_cores;
    for (int k = 0; k < n_cores; k++) cq.q[k] = core_q[k];
    CHK(run_depth_reduce(ctx, (uint32_t)max_seg_id, cq, bad_label_out));
    if (steps_ms_out)
        for (int i = 0; i < 4; i++) steps_ms_out[i] = ctx->depth.ms[i];
    return 0;
}

API int shp_depth_download(shp_ctx *ctx, uint64_t *rows, uint32_t *depth2)
{
    CHK(enter(ctx));
    if (ctx->depth.stage != 3) SHP_FAIL(ctx, SHP_ERR_STATE, "no reduced depths: shp_depth_reduce must come first");
    if (!rows) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_depth_download(ctx, rows, depth2);
}

// ---- convex hulls of the outline rings (hull.h) ------------------------------------------------------------
API int shp_hull_need(shp_ctx *ctx, int64_t n_vertices, int64_t n_rings, int64_t max_seg_id, int upload, int64_t *need_out,
                      int64_t *free_out)
{
    CHK(enter(ctx));
    if (!need_out || !free_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_max_seg_id(ctx, max_seg_id));
    CHK(chk_ring_counts(ctx, n_vertices, n_rings, OL_MAX_ITEMS, false));
    return run_hull_need(ctx, (size_t)n_vertices, (size_t)n_rings, (size_t)max_seg_id, upload, (long long *)need_out,
                         (long long *)free_out);
}

API int shp_hull_source(shp_ctx *ctx, const int64_t *ring_offsets, const int64_t *vertex_offsets, const int64_t *vertices,
                        const int64_t *ring_area2, int64_t max_seg_id, int64_t n_rings, int64_t n_vertices, double *upload_ms_out)
{
    CHK(enter(ctx));
    ctx->hull.stage = 0;
    if (upload_ms_out) *upload_ms_out = 0.0;
    if (!ring_offsets && !vertex_offsets && !vertices && !ring_area2) {
        CHK(need_traced(ctx));
        return run_hull_source(ctx, nullptr, nullptr, nullptr, nullptr, 0u, 0u, 0u, nullptr);
    }
    CHK(chk_max_seg_id(ctx, max_seg_id));
    CHK(chk_ring_counts(ctx, n_vertices, n_rings, OL_MAX_ITEMS, true));
    CHK(chk_ring_arrays(ctx, ring_offsets, vertex_offsets, vertices, ring_area2, nullptr, false, max_seg_id, n_rings, n_vertices));
    return run_hull_source(ctx, ring_offsets, vertex_offsets, vertices, ring_area2, (uint32_t)max_seg_id, (uint32_t)n_rings,
                           (uint32_t)n_vertices, upload_ms_out);
}

API int shp_hull_build(shp_ctx *ctx, int64_t row_base, int64_t col_base, int64_t row_span, int64_t col_span, int convex_only,
                       int64_t *counts_out, double *steps_ms_out)
{
    CHK(enter(ctx));
    if (ctx->hull.stage < 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no rings to hull: shp_hull_source must come first");
    CHK(chk_rings_current(ctx, ctx->hull.src, ctx->hull.stage, "shp_hull_source"));
    if (!counts_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_base_spans(ctx, row_base, col_base, row_span, col_span));
    CHK(run_hull_build(ctx, (long long)row_base, (long long)col_base, (uint32_t)row_span, (uint32_t)col_span, convex_only ? 1 : 0));
    counts_out[0] = (int64_t)ctx->hull.nh;
    counts_out[1] = (int64_t)ctx->hull.ncand;
    counts_out[2] = (int64_t)ctx->hull.nkept;
    if (steps_ms_out)
        for (int i = 0; i < 5; i++) steps_ms_out[i] = ctx->hull.ms[i];
    return 0;
}

API int shp_hull_download(shp_ctx *ctx, int64_t *hull_offsets, int64_t *hull_points, int64_t *hull_reach, int64_t *hull_area2,
                          int64_t *feret_max2)
{
    CHK(enter(ctx));
    if (ctx->hull.stage != 2) SHP_FAIL(ctx, SHP_ERR_STATE, "no hulls built: shp_hull_build must come first");
    if (!hull_offsets || !hull_area2 || !feret_max2 || (ctx->hull.nh && (!hull_points || !hull_reach))) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_hull_download(ctx, hull_offsets, hull_points, hull_reach, hull_area2, feret_max2);
}

// ---- Douglas-Peucker simplification of the outline rings (simplify.h) -----------------------------------------
API int shp_simplify_need(shp_ctx *ctx, int64_t n_vertices, int64_t n_rings, int64_t max_seg_id, int upload, int64_t *need_out,
                          int64_t *free_out)
{
    CHK(enter(ctx));
    if (!need_out || !free_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_max_seg_id(ctx, max_seg_id));
    CHK(chk_ring_counts(ctx, n_vertices, n_rings, SP_MAX_VERTS, false));
    return run_simplify_need(ctx, (size_t)n_vertices, (size_t)n_rings, (size_t)max_seg_id, upload, (long long *)need_out,
                             (long long *)free_out);
}

API int shp_simplify_source(shp_ctx *ctx, const int64_t *ring_offsets, const int64_t *vertex_offsets, const int64_t *vertices,
                            const int64_t *ring_area2, const uint8_t *junction, int64_t max_seg_id, int64_t n_rings,
                            int64_t n_vertices, double *upload_ms_out)
{
    CHK(enter(ctx));
    ctx->simplify.stage = 0;
    if (upload_ms_out) *upload_ms_out = 0.0;
    if (!ring_offsets && !vertex_offsets && !vertices && !ring_area2 && !junction) {
        CHK(need_traced(ctx));
        if (!ctx->outline.has_flags)
            SHP_FAIL(ctx, SHP_ERR_STATE, "the outlines were traced without junctions: shp_outline_junctions must come first");
        if (ctx->outline.verts > SP_MAX_VERTS) SHP_FAIL(ctx, SHP_ERR_ARG, "%u vertices: more than %u", ctx->outline.verts, SP_MAX_VERTS);
        return run_simplify_source(ctx, nullptr, nullptr, nullptr, nullptr, nullptr, 0u, 0u, 0u, nullptr);
    }
    CHK(chk_max_seg_id(ctx, max_seg_id));
    CHK(chk_ring_counts(ctx, n_vertices, n_rings, SP_MAX_VERTS, true));
    CHK(chk_ring_arrays(ctx, ring_offsets, vertex_offsets, vertices, ring_area2, junction, true, max_seg_id, n_rings, n_vertices));
    return run_simplify_source(ctx, ring_offsets, vertex_offsets, vertices, ring_area2, junction, (uint32_t)max_seg_id, (uint32_t)n_rings,
                               (uint32_t)n_vertices, upload_ms_out);
}

API int shp_simplify_build(shp_ctx *ctx, uint64_t tolerance2q, int path, int64_t row_base, int64_t col_base, int64_t row_span,
                           int64_t col_span, int64_t *counts_out, double *steps_ms_out)
{
    CHK(enter(ctx));
    if (ctx->simplify.stage < 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no rings to simplify: shp_simplify_source must come first");
    CHK(chk_rings_current(ctx, ctx->simplify.src, ctx->simplify.stage, "shp_simplify_source"));
    if (!counts_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (tolerance2q > (1ull << 46)) SHP_FAIL(ctx, SHP_ERR_ARG, "tolerance2q %llu is above 2^46", (unsigned long long)tolerance2q);
    if (path < 0 || path > 3) SHP_FAIL(ctx, SHP_ERR_ARG, "path %d is none of 0 (auto), 1 (short), 2 (group), 3 (global)", path);
    CHK(chk_base_spans(ctx, row_base, col_base, row_span, col_span));
    CHK(run_simplify_build(ctx, (unsigned long long)tolerance2q, path, (long long)row_base, (long long)col_base));
    const SimplifyState &z = ctx->simplify;
    const int64_t counts[10] = {z.rings, z.verts, z.rounds, z.narcs, z.longest, z.nshort, z.ngroup, z.nglobal, z.kept, 0};
    for (int i = 0; i < 10; i++) counts_out[i] = counts[i];
    if (steps_ms_out)
        for (int i = 0; i < 4; i++) steps_ms_out[i] = z.ms[i];
    return 0;
}

API int shp_simplify_download(shp_ctx *ctx, int64_t *ring_offsets, int64_t *vertex_offsets, int64_t *vertices, int64_t *ring_area2,
                              int64_t *source_ring, int64_t *kept_vertex)
{
    CHK(enter(ctx));
    if (ctx->simplify.stage != 2) SHP_FAIL(ctx, SHP_ERR_STATE, "no simplified rings: shp_simplify_build must come first");
    if (!ring_offsets || !vertex_offsets || (ctx->simplify.rings && (!ring_area2 || !source_ring)) ||
        (ctx->simplify.verts && (!vertices || !kept_vertex)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_simplify_download(ctx, ring_offsets, vertex_offsets, vertices, ring_area2, source_ring, kept_vertex);
}

// ---- columns reduced over the neighbour table (nbrreduce.h) -----------------------------------------------
API int shp_nbr_upload(shp_ctx *ctx, const int64_t *offsets, const uint32_t *neighbours, const int64_t *border_lengths,
                       int64_t max_seg_id, int64_t n_entries, double *dev_ms_out)
{
    CHK(enter(ctx));
    CHK(chk_max_seg_id(ctx, max_seg_id));
    CHK(chk_table_arrays(ctx, offsets, neighbours, border_lengths, n_entries));
    return run_nbr_upload(ctx, offsets, neighbours, border_lengths, (uint32_t)max_seg_id, (long long)n_entries, dev_ms_out);
}

API int shp_nbr_table_serial(shp_ctx *ctx, uint64_t *serial_out, int *finished_out)
{
    if (!ctx) return SHP_ERR_ARG;
    ctx->err.clear();
    if (!serial_out || !finished_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    *serial_out = ctx->nbr_tab.serial;
    *finished_out = ctx->nbr_tab.finished ? 1 : 0;
    return 0;
}

API int shp_nbr_reduce(shp_ctx *ctx, const void *col, int ctype, int64_t n_rows, int has_ignore, double ignore_value,
                       double missing_value, uint32_t stat_mask, void *const *outs, double *dev_ms_out)
{
    CHK(enter(ctx));
    CHK(need_table(ctx));
    if (!col || !outs) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_column_call(ctx, ctype, n_rows, ctx->nbr_tab.S, false, stat_mask, NBRR_NPUBLIC, outs));
    return run_nbr_reduce(ctx, col, ctype, has_ignore, ignore_value, missing_value, stat_mask, outs, dev_ms_out);
}

// ---- touching segments of one class merged into one (nbrmerge.h) -------------------------------------------
API int shp_nbr_merge(shp_ctx *ctx, const int64_t *keys, int64_t n_rows, int has_ignore, int64_t ignore_key,
                      int64_t min_border, const int64_t *seg_size, uint32_t *max_group_out, int64_t *counters_out,
                      double *dev_ms_out)
{
    CHK(enter(ctx));
    ctx->mrg.stage = 0;
    CHK(need_table(ctx));
    if (!keys || !max_group_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_column_rows(ctx, n_rows, ctx->nbr_tab.S));
    if (min_border < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "min_border %lld", (long long)min_border);
    return run_nbr_merge(ctx, keys, has_ignore, ignore_key, min_border, seg_size, max_group_out, counters_out, dev_ms_out);
}

API int shp_nbr_merge_groups(shp_ctx *ctx, uint32_t *recode, uint32_t *representative, int64_t *group_size, int64_t *hist)
{
    CHK(enter(ctx));
    if (ctx->mrg.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no groups: shp_nbr_merge must come first");
    return run_nbr_merge_groups(ctx, recode, representative, group_size, hist);
}

API int shp_nbr_merge_contract(shp_ctx *ctx, int64_t *n_entries_out, int64_t *records_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (!n_entries_out || !records_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (ctx->mrg.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no groups: shp_nbr_merge must come first");
    if (ctx->mrg.contracted || !ctx->nbr_tab.finished || ctx->nbr_tab.serial != ctx->mrg.table_serial)
        SHP_FAIL(ctx, SHP_ERR_STATE, "the table the groups were found in is no longer the context's finished table");
    return run_nbr_merge_contract(ctx, n_entries_out, records_out, dev_ms_out);
}

API int shp_nbr_merge_recode_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t npix, uint32_t *d_out, int count_hist,
                                 uint32_t *bad_label_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->mrg.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no groups: shp_nbr_merge must come first");
    if (npix < 0 || !bad_label_out) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (npix > 0 && (!d_seg || !d_out)) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (((uintptr_t)d_seg & 3u) || ((uintptr_t)d_out & 3u)) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned raster");
    if (count_hist && ctx->mrg.has_size) SHP_FAIL(ctx, SHP_ERR_ARG, "the histogram holds the sums of seg_size: nothing to count");
    return run_nbr_merge_recode(ctx, d_seg, (size_t)npix, d_out, count_hist, bad_label_out, dev_ms_out);
}

API int shp_nbr_merge_similar(shp_ctx *ctx, const double *const *cols, int n_cols, int64_t n_rows, int has_ignore_value,
                              double ignore_value, int has_threshold, double thr2, int mutual_nearest, const int64_t *keys,
                              int has_ignore_key, int64_t ignore_key, int64_t min_border, const int64_t *seg_size,
                              uint32_t *max_group_out, int64_t *counters_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    ctx->mrg.stage = 0;
    CHK(need_table(ctx));
    if (!cols || !max_group_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (n_cols < 1 || n_cols > MRGS_MAX_COLS) SHP_FAIL(ctx, SHP_ERR_ARG, "%d distance columns: 1 to %d wanted", n_cols, MRGS_MAX_COLS);
    for (int c = 0; c < n_cols; c++)
        if (!cols[c]) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_column_rows(ctx, n_rows, ctx->nbr_tab.S));
    if (min_border < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "min_border %lld", (long long)min_border);
    if (!has_threshold && !mutual_nearest) SHP_FAIL(ctx, SHP_ERR_ARG, "no threshold: only the mutual-nearest rule does without");
    if (has_threshold && !(thr2 >= 0.0)) SHP_FAIL(ctx, SHP_ERR_ARG, "thr2 %g", thr2);
    return run_nbr_merge_similar(ctx, cols, n_cols, has_ignore_value, ignore_value, has_threshold, thr2, mutual_nearest, keys,
                                 has_ignore_key, ignore_key, min_border, seg_size, max_group_out, counters_out, dev_ms_out);
}

// ---- columns carried to the groups of a merge (nbragg.h) ---------------------------------------------------
API int shp_nbr_groups_serial(shp_ctx *ctx, uint64_t *groups_serial_out, uint64_t *members_serial_out)
{
    if (!ctx) return SHP_ERR_ARG;
    ctx->err.clear();
    if (!groups_serial_out || !members_serial_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    *groups_serial_out = ctx->mrg.stage == 1 ? ctx->mrg.serial : 0;
    *members_serial_out = ctx->agg.stage == 1 ? ctx->agg.serial : 0;
    return 0;
}

API int shp_nbr_members_build(shp_ctx *ctx, const uint32_t *recode, int64_t n_rows, int64_t max_group, uint64_t *serial_out,
                              int64_t *n_members_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (!serial_out || !n_members_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (recode) {
        if (n_rows < 1 || n_rows > 0xfffffffell) SHP_FAIL(ctx, SHP_ERR_ARG, "a recode of %lld rows", (long long)n_rows);
        if (max_group < 0 || max_group >= n_rows)
            SHP_FAIL(ctx, SHP_ERR_ARG, "%lld groups of %lld ids", (long long)max_group, (long long)n_rows - 1);
        CHK(run_agg_build(ctx, recode, (uint32_t)(n_rows - 1), (uint32_t)max_group));
    } else {
        if (ctx->mrg.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no groups: shp_nbr_merge must come first");
        if (ctx->agg.stage != 1 || ctx->agg.serial != ctx->mrg.serial) CHK(run_agg_build(ctx, nullptr, ctx->mrg.S, ctx->mrg.M));
    }
    *serial_out = ctx->agg.serial;
    *n_members_out = (int64_t)ctx->agg.nmem;
    if (dev_ms_out) *dev_ms_out = ctx->agg.dev_ms;
    return 0;
}

API int shp_nbr_members_download(shp_ctx *ctx, int64_t *offsets, uint32_t *members)
{
    CHK(enter(ctx));
    if (ctx->agg.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no member list: shp_nbr_members_build must come first");
    if (!offsets || (ctx->agg.nmem > 0 && !members)) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_agg_download(ctx, offsets, members);
}

API int shp_nbr_aggregate(shp_ctx *ctx, const void *col, int ctype, int64_t n_rows, const int64_t *weights, int has_ignore,
                          double ignore_value, double missing_value, uint32_t stat_mask, void *const *outs, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->agg.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no member list: shp_nbr_members_build must come first");
    if (!col || !outs) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_column_call(ctx, ctype, n_rows, ctx->agg.S, true, stat_mask, AGG_NSTATS, outs));
    return run_agg(ctx, col, ctype, weights, has_ignore, ignore_value, missing_value, stat_mask, outs, dev_ms_out);
}

// ---- the neighbour table of a row-sharded raster, by id share (dneighbours.h) ------------------------------
API int shp_dnbr_local_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, const uint32_t *d_halo_row,
                           int64_t max_seg_id, int four_connected, int64_t id_lo, int64_t id_hi, uint32_t *max_label_out,
                           int64_t *counts_out, void **d_travel_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (!max_label_out || !counts_out || !d_travel_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_max_seg_id(ctx, max_seg_id));
    CHK(chk_id_share(ctx, id_lo, id_hi, max_seg_id));
    CHK(chk_row_block(ctx, d_seg, nrows, ncols, d_halo_row));
    CHK(run_dnbr_local(ctx, d_seg, (uint32_t)nrows, (uint32_t)ncols, nrows > 0 ? d_halo_row : nullptr, (uint32_t)max_seg_id,
                       four_connected, (uint32_t)id_lo, (uint32_t)id_hi, max_label_out, counts_out, d_travel_out));
    if (dev_ms_out) *dev_ms_out = ctx->dnbr.dev_ms;
    return 0;
}

API int shp_dnbr_merge_dev(shp_ctx *ctx, const void *d_all, int64_t slot, int world, const uint32_t *counts, void *d_cols,
                           int64_t *n_picked_out, int64_t *n_entries_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->dnbr.stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no local step: shp_dnbr_local_dev must come first");
    if (!d_cols || !n_picked_out || !n_entries_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_gathered(ctx, d_all, slot, world, counts));
    if (((uintptr_t)d_all & 15u) || ((uintptr_t)d_cols & 7u)) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned buffer");
    if (slot == 0) world = 0;
    CHK(run_dnbr_merge(ctx, (const uint4 *)d_all, (unsigned long long)slot, (uint32_t)world, counts, (long long *)d_cols,
                       n_picked_out, n_entries_out));
    if (dev_ms_out) *dev_ms_out = ctx->dnbr.dev_ms;
    return 0;
}

API int shp_dnbr_download(shp_ctx *ctx, int64_t *offsets, uint32_t *neighbours, int64_t *border_lengths)
{
    CHK(enter(ctx));
    if (!ctx->dnbr_tab.finished) SHP_FAIL(ctx, SHP_ERR_STATE, "no share table: shp_dnbr_merge_dev must come first");
    CHK(chk_table_ptrs(ctx, offsets, neighbours, border_lengths, (int64_t)ctx->dnbr_tab.nent));
    return nbr_table_download(ctx, ctx->dnbr_tab, offsets, neighbours, border_lengths);
}

API int shp_dnbr_upload(shp_ctx *ctx, const int64_t *offsets, const uint32_t *neighbours, const int64_t *border_lengths,
                        int64_t max_seg_id, int64_t id_lo, int64_t id_hi, int64_t n_entries)
{
    CHK(enter(ctx));
    CHK(chk_max_seg_id(ctx, max_seg_id));
    CHK(chk_id_share(ctx, id_lo, id_hi, max_seg_id));
    CHK(chk_table_arrays(ctx, offsets, neighbours, border_lengths, n_entries));
    if (offsets[0] != 0 || offsets[id_hi - id_lo] != n_entries)
        SHP_FAIL(ctx, SHP_ERR_ARG, "not a share table: the offsets must run from 0 to the number of entries");
    return run_dnbr_upload(ctx, offsets, neighbours, border_lengths, (uint32_t)max_seg_id, (uint32_t)id_lo, (uint32_t)id_hi,
                           (unsigned long long)n_entries);
}

API int shp_dnbr_table_serial(shp_ctx *ctx, uint64_t *serial_out, int *finished_out)
{
    if (!ctx) return SHP_ERR_ARG;
    ctx->err.clear();
    if (!serial_out || !finished_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    *serial_out = ctx->dnbr_tab.serial;
    *finished_out = ctx->dnbr_tab.finished ? 1 : 0;
    return 0;
}

API int shp_dnbr_reduce_dev(shp_ctx *ctx, const void *col, int ctype, int64_t n_rows, int has_ignore, double ignore_value,
                            double missing_value, uint32_t stat_mask, void *d_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    CHK(need_share_table(ctx));
    if (!col || !d_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if ((uintptr_t)d_out & 7u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned buffer");
    CHK(chk_column_call(ctx, ctype, n_rows, ctx->dnbr_tab.S, false, stat_mask, NBRR_NPUBLIC, nullptr));
    return run_dnbr_reduce(ctx, col, ctype, has_ignore, ignore_value, missing_value, stat_mask, d_out, dev_ms_out);
}

// ---- the merges of nbrmerge.h over the share table (dnbrmerge.h) ------------------------------------------
API int shp_dnbr_mrg_begin(shp_ctx *ctx, const double *const *cols, int n_cols, int64_t n_rows, int has_ignore_value,
                           double ignore_value, int has_threshold, double thr2, int mutual_nearest, const int64_t *keys,
                           int has_ignore_key, int64_t ignore_key, int64_t min_border, const int64_t *seg_size,
                           void **d_best_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    ctx->mrg.stage = 0;
    ctx->dmrg.stage = 0;
    CHK(need_share_table(ctx));
    if (!d_best_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (n_cols < 0 || n_cols > MRGS_MAX_COLS) SHP_FAIL(ctx, SHP_ERR_ARG, "%d distance columns: 0 to %d wanted", n_cols, MRGS_MAX_COLS);
    if (n_cols > 0 && !cols) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    for (int c = 0; c < n_cols; c++)
        if (!cols[c]) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (n_cols == 0 && !keys) SHP_FAIL(ctx, SHP_ERR_ARG, "the key rule needs keys");
    CHK(chk_column_rows(ctx, n_rows, ctx->dnbr_tab.S));
    if (min_border < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "min_border %lld", (long long)min_border);
    if (n_cols > 0 && !has_threshold && !mutual_nearest)
        SHP_FAIL(ctx, SHP_ERR_ARG, "no threshold: only the mutual-nearest rule does without");
    if (n_cols > 0 && has_threshold && !(thr2 >= 0.0)) SHP_FAIL(ctx, SHP_ERR_ARG, "thr2 %g", thr2);
    return run_dmrg_begin(ctx, cols, n_cols, has_ignore_value, ignore_value, has_threshold, thr2, mutual_nearest, keys,
                          has_ignore_key, ignore_key, min_border, seg_size, d_best_out, dev_ms_out);
}

API int shp_dnbr_mrg_hook(shp_ctx *ctx, int64_t *counts_out, void **d_pairs_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->dmrg.stage != 1 || !ctx->dnbr_tab.finished || ctx->dnbr_tab.serial != ctx->dmrg.table_serial)
        SHP_FAIL(ctx, SHP_ERR_STATE, "no merge begun on the context's share table: shp_dnbr_mrg_begin must come first");
    if (!counts_out || !d_pairs_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_dmrg_hook(ctx, counts_out, d_pairs_out, dev_ms_out);
}

API int shp_dnbr_mrg_number(shp_ctx *ctx, const void *d_all, int64_t slot, int world, const uint32_t *counts, int rank,
                            uint32_t *max_group_out, void **d_hist_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->dmrg.stage != 2 || !ctx->dnbr_tab.finished || ctx->dnbr_tab.serial != ctx->dmrg.table_serial)
        SHP_FAIL(ctx, SHP_ERR_STATE, "no hooked merge on the context's share table: shp_dnbr_mrg_hook must come first");
    if (!max_group_out || !d_hist_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_gathered(ctx, d_all, slot, world, counts, rank));
    if ((uintptr_t)d_all & 7u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned buffer");
    if (slot == 0) world = 0;
    return run_dmrg_number(ctx, (const uint2 *)d_all, (unsigned long long)slot, (uint32_t)world, counts, (uint32_t)rank,
                           max_group_out, d_hist_out, dev_ms_out);
}

API int shp_dnbr_mrg_records(shp_ctx *ctx, int64_t new_id_lo, int64_t new_id_hi, int64_t *counts_out, void **d_travel_out,
                             double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->dmrg.stage != 3 || ctx->mrg.stage != 1 || !ctx->dnbr_tab.finished || ctx->dnbr_tab.serial != ctx->dmrg.table_serial)
        SHP_FAIL(ctx, SHP_ERR_STATE, "no numbered merge on the context's share table: shp_dnbr_mrg_number must come first");
    if (!counts_out || !d_travel_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(chk_id_share(ctx, new_id_lo, new_id_hi, (int64_t)ctx->mrg.M));
    return run_dmrg_records(ctx, (uint32_t)new_id_lo, (uint32_t)new_id_hi, counts_out, d_travel_out, dev_ms_out);
}

// a column shared by rows over the ranks: shp_colour_stretch in steps (colour.h)
API int shp_dcolour_begin(shp_ctx *ctx, const void *col, int ctype, int64_t m, int64_t n, void **d_block_out)
{
    CHK(enter(ctx));
    if (!d_block_out || (m > 0 && !col)) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (ctype != COL_F64 && ctype != COL_F32 && ctype != COL_I64) SHP_FAIL(ctx, SHP_ERR_ARG, "unknown column type %d", ctype);
    if (n < 1 || n > 0xffffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "a column of %lld rows", (long long)n);
    if (m < 0 || m > n) SHP_FAIL(ctx, SHP_ERR_ARG, "a share of %lld rows of %lld", (long long)m, (long long)n);
    return run_dcolour_begin(ctx, col, ctype, (size_t)m, (size_t)n, d_block_out);
}

API int shp_dcolour_hist(shp_ctx *ctx, int pass)
{
    CHK(enter(ctx));
    if (pass < 0 || pass >= SEL_PASSES) SHP_FAIL(ctx, SHP_ERR_ARG, "pass %d", pass);
    return run_dcolour_hist(ctx, pass);
}

API int shp_dcolour_pick(shp_ctx *ctx, int pass)
{
    CHK(enter(ctx));
    if (pass < 0 || pass >= SEL_PASSES) SHP_FAIL(ctx, SHP_ERR_ARG, "pass %d", pass);
    return run_dcolour_pick(ctx, pass);
}

API int shp_dcolour_finish(shp_ctx *ctx, double *stretch_out, int *bad_out)
{
    CHK(enter(ctx));
    if (!stretch_out || !bad_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    return run_dcolour_finish(ctx, stretch_out, bad_out);
}

API int shp_dcolour_stretch_dev(shp_ctx *ctx, uint8_t *d_out, double *dev_ms_out)
{
    CHK(enter(ctx));
    if (ctx->dcol.m > 0 && !d_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if ((uintptr_t)d_out & 3u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned byte column");
    return run_dcolour_stretch(ctx, d_out, dev_ms_out);
}

API int shp_colour_pack_dev(shp_ctx *ctx, const uint8_t *d_red, const uint8_t *d_green, const uint8_t *d_blue,
                            const uint8_t *d_alpha, int64_t n, uint32_t *d_table)
{
    CHK(enter(ctx));
    if (!d_red || !d_green || !d_blue || !d_alpha || !d_table) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (n < 1 || n > 0xffffffffll) SHP_FAIL(ctx, SHP_ERR_ARG, "a colour table of %lld rows", (long long)n);
    const uint8_t *const cols[4] = {d_red, d_green, d_blue, d_alpha};
    for (int k = 0; k < 4; k++)
        if ((uintptr_t)cols[k] & 3u) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned byte column");
    return run_colour_pack_dev(ctx, cols, (size_t)n, d_table);
}

API int shp_colour_render_rows_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t npix, int64_t block_pixels,
                                   const uint32_t *d_table, int64_t nrows, uint32_t *h_dst, uint32_t *bad_out,
                                   double *ms_out)
{
    CHK(enter(ctx));
    if (npix < 0 || nrows < 1 || nrows > 0xffffffffll || block_pixels < 1 || block_pixels > 0x7fffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (!bad_out || !ms_out || (npix > 0 && (!d_seg || !d_table || !h_dst))) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (((uintptr_t)d_seg & 3u) || ((uintptr_t)h_dst & 3u)) SHP_FAIL(ctx, SHP_ERR_ARG, "unaligned raster");
    return run_colour_render_rows(ctx, d_seg, (size_t)npix, (size_t)block_pixels, d_table, (uint32_t)nrows, h_dst, bad_out,
                                  ms_out);
}

API int shp_colour_overview_rects_dev(shp_ctx *ctx, const uint32_t *d_raster, int64_t npix, const int64_t *rects,
                                      int nrects, const uint32_t *d_table, int64_t nrows, uint32_t *d_packed,
                                      int64_t npacked, uint32_t *bad_out)
{
    CHK(enter(ctx));
    if (npix < 0 || nrects < 0 || npacked < 0 || nrows < 1 || nrows > 0xffffffffll || !bad_out || (nrects > 0 && !rects) ||
        (npacked > 0 && (!d_raster || !d_packed || !d_table)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    CHK(overview_rects_check(ctx, npix, rects, nrects, npacked));
    bad_out[0] = 0u;
    bad_out[1] = 0xffffffffu;
    if (npacked == 0) return 0;
    return run_colour_overview_rects(ctx, d_raster, rects, nrects, d_table, (uint32_t)nrows, d_packed, (size_t)npacked,
                                     bad_out);
}

// ---- spatial statistics ------------------------------------------------------------
static int spatial_check(shp_ctx *ctx, int dtype, int64_t nrows, int64_t ncols, int func,
                         const double *params, int nint, int nflt)
{
    if (dtype_size(dtype) == 0 || nrows < 0 || ncols < 0 || !params || nint < 0 || nflt < 0 || nint + nflt < 1)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (func < 0 || func > 2) SHP_FAIL(ctx, SHP_ERR_ARG, "unknown built-in spatial function %d", func);
    if ((uint64_t)nrows * (uint64_t)ncols >= 0xffffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large");
    return 0;
}

API int shp_spatialstats_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                             int64_t nrows, int64_t ncols, uint32_t max_seg_id, int64_t null_val,
                             int func, const double *params, int64_t missing, int nint, int nflt,
                             int64_t *intcols_out, float *floatcols_out)
{
    CHK(enter(ctx));
    if (!d_seg || !d_band || (nint && !intcols_out) || (nflt && !floatcols_out))
        SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(spatial_check(ctx, dtype, nrows, ncols, func, params, nint, nflt));
    return run_spatialstats(ctx, d_seg, d_band, dtype, (uint32_t)nrows, (uint32_t)ncols, max_seg_id,
                            null_val, func, params, missing, nint, nflt, intcols_out, floatcols_out);
}

API int shp_spatialstats(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t nrows,
                         int64_t ncols, uint32_t max_seg_id, int64_t null_val, int func,
                         const double *params, int64_t missing, int nint, int nflt,
                         int64_t *intcols_out, float *floatcols_out)
{
    CHK(enter(ctx));
    if (!seg || !band || (nint && !intcols_out) || (nflt && !floatcols_out))
        SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(spatial_check(ctx, dtype, nrows, ncols, func, params, nint, nflt));
    const size_t npix = (size_t)nrows * (size_t)ncols;
    CHK(buf_ensure(ctx, ctx->seg, npix * 4));
    CHK(buf_ensure(ctx, ctx->img, npix * dtype_size(dtype)));
    if (npix) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->seg.p, seg, npix * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->img.p, band, npix * dtype_size(dtype), hipMemcpyHostToDevice,
                                   ctx->stream));
    }
    return run_spatialstats(ctx, bp<uint32_t>(ctx->seg), ctx->img.p, dtype, (uint32_t)nrows, (uint32_t)ncols,
                            max_seg_id, null_val, func, params, missing, nint, nflt, intcols_out,
                            floatcols_out);
}

// ---- per-segment point lists for user-defined spatial statistics (segpoints.h) -----------------------------
static int pts_check(shp_ctx *ctx, const void *seg, const void *band, int dtype, int64_t nrows, int64_t ncols,
                     uint32_t max_seg_id)
{
    if (!seg || !band) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    if (dtype_size(dtype) == 0 || nrows < 0 || ncols < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if ((uint64_t)nrows * (uint64_t)ncols >= 0xffffffffull) SHP_FAIL(ctx, SHP_ERR_ARG, "raster too large");
    if (max_seg_id == 0xffffffffu) SHP_FAIL(ctx, SHP_ERR_ARG, "max_seg_id too large");
    return 0;
}

// the two rasters into the context's workspace
static int pts_upload(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t nrows, int64_t ncols)
{
    const size_t npix = (size_t)nrows * (size_t)ncols;
    CHK(buf_ensure(ctx, ctx->seg, npix * 4));
    CHK(buf_ensure(ctx, ctx->img, npix * dtype_size(dtype)));
    if (npix) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->seg.p, seg, npix * 4, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipMemcpyAsync(ctx->img.p, band, npix * dtype_size(dtype), hipMemcpyHostToDevice, ctx->stream));
    }
    return 0;
}

API int shp_segpoints_count_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                                int64_t ncols, uint32_t max_seg_id, int64_t null_val, uint32_t *counts_out)
{
    CHK(enter(ctx));
    if (!counts_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(pts_check(ctx, d_seg, d_band, dtype, nrows, ncols, max_seg_id));
    return run_segpoints_count(ctx, d_seg, d_band, dtype, (uint32_t)nrows, (uint32_t)ncols, max_seg_id, null_val,
                               counts_out);
}

API int shp_segpoints_count(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t nrows,
                            int64_t ncols, uint32_t max_seg_id, int64_t null_val, uint32_t *counts_out)
{
    CHK(enter(ctx));
    if (!counts_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(pts_check(ctx, seg, band, dtype, nrows, ncols, max_seg_id));
    CHK(pts_upload(ctx, seg, band, dtype, nrows, ncols));
    return run_segpoints_count(ctx, bp<uint32_t>(ctx->seg), ctx->img.p, dtype, (uint32_t)nrows, (uint32_t)ncols,
                               max_seg_id, null_val, counts_out);
}

API int shp_segpoints_build_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                                int64_t ncols, uint32_t max_seg_id, int64_t null_val, int64_t tile_size,
                                int64_t *npts_out)
{
    CHK(enter(ctx));
    if (!npts_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(pts_check(ctx, d_seg, d_band, dtype, nrows, ncols, max_seg_id));
    if (tile_size < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "tile_size must be positive (got %lld)", (long long)tile_size);
    const uint32_t ts = tile_size > 0xffffffffll ? 0xffffffffu : (uint32_t)tile_size;
    return run_segpoints_build(ctx, d_seg, d_band, dtype, (uint32_t)nrows, (uint32_t)ncols, max_seg_id, null_val,
                               ts, npts_out);
}

API int shp_segpoints_build(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t nrows,
                            int64_t ncols, uint32_t max_seg_id, int64_t null_val, int64_t tile_size,
                            int64_t *npts_out)
{
    CHK(enter(ctx));
    if (!npts_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    CHK(pts_check(ctx, seg, band, dtype, nrows, ncols, max_seg_id));
    if (tile_size < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "tile_size must be positive (got %lld)", (long long)tile_size);
    const uint32_t ts = tile_size > 0xffffffffll ? 0xffffffffu : (uint32_t)tile_size;
    CHK(pts_upload(ctx, seg, band, dtype, nrows, ncols));
    return run_segpoints_build(ctx, bp<uint32_t>(ctx->seg), ctx->img.p, dtype, (uint32_t)nrows, (uint32_t)ncols,
                               max_seg_id, null_val, ts, npts_out);
}

API int shp_segpoints_emit(shp_ctx *ctx, uint32_t id_lo, uint32_t id_hi, int64_t *offs_out, void *pts_out,
                           int64_t cap, int64_t *npts_out)
{
    const bool built = ctx && ctx->pts.valid;
    CHK(enter(ctx));
    if (!offs_out || !npts_out || (cap > 0 && !pts_out) || cap < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (!built) SHP_FAIL(ctx, SHP_ERR_STATE, "no point lists: shp_segpoints_build must be the context's previous call");
    ctx->pts.valid = true;
    if (id_lo > id_hi || (uint64_t)id_hi > (uint64_t)ctx->pts.S + 1u)
        SHP_FAIL(ctx, SHP_ERR_ARG, "id range %u..%u outside 0..%llu", id_lo, id_hi,
                 (unsigned long long)ctx->pts.S + 1ull);
    return run_segpoints_emit(ctx, id_lo, id_hi, offs_out, pts_out, cap, npts_out);
}

// ---- the point lists of row shards (dsegpoints.h) ------------------------------------------------------------
API int shp_dsegpoints_build_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                                 int64_t ncols, int64_t row0, int64_t img_rows, uint32_t max_seg_id, int64_t null_val,
                                 int64_t tile_size, const uint32_t *d_hist, uint32_t *lh_out, uint32_t *pts_out,
                                 void **d_rec_out, int64_t *n_rec_out)
{
    CHK(enter(ctx));
    if (!d_hist || !lh_out || !pts_out || !d_rec_out || !n_rec_out || dtype_size(dtype) == 0 || nrows < 0 ||
        ncols < 0 || row0 < 0 || (nrows > 0 && (!d_seg || !d_band)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (tile_size < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "tile_size must be positive (got %lld)", (long long)tile_size);
    if (row0 + nrows > img_rows || img_rows >= 0xffffffffll || ncols >= 0xffffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "rows %lld..%lld outside the image's %lld rows", (long long)row0,
                 (long long)(row0 + nrows), (long long)img_rows);
    // per rank: the own rows stay below 2^32 pixels, the whole raster need not
    if ((uint64_t)nrows * (uint64_t)ncols >= 0xffffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "shard too large (%lld x %lld px)", (long long)nrows, (long long)ncols);
    if (max_seg_id == 0xffffffffu) SHP_FAIL(ctx, SHP_ERR_ARG, "max_seg_id too large");
    const uint32_t ts = tile_size > 0xffffffffll ? 0xffffffffu : (uint32_t)tile_size;
    // pts_visit_pos divides by the pixels of a tile row in 32 bits once a shard reaches past its first one; the
    // test names the whole raster alone, so every rank refuses alike
    const uint64_t th = (uint64_t)ts < (uint64_t)img_rows ? (uint64_t)ts : (uint64_t)img_rows;
    if ((uint64_t)img_rows > th && th * (uint64_t)ncols >= 0x100000000ull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "a tile row of %llu x %lld px reaches 2^32 pixels (tile_size %lld)",
                 (unsigned long long)th, (long long)ncols, (long long)tile_size);
    return run_dsegpoints_build(ctx, d_seg, d_band, dtype, (uint32_t)nrows, (uint32_t)ncols, (uint32_t)row0,
                                (uint32_t)img_rows, max_seg_id, null_val, ts, d_hist, lh_out, pts_out, d_rec_out,
                                n_rec_out);
}

API int shp_dsegpoints_merge_dev(shp_ctx *ctx, const void *d_recs, int64_t slot, int world, const uint32_t *counts,
                                 uint32_t id_lo, uint32_t id_hi, uint32_t *merged_out, int64_t *n_merged_out)
{
    const int stage = ctx ? ctx->dpts.stage : 0;
    CHK(enter(ctx));
    if (!counts || !n_merged_out || slot < 0 || world < 1 || (slot > 0 && !d_recs) ||
        (uint64_t)slot * (uint64_t)world >= 0xffffffffull || (id_hi > id_lo && !merged_out))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (stage != 1) SHP_FAIL(ctx, SHP_ERR_STATE, "no local point lists: shp_dsegpoints_build_dev must come first");
    ctx->dpts.stage = 1;
    if (id_lo > id_hi || (uint64_t)id_hi > (uint64_t)ctx->pts.S + 1u)
        SHP_FAIL(ctx, SHP_ERR_ARG, "id share %u..%u outside 0..%llu", id_lo, id_hi,
                 (unsigned long long)ctx->pts.S + 1ull);
    for (int r = 0; r < world; r++) if ((int64_t)counts[r] > slot) SHP_FAIL(ctx, SHP_ERR_ARG, "counts[%d] exceeds the slot", r);
    return run_dsegpoints_merge(ctx, (const unsigned long long *)d_recs, (uint32_t)slot, (uint32_t)world, counts,
                                id_lo, id_hi, merged_out, n_merged_out);
}

API int shp_dsegpoints_emit(shp_ctx *ctx, uint32_t id_lo, uint32_t id_hi, int64_t *offs_out, void *pts_out,
                            int64_t cap, int64_t *npts_out)
{
    const int stage = ctx ? ctx->dpts.stage : 0;
    CHK(enter(ctx));
    if (!offs_out || !npts_out || (cap > 0 && !pts_out) || cap < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (stage != 2) SHP_FAIL(ctx, SHP_ERR_STATE, "no merged point lists: shp_dsegpoints_merge_dev must come first");
    ctx->dpts.stage = 2;
    if (id_lo > id_hi || (uint64_t)id_hi > (uint64_t)ctx->pts.S + 1u)
        SHP_FAIL(ctx, SHP_ERR_ARG, "id range %u..%u outside 0..%llu", id_lo, id_hi,
                 (unsigned long long)ctx->pts.S + 1ull);
    return run_dsegpoints_emit(ctx, id_lo, id_hi, offs_out, pts_out, cap, npts_out);
}

// the multi-GPU split with everything left in device memory (spatial.h: run_dspatial_local / run_dspatial_merge)
static int dspatial_check(shp_ctx *ctx, int func, const double *params, uint32_t max_seg_id, int nint, int nflt)
{
    if (!params || nint < 0 || nflt < 0 || nint + nflt < 1) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if (func < 0 || func > 2) SHP_FAIL(ctx, SHP_ERR_ARG, "unknown built-in spatial function %d", func);
    if (func == 2 && !(params[0] >= 1.0 && params[0] <= 255.0))
        SHP_FAIL(ctx, SHP_ERR_ARG, "variogram maxDist must be 1..255 (got %g)", params[0]);
    if (max_seg_id == 0xffffffffu) SHP_FAIL(ctx, SHP_ERR_ARG, "max_seg_id too large");
    return 0;
}

API int shp_dspatial_local_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                               int64_t ncols, const uint32_t *d_seg_up, const void *d_band_up, int64_t rows_up,
                               const uint32_t *d_seg_dn, const void *d_band_dn, int64_t rows_dn, int64_t row0,
                               int64_t img_rows, uint32_t max_seg_id, int64_t null_val, int func, const double *params,
                               int64_t missing, int nint, int nflt, const uint32_t *d_hist, int keep_unheld,
                               void *d_cols, void **d_rec_out, int64_t *n_rec_out, int64_t *rec_words_out,
                               int64_t *checks_out)
{
    CHK(enter(ctx));
    if (!d_hist || !d_cols || !d_rec_out || !n_rec_out || !rec_words_out || !checks_out || dtype_size(dtype) == 0 ||
        nrows < 0 || ncols < 0 || rows_up < 0 || rows_dn < 0 || row0 < 0 ||
        (nrows > 0 && (!d_seg || !d_band)) || (rows_up > 0 && (!d_seg_up || !d_band_up)) ||
        (rows_dn > 0 && (!d_seg_dn || !d_band_dn)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    CHK(dspatial_check(ctx, func, params, max_seg_id, nint, nflt));
    if (rows_up > row0 || row0 + nrows + rows_dn > img_rows)
        SHP_FAIL(ctx, SHP_ERR_ARG, "window rows %lld..%lld outside the image's %lld rows", (long long)(row0 - rows_up),
                 (long long)(row0 + nrows + rows_dn), (long long)img_rows);
    // per rank: the own rows and each halo must stay below 2^32 pixels, the whole raster need not
    if ((uint64_t)nrows * (uint64_t)ncols >= 0xffffffffull || (uint64_t)rows_up * (uint64_t)ncols >= 0xffffffffull ||
        (uint64_t)rows_dn * (uint64_t)ncols >= 0xffffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "shard too large (%lld x %lld px)", (long long)nrows, (long long)ncols);
    SpatialWin w{d_seg, d_seg_up, d_seg_dn, d_band, d_band_up, d_band_dn, dtype, (uint32_t)ncols, (uint32_t)nrows,
                 (uint32_t)rows_up, (uint32_t)rows_dn, max_seg_id, (long long)null_val, (unsigned long long)row0};
    return run_dspatial_local(ctx, w, func, params, missing, nint, nflt, d_hist, keep_unheld, d_cols, d_rec_out,
                              n_rec_out, rec_words_out, checks_out);
}

API int shp_dspatial_merge_dev(shp_ctx *ctx, const void *d_recs, int64_t slot, int world, const uint32_t *counts,
                               uint32_t max_seg_id, int func, const double *params, int64_t missing, int nint, int nflt,
                               uint32_t id_lo, uint32_t id_hi, void *d_cols, int64_t *n_ids_out)
{
    CHK(enter(ctx));
    if (!counts || !d_cols || !n_ids_out || slot < 0 || world < 1 || slot >= 0xffffffffll || (slot > 0 && !d_recs))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    CHK(dspatial_check(ctx, func, params, max_seg_id, nint, nflt));
    if (id_hi > max_seg_id + 1u) SHP_FAIL(ctx, SHP_ERR_ARG, "id share beyond max_seg_id");
    for (int r = 0; r < world; r++) if ((int64_t)counts[r] > slot) SHP_FAIL(ctx, SHP_ERR_ARG, "counts[%d] exceeds the slot", r);
    return run_dspatial_merge(ctx, (const unsigned long long *)d_recs, (uint32_t)slot, (uint32_t)world, counts, max_seg_id,
                              func, params, missing, nint, nflt, id_lo, id_hi, d_cols, n_ids_out);
}

// the (segment, bin) pairs the last built-in variogram recomputed in the reference's order (one GPU)
API int shp_spatial_vario_redo_count(shp_ctx *ctx, int64_t *n_out)
{
    CHK(enter(ctx));
    if (!n_out) SHP_FAIL(ctx, SHP_ERR_ARG, "NULL argument");
    *n_out = ctx->vario_redo;
    return 0;
}

// the flagged pairs (s * maxd + bin, ascending) of the last shp_dspatial_local_dev / shp_dspatial_merge_dev call:
// *n_out of them, copied into out when cap holds them all
API int shp_dspatial_vario_pairs(shp_ctx *ctx, uint64_t *out, int64_t cap, int64_t *n_out)
{
    CHK(enter(ctx));
    if (!n_out || cap < 0) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    *n_out = (int64_t)ctx->vario_pairs.size();
    if (out && cap >= *n_out && *n_out) memcpy(out, ctx->vario_pairs.data(), (size_t)*n_out * 8);
    return 0;
}

// The variogram's pairs (ascending, all ids <= max_seg_id) again over the own rows nrows x ncols, the halo of
// rows_dn rows below them holding the partners there; sum / cnt (host, np each) carry the rows above in and the
// rows up to the end of the own rows out.
API int shp_dspatial_vario_redo_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                                    int64_t ncols, const uint32_t *d_seg_dn, const void *d_band_dn, int64_t rows_dn,
                                    uint32_t max_seg_id, int64_t null_val, int maxd, const uint64_t *pairs,
                                    int64_t np, double *sum, uint32_t *cnt)
{
    CHK(enter(ctx));
    if (dtype_size(dtype) == 0 || nrows < 0 || ncols < 0 || rows_dn < 0 || np < 0 || np >= 0x7fffffffll ||
        maxd < 1 || maxd > 255 || (nrows > 0 && (!d_seg || !d_band)) || (rows_dn > 0 && (!d_seg_dn || !d_band_dn)) ||
        (np > 0 && (!pairs || !sum || !cnt)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    if ((uint64_t)nrows * (uint64_t)ncols >= 0xffffffffull || (uint64_t)rows_dn * (uint64_t)ncols >= 0xffffffffull)
        SHP_FAIL(ctx, SHP_ERR_ARG, "shard too large (%lld x %lld px)", (long long)nrows, (long long)ncols);
    if (max_seg_id == 0xffffffffu) SHP_FAIL(ctx, SHP_ERR_ARG, "max_seg_id too large");
    for (int64_t j = 0; j < np; j++)
        if (pairs[j] / (uint64_t)maxd > max_seg_id) SHP_FAIL(ctx, SHP_ERR_ARG, "pair %lld beyond max_seg_id", (long long)j);
    SpatialWin w{d_seg, nullptr, d_seg_dn, d_band, nullptr, d_band_dn, dtype, (uint32_t)ncols, (uint32_t)nrows, 0u,
                 (uint32_t)rows_dn, max_seg_id, (long long)null_val, 0ull};
    return spatial_vario_redo(ctx, w, (uint32_t)maxd, (const unsigned long long *)pairs, (uint32_t)np, sum, cnt);
}

// the pairs' variogram entries of the column block d_cols (nint int64 columns, then nflt float32 columns of
// max_seg_id + 1 ids): (float)sqrt(sum / cnt) where write, else 0
API int shp_dspatial_vario_store_dev(shp_ctx *ctx, const uint64_t *pairs, int64_t np, const double *sum,
                                     const uint32_t *cnt, int maxd, uint32_t max_seg_id, int nint, int nflt,
                                     void *d_cols, int write)
{
    CHK(enter(ctx));
    if (np < 0 || np >= 0x7fffffffll || maxd < 1 || maxd > 255 || nint < 0 || nflt < 0 || !d_cols ||
        (np > 0 && (!pairs || !sum || !cnt)))
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    const size_t ns = (size_t)max_seg_id + 1;
    return spatial_vario_store(ctx, (const unsigned long long *)pairs, (uint32_t)np, sum, cnt, (uint32_t)maxd, ns,
                               nflt, (float *)((long long *)d_cols + (size_t)nint * ns), write);
}

// Grow the context's workspace for tiles of up to npix pixels now (the buffers are grow-only and
// a regrow synchronises and reallocates in the middle of a run): the tiled drivers call this once
// per worker with the largest tile of the job, so that a pooled context does not keep growing
// until it has met that tile itself.
// the buffers one tile of npix pixels makes a worker context hold, and their sizes
typedef std::vector<std::pair<DevBuf shp_ctx::*, size_t>> ReservePlan;
static ReservePlan reserve_plan(int dtype, int nbands, size_t n)
{
    const size_t ns = n / 4 + 2;
    const uint32_t maxbig = (uint32_t)(n / (MAX_CLUMP_SIZE + 2u) + 1u);
    const size_t nblk = (n + SORT_TILE - 1) / SORT_TILE, nh = (size_t)256 * (nblk ? nblk : 1);
    ReservePlan pl;
    pl.push_back({&shp_ctx::img, (size_t)nbands * n * dtype_size(dtype)});
    pl.push_back({&shp_ctx::clus, n * 2});
    DevBuf shp_ctx::*perpix[] = {&shp_ctx::lab, &shp_ctx::aux, &shp_ctx::aux2, &shp_ctx::stack,
                                 &shp_ctx::sort_k0, &shp_ctx::sort_k1, &shp_ctx::sort_v1, &shp_ctx::pix};
    for (auto m : perpix) pl.push_back({m, n * 4});
    pl.push_back({&shp_ctx::segsz, (n + 2) * 4});
    pl.push_back({&shp_ctx::singles, (n + 2) * 4});
    pl.push_back({&shp_ctx::bigbits, (n / 32 + 2) * 4});
    pl.push_back({&shp_ctx::big, (size_t)maxbig * (sizeof(BigInfo) + 4) + 128});
    {       // the replay's bitmap snapshots: a walker-pool-sized slot per walker (run_clump)
        const size_t walkers = ((size_t)maxbig + DFS_WAVES - 1) / DFS_WAVES * DFS_WAVES;
        const size_t cap = (size_t)DFS_MAX_BLOCKS * DFS_WAVES;
        pl.push_back({&shp_ctx::snap, (walkers < cap ? walkers : cap) * DFS_POOL_GRANS_DEFAULT * DFS_GRAN_WORDS * 4});
    }
    pl.push_back({&shp_ctx::sort_hist, 2 * nh * 4});
    pl.push_back({&shp_ctx::scan_tmp, scan_tmp_bytes(n > nh ? n : nh)});
    pl.push_back({&shp_ctx::chnext, ns * 16});       // the pass loop's chunk records (uint4 per segment)
    DevBuf shp_ctx::*perseg[] = {&shp_ctx::origsz, &shp_ctx::mergeto,
                                 &shp_ctx::tcount, &shp_ctx::tfill, &shp_ctx::tsorted, &shp_ctx::srclist,
                                 &shp_ctx::tgtlist};
    for (auto m : perseg) pl.push_back({m, ns * 4});
    pl.push_back({&shp_ctx::off, ns * 4 + 16});
    pl.push_back({&shp_ctx::toff, ns * 4 + 16});
    pl.push_back({&shp_ctx::tlist, (ns + 32) * 4});
    pl.push_back({&shp_ctx::ssum, ns * (size_t)nbands * 4});
    pl.push_back({&shp_ctx::small, 8192});
    return pl;
}

API int shp_ctx_reserve(shp_ctx *ctx, int dtype, int nbands, int64_t npix)
{
    CHK(enter(ctx));
    if (dtype_size(dtype) == 0 || nbands < 1 || npix < 0 || npix >= 0x7fffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    for (const auto &e : reserve_plan(dtype, nbands, (size_t)npix)) CHK(buf_ensure(ctx, ctx->*(e.first), e.second));
    return 0;
}

// How much more device memory shp_ctx_reserve(dtype, nbands, npix) would allocate on this context
// (what it already holds counts), and the device's free / total memory: the tiled driver sizes its
// worker count with these instead of running out of memory on very large tiles.
API int shp_ctx_reserve_query(shp_ctx *ctx, int dtype, int nbands, int64_t npix, int64_t *extra_bytes,
                              int64_t *free_bytes, int64_t *total_bytes)
{
    CHK(enter(ctx));
    if (dtype_size(dtype) == 0 || nbands < 1 || npix < 0 || npix >= 0x7fffffffll)
        SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    size_t extra = 0;
    for (const auto &e : reserve_plan(dtype, nbands, (size_t)npix)) {
        const size_t bytes = e.second ? e.second : 16;
        if ((ctx->*(e.first)).cap < bytes) extra += bytes + bytes / 8 + 256;       // as buf_ensure grows
    }
    if (extra_bytes) *extra_bytes = (int64_t)extra;
    if (free_bytes || total_bytes) {
        size_t fr = 0, tot = 0;
        HIPCHK(ctx, hipMemGetInfo(&fr, &tot));
        if (free_bytes) *free_bytes = (int64_t)fr;
        if (total_bytes) *total_bytes = (int64_t)tot;
    }
    return 0;
}

// ---- RCCL communicator (multi-GPU stitch exchange) ----------------------------------------------
API int shp_comm_unique_id(void *id_out_128)
{
    if (!id_out_128) return SHP_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    return ncclGetUniqueId((ncclUniqueId *)id_out_128) == ncclSuccess ? SHP_OK : SHP_ERR_HIP;
}

API int shp_comm_create(shp_ctx *ctx, int rank, int world, const void *unique_id_128, shp_comm **out)
{
    CHK(enter(ctx));
    if (!out || !unique_id_128 || world < 1 || rank < 0 || rank >= world) SHP_FAIL(ctx, SHP_ERR_ARG, "bad argument");
    *out = nullptr;
    shp_comm *cm = new shp_comm();
    cm->ctx = ctx; cm->rank = rank; cm->world = world;
    ncclUniqueId id;
    memcpy(&id, unique_id_128, sizeof(id));
    ncclResult_t r = ncclCommInitRank(&cm->nc, world, id, rank);        // (the context's device is current)
    if (r != ncclSuccess) {
        delete cm;
        SHP_FAIL(ctx, SHP_ERR_HIP, "ncclCommInitRank(rank %d of %d): %s", rank, world, ncclGetErrorString(r));
    }
    if (hipStreamCreateWithFlags(&cm->cstream, hipStreamNonBlocking) != hipSuccess) {
        ncclCommDestroy(cm->nc);
        delete cm;
        SHP_FAIL(ctx, SHP_ERR_HIP, "hipStreamCreate for the communicator failed");
    }
    *out = cm;
    return 0;
}

API void shp_comm_destroy(shp_comm *cm)
{
    if (!cm) return;
    if (cm->ctx) { hipSetDevice(cm->ctx->device); hipStreamSynchronize(cm->ctx->stream); }
    if (cm->cstream) { hipStreamSynchronize(cm->cstream); hipStreamDestroy(cm->cstream); }
    for (hipEvent_t e : cm->evpool) hipEventDestroy(e);
    if (cm->nc) ncclCommDestroy(cm->nc);
    delete cm;
}

// what RCCL itself says the communicator spans (ncclCommCount): bench lines quote it
API int shp_comm_count(shp_comm *cm, int *nranks_out)
{
    if (!cm || !nranks_out) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    NCCLCHK(cm->ctx, ncclCommCount(cm->nc, nranks_out));
    return 0;
}

// ncclGroupStart / ncclGroupEnd around the asynchronous calls (a send and its matching receive of ONE
// rank must be grouped; between different ranks the calls pair up by themselves)
API int shp_comm_group(shp_comm *cm, int begin)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    NCCLCHK(cm->ctx, begin ? ncclGroupStart() : ncclGroupEnd());
    return 0;
}

// Asynchronous send of a device buffer that `producer`'s stream is still writing: enqueued on the
// communicator's stream behind an event recorded on the producer's stream now.  Returns at once.
API int shp_comm_isend(shp_comm *cm, const void *d_buf, size_t bytes, int dst, shp_ctx *producer)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    if ((!d_buf && bytes) || dst < 0 || dst >= cm->world) SHP_FAIL(cm->ctx, SHP_ERR_ARG, "bad argument");
    if (producer) {
        hipEvent_t e = comm_event(cm);
        if (!e) SHP_FAIL(cm->ctx, SHP_ERR_HIP, "hipEventCreate failed");
        HIPCHK(cm->ctx, hipEventRecord(e, producer->stream));
        HIPCHK(cm->ctx, hipStreamWaitEvent(cm->cstream, e, 0));
    }
    NCCLCHK(cm->ctx, ncclSend(d_buf, bytes, ncclUint8, dst, cm->nc, cm->cstream));
    return 0;
}

// Asynchronous receive into a device buffer that `consumer`'s stream will read: enqueued on the
// communicator's stream; the consumer's stream is made to wait (on the device) for its completion.
API int shp_comm_irecv(shp_comm *cm, void *d_buf, size_t bytes, int src, shp_ctx *consumer)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    if ((!d_buf && bytes) || src < 0 || src >= cm->world) SHP_FAIL(cm->ctx, SHP_ERR_ARG, "bad argument");
    NCCLCHK(cm->ctx, ncclRecv(d_buf, bytes, ncclUint8, src, cm->nc, cm->cstream));
    if (consumer) {
        hipEvent_t e = comm_event(cm);
        if (!e) SHP_FAIL(cm->ctx, SHP_ERR_HIP, "hipEventCreate failed");
        HIPCHK(cm->ctx, hipEventRecord(e, cm->cstream));
        HIPCHK(cm->ctx, hipStreamWaitEvent(consumer->stream, e, 0));
    }
    return 0;
}

// `consumer`'s stream waits (on the device) for everything enqueued on the communicator's stream so far:
// for receives issued inside a group, whose ncclRecv is only enqueued by shp_comm_group(0)
API int shp_comm_wait(shp_comm *cm, shp_ctx *consumer)
{
    if (!cm || !consumer) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    hipEvent_t e = comm_event(cm);
    if (!e) SHP_FAIL(cm->ctx, SHP_ERR_HIP, "hipEventCreate failed");
    HIPCHK(cm->ctx, hipEventRecord(e, cm->cstream));
    HIPCHK(cm->ctx, hipStreamWaitEvent(consumer->stream, e, 0));
    return 0;
}

// host waits until every asynchronous operation issued so far has completed
API int shp_comm_drain(shp_comm *cm)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    HIPCHK(cm->ctx, hipStreamSynchronize(cm->cstream));
    return 0;
}

API int shp_comm_send(shp_comm *cm, const void *d_buf, size_t bytes, int dst)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    if ((!d_buf && bytes) || dst < 0 || dst >= cm->world) SHP_FAIL(cm->ctx, SHP_ERR_ARG, "bad argument");
    NCCLCHK(cm->ctx, ncclSend(d_buf, bytes, ncclUint8, dst, cm->nc, cm->ctx->stream));
    return comm_finish(cm);
}

API int shp_comm_recv(shp_comm *cm, void *d_buf, size_t bytes, int src)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    if ((!d_buf && bytes) || src < 0 || src >= cm->world) SHP_FAIL(cm->ctx, SHP_ERR_ARG, "bad argument");
    NCCLCHK(cm->ctx, ncclRecv(d_buf, bytes, ncclUint8, src, cm->nc, cm->ctx->stream));
    return comm_finish(cm);
}

API int shp_comm_bcast(shp_comm *cm, void *d_buf, size_t bytes, int root)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    if ((!d_buf && bytes) || root < 0 || root >= cm->world) SHP_FAIL(cm->ctx, SHP_ERR_ARG, "bad argument");
    NCCLCHK(cm->ctx, ncclBroadcast(d_buf, d_buf, bytes, ncclUint8, root, cm->nc, cm->ctx->stream));
    return comm_finish(cm);
}

// every rank contributes bytes_per_rank bytes; d_recv holds world * bytes_per_rank
API int shp_comm_allgather(shp_comm *cm, const void *d_send, void *d_recv, size_t bytes_per_rank)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    if (!d_send || !d_recv) SHP_FAIL(cm->ctx, SHP_ERR_ARG, "NULL argument");
    NCCLCHK(cm->ctx, ncclAllGather(d_send, d_recv, bytes_per_rank, ncclUint8, cm->nc, cm->ctx->stream));
    return comm_finish(cm);
}

// in place; op 0 = sum of int64, 1 = max of float64
API int shp_comm_allreduce(shp_comm *cm, void *d_buf, size_t count, int op)
{
    if (!cm) return SHP_ERR_ARG;
    CHK(enter(cm->ctx));
    if ((!d_buf && count) || (op != 0 && op != 1)) SHP_FAIL(cm->ctx, SHP_ERR_ARG, "bad argument");
    NCCLCHK(cm->ctx, ncclAllReduce(d_buf, d_buf, count, op == 0 ? ncclInt64 : ncclFloat64,
                                   op == 0 ? ncclSum : ncclMax, cm->nc, cm->ctx->stream));
    return comm_finish(cm);
}
