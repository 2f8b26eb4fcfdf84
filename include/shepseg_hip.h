/*
 * shepseg_hip.h -- C-ABI of libshepseg_hip.so, the MI355X (gfx950) implementation of the
 * pyshepseg per-tile segmentation hot path and its tiled driver.
 *
 * The reference (ubarsc/pyshepseg v2.0.3) has no native/FFI boundary: its operator API is
 * three Python call signatures whose arithmetic runs in numba @njit functions and in
 * sklearn.cluster.KMeans.  Each entry point below replaces the reference function(s)
 * cited next to it; pyshepseg_amd/{shepseg,tiling,tilingstats}.py bind them with ctypes
 * under the reference's own Python names (see INTEGRATION.md for the stub).
 *
 * Conventions
 *  - return 0 = OK, negative = error; message via shp_last_error(ctx).
 *  - the caller owns every host buffer; the library borrows pointers for the call only.
 *  - all arrays C-contiguous; images are band-planar (nBands, nRows, nCols) like the
 *    reference's `img` (shepseg.py:140).
 *  - one shp_ctx per host thread / HIP stream; calls on different contexts are re-entrant
 *    (the reference calls doShepherdSegmentation from N threads, tiling.py:1560-1595).
 *  - there is NO CPU fallback: every entry point fails with SHP_ERR_NO_DEVICE when no
 *    gfx950 device is usable.
 */
#ifndef SHEPSEG_HIP_H
#define SHEPSEG_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct shp_ctx shp_ctx;

/* image dtypes (the integer dtypes the reference accepts for `img`) */
enum { SHP_U8 = 0, SHP_I16 = 1, SHP_U16 = 2, SHP_I32 = 3, SHP_U32 = 4 };

enum {
    SHP_OK = 0,
    SHP_ERR_NO_DEVICE = -1,
    SHP_ERR_HIP = -2,
    SHP_ERR_ARG = -3,
    SHP_ERR_NOMEM = -4,
    SHP_ERR_STATE = -5
};

int shp_version(void);
int shp_device_count(void);                      /* number of usable HIP devices (0 = none) */
int shp_ctx_create(int device, shp_ctx **out);   /* owns one HIP stream + device workspace */
int shp_ctx_create_priority(int device, shp_ctx **out);  /* same, highest stream priority */
/* A worker context of the tiled drivers: device workspace without a stream of its own.  Inside the
 * worker calls (shp_assign_rects_dev, shp_segment_window_dev, shp_segment_tile_to_dev,
 * shp_stitch_prepare_dev) it borrows a stream of a process-wide pool for each phase (SHEPSEG_FILL_MAX
 * fill streams, SHEPSEG_WALK_STREAMS = 12 walker streams), so that more tiles than hardware queues
 * can be in flight; other calls run on one idle stream all shared contexts use. */
int shp_ctx_create_shared(int device, shp_ctx **out);
/* Grow the context's (grow-only) workspace for tiles of up to npix pixels of this type now, instead
 * of in the middle of a run when the first such tile arrives.  The reference has no counterpart
 * (numpy allocates per call); the tiled drivers call it once per worker thread
 * (SegThreadsMgr.worker, tiling.py:1560-1600) with the job's largest tile. */
int shp_ctx_reserve(shp_ctx *ctx, int dtype, int nbands, int64_t npix);
/* what that reservation would still allocate on this context (bytes), and the device's free and
 * total memory: the tiled driver starts only as many workers as fit (SegThreadsMgr's numWorkers,
 * tiling.py:1531-1600, has no such limit because its tiles live in host memory) */
int shp_ctx_reserve_query(shp_ctx *ctx, int dtype, int nbands, int64_t npix, int64_t *extra_bytes,
                          int64_t *free_bytes, int64_t *total_bytes);
void shp_ctx_destroy(shp_ctx *ctx);
const char *shp_last_error(const shp_ctx *ctx);  /* valid until the next call on ctx */
/* device-time (HIP events on the ctx stream) of the stages of the last shp_segment_tile /
 * stage call, milliseconds: [0]=assign [1]=clump [2]=single-pixel [3]=small-segment
 * [4]=h2d [5]=d2h [6]=total.  out must hold 8 doubles. */
int shp_last_timings(const shp_ctx *ctx, double *out);
/* accumulated device time (ms, HIP events on the ctx stream) and launch count of the
 * instrumented kernels: ids 0 assign, 1 ccl, 2 dfs_pool (the replay), 3 radix sort, 4 spectra,
 * 5 small-segment pass loop, 7 seed scan + final labels.  reset != 0 clears the counters. */
int shp_prof_get(shp_ctx *ctx, double *ms_out, uint64_t *count_out, int n, int reset);
/* process-wide counters of the launches that carry the tiles' latency-bound kernels, one launch for every
 * tile that is ready (csrc/walkbatch.h).  out receives six values: launches, jobs (tiles) and the largest
 * batch of the depth-first replay, then the same three of the small-segment pass loop.  A launch of a
 * context that owns its stream counts as a batch of one.  reset != 0 clears the counters.  Read-only
 * otherwise: it changes nothing about how the work runs. */
int shp_walk_batch_stats(uint64_t *out, int reset);
/* the workgroups of the same launches.  out receives four values: the sum of workgroups over all launches
 * and the most workgroups in one launch of the replay, then the same two of the pass loop.  The reset of
 * shp_walk_batch_stats clears them too.  Read-only. */
int shp_walk_batch_blocks(uint64_t *out);
/* process-wide count of pass-loop launches per compiled instance of the loop (csrc/elim_small.h).  out receives
 * five values: launches of the generic instance (any band count, either connectivity, diagnostics), of the
 * 6-band 4-connected and 8-connected instances, of the 10-band 4-connected and 8-connected instances.  A batch
 * is one launch; jobs that disagree run on the generic instance.  reset != 0 clears the counters after they
 * are read.  Read-only otherwise. */
int shp_small_loop_instances(uint64_t *out, int reset);

/* ---- k-means ------------------------------------------------------------------------ */
/* replaces sklearn KMeans(init=<array>, n_init=1).fit as called by
 * shepseg.fitSpectralClusters (shepseg.py:305-312).  xsample: nrows*nbands float64 rows.
 * The reference's sklearn 0.24.2 runs ELKAN's variant for k > 1 (algorithm="auto").  The fit runs
 * Lloyd iterations (same partitions, far fewer bytes) under a guard and starts over with Elkan's
 * algorithm as the reference evaluates it -- bounds, strict-improvement relabelling, row-order sums --
 * as soon as a sample's two nearest centres are within 1e-12 (relative): there the result is the
 * reference's with one OpenMP thread bit for bit (pyshepseg_amd/csrc/fit_elkan.h).
 * SHEPSEG_FIT_ALGO=lloyd|elkan forces one path. */
int shp_kmeans_fit(shp_ctx *ctx, const double *xsample, int64_t nrows, int nbands, int k,
                   const double *init_centres, int max_iter, double tol_rel,
                   double *centres_out, int32_t *labels_out, int *n_iter_out);
/* the same with the sample rows in the image's pixel type (SHP_U8 ... SHP_U32): sklearn's
 * check_array conversion to float64 happens on the fly, the arithmetic is unchanged. */
int shp_kmeans_fit_typed(shp_ctx *ctx, const void *xsample, int dtype, int64_t nrows, int nbands,
                         int k, const double *init_centres, int max_iter, double tol_rel,
                         double *centres_out, int32_t *labels_out, int *n_iter_out);
/* The same from the BAND-PLANAR sub-sample (nbands planes of npix pixels, as shp_dev_subsample
 * returns it): rows with null_val in any band are dropped when has_null, init_centres == NULL means
 * the reference's diagonalClusterCentres (shepseg.py:364-397) of the rows kept; *nrows_out = rows the
 * model was fitted on (labels_out, optional, receives that many).  Identical arithmetic (each band's
 * sums are one chain in row order), prepared by one host thread per band, no host transposition. */
int shp_kmeans_fit_planar(shp_ctx *ctx, const void *planes, int dtype, int64_t npix, int nbands,
                          int has_null, int64_t null_val, int k, const double *init_centres,
                          int max_iter, double tol_rel, double *centres_out, int32_t *labels_out,
                          int *n_iter_out, int64_t *nrows_out);

/* The same with the E-step of the reference's algorithm SHARDED BY SAMPLE ROWS over the ranks of an RCCL
 * communicator (shp_comm_create): every rank passes the SAME sample and receives the SAME model.  Rank r keeps
 * the bounds of rows [r n/N, (r+1) n/N) and relabels them; the labels are all-gathered in place on the fit's
 * stream every iteration (ncclAllGather, no host round trip) and every rank runs the M-step on all of them --
 * same sums in the same order, so no broadcast of centres.  The reference's fit is one process
 * (shepseg.py:305-312); bit-identical to shp_kmeans_fit_planar.  cm == NULL or one rank: that call. */
struct shp_comm;
int shp_kmeans_fit_planar_dist(shp_ctx *ctx, struct shp_comm *cm, const void *planes, int dtype, int64_t npix,
                               int nbands, int has_null, int64_t null_val, int k, const double *init_centres,
                               int max_iter, double tol_rel, double *centres_out, int32_t *labels_out,
                               int *n_iter_out, int64_t *nrows_out);

/* which path the context's last fit took: 0 Lloyd iterations (no near tie met), 1 Elkan's */
int shp_last_fit_path(const shp_ctx *ctx);

/* replaces shepseg.applySpectralClusters (shepseg.py:317-361) + KMeans.predict:
 * clusters_out[nrows*ncols] int32, 1..k, 0 where any band == null_val. */
int shp_kmeans_assign(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows, int ncols,
                      const double *centres, int k, int has_null, int64_t null_val,
                      int32_t *clusters_out);

/* ---- per-tile stages (individually callable, like the reference's njit functions) ------ */
/* replaces shepseg.clump(img, ignoreVal=0, fourConnected, clumpId=1) (shepseg.py:452-541),
 * including the MAX_CLUMP_SIZE=10000 depth-first cut.  max_seg_id_out = next id - 1. */
int shp_clump(shp_ctx *ctx, const int32_t *clusters, int nrows, int ncols, int four_connected,
              uint32_t *seg_out, uint32_t *max_seg_id_out);

/* replaces shepseg.makeSegSize (shepseg.py:544-569): seg_size_out has max_seg_id+1 entries */
int shp_make_seg_size(shp_ctx *ctx, const uint32_t *seg, int64_t npix, uint32_t max_seg_id,
                      uint32_t *seg_size_out);

/* replaces shepseg.eliminateSinglePixels (shepseg.py:572-615): seg relabelled in place;
 * max_seg_id_inout: in = largest id in seg, out = seg.max() after the relabel (when an id
 * >= min_seg_id survives).  min_seg_id >= 1: relabelSegments keeps the ids up to it and closes
 * the gaps above it (shepseg.py:766-769). */
int shp_eliminate_single(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows,
                         int ncols, int four_connected, uint32_t *seg_inout,
                         uint32_t *max_seg_id_inout, uint32_t min_seg_id);

/* replaces shepseg.eliminateSmallSegments (shepseg.py:918-1000); min_seg_id >= 1: segments with
 * smaller ids are never eliminated (segIdRange, shepseg.py:964), and the relabel is as above */
int shp_eliminate_small(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows,
                        int ncols, int four_connected, int min_seg_size,
                        double max_spectral_diff, uint32_t *seg_inout,
                        uint32_t *max_seg_id_inout, int64_t *num_elim_out, uint32_t min_seg_id);

/* replaces shepseg.doShepherdSegmentation with a supplied k-means model
 * (shepseg.py:130-249, stages :206 :212 :219 :225 :235), fused on the device. */
int shp_segment_tile(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows, int ncols,
                     const double *centres, int k, int has_null, int64_t null_val,
                     int four_connected, int min_seg_size, double max_spectral_diff,
                     uint32_t *seg_out, uint32_t *max_seg_id_out, int64_t *singles_elim_out,
                     int64_t *small_elim_out, uint32_t *num_clumps_out);

/* ---- synthetic imagery (benchmark input; SURVEY.md Appendix B `synthimg v1`) ----------- */
int shp_synthimg(shp_ctx *ctx, uint64_t seed, int nbands, int64_t y0, int64_t x0, int nrows,
                 int ncols, uint16_t *out_host);

/* ---- device-resident rasters: tiled driver + cross-tile stitch --------------------------------
 * Device pointers cross the boundary as plain void* / uint32_t* (they come from shp_dev_alloc).
 * These replace the per-tile loop and the stitch of tiling.doTiledShepherdSegmentation:
 *   SegNoConcurrencyMgr.segmentAllTiles / SegThreadsMgr.worker (tiling.py:1413-1469, :1560-1600)
 *   stitchTiles / recodeTile / recodeSharedSegments / relabelSegments (tiling.py:950-1306)
 *   HistogramAccumulator (tiling.py:1915-1963), readSubsampledImageBand (tiling.py:259-314). */
int shp_dev_alloc(shp_ctx *ctx, size_t bytes, void **dptr);
int shp_dev_free(shp_ctx *ctx, void *dptr);
int shp_dev_upload(shp_ctx *ctx, void *dst_dev, const void *src_host, size_t bytes);
int shp_dev_download(shp_ctx *ctx, void *dst_host, const void *src_dev, size_t bytes);
int shp_dev_memset(shp_ctx *ctx, void *dst_dev, int value, size_t bytes);
int shp_dev_copy(shp_ctx *ctx, void *dst_dev, const void *src_dev, size_t bytes);   /* D2D */
/* page-locked host buffers for the raster I/O pipeline (reads staged for H2D, finished output rows
 * staged from D2H): what the reference's per-tile GDAL ReadAsArray / WriteArray buffers become
 * (tiling.py:1436-1443, :1032-1034) */
int shp_host_alloc(shp_ctx *ctx, size_t bytes, void **hptr);
int shp_host_free(shp_ctx *ctx, void *hptr);
int shp_sync(shp_ctx *ctx);
/* synthimg v1 window written straight into device memory (band-planar uint16) */
int shp_dev_synthimg(shp_ctx *ctx, uint64_t seed, int nbands, int64_t y0, int64_t x0, int nrows,
                     int ncols, void *d_out);
/* synthetic label raster of block_rows x block_cols-pixel blocks numbered row-major from 1 (the
 * benchmark input of the statistics path, BASELINE config 5: "~50M segments"); *max_id_out = the
 * number of blocks.  Benchmark plumbing like shp_dev_synthimg: it replaces nothing in the reference. */
int shp_dev_block_labels(shp_ctx *ctx, int nrows, int ncols, int block_rows, int block_cols,
                         uint32_t *d_out, uint32_t *max_id_out);
/* out_host[b][i][j] = img[b][row_idx[i]][col_idx[j]] of a device raster (k-means subsample) */
int shp_dev_subsample(shp_ctx *ctx, const void *d_img, int dtype, int nbands, int nrows, int ncols,
                      const uint32_t *row_idx, int ny, const uint32_t *col_idx, int nx,
                      void *out_host);
/* doShepherdSegmentation on window (x, y, xs, ys) of a device raster; labels (ys*xs uint32,
 * local ids) are written to device memory d_seg_out.  Synchronous on return.  d_clusmap: NULL, or
 * the raster-wide cluster map whose window has been filled by shp_assign_rects_dev (the k-means
 * predict step of shepseg.py:211 is then not repeated for the pixels tiles share). */
int shp_segment_window_dev(shp_ctx *ctx, const void *d_img, int dtype, int nbands, int img_rows,
                           int img_cols, int x, int y, int xs, int ys, const double *centres, int k,
                           int has_null, int64_t null_val, int four_connected, int min_seg_size,
                           double max_spectral_diff, uint32_t *d_seg_out, uint32_t *max_seg_id_out,
                           int64_t *singles_elim_out, int64_t *small_elim_out,
                           uint32_t *num_clumps_out, const uint16_t *d_clusmap);
/* km.predict (shepseg.py:211, with the null mask of :205-207) on rectangles of a device raster:
 * d_clusmap[y][x] (uint16, img_rows x img_cols) = 0 for a null pixel, else cluster + 1.
 * rects = nrects x (x, y, xs, ys).  The model is global (tiling.py:154-226), so the tiled driver
 * assigns every pixel once instead of once per overlapping tile. */
int shp_assign_rects_dev(shp_ctx *ctx, const void *d_img, int dtype, int nbands, int img_rows,
                         int img_cols, const int32_t *rects, int nrects, const double *centres,
                         int k, int has_null, int64_t null_val, uint16_t *d_clusmap);
/* same with the tile image handed over as a host buffer (read -> H2D -> segment) */
int shp_segment_tile_to_dev(shp_ctx *ctx, const void *img, int dtype, int nbands, int nrows,
                            int ncols, const double *centres, int k, int has_null, int64_t null_val,
                            int four_connected, int min_seg_size, double max_spectral_diff,
                            uint32_t *d_seg_out, uint32_t *max_seg_id_out,
                            int64_t *singles_elim_out, int64_t *small_elim_out,
                            uint32_t *num_clumps_out);
/* one tile of stitchTiles, asynchronous on the ctx stream (call shp_sync to wait):
 * d_tile (ys*xs local ids) is recoded in place against the already-recoded strips of the tile
 * above (d_top_b: first row of its last `overlap` rows, row pitch top_pitch elements) and of the
 * tile to the left (d_left_b: first of its last `overlap` columns, pitch left_pitch); NULL where
 * there is no such neighbour.  The trimmed window [top,bottom) x [left,right) is written to
 * d_out at (yout, xout) (row pitch out_pitch) and *d_max_seg_id (device scalar) advances to the
 * largest id in it.  max_local = largest local id in d_tile. */
int shp_stitch_tile_dev(shp_ctx *ctx, uint32_t *d_tile, int ys, int xs, int overlap,
                        const uint32_t *d_top_b, int64_t top_pitch, const uint32_t *d_left_b,
                        int64_t left_pitch, uint32_t max_local, int simple_recode,
                        uint32_t *d_max_seg_id, int top, int bottom, int left, int right,
                        uint32_t *d_out, int64_t out_pitch, int xout, int yout);
/* The same stitch split in phases so that only a thin part is sequential (tiling.py:950-1306):
 *  shp_stitch_prepare_dev -- purely local to the tile, run by the worker that segmented it:
 *     fills d_meta = 4 x (max_local+1) uint32: flags (1 = crosses the top strip's midline,
 *     2 = crosses the left strip's, 4 = has a pixel in the trimmed window), bounding-box top row,
 *     bounding-box left column, and room for the LUT.  cross_px_out (may be NULL) receives the
 *     number of pixels of the top / left strip that belong to midline-crossing segments: handed
 *     to the chain call, it bounds the (segment, neighbour id) pair table there.  Synchronous.
 *  shp_stitch_chain_dev -- the sequential step (asynchronous on the ctx stream): modes over the
 *     overlap strips of the tile above / to the left (d_top_b / d_left_b as in
 *     shp_stitch_tile_dev, but they now point at the DENSE recoded strips written by earlier
 *     chain calls), new-id ranks, LUT, *d_max_seg_id advance, and the tile's own recoded right
 *     strip (ys x overlap, pitch overlap) / bottom strip (overlap x xs, pitch xs) into
 *     d_right_out / d_bottom_out (NULL = not needed).  The tile itself is not modified.  If
 *     d_out is not NULL the trimmed window is written through the LUT to d_out on the ctx's side
 *     stream, off the chain (shp_sync waits for both streams). */
int shp_stitch_prepare_dev(shp_ctx *ctx, const uint32_t *d_tile, int ys, int xs, int overlap,
                           int has_top, int has_left, uint32_t max_local, int top, int bottom,
                           int left, int right, uint32_t *d_meta, uint32_t *cross_px_out);
int shp_stitch_chain_dev(shp_ctx *ctx, const uint32_t *d_tile, int ys, int xs, int overlap,
                         const uint32_t *d_top_b, int64_t top_pitch, const uint32_t *d_left_b,
                         int64_t left_pitch, uint32_t max_local, int simple_recode,
                         uint32_t *d_max_seg_id, int top, int bottom, int left, int right,
                         uint32_t *d_meta, uint32_t *d_right_out, uint32_t *d_bottom_out,
                         uint32_t *d_out, int64_t out_pitch, int xout, int yout,
                         uint32_t top_cross_px, uint32_t left_cross_px /* 0xFFFFFFFF = unknown */);

/* Parallel stitch of the sharded driver: every tile runs the chain step with a
 * PROVISIONAL base (tile index * stride, in *d_max_seg_id) so that it depends on its two
 * neighbours' strips only, not on the running maxSegId of all earlier tiles (reference
 * tiling.py:1029-1043).  shp_stitch_counts_dev reports what the step did -- d_out2[0] = new ids
 * handed out, d_out2[1] = the largest of them present in the trimmed window, both relative to
 * base (asynchronous) -- and once every tile's count is known shp_renumber_dev maps
 * id -> new_base[id / stride] + id % stride over a raster (new_base: ntiles host values;
 * synchronous).  The result equals the sequential chain iff out2[0] == out2[1] for every tile;
 * otherwise the driver reruns the sequential chain. */
int shp_stitch_counts_dev(shp_ctx *ctx, const uint32_t *d_meta, uint32_t max_local, uint32_t base,
                          uint32_t *d_out2);
int shp_renumber_dev(shp_ctx *ctx, uint32_t *d_raster, int64_t npix, uint32_t stride,
                     const uint32_t *new_base, int ntiles);
/* one stitched, trimmed tile (w x h at xout, yout of the device raster) sub-sampled into one overview
 * layer exactly as SegmentationConcurrencyMgr.writeOverviews does tile by tile (tiling.py:1360-1383):
 * every level-th pixel from offset level / 2 of the tile, written at (xout / level, yout / level),
 * clipped to the ov_w x ov_h layer.  Asynchronous, ordered behind the tile's output write. */
int shp_overview_window_dev(shp_ctx *ctx, const uint32_t *d_raster, int64_t pitch, int xout, int yout,
                            int w, int h, int level, uint32_t *d_ov, int ov_w, int ov_h);
/* overview layers of a row-sharded label raster (distributed.writeOutputDistributed): nrects rectangles of
 * six int64 each, {src0, rowStep, colStep, nrows, ncols, dst0}, host memory; pixel (r, c) of rectangle k is
 * d_raster[src0 + r * rowStep + c * colStep] and goes to d_packed[dst0 + r * ncols + c].  The rectangles are
 * non-empty and packed back to back (dst0 of the first 0, the last one ending at npacked); every index read
 * must lie in [0, npix), which is checked before the launch.  Synchronous. */
int shp_overview_rects_dev(shp_ctx *ctx, const uint32_t *d_raster, int64_t npix, const int64_t *rects,
                           int nrects, uint32_t *d_packed, int64_t npacked);
/* the band statistics the reference derives from the segment histogram (utils.estimateStatsFromHisto,
 * utils.py:47-95), evaluated as numpy evaluates them there (int64 sums, float64 pairwise sum for the
 * variance, float64 comparison for the median): out[0..5] = minimum, maximum, mean, standard deviation,
 * mode, median of hist[0..n).  Host only: no device work, no context. */
int shp_hist_stats(const uint32_t *hist, int64_t n, double *out);
/* histogram of a device label raster, hist_out_host[0..max_seg_id], entry 0 zeroed (the RAT
 * Histogram column, HistogramAccumulator tiling.py:1915-1963).  ncols = the raster's row length
 * (npix a multiple of it; lets a segment's pixels be combined per 2-D patch), or 0. */
int shp_histogram_dev(shp_ctx *ctx, const uint32_t *d_raster, int64_t npix, int64_t ncols,
                      uint32_t max_seg_id, uint32_t *hist_out_host);

/* ---- the tables of the elimination stage, exported ------------------------------------------------
 * shepseg.makeSegmentLocations (shepseg.py:880-915; RowColArray :816-870) as a CSR: segment s's pixels
 * are pix_out[offsets_out[s] .. offsets_out[s + 1]) (linear indices row * ncols + col, raster
 * order), s = 0 .. max_seg_id; offsets_out has max_seg_id + 2 entries, pix_out nrows * ncols.
 * (Entry 0 lists the null pixels; the reference's dict has no key 0.) */
int shp_segment_locations(shp_ctx *ctx, const uint32_t *seg, int nrows, int ncols, uint32_t max_seg_id,
                          uint32_t *offsets_out, uint32_t *pix_out);
/* shepseg.buildSegmentSpectra (shepseg.py:780-813): float32 per-band sums of every segment's pixels
 * accumulated in raster order, spect_sum_out[(max_seg_id + 1) * nbands], row 0 = the null pixels */
int shp_build_segment_spectra(shp_ctx *ctx, const uint32_t *seg, const void *img, int dtype, int nbands,
                              int nrows, int ncols, uint32_t max_seg_id, float *spect_sum_out);

/* ---- per-segment statistics ("tilingstats") ----------------------------------------------------
 * replaces tilingstats.accumulateSegDict / calcStatsForCompletedSegs / SegmentStats / RatPage
 * (tilingstats.py:466-617, :866-1008, :1949-2045) for one image band against a label raster.
 * stats_sel: nstats x 5 uint32 = {globalCol, statId, colType, colArrayIdx, param} exactly as
 * tilingstats.makeFastStatsSelection (:798-863) builds it; statId 0..7 = min, max, mean, stddev,
 * median, mode, percentile, pixcount; colType 0 = integer column, 1 = float column.
 * intcols_out: (#int stats) x (max_seg_id+1) int64; floatcols_out: (#float stats) x
 * (max_seg_id+1) float32 (the RatPage arrays, all pages concatenated); row 0 is zero. */
int shp_segstats(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t npix,
                 uint32_t max_seg_id, int has_null, int64_t null_val, const uint32_t *stats_sel,
                 int nstats, int64_t missing, int64_t *intcols_out, float *floatcols_out);
/* same with the label raster and the band already in device memory */
int shp_segstats_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                     int64_t npix, uint32_t max_seg_id, int has_null, int64_t null_val,
                     const uint32_t *stats_sel, int nstats, int64_t missing,
                     int64_t *intcols_out, float *floatcols_out);
/* The same for a raster whose shape is known (nrows x ncols pixels, row-major; one tile block of
 * calcPerSegmentStatsTiled, tilingstats.py:183-206): where the average segment is at most 64 pixels the
 * statistics are computed patch by patch in LDS and only the segments that straddle patches are sorted. */
int shp_segstats2d_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                       int64_t nrows, int64_t ncols, uint32_t max_seg_id, int has_null, int64_t null_val,
                       const uint32_t *stats_sel, int nstats, int64_t missing,
                       int64_t *intcols_out, float *floatcols_out);

/* Multi-GPU split of the statistics: a segment that straddles two ranks' rows needs its
 * pixels from both.  Writes (segment id, band value) of every pixel whose segment id s has
 * flags[s] != 0 (flags: max_seg_id+1 bytes, host) to the host arrays, in no particular order;
 * *count_out = number of such pixels (when it exceeds cap only the first cap pairs are stored).
 * Plays the part of the per-segment dictionaries the reference keeps alive across tiles until
 * checkSegComplete sees the whole segment (tilingstats.py:518-553). */
int shp_gather_flagged_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                           int64_t npix, uint32_t max_seg_id, const uint8_t *flags, int64_t cap,
                           uint32_t *seg_out, int64_t *val_out, int64_t *count_out);

/* Several bands of one image against the same label raster in one pass over the labels (the reference loops
 * calcPerSegmentStatsTiled over the bands, cmdline/tiling.py:238-251).  d_bands: nbands device pointers, the bands'
 * planes of the row block, all of pixel type dtype; has_null / null_val: one entry per band.  stats_sel: the bands'
 * selections one after the other (nstats_per_band[b] rows for band b), built as for ONE call: the column array
 * index runs through all bands.  intcols_out / floatcols_out: all bands' columns, (#int stats) x (max_seg_id+1)
 * int64 and (#float stats) x (max_seg_id+1) float32.  Every column has the bits shp_segstats2d_dev gives for its
 * band alone. */
int shp_segstats2d_bands_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *const *d_bands, int dtype, int nbands,
                             int64_t nrows, int64_t ncols, uint32_t max_seg_id, const int *has_null,
                             const int64_t *null_val, const uint32_t *stats_sel, const int *nstats_per_band,
                             int64_t missing, int64_t *intcols_out, float *floatcols_out);
/* shp_gather_flagged_dev for several bands: the ids once (seg_out), and val_out = nbands rows of cap int64 values,
 * every band's in the order of seg_out. */
int shp_gather_flagged_bands_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *const *d_bands, int dtype,
                                 int nbands, int64_t npix, uint32_t max_seg_id, const uint8_t *flags, int64_t cap,
                                 uint32_t *seg_out, int64_t *val_out, int64_t *count_out);

/* The same split with everything left in device memory (the data path of calcPerSegmentStatsDistributed and
 * calcPerSegmentStatsDistributedBands under RCCL; the reference has no counterpart: its per-segment dictionaries
 * live in one process, tilingstats.py:466-553).  One pair of calls serves any number of entries, and does what
 * depends on the labels alone once; a one-band caller passes nbands = nplanes = 1.  A "band" is an entry of the
 * caller's list (a plane, a null value, nstats_per_band[b] rows of stats_sel, built as for
 * shp_segstats2d_bands_dev), a "plane" a distinct image band; plane_of_band[b] < nplanes names the plane entry b
 * reads.
 *  shp_dstats_local_bands_dev: the statistics of all entries over this rank's nrows x ncols rows in one pass over
 *    the labels (as shp_segstats2d_bands_dev; one entry as shp_segstats2d_dev), then every id judged against the
 *    GLOBAL histogram d_hist (max_seg_id + 1 uint32 in device memory: the reference's segSize, :165): rows of
 *    segments complete on this rank stay, rows of straddlers (fewer pixels here than the histogram says) are
 *    cleared and their pixels packed, rows of ids nobody holds keep the "missing" values on the one rank that
 *    passes keep_unheld != 0 -- so the ranks' columns ADD UP to the one-GPU columns.  d_cols (caller's device
 *    memory): (#int stats) int64 columns then (#float stats) float32 columns of max_seg_id + 1 rows, all entries'
 *    side by side.  The straddlers' pixels: *d_pair_seg_out = *n_pairs_out uint32 ids (of *n_straddlers_out
 *    segments), *d_pair_val_out = nplanes rows of raw pixel values IN THE PLANES' PIXEL TYPE, *pair_row_bytes_out
 *    bytes apart (a multiple of 16), every row in the order of the ids; both in the context's workspace, valid
 *    until its next call.  Null values are not applied to the pairs: they belong to the entries and are applied at
 *    the merge.  A histogram that cannot belong to these labels is refused: ids with MORE pixels in these rows than
 *    d_hist gives them fail with SHP_ERR_ARG, the message naming their number.  nrows * ncols may be 0 (d_seg is
 *    not read).
 *  shp_dstats_merge_bands_dev: after the all-gathers -- d_pair_seg = `world` slots of `slot` ids, counts[r] valid in
 *    slot r, d_pair_val = `world` blocks of nplanes rows of values, slot_row_bytes apart on every rank -- the pairs
 *    with id_lo <= id < id_hi (*n_merged_out of them, of *n_ids_out segments) are picked once, all planes' values
 *    with them, reduced per entry with the same code and their rows written into d_cols.
 *  4 + nplanes * itemsize bytes per straddler pixel travel.  Summing d_cols over the ranks (one integer all-reduce
 *  over the whole block read as int64 words: every 32-bit half has at most one non-zero contributor) gives the
 *  columns shp_segstats2d_bands_dev returns, each with the bits shp_segstats2d_dev gives for its entry alone. */
int shp_dstats_local_bands_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *const *d_planes, int nplanes,
                               const int *plane_of_band, int dtype, int nbands, int64_t nrows, int64_t ncols,
                               uint32_t max_seg_id, const int *has_null, const int64_t *null_val,
                               const uint32_t *stats_sel, const int *nstats_per_band, int64_t missing,
                               const uint32_t *d_hist, int keep_unheld, void *d_cols, void **d_pair_seg_out,
                               void **d_pair_val_out, int64_t *pair_row_bytes_out, int64_t *n_pairs_out,
                               int64_t *n_straddlers_out);
int shp_dstats_merge_bands_dev(shp_ctx *ctx, const uint32_t *d_pair_seg, const void *d_pair_val, int64_t slot,
                               int64_t slot_row_bytes, int world, const uint32_t *counts, int dtype, int nbands,
                               int nplanes, const int *plane_of_band, uint32_t max_seg_id, const int *has_null,
                               const int64_t *null_val, const uint32_t *stats_sel, const int *nstats_per_band,
                               int64_t missing, uint32_t id_lo, uint32_t id_hi, void *d_cols, int64_t *n_merged_out,
                               int64_t *n_ids_out);

/* ---- subset --------------------------------------------------------------------------
 * replaces the tile loop of subset.subsetImage (subset.py:124-166) and its njit kernel
 * processSubsetTile (subset.py:366-425): the window (tlx, tly, xs, ys) of a label raster is
 * recoded to ids 1..n in first-seen order, the window being visited in tiles of tile_size x
 * tile_size (the reference uses tiling.TILESIZE = 1024), tile rows outer, raster order inside a
 * tile; pixels that are null (0) or masked out (mask byte == 0; mask may be NULL) become 0.
 * out: xs*ys labels; orig_out[new id] = old id (row 0 = 0) is the reference's recodeDict
 * inverted -- the row gather that copySubsettedSegmentsToNew (:232-266) applies to every RAT
 * column and the optional origSegIdColName column (:207-226); hist_out[new id] = pixel count
 * (histogramDict).  orig_out / hist_out hold cap rows (n + 1 are written); *n_new_out = n.
 * Error "Requested subset is not within input image" as subset.py:86-88; max_seg_id = 0xffffffff is
 * refused ("max_seg_id too large"): max_seg_id + 1 ids are counted in 32 bits. */
int shp_subset_recode(shp_ctx *ctx, const uint32_t *seg, int64_t img_rows, int64_t img_cols,
                      int64_t tlx, int64_t tly, int64_t xs, int64_t ys, const uint8_t *mask,
                      int tile_size, uint32_t max_seg_id, uint32_t *out, uint32_t *orig_out,
                      uint32_t *hist_out, int64_t cap, uint32_t *n_new_out);
/* same with the label raster, the mask and the output window in device memory */
int shp_subset_recode_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t img_rows, int64_t img_cols,
                          int64_t tlx, int64_t tly, int64_t xs, int64_t ys, const uint8_t *d_mask,
                          int tile_size, uint32_t max_seg_id, uint32_t *d_out, uint32_t *orig_out,
                          uint32_t *hist_out, int64_t cap, uint32_t *n_new_out);

/* The subset recode split by rows over the ranks (the data path of distributed.deviceSubset /
 * subsetImageDistributed).  A rank holds rows [row0, row0 + nrows) of the label raster in place (d_seg, row
 * pitch ncols, fewer than 2^32 pixels), hence the window rows [a, b) = [max(0, row0 - tly), min(ys, row0 + nrows
 * - tly)) (empty when b <= a); d_mask (optional) holds (b - a) * xs bytes, the mask rows of those window rows.
 * Keys are positions in the WHOLE window's visiting order (tile_size tiles), so they compare across ranks.
 *  shp_dsubset_local_dev: first-seen key of every id in the held rows; the ids present are packed as
 *    *n_pairs_out keys followed by as many ids (uint32) at *d_pairs_out in the context's workspace, valid until
 *    its next call.  *bad_out = 1 when a held pixel has an id above max_seg_id (such ids are left out; the
 *    caller decides, after a collective, whether to raise).
 *  shp_dsubset_merge_dev: after the all-gather of the pairs -- `world` slots of 2 * slot words, slot r holds
 *    counts[r] keys then counts[r] ids -- the minimum key of every id gives its new id, the same on every rank.
 *    The held window rows are recoded into d_out ((b - a) * xs uint32) and their new ids counted into d_hist
 *    (cap uint32, device, zeroed first); orig_out (host, cap rows) = old id per new id (row 0 = 0);
 *    *n_new_out = m.  Summing d_hist over the ranks gives shp_subset_recode's hist_out. */
int shp_dsubset_local_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int64_t row0,
                          uint32_t max_seg_id, int64_t tlx, int64_t tly, int64_t xs, int64_t ys, int tile_size,
                          const uint8_t *d_mask, void **d_pairs_out, int64_t *n_pairs_out, int *bad_out);
int shp_dsubset_merge_dev(shp_ctx *ctx, const void *d_pairs, int64_t slot, int world, const uint32_t *counts,
                          const uint32_t *d_seg, int64_t nrows, int64_t ncols, int64_t row0, uint32_t max_seg_id,
                          int64_t tlx, int64_t tly, int64_t xs, int64_t ys, int tile_size, const uint8_t *d_mask,
                          uint32_t *d_out, uint32_t *d_hist, uint32_t *orig_out, int64_t cap, uint32_t *n_new_out);

/* ---- spatial statistics --------------------------------------------------------------
 * replaces the tile loop of tilingstats.calcPerSegmentSpatialStatsTiled (tilingstats.py:1262-1390)
 * for the reference's built-in user functions, func = 0 userFuncMeanCoord (:1098-1142; params =
 * the six GDAL geotransform numbers; float columns 0, 1 = mean easting, northing), 1
 * userFuncNumEdgePixels (:1146-1216; params[0] = fourConnected; int column 0), 2 userFuncVariogram
 * (:1037-1094; params[0] = maxDist in 1..255; float columns 0..maxDist-1).  Only a segment's pixels
 * whose band value differs from null_val count (accumulateSegSpatial :1686-1699; the reference
 * insists on a nodata value, :1325-1333).  nint / nflt = number of integer / real columns of
 * colNamesAndTypes; intcols_out: nint x (max_seg_id+1) int64, floatcols_out: nflt x
 * (max_seg_id+1) float32; entries the function does not set, and segments without a valid pixel,
 * hold `missing`; row 0 is zero.  A user-defined function (tilingstats.spatialUserFunc) runs on the host
 * over the point lists of shp_segpoints_build / shp_segpoints_emit (tilingstats.calcPerSegmentSpatialStats). */
int shp_spatialstats(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t nrows,
                     int64_t ncols, uint32_t max_seg_id, int64_t null_val, int func,
                     const double *params, int64_t missing, int nint, int nflt,
                     int64_t *intcols_out, float *floatcols_out);
/* same with the label raster and the band already in device memory */
int shp_spatialstats_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype,
                         int64_t nrows, int64_t ncols, uint32_t max_seg_id, int64_t null_val,
                         int func, const double *params, int64_t missing, int nint, int nflt,
                         int64_t *intcols_out, float *floatcols_out);

/* Per-segment point lists for user-defined spatial functions: replace accumulateSegSpatial
 * (tilingstats.py:1652-1699) and the segment-completion bookkeeping of calcPerSegmentSpatialStatsTiled
 * (:1262-1390, :1703-1741).  A point is a pixel whose label is in 1..max_seg_id and whose band value differs
 * from null_val; a segment's points come in the reference's visit order: tile_size x tile_size tiles in
 * row-major order, pixels row-major inside a tile (the result is a stable sort of all points by id in that order).
 *  shp_segpoints_count: counts_out (max_seg_id + 1 uint32) = points per id (0 for id 0).
 *  shp_segpoints_build: sorts the points of the whole raster by id; *npts_out = their number.  The result stays
 *    in the context's workspace for shp_segpoints_emit, which must be the context's next calls; the _dev variant
 *    reads the band from d_band then, so it must stay in place.
 *  shp_segpoints_emit: the points of ids [id_lo, id_hi) (id_hi <= max_seg_id + 1): offs_out (id_hi - id_lo + 1
 *    int64) = where each id's points start, relative to the first, and pts_out = *npts_out records of 16 bytes,
 *    {uint32 x (column); uint32 y (row); int64 val} (the reference's SegPoint, :1225-1240, with val as
 *    numbaTypeForImageType).  More points than cap: SHP_ERR_ARG, *npts_out says how many.
 * The raster must hold fewer than 2^32 pixels. */
int shp_segpoints_count(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t nrows,
                        int64_t ncols, uint32_t max_seg_id, int64_t null_val, uint32_t *counts_out);
int shp_segpoints_count_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                            int64_t ncols, uint32_t max_seg_id, int64_t null_val, uint32_t *counts_out);
int shp_segpoints_build(shp_ctx *ctx, const uint32_t *seg, const void *band, int dtype, int64_t nrows,
                        int64_t ncols, uint32_t max_seg_id, int64_t null_val, int64_t tile_size, int64_t *npts_out);
int shp_segpoints_build_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                            int64_t ncols, uint32_t max_seg_id, int64_t null_val, int64_t tile_size,
                            int64_t *npts_out);
int shp_segpoints_emit(shp_ctx *ctx, uint32_t id_lo, uint32_t id_hi, int64_t *offs_out, void *pts_out, int64_t cap,
                       int64_t *npts_out);

/* Per-segment point lists of row shards: the data path of distributed.deviceSpatialStats with a user function
 * (calcPerSegmentSpatialStatsDistributed).  Replace, per rank, what shp_segpoints_build / _emit replace for one
 * raster (accumulateSegSpatial, tilingstats.py:1652-1699, and the completion bookkeeping of
 * calcPerSegmentSpatialStatsTiled, :1262-1390 / :1703-1741): every segment's points in the WHOLE raster's visit
 * order (tile_size x tile_size tiles of the img_rows x ncols raster), although its rows lie on several ranks.
 *  shp_dsegpoints_build_dev: this rank's rows [row0, row0 + nrows) in place (d_seg, d_band: nrows x ncols, fewer
 *    than 2^32 pixels; the raster as a whole may hold more, but one of its tile rows -- min(tile_size, img_rows)
 *    rows -- may reach 2^32 pixels only when it is the only one: SHP_ERR_ARG otherwise, on every rank alike).
 *    Sorts the rows' points by id in visit order and judges
 *    every id against the GLOBAL label histogram d_hist: complete here (local label count == d_hist), straddler
 *    (fewer) or absent.  lh_out / pts_out (max_seg_id + 1 uint32 each, host) = labelled pixels / points per id
 *    here.  The straddlers' points are packed as *n_rec_out records of 24 bytes, {uint64 global visit index;
 *    uint32 id; uint32 x; uint32 y; uint32 value bits}, in (id, visit index) order, at *d_rec_out in the context's
 *    workspace (valid until its next call).
 *  shp_dsegpoints_merge_dev: must be the context's next call.  After the all-gather of the records (`world` slots of
 *    `slot`, counts[r] valid in slot r) the records of ids in [id_lo, id_hi) (this rank's share) are sorted stably
 *    by (id, visit index); merged_out (id_hi - id_lo uint32, host) = records per id of the share.
 *  shp_dsegpoints_emit: as shp_segpoints_emit, for the ids this rank answers for: ids complete here (their points
 *    from the local rows) and straddlers of its share (from the merged records); every other id has no points.  The
 *    context's next calls must be its emissions. */
int shp_dsegpoints_build_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                             int64_t ncols, int64_t row0, int64_t img_rows, uint32_t max_seg_id, int64_t null_val,
                             int64_t tile_size, const uint32_t *d_hist, uint32_t *lh_out, uint32_t *pts_out,
                             void **d_rec_out, int64_t *n_rec_out);
int shp_dsegpoints_merge_dev(shp_ctx *ctx, const void *d_recs, int64_t slot, int world, const uint32_t *counts,
                             uint32_t id_lo, uint32_t id_hi, uint32_t *merged_out, int64_t *n_merged_out);
int shp_dsegpoints_emit(shp_ctx *ctx, uint32_t id_lo, uint32_t id_hi, int64_t *offs_out, void *pts_out, int64_t cap,
                        int64_t *npts_out);

/* The spatial statistics split by rows over the ranks (the data path of
 * distributed.calcPerSegmentSpatialStatsDistributed), modelled on shp_dstats_local_bands_dev / _merge_bands_dev.
 *  shp_dspatial_local_dev: this rank's rows [row0, row0 + nrows) of an img_rows-row raster in place (d_seg,
 *    d_band: nrows x ncols), with rows_up halo rows just above them (d_seg_up / d_band_up) and rows_dn just
 *    below (d_seg_dn / d_band_dn) -- other ranks' rows; the halo must reach the needed distance or the
 *    image's border (edges: 1 row each way, variogram: maxDist rows below, mean coordinates: none).  The own
 *    pixels are accumulated, then every id is judged against the GLOBAL label histogram d_hist as in
 *    shp_dstats_local_bands_dev: rows of segments complete here are finished, ids nobody holds get their "missing"
 *    row where keep_unheld != 0, all other rows of d_cols are zero.  The straddlers' partial sums are packed
 *    as records of *rec_words_out uint64 words -- (id, cnt, sumx, sumy), (id, cnt, edges) or (id, cnt,
 *    vcnt[maxDist], vsum[maxDist]) -- *n_rec_out of them at *d_rec_out in the context's workspace, valid until
 *    its next call.  checks_out[3]: ids with more pixels here than d_hist says, labelled pixels here, pixels
 *    of d_hist (a wrong histogram shows in them; the caller decides, after a collective, whether to raise).
 *    func, params, null_val, missing, nint, nflt: as shp_spatialstats.  Each of the own rows and the two
 *    halos must hold fewer than 2^32 pixels; the raster as a whole may hold more.
 *  shp_dspatial_merge_dev: after the all-gather of the records -- `world` slots of `slot` records, counts[r]
 *    valid in slot r -- the records with id_lo <= id < id_hi are summed, those ids (*n_ids_out of them)
 *    finished and their rows written into d_cols.
 *  Summing d_cols over the ranks as int64 words gives the columns shp_spatialstats returns, bit for bit. */
int shp_dspatial_local_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                           int64_t ncols, const uint32_t *d_seg_up, const void *d_band_up, int64_t rows_up,
                           const uint32_t *d_seg_dn, const void *d_band_dn, int64_t rows_dn, int64_t row0,
                           int64_t img_rows, uint32_t max_seg_id, int64_t null_val, int func, const double *params,
                           int64_t missing, int nint, int nflt, const uint32_t *d_hist, int keep_unheld,
                           void *d_cols, void **d_rec_out, int64_t *n_rec_out, int64_t *rec_words_out,
                           int64_t *checks_out);
int shp_dspatial_merge_dev(shp_ctx *ctx, const void *d_recs, int64_t slot, int world, const uint32_t *counts,
                           uint32_t max_seg_id, int func, const double *params, int64_t missing, int nint, int nflt,
                           uint32_t id_lo, uint32_t id_hi, void *d_cols, int64_t *n_ids_out);
/* The variogram (func 2) adds squares as integers; a (segment, bin) pair whose float64 sum in the reference's
 * order may differ from that (a square or the total at 2^53 or beyond) is flagged and recomputed.
 *  shp_spatial_vario_redo_count: the pairs the last shp_spatialstats(_dev) call recomputed.
 *  shp_dspatial_vario_pairs: the flagged pairs (s * maxd + bin, ascending) of the last local or merge call
 *    (*n_out; copied into out when cap >= *n_out).
 *  shp_dspatial_vario_redo_dev: the reference's sums of the pairs (the union over the ranks, ascending) over the
 *    own rows and the rows_dn halo rows below them, continuing from sum / cnt (host arrays, in and out): the
 *    ranks run it one after the other from the top of the image.
 *  shp_dspatial_vario_store_dev: before the column block is summed over the ranks, one rank stores the pairs'
 *    entries (write = 1: (float)sqrt(sum / cnt)) and every other rank zeroes them (write = 0). */
int shp_spatial_vario_redo_count(shp_ctx *ctx, int64_t *n_out);
int shp_dspatial_vario_pairs(shp_ctx *ctx, uint64_t *out, int64_t cap, int64_t *n_out);
int shp_dspatial_vario_redo_dev(shp_ctx *ctx, const uint32_t *d_seg, const void *d_band, int dtype, int64_t nrows,
                                int64_t ncols, const uint32_t *d_seg_dn, const void *d_band_dn, int64_t rows_dn,
                                uint32_t max_seg_id, int64_t null_val, int maxd, const uint64_t *pairs, int64_t np,
                                double *sum, uint32_t *cnt);
int shp_dspatial_vario_store_dev(shp_ctx *ctx, const uint64_t *pairs, int64_t np, const double *sum,
                                 const uint32_t *cnt, int maxd, uint32_t max_seg_id, int nint, int nflt,
                                 void *d_cols, int write);

/* ---- colour tables and their rendering ---------------------------------------------------------------
 * utils.writeColorTableFromRatColumns (utils.py:162-230) stretches three RAT columns to 0..255 between their
 * 5th and 95th percentiles with numpy (:216-221), a desktop viewer then paints the labels through the table.
 *  shp_colour_stretch: one column (host, n rows; ctype 0 float64, 1 float32, 2 int64 -- the last two are
 *    converted to float64 on the device, int64 exactly: a magnitude of 2^53 or more is an error, as is a NaN or
 *    an infinity in any column) -> out (host, n bytes) = (255 * ((col - lo) / (hi - lo)).clip(0, 1)).astype(uint8)
 *    with lo, hi = numpy.percentile(col, 5), numpy.percentile(col, 95) (method 'linear'), byte for byte;
 *    stretch_out[2] = (lo, hi).  hi == lo gives 255 where col > lo and 0 elsewhere (numpy's result on x86-64).
 *    The four order statistics come from a radix selection on the device (csrc/colour.h), not from a sort.
 *    dev_ms_out (may be NULL): device time between the column's upload and the bytes' download.
 *  shp_colour_pack: four byte columns (host, n rows each) -> d_table (device, n words): row i =
 *    red[i] | green[i] << 8 | blue[i] << 16 | alpha[i] << 24, the (rows, cols, 4) uint8 pixel of label i.
 *  shp_colour_lookup_dev: d_out[p] = d_table[d_seg[p]] for npix labels in device memory.  A label that is not
 *    below nrows is an error whose message names the smallest such label; nothing is read outside the table. */
int shp_colour_stretch(shp_ctx *ctx, const void *col, int ctype, int64_t n, uint8_t *out, double *stretch_out,
                       double *dev_ms_out);
int shp_colour_pack(shp_ctx *ctx, const uint8_t *red, const uint8_t *green, const uint8_t *blue, const uint8_t *alpha,
                    int64_t n, uint32_t *d_table);
int shp_colour_lookup_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t npix, const uint32_t *d_table, int64_t nrows,
                          uint32_t *d_out);

/* The same on the row-sharded output of several ranks (distributed.writeColorTableFromRatColumnsDistributed,
 * renderColourTableDistributed).  They replace what a user of the multi-rank driver had to do in one process on one
 * GPU: stretch the whole columns with shp_colour_stretch and push the written label file through
 * shp_colour_lookup_dev.
 *  shp_dcolour_begin / _hist / _pick / _finish / shp_dcolour_stretch_dev: shp_colour_stretch of a column of n rows of
 *    which this rank holds m (host, may be 0), in steps the caller puts a collective between.  begin uploads and
 *    widens the share and sets the four ranks of the WHOLE column; *d_block_out is the device block the ranks sum
 *    (as int64 words) between _hist(pass) and _pick(pass), pass = 0..7: 512 words of digit histograms (two uint32
 *    counts per word; n < 2^32, so no carry) and, in pass 0 only, a 513th whose lanes count the ranks whose share
 *    holds a NaN or an infinity / an integer of magnitude 2^53 or more.  After the sum every rank picks the same
 *    digits.  finish: stretch_out[2] = (lo, hi), the whole column's percentiles as shp_colour_stretch gives them;
 *    *bad_out = bit 0 a non-finite value, bit 1 a wide integer, in ANY rank's share (then nothing can be
 *    stretched).  stretch_dev: the share's m bytes -> d_out (device, 4-byte aligned); dev_ms_out (may be NULL): the
 *    device time of the column's steps.  The share lives in the context's workspace: no other call of the context
 *    that uses the workspace may come between the steps (shp_dev_* transfers may).
 *  shp_colour_pack_dev: shp_colour_pack from four byte columns that are in device memory already (each 4-byte
 *    aligned): the ranks' gathered bytes become the table without a host round trip.
 *  shp_colour_render_rows_dev: shp_colour_lookup_dev plus the download, pipelined: npix labels in device memory ->
 *    h_dst (npix words of pinned memory, shp_host_alloc) in blocks of block_pixels; the download of a block runs on
 *    the context's side stream while the next block is looked up into a second device buffer.  bad_out[2] =
 *    (1 when a label has no row in the table, the smallest such label) -- reported, not raised, so that the ranks
 *    can agree on one message; ms_out[3] = summed device time of the lookups, of the downloads, wall time of the
 *    call (the overlap pays when the third is below the sum of the first two).
 *  shp_colour_overview_rects_dev: shp_overview_rects_dev with the table lookup fused in -- the rectangle table and
 *    its checks are the label layers', d_packed receives (R, G, B, A) words; bad_out as above. */
int shp_dcolour_begin(shp_ctx *ctx, const void *col, int ctype, int64_t m, int64_t n, void **d_block_out);
int shp_dcolour_hist(shp_ctx *ctx, int pass);
int shp_dcolour_pick(shp_ctx *ctx, int pass);
int shp_dcolour_finish(shp_ctx *ctx, double *stretch_out, int *bad_out);
int shp_dcolour_stretch_dev(shp_ctx *ctx, uint8_t *d_out, double *dev_ms_out);
int shp_colour_pack_dev(shp_ctx *ctx, const uint8_t *d_red, const uint8_t *d_green, const uint8_t *d_blue,
                        const uint8_t *d_alpha, int64_t n, uint32_t *d_table);
int shp_colour_render_rows_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t npix, int64_t block_pixels,
                               const uint32_t *d_table, int64_t nrows, uint32_t *h_dst, uint32_t *bad_out,
                               double *ms_out);
int shp_colour_overview_rects_dev(shp_ctx *ctx, const uint32_t *d_raster, int64_t npix, const int64_t *rects,
                                  int nrects, const uint32_t *d_table, int64_t nrows, uint32_t *d_packed,
                                  int64_t npacked, uint32_t *bad_out);

/* ---- segment neighbours and border lengths (neighbours.findSegmentNeighbours; csrc/neighbours.h) ------------
 * Which segments of a uint32 label raster touch which, and along how many pixel pairs.  Two pixels are adjacent when
 * one is the E or S neighbour of the other (four_connected == 0: SE and SW as well); every adjacent pair with labels
 * a != b, both non-zero, adds 1 to the border length of (a, b) and of (b, a).  The result is a CSR table over the ids
 * 0 .. max_seg_id: offsets (max_seg_id + 2 int64; offsets[0] == offsets[1] == 0, label 0 is no segment), neighbour ids
 * (uint32, ascending within a row) and border lengths (int64).  All of it is integer work: the table does not depend
 * on how the raster is cut into row blocks.  The state lives in buffers of its own, so other calls of the context
 * (shp_dev_* transfers, say) may come between the steps.
 *  shp_nbr_begin: starts a table.  max_seg_id >= 0: the rows the table gets; -1: the largest label met.
 *  shp_nbr_accumulate_dev: a block of nrows rows of ncols labels in device memory (4-byte aligned).  has_next_row != 0:
 *    the block is not the raster's last and one more row follows it in memory (nrows + 1 rows are readable); only
 *    pairs whose UPPER pixel lies in the block count, so a pair across two blocks counts once.  Blocks may come in
 *    any order.  Workgroups count the pairs of 32 x 64 patches in LDS and append their distinct pairs to a record
 *    buffer that grows between blocks (device memory is bounded by records, not by pixel pairs).
 *  shp_nbr_finish: sorts and reduces the records and builds the table on the device.  *max_seg_id_out: the table's
 *    last row; *n_entries_out: entries of the neighbour and length arrays; *bad_label_out: 0, or the largest label
 *    above the max_seg_id given to begin -- then there is no table (n_entries_out = 0) and download fails.
 *    counters_out (may be NULL) [3]: differing pixel pairs met, records handed to the sort, row blocks that did not
 *    fit the record buffer and ran a second time since shp_nbr_begin; dev_ms_out (may be NULL): device time of the
 *    accumulate kernels and of this call.
 *  shp_nbr_download: the three arrays to host memory (max_seg_id + 2, n_entries, n_entries elements). */
int shp_nbr_begin(shp_ctx *ctx, int64_t max_seg_id, int four_connected);
int shp_nbr_accumulate_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int has_next_row);
int shp_nbr_finish(shp_ctx *ctx, uint32_t *max_seg_id_out, int64_t *n_entries_out, uint32_t *bad_label_out,
                   int64_t *counters_out, double *dev_ms_out);
int shp_nbr_download(shp_ctx *ctx, int64_t *offsets, uint32_t *neighbours, int64_t *border_lengths);

/* ---- per-segment shape attributes of a label raster (shapes.calcSegmentShapes) --------------------------
 * Per id 1 .. max_seg_id, with (r, c) a pixel's coordinates from the caller's origin: area; the sums of r, c, r^2, c^2
 * and r c modulo 2^64; the minimum and maximum of r and of c; perimeter (the N, S, W, E sides of the id's pixels whose
 * other side is another label, label 0 or outside the raster), outer border (those whose other side is label 0 or
 * outside) and edge pixels (pixels with at least one such side).  Integers throughout: the result does not depend on
 * the row blocks.  The table lives in buffers of the context's own (88 bytes per id) that are reused between calls;
 * the neighbour table and the group lists of the context are not touched.
 *  shp_shape_label_max_dev: *max_label_out = the largest of npix labels in device memory (4-byte aligned), 0 without
 *    pixels; dev_ms_out (may be NULL): device time of the kernel.
 *  shp_shape_begin: an empty table of the rows 0 .. max_seg_id; pixel (0, 0) of the raster has the coordinates
 *    (row0, col0), both 0 .. 2^32 - 1.
 *  shp_shape_accumulate_dev: the next block of nrows rows of ncols labels, top to bottom.  d_seg is the first row
 *    handed over: with has_above != 0 that is the raster's row above the block, with has_below != 0 the row below the
 *    block follows it in memory (has_above + nrows + has_below rows are readable).  Sides of the block's own pixels
 *    count, the two extra rows are only looked at.  Coordinates of 2^32 and more are SHP_ERR_ARG.
 *  shp_shape_finish: the extents of ids without pixels become 0.  *bad_label_out: 0, or the largest label above
 *    max_seg_id -- such labels were never looked up, there is no result and download fails.  dev_ms_out (may be
 *    NULL): device time of the kernels since shp_shape_begin.
 *  shp_shape_download: max_seg_id + 1 rows of 11 uint64 to host memory: area, sum r, sum c, sum r^2, sum c^2, sum r c,
 *    perimeter, outer border, edge pixels, rowMin | rowMax << 32, colMin | colMax << 32.
 * Out of order the calls fail with SHP_ERR_STATE ("shp_shape_begin must come first", "shp_shape_finish must come
 * first"). */
int shp_shape_label_max_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t npix, uint32_t *max_label_out, double *dev_ms_out);
int shp_shape_begin(shp_ctx *ctx, int64_t max_seg_id, int64_t row0, int64_t col0);
int shp_shape_accumulate_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int has_above,
                             int has_below);
int shp_shape_finish(shp_ctx *ctx, uint32_t *max_seg_id_out, uint32_t *bad_label_out, double *dev_ms_out);
int shp_shape_download(shp_ctx *ctx, uint64_t *rows);

/* ---- the shape table of a raster sharded by rows over the ranks (dist_shapes.deviceShapes) ---------------
 * A rank begins a table of all ids with row0 = its first image row (shp_shape_begin), accumulates its rows, hands the
 * rows of the segments that straddle a cut to the ranks that own their ids and ends with a table in which every id's
 * row is non-zero on at most one rank: an integer all-reduce of the (max_seg_id + 1) x 11 words then completes it.
 *  shp_shape_accumulate_halo_dev: shp_shape_accumulate_dev with the two extra rows wherever they lie: d_seg is the
 *    block's own first row, d_above / d_below the raster's row before / after the block (ncols labels each, in device
 *    memory, only looked at), NULL where the raster ends.  A rank's gigabytes of labels need not be copied to stand
 *    between their halo rows.
 *  shp_dshape_local_dev: after the accumulation.  d_hist: the whole raster's pixel count per id, n_hist = max_seg_id
 *    + 1 uint32 in device memory.  *max_label_out: 0, or the largest label above max_seg_id in this rank's rows --
 *    then nothing else is done and the table is gone.  Otherwise, with l an id's area here: l == hist[id] keeps the
 *    row; 0 < l < hist[id] packs it as a record of 96 bytes (the id as uint64, then the row's 11 words) and empties
 *    it; counts_out[0] = such records, at *d_records_out in device memory until the context's next shape call
 *    (NULL without records); counts_out[1] = ids with l > hist[id] (the histogram is not these labels').
 *  shp_dshape_merge_dev: d_all holds `world` blocks of `slot` records (16-byte aligned), the first counts[r] of block
 *    r valid (slot 0: no rank sent any, d_all is not read).  Records with an id in [id_lo, id_hi) are folded into
 *    that id's row (sums and counts add, extents combine by min / max); then the extents of ids without pixels
 *    become 0 and the table is finished (shp_shape_download).  counts_out[0] = records folded, [1] = distinct ids
 *    folded, [2] = ids of the share whose area is neither 0 nor d_hist's.  *d_table_out: the table in device memory,
 *    for the all-reduce; it is what shp_shape_download copies.
 * dev_ms_out (may be NULL): device time of the kernels since shp_shape_begin.  Out of order: SHP_ERR_STATE
 * ("shp_shape_begin must come first", "shp_dshape_local_dev must come first"). */
int shp_shape_accumulate_halo_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, const uint32_t *d_above,
                                  const uint32_t *d_below);
int shp_dshape_local_dev(shp_ctx *ctx, const uint32_t *d_hist, int64_t n_hist, uint32_t *max_label_out, int64_t *counts_out,
                         void **d_records_out, double *dev_ms_out);
int shp_dshape_merge_dev(shp_ctx *ctx, const void *d_all, int64_t slot, int world, const uint32_t *counts, const uint32_t *d_hist,
                         int64_t n_hist, int64_t id_lo, int64_t id_hi, int64_t *counts_out, void **d_table_out,
                         double *dev_ms_out);

/* ---- segment outlines as vertex rings, traced from the label raster (outlines.traceSegmentOutlines) ----
 * Pixel (y, x) covers [y, y + 1] x [x, x + 1]; corners are (row, col) pairs; label 0 is no segment.  A side of a pixel
 * of id A is an edge of A when the label across it is not A (another id, label 0, outside the raster: the perimeter of
 * the shape table).  Edges are directed with A's pixel on the right of travel (N eastwards, E southwards, S westwards,
 * W northwards) and ordered by the key (y, x, side) with N, E, S, W = 0 .. 3.  At its end corner an edge turns right
 * when the pixel right-ahead is not A, goes straight when it is and the pixel left-ahead is not, turns left when both
 * are; where only the pixel left-ahead is A (A touches itself diagonally) it turns right for four-connected segments
 * and left for eight-connected ones.  The cycles of that successor map are the rings.  A ring's vertices are the start
 * corners of its edges whose predecessor has another side, in cycle order from the one of the smallest key; rings are
 * ordered by (id, that key); ringArea2 = sum of c_i r_(i+1) - c_(i+1) r_i is positive for an outer ring, negative for a
 * hole, twice the pixels enclosed.  Integers throughout: the result does not depend on the launches or on the number
 * of doubling rounds.  The whole raster is in device memory (4-byte aligned, at most 2^32 - 8192 pixels and as many
 * edges); the work arrays live in buffers of the context's own that are reused between calls, and the neighbour
 * table, the group lists and the shape table of the context are not touched.
 *  shp_outline_need: *need_out = the bytes those buffers still have to grow by, *free_out = the device's free bytes.
 *    edges < 0: for shp_outline_edges_dev on npix pixels (5 bytes a pixel); edges >= 0: for shp_outline_trace on that
 *    many edges (37 bytes an edge, and room for as many vertices at 16 bytes and a quarter as many rings at 52).
 *  shp_outline_edges_dev: finds the edges of nrows x ncols labels and gives every one its index.  *edges_out: their
 *    number; *bad_label_out: 0, or the largest label above max_seg_id.  With such a label, or with more than 2^32 -
 *    8192 edges, there is nothing to trace and shp_outline_trace fails.  Otherwise d_seg must stay in place until
 *    shp_outline_trace returns.
 *  shp_outline_trace: successors, then pointer-doubling rounds launched one by one from the host until a round changes
 *    no window minimum (at most ceil(log2(edges)) + 2: beyond that the call fails with SHP_ERR_STATE and does not
 *    loop), then rings, vertices (row0 and col0, both 0 .. 2^32 - 1, added) and areas.  counts_out[3]: rings, vertices,
 *    rounds run.  steps_ms_out (may be NULL) [4]: device time of shp_outline_edges_dev's kernels, of the successors, of
 *    the rounds, of the rest.
 *  shp_outline_download: to host memory, all int64: ring_offsets (max_seg_id + 2: the rings of id i are
 *    ring_offsets[i] .. ring_offsets[i + 1]), vertex_offsets (rings + 1), vertices (vertices x 2, row then col),
 *    ring_area2 (rings); the last two may be NULL without rings.
 * Out of order the calls fail with SHP_ERR_STATE ("shp_outline_edges_dev must come first", "shp_outline_trace must come
 * first"). */
int shp_outline_need(shp_ctx *ctx, int64_t npix, int64_t edges, int64_t *need_out, int64_t *free_out);
int shp_outline_edges_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int64_t max_seg_id,
                          int four_connected, int64_t *edges_out, uint32_t *bad_label_out);
int shp_outline_trace(shp_ctx *ctx, int64_t row0, int64_t col0, int64_t *counts_out, double *steps_ms_out);
int shp_outline_download(shp_ctx *ctx, int64_t *ring_offsets, int64_t *vertex_offsets, int64_t *vertices, int64_t *ring_area2);
/* shp_outline_serial: *calls_out = the shp_outline_edges_dev calls this context has had (every one replaces the
 * outlines it holds, whatever becomes of it); *serial_out = the value of that count the traced outlines in the
 * context's buffers belong to, 0 when there are none.  A caller that counts its own calls can so tell, without a call
 * of its own at trace time, whether the outlines it once traced are still the resident ones.  No device work. */
int shp_outline_serial(shp_ctx *ctx, uint64_t *calls_out, uint64_t *serial_out);

/* ---- per-segment depth: the exact Euclidean distance transform of the labels (depths.calcSegmentDepths) ----------
 * depth2 of a pixel of label L != 0 is the smallest squared distance (between pixel centres) to a position outside the
 * raster or of another label (label 0 included); 0 where the label is 0.  The labels are whole in device memory.
 *  shp_depth_need: *need_out = the bytes the buffers still have to grow by, *free_out = the device's free bytes.
 *    marked < 0: for shp_depth_transform_dev on nrows x ncols pixels and the table of the ids 0 .. max_seg_id (6 bytes a
 *    pixel, 20 per column and band of 32 rows, 12 per 64 columns of a row, 88 an id, 16 per pixel / 65 -- per pixel with
 *    all_runs != 0);
 *    marked >= 0: for shp_depth_envelope on that many scratch positions (8 bytes each).
 *  shp_depth_transform_dev: the column step, the window of the row step and the list of the row runs the envelope has
 *    to solve: those that hold a pixel the window deferred, or, with all_runs != 0, every run (the window is then
 *    skipped).  counts_out[0] = pixels deferred, [1] = runs marked, [2] = scratch positions they take (their pixels
 *    and two a run).  d_seg must stay in place until shp_depth_reduce returns.
 *  shp_depth_envelope: solves the marked runs by the lower envelope of their parabolas.
 *  shp_depth_reduce: the table of the ids 0 .. max_seg_id with n_cores <= 8 thresholds core_q (host memory): per id
 *    the pixels, the sum of depth2, the largest (depth2 << 32 | 0xFFFFFFFF - linear pixel index) and per threshold the
 *    pixels with depth2 > core_q[k].  *bad_label_out: 0, or the largest label above max_seg_id (then there is no
 *    result and download fails).  steps_ms_out (may be NULL): 4 doubles, device time of the column step, the window,
 *    the runs and their envelope, the reduction.
 *  shp_depth_download: max_seg_id + 1 rows of 11 uint64 to host memory; depth2 (may be NULL): nrows x ncols uint32.
 * Out of order the calls fail with SHP_ERR_STATE ("shp_depth_transform_dev must come first", ...). */
int shp_depth_need(shp_ctx *ctx, int64_t nrows, int64_t ncols, int64_t max_seg_id, int all_runs, int64_t marked, int64_t *need_out,
                   int64_t *free_out);
int shp_depth_transform_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, int all_runs, int64_t *counts_out);
int shp_depth_envelope(shp_ctx *ctx);
int shp_depth_reduce(shp_ctx *ctx, int64_t max_seg_id, int n_cores, const uint32_t *core_q, uint32_t *bad_label_out,
                     double *steps_ms_out);
int shp_depth_download(shp_ctx *ctx, uint64_t *rows, uint32_t *depth2);

/* The junction switch of the trace.  Labels outside the raster read as 0; of the four pixels a b / c d round a corner the
 * pairs (a, b), (b, d), (c, d), (a, c) that differ number its degree, and a corner of degree >= 3 is a junction (three or
 * more segments meet, or two at a saddle), whatever four_connected.
 *  shp_outline_junctions: between shp_outline_edges_dev and shp_outline_trace (SHP_ERR_STATE elsewhere); on != 0: every
 *    edge whose start corner is a junction is a vertex edge like a turn edge, so a ring that runs straight through such a
 *    corner gets a collinear vertex there; a ring then starts at its vertex edge of the smallest key.  Ring order, areas
 *    and the rings' number are the plain trace's.  Every shp_outline_edges_dev clears the switch; asked after it and
 *    before shp_outline_need, that call's bytes include the flags (a byte a vertex).
 *  shp_outline_download_junction: junction[vertices], 1 where the vertex's corner is a junction; SHP_ERR_STATE unless the
 *    outlines were traced with the switch on. */
int shp_outline_junctions(shp_ctx *ctx, int on);
int shp_outline_download_junction(shp_ctx *ctx, uint8_t *junction);

/* ---- Douglas-Peucker simplification of the outline rings, shared borders staying shared (outlines.simplifySegmentOutlines) ----
 * Input: rings as shp_outline_download fills them and a junction flag per vertex.  A ring's anchors are its flagged
 * vertices; a ring without any takes its vertex of the smallest (row, col) (the first of equal ones).  An arc runs from
 * one anchor to the next in ring order, cyclically, both included (closed with one anchor).  Both ends of an arc are kept.
 * Between kept a and b: m(q) = |(b - a) x (q - a)| if a != b, |q - a|^2 if a = b; the candidate is the point of the largest
 * m, ties to the smallest (row, col), then to the first in arc order; it exceeds when m^2 65536 > tolerance2q |b - a|^2
 * (a != b) or m 65536 > tolerance2q (a = b), in 128-bit integers; if it exceeds it is kept and both halves are treated
 * the same way.  Every quantity is symmetric in the direction of travel, so the two rings along a border keep the same
 * vertices of it.  A ring's vertices are its kept source vertices in source order; it is dropped when fewer than three
 * remain or when its new ring_area2 is 0 or differs in sign from its source ring's; the others keep their order.
 * Integers throughout: the result does not depend on the launches, the atomics' order, the path or the rounds.  The
 * caller guarantees the coordinate spans of shp_hull_build.  The work arrays live in buffers of the context's own (sp_*):
 * the outlines, the hulls, the neighbour table, the group lists and the shape table of the context are not touched.
 *  shp_simplify_need: *need_out = the bytes the buffers still have to grow by for n_vertices (at most 2^31 - 8192)
 *    vertices in n_rings rings of the ids 0 .. max_seg_id, at the bounds arcs <= vertices and points of the global class <=
 *    2 vertices (13 bytes a vertex, 24 an arc, 40 a point, 40 a ring, the result 24 a vertex, 24 a ring and 8 an id; with
 *    upload != 0 17 a vertex, 16 a ring and 8 an id more); *free_out = the device's free bytes.
 *  shp_simplify_source: all five arrays NULL: the context's traced outlines and flags, read in place (the counts are
 *    ignored; SHP_ERR_STATE without traced outlines or without the junction switch).  Otherwise host arrays, uploaded
 *    once; both offset arrays must ascend from 0 to their counts (the kernels index by them).
 *  shp_simplify_build: tolerance2q = floor(tolerance^2 65536) <= 2^46; path 0 auto, 1 short, 2 group, 3 global: an arc of
 *    up to 64 points is taken by one wavefront, of up to 1024 by one workgroup (both in LDS with the round loop in the
 *    kernel), a longer one in global arrays with one round per set of launches from the host; 2 puts every arc up to
 *    1024 points into the group class, 3 every arc into the global one.  Bases and spans as shp_hull_build.  A round
 *    splits every open interval whose candidate exceeds; more rounds than the longest arc has points is SHP_ERR_STATE,
 *    never a loop.  counts_out[10]: rings, vertices, rounds that split (the recursion's depth), arcs, points of the
 *    longest arc, arcs of the short, group and global class, vertices kept before the drop rule, 0.  steps_ms_out (may
 *    be NULL) [4]: device time of anchors and arcs, the rounds, areas and drop rule, the emission.  SHP_ERR_STATE when
 *    the traced outlines a resident source named have been replaced.
 *  shp_simplify_download: to host memory, all int64: ring_offsets (max_seg_id + 2), vertex_offsets (rings + 1), vertices
 *    (vertices x 2), ring_area2, source_ring (rings: the ring's index in the source), kept_vertex (vertices: the vertex's
 *    index in the source); arrays of no entries may be NULL.
 * Out of order the calls fail with SHP_ERR_STATE ("shp_simplify_source must come first", "shp_simplify_build must come
 * first"). */
int shp_simplify_need(shp_ctx *ctx, int64_t n_vertices, int64_t n_rings, int64_t max_seg_id, int upload, int64_t *need_out,
                      int64_t *free_out);
int shp_simplify_source(shp_ctx *ctx, const int64_t *ring_offsets, const int64_t *vertex_offsets, const int64_t *vertices,
                        const int64_t *ring_area2, const uint8_t *junction, int64_t max_seg_id, int64_t n_rings,
                        int64_t n_vertices, double *upload_ms_out);
int shp_simplify_build(shp_ctx *ctx, uint64_t tolerance2q, int path, int64_t row_base, int64_t col_base, int64_t row_span,
                       int64_t col_span, int64_t *counts_out, double *steps_ms_out);
int shp_simplify_download(shp_ctx *ctx, int64_t *ring_offsets, int64_t *vertex_offsets, int64_t *vertices, int64_t *ring_area2,
                          int64_t *source_ring, int64_t *kept_vertex);

/* ---- convex hulls of the outline rings: solidity and Feret diameters (outlines.calcSegmentHulls) ----
 * The strict convex hull of all vertices of each id's rings: no repeated points, no three consecutive collinear points,
 * oriented like an outer ring (positive under ringArea2's formula), from the hull vertex of the smallest (row, col).
 * hull_reach of the hull edge from point k to its successor = the largest cross product |e x (q - p_k)| over the hull's
 * points q (twice the area of the largest triangle on that edge); hull_area2 = the ring formula over the hull;
 * feret_max2 = the largest squared distance between two hull points.  Integers throughout: the result does not depend on
 * the launches, the atomics' order or the one size threshold (csrc/hull.h: lists of more than 64 points are walked by
 * one lane).  With H and W the row and column spans of all vertices the caller guarantees H W <= 2^32 and max(H, W) <
 * 2^31 (shp_hull_build refuses other spans): every cross product then stays within 2^33 and every squared distance fits
 * int64.  Memory and work follow the vertices, rings and ids, never a bounding box.  The work arrays live in buffers of
 * the context's own (hl_*): the outlines (a later shp_outline_download), the neighbour table, the group lists and the
 * shape table of the context are not touched.
 *  shp_hull_need: *need_out = the bytes the buffers still have to grow by for n_vertices vertices in n_rings rings of the
 *    ids 0 .. max_seg_id, at the bounds candidates <= vertices and hull points <= vertices (64 bytes a vertex, 40 an id;
 *    with upload != 0 16 a vertex, 16 a ring and 8 an id more); *free_out = the device's free bytes.
 *  shp_hull_source: the rings to hull.  All four arrays NULL: the context's traced outlines, read in place (the counts
 *    are ignored; SHP_ERR_STATE without traced outlines).  Otherwise host arrays as shp_outline_download fills them
 *    (ring_offsets max_seg_id + 2, vertex_offsets n_rings + 1, vertices n_vertices x 2, ring_area2 n_rings), uploaded
 *    once; both offset arrays must ascend from 0 to their counts, as shp_simplify_source asks (SHP_ERR_ARG "the vertex
 *    offsets do not ascend at ring ...", "the ring offsets do not ascend at id ..."; earlier versions checked their ends
 *    only: the two calls now share one check of the arrays).  *upload_ms_out (may be NULL): device time of the copies.
 *  shp_hull_build: (row_base, col_base) = the smallest row and column of all vertices, (row_span, col_span) = H and W.
 *    convex_only != 0: only the left-turn vertices of rings with ring_area2 > 0 are candidates, which holds the hull
 *    vertices of traced rings but not of arbitrary ones.  counts_out[3]: hull points, candidates, points kept after
 *    the column filter.  steps_ms_out (may be NULL) [5]: device time of the candidates, the order, the chains, the
 *    points, the reach.  SHP_ERR_STATE when the traced outlines a resident source named have been replaced.
 *  shp_hull_download: to host memory, all int64: hull_offsets (max_seg_id + 2), hull_points (hull points x 2, row then
 *    col), hull_reach (hull points), hull_area2 and feret_max2 (max_seg_id + 1 each, 0 for an id without rings); the
 *    points and the reach may be NULL without hull points.
 * Out of order the calls fail with SHP_ERR_STATE ("shp_hull_source must come first", "shp_hull_build must come
 * first"). */
int shp_hull_need(shp_ctx *ctx, int64_t n_vertices, int64_t n_rings, int64_t max_seg_id, int upload, int64_t *need_out,
                  int64_t *free_out);
int shp_hull_source(shp_ctx *ctx, const int64_t *ring_offsets, const int64_t *vertex_offsets, const int64_t *vertices,
                    const int64_t *ring_area2, int64_t max_seg_id, int64_t n_rings, int64_t n_vertices, double *upload_ms_out);
int shp_hull_build(shp_ctx *ctx, int64_t row_base, int64_t col_base, int64_t row_span, int64_t col_span, int convex_only,
                   int64_t *counts_out, double *steps_ms_out);
int shp_hull_download(shp_ctx *ctx, int64_t *hull_offsets, int64_t *hull_points, int64_t *hull_reach, int64_t *hull_area2,
                      int64_t *feret_max2);

/* ---- columns reduced over the neighbour table (neighbours.reduceOverNeighbours) ----------------------
 * The finished table stays in the context; these calls reduce per-segment columns over its rows on the device.
 * Row r has entries with neighbour id n and border length w; v is the column widened to float64.  A value is ignored
 * when it is NaN or (has_ignore != 0) equals ignore_value; C is the set of the row's entries whose v[n] is not ignored.
 * Statistic i (bit i of stat_mask, output outs[i], max_seg_id + 1 rows of 8 bytes in host memory):
 *   0 count |C| (int64); 1 border: sum of w over C (int64); 2 min and 3 max of v[n] (float64); 4 mean: (sum v[n]) / |C|;
 *   5 bordermean: (sum w v[n]) / sum w; and with the row's own value v[r]: 6 meanabsdiff: (sum w |v[n] - v[r]|) / sum w;
 *   7 bordertohigher: sum of w over v[n] > v[r] (int64); 8 nearest: the id with the smallest |v[n] - v[r]|, ties to the
 *   smallest id (int64).  A float statistic without a value (C empty; 6 also when v[r] is ignored) is missing_value, an
 *   integer one 0.  All arithmetic is float64, a product rounded before it is added; the order of a row's additions
 *   depends on the row's length alone (csrc/nbrreduce.h states it), so a row's result does not depend on the other
 *   rows, on the launch or on how the table got here.
 *  shp_nbr_upload: a host table (max_seg_id + 2 offsets, n_entries ids and lengths) becomes the context's finished
 *    table, for tables read from disk or built by hand.  It is checked on the device: offsets[0] == offsets[1] == 0, the
 *    offsets do not decrease and end at n_entries, a row's ids ascend strictly, lie in 1..max_seg_id and differ from
 *    the row, every length is >= 1 (symmetry is not required).  The first violation fails with SHP_ERR_ARG and its
 *    position in the message, and leaves no finished table.  dev_ms_out (may be NULL): device time of the check.
 *  shp_nbr_table_serial: *serial_out: a number no other table of the process has, new with every shp_nbr_begin and
 *    shp_nbr_upload of this context; *finished_out: 1 while the context holds a finished table.  A caller that
 *    remembers (context, serial) of a table can tell whether it is still resident and skip the upload.
 *  shp_nbr_reduce: one column (host memory, ctype 0 float64, 1 float32, 2 int64; n_rows == max_seg_id + 1) over the
 *    finished table; SHP_ERR_STATE ("no finished table") without one.  outs: 9 host pointers, those of the mask's
 *    bits non-NULL.  Device memory beyond the table: the widened column and the selected outputs.  dev_ms_out (may be
 *    NULL): device time of the kernels (with the listing of the table's long rows in the first call after a new
 *    table), transfers excluded. */
int shp_nbr_upload(shp_ctx *ctx, const int64_t *offsets, const uint32_t *neighbours, const int64_t *border_lengths,
                   int64_t max_seg_id, int64_t n_entries, double *dev_ms_out);
int shp_nbr_table_serial(shp_ctx *ctx, uint64_t *serial_out, int *finished_out);
int shp_nbr_reduce(shp_ctx *ctx, const void *col, int ctype, int64_t n_rows, int has_ignore, double ignore_value,
                   double missing_value, uint32_t stat_mask, void *const *outs, double *dev_ms_out);

/* ---- touching segments of one class merged into one (neighbours.mergeSegments; csrc/nbrmerge.h) ---------------
 * keys[i] is the class of id i.  Entry (a, b, w) of the finished table is a LINK when keys[a] == keys[b], that key is
 * not the ignored one, w >= min_border and (with seg_size) both ids have pixels; a GROUP is a connected component of
 * the links over the ids 1 .. max_seg_id.  With seg_size an id of size 0 belongs to no group and recodes to 0; without
 * it every id is a vertex and an id without links is a group of one.  Groups are numbered 1 .. M in ascending order of
 * their smallest member.  The table is taken to name every pair from both sides, as every table built here does: only
 * its entries with a < b are read.  All of it is integer work and a pure function of the arguments.
 *  shp_nbr_merge: keys and seg_size (may be NULL) are host columns of n_rows == max_seg_id + 1 int64; has_ignore != 0:
 *    ids of key ignore_key link to nobody.  The links are hooked into a union-find forest on the device, the roots
 *    flagged, scanned and numbered.  *max_group_out = M; counters_out (may be NULL) [2]: the links, the entries with
 *    a < b; dev_ms_out (may be NULL) [2]: device time of the hook, of the renumbering.  The groups stay in the context,
 *    in buffers of their own, until the next shp_nbr_merge or shp_nbr_merge_similar.
 *  shp_nbr_merge_groups: the groups to host memory, a NULL pointer skipping its array: recode (max_seg_id + 1 uint32,
 *    recode[0] == 0), representative (M + 1 uint32: the smallest old id of a group, row 0 is 0), group_size (M + 1
 *    int64: the old ids of a group, row 0 is 0), hist (M + 1 int64: the sums of seg_size, row 0 the pixels of the ids
 *    that recode to 0; without seg_size what shp_nbr_merge_recode_dev has counted so far).
 *  shp_nbr_merge_contract: every entry (a, b, w), a < b, whose ends recode to different non-zero ids becomes a record
 *    (recode a, recode b, w); the records go through the sort and reduction of shp_nbr_finish, and the table over
 *    0 .. M that results REPLACES the table the groups were found in as the context's finished table, with a new
 *    serial: shp_nbr_download and shp_nbr_reduce then work on it.  SHP_ERR_STATE when that table is no longer the
 *    finished one.  *n_entries_out: its entries; *records_out: the records handed to the sort; a border length of
 *    2^32 or more is SHP_ERR_ARG.  dev_ms_out (may be NULL): device time of the call.
 *  shp_nbr_merge_recode_dev: d_out[p] = recode[d_seg[p]] for npix labels in device memory (both 4-byte aligned, not
 *    overlapping).  A label above max_seg_id is not looked up and its pixel becomes 0; *bad_label_out: 0, or the
 *    largest such label.  count_hist != 0: the new ids are counted into hist in the same pass (only for groups found
 *    without seg_size: SHP_ERR_ARG otherwise).  dev_ms_out (may be NULL): device time of the kernel. */
int shp_nbr_merge(shp_ctx *ctx, const int64_t *keys, int64_t n_rows, int has_ignore, int64_t ignore_key,
                  int64_t min_border, const int64_t *seg_size, uint32_t *max_group_out, int64_t *counters_out,
                  double *dev_ms_out);
int shp_nbr_merge_groups(shp_ctx *ctx, uint32_t *recode, uint32_t *representative, int64_t *group_size, int64_t *hist);
int shp_nbr_merge_contract(shp_ctx *ctx, int64_t *n_entries_out, int64_t *records_out, double *dev_ms_out);
int shp_nbr_merge_recode_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t npix, uint32_t *d_out, int count_hist,
                             uint32_t *bad_label_out, double *dev_ms_out);

/* ---- touching segments that look alike merged into one (neighbours.mergeSimilarSegments; csrc/nbrmerge.h) -------
 * shp_nbr_merge with another link rule; everything after the links is shp_nbr_merge's.  cols: n_cols (1 to 8) host
 * columns of n_rows == max_seg_id + 1 float64.  A value is IGNORED when it is NaN or (has_ignore_value != 0) equals
 * ignore_value; an id with an ignored value in any column links to nobody.  d2(a, b) = the sum over the columns, in
 * their order and from +0.0, of t * t with t = x[a] - x[b], every operation rounded to float64 once.  Entry (a, b, w)
 * is a CANDIDATE when w >= min_border, both ids have pixels (seg_size, may be NULL), d2 is finite and -- with keys
 * (may be NULL) -- keys[a] == keys[b] and that key is not the ignored one.
 *   mutual_nearest == 0: a candidate is a link when d2 <= thr2 (has_threshold must be set).  The groups are the
 *     connected components: single linkage.
 *   mutual_nearest != 0: best[a] is the candidate neighbour of row a with the smallest d2, the smallest id among
 *     equals; a candidate is a link when best[a] == b, best[b] == a and (has_threshold != 0) d2 <= thr2.  Groups have
 *     one or two members.  Every row is read from its own side: the table must name every pair from both sides.
 * thr2 is the squared distance (>= 0, +inf allowed: every finite d2 passes).  Device memory beyond shp_nbr_merge's:
 * one record of n_cols float64 per id, and for the mutual rule 12 bytes per id.  max_group_out and counters_out as
 * shp_nbr_merge; dev_ms_out (may be NULL) [3]: device time of the hook (with the two passes that find best), of the
 * renumbering, of laying the columns out as records.  The groups are left in the context exactly where shp_nbr_merge
 * leaves them: shp_nbr_merge_groups, _contract and _recode_dev follow as they follow shp_nbr_merge. */
int shp_nbr_merge_similar(shp_ctx *ctx, const double *const *cols, int n_cols, int64_t n_rows, int has_ignore_value,
                          double ignore_value, int has_threshold, double thr2, int mutual_nearest, const int64_t *keys,
                          int has_ignore_key, int64_t ignore_key, int64_t min_border, const int64_t *seg_size,
                          uint32_t *max_group_out, int64_t *counters_out, double *dev_ms_out);

/* ---- columns of the old ids carried to the groups of a merge (neighbours.aggregateToGroups; csrc/nbragg.h) -----
 * The groups of a merge have a serial, new with every shp_nbr_merge / shp_nbr_merge_similar, from the numbering of
 * the tables' serials.  Their MEMBER LIST is a CSR over the new ids 0 .. M: offsets (M + 2 int64, offsets[0] ==
 * offsets[1] == 0) and the old ids of every group in ascending order; ids that recode to 0 are in no group.  It is
 * kept in buffers of its own until the next merge call and does not touch the finished neighbour table.
 *  shp_nbr_groups_serial: *groups_serial_out: the serial of the groups the context holds (0: none);
 *    *members_serial_out: the serial of the groups whose member list it holds (0: none).
 *  shp_nbr_members_build: recode == NULL: the member list of the resident groups, built unless it is there already.
 *    Otherwise recode is a host column of n_rows uint32 with values 0 .. max_group and recode[0] == 0 (SHP_ERR_ARG
 *    if not): it is uploaded, the groups' sizes are counted and the list is built; it gets a serial of its own.  The
 *    list is a pure function of recode, so both ways give the same arrays.  *serial_out: the list's serial;
 *    *n_members_out: its entries; dev_ms_out (may be NULL): device time of the build.
 *  shp_nbr_members_download: offsets (M + 2 int64) and members (n_members uint32) to host memory.
 *  shp_nbr_aggregate: one column of the OLD ids (host; ctype and n_rows as shp_nbr_reduce, n_rows == the recode's
 *    rows) reduced per group over the members whose value is not ignored.  weights: host, n_rows int64 >= 0, or NULL
 *    (every weight 1).  stat_mask bits / outs slots (host, M + 1 rows of 8 bytes): 0 count, 1 weight (sum of the
 *    weights), both int64; 2 min, 3 max; 4 sum: int64, exact and wrapping, for ctype 2, float64 otherwise; 5 mean =
 *    (float64 sum) / count; 6 weightedmean = (sum of float64(w) * v, each product rounded) / (sum w).  Row 0 and every
 *    group without a value (for weightedmean also: weights that sum to 0) hold missing_value in the float statistics
 *    and 0 in the integer ones.  The float sums run over a group's members in the order csrc/nbrreduce.h states for a
 *    row of that length, so a group's result depends on nothing but the group. */
int shp_nbr_groups_serial(shp_ctx *ctx, uint64_t *groups_serial_out, uint64_t *members_serial_out);
int shp_nbr_members_build(shp_ctx *ctx, const uint32_t *recode, int64_t n_rows, int64_t max_group, uint64_t *serial_out,
                          int64_t *n_members_out, double *dev_ms_out);
int shp_nbr_members_download(shp_ctx *ctx, int64_t *offsets, uint32_t *members);
int shp_nbr_aggregate(shp_ctx *ctx, const void *col, int ctype, int64_t n_rows, const int64_t *weights, int has_ignore,
                      double ignore_value, double missing_value, uint32_t stat_mask, void *const *outs, double *dev_ms_out);

/* ---- the neighbour table of a row-sharded raster (distributed.findSegmentNeighboursDistributed; csrc/dneighbours.h)
 * The table above for a label raster whose rows are spread over the ranks, without gathering the labels.  The result
 * is sharded by ID: a rank ends up with the finished CSR rows of the ids id_lo .. id_hi - 1 (its share; the shares
 * partition 0 .. max_seg_id) -- whole rows, equal to those of the one-GPU table of the assembled raster.  The share
 * table lives in buffers of its own: it is not the "finished table" of shp_nbr_reduce and has a serial of its own.
 * shp_dnbr_local_dev starts a one-GPU accumulation internally, so it ends any one-GPU table of the context.
 *  shp_dnbr_local_dev: the rank's nrows rows of ncols labels in device memory (nrows may be 0) and d_halo_row, the
 *    raster's row after them (NULL when the raster ends there: it is the first row of the next rank that holds rows).
 *    Pairs whose upper pixel lies in the rank's rows are counted, sorted and reduced to the rank's distinct pairs
 *    and packed as 16-byte records (b, a, count low word, count high word), a < b, at most one per pair: the HOME
 *    records (both ids in the share) stay in the context, the TRAVELLING ones are at *d_travel_out (context memory,
 *    valid until the next shp_dnbr_local_dev).  *max_label_out: the largest label met; when it is above max_seg_id
 *    nothing else is done (the counts are 0) and shp_dnbr_merge_dev fails.  counts_out[3]: distinct pairs, home
 *    records, travelling records.
 *  shp_dnbr_merge_dev: d_all holds `world` blocks of `slot` records, the all-gathered travelling records, counts[r]
 *    (host) valid ones in block r.  The records with an id in the share are picked, joined with the home records,
 *    sorted, reduced with 64-bit sums, and the CSR of the share is built: offsets (id_hi - id_lo + 1 int64 from 0),
 *    neighbour ids ascending within a row, border lengths.  d_cols: 2 (max_seg_id + 1) int64 in device memory,
 *    numNeighbours then borderLength; they are zeroed and the share's rows filled, so an integer all-reduce over the
 *    ranks completes them.  *n_picked_out: records taken from d_all; *n_entries_out: entries of the share table.
 *  shp_dnbr_download: the share table's three arrays to host memory.
 *  shp_dnbr_upload: a share table from host memory (as downloaded; the caller vouches for its ids and order) becomes
 *    the context's share table, with a new serial.
 *  shp_dnbr_table_serial: as shp_nbr_table_serial, for the share table.  The serials of share tables and of one-GPU
 *    tables come from one numbering, so no two tables of a process share one.
 *  shp_dnbr_reduce_dev: shp_nbr_reduce over the share table.  col: the FULL column (host, max_seg_id + 1 values); row i
 *    of the share is id id_lo + i, its own value col[id_lo + i].  d_out: device memory for the mask's statistics in
 *    the order of their bits, max_seg_id + 1 values of 8 bytes each; zeroed, then the share's rows written (a row
 *    without neighbours gets missing_value from this rank), so an integer all-reduce of the bit patterns assembles
 *    the columns.  A row's additions run in the order csrc/nbrreduce.h states: the results are bit for bit those of
 *    shp_nbr_reduce over the whole table.  dev_ms_out of all calls may be NULL; local and merge report the device
 *    time of the build so far. */
int shp_dnbr_local_dev(shp_ctx *ctx, const uint32_t *d_seg, int64_t nrows, int64_t ncols, const uint32_t *d_halo_row,
                       int64_t max_seg_id, int four_connected, int64_t id_lo, int64_t id_hi, uint32_t *max_label_out,
                       int64_t *counts_out, void **d_travel_out, double *dev_ms_out);
int shp_dnbr_merge_dev(shp_ctx *ctx, const void *d_all, int64_t slot, int world, const uint32_t *counts, void *d_cols,
                       int64_t *n_picked_out, int64_t *n_entries_out, double *dev_ms_out);
int shp_dnbr_download(shp_ctx *ctx, int64_t *offsets, uint32_t *neighbours, int64_t *border_lengths);
int shp_dnbr_upload(shp_ctx *ctx, const int64_t *offsets, const uint32_t *neighbours, const int64_t *border_lengths,
                    int64_t max_seg_id, int64_t id_lo, int64_t id_hi, int64_t n_entries);
int shp_dnbr_table_serial(shp_ctx *ctx, uint64_t *serial_out, int *finished_out);
int shp_dnbr_reduce_dev(shp_ctx *ctx, const void *col, int ctype, int64_t n_rows, int has_ignore, double ignore_value,
                        double missing_value, uint32_t stat_mask, void *d_out, double *dev_ms_out);

/* ---- shp_nbr_merge / shp_nbr_merge_similar over the share table (csrc/dnbrmerge.h) ---------------------
 * The groups of the WHOLE table on every rank, from the ranks' share tables, and the contracted table sharded by the
 * new ids.  The links, the groups' numbering and the contracted table are shp_nbr_merge's; columns are the full ones
 * (max_seg_id + 1 values, host memory, the same on every rank).  Between the calls the caller runs the collectives.
 *  shp_dnbr_mrg_begin: the rule (n_cols 0: the key rule of shp_nbr_merge, keys required; otherwise the rule of
 *    shp_nbr_merge_similar) over the context's share table, which every later step reads.  With mutual_nearest the
 *    rows' best neighbours are found and *d_best_out is an int64 column of max_seg_id + 1 values in context memory,
 *    best + 1 in the share's rows and 0 elsewhere: an integer all-reduce over the ranks completes it in place.
 *    Otherwise *d_best_out is NULL.  dev_ms_out[2]: the records' kernels, the best passes.
 *  shp_dnbr_mrg_hook: the share's entries a < b that are links are hooked into a forest over all ids.
 *    counts_out[3]: links, entries a < b, forest pairs; *d_pairs_out: that many 8-byte pairs (id, root of the id in
 *    this rank's forest) of the ids that are not their own root, in context memory (NULL for none), for an all-gather
 *    with slot = the largest count.  dev_ms_out[2]: the hook, the flatten and the compaction.
 *  shp_dnbr_mrg_number: d_all holds `world` blocks of `slot` pairs, counts[r] (host) valid ones in block r; the pairs
 *    of the blocks other than `rank` are hooked into the rank's forest and the groups are numbered.  From here on the
 *    context holds the groups as after shp_nbr_merge: shp_nbr_merge_groups, shp_nbr_merge_recode_dev,
 *    shp_nbr_members_build and shp_nbr_aggregate serve them (shp_nbr_merge_contract does not: there is no one-GPU
 *    table).  *d_hist_out: the groups' histogram, max_group + 1 int64 in context memory (after
 *    shp_nbr_merge_recode_dev with count_hist an integer all-reduce completes it).  dev_ms_out[2]: the pairs' hook,
 *    the renumbering.
 *  shp_dnbr_mrg_records: the share's entries a < b between two groups become records, are reduced to distinct pairs
 *    and split against the rank's share new_id_lo .. new_id_hi - 1 of the new ids, as shp_dnbr_local_dev leaves them:
 *    *d_travel_out for the all-gather, then shp_dnbr_merge_dev builds the new share table (max_seg_id = max_group),
 *    which replaces the old one under a new serial.  counts_out[5]: records, distinct pairs, home records, travelling
 *    records, border lengths outside 1 .. 2^32 - 1; with such a length nothing else is done, the old share table stays
 *    and the merge has ended. */
int shp_dnbr_mrg_begin(shp_ctx *ctx, const double *const *cols, int n_cols, int64_t n_rows, int has_ignore_value,
                       double ignore_value, int has_threshold, double thr2, int mutual_nearest, const int64_t *keys,
                       int has_ignore_key, int64_t ignore_key, int64_t min_border, const int64_t *seg_size,
                       void **d_best_out, double *dev_ms_out);
int shp_dnbr_mrg_hook(shp_ctx *ctx, int64_t *counts_out, void **d_pairs_out, double *dev_ms_out);
int shp_dnbr_mrg_number(shp_ctx *ctx, const void *d_all, int64_t slot, int world, const uint32_t *counts, int rank,
                        uint32_t *max_group_out, void **d_hist_out, double *dev_ms_out);
int shp_dnbr_mrg_records(shp_ctx *ctx, int64_t new_id_lo, int64_t new_id_hi, int64_t *counts_out, void **d_travel_out,
                         double *dev_ms_out);

/* ---- the shared prefix sum and radix sort on their own (csrc/prims.h; for the tests) -------------------------
 * csrc/scan.h's scan_exclusive and csrc/sort.h's sort_pairs, called as the product's forty call sites call them, on
 * buffers of the caller's in device memory (shp_dev_alloc; 4-byte aligned is enough, and a pointer that is not 16-byte
 * aligned makes the kernels take their 4-byte loads and stores).  No product path uses these two: they let a test
 * choose n, alignment and flags.  Both use the context's scan and sort workspaces (and the first words of its small
 * scratch block), so neither may come between the steps of a call sequence that keeps state in the workspace
 * (shp_segpoints_*, shp_dsegpoints_*, shp_dcolour_*); shp_dev_* transfers may come before and after.  n of 2^32 or
 * more and NULL pointers are SHP_ERR_ARG.
 *  shp_prim_scan: d_out[i] = sum of d_in[0 .. i - 1] modulo 2^32 for n words.  flags bit 0: read d_in through a
 *    functor without the 16-byte load (get4); bit 1: ask for the lazy add-back -- d_out is then left without the
 *    per-block offsets, which go to d_boff_out (device, ceil(n / 8192) words) with their count in *nboff_out (0 when
 *    the scan had one block and handed back no offsets).  Without bit 1 d_boff_out and nboff_out may be NULL.
 *    *total_dev_out: the total as the scan's device word holds it; *total_mirror_out: as the word of the pinned
 *    block holds it after the stream's synchronisation.  Both words hold 0xA5A5A5A5 before the scan.
 *  shp_prim_sort: sorts n (key, value) pairs stably by the low 8 * max(1, ceil(bits / 8)) key bits (sort_pairs sorts
 *    whole bytes), bits 0 .. 32.  d_vals NULL: the values are the indices 0 .. n - 1.  flags bit 0: the staged
 *    scatter.  d_keys_out NULL: sort_pairs is told the keys are not wanted (its last pass writes none).  The result
 *    is copied out of the library's ping-pong buffers, so d_keys_out / d_vals_out must not be those.
 *    digit_starts_out (host, 257 words, may be NULL): when the sort took one pass (bits <= 8), entry d is
 *    sort_digit_start(d) read on the device from the pass's scanned histogram as the k-means fit reads it -- the
 *    position of the first key whose low byte is d, and n for d = 256; all zero for n = 0; untouched for more
 *    passes. */
int shp_prim_scan(shp_ctx *ctx, const uint32_t *d_in, uint64_t n, uint32_t *d_out, int flags, uint32_t *total_dev_out,
                  uint32_t *total_mirror_out, uint32_t *d_boff_out, uint32_t *nboff_out);
int shp_prim_sort(shp_ctx *ctx, const uint32_t *d_keys, const uint32_t *d_vals, uint64_t n, int bits, int flags,
                  uint32_t *d_keys_out, uint32_t *d_vals_out, uint32_t *digit_starts_out);

/* ---- multi-GPU exchange -----------------------------------------------------------------
 * One process per GPU.  The reference ships whole pickled tile results to one process over a
 * multiprocessing.managers TCP channel (NetworkDataChannel, tiling.py:1799-1912; SegmentationResultCache
 * :1966-2001); here the tiles are sharded and only the stitch's boundary data crosses GPUs, over RCCL:
 * shp_comm_send / shp_comm_recv move a recoded overlap strip (device memory, xGMI point to point),
 * shp_comm_bcast the k-means centres, shp_comm_allgather the sample parts, shp_comm_allreduce
 * (op 0: int64 sum, op 1: float64 max) the segment histogram and the timing.  A communicator is
 * bound to a context (its device and stream); every call returns when the operation is complete.
 * shp_comm_unique_id: 128 bytes made by rank 0 and handed to the other ranks out of band. */
typedef struct shp_comm shp_comm;
int  shp_comm_unique_id(void *id_out_128);
int  shp_comm_create(shp_ctx *ctx, int rank, int world, const void *unique_id_128, shp_comm **out);
void shp_comm_destroy(shp_comm *comm);
int  shp_comm_send(shp_comm *comm, const void *d_buf, size_t bytes, int dst);
int  shp_comm_recv(shp_comm *comm, void *d_buf, size_t bytes, int src);
int  shp_comm_bcast(shp_comm *comm, void *d_buf, size_t bytes, int root);
int  shp_comm_allgather(shp_comm *comm, const void *d_send, void *d_recv, size_t bytes_per_rank);
int  shp_comm_allreduce(shp_comm *comm, void *d_buf, size_t count, int op);
/* ncclCommCount: how many ranks RCCL itself says the communicator spans (quoted by the bench line). */
int  shp_comm_count(shp_comm *comm, int *nranks_out);
/* The strips of the parallel stitch (distributed.py, replacing the whole-tile pickles of tiling.py:1799-1912)
 * travel asynchronously: shp_comm_isend enqueues the send on the communicator's own stream behind an event
 * recorded on `producer`'s stream (the chain step that writes the strip), shp_comm_irecv enqueues the
 * receive there and makes `consumer`'s stream wait for it on the device; neither waits on the host, so a
 * rank's chain never stalls for its neighbour.  Operations of one communicator complete in issue order; both
 * ends issue them in the order of the boundary plan.  shp_comm_group(1) / (0) = ncclGroupStart / End (a rank
 * that sends to itself must group the pair; inside a group pass consumer = NULL and call shp_comm_wait after
 * the group's end: the receive is only enqueued then); shp_comm_drain waits on the host for everything issued. */
int  shp_comm_isend(shp_comm *comm, const void *d_buf, size_t bytes, int dst, shp_ctx *producer);
int  shp_comm_irecv(shp_comm *comm, void *d_buf, size_t bytes, int src, shp_ctx *consumer);
int  shp_comm_group(shp_comm *comm, int begin);
int  shp_comm_wait(shp_comm *comm, shp_ctx *consumer);
int  shp_comm_drain(shp_comm *comm);

#ifdef __cplusplus
}
#endif
#endif /* SHEPSEG_HIP_H */
