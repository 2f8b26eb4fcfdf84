// common.h -- context, device buffers, error handling, small device helpers.
// Part of libshepseg_hip.so (gfx950 only; wavefront = 64 everywhere).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include <mutex>
#include <condition_variable>
#include "../../include/shepseg_hip.h"
#include "walkbatch.h"

#define WAVE 64
#define NULL_LAB 0xFFFFFFFFu   // CCL label of a null pixel
#define VIS_FLAG 0x80000000u   // set on labels assigned by the depth-first splitter
#define MAX_CLUMP_SIZE 10000u  // shepseg.py:481
#define PROF_N 16
#define PROF_POOL 32
#define SHP_PINNED_BYTES (1u << 20)   // pinned host staging per context
// The last 64 words of the staging block are MIRRORS: scalars the host needs after a phase (counts,
// scan totals) are stored there by the kernel that produces them (system-scope stores to the mapped
// pinned block) instead of by a copy command queued behind it -- under load every command on a
// stream costs 40-80 us, and there were ten such copies per tile.
#define PIN_MIRROR (SHP_PINNED_BYTES / 4u - 64u)
enum { MIR_NBIG = 0, MIR_RELABEL = 4, MIR_RUNS = 5, MIR_PTS = 8, MIR_NBR = 16, MIR_PRIM = 32 };     // (MIR_PTS: 8 words, segpoints.h; MIR_NBR: 3, neighbours.h; MIR_PRIM: 1, prims.h)
#define MIRROR_STORE(ptr, v) __hip_atomic_store((ptr), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM)

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

struct StageTimer {
    hipEvent_t a = nullptr, b = nullptr;
};

// what shp_segpoints_build leaves for shp_segpoints_emit (segpoints.h); any other call of the context clears
// `valid`, since it may reuse the workspace the sorted runs live in
struct SegPointsState {
    const uint32_t *skeys = nullptr, *order = nullptr, *roff = nullptr;
    const void *band = nullptr;
    int dtype = 0;
    uint32_t ncols = 0, S = 0, m = 0, npts = 0;
    bool valid = false;
};

// what shp_dsegpoints_build_dev leaves for shp_dsegpoints_merge_dev (stage 1), and that for
// shp_dsegpoints_emit (stage 2) (dsegpoints.h); any other call of the context resets stage to 0
struct DSegPointsState {
    int stage = 0;
    uint32_t row0 = 0, nrec = 0, npts_local = 0, id_lo = 0, id_hi = 0, nmerged = 0, npts_emit = 0;
    unsigned long long max_visit = 0;       // largest visit index of the whole raster
};

// a row-sharded column between the steps of its selection (colour.h: shp_dcolour_*): the share lives in the
// workspace, so no other workspace call of the context may come between the steps
struct DColourState {
    int stage = 0;                  // 0 none, 1 selecting (next: `pass`, histogram then pick), 2 (lo, hi) known
    int pass = 0, picked = 1;
    size_t m = 0, n = 0;            // rows of the share, of the whole column
    double gamma[2] = {}, lo = 0.0, hi = 0.0, dev_ms = 0.0;
};

// the rows of a CSR that the reduction kernels treat as long (nbrreduce.h: more than NBRR_LONG entries) and their
// chunks: lrow[k] the k-th long row, lcoff[k] the chunks of the long rows before it.  serial: the table or member
// list it was built for (0: none); nbrr_long_ensure builds it again only for another serial.
struct NbrLongList {
    DevBuf lrow, lcoff;
    uint32_t nlong = 0, nchunks = 0;
    unsigned long long serial = 0;
};

// A resident CSR neighbour table: rows row0 .. row0 + nrows - 1 of the ids 0 .. S, whole rows.  The one-GPU table
// (neighbours.h) is the share [0, S + 1); the share table of a row-sharded raster (dneighbours.h) holds the rows of
// distributed.idRange.  serial: a number no other table of the process has (nbr_next_serial); whoever remembers it
// and the context can tell whether the buffers still hold that table.  S, row0 and nrows are known from the step
// that begins a table; nent and finished once it stands.
struct NbrTable {
    DevBuf offs, ids, lens;         // nrows + 1 int64, nent uint32, nent int64
    uint32_t S = 0, row0 = 0, nrows = 0;
    unsigned long long nent = 0, serial = 0;
    bool finished = false;
    NbrLongList longs;
};
// the table is gone (its buffers and the list of its long rows stay allocated)
static inline void nbr_table_end(NbrTable &t)
{
    t.S = t.row0 = t.nrows = 0u;
    t.nent = t.serial = 0ull;
    t.finished = false;
}
static inline void nbr_long_bufs(NbrLongList &l, std::vector<DevBuf *> &out) { out.push_back(&l.lrow); out.push_back(&l.lcoff); }
static inline void nbr_table_bufs(NbrTable &t, std::vector<DevBuf *> &out)
{
    out.push_back(&t.offs); out.push_back(&t.ids); out.push_back(&t.lens);
    nbr_long_bufs(t.longs, out);
}

// the records of a one-GPU table between shp_nbr_begin and shp_nbr_finish (neighbours.h), in a buffer of their own
// (nbr_rec), so transfers and other calls may come between the steps.  The table they become is shp_ctx::nbr_tab.
struct NbrState {
    bool open = false;              // accumulating
    int eight = 0;
    int64_t given = -1;             // the caller's max_seg_id, -1: take the largest label
    unsigned long long cap = 0, used = 0, last_block = 0;      // records: room, stored, of the last block
    unsigned long long pairs = 0;   // differing pixel pairs met
    unsigned long long reruns = 0;  // row blocks that did not fit and ran a second time
    uint32_t max_label = 0;
    double dev_ms = 0.0;
};

// the exchange that builds a rank's share table (dneighbours.h, shp_ctx::dnbr_tab) between its local step and its
// merge: the share itself (S, row0, nrows) waits in the table
struct DNbrState {
    int stage = 0;                  // 0 none, 1 local step done (home and travelling records packed)
    unsigned long long nlocal = 0, nhome = 0, ntrav = 0;
    double dev_ms = 0.0;
};

// the groups of neighbours.mergeSegments between shp_nbr_merge and the calls that use them (nbrmerge.h), in buffers
// of their own (mrg_*): recode of S + 1 rows, representative / group size / histogram of M + 1.  table_serial: the
// table the groups were found in; contracted: that table has been replaced by the groups' own.
struct MrgState {
    int stage = 0;                  // 0 none, 1 groups known
    uint32_t S = 0, M = 0;
    unsigned long long links = 0, half = 0;     // links; entries with a < b
    unsigned long long table_serial = 0;
    unsigned long long serial = 0;  // of these groups, from the numbering of the tables: new with every merge
    bool has_size = false, contracted = false;
};

// a merge over a rank's share table (dnbrmerge.h) between its steps: the link rule as shp_dnbr_mrg_begin was given
// it (the columns lie in mrg_key / mrg_size / mrg_rec), the share table it reads, the forest pairs it sends
struct DMrgState {
    int stage = 0;                  // 0 none, 1 begun (columns placed, the mutual rule's best packed), 2 hooked, 3 numbered
    int similar = 0, ncol = 0, has_key = 0, has_size = 0, has_ign = 0, has_thr = 0, mutual = 0;
    long long ign = 0, minb = 1;
    double thr2 = 0.0;
    unsigned long long table_serial = 0;        // NbrTable::serial of the share table
    unsigned long long npairs = 0;
    double ms_records = 0.0;
};

// the member list of a merge's groups (nbragg.h): the old ids of every group in ascending order, as a CSR over the
// new ids 0 .. M in buffers of its own (agg_*); the list of its long rows is shp_ctx::agg_longs, which this state's
// resets leave alone.  serial: the groups it belongs to (MrgState::serial, or a number of its own when the recode
// came from the host).  It lasts until the next merge.
struct AggState {
    int stage = 0;                  // 0 none, 1 built
    uint32_t S = 0, M = 0;
    unsigned long long serial = 0, nmem = 0;
    const uint32_t *recode = nullptr;   // the device recode it was built from: mrg_recode or agg_recode
    double dev_ms = 0.0;
};

// the per-segment shape table between shp_shape_begin and shp_shape_download (segshape.h), in buffers of its own
// (shape_tab: 88 bytes per id; shape_ctr), so the neighbour table and the group lists stay where they are
// A rank's rows of a sharded raster (dsegshape.h) go 1 -> 3 -> 2: the straddlers' rows leave the table as records
// (dshape_rec, 96 bytes each; dshape_ctr, dshape_rcnt) before the ranks' records are folded into it.
struct ShapeState {
    int stage = 0;                  // 0 none, 1 accumulating, 2 finished, 3 classified: the straddlers' records packed
    uint32_t S = 0;
    unsigned long long nrec = 0;    // records packed by the classification
    unsigned long long row0 = 0, col0 = 0;      // coordinates of the raster's first pixel
    unsigned long long rows_done = 0;           // rows of the blocks so far
    double dev_ms = 0.0;
};

// the outlines between shp_outline_edges_dev, shp_outline_trace and shp_outline_download (outline.h), in buffers of
// their own (ol_*), so the neighbour table, the group lists and the shape table stay where they are.  seg: the
// caller's labels, which must stay in place from the first call to the second.
struct OutlineState {
    int stage = 0;                  // 0 none, 1 edges counted, 2 traced
    const uint32_t *seg = nullptr;
    uint32_t nrows = 0, ncols = 0, S = 0;
    int eight = 0;
    int junctions = 0;              // the junction switch (shp_outline_junctions): set after the edges, gone with the next ones
    bool has_flags = false;         // traced with the switch on: ol_jflag holds a flag per vertex
    uint32_t edges = 0, rings = 0, verts = 0, rounds = 0;
    size_t voff64_at = 0, area_at = 0;          // where the int64 vertex offsets and the ring areas lie in ol_ring
    double ms[4] = {};              // device time: sides and scan, successors, doubling rounds, rings and vertices
    unsigned long long serial = 0;  // shp_ctx::outline_calls when these edges were counted: which outlines these are
};

// where the rings come from that something built on the outlines works on (rings.h, which holds everything that reads
// or writes this; the struct stands here because the states below hold one each).  resident: the rings are read in
// place from the outline buffers, which must still hold the outlines of outline_serial; otherwise they were uploaded
// into buffers of the holder's own.
struct RingSource {
    bool resident = false;
    unsigned long long outline_serial = 0;
    uint32_t S = 0, nr = 0, nv = 0;     // the ids 0 .. S, rings, vertices
};

// the hulls of the outline rings between shp_hull_source, shp_hull_build and shp_hull_download (hull.h), in buffers
// of their own (hl_*): the outline state, the neighbour table, the group lists and the shape table stay where they
// are.  src: the rings taken by shp_hull_source, its own instance (the simplification may hold other rings).
struct HullState {
    int stage = 0;                  // 0 none, 1 rings known, 2 hulls built
    RingSource src;
    uint32_t ncand = 0, nkept = 0, nh = 0;      // candidates, points kept of them, hull points
    size_t hoff64_at = 0, area_at = 0, feret_at = 0;    // where the int64 offsets, areas and diameters lie in hl_id
    double ms[5] = {};              // device time: candidates, order, chains, points, reach
};

// the depth transform between shp_depth_transform_dev, shp_depth_envelope, shp_depth_reduce and shp_depth_download
// (segdepth.h), in buffers of their own (dp_*): the outlines, the hulls, the neighbour table, the group lists and the
// shape table stay where they are.  seg: the caller's labels, which must stay in place from the first call to the third.
struct DepthState {
    int stage = 0;                  // 0 none, 1 transformed up to the marked runs, 2 the envelope done, 3 reduced
    const uint32_t *seg = nullptr;
    uint32_t nrows = 0, ncols = 0, S = 0, nruns = 0;
    int all = 0;                    // every run marked (path 'envelope')
    unsigned long long deferred = 0, room = 0;      // pixels the window deferred; scratch positions of the marked runs
    double ms[4] = {};              // device time: column step, window, marked runs and envelope, reduction
};

// The context's named workspace buffers (grow-only), each named HERE ONLY: the list makes the members of shp_ctx and
// the entries of shp_ctx::bufs, which is what buf_ensure's regrow log indexes and shp_ctx_destroy frees.
#define SHP_CTX_BUFS(X) \
    X(img) X(clus) X(lab) X(seg) X(aux) X(aux2) X(stack) X(scan_tmp) X(sort_k0) X(sort_k1) X(sort_v1) \
    X(sort_hist) X(pix) X(segsz) X(origsz) X(off) X(ssum) X(chnext) X(chtail) X(mergeto) X(tcount) X(toff) \
    X(tfill) X(tlist) X(tsorted) X(small) X(cen) X(fit_x) X(fit_lab) X(fit_part) X(fit_lb) X(big) X(srclist) \
    X(tgtlist) X(bigbits) X(singles) X(dbg) X(snap) X(pts_runs) X(pts_off) X(pts_offs) X(pts_stage) X(dpts_lh) \
    X(dpts_cls) X(dpts_spos) X(dpts_rec) X(dpts_moff) X(dpts_eoff) X(dpts_cnt) X(dpts_kpos) X(dpts_mrec) \
    X(dpts_key) X(dpts_idx) X(dpts_k0) X(dpts_k1) X(dpts_v1) X(dpts_pix) X(vflag) X(vlist) X(vredo) X(nbr_ctr) \
    X(nbr_rec) X(nbr_key) X(nbr_val) X(nbr_uidx) X(nbr_ua) X(nbr_ub) X(nbr_ucnt) X(nbr_deg) X(nbr_hoff) \
    X(nbr_loff) X(nbrr_col) X(nbrr_out) X(nbrr_part) X(dnbr_blk) X(dnbr_cnt) X(dnbr_home) X(dnbr_trav) \
    X(dnbr_mrg) X(dnbr_rcnt) X(mrg_ctr) X(mrg_key) X(mrg_size) X(mrg_par) X(mrg_root) X(mrg_idx) X(mrg_recode) \
    X(mrg_rep) X(mrg_gsize) X(mrg_hist) X(mrg_rec) X(mrg_bestd) X(mrg_best) X(dmrg_b64) X(dmrg_pairs) \
    X(dmrg_pcnt) X(agg_recode) X(agg_gsize) X(agg_ctr) X(agg_scan) X(agg_offs) X(agg_mem) X(agg_wcol) X(agg_w) \
    X(shape_tab) X(shape_ctr) X(dshape_rec) X(dshape_ctr) X(dshape_rcnt) X(ol_ctr) X(ol_mask) X(ol_off) X(ol_epix) \
    X(ol_eside) X(ol_a) X(ol_b) X(ol_ring) X(ol_vtx) X(ol_roff) X(ol_jflag) X(hl_vtx) X(hl_voff) X(hl_roff) X(hl_area) X(hl_pos) \
    X(hl_cid) X(hl_ccol) X(hl_crow) X(hl_k) X(hl_v) X(hl_id) X(hl_pts) X(hl_reach) X(hl_ctr) \
    X(sp_vtx) X(sp_voff) X(sp_roff) X(sp_area) X(sp_jflag) X(sp_ctr) X(sp_keep) X(sp_pos) X(sp_ring) X(sp_arc) X(sp_pt) \
    X(sp_kv) X(sp_out) X(dp_g) X(dp_d2) X(dp_band) X(dp_runs) X(dp_piece) X(dp_scr) X(dp_tab) X(dp_ctr)

// the simplified rings between shp_simplify_source, shp_simplify_build and shp_simplify_download (simplify.h), in
// buffers of their own (sp_*): the outlines, the hulls, the neighbour table, the group lists and the shape table stay
// where they are.  src: the rings and junction flags taken by shp_simplify_source, its own instance (the hulls may
// hold other rings).
struct SimplifyState {
    int stage = 0;                  // 0 none, 1 rings known, 2 simplified
    RingSource src;
    uint32_t narcs = 0, longest = 0, rounds = 0, nshort = 0, ngroup = 0, nglobal = 0, kept = 0, rings = 0, verts = 0;
    size_t off[6] = {};             // where ring offsets, vertex offsets, vertices, areas, source rings, kept vertices lie in sp_out
    double ms[4] = {};              // device time: anchors and arcs, the rounds, the ring areas and the drop rule, the emission
};

struct shp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;     // side stream for fork/join inside one call (created lazily)
    int stream_priority = 0;
    hipEvent_t evfork = nullptr, evjoin = nullptr;
    std::string err;
    std::vector<DevBuf *> bufs;
#define X(name) DevBuf name;
    SHP_CTX_BUFS(X)
#undef X
    NbrTable nbr_tab, dnbr_tab;        // the one-GPU table and the rank's share table: neither displaces the other
    NbrLongList agg_longs;             // the long rows of the member list (nbragg.h)
    shp_ctx()
    {
#define X(name) bufs.push_back(&name);
        SHP_CTX_BUFS(X)
#undef X
        nbr_table_bufs(nbr_tab, bufs);
        nbr_table_bufs(dnbr_tab, bufs);
        nbr_long_bufs(agg_longs, bufs);
    }
    SegPointsState pts;
    ShapeState shape;
    OutlineState outline;
    unsigned long long outline_calls = 0;       // shp_outline_edges_dev calls of this context: each replaces the outlines
    HullState hull;
    SimplifyState simplify;
    DepthState depth;
    NbrState nbr;
    MrgState mrg;
    AggState agg;
    DNbrState dnbr;
    DMrgState dmrg;
    DSegPointsState dpts;
    DColourState dcol;
    uint32_t *h_pinned = nullptr;   // SHP_PINNED_BYTES of pinned host staging (small transfers)
    int64_t vario_redo = 0;         // last built-in variogram: (segment, bin) pairs recomputed in the reference's order
    std::vector<unsigned long long> vario_pairs;  // last multi-GPU variogram step: its flagged pairs
    int fit_path = 0;               // last k-means fit: 0 the fast (Lloyd) path, 1 the reference's Elkan path
    double *h_fit = nullptr;        // pinned, grow-only: the centred k-means sample
    size_t h_fit_cap = 0;
    hipEvent_t ev[16] = {};
    double timings[8] = {};
    // per-kernel device-time accounting (HIP events on this stream), see PROF_* below
    double prof_ms[PROF_N] = {};
    uint64_t prof_cnt[PROF_N] = {};
    hipEvent_t prof_ev[PROF_POOL][2] = {};
    int prof_id[PROF_POOL] = {};
    int prof_used = 0;
    uint32_t *scan_ctr = nullptr;   // device word, zero between scans: arrival counter of k_scan_local
    int gated = 0;      // this call takes part in the fill gate (tiled driver's worker calls)
    bool fill_held = false;
    bool gate_held = false;
    bool shared = false;    // a worker context without a stream of its own: it borrows one per phase
    int borrowed = 0;       // 0 = none (ctx->stream is the pool's idle stream), 1 = a fill stream, 2 = a walker stream
    hipEvent_t wb_ev[2] = {};       // around a batched walker launch this context leads (walkbatch.h)
    void *h_jobs = nullptr;         // pinned, SHP_JOBS_BYTES: the job records of such a launch
};
#define SHP_JOBS_BYTES 8192u

// Fill gate.  A tile alternates between phases that fill the GPU (HBM-bound passes over the whole
// tile: ~3.4 ms of device time) and phases that are one long dependent chain on a few wavefronts
// (the depth-first replay, the pass loop: ~35 ms).  Twenty worker streams started together stay
// in step -- every tile fills at once, then every tile waits at once, and the filling capacity
// idles a quarter of the time.  The gate lets only a few tiles be in a filling phase at any time
// (the others queue on the host), which staggers them: while some fill, the rest are in their
// chains.  Phases nearer the end of a tile go first.  SHEPSEG_FILL_MAX = 0 switches it off.
#define FILL_MAX_DEFAULT 6          // (round 4, with the shorter fit: 4 -> 6 fill and 12 -> 10 walker streams = -15 ms per step;
                                    //  fill + walker + 3 must stay <= 21 hardware queues: 7 + 12 costs 60 ms)
#define FILL_PRIOS 4
struct FillGate {
    std::mutex mu;
    std::condition_variable cv;
    int running = 0;
    int waiting[FILL_PRIOS] = {};
};
static FillGate g_fill;
// Stream counts from the queue budget.  Streams that share a hardware queue get in each other's way: a 10-ms
// walker kernel holds up the fill kernels queued behind it on the same queue (at 4 queues the fill kernels'
// union covers a third of the step, LABNOTES "walker batches"), so the pools are sized to the queues the
// process gets: Q = GPU_MAX_HW_QUEUES (read, never set; 4 when unset, the
// runtime's own default).  Three streams live beside the pools (the pool's idle stream, the main context's,
// the chain context's).  From Q = 21 the round-4 sizes hold; below, what is left of Q after those three is
// split two to one between fill and walker streams (the walker work of all ready tiles travels in one
// launch per stream, walkbatch.h, so few walker streams carry many tiles); where Q cannot hold even that,
// as at 4, the floors apply.  They were swept at 4 queues (LABNOTES "fill-stream hold"; three alternating processes a
// side, medians of the steps): 2 + 1 536-539 ms, 3 + 1 488-491, 4 + 1 477-482.  At 2 + 1 the two fill streams are
// held 0.88 of the tile phase, half of that between kernels (host round trips inside a borrow).  With four borrowers
// the kernels of different tiles overlap and each runs about twice as long, but some filling kernel is running 0.92
// of the tile phase where it was 0.77 (profiles/fill_hold_timeline_*.txt); one walker stream carries every ready tile
// in one launch and is busy 0.98 of the tile phase either way.
// Only Q = 4 was measured.  The floor also decides the fill count wherever the share above comes to less, that is
// for every Q up to 7 (Q = 7: 3 -> 4; Q = 8 gets 4 anyway): there it is extrapolated, not swept.
#define FILL_FLOOR_DEFAULT 4
#define WALK_FLOOR_DEFAULT 1
static inline int hw_queue_budget()
{
    const char *e = getenv("GPU_MAX_HW_QUEUES");
    const int q = e ? atoi(e) : 0;
    return q > 0 ? q : 4;
}
static inline int pool_default(int cls)
{
    const int q = hw_queue_budget();
    if (q >= 21) return cls ? 10 : FILL_MAX_DEFAULT;      // 6 + 10 + 3 and two to spare, as measured in round 4
    const int avail = q - 3;
    int walk = avail / 3, fill = avail - walk;
    if (walk < WALK_FLOOR_DEFAULT) walk = WALK_FLOOR_DEFAULT;
    if (fill < FILL_FLOOR_DEFAULT) fill = FILL_FLOOR_DEFAULT;
    if (fill > FILL_MAX_DEFAULT) fill = FILL_MAX_DEFAULT;
    return cls ? walk : fill;
}
static const int g_fill_max = getenv("SHEPSEG_FILL_MAX") ? atoi(getenv("SHEPSEG_FILL_MAX")) : pool_default(0);

// Stream pool.  A process gets GPU_MAX_HW_QUEUES hardware queues (4 unless the environment says otherwise)
// and streams beyond that share them, so a tile that owned a stream would hold a queue through its
// host-side waits (for the fill gate, for a pass-loop slot) as well.  A SHARED context has no stream
// of its own: inside a worker call of the tiled driver it borrows a fill stream for each GPU-filling
// phase (with the gate slot: there are as many as the gate admits) and gives it back once the phase
// has left the GPU (every phase ends in a host synchronisation, so the next phase may run on any
// other stream).  Its latency-bound kernels go through the walker batcher (g_walk below): whoever
// finds a walker stream free launches the pending jobs of all tiles at once.  More tiles than
// streams can then be in flight.  Outside worker calls a shared context uses the pool's idle stream,
// which all of them share.
struct StreamPool {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<hipStream_t> idle[2];     // 0 = fill streams, 1 = walker streams
    int made[2] = {0, 0};
    int device = -1;
    hipStream_t misc = nullptr;
};
static StreamPool g_streams;
static const int g_walk_streams = getenv("SHEPSEG_WALK_STREAMS") ? atoi(getenv("SHEPSEG_WALK_STREAMS")) : pool_default(1);
static inline int stream_pool_cap(int cls)
{
    if (cls == 1) return g_walk_streams < 1 ? 1 : g_walk_streams;
    return g_fill_max > 0 ? g_fill_max : 8;
}
static inline void stream_take(shp_ctx *ctx, int cls)
{
    std::unique_lock<std::mutex> lk(g_streams.mu);
    for (;;) {
        if (!g_streams.idle[cls].empty()) {
            ctx->stream = g_streams.idle[cls].back();
            g_streams.idle[cls].pop_back();
            break;
        }
        if (g_streams.made[cls] < stream_pool_cap(cls)) {
            hipStream_t s = nullptr;
            if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, 0) == hipSuccess) {
                g_streams.made[cls]++;
                ctx->stream = s;
                break;
            }
            (void)hipGetLastError();
            if (g_streams.made[cls] == 0) return;      // no stream of this class at all: stay on the idle stream
        }
        g_streams.cv.wait(lk);
    }
    ctx->borrowed = cls + 1;
}
// (the caller has synchronised the stream: the next borrower starts on an empty one)
static inline void stream_give(shp_ctx *ctx)
{
    if (!ctx->borrowed) return;
    {
        std::lock_guard<std::mutex> lk(g_streams.mu);
        g_streams.idle[ctx->borrowed - 1].push_back(ctx->stream);
        ctx->stream = g_streams.misc;
    }
    ctx->borrowed = 0;
    g_streams.cv.notify_all();
}
static inline bool stream_sharing(const shp_ctx *ctx) { return ctx->shared && ctx->gated; }

static inline bool fill_gating(const shp_ctx *ctx) { return g_fill_max > 0 && ctx->gated; }
static inline void fill_acquire(shp_ctx *ctx, int prio)
{
    if (ctx->fill_held || !(fill_gating(ctx) || stream_sharing(ctx))) return;
    if (fill_gating(ctx)) {
        std::unique_lock<std::mutex> lk(g_fill.mu);
        g_fill.waiting[prio]++;
        g_fill.cv.wait(lk, [&] {
            if (g_fill.running >= g_fill_max) return false;
            for (int p = prio + 1; p < FILL_PRIOS; p++)
                if (g_fill.waiting[p]) return false;
            return true;
        });
        g_fill.waiting[prio]--;
        g_fill.running++;
        ctx->gate_held = true;
        if (g_fill.running < g_fill_max) g_fill.cv.notify_all();
    }
    if (stream_sharing(ctx)) stream_take(ctx, 0);
    ctx->fill_held = true;
}
// sync: wait until the phase's kernels have left the GPU before letting the next tile in
static inline void fill_release(shp_ctx *ctx, bool sync)
{
    if (!ctx->fill_held) return;
    if (sync || ctx->borrowed) (void)hipStreamSynchronize(ctx->stream);
    stream_give(ctx);
    if (ctx->gate_held) {
        {
            std::lock_guard<std::mutex> lk(g_fill.mu);
            g_fill.running--;
        }
        ctx->gate_held = false;
        g_fill.cv.notify_all();
    }
    ctx->fill_held = false;
}
// The walker batcher: the latency-bound kernels of stream-sharing contexts (walkbatch.h).  It hands out as
// many leaderships as there are walker streams, so a leader's stream_take(ctx, 1) finds one.
static walkbatch::Batcher g_walk;
static inline walkbatch::Batcher &walk_batcher()
{
    static const bool once = [] { g_walk.set_streams(stream_pool_cap(1)); return true; }();
    (void)once;
    return g_walk;
}
struct FillScope {          // an API call never leaves with the gate or a borrowed stream held (error paths)
    shp_ctx *ctx;
    FillScope(shp_ctx *c, int gated) : ctx(c) { c->gated = gated; }
    ~FillScope()
    {
        fill_release(ctx, false);
        if (ctx->borrowed) { (void)hipStreamSynchronize(ctx->stream); stream_give(ctx); }
        ctx->gated = 0;
    }
};

// kernels whose launch durations bench.py reports against the roofline
enum { PROF_ASSIGN = 0, PROF_CCL = 1, PROF_DFS = 2, PROF_SORT = 3, PROF_SPECTRA = 4,
       PROF_SMALL_LOOP = 5, PROF_SINGLE = 6, PROF_LABEL = 7, PROF_SEGSTATS = 8 };

static inline int prof_begin(shp_ctx *ctx, int id)
{
    if (ctx->prof_used >= PROF_POOL) return -1;
    const int slot = ctx->prof_used++;
    if (!ctx->prof_ev[slot][0]) { hipEventCreate(&ctx->prof_ev[slot][0]); hipEventCreate(&ctx->prof_ev[slot][1]); }
    ctx->prof_id[slot] = id;
    hipEventRecord(ctx->prof_ev[slot][0], ctx->stream);
    return slot;
}
static inline void prof_end(shp_ctx *ctx, int slot)
{
    if (slot >= 0) hipEventRecord(ctx->prof_ev[slot][1], ctx->stream);
}
// call after the stream has been synchronised
static inline void prof_collect(shp_ctx *ctx)
{
    for (int i = 0; i < ctx->prof_used; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->prof_ev[i][0], ctx->prof_ev[i][1]) == hipSuccess) {
            ctx->prof_ms[ctx->prof_id[i]] += ms;
            ctx->prof_cnt[ctx->prof_id[i]] += 1;
        }
    }
    ctx->prof_used = 0;
}

#define SHP_FAIL(ctx, code, ...)                                  \
    do {                                                          \
        char _b[512];                                             \
        snprintf(_b, sizeof(_b), __VA_ARGS__);                    \
        (ctx)->err = _b;                                          \
        return (code);                                            \
    } while (0)

#define HIPCHK(ctx, call)                                                                   \
    do {                                                                                    \
        hipError_t _e = (call);                                                             \
        if (_e != hipSuccess)                                                               \
            SHP_FAIL(ctx, SHP_ERR_HIP, "%s:%d: %s -> %s", __FILE__, __LINE__, #call,        \
                     hipGetErrorString(_e));                                                \
    } while (0)

#define CHK(call)                    \
    do {                             \
        int _rc = (call);            \
        if (_rc != 0) return _rc;    \
    } while (0)

#define KCHK(ctx) HIPCHK(ctx, hipGetLastError())

// what a leader needs around its launch: a walker stream, the event pair, the pinned block of job records
static inline int walk_lead_begin(shp_ctx *ctx)
{
    if (!ctx->wb_ev[0]) { HIPCHK(ctx, hipEventCreate(&ctx->wb_ev[0])); HIPCHK(ctx, hipEventCreate(&ctx->wb_ev[1])); }
    if (!ctx->h_jobs) HIPCHK(ctx, hipHostMalloc(&ctx->h_jobs, SHP_JOBS_BYTES, hipHostMallocDefault));
    if (!ctx->borrowed) stream_take(ctx, 1);
    return 0;
}
// (copies a leader's error text into the batch's)
static inline void walk_msg(char *msg, size_t cap, const std::string &err)
{
    if (cap) { strncpy(msg, err.c_str(), cap - 1); msg[cap - 1] = 0; }
}

// the side stream is only created when a call really forks: every stream costs a slot in the
// hardware queues the worker streams are spread over
static inline int ensure_stream2(shp_ctx *ctx)
{
    if (ctx->stream2) return 0;
    HIPCHK(ctx, hipStreamCreateWithPriority(&ctx->stream2, hipStreamNonBlocking, ctx->stream_priority));
    return 0;
}

static inline int buf_ensure(shp_ctx *ctx, DevBuf &b, size_t bytes)
{
    if (bytes == 0) bytes = 16;
    if (b.cap >= bytes) return 0;
    static const bool regrow_log = getenv("SHEPSEG_REGROW_LOG") != nullptr;      // diagnostic: which workspace still grows
    if (regrow_log) {
        int which = -1;
        for (size_t i = 0; i < ctx->bufs.size(); i++) if (ctx->bufs[i] == &b) which = (int)i;
        fprintf(stderr, "regrow: ctx %p buffer #%d %zu -> %zu bytes\n", (void *)ctx, which, b.cap, bytes);
    }
    if (b.p) {
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        HIPCHK(ctx, hipFree(b.p));
        b.p = nullptr; b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess) {
        b.p = nullptr;
        SHP_FAIL(ctx, SHP_ERR_NOMEM, "hipMalloc(%zu) failed: %s", want, hipGetErrorString(e));
    }
    b.cap = want;
    return 0;
}

template <typename T> static inline T *bp(DevBuf &b) { return (T *)b.p; }

static inline unsigned grid_for(size_t n, unsigned block, unsigned cap = 0x7fffffffu)
{
    size_t g = (n + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (unsigned)g;
}

static inline size_t dtype_size(int dtype)
{
    switch (dtype) {
    case SHP_U8: return 1;
    case SHP_I16: case SHP_U16: return 2;
    case SHP_I32: case SHP_U32: return 4;
    default: return 0;
    }
}

// ---- device helpers ---------------------------------------------------------------------
// Pixel fetch as int64 (uniform branch on dtype; all supported dtypes fit).
__device__ __forceinline__ long long ld_px(const void *__restrict__ img, int dtype, size_t i)
{
    switch (dtype) {
    case SHP_U8: return ((const uint8_t *)img)[i];
    case SHP_I16: return ((const int16_t *)img)[i];
    case SHP_U16: return ((const uint16_t *)img)[i];
    case SHP_I32: return ((const int32_t *)img)[i];
    default: return ((const uint32_t *)img)[i];
    }
}

// relaxed agent-scope load: served by L2, where the atomics land (a plain load may be answered
// by a stale line of the CU's vector L1)
#define L2LOAD(ptr) __hip_atomic_load((ptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// Typed pixel fetch for kernels whose inner loops issue many loads: with the pixel type a template
// parameter the loads of an unrolled loop sit in one basic block and overlap, whereas the
// run-time switch of ld_px puts every load behind its own branch.
template <int DT> struct PxT { typedef uint32_t type; };
template <> struct PxT<SHP_U8> { typedef uint8_t type; };
template <> struct PxT<SHP_I16> { typedef int16_t type; };
template <> struct PxT<SHP_U16> { typedef uint16_t type; };
template <> struct PxT<SHP_I32> { typedef int32_t type; };
template <int DT> __device__ __forceinline__ long long ld_t(const void *__restrict__ img, size_t i)
{
    return ((const typename PxT<DT>::type *)img)[i];
}
// expands STMT once per pixel type with `DT` a compile-time constant
#define DISPATCH_DTYPE(dtype, ...)                                    \
    switch (dtype) {                                                  \
    case SHP_U8: { constexpr int DT = SHP_U8; __VA_ARGS__; } break;          \
    case SHP_I16: { constexpr int DT = SHP_I16; __VA_ARGS__; } break;        \
    case SHP_U16: { constexpr int DT = SHP_U16; __VA_ARGS__; } break;        \
    case SHP_I32: { constexpr int DT = SHP_I32; __VA_ARGS__; } break;        \
    default: { constexpr int DT = SHP_U32; __VA_ARGS__; } break;             \
    }

// Where a tile's pixels live: band b, tile pixel p (row-major in a tile xs pixels wide) is element
// b * bstride + origin + (p / xs) * pitch + p % xs of the image buffer.  A compact tile image has
// pitch == xs, bstride == pixels per band, origin == 0; a window of a resident raster is read in
// place (pitch = raster width, origin = first pixel of the window) instead of being copied out.
struct ImgGeom {
    size_t bstride, origin;
    uint32_t pitch, xs;
    float inv_xs;
};
static inline ImgGeom geom_compact(size_t n, uint32_t xs)
{
    return ImgGeom{n, 0, xs, xs, xs ? 1.0f / (float)xs : 0.0f};
}
__device__ __forceinline__ size_t geom_off(const ImgGeom &g, uint32_t p)
{
    if (g.pitch == g.xs) return g.origin + p;
    // row = p / xs without an integer division: the float quotient is within 0.02 of the true one
    // (p / xs < 65536 rows, three roundings of 2^-24 each), so its floor is off by at most one
    uint32_t r = (uint32_t)((float)p * g.inv_xs);
    uint32_t rem = p - r * g.xs;
    if (rem >= g.xs) {
        if ((int32_t)rem < 0) { r -= 1u; rem += g.xs; }
        else { r += 1u; rem -= g.xs; }
    }
    return g.origin + (size_t)r * g.pitch + rem;
}

// ---- workgroup-local aggregation of per-id minima / maxima ---------------------------------------
// Atomics on one address serialise at L2, and the pixels that update one id's bounding box sit
// close together.  Kernels that reduce per-id extremes therefore walk 2-D patches (AGG_ROWS x 64
// pixels per 256-thread workgroup, a wavefront per image row so loads stay coalesced), combine
// candidates in a small LDS hash table with LDS atomics, and issue one global atomic per
// (workgroup, id, field).  A full table sends the candidate straight to global memory.
#define AGG_SLOTS 128u
#define AGG_ROWS 32u
struct AggTable {
    uint32_t key[AGG_SLOTS];        // 0 = empty
    uint32_t v[3][AGG_SLOTS];
};
__device__ __forceinline__ void agg_init(AggTable &t, uint32_t i0, uint32_t i1, uint32_t i2)
{
    for (uint32_t i = threadIdx.x; i < AGG_SLOTS; i += 256u) {
        t.key[i] = 0u; t.v[0][i] = i0; t.v[1][i] = i1; t.v[2][i] = i2;
    }
}
// slot of `key` (claimed if new) or -1 when the table is full
__device__ __forceinline__ int agg_slot(AggTable &t, uint32_t key)
{
    uint32_t h = (key * 2654435761u) >> 25;
    for (uint32_t probe = 0; probe < AGG_SLOTS; probe++) {
        const uint32_t old = atomicCAS(&t.key[h], 0u, key);
        if (old == 0u || old == key) return (int)h;
        h = (h + 1u) & (AGG_SLOTS - 1u);
    }
    return -1;
}

__device__ __forceinline__ unsigned lane_id() { return threadIdx.x & 63u; }
__device__ __forceinline__ unsigned long long lanemask_lt()
{
    return (1ull << lane_id()) - 1ull;
}
