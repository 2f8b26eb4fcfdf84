// rings.h -- where the rings of a SegmentOutlines come from, for everything that is built on them (hull.h, simplify.h).
//
// A set of rings is what outline.h leaves: vertices as (row, col) int64 pairs, int64 vertex offsets per ring, int64 ring
// offsets per id, ringArea2 and, after a junction trace, a flag per vertex.  A user of rings either reads the trace's
// own, still in the context's outline buffers (RESIDENT: nothing is copied, and they must still be the outlines of
// RingSource::outline_serial when they are read), or has host arrays uploaded into buffers of its own, which it names
// in a RingBufs.  Every user keeps its own RingSource (common.h, next to the states that hold one) and its own upload
// buffers, so two users may hold different rings at the same time; nothing here is shared between them but the code.
//
// The four steps, each written here only: ring_upload_need (the bytes an upload would still allocate),
// ring_source_take (resident or uploaded, the upload timed by events), ring_source_current (are the resident rings
// still the ones taken) and ring_view (the pointers the kernels read, RingView).
#pragma once
#include "common.h"
#include "outline.h"

// the device view of a set of rings; the sources of hull.h and simplify.h begin with it
struct RingView {
    const longlong2 *vtx;           // nv vertices (row, col)
    const long long *voff;          // nr + 1
    const long long *roff;          // S + 2
    const long long *area2;         // nr
    const uint8_t *jflag;           // nv, NULL where the user takes no flags
    uint32_t nv, nr, S;
};

// the last k < n with a[k] <= v, for ascending a with a[0] <= v: the ring of vertex v (a = voff, n = nr), the id of
// ring k (a = roff, n = S + 1)
__device__ __forceinline__ uint32_t ring_last_le(const long long *__restrict__ a, uint32_t n, long long v)
{
    uint32_t lo = 0u, hi = n;               // a[lo] <= v < a[hi] (a[n] beyond every v)
    while (hi - lo > 1u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (a[mid] <= v) lo = mid; else hi = mid;
    }
    return lo;
}

// ---- host side --------------------------------------------------------------------------------------------
// a user's own upload buffers; jflag: NULL for a user that takes no flags
struct RingBufs {
    DevBuf &vtx, &voff, &roff, &area;
    DevBuf *jflag;
};

// what the upload buffers still have to grow by for nv vertices in nr rings of the ids 0 .. S
static size_t ring_upload_need(const RingBufs &b, size_t nv, size_t nr, size_t S)
{
    return ol_grown(b.vtx, nv * 16) + ol_grown(b.voff, (nr + 1) * 8) + ol_grown(b.area, nr * 8) + ol_grown(b.roff, (S + 2) * 8) +
           (b.jflag ? ol_grown(*b.jflag, nv) : 0);
}

// the rings to work on: the context's traced outlines in place (ring_offsets NULL), or host arrays uploaded into b
static int ring_source_take(shp_ctx *ctx, RingSource &src, const RingBufs &b, const int64_t *ring_offsets, const int64_t *vertex_offsets,
                            const int64_t *vertices, const int64_t *ring_area2, const uint8_t *junction, uint32_t S, uint32_t nr,
                            uint32_t nv, double *upload_ms_out)
{
    hipStream_t st = ctx->stream;
    src = RingSource{};
    if (!ring_offsets) {
        const OutlineState &o = ctx->outline;
        src.resident = true;
        src.outline_serial = o.serial;
        src.S = o.S; src.nr = o.rings; src.nv = o.verts;
        return 0;
    }
    CHK(buf_ensure(ctx, b.roff, ((size_t)S + 2) * 8));
    CHK(buf_ensure(ctx, b.voff, ((size_t)nr + 1) * 8));
    CHK(buf_ensure(ctx, b.area, (size_t)nr * 8));
    CHK(buf_ensure(ctx, b.vtx, (size_t)nv * 16));
    if (b.jflag) CHK(buf_ensure(ctx, *b.jflag, nv));
    HIPCHK(ctx, hipEventRecord(ctx->ev[0], st));
    HIPCHK(ctx, hipMemcpyAsync(b.roff.p, ring_offsets, ((size_t)S + 2) * 8, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(b.voff.p, vertex_offsets, ((size_t)nr + 1) * 8, hipMemcpyHostToDevice, st));
    if (nr) HIPCHK(ctx, hipMemcpyAsync(b.area.p, ring_area2, (size_t)nr * 8, hipMemcpyHostToDevice, st));
    if (nv) HIPCHK(ctx, hipMemcpyAsync(b.vtx.p, vertices, (size_t)nv * 16, hipMemcpyHostToDevice, st));
    if (nv && b.jflag) HIPCHK(ctx, hipMemcpyAsync(b.jflag->p, junction, nv, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipEventRecord(ctx->ev[1], st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    if (upload_ms_out) *upload_ms_out = ol_elapsed(ctx->ev[0], ctx->ev[1]);
    src.S = S; src.nr = nr; src.nv = nv;
    return 0;
}

// uploaded rings stay until the next upload; resident ones only while the context's outlines are those of the serial
static bool ring_source_current(const shp_ctx *ctx, const RingSource &src)
{
    return !src.resident || (ctx->outline.stage == 2 && ctx->outline.serial == src.outline_serial);
}

// what the kernels read: into the outline buffers (the only place outside outline.h that knows where the int64 vertex
// offsets and the areas lie in ol_ring) or into b
static RingView ring_view(shp_ctx *ctx, const RingSource &src, const RingBufs &b)
{
    if (!src.resident)
        return RingView{bp<longlong2>(b.vtx), bp<long long>(b.voff), bp<long long>(b.roff), bp<long long>(b.area),
                        b.jflag ? bp<uint8_t>(*b.jflag) : nullptr, src.nv, src.nr, src.S};
    const char *ring = (const char *)ctx->ol_ring.p;
    return RingView{bp<longlong2>(ctx->ol_vtx), (const long long *)(ring + ctx->outline.voff64_at), bp<long long>(ctx->ol_roff),
                    (const long long *)(ring + ctx->outline.area_at), b.jflag ? bp<uint8_t>(ctx->ol_jflag) : nullptr, src.nv, src.nr,
                    src.S};
}
