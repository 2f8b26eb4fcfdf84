// fit_layout.h -- where everything lives in the k-means fit's buffers, as plain host arithmetic.
//
// The fit's drivers (kmeans.h: run_kmeans_fit, fit_elkan.h: run_fit_elkan) carve a handful of grow-only
// buffers of the context into regions.  Every offset and every total is computed here and nowhere
// else: the drivers call buf_ensure with the totals and take each pointer from these structs.  All
// offsets are in BYTES from the buffer's start.
//
// No GPU types in here, so that a host-only program can check the layouts
// (tests/native/fit_layout_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

// Words between the fit's two label arrays.  The sharded E-step all-gathers the labels IN PLACE:
// world ranks x ceil(n / world) words, i.e. up to world - 1 words past the first array's n.  They land
// in this gap, which is why run_fit_elkan shards over at most FIT_SHARD_MAX ranks and checks
// world * ceil(n / world) <= FitLayout::lab_words before its first launch.
#define FIT_LAB_GAP 128u
#define FIT_SHARD_MAX 64
// sizeof(FitCtl), sizeof(ElkCtl) (static_asserts next to the structs)
#define FIT_CTL_BYTES 24u
#define ELK_CTL_BYTES 24u
// bytes of the context's pinned block in front of its mirror words (common.h: PIN_MIRROR * 4)
#define FIT_PIN_STAGE_BYTES ((1u << 20) - 256u)

// One extent of a buffer: [off, off + bytes)
struct FitRegion { size_t off, bytes; };
template <class T> static inline T *fit_at(void *base, const FitRegion &r) { return (T *)((char *)base + r.off); }

// The buffers run_kmeans_fit owns: the sample, the labels, the E-step operands and the Lloyd loop's small block.
struct FitLayout {
    // ctx->fit_x: the centred sample (n rows of nb float64) | a distance per sample (the empty-cluster finish)
    FitRegion x, dist;
    size_t x_total;
    // ctx->fit_lab: labels A | FIT_LAB_GAP words | labels B | FitCtl
    FitRegion labA, labB, ctl;
    size_t lab_total;
    size_t lab_words;           // words writable from labA before labB begins: n + FIT_LAB_GAP
    // ctx->cen: m2c (-2 c) | cnorm (|c|^2) | C
    FitRegion m2c, cnorm, C;
    size_t cen_total;
    // ctx->fit_part, the Lloyd form: row-order sums | their counts as float64 (unused by Lloyd) | S | w (k + 2) |
    // counts | list offsets (k + 1) and the word k_elk_offsets zeroes
    FitRegion sums, cntd, S, w, counts, off;
    size_t part_total;
    // the pinned block: FitCtl | m2c, cnorm, C on their way up (C alone on its way down)
    FitRegion pin_ctl, pin_up;
    size_t pin_total;           // must not exceed the pinned block
};

static inline FitLayout fit_layout(uint32_t n, int nb, int k)
{
    const size_t kn = (size_t)k * nb, K = (size_t)k, N = n;
    FitLayout L;
    L.x = {0, N * nb * 8};
    L.dist = {L.x.bytes, N * 8};
    L.x_total = N * nb * 8 + N * 8;
    L.labA = {0, N * 4};
    L.labB = {(N + FIT_LAB_GAP) * 4, N * 4};
    L.ctl = {L.labB.off + N * 4, FIT_CTL_BYTES};
    L.lab_total = N * 4 * 2 + 64 + 1024;
    L.lab_words = N + FIT_LAB_GAP;
    L.m2c = {0, kn * 8};
    L.cnorm = {kn * 8, K * 8};
    L.C = {(kn + K) * 8, kn * 8};
    L.cen_total = (kn + K) * 8 * 2;
    L.sums = {0, kn * 8};
    L.cntd = {kn * 8, K * 8};
    L.S = {(kn + K) * 8, kn * 8};
    L.w = {(2 * kn + K) * 8, (K + 2) * 8};
    L.counts = {(2 * kn + 2 * K + 2) * 8, K * 4};
    L.off = {L.counts.off + K * 4, (K + 2) * 4};
    L.part_total = (kn + K) * 8 * 3 + (2 * K + 4) * 4 + 512;
    L.pin_ctl = {0, FIT_CTL_BYTES};
    L.pin_up = {64, (2 * kn + K) * 8};
    L.pin_total = (2 * kn + 2 * K + 8) * 8;
    return L;
}

// The buffers of the reference's algorithm (fit_elkan.h).  lazy: float32 brackets + stamps + the history of
// shifts and centres (fit_bounds.h); else the exact table of lower bounds, cluster-major.
struct ElkLayout {
    bool lazy;
    size_t hist_rows;           // iterations the history has room for: max_iter + 3
    // ctx->fit_lb, lazy: ub | cmask | mmask | cs | cum | cen | csT | diag (8 counters) | A (256-aligned) | stamps
    // ctx->fit_lb, table: lb (k x n) | ub
    FitRegion lb, ub, cmask, mmask, cs, cum, cen, csT, diag, A, stamps;
    size_t lb_total;
    // ctx->fit_part, the Elkan form: C | cshift | half | next | S | cnt | scratch (3k) | ElkCtl | off (k + 1) | done
    FitRegion C, cshift, half, next, S, cnt, scratch, ctl, off, done;
    size_t part_total;
    // host staging: C, cshift, half, next on their way up | S, cnt on their way down | ElkCtl
    FitRegion up, down, stage_ctl;
    size_t stage_doubles;       // what a pageable stand-in is sized by
    bool stage_pinned;          // it fits the context's pinned block
};

static inline ElkLayout elk_layout(uint32_t n, int nb, int k, int max_iter, bool lazy)
{
    const size_t kn = (size_t)k * nb, K = (size_t)k, N = n;
    ElkLayout L{};
    L.lazy = lazy;
    L.hist_rows = (size_t)max_iter + 3;
    if (lazy) {
        const size_t hr = L.hist_rows, hist_doubles = hr * (3 * K + kn);
        L.ub = {0, N * 8};
        L.cmask = {N * 8, N * 8};
        L.mmask = {N * 16, N * 8};
        L.cs = {N * 24, hr * K * 8};
        L.cum = {L.cs.off + hr * K * 8, hr * K * 8};
        L.cen = {L.cum.off + hr * K * 8, hr * kn * 8};
        L.csT = {L.cen.off + hr * kn * 8, hr * K * 8};
        L.diag = {L.csT.off + hr * K * 8, 64};
        // (device allocations are 256-aligned, so the offset's alignment is the pointer's)
        L.A = {(L.diag.off + 64 + 255) & ~(size_t)255, N * K * 4};
        L.stamps = {L.A.off + N * K * 4, N * K * 2};
        L.lb_total = N * K * 6 + 512 + N * 8 * 3 + hist_doubles * 8 + 64;
    } else {
        L.lb = {0, K * N * 8};
        L.ub = {K * N * 8, N * 8};
        L.lb_total = (K * N + N) * 8;
    }
    const size_t small_doubles = kn + K + K * K + K + kn + K + 3 * K;
    L.C = {0, kn * 8};
    L.cshift = {kn * 8, K * 8};
    L.half = {(kn + K) * 8, K * K * 8};
    L.next = {L.half.off + K * K * 8, K * 8};
    L.S = {L.next.off + K * 8, kn * 8};
    L.cnt = {L.S.off + kn * 8, K * 8};
    L.scratch = {L.cnt.off + K * 8, 3 * K * 8};
    L.ctl = {small_doubles * 8, ELK_CTL_BYTES};
    L.off = {L.ctl.off + ELK_CTL_BYTES, (K + 1) * 4};
    L.done = {L.off.off + (K + 1) * 4, 4};
    L.part_total = small_doubles * 8 + ELK_CTL_BYTES + (K + 4) * 4 + 64;
    const size_t up_doubles = kn + K + K * K + K, dn_doubles = kn + K;
    L.up = {0, up_doubles * 8};
    L.down = {up_doubles * 8, dn_doubles * 8};
    L.stage_ctl = {(up_doubles + dn_doubles) * 8, ELK_CTL_BYTES};
    L.stage_doubles = up_doubles + dn_doubles + 8;
    L.stage_pinned = (up_doubles + dn_doubles) * 8 + ELK_CTL_BYTES + 256 <= (size_t)FIT_PIN_STAGE_BYTES;
    return L;
}

// rows per rank of the E-step sharded over `world` ranks
static inline uint32_t fit_shard_rows(uint32_t n, int world)
{
    return (n + (uint32_t)world - 1u) / (uint32_t)world;
}
