// Host-only check of the k-means fit's buffer layouts (pyshepseg_amd/csrc/fit_layout.h): the regions of one
// buffer are disjoint and inside its total, every float64 / 64-bit region is 8-aligned, the float32 brackets
// are 256-aligned, the totals are the formulas the allocations have always had, and the sharded E-step's in-place
// all-gather fits the gap behind the first label array at every world size the fit shards over.
// Built with AddressSanitizer + UBSan by tests/test_fit_layout_host.py; prints "ok".
#include "../../pyshepseg_amd/csrc/fit_layout.h"
#include <algorithm>
#include <stdio.h>
#include <stdlib.h>
#include <unistd.h>
#include <vector>

static int failures = 0;
#define EXPECT(cond, ...)                                                          \
    do {                                                                           \
        if (!(cond)) {                                                             \
            failures++;                                                            \
            fprintf(stderr, "%s:%d: %s: ", __FILE__, __LINE__, #cond);             \
            fprintf(stderr, __VA_ARGS__);                                          \
            fprintf(stderr, "\n");                                                 \
        }                                                                          \
    } while (0)

struct Named { const char *name; FitRegion r; size_t align; };

// regions sorted by offset: each aligned, none empty unless its count is, none overlapping, all inside total
static void check_buffer(const char *buf, std::vector<Named> regs, size_t total, const char *shape)
{
    std::sort(regs.begin(), regs.end(), [](const Named &a, const Named &b) { return a.r.off < b.r.off; });
    size_t end = 0;
    for (const Named &g : regs) {
        EXPECT(g.r.off % g.align == 0, "%s %s.%s at %zu is not %zu-aligned", shape, buf, g.name, g.r.off, g.align);
        EXPECT(g.r.off >= end, "%s %s.%s at %zu overlaps the region before it (ends %zu)", shape, buf, g.name, g.r.off, end);
        EXPECT(g.r.bytes > 0, "%s %s.%s is empty", shape, buf, g.name);
        end = g.r.off + g.r.bytes;
        EXPECT(end <= total, "%s %s.%s ends at %zu beyond the total %zu", shape, buf, g.name, end, total);
    }
}

static void check_fit(uint32_t n32, int nb, int k)
{
    char shape[96];
    snprintf(shape, sizeof shape, "(n=%u nb=%d k=%d)", n32, nb, k);
    const FitLayout L = fit_layout(n32, nb, k);
    const size_t n = n32, kn = (size_t)k * nb, K = (size_t)k;
    EXPECT(L.x_total == 8 * n * nb + 8 * n, "%s fit_x %zu", shape, L.x_total);
    EXPECT(L.lab_total == 8 * n + 64 + 1024, "%s fit_lab %zu", shape, L.lab_total);
    EXPECT(L.cen_total == 16 * (kn + K), "%s cen %zu", shape, L.cen_total);
    EXPECT(L.part_total == 24 * (kn + K) + 4 * (2 * K + 4) + 512, "%s fit_part %zu", shape, L.part_total);
    EXPECT(L.pin_total == 8 * (2 * kn + 2 * K + 8), "%s pinned %zu", shape, L.pin_total);
    EXPECT(L.lab_words == n + FIT_LAB_GAP, "%s lab_words %zu", shape, L.lab_words);
    EXPECT(L.labA.off == 0 && L.labB.off == 4 * L.lab_words, "%s labB at %zu", shape, L.labB.off);
    EXPECT(L.x.off == 0 && L.x.bytes == 8 * n * nb && L.dist.bytes == 8 * n, "%s X / dist sizes", shape);
    EXPECT(L.labA.bytes == 4 * n && L.labB.bytes == 4 * n, "%s label sizes", shape);
    // m2c | cnorm | C go up in ONE copy of 2kn + k doubles, from a pinned run of the same shape
    EXPECT(L.m2c.off == 0 && L.cnorm.off == 8 * kn && L.C.off == 8 * (kn + K), "%s m2c | cnorm | C adjacent", shape);
    EXPECT(L.pin_up.bytes == 8 * (2 * kn + K), "%s pinned upload run", shape);
    check_buffer("fit_x", {{"X", L.x, 8}, {"dist", L.dist, 8}}, L.x_total, shape);
    check_buffer("fit_lab", {{"labA", L.labA, 4}, {"labB", L.labB, 4}, {"ctl", L.ctl, 8}}, L.lab_total, shape);
    check_buffer("cen", {{"m2c", L.m2c, 8}, {"cnorm", L.cnorm, 8}, {"C", L.C, 8}}, L.cen_total, shape);
    check_buffer("fit_part", {{"sums", L.sums, 8}, {"cntd", L.cntd, 8}, {"S", L.S, 8}, {"w", L.w, 8},
                              {"counts", L.counts, 4}, {"off", L.off, 4}}, L.part_total, shape);
    check_buffer("pinned", {{"ctl", L.pin_ctl, 8}, {"up", L.pin_up, 8}}, L.pin_total, shape);
    EXPECT(L.off.bytes == 4 * (K + 2), "%s k + 1 offsets and the zeroed word", shape);
}

static void check_elk(uint32_t n32, int nb, int k, int max_iter, bool lazy)
{
    char shape[128];
    snprintf(shape, sizeof shape, "(n=%u nb=%d k=%d max_iter=%d %s)", n32, nb, k, max_iter, lazy ? "lazy" : "table");
    const ElkLayout L = elk_layout(n32, nb, k, max_iter, lazy);
    const size_t n = n32, kn = (size_t)k * nb, K = (size_t)k, hr = (size_t)max_iter + 3;
    EXPECT(L.lazy == lazy && L.hist_rows == hr, "%s form", shape);
    if (lazy) {
        EXPECT(L.lb_total == 6 * n * K + 512 + 24 * n + 8 * hr * (3 * K + kn) + 64, "%s fit_lb %zu", shape, L.lb_total);
        EXPECT(L.A.off % 256 == 0, "%s A at %zu", shape, L.A.off);
        EXPECT(L.A.bytes == 4 * n * K && L.stamps.bytes == 2 * n * K && L.diag.bytes == 64, "%s A / stamps / diag sizes", shape);
        EXPECT(L.cs.bytes == 8 * hr * K && L.cum.bytes == 8 * hr * K && L.csT.bytes == 8 * hr * K && L.cen.bytes == 8 * hr * kn,
               "%s history sizes", shape);
        check_buffer("fit_lb", {{"ub", L.ub, 8}, {"cmask", L.cmask, 8}, {"mmask", L.mmask, 8}, {"cs", L.cs, 8}, {"cum", L.cum, 8},
                                {"cen", L.cen, 8}, {"csT", L.csT, 8}, {"diag", L.diag, 8}, {"A", L.A, 256}, {"stamps", L.stamps, 2}},
                     L.lb_total, shape);
    } else {
        EXPECT(L.lb_total == 8 * (K * n + n), "%s fit_lb %zu", shape, L.lb_total);
        EXPECT(L.lb.bytes == 8 * K * n, "%s lb size", shape);
        check_buffer("fit_lb", {{"lb", L.lb, 8}, {"ub", L.ub, 8}}, L.lb_total, shape);
    }
    EXPECT(L.ub.bytes == 8 * n, "%s ub size", shape);
    EXPECT(L.part_total == 8 * (2 * kn + 6 * K + K * K) + 24 + 4 * (K + 4) + 64, "%s fit_part %zu", shape, L.part_total);
    check_buffer("fit_part", {{"C", L.C, 8}, {"cshift", L.cshift, 8}, {"half", L.half, 8}, {"next", L.next, 8}, {"S", L.S, 8},
                              {"cnt", L.cnt, 8}, {"scratch", L.scratch, 8}, {"ctl", L.ctl, 8}, {"off", L.off, 4}, {"done", L.done, 4}},
                 L.part_total, shape);
    // C | cshift | half | next go up in one copy, S | cnt come down in one
    EXPECT(L.C.off == 0 && L.cshift.off == 8 * kn && L.half.off == 8 * (kn + K) && L.next.off == 8 * (kn + K + K * K),
           "%s C | cshift | half | next adjacent", shape);
    EXPECT(L.cnt.off == L.S.off + 8 * kn, "%s S | cnt adjacent", shape);
    EXPECT(L.up.bytes == 8 * (kn + 2 * K + K * K) && L.down.bytes == 8 * (kn + K), "%s staging sizes", shape);
    EXPECT(L.scratch.bytes == 24 * K, "%s scratch size", shape);
    const size_t stage = L.up.bytes + L.down.bytes + 24;
    check_buffer("staging", {{"up", L.up, 8}, {"down", L.down, 8}, {"ctl", L.stage_ctl, 8}}, stage, shape);
    EXPECT(L.stage_doubles * 8 >= stage, "%s the pageable stand-in holds %zu of %zu bytes", shape, L.stage_doubles * 8, stage);
    EXPECT(L.stage_pinned == (stage + 256 <= ((size_t)1 << 20) - 256), "%s pinned decision", shape);
}

int main()
{
    alarm(30);
    static const struct { uint32_t n; int nb, k; } shapes[] = {
        {1, 1, 1}, {64, 2, 64}, {65, 1, 65}, {700, 3, 300}, {3000, 70, 5}, {4000, 8, 65}, {1000000, 6, 60}, {1000000, 10, 60}};
    static const int max_iters[] = {0, 1, 300, 64999};
    int lazy_seen = 0, table_seen = 0;
    for (const auto &s : shapes) {
        check_fit(s.n, s.nb, s.k);
        for (int mi : max_iters) {
            // (the lazy form exists for k <= 64, nb <= 64, max_iter < 65000: fit_elkan.h elk_plan; the table form always)
            if (s.k <= 64 && s.nb <= 64 && mi < 65000) { check_elk(s.n, s.nb, s.k, mi, true); lazy_seen++; }
            check_elk(s.n, s.nb, s.k, mi, false);
            table_seen++;
        }
    }
    EXPECT(lazy_seen == 16 && table_seen == 32, "forms covered: %d lazy, %d table", lazy_seen, table_seen);
    // the in-place all-gather of the sharded E-step writes world * ceil(n / world) words from the first label array
    for (int world = 2; world <= FIT_SHARD_MAX; world++)
        for (uint32_t n = (uint32_t)world; n <= (uint32_t)world + 200u; n++) {
            const size_t words = (size_t)world * fit_shard_rows(n, world);
            EXPECT(fit_shard_rows(n, world) == (n + world - 1) / world, "rows per rank at n=%u world=%d", n, world);
            EXPECT(words <= (size_t)n + FIT_LAB_GAP, "n=%u world=%d: %zu words gathered", n, world, words);
            EXPECT(words <= fit_layout(n, 1, 1).lab_words, "n=%u world=%d: %zu words gathered", n, world, words);
        }
    EXPECT(FIT_LAB_GAP == 128u && FIT_SHARD_MAX == 64, "the gap and the rank cap");
    if (failures) { fprintf(stderr, "%d checks failed\n", failures); return 1; }
    printf("ok\n");
    return 0;
}
