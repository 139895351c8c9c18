// plan_correlate and corr_term of plan.h on a machine without a GPU:
//   correlate_check plan    reads lines "rows k limit x_bytes y_bytes what" from stdin and prints, for each, "refused" or
//                           n levels level_n[0..3] tie_grid and the bytes of x, y, one key buffer, one payload buffer, the table,
//                           the block sums, the histograms, the runs, the starts, one doubled-rank buffer, their number, the NaN
//                           counts, the two partial-sum buffers, and all of them together
//   correlate_check sweep   walks the moment kernels' order on the host for a set of N: every level, every tile, every lane,
//                           the way the kernels enumerate them, and exits non-zero on a broken invariant
//   correlate_check sum     reads a count and that many float64 bit patterns (hexadecimal) from stdin, adds them in the plan's
//                           order -- the kernels' loops with corr_term, on the host -- and prints the sum's bit pattern
// Built with the host compiler and -fsanitize=address,undefined (make correlate_check).
#include "plan.h"

#include <inttypes.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static int g_failures = 0;
static void fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "correlate_check: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    g_failures++;
}

static const int64_t MAX_GRID_X = 2147483647;

// one level of moment_f64_kernel on the host: the same loops over tiles, lanes and terms, the same tree
static std::vector<double> sum_level(const std::vector<double> &in)
{
    const uint64_t n = in.size(), tiles = (n + CORR_TILE - 1) / CORR_TILE;
    std::vector<double> out((size_t)tiles);
    for (uint64_t t = 0; t < tiles; t++) {
        double lane[CORR_LANES];
        for (int j = 0; j < CORR_LANES; j++) {
            double a = 0.0;
            for (int i = 0; i < CORR_TILE / CORR_LANES; i++) {
                const uint64_t e = corr_term(t, j, i);
                if (e < n) a = a + in[(size_t)e];
            }
            lane[j] = a;
        }
        for (int off = CORR_LANES / 2; off > 0; off >>= 1)
            for (int j = 0; j < off; j++) lane[j] = lane[j] + lane[j + off];
        out[(size_t)t] = lane[0];
    }
    return out;
}

static void check_plan(const CorrelatePlan &p, int64_t rows, int64_t k, int64_t limit, int xb, int yb, int what)
{
    const int64_t n = rows * limit;
    const size_t un = (size_t)n;
    if (p.n != n || p.what != what) return fail("rows %lld limit %lld: n / what", (long long)rows, (long long)limit);
    // the levels: each the tiles of the one before, the last one a single sum, none a grid the launch refuses
    if (p.levels < 1 || p.levels > CORR_MAX_LEVELS || p.level_n[0] != n || p.level_n[p.levels] != 1) fail("n %lld: %d levels", (long long)n, p.levels);
    for (int l = 0; l < p.levels; l++) {
        if (p.level_n[l + 1] != (p.level_n[l] + CORR_TILE - 1) / CORR_TILE) fail("n %lld: level %d", (long long)n, l);
        if (p.level_n[l] < 2 || p.level_n[l + 1] < 1 || p.level_n[l + 1] > MAX_GRID_X) fail("n %lld: level %d has %lld terms", (long long)n, l, (long long)p.level_n[l]);
    }
    if (p.tie_grid < 1 || p.tie_grid > CORR_GRID) fail("n %lld: tie_grid %lld", (long long)n, (long long)p.tie_grid);
    RankPlan rx, ry;
    if (!plan_rank(rows, k, limit, xb, false, true, false, &rx)) return fail("n %lld: the rank refuses what the correlation accepts", (long long)n);
    ry = rx;
    if (yb && !plan_rank(rows, k, limit, yb, false, true, false, &ry)) return fail("n %lld: the rank refuses y", (long long)n);
    const bool sorts = what != KNN_CORR_PEARSON;
    const int wb = std::max(xb, yb);
    const size_t ntiles = (un + RANK_TILE - 1) / RANK_TILE, entry = 3 * (size_t)((what & KNN_CORR_SPEARMAN) ? 16 : 8);
    const size_t want[] = {rx.scores_bytes, yb ? ry.scores_bytes : 0, sorts ? un * wb : 0, sorts ? un * 4 : 0, sorts ? ntiles * 1024 : 0,
                           sorts ? std::max((ntiles * 256 + RANK_SCAN_BLOCK - 1) / RANK_SCAN_BLOCK, (un + RANK_SCAN_BLOCK - 1) / RANK_SCAN_BLOCK) * 4 : 0,
                           sorts ? (size_t)wb * 1024 : 0, sorts ? un * 4 : 0, sorts ? (un + 1) * 4 : 0, sorts ? un * (what ? 4 : 8) : 0, sorts ? (size_t)16 : 0,
                           what ? (size_t)p.level_n[1] * entry : 0, what ? (size_t)p.level_n[2] * entry : 0};
    const size_t got[] = {p.x_bytes, p.y_bytes, p.keys_bytes, p.pay_bytes, p.table_bytes, p.partial_bytes, p.hist_bytes, p.run_bytes, p.start_bytes,
                          p.rank2_bytes, p.nan_bytes, p.moment_a_bytes, p.moment_b_bytes};
    const size_t times[] = {1, 1, 2, 2, 1, 1, 1, 1, 1, (size_t)p.rank2_buffers, 1, 1, 1};
    size_t sum = 0;
    for (int i = 0; i < 13; i++) {
        if (want[i] != got[i]) fail("rows %lld k %lld limit %lld what %d: buffer %d has %zu bytes, not %zu", (long long)rows, (long long)k, (long long)limit, what, i, got[i], want[i]);
        sum += times[i] * got[i];
    }
    if (p.rank2_buffers != (sorts ? (what ? 2 : 1) : 0)) fail("what %d: %d doubled-rank buffers", what, p.rank2_buffers);
    if (sum != p.resident_bytes) fail("n %lld what %d: the buffers add up to %zu, resident_bytes is %zu", (long long)n, what, sum, p.resident_bytes);
    // what the kernels index: the scan's block sums cover the N flags, the sorts' buffers hold either array
    if (sorts && p.partial_bytes < (un + RANK_SCAN_BLOCK - 1) / RANK_SCAN_BLOCK * 4) fail("n %lld: block sums short of the flags", (long long)n);
    if (sorts && (p.keys_bytes < rx.keys_bytes || p.keys_bytes < ry.keys_bytes || p.hist_bytes < rx.hist_bytes || p.hist_bytes < ry.hist_bytes ||
                  p.table_bytes < rx.table_bytes || p.partial_bytes < rx.partial_bytes || p.partial_bytes < ry.partial_bytes))
        fail("n %lld: a shared buffer is smaller than one of the sorts needs", (long long)n);
    // the partial sums: level l writes 3 * level_n[l + 1] entries into a (l even) or b (l odd)
    for (int l = 0; what && l < p.levels; l++) {
        const size_t need = (size_t)p.level_n[l + 1] * entry, have = (l & 1) ? p.moment_b_bytes : p.moment_a_bytes;
        if (need > have) fail("n %lld: level %d writes %zu bytes into %zu", (long long)n, l, need, have);
    }
}

// every term of a level is taken exactly once, by the lane and step corr_term names, and no tile is empty
static void walk_order(int64_t n)
{
    std::vector<uint8_t> seen((size_t)n, 0);
    const uint64_t tiles = ((uint64_t)n + CORR_TILE - 1) / CORR_TILE;
    for (uint64_t t = 0; t < tiles; t++) {
        int64_t in_tile = 0;
        for (int j = 0; j < CORR_LANES; j++) {
            uint64_t prev = 0;
            for (int i = 0; i < CORR_TILE / CORR_LANES; i++) {
                const uint64_t e = corr_term(t, j, i);
                if (i && e <= prev) return fail("n %lld: lane %d of tile %llu goes backwards", (long long)n, j, (unsigned long long)t);
                prev = e;
                if (e / CORR_TILE != t) return fail("n %lld: term %llu is not of tile %llu", (long long)n, (unsigned long long)e, (unsigned long long)t);
                if (e < (uint64_t)n) {
                    seen[(size_t)e]++;
                    in_tile++;
                }
            }
        }
        if (in_tile < 1) return fail("n %lld: tile %llu is empty", (long long)n, (unsigned long long)t);
    }
    for (int64_t e = 0; e < n; e++)
        if (seen[(size_t)e] != 1) return fail("n %lld: term %lld taken %d times", (long long)n, (long long)e, seen[(size_t)e]);
}

static int run_sweep()
{
    if (CORR_TILE % CORR_LANES || (CORR_LANES & (CORR_LANES - 1))) fail("the tile is not whole lanes, or the lanes no power of two");
    const int64_t ns[] = {2, 3, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096, 4097, 262145, 4194304, 4194305};
    int64_t plans = 0;
    for (int64_t n : ns) {
        walk_order(n);
        for (int xb : {4, 8})
            for (int yb : {0, 4, 8})
                for (int what = 0; what <= 3; what++) {
                    CorrelatePlan p;
                    const bool legal = (what == 0) == (yb == 0);
                    if (plan_correlate(n, 1, 1, xb, yb, what, &p) != legal) {
                        fail("n %lld yb %d what %d: %s", (long long)n, yb, what, legal ? "refused" : "accepted");
                        continue;
                    }
                    if (!legal) continue;
                    check_plan(p, n, 1, 1, xb, yb, what);
                    plans++;
                }
    }
    // [rows][k] with a limit: as given (limit > k / 2) and packed
    for (int64_t limit : {1, 3, 5, 6, 10}) {
        CorrelatePlan p;
        if (!plan_correlate(700, 10, limit, 4, 8, 3, &p)) fail("limit %lld refused", (long long)limit);
        else {
            check_plan(p, 700, 10, limit, 4, 8, 3);
            if (p.x_bytes != (size_t)700 * (2 * limit <= 10 ? limit : 10) * 4) fail("limit %lld: x has %zu bytes", (long long)limit, p.x_bytes);
            plans++;
        }
    }
    // the largest legal problem: sizes and levels only
    CorrelatePlan big;
    if (!plan_correlate(2147483647, 1, 1, 8, 8, 3, &big)) fail("the largest problem refused");
    else {
        check_plan(big, 2147483647, 1, 1, 8, 8, 3);
        if (big.levels != CORR_MAX_LEVELS) fail("the largest problem has %d levels", big.levels);
    }
    // one refused case per argument error
    CorrelatePlan q;
    struct { int64_t rows, k, limit; int xb, yb, what; const char *why; } bad[] = {
        {1, 1, 1, 4, 4, 3, "N < 2"}, {0, 1, 1, 4, 4, 3, "rows < 1"}, {(int64_t)1 << 31, 1, 1, 4, 4, 3, "N > 2^31 - 1"}, {10, 4, 5, 4, 4, 3, "limit > k"},
        {10, 4, 0, 4, 4, 3, "limit < 1"}, {10, 1, 1, 2, 4, 3, "x width"}, {10, 1, 1, 4, 2, 3, "y width"}, {10, 1, 1, 4, 4, 4, "what > 3"},
        {10, 1, 1, 4, 4, -1, "what < 0"}, {10, 1, 1, 4, 4, 0, "ranks of x alone with a y"}, {10, 1, 1, 4, 0, 1, "a correlation without y"}};
    for (const auto &b : bad)
        if (plan_correlate(b.rows, b.k, b.limit, b.xb, b.yb, b.what, &q)) fail("accepted: %s", b.why);
    // the order on the host: sums of integers that every order gives exactly
    for (int64_t n : {2, 2049, 262145}) {
        std::vector<double> v((size_t)n);
        for (int64_t i = 0; i < n; i++) v[(size_t)i] = (double)(i % 7) - 3.0;
        double want = 0;
        for (double d : v) want += d;
        int levels = 0;
        while (v.size() > 1 || !levels) {
            v = sum_level(v);
            levels++;
        }
        CorrelatePlan p;
        if (!plan_correlate(n, 1, 1, 8, 8, 1, &p) || p.levels != levels) fail("n %lld: %d levels walked", (long long)n, levels);
        if (v[0] != want) fail("n %lld: the order's sum is %g, not %g", (long long)n, v[0], want);
    }
    printf("correlate_check sweep: %lld plans, %d failures\n", (long long)plans, g_failures);
    return g_failures ? 1 : 0;
}

static int run_plan()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        long long rows, k, limit;
        int xb, yb, what;
        if (sscanf(line, "%lld %lld %lld %d %d %d", &rows, &k, &limit, &xb, &yb, &what) != 6) {
            fprintf(stderr, "correlate_check: bad line: %s", line);
            return 2;
        }
        CorrelatePlan p;
        if (!plan_correlate(rows, k, limit, xb, yb, what, &p)) {
            printf("refused\n");
            continue;
        }
        printf("%lld %d %lld %lld %lld %lld %lld %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %zu %zu %zu %zu\n", (long long)p.n, p.levels, (long long)p.level_n[0],
               (long long)p.level_n[1], (long long)p.level_n[2], (long long)p.level_n[3], (long long)p.tie_grid, p.x_bytes, p.y_bytes, p.keys_bytes, p.pay_bytes,
               p.table_bytes, p.partial_bytes, p.hist_bytes, p.run_bytes, p.start_bytes, p.rank2_bytes, p.rank2_buffers, p.nan_bytes, p.moment_a_bytes,
               p.moment_b_bytes, p.resident_bytes);
    }
    return 0;
}

static int run_sum()
{
    long long n;
    if (scanf("%lld", &n) != 1 || n < 1 || n > (1 << 24)) {
        fprintf(stderr, "correlate_check: sum needs a count in [1, 2^24]\n");
        return 2;
    }
    std::vector<double> v((size_t)n);
    for (long long i = 0; i < n; i++) {
        uint64_t bits;
        if (scanf("%" SCNx64, &bits) != 1) {
            fprintf(stderr, "correlate_check: sum: value %lld is missing\n", i);
            return 2;
        }
        memcpy(&v[(size_t)i], &bits, 8);
    }
    do v = sum_level(v);
    while (v.size() > 1);
    uint64_t bits;
    memcpy(&bits, &v[0], 8);
    printf("%016" PRIx64 "\n", bits);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) return run_sweep();
    if (argc == 2 && !strcmp(argv[1], "plan")) return run_plan();
    if (argc == 2 && !strcmp(argv[1], "sum")) return run_sum();
    fprintf(stderr, "usage: correlate_check plan < lines | correlate_check sweep | correlate_check sum < values\n");
    return 2;
}
