// plan_windows and window_piece of plan.h on a machine without a GPU:
//   windows_check plan    reads lines "n key_bytes m window want_order nbins" from stdin and prints, for each, "refused" or
//                         nout nblocks run blocks_per_run runs_per_block group chain_grid chain_lds scan_blocks and the bytes of
//                         the columns, the masks, the running counts, the block sums, the float64 keys, one chain buffer, the
//                         means, the bins, and all of them with the rank's
//   windows_check sweep   walks window_chain_kernel's staging on the host for a grid of (n, window): every workgroup, every
//                         step, both directions, the way the kernel enumerates them, and exits non-zero on a broken invariant
// Built with the host compiler and -fsanitize=address,undefined (make windows_check).
#include "plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>

static int g_failures = 0;
static void fail(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    fprintf(stderr, "windows_check: ");
    vfprintf(stderr, fmt, ap);
    fprintf(stderr, "\n");
    va_end(ap);
    g_failures++;
}

static const int64_t MAX_GRID_X = 2147483647, MAX_GRID_Y = 65535;
static const size_t MAX_LDS = 64 * 1024; // a workgroup's LDS without an opt-in

static void check_sizes(const WindowsPlan &p, int64_t n, int key_bytes, int64_t m, int64_t window, bool want_order, int64_t nbins)
{
    const size_t un = (size_t)n;
    RankPlan r;
    if (!plan_rank(n, 1, 1, key_bytes, false, false, want_order, &r)) return fail("n %lld: the rank refuses what the windows accept", (long long)n);
    if (r.resident_bytes != p.rank.resident_bytes || p.rank.n != n) fail("n %lld: not the rank's plan", (long long)n);
    size_t sum = p.rank.resident_bytes;
    const size_t want[] = {(size_t)m * un, m ? un * 4 : 0, (size_t)m * un * 4, m ? (size_t)((n + RANK_SCAN_BLOCK - 1) / RANK_SCAN_BLOCK) * 4 : 0,
                           window ? ((un + 1) / 2 * 2) * 8 : 0, window ? un * 8 : 0, window ? (size_t)(m + 1) * (size_t)(n - window + 1) * 8 : 0,
                           (size_t)nbins * (16 + (size_t)m * 8 + 3 * (size_t)key_bytes)};
    const size_t got[] = {p.values_bytes, p.mask_bytes, p.cum_bytes, p.wpartial_bytes, p.keyd_bytes, p.chain_bytes, p.means_bytes, p.bins_bytes};
    for (int i = 0; i < 8; i++) {
        if (want[i] != got[i]) fail("n %lld m %lld window %lld nbins %lld: buffer %d has %zu bytes, not %zu", (long long)n, (long long)m, (long long)window, (long long)nbins, i, got[i], want[i]);
        sum += got[i];
    }
    sum += p.chain_bytes; // P and S
    if (sum != p.resident_bytes) fail("n %lld m %lld window %lld: the buffers add up to %zu, resident_bytes is %zu", (long long)n, (long long)m, (long long)window, sum, p.resident_bytes);
    // grids: none is 0 where its kernel runs, none above the launch limits
    const int64_t gx[] = {p.gather_grid, window ? p.chain_grid : 1, window ? p.combine_grid : 1, window && m ? p.means_grid : 1, nbins ? p.ranges_grid : 1,
                          m ? p.scan_blocks : 1};
    for (int64_t g : gx)
        if (g < 1 || g > MAX_GRID_X) fail("n %lld m %lld window %lld nbins %lld: a grid of %lld", (long long)n, (long long)m, (long long)window, (long long)nbins, (long long)g);
    if (m > MAX_GRID_Y) fail("m %lld above grid.y", (long long)m);
    if (p.chain_lds > MAX_LDS || p.chain_lds != 2 * (size_t)(p.run + (p.run >> WINDOW_PAD_SHIFT)) * 8) fail("chain_lds %zu", p.chain_lds);
    if (window) {
        if (p.nout != n - window + 1 || p.nblocks != (n + window - 1) / window) fail("n %lld window %lld: nout / nblocks", (long long)n, (long long)window);
        if ((p.blocks_per_run != 1) && (p.runs_per_block != 1)) fail("window %lld: both layouts at once", (long long)window);
        if (p.blocks_per_run < 1 || 2 * p.blocks_per_run > WINDOW_CHAINS) fail("window %lld: %lld blocks per run", (long long)window, (long long)p.blocks_per_run);
        if (window <= p.run && p.blocks_per_run * window > p.run) fail("window %lld: a group longer than a run", (long long)window);
        if (window > p.run && (p.runs_per_block - 1) * p.run >= window) fail("window %lld: an empty run", (long long)window);
        if (window > p.run && p.runs_per_block * p.run < window) fail("window %lld: runs short of a block", (long long)window);
        if (p.group != p.blocks_per_run * window || p.chain_grid != (n + p.group - 1) / p.group) fail("window %lld: group / chain_grid", (long long)window);
    }
}

// window_chain_kernel on the host: the same loops over workgroups, steps, directions and chains, with marks for loads.
static void walk_chains(const WindowsPlan &p)
{
    const int64_t n = p.n, W = p.window, run = p.run;
    std::vector<uint8_t> staged[2], walked[2];
    for (int d = 0; d < 2; d++) {
        staged[d].assign((size_t)n, 0);
        walked[d].assign((size_t)n, 0);
    }
    const int64_t lds_slots = run + (run >> WINDOW_PAD_SHIFT);
    for (int64_t wg = 0; wg < p.chain_grid; wg++) {
        const int64_t g0 = wg * p.group, len = std::min<int64_t>(p.group, n - g0);
        if (len < 1) return fail("n %lld window %lld: workgroup %lld has no ranks", (long long)n, (long long)W, (long long)wg);
        const int64_t steps = (len + run - 1) / run;
        std::vector<int64_t> next((size_t)WINDOW_CHAINS, -1); // per chain: the rank it must read next
        for (int64_t step = 0; step < steps; step++) {
            for (int d = 0; d < 2; d++) {
                const WindowPiece q = window_piece(g0, len, run, step, d);
                if (q.lo < g0 || q.hi > g0 + len || q.hi <= q.lo || q.hi - q.lo > run) return fail("n %lld window %lld: piece [%lld, %lld)", (long long)n, (long long)W, (long long)q.lo, (long long)q.hi);
                // the 16-byte loads: from an even rank, inside the padded float64 keys
                const int64_t e0 = q.lo & ~(int64_t)1;
                for (int64_t e = e0; e < q.hi; e += 2)
                    if ((size_t)(e + 2) * 8 > p.keyd_bytes) return fail("n %lld window %lld: a load past the keys at %lld", (long long)n, (long long)W, (long long)e);
                for (int64_t e = q.lo; e < q.hi; e++) {
                    const int64_t slot = (e - q.lo) + ((e - q.lo) >> WINDOW_PAD_SHIFT);
                    if (slot < 0 || slot >= lds_slots) return fail("n %lld window %lld: LDS slot %lld", (long long)n, (long long)W, (long long)slot);
                    staged[d][(size_t)e]++;
                }
            }
            for (int tid = 0; tid < WINDOW_CHAINS; tid++) {
                const int back = tid & 1;
                const int64_t bs = g0 + (int64_t)(tid >> 1) * W, be = std::min<int64_t>(bs + W, g0 + len);
                if (!((tid >> 1) < p.blocks_per_run && bs < g0 + len)) continue;
                const WindowPiece q = window_piece(g0, len, run, step, back);
                const int64_t a = std::max<int64_t>(bs, q.lo), b = std::min<int64_t>(be, q.hi);
                if (a >= b) continue;
                // contiguous and in order: this piece starts where the chain stopped (or at the block's end it starts from)
                const int64_t first = back ? b - 1 : a, expect = next[(size_t)tid] < 0 ? (back ? be - 1 : bs) : next[(size_t)tid];
                if (first != expect) return fail("n %lld window %lld: chain %d of workgroup %lld resumes at %lld, not %lld", (long long)n, (long long)W, tid, (long long)wg, (long long)first, (long long)expect);
                for (int64_t e = a; e < b; e++) walked[back][(size_t)e]++;
                next[(size_t)tid] = back ? a - 1 : b;
            }
        }
        for (int tid = 0; tid < WINDOW_CHAINS; tid++) { // every chain has reached its block's other end
            const int64_t bs = g0 + (int64_t)(tid >> 1) * W, be = std::min<int64_t>(bs + W, g0 + len);
            if (!((tid >> 1) < p.blocks_per_run && bs < g0 + len)) continue;
            if (next[(size_t)tid] != ((tid & 1) ? bs - 1 : be)) return fail("n %lld window %lld: chain %d of workgroup %lld stops at %lld", (long long)n, (long long)W, tid, (long long)wg, (long long)next[(size_t)tid]);
        }
    }
    for (int d = 0; d < 2; d++)
        for (int64_t e = 0; e < n; e++)
            if (staged[d][(size_t)e] != 1 || walked[d][(size_t)e] != 1)
                return fail("n %lld window %lld: rank %lld direction %d staged %d times, walked %d times", (long long)n, (long long)W, (long long)e, d, staged[d][(size_t)e], walked[d][(size_t)e]);
}

static int run_sweep()
{
    const int64_t ns[] = {1, 2, 255, 256, 2047, 2048, 2049, 70000};
    int64_t plans = 0;
    for (int64_t n : ns) {
        const int64_t R = WINDOW_RUN;
        const int64_t ws[] = {1, 2, 3, n, n - 1, R - 1, R, R + 1, 2 * R + 1, 1000, 64, 3 * R};
        for (int64_t w0 : ws) {
            const int64_t w = std::max<int64_t>(1, std::min<int64_t>(w0, n));
            for (int key_bytes : {4, 8})
                for (int64_t m : {0, 1, 5, 32})
                    for (int want_order = 0; want_order < 2; want_order++)
                        for (int64_t nbins : {0, 1, 7}) {
                            WindowsPlan p;
                            if (!plan_windows(n, key_bytes, m, w, want_order != 0, nbins, &p)) {
                                fail("n %lld window %lld refused", (long long)n, (long long)w);
                                continue;
                            }
                            check_sizes(p, n, key_bytes, m, w, want_order != 0, nbins);
                            plans++;
                            if (key_bytes == 8 && m == 0 && !want_order && nbins == 0) walk_chains(p);
                        }
        }
        // bins alone
        WindowsPlan p;
        if (!plan_windows(n, 8, 3, 0, false, 10, &p)) fail("n %lld bins alone refused", (long long)n);
        else check_sizes(p, n, 8, 3, 0, false, 10);
    }
    // the largest legal problem: sizes only
    WindowsPlan big;
    if (!plan_windows(2147483647, 8, 32, 1000, true, KNN_WINDOWS_MAX_BINS, &big)) fail("the largest problem refused");
    else check_sizes(big, 2147483647, 8, 32, 1000, true, KNN_WINDOWS_MAX_BINS);
    // one refused case per argument error
    WindowsPlan q;
    struct { int64_t n; int kb; int64_t m, w; int64_t nb; const char *what; } bad[] = {
        {0, 4, 1, 1, 0, "n < 1"}, {(int64_t)1 << 31, 4, 1, 1, 0, "n > 2^31 - 1"}, {10, 2, 1, 1, 0, "key width"}, {10, 4, -1, 1, 0, "m < 0"},
        {10, 4, 33, 1, 0, "m > 32"}, {10, 4, 1, -1, 0, "window < 0"}, {10, 4, 1, 11, 0, "window > n"}, {10, 4, 1, 0, 0, "neither window nor bins"},
        {10, 4, 1, 1, -1, "nbins < 0"}, {10, 4, 1, 1, (int64_t)KNN_WINDOWS_MAX_BINS + 1, "nbins too large"}};
    for (const auto &b : bad)
        if (plan_windows(b.n, b.kb, b.m, b.w, false, b.nb, &q)) fail("accepted: %s", b.what);
    printf("windows_check sweep: %lld plans, %d failures\n", (long long)plans, g_failures);
    return g_failures ? 1 : 0;
}

static int run_plan()
{
    char line[256];
    while (fgets(line, sizeof line, stdin)) {
        long long n, m, window, nbins;
        int key_bytes, want_order;
        if (sscanf(line, "%lld %d %lld %lld %d %lld", &n, &key_bytes, &m, &window, &want_order, &nbins) != 6) {
            fprintf(stderr, "windows_check: bad line: %s", line);
            return 2;
        }
        WindowsPlan p;
        if (!plan_windows(n, key_bytes, m, window, want_order != 0, nbins, &p)) {
            printf("refused\n");
            continue;
        }
        printf("%lld %lld %lld %lld %lld %lld %lld %zu %lld %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", (long long)p.nout, (long long)p.nblocks, (long long)p.run,
               (long long)p.blocks_per_run, (long long)p.runs_per_block, (long long)p.group, (long long)p.chain_grid, p.chain_lds, (long long)p.scan_blocks,
               p.values_bytes, p.mask_bytes, p.cum_bytes, p.wpartial_bytes, p.keyd_bytes, p.chain_bytes, p.means_bytes, p.bins_bytes, p.resident_bytes);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "sweep")) return run_sweep();
    if (argc == 2 && !strcmp(argv[1], "plan")) return run_plan();
    fprintf(stderr, "usage: windows_check plan < lines | windows_check sweep\n");
    return 2;
}
