// The flat search's planner (plan.h) on a machine without a GPU:
//   plan_check cases   reads lines "nb nq k metric flags force_qt force_chunks batch_nq allow_stat [approx16]" from stdin and prints,
//                      for each, the pieces of the batch and the plan of every piece (tests/plan_cases.py, tests/test_plan_cpu.py)
//   plan_check sweep   walks a grid of shapes and flags and exits non-zero on a broken invariant
// The device has 256 CUs in both.  Built with the host compiler and -fsanitize=address,undefined (make plan_check).
#include "plan.h"

#include <stdio.h>
#include <string.h>

static const int MAX_LEVELS = 8; // (knn_index_s::MAX_LEVELS: levels of seed recursion)

static PlanCtx make_ctx(int64_t nb, int64_t nq, int metric, int flags, int force_qt, int force_chunks, int64_t batch, bool approx16)
{
    PlanCtx c;
    c.metric = metric;
    c.approx16 = approx16;
    c.flags = flags & ~KNN_TUNE_PUB_ROUNDS_MASK; // (as knn_set_tuning stores them)
    c.pub_rounds_force = (flags & KNN_TUNE_PUB_ROUNDS_MASK) >> KNN_TUNE_PUB_ROUNDS_SHIFT;
    c.force_qt = force_qt;
    c.force_chunks = force_chunks;
    c.num_cus = 256;
    c.batch_nq = batch > 0 ? std::max(nq, batch) : nq; // (BatchScope: the caller's whole batch, or knn_flat_set_batch's)
    c.ntotal = nb;
    return c;
}

// the sample level of a plan: its view (stride, block shift, rows) under a view with stride row_mul and block shift vshift
struct SampleView {
    int row_mul, vshift;
    int64_t nb;
};
static SampleView sample_view(const SearchPlan &s, int64_t nb, int row_mul, int vshift)
{
    SampleView v;
    v.vshift = s.svshift < 0 ? vshift : s.svshift;
    v.row_mul = row_mul * s.sstride;
    v.nb = view_rows(nb, s.sstride, v.vshift);
    return v;
}

static void print_plan(const char *tag, const SearchPlan &s, int64_t sample_rows)
{
    const ScanPlan &p = s.pl;
    printf(" %s %s %d %d %d %d %d %d %zu %d %d %d %d %d %d %d %d %lld", tag, p.name, p.qt, p.dt, p.nchunks, p.grid, p.npairs, p.cap, p.lds, s.sstride,
           s.seed_stat, s.seed_j, s.pub_rounds, s.pub_m, s.kslot, s.qcap, s.pool_tiles, (long long)sample_rows);
}

static int run_cases()
{
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long nb, nq, batch;
        int k, metric, flags, force_qt, force_chunks, allow_stat, approx16 = 0;
        const int n = sscanf(line, "%lld %lld %d %d %d %d %d %lld %d %d", &nb, &nq, &k, &metric, &flags, &force_qt, &force_chunks, &batch, &allow_stat, &approx16);
        if (n < 9) {
            if (line[0] == '\n' || line[0] == '#') continue;
            fprintf(stderr, "plan_check: bad case line: %s", line);
            return 2;
        }
        const PlanCtx c = make_ctx(nb, nq, metric, flags, force_qt, force_chunks, batch, approx16 != 0);
        const std::vector<Piece> pieces = plan_pieces(c, nq, k, allow_stat != 0);
        printf("pieces %zu", pieces.size());
        for (const Piece &pc : pieces) {
            // (search_keys_impl: the database in blocks of 8 rows, every one of them)
            const int64_t vnb = view_rows(nb, 1, 3);
            const SearchPlan s = plan_search(c, vnb, pc.m, k, 0, 1, allow_stat != 0, 0);
            printf(" | %lld %lld", (long long)pc.q0, (long long)pc.m);
            if (s.sstride) {
                const SampleView v = sample_view(s, vnb, 1, 3);
                print_plan("L0", s, v.nb);
                print_plan("L1", plan_search(c, v.nb, pc.m, s.k_sample, 1, v.row_mul, false, 0), 0);
            } else {
                print_plan("L0", s, 0);
            }
        }
        printf("\n");
    }
    return 0;
}

static long long g_checked = 0, g_broken = 0;
#define INVARIANT(cond)                                                                                                                  \
    do {                                                                                                                                 \
        if (!(cond)) {                                                                                                                   \
            if (g_broken++ < 20)                                                                                                         \
                fprintf(stderr, "broken: %s  [nb %lld view %lld nq %lld k %d metric %d flags %d qt %d approx16 %d stat %d level %d: %s grid %d chunks %d]\n", #cond, \
                        (long long)c.ntotal, (long long)nb, (long long)nq, k, c.metric, c.flags, c.force_qt, (int)c.approx16, (int)allow_stat, level, p.name, p.grid, p.nchunks); \
        }                                                                                                                                \
    } while (0)

// one search_view call and the sample levels below it
static void check_view(const PlanCtx &c, int64_t nb, int64_t nq, int k, int level, int row_mul, int vshift, bool allow_stat)
{
    const SearchPlan s = plan_search(c, nb, nq, k, level, row_mul, allow_stat, 0);
    const ScanPlan &p = s.pl;
    g_checked++;
    const int64_t ntiles = (nb + p.dt - 1) / p.dt;
    INVARIANT(level < MAX_LEVELS);
    INVARIANT(p.npairs ? p.grid == 2 * p.npairs && p.nchunks == p.grid : p.grid == p.nqtiles * p.nchunks);
    INVARIANT((int64_t)p.tiles_base * (p.npairs ? p.npairs : p.nchunks) + p.tiles_rem == ntiles);
    INVARIANT(p.tiles_rem >= 0 && p.tiles_rem < (p.npairs ? p.npairs : p.nchunks));
    INVARIANT(p.lds <= 160 * 1024);
    INVARIANT(p.lds == scan_lds_bytes(p.qt, p.dt, p.cap));
    INVARIANT(p.nchunks <= 1 || (int64_t)p.grid * p.qt * p.cap * 8 <= (int64_t)2 << 30);
    INVARIANT((int64_t)s.pub_rounds * s.pub_m * p.nchunks <= 4096);
    INVARIANT(s.pool_tiles >= 0 && s.pool_tiles <= p.tiles_base / 4);
    INVARIANT(!(s.pub_rounds && s.sstride));
    INVARIANT(scan_kernel_illegal(p.qt, c.metric == KNN_METRIC_L2, c.approx16, p.nqtiles == 1, 0) == nullptr);
    if (s.sstride && level + 1 < MAX_LEVELS) {
        const SampleView v = sample_view(s, nb, row_mul, vshift);
        INVARIANT(v.nb > 0 && v.nb < nb);
        check_view(c, v.nb, nq, s.k_sample, level + 1, v.row_mul, v.vshift, false);
    }
}

static void check_batch(const PlanCtx &c, int64_t nq, int k, bool allow_stat)
{
    const std::vector<Piece> pieces = plan_pieces(c, nq, k, allow_stat);
    int64_t at = 0, last_m = -1;
    bool tiled = !pieces.empty();
    for (const Piece &pc : pieces) {
        tiled = tiled && pc.q0 == at && pc.m > 0;
        at += pc.m;
    }
    if (!tiled || at != nq) {
        if (g_broken++ < 20) fprintf(stderr, "broken: pieces do not tile [0, %lld) [nb %lld k %d flags %d qt %d]\n", (long long)nq, (long long)c.ntotal, k, c.flags, c.force_qt);
        return;
    }
    for (const Piece &pc : pieces) {
        if (pc.m == last_m) continue; // (the full blocks of a long batch: one plan)
        last_m = pc.m;
        check_view(c, view_rows(c.ntotal, 1, 3), pc.m, k, 0, 1, 3, allow_stat);
    }
}

static int run_sweep()
{
    const int64_t nbs[] = {1, 255, 256, 257, 1023, 4096, 8192, 16385, 1 << 15, 1 << 18, (1 << 18) + 1, 1250000, 10000000, 2147483647};
    const int64_t nqs[] = {1, 8, 19, 20, 32, 33, 48, 49, 64, 65, 96, 97, 128, 129, 256, 384, 640, 16384, 24576, 24577, 200000};
    const int ks[] = {1, 10, 100, 301, 1000, 1400, 1401, 2048};
    const int flagset[] = {0, KNN_TUNE_NO_POOL, KNN_TUNE_NO_PAIRS, KNN_TUNE_NO_SEED, KNN_TUNE_EXACT_SEED, KNN_TUNE_NORM_L2, KNN_TUNE_ALWAYS_RESET,
                           KNN_TUNE_STAT_SEED, KNN_TUNE_NO_TURNS, KNN_TUNE_NO_STAT_SEED, KNN_TUNE_NO_SYM, KNN_TUNE_NO_TILE_MIN_SEED,
                           1 << KNN_TUNE_PUB_ROUNDS_SHIFT, 2 << KNN_TUNE_PUB_ROUNDS_SHIFT, KNN_TUNE_NO_REMAINDER_SPLIT, KNN_TUNE_NO_Q16,
                           KNN_TUNE_NO_BIG_TILE, KNN_TUNE_BIG_TILE, KNN_TUNE_NO_SCAN16, KNN_TUNE_SCAN16_ANY_NB};
    const int qts[] = {0, 32, 48, 64, 96, 128, 256};
    for (int64_t nb : nbs)
        for (int64_t nq : nqs)
            for (int k : ks)
                for (int metric = 0; metric < 2; metric++)
                    for (int flags : flagset)
                        for (int qt : qts)
                            for (int allow_stat = 0; allow_stat < 2; allow_stat++)
                                check_batch(make_ctx(nb, nq, metric, flags, qt, 0, 0, false), nq, k, allow_stat != 0);
    // beside the issue's grid: the bf16 index of HNSW's coarse entry scan (no entry point reaches its introspection from outside),
    // a forced chunk count, a piece of a larger batch, and the symmetric self-search's launch
    for (int64_t nb : nbs)
        for (int64_t nq : nqs)
            for (int k : ks)
                for (int metric = 0; metric < 2; metric++) {
                    check_batch(make_ctx(nb, nq, metric, 0, 0, 0, 0, true), nq, k, false);
                    check_batch(make_ctx(nb, nq, metric, 0, 0, 3, 0, false), nq, k, true);
                    check_batch(make_ctx(nb, nq, metric, 0, 0, 0, 100, false), nq, k, true);
                    for (int flags : {0, (int)KNN_TUNE_BIG_TILE}) {
                        const PlanCtx c = make_ctx(nb, nb, metric, flags, 0, 0, 0, false);
                        int j = 0, qcap = 0;
                        if (nq != 1 || !self_search_symmetric_eligible(c, k, &j, &qcap)) continue;
                        ScanPlan p;
                        PlanOpts po;
                        po.seeded = true; po.allow_big = flags != 0;
                        make_plan(c, nb, nb, k, po, p);
                        g_checked++;
                        const bool allow_stat = true;
                        const int level = 0;
                        INVARIANT(j > 0 && qcap > 0);
                        INVARIANT(scan_lds_bytes(p.qt, p.dt, p.cap, p.qt == 128 ? 73728 : 0) + (size_t)4 * p.dt * 4 <= 160 * 1024);
                    }
                }
    printf("plan_check sweep: %lld plans checked, %lld broken\n", g_checked, g_broken);
    return g_broken ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "cases")) return run_cases();
    if (argc == 2 && !strcmp(argv[1], "sweep")) return run_sweep();
    fprintf(stderr, "usage: plan_check cases < lines | plan_check sweep\n");
    return 2;
}
