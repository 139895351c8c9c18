// The planners of plan.h on a machine without a GPU:
//   plan_check cases   reads lines "nb nq k metric flags force_qt force_chunks batch_nq allow_stat [approx16]" from stdin and prints,
//                      for each, the pieces of the batch and the plan of every piece (tests/plan_cases.py, tests/test_plan_cpu.py)
//   plan_check sym     reads lines "n k metric flags can_stream [force_qt]": the symmetric self-search's plan and work table --
//                      "plain", or kernel ts tiles st S j qcap k_sample n_expect groups gstart[0..groups] first_run items lds
//                      max_wgs and the 64-bit FNV-1a hash of the items' integers
//   plan_check range   reads lines "n nq metric batch [num_cus]": the range scan's plan of one block of nq queries -- kernel qt dt
//                      nqtiles nchunks tiles_base tiles_rem grid diff lds segcap
//   plan_check rank    reads lines "rows k limit key_bytes has_correct want_cum want_wide": the size plan of the device-wide rank -- n
//                      ntiles table_entries table_blocks cum_blocks passes pack dev_k and the bytes of the scores, correct, one key buffer,
//                      one payload buffer, table, block sums, histograms, running count, int64 staging and all of them, or "refused"
//   plan_check pool    reads lines "n d row_stride base elem_bytes normalize": the pooling launch -- ncb waves grid_x grid_y aligned,
//                      or "refused"
//   plan_check kde     reads lines "n ncols m": the density launch -- group_rows groups tiles chunks tail_rows tail_points part_bytes,
//                      or "refused"
//   plan_check poolchunks  reads "n chunk_rows" and n lines "start stop": the host pooling entry's uploads, one line per chunk --
//                      "row0 row1 count: the indices of its ranges" (the host code of knn_pool_ranges that is separable from its
//                      launches, under the sanitizers here)
//   plan_check sweep   walks a grid of shapes and flags and exits non-zero on a broken invariant
// The device has 256 CUs throughout, but for a `range` line that names another count.  Built with the host compiler and -fsanitize=address,undefined (make plan_check).
#include "plan.h"

#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <set>
#include <string>
#include <tuple>

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

static int run_sym()
{
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long n;
        int k, metric, flags, can_stream, force_qt = 0;
        if (sscanf(line, "%lld %d %d %d %d %d", &n, &k, &metric, &flags, &can_stream, &force_qt) < 5) {
            if (line[0] == '\n' || line[0] == '#') continue;
            fprintf(stderr, "plan_check: bad case line: %s", line);
            return 2;
        }
        SymPlan sp;
        if (!plan_self_symmetric(make_ctx(n, n, metric, flags, force_qt, 0, 0, false), k, can_stream != 0, sp)) {
            printf("plain\n");
            continue;
        }
        const SymTable t = sym_work_table(sp.tiles, sp.groups, sp.slots);
        uint64_t hash = 0xcbf29ce484222325ull;
        for (const SymItem &it : t.items)
            for (int v : {it.qtile, it.jt0, it.jcount})
                for (int b = 0; b < 4; b++) hash = (hash ^ (((uint32_t)v >> (8 * b)) & 0xff)) * 0x100000001b3ull;
        printf("%s %d %d %d %lld %d %d %d %d %d", sp.name, sp.ts, sp.tiles, sp.st, (long long)sp.S, sp.j, sp.qcap, sp.k_sample, sp.n_expect, sp.groups);
        for (int64_t g : t.gstart) printf(" %lld", (long long)g);
        printf(" %d %zu %zu %lld %016llx\n", t.first_run, t.items.size(), sp.lds, (long long)sp.max_wgs, (unsigned long long)hash);
    }
    return 0;
}

static int run_range()
{
    char line[512];
    while (fgets(line, sizeof line, stdin)) {
        long long n, nq, batch;
        int metric, cus = 256;
        if (sscanf(line, "%lld %lld %d %lld %d", &n, &nq, &metric, &batch, &cus) < 4) {
            if (line[0] == '\n' || line[0] == '#') continue;
            fprintf(stderr, "plan_check: bad case line: %s", line);
            return 2;
        }
        PlanCtx c = make_ctx(n, nq, metric, 0, 0, 0, batch, false);
        c.num_cus = cus;
        const RangePlan p = plan_range(c, nq);
        printf("%s %d %d %d %d %d %d %d %d %zu %lld\n", p.name, p.qt, p.dt, p.nqtiles, p.nchunks, p.tiles_base, p.tiles_rem, p.grid, (int)p.diff, p.lds,
               (long long)range_segcap(p, nq));
    }
    return 0;
}

static long long g_checked = 0, g_broken = 0;
static void broken(const char *what, const std::string &where)
{
    if (g_broken++ < 20) fprintf(stderr, "broken: %s  [%s]\n", what, where.c_str());
}
// (where: the checking function's description of the plan at hand)
#define INVARIANT(cond)                       \
    do {                                      \
        if (!(cond)) broken(#cond, where());  \
    } while (0)

static std::string describe(const char *fmt, ...) __attribute__((format(printf, 1, 2)));
static std::string describe(const char *fmt, ...)
{
    char buf[400];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return buf;
}

// one search_view call and the sample levels below it
static void check_view(const PlanCtx &c, int64_t nb, int64_t nq, int k, int level, int row_mul, int vshift, bool allow_stat)
{
    const SearchPlan s = plan_search(c, nb, nq, k, level, row_mul, allow_stat, 0);
    const ScanPlan &p = s.pl;
    const auto where = [&] {
        return describe("nb %lld view %lld nq %lld k %d metric %d flags %d qt %d approx16 %d stat %d level %d: %s grid %d chunks %d", (long long)c.ntotal, (long long)nb,
                        (long long)nq, k, c.metric, c.flags, c.force_qt, (int)c.approx16, (int)allow_stat, level, p.name, p.grid, p.nchunks);
    };
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

// the symmetric self-search: every tile pair (I, J >= I) is served exactly once, by the group that owns query tile I
static void check_sym(const PlanCtx &c, int k, bool can_stream)
{
    SymPlan sp;
    if (!plan_self_symmetric(c, k, can_stream, sp)) return;
    const int64_t n = c.ntotal;
    const int T = sp.tiles, G = sp.groups;
    const auto where = [&] {
        return describe("self-search n %lld k %d metric %d flags %d can_stream %d: %s tiles %d groups %d", (long long)n, k, c.metric, c.flags, (int)can_stream, sp.name, T, G);
    };
    g_checked++;
    INVARIANT(sp.j > 0 && sp.qcap > 0 && sp.n_expect > 0 && sp.n_expect <= sp.qcap && sp.k_sample <= k);
    INVARIANT(sp.lds <= 160 * 1024);
    INVARIANT(sp.max_wgs >= sp.slots);
    INVARIANT(G >= 1 && G <= SYM_MAX_GROUPS && (G == 1 || can_stream));
    // (the table and the row ranges depend on these four only: each distinct table is built and checked once)
    static std::set<std::tuple<int64_t, int, int, int64_t>> seen;
    if (!seen.insert(std::make_tuple(n, sp.ts, G, sp.slots)).second) return;
    const SymTable t = sym_work_table(T, G, sp.slots);
    INVARIANT((int)t.gstart.size() == G + 1 && t.gstart[0] == 0 && t.gstart[(size_t)G] == (int64_t)t.items.size());
    INVARIANT(sym_group_row0(sp, n, 0) == 0 && sym_group_row0(sp, n, G) == n); // the groups' row ranges [row0(g), row0(g + 1)) tile [0, n)
    std::vector<int> next((size_t)T); // per query tile: where its runs so far end (the stable sort keeps a tile's runs of one length in order)
    for (int I = 0; I < T; I++) next[(size_t)I] = I;
    for (int g = 0; g < G; g++) {
        const int64_t i0 = t.gstart[(size_t)g], i1 = t.gstart[(size_t)g + 1];
        INVARIANT(i0 <= i1 && i1 <= (int64_t)t.items.size());
        if (i0 > i1 || i1 > (int64_t)t.items.size()) return;
        // group g owns the query tiles whose rows it selects and downloads
        const int I0 = (int)((sym_group_row0(sp, n, g) + sp.ts - 1) / sp.ts), I1 = (int)((sym_group_row0(sp, n, g + 1) + sp.ts - 1) / sp.ts);
        INVARIANT(I0 <= I1);
        for (int64_t i = i0; i < i1; i++) {
            const SymItem &it = t.items[(size_t)i];
            INVARIANT(it.qtile >= I0 && it.qtile < I1);
            if (it.qtile < 0 || it.qtile >= T) return;
            // the runs of a query tile start at the tile and touch end to start
            INVARIANT(it.jcount >= 1 && it.jt0 == next[(size_t)it.qtile] && it.jt0 + it.jcount <= T);
            next[(size_t)it.qtile] = it.jt0 + it.jcount;
            INVARIANT(i == i0 || t.items[(size_t)i - 1].jcount >= it.jcount); // inside a group jcount does not rise
        }
    }
    for (int I = 0; I < T; I++) INVARIANT(next[(size_t)I] == T); // ... and end at `tiles`
}

static void check_range(const PlanCtx &c, int64_t nq)
{
    const RangePlan p = plan_range(c, nq);
    const auto where = [&] { return describe("range n %lld nq %lld metric %d: %s grid %d chunks %d", (long long)c.ntotal, (long long)nq, c.metric, p.name, p.grid, p.nchunks); };
    g_checked++;
    INVARIANT((int64_t)p.tiles_base * p.nchunks + p.tiles_rem == (c.ntotal + p.dt - 1) / p.dt);
    INVARIANT(p.grid == p.nqtiles * p.nchunks);
    INVARIANT(p.lds <= 160 * 1024);
    INVARIANT(range_segcap(p, nq) >= 1);
}

// the size plan of the device-wide rank: the tiles cover [0, n) and no more, the table is 256 counts per tile, the scan blocks
// cover what they scan, every index a kernel forms fits its 32-bit type, the packing rule, and every buffer's bytes
static void check_rank(int64_t rows, int64_t k, int64_t limit, int key_bytes, int outs)
{
    const bool has_correct = outs & 1, want_cum = has_correct && (outs & 2), want_wide = outs & 4;
    RankPlan p;
    const bool ok = plan_rank(rows, k, limit, key_bytes, has_correct, want_cum, want_wide, &p);
    const auto where = [&] {
        return describe("rank rows %lld k %lld limit %lld key %d outs %d", (long long)rows, (long long)k, (long long)limit, key_bytes, outs);
    };
    g_checked++;
    const bool legal = rows >= 1 && k >= 1 && limit >= 1 && limit <= k && k <= INT32_MAX && (key_bytes == 4 || key_bytes == 8) &&
                       (__int128)rows * limit <= INT32_MAX && (__int128)rows * k <= INT64_MAX / 16;
    INVARIANT(ok == legal);
    if (!ok || !legal) return;
    INVARIANT(p.n == rows * limit && p.n <= INT32_MAX);
    INVARIANT(p.ntiles >= 1 && p.ntiles * RANK_TILE >= p.n && (p.ntiles - 1) * RANK_TILE < p.n);
    INVARIANT(p.ntiles * RANK_TILE <= (int64_t)UINT32_MAX); // (a tile's last element index, valid or not, is a uint32_t)
    INVARIANT(p.table_entries == 256 * p.ntiles);
    INVARIANT(p.table_blocks * RANK_SCAN_BLOCK >= p.table_entries && (p.table_blocks - 1) * RANK_SCAN_BLOCK < p.table_entries);
    INVARIANT(want_cum ? (p.cum_blocks * RANK_SCAN_BLOCK >= p.n && (p.cum_blocks - 1) * RANK_SCAN_BLOCK < p.n) : p.cum_blocks == 0);
    INVARIANT(p.table_blocks <= INT32_MAX && p.cum_blocks <= INT32_MAX); // grids
    INVARIANT(p.passes == key_bytes);
    // packed exactly when that at least halves the upload; the device copy holds every column a kernel reads
    INVARIANT(p.pack == (2 * limit <= k) && p.dev_k == (p.pack ? limit : k) && p.dev_k >= limit && p.dev_k <= INT32_MAX);
    const size_t n = (size_t)p.n, cells = (size_t)rows * (size_t)p.dev_k;
    INVARIANT(p.scores_bytes == cells * (size_t)key_bytes && p.correct_bytes == (has_correct ? cells : 0));
    INVARIANT(p.keys_bytes == n * (size_t)key_bytes && p.pay_bytes == n * 4 && p.table_bytes == (size_t)p.table_entries * 4);
    INVARIANT(p.partial_bytes == (size_t)std::max(p.table_blocks, p.cum_blocks) * 4 && p.hist_bytes == (size_t)key_bytes * 1024);
    INVARIANT(p.cum_bytes == (want_cum ? n * 4 : 0) && p.wide_bytes == (want_wide ? n * 8 : 0));
    INVARIANT(p.resident_bytes == p.scores_bytes + p.correct_bytes + 2 * p.keys_bytes + 2 * p.pay_bytes + p.table_bytes + p.partial_bytes + p.hist_bytes +
                                      p.cum_bytes + p.wide_bytes);
}

static int run_rank()
{
    long long rows, k, limit;
    int key_bytes, has_correct, want_cum, want_wide;
    while (scanf("%lld %lld %lld %d %d %d %d", &rows, &k, &limit, &key_bytes, &has_correct, &want_cum, &want_wide) == 7) {
        RankPlan p;
        if (!plan_rank(rows, k, limit, key_bytes, has_correct != 0, want_cum != 0, want_wide != 0, &p)) {
            printf("refused\n");
            continue;
        }
        printf("%lld %lld %lld %lld %lld %d %d %lld %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", (long long)p.n, (long long)p.ntiles, (long long)p.table_entries,
               (long long)p.table_blocks, (long long)p.cum_blocks, p.passes, (int)p.pack, (long long)p.dev_k, p.scores_bytes, p.correct_bytes, p.keys_bytes,
               p.pay_bytes, p.table_bytes, p.partial_bytes, p.hist_bytes, p.cum_bytes, p.wide_bytes, p.resident_bytes);
    }
    return 0;
}

// ---- mean pooling (pool.inc) ----
// `plan_check pool`: lines "n d row_stride base elem_bytes normalize" -> ncb waves grid_x grid_y aligned, or "refused"
static int run_pool()
{
    long long n, d, stride;
    unsigned long long base;
    int elem, normalize;
    while (scanf("%lld %lld %lld %llu %d %d", &n, &d, &stride, &base, &elem, &normalize) == 6) {
        PoolPlan p;
        if (!plan_pool(n, d, stride, (uintptr_t)base, elem, normalize != 0, &p)) {
            printf("refused\n");
            continue;
        }
        printf("%d %d %lld %d %d\n", p.ncb, p.waves, (long long)p.grid_x, p.grid_y, (int)p.aligned);
    }
    return 0;
}

// `plan_check poolchunks`: the line "n chunk_rows", then n lines "start stop" -> per chunk "row0 row1 count: the ranges' indices"
static int run_poolchunks()
{
    long long n, chunk_rows;
    if (scanf("%lld %lld", &n, &chunk_rows) != 2 || n < 0 || chunk_rows < 1) return 2;
    std::vector<int64_t> starts((size_t)n), stops((size_t)n), order;
    for (long long i = 0; i < n; i++) {
        long long a, b;
        if (scanf("%lld %lld", &a, &b) != 2) return 2;
        starts[(size_t)i] = a;
        stops[(size_t)i] = b;
    }
    std::vector<PoolChunk> chunks;
    pool_assign_chunks(starts.data(), stops.data(), n, chunk_rows, order, chunks);
    for (const PoolChunk &c : chunks) {
        printf("%lld %lld %lld:", (long long)c.row0, (long long)c.row1, (long long)c.count);
        for (int64_t i = 0; i < c.count; i++) printf(" %lld", (long long)order[(size_t)(c.first + i)]);
        printf("\n");
    }
    return 0;
}

// ---- kernel density estimates (kde.inc) ----
// `plan_check kde`: lines "n ncols m" -> group_rows groups tiles chunks tail_rows tail_points part_bytes, or "refused"
static int run_kde()
{
    long long n, ncols, m;
    while (scanf("%lld %lld %lld", &n, &ncols, &m) == 3) {
        KdePlan p;
        if (!plan_kde(n, ncols, m, &p)) {
            printf("refused\n");
            continue;
        }
        printf("%lld %d %lld %lld %d %d %lld\n", (long long)p.group_rows, p.groups, (long long)p.tiles, (long long)p.chunks, p.tail_rows, p.tail_points,
               (long long)p.part_bytes);
    }
    return 0;
}

// every row is in one group and one chunk, every grid point in one tile; the grid fits a launch
static void check_kde(int64_t n, int64_t ncols, int64_t m)
{
    const auto where = [&] { return describe("kde n %lld ncols %lld m %lld", (long long)n, (long long)ncols, (long long)m); };
    KdePlan p;
    const bool legal = n >= 2 && n <= KNN_KDE_MAX_ROWS && ncols >= 1 && ncols <= KNN_KDE_MAX_COLS && m >= 1 && m <= KNN_KDE_MAX_POINTS;
    if (!plan_kde(n, ncols, m, &p)) {
        INVARIANT(!legal);
        return;
    }
    INVARIANT(legal);
    INVARIANT(p.group_rows % 4096 == 0 && p.groups >= 1 && p.groups <= 256);
    INVARIANT((int64_t)(p.groups - 1) * p.group_rows < n && (int64_t)p.groups * p.group_rows >= n);
    INVARIANT(p.chunks >= 1 && p.chunks <= 65535 && (p.chunks - 1) * KDE_CHUNK + p.tail_rows == n && p.tail_rows >= 1 && p.tail_rows <= KDE_CHUNK);
    INVARIANT(p.tiles >= 1 && p.tiles <= INT32_MAX && (p.tiles - 1) * KDE_TILE + p.tail_points == m && p.tail_points >= 1 && p.tail_points <= KDE_TILE);
    INVARIANT(ncols <= 65535 && p.part_bytes == ncols * p.chunks * m * 8);
}

static void sweep_kde()
{
    const int64_t ns[] = {0, 1, 2, 255, 256, 257, 4096, 4097, 16383, 16384, 16385, 40000, 200000, 4096 * 256, 4096 * 256 + 1, 1048581,
                          KNN_KDE_MAX_ROWS - 1, KNN_KDE_MAX_ROWS, KNN_KDE_MAX_ROWS + 1};
    const int64_t ms[] = {0, 1, 15, 16, 17, 1000, KNN_KDE_MAX_POINTS, KNN_KDE_MAX_POINTS + 1};
    const int64_t cs[] = {0, 1, 3, 12, KNN_KDE_MAX_COLS, KNN_KDE_MAX_COLS + 1};
    for (int64_t n : ns)
        for (int64_t m : ms)
            for (int64_t c : cs) check_kde(n, c, m);
}

// every (range, column) pair of a launch is owned by exactly one (workgroup, wave, lane, element); the waves divide 64 in the
// normalizing build; the grid fits; aligned is the pointer's and the stride's doing
static void check_pool(int64_t n, int64_t d, int64_t stride, uintptr_t base, int elem, bool normalize)
{
    PoolPlan p;
    const auto where = [&] {
        return describe("pool n %lld d %lld stride %lld base %llx elem %d normalize %d", (long long)n, (long long)d, (long long)stride, (unsigned long long)base, elem,
                        (int)normalize);
    };
    g_checked++;
    const bool legal = n >= 1 && n <= INT32_MAX && d >= 2 && d <= KNN_POOL_MAX_D && stride >= d && (elem == 2 || elem == 4);
    if (!plan_pool(n, d, stride, base, elem, normalize, &p)) {
        INVARIANT(!legal);
        return;
    }
    INVARIANT(legal);
    INVARIANT(p.grid_x == n && p.grid_y >= 1 && p.grid_y <= 65535 && p.waves >= 1 && p.waves <= POOL_MAX_WAVES);
    INVARIANT(p.ncb == (d + POOL_COLS - 1) / POOL_COLS && p.grid_y == (p.ncb + p.waves - 1) / p.waves);
    INVARIANT(!normalize || POOL_NORM_ROWS % p.waves == 0);
    INVARIANT(normalize || p.waves <= 4);
    INVARIANT((int64_t)(p.grid_y - 1) * p.waves < p.ncb); // (no workgroup without a column block)
    INVARIANT(p.aligned == (base % (uintptr_t)(4 * elem) == 0 && stride % 4 == 0));
    // the kernel's own arithmetic: c0 = (y * waves + wave) * 256 + 4 * lane, nvalid = min(4, d - c0)
    if (d > 8192 && (n != 1 || base != 0x1000)) return; // (the widest rows once per build, not per pointer and count)
    std::vector<uint8_t> owners((size_t)d, 0);
    for (int y = 0; y < p.grid_y; y++)
        for (int w = 0; w < p.waves; w++)
            for (int lane = 0; lane < 64; lane++) {
                const int64_t c0 = ((int64_t)y * p.waves + w) * POOL_COLS + 4 * lane;
                for (int64_t e = 0; e < std::min<int64_t>(4, d - c0); e++) owners[(size_t)(c0 + e)]++;
            }
    bool once = true;
    for (uint8_t v : owners) once = once && v == 1;
    INVARIANT(once);
}

// every range in exactly one chunk and inside its rows; chunks within the budget, but for a chunk that begins with a longer range
static void check_pool_chunks(const std::vector<int64_t> &starts, const std::vector<int64_t> &stops, int64_t chunk_rows)
{
    std::vector<int64_t> order;
    std::vector<PoolChunk> chunks;
    const int64_t n = (int64_t)starts.size();
    const auto where = [&] { return describe("pool chunks: %lld ranges, first %lld-%lld, chunk_rows %lld", (long long)n, (long long)starts[0], (long long)stops[0], (long long)chunk_rows); };
    g_checked++;
    pool_assign_chunks(starts.data(), stops.data(), n, chunk_rows, order, chunks);
    std::vector<int> seen((size_t)n, 0);
    int64_t next = 0;
    bool ok = (int64_t)order.size() == n;
    for (const PoolChunk &c : chunks) {
        ok = ok && c.first == next && c.count >= 1 && c.first + c.count <= n;
        if (!ok) break;
        next += c.count;
        int64_t hi = 0;
        for (int64_t i = 0; i < c.count; i++) {
            const int64_t o = order[(size_t)(c.first + i)];
            ok = ok && o >= 0 && o < n && starts[(size_t)o] >= c.row0 && stops[(size_t)o] <= c.row1;
            if (!ok) break;
            seen[(size_t)o]++;
            hi = std::max(hi, stops[(size_t)o]);
        }
        const int64_t o0 = order[(size_t)c.first];
        ok = ok && hi == c.row1 && starts[(size_t)o0] == c.row0;
        ok = ok && (c.row1 - c.row0 <= chunk_rows || (stops[(size_t)o0] - starts[(size_t)o0] > chunk_rows && stops[(size_t)o0] == c.row1));
    }
    ok = ok && next == n;
    for (int v : seen) ok = ok && v == 1;
    INVARIANT(ok);
}

static void sweep_pool()
{
    const int64_t ds[] = {-1, 0, 1, 2, 3, 4, 8, 20, 255, 256, 257, 1023, 1024, 1025, 1028, 3072, 4095, 4097, 5000, KNN_POOL_MAX_D, KNN_POOL_MAX_D + 1};
    for (int64_t d : ds)
        for (int64_t n : {(int64_t)0, (int64_t)1, (int64_t)7, (int64_t)INT32_MAX, (int64_t)INT32_MAX + 1})
            for (int64_t extra : {(int64_t)-1, (int64_t)0, (int64_t)1, (int64_t)2, (int64_t)4})
                for (uintptr_t base : {(uintptr_t)0x1000, (uintptr_t)0x1002, (uintptr_t)0x1004, (uintptr_t)0x1008, (uintptr_t)0x1010})
                    for (int elem : {1, 2, 4, 8})
                        for (int normalize = 0; normalize < 2; normalize++) check_pool(n, d, d + extra, base, elem, normalize != 0);
    // chunk assignment: seeded ranges (overlapping, unordered, duplicates, all rows) against every budget around their lengths
    uint64_t state = 12345;
    auto rnd = [&](int64_t m) {
        state = state * 6364136223846793005ull + 1442695040888963407ull;
        return (int64_t)((state >> 33) % (uint64_t)m);
    };
    for (int round = 0; round < 40; round++) {
        const int64_t rows = 1 + rnd(400), n = 1 + rnd(40);
        std::vector<int64_t> starts, stops;
        for (int64_t i = 0; i < n; i++) {
            const int64_t a = rnd(rows);
            starts.push_back(a);
            stops.push_back(a + 1 + rnd(std::min<int64_t>(rows - a, 1 + rnd(120))));
        }
        starts.push_back(0);
        stops.push_back(rows);
        starts.push_back(starts[0]);
        stops.push_back(stops[0]);
        for (int64_t chunk_rows : {(int64_t)1, (int64_t)2, (int64_t)7, (int64_t)64, (int64_t)119, (int64_t)120, rows - 1, rows, rows + 1, (int64_t)1 << 40})
            if (chunk_rows >= 1) check_pool_chunks(starts, stops, chunk_rows);
    }
}

// ---- weighted layer mixes (mix.inc) ----
// `plan_check mix`: lines "n d dp nlayers out_base base0 stride0 ... base3 stride3" (four pairs, those past nlayers ignored)
// -> vec per_row items grid, or "refused"; every plan that is not refused is walked as mix_rows_kernel walks it, a wrong
// walk prints "broken"
static int run_mix()
{
    long long n, d, dp, stride[KNN_MIX_MAX_LAYERS];
    unsigned long long out_base, base[KNN_MIX_MAX_LAYERS];
    int nlayers;
    while (scanf("%lld %lld %lld %d %llu %llu %lld %llu %lld %llu %lld %llu %lld", &n, &d, &dp, &nlayers, &out_base, &base[0], &stride[0], &base[1], &stride[1],
                 &base[2], &stride[2], &base[3], &stride[3]) == 13) {
        uintptr_t bases[KNN_MIX_MAX_LAYERS];
        int64_t strides[KNN_MIX_MAX_LAYERS];
        for (int i = 0; i < KNN_MIX_MAX_LAYERS; i++) {
            bases[i] = (uintptr_t)base[i];
            strides[i] = stride[i];
        }
        MixPlan p;
        if (!plan_mix(n, d, dp, nlayers, bases, strides, (uintptr_t)out_base, &p)) {
            printf("refused\n");
            continue;
        }
        bool ok = p.grid >= 1 && p.grid <= MIX_MAX_GRID && p.items == n * p.per_row && p.per_row == (p.vec ? dp / 4 : dp);
        ok = ok && (int64_t)p.grid * MIX_BLOCK >= std::min<int64_t>(p.items, (int64_t)MIX_MAX_GRID * MIX_BLOCK);
        // the kernel's own walk, for outputs small enough to count: every float of [n][dp] is written exactly once, nothing
        // is read at or past column d, and the running (row, item) pair is the item's quotient and remainder
        if (ok && n * dp <= (1 << 22)) {
            std::vector<uint8_t> written((size_t)(n * dp), 0);
            const int64_t step = (int64_t)p.grid * MIX_BLOCK;
            for (int64_t first = 0; first < step && ok; first++) {
                int64_t r = first / p.per_row;
                int q = (int)(first - r * p.per_row);
                const int64_t step_r = step / p.per_row;
                const int step_q = (int)(step - step_r * p.per_row);
                for (int64_t it = first; it < p.items; it += step) {
                    ok = ok && r == it / p.per_row && q == it % p.per_row && r < n;
                    const int c0 = p.vec ? 4 * q : q;
                    for (int e = 0; e < (p.vec ? 4 : 1); e++) {
                        ok = ok && c0 + e < dp;
                        if (ok) written[(size_t)(r * dp + c0 + e)]++;
                    }
                    r += step_r;
                    q += step_q;
                    if (q >= p.per_row) {
                        q -= p.per_row;
                        r++;
                    }
                }
            }
            for (uint8_t v : written) ok = ok && v == 1;
        }
        if (!ok) printf("broken\n");
        else printf("%d %d %lld %d\n", (int)p.vec, p.per_row, (long long)p.items, p.grid);
    }
    return 0;
}

// `plan_check mixargs`: lines "d nlayers layers_set flat_d flat_is_view sweep g k column nlevels" -> "ok", or the refusal's message
static int run_mixargs()
{
    int d, nlayers, flat_d, is_view, sweep;
    unsigned set;
    long long g, k, column, nlevels;
    while (scanf("%d %d %u %d %d %d %lld %lld %lld %lld", &d, &nlayers, &set, &flat_d, &is_view, &sweep, &g, &k, &column, &nlevels) == 10) {
        const char *why = mix_args_illegal(d, nlayers, set, flat_d, is_view != 0, sweep != 0, g, k, column, nlevels);
        printf("%s\n", why ? why : "ok");
    }
    return 0;
}

// `plan_check s16`: lines "nb nq k flags" -> the prefilter's eligibility and k' for the fp16 and the 12-bit row copies
static int run_s16()
{
    long long nb, nq;
    int k, flags;
    while (scanf("%lld %lld %d %d", &nb, &nq, &k, &flags) == 4) {
        const PlanCtx c = make_ctx(nb, nq, KNN_METRIC_INNER_PRODUCT, flags, 0, 0, 0, false);
        printf("%lld %lld %d %d: fp16 kprime %d eligible %d, 12-bit kprime %d eligible %d\n", nb, nq, k, flags, s16_kprime(k, 16),
               (int)s16_eligible(c, 0, nb, nq, k, 1, 0, 1024, 16), s16_kprime(k, 12), (int)s16_eligible(c, 0, nb, nq, k, 1, 0, 1024, 12));
    }
    return 0;
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
    // a forced chunk count, a piece of a larger batch; the symmetric self-search of every eligible (n, k, flags, can_stream) and
    // the range scan of every (n, nq, metric)
    for (int64_t nb : nbs)
        for (int64_t nq : nqs)
            for (int k : ks)
                for (int metric = 0; metric < 2; metric++) {
                    check_batch(make_ctx(nb, nq, metric, 0, 0, 0, 0, true), nq, k, false);
                    check_batch(make_ctx(nb, nq, metric, 0, 0, 3, 0, false), nq, k, true);
                    check_batch(make_ctx(nb, nq, metric, 0, 0, 0, 100, false), nq, k, true);
                    if (nq == 1) // (a self-search has no query count of its own)
                        for (int flags : flagset)
                            for (int can_stream = 0; can_stream < 2; can_stream++) check_sym(make_ctx(nb, nb, metric, flags, 0, 0, 0, false), k, can_stream != 0);
                    check_range(make_ctx(nb, nq, metric, 0, 0, 0, 0, false), nq);
                }
    // the device-wide rank: sizes around every internal width, the largest legal one, and illegal ones
    const int64_t rank_rows[] = {0, 1, 2, 7, RANK_SCAN_BLOCK - 1, RANK_SCAN_BLOCK, RANK_SCAN_BLOCK + 1, RANK_TILE - 1, RANK_TILE, RANK_TILE + 1, 3 * RANK_TILE + 5,
                                 (int64_t)RANK_SCAN_TOP * RANK_SCAN_BLOCK + 1, (int64_t)(RANK_SCAN_TOP * (RANK_SCAN_BLOCK / 256) + 1) * RANK_TILE + 5, 200000,
                                 7158278, 2147483647, 2147483648LL, INT64_MAX};
    const int64_t rank_limits[] = {0, 1, 2, 10, 300, 301, 2147483647, INT64_MAX};
    for (int64_t rows : rank_rows)
        for (int64_t limit : rank_limits) {
            // k around the limit and around the packing rule's 2 * limit, and at the edge of what a kernel's int holds
            std::vector<int64_t> ks = {limit};
            if (limit <= (int64_t)INT32_MAX) ks = {limit - 1, limit, limit + 1, 2 * limit - 1, 2 * limit, (int64_t)INT32_MAX, (int64_t)INT32_MAX + 1};
            for (int64_t k : ks)
                for (int key_bytes : {2, 4, 8})
                    for (int outs = 0; outs < 8; outs++) check_rank(rows, k, limit, key_bytes, outs);
        }
    // the pooling launch of every (n, d, stride, base, element size, build) and the host entry's chunks
    sweep_pool();
    // the density launch: groups, chunks and tiles cover every row and grid point once
    sweep_kde();
    printf("plan_check sweep: %lld plans checked, %lld broken\n", g_checked, g_broken);
    return g_broken ? 1 : 0;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !strcmp(argv[1], "cases")) return run_cases();
    if (argc == 2 && !strcmp(argv[1], "sym")) return run_sym();
    if (argc == 2 && !strcmp(argv[1], "range")) return run_range();
    if (argc == 2 && !strcmp(argv[1], "s16")) return run_s16();
    if (argc == 2 && !strcmp(argv[1], "rank")) return run_rank();
    if (argc == 2 && !strcmp(argv[1], "pool")) return run_pool();
    if (argc == 2 && !strcmp(argv[1], "poolchunks")) return run_poolchunks();
    if (argc == 2 && !strcmp(argv[1], "kde")) return run_kde();
    if (argc == 2 && !strcmp(argv[1], "mix")) return run_mix();
    if (argc == 2 && !strcmp(argv[1], "mixargs")) return run_mixargs();
    if (argc == 2 && !strcmp(argv[1], "sweep")) return run_sweep();
    fprintf(stderr, "usage: plan_check cases|sym|range|s16|rank|pool|poolchunks|kde|mix|mixargs < lines | plan_check sweep\n");
    return 2;
}
