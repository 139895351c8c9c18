// The planners of the flat search, the symmetric self-search and the range scan: which kernel build runs, over how many chunks
// or runs of tiles, with which seed, with how much LDS, and how a batch is cut into pieces.  Plain host arithmetic on (nb, nq,
// k, metric, flags, num_cus): no HIP header, no handle -- flat_search.inc copies what the rules read into a PlanCtx (plan_ctx) and
// launches what plan_pieces / plan_search / plan_self_symmetric / plan_range return; plan_check.cpp runs the same rules on a
// machine without a GPU.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <math.h>
#include <algorithm>
#include <vector>

#include "../../include/knn355.h"

// what the rules read from an index handle
struct PlanCtx {
    int metric = KNN_METRIC_INNER_PRODUCT;
    bool approx16 = false;        // the scan multiplies bf16 copies (HNSW's coarse entry index)
    int flags = 0, force_qt = 0, force_chunks = 0; // knn_set_tuning
    int num_cus = 256;
    int64_t batch_nq = 0;         // the caller's whole batch while a search works through it in pieces (0: this call is the batch)
    int pub_rounds_force = 0;     // tile-minimum seed: rounds of publications (0: the planner's choice)
    int64_t ntotal = 0;
    int s16_fmt = 16;             // the prefilter's row copies: 16 = fp16, 12 = 12-bit tiles (knn_flat_set_scan16 mode 2)
};

// rows of the view with stride row_mul over a database of n rows
static inline int64_t view_rows(int64_t n, int row_mul, int vshift)
{
    const int64_t B = (int64_t)1 << vshift, span = B * row_mul;
    if (n <= 0) return 0;
    const int64_t last = (n - 1) / span; // last block that starts inside the database
    return last * B + std::min<int64_t>(B, n - last * span);
}

// ---- search ---------------------------------------------------------------
// A chunk hands on at most kslot = 1.25 k keys per query (k for k > 1536); the final selection
// is exact.  The register select inside the scan kernels serves k <= 1536 (lists of <= 2048
// keys, 32 per lane, so that 1.25 k + one tile fits); beyond that the workgroup sort takes
// exactly k.
static const int KNN_WAVE_SELECT_MAX_K = 2048;    // one wave selects a list: in registers up to ...
// ... this k (2048-key lists), by probing a 4096-key list in memory beyond.  1.25 k keys + a tile of appends fit a 2048-key
// list up to k = 1536, but the closer k gets the less room a cut leaves and the more often a list is cut: measured crossover
// at k ~ 1400 (2 M rows x 1024 queries: k = 1400 43.4 ms either way, k = 1536 51.3 ms with 2048-key lists, 44.8 with 4096)
static const int KNN_REGISTER_SELECT_MAX_K = 1400;
// (developer build: integer knobs from the environment; the shipped library has the defaults compiled in)
static int dev_knob(const char *name, int dflt)
{
#ifdef KNN355_DEV
    if (getenv(name)) return atoi(getenv(name));
#endif
    (void)name;
    return dflt;
}
static int knn_kslot(int k) { return k > KNN_WAVE_SELECT_MAX_K ? k : k + k / 4; }

static int next_pow2_host(int n)
{
    int p = 64;
    while (p < n) p <<= 1;
    return p;
}

struct ScanPlan {
    int qt, dt, nqtiles, nchunks, cap, grid;
    int npairs; // > 0: paired walk -- grid = nchunks = 2 npairs workgroups, tiles_base / tiles_rem split the tiles over the PAIRS
    bool diff;  // squared L2 as the sum of squared differences (FAISS's small-batch formula), see flat_scan_kernel<..., DIFF>
    int64_t chunk_rows;
    int tiles_base, tiles_rem;
    size_t lds;
    const char *name;
};

// the difference build that serves a batch of nq < 20 queries: its width (a multiple of 4: two query pairs per thread half)
// (no 4-query build: with two chains per thread it is bound by their dependent latency -- 6.9 ms per 10 M rows where the 8-query
// build, four chains per thread, reads at the HBM rate: 6.25 ms)
static int diff_build_width(int64_t nq) { return nq <= 8 ? 8 : (nq <= 12 ? 12 : (nq <= 16 ? 16 : 20)); }

// Dynamic LDS of one flat_scan_kernel workgroup with a qt x dt tile and cap-key lists, as the kernel lays it out: lds_main (the
// two staging buffers of (dt + qt) rows x 128 bytes, re-used for a cap-key list when it is cut; the symmetric 128-row build
// asks for main_min = 72 KB, see lds_main there), then L.s_thr, L.s_cnt ([qt] each), L.s_need (4 words), s_base ([qt]), s_yn
// ([dt]) and s_pub ([qt] keys; a symmetric launch has s_thr2, s_cnt2, s_base2 there and adds them itself).
static size_t scan_lds_bytes(int qt, int dt, int cap, size_t main_min = 0)
{
    return std::max(main_min, std::max((size_t)2 * (dt + qt) * 128, (size_t)cap * 8)) + (size_t)qt * 12 + 16 + (size_t)dt * 4 + (size_t)qt * 8;
}

// knn_set_tuning rules that several plan decisions share
// the statistical seed may run: seeding on, the exact seed not forced, the estimate not forbidden
static bool stat_seed_allowed(const PlanCtx &c) { return !(c.flags & (KNN_TUNE_NO_SEED | KNN_TUNE_EXACT_SEED | KNN_TUNE_NO_STAT_SEED)); }
// the tile-minimum seed may run: seeding on, neither the exact nor the statistical seed forced, the tile-minimum seed not forbidden
static bool tile_min_seed_allowed(const PlanCtx &c)
{
    return !(c.flags & (KNN_TUNE_NO_SEED | KNN_TUNE_EXACT_SEED | KNN_TUNE_STAT_SEED | KNN_TUNE_NO_TILE_MIN_SEED));
}

// Does the 256 x 256 tile (flat_scan_kernel<2, 2, 4, 4>: one workgroup per CU) serve this search?  Its K loop keeps the matrix
// pipe busier than two co-resident 128 x 128 workgroups do, but nothing hides its epilogues, a launch has half the
// workgroups and four times the tile: it wants long chunks on every CU -- Pfam-sized batches, not CATH-sized ones.
// KNN_TUNE_NO_BIG_TILE: never; KNN_TUNE_BIG_TILE: wherever a batch has more than 128 queries (tests, A/B).
static bool big_tile_pays(const PlanCtx &c, int64_t nb, int64_t nq)
{
    if (c.approx16 || (c.flags & KNN_TUNE_NO_BIG_TILE) || nq <= 128) return false;
    if (c.flags & KNN_TUNE_BIG_TILE) return nb >= 1024;
    if (nb < 65536) return false; // (never a seed sample's own scan)
    const int64_t cus = std::max(1, c.num_cus);
    const int64_t work = ((nq + 255) / 256) * ((nb + 255) / 256); // 256 x 256 tiles of the search
    // (24 tiles per CU: 1 M rows x 512 queries 8.27 against 8.78 ms, 500 k x 1024 8.16 against 8.47, 400 k x 1024 7.11 against 7.3,
    // 200 k x 2048 6.73 against 6.80 -- the bound was 32 until late in round 5.)
    // (from ONE wide query tile on: 10 M rows x 256 / 512 / 768 / 1024 / 1536 queries 38.1 / 79.1 / 117.6 / 152.4 / 234.4 ms against
    // 41.4 / 89.4 / 130.8 / 172.0 / 248.8 on the 128 x 128 tile, one box; until late in round 5 the bound was 2048)
    return nq >= dev_knob("KNN355_BIG_MIN_NQ", 256) && work >= (int64_t)dev_knob("KNN355_BIG_MIN_TILES_PER_CU", 24) * cus;
}

// what a make_plan call may choose
struct PlanOpts {
    bool seeded = false;      // the chunks start from a seed's thresholds (or are a seed sample's own: parallelism over warm-up)
    bool allow_pairs = false; // a one-query-tile launch may pair its workgroups
    bool allow_big = true;    // the 256 x 256 tile may serve it
};

static void make_plan(const PlanCtx &c, int64_t nb, int64_t nq, int k, const PlanOpts &o, ScanPlan &pl)
{
    const bool seeded = o.seeded, allow_pairs = o.allow_pairs, allow_big = o.allow_big;
    int qt = c.force_qt;
    // (48 and 96: the 16-query-block builds, one query tile per launch only -- a forced one is honoured if it holds the batch)
    if ((qt == 48 || qt == 96) && (nq > qt || c.approx16)) qt = 0;
    if (qt == 256 && (c.approx16 || nq <= 128)) qt = 0; // (the 256 x 256 tile: plain fp32 rows, more than one 128-query tile of queries)
    if (qt != 32 && qt != 48 && qt != 64 && qt != 96 && qt != 128 && qt != 256) {
        qt = nq <= 32 ? 32 : (nq <= 64 ? 64 : 128);
        if (!c.approx16 && !(c.flags & KNN_TUNE_NO_Q16)) { // (KNN_TUNE_NO_Q16: without the 16-query-block builds)
            if (nq > 32 && nq <= 48) qt = 48;
            else if (nq > 64 && nq <= 96) qt = 96;
        }
        if (allow_big && big_tile_pays(c, nb, nq)) qt = 256;
    }
    // FAISS's squared L2 for fewer than 20 queries: the sum of squared differences (KNN_TUNE_NORM_L2: the norm formula throughout).
    // FAISS decides on the batch its caller handed over, so a piece of a larger batch (the last block of 16384 queries, the
    // remainder behind the full query tiles) keeps the formula of the whole.
    const bool small_batch = (c.batch_nq ? c.batch_nq : nq) < 20 && nq < 20;
    if (c.metric == KNN_METRIC_L2 && small_batch && !c.approx16 && !(c.flags & KNN_TUNE_NORM_L2)) qt = 32; // (the difference build exists for the 32-query tile only)
    pl.qt = qt;
    pl.dt = (qt == 32 || qt == 48 || qt == 256) ? 256 : 128;
    pl.diff = c.metric == KNN_METRIC_L2 && small_batch && qt == 32 && !c.approx16 && !(c.flags & KNN_TUNE_NORM_L2);
    pl.name = pl.diff ? "flat_scan_q32_d256_l2diff"
                      : (qt == 256 ? "flat_scan_q256_d256" : qt == 128 ? "flat_scan_q128_d128" : (qt == 96 ? "flat_scan_q96_d128" : (qt == 64 ? "flat_scan_q64_d128" : (qt == 48 ? "flat_scan_q48_d256" : "flat_scan_q32_d256"))));
    pl.nqtiles = (int)((nq + qt - 1) / qt);
    pl.cap = next_pow2_host(2 * k + pl.dt);
    if (pl.cap < 512) pl.cap = 512;
    // (the 256 x 256 tile: nothing hides a cut of its 256 lists on four waves -- 220 us, a K loop's worth: room for three tiles
    // of appends between cuts)
    if (qt == 256 && pl.cap < 1024) pl.cap = 1024;
    int regsel_max = KNN_REGISTER_SELECT_MAX_K;
#ifdef KNN355_DEV
    if (getenv("KNN355_REGSEL_MAX_K")) regsel_max = atoi(getenv("KNN355_REGSEL_MAX_K")); // (developer build: where the 4096-key lists take over)
#endif
    if (k <= regsel_max) pl.cap = std::min(pl.cap, 2048); // register select: <= 32 keys per lane
    else if (k <= KNN_WAVE_SELECT_MAX_K) pl.cap = std::min(pl.cap, 4096);  // wave_select_mem: 1.25 k + a tile of appends fit
    const int64_t ntiles = (nb + pl.dt - 1) / pl.dt;
    pl.npairs = 0;
    if (allow_pairs && pl.nqtiles == 1 && qt != 256 && c.force_chunks <= 0 && !(c.flags & KNN_TUNE_NO_PAIRS) && ntiles >= (int64_t)dev_knob("KNN355_PAIR_MIN_TILES", 64)) {
        // one query tile, plenty of tiles: two workgroups per CU, paired (see flat_scan_kernel): each pair shares a
        // contiguous range of ~ ntiles / CUs tiles (at least two: fewer pairs than CUs on a small database)
        pl.npairs = (int)std::min<int64_t>(std::max(1, c.num_cus), ntiles / 2);
        pl.nchunks = 2 * pl.npairs;
        pl.grid = pl.nchunks;
        pl.tiles_base = (int)(ntiles / pl.npairs);
        pl.tiles_rem = (int)(ntiles % pl.npairs);
        pl.chunk_rows = (int64_t)(pl.tiles_base + (pl.tiles_rem ? 1 : 0)) * pl.dt;
        pl.lds = scan_lds_bytes(pl.qt, pl.dt, pl.cap);
        return;
    }
    // workgroups resident per CU: two, or the one 256 x 256 workgroup
    const int per_cu = qt == 256 ? 1 : 2;
    int64_t want = c.force_chunks > 0 ? c.force_chunks : (512 * per_cu + pl.nqtiles - 1) / pl.nqtiles;
    // an unseeded chunk should see enough rows to amortise its threshold warm-up; a seeded pass
    // starts with good thresholds and a tiny view (a seed sample) just wants parallelism
    int64_t min_tiles = std::max<int64_t>(2, (4 * (int64_t)k + pl.dt - 1) / pl.dt);
    if (c.force_chunks <= 0 && !seeded && nb >= 8192) want = std::min(want, std::max<int64_t>(1, ntiles / min_tiles));
    want = std::max<int64_t>(1, std::min(want, ntiles));
    // bound the candidate-list workspace (<= 2 GiB)
    const size_t per_wg = (size_t)qt * pl.cap * 8;
    int64_t max_wgs = std::max<int64_t>(pl.nqtiles, (int64_t)((2ull << 30) / per_wg));
    const int64_t want_max = std::max<int64_t>(1, std::min(ntiles, max_wgs / pl.nqtiles));
    want = std::min(want, want_max);
    if (c.force_chunks <= 0) {
        // wave quantisation: workgroups run in rounds of (2 per CU); pick the chunk count near
        // `want` that minimises rounds x tiles-per-chunk (14433 x 14433: 9 chunks = 2 full
        // rounds of 13 tiles beat 10 chunks = 2.2 rounds of 12)
        const int64_t slots = per_cu * (int64_t)std::max(1, c.num_cus);
        int64_t best = want, best_cost = INT64_MAX;
        for (int64_t n = std::max<int64_t>(1, want / 2); n <= std::min(want_max, want + want / 2 + 1); n++) {
            const int64_t rounds = (pl.nqtiles * n + slots - 1) / slots;
            // per chunk: its tiles + about half a tile of fixed work (prologue, cutting the lists
            // and writing the survivors) -- 1.25 M rows x 32 queries: 489 chunks of 10 tiles in
            // one round beat 977 chunks of 5 tiles in two
            const int64_t cost = rounds * (2 * ((ntiles + n - 1) / n) + 1);
            if (cost < best_cost || (cost == best_cost && n > best)) { best = n; best_cost = cost; }
        }
        want = best;
    }
    int64_t tiles_per = (ntiles + want - 1) / want;
    // balanced split: the first (ntiles mod nchunks) chunks walk one tile more.  (A uniform chunk length left the
    // last chunk short -- 14433 rows in 9 chunks: 8 x 13 tiles + 9 -- and the two rounds of workgroups took 13 + 13
    // tile times; 5 x 13 + 4 x 12 takes 13 + 12.)
    pl.nchunks = (int)((ntiles + tiles_per - 1) / tiles_per);
    pl.tiles_base = (int)(ntiles / pl.nchunks);
    pl.tiles_rem = (int)(ntiles % pl.nchunks);
    pl.chunk_rows = (int64_t)(pl.tiles_base + (pl.tiles_rem ? 1 : 0)) * pl.dt; // (the longest chunk)
    pl.grid = pl.nqtiles * pl.nchunks;
    pl.lds = scan_lds_bytes(pl.qt, pl.dt, pl.cap);
}

// Seed stride of a view with nb rows: a power of two s such that the sample (every s-th 8-row block)
// has about max(2 * chunk_rows, 64 k) rows (and at most nb/8).  The sample is searched first,
// exactly; its k-th score bounds the global k-th from above, so every chunk of the main pass
// starts with a tight threshold and appends about chunk_rows * k / sample_rows <= k/2
// candidates per query instead of warming up (and compacting) on its own.
static int seed_stride(int64_t nb, int k, int64_t chunk_rows)
{
    const int64_t target = std::min<int64_t>(std::max<int64_t>(2 * chunk_rows, 64 * (int64_t)k), nb / 8);
    int s = 8;
    while ((int64_t)s * 2 * target <= nb && s < (1 << 20)) s *= 2;
    return s;
}

// Statistical seed (batch regime).  The exact seed above needs a sample of >= k rows whose k-th
// score is a PROVEN bound of the global k-th: with k = 301 of 14433 rows no affordable sample gives a
// useful one, every chunk warms up on its own and half of all scores go through the candidate lists.
// Instead: T = the j-th best score of a sample of S rows, j << k chosen so that, were the sample
// drawn at random, fewer than k of the N rows beat T with probability <= 1e-9 per query
// (P[Binomial(S, k/N) >= j] <= 1e-9).  Every chunk filters with T from its first tile on (about
// j N / S candidates per query instead of ~ chunks x k (1 + ln(rows per chunk / k))).  T is only
// an estimate, so the result is VERIFIED: the final selection checks that the k-th score it found is
// <= T -- then at least k rows beat T, all of them were candidates, and the result is exact.  A
// query that fails the check raises a flag and the search is redone without the estimate (the
// caller must be able to wait for the flag: synchronous entry points only).
static int stat_seed_rank(int64_t S, int64_t N, int k)
{
    if (S < 64 || N <= 0 || k >= N) return -1;
    const double pr = (double)k / (double)N, eps = 1e-9;
    // smallest j with P[Bin(S, pr) >= j] <= eps: walk the pmf upwards, accumulating the lower tail
    const double lp = log(pr), lq = log1p(-pr);
    double cdf = 0.0;
    const int64_t jmax = std::min<int64_t>(S, k);
    for (int64_t i = 0; i <= jmax; i++) {
        if (1.0 - cdf <= eps) return i >= 1 ? (int)i : 1; // P[X >= i] = 1 - P[X <= i-1]
        cdf += exp(lgamma((double)S + 1.0) - lgamma((double)i + 1.0) - lgamma((double)(S - i) + 1.0) + (double)i * lp + (double)(S - i) * lq);
    }
    return -1; // would need more than min(S, k) sample hits: no statistical seed
}

// approximate keys the 16-bit pass hands to the re-scoring tail: room for the window above the k-th (fp16 on normalised
// rows: a few percent of k beyond it at 10 M rows, k = 100)
// (fmt: the row copies' format, 16 = fp16, 12 = 12-bit fixed point -- its copy error R is about five times fp16's, so its
// window is wider: 62 rows expected beyond the k-th at 10 M normalised rows, k = 100, against 24)
static int s16_kprime(int k, int fmt = 16)
{
    if (fmt == 12) return std::min(KNN_WAVE_SELECT_MAX_K, std::max(3 * k, k + 128));
    return std::min(KNN_WAVE_SELECT_MAX_K, std::max(2 * k, k + 64));
}

// Does a search of the view take the prefiltered path?  A one-query-tile streaming search (the 32-query build) by inner
// product over an index whose fp16 copies cover every row, from nb >= 2^18 rows on (below that the fp32 scan's fixed costs
// dominate and the tail's launches would not pay).  Batch, symmetric, difference, HNSW and range searches never do.
// (the shape's half of the question; whether the copies exist and the search seeds no other is asked where the handle is: search_view.
// dp: floats per padded row)
static bool s16_eligible(const PlanCtx &c, int pass_mode, int64_t nb, int64_t nq, int k, int row_mul, int level, int dp, int fmt = 16)
{
    if (pass_mode || level != 0 || row_mul != 1) return false;
    if (c.metric != KNN_METRIC_INNER_PRODUCT || c.approx16 || (c.flags & KNN_TUNE_NO_SCAN16)) return false;
    if (nq < 1 || nq > 32 || (c.force_qt != 0 && c.force_qt != 32) || s16_kprime(k, fmt) <= k) return false; // (k' = k: no room for a window)
    if ((size_t)dp * 4 + 64 > 65536) return false; // (the widest row the path has served: rescore16_kernel walks a row in 1024-float slabs, its LDS does not grow with dp)
    return nb >= (1 << 18) || (c.flags & KNN_TUNE_SCAN16_ANY_NB);
}

// Everything one search_view call decides before it allocates and launches.
struct SearchPlan {
    ScanPlan pl;
    int sstride;         // > 0: a sample pass (every sstride-th block of the view) is searched first and seeds this launch
    int svshift;         // ... its block shift: 0 for a statistical sample (single rows), -1 = the view's own
    int seed_j, seed_stat, k_sample; // ... the rank of its bound, statistical (verified) or exact, the k it is searched with
    int pub_rounds, pub_m;           // tile-minimum seed: rounds of publications, keys per workgroup and query
    int kslot, qcap;     // most keys a chunk hands on per query; capacity of a query's compact candidate array
    double expect_n;     // typical candidates per query at the final selection (0: see select_expect_n)
    int pool_tiles;      // paired walk: tiles of every pair's range that go to the shared pool
    bool sparse_epi, cu_turn;
};

static SearchPlan plan_search(const PlanCtx &c, int64_t nb, int64_t nq, int k, int level, int row_mul, bool allow_stat, int pass_mode)
{
    ScanPlan pl;
    const bool allow_pairs = !c.approx16; // (the bf16 build has no one-query-tile streaming case worth pairing)
    // the statistical seed may serve this search (its caller checks the verification flag)
    const bool stat_ok = allow_stat && level == 0 && row_mul == 1 && stat_seed_allowed(c);
    // (the 256 x 256 tile needs the statistical seed -- see below -- so only callers that can check its verification flag get it)
    const bool allow_big = stat_ok || (c.flags & KNN_TUNE_BIG_TILE);
    PlanOpts seeded_plan;
    seeded_plan.seeded = true; seeded_plan.allow_pairs = allow_pairs; seeded_plan.allow_big = allow_big;
    make_plan(c, nb, nq, k, seeded_plan, pl);
    // Exact seeding pays when the sample that gives every chunk a tight threshold (about two chunks'
    // worth of rows, at least 64 k) is a small fraction of the view: the streaming regime (few
    // queries, huge database, hundreds of chunks).  KNN_TUNE_NO_SEED turns all seeding off, KNN_TUNE_EXACT_SEED
    // forces the exact seed, KNN_TUNE_STAT_SEED forces the statistical one, KNN_TUNE_NO_STAT_SEED forbids it (tests).
    bool seed = nb >= 512 * (int64_t)k && std::max<int64_t>(2 * pl.chunk_rows, 64 * (int64_t)k) <= nb / 32;
    if (c.flags & KNN_TUNE_EXACT_SEED) seed = nb >= 8192 && nb >= 32 * (int64_t)k;
    if (c.flags & (KNN_TUNE_NO_SEED | KNN_TUNE_STAT_SEED)) seed = false;
    // (the 256 x 256 tile under a caller that can check the verification flag: the statistical estimate from every 256th row
    // instead of an exact search of every 32nd -- 10 M rows x 512 / 768 / 1536 queries 0.854 / 0.869 / 0.858 of the MFMA peak with
    // the exact seed where 1024 / 2048 queries, which the rule above leaves to the estimate, reach 0.887; the exact seed stays
    // the fallback when no rank qualifies)
    const bool exact_ok = seed;
    if (seed && pl.qt == 256 && stat_ok) seed = false;
    int sstride = seed ? seed_stride(nb, k, pl.chunk_rows) : 0;
    int seed_j = k, seed_stat = 0, svshift = -1;
    double expect_n = 0; // typical candidates per query at the final selection (0: unknown, assume the capacity)
    if (!seed && stat_ok) {
        // statistical seed: single rows, every 32nd (every 16th of a small database, every 64th of a
        // large one): a few percent of the work, one round of workgroups at CATH size
        int st = nb >= (1 << 20) ? 64 : (nb >= 8192 ? 32 : 16);
        // The 256 x 256 tile (one workgroup per CU) ALWAYS wants the estimate, and from a sparser sample: nothing on the CU hides
        // an unseeded chunk's warm-up -- every score appended until the lists first fill, a stale bound for the ~25 tiles up to
        // the next cut (10 % of the scores pass: the sparse epilogue's lanes run out of slots and the tiles are filtered the
        // dense way), cuts of 256 lists on four waves -- Pfam-sized k = 100: 52.2 ms per 16384-query launch unseeded, 48.1
        // seeded; and the sample pass is what the seed costs: 1.93 ms per launch with every 32nd row, a quarter of that with
        // every 128th, for twice the candidates (0.8 % of the scores instead of 0.4 %: the epilogue does not notice).
        ScanPlan un;
        PlanOpts unseeded_plan;
        unseeded_plan.allow_big = allow_big;
        make_plan(c, nb, nq, k, unseeded_plan, un);
        const bool big = un.qt == 256;
        if (big) st *= k <= 256 ? 4 : 2;
#ifdef KNN355_DEV
        if (getenv("KNN355_STAT_STRIDE")) st = atoi(getenv("KNN355_STAT_STRIDE")); // (developer build: the statistical sample's stride)
#endif
        const bool force = (c.flags & KNN_TUNE_STAT_SEED) != 0;
        const int64_t S = view_rows(nb, st, 0);
        const int j = stat_seed_rank(S, nb, k);
        if (j > 0 && (force || (nq >= dev_knob("KNN355_STAT_MIN_NQ", 65) && nb >= 8192))) {
            // worth it only if it removes most of the candidates an unseeded pass would collect
            // (an unseeded chunk appends every score until its list first fills, cap - dt keys, whatever k is; then about
            // k more per e-fold of rows)
            const double warm = std::min<double>((double)un.cap - un.dt, (double)un.chunk_rows);
            const double unseeded = (double)un.nchunks * std::max(warm, k * (1.0 + log(std::max(1.0, (double)un.chunk_rows / k))));
            const double seeded = (double)j * (double)nb / (double)S;
            // ... and if those candidates are a sizeable share of all scores (Pfam-sized k = 100: 5 % of the scores go
            // through the lists, an unseeded scan loses ~5 % to them and the sample pass would cost 3 %: not worth it;
            // k = 1000: 17 %, CATH-sized k = 301: 50 %)
            if (force || big || (seeded <= 0.5 * unseeded && unseeded >= 0.08 * (double)nb)) {
                sstride = st;
                seed_j = j;
                seed_stat = 1;
                svshift = 0;
                expect_n = 1.3 * seeded + 1.25 * k; // (the bound's rank is in [j, 1.25 j]) + the sample's own rows
            }
        }
        if (!seed_stat && exact_ok) { // (no estimate after all: the exact seed the rule had chosen)
            seed = true;
            sstride = seed_stride(nb, k, pl.chunk_rows);
        }
    }
    // Tile-minimum seed (see flat_scan_kernel): where the exact seed would run a sample pass first, a launch with enough
    // chunks seeds itself -- each chunk publishes its first tiles' best key per query, the k-th smallest published key
    // is the bound.  Needs: the 32- or 64-query tile, plain fp32 rows, enough publications for k (<= 4096 of them).
    // KNN_TUNE_NO_TILE_MIN_SEED: never.  (The 128-query tile of a one-query-tile launch was tried: 100 k rows x 128 queries 0.66 -> 0.38 ms
    // where no sample pass exists, but the code in that build cost its other launches 2-14 % -- 1.25 M rows 2.80 -> 3.20 ms;
    // such batches are searched as two 64-query pieces instead, see search_keys_impl.)
    int pub_rounds = 0, pub_m = 1;
    const bool pub_shape = tile_min_seed_allowed(c) && !c.approx16 && pl.qt <= 64 && pl.cap >= 2 * pl.dt && pl.tiles_base >= (pl.npairs ? dev_knob("KNN355_PUB_MIN_TILES_PAIRED", 2) : 4);
    if (seed && pub_shape) {
        for (int r = 2; r >= 1; r--) // (one round if it gives enough publications)
            if ((int64_t)r * pl.nchunks <= 2048 && (int64_t)r * pl.nchunks >= 2 * (int64_t)k + 64 && r < pl.tiles_base) pub_rounds = r;
        if (c.pub_rounds_force > 0 && (int64_t)c.pub_rounds_force * pl.nchunks <= 2048 && c.pub_rounds_force < pl.tiles_base &&
            (int64_t)c.pub_rounds_force * pl.nchunks >= (int64_t)k + 32)
            pub_rounds = c.pub_rounds_force;
    }
    if (!pub_rounds && pub_shape && !c.pub_rounds_force && nb >= 16 * (int64_t)k && k <= KNN_WAVE_SELECT_MAX_K) {
        // A k beyond what one key per workgroup supports (512 workgroups, two rounds: k <= 480): every WAVE publishes the
        // best key of its own rows of the first tile -- 4 keys per workgroup and query with the 32-query tile, 2 with the
        // 64-query one, all of different rows, no reduction across the waves.  The k-th smallest of P such keys sits near the
        // -P ln(1 - k / P) / (P x rows per wave) quantile (k = 1000, P = 2048: 1372 of 131 k sampled rows; 2 M rows x 32
        // queries: 2.30 ms unseeded -- every workgroup warming up its own 1000 best -- against 1.45 at k = 100).
        const int wm = (pl.qt == 32 || pl.qt == 48) ? 4 : 2;
        for (int r = 2; r >= 1; r--) { // (one round if it gives enough publications; 4096 keys are selected by probing them in memory)
            const int64_t P = (int64_t)r * wm * pl.nchunks;
            if (P <= 4096 && P >= (int64_t)k + k / 4 + 32 && r < pl.tiles_base) {
                pub_rounds = r;
                pub_m = wm;
            }
        }
    }
    if (pass_mode == 2 && !pub_rounds) sstride = 0; // (a gated fallback runs no sample pass: its memsets could not be gated)
    // (nor does the 16-bit pass over 12-bit copies: they lie in tiles of 256 consecutive rows, which a strided view cannot
    // address -- without a tile-minimum seed that pass starts unseeded)
    if (pass_mode == 1 && c.s16_fmt == 12 && !pub_rounds) sstride = 0;
    if (pub_rounds) {
        sstride = 0;
        // the bound sits near the k / (publications x tile rows) quantile; the first tile(s) of every chunk are filtered
        // again at the end of the chunk
        expect_n = 2.0 * (double)k * (double)nb / ((double)pub_rounds * pl.nchunks * pl.dt) + 2.0 * k + 64;
        if (pub_m > 1) {
            const double P = (double)pub_rounds * pub_m * pl.nchunks;
            expect_n = 1.3 * (-P * log(1.0 - (double)k / P)) * (double)nb / ((double)pub_rounds * pl.nchunks * pl.dt) + 2.0 * k + 64;
        }
    }
    if (!sstride && !pub_rounds) { // a seed sample is small: parallelism over warm-up
        PlanOpts final_plan;
        final_plan.seeded = level > 0; final_plan.allow_pairs = allow_pairs && level == 0; final_plan.allow_big = allow_big;
        make_plan(c, nb, nq, k, final_plan, pl);
    }
    // Most keys a chunk hands on per query.  Chunks of a single tile (a seed sample, a tiny database)
    // hand on ALL their candidates: cutting 32 lists of one tile down to 1.25 k at the end of the only
    // tile is serial work per workgroup that the final selection does anyway, one workgroup per query.
    int kslot = knn_kslot(k);
    if (pl.chunk_rows == pl.dt && pl.dt > kslot && pl.dt <= pl.cap - pl.dt && k <= KNN_WAVE_SELECT_MAX_K) kslot = pl.dt;
    const int qcap = pl.nchunks * kslot + (sstride ? k + std::max(k >> 2, 32) : 0); // (a seed sample hands on up to kmax keys)
    SearchPlan sp;
    sp.pl = pl;
    sp.sstride = sstride; sp.svshift = svshift; sp.seed_j = seed_j; sp.seed_stat = seed_stat;
    // a statistical seed needs the sample's best ~1.25 j rows only (its bound has rank <= 1.25 j, and only rows that
    // beat the bound are handed on): the sample is searched with that k, not the caller's
    sp.k_sample = seed_stat ? std::min(k, seed_j + std::max(seed_j >> 2, 8) + 8) : k;
    sp.pub_rounds = pub_rounds; sp.pub_m = pub_m; sp.kslot = kslot; sp.qcap = qcap; sp.expect_n = expect_n;
    sp.sparse_epi = !(sstride && !seed_stat) && !pub_rounds; // (not exactly seeded: a statistical estimate, or no seed at all)
    // (turn taking: batch launches with real chunks, two workgroups per CU)
    sp.cu_turn = pl.nqtiles > 1 && !c.approx16 && pl.tiles_base >= 2 && pl.qt != 256 && !(c.flags & KNN_TUNE_NO_TURNS);
    // the pool: about a tenth of every pair's tiles (none with KNN_TUNE_NO_POOL)
    sp.pool_tiles = pl.npairs && !(c.flags & KNN_TUNE_NO_POOL) ? std::min(std::max(1, (pl.tiles_base + 5) / 10), pl.tiles_base / 4) : 0;
#ifdef KNN355_DEV
    if (sp.pool_tiles && getenv("KNN355_POOL_PCT")) // (developer build: the pool's share of every pair's range, in percent)
        sp.pool_tiles = std::min(std::max(1, pl.tiles_base * atoi(getenv("KNN355_POOL_PCT")) / 100), pl.tiles_base - 2);
#endif
    return sp;
}

// candidates per query the final selection should expect (sample_rows: rows of the plan's sample pass, 0 without one)
static int select_expect_n(const SearchPlan &sp, int64_t nb, int k, int64_t sample_rows)
{
    double expect_n = sp.expect_n;
    if (expect_n <= 0 && sp.sstride && !sp.seed_stat) {
        // exact seed: the sample's k-th score admits about k rows per sample-sized slice of the rest of the view
        const double S = (double)sample_rows;
        expect_n = 1.5 * (double)k * (double)nb / std::max(1.0, S) + 1.25 * k;
    }
    if (expect_n <= 0) expect_n = (double)sp.qcap;
    return (int)std::min<double>(std::min<double>((double)sp.qcap, expect_n), (double)nb); // (never more than the view has rows)
}

// a piece of a batch: queries [q0, q0 + m), one search_view call
struct Piece {
    int64_t q0, m;
};

// How search_keys_impl cuts a batch of nq queries (allow_stat: its caller can check the statistical seed's verification flag).
static std::vector<Piece> plan_pieces(const PlanCtx &c, int64_t nq, int k, bool allow_stat)
{
    // Many queries: blocks of 16384 (128 query tiles), one launch each.  A launch keeps two workgroups per CU in flight;
    // with 128 query tiles those share 4 chunks of rows and their 64 MB of query tiles stay in the Infinity Cache, with
    // 1563 query tiles (200 k queries at once) 512 different query tiles are streamed beside ONE chunk and the last of
    // 3.05 rounds of workgroups runs almost alone (200 k x 200 k x 1024: 0.79 -> 0.83 of the fp32 MFMA peak).  The
    // verification flag of a statistically seeded search is cleared by the first block only: it accumulates.
    const int64_t QB = 16384;
    const int64_t nblocks = nq > QB + QB / 2 ? (nq + QB - 1) / QB : 1;
    // The remainder behind the full 128-query tiles.  A query tile costs its whole width whatever it holds: on a database
    // that is streamed from HBM 129 queries took two passes of the 128-query build (10 M rows: 39.2 ms; 128 queries: 20.9).
    // The remainder is searched on its own with the narrowest build that holds it -- <= 32 queries: the streaming build
    // (7.1 ms per 10 M rows), <= 64: the 64-query build (11.6), a batch of 65..96: both (18.4-18.9 ms against 20.2-20.5 for
    // one 128-query pass).  Queries are independent, so the pieces return what one launch would.  Small databases keep one launch (the
    // pieces' own seeds and selections cost more than a padded tile saves).
    std::vector<Piece> pieces;
    const bool split = c.ntotal >= (1 << 18) && !c.force_qt && !(c.flags & KNN_TUNE_NO_REMAINDER_SPLIT);
    // A database of 32 k .. 262 k rows has no sample pass to seed a 128-query launch with, and the 64-query build seeds
    // itself: a batch of 65..128 queries goes as two 64-query pieces (100 k rows x 100 queries: 0.56 -> 0.41 ms) -- unless the
    // statistical seed can serve the one launch (synchronous callers) and k is large: from k ~ 200 on the one seeded
    // 128-query launch is ahead (100 k rows x 128 queries, k = 1000: 0.53 ms against 0.85 in pieces; k = 100: 0.49 against 0.44).
    const bool split_small = !split && c.ntotal >= (1 << 15) && nq > 64 && nq <= 128 && !c.force_qt && !c.force_chunks && !c.approx16 &&
                             tile_min_seed_allowed(c) && !(c.flags & KNN_TUNE_NO_REMAINDER_SPLIT) &&
                             (k <= 200 || !allow_stat || (c.flags & KNN_TUNE_NO_STAT_SEED));
    for (int64_t b = 0; b < nblocks; b++) {
        int64_t q0 = b * QB, m = nblocks == 1 ? nq : std::min(QB, nq - q0);
        if (split_small) {
            pieces.push_back({q0, 64});
            pieces.push_back({q0 + 64, m - 64});
            continue;
        }
        int64_t full = m / 128 * 128;
        const int64_t r = m - full;
        // A batch the 256 x 256 tile serves (big_tile_pays; synchronous callers: it needs the statistical seed) whose full tiles
        // end in half a 256-query tile: that half goes with the remainder, on the 128 x 128 tile -- 10 M rows x 640 queries:
        // 512 on the wide tile + 128 on the narrow one, not three wide query tiles of which one is half empty.
        const bool may_big = (allow_stat && stat_seed_allowed(c)) || (c.flags & KNN_TUNE_BIG_TILE);
        if (split && may_big && !c.force_chunks && full % 256 == 128 && full >= 384 && big_tile_pays(c, c.ntotal, full - 128)) {
            pieces.push_back({q0, full - 128});
            q0 += full - 128;
            m -= full - 128;
            full = 128;
        }
        // (round 4: 33..48 and 65..96 queries have builds of their own width -- 16-query blocks, make_plan -- so a remainder of
        // up to 96 queries is one piece: 10 M rows x 80 queries: 18.7 ms as 64 + 16, ~16 as one 96-query pass)
        const bool q96 = !c.approx16 && !(c.flags & KNN_TUNE_NO_Q16);
        if (!split || m <= 64 || r == 0 || r > 96 || (r > 64 && full && !q96) || (!full && q96)) { // (without the 96-query build: 65..96 behind full tiles cost two narrow passes what the padded tile does)
            pieces.push_back({q0, m});
            continue;
        }
        if (full) pieces.push_back({q0, full});
        if (r > 64 && !q96) {
            pieces.push_back({q0 + full, 64});
            pieces.push_back({q0 + full + 64, r - 64});
        } else {
            pieces.push_back({q0 + full, r});
        }
    }
    return pieces;
}

// ---- symmetric self-search ---------------------------------------------------
// Symmetric all-vs-all (the queries ARE the database rows): workgroup w multiplies query tile qtile with the
// database tiles [jt0, jt0 + jcount), all of them on or above the diagonal; see flat_scan_kernel<..., SYM>.
struct SymItem {
    int qtile, jt0, jcount;
};

static const int SYM_MAX_GROUPS = 8;

// Everything self_search_symmetric decides before it allocates and launches.
struct SymPlan {
    ScanPlan pl;      // tile shape and list capacity (pl.lds and pl.name are the plain build's: see lds, name)
    int ts, tiles;    // square tiles of ts rows (128: two workgroups per CU; 256: one, flat_scan_kernel<2, 2, 4, 4>), tiles of them
    int st;           // the statistical sample: every st-th row ...
    int64_t S;        // ... S rows ...
    int j;            // ... whose j-th best score is the bound (stat_seed_rank) ...
    int k_sample;     // ... searched with this k (the sample's best ~1.25 j rows, as plan_search does)
    int qcap;         // capacity of a row's compact candidate array
    int n_expect;     // candidates per row the final selections should expect
    int64_t slots;    // workgroups resident on the device
    int64_t max_wgs;  // workgroups per launch: their candidate lists stay below 2 GB
    int groups;       // launches of consecutive query tiles, each followed by its rows' selection; > 1: the result streams out
    bool cu_turn;
    size_t lds;
    const char *name; // the introspection's name of the kernel
};

// The statistical sample of a symmetric self-search: every 64th row from 131 072 rows on (Pfam-sized k = 100 / 1000 340.0 / 356.8 ms
// against 348.7 / 366.2 with every 32nd -- the sample pass is 6 % of that search --, 100 k rows 89.2 against 90.8, 60 k rows and
// fewer: within 1 % either way; CATH-sized: 3.06 against 2.87 ms; until late in round 5 the step to 64 came at 2^20 rows).
static int sym_stat_stride(int64_t n)
{
    int st = n >= (1 << 17) ? 64 : 32;
#ifdef KNN355_DEV
    if (getenv("KNN355_STAT_STRIDE")) st = atoi(getenv("KNN355_STAT_STRIDE"));
#endif
    return st;
}

// Will the symmetric launch take this self-search?  (knn_flat_search_self asks BEFORE it sets aside device memory for the whole
// n x k result.)  Fills the sample's half of the plan, in ONE place: the rank j, the sample it is taken from and what the
// selections expect must belong together (a rank worked out for a sparser sample is too tight a bound on a denser one: every
// verification fails and the plain path repeats the search).
static bool self_search_symmetric_eligible(const PlanCtx &c, int k, SymPlan *out = nullptr)
{
    const int64_t n = c.ntotal;
    if (n < dev_knob("KNN355_SYM_MIN_N", 3000) || k > KNN_REGISTER_SELECT_MAX_K || k >= n || !stat_seed_allowed(c) || (c.flags & KNN_TUNE_NO_SYM) || c.force_qt || c.force_chunks || c.approx16) return false;
    const int st = sym_stat_stride(n);
    const int64_t S = view_rows(n, st, 0);
    const int j = stat_seed_rank(S, n, k);
    if (j <= 0) return false;
    const double expect = 1.3 * (double)j * (double)n / (double)S + 1.25 * k;
    const int qcap = (int)std::min<double>(((int64_t)(2.0 * expect) + 1024 + 63) / 64 * 64, 1 << 20);
    if ((double)n * qcap * 8.0 > 24.0 * (1u << 30)) return false;
    if (out) {
        out->st = st; out->S = S; out->j = j; out->qcap = qcap;
        out->n_expect = (int)std::min<double>((double)qcap, expect);
    }
    return true;
}

// Dynamic LDS of a symmetric workgroup: the plain layout with at least 72 KB of lds_main on the 128-row tile (8 KB of slots
// for its sparse epilogue, see lds_main in the kernel) + thresholds, per-half counts and bases of the database tile's rows
// (s_thr2, s_cnt2, s_base2).
static size_t scan_lds_bytes_sym(int qt, int dt, int cap) { return scan_lds_bytes(qt, dt, cap, qt == 128 ? 73728 : 0) + (size_t)(2 + 2) * dt * 4; }

// The plan of a self-search of every row against every row; false where the plain path must serve it.  can_stream: the caller
// gave host arrays and holds the copy stream.
static bool plan_self_symmetric(const PlanCtx &c, int k, bool can_stream, SymPlan &sp)
{
    if (!self_search_symmetric_eligible(c, k, &sp)) return false;
    const int64_t n = c.ntotal;
    ScanPlan &pl = sp.pl;
    // (tile shape, list capacity.  256-row tiles only on demand, KNN_TUNE_BIG_TILE: the symmetric launch filters every tile
    // twice and executes half the flops per row pair, its epilogue weighs twice as much beside the K loop -- Pfam-sized
    // k = 100 / 1000: 372.7 / 392.6 ms on 256-row tiles against 349.7 / 377.4 on 128-row tiles, one box)
    PlanOpts po;
    po.seeded = true; po.allow_big = (c.flags & KNN_TUNE_BIG_TILE) != 0;
    make_plan(c, n, n, k, po, pl);
    if (pl.qt != pl.dt || (pl.qt != 128 && pl.qt != 256)) return false;
    sp.ts = pl.qt;
    sp.tiles = (int)((n + sp.ts - 1) / sp.ts);
    sp.k_sample = std::min(k, sp.j + std::max(sp.j >> 2, 8) + 8);
    sp.slots = (sp.ts == 256 ? 1 : 2) * (int64_t)std::max(1, c.num_cus);
    sp.max_wgs = std::max<int64_t>(sp.slots, (int64_t)((2ull << 30) / ((size_t)pl.qt * pl.cap * 8)));
    // (eight groups for gigabytes of result; four from 32 MB on -- CATH-sized, 113 query tiles, 52 MB: cath.search end to end
    // 5.03 -> 4.43 ms with four, 4.62 with five, 4.94 with eight: every group is a launch with its own tail and selection)
    const size_t result_bytes = (size_t)n * k * 12;
    const int want_groups = std::min(SYM_MAX_GROUPS, std::max(2, dev_knob("KNN355_SELF_GROUPS", result_bytes >= ((size_t)256 << 20) && sp.tiles >= 16 * SYM_MAX_GROUPS ? SYM_MAX_GROUPS : 4)));
    const bool stream_out = can_stream && result_bytes >= ((size_t)dev_knob("KNN355_SELF_STREAM_MIN_MB", 32) << 20) && sp.tiles >= 16 * want_groups;
    sp.groups = stream_out ? want_groups : 1;
    sp.cu_turn = !(c.flags & KNN_TUNE_NO_TURNS) && sp.ts == 128;
    sp.lds = scan_lds_bytes_sym(pl.qt, pl.dt, pl.cap) + (size_t)dev_knob("KNN355_LDS_PAD", 0); // (developer build: more LDS than a second workgroup leaves room for = one workgroup per CU)
    sp.name = sp.ts == 256 ? "flat_scan_q256_d256_sym" : "flat_scan_q128_d128_sym";
    return true;
}

// first row of group g's query tiles: group g serves rows [sym_group_row0(g), sym_group_row0(g + 1)) -- equal shares of the RESULT
static int64_t sym_group_row0(const SymPlan &sp, int64_t n, int g) { return std::min<int64_t>(n, (int64_t)sp.tiles * g / sp.groups * sp.ts); }

// The work table of a symmetric launch: workgroup = (query tile I, a run of database tiles J >= I), group after group
// (gstart[g] .. gstart[g + 1]: the items of group g, the launch that serves query tiles [tiles g / groups, tiles (g + 1) /
// groups); the first group is the longest).  It depends on (tiles, groups, slots) only.
struct SymTable {
    std::vector<SymItem> items;
    std::vector<int64_t> gstart;
    int first_run; // the first group's run length (introspection)
};

static SymTable sym_work_table(int tiles, int groups, int64_t slots)
{
    SymTable t;
    t.gstart.assign(1, 0);
    t.first_run = 16;
    for (int g = 0; g < groups; g++) {
        const int I0 = (int)((int64_t)tiles * g / groups), I1 = (int)((int64_t)tiles * (g + 1) / groups);
        // the run length that minimises rounds x (tiles + half a tile of fixed work), of each group by itself: a group is a
        // launch, and a short one -- the later groups of a CATH-sized index -- fills the slots only with short runs
        int best_tp = 16;
        int64_t best_cost = INT64_MAX;
        for (int tp = dev_knob("KNN355_SYM_MIN_TP", 1); tp <= 96; tp++) {
            int64_t wgs = 0;
            for (int I = I0; I < I1; I++) wgs += (tiles - I + tp - 1) / tp;
            const int64_t rounds = (wgs + slots - 1) / slots;
            const int64_t cost = rounds * (2 * tp + 1);
            if (cost < best_cost || (cost == best_cost && tp > best_tp)) { best_cost = cost; best_tp = tp; }
        }
        if (g == 0) t.first_run = best_tp;
        const size_t at = t.items.size();
        for (int I = I0; I < I1; I++)
            for (int j0 = I; j0 < tiles; j0 += best_tp) t.items.push_back({I, j0, std::min(best_tp, tiles - j0)});
        // long runs first: the short tails of every query tile fill the last round
        std::stable_sort(t.items.begin() + at, t.items.end(), [](const SymItem &a, const SymItem &b) { return a.jcount > b.jcount; });
        t.gstart.push_back((int64_t)t.items.size());
    }
    return t;
}

// ---- range scan ---------------------------------------------------------------
struct RangePlan {
    int qt, dt, nqtiles, nchunks, tiles_base, tiles_rem, grid;
    bool diff;
    size_t lds;
    const char *name;
};

// One block of nq queries of a range search.  The tile: 32 queries x 256 rows for small batches (a 10 M-row scan of 32 queries
// is HBM-bound; a 128-wide tile would do 4x its matrix work), 128 x 128 for large ones; the difference build is the 32-query tile.
static RangePlan plan_range(const PlanCtx &c, int64_t nq)
{
    RangePlan pl;
    // FAISS's small-batch rule, as make_plan applies it: the caller's whole batch decides the formula, for every block
    pl.diff = c.metric == KNN_METRIC_L2 && c.batch_nq < 20;
    const bool wide = !pl.diff && nq > 64;
    pl.qt = wide ? 128 : 32;
    pl.dt = wide ? 128 : 256;
    pl.nqtiles = (int)((nq + pl.qt - 1) / pl.qt);
    const int64_t tiles = (c.ntotal + pl.dt - 1) / pl.dt;
    // about two workgroups per CU, contiguous rows per chunk
    pl.nchunks = (int)std::max<int64_t>(1, std::min<int64_t>(tiles, (2 * (int64_t)c.num_cus + pl.nqtiles - 1) / pl.nqtiles));
    pl.tiles_base = (int)(tiles / pl.nchunks);
    pl.tiles_rem = (int)(tiles % pl.nchunks);
    pl.grid = pl.nqtiles * pl.nchunks;
    const size_t stage = (size_t)(pl.dt + pl.qt) * 128 * 2, park = (size_t)pl.qt * (pl.dt + 1) * 4;
    pl.lds = std::max(stage, park) + (size_t)pl.dt * 4 + (size_t)pl.qt * 4;
    pl.name = pl.diff ? "range_scan_q32_d256_diff" : (wide ? "range_scan_q128_d128" : "range_scan_q32_d256");
    return pl;
}

static const size_t KNN_RANGE_STAGE_BYTES = (size_t)192 << 20; // staging segments of one block (12 bytes per entry)

// entries of a staging segment: the block's share of the budget per (query, chunk), never more than a chunk's rows
static int64_t range_segcap(const RangePlan &pl, int64_t nq)
{
    const int64_t chunk_rows = (int64_t)(pl.tiles_base + (pl.tiles_rem ? 1 : 0)) * pl.dt;
    return std::max<int64_t>(1, std::min<int64_t>(chunk_rows, (int64_t)(KNN_RANGE_STAGE_BYTES / 12) / (nq * pl.nchunks)));
}

// ---- device-wide rank (rank.inc) ---------------------------------------------------
static const int RANK_TILE = 2048;       // elements per workgroup of a counting or scatter pass: 256 threads x 8
static const int RANK_SCAN_BLOCK = 1024; // entries per workgroup of the two-level scans: 256 threads x 4
static const int RANK_SCAN_TOP = 256;    // block sums per step of the one workgroup that scans them
static const int RANK_HIST_GRID = 1024;  // workgroups, at most, of the histogram of every pass

struct RankPlan {
    int64_t n;             // rows * limit elements
    int64_t ntiles;        // tiles of RANK_TILE elements: the grid of a pass
    int64_t table_entries; // 256 * ntiles digit counts
    int64_t table_blocks;  // scan blocks over the table
    int64_t cum_blocks;    // scan blocks over the n flags (0 without the running count)
    int passes;            // 8-bit digits of a key: the passes at most
    int key_bytes;
    // the upload: with limit <= k / 2 the host packs the first `limit` columns of every row and the device copy is
    // [rows][limit]; otherwise the arrays go up as they are, [rows][k], and the kernels skip the columns past the limit
    bool pack;
    int64_t dev_k; // row stride, in cells, of the device copy
    // every device buffer of a call but the look-ups' own vectors (targets, ranks and their outputs): rank_run allocates
    // exactly these
    size_t scores_bytes, correct_bytes; // the device copies of the two arrays (correct: 0 without one)
    size_t keys_bytes, pay_bytes;       // ONE key / payload buffer; the sort ping-pongs between two of each
    size_t table_bytes, partial_bytes;  // the digit counts; the block sums of whichever scan has more blocks
    size_t hist_bytes;                  // the digit histograms of every pass
    size_t cum_bytes;                   // C(r) as 32-bit counts (0 without the running count)
    size_t wide_bytes;                  // one int64 [n] staging buffer for order_out / cum_out (0 when neither is wanted)
    size_t resident_bytes;              // the sum: scores + correct + 2 keys + 2 payloads + the rest
};

// false: not a legal problem (rows, k or limit below 1, limit above k, k above INT32_MAX, a key width other than 4 or 8 bytes,
// rows * limit above 2^31 - 1 -- the payload keeps the position in 31 bits beside the flag -- or rows * k cells beyond size_t)
static bool plan_rank(int64_t rows, int64_t k, int64_t limit, int key_bytes, bool has_correct, bool want_cum, bool want_wide, RankPlan *out)
{
    if (rows < 1 || k < 1 || limit < 1 || limit > k || k > (int64_t)INT32_MAX || (key_bytes != 4 && key_bytes != 8)) return false;
    if (rows > (int64_t)INT32_MAX / limit) return false;
    if (rows > (int64_t)(INT64_MAX / 16) / k) return false;
    RankPlan pl;
    pl.n = rows * limit;
    pl.ntiles = (pl.n + RANK_TILE - 1) / RANK_TILE;
    pl.table_entries = 256 * pl.ntiles;
    pl.table_blocks = (pl.table_entries + RANK_SCAN_BLOCK - 1) / RANK_SCAN_BLOCK;
    pl.cum_blocks = want_cum ? (pl.n + RANK_SCAN_BLOCK - 1) / RANK_SCAN_BLOCK : 0;
    pl.passes = key_bytes;
    pl.key_bytes = key_bytes;
    pl.pack = 2 * limit <= k;
    pl.dev_k = pl.pack ? limit : k;
    const size_t n = (size_t)pl.n, cells = (size_t)rows * (size_t)pl.dev_k;
    pl.scores_bytes = cells * (size_t)key_bytes;
    pl.correct_bytes = has_correct ? cells : 0;
    pl.keys_bytes = n * (size_t)key_bytes;
    pl.pay_bytes = n * 4;
    pl.table_bytes = (size_t)pl.table_entries * 4;
    pl.partial_bytes = (size_t)std::max(pl.table_blocks, pl.cum_blocks) * 4;
    pl.hist_bytes = (size_t)pl.passes * 256 * 4;
    pl.cum_bytes = want_cum ? n * 4 : 0;
    pl.wide_bytes = want_wide ? n * 8 : 0;
    pl.resident_bytes = pl.scores_bytes + pl.correct_bytes + 2 * pl.keys_bytes + 2 * pl.pay_bytes + pl.table_bytes + pl.partial_bytes + pl.hist_bytes +
                        pl.cum_bytes + pl.wide_bytes;
    *out = pl;
    return true;
}

// ---- windowed statistics over the ranked order (windows.inc) -----------------------
static const int WINDOW_RUN = 2048;   // ranked keys of one staging run: 16 KiB of float64 per direction, 33 KiB per workgroup with the padding
static const int WINDOW_CHAINS = 256; // chains of a workgroup at most, one per thread: 128 blocks x 2 directions
static const int WINDOW_PAD_SHIFT = 5; // LDS index of staged element e: e + (e >> 5) -- one float64 of padding per 32

#if defined(__HIPCC__)
#define PLAN_HD __host__ __device__
#else
#define PLAN_HD
#endif

// The ranks [lo, hi) of a group [g0, g0 + len) that are staged at step `step` for one direction: forward chains take the
// group's runs from its first rank up, backward chains from its last rank down.  Steps past the group's end are empty
// (lo == hi).  window_chain_kernel and windows_check.cpp both call this: the kernel has no layout of its own.
struct WindowPiece {
    int64_t lo, hi;
};
PLAN_HD static inline WindowPiece window_piece(int64_t g0, int64_t len, int64_t run, int64_t step, int backward)
{
    WindowPiece p;
    const int64_t a = step * run < len ? step * run : len, b = (step + 1) * run < len ? (step + 1) * run : len;
    if (backward) {
        p.lo = g0 + len - b;
        p.hi = g0 + len - a;
    } else {
        p.lo = g0 + a;
        p.hi = g0 + b;
    }
    return p;
}

struct WindowsPlan {
    RankPlan rank;          // the order: plan_rank(n, 1, 1, key_bytes, no flags, no running count, want_order)
    int64_t n, window, nout; // window 0: no rolling means (nout 0); else nout = n - window + 1
    int64_t nbins;          // ranges or edges (0: none)
    int m, key_bytes;
    // the chains: blocks of `window` consecutive ranks, two chains (forward P, backward S) per block
    int64_t nblocks;        // ceil(n / window)
    int64_t run;            // WINDOW_RUN
    int64_t blocks_per_run; // window <= run: min(run / window, WINDOW_CHAINS / 2) whole blocks share one staged run; else 1
    int64_t runs_per_block; // window > run: ceil(window / run) runs make one block, the chain's sum carried across; else 1
    int64_t group;          // ranks of one workgroup: blocks_per_run * window
    int64_t chain_grid;     // ceil(n / group) workgroups of 256 threads
    size_t chain_lds;       // 2 directions x (run + run / 32) float64
    int64_t scan_blocks;    // blocks of RANK_SCAN_BLOCK ranks of one column's scan
    int64_t gather_grid, means_grid, combine_grid, ranges_grid; // workgroups of 256 (means: x; y is m)
    // every device buffer of a call beyond the rank's: knn_eval_windows allocates exactly these (0: not allocated)
    size_t values_bytes;  // the columns, uint8 [m][n]
    size_t mask_bytes;    // one uint32 per rank: bit c = column c at the rank's position
    size_t cum_bytes;     // C_c(r), uint32 [m][n]
    size_t wpartial_bytes; // the block sums of one column's scan
    size_t keyd_bytes;    // the keys in rank order as float64, padded to a whole 16-byte load
    size_t chain_bytes;   // ONE of the two chain buffers P and S, float64 [n]
    size_t means_bytes;   // float64 [m + 1][nout]: the columns' means, then the key's
    size_t bins_bytes;    // start, stop int64 [nbins]; counts int64 [m][nbins]; key_lo, key_hi and the edges in the keys' type [nbins]
    size_t resident_bytes; // rank.resident_bytes + values + mask + cum + wpartial + keyd + 2 chains + means + bins
};

// false: not a legal problem (n outside [1, 2^31 - 1], a key width other than 4 or 8 bytes, m outside [0, KNN_WINDOWS_MAX_COLS],
// window outside [0, n], nbins outside [0, KNN_WINDOWS_MAX_BINS], or neither a window nor bins)
static bool plan_windows(int64_t n, int key_bytes, int64_t m, int64_t window, bool want_order, int64_t nbins, WindowsPlan *out)
{
    if (m < 0 || m > KNN_WINDOWS_MAX_COLS || window < 0 || window > n || nbins < 0 || nbins > KNN_WINDOWS_MAX_BINS) return false;
    if (window == 0 && nbins == 0) return false;
    WindowsPlan pl;
    if (!plan_rank(n, 1, 1, key_bytes, false, false, want_order, &pl.rank)) return false;
    pl.n = n;
    pl.window = window;
    pl.nout = window ? n - window + 1 : 0;
    pl.nbins = nbins;
    pl.m = (int)m;
    pl.key_bytes = key_bytes;
    pl.run = WINDOW_RUN;
    pl.nblocks = window ? (n + window - 1) / window : 0;
    pl.blocks_per_run = window && window <= pl.run ? std::min<int64_t>(pl.run / window, WINDOW_CHAINS / 2) : (window ? 1 : 0);
    pl.runs_per_block = window > pl.run ? (window + pl.run - 1) / pl.run : (window ? 1 : 0);
    pl.group = pl.blocks_per_run * window;
    pl.chain_grid = window ? (n + pl.group - 1) / pl.group : 0;
    pl.chain_lds = 2 * (size_t)(pl.run + (pl.run >> WINDOW_PAD_SHIFT)) * 8;
    pl.scan_blocks = m ? (n + RANK_SCAN_BLOCK - 1) / RANK_SCAN_BLOCK : 0;
    pl.gather_grid = std::min<int64_t>(65536, (n + 255) / 256);
    pl.means_grid = m ? (pl.nout + 255) / 256 : 0;
    pl.combine_grid = (pl.nout + 255) / 256;
    pl.ranges_grid = (nbins + 255) / 256;
    const size_t un = (size_t)n;
    pl.values_bytes = (size_t)m * un;
    pl.mask_bytes = m ? un * 4 : 0;
    pl.cum_bytes = (size_t)m * un * 4;
    pl.wpartial_bytes = (size_t)pl.scan_blocks * 4;
    pl.keyd_bytes = window ? ((un + 1) & ~(size_t)1) * 8 : 0;
    pl.chain_bytes = window ? un * 8 : 0;
    pl.means_bytes = (size_t)(m + 1) * (size_t)pl.nout * 8;
    pl.bins_bytes = (size_t)nbins * (16 + (size_t)m * 8 + 3 * (size_t)key_bytes);
    pl.resident_bytes = pl.rank.resident_bytes + pl.values_bytes + pl.mask_bytes + pl.cum_bytes + pl.wpartial_bytes + pl.keyd_bytes + 2 * pl.chain_bytes +
                        pl.means_bytes + pl.bins_bytes;
    *out = pl;
    return true;
}

// ---- tie-averaged ranks and correlation moments (correlate.inc) --------------------
// The order of every sum of the moments, a function of N alone.  The N terms are cut into tiles of CORR_TILE consecutive
// terms; lane j of a tile's CORR_LANES lanes adds, to a +0.0 it starts from, the terms corr_term(tile, j, 0), (tile, j, 1),
// ... in that order (the ones below N); the lanes' sums are folded by the tree lane[j] = lane[j] + lane[j + off] for j <
// off, off = CORR_LANES / 2, ..., 2, 1; lane 0 holds the tile's sum.  The tiles' sums, in tile order, are the terms of the
// next level, summed the same way, until one is left: level_n[0] = N, level_n[i + 1] = ceil(level_n[i] / CORR_TILE).
// moment_kernel and correlate_check.cpp both call corr_term: the kernel has no layout of its own.
static const int CORR_TILE = 2048;    // terms of one workgroup
static const int CORR_LANES = 256;    // its threads: CORR_TILE / CORR_LANES terms each
static const int CORR_MAX_LEVELS = 3; // 2^31 - 1 -> 2^20 -> 512 -> 1
static const int CORR_GRID = 65536;   // workgroups, at most, of the grid-stride tie kernels

PLAN_HD static inline uint64_t corr_term(uint64_t tile, int lane, int i) { return tile * CORR_TILE + (uint64_t)i * CORR_LANES + lane; }

struct CorrelatePlan {
    RankPlan rank_x, rank_y; // the two orders: plan_rank(rows, k, limit, the array's bytes, no flags, running count, no wide)
    int64_t n;               // rows * limit pairs
    int what;                // KNN_CORR_PEARSON | KNN_CORR_SPEARMAN; 0: the doubled ranks of x alone (knn_eval_rankdata)
    bool sorts;              // any order at all: what != KNN_CORR_PEARSON
    int levels;              // launches of one reduction: 1 .. CORR_MAX_LEVELS
    int64_t level_n[CORR_MAX_LEVELS + 1]; // terms of every level; level_n[levels] = 1
    int64_t tie_grid;        // workgroups of 256 of tie_heads / tie_starts / tie_scatter
    // every device buffer of a call: the entries allocate exactly these (0: not allocated)
    size_t x_bytes, y_bytes;            // the device copies (rank_x.scores_bytes, rank_y.scores_bytes)
    size_t keys_bytes, pay_bytes;       // ONE key / payload buffer, the wider array's; both sorts ping-pong between the same two of each
    size_t table_bytes, partial_bytes;  // the digit counts; the block sums of the scan of the N head flags
    size_t hist_bytes;                  // the digit histograms, the wider array's
    size_t run_bytes;                   // uint32 [N]: the head flags, then (scanned in place) the 1-based run number of every rank
    size_t start_bytes;                 // uint32 [N + 1]: the first rank of every run, and N behind the last
    size_t rank2_bytes;                 // ONE doubled-rank buffer: int64 [N] for rankdata, uint32 [N] for Spearman (which has two)
    int rank2_buffers;                  // 1, 2, or 0
    size_t nan_bytes;                   // int64 [2]: NaN cells of x and of y
    size_t moment_a_bytes, moment_b_bytes; // the partial sums of levels 1 and 2, three quantities each: float64, or 128-bit integers for Spearman
    size_t resident_bytes;              // the sum
};

// false: not a legal problem (what plan_rank refuses, a width other than 4 or 8 bytes, N below 2, `what` outside the bit
// set; y_bytes is 0 exactly when what is 0)
static bool plan_correlate(int64_t rows, int64_t k, int64_t limit, int x_bytes, int y_bytes, int what, CorrelatePlan *out)
{
    if (what < 0 || what > (KNN_CORR_PEARSON | KNN_CORR_SPEARMAN)) return false;
    if ((what == 0) != (y_bytes == 0)) return false;
    CorrelatePlan pl;
    if (!plan_rank(rows, k, limit, x_bytes, false, true, false, &pl.rank_x)) return false;
    if (y_bytes && !plan_rank(rows, k, limit, y_bytes, false, true, false, &pl.rank_y)) return false;
    if (!y_bytes) pl.rank_y = pl.rank_x;
    if (pl.rank_x.n < 2) return false;
    pl.n = pl.rank_x.n;
    pl.what = what;
    pl.sorts = what != KNN_CORR_PEARSON;
    pl.levels = 0;
    pl.level_n[0] = pl.n;
    for (int i = 1; i <= CORR_MAX_LEVELS; i++) pl.level_n[i] = 1;
    while (pl.level_n[pl.levels] > 1) {
        if (pl.levels == CORR_MAX_LEVELS) return false; // (never: N <= 2^31 - 1)
        pl.level_n[pl.levels + 1] = (pl.level_n[pl.levels] + CORR_TILE - 1) / CORR_TILE;
        pl.levels++;
    }
    pl.tie_grid = std::min<int64_t>(CORR_GRID, (pl.n + 255) / 256);
    const RankPlan &wide = pl.rank_y.key_bytes > pl.rank_x.key_bytes ? pl.rank_y : pl.rank_x;
    const size_t n = (size_t)pl.n;
    pl.x_bytes = pl.rank_x.scores_bytes;
    pl.y_bytes = y_bytes ? pl.rank_y.scores_bytes : 0;
    pl.keys_bytes = pl.sorts ? wide.keys_bytes : 0;
    pl.pay_bytes = pl.sorts ? wide.pay_bytes : 0;
    pl.table_bytes = pl.sorts ? wide.table_bytes : 0;
    pl.partial_bytes = pl.sorts ? wide.partial_bytes : 0;
    pl.hist_bytes = pl.sorts ? wide.hist_bytes : 0;
    pl.run_bytes = pl.sorts ? n * 4 : 0;
    pl.start_bytes = pl.sorts ? (n + 1) * 4 : 0;
    pl.rank2_bytes = pl.sorts ? n * (what ? 4 : 8) : 0;
    pl.rank2_buffers = pl.sorts ? (what ? 2 : 1) : 0;
    pl.nan_bytes = pl.sorts ? 16 : 0;
    const size_t entry = 3 * (size_t)((what & KNN_CORR_SPEARMAN) ? 16 : 8);
    pl.moment_a_bytes = what ? (size_t)pl.level_n[1] * entry : 0;
    pl.moment_b_bytes = what ? (size_t)pl.level_n[2] * entry : 0;
    pl.resident_bytes = pl.x_bytes + pl.y_bytes + 2 * pl.keys_bytes + 2 * pl.pay_bytes + pl.table_bytes + pl.partial_bytes + pl.hist_bytes + pl.run_bytes +
                        pl.start_bytes + (size_t)pl.rank2_buffers * pl.rank2_bytes + pl.nan_bytes + pl.moment_a_bytes + pl.moment_b_bytes;
    *out = pl;
    return true;
}

// ---- mean pooling over row ranges (pool.inc) ---------------------------------------
static const int POOL_COLS = 256;      // columns of one wave: 64 lanes x 4
static const int POOL_GROUP = 8;       // rows whose loads are issued in front of the first add of the group
static const int POOL_NORM_ROWS = 64;  // rows per batch of norms of the normalizing build
static const int POOL_MAX_WAVES = 16;  // waves of a workgroup, at most (normalizing build; the plain one takes 4)
static const int64_t POOL_MAX_LEN = (int64_t)1 << 24; // a range is shorter than this: (float)L is exact

struct PoolPlan {
    int ncb;        // column blocks of POOL_COLS columns: ceil(d / 256)
    int waves;      // waves of a workgroup = neighbouring column blocks of one range
    int64_t grid_x; // ranges
    int grid_y;     // workgroups per range: ceil(ncb / waves)
    bool aligned;   // a lane reads its four columns as one 16-byte (fp16: 8-byte) load; false: element by element
};

// false: not a legal launch (n outside [1, 2^31 - 1], d outside [2, KNN_POOL_MAX_D], a row stride below d, an element size
// other than 2 or 4 bytes).  The plain build puts up to 4 neighbouring column blocks of a range into one workgroup.  The
// normalizing build shares a batch's 64 norms between the waves of a workgroup, so it takes every column block of the range
// it can: the smallest power of two (it divides 64) that covers ncb, 16 at most; waves past the last column block compute
// norms and add nothing.  Aligned: the base is a multiple of four elements and so is the row stride.
static bool plan_pool(int64_t n, int64_t d, int64_t row_stride, uintptr_t base, int elem_bytes, bool normalize, PoolPlan *out)
{
    if (n < 1 || n > (int64_t)INT32_MAX || d < 2 || d > KNN_POOL_MAX_D || row_stride < d || (elem_bytes != 2 && elem_bytes != 4)) return false;
    PoolPlan pl;
    pl.ncb = (int)((d + POOL_COLS - 1) / POOL_COLS);
    if (normalize) {
        pl.waves = 1;
        while (pl.waves < pl.ncb && pl.waves < POOL_MAX_WAVES) pl.waves *= 2;
    } else {
        pl.waves = std::min(pl.ncb, 4);
    }
    pl.grid_x = n;
    pl.grid_y = (pl.ncb + pl.waves - 1) / pl.waves;
    pl.aligned = base % (uintptr_t)(4 * elem_bytes) == 0 && row_stride % 4 == 0;
    *out = pl;
    return true;
}

// The host entry's cut of the residue matrix into uploads.  order: the ranges by ascending (start, stop, index); a chunk is
// a run of `order` (first, count) and the rows [row0, row1) that hold every range of the run.  A chunk spans at most
// chunk_rows rows, but for a single range longer than that, which is a chunk of its own.  Ranges are valid (0 <= start <
// stop) and chunk_rows >= 1.  Overlapping ranges that fall into different chunks have their shared rows uploaded twice.
struct PoolChunk {
    int64_t row0, row1, first, count;
};
static void pool_assign_chunks(const int64_t *starts, const int64_t *stops, int64_t n, int64_t chunk_rows, std::vector<int64_t> &order,
                               std::vector<PoolChunk> &chunks)
{
    order.resize((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = i;
    std::sort(order.begin(), order.end(), [&](int64_t a, int64_t b) {
        if (starts[a] != starts[b]) return starts[a] < starts[b];
        if (stops[a] != stops[b]) return stops[a] < stops[b];
        return a < b;
    });
    chunks.clear();
    for (int64_t i = 0; i < n; i++) {
        const int64_t o = order[(size_t)i];
        if (!chunks.empty() && stops[o] - chunks.back().row0 <= chunk_rows) {
            chunks.back().row1 = std::max(chunks.back().row1, stops[o]);
            chunks.back().count++;
        } else {
            chunks.push_back({starts[o], stops[o], i, 1});
        }
    }
}

// ---- weighted layer mixes (mix.inc) --------------------------------------------------
static const int MIX_BLOCK = 256;     // threads of a workgroup of mix_rows_kernel and mix_top1_kernel
static const int MIX_MAX_GRID = 2048; // workgroups of mix_rows_kernel, at most (256 CUs x 8): the rest is a grid-stride loop

struct MixPlan {
    bool vec;             // an item is four columns moved by 16-byte loads and one 16-byte store; false: one column
    int per_row;          // items of one output row: dp / 4, or dp
    int64_t items;        // n * per_row (the padding columns d .. dp - 1 are items too: they are written as zeros)
    int grid;             // workgroups of MIX_BLOCK threads: ceil(items / MIX_BLOCK), MIX_MAX_GRID at most
};

// false: not a legal launch (n outside [1, 0xFFFFFFF0], d < 1, dp < d or dp >= 2^30, nlayers outside [1, KNN_MIX_MAX_LAYERS], a
// null base, a row stride below d).  The 16-byte build needs every layer's base and the output's to be multiples of 16 bytes
// and every row stride, the output's (dp) included, to be a multiple of four floats; anything else is moved float by float.
// A quad that straddles d (d no multiple of four) is handled float by float inside the 16-byte build.
static bool plan_mix(int64_t n, int64_t d, int64_t dp, int nlayers, const uintptr_t *bases, const int64_t *strides, uintptr_t out_base, MixPlan *out)
{
    if (n < 1 || n > 0xFFFFFFF0ll || d < 1 || dp < d || dp >= ((int64_t)1 << 30) || nlayers < 1 || nlayers > KNN_MIX_MAX_LAYERS || !out_base) return false;
    MixPlan pl;
    pl.vec = out_base % 16 == 0 && dp % 4 == 0;
    for (int i = 0; i < nlayers; i++) {
        if (!bases[i] || strides[i] < d) return false;
        pl.vec = pl.vec && bases[i] % 16 == 0 && strides[i] % 4 == 0;
    }
    pl.per_row = (int)(pl.vec ? dp / 4 : dp);
    pl.items = n * pl.per_row;
    pl.grid = (int)std::min<int64_t>((pl.items + MIX_BLOCK - 1) / MIX_BLOCK, MIX_MAX_GRID);
    *out = pl;
    return true;
}

// What knn_mix_into and knn_mix_sweep refuse before anything is allocated, copied or launched: nullptr, or the message.
// layers_set: bit i = layer i has rows; sweep: the arguments of knn_mix_sweep are checked too (k, column, nlevels).
static const char *mix_args_illegal(int d, int nlayers, unsigned layers_set, int flat_d, bool flat_is_view, bool sweep, int64_t g, int64_t k, int64_t column,
                                    int64_t nlevels)
{
    if (nlayers < 1 || nlayers > KNN_MIX_MAX_LAYERS) return "nlayers must be 1 .. KNN_MIX_MAX_LAYERS";
    if (d < 1) return "d must be positive";
    for (int i = 0; i < nlayers; i++)
        if (!((layers_set >> i) & 1u)) return "a layer has no rows (knn_mix_set_layer)";
    if (flat_d != d) return "the index's dimension is not the layers'";
    if (flat_is_view) return "a view is read-only";
    if (!sweep) return nullptr;
    if (g < 0) return "negative number of mixes";
    if (k < 1 || k > KNN_MAX_K) return "k must be 1 .. KNN_MAX_K";
    if (column < 0 || column >= k) return "column must be 0 .. k - 1";
    if (nlevels < 1 || nlevels > KNN_MIX_MAX_LEVELS) return "nlevels must be 1 .. KNN_MIX_MAX_LEVELS";
    return nullptr;
}

// ---- one-dimensional kernel density estimates (kde.inc) -----------------------------
// Constants of the arithmetic contract above knn_kde_stats (include/knn355.h), not functions of the device.
static const int KDE_CHUNK = 16384; // consecutive rows whose terms are summed by one workgroup
static const int KDE_LANES = 256;   // partial sums of a chunk = threads of the workgroup
static const int KDE_TILE = 16;     // grid points of one workgroup = accumulators of a lane

struct KdePlan {
    int64_t group_rows; // rows per group of the statistics: 4096 * ceil(n / (4096 * 256)), the rule of the PCA contract
    int groups;         // ceil(n / group_rows), at most 256
    int64_t tiles;      // ceil(m / KDE_TILE): grid.x of the evaluation
    int64_t chunks;     // ceil(n / KDE_CHUNK): grid.y
    int tail_rows;      // rows of the last chunk, 1 .. KDE_CHUNK
    int tail_points;    // grid points of the last tile, 1 .. KDE_TILE
    int64_t part_bytes; // part[ncols][chunks][m] float64
};

// false: not a legal launch (n < 2, ncols outside [1, KNN_KDE_MAX_COLS], m outside [1, KNN_KDE_MAX_POINTS], more than 65 535
// chunks: n above KNN_KDE_MAX_ROWS)
static bool plan_kde(int64_t n, int64_t ncols, int64_t m, KdePlan *out)
{
    if (n < 2 || n > KNN_KDE_MAX_ROWS || ncols < 1 || ncols > KNN_KDE_MAX_COLS || m < 1 || m > KNN_KDE_MAX_POINTS) return false;
    KdePlan pl;
    pl.group_rows = 4096 * ((n + 4096 * 256 - 1) / (4096 * 256));
    pl.groups = (int)((n + pl.group_rows - 1) / pl.group_rows);
    pl.tiles = (m + KDE_TILE - 1) / KDE_TILE;
    pl.chunks = (n + KDE_CHUNK - 1) / KDE_CHUNK;
    pl.tail_rows = (int)(n - (pl.chunks - 1) * KDE_CHUNK);
    pl.tail_points = (int)(m - (pl.tiles - 1) * KDE_TILE);
    pl.part_bytes = ncols * pl.chunks * m * 8;
    *out = pl;
    return true;
}

// Which flat_scan_kernel build serves a launch is pick_scan_kernel's choice (flat_search.inc) from (query tile, metric, bf16 rows,
// one query tile, width of the difference build or 0, pass of a prefiltered search); this is its legality rule: nullptr, or
// why no build serves the combination (the width of a difference build does not enter: every width has its build).
static const char *scan_kernel_illegal(int qt, bool l2, bool approx16, bool one_qtile, int pass_mode)
{
    // the 256 x 256 tile (2 x 2 waves of 4 x 4 MFMA tiles, one workgroup per CU): plain fp32 rows, several query tiles per launch
    if (qt == 256) return approx16 || pass_mode == 1 ? "scan: the 256-query tile serves plain fp32 rows" : nullptr;
    // the builds on 16-query blocks (48 queries: 4 x 1 waves, 96: 2 x 2 waves): one query tile per launch
    if (qt == 48 || qt == 96) return !one_qtile || approx16 || pass_mode == 1 ? "scan: the 16-query-block builds serve one query tile of plain fp32 rows" : nullptr;
    if (pass_mode == 1) { // the 16-bit pass of a prefiltered search (search_view_s16)
        if (qt != 32) return "scan: the 16-bit prefilter has the 32-query build only";
        return !one_qtile || l2 ? "scan: the 16-bit prefilter serves one 32-query tile, inner product" : nullptr;
    }
    return nullptr;
}
