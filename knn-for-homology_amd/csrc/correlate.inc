// correlate.inc -- tie-averaged ranks and the moment sums of two correlations (included by knn355_lib.hip at the end).
//
// The reference ends its CATH analysis with scipy.stats.pearsonr(scores_best, logged) and scipy.stats.spearmanr(scores_best,
// e_values_cath) (cath/cath.py:949-952).  Spearman's rho is Pearson's r of the tie-averaged ranks, so it needs the order of
// both arrays; that order is rank.inc's (rank_sort with the flat position as payload, no flags).  This file is everything
// behind the sort.  The contract is above knn_eval_rankdata in include/knn355.h; the sizes, the levels of the sums and
// their order are plan_correlate's (plan.h).
//   tie_heads_kernel    flag[r] = 1 when rank r's key image differs from rank r - 1's (rank 0 is a head)
//   rank.inc's scan     the inclusive running count of the flags, in place: the 1-based run number of every rank
//   tie_starts_kernel   every head writes start[run - 1] = r; the last rank writes start[its run] = N behind the last run
//   tie_nan_kernel      one lane: the first rank with the all-ones image (every NaN sorts last); N minus it is the NaN count
//   tie_scatter_kernel  rank2[position of rank r] = start[run - 1] + (start[run] - 1) + 2
//   moment_int_kernel   u = rank2_x - (N + 1), v = rank2_y - (N + 1): the 128-bit sums of u * u, u * v, v * v
//   moment_f64_kernel   the sums of x and y; with the means, the sums of dx * dx, dx * dy, dy * dy
// Both moment kernels sum a level of plan_correlate's order per launch: one workgroup per tile of CORR_TILE terms, lane j
// taking corr_term(tile, j, 0 ..), the lanes folded through LDS by halving offsets, one partial per tile and quantity.
// The integer sums are exact in any order; they take the same one.
// No workgroup waits on another one; there is no atomic; every store is a plain vector store.

template <typename K>
__global__ __launch_bounds__(256) void tie_heads_kernel(const K *__restrict__ keys, uint32_t n, uint32_t *__restrict__ flag)
{
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) flag[r] = (r == 0 || keys[r] != keys[r - 1]) ? 1u : 0u;
}

// run[r] in [1, runs]; start has n + 1 entries and runs <= n
__global__ __launch_bounds__(256) void tie_starts_kernel(const uint32_t *__restrict__ run, uint32_t n, uint32_t *__restrict__ start)
{
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) {
        const uint32_t id = run[r];
        if (id < 1 || id > n) continue; // (never, when run is the scan of this input's flags: a store never leaves the buffer)
        if (r == 0 || run[r - 1] != id) start[id - 1] = (uint32_t)r;
        if (r == (uint64_t)n - 1) start[id] = n;
    }
}

template <typename K>
__global__ __launch_bounds__(64) void tie_nan_kernel(const K *__restrict__ keys, uint32_t n, int64_t *__restrict__ count)
{
    if (blockIdx.x || threadIdx.x) return;
    const K all = ~(K)0;
    const int64_t lo = lower_bound_dev((int64_t)0, (int64_t)n, [&](int64_t i) { return keys[i] < all; });
    *count = (int64_t)n - lo;
}

template <typename OUT>
__global__ __launch_bounds__(256) void tie_scatter_kernel(const uint32_t *__restrict__ pay, const uint32_t *__restrict__ run,
                                                          const uint32_t *__restrict__ start, uint32_t n, OUT *__restrict__ rank2)
{
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) {
        const uint32_t id = run[r], p = pay[r] >> 1;
        if (id < 1 || id > n || p >= n) continue; // (never: see tie_starts_kernel)
        rank2[p] = (OUT)((uint64_t)start[id - 1] + (uint64_t)start[id] + 1u); // s + e + 2 with e = start[id] - 1
    }
}

// ---- the moments
struct MomentSrc {
    const void *x, *y; // the device copies, [rows][k]
    int x64, y64;      // float64, else float32
    uint32_t k, limit;
    int centred;       // 0: the terms are x, y, 0; else dx * dx, dx * dy, dy * dy
    double mx, my;
};

__device__ __forceinline__ double moment_value(const void *a, int is64, size_t cell)
{
    return is64 ? ((const double *)a)[cell] : (double)((const float *)a)[cell];
}

// level 0 reads the arrays, a later level the partials in[3][n]; out is [3][n_out], n_out = gridDim.x = ceil(n / CORR_TILE)
template <bool LEVEL0>
__global__ __launch_bounds__(CORR_LANES) void moment_f64_kernel(MomentSrc s, const double *__restrict__ in, uint64_t n, double *__restrict__ out)
{
    __shared__ double s_r[3][CORR_LANES];
    const int tid = threadIdx.x;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0;
#pragma unroll
    for (int i = 0; i < CORR_TILE / CORR_LANES; i++) {
        const uint64_t e = corr_term(blockIdx.x, tid, i);
        if (e < n) {
            double t0, t1, t2;
            if (LEVEL0) {
                const uint32_t p = (uint32_t)e, row = p / s.limit, col = p - row * s.limit;
                const size_t cell = (size_t)row * s.k + col;
                const double x = moment_value(s.x, s.x64, cell), y = moment_value(s.y, s.y64, cell);
                if (s.centred) {
                    const double dx = x - s.mx, dy = y - s.my;
                    t0 = dx * dx;
                    t1 = dx * dy;
                    t2 = dy * dy;
                } else {
                    t0 = x;
                    t1 = y;
                    t2 = 0.0;
                }
            } else {
                t0 = in[e];
                t1 = in[n + e];
                t2 = in[2 * n + e];
            }
            a0 = a0 + t0;
            a1 = a1 + t1;
            a2 = a2 + t2;
        }
    }
    s_r[0][tid] = a0;
    s_r[1][tid] = a1;
    s_r[2][tid] = a2;
    __syncthreads();
    for (int off = CORR_LANES / 2; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int q = 0; q < 3; q++) s_r[q][tid] = s_r[q][tid] + s_r[q][tid + off];
        }
        __syncthreads();
    }
    if (tid < 3) out[(uint64_t)tid * gridDim.x + blockIdx.x] = s_r[tid][0];
}

// a 128-bit two's-complement sum as (lo, hi)
struct Wide128 {
    uint64_t lo, hi;
};
__device__ __forceinline__ void wide_add(Wide128 &a, uint64_t lo, uint64_t hi)
{
    a.lo += lo;
    a.hi += hi + (a.lo < lo ? 1u : 0u);
}

// level 0 reads the doubled ranks, a later level the partials in[3][n] of (lo, hi) pairs; out is [3][n_out] pairs
template <bool LEVEL0>
__global__ __launch_bounds__(CORR_LANES) void moment_int_kernel(const uint32_t *__restrict__ rx, const uint32_t *__restrict__ ry, int64_t centre,
                                                                const uint64_t *__restrict__ in, uint64_t n, uint64_t *__restrict__ out)
{
    __shared__ uint64_t s_lo[3][CORR_LANES], s_hi[3][CORR_LANES];
    const int tid = threadIdx.x;
    Wide128 a[3] = {{0, 0}, {0, 0}, {0, 0}};
#pragma unroll
    for (int i = 0; i < CORR_TILE / CORR_LANES; i++) {
        const uint64_t e = corr_term(blockIdx.x, tid, i);
        if (e < n) {
            if (LEVEL0) {
                const int64_t u = (int64_t)rx[e] - centre, v = (int64_t)ry[e] - centre; // |u|, |v| <= N - 1 < 2^31
                const int64_t t[3] = {u * u, u * v, v * v};
#pragma unroll
                for (int q = 0; q < 3; q++) wide_add(a[q], (uint64_t)t[q], t[q] < 0 ? ~(uint64_t)0 : 0); // sign-extended
            } else {
#pragma unroll
                for (int q = 0; q < 3; q++) wide_add(a[q], in[2 * (q * n + e)], in[2 * (q * n + e) + 1]);
            }
        }
    }
#pragma unroll
    for (int q = 0; q < 3; q++) {
        s_lo[q][tid] = a[q].lo;
        s_hi[q][tid] = a[q].hi;
    }
    __syncthreads();
    for (int off = CORR_LANES / 2; off > 0; off >>= 1) {
        if (tid < off) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                Wide128 w = {s_lo[q][tid], s_hi[q][tid]};
                wide_add(w, s_lo[q][tid + off], s_hi[q][tid + off]);
                s_lo[q][tid] = w.lo;
                s_hi[q][tid] = w.hi;
            }
        }
        __syncthreads();
    }
    if (tid < 3) {
        const uint64_t o = 2 * ((uint64_t)tid * gridDim.x + blockIdx.x);
        out[o] = s_lo[tid][0];
        out[o + 1] = s_hi[tid][0];
    }
}

// ---- host -------------------------------------------------------------------------------
// measurement (tools/bench_correlation.py): how this thread's last successful knn_eval_rankdata / knn_eval_correlate ran
// host clock: allocations; HIP events (the clock's phases): uploads, sorts, ranks, moments, downloads
enum { CORR_ALLOC, CORR_UP, CORR_SORT, CORR_RANKS, CORR_MOMENTS, CORR_DOWN, CORR_PHASES };
static thread_local struct {
    float ms[CORR_PHASES];
} g_correlate_info = {{0, 0, 0, 0, 0, 0}};

// the buffers of a CorrelatePlan that both sorts share, untyped
struct CorrShared {
    void *k0 = nullptr, *k1 = nullptr;
    uint32_t *p0 = nullptr, *p1 = nullptr, *table = nullptr, *partial = nullptr, *run = nullptr, *start = nullptr;
    unsigned int *hist = nullptr;
    int64_t *nan = nullptr;
};

// one array: upload, sort, the run of every rank, the NaN count into *d_nan, and -- d_rank2 given -- the doubled ranks
template <typename K, typename OUT>
static int corr_ranks(const void *a, int64_t rows, int64_t k, int64_t limit, const RankPlan &rp, const CorrelatePlan &pl, const CorrShared &sh,
                      typename RankFloat<K>::F *d_a, PhaseClock &clock, int64_t *d_nan, OUT *d_rank2)
{
    const uint32_t n = (uint32_t)pl.n;
    RankSorted<K> rs;
    rs.d_scores = d_a;
    rs.d_k0 = (K *)sh.k0;
    rs.d_k1 = (K *)sh.k1;
    rs.d_p0 = sh.p0;
    rs.d_p1 = sh.p1;
    rs.d_table = sh.table;
    rs.d_partial = sh.partial;
    rs.d_hist = sh.hist;
    EVAL_TRY(rank_sort<K>(a, rows, k, limit, nullptr, 0, rp, clock, CORR_UP, CORR_SORT, CORR_RANKS, rs));
    const dim3 grid((unsigned)pl.tie_grid), block(256);
    hipLaunchKernelGGL(tie_heads_kernel<K>, grid, block, 0, 0, rs.keys, n, sh.run);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(rank_scan<true>(sh.run, (uint64_t)n, sh.partial, sh.run));
    hipLaunchKernelGGL(tie_starts_kernel, grid, block, 0, 0, (const uint32_t *)sh.run, n, sh.start);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tie_nan_kernel<K>, dim3(1), dim3(64), 0, 0, rs.keys, n, d_nan);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(tie_scatter_kernel<OUT>, grid, block, 0, 0, rs.pay, (const uint32_t *)sh.run, (const uint32_t *)sh.start, n, d_rank2);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(clock.close(nullptr)); // (the next array's packing on the host is in no phase)
    return 0;
}

// an array that is not sorted (KNN_CORR_PEARSON alone): rank_sort's packing and upload
template <typename F>
static int corr_upload(const void *a, int64_t rows, int64_t k, int64_t limit, const RankPlan &rp, F *d_a, PhaseClock &clock)
{
    const F *up = (const F *)a;
    std::vector<F> packed;
    if (rp.pack) {
        packed.resize((size_t)rp.n);
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < rows; r++) memcpy(packed.data() + (size_t)r * limit, (const F *)a + (size_t)r * k, (size_t)limit * sizeof(F));
        up = packed.data();
    }
    EVAL_TRY(clock.open(CORR_UP, nullptr));
    HIP_TRY(hipMemcpy(d_a, up, rp.scores_bytes, hipMemcpyHostToDevice));
    EVAL_TRY(clock.close(nullptr));
    return 0;
}

// one reduction of plan_correlate's levels; *result = the device address of the three sums
template <typename LAUNCH>
static int corr_levels(const CorrelatePlan &pl, void *d_a, void *d_b, LAUNCH launch, void **result)
{
    void *in = nullptr, *out = d_a;
    for (int l = 0; l < pl.levels; l++) {
        launch(l, in, (uint64_t)pl.level_n[l], out, (unsigned)pl.level_n[l + 1]);
        HIP_TRY(hipGetLastError());
        in = out;
        out = out == d_a ? d_b : d_a;
    }
    *result = in;
    return 0;
}

template <typename KX, typename KY>
static int correlate_run(const void *x, const void *y, int64_t rows, int64_t k, int64_t limit, const CorrelatePlan &pl, int64_t *rank2_out,
                         double *pearson_out, uint64_t *spearman_out, int64_t *nan_out /* [2] */)
{
    typedef typename RankFloat<KX>::F FX;
    typedef typename RankFloat<KY>::F FY;
    const uint32_t n = (uint32_t)pl.n;
    const bool pearson = (pl.what & KNN_CORR_PEARSON) != 0, spearman = (pl.what & KNN_CORR_SPEARMAN) != 0;
    const auto t_alloc = std::chrono::steady_clock::now();
    EvalBufs bufs;
    PhaseClock clock;
    auto opt = [&](size_t bytes, bool &ok) -> void * {
        if (!bytes) return nullptr;
        void *p = bufs.get(bytes);
        if (!p) ok = false;
        return p;
    };
    bool ok = true;
    CorrShared sh;
    FX *d_x = (FX *)opt(pl.x_bytes, ok);
    FY *d_y = (FY *)opt(pl.y_bytes, ok);
    sh.k0 = opt(pl.keys_bytes, ok);
    sh.k1 = opt(pl.keys_bytes, ok);
    sh.p0 = (uint32_t *)opt(pl.pay_bytes, ok);
    sh.p1 = (uint32_t *)opt(pl.pay_bytes, ok);
    sh.table = (uint32_t *)opt(pl.table_bytes, ok);
    sh.partial = (uint32_t *)opt(pl.partial_bytes, ok);
    sh.hist = (unsigned int *)opt(pl.hist_bytes, ok);
    sh.run = (uint32_t *)opt(pl.run_bytes, ok);
    sh.start = (uint32_t *)opt(pl.start_bytes, ok);
    void *d_r0 = pl.rank2_buffers > 0 ? opt(pl.rank2_bytes, ok) : nullptr;
    void *d_r1 = pl.rank2_buffers > 1 ? opt(pl.rank2_bytes, ok) : nullptr;
    sh.nan = (int64_t *)opt(pl.nan_bytes, ok);
    void *d_ma = opt(pl.moment_a_bytes, ok);
    void *d_mb = opt(pl.moment_b_bytes, ok);
    if (!ok) return set_err(KNN_ERR_HIP, "eval: out of device memory");
    size_t allocated = 0;
    for (const auto &b : bufs.dev) allocated += b.second;
    if (allocated != pl.resident_bytes) return set_err(KNN_ERR_INVALID, "correlate: the buffers are not the plan's");
    const auto t_up = std::chrono::steady_clock::now();
    int64_t nan[2] = {0, 0};
    // ---- the orders and the doubled ranks
    if (pl.what == 0) {
        EVAL_TRY((corr_ranks<KX, int64_t>(x, rows, k, limit, pl.rank_x, pl, sh, d_x, clock, sh.nan, (int64_t *)d_r0)));
    } else if (spearman) {
        EVAL_TRY((corr_ranks<KX, uint32_t>(x, rows, k, limit, pl.rank_x, pl, sh, d_x, clock, sh.nan, (uint32_t *)d_r0)));
        EVAL_TRY((corr_ranks<KY, uint32_t>(y, rows, k, limit, pl.rank_y, pl, sh, d_y, clock, sh.nan + 1, (uint32_t *)d_r1)));
    } else {
        EVAL_TRY(corr_upload<FX>(x, rows, k, limit, pl.rank_x, d_x, clock));
        EVAL_TRY(corr_upload<FY>(y, rows, k, limit, pl.rank_y, d_y, clock));
    }
    if (pl.sorts) {
        EVAL_TRY(clock.open(CORR_DOWN, nullptr));
        HIP_TRY(hipMemcpy(nan, sh.nan, (pl.what ? 2 : 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        EVAL_TRY(clock.close(nullptr));
    }
    const bool has_nan = nan[0] != 0 || nan[1] != 0;
    // ---- the moments
    uint64_t sums_int[6];
    double pear[5];
    if (spearman && !has_nan) {
        EVAL_TRY(clock.open(CORR_MOMENTS, nullptr));
        void *res = nullptr;
        EVAL_TRY(corr_levels(pl, d_ma, d_mb, [&](int l, void *in, uint64_t m, void *out, unsigned grid) {
            if (l == 0)
                hipLaunchKernelGGL(moment_int_kernel<true>, dim3(grid), dim3(CORR_LANES), 0, 0, (const uint32_t *)d_r0, (const uint32_t *)d_r1,
                                   (int64_t)n + 1, (const uint64_t *)nullptr, m, (uint64_t *)out);
            else
                hipLaunchKernelGGL(moment_int_kernel<false>, dim3(grid), dim3(CORR_LANES), 0, 0, (const uint32_t *)nullptr, (const uint32_t *)nullptr,
                                   (int64_t)0, (const uint64_t *)in, m, (uint64_t *)out);
        }, &res));
        EVAL_TRY(clock.next(CORR_DOWN, nullptr));
        HIP_TRY(hipMemcpy(sums_int, res, sizeof sums_int, hipMemcpyDeviceToHost));
        EVAL_TRY(clock.close(nullptr));
    }
    if (pearson) {
        MomentSrc src = {d_x, d_y, sizeof(FX) == 8, sizeof(FY) == 8, (uint32_t)pl.rank_x.dev_k, (uint32_t)limit, 0, 0.0, 0.0};
        for (int pass = 0; pass < 2; pass++) { // the sums of x and y; then, about the means, the three centred sums
            src.centred = pass;
            EVAL_TRY(clock.open(CORR_MOMENTS, nullptr));
            void *res = nullptr;
            EVAL_TRY(corr_levels(pl, d_ma, d_mb, [&](int l, void *in, uint64_t m, void *out, unsigned grid) {
                if (l == 0) hipLaunchKernelGGL(moment_f64_kernel<true>, dim3(grid), dim3(CORR_LANES), 0, 0, src, (const double *)nullptr, m, (double *)out);
                else hipLaunchKernelGGL(moment_f64_kernel<false>, dim3(grid), dim3(CORR_LANES), 0, 0, src, (const double *)in, m, (double *)out);
            }, &res));
            EVAL_TRY(clock.next(CORR_DOWN, nullptr));
            double s[3];
            HIP_TRY(hipMemcpy(s, res, sizeof s, hipMemcpyDeviceToHost));
            EVAL_TRY(clock.close(nullptr));
            if (pass == 0) {
                pear[0] = src.mx = s[0] / (double)pl.n;
                pear[1] = src.my = s[1] / (double)pl.n;
            } else {
                memcpy(pear + 2, s, sizeof s);
            }
        }
    }
    if (rank2_out && !has_nan) {
        EVAL_TRY(clock.open(CORR_DOWN, nullptr));
        HIP_TRY(hipMemcpy(rank2_out, d_r0, (size_t)n * 8, hipMemcpyDeviceToHost));
        EVAL_TRY(clock.close(nullptr));
    }
    HIP_TRY(hipDeviceSynchronize());
    float ms[CORR_PHASES];
    EVAL_TRY(clock.read(ms, CORR_PHASES));
    ms[CORR_ALLOC] = std::chrono::duration<float, std::milli>(t_up - t_alloc).count();
    // the call has succeeded: only now are the outputs written
    if (pl.sorts && nan_out) memcpy(nan_out, nan, (pl.what ? 2 : 1) * sizeof(int64_t));
    if (spearman && !has_nan) memcpy(spearman_out, sums_int, sizeof sums_int);
    if (pearson) memcpy(pearson_out, pear, sizeof pear);
    memcpy(g_correlate_info.ms, ms, sizeof ms);
    return 0;
}

static int correlate_shape_illegal(const char *who, int64_t rows, int64_t k, int64_t limit)
{
    if (rows < 1) return set_err(KNN_ERR_INVALID, std::string(who) + ": need rows >= 1");
    if (k < 1) return set_err(KNN_ERR_INVALID, std::string(who) + ": need k >= 1");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, std::string(who) + ": k > INT32_MAX");
    if (limit < 1 || limit > k) return set_err(KNN_ERR_INVALID, std::string(who) + ": limit outside [1, k]");
    return 0;
}

extern "C" int knn_eval_rankdata(const void *a, int32_t key_type, int64_t rows, int64_t k, int64_t limit, int64_t *rank2_out, int32_t *nan_count_out)
{
    if (key_type != KNN_RANK_F32 && key_type != KNN_RANK_F64) return set_err(KNN_ERR_INVALID, "rankdata: unknown key type");
    EVAL_TRY(correlate_shape_illegal("rankdata", rows, k, limit));
    CorrelatePlan pl;
    if (!plan_correlate(rows, k, limit, key_type == KNN_RANK_F64 ? 8 : 4, 0, 0, &pl))
        return set_err(KNN_ERR_INVALID, "rankdata: rows * limit outside [2, 2^31 - 1], or rows * k too large");
    if (!a || !rank2_out || !nan_count_out) return set_err(KNN_ERR_INVALID, "rankdata: null pointer");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    int64_t nan[2] = {0, 0};
    rc = key_type == KNN_RANK_F64 ? correlate_run<uint64_t, uint64_t>(a, nullptr, rows, k, limit, pl, rank2_out, nullptr, nullptr, nan)
                                  : correlate_run<uint32_t, uint32_t>(a, nullptr, rows, k, limit, pl, rank2_out, nullptr, nullptr, nan);
    if (rc) return rc;
    *nan_count_out = (int32_t)nan[0]; // (<= N <= 2^31 - 1)
    return 0;
}

extern "C" int knn_eval_correlate(const void *x, int32_t x_type, const void *y, int32_t y_type, int64_t rows, int64_t k, int64_t limit, int32_t what,
                                  double *pearson_out, uint64_t *spearman_out, int64_t *nan_count_out)
{
    if ((x_type != KNN_RANK_F32 && x_type != KNN_RANK_F64) || (y_type != KNN_RANK_F32 && y_type != KNN_RANK_F64))
        return set_err(KNN_ERR_INVALID, "correlate: unknown type");
    EVAL_TRY(correlate_shape_illegal("correlate", rows, k, limit));
    if (what < 1 || what > (KNN_CORR_PEARSON | KNN_CORR_SPEARMAN)) return set_err(KNN_ERR_INVALID, "correlate: what is KNN_CORR_PEARSON | KNN_CORR_SPEARMAN");
    CorrelatePlan pl;
    if (!plan_correlate(rows, k, limit, x_type == KNN_RANK_F64 ? 8 : 4, y_type == KNN_RANK_F64 ? 8 : 4, what, &pl))
        return set_err(KNN_ERR_INVALID, "correlate: rows * limit outside [2, 2^31 - 1], or rows * k too large");
    if (!x || !y) return set_err(KNN_ERR_INVALID, "correlate: null pointer");
    if ((what & KNN_CORR_PEARSON) && !pearson_out) return set_err(KNN_ERR_INVALID, "correlate: null pearson_out");
    if ((what & KNN_CORR_SPEARMAN) && (!spearman_out || !nan_count_out)) return set_err(KNN_ERR_INVALID, "correlate: null spearman_out or nan_count_out");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    if (x_type == KNN_RANK_F64)
        return y_type == KNN_RANK_F64 ? correlate_run<uint64_t, uint64_t>(x, y, rows, k, limit, pl, nullptr, pearson_out, spearman_out, nan_count_out)
                                      : correlate_run<uint64_t, uint32_t>(x, y, rows, k, limit, pl, nullptr, pearson_out, spearman_out, nan_count_out);
    return y_type == KNN_RANK_F64 ? correlate_run<uint32_t, uint64_t>(x, y, rows, k, limit, pl, nullptr, pearson_out, spearman_out, nan_count_out)
                                  : correlate_run<uint32_t, uint32_t>(x, y, rows, k, limit, pl, nullptr, pearson_out, spearman_out, nan_count_out);
}

extern "C" int knn_last_correlate_info(float *ms)
{
    if (!ms) return set_err(KNN_ERR_INVALID, "last_correlate_info: null pointer");
    for (int i = 0; i < CORR_PHASES; i++) ms[i] = g_correlate_info.ms[i];
    return 0;
}
