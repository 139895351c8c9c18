// buckets.inc -- accuracy per score bucket and the accuracy-over-hits curve of (is_correct, scores) (included by knn355_lib.hip
// behind pr_curve.inc).
//
// The reference bins its hits in a Python loop over 300 buckets, each iteration a handful of passes over the whole
// [queries, 300] matrix (pfam/proteins.py:689-729), and draws the "fraction of homologues found after j hits" curve from
// a cumsum / tile / mean over the same matrix (proteins.py:502-507; the last column of it before the mean is the per-query
// recall of proteins.py:476-496).  Here each is one pass; the contracts are above knn_eval_bucket_counts and
// knn_eval_hit_curve in include/knn355.h.
//
//   bucket_hist_kernel  256 threads, one wave per row, the workgroups striding over the slab's rows; the lanes stride over
//     the row's `limit` cells (coalesced loads of the score row and the byte row).
//     binning    with lo and hi sorted and lo <= hi, the buckets of a cell with score s are h .. a - 1, where
//                a = #{i : lo[i] < s} and h = #{i : hi[i] < s} <= a: two binary searches over the edges in LDS, the second
//                over [0, a) only.  A NaN compares false everywhere: a = h = 0, no bucket.
//     histogram  a cell with a > h adds (1 << 32 | correct) to word a of one LDS histogram and to word h of another
//                (ds_add_u64; a slab holds at most 2^31 cells, so neither half overflows).  count[b] is then
//                #{h <= b} - #{a <= b}: a difference of two prefix sums, taken on the host over the nb + 1 words.
//     contention real cosine scores pile into a few dozen buckets and a wave whose lanes hit one LDS word serialises there.
//                Measured (DESIGN 4.7j), that costs little: every lane adding for itself takes the same time on
//                clustered scores as on uniform ones and 1.4 times that with every cell in one bucket.  So that is what
//                runs.  KNN355_BUCKET_AGG=1 first merges equal (a, h) pairs inside the wave -- up to BUCKET_AGG_ROUNDS times
//                the first pending lane broadcasts its pair, the lanes that hold the same pair are counted by ballot and
//                popcount, and the leader adds for all of them -- which wins only in the one-bucket case: the knob is
//                kept so that tools/bench_buckets.py can repeat the comparison.
//     flush      the non-zero words go to four global arrays of 64-bit counters by integer atomicAdd.
//   hit_terms_kernel    one wave per row: C(q, j) by ballot and popcount over groups of 64 columns with a carry, the
//                       quotient t(q, j) into a [slab rows][limit] scratch of doubles, the row's count, and the number of
//                       correct cells per column (LDS counters, flushed by atomicAdd; the column sums of C are their
//                       prefix sum).
//   hit_fold_kernel     one workgroup per 32 columns.  All 256 threads carry tiles of 128 rows x 32 columns from the
//                       scratch into LDS, one tile ahead; the first 32 threads add a tile's rows to the running S(j) in
//                       row order.  Only the adds are serial.

#define BUCKET_AGG_ROUNDS 4

struct BucketParams {
    const void *scores;        // the slab's rows [rows][k], float or double
    const uint8_t *is_correct; // [rows][k]
    const double *lo, *hi;     // [nb]
    int64_t rows;
    int k, limit, nb, agg;
    unsigned long long *cnt; // [4][nb + 1]: selected marks at a, at h; correct marks at a, at h
};

template <typename T>
__global__ __launch_bounds__(256) void bucket_hist_kernel(BucketParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int nb = p.nb, n1 = nb + 1;
    double *s_lo = (double *)smem, *s_hi = s_lo + nb;             // [nb] each
    unsigned long long *s_a = (unsigned long long *)(s_hi + nb); // [n1] marks at a, then [n1] marks at h
    unsigned long long *s_h = s_a + n1;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < nb; i += 256) {
        s_lo[i] = p.lo[i];
        s_hi[i] = p.hi[i];
    }
    for (int i = tid; i < 2 * n1; i += 256) s_a[i] = 0;
    __syncthreads();
    const T *scores = (const T *)p.scores;
    const int64_t limit = p.limit;
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < p.rows; r += (int64_t)gridDim.x * 4) {
        const T *sc = scores + r * p.k;
        const uint8_t *ic = p.is_correct + r * p.k;
        for (int64_t c0 = 0; c0 < limit; c0 += 64) { // (uniform in the wave)
            const int64_t c = c0 + lane;
            int a = 0, h = 0;
            bool ok = false;
            if (c < limit) {
                const double v = (double)sc[c];
                a = lower_bound_dev(0, nb, [&](int i) { return s_lo[i] < v; });
                h = lower_bound_dev(0, a, [&](int i) { return s_hi[i] < v; });
                ok = ic[c] != 0;
            }
            bool pending = a > h;
            if (p.agg) {
                const int key = a * 8192 + h; // (a, h <= 4096)
                for (int round = 0; round < BUCKET_AGG_ROUNDS; round++) {
                    const unsigned long long pm = __ballot(pending);
                    if (!pm) break;
                    const int leader = __ffsll((long long)pm) - 1;
                    const bool same = pending && key == __shfl(key, leader, 64);
                    const unsigned long long sm = __ballot(same), sc_ok = __ballot(same && ok);
                    if (lane == leader) {
                        const unsigned long long inc = ((unsigned long long)__popcll(sm) << 32) | (unsigned long long)__popcll(sc_ok);
                        atomicAdd(&s_a[a], inc);
                        atomicAdd(&s_h[h], inc);
                    }
                    pending = pending && !same;
                }
            }
            if (pending) {
                const unsigned long long inc = (1ull << 32) | (ok ? 1ull : 0ull);
                atomicAdd(&s_a[a], inc);
                atomicAdd(&s_h[h], inc);
            }
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * n1; i += 256) {
        const unsigned long long v = s_a[i];
        if (v >> 32) atomicAdd(&p.cnt[i], v >> 32);
        if (v & 0xFFFFFFFFull) atomicAdd(&p.cnt[2 * (size_t)n1 + i], v & 0xFFFFFFFFull);
    }
}

template <typename T>
static int bucket_hist_launch(const BucketParams &p, unsigned blocks, size_t lds)
{
    HIP_TRY(hipFuncSetAttribute((const void *)bucket_hist_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(bucket_hist_kernel<T>, dim3(blocks), dim3(256), lds, 0, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// KNN355_BUCKET_AGG=1: merge equal bins inside the wave first (read on every call; anything else, or nothing: no merging)
static int bucket_agg_mode()
{
    const char *e = getenv("KNN355_BUCKET_AGG");
    return e && e[0] == '1' && e[1] == '\0' ? 1 : 0;
}

// the phases of this thread's last successful knn_eval_bucket_counts [0] and knn_eval_hit_curve [1]
enum { BUCKETS_UP, BUCKETS_KERNELS, BUCKETS_DOWN, BUCKETS_PHASES };
static thread_local float g_buckets_ms[2][BUCKETS_PHASES] = {{0, 0, 0}, {0, 0, 0}};

extern "C" int knn_eval_bucket_counts(const void *scores, int32_t key_type, const uint8_t *is_correct, int64_t nq, int64_t k, int64_t limit,
                                      const double *lo, const double *hi, int32_t nb, int64_t *count_out, int64_t *correct_out)
{
    if (key_type != KNN_RANK_F32 && key_type != KNN_RANK_F64) return set_err(KNN_ERR_INVALID, "bucket_counts: unknown key type");
    if (nq < 1) return set_err(KNN_ERR_INVALID, "bucket_counts: need nq >= 1");
    if (k < 1) return set_err(KNN_ERR_INVALID, "bucket_counts: need k >= 1");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "bucket_counts: k > INT32_MAX");
    if (limit < 1 || limit > k) return set_err(KNN_ERR_INVALID, "bucket_counts: limit outside [1, k]");
    if (nb < 1 || nb > 4096) return set_err(KNN_ERR_INVALID, "bucket_counts: nb outside [1, 4096]");
    if (!scores || !is_correct || !lo || !hi || !count_out || !correct_out) return set_err(KNN_ERR_INVALID, "bucket_counts: null pointer");
    for (int32_t b = 0; b < nb; b++) {
        if (lo[b] != lo[b] || hi[b] != hi[b]) return set_err(KNN_ERR_INVALID, "bucket_counts: NaN edge");
        if (b && (lo[b] < lo[b - 1] || hi[b] < hi[b - 1])) return set_err(KNN_ERR_INVALID, "bucket_counts: edges decrease");
        if (lo[b] > hi[b]) return set_err(KNN_ERR_INVALID, "bucket_counts: a lower edge above its upper edge");
    }
    int rc = ensure_device(g_device);
    if (rc) return rc;
    // a slab holds at most 2^31 cells: the packed LDS words of one workgroup cannot overflow
    const int64_t slab = std::min(nq, std::min(eval_slab_rows(k), std::max<int64_t>(1, ((int64_t)1 << 31) / limit)));
    const size_t esz = key_type == KNN_RANK_F64 ? 8 : 4, n1 = (size_t)nb + 1, lds = (size_t)nb * 16 + 2 * n1 * 8;
    const int agg = bucket_agg_mode();
    HostCall call;
    EvalBufs &bufs = call.bufs;
    PhaseClock &clock = call.clock;
    std::vector<int64_t> cnt(4 * n1);
    EvalCols tab(bufs, 1), w(bufs, slab);
    const double *d_lo = tab.in(lo, (size_t)nb * 8);
    const double *d_hi = tab.in(hi, (size_t)nb * 8);
    unsigned long long *d_cnt = (unsigned long long *)tab.out(cnt.data(), cnt.size() * 8);
    const uint8_t *d_ic = w.in(is_correct, (size_t)k);
    const char *d_sc = w.in((const char *)scores, (size_t)k * esz);
    EVAL_TRY(w.ready());
    EVAL_TRY(clock.open(BUCKETS_UP, call.s));
    EVAL_TRY(tab.upload(0, 1));
    HIP_TRY(hipMemset(d_cnt, 0, cnt.size() * 8));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(clock.next(BUCKETS_UP, call.s));
        EVAL_TRY(w.upload(r0, m));
        const BucketParams p = {d_sc, d_ic, d_lo, d_hi, m, (int)k, (int)limit, nb, agg, d_cnt};
        const unsigned blocks = (unsigned)std::min<int64_t>((m + 3) / 4, 1024);
        EVAL_TRY(clock.next(BUCKETS_KERNELS, call.s));
        EVAL_TRY(esz == 8 ? bucket_hist_launch<double>(p, blocks, lds) : bucket_hist_launch<float>(p, blocks, lds));
    }
    EVAL_TRY(clock.next(BUCKETS_DOWN, call.s));
    EVAL_TRY(tab.download(0, 1));
    EVAL_TRY(clock.close(call.s));
    EVAL_TRY(call.finish("bucket_counts", 0));
    float ms[BUCKETS_PHASES];
    EVAL_TRY(clock.read(ms, BUCKETS_PHASES));
    // count[b] = #{cells with h <= b} - #{cells with a <= b}, over the cells with a > h
    int64_t sel = 0, cor = 0;
    for (size_t b = 0; b < (size_t)nb; b++) {
        sel += cnt[n1 + b] - cnt[b];
        cor += cnt[3 * n1 + b] - cnt[2 * n1 + b];
        count_out[b] = sel;
        correct_out[b] = cor;
    }
    memcpy(g_buckets_ms[0], ms, sizeof ms);
    return 0;
}

#define HIT_LDS_COLS 16384 // columns whose correct cells are counted in LDS (64 KB); past them: global atomics
#define HIT_FOLD_COLS 32
#define HIT_FOLD_ROWS 128

struct HitParams {
    const uint8_t *is_correct; // the slab's rows [rows][k]
    const int64_t *totals;     // [rows]
    int64_t rows;
    int k, limit, lds_cols;
    double *terms;            // [rows][limit]
    int64_t *row_correct;     // [rows], or null
    unsigned long long *cols; // [limit] correct cells per column over the whole call, or null
};

__global__ __launch_bounds__(256) void hit_terms_kernel(HitParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    unsigned int *s_col = (unsigned int *)smem; // [lds_cols]; a slab has fewer than 2^32 rows
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t limit = p.limit;
    if (p.cols) {
        for (int i = tid; i < p.lds_cols; i += 256) s_col[i] = 0;
        __syncthreads();
    }
    for (int64_t r = (int64_t)blockIdx.x * 4 + wave; r < p.rows; r += (int64_t)gridDim.x * 4) {
        const uint8_t *ic = p.is_correct + r * p.k;
        const double total = (double)p.totals[r];
        double *t = p.terms + r * limit;
        int64_t carry = 0; // correct cells in front of this group of 64 columns
        for (int64_t c0 = 0; c0 < limit; c0 += 64) {
            const int64_t c = c0 + lane;
            const bool ok = c < limit && ic[c] != 0;
            const unsigned long long m = __ballot(ok);
            if (c < limit) t[c] = (double)(carry + __popcll(m & (~0ull >> (63 - lane)))) / total;
            if (ok && p.cols) {
                if (c < p.lds_cols) atomicAdd(&s_col[c], 1u);
                else atomicAdd(&p.cols[c], 1ull);
            }
            carry += __popcll(m);
        }
        if (lane == 0 && p.row_correct) p.row_correct[r] = carry;
    }
    if (p.cols) {
        __syncthreads();
        for (int i = tid; i < p.lds_cols; i += 256)
            if (s_col[i]) atomicAdd(&p.cols[i], (unsigned long long)s_col[i]);
    }
}

// sums[j] += terms[0][j], then terms[1][j], ...: the running S of the contract
__global__ __launch_bounds__(256) void hit_fold_kernel(const double *__restrict__ terms, int64_t rows, int64_t limit, double *__restrict__ sums)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double(*s_t)[HIT_FOLD_ROWS][HIT_FOLD_COLS] = (double(*)[HIT_FOLD_ROWS][HIT_FOLD_COLS])smem; // two tiles
    const int tid = threadIdx.x, col = tid & (HIT_FOLD_COLS - 1), rs = tid / HIT_FOLD_COLS; // rs: 0 .. 7
    constexpr int PER = HIT_FOLD_ROWS * HIT_FOLD_COLS / 256; // rows of a tile per thread
    constexpr int STEP = 256 / HIT_FOLD_COLS;
    const int64_t j = (int64_t)blockIdx.x * HIT_FOLD_COLS + col;
    const bool live = j < limit, adder = tid < HIT_FOLD_COLS;
    const int64_t ntiles = (rows + HIT_FOLD_ROWS - 1) / HIT_FOLD_ROWS;
    double s = adder && live ? sums[j] : 0.0;
    double reg[PER];
    auto load = [&](int64_t row0) {
#pragma unroll
        for (int i = 0; i < PER; i++) {
            const int64_t r = row0 + rs + STEP * i;
            reg[i] = live && r < rows ? terms[r * limit + j] : 0.0;
        }
    };
    auto store = [&](int b) {
#pragma unroll
        for (int i = 0; i < PER; i++) s_t[b][rs + STEP * i][col] = reg[i];
    };
    load(0);
    store(0);
    __syncthreads();
    for (int64_t t = 0; t < ntiles; t++) {
        const int b = (int)(t & 1);
        if (t + 1 < ntiles) load((t + 1) * HIT_FOLD_ROWS); // in flight while the adders work
        if (adder) {
            const int64_t n = std::min<int64_t>(HIT_FOLD_ROWS, rows - t * HIT_FOLD_ROWS);
            if (n == HIT_FOLD_ROWS) {
#pragma unroll 16
                for (int r = 0; r < HIT_FOLD_ROWS; r++) s += s_t[b][r][col];
            } else {
                for (int r = 0; r < (int)n; r++) s += s_t[b][r][col];
            }
        }
        if (t + 1 < ntiles) store(b ^ 1);
        __syncthreads(); // the next tile is in LDS; this one has been added and may be overwritten
    }
    if (adder && live) sums[j] = s;
}

extern "C" int knn_eval_hit_curve(const uint8_t *is_correct, int64_t nq, int64_t k, int64_t limit, const int64_t *totals, double *mean_out,
                                  int64_t *row_correct_out, int64_t *column_correct_out)
{
    if (nq < 1) return set_err(KNN_ERR_INVALID, "hit_curve: need nq >= 1");
    if (k < 1) return set_err(KNN_ERR_INVALID, "hit_curve: need k >= 1");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "hit_curve: k > INT32_MAX");
    if (limit < 1 || limit > k) return set_err(KNN_ERR_INVALID, "hit_curve: limit outside [1, k]");
    if (!is_correct || !totals || !mean_out) return set_err(KNN_ERR_INVALID, "hit_curve: null pointer");
    for (int64_t q = 0; q < nq; q++)
        if (totals[q] < 1) return set_err(KNN_ERR_INVALID, "hit_curve: a total below 1");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    // the scratch of terms stays within 256 MiB
    const int64_t slab = std::min(nq, std::min(eval_slab_rows(k), std::max<int64_t>(1, (int64_t)(256ull << 20) / (limit * 8))));
    const int lds_cols = (int)std::min<int64_t>(limit, HIT_LDS_COLS);
    HostCall call;
    EvalBufs &bufs = call.bufs;
    PhaseClock &clock = call.clock;
    std::vector<double> sums((size_t)limit);
    std::vector<int64_t> cols(column_correct_out ? (size_t)limit : 0);
    EvalCols tab(bufs, 1), w(bufs, slab);
    double *d_sums = tab.out(sums.data(), (size_t)limit * 8);
    unsigned long long *d_cols = (unsigned long long *)tab.out(column_correct_out ? cols.data() : nullptr, (size_t)limit * 8);
    const uint8_t *d_ic = w.in(is_correct, (size_t)k);
    const int64_t *d_tot = w.in(totals, 8);
    int64_t *d_rows = w.out(row_correct_out, 8);
    EVAL_ALLOC(d_terms, double *, (size_t)slab * limit * 8);
    EVAL_TRY(w.ready());
    HIP_TRY(hipFuncSetAttribute((const void *)hit_terms_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, HIT_LDS_COLS * 4));
    HIP_TRY(hipFuncSetAttribute((const void *)hit_fold_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 2 * HIT_FOLD_ROWS * HIT_FOLD_COLS * 8));
    HIP_TRY(hipMemset(d_sums, 0, (size_t)limit * 8)); // (all bits zero: +0.0)
    if (d_cols) HIP_TRY(hipMemset(d_cols, 0, (size_t)limit * 8));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(clock.next(BUCKETS_UP, call.s));
        EVAL_TRY(w.upload(r0, m));
        const HitParams p = {d_ic, d_tot, m, (int)k, (int)limit, lds_cols, d_terms, d_rows, d_cols};
        EVAL_TRY(clock.next(BUCKETS_KERNELS, call.s));
        hipLaunchKernelGGL(hit_terms_kernel, dim3((unsigned)std::min<int64_t>((m + 3) / 4, 1024)), dim3(256), d_cols ? (size_t)lds_cols * 4 : 0, 0, p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(hit_fold_kernel, dim3((unsigned)((limit + HIT_FOLD_COLS - 1) / HIT_FOLD_COLS)), dim3(256),
                           2 * HIT_FOLD_ROWS * HIT_FOLD_COLS * 8, 0, d_terms, m, limit, d_sums);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(clock.next(BUCKETS_DOWN, call.s));
        EVAL_TRY(w.download(r0, m));
    }
    EVAL_TRY(clock.next(BUCKETS_DOWN, call.s));
    EVAL_TRY(tab.download(0, 1));
    EVAL_TRY(clock.close(call.s));
    EVAL_TRY(call.finish("hit_curve", 0));
    float ms[BUCKETS_PHASES];
    EVAL_TRY(clock.read(ms, BUCKETS_PHASES));
    int64_t run = 0;
    for (int64_t j = 0; j < limit; j++) {
        mean_out[j] = sums[(size_t)j] / (double)nq;
        if (column_correct_out) column_correct_out[j] = run += cols[(size_t)j]; // the column sums of C: the prefix sum of the counts
    }
    memcpy(g_buckets_ms[1], ms, sizeof ms);
    return 0;
}

extern "C" int knn_eval_buckets_last_ms(float *counts_ms, float *curve_ms)
{
    if (!counts_ms || !curve_ms) return set_err(KNN_ERR_INVALID, "buckets_last_ms: null pointer");
    for (int i = 0; i < BUCKETS_PHASES; i++) {
        counts_ms[i] = g_buckets_ms[0][i];
        curve_ms[i] = g_buckets_ms[1][i];
    }
    return 0;
}
