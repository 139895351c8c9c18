// kde.inc -- one-dimensional Gaussian kernel density estimates: density.gaussian_kde, density.density_curves (included
// by knn355_lib.hip last).
//
// The reference draws DataFrame({...}).plot.density() over the projected columns and over raw embedding dimensions
// (pfam/reverse_evaluate.py:63-70, 113-118, 139-142); pandas turns every column into
// scipy.stats.gaussian_kde(column).evaluate(grid) on a 1000-point grid: n x 1000 double-precision exponentials per
// column.  The arithmetic contract is above knn_kde_stats in include/knn355.h; the launch shapes are plan_kde's (plan.h).
//
//   kde_stats_kernel        <T, PASS>: one thread per (group, column) walks the group's rows with float64 accumulators,
//                           pca_colsum_kernel's pattern; neighbouring threads are neighbouring columns of one row.
//                           PASS 0: the sum, the minimum and the maximum.  PASS 1: the sum of (x - mean)^2.
//   kde_stats_reduce_kernel <PASS>: one thread per column: the group sums in group order and the division.
//   kde_eval_kernel         <T>: one workgroup of 256 threads per (tile of 16 grid points, chunk of 16 384 rows, column).
//                           Lane j owns the contract's partial j of all 16 grid points: 16 float64 accumulators in
//                           registers.  It reads its (at most) 64 samples, rows j, j + 256, ... of the chunk, one ahead of
//                           the one it works on (neighbouring lanes read neighbouring rows); the 16 grid values and 1 / h
//                           are the same for the whole workgroup and sit in scalar registers.  Per sample the 16
//                           exponentials are 16 independent chains of float64 multiplies and adds (kde_kexp: no LDS, no
//                           hardware transcendental, whose results the ISA does not pin down), so the float64 pipe always
//                           has an instruction that waits for nothing.  A grid point past m repeats the last one and is
//                           not stored; a row past n is not visited.  Behind the loop the 256 partials of every grid
//                           point are combined once through LDS in the contract's pair order: thread (p, q) folds the
//                           partials 16 q .. 16 q + 15 of point p (strides 1, 2, 4, 8), thread (p, 0) the 16 results
//                           (strides 16 .. 128).  The chunk's sums go to part[column][chunk][m] with plain stores.
//   kde_reduce_kernel       one thread per (column, grid point): the chunk sums in chunk order, times norm.
//   No atomics, no fma: __dadd_rn / __dsub_rn / __dmul_rn, and the library is built with -ffp-contract=off.

static constexpr double KDE_LOG2E = 0x1.71547652b82fep+0;
static constexpr double KDE_LN2_HI = 0x1.62e42fee00000p-1; // the low 21 bits are zero: k * LN2_HI is exact for |k| < 2^11
static constexpr double KDE_LN2_LO = 0x1.a39ef35793c76p-33;
static constexpr double KDE_CUT = -745.0; // below it the term is exactly 0

// exp(t) for t <= 0 as the contract spells it: every step one IEEE operation
__device__ __forceinline__ double kde_kexp(double t)
{
    const double tc = fmax(t, KDE_CUT - 1.0); // (keeps k an int whatever t is; such a t takes the cut below)
    const double kd = rint(__dmul_rn(tc, KDE_LOG2E));
    const double r = __dsub_rn(__dsub_rn(tc, __dmul_rn(kd, KDE_LN2_HI)), __dmul_rn(kd, KDE_LN2_LO));
    // 1 / i!, each the double nearest to it (i! is exact up to 13!, the division rounds once)
    constexpr double c[14] = {1.0,
                              1.0,
                              1.0 / 2.0,
                              1.0 / 6.0,
                              1.0 / 24.0,
                              1.0 / 120.0,
                              1.0 / 720.0,
                              1.0 / 5040.0,
                              1.0 / 40320.0,
                              1.0 / 362880.0,
                              1.0 / 3628800.0,
                              1.0 / 39916800.0,
                              1.0 / 479001600.0,
                              1.0 / 6227020800.0};
    double p = c[13];
#pragma unroll
    for (int i = 12; i >= 0; i--) p = __dadd_rn(__dmul_rn(p, r), c[i]);
    const double e = ldexp(p, (int)kd); // one rounding where the result is subnormal (k < -1022)
    return t < KDE_CUT ? 0.0 : e;
}

template <typename T, int PASS>
__global__ __launch_bounds__(256) void kde_stats_kernel(const T *__restrict__ x, int64_t n, int ncols, int64_t stride, int64_t L, int groups,
                                                        const double *__restrict__ mean, double *__restrict__ gsum, double *__restrict__ gmin,
                                                        double *__restrict__ gmax)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)groups * ncols) return;
    const int c = (int)(t % ncols);
    const int64_t g = t / ncols, r0 = g * L, r1 = min(n, r0 + L);
    const T *p = x + (size_t)r0 * stride + c;
    const double mu = PASS ? mean[c] : 0.0;
    auto value = [&](double v) {
        if (!PASS) return v;
        const double d = __dsub_rn(v, mu);
        return __dmul_rn(d, d);
    };
    const double first = (double)*p;
    double s = value(first), mn = first, mx = first; // (a group has one row at least)
    int64_t r = r0 + 1;
    p += stride;
    for (; r + 8 <= r1; r += 8, p += (size_t)8 * stride) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = (double)p[(size_t)u * stride];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            s = __dadd_rn(s, value(v[u]));
            if (!PASS) {
                mn = fmin(mn, v[u]);
                mx = fmax(mx, v[u]);
            }
        }
    }
    for (; r < r1; r++, p += stride) {
        const double v = (double)*p;
        s = __dadd_rn(s, value(v));
        if (!PASS) {
            mn = fmin(mn, v);
            mx = fmax(mx, v);
        }
    }
    gsum[t] = s; // [group][column]
    if (!PASS) {
        gmin[t] = mn;
        gmax[t] = mx;
    }
}

// stats: [4][ncols] = minimum, maximum, mean, variance
template <int PASS>
__global__ __launch_bounds__(256) void kde_stats_reduce_kernel(const double *__restrict__ gsum, const double *__restrict__ gmin,
                                                               const double *__restrict__ gmax, int groups, int ncols, int64_t n,
                                                               double *__restrict__ stats)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    double s = gsum[c];
    for (int g = 1; g < groups; g++) s = __dadd_rn(s, gsum[(size_t)g * ncols + c]);
    if (PASS) {
        stats[(size_t)3 * ncols + c] = s / (double)(n - 1);
        return;
    }
    double mn = gmin[c], mx = gmax[c];
    for (int g = 1; g < groups; g++) {
        mn = fmin(mn, gmin[(size_t)g * ncols + c]);
        mx = fmax(mx, gmax[(size_t)g * ncols + c]);
    }
    stats[c] = mn;
    stats[(size_t)ncols + c] = mx;
    stats[(size_t)2 * ncols + c] = s / (double)n;
}

// the contract's tree over 16 neighbouring values: adjacent pairs, strides 1, 2, 4, 8
__device__ __forceinline__ double kde_tree16(double (&v)[16])
{
#pragma unroll
    for (int s = 1; s < 16; s <<= 1)
#pragma unroll
        for (int e = 0; e < 16; e += 2 * s) v[e] = __dadd_rn(v[e], v[e + s]);
    return v[0];
}

template <typename T>
__global__ __launch_bounds__(KDE_LANES) void kde_eval_kernel(const T *__restrict__ x, int64_t n, int64_t stride, const double *__restrict__ grid, int64_t m,
                                                             const double *__restrict__ inv_h, double *__restrict__ part)
{
    static_assert(KDE_TILE == 16 && KDE_LANES == 256, "the combine below is written for 16 points and 16 x 16 partials");
    __shared__ double s_p[KDE_TILE][KDE_LANES];
    __shared__ double s_q[KDE_TILE][16];
    const int tid = threadIdx.x, col = blockIdx.z;
    const int64_t p0 = (int64_t)blockIdx.x * KDE_TILE;
    const int64_t r0 = (int64_t)blockIdx.y * KDE_CHUNK, r1 = min(n, r0 + KDE_CHUNK);
    const double ih = inv_h[col];
    double g[KDE_TILE], acc[KDE_TILE];
#pragma unroll
    for (int p = 0; p < KDE_TILE; p++) {
        g[p] = grid[(size_t)col * m + min(p0 + p, m - 1)]; // a point past m repeats the last one and is not stored
        acc[p] = 0.0;
    }
    const T *px = x + col;
    int64_t i = r0 + tid;
    double xn = i < r1 ? (double)px[(size_t)i * stride] : 0.0;
    for (; i < r1; i += KDE_LANES) {
        const double xv = xn;
        if (i + KDE_LANES < r1) xn = (double)px[(size_t)(i + KDE_LANES) * stride];
#pragma unroll
        for (int p = 0; p < KDE_TILE; p++) {
            const double z = __dmul_rn(__dsub_rn(g[p], xv), ih);
            const double t = __dmul_rn(__dmul_rn(z, z), -0.5);
            acc[p] = __dadd_rn(acc[p], kde_kexp(t));
        }
    }
    // a lane without a row holds +0.0, which changes no sum of non-negative terms
#pragma unroll
    for (int p = 0; p < KDE_TILE; p++) s_p[p][tid] = acc[p];
    __syncthreads();
    const int p = tid >> 4, q = tid & 15;
    double v[16];
#pragma unroll
    for (int e = 0; e < 16; e++) v[e] = s_p[p][16 * q + e];
    s_q[p][q] = kde_tree16(v);
    __syncthreads();
    if (q != 0 || p0 + p >= m) return;
#pragma unroll
    for (int e = 0; e < 16; e++) v[e] = s_q[p][e];
    part[((size_t)col * gridDim.y + blockIdx.y) * m + p0 + p] = kde_tree16(v);
}

__global__ __launch_bounds__(256) void kde_reduce_kernel(const double *__restrict__ part, int64_t chunks, int64_t m, const double *__restrict__ norm,
                                                         double *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= m) return;
    const int col = blockIdx.y;
    const double *p = part + (size_t)col * chunks * m + j;
    double s = p[0];
    for (int64_t c = 1; c < chunks; c++) s = __dadd_rn(s, p[(size_t)c * m]);
    out[(size_t)col * m + j] = __dmul_rn(s, norm[col]);
}

// ---- host -------------------------------------------------------------------------------
// measurement (tools/bench_kde.py): HIP-event milliseconds of this thread's last successful calls
enum { KDE_STATS_UP, KDE_STATS_KERNELS, KDE_STATS_PHASES };
static thread_local float g_kde_stats_ms[KDE_STATS_PHASES] = {0, 0};
enum { KDE_EVAL_UP, KDE_EVAL_KERNEL, KDE_EVAL_REDUCE, KDE_EVAL_PHASES };
static thread_local float g_kde_eval_ms[KDE_EVAL_PHASES] = {0, 0, 0};

template <typename T>
static bool kde_all_finite(const T *x, int64_t n, int64_t ncols, int64_t stride)
{
    for (int64_t i = 0; i < n; i++)
        for (int64_t c = 0; c < ncols; c++)
            if (!std::isfinite(x[(size_t)i * stride + c])) return false;
    return true;
}

// what both entries refuse about the rows before anything is allocated
static int kde_check_rows(const char *who, const void *x, int32_t dtype, int64_t n, int32_t ncols, int64_t row_stride, int64_t m, KdePlan *pl)
{
    const std::string w = std::string(who) + ": ";
    if (dtype != 0 && dtype != 1) return set_err(KNN_ERR_INVALID, w + "dtype must be 0 (float32) or 1 (float64)");
    if (n < 2) return set_err(KNN_ERR_INVALID, w + "need n >= 2");
    if (ncols < 1 || ncols > KNN_KDE_MAX_COLS) return set_err(KNN_ERR_INVALID, w + "need 1 <= ncols <= KNN_KDE_MAX_COLS");
    if (row_stride < ncols) return set_err(KNN_ERR_INVALID, w + "row_stride is below ncols");
    if (m < 1) return set_err(KNN_ERR_INVALID, w + "need m >= 1");
    if (!plan_kde(n, ncols, m, pl)) return set_err(KNN_ERR_INVALID, w + "n or m is beyond what one launch covers");
    if (!x) return set_err(KNN_ERR_INVALID, w + "null pointer");
    if (!(dtype ? kde_all_finite((const double *)x, n, ncols, row_stride) : kde_all_finite((const float *)x, n, ncols, row_stride)))
        return set_err(KNN_ERR_INVALID, w + "the data hold a NaN or an infinity");
    return 0;
}

// the rows as they lie on the host, from the first used element to the last: (n - 1) * row_stride + ncols elements
static size_t kde_span_bytes(int dtype, int64_t n, int ncols, int64_t row_stride)
{
    return ((size_t)(n - 1) * (size_t)row_stride + (size_t)ncols) * (dtype ? 8 : 4);
}

static int kde_stats_enqueue(const void *x, int dtype, int64_t n, int ncols, int64_t stride, const KdePlan &pl, double *stats_host, EvalBufs &bufs,
                             hipStream_t s, PhaseClock &clock)
{
    const size_t gc = (size_t)pl.groups * ncols;
    EVAL_ALLOC(d_x, void *, kde_span_bytes(dtype, n, ncols, stride));
    EVAL_ALLOC(d_g, double *, 3 * gc * 8); // group sums, minima, maxima
    EVAL_ALLOC(d_stats, double *, (size_t)4 * ncols * 8);
    EVAL_TRY(clock.open(KDE_STATS_UP, s));
    HIP_TRY(hipMemcpyAsync(d_x, x, kde_span_bytes(dtype, n, ncols, stride), hipMemcpyHostToDevice, s));
    EVAL_TRY(clock.next(KDE_STATS_KERNELS, s));
    const dim3 gg((unsigned)((gc + 255) / 256)), gr((unsigned)((ncols + 255) / 256)), b(256);
    const double *d_mean = d_stats + (size_t)2 * ncols;
#define KDE_STATS_PASS(PASS)                                                                                                                             \
    do {                                                                                                                                                 \
        if (dtype) hipLaunchKernelGGL((kde_stats_kernel<double, PASS>), gg, b, 0, s, (const double *)d_x, n, ncols, stride, pl.group_rows, pl.groups,  \
                                      d_mean, d_g, d_g + gc, d_g + 2 * gc);                                                                              \
        else hipLaunchKernelGGL((kde_stats_kernel<float, PASS>), gg, b, 0, s, (const float *)d_x, n, ncols, stride, pl.group_rows, pl.groups, d_mean,   \
                                d_g, d_g + gc, d_g + 2 * gc);                                                                                            \
        HIP_TRY(hipGetLastError());                                                                                                                      \
        hipLaunchKernelGGL((kde_stats_reduce_kernel<PASS>), gr, b, 0, s, d_g, d_g + gc, d_g + 2 * gc, pl.groups, ncols, n, d_stats);                    \
        HIP_TRY(hipGetLastError());                                                                                                                      \
    } while (0)
    KDE_STATS_PASS(0);
    KDE_STATS_PASS(1);
#undef KDE_STATS_PASS
    EVAL_TRY(clock.close(s));
    HIP_TRY(hipMemcpyAsync(stats_host, d_stats, (size_t)4 * ncols * 8, hipMemcpyDeviceToHost, s));
    return 0;
}

extern "C" int knn_kde_stats(const void *x, int32_t dtype, int64_t n, int32_t ncols, int64_t row_stride, double *min_out, double *max_out, double *mean_out,
                             double *var_out)
{
    KdePlan pl;
    int rc = kde_check_rows("kde_stats", x, dtype, n, ncols, row_stride, 1, &pl);
    if (rc) return rc;
    if (!min_out || !max_out || !mean_out || !var_out) return set_err(KNN_ERR_INVALID, "kde_stats: null pointer");
    if ((rc = ensure_device(g_device))) return rc;
    std::vector<double> stats((size_t)4 * ncols); // the caller's arrays are written when the whole call has succeeded
    // the upload rides the copy pipeline's host-to-device stream when no host search holds it; the kernels follow it on
    // the same stream (the null stream otherwise)
    HostCall call;
    if ((rc = call.lease(g_device, true))) return rc;
    rc = kde_stats_enqueue(x, dtype, n, ncols, row_stride, pl, stats.data(), call.bufs, call.s, call.clock);
    if ((rc = call.finish("kde_stats", rc))) return rc;
    float ms[KDE_STATS_PHASES];
    EVAL_TRY(call.clock.read(ms, KDE_STATS_PHASES));
    for (int c = 0; c < ncols; c++) {
        min_out[c] = stats[c];
        max_out[c] = stats[(size_t)ncols + c];
        mean_out[c] = stats[(size_t)2 * ncols + c];
        var_out[c] = stats[(size_t)3 * ncols + c];
    }
    memcpy(g_kde_stats_ms, ms, sizeof ms);
    return 0;
}

static int kde_eval_enqueue(const void *x, int dtype, int64_t n, int ncols, int64_t stride, const double *grid, int64_t m, const double *inv_h,
                            const double *norm, const KdePlan &pl, double *out, EvalBufs &bufs, hipStream_t s, PhaseClock &clock)
{
    const size_t cm = (size_t)ncols * m;
    EVAL_ALLOC(d_x, void *, kde_span_bytes(dtype, n, ncols, stride));
    EVAL_ALLOC(d_grid, double *, cm * 8);
    EVAL_ALLOC(d_scale, double *, (size_t)2 * ncols * 8); // 1 / h, norm
    EVAL_ALLOC(d_part, double *, (size_t)pl.part_bytes);
    EVAL_ALLOC(d_out, double *, cm * 8);
    EVAL_TRY(clock.open(KDE_EVAL_UP, s));
    HIP_TRY(hipMemcpyAsync(d_x, x, kde_span_bytes(dtype, n, ncols, stride), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_grid, grid, cm * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_scale, inv_h, (size_t)ncols * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_scale + ncols, norm, (size_t)ncols * 8, hipMemcpyHostToDevice, s));
    EVAL_TRY(clock.next(KDE_EVAL_KERNEL, s));
    const dim3 ge((unsigned)pl.tiles, (unsigned)pl.chunks, (unsigned)ncols);
    if (dtype) hipLaunchKernelGGL((kde_eval_kernel<double>), ge, dim3(KDE_LANES), 0, s, (const double *)d_x, n, stride, d_grid, m, d_scale, d_part);
    else hipLaunchKernelGGL((kde_eval_kernel<float>), ge, dim3(KDE_LANES), 0, s, (const float *)d_x, n, stride, d_grid, m, d_scale, d_part);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(clock.next(KDE_EVAL_REDUCE, s));
    hipLaunchKernelGGL(kde_reduce_kernel, dim3((unsigned)((m + 255) / 256), (unsigned)ncols), dim3(256), 0, s, d_part, pl.chunks, m, d_scale + ncols, d_out);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(clock.close(s));
    HIP_TRY(hipMemcpyAsync(out, d_out, cm * 8, hipMemcpyDeviceToHost, s));
    return 0;
}

extern "C" int knn_kde_eval(const void *x, int32_t dtype, int64_t n, int32_t ncols, int64_t row_stride, const double *grid, int64_t m, const double *inv_h,
                            const double *norm, double *out)
{
    KdePlan pl;
    int rc = kde_check_rows("kde_eval", x, dtype, n, ncols, row_stride, m, &pl);
    if (rc) return rc;
    if (!grid || !inv_h || !norm || !out) return set_err(KNN_ERR_INVALID, "kde_eval: null pointer");
    for (int c = 0; c < ncols; c++)
        if (!std::isfinite(inv_h[c]) || !(inv_h[c] > 0.0) || !std::isfinite(norm[c]) || !(norm[c] > 0.0))
            return set_err(KNN_ERR_INVALID, "kde_eval: inv_h and norm must be positive and finite (a zero variance or a bad factor)");
    if (!kde_all_finite(grid, 1, (int64_t)ncols * m, 0)) return set_err(KNN_ERR_INVALID, "kde_eval: the grid holds a NaN or an infinity");
    if ((rc = ensure_device(g_device))) return rc;
    HostCall call;
    if ((rc = call.lease(g_device, true))) return rc;
    rc = kde_eval_enqueue(x, dtype, n, ncols, row_stride, grid, m, inv_h, norm, pl, out, call.bufs, call.s, call.clock);
    if ((rc = call.finish("kde_eval", rc))) return rc;
    float ms[KDE_EVAL_PHASES];
    EVAL_TRY(call.clock.read(ms, KDE_EVAL_PHASES));
    memcpy(g_kde_eval_ms, ms, sizeof ms);
    return 0;
}

extern "C" int knn_kde_last_ms(float *stats_ms, float *eval_ms)
{
    if (!stats_ms || !eval_ms) return set_err(KNN_ERR_INVALID, "kde_last_ms: null pointer");
    for (int i = 0; i < KDE_STATS_PHASES; i++) stats_ms[i] = g_kde_stats_ms[i];
    for (int i = 0; i < KDE_EVAL_PHASES; i++) eval_ms[i] = g_kde_eval_ms[i];
    return 0;
}
