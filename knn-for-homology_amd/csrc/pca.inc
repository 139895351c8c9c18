// pca.inc -- the moments and the projection behind decomposition.PCA (included by knn355_lib.hip behind eval.inc).
//
// The reference runs sklearn.decomposition.PCA(n_components=2) over the concatenated forward and scrambled embedding
// matrices (pfam/reverse_evaluate.py:34-44, 100-108).  Its array-sized work is a d x d covariance over n rows and the
// projection of the rows onto a few components; the eigen-solve of the d x d matrix stays on the host
// (decomposition.py).  The arithmetic contract is above knn_pca_moments in include/knn355.h.
//
//   pca_colsum_kernel      one thread per (group, column) walks the group's rows with a float64 accumulator; the 256
//                          threads of a workgroup read 1 KiB of consecutive columns of one row at a time.
//   pca_mean_kernel        one thread per column: the group sums in group order, the division, the rounding to float32.
//   pca_cov_kernel         one workgroup of four waves per (pair of 128-column tiles TI <= TJ, group).  Per 32 rows both
//                          panels [32 rows][128 columns] are staged in LDS, the mean subtracted on the way in, rows past
//                          the group's end and columns past d as zeros; a diagonal pair stages one panel.  A K step is two
//                          consecutive rows: lane l of v_mfma_f32_32x32x2_f32 holds xc[r0 + l / 32][i0 + l % 32] as A and
//                          xc[r0 + l / 32][j0 + l % 32] as B, both one conflict-free ds_read_b32 of a panel row, so the
//                          instruction's two fmas are rows r0 and r0 + 1 and K steps in ascending r0 walk the rows in
//                          the contract's order.  Wave (wm, wn) owns the 64 x 64 quarter of the tile pair: four 32 x 32
//                          accumulators, two A and two B reads per four MFMAs.  On a diagonal pair the wave below the
//                          diagonal has nothing to compute.  The next panel's global loads are in flight in registers
//                          while the MFMAs of this one run.  The partial sums go to part[group][d][d] with plain
//                          stores (every accumulator register is two 128-byte row segments), upper tiles only.
//   pca_cov_reduce_kernel  one thread per (i <= j): the float64 sum over the groups in group order, the division by
//                          n - 1, and both mirrored stores.
//   pca_project_kernel     one workgroup per 64 rows, refine.inc's pattern: 32-float slabs of the centred rows in LDS at
//                          pitch 36 (conflict-free ds_read_b128, refine.inc's note), the components' slab beside them;
//                          lane = row, wave w = components w, w + 4, ..., so a component read is a broadcast.  Every
//                          (row, component) is one lane's chain in the order of the library's dot.
//   No float atomics anywhere: every sum has one writer and a fixed order.

static constexpr int PCA_TC = 128; // columns per tile side of pca_cov_kernel
static constexpr int PCA_PR = 32;  // rows per staged panel
// rows per group: a function of n alone (the contract's rule 1)
static int64_t pca_group_rows(int64_t n) { return 4096 * ((n + 4096 * 256 - 1) / (4096 * 256)); }

__global__ __launch_bounds__(256) void pca_colsum_kernel(const float *__restrict__ x, int64_t n, int d, int64_t L, double *__restrict__ gsum)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    const int64_t r0 = (int64_t)blockIdx.y * L, r1 = min(n, r0 + L);
    const float *p = x + (size_t)r0 * d + j;
    double s = (double)*p; // (a group has one row at least)
    int64_t r = r0 + 1;
    p += d;
    for (; r + 8 <= r1; r += 8, p += (size_t)8 * d) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = p[(size_t)u * d];
#pragma unroll
        for (int u = 0; u < 8; u++) s += (double)v[u];
    }
    for (; r < r1; r++, p += d) s += (double)*p;
    gsum[(size_t)blockIdx.y * d + j] = s;
}

__global__ __launch_bounds__(256) void pca_mean_kernel(const double *__restrict__ gsum, int groups, int d, int64_t n, float *__restrict__ mean)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= d) return;
    double s = gsum[j];
    for (int g = 1; g < groups; g++) s += gsum[(size_t)g * d + j];
    mean[j] = (float)(s / (double)n);
}

__global__ __launch_bounds__(256) void pca_cov_kernel(const float *__restrict__ x, int64_t n, int d, int64_t L, const float *__restrict__ mean,
                                                      float *__restrict__ part)
{
    const int TI = blockIdx.x, TJ = blockIdx.y;
    if (TI > TJ) return;
    const bool diag = TI == TJ;
    __shared__ __attribute__((aligned(16))) float s_a[PCA_PR][PCA_TC];
    __shared__ __attribute__((aligned(16))) float s_b[PCA_PR][PCA_TC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int64_t r_begin = (int64_t)blockIdx.z * L, r_end = min(n, r_begin + L);
    // staging: this thread moves the 16-byte piece c4 of the panel rows pr, pr + 8, pr + 16, pr + 24 of each side
    const int c4 = tid & 31, pr = tid >> 5;
    const int ca = TI * PCA_TC + c4 * 4, cb = TJ * PCA_TC + c4 * 4;
    const bool oka = ca < d, okb = !diag && cb < d; // (d is a multiple of 4: a piece is inside or outside as a whole)
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    const f32x4 ma = oka ? *(const f32x4 *)(mean + ca) : zero4, mb = okb ? *(const f32x4 *)(mean + cb) : zero4;
    f32x4 va[4], vb[4];
    auto fetch = [&](int64_t r0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int64_t r = r0 + pr + 8 * i;
            const bool in = r < r_end;
            va[i] = oka && in ? *(const f32x4 *)(x + (size_t)r * d + ca) : zero4;
            vb[i] = okb && in ? *(const f32x4 *)(x + (size_t)r * d + cb) : zero4;
        }
    };
    // centred on the way in; a row past the group's end or a column past d is 0, not 0 - mean
    auto stage = [&](int64_t r0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const bool in = r0 + pr + 8 * i < r_end;
            *(f32x4 *)&s_a[pr + 8 * i][c4 * 4] = oka && in ? va[i] - ma : zero4;
            if (!diag) *(f32x4 *)&s_b[pr + 8 * i][c4 * 4] = okb && in ? vb[i] - mb : zero4;
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
    const bool active = !diag || wm <= wn; // (the wave's 64 x 64 quarter touches the upper triangle)
    fetch(r_begin);
    for (int64_t r0 = r_begin; r0 < r_end; r0 += PCA_PR) {
        stage(r0);
        __syncthreads();
        if (r0 + PCA_PR < r_end) fetch(r0 + PCA_PR);
        // a K step is two rows; a step whose two rows are both past the end is skipped, a lone last row pairs with a zero row
        const int ksteps = ((int)min((int64_t)PCA_PR, r_end - r0) + 1) >> 1;
        if (active) {
            for (int k = 0; k < ksteps; k++) {
                const float *ra = s_a[2 * k + lh];
                const float *rb = diag ? ra : s_b[2 * k + lh];
                const float a0 = ra[wm * 64 + li], a1 = ra[wm * 64 + 32 + li];
                const float b0 = rb[wn * 64 + li], b1 = rb[wn * 64 + 32 + li];
                acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
                acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
                acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
                acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
            }
        }
        __syncthreads();
    }
    if (!active) return;
    float *out = part + (size_t)blockIdx.z * d * d;
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int j = TJ * PCA_TC + wn * 64 + b * 32 + li;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int i = TI * PCA_TC + wm * 64 + a * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
                if (i < d && j < d) out[(size_t)i * d + j] = acc[a][b][r];
            }
        }
}

__global__ __launch_bounds__(256) void pca_cov_reduce_kernel(const float *__restrict__ part, int groups, int d, int64_t n, double *__restrict__ cov)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= d || i > j) return;
    const size_t o = (size_t)i * d + j, dd = (size_t)d * d;
    double s = (double)part[o];
    for (int g = 1; g < groups; g++) s += (double)part[(size_t)g * dd + o];
    const double c = s / (double)(n - 1);
    cov[o] = c;
    cov[(size_t)j * d + i] = c;
}

static constexpr int PJ_ROWS = 64, PJ_KS = 32, PJ_PITCH = 36; // rows per workgroup, floats per slab, LDS row pitch in floats

__global__ __launch_bounds__(256) void pca_project_kernel(const float *__restrict__ x, int64_t m, int d, const float *__restrict__ mean,
                                                          const float *__restrict__ comp, int nc, float *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) float s_x[PJ_ROWS * PJ_PITCH];
    __shared__ __attribute__((aligned(16))) float s_c[KNN_PCA_MAX_COMPONENTS * PJ_KS];
    const int tid = threadIdx.x, row = tid & 63, cg = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * PJ_ROWS;
    const int piece = tid & 7, fr = tid >> 3; // fetch: the 16-byte piece of the slab's rows fr and fr + 32
    const f32x4 zero4 = {0.0f, 0.0f, 0.0f, 0.0f};
    float acc[KNN_PCA_MAX_COMPONENTS / 4];
#pragma unroll
    for (int u = 0; u < KNN_PCA_MAX_COMPONENTS / 4; u++) acc[u] = 0.0f;
    for (int k0 = 0; k0 < d; k0 += PJ_KS) {
        const int kc = k0 + piece * 4;
        const bool kok = kc < d;
        const f32x4 mu = kok ? *(const f32x4 *)(mean + kc) : zero4;
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int64_t r = r0 + fr + 32 * i;
            *(f32x4 *)&s_x[(fr + 32 * i) * PJ_PITCH + piece * 4] = kok && r < m ? *(const f32x4 *)(x + (size_t)r * d + kc) - mu : zero4;
        }
        if (tid < nc * 8) *(f32x4 *)&s_c[fr * PJ_KS + piece * 4] = kok ? *(const f32x4 *)(comp + (size_t)fr * d + kc) : zero4;
        __syncthreads();
        // the chain's blocks of 8: the last one of the row is zero padded (fmaf(0, 0, acc)), none follows it
        const int kmax = min(PJ_KS, (d - k0 + 7) & ~7);
        const float *y = s_x + row * PJ_PITCH;
        for (int kk = 0; kk < kmax; kk += 8) {
            const f32x4 y0 = *(const f32x4 *)(y + kk), y1 = *(const f32x4 *)(y + kk + 4);
#pragma unroll
            for (int u = 0; u < KNN_PCA_MAX_COMPONENTS / 4; u++) {
                const int c = cg + 4 * u;
                if (c < nc) { // (uniform in the wave)
                    const f32x4 q0 = *(const f32x4 *)(s_c + c * PJ_KS + kk), q1 = *(const f32x4 *)(s_c + c * PJ_KS + kk + 4);
#pragma unroll
                    for (int e = 0; e < 4; e++) {
                        acc[u] = __builtin_fmaf(y0[e], q0[e], acc[u]);
                        acc[u] = __builtin_fmaf(y1[e], q1[e], acc[u]);
                    }
                }
            }
        }
        __syncthreads();
    }
    if (r0 + row >= m) return;
#pragma unroll
    for (int u = 0; u < KNN_PCA_MAX_COMPONENTS / 4; u++) {
        const int c = cg + 4 * u;
        if (c < nc) out[(size_t)(r0 + row) * nc + c] = acc[u];
    }
}

// ---- host -------------------------------------------------------------------------------
// measurement (tools/bench_pca.py): HIP-event milliseconds of this thread's last successful calls
enum { PCA_UP, PCA_MEAN, PCA_COV, PCA_REDUCE, PCA_MOMENT_PHASES }; // upload, column sums + mean, covariance kernel, reduce
static thread_local float g_pca_moments_ms[PCA_MOMENT_PHASES] = {0, 0, 0, 0};
enum { PCA_PROJECT }; // the one phase of knn_pca_project: its kernel, summed over the slabs
static thread_local float g_pca_project_ms = 0;

static int pca_check_shape(const char *who, int64_t n, int64_t n_min, int32_t d)
{
    if (n < n_min) return set_err(KNN_ERR_INVALID, std::string(who) + ": need n >= " + std::to_string(n_min));
    if (d < 4 || d > KNN_PCA_MAX_D || d % 4) return set_err(KNN_ERR_INVALID, std::string(who) + ": need d a multiple of 4 in [4, KNN_PCA_MAX_D]");
    return 0;
}

// everything of knn_pca_moments that runs on stream s, enqueued; the caller waits for s whatever this returns
static int pca_moments_enqueue(const float *x, int64_t n, int d, float *mean, double *cov, EvalBufs &bufs, hipStream_t s, PhaseClock &clock)
{
    const int64_t L = pca_group_rows(n);
    const int groups = (int)((n + L - 1) / L);
    const size_t dd = (size_t)d * d;
    EVAL_ALLOC(d_x, float *, (size_t)n * d * 4);
    EVAL_ALLOC(d_gsum, double *, (size_t)groups * d * 8);
    EVAL_ALLOC(d_mean, float *, (size_t)d * 4);
    EVAL_ALLOC(d_part, float *, (size_t)groups * dd * 4);
    EVAL_ALLOC(d_cov, double *, dd * 8);
    EVAL_TRY(clock.open(PCA_UP, s));
    HIP_TRY(hipMemcpyAsync(d_x, x, (size_t)n * d * 4, hipMemcpyHostToDevice, s));
    EVAL_TRY(clock.next(PCA_MEAN, s));
    const unsigned cblocks = (unsigned)((d + 255) / 256), tiles = (unsigned)((d + PCA_TC - 1) / PCA_TC);
    hipLaunchKernelGGL(pca_colsum_kernel, dim3(cblocks, (unsigned)groups), dim3(256), 0, s, d_x, n, d, L, d_gsum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pca_mean_kernel, dim3(cblocks), dim3(256), 0, s, d_gsum, groups, d, n, d_mean);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(clock.next(PCA_COV, s));
    hipLaunchKernelGGL(pca_cov_kernel, dim3(tiles, tiles, (unsigned)groups), dim3(256), 0, s, d_x, n, d, L, d_mean, d_part);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(clock.next(PCA_REDUCE, s));
    hipLaunchKernelGGL(pca_cov_reduce_kernel, dim3(cblocks, (unsigned)d), dim3(256), 0, s, d_part, groups, d, n, d_cov);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(clock.close(s));
    HIP_TRY(hipMemcpyAsync(mean, d_mean, (size_t)d * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(cov, d_cov, dd * 8, hipMemcpyDeviceToHost, s));
    return 0;
}

extern "C" int knn_pca_moments(const float *x, int64_t n, int32_t d, float *mean, double *cov)
{
    int rc = pca_check_shape("pca_moments", n, 2, d);
    if (rc) return rc;
    if (!x || !mean || !cov) return set_err(KNN_ERR_INVALID, "pca_moments: null pointer");
    if ((rc = ensure_device(g_device))) return rc;
    // the upload rides the copy pipeline's host-to-device stream when no host search holds it; the kernels follow it on
    // the same stream (the null stream otherwise)
    HostCall call;
    if ((rc = call.lease(g_device, true))) return rc;
    rc = pca_moments_enqueue(x, n, d, mean, cov, call.bufs, call.s, call.clock);
    if ((rc = call.finish("pca_moments", rc))) return rc;
    float ms[PCA_MOMENT_PHASES];
    EVAL_TRY(call.clock.read(ms, PCA_MOMENT_PHASES));
    memcpy(g_pca_moments_ms, ms, sizeof ms);
    return 0;
}

extern "C" int knn_pca_project(const float *x, int64_t n, int32_t d, const float *mean, const float *components, int32_t nc, float *out)
{
    int rc = pca_check_shape("pca_project", n, 0, d);
    if (rc) return rc;
    if (nc < 1 || nc > KNN_PCA_MAX_COMPONENTS || nc > d) return set_err(KNN_ERR_INVALID, "pca_project: need 1 <= nc <= min(d, KNN_PCA_MAX_COMPONENTS)");
    if (n == 0) return 0;
    if (!x || !mean || !components || !out) return set_err(KNN_ERR_INVALID, "pca_project: null pointer");
    if ((rc = ensure_device(g_device))) return rc;
    EvalBufs bufs;
    // a row of d floats is d / 2 words of 8 bytes: the 256 MiB rule of the evaluation entries, in their unit
    const int64_t slab = std::min(n, eval_slab_rows(d / 2));
    EvalCols tab(bufs, 1), w(bufs, slab);
    const float *d_mean = tab.in(mean, (size_t)d * 4);
    const float *d_comp = tab.in(components, (size_t)nc * d * 4);
    const float *d_x = w.in(x, (size_t)d * 4);
    float *d_out = w.out(out, (size_t)nc * 4);
    EVAL_TRY(w.ready());
    EVAL_TRY(tab.upload(0, 1));
    PhaseClock clock;
    for (int64_t r0 = 0; r0 < n; r0 += slab) {
        const int64_t m = std::min(slab, n - r0);
        EVAL_TRY(w.upload(r0, m));
        EVAL_TRY(clock.open(PCA_PROJECT, nullptr));
        hipLaunchKernelGGL(pca_project_kernel, dim3((unsigned)((m + PJ_ROWS - 1) / PJ_ROWS)), dim3(256), 0, 0, d_x, m, (int)d, d_mean, d_comp, (int)nc, d_out);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(clock.close(nullptr));
        EVAL_TRY(w.download(r0, m));
    }
    float ms;
    EVAL_TRY(clock.read(&ms, 1));
    g_pca_project_ms = ms;
    return 0;
}

extern "C" int knn_pca_last_ms(float *moments_ms, float *project_ms)
{
    if (!moments_ms || !project_ms) return set_err(KNN_ERR_INVALID, "pca_last_ms: null pointer");
    for (int i = 0; i < 4; i++) moments_ms[i] = g_pca_moments_ms[i];
    *project_ms = g_pca_project_ms;
    return 0;
}
