// windows.inc -- statistics of boolean columns, and of the key itself, over contiguous ranges of the ranked order
// (included by knn355_lib.hip behind rank.inc).
//
// The reference draws three families of curves from arrays "put into the order of a key": rolling means over a window
// of W ranks (seqvec_search/utils.py:103 rolling_mean = numpy.convolve(data, ones(W) / W, "valid"), called at
// pfam/pfam.py:247-253, cath/cath.py:799-813 and 913-919), mean and standard error over equal-count slices of the order
// (hist_evenly, cath/cath.py:863-875, pfam/pfam.py:282-297) and over fixed key edges (cath/cath.py:831-857).  The order
// is rank.inc's (rank_alloc, rank_sort); this file is everything behind the sort.  The contract is above
// knn_eval_windows in include/knn355.h; the sizes, the staging run and the grids are plan_windows' (plan.h).
//   window_gather_kernel   one coalesced pass over the sorted payloads: rank r's position p is read from the payload, the M
//                          value bytes at p become one uint32 mask (bit c = column c), and the key at p is stored as
//                          float64 in rank order
//   rank.inc's scan        per column c the inclusive running count C_c(r) of bit c of the masks (the reduce / top /
//                          apply kernels with their bit selector): M scans
//   window_means_kernel    (C_c(i + W - 1) - C_c(i - 1)) / W, one float64 division of two exact integers, [M][N - W + 1]
//   window_chain_kernel    the key's two chains.  The order is cut into blocks of W ranks; per block P[r] is the sum from
//                          the block's first rank through r, added in rank order, and S[r] the sum from r through the
//                          block's last rank, added from the block's end backwards.  A workgroup owns a group of
//                          blocks_per_run whole blocks (W <= run) or one block (W > run) and walks it in steps: all 256
//                          threads stage one run of the ranked keys per direction into LDS with 16-byte loads (the
//                          forward run from the group's front, the backward run from its end: window_piece, plan.h),
//                          then one lane per (block, direction) walks its chain through the staged run, writing each
//                          running sum over the element it has just read, and all threads store the run's sums
//                          coalesced.  A chain that spans several runs keeps its sum in the lane's register.  A chain
//                          starts with its first element, not with 0 + element: numpy.cumsum does, and -0.0 shows it.
//                          The chains are serial by contract, so this kernel is bound by the latency of one dependent
//                          float64 add per element and lane, not by bandwidth.
//   window_combine_kernel  output i = P[i + W - 1] / W when i % W == 0, else (S[i] + P[i + W - 1]) / W
//   window_ranges_kernel   one thread per bin: its ranks [start, stop) -- given, or, for edges, the lower bounds of the
//                          edges' images in the sorted keys (the last bin stops at the first NaN) -- C_c at the two ends,
//                          and the keys at ranks start and stop, bits untouched
// No workgroup waits on another one; there is no atomic; every store is a plain vector store.

template <typename K>
__global__ __launch_bounds__(256) void window_gather_kernel(RankSrc<K> src, const uint32_t *__restrict__ pay, uint32_t n, const uint8_t *__restrict__ values,
                                                            int m, uint32_t *__restrict__ mask, double *__restrict__ keyd)
{
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (uint64_t)gridDim.x * 256) {
        const uint32_t p = pay[r] >> 1;
        if (mask) {
            uint32_t w = 0;
            for (int c = 0; c < m; c++) w |= (values[(size_t)c * n + p] ? 1u : 0u) << c;
            mask[r] = w;
        }
        if (keyd) keyd[r] = (double)src.scores[rank_cell(src, p)];
    }
}

__global__ __launch_bounds__(256) void window_means_kernel(const uint32_t *__restrict__ cum /* [m][n] */, uint32_t n, uint32_t window, uint32_t nout,
                                                           double *__restrict__ out /* [m][nout] */)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nout) return;
    const uint32_t *c = cum + (size_t)blockIdx.y * n;
    const uint32_t hi = c[i + window - 1], lo = i ? c[i - 1] : 0u;
    out[(size_t)blockIdx.y * nout + i] = (double)(hi - lo) / (double)window;
}

__device__ __forceinline__ int window_lds(int64_t e) { return (int)(e + (e >> WINDOW_PAD_SHIFT)); }

__global__ __launch_bounds__(256) void window_chain_kernel(const double *__restrict__ keyd, int64_t n, int64_t window, int64_t run, int64_t group,
                                                           int blocks_per_run, double *__restrict__ P, double *__restrict__ S)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *s_dir[2];
    s_dir[0] = (double *)smem;                              // the forward run
    s_dir[1] = s_dir[0] + (run + (run >> WINDOW_PAD_SHIFT)); // the backward run
    const int tid = threadIdx.x;
    const int64_t g0 = (int64_t)blockIdx.x * group, len = std::min<int64_t>(group, n - g0);
    const int64_t steps = (len + run - 1) / run;
    // thread = chain: block tid >> 1 of the group, direction tid & 1
    const int back = tid & 1;
    const int64_t bs = g0 + (int64_t)(tid >> 1) * window, be = std::min<int64_t>(bs + window, g0 + len);
    const bool chain = (tid >> 1) < blocks_per_run && bs < g0 + len;
    double sum = 0.0;
    bool started = false;
    for (int64_t step = 0; step < steps; step++) {
        WindowPiece pc[2];
        pc[0] = window_piece(g0, len, run, step, 0);
        pc[1] = window_piece(g0, len, run, step, 1);
#pragma unroll
        for (int d = 0; d < 2; d++) { // stage: pairs of float64 from an even rank on (keyd holds a whole pair past n)
            const int64_t e0 = pc[d].lo & ~(int64_t)1;
            for (int64_t e = e0 + 2 * tid; e < pc[d].hi; e += 512) {
                const double2 v = *(const double2 *)(keyd + e);
                if (e >= pc[d].lo) s_dir[d][window_lds(e - pc[d].lo)] = v.x;
                if (e + 1 < pc[d].hi) s_dir[d][window_lds(e + 1 - pc[d].lo)] = v.y;
            }
        }
        __syncthreads();
        if (chain) {
            const WindowPiece q = back ? pc[1] : pc[0]; // (selects, not indexing by lane: the arrays stay in registers)
            const int64_t a = std::max<int64_t>(bs, q.lo), b = std::min<int64_t>(be, q.hi);
            double *s = back ? s_dir[1] : s_dir[0];
            if (!back) {
                for (int64_t e = a; e < b; e++) {
                    const int j = window_lds(e - q.lo);
                    sum = started ? sum + s[j] : s[j];
                    started = true;
                    s[j] = sum;
                }
            } else {
                for (int64_t e = b - 1; e >= a; e--) {
                    const int j = window_lds(e - q.lo);
                    sum = started ? sum + s[j] : s[j];
                    started = true;
                    s[j] = sum;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int d = 0; d < 2; d++) {
            double *out = d ? S : P;
            for (int64_t e = pc[d].lo + tid; e < pc[d].hi; e += 256) out[e] = s_dir[d][window_lds(e - pc[d].lo)];
        }
        __syncthreads(); // the sums are out: the runs may be overwritten
    }
}

__global__ __launch_bounds__(256) void window_combine_kernel(const double *__restrict__ P, const double *__restrict__ S, int64_t window, int64_t nout,
                                                             double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nout) return;
    const double p = P[i + window - 1];
    out[i] = (i % window == 0 ? p : S[i] + p) / (double)window;
}

template <typename K> struct WindowBins {
    int64_t *start, *stop, *counts;                // [nb], [nb], [m][nb]
    typename RankFloat<K>::F *key_lo, *key_hi;     // [nb]
    const typename RankFloat<K>::F *edges;         // [nb], or null: start and stop are given
};

template <typename K>
__global__ __launch_bounds__(256) void window_ranges_kernel(RankSrc<K> src, const K *__restrict__ keys, const uint32_t *__restrict__ pay,
                                                            const uint32_t *__restrict__ cum, int64_t n, int m, int64_t nb, WindowBins<K> b)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nb) return;
    int64_t start, stop;
    if (b.edges) {
        const K lo = rank_image<K>(b.edges[j], 0), hi = j + 1 < nb ? rank_image<K>(b.edges[j + 1], 0) : ~(K)0; // (all ones: the first NaN)
        start = lower_bound_dev((int64_t)0, n, [&](int64_t i) { return keys[i] < lo; });
        stop = lower_bound_dev(start, n, [&](int64_t i) { return keys[i] < hi; });
        b.start[j] = start;
        b.stop[j] = stop;
    } else {
        start = b.start[j];
        stop = b.stop[j];
    }
    for (int c = 0; c < m; c++) {
        const uint32_t *cc = cum + (size_t)c * n;
        const uint32_t hi = stop > 0 ? cc[stop - 1] : 0u, lo = start > 0 ? cc[start - 1] : 0u;
        b.counts[(size_t)c * nb + j] = stop > start ? (int64_t)(hi - lo) : 0;
    }
    b.key_lo[j] = src.scores[rank_cell(src, pay[std::min<int64_t>(start, n - 1)] >> 1)];
    b.key_hi[j] = src.scores[rank_cell(src, pay[std::min<int64_t>(stop, n - 1)] >> 1)];
}

// ---- host -------------------------------------------------------------------------------
// measurement (tools/bench_windows.py): how this thread's last successful knn_eval_windows ran
// host clock: allocations; HIP events (the clock's phases): upload, sort, gather and scans, chains, means, bins, downloads
enum { WIN_ALLOC, WIN_UP, WIN_SORT, WIN_GATHER, WIN_CHAINS, WIN_MEANS, WIN_BINS, WIN_DOWN, WIN_PHASES };
static thread_local struct {
    int64_t run, blocks_per_run, runs_per_block;
    float ms[WIN_PHASES];
} g_windows_info = {0, 0, 0, {0, 0, 0, 0, 0, 0, 0, 0}};

template <typename K>
static int windows_run(const void *keys, const uint8_t *values, int desc, const WindowsPlan &pl, double *key_means_out, double *value_means_out,
                       int64_t *order_out, const int64_t *starts, const int64_t *stops, const void *edges, int64_t *start_out, int64_t *stop_out,
                       int64_t *counts_out, void *key_lo_out, void *key_hi_out)
{
    typedef typename RankFloat<K>::F F;
    const uint32_t n = (uint32_t)pl.n;
    const int m = pl.m;
    const int64_t nb = pl.nbins, W = pl.window, nout = pl.nout;
    const auto t_alloc = std::chrono::steady_clock::now();
    EvalBufs bufs;
    PhaseClock clock;
    RankSorted<K> rs;
    EVAL_TRY(rank_alloc<K>(bufs, pl.rank, rs));
    auto opt = [&](size_t bytes, bool &ok) -> void * {
        if (!bytes) return nullptr;
        void *p = bufs.get(bytes);
        if (!p) ok = false;
        return p;
    };
    bool ok = true;
    int64_t *d_wide = (int64_t *)opt(pl.rank.wide_bytes, ok);
    uint8_t *d_values = (uint8_t *)opt(pl.values_bytes, ok);
    uint32_t *d_mask = (uint32_t *)opt(pl.mask_bytes, ok);
    uint32_t *d_cum = (uint32_t *)opt(pl.cum_bytes, ok);
    uint32_t *d_wpartial = (uint32_t *)opt(pl.wpartial_bytes, ok);
    double *d_keyd = (double *)opt(pl.keyd_bytes, ok);
    double *d_P = (double *)opt(pl.chain_bytes, ok);
    double *d_S = (double *)opt(pl.chain_bytes, ok);
    double *d_means = (double *)opt(pl.means_bytes, ok);
    char *d_bins = (char *)opt(pl.bins_bytes, ok);
    if (!ok) return set_err(KNN_ERR_HIP, "eval: out of device memory");
    size_t allocated = 0;
    for (const auto &b : bufs.dev) allocated += b.second;
    if (allocated != pl.resident_bytes) return set_err(KNN_ERR_INVALID, "windows: the buffers are not the plan's");
    const auto t_up = std::chrono::steady_clock::now();
    EVAL_TRY(clock.open(WIN_UP, nullptr)); // the columns and the bins' vectors (the keys: rank_sort's interval of the phase)
    if (m) HIP_TRY(hipMemcpy(d_values, values, pl.values_bytes, hipMemcpyHostToDevice));
    WindowBins<K> bins = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    if (nb) {
        bins.start = (int64_t *)d_bins;
        bins.stop = bins.start + nb;
        bins.counts = bins.stop + nb;
        bins.key_lo = (F *)(bins.counts + (size_t)m * nb);
        bins.key_hi = bins.key_lo + nb;
        F *d_edges = bins.key_hi + nb;
        if (edges) {
            HIP_TRY(hipMemcpy(d_edges, edges, (size_t)nb * sizeof(F), hipMemcpyHostToDevice));
            bins.edges = d_edges;
        } else {
            HIP_TRY(hipMemcpy(bins.start, starts, (size_t)nb * 8, hipMemcpyHostToDevice));
            HIP_TRY(hipMemcpy(bins.stop, stops, (size_t)nb * 8, hipMemcpyHostToDevice));
        }
    }
    EVAL_TRY(rank_sort<K>(keys, pl.n, 1, 1, nullptr, desc, pl.rank, clock, WIN_UP, WIN_SORT, WIN_GATHER, rs));
    // ---- masks, keys in rank order, C_c(r)
    if (d_mask || d_keyd) {
        hipLaunchKernelGGL(window_gather_kernel<K>, dim3((unsigned)pl.gather_grid), dim3(256), 0, 0, rs.src, rs.pay, n, (const uint8_t *)d_values, m, d_mask,
                           d_keyd);
        HIP_TRY(hipGetLastError());
    }
    for (int c = 0; c < m; c++) EVAL_TRY(rank_scan<true>(d_mask, (uint64_t)n, d_wpartial, d_cum + (size_t)c * n, c));
    // ---- the key's chains (a phase that does not run has no interval: it reads exactly 0)
    if (W) {
        EVAL_TRY(clock.next(WIN_CHAINS, nullptr));
        hipLaunchKernelGGL(window_chain_kernel, dim3((unsigned)pl.chain_grid), dim3(256), pl.chain_lds, 0, (const double *)d_keyd, pl.n, W, pl.run, pl.group,
                           (int)pl.blocks_per_run, d_P, d_S);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(window_combine_kernel, dim3((unsigned)pl.combine_grid), dim3(256), 0, 0, (const double *)d_P, (const double *)d_S, W, nout,
                           d_means + (size_t)m * nout);
        HIP_TRY(hipGetLastError());
    }
    if (W && m) {
        EVAL_TRY(clock.next(WIN_MEANS, nullptr));
        hipLaunchKernelGGL(window_means_kernel, dim3((unsigned)pl.means_grid, (unsigned)m), dim3(256), 0, 0, (const uint32_t *)d_cum, n, (uint32_t)W,
                           (uint32_t)nout, d_means);
        HIP_TRY(hipGetLastError());
    }
    if (nb) {
        EVAL_TRY(clock.next(WIN_BINS, nullptr));
        hipLaunchKernelGGL(window_ranges_kernel<K>, dim3((unsigned)pl.ranges_grid), dim3(256), 0, 0, rs.src, rs.keys, rs.pay, (const uint32_t *)d_cum, pl.n, m, nb,
                           bins);
        HIP_TRY(hipGetLastError());
    }
    // ---- downloads
    EVAL_TRY(clock.next(WIN_DOWN, nullptr));
    if (order_out) {
        hipLaunchKernelGGL(rank_order_kernel, dim3((unsigned)pl.gather_grid), dim3(256), 0, 0, rs.pay, n, d_wide);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(order_out, d_wide, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    if (W) {
        if (m) HIP_TRY(hipMemcpy(value_means_out, d_means, (size_t)m * nout * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(key_means_out, d_means + (size_t)m * nout, (size_t)nout * 8, hipMemcpyDeviceToHost));
    }
    if (nb) {
        HIP_TRY(hipMemcpy(start_out, bins.start, (size_t)nb * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(stop_out, bins.stop, (size_t)nb * 8, hipMemcpyDeviceToHost));
        if (m) HIP_TRY(hipMemcpy(counts_out, bins.counts, (size_t)m * nb * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(key_lo_out, bins.key_lo, (size_t)nb * sizeof(F), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(key_hi_out, bins.key_hi, (size_t)nb * sizeof(F), hipMemcpyDeviceToHost));
    }
    EVAL_TRY(clock.close(nullptr));
    HIP_TRY(hipDeviceSynchronize());
    float ms[WIN_PHASES];
    EVAL_TRY(clock.read(ms, WIN_PHASES));
    ms[WIN_ALLOC] = std::chrono::duration<float, std::milli>(t_up - t_alloc).count();
    memcpy(g_windows_info.ms, ms, sizeof ms);
    g_windows_info.run = pl.run;
    g_windows_info.blocks_per_run = pl.blocks_per_run;
    g_windows_info.runs_per_block = pl.runs_per_block;
    return 0;
}

extern "C" int knn_eval_windows(const void *keys, int32_t key_type, int64_t n, const uint8_t *values, int32_t m, int32_t descending, int64_t window,
                                double *key_means_out, double *value_means_out, int64_t *order_out, const int64_t *starts, const int64_t *stops,
                                const void *edges, int64_t nbins, int64_t *start_out, int64_t *stop_out, int64_t *counts_out, void *key_lo_out,
                                void *key_hi_out)
{
    if (key_type != KNN_RANK_F32 && key_type != KNN_RANK_F64) return set_err(KNN_ERR_INVALID, "windows: unknown key type");
    if (n < 1 || n > (int64_t)INT32_MAX) return set_err(KNN_ERR_INVALID, "windows: n outside [1, 2^31 - 1]");
    if (m < 0 || m > KNN_WINDOWS_MAX_COLS) return set_err(KNN_ERR_INVALID, "windows: m outside [0, 32]");
    if (window < 0 || window > n) return set_err(KNN_ERR_INVALID, "windows: window outside [1, n] (0: none)");
    if (nbins < 0 || nbins > KNN_WINDOWS_MAX_BINS) return set_err(KNN_ERR_INVALID, "windows: nbins outside [0, 2^20]");
    if (window == 0 && nbins == 0) return set_err(KNN_ERR_INVALID, "windows: neither a window nor bins");
    if (!keys || (m > 0 && !values)) return set_err(KNN_ERR_INVALID, "windows: null pointer");
    if (window > 0 && (!key_means_out || (m > 0 && !value_means_out))) return set_err(KNN_ERR_INVALID, "windows: null pointer");
    if (nbins > 0) {
        if (!start_out || !stop_out || (m > 0 && !counts_out) || !key_lo_out || !key_hi_out) return set_err(KNN_ERR_INVALID, "windows: null pointer");
        if (edges ? (starts || stops) : (!starts || !stops)) return set_err(KNN_ERR_INVALID, "windows: bins are either starts and stops or edges");
        if (edges && descending) return set_err(KNN_ERR_INVALID, "windows: edges need the ascending order");
        for (int64_t j = 0; j < nbins; j++) {
            if (edges) {
                const double e = key_type == KNN_RANK_F64 ? ((const double *)edges)[j] : (double)((const float *)edges)[j];
                const double prev = j == 0 ? e : (key_type == KNN_RANK_F64 ? ((const double *)edges)[j - 1] : (double)((const float *)edges)[j - 1]);
                if (!std::isfinite(e) || e < prev) return set_err(KNN_ERR_INVALID, "windows: edges must be finite and ascending");
            } else if (starts[j] < 0 || starts[j] > stops[j] || stops[j] > n) {
                return set_err(KNN_ERR_INVALID, "windows: a range outside 0 <= start <= stop <= n");
            }
        }
    } else if (starts || stops || edges) {
        return set_err(KNN_ERR_INVALID, "windows: bins without nbins");
    }
    WindowsPlan pl;
    if (!plan_windows(n, key_type == KNN_RANK_F64 ? 8 : 4, m, window, order_out != nullptr, nbins, &pl)) return set_err(KNN_ERR_INVALID, "windows: no plan");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    if (key_type == KNN_RANK_F64)
        return windows_run<uint64_t>(keys, values, descending != 0, pl, key_means_out, value_means_out, order_out, starts, stops, edges, start_out, stop_out,
                                     counts_out, key_lo_out, key_hi_out);
    return windows_run<uint32_t>(keys, values, descending != 0, pl, key_means_out, value_means_out, order_out, starts, stops, edges, start_out, stop_out,
                                 counts_out, key_lo_out, key_hi_out);
}

extern "C" int knn_last_windows_info(int64_t *run, int64_t *blocks_per_run, int64_t *runs_per_block, float *ms)
{
    if (!run || !blocks_per_run || !runs_per_block || !ms) return set_err(KNN_ERR_INVALID, "last_windows_info: null pointer");
    *run = g_windows_info.run;
    *blocks_per_run = g_windows_info.blocks_per_run;
    *runs_per_block = g_windows_info.runs_per_block;
    for (int i = 0; i < WIN_PHASES; i++) ms[i] = g_windows_info.ms[i];
    return 0;
}
