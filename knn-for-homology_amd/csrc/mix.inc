// mix.inc -- weighted mixes of embedding layers, made, searched and scored on the device (included by knn355_lib.hip last).
//
// The reference builds ratio[0] * cnn + ratio[1] * lstm1 + ratio[2] * lstm2 on the host for every point of a simplex grid,
// searches each mix (cath/compare_seqvec_layer.py:44-64) and keeps one number of it, the top-1 correctness at the homology
// level (:87-91).  Here the layers go up once (knn_mix handle), a mix is written straight into a flat index's rows and only
// [G][nlevels] integers come back.  The arithmetic contract is above knn_mix_create in include/knn355.h.
//
//   mix_rows_kernel  <L, VEC>: a grid-stride loop over the items of the output, an item being four columns of one row
//                    (VEC: one 16-byte load per layer, one 16-byte store) or one column (plan_mix decides: bases and row
//                    strides).  The padding columns d .. dp - 1 of the index's rows are items too and are written as zeros,
//                    as pad_rows_kernel leaves them.  Bandwidth-bound: L reads and one write per element, nothing is
//                    reused; at most MIX_MAX_GRID workgroups.
//   mix_top1_kernel  one thread per row q of a self-search result: is hit I[q][column] of q's class, per level?  A ballot
//                    per wave and level, the popcounts into LDS, one 64-bit integer atomic per workgroup and level.
//   No fma: __fmul_rn / __fadd_rn, and the library is built with -ffp-contract=off.

struct MixArgs {
    const float *x[KNN_MIX_MAX_LAYERS];
    int64_t stride[KNN_MIX_MAX_LAYERS]; // floats between rows of layer i
    float w[KNN_MIX_MAX_LAYERS];
    float *out;                         // [n][dp]
    int64_t items;                      // n * per_row
    int per_row, d, dp;
};

// ((w0 * x0 + w1 * x1) + w2 * x2) + w3 * x3 over the first L layers: one rounding per product and per sum
template <int L>
__device__ __forceinline__ float mix_value(const MixArgs &a, const float *v)
{
    float acc = __fmul_rn(a.w[0], v[0]);
#pragma unroll
    for (int i = 1; i < L; i++) acc = __fadd_rn(acc, __fmul_rn(a.w[i], v[i]));
    return acc;
}

template <int L, bool VEC>
__global__ __launch_bounds__(MIX_BLOCK) void mix_rows_kernel(MixArgs a)
{
    const int64_t step = (int64_t)gridDim.x * MIX_BLOCK;
    const int64_t first = (int64_t)blockIdx.x * MIX_BLOCK + threadIdx.x;
    // (row, item of the row) advance by the step's quotient and remainder: one division per thread, none per item
    int64_t r = first / a.per_row;
    int q = (int)(first - r * a.per_row);
    const int64_t step_r = step / a.per_row;
    const int step_q = (int)(step - step_r * a.per_row);
    for (int64_t it = first; it < a.items; it += step) {
        const int c0 = VEC ? 4 * q : q;
        float *o = a.out + (size_t)r * a.dp + c0;
        if (VEC && c0 + 4 <= a.d) {
            f32x4 v[L];
#pragma unroll
            for (int i = 0; i < L; i++) v[i] = *(const f32x4 *)(a.x[i] + (size_t)r * a.stride[i] + c0);
            f32x4 res;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                float t[L];
#pragma unroll
                for (int i = 0; i < L; i++) t[i] = v[i][e];
                res[e] = mix_value<L>(a, t);
            }
            *(f32x4 *)o = res;
        } else {
            // one column, or a quad that reaches past d: the columns inside the row float by float, zeros behind them
#pragma unroll
            for (int e = 0; e < (VEC ? 4 : 1); e++) {
                const int c = c0 + e;
                float res = 0.0f;
                if (c < a.d) {
                    float t[L];
#pragma unroll
                    for (int i = 0; i < L; i++) t[i] = a.x[i][(size_t)r * a.stride[i] + c];
                    res = mix_value<L>(a, t);
                }
                o[e] = res;
            }
        }
        r += step_r;
        q += step_q;
        if (q >= a.per_row) {
            q -= a.per_row;
            r++;
        }
    }
}

__global__ __launch_bounds__(MIX_BLOCK) void mix_top1_kernel(const int64_t *__restrict__ I, int64_t n, int k, int column, const int32_t *__restrict__ mapping,
                                                             int nlevels, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned int s_count[KNN_MIX_MAX_LEVELS];
    if (threadIdx.x < KNN_MIX_MAX_LEVELS) s_count[threadIdx.x] = 0u;
    __syncthreads();
    const int64_t q = (int64_t)blockIdx.x * MIX_BLOCK + threadIdx.x;
    const int64_t hit = q < n ? I[q * k + column] : -1;
    const bool inside = q < n && hit >= 0 && hit < n; // (knn_eval_levels' rule: a hit outside the rows is wrong)
    for (int l = 0; l < nlevels; l++) {
        const bool ok = inside && mapping[q * nlevels + l] == mapping[hit * nlevels + l];
        const unsigned long long votes = __ballot(ok);
        if ((threadIdx.x & 63) == 0 && votes) atomicAdd(&s_count[l], (unsigned int)__popcll(votes));
    }
    __syncthreads();
    if ((int)threadIdx.x < nlevels && s_count[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_count[threadIdx.x]);
}

// ---- host -------------------------------------------------------------------------------
struct knn_mix_s {
    int d = 0, nlayers = 0, device = 0;
    int64_t n = 0; // rows of every layer that is set
    struct Layer {
        const float *p = nullptr; // own.p, or the caller's device rows (knn_mix_set_layer_dev)
        int64_t stride = 0;
        DevBuf own;
    } layer[KNN_MIX_MAX_LAYERS];
    DevBuf ws_D, ws_I, ws_map, ws_counts; // knn_mix_sweep: one mix's results, the mapping, [G][nlevels] counts
    std::mutex mu;
};

// measurement (tools/bench_layer_mix.py): HIP-event milliseconds of this thread's last successful call, summed over its mixes
enum { MIX_MIX, MIX_SEARCH, MIX_SCORE, MIX_PHASES }; // knn_mix_into's launches, self-search, scoring
static thread_local float g_mix_ms[MIX_PHASES] = {0, 0, 0};

extern "C" int knn_mix_create(int32_t d, int32_t nlayers, knn_mix_handle *out)
{
    if (!out) return set_err(KNN_ERR_INVALID, "mix_create: null out");
    if (d < 1) return set_err(KNN_ERR_INVALID, "mix_create: d must be positive");
    if (nlayers < 1 || nlayers > KNN_MIX_MAX_LAYERS) return set_err(KNN_ERR_INVALID, "mix_create: nlayers must be 1 .. KNN_MIX_MAX_LAYERS");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    knn_mix_s *h = new knn_mix_s();
    h->d = d;
    h->nlayers = nlayers;
    h->device = g_device;
    *out = h;
    return 0;
}

extern "C" void knn_mix_free(knn_mix_handle h)
{
    if (!h) return;
    if (hipSetDevice(h->device) == hipSuccess) {
        (void)hipDeviceSynchronize(); // (the buffers go back to the pool: nothing may still read them)
        for (auto &l : h->layer) l.own.release();
        DevBuf *bufs[] = {&h->ws_D, &h->ws_I, &h->ws_map, &h->ws_counts};
        for (DevBuf *b : bufs) b->release();
    }
    delete h;
}

// what both setters refuse; the caller holds h->mu
static int mix_check_layer(const knn_mix_s *h, const char *who, int32_t i, const float *x, int64_t n, int64_t row_stride)
{
    const std::string w = std::string(who) + ": ";
    if (i < 0 || i >= h->nlayers) return set_err(KNN_ERR_INVALID, w + "layer index out of range");
    if (!x) return set_err(KNN_ERR_INVALID, w + "null pointer");
    if (n < 1 || n > 0xFFFFFFF0ll) return set_err(KNN_ERR_INVALID, w + "need 1 <= n <= 2^32 - 16 rows");
    if (row_stride < h->d || row_stride >= ((int64_t)1 << 40)) return set_err(KNN_ERR_INVALID, w + "row_stride is below d (or absurd)");
    for (int j = 0; j < h->nlayers; j++)
        if (j != i && h->layer[j].p && h->n != n) return set_err(KNN_ERR_INVALID, w + "all layers must have the same n");
    return 0;
}

extern "C" int knn_mix_set_layer(knn_mix_handle h, int32_t i, const float *x_host, int64_t n, int64_t row_stride)
{
    if (!h) return set_err(KNN_ERR_INVALID, "mix_set_layer: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = mix_check_layer(h, "mix_set_layer", i, x_host, n, row_stride);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    knn_mix_s::Layer &l = h->layer[i];
    l.p = nullptr;
    const size_t row_bytes = (size_t)h->d * 4;
    if (l.own.ensure((size_t)n * row_bytes)) return set_err(KNN_ERR_HIP, "mix_set_layer: out of device memory");
    // (packed on the device: [n][d])
    HIP_TRY(hipMemcpy2D(l.own.p, row_bytes, x_host, (size_t)row_stride * 4, row_bytes, (size_t)n, hipMemcpyHostToDevice));
    l.p = (const float *)l.own.p;
    l.stride = h->d;
    h->n = n;
    return 0;
}

extern "C" int knn_mix_set_layer_dev(knn_mix_handle h, int32_t i, const float *x_dev, int64_t n, int64_t row_stride, void *stream)
{
    if (!h) return set_err(KNN_ERR_INVALID, "mix_set_layer_dev: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = mix_check_layer(h, "mix_set_layer_dev", i, x_dev, n, row_stride);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream)); // (the rows are complete before a mix reads them on the index's stream)
    knn_mix_s::Layer &l = h->layer[i];
    l.own.release();
    l.p = x_dev;
    l.stride = row_stride;
    h->n = n;
    return 0;
}

static int mix_check_args(const knn_mix_s *h, const char *who, const float *weights, knn_index_s *flat, bool sweep, int64_t g, int64_t k, int64_t column,
                          int64_t nlevels)
{
    const std::string w = std::string(who) + ": ";
    if (!h || !flat) return set_err(KNN_ERR_INVALID, w + "null handle");
    if (!weights) return set_err(KNN_ERR_INVALID, w + "null weights");
    unsigned set = 0;
    for (int i = 0; i < h->nlayers; i++) set |= h->layer[i].p ? 1u << i : 0u;
    if (const char *why = mix_args_illegal(h->d, h->nlayers, set, flat->d, flat->is_view, sweep, g, k, column, nlevels)) return set_err(KNN_ERR_INVALID, w + why);
    if (flat->device != h->device) return set_err(KNN_ERR_INVALID, w + "the index lives on another device than the layers");
    return 0;
}

static int mix_launch(const MixPlan &pl, int nlayers, const MixArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)pl.grid), block(MIX_BLOCK);
#define MIX_LAUNCH(L)                                                                        \
    do {                                                                                     \
        if (pl.vec) hipLaunchKernelGGL((mix_rows_kernel<L, true>), grid, block, 0, s, a);    \
        else hipLaunchKernelGGL((mix_rows_kernel<L, false>), grid, block, 0, s, a);          \
    } while (0)
    switch (nlayers) {
    case 1: MIX_LAUNCH(1); break;
    case 2: MIX_LAUNCH(2); break;
    case 3: MIX_LAUNCH(3); break;
    default: MIX_LAUNCH(4); break;
    }
#undef MIX_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

// knn_mix_into behind its checks; the caller holds h->mu, this takes flat's.  Everything runs on flat's stream and is waited
// for.  The launches are a MIX_MIX interval of the clock; the event behind them starts one of phase `then` (PhaseClock::NONE:
// it only ends theirs).
static int mix_into_impl(knn_mix_s *h, const float *weights, knn_index_s *flat, bool normalize, PhaseClock &clock, int then)
{
    std::lock_guard<std::mutex> lk(flat->mu);
    HIP_TRY(hipSetDevice(flat->device));
    hipStream_t s = flat->stream;
    const int64_t n = h->n;
    // reset, then reserve: the storage goes through the pool and comes back from it
    HIP_TRY(hipStreamSynchronize(s));
    free_index_buffers(flat);
    int rc = move_storage(flat, n, "mix_into");
    if (rc) return rc;
    if ((rc = scan16_sync_rows(flat, 0, 0, s))) return rc;
    MixArgs a = {};
    uintptr_t bases[KNN_MIX_MAX_LAYERS];
    for (int i = 0; i < h->nlayers; i++) {
        a.x[i] = h->layer[i].p;
        a.stride[i] = h->layer[i].stride;
        a.w[i] = weights[i];
        bases[i] = (uintptr_t)a.x[i];
    }
    MixPlan pl;
    if (!plan_mix(n, h->d, flat->dp, h->nlayers, bases, a.stride, (uintptr_t)flat->xb, &pl)) return set_err(KNN_ERR_INVALID, "mix_into: no plan");
    a.out = flat->xb;
    a.items = pl.items;
    a.per_row = pl.per_row;
    a.d = h->d;
    a.dp = flat->dp;
    EVAL_TRY(clock.open(MIX_MIX, s));
    EVAL_TRY(mix_launch(pl, h->nlayers, a, s));
    if (normalize) EVAL_TRY(normalize_dev_impl(flat->xb, n, flat->d, flat->dp, s));
    // what add_dev_impl does behind its copy
    EVAL_TRY(norms_dev_impl(flat->xb, n, flat->d, flat->dp, flat->yn, s));
    EVAL_TRY(approx16_sync_rows(flat, 0, n, s));
    EVAL_TRY(scan16_sync_rows(flat, 0, n, s));
    EVAL_TRY(clock.next(then, s));
    flat->ntotal = n;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

extern "C" int knn_mix_into(knn_mix_handle h, const float *weights, knn_handle flat, int32_t normalize)
{
    if (!h) return set_err(KNN_ERR_INVALID, "mix_into: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = mix_check_args(h, "mix_into", weights, flat, false, 0, 0, 0, 0);
    if (rc) return rc;
    PhaseClock clock;
    if ((rc = mix_into_impl(h, weights, flat, normalize != 0, clock, PhaseClock::NONE))) return rc;
    float ms[MIX_PHASES]; // (no search, no scoring: both read 0)
    EVAL_TRY(clock.read(ms, MIX_PHASES));
    memcpy(g_mix_ms, ms, sizeof ms);
    return 0;
}

extern "C" int knn_mix_sweep(knn_mix_handle h, const float *weights, int64_t G, knn_handle flat, int64_t k, const int32_t *mapping, int32_t nlevels,
                             int64_t column, int64_t *counts_out, float *D_host, int64_t *I_host)
{
    if (!h) return set_err(KNN_ERR_INVALID, "mix_sweep: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    int rc = mix_check_args(h, "mix_sweep", weights, flat, true, G, k, column, nlevels);
    if (rc) return rc;
    if (!mapping || !counts_out) return set_err(KNN_ERR_INVALID, "mix_sweep: null pointer");
    if ((D_host == nullptr) != (I_host == nullptr)) return set_err(KNN_ERR_INVALID, "mix_sweep: D_host and I_host go together");
    if (G == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    const int64_t n = h->n;
    const size_t cells = (size_t)n * (size_t)k;
    hipStream_t s = flat->stream;
    float *D_dev;
    int64_t *I_dev;
    int32_t *d_map;
    unsigned long long *d_counts;
    const char *oom = "mix_sweep: out of device memory";
    if (!(D_dev = scratch_device_wide<float>(h->ws_D, cells, oom)) || !(I_dev = scratch_device_wide<int64_t>(h->ws_I, cells, oom)) ||
        !(d_map = scratch_device_wide<int32_t>(h->ws_map, (size_t)n * nlevels, oom)) ||
        !(d_counts = scratch_device_wide<unsigned long long>(h->ws_counts, (size_t)G * nlevels, oom)))
        return KNN_ERR_HIP;
    std::vector<long long> counts((size_t)G * nlevels);
    PhaseClock clock; // per mix: the mix, the search, the scoring, one behind the other
    const bool normalize = flat->metric == KNN_METRIC_INNER_PRODUCT;
    auto enqueue = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(d_map, mapping, (size_t)n * nlevels * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(d_counts, 0, (size_t)G * nlevels * 8, s));
        for (int64_t g = 0; g < G; g++) {
            EVAL_TRY(mix_into_impl(h, weights + g * h->nlayers, flat, normalize, clock, MIX_SEARCH));
            EVAL_TRY(knn_flat_search_self_dev(flat, k, D_dev, I_dev));
            EVAL_TRY(clock.next(MIX_SCORE, s));
            hipLaunchKernelGGL(mix_top1_kernel, dim3((unsigned)((n + MIX_BLOCK - 1) / MIX_BLOCK)), dim3(MIX_BLOCK), 0, s, I_dev, n, (int)k, (int)column, d_map,
                               (int)nlevels, d_counts + g * nlevels);
            HIP_TRY(hipGetLastError());
            EVAL_TRY(clock.close(s));
            if (D_host) {
                HIP_TRY(hipMemcpyAsync(D_host + (size_t)g * cells, D_dev, cells * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipMemcpyAsync(I_host + (size_t)g * cells, I_dev, cells * 8, hipMemcpyDeviceToHost, s));
            }
        }
        HIP_TRY(hipMemcpyAsync(counts.data(), d_counts, counts.size() * 8, hipMemcpyDeviceToHost, s));
        return 0;
    };
    rc = enqueue();
    const hipError_t e = hipStreamSynchronize(s); // (always: copies already queued write the caller's arrays and this frame's vector)
    if (rc) return rc;
    if (e != hipSuccess) return set_err(KNN_ERR_HIP, std::string("mix_sweep: ") + hipGetErrorString(e));
    float ms[MIX_PHASES];
    EVAL_TRY(clock.read(ms, MIX_PHASES));
    for (size_t i = 0; i < counts.size(); i++) counts_out[i] = (int64_t)counts[i];
    memcpy(g_mix_ms, ms, sizeof ms);
    return 0;
}

extern "C" int knn_mix_last_ms(float *mix_ms, float *search_ms, float *score_ms)
{
    if (!mix_ms || !search_ms || !score_ms) return set_err(KNN_ERR_INVALID, "mix_last_ms: null pointer");
    *mix_ms = g_mix_ms[0];
    *search_ms = g_mix_ms[1];
    *score_ms = g_mix_ms[2];
    return 0;
}
