// pool.inc -- mean pooling of row ranges: the per-protein and per-domain embeddings (included by knn355_lib.hip last).
//
// The reference produces the matrix an index stores with a Python loop over ragged [L, d] per-residue arrays:
// embedding[start - 1 : stop].mean(axis=0) per Pfam domain (pfam/embed_pfam_seqvec.py:29-40), reduce_per_protein
// (pfam/embed_pfam_t5.py:40-43, pfam/embed_t5_fp16.py:45-47, cath/embed.py:92-94) and normalize_L2 on every residue row in
// front of it (pfam/embed_t5_l2.py:68-71).  The arithmetic contract is above knn_pool_ranges in include/knn355.h: per
// (range, column) one chain of fp32 adds in ascending row order starting from the first row's value, one division.
//
//   pool_check_kernel    one thread per range: the lowest index of a bad range into the status word (atomicMin).
//   pool_ranges_kernel   <T, NORMALIZE, ALIGNED>: one wave per (range, block of 256 columns), lane l owns the columns
//                        256 cb + 4 l .. + 3 and reads them as one 16-byte load per row (8-byte for fp16); the waves of a
//                        workgroup are neighbouring column blocks of ONE range (plan_pool), so the workgroup reads a row
//                        as consecutive 128-byte lines.  Rows are walked in order in batches of 64 and, inside a batch,
//                        in groups of eight: the eight loads are issued, then the eight adds follow in row order -- the
//                        add chain is a dependency chain and only loads in flight hide the latency.  A range is never
//                        split by rows: the order of the adds is the contract.
//                        NORMALIZE: in front of each batch its (at most) 64 norms are computed with lane_norm_row, one
//                        lane per row, the rows dealt out over the workgroup's waves; the factors go through LDS (two
//                        buffers taking turns, one barrier per batch) and every wave reads factor r as a broadcast.  The
//                        rows are then read again for the scaled adds.
//                        ALIGNED false (a base that is no multiple of four elements, a row stride that is no multiple of
//                        four): element loads.  A lane whose four columns cross d loads the ones inside element by
//                        element in either build.
//   No atomics on floats, no fma: __fadd_rn / __fmul_rn / __fdiv_rn, and the library is built with -ffp-contract=off.

// the one rule for a range, for the check kernel and for the pooling kernel's own guard
__device__ __forceinline__ bool pool_range_ok(int64_t start, int64_t stop, int64_t rows)
{
    return start >= 0 && start < stop && stop <= rows && stop - start < POOL_MAX_LEN;
}

__global__ __launch_bounds__(256) void pool_check_kernel(const int64_t *__restrict__ starts, const int64_t *__restrict__ stops, int64_t n, int64_t rows,
                                                         unsigned long long *__restrict__ status)
{
    const int64_t o = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (o < n && !pool_range_ok(starts[o], stops[o], rows)) atomicMin(status, (unsigned long long)o);
}

// the lane's columns of one row as four floats: nvalid of them (1 .. 4) are inside the row, the others come back as 0
template <typename T, bool ALIGNED>
__device__ __forceinline__ f32x4 pool_load4(const T *__restrict__ p, int nvalid)
{
    f32x4 v = {0.0f, 0.0f, 0.0f, 0.0f};
    if (ALIGNED && nvalid == 4) {
        if constexpr (sizeof(T) == 4) {
            v = *(const f32x4 *)p;
        } else {
            const f16x4 h = *(const f16x4 *)p;
#pragma unroll
            for (int e = 0; e < 4; e++) v[e] = (float)h[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (e < nvalid) v[e] = (float)p[e];
    }
    return v;
}

// s < 0: the row is used as it is (normalize_rows_kernel's rule)
template <bool NORMALIZE>
__device__ __forceinline__ f32x4 pool_value(f32x4 v, float s)
{
    if (NORMALIZE && !(s < 0.0f)) {
#pragma unroll
        for (int e = 0; e < 4; e++) v[e] = __fmul_rn(v[e], s);
    }
    return v;
}

struct PoolArgs {
    const void *x;          // [rows][stride] elements of T
    int64_t rows, stride;
    int d;
    const int64_t *starts, *stops; // [n]
    const int64_t *out_row;        // [n] output row of range o, or null: o
    float *out;                    // [.][d]
};

template <typename T, bool NORMALIZE, bool ALIGNED>
__global__ __launch_bounds__(64 * POOL_MAX_WAVES) void pool_ranges_kernel(PoolArgs a)
{
    __shared__ float s_fac[2][POOL_NORM_ROWS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const int64_t o = blockIdx.x;
    const int64_t start = a.starts[o], stop = a.stops[o];
    if (!pool_range_ok(start, stop, a.rows)) return; // (the whole workgroup: nothing of x is read for a bad range)
    const T *__restrict__ x = (const T *)a.x;
    const int d = a.d;
    const int c0 = (blockIdx.y * nwaves + wave) * POOL_COLS + 4 * lane;
    const int nvalid = min(4, d - c0); // <= 0: the lane (past the last column block: the whole wave) adds nothing
    const T *__restrict__ col = x + (nvalid > 0 ? c0 : 0);
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    int turn = 0;
    for (int64_t b0 = start; b0 < stop; b0 += POOL_NORM_ROWS, turn ^= 1) {
        const int nb = (int)min((int64_t)POOL_NORM_ROWS, stop - b0);
        if constexpr (NORMALIZE) {
            // row j of the batch is lane j % per of wave j / per
            const int per = POOL_NORM_ROWS / nwaves, j = wave * per + lane;
            if (lane < per && j < nb) {
                const float nr = lane_norm_row<ALIGNED, T>(x + (size_t)(b0 + j) * a.stride, d);
                s_fac[turn][j] = nr > 0.0f ? (float)(1.0 / (double)sqrtf(nr)) : -1.0f;
            }
            __syncthreads();
        }
        if (nvalid <= 0) continue;
        const T *__restrict__ p = col + (size_t)b0 * a.stride;
        int j = 0;
        if (b0 == start) {
            acc = pool_value<NORMALIZE>(pool_load4<T, ALIGNED>(p, nvalid), NORMALIZE ? s_fac[turn][0] : -1.0f);
            j = 1;
        }
        for (; j + POOL_GROUP <= nb; j += POOL_GROUP) {
            f32x4 v[POOL_GROUP];
#pragma unroll
            for (int u = 0; u < POOL_GROUP; u++) v[u] = pool_load4<T, ALIGNED>(p + (size_t)(j + u) * a.stride, nvalid);
#pragma unroll
            for (int u = 0; u < POOL_GROUP; u++) {
                const f32x4 w = pool_value<NORMALIZE>(v[u], NORMALIZE ? s_fac[turn][j + u] : -1.0f);
#pragma unroll
                for (int e = 0; e < 4; e++) acc[e] = __fadd_rn(acc[e], w[e]);
            }
        }
        for (; j < nb; j++) {
            const f32x4 w = pool_value<NORMALIZE>(pool_load4<T, ALIGNED>(p + (size_t)j * a.stride, nvalid), NORMALIZE ? s_fac[turn][j] : -1.0f);
#pragma unroll
            for (int e = 0; e < 4; e++) acc[e] = __fadd_rn(acc[e], w[e]);
        }
    }
    if (nvalid <= 0) return;
    const float len = (float)(stop - start);
#pragma unroll
    for (int e = 0; e < 4; e++) acc[e] = __fdiv_rn(acc[e], len);
    float *q = a.out + (size_t)(a.out_row ? a.out_row[o] : o) * d + c0;
    if (nvalid == 4 && (d & 3) == 0 && ((uintptr_t)a.out & 15) == 0) {
        *(f32x4 *)q = acc;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
            if (e < nvalid) q[e] = acc[e];
    }
}

// ---- host -------------------------------------------------------------------------------
// measurement (tools/bench_pool.py): HIP-event milliseconds of this thread's last successful call
enum { POOL_UP, POOL_KERNELS, POOL_DOWN, POOL_PHASES };
static thread_local float g_pool_ms[POOL_PHASES] = {0, 0, 0};

static int pool_launch(const PoolPlan &pl, int dtype, bool normalize, const PoolArgs &a, hipStream_t s)
{
    const dim3 grid((unsigned)pl.grid_x, (unsigned)pl.grid_y), block(64 * pl.waves);
#define POOL_LAUNCH(T, N, A) hipLaunchKernelGGL((pool_ranges_kernel<T, N, A>), grid, block, 0, s, a)
#define POOL_PICK(T)                                                     \
    do {                                                                 \
        if (normalize) {                                                 \
            if (pl.aligned) POOL_LAUNCH(T, true, true);                  \
            else POOL_LAUNCH(T, true, false);                            \
        } else {                                                         \
            if (pl.aligned) POOL_LAUNCH(T, false, true);                 \
            else POOL_LAUNCH(T, false, false);                           \
        }                                                                \
    } while (0)
    if (dtype == 0) POOL_PICK(float);
    else POOL_PICK(_Float16);
#undef POOL_PICK
#undef POOL_LAUNCH
    HIP_TRY(hipGetLastError());
    return 0;
}

// what both entries refuse before they look at a range
static int pool_check_args(const char *who, const void *x, int32_t dtype, int64_t rows, int32_t d, int64_t row_stride, const int64_t *starts,
                           const int64_t *stops, int64_t n, int32_t flags, const float *out)
{
    const std::string w = std::string(who) + ": ";
    if (dtype != 0 && dtype != 1) return set_err(KNN_ERR_INVALID, w + "dtype must be 0 (float32) or 1 (float16)");
    if (flags & ~KNN_POOL_NORMALIZE) return set_err(KNN_ERR_INVALID, w + "unknown flags");
    if (d < 2 || d > KNN_POOL_MAX_D) return set_err(KNN_ERR_INVALID, w + "need 2 <= d <= KNN_POOL_MAX_D");
    if (rows < 0 || n < 0) return set_err(KNN_ERR_INVALID, w + "negative row or range count");
    if (n > (int64_t)INT32_MAX) return set_err(KNN_ERR_INVALID, w + "more than 2^31 - 1 ranges");
    if (row_stride < d) return set_err(KNN_ERR_INVALID, w + "row_stride is below d");
    if (n > 0 && (!x || !starts || !stops || !out)) return set_err(KNN_ERR_INVALID, w + "null pointer");
    return 0;
}

// rows per upload of the host entry: 64 MiB.  KNN355_POOL_CHUNK_ROWS (read on every call; a positive decimal integer,
// anything else is ignored) replaces the count, so that a test crosses chunk ends with a handful of rows
static int64_t pool_chunk_rows(size_t row_bytes)
{
    const char *e = getenv("KNN355_POOL_CHUNK_ROWS");
    if (e && *e >= '0' && *e <= '9') {
        char *end = nullptr;
        errno = 0;
        const long long v = strtoll(e, &end, 10);
        if (errno == 0 && *end == '\0' && v > 0) return (int64_t)v;
    }
    return std::max<int64_t>(1, (int64_t)((size_t)(64u << 20) / row_bytes));
}

extern "C" int knn_pool_ranges_dev(const void *x_dev, int32_t dtype, int64_t rows, int32_t d, int64_t row_stride, const int64_t *starts_dev,
                                   const int64_t *stops_dev, int64_t n, int32_t flags, float *out_dev, void *stream)
{
    int rc = pool_check_args("pool_ranges_dev", x_dev, dtype, rows, d, row_stride, starts_dev, stops_dev, n, flags, out_dev);
    if (rc || n == 0) return rc;
    PoolPlan pl;
    if (!plan_pool(n, d, row_stride, (uintptr_t)x_dev, dtype ? 2 : 4, flags & KNN_POOL_NORMALIZE, &pl)) return set_err(KNN_ERR_INVALID, "pool_ranges_dev: no plan");
    int device = 0;
    HIP_TRY(hipGetDevice(&device));
    unsigned long long status = 0;
    HostCall call((hipStream_t)stream);
    hipStream_t s = call.s;
    PoolBuf status_buf(64, device); // (goes back behind finish()'s wait)
    unsigned long long *d_status = status_buf.get<unsigned long long>();
    if (!d_status) return set_err(KNN_ERR_HIP, "pool_ranges_dev: out of device memory");
    auto enqueue = [&]() -> int {
        HIP_TRY(hipMemsetAsync(d_status, 0xFF, 8, s));
        hipLaunchKernelGGL(pool_check_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, starts_dev, stops_dev, n, rows, d_status);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(call.clock.open(POOL_KERNELS, s));
        const PoolArgs a = {x_dev, rows, row_stride, (int)d, starts_dev, stops_dev, nullptr, out_dev};
        EVAL_TRY(pool_launch(pl, dtype, flags & KNN_POOL_NORMALIZE, a, s));
        EVAL_TRY(call.clock.close(s));
        HIP_TRY(hipMemcpyAsync(&status, d_status, 8, hipMemcpyDeviceToHost, s));
        return 0;
    };
    // (finish() always waits: the copy already queued writes this frame's status word)
    if ((rc = call.finish("pool_ranges_dev", enqueue()))) return rc;
    float ms[POOL_PHASES]; // (nothing is moved: the upload and the download read 0)
    EVAL_TRY(call.clock.read(ms, POOL_PHASES));
    if (status != ~0ull)
        return set_err(KNN_ERR_INVALID, "pool_ranges_dev: range " + std::to_string(status) + " is not 0 <= start < stop <= rows with stop - start < 2^24");
    memcpy(g_pool_ms, ms, sizeof ms);
    return 0;
}

// everything of knn_pool_ranges that is enqueued; the caller waits for both streams whatever this returns.
// s: the kernels and the download; up: the uploads (the copy pipeline's host-to-device stream, or s itself)
static int pool_host_enqueue(const char *x, int dtype, int d, const std::vector<int64_t> &order, const std::vector<PoolChunk> &chunks, const int64_t *starts,
                             const int64_t *stops, int64_t n, int flags, float *out, EvalBufs &bufs, hipStream_t s, CopyPipes *cp, PhaseClock &clock,
                             std::vector<int64_t> &meta)
{
    const size_t esz = dtype ? 2 : 4, row_bytes = (size_t)d * esz;
    int64_t max_rows = 0, max_count = 0;
    for (const PoolChunk &c : chunks) {
        max_rows = std::max(max_rows, c.row1 - c.row0);
        max_count = std::max(max_count, c.count);
    }
    const int slots = cp && chunks.size() > 1 ? 2 : 1;
    hipStream_t up = cp ? cp->h2d : s;
    char *d_x[2] = {nullptr, nullptr};
    int64_t *d_meta[2] = {nullptr, nullptr}; // per slot: starts, stops (rebased to the chunk's first row), output rows
    for (int i = 0; i < slots; i++) {
        EVAL_ALLOC(px, char *, (size_t)max_rows * row_bytes);
        EVAL_ALLOC(pm, int64_t *, (size_t)max_count * 3 * 8);
        d_x[i] = px;
        d_meta[i] = pm;
    }
    EVAL_ALLOC(d_out, float *, (size_t)n * d * 4);
    // the host copy of every chunk's three arrays, alive until the streams have drained (the caller holds `meta`)
    meta.resize((size_t)n * 3);
    size_t at = 0;
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        const PoolChunk &c = chunks[ci];
        const int slot = (int)(ci & (size_t)(slots - 1));
        const size_t m = (size_t)c.count;
        int64_t *h = meta.data() + at;
        at += 3 * m;
        for (size_t i = 0; i < m; i++) {
            const int64_t o = order[(size_t)c.first + i];
            h[i] = starts[o] - c.row0;
            h[m + i] = stops[o] - c.row0;
            h[2 * m + i] = o;
        }
        // the slot's previous chunk has been pooled
        if (cp && ci >= 2) HIP_TRY(hipStreamWaitEvent(up, cp->ev_batch[slot], 0));
        EVAL_TRY(clock.open(POOL_UP, up));
        HIP_TRY(hipMemcpyAsync(d_x[slot], x + (size_t)c.row0 * row_bytes, (size_t)(c.row1 - c.row0) * row_bytes, hipMemcpyHostToDevice, up));
        HIP_TRY(hipMemcpyAsync(d_meta[slot], h, 3 * m * 8, hipMemcpyHostToDevice, up));
        EVAL_TRY(clock.close(up));
        if (cp) {
            HIP_TRY(hipEventRecord(cp->ev_query[slot], up));
            HIP_TRY(hipStreamWaitEvent(s, cp->ev_query[slot], 0));
        }
        PoolPlan pl;
        if (!plan_pool(c.count, d, d, (uintptr_t)d_x[slot], (int)esz, flags & KNN_POOL_NORMALIZE, &pl)) return set_err(KNN_ERR_INVALID, "pool_ranges: no plan");
        const PoolArgs a = {d_x[slot], c.row1 - c.row0, (int64_t)d, d, d_meta[slot], d_meta[slot] + m, d_meta[slot] + 2 * m, d_out};
        EVAL_TRY(clock.open(POOL_KERNELS, s));
        EVAL_TRY(pool_launch(pl, dtype, flags & KNN_POOL_NORMALIZE, a, s));
        EVAL_TRY(clock.close(s));
        if (cp) HIP_TRY(hipEventRecord(cp->ev_batch[slot], s));
    }
    EVAL_TRY(clock.open(POOL_DOWN, s));
    HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * d * 4, hipMemcpyDeviceToHost, s));
    EVAL_TRY(clock.close(s));
    return 0;
}

extern "C" int knn_pool_ranges(const void *x_host, int32_t dtype, int64_t rows, int32_t d, const int64_t *starts_host, const int64_t *stops_host, int64_t n,
                               int32_t flags, float *out_host)
{
    int rc = pool_check_args("pool_ranges", x_host, dtype, rows, d, d, starts_host, stops_host, n, flags, out_host);
    if (rc || n == 0) return rc;
    for (int64_t o = 0; o < n; o++) {
        const int64_t a = starts_host[o], b = stops_host[o];
        if (a < 0 || a >= b || b > rows) return set_err(KNN_ERR_INVALID, "pool_ranges: range " + std::to_string(o) + " is not 0 <= start < stop <= rows");
        if (b - a >= POOL_MAX_LEN) return set_err(KNN_ERR_INVALID, "pool_ranges: range " + std::to_string(o) + " has 2^24 rows or more");
    }
    if ((rc = ensure_device(g_device))) return rc;
    std::vector<int64_t> order, meta;
    std::vector<PoolChunk> chunks;
    pool_assign_chunks(starts_host, stops_host, n, pool_chunk_rows((size_t)d * (dtype ? 2 : 4)), order, chunks);
    // the uploads ride the copy pipeline's host-to-device stream when no host search holds it and there is something to
    // overlap; the kernels and the download run on a stream of this call's
    HostCall call(g_device);
    if (!call.s) return set_err(KNN_ERR_HIP, "pool_ranges: no stream");
    if ((rc = call.lease(g_device, chunks.size() > 1))) return rc;
    rc = pool_host_enqueue((const char *)x_host, dtype, d, order, chunks, starts_host, stops_host, n, flags, out_host, call.bufs, call.s, call.pipes.cp,
                           call.clock, meta);
    if ((rc = call.finish("pool_ranges", rc))) return rc;
    float ms[POOL_PHASES];
    EVAL_TRY(call.clock.read(ms, POOL_PHASES));
    memcpy(g_pool_ms, ms, sizeof ms);
    return 0;
}

extern "C" int knn_pool_last_ms(float *upload_ms, float *kernel_ms, float *download_ms)
{
    if (!upload_ms || !kernel_ms || !download_ms) return set_err(KNN_ERR_INVALID, "pool_last_ms: null pointer");
    *upload_ms = g_pool_ms[0];
    *kernel_ms = g_pool_ms[1];
    *download_ms = g_pool_ms[2];
    return 0;
}
