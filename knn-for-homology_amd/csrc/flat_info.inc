// flat_info.inc -- introspection, tuning and measurement entries of the flat index (included by knn355_lib.hip behind
// flat_search.inc): knn_last_*, the tuning setters, pinned host memory, reserve, set_scan16, the two rate probes with
// their kernels, knn_flat_set_batch, knn_gather_distances.

extern "C" int knn_last_scan_info(knn_handle h, char *name, int32_t name_len, int32_t *query_tile, int32_t *db_tile,
                                  int32_t *nchunks, int32_t *grid)
{
    if (!h) return set_err(KNN_ERR_INVALID, "null handle");
    if (name && name_len > 0) {
        strncpy(name, h->last_kernel.c_str(), (size_t)name_len - 1);
        name[name_len - 1] = 0;
    }
    if (query_tile) *query_tile = h->last_qt;
    if (db_tile) *db_tile = h->last_dt;
    if (nchunks) *nchunks = h->last_chunks;
    if (grid) *grid = h->last_grid;
    return 0;
}

extern "C" float knn_last_scan_ms(knn_handle h)
{
    if (!h) return -1.f;
    std::lock_guard<std::mutex> lk(h->mu);
    float ms = 0.f;
    if (h->last_ms >= 0.f) return h->last_ms;
    if (!h->ev0 || hipEventElapsedTime(&ms, h->ev0, h->ev1) != hipSuccess) return -1.f;
    return ms;
}

extern "C" int32_t knn_scan_times(knn_handle h, float *out_ms, int32_t max_n)
{
    if (!h || !out_ms || max_n < 0) return set_err(KNN_ERR_INVALID, "scan_times: bad arguments");
    std::lock_guard<std::mutex> lk(h->mu);
    int64_t n = std::min<int64_t>(std::min<int64_t>(h->nlaunches, knn_index_s::RING), max_n);
    // oldest first among the n most recent launches; launches whose events have not completed read -1
    for (int64_t i = 0; i < n; i++) {
        int64_t idx = h->nlaunches - n + i;
        int slot = (int)(idx % knn_index_s::RING);
        float ms = -1.f;
        if (hipEventElapsedTime(&ms, h->ring0[slot], h->ring1[slot]) != hipSuccess) ms = -1.f;
        out_ms[i] = ms;
    }
    return (int32_t)n;
}

// Page-locked host memory for result arrays: the download of a search result into it is one DMA at PCIe
// line rate (into pageable memory the runtime stages through its own pinned buffer at a third of that).
extern "C" void *knn_host_alloc(int64_t bytes)
{
    if (bytes <= 0) return nullptr;
    if (ensure_device(g_device)) return nullptr;
    void *p = nullptr;
    if (hipHostMalloc(&p, (size_t)bytes, hipHostMallocPortable) != hipSuccess) {
        set_err(KNN_ERR_HIP, "host_alloc: hipHostMalloc failed");
        return nullptr;
    }
    return p;
}
extern "C" void knn_host_free(void *p)
{
    if (p) (void)hipHostFree(p);
}

extern "C" int knn_last_seed_info(knn_handle h, int32_t *seed_stride, int32_t *stat_rank, int64_t *stat_redo, int64_t *sample_rows)
{
    if (!h) return set_err(KNN_ERR_INVALID, "null handle");
    if (sample_rows) *sample_rows = h->last_sample_rows;
    if (seed_stride) *seed_stride = h->last_seed_stride;
    if (stat_rank) *stat_rank = h->last_seed_stat;
    if (stat_redo) *stat_redo = h->stat_redo;
    return 0;
}

extern "C" int knn_flat_reserve(knn_handle h, int64_t nrows)
{
    if (!h) return set_err(KNN_ERR_INVALID, "reserve: null handle");
    if (nrows < 0 || nrows > 0xFFFFFFF0ll) return set_err(KNN_ERR_INVALID, "reserve: bad row count");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->is_view) return set_err(KNN_ERR_INVALID, "reserve: a view is read-only");
    HIP_TRY(hipSetDevice(h->device));
    if (nrows <= h->cap_rows) return 0;
    // exact-size allocation (grow_index over-allocates only when it has to guess)
    if (int rc = move_storage(h, nrows, "reserve")) return rc;
    return scan16_sync_rows(h, h->ntotal, 0, h->stream); // (the fp16 copies grow with the rows)
}

extern "C" int knn_flat_set_scan16(knn_handle h, int32_t mode)
{
    if (!h) return set_err(KNN_ERR_INVALID, "set_scan16: null handle");
    if (mode != 0 && mode != 1 && mode != 2) return set_err(KNN_ERR_INVALID, "set_scan16: mode must be 0, 1 or 2");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->is_view) return set_err(KNN_ERR_INVALID, "set_scan16: a view uses its parent's setting");
    if (mode && (h->approx16 || h->keep16)) return set_err(KNN_ERR_UNSUPPORTED, "set_scan16: not for an index that keeps bf16 copies (HNSW)");
    if (h->ntotal != 0) return set_err(KNN_ERR_INVALID, "set_scan16: the index already holds rows");
    const char *env = getenv("KNN355_SCAN16");
    if (mode && env && strcmp(env, "0") == 0) mode = 0; // (same-tree A/B runs)
    const char *fenv = getenv("KNN355_SCAN_FORMAT");
    if (mode == 2 && fenv && strcmp(fenv, "16") == 0) mode = 1; // (... of the two formats)
    h->scan16 = mode ? 1 : 0;
    h->s16_fmt = mode == 2 ? 12 : 16;
    h->dp16 = round_up(h->d, 64);
    h->s16_note = mode ? "on" : "off";
    return 0;
}

extern "C" int knn_last_scan16_info(knn_handle h, int32_t *used, int32_t *candidates_max, int64_t *fallbacks)
{
    if (!h) return set_err(KNN_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    uint32_t st[2] = {0u, 0u};
    if (h->ws_s16stat.p) {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipDeviceSynchronize()); // (the searches ran on their callers' streams)
        HIP_TRY(hipMemcpy(st, h->ws_s16stat.p, sizeof st, hipMemcpyDeviceToHost));
    }
    if (used) *used = h->last_s16_used ? 1 : 0;
    if (candidates_max) *candidates_max = h->last_s16_used ? (int32_t)st[0] : 0;
    if (fallbacks) *fallbacks = (int64_t)st[1];
    return 0;
}

extern "C" int knn_last_scan16_format(knn_handle h, int32_t *format)
{
    if (!h || !format) return set_err(KNN_ERR_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    *format = h->last_s16_used ? h->last_s16_fmt : 0;
    return 0;
}

extern "C" int knn_set_tuning(knn_handle h, int32_t query_tile, int32_t nchunks, int32_t flags)
{
    if (!h) return set_err(KNN_ERR_INVALID, "null handle");
    if (query_tile != 0 && query_tile != 32 && query_tile != 48 && query_tile != 64 && query_tile != 96 && query_tile != 128 && query_tile != 256)
        return set_err(KNN_ERR_INVALID, "set_tuning: query_tile must be 0, 32, 48, 64, 96, 128 or 256");
    std::lock_guard<std::mutex> lk(h->mu);
    h->force_qt = query_tile;
    h->force_chunks = nchunks;
    h->flags = flags & ~KNN_TUNE_PUB_ROUNDS_MASK;
    h->pub_rounds_force = (flags & KNN_TUNE_PUB_ROUNDS_MASK) >> KNN_TUNE_PUB_ROUNDS_SHIFT; // (0: the host's choice)
    return 0;
}

// ---- measurement aid: the box's read rate over the index's own rows -----------------------------------------------
__global__ __launch_bounds__(256) void read_rate_kernel(const f32x4 *__restrict__ p, size_t n4, float *__restrict__ sink)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
    for (; i + 3 * stride < n4; i += 4 * stride) { // four independent 16-byte loads in flight per lane
        const f32x4 a = p[i], b = p[i + stride], c = p[i + 2 * stride], d = p[i + 3 * stride];
        acc += a + b + c + d;
    }
    for (; i < n4; i += stride) acc += p[i];
    if (acc[0] + acc[1] + acc[2] + acc[3] == 12345.678f) *sink = acc[0]; // (keeps the loads alive)
}

extern "C" int knn_flat_read_rate(knn_handle h, int32_t reps, float *best_ms, int64_t *bytes_read)
{
    if (!h || !best_ms || !bytes_read) return set_err(KNN_ERR_INVALID, "read_rate: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (view_is_stale(h)) return set_err(KNN_ERR_INVALID, "read_rate" KNN_STALE_VIEW_MSG);
    if (h->approx16) return set_err(KNN_ERR_UNSUPPORTED, "read_rate: not for an approximate (bf16) index"); // (its scans read the bf16 copies: the fp32 rows' rate bounds nothing)
    HIP_TRY(hipSetDevice(h->device));
    const size_t bytes = (size_t)h->ntotal * h->dp * 4;
    *bytes_read = (int64_t)bytes;
    *best_ms = 0.0f;
    if (!bytes) return 0;
    if (!scratch<int>(h, h->ws_flag, 16, h->stream, "read_rate: out of device memory")) return KNN_ERR_HIP;
    EventList ev; // one pair, recorded again around every launch
    int rc = ev.mark(h->stream);
    if (!rc) rc = ev.mark(h->stream);
    if (rc) return rc;
    const hipEvent_t e0 = ev.ev[0], e1 = ev.ev[1];
    float best = FLT_MAX;
    for (int grid : {2048, 4096, 8192})
        for (int r = 0; r < std::max(1, reps); r++) {
            HIP_TRY(hipEventRecord(e0, h->stream));
            hipLaunchKernelGGL(read_rate_kernel, dim3(grid), dim3(256), 0, h->stream, (const f32x4 *)h->xb, bytes / 16, (float *)h->ws_flag.p + 8);
            HIP_TRY(hipEventRecord(e1, h->stream));
            HIP_TRY(hipEventSynchronize(e1));
            float ms = 0.0f;
            HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
            best = std::min(best, ms);
        }
    *best_ms = best;
    return 0;
}

// ---- measurement aid: the box's fp32 MFMA rate -----------------------------------------------------------------
// every wave issues back-to-back v_mfma_f32_32x32x2_f32 on four independent accumulators, operands in registers, no
// memory traffic: what the matrix pipes of THIS box sustain under load (the chip lowers its clock: the in-kernel clock is
// d(s_memtime) / d(s_memrealtime) x 100 MHz), to set beside the data sheet's 157.3 TFLOP/s
__global__ __launch_bounds__(256) void mfma_rate_kernel(float *out, int iters, unsigned long long *clk)
{
    float x[8], y[8];
    unsigned s0 = (blockIdx.x * 256u + threadIdx.x) * 16u;
    for (int i = 0; i < 16; i++) { // (random operands: constant ones toggle fewer wires and run at a higher clock than real data)
        unsigned s = (s0 + i) * 747796405u + 2891336453u;
        s = ((s >> ((s >> 28) + 4)) ^ s) * 277803737u;
        s = (s >> 22) ^ s;
        const float v = (float)(s & 0xFFFFFF) / 8388608.0f - 1.0f;
        if (i < 8) x[i] = v;
        else y[i - 8] = v;
    }
    const unsigned long long t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
    f32x16 a0 = {}, a1 = {}, a2 = {}, a3 = {};
    for (int i = 0; i < iters; i++) {
#pragma unroll
        for (int u = 0; u < 8; u += 2) {
            a0 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u], y[u], a0, 0, 0, 0);
            a1 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u + 1], y[u], a1, 0, 0, 0);
            a2 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u], y[u + 1], a2, 0, 0, 0);
            a3 = __builtin_amdgcn_mfma_f32_32x32x2f32(x[u + 1], y[u + 1], a3, 0, 0, 0);
        }
    }
    float s = 0.0f;
    for (int r = 0; r < 16; r++) s += a0[r] + a1[r] + a2[r] + a3[r];
    const unsigned long long t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    if (s == 12345.678f) out[0] = s; // (keeps the accumulators alive)
    if (threadIdx.x == 0) {
        clk[2 * blockIdx.x] = t1 - t0;
        clk[2 * blockIdx.x + 1] = r1 - r0;
    }
}

extern "C" int knn_mfma_rate(int32_t warm_ms, float *tflops, float *clock_mhz)
{
    if (!tflops) return set_err(KNN_ERR_INVALID, "mfma_rate: null pointer");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g_device);
    const int grid = 2 * std::max(1, cus), iters = 8000; // (two workgroups per CU: two waves per SIMD, as in the scan)
    // (the stream is declared behind the buffers: it goes first, drained, whichever way the call returns)
    PoolBuf bo(64, g_device), bc((size_t)grid * 16, g_device);
    StreamLease s(g_device);
    EventList ev; // one pair, recorded again around every launch
    if (!bo || !bc || !s || ev.mark(s) || ev.mark(s)) return set_err(KNN_ERR_HIP, "mfma_rate: out of resources");
    float *o = bo.get<float>();
    unsigned long long *c = bc.get<unsigned long long>();
    const hipEvent_t e0 = ev.ev[0], e1 = ev.ev[1];
    // back-to-back launches until warm_ms of them have run (the clock settles under load), then the best of eight
    const double flop = (double)grid * 4 /* waves */ * iters * 16.0 * (32.0 * 32 * 2 * 2);
    float best = FLT_MAX, total = 0.0f;
    double mhz = 0.0;
    std::vector<unsigned long long> hc((size_t)grid * 2);
    int timed = 0;
    for (int r = 0; r < 4000 && timed < 8; r++) {
        hipError_t e = hipEventRecord(e0, s);
        hipLaunchKernelGGL(mfma_rate_kernel, dim3(grid), dim3(256), 0, s, o, iters, c);
        if (e == hipSuccess) e = hipEventRecord(e1, s);
        if (e == hipSuccess) e = hipEventSynchronize(e1);
        float ms = 0.0f;
        if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
        if (e != hipSuccess) return set_err(KNN_ERR_HIP, std::string("mfma_rate: ") + hipGetErrorString(e));
        total += ms;
        if (total < (float)warm_ms) continue;
        timed++;
        if (ms < best) {
            best = ms;
            if (hipMemcpy(hc.data(), c, hc.size() * 8, hipMemcpyDeviceToHost) == hipSuccess) {
                double acc = 0.0;
                for (int b = 0; b < grid; b++) acc += (double)hc[2 * b] / (double)std::max<unsigned long long>(1, hc[2 * b + 1]) * 100.0;
                mhz = acc / grid;
            }
        }
    }
    *tflops = (float)(flop / (best * 1e-3) / 1e12);
    if (clock_mhz) *clock_mhz = (float)mhz;
    return 0;
}

extern "C" int knn_flat_set_batch(knn_handle h, int64_t nq_whole)
{
    if (!h) return set_err(KNN_ERR_INVALID, "null handle");
    if (nq_whole < 0) return set_err(KNN_ERR_INVALID, "set_batch: negative batch size");
    std::lock_guard<std::mutex> lk(h->mu);
    h->batch_hint = nq_whole;
    return 0;
}

// ---- gather distances -------------------------------------------------------
extern "C" int knn_gather_distances(knn_handle h, const float *q_host, int64_t nq, const int64_t *cand_ids,
                                    const int64_t *cand_offsets, float *out_host)
{
    if (!h) return set_err(KNN_ERR_INVALID, "gather_distances: null handle");
    if (nq < 0) return set_err(KNN_ERR_INVALID, "gather_distances: negative nq");
    if (view_is_stale(h)) return set_err(KNN_ERR_INVALID, "gather_distances" KNN_STALE_VIEW_MSG); // (an empty list too: nothing of a stale view is served)
    if (h->approx16) return set_err(KNN_ERR_UNSUPPORTED, "gather_distances: not for an approximate (bf16) index"); // (fp32 scores: not the ones its searches return)
    if (nq == 0) return 0;
    if (!q_host || !cand_offsets) return set_err(KNN_ERR_INVALID, "gather_distances: null pointer");
    const int64_t np = cand_offsets[nq];
    if (np == 0) return 0;
    if (!cand_ids || !out_host) return set_err(KNN_ERR_INVALID, "gather_distances: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    std::vector<int32_t> pq((size_t)np);
    for (int64_t i = 0; i < nq; i++) {
        if (cand_offsets[i + 1] < cand_offsets[i]) return set_err(KNN_ERR_INVALID, "gather_distances: offsets not monotone");
        for (int64_t p = cand_offsets[i]; p < cand_offsets[i + 1]; p++) {
            if (cand_ids[p] < 0 || cand_ids[p] >= h->ntotal) return set_err(KNN_ERR_INVALID, "gather_distances: candidate id out of range");
            pq[(size_t)p] = (int32_t)i;
        }
    }
    hipStream_t s = h->stream;
    const char *oom = "gather_distances: out of device memory";
    float *raw, *q, *qn, *dist;
    int64_t *ids;
    int32_t *owner;
    if (!(raw = scratch_device_wide<float>(h->ws_tmp2, (size_t)nq * h->d, oom)) || !(q = scratch_device_wide<float>(h->ws_q, (size_t)nq * h->dp, oom)) ||
        !(qn = scratch_device_wide<float>(h->ws_qn, (size_t)nq, oom)) || !(ids = scratch_device_wide<int64_t>(h->ws_I, (size_t)np, oom)) ||
        !(owner = scratch_device_wide<int32_t>(h->ws_tmp, (size_t)np, oom)) || !(dist = scratch_device_wide<float>(h->ws_D, (size_t)np, oom)))
        return KNN_ERR_HIP;
    HIP_TRY(hipMemcpyAsync(raw, q_host, (size_t)nq * h->d * 4, hipMemcpyHostToDevice, s));
    int rc = pad_rows_dev(raw, nq, h->d, q, h->dp, s);
    if (rc) return rc;
    rc = norms_dev_impl(q, nq, h->d, h->dp, qn, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(ids, cand_ids, (size_t)np * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(owner, pq.data(), (size_t)np * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pair_distance_kernel, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, s, h->xb, h->yn, q, qn, h->dp, h->metric, np, owner, ids, dist);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out_host, dist, (size_t)np * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

