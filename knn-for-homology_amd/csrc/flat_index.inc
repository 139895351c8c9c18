// flat_index.inc -- the flat index's storage (included by knn355_lib.hip behind host_core.inc): create, view, free, reset,
// move_storage / grow_index, the bf16 and 16/12-bit row copies kept in step with the rows, add, reconstruct.
// ---- index lifecycle ------------------------------------------------------
extern "C" int knn_flat_create(int32_t d, int32_t metric, knn_handle *out)
{
    if (!out) return set_err(KNN_ERR_INVALID, "flat_create: null out");
    if (d <= 0) return set_err(KNN_ERR_INVALID, "flat_create: d must be positive");
    if (metric != KNN_METRIC_INNER_PRODUCT && metric != KNN_METRIC_L2)
        return set_err(KNN_ERR_UNSUPPORTED, "flat_create: metric must be METRIC_INNER_PRODUCT (0) or METRIC_L2 (1)");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    knn_index_s *h = new knn_index_s();
    h->d = d;
    h->dp = round_up(d, 32);
    h->metric = metric;
    h->device = g_device;
#ifdef KNN355_DEV
    if (const char *e = getenv("KNN355_FLAGS")) h->flags = atoi(e); // (developer build only, A/B runs: the tuning flags every index starts with)
#endif
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, g_device) == hipSuccess && cus > 0) h->num_cus = cus;
    }
    if (!(h->stream = g_streams.take(h->device))) {
        delete h;
        return set_err(KNN_ERR_HIP, "flat_create: stream creation failed");
    }
    (void)hipEventCreateWithFlags(&h->done, hipEventDisableTiming); // (without it a growing buffer waits for the whole device)
    *out = h;
    return 0;
}

extern "C" int knn_flat_view(knn_handle parent, knn_handle *out)
{
    if (!parent || !out) return set_err(KNN_ERR_INVALID, "flat_view: null argument");
    std::lock_guard<std::mutex> lk(parent->mu);
    if (parent->approx16) return set_err(KNN_ERR_UNSUPPORTED, "flat_view: not for an approximate (bf16) index");
    if (view_is_stale(parent)) return set_err(KNN_ERR_INVALID, "flat_view" KNN_STALE_VIEW_MSG); // (its xb / yn dangle: a copy of them must not pass for fresh)
    HIP_TRY(hipSetDevice(parent->device));
    knn_index_s *h = new knn_index_s();
    h->flags = parent->flags;
    h->pub_rounds_force = parent->pub_rounds_force;
    h->force_qt = parent->force_qt;
    h->force_chunks = parent->force_chunks;
    h->d = parent->d;
    h->dp = parent->dp;
    h->metric = parent->metric;
    h->device = parent->device;
    h->num_cus = parent->num_cus;
    h->is_view = true;
    h->storage_gen = parent->storage_gen;
    // a view of a live view goes stale together with it: the generation its rows were read at, not today's (the owner may have
    // moved on between the check above and here)
    h->view_gen = parent->is_view ? parent->view_gen : parent->storage_gen->load();
    h->xb = parent->xb;
    h->yn = parent->yn;
    h->ntotal = parent->ntotal;
    h->cap_rows = parent->ntotal;
    h->scan16 = parent->scan16;
    h->dp16 = parent->dp16;
    h->s16_fmt = parent->s16_fmt;
    h->s16_rows = parent->s16_rows;
    h->s16_exp = parent->s16_exp;
    h->s16_stat = parent->s16_stat;
    h->s16_ok = parent->s16_ok;
    h->s16_note = parent->s16_note;
    if (!(h->stream = g_streams.take(h->device))) {
        delete h;
        return set_err(KNN_ERR_HIP, "flat_view: stream creation failed");
    }
    (void)hipEventCreateWithFlags(&h->done, hipEventDisableTiming);
    *out = h;
    return 0;
}

static void free_index_buffers(knn_index_s *h)
{
    if (!h->is_view) h->storage_gen->fetch_add(1);
    if (h->xb && !h->is_view) g_pool.give(h->xb, h->xb_bytes, h->device);
    if (h->yn && !h->is_view) g_pool.give(h->yn, h->yn_bytes, h->device);
    if (!h->is_view) {
        h->s16_rows_buf.release();
        h->s16_exp_buf.release();
        h->s16_stat_buf.release();
        if (h->scan16 == 2) h->scan16 = 1; // (dropped copies are tried again from the next add on)
    }
    h->s16_rows = nullptr;
    h->s16_exp = nullptr;
    h->s16_stat = nullptr;
    if (!h->is_view) h->s16_ok->store(false);
    h->xb = nullptr;
    h->yn = nullptr;
    h->ntotal = 0;
    h->cap_rows = 0;
}

extern "C" void knn_free(knn_handle h)
{
    if (!h) return;
    if (hipSetDevice(h->device) == hipSuccess) {
        if (h->stream) (void)hipStreamSynchronize(h->stream);
        if (!h->is_view && h->xb) (void)hipDeviceSynchronize(); // a view's stream may still be scanning these rows
        free_index_buffers(h);
        DevBuf *bufs[] = {&h->xb16, &h->ws_q16, &h->ws_sym, &h->ws_qdiff, &h->ws_defer, &h->ws_turn, &h->ws_flag, &h->ws_q, &h->ws_qn, &h->ws_lists, &h->ws_D, &h->ws_I, &h->ws_tmp, &h->ws_tmp2, &h->ws_D1, &h->ws_I1, &h->ws_tmp3,
                          &h->ws_rq, &h->ws_rqn, &h->ws_rcnt, &h->ws_rsegD, &h->ws_rsegI, &h->ws_roff, &h->ws_routD, &h->ws_routI, &h->ws_rsel, &h->ws_rq2, &h->ws_rexp,
                          &h->ws_q16x, &h->ws_s16q, &h->ws_s16ak, &h->ws_s16ok, &h->ws_s16stat,
                          &h->ws_rfq, &h->ws_rfqp, &h->ws_rfI, &h->ws_rfkeys, &h->ws_rfD, &h->ws_rfI2};
        for (DevBuf *b : bufs) b->release();
        for (LevelBufs &b : h->ws_level) {
            b.qlist.release();
            b.qcnt.release();
            b.gthr.release();
            b.qthr.release();
            b.pub.release();
            b.arrive.release();
            b.pair_ctr.release();
        }
        for (int i = 0; i < knn_index_s::RING; i++) {
            if (h->ring0[i]) (void)hipEventDestroy(h->ring0[i]);
            if (h->ring1[i]) (void)hipEventDestroy(h->ring1[i]);
        }
        if (h->stream) g_streams.give(h->device, h->stream); // (synchronised above)
        if (h->flag_host) (void)hipHostFree(h->flag_host);
        if (h->done) (void)hipEventDestroy(h->done);
    }
    delete h;
}

extern "C" int64_t knn_ntotal(knn_handle h) { return h ? h->ntotal : -1; }
extern "C" int32_t knn_dim(knn_handle h) { return h ? h->d : -1; }
extern "C" int32_t knn_metric(knn_handle h) { return h ? h->metric : -1; }
extern "C" int32_t knn_device_of(knn_handle h) { return h ? h->device : -1; }

extern "C" int knn_reset(knn_handle h)
{
    if (!h) return set_err(KNN_ERR_INVALID, "reset: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->is_view) return set_err(KNN_ERR_INVALID, "reset: a view is read-only");
    HIP_TRY(hipSetDevice(h->device));
    free_index_buffers(h);
    return 0;
}

// The handle's rows move to fresh storage of new_cap rows (> cap_rows; the caller holds h->mu and has set the device): the
// common tail of grow_index and knn_flat_reserve.  A failure leaves the handle as it was, and the new buffers go back.
static int move_storage(knn_index_s *h, int64_t new_cap, const char *who)
{
    const size_t row_bytes = (size_t)h->dp * 4;
    PoolBuf bxb((size_t)new_cap * row_bytes, h->device);
    if (!bxb) return set_err(KNN_ERR_HIP, std::string(who) + ": out of device memory");
    PoolBuf byn(((size_t)new_cap + 64) * 4, h->device);
    if (!byn) return set_err(KNN_ERR_HIP, std::string(who) + ": out of device memory");
    float *nxb = bxb.get<float>(), *nyn = byn.get<float>();
    auto copy = [&]() -> int {
        HIP_TRY(hipMemcpyAsync(nxb, h->xb, (size_t)h->ntotal * row_bytes, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(nyn, h->yn, (size_t)h->ntotal * 4, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return 0;
    };
    if (h->ntotal > 0)
        if (int rc = copy()) {
            (void)hipStreamSynchronize(h->stream); // (a copy already queued writes a buffer that goes back to the pool)
            return rc;
        }
    if (h->xb) {
        h->storage_gen->fetch_add(1); // views of the old storage are dead
        (void)hipDeviceSynchronize(); // ... and nothing may still be scanning it
        g_pool.give(h->xb, h->xb_bytes, h->device);
    }
    if (h->yn) g_pool.give(h->yn, h->yn_bytes, h->device);
    h->xb = (float *)bxb.release(&h->xb_bytes);
    h->yn = (float *)byn.release(&h->yn_bytes);
    h->cap_rows = new_cap;
    return 0;
}

static int grow_index(knn_index_s *h, int64_t need_rows)
{
    if (need_rows <= h->cap_rows) return 0;
    int64_t new_cap = std::max<int64_t>(need_rows, h->cap_rows + h->cap_rows / 2);
    if (h->cap_rows == 0) new_cap = need_rows; // first add: exact fit (the reference adds once)
    int rc = move_storage(h, new_cap, "add");
    if (rc && new_cap > need_rows) rc = move_storage(h, need_rows, "add"); // (the guess was too large: the exact fit)
    return rc;
}

// bf16 copies of rows [r0, r0 + n) of an approximate index (kept beside the fp32 rows: reconstruct, norms and the
// exact re-scoring use those)
static int approx16_sync_rows(knn_index_s *h, int64_t r0, int64_t n, hipStream_t s)
{
    if (!(h->approx16 || h->keep16) || n <= 0) return 0;
    const size_t need = (size_t)h->cap_rows * h->dp * 2;
    if (h->xb16.bytes < need) {
        // (regrown with the fp32 storage: convert everything that is there)
        if (h->xb16.ensure(need)) return set_err(KNN_ERR_HIP, "add: out of device memory (bf16 rows)");
        n += r0;
        r0 = 0;
    }
    const int64_t total = n * h->dp;
    const unsigned grid = (unsigned)std::min<int64_t>((total / 4 + 255) / 256, 65535);
    hipLaunchKernelGGL(to_bf16_kernel, dim3(grid), dim3(256), 0, s, h->xb + (size_t)r0 * h->dp, total, (__bf16 *)h->xb16.p + (size_t)r0 * h->dp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// fp16 copies of rows [r0, r0 + n) for the exact 16-bit prefilter (DESIGN 4.9).  Storage that has to grow is rebuilt from all
// rows, and r0 = 0 restarts the index-wide statistics.  Copies that cannot be allocated are dropped: the index goes on with its
// fp32 scans.  Waits for the stream (adds are synchronous): whether every row is finite decides whether searches may use them.
// Called with n = 0 by knn_flat_reserve: the copies grow with the fp32 rows.  Copies that move (or are dropped) make every
// view of the index stale, as moved fp32 rows do: a view holds their addresses.
static int scan16_sync_rows(knn_index_s *h, int64_t r0, int64_t n, hipStream_t s)
{
    if (h->scan16 != 1 || h->is_view) return 0;
    // (12-bit copies: whole tiles of 256 rows, 1.5 bytes per value)
    const size_t need = h->s16_fmt == 12 ? (size_t)((h->cap_rows + 255) / 256) * (h->dp16 / 64) * 24576 : (size_t)h->cap_rows * h->dp16 * 2;
    if (h->cap_rows > 0 && (h->s16_rows_buf.bytes < need || h->s16_exp_buf.bytes < (size_t)h->cap_rows || !h->s16_stat_buf.p)) {
        HIP_TRY(hipStreamSynchronize(s));
        if (h->s16_rows_buf.p || h->s16_exp_buf.p) {
            h->storage_gen->fetch_add(1); // (views of the old copies are dead ...)
            (void)hipDeviceSynchronize(); // (... and nothing may still be scanning them: ensure() below hands them back to the pool)
        }
        if (h->s16_rows_buf.ensure(need) || h->s16_exp_buf.ensure((size_t)h->cap_rows) || h->s16_stat_buf.ensure(S16_NSTAT * 4)) {
            h->s16_rows_buf.release();
            h->s16_exp_buf.release();
            h->s16_stat_buf.release();
            h->s16_rows = nullptr;
            h->s16_exp = nullptr;
            h->s16_stat = nullptr;
            h->s16_ok->store(false);
            h->scan16 = 2;
            h->s16_note = "dropped: no device memory for the row copies";
            return 0;
        }
        n += r0;
        r0 = 0;
    }
    if (n <= 0) return 0;
    h->s16_rows = (const _Float16 *)h->s16_rows_buf.p;
    h->s16_exp = (const int8_t *)h->s16_exp_buf.p;
    h->s16_stat = (const uint32_t *)h->s16_stat_buf.p;
    uint32_t init[S16_NSTAT] = {0u, 0u, 0u, 0x80000000u, 0u, 0u, 0u, 0u}; // (largest exponent: INT_MIN)
    if (r0 == 0) HIP_TRY(hipMemcpyAsync(h->s16_stat_buf.p, init, sizeof init, hipMemcpyHostToDevice, s));
    if (h->s16_fmt == 12)
        hipLaunchKernelGGL(scan12_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, h->xb, h->dp, r0, n, h->dp16,
                           (uint8_t *)h->s16_rows_buf.p, (int8_t *)h->s16_exp_buf.p, (uint32_t *)h->s16_stat_buf.p);
    else
        hipLaunchKernelGGL(scan16_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s, h->xb, h->dp, r0, n, h->dp16,
                           (_Float16 *)h->s16_rows_buf.p, (int8_t *)h->s16_exp_buf.p, (uint32_t *)h->s16_stat_buf.p);
    HIP_TRY(hipGetLastError());
    uint32_t nonfinite = 0;
    HIP_TRY(hipMemcpyAsync(&nonfinite, (const uint32_t *)h->s16_stat_buf.p + S16_NONFINITE, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    h->s16_ok->store(nonfinite == 0);
    h->s16_note = nonfinite ? "off: a row holds a value that is not finite" : "on";
    return 0;
}

// before the first add and before knn_flat_reserve: the index multiplies bf16 copies (rows padded to a multiple of 64 values).
// The row stride changes, so storage that was sized with the old one (reserve on an empty index) must not exist.
static int flat_set_approx16(knn_index_s *h)
{
    if (h->ntotal != 0) return set_err(KNN_ERR_INVALID, "approx16: the index already holds rows");
    if (h->cap_rows != 0 || h->xb) return set_err(KNN_ERR_INVALID, "approx16: the index already has storage (knn_flat_reserve): set it first, or knn_reset");
    if (h->scan16) return set_err(KNN_ERR_UNSUPPORTED, "approx16: the index keeps fp16 copies for the 16-bit prefilter");
    if (h->keep16) return set_err(KNN_ERR_UNSUPPORTED, "approx16: not for an index that keeps bf16 copies (HNSW)");
    h->approx16 = true;
    h->dp = round_up(h->d, 64);
    return 0;
}

// the same for a caller's index: the way in for the tests of the bf16 builds (include/knn355.h)
extern "C" int knn_flat_set_approx16(knn_handle h)
{
    if (!h) return set_err(KNN_ERR_INVALID, "set_approx16: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->is_view) return set_err(KNN_ERR_INVALID, "set_approx16: a view uses its parent's rows");
    return flat_set_approx16(h);
}

// before the first add: bf16 copies of the rows are kept (the scans do not use them)
static int flat_keep16(knn_index_s *h)
{
    if (h->ntotal != 0) return set_err(KNN_ERR_INVALID, "keep16: the index already holds rows");
    if (h->scan16) return set_err(KNN_ERR_UNSUPPORTED, "keep16: the index keeps fp16 copies for the 16-bit prefilter");
    h->keep16 = true;
    return 0;
}

// appends rows that already live on the device ([n][d], contiguous)
static int add_dev_impl(knn_index_s *h, const float *x_dev, int64_t n, hipStream_t s)
{
    float *dst = h->xb + (size_t)h->ntotal * h->dp;
    if (h->dp == h->d) {
        HIP_TRY(hipMemcpyAsync(dst, x_dev, (size_t)n * h->d * 4, hipMemcpyDeviceToDevice, s));
    } else {
        int rc = pad_rows_dev(x_dev, n, h->d, dst, h->dp, s);
        if (rc) return rc;
    }
    // norms are kept for both metrics: reconstruct/HNSW-L2 need them and they cost one pass
    int rc = norms_dev_impl(dst, n, h->d, h->dp, h->yn + h->ntotal, s);
    if (rc) return rc;
    rc = approx16_sync_rows(h, h->ntotal, n, s);
    if (rc) return rc;
    rc = scan16_sync_rows(h, h->ntotal, n, s);
    if (rc) return rc;
    h->ntotal += n;
    return 0;
}

extern "C" int knn_flat_add_dev(knn_handle h, const float *x_dev, int64_t n, void *stream)
{
    if (!h) return set_err(KNN_ERR_INVALID, "add: null handle");
    if (n < 0) return set_err(KNN_ERR_INVALID, "add: negative n");
    if (n == 0) return 0;
    if (!x_dev) return set_err(KNN_ERR_INVALID, "add: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->is_view) return set_err(KNN_ERR_INVALID, "add: a view is read-only");
    HIP_TRY(hipSetDevice(h->device));
    if (h->ntotal + n > 0xFFFFFFF0ll) return set_err(KNN_ERR_UNSUPPORTED, "add: more than 2^32 rows per index");
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    if (stream) HIP_TRY(hipStreamSynchronize(h->stream));
    int rc = grow_index(h, h->ntotal + n);
    if (rc) return rc;
    rc = add_dev_impl(h, x_dev, n, s);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

extern "C" int knn_flat_add(knn_handle h, const float *x_host, int64_t n)
{
    if (!h) return set_err(KNN_ERR_INVALID, "add: null handle");
    if (n < 0) return set_err(KNN_ERR_INVALID, "add: negative n");
    if (n == 0) return 0;
    if (!x_host) return set_err(KNN_ERR_INVALID, "add: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->is_view) return set_err(KNN_ERR_INVALID, "add: a view is read-only");
    HIP_TRY(hipSetDevice(h->device));
    if (h->ntotal + n > 0xFFFFFFF0ll) return set_err(KNN_ERR_UNSUPPORTED, "add: more than 2^32 rows per index");
    int rc = grow_index(h, h->ntotal + n);
    if (rc) return rc;
    if (h->dp == h->d) {
        float *dst = h->xb + (size_t)h->ntotal * h->dp;
        HIP_TRY(hipMemcpy(dst, x_host, (size_t)n * h->d * 4, hipMemcpyHostToDevice));
        rc = norms_dev_impl(dst, n, h->d, h->dp, h->yn + h->ntotal, h->stream);
        if (rc) return rc;
        rc = approx16_sync_rows(h, h->ntotal, n, h->stream);
        if (rc) return rc;
        rc = scan16_sync_rows(h, h->ntotal, n, h->stream);
        if (rc) return rc;
        h->ntotal += n;
    } else {
        const int64_t rows_per = std::max<int64_t>(1, (int64_t)(256ull << 20) / ((int64_t)h->d * 4));
        if (h->ws_tmp.ensure((size_t)std::min(n, rows_per) * h->d * 4)) return set_err(KNN_ERR_HIP, "add: out of device memory");
        for (int64_t i0 = 0; i0 < n; i0 += rows_per) {
            int64_t m = std::min(rows_per, n - i0);
            HIP_TRY(hipMemcpy(h->ws_tmp.p, x_host + i0 * h->d, (size_t)m * h->d * 4, hipMemcpyHostToDevice));
            rc = add_dev_impl(h, (const float *)h->ws_tmp.p, m, h->stream);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

extern "C" int knn_flat_reconstruct(knn_handle h, int64_t i0, int64_t n, float *out_host)
{
    if (!h) return set_err(KNN_ERR_INVALID, "reconstruct: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (view_is_stale(h)) return set_err(KNN_ERR_INVALID, "reconstruct" KNN_STALE_VIEW_MSG);
    if (i0 < 0 || n < 0 || i0 + n > h->ntotal) return set_err(KNN_ERR_INVALID, "reconstruct: range out of bounds");
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy2D(out_host, (size_t)h->d * 4, h->xb + (size_t)i0 * h->dp, (size_t)h->dp * 4, (size_t)h->d * 4,
                        (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

