// hnsw_search.inc -- HNSW search: queries up, hnsw_beam_pipeline (hnsw_build.inc), results down; host walkers where the
// device beam does not serve.

// Search on the device: queries up, the pipeline above, results down.
static int hnsw_search_device(knn_hnsw_s *H, const float *q_host, int64_t nq, int64_t k, int ef, float *D_host, int64_t *I_host)
{
    knn_index_s *f = H->flat;
    int rc = 0;
    if (H->nbr0_dirty || H->mirror_count != H->linked_count) {
        rc = hnsw_upload_graph(H);
        if (rc) return rc;
    }
    const int64_t B = 16384;
    const int64_t mb = std::min(nq, B);
    const int64_t nbatches = (nq + B - 1) / B;
    // Several batches: two sets of result buffers, and while batch b is walked the results of batch b - 1 go down on the
    // device's copy stream (ResultPipe; the reference's run, all-vs-all k = 1000: 200 MB per batch -- an eighth of the
    // batch's time when it waited its turn on the search's own stream)
    PipeLease lease;
    rc = lease_pipes(f->device, nbatches > 1, lease);
    if (rc) return rc;
    const bool piped = lease.cp != nullptr;
    DevBuf *dD[2] = {&H->d_D, &H->d_D2}, *dI[2] = {&H->d_I, &H->d_I2};
    const char *oom_what = "hnsw_search: out of device memory";
    int oom = hnsw_grow(oom_what, H->d_q, (size_t)mb * f->dp * 4, H->d_qn, (size_t)mb * 4, f->ws_tmp2, (size_t)mb * f->d * 4,
                        H->d_D, (size_t)mb * k * 4, H->d_I, (size_t)mb * k * 8, H->d_st2, 64);
    if (!oom && piped) oom = hnsw_grow(oom_what, H->d_D2, (size_t)mb * k * 4, H->d_I2, (size_t)mb * k * 8);
    if (oom) return oom;
    hipStream_t s = f->stream;
    const ResultPipe rp{lease.cp, s, "hnsw_search: "};
    std::vector<unsigned long long> st((size_t)nbatches * 2, 0ull);
    // batch b: queries up, the pipeline above into the result buffers of `slot`, the walk's counters kept beside them
    auto walk = [&](int64_t b, int slot) -> int {
        const int64_t b0 = b * B, m = std::min(B, nq - b0);
        int r = rp.hip(hipMemcpyAsync(f->ws_tmp2.p, q_host + b0 * f->d, (size_t)m * f->d * 4, hipMemcpyHostToDevice, s));
        if (!r) r = pad_rows_dev((const float *)f->ws_tmp2.p, m, f->d, (float *)H->d_q.p, f->dp, s);
        if (!r) r = norms_dev_impl((const float *)H->d_q.p, m, f->d, f->dp, (float *)H->d_qn.p, s);
        if (!r)
            r = hnsw_beam_pipeline(H, (const float *)H->d_q.p, (const float *)f->ws_tmp2.p, (const float *)H->d_qn.p, m, ef, (int)k,
                                   (float *)dD[slot]->p, (int64_t *)dI[slot]->p, nullptr, s);
        if (!r) r = rp.hip(hipMemcpyAsync((char *)H->d_st2.p + slot * 16, H->d_stats.p, 16, hipMemcpyDeviceToDevice, s));
        return r;
    };
    // results (and the walk's counters) of batch b: device -> host, on `on`
    auto copy = [&](int64_t b, int slot, hipStream_t on) -> hipError_t {
        const int64_t b0 = b * B, m = std::min(B, nq - b0);
        hipError_t r = hipMemcpyAsync(D_host + b0 * k, dD[slot]->p, (size_t)m * k * 4, hipMemcpyDeviceToHost, on);
        if (r == hipSuccess) r = hipMemcpyAsync(I_host + b0 * k, dI[slot]->p, (size_t)m * k * 8, hipMemcpyDeviceToHost, on);
        if (r == hipSuccess) r = hipMemcpyAsync(&st[(size_t)b * 2], (const char *)H->d_st2.p + slot * 16, 16, hipMemcpyDeviceToHost, on);
        return r;
    };
    for (int64_t b = 0; b < nbatches && !rc; b++) {
        rc = rp.before(b);
        if (!rc) rc = walk(b, rp.slot(b));
        if (!rc) rc = rp.after(b, copy);
    }
    rc = rp.finish(rc, nbatches, copy);
    if (rc) return rc;
    for (int64_t b = 0; b < nbatches; b++) {
        H->stat_pairs += (int64_t)st[(size_t)b * 2];
        H->stat_rounds += 1;
        H->stat_expansions += (int64_t)st[(size_t)b * 2 + 1];
    }
    return 0;
}

extern "C" int knn_hnsw_search(knn_hnsw_s *H, const float *q_host, int64_t nq, int64_t k, float *D_host, int64_t *I_host)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_search: null handle");
    if (nq < 0 || k < 1) return set_err(KNN_ERR_INVALID, "hnsw_search: bad shape");
    if (nq == 0) return 0;
    if (!q_host || !D_host || !I_host) return set_err(KNN_ERR_INVALID, "hnsw_search: null pointer");
    std::lock_guard<std::mutex> lk(H->mu);
    knn_index_s *f = H->flat;
    HIP_TRY(hipSetDevice(f->device));
    const float pad = f->metric == KNN_METRIC_INNER_PRODUCT ? -FLT_MAX : FLT_MAX;
    const int ef = (int)std::max<int64_t>(H->efSearch, k);
    if (H->g.ntotal() == 0) {
        fill_empty_host(D_host, I_host, nq * k, f->metric);
        return 0;
    }
    // the device beam serves rows of up to 1024 floats, beams of up to 1024 entries and 2^31 rows
    static const bool host_beam = hnsw_env_int("KNN355_HNSW_HOST_BEAM", 0) != 0; // (once per process; the construction reads it for every batch)
    if (H->device_beam && !host_beam && f->dp <= 1024 && ef <= 1024 && k <= KNN_MAX_K && H->g.ntotal() < (1ll << 31))
        return hnsw_search_device(H, q_host, nq, k, ef, D_host, I_host);
    if (H->host0_stale) { // (the host walkers read level 0)
        int rc0 = hnsw_host0_sync(H);
        if (rc0) return rc0;
    }
    const int64_t B = H->max_batch;
    if (int oom = hnsw_grow("hnsw_search: out of device memory", H->d_q, (size_t)std::min(nq, B) * f->dp * 4,
                            H->d_qn, (size_t)std::min(nq, B) * 4, f->ws_tmp2, (size_t)std::min(nq, B) * f->d * 4)) return oom;
    for (int64_t b0 = 0; b0 < nq; b0 += B) {
        const int64_t m = std::min(B, nq - b0);
        hipStream_t s = f->stream;
        HIP_TRY(hipMemcpyAsync(f->ws_tmp2.p, q_host + b0 * f->d, (size_t)m * f->d * 4, hipMemcpyHostToDevice, s));
        int rc = pad_rows_dev((const float *)f->ws_tmp2.p, m, f->d, (float *)H->d_q.p, f->dp, s);
        if (rc) return rc;
        rc = norms_dev_impl((const float *)H->d_q.p, m, f->d, f->dp, (float *)H->d_qn.p, s);
        if (rc) return rc;
        std::vector<Walker> ws((size_t)m);
        for (int64_t i = 0; i < m; i++) {
            ws[i].qslot = (uint32_t)i;
            ws[i].ef = ef;
            ws[i].greedy_until = 0;
            ws[i].stop_level = 0;
        }
        rc = hnsw_walk(H, ws, (const float *)H->d_q.p, (const float *)H->d_qn.p, false);
        if (rc) return rc;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t i = 0; i < m; i++) {
            const auto &W = ws[i].W; // sorted ascending by (v, id)
            float *Dq = D_host + (b0 + i) * k;
            int64_t *Iq = I_host + (b0 + i) * k;
            for (int64_t j = 0; j < k; j++) {
                if (j < (int64_t)W.size()) {
                    Dq[j] = f->metric == KNN_METRIC_INNER_PRODUCT ? -W[j].first : W[j].first;
                    Iq[j] = W[j].second;
                } else {
                    Dq[j] = pad;
                    Iq[j] = -1;
                }
            }
        }
    }
    return 0;
}
