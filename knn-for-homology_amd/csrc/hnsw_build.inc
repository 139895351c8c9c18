// hnsw_build.inc -- HNSW construction: the host walkers, the pruning launches, the device mirror of level 0, the device
// pipeline that search and construction share (hnsw_beam_pipeline: it stands here because the level-0 candidates call it),
// the candidates of every level, a batch's links, the add entries.  Defined in the order of use: no forward declarations.

// Lock-step walk of all walkers over the frozen graph.  xa/an: the walkers' vectors on the
// device (row = Walker::qslot).  For searches level_cands stays empty and W holds the result.
// The walkers run in two halves: while the GPU computes the distances one half asked for, the
// host consumes the other half's results and collects its next proposals (walkers are independent,
// so the split changes nothing in what each of them visits).
static int hnsw_walk(knn_hnsw_s *H, std::vector<Walker> &ws, const float *xa, const float *an, bool keep_levels)
{
    const HnswGraph &g = H->g;
    if (g.entry < 0) {
        for (auto &w : ws) w.phase = 3;
        return 0;
    }
    knn_index_s *f = H->flat;
    const int nw = (int)ws.size();
    const int nt = nw >= 128 ? hnsw_threads() : 1;
    (void)nt; // (only the host pass sees the OpenMP pragmas that use it)
    const bool use_bitmap = (size_t)nw * ((size_t)g.ntotal() / 8 + 8) <= (256ull << 20);
    std::vector<std::vector<uint32_t>> props(nw);
    const int nhalves = nw >= 512 ? 2 : 1;
    if (nhalves == 2 && !H->stream2) HIP_TRY(hipStreamCreateWithFlags(&H->stream2, hipStreamNonBlocking));
    for (auto &e : H->ev_pairs)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    struct Half {
        int lo, hi;
        DevBuf *d_pa, *d_pb, *d_out;
        PinnedBuf *h_pa, *h_pb, *h_out;
        hipStream_t stream;
        hipEvent_t done;
        bool active = true;
        size_t total = 0;
    } halves[2] = {{0, nhalves == 2 ? nw / 2 : nw, &H->d_pa, &H->d_pb, &H->d_out, &H->h_pa, &H->h_pb, &H->h_out, f->stream, H->ev_pairs[0]},
                   {nw / 2, nw, &H->d_pa2, &H->d_pb2, &H->d_out2, &H->h_pa2, &H->h_pb2, &H->h_out2, H->stream2, H->ev_pairs[1]}};

    // proposals of one half, staged in its pinned buffers; returns -1 on error, 0 if the half is done
    auto propose = [&](Half &hf) -> int {
        const int lo = hf.lo, hi = hf.hi;
        double th0 = now_s();
        // 1. proposals
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt)
        for (int i = lo; i < hi; i++) {
            Walker &w = ws[i];
            std::vector<uint32_t> &pr = props[i];
            pr.clear();
            if (w.phase == 3) continue;
            if (w.phase == 0) {
                pr.push_back((uint32_t)g.entry);
            } else if (w.phase == 1) {
                const uint32_t *l = g.list(w.cur, w.level);
                const int nn = g.nb_neighbors(w.level);
                for (int j = 0; j < nn && l[j] != HNSW_EMPTY; j++) pr.push_back(l[j]);
                if (pr.empty()) { // isolated at this level: drop a level right away
                    // handled in the consume step with an empty result
                }
            } else {
                // beam: expand up to `expand` of the closest open candidates per round (fewer
                // lock-step rounds for a few extra distances); keep popping while nothing
                // unvisited showed up
                int expanded = 0;
                while (expanded < H->expand || pr.empty()) {
                    if (w.C.empty()) break;
                    expanded++;
                    std::pop_heap(w.C.begin(), w.C.end(), std::greater<DistId>());
                    DistId c = w.C.back();
                    w.C.pop_back();
                    if ((int)w.W.size() >= w.ef && c > w.W.front()) {
                        w.C.clear();
                        break;
                    }
                    const uint32_t *l = g.list(c.second, w.level);
                    const int nn = g.nb_neighbors(w.level);
                    for (int j = 0; j < nn && l[j] != HNSW_EMPTY; j++)
                        if (w.vis.insert(l[j])) pr.push_back(l[j]);
                }
            }
        }
        size_t total = 0;
        bool any_active = false;
        for (int i = lo; i < hi; i++) {
            ws[i].prop_off = total;
            ws[i].prop_n = props[i].size();
            total += props[i].size();
            if (ws[i].phase != 3) any_active = true;
        }
        hf.total = total;
        if (!any_active) {
            H->stat_host_s += now_s() - th0;
            return 0;
        }
        if (hnsw_grow("hnsw: out of pinned host memory", *hf.h_pa, total * 4 + 64, *hf.h_pb, total * 4 + 64, *hf.h_out, total * 4 + 64)) return -1;
        uint32_t *pa = (uint32_t *)hf.h_pa->p, *pb = (uint32_t *)hf.h_pb->p;
#pragma omp parallel for schedule(static) num_threads(nt)
        for (int i = lo; i < hi; i++) {
            const Walker &w = ws[i];
            for (size_t j = 0; j < w.prop_n; j++) {
                pa[w.prop_off + j] = w.qslot;
                pb[w.prop_off + j] = props[i][j];
            }
        }
        H->stat_host_s += now_s() - th0;
        return 1;
    };
    // distances of the staged pairs, asynchronously on the half's stream
    auto launch = [&](Half &hf) -> int {
        const int64_t np = (int64_t)hf.total;
        hipStream_t s = hf.stream;
        if (np > 0) {
            if (int oom = hnsw_grow("hnsw: out of device memory", *hf.d_pa, (size_t)np * 4, *hf.d_pb, (size_t)np * 4,
                                    *hf.d_out, (size_t)np * 4)) return oom;
            HIP_TRY(hipMemcpyAsync(hf.d_pa->p, hf.h_pa->p, (size_t)np * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(hf.d_pb->p, hf.h_pb->p, (size_t)np * 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(pair_v_kernel, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, s, xa, an, f->xb, f->yn, f->dp, f->metric, np,
                               (const uint32_t *)hf.d_pa->p, (const uint32_t *)hf.d_pb->p, (float *)hf.d_out->p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(hf.h_out->p, hf.d_out->p, (size_t)np * 4, hipMemcpyDeviceToHost, s));
            H->stat_pairs += np;
        }
        HIP_TRY(hipEventRecord(hf.done, s));
        H->stat_rounds++;
        return 0;
    };
    auto consume = [&](Half &hf) {
        const int lo = hf.lo, hi = hf.hi;
        const float *out = (const float *)hf.h_out->p;
        double th0 = now_s();
        // 4. consume
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt)
        for (int i = lo; i < hi; i++) {
            Walker &w = ws[i];
            if (w.phase == 3) continue;
            const float *d = out + w.prop_off;
            const std::vector<uint32_t> &pr = props[i];
            auto start_beam = [&]() {
                if (w.descent_only) {
                    w.phase = 3;
                    return;
                }
                w.phase = 2;
                w.C.clear();
                w.W.clear();
                w.vis.reset((size_t)w.ef * 8, (size_t)g.ntotal(), use_bitmap);
                w.vis.insert(w.cur);
                w.C.push_back(DistId(w.cur_d, w.cur));
                w.W.push_back(DistId(w.cur_d, w.cur));
            };
            auto after_descent_step = [&]() {
                // called when no improvement at w.level
                if (w.level > w.greedy_until) {
                    w.level--;
                    if (w.level > w.greedy_until) return; // keep descending greedily
                }
                // w.level == greedy_until: beam search starts here
                start_beam();
            };
            if (w.phase == 0) {
                w.cur = (uint32_t)g.entry;
                w.cur_d = d[0];
                w.level = g.max_level;
                if (w.level > w.greedy_until) w.phase = 1;
                else { w.level = std::min(w.level, w.greedy_until); start_beam(); }
            } else if (w.phase == 1) {
                bool improved = false;
                for (size_t j = 0; j < pr.size(); j++) {
                    if (DistId(d[j], pr[j]) < DistId(w.cur_d, w.cur)) {
                        w.cur_d = d[j];
                        w.cur = pr[j];
                        improved = true;
                    }
                }
                if (!improved) after_descent_step();
            } else {
                for (size_t j = 0; j < pr.size(); j++) {
                    DistId e(d[j], pr[j]);
                    if ((int)w.W.size() < w.ef || e < w.W.front()) {
                        w.C.push_back(e);
                        std::push_heap(w.C.begin(), w.C.end(), std::greater<DistId>());
                        if ((int)w.W.size() < w.ef) {
                            w.W.push_back(e);
                            std::push_heap(w.W.begin(), w.W.end());
                        } else {
                            heap_replace_top(w.W, e); // e < current maximum: one sift-down instead of push + pop
                        }
                    }
                }
                if (w.C.empty() && pr.empty()) {
                    // beam at this level finished
                    std::sort(w.W.begin(), w.W.end());
                    if (keep_levels) {
                        if ((int)w.level_cands.size() <= w.level) w.level_cands.resize(w.level + 1);
                        w.level_cands[w.level] = w.W;
                    }
                    if (w.level > w.stop_level) {
                        // next level down starts from the closest point found here
                        w.cur = w.W[0].second;
                        w.cur_d = w.W[0].first;
                        w.level--;
                        start_beam();
                    } else {
                        w.phase = 3;
                    }
                }
            }
        }
        H->stat_host_s += now_s() - th0;
    };

    // the walkers' vectors (xa) may have been produced on f->stream: the second stream starts after it
    if (nhalves == 2) {
        HIP_TRY(hipEventRecord(H->ev_pairs[1], f->stream));
        HIP_TRY(hipStreamWaitEvent(H->stream2, H->ev_pairs[1], 0));
    }
    for (int h = 0; h < nhalves; h++) {
        int r = propose(halves[h]);
        if (r < 0) return KNN_ERR_HIP;
        halves[h].active = r > 0;
        if (halves[h].active) {
            int rc = launch(halves[h]);
            if (rc) return rc;
        }
    }
    for (;;) {
        bool any = false;
        for (int h = 0; h < nhalves; h++) {
            Half &hf = halves[h];
            if (!hf.active) continue;
            any = true;
            double tg0 = now_s();
            HIP_TRY(hipEventSynchronize(hf.done));
            H->stat_gpu_s += now_s() - tg0; // time the host actually waited for the GPU
            consume(hf);
            int r = propose(hf);
            if (r < 0) return KNN_ERR_HIP;
            hf.active = r > 0;
            if (hf.active) {
                int rc = launch(hf);
                if (rc) return rc;
            }
        }
        if (!any) break;
    }
    if (nhalves == 2) HIP_TRY(hipStreamSynchronize(H->stream2));
    return 0;
}

// one workgroup per group; nr: the largest group's members rounded up to 64, 96 or 128
template <int NR>
static int launch_shrink_nr(const ShrinkParams &p, int grid, hipStream_t s)
{
    const size_t lds = std::max((size_t)2 * NR * 128, (size_t)NR * (NR + 1) * 4) + (size_t)NR * 16;
    HIP_TRY(hipFuncSetAttribute((const void *)gram_shrink_kernel<NR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(gram_shrink_kernel<NR>, dim3((unsigned)grid), dim3(256), lds, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int launch_shrink(const ShrinkParams &p, int grid, int max_members, hipStream_t s)
{
    if (grid <= 0) return 0;
    if (max_members <= 64) return launch_shrink_nr<64>(p, grid, s);
    if (max_members <= 96) return launch_shrink_nr<96>(p, grid, s);
    return launch_shrink_nr<128>(p, grid, s);
}

// runs the pruning heuristic on the GPU for `ngroups` groups staged in h_goff/h_mem/h_maxo (max_members: the largest group)
static int hnsw_run_shrink(knn_hnsw_s *H, int ngroups, size_t nmembers, int out_stride, int max_members = SHRINK_MAX_MEMBERS)
{
    if (ngroups == 0) return 0;
    knn_index_s *f = H->flat;
    hipStream_t s = f->stream;
    if (int oom = hnsw_grow("hnsw: out of device memory", H->d_goff, (size_t)(ngroups + 1) * 4, H->d_mem, nmembers * 4,
                            H->d_maxo, (size_t)ngroups * 4, H->d_oid, (size_t)ngroups * out_stride * 4,
                            H->d_od, (size_t)ngroups * out_stride * 4, H->d_on, (size_t)ngroups * 4)) return oom;
    if (int oom = hnsw_grow("hnsw: out of pinned host memory", H->h_oid, (size_t)ngroups * out_stride * 4,
                            H->h_od, (size_t)ngroups * out_stride * 4, H->h_on, (size_t)ngroups * 4)) return oom;
    double t0 = now_s();
    HIP_TRY(hipMemcpyAsync(H->d_goff.p, H->h_goff.p, (size_t)(ngroups + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(H->d_mem.p, H->h_mem.p, nmembers * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(H->d_maxo.p, H->h_maxo.p, (size_t)ngroups * 4, hipMemcpyHostToDevice, s));
    ShrinkParams p;
    p.xb = f->xb; p.yn = f->yn; p.dp = f->dp; p.metric = f->metric;
    p.group_off = (const int32_t *)H->d_goff.p; p.group_cnt = nullptr; p.ngroups = nullptr; p.members = (const uint32_t *)H->d_mem.p;
    p.max_out = (const int32_t *)H->d_maxo.p; p.out_ids = (uint32_t *)H->d_oid.p; p.out_d = (float *)H->d_od.p;
    p.out_n = (int32_t *)H->d_on.p; p.out_stride = out_stride;
    int rc = launch_shrink(p, ngroups, max_members, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(H->h_oid.p, H->d_oid.p, (size_t)ngroups * out_stride * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(H->h_od.p, H->d_od.p, (size_t)ngroups * out_stride * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(H->h_on.p, H->d_on.p, (size_t)ngroups * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    H->stat_gpu_s += now_s() - t0;
    H->stat_shrinks += ngroups;
    return 0;
}

// the host graph's level-0 lists (and fills) brought up to date from the device's (every row of the mirror is valid)
static int hnsw_host0_sync(knn_hnsw_s *H)
{
    if (!H->host0_stale) return 0;
    HnswGraph &g = H->g;
    knn_index_s *f = H->flat;
    const int M0 = g.nb_neighbors(0);
    const int64_t n = std::min<int64_t>((int64_t)(H->d_nbr0.bytes / ((size_t)M0 * 4)), g.ntotal());
    HIP_TRY(hipSetDevice(f->device));
    const int64_t CH = 1 << 18; // 64 MB of lists per piece at M = 32
    if (n > 0)
        if (int oom = hnsw_grow("hnsw: out of pinned host memory", H->h_scatter_rows, (size_t)std::min(CH, n) * M0 * 4, H->h_scatter_ids, (size_t)std::min(CH, n)))
            return oom;
    for (int64_t i0 = 0; i0 < n; i0 += CH) {
        const int64_t m = std::min(CH, n - i0);
        HIP_TRY(hipMemcpyAsync(H->h_scatter_rows.p, (const uint32_t *)H->d_nbr0.p + (size_t)i0 * M0, (size_t)m * M0 * 4, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipMemcpyAsync(H->h_scatter_ids.p, (const uint8_t *)H->d_cnt0.p + i0, (size_t)m, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        const uint32_t *rows = (const uint32_t *)H->h_scatter_rows.p;
        const uint8_t *cn = (const uint8_t *)H->h_scatter_ids.p;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t i = 0; i < m; i++) {
            memcpy(g.list(i0 + i, 0), rows + (size_t)i * M0, (size_t)M0 * 4);
            g.cnt0[i0 + i] = cn[i];
        }
    }
    H->host0_stale = false;
    return 0;
}

// rows of the nodes `add` (level >= 2, linked) -> the index the construction candidates of the levels >= 2 are scanned from
static int hnsw_coarse2_append(knn_hnsw_s *H, const std::vector<uint32_t> &add)
{
    if (add.empty()) return 0;
    knn_index_s *f = H->flat;
    hipStream_t s = f->stream;
    if (!H->coarse2) {
        const int dev_before = g_device;
        g_device = f->device; // (knn_flat_create builds on the calling thread's current device)
        int rc = knn_flat_create(f->d, f->metric, &H->coarse2);
        g_device = dev_before;
        if (rc) return rc;
        if (H->coarse_bf16) {
            rc = flat_set_approx16(H->coarse2);
            if (rc) return rc;
        }
    }
    DevBuf d_ids, d_rows;
    if (int oom = hnsw_grow("hnsw: out of device memory (level-2 rows)", d_ids, add.size() * 4, d_rows, add.size() * (size_t)f->d * 4)) return oom;
    HIP_TRY(hipMemcpy(d_ids.p, add.data(), add.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)add.size()), dim3(256), 0, s, f->xb, f->dp, f->d, (const uint32_t *)d_ids.p, (int64_t)add.size(),
                       (float *)d_rows.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    int rc = knn_flat_add_dev(H->coarse2, (const float *)d_rows.p, (int64_t)add.size(), nullptr);
    d_ids.release();
    d_rows.release();
    if (rc) return rc;
    H->coarse2_ids_host.insert(H->coarse2_ids_host.end(), add.begin(), add.end());
    H->ncoarse2 = (int64_t)H->coarse2_ids_host.size();
    return 0;
}

// level-0 lists -> device ([n][M0] rows of 4 * M0 bytes: one coalesced load per expansion)
static int hnsw_upload_graph(knn_hnsw_s *H)
{
    if (!H->nbr0_dirty) return 0;
    if (H->host0_stale) { // (the mirror is rebuilt from the host's lists: they must be the current ones)
        int rc0 = hnsw_host0_sync(H);
        if (rc0) return rc0;
    }
    const HnswGraph &g = H->g;
    const int64_t n = g.ntotal();
    const int M0 = g.nb_neighbors(0);
#ifdef KNN355_DEV
    if (hnsw_env_set("KNN355_HNSW_DEBUG")) fprintf(stderr, "hnsw_upload_graph: n=%lld linked=%lld mirror_n=%lld nbr0 bytes=%zu\n", (long long)n, (long long)H->linked_count, (long long)H->mirror_count, H->d_nbr0.bytes);
#endif
    // (room for every row the storage has reserved space for, and half as much again when it has to guess: a graph filled
    // by several add calls otherwise outgrew its mirror at every call and rebuilt it from the host -- a quarter of the
    // build time of a 2 M-row graph added in four pieces)
    const int64_t room = std::max<int64_t>(std::max<int64_t>(n + n / 2, 1), H->flat->cap_rows);
    if (H->d_nbr0.bytes < (size_t)std::max<int64_t>(n, 1) * M0 * 4 &&
        H->d_nbr0.ensure((size_t)room * M0 * 4) && H->d_nbr0.ensure((size_t)std::max<int64_t>(n, 1) * M0 * 4))
        return set_err(KNN_ERR_HIP, "hnsw: out of device memory (neighbour lists)");
    // (every row of the mirror is valid: the lists of the linked nodes, "no link" everywhere else -- nodes waiting for their
    // batch, room for rows to come.  Few linked nodes in a large table -- the first device batch of a 10 M-row add call --
    // are scattered into a cleared table instead of uploading gigabytes of empty lists)
    const int64_t rows_dev = (int64_t)(H->d_nbr0.bytes / ((size_t)M0 * 4));
    if (H->d_cnt0.bytes < (size_t)rows_dev && H->d_cnt0.ensure((size_t)rows_dev))
        return set_err(KNN_ERR_HIP, "hnsw: out of device memory (neighbour counts)");
    if ((int64_t)H->linked.size() < n) H->linked.resize((size_t)n, 0);
    const bool sparse = H->linked_count * 8 < n;
    std::vector<uint32_t> who;
    if (sparse) {
        for (int64_t i = 0; i < n; i++)
            if (H->linked[(size_t)i]) who.push_back((uint32_t)i);
        HIP_TRY(hipMemset(H->d_nbr0.p, 0xFF, (size_t)rows_dev * M0 * 4));
        HIP_TRY(hipMemset(H->d_cnt0.p, 0, (size_t)rows_dev));
    } else if (rows_dev > n) {
        HIP_TRY(hipMemset((uint32_t *)H->d_nbr0.p + (size_t)n * M0, 0xFF, (size_t)(rows_dev - n) * M0 * 4));
        HIP_TRY(hipMemset((uint8_t *)H->d_cnt0.p + n, 0, (size_t)(rows_dev - n)));
    }
    const int64_t nl = sparse ? (int64_t)who.size() : n;
    std::vector<uint32_t> flat((size_t)nl * M0);
    std::vector<uint8_t> fills((size_t)nl);
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
    for (int64_t i = 0; i < nl; i++) {
        const int64_t node = sparse ? who[(size_t)i] : i;
        memcpy(flat.data() + (size_t)i * M0, g.list(node, 0), (size_t)M0 * 4);
        fills[(size_t)i] = g.cnt0[(size_t)node];
    }
    if (nl > 0 && !sparse) {
        HIP_TRY(hipMemcpy(H->d_nbr0.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(H->d_cnt0.p, fills.data(), (size_t)nl, hipMemcpyHostToDevice));
    } else if (nl > 0) {
        DevBuf d_who, d_rows, d_fill;
        if (int oom = hnsw_grow("hnsw: out of device memory (mirror upload)", d_who, (size_t)nl * 4, d_rows, flat.size() * 4,
                                d_fill, (size_t)nl)) return oom;
        HIP_TRY(hipMemcpy(d_who.p, who.data(), (size_t)nl * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_rows.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_fill.p, fills.data(), (size_t)nl, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)nl), dim3(64), 0, H->flat->stream, (const uint32_t *)d_who.p, (const uint32_t *)d_rows.p, M0,
                           (int64_t)nl, (uint32_t *)H->d_nbr0.p);
        hipLaunchKernelGGL(scatter_bytes_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, H->flat->stream, (const uint32_t *)d_who.p, (const uint8_t *)d_fill.p,
                           (int64_t)nl, (uint8_t *)H->d_cnt0.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(H->flat->stream));
        d_who.release(); d_rows.release(); d_fill.release();
    }
    // Coarse entry index: the rows of all nodes above level 0 (one in M), copied into a flat index of their
    // own.  A search starts with an EXACT scan of these rows on the flat kernel and enters level 0 at the
    // nearest of them -- the upper levels' greedy descent (a host loop over a few hundred nodes, and a coin toss
    // when cluster centres are equidistant) is replaced by what this GPU is best at.  10 M rows: 312 k coarse
    // rows, 20 ms per 4096 queries.
    if (H->coarse) {
        knn_free(H->coarse);
        H->coarse = nullptr;
    }
    H->ncoarse = 0;
    if (H->coarse2) {
        knn_free(H->coarse2);
        H->coarse2 = nullptr;
    }
    H->coarse2_ids_host.clear();
    H->ncoarse2 = 0;
    std::vector<uint32_t> &up = H->coarse_ids_host;
    up.clear();
    for (int64_t i = 0; i < n; i++) // (nodes still waiting for their batch have no links: never an entry point)
        if (H->linked[(size_t)i] && g.levels[i] >= 1) up.push_back((uint32_t)i);
    H->mirror_count = H->linked_count;
    knn_index_s *f = H->flat;
    if ((int64_t)up.size() >= 64 && H->coarse_entries > 0) {
        if (int oom = hnsw_grow("hnsw: out of device memory (coarse ids)", H->d_coarse_ids, up.size() * 4)) return oom;
        HIP_TRY(hipMemcpy(H->d_coarse_ids.p, up.data(), up.size() * 4, hipMemcpyHostToDevice));
        const int dev_before = g_device;
        g_device = f->device; // (knn_flat_create builds on the calling thread's current device)
        int rc = knn_flat_create(f->d, f->metric, &H->coarse);
        g_device = dev_before;
        if (rc) return rc;
        // only the neighbourhood matters for an entry point (the beam's rows are re-scored exactly): the coarse scan
        // multiplies bf16 copies -- 1/16 of the matrix time, half the bytes
        if (H->coarse_bf16) {
            rc = flat_set_approx16(H->coarse);
            if (rc) return rc;
        }
        rc = knn_flat_reserve(H->coarse, (int64_t)up.size());
        if (rc) return rc;
        const int64_t CH = 1 << 18;
        DevBuf tmp;
        if (int oom = hnsw_grow("hnsw: out of device memory (coarse rows)",
                                tmp, (size_t)std::min<int64_t>(CH, (int64_t)up.size()) * f->d * 4)) return oom;
        for (int64_t i0 = 0; i0 < (int64_t)up.size(); i0 += CH) {
            const int64_t m = std::min<int64_t>(CH, (int64_t)up.size() - i0);
            hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)m), dim3(256), 0, f->stream, f->xb, f->dp, f->d,
                               (const uint32_t *)H->d_coarse_ids.p + i0, m, (float *)tmp.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(f->stream));
            rc = knn_flat_add_dev(H->coarse, (const float *)tmp.p, m, nullptr);
            if (rc) { tmp.release(); return rc; }
        }
        tmp.release();
        H->ncoarse = (int64_t)up.size();
        std::vector<uint32_t> up2;
        for (uint32_t node : up)
            if (g.levels[node] >= 2) up2.push_back(node);
        const size_t CH2 = 1 << 17;
        for (size_t i0 = 0; i0 < up2.size(); i0 += CH2) {
            rc = hnsw_coarse2_append(H, std::vector<uint32_t>(up2.begin() + i0, up2.begin() + std::min(up2.size(), i0 + CH2)));
            if (rc) return rc;
        }
    }
    H->nbr0_dirty = false;
    return 0;
}

// after a batch: changed level-0 lists -> device mirror, the batch's nodes above level 0 -> coarse index
static int hnsw_mirror_update(knn_hnsw_s *H, const int64_t *ids, int count, std::vector<uint32_t> &dirty)
{
    const HnswGraph &g = H->g;
    knn_index_s *f = H->flat;
    const int M0 = g.nb_neighbors(0);
    hipStream_t s = f->stream;
    std::sort(dirty.begin(), dirty.end());
    dirty.erase(std::unique(dirty.begin(), dirty.end()), dirty.end());
    const size_t nd = dirty.size();
    if (nd) {
        if (int oom = hnsw_grow("hnsw: out of memory (mirror update)", H->h_scatter_ids, nd * 4, H->h_scatter_rows, nd * M0 * 4,
                                H->d_scatter_ids, nd * 4, H->d_scatter_rows, nd * M0 * 4)) return oom;
        uint32_t *hi = (uint32_t *)H->h_scatter_ids.p, *hr = (uint32_t *)H->h_scatter_rows.p;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t i = 0; i < (int64_t)nd; i++) {
            hi[i] = dirty[i];
            memcpy(hr + (size_t)i * M0, g.list(dirty[i], 0), (size_t)M0 * 4);
        }
        HIP_TRY(hipMemcpyAsync(H->d_scatter_ids.p, hi, nd * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(H->d_scatter_rows.p, hr, nd * M0 * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)nd), dim3(64), 0, s, (const uint32_t *)H->d_scatter_ids.p,
                           (const uint32_t *)H->d_scatter_rows.p, M0, (int64_t)nd, (uint32_t *)H->d_nbr0.p);
        HIP_TRY(hipGetLastError());
    }
    // coarse index: append the batch's nodes above level 0
    std::vector<uint32_t> add;
    for (int i = 0; i < count; i++)
        if (g.levels[ids[i]] >= 1) add.push_back((uint32_t)ids[i]);
    if (!add.empty()) {
        std::vector<uint32_t> &up = H->coarse_ids_host;
        const size_t old = up.size();
        up.insert(up.end(), add.begin(), add.end());
        if (H->d_coarse_ids.bytes < up.size() * 4) {
            // (DevBuf::ensure does not keep contents: the whole id list goes up again, a few hundred KB)
            if (int oom = hnsw_grow("hnsw: out of device memory (coarse ids)", H->d_coarse_ids, up.size() * 4 + (up.size() * 4) / 2)) return oom;
            HIP_TRY(hipMemcpyAsync(H->d_coarse_ids.p, up.data(), up.size() * 4, hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync((uint32_t *)H->d_coarse_ids.p + old, add.data(), add.size() * 4, hipMemcpyHostToDevice, s));
        }
        DevBuf &tmp = H->d_scatter_rows; // (free again: the scatter above is ordered before on this stream)
        if (int oom = hnsw_grow("hnsw: out of device memory (coarse rows)", tmp, add.size() * (size_t)f->d * 4)) return oom;
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)add.size()), dim3(256), 0, s, f->xb, f->dp, f->d,
                           (const uint32_t *)H->d_coarse_ids.p + old, (int64_t)add.size(), (float *)tmp.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        int rc = knn_flat_add_dev(H->coarse, (const float *)tmp.p, (int64_t)add.size(), nullptr);
        if (rc) return rc;
        H->ncoarse = (int64_t)up.size();
        std::vector<uint32_t> add2;
        for (uint32_t node : add)
            if (g.levels[node] >= 2) add2.push_back(node);
        rc = hnsw_coarse2_append(H, add2);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s)); // (the pinned staging buffers are reused by the next batch)
    H->mirror_count = H->linked_count + count; // (the caller marks the batch linked)
    return 0;
}

template <int NCH, int RB, bool B16 = false>
static int launch_beam(const BeamParams &bp, int grid, size_t lds, hipStream_t s)
{
    HIP_TRY(hipFuncSetAttribute((const void *)hnsw_beam_kernel<NCH, RB, B16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((hnsw_beam_kernel<NCH, RB, B16>), dim3(grid), dim3(256), lds, s, bp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The device pipeline shared by search and construction, for m queries already on the device (xq: [m][dp] zero
// padded, xq_raw: [m][d] as the flat index takes them, qn: squared norms): entry points from an exact scan of the
// nodes above level 0 (or, for small graphs, from the host's greedy descent), the level-0 beam of `ef` entries,
// exact re-scoring of the beam, selection of the k best -> D/I and/or sorted keys [m][k] (device pointers).
static int hnsw_beam_pipeline(knn_hnsw_s *H, const float *xq, const float *xq_raw, const float *qn, int64_t m, int ef, int k,
                              float *D_dev, int64_t *I_dev, uint64_t *keys_dev, hipStream_t s)
{
    knn_index_s *f = H->flat;
    const HnswGraph &g = H->g;
    const int64_t n = g.ntotal();
    const int M0 = g.nb_neighbors(0);
    const int R = (ef + 63) / 64;
    const size_t lds = (size_t)4 * R * 64 * 8 + 4 * 64 * 4;
    const int64_t vis_words = ((n + 31) / 32 + 3) / 4 * 4;
    const int rb = H->beam_rows;
    const int max_grid = (rb == 8 && !f->keep16 ? 2 : 4) * std::max(1, f->num_cus); // (workgroups per CU the registers allow)
    int rc;
    if (int oom = hnsw_grow("hnsw: out of device memory", H->d_entry, (size_t)m * std::max(1, H->coarse_entries) * 4,
                            H->d_beam_ids, (size_t)m * ef * 4, H->d_beam_keys, (size_t)m * ef * 8, H->d_stats, 64)) return oom;
    int nentry = 1;
    if (H->coarse && H->ncoarse > 0) {
        // exact nearest nodes above level 0: one scan of the coarse rows on the flat kernel
        nentry = (int)std::min<int64_t>(H->coarse_entries, H->ncoarse);
        if (int oom = hnsw_grow("hnsw: out of device memory", H->d_coarse_keys, (size_t)m * nentry * 8)) return oom;
        rc = knn_flat_search_keys_dev(H->coarse, xq_raw, m, nentry, 0, (uint64_t *)H->d_coarse_keys.p, (void *)s);
        if (rc) return rc;
        const int64_t tot = m * nentry;
        hipLaunchKernelGGL(coarse_entries_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, (const uint64_t *)H->d_coarse_keys.p,
                           tot, (const uint32_t *)H->d_coarse_ids.p, (uint32_t *)H->d_entry.p);
        HIP_TRY(hipGetLastError());
    } else {
        // few nodes above level 0 (small graphs): greedy descent on the host graph, GPU distances in lock step
        if (int oom = hnsw_grow("hnsw: out of pinned host memory", H->h_entry, (size_t)m * 4)) return oom;
        uint32_t *entry = (uint32_t *)H->h_entry.p;
        if (g.max_level > 0) {
            std::vector<Walker> ws((size_t)m);
            for (int64_t i = 0; i < m; i++) {
                ws[i].qslot = (uint32_t)i;
                ws[i].greedy_until = 0;
                ws[i].stop_level = 0;
                ws[i].descent_only = true;
            }
            rc = hnsw_walk(H, ws, xq, qn, false);
            if (rc) return rc;
            for (int64_t i = 0; i < m; i++) entry[i] = ws[i].cur;
        } else {
            for (int64_t i = 0; i < m; i++) entry[i] = (uint32_t)g.entry;
        }
        HIP_TRY(hipMemcpyAsync(H->d_entry.p, entry, (size_t)m * 4, hipMemcpyHostToDevice, s));
    }
    // rows handed on to the exact re-scoring per query
    int keep = ef, kmin = ef;
    if (k < ef) {
        kmin = std::min(ef, k + std::max(k >> 3, 8));
        keep = std::min(ef, k + std::max(k >> 2, 16));
        if (keep + 8 >= ef) keep = kmin = ef;
    }
    const int grid = (int)std::min<int64_t>((m + 3) / 4, max_grid);
    // Lazy clearing pays when a bitmap (n / 128 sixteen-byte stores) is much longer than what a walk touches (about
    // ef x M0 words at most): graphs of millions of rows.  The bitmaps must then be zero between launches: they are
    // zeroed when (re)allocated or after an eager launch, and every lazy walk leaves its own zero again.
    const int tcap = 16384;
    // (KNN355_HNSW_CLEAR=lazy|eager forces one or the other: tests)
    const bool lazy = hnsw_env_is("KNN355_HNSW_CLEAR", "lazy") ? true : (hnsw_env_is("KNN355_HNSW_CLEAR", "eager") ? false : vis_words / 4 > 2 * (int64_t)ef * M0);
    {
        const size_t need = (size_t)grid * 4 * vis_words * 4;
        const void *before = H->d_vis.p;
        const size_t before_bytes = H->d_vis.bytes;
        if (int oom = hnsw_grow("hnsw: out of device memory (visited bitmaps)", H->d_vis, need)) return oom;
        if (H->d_vis.p != before || H->d_vis.bytes != before_bytes) H->vis_zero_bytes = 0;
        if (lazy) {
            if (int oom = hnsw_grow("hnsw: out of device memory (visited lists)", H->d_touched, (size_t)grid * 4 * tcap * 4)) return oom;
            if (H->vis_zero_bytes < need) {
                HIP_TRY(hipMemsetAsync(H->d_vis.p, 0, need, s));
                H->vis_zero_bytes = need;
            }
        } else {
            H->vis_zero_bytes = 0; // (an eager launch leaves the last walks' bits behind)
        }
    }
    HIP_TRY(hipMemsetAsync(H->d_stats.p, 0, 16, s));
    BeamParams bp;
    bp.xb = f->xb; bp.yn = f->yn; bp.xq = xq; bp.qn = qn;
    bp.nbr0 = (const uint32_t *)H->d_nbr0.p; bp.entry = (const uint32_t *)H->d_entry.p;
    bp.visited = (uint32_t *)H->d_vis.p; bp.out_ids = (uint32_t *)H->d_beam_ids.p;
    bp.touched = lazy ? (uint32_t *)H->d_touched.p : nullptr; bp.tcap = tcap;
    bp.stats = (unsigned long long *)H->d_stats.p;
    bp.nq = m; bp.n = n; bp.vis_words = vis_words; bp.dp = f->dp; bp.metric = f->metric; bp.M0 = M0; bp.ef = ef; bp.nentry = nentry; bp.keep = keep; bp.kmin = kmin; bp.expand2 = H->beam_expand2;
    const bool b16 = f->keep16 && f->xb16.p != nullptr;
    bp.xb16 = (const uint16_t *)f->xb16.p;
    if (b16) {
        // (eight rows in flight again: a bf16 row is half the registers)
        if (f->dp <= 512) rc = launch_beam<1, 8, true>(bp, grid, lds, s);
        else rc = launch_beam<2, 8, true>(bp, grid, lds, s);
        if (rc) return rc;
    }
    const int nch = (f->dp + 255) / 256;
    if (b16) {
    } else if (rb == 8) {
        if (nch <= 1) rc = launch_beam<1, 8>(bp, grid, lds, s);
        else if (nch <= 2) rc = launch_beam<2, 8>(bp, grid, lds, s);
        else rc = launch_beam<4, 8>(bp, grid, lds, s);
    } else {
        if (nch <= 1) rc = launch_beam<1, 4>(bp, grid, lds, s);
        else if (nch <= 2) rc = launch_beam<2, 4>(bp, grid, lds, s);
        else rc = launch_beam<4, 4>(bp, grid, lds, s);
    }
    if (rc) return rc;
    // exact scores of the beam's rows (the flat scan's chain), then the k best of them, sorted
    const int64_t np = m * keep;
    if (hnsw_env_set("KNN355_HNSW_KEYS_DIRECT"))
        hipLaunchKernelGGL(beam_keys_kernel, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, s, xq, qn, f->xb, f->yn, f->dp, f->metric, m, keep,
                           (const uint32_t *)H->d_beam_ids.p, (uint64_t *)H->d_beam_keys.p);
    else
        hipLaunchKernelGGL(beam_keys_lds_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, xq, qn, f->xb, f->yn, f->dp, f->metric, m,
                           keep, (const uint32_t *)H->d_beam_ids.p, (uint64_t *)H->d_beam_keys.p);
    HIP_TRY(hipGetLastError());
    SelectParams sp = {};
    sp.in = (const uint64_t *)H->d_beam_keys.p; sp.in_stride = keep; sp.n_fixed = keep; sp.cap = keep;
    sp.nq = m; sp.k = k; sp.metric = f->metric;
    sp.D = D_dev; sp.I = I_dev;
    sp.out_keys = keys_dev; sp.out_stride = k; sp.out_fill = keys_dev ? k : 0;
    return launch_select(sp, s);
}

static inline float host_ord2f(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// the batch being linked on the device: its node ids -> d_bids, its rows gathered into d_bq ([count][dp]; the device path has
// dp == d) and their norms into d_bqn -- the batch's rows are their own queries
static int hnsw_batch_queries(knn_hnsw_s *H, const int64_t *ids, int count, hipStream_t s)
{
    knn_index_s *f = H->flat;
    if (int oom = hnsw_grow("hnsw: out of memory (batch rows)", H->d_bids, (size_t)count * 4, H->d_bq, (size_t)count * f->dp * 4,
                            H->d_bqn, (size_t)count * 4, H->h_scatter_ids, (size_t)count * 4)) return oom;
    uint32_t *hi = (uint32_t *)H->h_scatter_ids.p;
    for (int i = 0; i < count; i++) hi[i] = (uint32_t)ids[i];
    HIP_TRY(hipMemcpyAsync(H->d_bids.p, hi, (size_t)count * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)count), dim3(256), 0, s, f->xb, f->dp, f->dp, (const uint32_t *)H->d_bids.p, (int64_t)count,
                       (float *)H->d_bq.p);
    hipLaunchKernelGGL(gather_f32_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, f->yn, (const uint32_t *)H->d_bids.p, (int64_t)count,
                       (float *)H->d_bqn.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s)); // (the pinned id list is reused)
    return 0;
}

// construction: level-0 candidates (efConstruction best, ascending) of rows ids[0 .. count) against the frozen graph
static int hnsw_level0_candidates_device(knn_hnsw_s *H, const int64_t *ids, int count, std::vector<std::vector<DistId>> &cand0)
{
    knn_index_s *f = H->flat;
    const int efc = H->efConstruction;
    hipStream_t s = f->stream;
    if (int oom = hnsw_grow("hnsw: out of memory (construction candidates)", H->d_beam_out, (size_t)count * efc * 8,
                            H->h_keys, (size_t)count * efc * 8)) return oom;
    // the new rows are their own queries: on the device, padded (dp == d here), with their norms
    int rc = hnsw_batch_queries(H, ids, count, s);
    if (rc) return rc;
    const float *xq = (const float *)H->d_bq.p;
    rc = hnsw_beam_pipeline(H, xq, xq, (const float *)H->d_bqn.p, count, efc, efc, nullptr, nullptr, (uint64_t *)H->d_beam_out.p, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(H->h_keys.p, H->d_beam_out.p, (size_t)count * efc * 8, hipMemcpyDeviceToHost, s));
    unsigned long long st[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(st, H->d_stats.p, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    H->stat_pairs += (int64_t)st[0];
    H->stat_expansions += (int64_t)st[1];
    const uint64_t *keys = (const uint64_t *)H->h_keys.p;
    cand0.assign((size_t)count, std::vector<DistId>());
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
    for (int i = 0; i < count; i++) {
        std::vector<DistId> &c = cand0[i];
        c.reserve(efc);
        for (int j = 0; j < efc; j++) {
            const uint64_t kk = keys[(size_t)i * efc + j];
            if (kk == KEY_PAD) break;
            c.push_back(DistId(host_ord2f((uint32_t)(kk >> 32)), (uint32_t)kk));
        }
    }
    return 0;
}

// level-0 links of rows ids[0 .. count): candidates from the beam (left on the device), everything else as above
static int hnsw_level0_links_device(knn_hnsw_s *H, const int64_t *ids, int count)
{
    knn_index_s *f = H->flat;
    const HnswGraph &g = H->g;
    const int efc = H->efConstruction;
    const int M0 = g.nb_neighbors(0);
    hipStream_t s = f->stream;
    double tp = now_s();
    (void)tp;
    if (int oom = hnsw_grow("hnsw: out of memory (construction candidates)", H->d_beam_out, (size_t)count * efc * 8)) return oom;
    int rc = hnsw_batch_queries(H, ids, count, s); // (the new rows are their own queries: on the device, padded, with their norms)
    if (rc) return rc;
    const float *xq = (const float *)H->d_bq.p;
    rc = hnsw_beam_pipeline(H, xq, xq, (const float *)H->d_bqn.p, count, efc, efc, nullptr, nullptr, (uint64_t *)H->d_beam_out.p, s);
    if (rc) return rc;
#ifdef KNN355_DEV
    HIP_TRY(hipStreamSynchronize(s)); // (developer build: the beam's time apart from the selection's)
    HNSW_PROF(1, tp);
#endif
    const int take = std::min(efc, SHRINK_MAX_MEMBERS - 1);
    const int stride = take + 1;
    const size_t nrev_max = (size_t)count * M0;
    if (int oom = hnsw_grow("hnsw: out of device memory (construction, level 0)", H->dl_mem, (size_t)count * stride * 4,
                            H->dl_goff, (size_t)count * 4, H->dl_gcnt, (size_t)count * 4, H->dl_maxo, (size_t)count * 4,
                            H->dl_oid, (size_t)count * M0 * 4, H->dl_od, (size_t)count * M0 * 4, H->dl_on, (size_t)count * 4,
                            H->dl_roff, (size_t)(count + 1) * 4, H->dl_ctr, 64, H->dl_key0, nrev_max * 8, H->dl_key1, nrev_max * 8,
                            H->dl_from0, nrev_max * 4, H->dl_from1, nrev_max * 4)) return oom;
    uint32_t *mem = (uint32_t *)H->dl_mem.p, *nbr0 = (uint32_t *)H->d_nbr0.p, *ctr = (uint32_t *)H->dl_ctr.p;
    uint8_t *cnt0 = (uint8_t *)H->d_cnt0.p;
    int32_t *goff = (int32_t *)H->dl_goff.p, *gcnt = (int32_t *)H->dl_gcnt.p, *maxo = (int32_t *)H->dl_maxo.p;
    // forward selection
    {
        const int64_t tot = (int64_t)count * stride;
        hipLaunchKernelGGL(dl_fwd_groups_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, (const uint64_t *)H->d_beam_out.p, count, efc, take,
                           (const uint32_t *)H->d_bids.p, M0, mem, goff, gcnt, maxo);
        HIP_TRY(hipGetLastError());
    }
    ShrinkParams p;
    p.xb = f->xb; p.yn = f->yn; p.dp = f->dp; p.metric = f->metric;
    p.group_off = goff; p.group_cnt = gcnt; p.ngroups = nullptr; p.members = mem; p.max_out = maxo;
    p.out_ids = (uint32_t *)H->dl_oid.p; p.out_d = (float *)H->dl_od.p; p.out_n = (int32_t *)H->dl_on.p; p.out_stride = M0;
    rc = launch_shrink(p, count, stride, s);
    if (rc) return rc;
    // forward links + reverse requests
    hipLaunchKernelGGL(dl_scan_kernel, dim3(1), dim3(1024), 0, s, (const int32_t *)H->dl_on.p, count, (int32_t *)H->dl_roff.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dl_fwd_write_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, (const uint32_t *)H->dl_oid.p, (const float *)H->dl_od.p,
                       (const int32_t *)H->dl_on.p, (const int32_t *)H->dl_roff.p, count, (const uint32_t *)H->d_bids.p, M0, nbr0, cnt0,
                       (uint64_t *)H->dl_key0.p, (uint32_t *)H->dl_from0.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(ctr, 0, 16, s));
    int32_t nrev = 0;
    unsigned long long st[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&nrev, (const int32_t *)H->dl_roff.p + count, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st, H->d_stats.p, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    H->stat_pairs += (int64_t)st[0];
    H->stat_expansions += (int64_t)st[1];
    H->stat_shrinks += count;
    HNSW_PROF(2, tp); // forward selection + forward links (device; with the beam's time in a build without KNN355_DEV)
    if (nrev > 0) {
        // (the groups of the forward selection are done with: their arrays now hold the pruning groups -- at most one per
        // request, 1 + M0 members of its own each besides the requests it takes in)
        if (int oom = hnsw_grow("hnsw: out of device memory (construction, level 0)", H->dl_mem, (size_t)nrev * (M0 + 2) * 4,
                                H->dl_goff, (size_t)nrev * 4, H->dl_gcnt, (size_t)nrev * 4, H->dl_maxo, (size_t)nrev * 4,
                                H->dl_gnode, (size_t)nrev * 4)) return oom;
        mem = (uint32_t *)H->dl_mem.p;
        goff = (int32_t *)H->dl_goff.p; gcnt = (int32_t *)H->dl_gcnt.p; maxo = (int32_t *)H->dl_maxo.p;
        p.group_off = goff; p.group_cnt = gcnt; p.members = mem; p.max_out = maxo;
        // sorted by (node, v); the node's bits that are always zero are left out of the passes
        int node_bits = 1;
        while (node_bits < 32 && (1ll << node_bits) < g.ntotal()) node_bits++;
        size_t tb = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint64_t *)H->dl_key0.p, (uint64_t *)H->dl_key1.p, (const uint32_t *)H->dl_from0.p,
                                                   (uint32_t *)H->dl_from1.p, (int)nrev, 0, 32 + node_bits, s));
        if (int oom = hnsw_grow("hnsw: out of device memory (sort)", H->dl_tmp, std::max<size_t>(tb, 256))) return oom;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(H->dl_tmp.p, tb, (const uint64_t *)H->dl_key0.p, (uint64_t *)H->dl_key1.p, (const uint32_t *)H->dl_from0.p,
                                                   (uint32_t *)H->dl_from1.p, (int)nrev, 0, 32 + node_bits, s));
        hipLaunchKernelGGL(dl_rev_apply_kernel, dim3((unsigned)((nrev + 255) / 256)), dim3(256), 0, s, (const uint64_t *)H->dl_key1.p, (const uint32_t *)H->dl_from1.p,
                           (int)nrev, M0, nbr0, cnt0, ctr, goff, gcnt, maxo, (uint32_t *)H->dl_gnode.p, mem);
        HIP_TRY(hipGetLastError());
        uint32_t hc[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(hc, ctr, 12, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HNSW_PROF(4, tp); // reverse requests sorted and appended (device)
        const int nprune = (int)hc[0];
        if (nprune > 0) {
            if (int oom = hnsw_grow("hnsw: out of device memory (construction, level 0)",
                                    H->dl_oid, (size_t)std::max(count, nprune) * M0 * 4,
                                    H->dl_od, (size_t)std::max(count, nprune) * M0 * 4, H->dl_on, (size_t)std::max(count, nprune) * 4)) return oom;
            p.out_ids = (uint32_t *)H->dl_oid.p; p.out_d = (float *)H->dl_od.p; p.out_n = (int32_t *)H->dl_on.p;
            rc = launch_shrink(p, nprune, (int)hc[2], s);
            if (rc) return rc;
            hipLaunchKernelGGL(dl_prune_write_kernel, dim3((unsigned)((nprune + 3) / 4)), dim3(256), 0, s, (const uint32_t *)H->dl_gnode.p, (const uint32_t *)H->dl_oid.p,
                               (const int32_t *)H->dl_on.p, nprune, M0, nbr0, cnt0);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));
            H->stat_shrinks += nprune;
        }
        HNSW_PROF(5, tp); // reverse pruning (device)
    }
    H->host0_stale = true;
    return 0;
}

// construction: candidates of the levels ABOVE 0.  Every node above level 0 has a row in the coarse index (the flat index the
// searches take their entry points from), so the efConstruction nearest nodes of level >= 1 are ONE exact scan of it --
// no walk at all, and better than a walk's approximation.  Levels >= 2 (one point in M^2 has any): a scan with a large k,
// filtered by level.  Until round 3 these levels were walked on the host with GPU distances in lock step: a third of the
// build time (2 M rows: 2.8 of 8.0 s) went into the thousands of round trips of one point in M.
// `starved` receives the points (members of `up`) for which that large-k scan is NOT enough: on a big graph the best
// KNN_MAX_K coarse rows hold only a handful of the nodes of the highest levels (10 M rows, M = 42: ~240 k coarse rows,
// ~135 nodes of level >= 3 -- about one of them among 2048), a level's list then comes back shorter than
// min(efConstruction, nodes of that level) and a node linked from it would sit (almost) disconnected on that level --
// invisible to the searches that enter through the coarse scan, fatal for FAISS's greedy descent (knn_hnsw_set_entry(H, 0),
// IHNf files read by the real faiss).  The caller walks those points' upper levels on the host, as before round 3: one
// point in M^2 at most, a few hundred in a 10 M-row build (ADVICE r3).
static int hnsw_upper_candidates_device(knn_hnsw_s *H, const int64_t *ids, const std::vector<int> &up, std::vector<std::vector<std::vector<DistId>>> &lc,
                                        std::vector<int> &starved)
{
    knn_index_s *f = H->flat;
    const HnswGraph &g = H->g;
    const int efc = H->efConstruction;
    hipStream_t s = f->stream;
    const int64_t nu = (int64_t)up.size();
    std::vector<int> up2; // positions in `up` of the points with levels >= 2
    for (int64_t j = 0; j < nu; j++)
        if (std::min(g.levels[ids[up[j]]], g.max_level) >= 2) up2.push_back((int)j);
    const int k1 = (int)std::min<int64_t>(efc, H->ncoarse);
    // the levels >= 2 are scanned in their own index once it holds a few rows (one node in M of the coarse index: the large-k scan
    // then reaches 32 times deeper into those levels -- on a 10 M-row graph it is the level-4 nodes that run short, not the level-3 ones)
    const bool own2 = H->coarse2 && H->ncoarse2 >= 64;
    const int64_t n2 = own2 ? H->ncoarse2 : H->ncoarse;
    const int k2 = (int)std::min<int64_t>(KNN_MAX_K, n2);
    const size_t nkeys = (size_t)nu * k1 + up2.size() * (size_t)k2;
    if (int oom = hnsw_grow("hnsw: out of memory (upper-level candidates)", H->h_scatter_ids, (size_t)nu * 4,
                            H->d_scatter_ids, (size_t)nu * 4, H->d_q, (size_t)nu * f->d * 4, H->d_beam_out, nkeys * 8,
                            H->h_keys, nkeys * 8)) return oom;
    uint32_t *uids = (uint32_t *)H->h_scatter_ids.p;
    for (int64_t j = 0; j < nu; j++) uids[j] = (uint32_t)ids[up[j]];
    HIP_TRY(hipMemcpyAsync(H->d_scatter_ids.p, uids, (size_t)nu * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)nu), dim3(256), 0, s, f->xb, f->dp, f->d, (const uint32_t *)H->d_scatter_ids.p, nu,
                       (float *)H->d_q.p);
    HIP_TRY(hipGetLastError());
    uint64_t *dk = (uint64_t *)H->d_beam_out.p;
    int rc = knn_flat_search_keys_dev(H->coarse, (const float *)H->d_q.p, nu, k1, 0, dk, (void *)s);
    if (rc) return rc;
    if (!up2.empty()) {
        // their rows, gathered again behind the first block of queries
        if (int oom = hnsw_grow("hnsw: out of memory (upper-level candidates)", H->d_scatter_rows, up2.size() * 4,
                                H->h_scatter_rows, up2.size() * 4, H->d_qn, up2.size() * (size_t)f->d * 4)) return oom;
        uint32_t *ids2 = (uint32_t *)H->h_scatter_rows.p;
        for (size_t j = 0; j < up2.size(); j++) ids2[j] = (uint32_t)ids[up[up2[j]]];
        HIP_TRY(hipMemcpyAsync(H->d_scatter_rows.p, ids2, up2.size() * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)up2.size()), dim3(256), 0, s, f->xb, f->dp, f->d, (const uint32_t *)H->d_scatter_rows.p,
                           (int64_t)up2.size(), (float *)H->d_qn.p);
        HIP_TRY(hipGetLastError());
        rc = knn_flat_search_keys_dev(own2 ? H->coarse2 : H->coarse, (const float *)H->d_qn.p, (int64_t)up2.size(), k2, 0, dk + (size_t)nu * k1, (void *)s);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(H->h_keys.p, dk, nkeys * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t *keys = (const uint64_t *)H->h_keys.p;
    const uint32_t *cid = H->coarse_ids_host.data();
    for (int64_t j = 0; j < nu; j++) {
        const int top = std::min(g.levels[ids[up[j]]], g.max_level);
        auto &mine = lc[(size_t)up[j]];
        mine.resize((size_t)top + 1);
        std::vector<DistId> &c = mine[1];
        c.reserve(k1);
        for (int i = 0; i < k1; i++) {
            const uint64_t kk = keys[(size_t)j * k1 + i];
            if (kk == KEY_PAD) break;
            c.push_back(DistId(host_ord2f((uint32_t)(kk >> 32)), cid[(uint32_t)kk]));
        }
    }
    for (size_t u = 0; u < up2.size(); u++) {
        const int64_t j = up2[u];
        const int top = std::min(g.levels[ids[up[j]]], g.max_level);
        auto &mine = lc[(size_t)up[j]];
        const uint64_t *kr = keys + (size_t)nu * k1 + u * (size_t)k2;
        for (int i = 0; i < k2; i++) {
            if (kr[i] == KEY_PAD) break;
            const uint32_t node = own2 ? H->coarse2_ids_host[(uint32_t)kr[i]] : cid[(uint32_t)kr[i]];
            const int lv = g.levels[node];
            for (int l = 2; l <= std::min(lv, top); l++)
                if ((int)mine[l].size() < efc) mine[l].push_back(DistId(host_ord2f((uint32_t)(kr[i] >> 32)), node));
        }
    }
    static const bool fallback_on = hnsw_env_int("KNN355_HNSW_STARVED_FALLBACK", 1) != 0; // (tests: the round-3 behaviour)
    if (fallback_on && !up2.empty() && (int64_t)k2 < n2) {
        // (the scan saw only part of its index) nodes of each level among ALL coarse rows
        std::vector<int64_t> at_least((size_t)g.max_level + 2, 0);
        for (int64_t c = 0; c < H->ncoarse; c++) at_least[(size_t)std::min(g.levels[cid[c]], g.max_level)]++;
        for (int l = g.max_level - 1; l >= 0; l--) at_least[(size_t)l] += at_least[(size_t)l + 1];
        for (size_t u = 0; u < up2.size(); u++) {
            const int64_t j = up2[u];
            auto &mine = lc[(size_t)up[j]];
            bool short_list = false;
            for (int l = 2; l < (int)mine.size(); l++)
                short_list |= (int64_t)mine[l].size() < std::min<int64_t>(efc, at_least[(size_t)l]);
            if (short_list) starved.push_back(up[j]);
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// One batch of insertions: what its phases hand to each other.  hnsw_insert_batch (below) runs them in order.
// ---------------------------------------------------------------------------
struct BatchJob { int point; int level; };                        // one selection group: a point of the batch at one of its levels
struct BatchRev { uint32_t node; int level; uint32_t from; float d; }; // reverse link request: `node` should link back to `from`
struct BatchPrune { uint32_t node; int level; size_t r0, r1; };   // a list the requests revs[r0 .. r1) overfill
struct HnswBatch {
    knn_hnsw_s *H;
    const int64_t *ids; // rows of the batch, ascending
    int count;
    int M0;
    bool dev = false;       // level-0 candidates come from the device beam
    bool dev_links = false; // ... and level 0 is linked there as well (the host phases then see the upper levels only)
    double tp = 0;          // HNSW_PROF's clock
    std::vector<std::vector<std::vector<DistId>>> lc; // [point][level] candidates, ascending
    std::vector<BatchJob> jobs;
    std::vector<std::vector<DistId>> fwd; // selected (v, id) per job
    std::vector<BatchRev> revs;
    std::vector<uint32_t> dirty; // nodes whose level-0 list changed (the device mirror follows)
    std::vector<BatchPrune> prunes;
};

// total order of the reverse requests: the result of the sort does not depend on how it is split over threads
static inline bool rev_less(const BatchRev &a, const BatchRev &b)
{
    if (a.node != b.node) return a.node < b.node;
    if (a.level != b.level) return a.level < b.level;
    if (a.d != b.d) return a.d < b.d;
    return a.from < b.from;
}

// pinned staging of `ngroups` pruning groups of `nmem` members in all: what the callers fill before hnsw_run_shrink
struct ShrinkStage { int32_t *goff; uint32_t *mem; int32_t *maxo; };
static int hnsw_shrink_stage(knn_hnsw_s *H, size_t ngroups, size_t nmem, ShrinkStage &st)
{
    if (int oom = hnsw_grow("hnsw: out of pinned host memory", H->h_goff, (ngroups + 1) * 4, H->h_mem, nmem * 4, H->h_maxo, ngroups * 4)) return oom;
    st.goff = (int32_t *)H->h_goff.p;
    st.mem = (uint32_t *)H->h_mem.p;
    st.maxo = (int32_t *)H->h_maxo.p;
    return 0;
}

// which paths the batch takes; the device mirror and the host's level-0 lists brought up to date for them
static int hnsw_batch_paths(HnswBatch &b)
{
    knn_hnsw_s *H = b.H;
    HnswGraph &g = H->g;
    knn_index_s *f = H->flat;
    // Level-0 candidates come from the device once the graph has enough nodes above level 0 for a coarse entry
    // scan: the same beam kernel as the search, ef = efConstruction, entered at the exact nearest of those nodes.
    // (Entering through the greedy descent, one cluster in eight of a 10 M-row graph was linked to the wrong
    // neighbourhood: recall@100 stalled at 0.88 whatever the efSearch.)  The upper levels -- one node in M has
    // any -- are still searched by the host walkers.
    bool dev = H->device_beam && H->coarse_entries > 0 && f->dp <= 1024 && f->dp == f->d && H->efConstruction <= 1024 &&
               g.ntotal() < (1ll << 31) && hnsw_env_int("KNN355_HNSW_HOST_BEAM", 0) == 0; // (read for every batch; the search reads it once per process)
    if (dev && (H->nbr0_dirty || H->mirror_count != H->linked_count)) {
        // (the mirror is rebuilt from the host graph, which holds the new nodes already: they have no links yet)
        int rc = hnsw_upload_graph(H);
        if (rc) return rc;
    }
    if (dev && H->ncoarse < 64) dev = false;
    const bool dev_links = dev && H->device_links && b.M0 <= 255;
    if (!dev_links && H->host0_stale) { // (this batch reads and writes the host's level-0 lists)
        int rc = hnsw_host0_sync(H);
        if (rc) return rc;
    }
    b.dev = dev;
    b.dev_links = dev_links;
    HNSW_PROF(7, b.tp); // (re)building the device mirror
    return 0;
}

// 1. search the frozen graph for every new point -> b.lc (with dev_links, level 0 is linked here as well)
static int hnsw_batch_candidates(HnswBatch &b)
{
    knn_hnsw_s *H = b.H;
    HnswGraph &g = H->g;
    knn_index_s *f = H->flat;
    const int64_t *ids = b.ids;
    const int count = b.count;
    const bool dev = b.dev;
    std::vector<std::vector<std::vector<DistId>>> &lc = b.lc;
    lc.assign((size_t)count, std::vector<std::vector<DistId>>());
    int rc;
    {
        std::vector<int> widx; // points that need a host walker
        std::vector<int> up;   // points with levels above 0 whose candidates come from the device
        const bool dev_upper = dev && hnsw_env_int("KNN355_HNSW_HOST_UPPER", 0) == 0;
        for (int i = 0; i < count; i++) {
            const int top = std::min(g.levels[ids[i]], g.max_level);
            if (!dev) widx.push_back(i);
            else if (top >= 1) (dev_upper ? up : widx).push_back(i);
        }
        if (!up.empty()) {
            std::vector<int> starved;
            rc = hnsw_upper_candidates_device(H, ids, up, lc, starved);
            if (rc) return rc;
            for (int i : starved) { // (the scan found too few nodes of their highest levels: host walkers, every upper level)
                lc[(size_t)i].clear();
                widx.push_back(i);
            }
            H->stat_starved += (int64_t)starved.size();
        }
        std::vector<Walker> ws(widx.size());
        for (size_t wi = 0; wi < widx.size(); wi++) {
            Walker &w = ws[wi];
            const int64_t id = ids[widx[wi]];
            w.qslot = (uint32_t)id;
            w.ef = H->efConstruction;
            w.greedy_until = std::min(g.levels[id], g.max_level);
            w.stop_level = dev ? 1 : 0;
            w.phase = 0;
        }
        if (!ws.empty()) {
            rc = hnsw_walk(H, ws, f->xb, f->yn, true);
            if (rc) return rc;
        }
        for (size_t wi = 0; wi < widx.size(); wi++) lc[widx[wi]] = std::move(ws[wi].level_cands);
    }
    HNSW_PROF(0, b.tp); // host walkers (upper levels)
    if (b.dev_links) {
        // level 0 stays on the device: candidates, selection, links, reverse links (the phases below then see the upper levels only)
        rc = hnsw_level0_links_device(H, ids, count);
        if (rc) return rc;
        b.tp = now_s(); // (the function keeps its own account of the phases)
    } else if (dev) {
        std::vector<std::vector<DistId>> cand0;
        rc = hnsw_level0_candidates_device(H, ids, count, cand0);
        if (rc) return rc;
        for (int i = 0; i < count; i++) {
            if (lc[i].empty()) lc[i].resize(1);
            lc[i][0] = std::move(cand0[i]);
        }
    }
    HNSW_PROF(1, b.tp); // level-0 candidates on the device
    return 0;
}

// 2. forward selection: one group per (point, level) with candidates -> b.jobs, b.fwd
static int hnsw_batch_select(HnswBatch &b)
{
    knn_hnsw_s *H = b.H;
    const HnswGraph &g = H->g;
    const int64_t *ids = b.ids;
    const int M0 = b.M0;
    const std::vector<std::vector<std::vector<DistId>>> &lc = b.lc;
    std::vector<BatchJob> &jobs = b.jobs;
    for (int i = 0; i < b.count; i++)
        for (int l = 0; l < (int)lc[i].size(); l++)
            if (!lc[i][l].empty()) jobs.push_back({i, l});
    std::vector<std::vector<DistId>> &fwd = b.fwd;
    fwd.assign(jobs.size(), std::vector<DistId>());
    if (!jobs.empty()) {
        size_t nmem = 0;
        for (auto &j : jobs) nmem += 1 + std::min<size_t>(lc[j.point][j.level].size(), SHRINK_MAX_MEMBERS - 1);
        ShrinkStage st;
        int rc = hnsw_shrink_stage(H, jobs.size(), nmem, st);
        if (rc) return rc;
        int32_t *goff = st.goff;
        uint32_t *mem = st.mem;
        int32_t *maxo = st.maxo;
        size_t o = 0, largest = 0;
        for (size_t j = 0; j < jobs.size(); j++) { // (offsets first, then the host threads fill their groups)
            goff[j] = (int32_t)o;
            const size_t nm = 1 + std::min<size_t>(lc[jobs[j].point][jobs[j].level].size(), SHRINK_MAX_MEMBERS - 1);
            largest = std::max(largest, nm);
            o += nm;
        }
        goff[jobs.size()] = (int32_t)o;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t j = 0; j < (int64_t)jobs.size(); j++) {
            size_t w = (size_t)goff[j];
            mem[w++] = (uint32_t)ids[jobs[j].point];
            const auto &cl = lc[jobs[j].point][jobs[j].level];
            const size_t take = std::min<size_t>(cl.size(), SHRINK_MAX_MEMBERS - 1);
            for (size_t c = 0; c < take; c++) mem[w++] = cl[c].second;
            maxo[j] = g.nb_neighbors(jobs[j].level);
        }
        rc = hnsw_run_shrink(H, (int)jobs.size(), o, M0, (int)largest);
        if (rc) return rc;
        const uint32_t *oid = (const uint32_t *)H->h_oid.p;
        const float *od = (const float *)H->h_od.p;
        const int32_t *on = (const int32_t *)H->h_on.p;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t j = 0; j < (int64_t)jobs.size(); j++) {
            fwd[j].reserve((size_t)on[j]);
            for (int c = 0; c < on[j]; c++) fwd[j].push_back(DistId(od[j * M0 + c], oid[j * M0 + c]));
        }
    }
    HNSW_PROF(2, b.tp); // forward selection (gram_shrink)
    return 0;
}

// 3. write forward links; collect reverse link requests per (node, level), sorted by rev_less -> b.revs, b.dirty
static void hnsw_batch_forward_links(HnswBatch &b)
{
    HnswGraph &g = b.H->g;
    const int64_t *ids = b.ids;
    const std::vector<BatchJob> &jobs = b.jobs;
    const std::vector<std::vector<DistId>> &fwd = b.fwd;
    std::vector<BatchRev> &revs = b.revs;
    {
        std::vector<size_t> roff(jobs.size() + 1, 0);
        for (size_t j = 0; j < jobs.size(); j++) roff[j + 1] = roff[j] + fwd[j].size();
        revs.resize(roff[jobs.size()]);
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t j = 0; j < (int64_t)jobs.size(); j++) {
            const uint32_t pid = (uint32_t)ids[jobs[j].point];
            uint32_t *l = g.list(pid, jobs[j].level);
            int c = 0;
            size_t w = roff[j];
            for (auto &e : fwd[j]) {
                l[c++] = e.second;
                revs[w++] = BatchRev{e.second, jobs[j].level, pid, e.first};
            }
            if (jobs[j].level == 0) g.cnt0[pid] = (uint8_t)c;
        }
    }
    if (!b.dev_links) // (the device wrote the new nodes' rows itself)
        for (int i = 0; i < b.count; i++) b.dirty.push_back((uint32_t)ids[i]);
    {
        // sorted in slices by the host threads, then merged pairwise (the order is total: the result does not depend on
        // the number of threads)
        const int nt = std::max(1, std::min<int>(hnsw_threads(), (int)(revs.size() / 65536)));
        if (nt <= 1) {
            std::sort(revs.begin(), revs.end(), rev_less);
        } else {
            std::vector<size_t> cut((size_t)nt + 1);
            for (int t = 0; t <= nt; t++) cut[t] = revs.size() * (size_t)t / nt;
#pragma omp parallel for schedule(static, 1) num_threads(nt)
            for (int t = 0; t < nt; t++) std::sort(revs.begin() + cut[t], revs.begin() + cut[t + 1], rev_less);
            for (int w = 1; w < nt; w *= 2) {
#pragma omp parallel for schedule(static, 1) num_threads(nt)
                for (int t = 0; t < nt; t += 2 * w)
                    if (t + w < nt) std::inplace_merge(revs.begin() + cut[t], revs.begin() + cut[t + w], revs.begin() + cut[std::min(nt, t + 2 * w)], rev_less);
            }
        }
    }
    HNSW_PROF(3, b.tp); // forward links + sorting the reverse requests
}

// 4. reverse links: append where there is room, otherwise the list goes to b.prunes
static void hnsw_batch_reverse_append(HnswBatch &b)
{
    HnswGraph &g = b.H->g;
    const std::vector<BatchRev> &revs = b.revs;
    {
        // groups of requests for one (node, level): every group writes its own list, so the groups are shared out to the host
        // threads (cut at group boundaries); the per-thread results are concatenated in thread order = request order
        const int nt = std::max(1, std::min<int>(hnsw_threads(), (int)(revs.size() / 65536)));
        std::vector<size_t> cut((size_t)nt + 1, revs.size());
        cut[0] = 0;
        for (int t = 1; t < nt; t++) {
            size_t c = revs.size() * (size_t)t / nt;
            while (c < revs.size() && c > 0 && revs[c].node == revs[c - 1].node && revs[c].level == revs[c - 1].level) c++;
            cut[t] = std::max(c, cut[t - 1]);
        }
        std::vector<std::vector<BatchPrune>> tp_prunes((size_t)nt);
        std::vector<std::vector<uint32_t>> tp_dirty((size_t)nt);
#pragma omp parallel for schedule(static, 1) num_threads(nt)
        for (int t = 0; t < nt; t++) {
            for (size_t r0 = cut[t]; r0 < cut[t + 1];) {
                size_t r1 = r0;
                while (r1 < cut[t + 1] && revs[r1].node == revs[r0].node && revs[r1].level == revs[r0].level) r1++;
                uint32_t *l = g.list(revs[r0].node, revs[r0].level);
                const int cap = g.nb_neighbors(revs[r0].level);
                int have = 0;
                if (revs[r0].level == 0) have = g.cnt0[revs[r0].node];
                else while (have < cap && l[have] != HNSW_EMPTY) have++;
                if (revs[r0].level == 0) tp_dirty[t].push_back(revs[r0].node);
                if (have + (int)(r1 - r0) <= cap) {
                    for (size_t r = r0; r < r1; r++) l[have++] = revs[r].from;
                    if (revs[r0].level == 0) g.cnt0[revs[r0].node] = (uint8_t)have;
                } else {
                    tp_prunes[t].push_back({revs[r0].node, revs[r0].level, r0, r1});
                }
                r0 = r1;
            }
        }
        for (int t = 0; t < nt; t++) {
            b.prunes.insert(b.prunes.end(), tp_prunes[t].begin(), tp_prunes[t].end());
            b.dirty.insert(b.dirty.end(), tp_dirty[t].begin(), tp_dirty[t].end());
        }
    }
    HNSW_PROF(4, b.tp); // reverse links appended
}

// ... the overfull lists pruned on the GPU: the node, its links and the closest new ones are one group each
static int hnsw_batch_prune(HnswBatch &b)
{
    knn_hnsw_s *H = b.H;
    HnswGraph &g = H->g;
    const int M0 = b.M0;
    const std::vector<BatchRev> &revs = b.revs;
    const std::vector<BatchPrune> &prunes = b.prunes;
    if (!prunes.empty()) {
        size_t nmem = prunes.size() * (size_t)SHRINK_MAX_MEMBERS;
        ShrinkStage st;
        int rc = hnsw_shrink_stage(H, prunes.size(), nmem, st);
        if (rc) return rc;
        int32_t *goff = st.goff;
        uint32_t *mem = st.mem;
        int32_t *maxo = st.maxo;
        size_t o = 0, largest = 0;
        for (size_t j = 0; j < prunes.size(); j++) {
            goff[j] = (int32_t)o;
            largest = std::max(largest, o - (j ? (size_t)goff[j - 1] : 0));
            const uint32_t *l = g.list(prunes[j].node, prunes[j].level);
            const int cap = g.nb_neighbors(prunes[j].level);
            mem[o++] = prunes[j].node;
            int nm = 1;
            for (int c = 0; c < cap && l[c] != HNSW_EMPTY; c++, nm++) mem[o++] = l[c];
            // closest new links first (revs are sorted by distance), as many as fit
            for (size_t r = prunes[j].r0; r < prunes[j].r1 && nm < SHRINK_MAX_MEMBERS; r++, nm++) mem[o++] = revs[r].from;
            maxo[j] = cap;
        }
        goff[prunes.size()] = (int32_t)o;
        largest = std::max(largest, o - (size_t)goff[prunes.size() - 1]);
        rc = hnsw_run_shrink(H, (int)prunes.size(), o, M0, (int)largest);
        if (rc) return rc;
        const uint32_t *oid = (const uint32_t *)H->h_oid.p;
        const int32_t *on = (const int32_t *)H->h_on.p;
        for (size_t j = 0; j < prunes.size(); j++) {
            uint32_t *l = g.list(prunes[j].node, prunes[j].level);
            const int cap = g.nb_neighbors(prunes[j].level);
            for (int c = 0; c < cap; c++) l[c] = c < on[j] ? oid[j * M0 + c] : HNSW_EMPTY;
            if (prunes[j].level == 0) g.cnt0[prunes[j].node] = (uint8_t)std::min(on[j], cap);
        }
    }
    HNSW_PROF(5, b.tp); // reverse pruning (gram_shrink)
    return 0;
}

// 5. entry point / max level; 6. the device mirror follows (changed level-0 rows, new nodes above level 0 join the coarse index)
static int hnsw_batch_entry_and_mirror(HnswBatch &b)
{
    knn_hnsw_s *H = b.H;
    HnswGraph &g = H->g;
    for (int i = 0; i < b.count; i++) {
        const int64_t id = b.ids[i];
        if (g.levels[id] > g.max_level) {
            g.max_level = g.levels[id];
            g.entry = id;
        }
    }
    if (b.dev) {
        int rc = hnsw_mirror_update(H, b.ids, b.count, b.dirty);
        HNSW_PROF(6, b.tp); // device mirror + coarse index update
        return rc;
    }
    H->nbr0_dirty = true;
    return 0;
}

// inserts rows ids[0 .. count) (ascending; already stored in the flat index, not linked yet) into the graph
static int hnsw_insert_batch(knn_hnsw_s *H, const int64_t *ids, int count)
{
    HnswBatch b;
    b.H = H;
    b.ids = ids;
    b.count = count;
    b.M0 = H->g.nb_neighbors(0);
    b.tp = now_s();
    int rc = hnsw_batch_paths(b);
    if (!rc) rc = hnsw_batch_candidates(b);
    if (!rc) rc = hnsw_batch_select(b);
    if (rc) return rc;
    hnsw_batch_forward_links(b);
    hnsw_batch_reverse_append(b);
    rc = hnsw_batch_prune(b);
    if (rc) return rc;
    return hnsw_batch_entry_and_mirror(b);
}


// links rows [n0, n0 + n) (already stored in the flat index) into the graph
static int hnsw_link_rows(knn_hnsw_s *H, int64_t n0, int64_t n)
{
    for (int64_t i = 0; i < n; i++) H->g.append_node(H->g.random_level());
    H->linked.resize((size_t)H->g.ntotal(), 0);
    // the device mirror holds one row per node: too small for the new total -> rebuilt at the next use
    if ((size_t)H->g.ntotal() * H->g.nb_neighbors(0) * 4 > H->d_nbr0.bytes) H->nbr0_dirty = true;
    std::vector<int64_t> order = hnsw_link_order(n0, n, H->shuffle != 0);
    int64_t pos = 0;
    while (pos < n) {
        const int64_t b = hnsw_batch_rows(H->linked_count, n, pos, H->max_batch);
        if (H->g.entry < 0) {
            // very first point: becomes the entry point, no links yet
            const int64_t id = order[(size_t)pos];
            H->g.entry = id;
            H->g.max_level = H->g.levels[id];
            H->linked[(size_t)id] = 1;
            H->linked_count++;
            pos += 1;
            H->nbr0_dirty = true;
            continue;
        }
        std::sort(order.begin() + pos, order.begin() + pos + b); // (inside a batch the order means nothing: ascending rows read better)
        int rc = hnsw_insert_batch(H, order.data() + pos, (int)b);
        if (rc) return rc;
        for (int64_t i = 0; i < b; i++) H->linked[(size_t)order[(size_t)(pos + i)]] = 1;
        H->linked_count += b;
        pos += b;
    }
    return 0;
}

extern "C" int knn_hnsw_add(knn_hnsw_s *H, const float *x_host, int64_t n)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_add: null handle");
    if (n < 0) return set_err(KNN_ERR_INVALID, "hnsw_add: negative n");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(H->mu);
    const int64_t n0 = H->g.ntotal();
    int rc = knn_flat_add(H->flat, x_host, n); // rows + norms on the device
    if (rc) return rc;
    HIP_TRY(hipSetDevice(H->flat->device));
    return hnsw_link_rows(H, n0, n);
}

// rows already on the device ([n][d] contiguous): no host copy of the database is needed to build the graph
extern "C" int knn_hnsw_add_dev(knn_hnsw_s *H, const float *x_dev, int64_t n, void *stream)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_add: null handle");
    if (n < 0) return set_err(KNN_ERR_INVALID, "hnsw_add: negative n");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(H->mu);
    const int64_t n0 = H->g.ntotal();
    int rc = knn_flat_add_dev(H->flat, x_dev, n, stream); // (synchronises)
    if (rc) return rc;
    HIP_TRY(hipSetDevice(H->flat->device));
    return hnsw_link_rows(H, n0, n);
}
