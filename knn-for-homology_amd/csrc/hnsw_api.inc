// hnsw_api.inc -- the other exported HNSW entries: create, free, the setters and getters, graph export / import, stats.

extern "C" int knn_hnsw_create(int32_t d, int32_t M, int32_t metric, knn_hnsw_s **out)
{
    if (!out) return set_err(KNN_ERR_INVALID, "hnsw_create: null out");
    if (M < 2 || M > 63) return set_err(KNN_ERR_INVALID, "hnsw_create: M must be in [2, 63] (2M+1 rows per pruning group <= 128)");
    knn_handle flat = nullptr;
    int rc = knn_flat_create(d, metric, &flat);
    if (rc) return rc;
    knn_hnsw_s *H = new knn_hnsw_s();
    H->flat = flat;
    H->g.init(M);
    // the level-0 beam walks on bf16 copies of the rows, kept by the storage index beside the fp32 rows (+50 % memory;
    // every returned row is re-scored from the fp32 rows).  KNN355_HNSW_BEAM_FP32=1: no copies, the beam reads fp32.
    // (rows wider than the device beam serves are walked on the host: no copies for those)
    if (round_up(d, 32) <= 1024 && hnsw_env_int("KNN355_HNSW_BEAM_FP32", 0) == 0) {
        rc = flat_keep16(flat);
        if (rc) {
            knn_free(flat);
            delete H;
            return rc;
        }
    }
    *out = H;
    return 0;
}

extern "C" void knn_hnsw_free(knn_hnsw_s *H)
{
    if (!H) return;
    if (hipSetDevice(H->flat->device) == hipSuccess) {
#define X(name) H->name.release();
        HNSW_DEV_BUFS(X)
        HNSW_PINNED_BUFS(X)
#undef X
        if (H->stream2) (void)hipStreamDestroy(H->stream2);
        for (auto &e : H->ev_pairs)
            if (e) (void)hipEventDestroy(e);
    }
    if (H->coarse) knn_free(H->coarse);
    if (H->coarse2) knn_free(H->coarse2);
    knn_free(H->flat);
    delete H;
}

extern "C" int knn_hnsw_set_ef(knn_hnsw_s *H, int32_t efSearch, int32_t efConstruction)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_set_ef: null handle");
    std::lock_guard<std::mutex> lk(H->mu);
    if (efSearch > 0) H->efSearch = efSearch;
    // efConstruction is the width of the construction beam, as in FAISS, and is kept as given.  The closest
    // SHRINK_MAX_MEMBERS - 1 of the beam's candidates, by the walk's key, take part in the selection; above 1024 the device
    // beam is off and host walkers link the rows (hnsw_insert_batch).
    if (efConstruction > 0) H->efConstruction = efConstruction;
    return 0;
}

// walk tuning (not part of the faiss surface): candidates expanded per walker per round
// (1 = strict best-first order) and walkers per lock-step batch
extern "C" int knn_hnsw_set_walk(knn_hnsw_s *H, int32_t expand, int32_t max_batch)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_set_walk: null handle");
    std::lock_guard<std::mutex> lk(H->mu);
    if (expand > 0) H->expand = std::min(expand, 64);
    if (max_batch > 0) H->max_batch = std::min(max_batch, 1 << 16);
    return 0;
}

// entry points of the level-0 walk: n > 0 -- the n nearest nodes above level 0, found by an exact scan on the flat
// kernel (default 4); 0 -- the classic greedy descent through the upper levels
extern "C" int knn_hnsw_set_entry(knn_hnsw_s *H, int32_t coarse_entries)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_set_entry: null handle");
    if (coarse_entries < 0 || coarse_entries > 64) return set_err(KNN_ERR_INVALID, "hnsw_set_entry: 0..64 entry points");
    std::lock_guard<std::mutex> lk(H->mu);
    if ((coarse_entries > 0) != (H->coarse_entries > 0)) H->nbr0_dirty = true; // (the coarse index exists only when used)
    H->coarse_entries = coarse_entries;
    return 0;
}

extern "C" int knn_hnsw_get_params(knn_hnsw_s *H, int32_t *M, int32_t *efSearch, int32_t *efConstruction, int32_t *max_level,
                                   int64_t *entry_point)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_get_params: null handle");
    if (M) *M = H->g.M;
    if (efSearch) *efSearch = H->efSearch;
    if (efConstruction) *efConstruction = H->efConstruction;
    if (max_level) *max_level = H->g.max_level;
    if (entry_point) *entry_point = H->g.entry;
    return 0;
}

extern "C" int64_t knn_hnsw_ntotal(knn_hnsw_s *H) { return H ? H->g.ntotal() : -1; }
extern "C" knn_handle knn_hnsw_storage(knn_hnsw_s *H) { return H ? H->flat : nullptr; }

// graph export / import (serialisation, tests)
extern "C" int knn_hnsw_graph_sizes(knn_hnsw_s *H, int64_t *ntotal, int64_t *nslots, int32_t *nlevels_tab)
{
    if (!H) return set_err(KNN_ERR_INVALID, "null handle");
    if (ntotal) *ntotal = H->g.ntotal();
    if (nslots) *nslots = (int64_t)H->g.nbrs.size();
    if (nlevels_tab) *nlevels_tab = (int32_t)H->g.cum_nb.size();
    return 0;
}
extern "C" int knn_hnsw_graph_export(knn_hnsw_s *H, int32_t *levels, int64_t *offsets, int32_t *nbrs, int32_t *cum_nb,
                                     double *assign_probas)
{
    if (!H) return set_err(KNN_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(H->mu);
    if (H->host0_stale) {
        int rc0 = hnsw_host0_sync(H);
        if (rc0) return rc0;
    }
    const HnswGraph &g = H->g;
    for (size_t i = 0; i < g.levels.size(); i++) levels[i] = g.levels[i];
    for (size_t i = 0; i < g.offsets.size(); i++) offsets[i] = (int64_t)g.offsets[i];
    for (size_t i = 0; i < g.nbrs.size(); i++) nbrs[i] = g.nbrs[i] == HNSW_EMPTY ? -1 : (int32_t)g.nbrs[i];
    for (size_t i = 0; i < g.cum_nb.size(); i++) cum_nb[i] = g.cum_nb[i];
    if (assign_probas)
        for (size_t i = 0; i < g.assign_probas.size(); i++) assign_probas[i] = g.assign_probas[i];
    return 0;
}
// storage rows must already be in place (knn_hnsw_storage + knn_flat_add)
extern "C" int knn_hnsw_graph_import(knn_hnsw_s *H, int64_t ntotal, const int32_t *levels, const int32_t *nbrs, int64_t nslots,
                                     int32_t max_level, int64_t entry_point)
{
    if (!H) return set_err(KNN_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(H->mu);
    HnswGraph &g = H->g;
    if (g.ntotal() != 0) return set_err(KNN_ERR_INVALID, "hnsw_graph_import: graph not empty");
    if (ntotal != H->flat->ntotal) return set_err(KNN_ERR_INVALID, "hnsw_graph_import: storage holds a different number of rows");
    // every refusal from here on leaves the graph empty
    auto refuse = [&](const char *why) {
        const int M = g.M;
        g = HnswGraph();
        g.init(M);
        return set_err(KNN_ERR_INVALID, why);
    };
    for (int64_t i = 0; i < ntotal; i++) {
        if (levels[i] < 0 || levels[i] + 1 >= (int)g.cum_nb.size()) return refuse("hnsw_graph_import: bad level");
        g.append_node(levels[i]);
    }
    if ((int64_t)g.nbrs.size() != nslots) return refuse("hnsw_graph_import: neighbour table size mismatch");
    for (int64_t i = 0; i < nslots; i++) {
        if (nbrs[i] >= ntotal || nbrs[i] < -1) return refuse("hnsw_graph_import: neighbour id out of range");
        g.nbrs[i] = nbrs[i] < 0 ? HNSW_EMPTY : (uint32_t)nbrs[i];
    }
    // a walk at level l >= 1 reads list(node, l) of every node it is handed there: a node named at a level it does not have
    // owns no such slots, and the read would run into the next node's (past the table's end for the last node).  Every slot
    // counts, the ones behind a hole too: construction appends to these lists.
    for (int64_t i = 0; i < ntotal; i++)
        for (int l = 1; l <= g.levels[i]; l++) {
            const uint32_t *ul = g.list(i, l);
            for (int c = 0; c < g.nb_neighbors(l); c++)
                if (ul[c] != HNSW_EMPTY && g.levels[ul[c]] < l)
                    return refuse("hnsw_graph_import: an upper-level list names a node that does not have that level");
        }
    // (an imported list may have holes: the fill is the position of the first one, as in FAISS, whose walk stops at the
    // first -1.  What lies behind it is not part of the list and is dropped here: the device beam reads a level-0 list as
    // one whole row and tells links from empty slots by value, so ids left behind a hole would be walked on the device and
    // not on the host)
    for (int64_t i = 0; i < ntotal; i++) {
        uint32_t *l = g.list(i, 0);
        const int cap = g.nb_neighbors(0);
        int have = 0;
        while (have < cap && l[have] != HNSW_EMPTY) have++;
        g.cnt0[i] = (uint8_t)have;
        for (int c = have; c < cap; c++) l[c] = HNSW_EMPTY;
    }
    // the walk starts at (entry_point, max_level): both must describe a node of this graph
    const bool empty_ok = ntotal == 0 && entry_point == -1;
    if (!empty_ok && (entry_point < 0 || entry_point >= ntotal || max_level != g.levels[entry_point]))
        return refuse("hnsw_graph_import: entry point / max level do not match the level table");
    g.max_level = ntotal ? max_level : -1;
    g.entry = entry_point;
    H->nbr0_dirty = true;
    H->linked.assign((size_t)ntotal, 1);
    H->linked_count = ntotal;
    return 0;
}

extern "C" int knn_hnsw_stats(knn_hnsw_s *H, int64_t *pairs, int64_t *rounds, int64_t *shrinks, double *gpu_s, double *host_s,
                              int32_t reset)
{
    if (!H) return set_err(KNN_ERR_INVALID, "null handle");
    if (pairs) *pairs = H->stat_pairs;
    if (rounds) *rounds = H->stat_rounds;
    if (shrinks) *shrinks = H->stat_shrinks;
    if (gpu_s) *gpu_s = H->stat_gpu_s;
    if (host_s) *host_s = H->stat_host_s;
    if (reset) { H->stat_pairs = H->stat_rounds = H->stat_shrinks = 0; H->stat_gpu_s = H->stat_host_s = 0; }
    return 0;
}
