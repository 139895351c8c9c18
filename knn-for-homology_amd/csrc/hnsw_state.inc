// hnsw_state.inc -- what an HNSW handle owns: the KNN355_HNSW_* knob reader, pinned staging memory, the two buffer lists, knn_hnsw_s,
// hnsw_grow, the host threads, the developer profile.
#include <omp.h>
#include <sched.h>
#include <queue>

struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need)
    {
        if (need <= bytes) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        size_t want = need + need / 2;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return -1;
        bytes = want;
        return 0;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

// ---------------------------------------------------------------------------
// The environment knobs of the HNSW files, all read through the functions below (nothing else in hnsw_*.inc reads the environment).
// Rules:  on      set to a number other than 0        hnsw_env_int(name, 0) != 0
//         off     set to 0 (or to no number at all)   hnsw_env_int(name, 1) == 0
//         is      set to exactly this text             hnsw_env_is(name, text)
//         set     present, whatever the value          hnsw_env_set(name)
//
//   name (KNN355_HNSW_...)  rule            default            read                        used by
//   ORDER                   is "sequential" shuffled link order at create (knn_hnsw_s)     test_hnsw_gpu, test_hnsw_build_exact_gpu
//   EXPAND1                 on              two expansions/step at create                  (developer A/B)
//   BEAM_ROWS               number, 8 or 4  4 rows in flight    at create                  test_hnsw_exact_gpu
//   COARSE_FP32             on              bf16 coarse scan    at create                  test_hnsw_gpu, test_hnsw_entry_exact_gpu
//   HOST_LINKS              on              level-0 links on the device  at create         test_hnsw_gpu, test_hnsw_build_exact_gpu
//   BEAM_FP32               on              bf16 row copies kept         at create (knn_hnsw_create)  test_hnsw_exact_gpu, test_hnsw_gpu, test_hnsw_build_exact_gpu
//   HOST_BEAM               on              device beam         construction: every batch (hnsw_insert_batch);
//                                                               search: ONCE PER PROCESS, at the first knn_hnsw_search that
//                                                               gets that far (a function-local static)  test_hnsw_build_exact_gpu
//   HOST_UPPER              on              upper candidates from the coarse scan  every batch  test_hnsw_build_exact_gpu
//   STARVED_FALLBACK        off             fallback to host walkers  once per process (hnsw_upper_candidates_device)  (developer A/B)
//   CLEAR                   is "lazy" / is "eager"  by graph size  every launch of the beam pipeline  test_hnsw_exact_gpu, test_hnsw_gpu
//   KEYS_DIRECT             set             LDS-staged re-scoring    every launch of the beam pipeline  test_hnsw_exact_gpu
//   DEBUG                   set             silent              every mirror rebuild, developer builds (KNN355_DEV) only  --
//   KNN355_THREADS          number >= 1     CPU affinity, at most 16  once per process (hnsw_threads)  --
//
// HOST_BEAM is the odd one: a process that changes it between two calls changes the construction and not the search.
// The tests set it in child processes before the library loads, where both readings agree.  Which lifetime is meant is
// open; nothing here changes it.
// ---------------------------------------------------------------------------
static inline const char *hnsw_env(const char *name) { return getenv(name); }
static inline bool hnsw_env_set(const char *name) { return hnsw_env(name) != nullptr; }
static inline int hnsw_env_int(const char *name, int unset)
{
    const char *v = hnsw_env(name);
    return v ? atoi(v) : unset;
}
static inline bool hnsw_env_is(const char *name, const char *text)
{
    const char *v = hnsw_env(name);
    return v && !strcmp(v, text);
}

// Every device and pinned buffer of a handle is named once, here: the members of knn_hnsw_s and the release loops of
// knn_hnsw_free are generated from the two lists (in this order).  DevBuf has no destructor on purpose (host_core.inc).
#define HNSW_DEV_BUFS(X)                                                                                                    \
    /* construction candidates (sorted keys); changed level-0 rows on their way to the mirror, also scratch for id lists */ \
    X(d_beam_out) X(d_scatter_ids) X(d_scatter_rows)                                                                        \
    /* coarse entry index: its rows' node ids, the scan's keys */                                                           \
    X(d_coarse_ids) X(d_coarse_keys)                                                                                        \
    /* level-0 neighbour lists mirrored on the device for the beam kernel ([n][M0]); rebuilt after add / import */          \
    X(d_nbr0) X(d_entry) X(d_vis) X(d_touched) X(d_beam_ids) X(d_beam_keys) X(d_D) X(d_I) X(d_stats)                        \
    /* the host walk: pairs and distances of the second half of the walkers, then of the first */                           \
    X(d_pa2) X(d_pb2) X(d_out2) X(d_pa) X(d_pb) X(d_out)                                                                    \
    /* queries and norms; pruning groups staged by the host (hnsw_run_shrink) */                                            \
    X(d_q) X(d_qn) X(d_goff) X(d_mem) X(d_maxo) X(d_oid) X(d_od) X(d_on)                                                    \
    /* second set of result buffers (searches of several batches), the counters of a batch kept for its download */         \
    X(d_D2) X(d_I2) X(d_st2)                                                                                                \
    /* [rows of d_nbr0] fill of every level-0 list */                                                                       \
    X(d_cnt0)                                                                                                               \
    /* the batch being linked: its node ids, its rows gathered ([count][dp]) and their norms */                             \
    X(d_bids) X(d_bq) X(d_bqn)                                                                                              \
    /* level-0 links on the device (hnsw_level0_links_device): groups, selections, reverse requests before (0) and after */ \
    /* (1) the sort, the sort's scratch, counters */                                                                        \
    X(dl_mem) X(dl_goff) X(dl_gcnt) X(dl_maxo) X(dl_gnode) X(dl_oid) X(dl_od) X(dl_on) X(dl_roff)                           \
    X(dl_key0) X(dl_key1) X(dl_from0) X(dl_from1) X(dl_tmp) X(dl_ctr)
#define HNSW_PINNED_BUFS(X)                                                                       \
    X(h_scatter_ids) X(h_scatter_rows) X(h_keys) X(h_entry)                                       \
    /* the walk runs its walkers in two halves: own staging buffers, stream and event each */     \
    X(h_pa2) X(h_pb2) X(h_out2) X(h_pa) X(h_pb) X(h_out)                                          \
    X(h_goff) X(h_mem) X(h_maxo) X(h_oid) X(h_od) X(h_on)

struct knn_hnsw_s {
    knn_index_s *flat = nullptr;
    HnswGraph g;
    int efSearch = 16, efConstruction = 40;
    int max_batch = 16384; // (rows per insertion batch at most: 2 M rows link in 2.1 s against 2.8 s with 4096, same recall)
    int expand = 8; // candidates expanded per walker per lock-step round (1 = strict best-first)
    std::mutex mu;
#define X(name) DevBuf name;
    HNSW_DEV_BUFS(X)
#undef X
#define X(name) PinnedBuf name;
    HNSW_PINNED_BUFS(X)
#undef X
    // the walk runs its walkers in two halves: while the GPU computes the distances of one half
    // the host consumes / proposes for the other (own staging buffers, stream and event each)
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_pairs[2] = {nullptr, nullptr};
    size_t vis_zero_bytes = 0; // leading bytes of d_vis known to be zero (lazy clearing of the visited bitmaps)
    bool nbr0_dirty = true;
    // Rows are linked in a shuffled order (FAISS's hnsw_add_vertices shuffles too, "to get rid of dataset order bias": a
    // batch-synchronous build links a batch against the frozen graph only, and rows that arrive grouped by cluster -- a Pfam
    // FASTA lists its families one after the other -- would otherwise be inserted blind to their own neighbours): the linked
    // nodes are a set, not a prefix
    std::vector<uint8_t> linked;   // [ntotal] node is linked into the graph (the others wait for their batch: no links, never an entry point)
    int64_t linked_count = 0;
    int64_t mirror_count = 0;      // linked nodes the device mirror (level-0 lists, coarse index) reflects
    int shuffle = !hnsw_env_is("KNN355_HNSW_ORDER", "sequential"); // (sequential: rounds 1-3, A/B)
    std::vector<uint32_t> coarse_ids_host;
    knn_index_s *coarse = nullptr; // flat index over the rows of the nodes above level 0 (entry search)
    knn_index_s *coarse2 = nullptr; // ... and one over the rows of the nodes of level >= 2 (construction candidates of those levels)
    std::vector<uint32_t> coarse2_ids_host; // its rows' node ids
    int64_t ncoarse2 = 0;
    int64_t ncoarse = 0;
    int coarse_entries = 4;        // level-0 entry points per query taken from the coarse scan (0: greedy descent on the host)
    int beam_expand2 = hnsw_env_int("KNN355_HNSW_EXPAND1", 0) == 0;
    int beam_rows = hnsw_env_int("KNN355_HNSW_BEAM_ROWS", 4) == 8 ? 8 : 4; // rows in flight per walker
    bool coarse_bf16 = hnsw_env_int("KNN355_HNSW_COARSE_FP32", 0) == 0;
    int device_beam = 1; // 0: walk level 0 on the host as well (the round-1 path; KNN355_HNSW_HOST_BEAM=1)
    // Construction, level 0 on the device (hnsw_level0_links_device): the device's lists are then the master copy of level 0 and
    // the host graph's level-0 lists are brought up to date when something on the host reads them (hnsw_host0_sync).
    // KNN355_HNSW_HOST_LINKS=1: the round-3 path (candidates down, host bookkeeping, dirty rows up).
    int device_links = hnsw_env_int("KNN355_HNSW_HOST_LINKS", 0) == 0;
    bool host0_stale = false;      // level-0 lists are newer on the device than in g.nbrs / g.cnt0
    // stats
    int64_t stat_pairs = 0, stat_rounds = 0, stat_shrinks = 0, stat_expansions = 0;
    int64_t stat_starved = 0; // construction: points whose upper-level candidates fell back to the host walkers
    double stat_gpu_s = 0, stat_host_s = 0;
};

// Grows every (buffer, bytes) pair it is given, device or pinned, in the order given; stops at the first that fails, as
// the || chains this replaces did, and reports `what` once.  No owner event is passed: a device buffer that grows waits
// for the whole device (DevBuf::ensure).
static inline bool hnsw_grow_any() { return false; }
template <class Buf, class... Rest>
static inline bool hnsw_grow_any(Buf &b, size_t bytes, Rest &&...rest)
{
    return b.ensure(bytes) || hnsw_grow_any(rest...);
}
template <class... Pairs>
static inline int hnsw_grow(const char *what, Pairs &&...pairs)
{
    return hnsw_grow_any(pairs...) ? set_err(KNN_ERR_HIP, what) : 0;
}

// host threads for the walk: the CPUs this process may run on, at most 16 (a GPU box hands
// each single-GPU job about that share of the machine; more threads only spin); KNN355_THREADS
// overrides
static int hnsw_threads()
{
    static int nt = 0;
    if (nt == 0) {
        int n = 1;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
        if (hnsw_env_set("KNN355_THREADS")) nt = std::max(1, hnsw_env_int("KNN355_THREADS", 1));
        else nt = std::max(1, std::min(n, 16));
    }
    return nt;
}

static double now_s()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

#ifdef KNN355_DEV
static double g_hnsw_prof[8] = {0};
#define HNSW_PROF(i, t0) do { g_hnsw_prof[i] += now_s() - (t0); (t0) = now_s(); } while (0)
#else
#define HNSW_PROF(i, t0) do { } while (0)
#endif
#ifdef KNN355_DEV
extern "C" void knn_dev_hnsw_profile(double *out8, int reset)
{
    for (int i = 0; i < 8; i++) {
        out8[i] = g_hnsw_prof[i];
        if (reset) g_hnsw_prof[i] = 0;
    }
}
#endif
