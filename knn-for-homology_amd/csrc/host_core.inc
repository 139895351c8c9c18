// host_core.inc -- what the whole host side stands on (included by knn355_lib.hip right behind knn355.hip): the error
// channel, the owners of what one call holds and its phase clock (DESIGN 4.10), the device and stream pools, DevBuf, knn_index_s with its
// scratch helpers, knn_init, the normalize / norm / pad helpers with knn_normalize_l2*, the copy pipes and HostCall.
// ===========================================================================
// host side
// ===========================================================================
static thread_local std::string g_err;
static thread_local int g_device = 0;

static int set_err(int code, const std::string &msg)
{
    g_err = msg;
    return code;
}
#define HIP_TRY(expr)                                                                         \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return set_err(KNN_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));   \
    } while (0)

// ---- what one call owns (DESIGN 4.10): every host entry releases its transient device memory, events and streams
// through these and HostCall below, whichever way it returns
// device buffers of one call, straight from hipMalloc and hipFree'd with it
struct EvalBufs {
    std::vector<std::pair<void *, size_t>> dev;
    bool oom = false; // a get() has failed
    ~EvalBufs() { for (auto &b : dev) if (b.first) (void)hipFree(b.first); }
    void *get(size_t bytes)
    {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) {
            oom = true;
            return nullptr;
        }
        dev.push_back({p, bytes});
        return p;
    }
};
// a device-only buffer
#define EVAL_ALLOC(var, type, bytes)                                                    \
    type var = (type)bufs.get(bytes);                                                   \
    if (!var) return set_err(KNN_ERR_HIP, "eval: out of device memory")
#define EVAL_TRY(expr)                                                                  \
    do {                                                                                \
        const int rc_ = (expr);                                                         \
        if (rc_) return rc_;                                                            \
    } while (0)

// HIP events of one call that are not phase timing (ordering events, pairs recorded again and again), in the order they
// were recorded
struct EventList {
    std::vector<hipEvent_t> ev;
    ~EventList()
    {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
    int mark(hipStream_t s, unsigned flags = 0)
    {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, flags));
        ev.push_back(e);
        HIP_TRY(hipEventRecord(e, s));
        return 0;
    }
};

// The HIP-event times of one call, by phase: every interval of enqueued work belongs to one phase (an enum next to the
// entry's thread_local result), and the time of a phase is the sum over its intervals.  One interval is open at a time.  The
// caller reads into a local array once its streams have drained and copies that to where the getters look only when the
// whole call has succeeded: a failed call leaves the previous figures as they were.
struct PhaseClock {
    static constexpr int NONE = -1;
    struct Mark {
        hipEvent_t e;
        int phase; // of the interval this event starts (it ends at the next event), or NONE
    };
    std::vector<Mark> marks; // in the order they were recorded
    PhaseClock() = default;
    PhaseClock(const PhaseClock &) = delete;
    PhaseClock &operator=(const PhaseClock &) = delete;
    ~PhaseClock()
    {
        for (const Mark &m : marks) (void)hipEventDestroy(m.e);
    }
    hipStream_t stream = nullptr; // of the open interval
    bool is_open() const { return !marks.empty() && marks.back().phase != NONE; }
    // starts an interval of phase p; none may be open
    int open(int p, hipStream_t s)
    {
        if (is_open()) return set_err(KNN_ERR_INVALID, "PhaseClock: open() while an interval is open");
        return next(p, s);
    }
    // ends the open interval
    int close(hipStream_t s)
    {
        if (!is_open()) return set_err(KNN_ERR_INVALID, "PhaseClock: close() without an open interval");
        return next(NONE, s);
    }
    // one event that ends the open interval, if there is one, and starts one of phase p (consecutive phases on one stream:
    // an interval ends on the stream it began on)
    int next(int p, hipStream_t s)
    {
        if (is_open() && s != stream) return set_err(KNN_ERR_INVALID, "PhaseClock: an interval ends on another stream than it began on");
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreateWithFlags(&e, 0));
        marks.push_back({e, NONE}); // (an event that failed to record starts nothing)
        HIP_TRY(hipEventRecord(e, s));
        marks.back().phase = p;
        stream = s;
        return 0;
    }
    // after the streams have drained: ms[p] = the summed time of phase p's intervals, exactly 0.0f where it has none, p < n.
    // ms is written only when every query has succeeded.
    int read(float *ms, int n) const
    {
        if (is_open()) return set_err(KNN_ERR_INVALID, "PhaseClock: read() while an interval is open");
        std::vector<float> sum((size_t)n, 0.0f);
        for (size_t i = 0; i + 1 < marks.size(); i++) {
            if (marks[i].phase == NONE) continue;
            if (marks[i].phase < 0 || marks[i].phase >= n) return set_err(KNN_ERR_INVALID, "PhaseClock: a phase outside the array read()");
            float t = 0;
            HIP_TRY(hipEventElapsedTime(&t, marks[i].e, marks[i + 1].e));
            sum[(size_t)marks[i].phase] += t;
        }
        std::copy(sum.begin(), sum.end(), ms);
        return 0;
    }
};

// Device scratch buffers are recycled through a small per-device pool: the reference's scripts
// build a fresh index per embedding file (cath/search.py:20-24), and hipMalloc/hipFree of the
// gigabyte-sized candidate-list workspace would otherwise dominate their end-to-end time.
struct DevPool {
    struct Item { void *p; size_t bytes; int device; };
    std::mutex mu;
    std::vector<Item> items;
    size_t total = 0;
    static constexpr size_t kMaxBytes = 8ull << 30;
    void *take(size_t need, int device, size_t *got)
    {
        std::lock_guard<std::mutex> lk(mu);
        int best = -1;
        for (int i = 0; i < (int)items.size(); i++)
            if (items[i].device == device && items[i].bytes >= need && items[i].bytes <= need * 4 + (1u << 20) &&
                (best < 0 || items[i].bytes < items[best].bytes))
                best = i;
        if (best < 0) return nullptr;
        void *p = items[best].p;
        *got = items[best].bytes;
        total -= items[best].bytes;
        items.erase(items.begin() + best);
        return p;
    }
    void give(void *p, size_t bytes, int device)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (total + bytes <= kMaxBytes && items.size() < 64) {
                items.push_back({p, bytes, device});
                total += bytes;
                return;
            }
        }
        (void)hipFree(p);
    }
};
static DevPool g_pool;

// database storage goes through the same pool as the scratch buffers
static void *pool_alloc(size_t bytes, int device, size_t *got)
{
    if (void *q = g_pool.take(bytes, device, got)) return q;
    void *p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    *got = bytes;
    return p;
}

// A pool_alloc that goes back to the pool with its scope (null: the allocation failed, or 0 bytes were asked for), unless
// release() has handed it to a new owner.  The destructor waits for nothing: whoever enqueued work on the buffer has
// drained that stream first.
struct PoolBuf {
    void *p = nullptr;
    size_t got = 0;
    int device = 0;
    PoolBuf(size_t bytes, int dev) : device(dev) { if (bytes) p = pool_alloc(bytes, dev, &got); }
    PoolBuf(const PoolBuf &) = delete;
    PoolBuf &operator=(const PoolBuf &) = delete;
    ~PoolBuf() { if (p) g_pool.give(p, got, device); }
    explicit operator bool() const { return p != nullptr; }
    template <typename T> T *get() const { return (T *)p; }
    void *release(size_t *bytes)
    {
        void *q = p;
        *bytes = got;
        p = nullptr;
        return q;
    }
};

extern "C" int64_t knn_trim(void)
{
    std::vector<DevPool::Item> items;
    {
        std::lock_guard<std::mutex> lk(g_pool.mu);
        items.swap(g_pool.items);
        g_pool.total = 0;
    }
    int64_t freed = 0;
    int cur = 0;
    (void)hipGetDevice(&cur);
    for (auto &it : items) {
        if (hipSetDevice(it.device) == hipSuccess && hipFree(it.p) == hipSuccess) freed += (int64_t)it.bytes;
    }
    (void)hipSetDevice(cur);
    return freed;
}

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int device = 0;
    // done / s: the owner's "everything my earlier calls enqueued" event and the stream of the call in progress.  A buffer
    // that grows goes back to the pool, which may hand it to another handle right away: whatever still uses it must have
    // finished.  With both given that is a host wait for the OWNER's work only (its previous calls through `done`, this
    // call's launches through `s`); rounds 1-2 called hipDeviceSynchronize() here, which also stalled the other lane and
    // every caller stream at the first searches of a handle.  Without them (users unknown): the whole device.
    int ensure(size_t need, hipEvent_t done = nullptr, hipStream_t s = nullptr)
    {
        int cur = 0;
        (void)hipGetDevice(&cur);
        if (need <= bytes && cur == device) return 0;
        if (p) {
            (void)hipSetDevice(device);
            if (done && cur == device) {
                (void)hipEventSynchronize(done);
                (void)hipStreamSynchronize(s);
            } else {
                (void)hipDeviceSynchronize();
            }
            (void)hipSetDevice(cur);
        }
        release();
        device = cur;
        size_t got = 0;
        if (void *q = g_pool.take(need, device, &got)) {
            p = q;
            bytes = got;
            return 0;
        }
        size_t want = need + need / 4;
        if (hipMalloc(&p, want) != hipSuccess) {
            if (hipMalloc(&p, need) != hipSuccess) { p = nullptr; return -1; }
            want = need;
        }
        bytes = want;
        return 0;
    }
    void release()
    {
        if (p) g_pool.give(p, bytes, device);
        p = nullptr;
        bytes = 0;
    }
};

#ifdef KNN355_TRACE
static DevBuf g_trace_buf;
static int g_trace_grid = 0;
// developer build only: the stamps of the last traced scan launch, [grid][128]; returns the grid
extern "C" int knn_dev_trace_read(unsigned long long *out, int max_wgs)
{
    const int n = std::min(max_wgs, g_trace_grid);
    if (n > 0 && hipMemcpy(out, g_trace_buf.p, (size_t)n * 128 * 8, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return g_trace_grid;
}
#endif

// per seed-recursion level: compact candidate arrays [nq][qcap] + their fill, the shared running
// thresholds and the verification bounds of a statistically seeded pass
struct LevelBufs {
    DevBuf qlist, qcnt, gthr, qthr;
    DevBuf pub, arrive; // tile-minimum seed: published keys [nslots][rounds * nchunks], arrival counters [nqtiles]
    DevBuf pair_ctr;    // paired walk: ticket counter of every pair of workgroups
    uint64_t clean_sig = 0; // != 0: the last search's selection reset this state for a search of exactly this shape
};

// HIP streams are recycled: creating one costs a third of a millisecond, and the reference's scripts build a fresh
// index per embedding file (cath/search.py:20-24).  A stream goes back to the pool fully drained.
struct StreamPool {
    std::mutex mu;
    std::vector<std::pair<int, hipStream_t>> free_list;
    hipStream_t take(int device)
    {
        {
            std::lock_guard<std::mutex> lk(mu);
            for (size_t i = 0; i < free_list.size(); i++)
                if (free_list[i].first == device) {
                    hipStream_t s = free_list[i].second;
                    free_list.erase(free_list.begin() + i);
                    return s;
                }
        }
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
        return s;
    }
    void give(int device, hipStream_t s)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (free_list.size() < 16) free_list.push_back({device, s});
        else (void)hipStreamDestroy(s);
    }
};
static StreamPool g_streams;

// A stream of the pool for one scope (null: the take failed, or `want` was false); it goes back drained.
struct StreamLease {
    int device;
    hipStream_t s;
    explicit StreamLease(int dev, bool want = true) : device(dev), s(want ? g_streams.take(dev) : nullptr) {}
    StreamLease(const StreamLease &) = delete;
    StreamLease &operator=(const StreamLease &) = delete;
    ~StreamLease()
    {
        if (!s) return;
        (void)hipStreamSynchronize(s);
        g_streams.give(device, s);
    }
    operator hipStream_t() const { return s; }
};

struct knn_index_s {
    int d = 0, dp = 0, metric = 0, device = 0;
    int num_cus = 256;
    int64_t ntotal = 0, cap_rows = 0;
    bool is_view = false; // shares another handle's database (knn_flat_view): read-only, frees nothing of it
    // storage generation: bumped whenever xb/yn are reallocated, reset or freed.  A view remembers the
    // value it was made at and refuses to search once its parent's storage has moved on.
    std::shared_ptr<std::atomic<int64_t>> storage_gen = std::make_shared<std::atomic<int64_t>>(0);
    int64_t view_gen = 0;
    float *xb = nullptr; // [cap_rows][dp]
    bool approx16 = false;  // the scan multiplies bf16 copies of rows and queries (HNSW's coarse entry index: approximate on purpose)
    bool keep16 = false;    // bf16 copies of the rows are kept beside the fp32 ones (HNSW storage: the beam walks on them); scans stay fp32
    DevBuf xb16, ws_q16;    // approx16: [cap_rows][dp] bf16 rows, [nq][dp] bf16 queries
    // exact 16-bit prefilter (knn_flat_set_scan16, DESIGN 4.9): fp16 copies of the rows, [cap_rows][dp16] (dp16 = d rounded
    // up to 64), one int8 exponent per row, the index-wide statistics (S16_*).  Views use their parent's.
    int scan16 = 0;               // 0 off, 1 copies kept, 2 dropped (allocation failed) until the index is reset
    int s16_fmt = 16;             // the copies' format: 16 = fp16 [cap_rows][dp16]; 12 = 12-bit fixed point in tiles (scan12_rows_kernel)
    // the copies cover every row and every row is finite -- shared with the views, so a row added to the parent that is not
    // finite turns the path off for them too
    std::shared_ptr<std::atomic<bool>> s16_ok = std::make_shared<std::atomic<bool>>(false);
    int dp16 = 0;
    DevBuf s16_rows_buf, s16_exp_buf, s16_stat_buf;
    const _Float16 *s16_rows = nullptr;
    const int8_t *s16_exp = nullptr;
    const uint32_t *s16_stat = nullptr;
    std::string s16_note;
    DevBuf ws_q16x, ws_s16q, ws_s16ak, ws_s16ok, ws_s16stat; // fp16 queries; exponents, bounds, flags; keys; [largest window, fallbacks]
    bool last_s16_used = false;   // some piece of the last search (search_keys_impl) took the prefilter
    int last_s16_fmt = 0;         // ... on copies of this format (recorded where the pass is enqueued)
    int s16_pieces = 0;           // ... how many: the first one restarts the largest-window counter
    float *yn = nullptr; // [cap_rows + pad]
    size_t xb_bytes = 0, yn_bytes = 0; // allocation sizes (may exceed the row capacity: pooled)
    hipStream_t stream = nullptr;
    hipEvent_t done = nullptr;               // recorded behind everything a search of this handle enqueued (DevBuf::ensure)
    hipEvent_t ev0 = nullptr, ev1 = nullptr; // the pair of the most recent scan launch
    static const int RING = 64;
    hipEvent_t ring0[RING] = {nullptr}, ring1[RING] = {nullptr};
    int64_t nlaunches = 0;
    std::mutex mu;
    DevBuf ws_q, ws_qn, ws_lists, ws_D, ws_I, ws_tmp, ws_tmp2;
    DevBuf ws_D1, ws_I1, ws_tmp3; // second set for the pipelined host search
    DevBuf ws_flag;               // [0]: a statistically seeded search failed its verification
    DevBuf ws_sym;                // work table of a symmetric all-vs-all launch
    int sym_tiles = -1, sym_run = 0; // ... which is the table for this many tiles (run length sym_run, sym_items entries)
    int sym_ts = 0;               // ... of this many rows each
    int64_t sym_items = 0;
    int sym_groups = 1;           // ... in this many groups of query tiles, one launch each (results streamed to the host group by group)
    std::vector<int64_t> sym_gstart; // [sym_groups + 1] first entry of each group
    DevBuf ws_qdiff;              // difference builds: the queries interleaved by pairs
    DevBuf ws_defer;              // tile-minimum seed: the parked first-tile scores of every workgroup
    DevBuf ws_turn;               // batch launches: one word per CU (the resident workgroups take turns in their K loops)
    void *turn_zeroed = nullptr;  // the ws_turn allocation that has been cleared (every holder gives its word back: a launch leaves them all zero)
    int64_t sym_searches = 0;     // self-searches served by the symmetric path
    static const int MAX_LEVELS = 8;
    LevelBufs ws_level[MAX_LEVELS]; // per seed-recursion level
    int last_seed_stride = 0, last_seed_stat = 0;
    int64_t last_sample_rows = 0; // rows the seed sample took out of the main pass of the last search
    int64_t stat_redo = 0;        // searches repeated because the statistical threshold was too tight
    int *flag_host = nullptr;     // pinned: [slot] copy of ws_flag behind each batch of a host search
    // tuning + introspection
    int force_qt = 0, force_chunks = 0, flags = 0;
    int64_t batch_nq = 0; // the caller's whole batch while a search works through it in pieces (BatchScope); 0: outside a search
    int64_t batch_hint = 0; // knn_flat_set_batch: the calls that follow are pieces of a batch of this many queries (0: each its own)
    int pub_rounds_force = 0; // tile-minimum seed: rounds of publications (0: the host's choice)
    std::string last_kernel;
    int last_qt = 0, last_dt = 0, last_chunks = 0, last_grid = 0;
    // range search (range.inc): scratch, and the results of the last search until knn_flat_range_fetch takes them
    DevBuf ws_rq, ws_rqn, ws_rcnt, ws_rsegD, ws_rsegI, ws_roff, ws_routD, ws_routI, ws_rsel, ws_rq2, ws_rexp;
    std::vector<float> range_D;
    std::vector<int64_t> range_I;
    int64_t range_qblocks = 0, range_redos = 0, range_redo_queries = 0; // query blocks, overflow rescans, queries rescanned
    // refine (refine.inc): queries as uploaded / padded, labels, rescored keys, results; HIP-event times of the last call
    DevBuf ws_rfq, ws_rfqp, ws_rfI, ws_rfkeys, ws_rfD, ws_rfI2;
    float refine_ms[2] = {0.f, 0.f}; // rescore launches, final selections
    float last_ms = 0.f;
};

// A view whose parent's storage has moved on (grown, reset, freed): its xb / yn went back to the pool.  Every entry point
// that reads a handle's rows asks this first, before anything is copied or launched.
static bool view_is_stale(const knn_index_s *h) { return h->is_view && h->storage_gen->load() != h->view_gen; }
#define KNN_STALE_VIEW_MSG ": this view is stale (its parent index was grown, reset or freed after the view was made)"

// Workspace of a call on handle h: buffer b holds at least n elements of T, or the error is `what` (KNN_ERR_HIP) and the
// result null.  scratch(): a buffer that has to grow waits for the owner's work only -- h->done, then stream s
// (DevBuf::ensure).  scratch_device_wide(): the sites that know no owner's event, or never passed one, wait for the whole
// device.  Which of the two a site calls is which wait it gets.  Several buffers under one message are chained with ||, so
// that nothing more is asked for behind a failure.  n > 0 at every call: null is the only failure report, and 0 elements
// of a buffer that was never allocated would come back null with no message set.
template <typename T>
static T *scratch(knn_index_s *h, DevBuf &b, size_t n, hipStream_t s, const char *what = "search: out of device memory")
{
    if (!b.ensure(n * sizeof(T), h->done, s)) return (T *)b.p;
    set_err(KNN_ERR_HIP, what);
    return nullptr;
}
template <typename T>
static T *scratch_device_wide(DevBuf &b, size_t n, const char *what = "search: out of device memory")
{
    if (!b.ensure(n * sizeof(T))) return (T *)b.p;
    set_err(KNN_ERR_HIP, what);
    return nullptr;
}

static int ensure_device(int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return set_err(KNN_ERR_NO_DEVICE, "no HIP device available (libknn355 has no CPU fallback)");
    if (device < 0 || device >= n) return set_err(KNN_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    return 0;
}

extern "C" const char *knn_last_error(void) { return g_err.c_str(); }
extern "C" const char *knn_version(void) { return "knn355 0.1 (gfx950)"; }
extern "C" int knn_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}
extern "C" int knn_init(int device)
{
    int rc = ensure_device(device);
    if (rc) return rc;
    g_device = device;
    return 0;
}

static inline int round_up(int x, int m) { return (x + m - 1) / m * m; }

// ---- normalize ------------------------------------------------------------
static int normalize_dev_impl(float *x, int64_t n, int d, int64_t stride, hipStream_t s)
{
    if (n == 0) return 0;
    unsigned grid = (unsigned)((n + 63) / 64);
    if ((stride % 4) == 0 && (((uintptr_t)x) % 16) == 0)
        hipLaunchKernelGGL(normalize_rows_kernel<true>, dim3(grid), dim3(64), 0, s, x, n, d, stride);
    else
        hipLaunchKernelGGL(normalize_rows_kernel<false>, dim3(grid), dim3(64), 0, s, x, n, d, stride);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int norms_dev_impl(const float *x, int64_t n, int d, int64_t stride, float *out, hipStream_t s)
{
    if (n == 0) return 0;
    unsigned grid = (unsigned)((n + 63) / 64);
    if ((stride % 4) == 0 && (((uintptr_t)x) % 16) == 0)
        hipLaunchKernelGGL(norm_rows_kernel<true>, dim3(grid), dim3(64), 0, s, x, n, d, stride, out);
    else
        hipLaunchKernelGGL(norm_rows_kernel<false>, dim3(grid), dim3(64), 0, s, x, n, d, stride, out);
    HIP_TRY(hipGetLastError());
    return 0;
}
// dst[n][dp] <- src[n][d], zero padded, on stream s (both on the device)
static int pad_rows_dev(const float *src, int64_t n, int d, float *dst, int dp, hipStream_t s)
{
    const unsigned grid = (unsigned)std::min<int64_t>((n * dp + 255) / 256, 65535);
    hipLaunchKernelGGL(pad_rows_kernel, dim3(grid), dim3(256), 0, s, src, n, d, dst, dp);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int knn_normalize_l2_dev(float *x_dev, int64_t n, int32_t d, void *stream)
{
    if (n < 0 || d <= 0) return set_err(KNN_ERR_INVALID, "normalize_l2: bad shape");
    int rc = normalize_dev_impl(x_dev, n, d, d, (hipStream_t)stream);
    if (rc) return rc;
    if (!stream) HIP_TRY(hipStreamSynchronize(nullptr));
    return 0;
}

extern "C" int knn_normalize_l2(float *x_host, int64_t n, int32_t d)
{
    if (n < 0 || d <= 0) return set_err(KNN_ERR_INVALID, "normalize_l2: bad shape");
    if (n == 0) return 0;
    if (!x_host) return set_err(KNN_ERR_INVALID, "normalize_l2: null pointer");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    // Two pooled device buffers (no hipMalloc / hipFree per call: the reference's scripts normalise per embedding file)
    // and two streams taking turns in chunks of <= 64 MB: the download of chunk i overlaps the upload of chunk i + 1 (PCIe
    // is full duplex).  (A caller that adds the rows to an index anyway should add them raw and use knn_flat_normalize_rows
    // + knn_flat_reconstruct: one crossing each way -- pfam/proteins_search.py's flat mode does.)
    const int64_t rows_per = std::max<int64_t>(1, (int64_t)(64ull << 20) / ((int64_t)d * 4));
    const int64_t nbuf = std::min(n, rows_per);
    const int lanes = n > nbuf ? 2 : 1;
    // (the streams are declared behind the buffers: they go first, drained, whichever way the call returns)
    const size_t bytes = (size_t)nbuf * d * 4;
    PoolBuf buf0(bytes, g_device), buf1(lanes > 1 ? bytes : 0, g_device);
    StreamLease st0(g_device), st1(g_device, lanes > 1);
    if (!buf0 || !st0 || (lanes > 1 && (!buf1 || !st1))) return set_err(KNN_ERR_HIP, "normalize_l2: out of device memory");
    float *buf[2] = {buf0.get<float>(), buf1.get<float>()};
    const hipStream_t st[2] = {st0, st1};
    int turn = 0;
    for (int64_t i0 = 0; i0 < n; i0 += nbuf, turn ^= (lanes - 1)) {
        const int64_t m = std::min(nbuf, n - i0);
        hipError_t e = hipStreamSynchronize(st[turn]); // (this buffer's previous chunk is home)
        if (e == hipSuccess) e = hipMemcpyAsync(buf[turn], x_host + i0 * d, (size_t)m * d * 4, hipMemcpyHostToDevice, st[turn]);
        if (e == hipSuccess) {
            rc = normalize_dev_impl(buf[turn], m, d, d, st[turn]);
            if (rc) return rc;
            e = hipMemcpyAsync(x_host + i0 * d, buf[turn], (size_t)m * d * 4, hipMemcpyDeviceToHost, st[turn]);
        }
        if (e != hipSuccess) return set_err(KNN_ERR_HIP, std::string("normalize_l2 copy: ") + hipGetErrorString(e));
    }
    for (int i = 0; i < lanes; i++) {
        hipError_t e = hipStreamSynchronize(st[i]);
        if (e != hipSuccess) return set_err(KNN_ERR_HIP, std::string("normalize_l2: ") + hipGetErrorString(e));
    }
    return 0;
}

// ---- the owners of the batched host searches (DESIGN 4.10, 4.5): the device's copy pipes, the scaffold of a host entry, the
// piped result download.  hnsw_search.inc, lsh.inc, pca.inc, kde.inc, pool.inc and overlap.inc use them as host_search does
// Copy streams of the pipelined host search: one set per device for the whole process, created on
// first use (a HIP stream costs milliseconds to create and callers such as cath/search.py build a
// fresh index per file).  Whoever holds `mu` pipelines; a concurrent host search on the same
// device simply runs its batches one after the other on its own stream.
struct CopyPipes {
    std::mutex mu;
    hipStream_t h2d = nullptr, d2h = nullptr;
    // per result slot, for the holder of `mu` alone: the slot's queries are up, its batch is done on the search stream,
    // its results have left the buffers
    hipEvent_t ev_query[2] = {nullptr, nullptr}, ev_batch[2] = {nullptr, nullptr}, ev_left[2] = {nullptr, nullptr};
};
static CopyPipes g_pipes[64];

// A caller's hold on its device's copy pipes: cp is null when the caller did not want them (`want`: its own rule, one batch
// has nothing to overlap with) or another host search holds them; otherwise they are this caller's until the lease goes.
// The streams and events are made on first use (the caller has set the device).
struct PipeLease {
    std::unique_lock<std::mutex> lock;
    CopyPipes *cp = nullptr;
};
static int lease_pipes(int device, bool want, PipeLease &lease)
{
    CopyPipes &cp = g_pipes[device & 63];
    lease.lock = std::unique_lock<std::mutex>(cp.mu, std::defer_lock);
    if (!want || !lease.lock.try_lock()) return 0;
    if (!cp.h2d) HIP_TRY(hipStreamCreateWithFlags(&cp.h2d, hipStreamNonBlocking));
    if (!cp.d2h) HIP_TRY(hipStreamCreateWithFlags(&cp.d2h, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        if (!cp.ev_query[i]) HIP_TRY(hipEventCreateWithFlags(&cp.ev_query[i], hipEventDisableTiming));
        if (!cp.ev_batch[i]) HIP_TRY(hipEventCreateWithFlags(&cp.ev_batch[i], hipEventDisableTiming));
        if (!cp.ev_left[i]) HIP_TRY(hipEventCreateWithFlags(&cp.ev_left[i], hipEventDisableTiming));
    }
    lease.cp = &cp;
    return 0;
}

// The scaffold of a host entry that keeps nothing behind: enqueue on `s` (uploads may ride pipes.cp->h2d), then finish().
// ORDER: streams are drained before any buffer goes back to the pool or to hipFree -- the pool may hand a buffer to
// another handle at once -- and a stream of g_streams goes back behind the buffers.  finish() drains; the members then go
// in reverse: events, buffers, the stream, the pipes.  (An entry without a HostCall declares its StreamLease behind its
// PoolBufs: the lease's destructor drains, and it runs first.)
struct HostCall {
    PipeLease pipes;
    StreamLease own;
    EvalBufs bufs;
    PhaseClock clock;
    hipStream_t s; // where the call's kernels run: its own stream, else the leased h2d stream, else the caller's / the null stream
    // on a stream the caller names (null: the null stream)
    explicit HostCall(hipStream_t caller = nullptr) : own(0, false), s(caller) {}
    // on a stream of g_streams (s is null when there is none)
    explicit HostCall(int device) : own(device), s(own) {}
    // the device's copy pipes, if wanted and free; a call without a stream of its own then runs on their h2d stream
    int lease(int device, bool want)
    {
        EVAL_TRY(lease_pipes(device, want, pipes));
        if (pipes.cp && !own) s = pipes.cp->h2d;
        return 0;
    }
    // Behind the enqueueing, whatever it returned (rc): waits for the h2d stream and for s -- always, copies already queued
    // read and write the caller's arrays -- then reports rc, else the first HIP error as "who: ...".  The clock is ready to
    // be read behind a 0.
    int finish(const char *who, int rc)
    {
        hipError_t e = pipes.cp && pipes.cp->h2d != s ? hipStreamSynchronize(pipes.cp->h2d) : hipSuccess;
        const hipError_t es = hipStreamSynchronize(s);
        if (rc) return rc;
        if (e == hipSuccess) e = es;
        if (e != hipSuccess) return set_err(KNN_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
        return 0;
    }
};

// The result download of a batched search whose batches follow one another on the search stream `s` (hnsw_search_device,
// lsh_search_batches).  Piped (cp given): two sets of result buffers, and while batch b runs on `s` the results of batch
// b - 1 go down on the copy stream, ordered by events alone -- this thread never waits inside the loop.  Not piped: one
// set, every batch downloaded on `s` and waited for.  The caller's loop is
//     for every batch b, while rc == 0: before(b); enqueue the batch into the buffers of slot(b); after(b, copy)
//     return finish(rc, nbatches, copy)
// with copy(b, slot, stream) -> hipError_t enqueueing the device-to-host copies of batch b.  Every HIP error is reported
// under `who` ("lsh_search: ").
struct ResultPipe {
    CopyPipes *cp;
    hipStream_t s;
    const char *who;
    int slot(int64_t b) const { return cp ? (int)(b & 1) : 0; }
    int hip(hipError_t e) const { return e == hipSuccess ? 0 : set_err(KNN_ERR_HIP, std::string(who) + hipGetErrorString(e)); }
    // the results of batch b - 2 have left the buffers batch b is about to write
    int before(int64_t b) const { return cp && b >= 2 ? hip(hipStreamWaitEvent(s, cp->ev_left[b & 1], 0)) : 0; }
    // batch b is enqueued: the copy of batch b - 1 may block this thread as long as it likes
    template <typename Copy>
    int after(int64_t b, Copy &&copy) const
    {
        if (!cp) {
            int rc = hip(copy(b, 0, s));
            return rc ? rc : hip(hipStreamSynchronize(s));
        }
        int rc = hip(hipEventRecord(cp->ev_batch[b & 1], s));
        if (rc || b == 0) return rc;
        rc = download(b - 1, copy);
        return rc ? rc : hip(hipEventRecord(cp->ev_left[(b - 1) & 1], cp->d2h));
    }
    // rc: how the loop ended.  If well, the last batch goes down; then, whichever way it ended, BOTH streams are waited
    // for: a download already queued writes into the caller's host arrays, and the lease is released on return.
    template <typename Copy>
    int finish(int rc, int64_t nbatches, Copy &&copy) const
    {
        if (!cp) return rc;
        if (!rc) rc = download(nbatches - 1, copy);
        const hipError_t e1 = hipStreamSynchronize(cp->d2h), e2 = hipStreamSynchronize(s);
        return rc ? rc : hip(e1 != hipSuccess ? e1 : e2);
    }
    template <typename Copy>
    int download(int64_t b, Copy &&copy) const
    {
        int rc = hip(hipStreamWaitEvent(cp->d2h, cp->ev_batch[b & 1], 0));
        return rc ? rc : hip(copy(b, (int)(b & 1), cp->d2h));
    }
};
