// comm.inc -- sharded search across processes (included by knn355_lib.hip behind flat_info.inc).
// ---------------------------------------------------------------------------
// Several GPUs without torch: RCCL inside the library.  One process per GPU; rank 0 makes a
// unique id (knn_comm_unique_id), the caller hands it to the other ranks by whatever means it
// has (a file, MPI, a socket), every rank creates its communicator, and a sharded search is
// local scan -> ncclAllGather of the [nq][k] packed keys -> selection, all on one stream.
// librccl is opened on first use (dlopen): a process that shards through torch.distributed
// instead (bench.py, sharded.py) never loads a second copy.
// ---------------------------------------------------------------------------
#include <dlfcn.h>
struct Id128 { char b[128]; };
struct RcclApi {
    void *lib = nullptr;
    int (*GetUniqueId)(void *) = nullptr;
    int (*CommInitRank)(void **, int, /* ncclUniqueId by value: 128 bytes */ Id128, int) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
};
static RcclApi g_rccl;
static std::mutex g_rccl_mu;
static int rccl_load()
{
    std::lock_guard<std::mutex> lk(g_rccl_mu);
    if (g_rccl.lib) return 0;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *L = nullptr;
    for (const char *nm : names)
        if ((L = dlopen(nm, RTLD_NOW | RTLD_GLOBAL))) break;
    if (!L) return set_err(KNN_ERR_UNSUPPORTED, std::string("comm: librccl not found (") + dlerror() + ")");
    RcclApi a;
    a.GetUniqueId = (int (*)(void *))dlsym(L, "ncclGetUniqueId");
    a.CommInitRank = (int (*)(void **, int, Id128, int))dlsym(L, "ncclCommInitRank");
    a.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))dlsym(L, "ncclAllGather");
    a.CommDestroy = (int (*)(void *))dlsym(L, "ncclCommDestroy");
    a.GetErrorString = (const char *(*)(int))dlsym(L, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString)
        return set_err(KNN_ERR_UNSUPPORTED, "comm: librccl lacks a required symbol");
    a.lib = L;
    g_rccl = a;
    return 0;
}
#define RCCL_TRY(expr)                                                                                        \
    do {                                                                                                      \
        int r_ = (expr);                                                                                      \
        if (r_ != 0) return set_err(KNN_ERR_HIP, std::string(#expr) + ": " + g_rccl.GetErrorString(r_));      \
    } while (0)

// how long a rank waits for its peers (communicator creation, a synchronous sharded search): KNN355_COMM_TIMEOUT_S, default 120 s
static double comm_timeout_s()
{
    const char *e = getenv("KNN355_COMM_TIMEOUT_S");
    const double v = e ? atof(e) : 120.0;
    return v > 0 ? v : 120.0;
}

struct knn_comm_s {
    void *comm = nullptr;
    int world = 1, rank = 0, device = 0;
    DevBuf keys, gathered;    // this rank's keys / everybody's: one search at a time uses them (see `done`)
    hipEvent_t done = nullptr; // recorded behind the last search's selection: a call on ANOTHER stream waits for it
    std::mutex mu;
};

extern "C" int knn_comm_unique_id(uint8_t *id128)
{
    if (!id128) return set_err(KNN_ERR_INVALID, "comm_unique_id: null pointer");
    int rc = rccl_load();
    if (rc) return rc;
    RCCL_TRY(g_rccl.GetUniqueId(id128));
    return 0;
}

extern "C" int knn_comm_create(const uint8_t *id128, int32_t world, int32_t rank, int32_t device, knn_comm_s **out)
{
    if (!id128 || !out) return set_err(KNN_ERR_INVALID, "comm_create: null pointer");
    if (world < 1 || rank < 0 || rank >= world) return set_err(KNN_ERR_INVALID, "comm_create: bad world / rank");
    int rc = rccl_load();
    if (rc) return rc;
    rc = ensure_device(device);
    if (rc) return rc;
    knn_comm_s *c = new knn_comm_s();
    c->world = world;
    c->rank = rank;
    c->device = device;
    Id128 id;
    memcpy(id.b, id128, 128);
    // ncclCommInitRank returns when EVERY rank has called it -- with a peer that never arrives, never.  It runs on a helper
    // thread and this call waits for it at most KNN355_COMM_TIMEOUT_S seconds (120): the first contact with a multi-GPU node
    // fails with the rank named, not as a hang.  (A helper that is still inside RCCL when the wait runs out is left to itself:
    // it owns its state and destroys the communicator should the call ever return.)
    struct InitState {
        std::mutex mu;
        std::condition_variable cv;
        bool finished = false, abandoned = false;
        int r = 0;
        void *comm = nullptr;
    };
    auto st = std::make_shared<InitState>();
    std::thread([st, id, world, rank, device]() {
        int r = hipSetDevice(device) == hipSuccess ? 0 : -1; // (the communicator belongs to the calling thread's current device)
        void *comm = nullptr;
        if (r == 0) r = g_rccl.CommInitRank(&comm, world, id, rank);
        std::unique_lock<std::mutex> lk(st->mu);
        st->r = r;
        st->comm = comm;
        st->finished = true;
        if (st->abandoned && r == 0 && comm) (void)g_rccl.CommDestroy(comm);
        st->cv.notify_all();
    }).detach();
    const double wait_s = comm_timeout_s();
    {
        std::unique_lock<std::mutex> lk(st->mu);
        if (!st->cv.wait_for(lk, std::chrono::duration<double>(wait_s), [&] { return st->finished; })) {
            st->abandoned = true;
            delete c;
            char msg[256];
            snprintf(msg, sizeof msg, "comm_create: rank %d of %d: ncclCommInitRank did not return within %.0f s (KNN355_COMM_TIMEOUT_S) -- "
                                      "a peer never arrived, or the ranks do not share the unique id", rank, world, wait_s);
            return set_err(KNN_ERR_TIMEOUT, msg);
        }
    }
    if (st->r != 0) {
        delete c;
        return set_err(KNN_ERR_HIP, st->r == -1 ? std::string("comm_create: hipSetDevice failed on the helper thread")
                                               : std::string("ncclCommInitRank: ") + g_rccl.GetErrorString(st->r));
    }
    c->comm = st->comm;
    *out = c;
    return 0;
}

extern "C" void knn_comm_free(knn_comm_s *c)
{
    if (!c) return;
    if (hipSetDevice(c->device) == hipSuccess) {
        if (c->comm && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(c->comm);
        (void)hipDeviceSynchronize();
        c->keys.release();
        c->gathered.release();
        if (c->done) (void)hipEventDestroy(c->done);
    }
    delete c;
}

// h holds THIS rank's rows (global id of local row r = id_base + r); q_dev [nq][d] is the same on every rank;
// D_dev / I_dev receive the global result on every rank.  Every rank must call with the same nq and k.
extern "C" int knn_sharded_search_dev(knn_handle h, knn_comm_s *c, const float *q_dev, int64_t nq, int64_t k, uint32_t id_base,
                                      float *D_dev, int64_t *I_dev, void *stream)
{
    if (!c) return set_err(KNN_ERR_INVALID, "sharded_search: null communicator");
    int rc = check_search_args(h, q_dev, nq, k, D_dev, I_dev);
    if (rc) return rc;
    if (h->approx16) return set_err(KNN_ERR_UNSUPPORTED, "sharded_search: not for an approximate (bf16) index"); // (before the collective, like every argument error)
    if (nq == 0) return 0;
    if (h->device != c->device) return set_err(KNN_ERR_INVALID, "sharded_search: index and communicator live on different devices");
    std::lock_guard<std::mutex> lc(c->mu);
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    const size_t nkeys = (size_t)nq * k;
    // The key and gather buffers belong to the communicator: a search on another stream than the previous one must not
    // overwrite them while that one's all-gather or selection is still running (ADVICE r2) -- it waits for the previous
    // search's `done` event (on the GPU; the host does not block).  RCCL wants the collectives of one communicator
    // issued in one order anyway.
    if (!c->done) HIP_TRY(hipEventCreateWithFlags(&c->done, hipEventDisableTiming));
    HIP_TRY(hipStreamWaitEvent(s, c->done, 0));
    const char *oom = "sharded_search: out of device memory (before the collective: the other ranks will wait for this one -- "
                      "treat a failure on any rank as fatal for the communicator)";
    if (!scratch_device_wide<uint64_t>(c->keys, nkeys, oom) || !scratch_device_wide<uint64_t>(c->gathered, nkeys * c->world, oom)) return KNN_ERR_HIP;
    h->last_ms = -1.f;
    rc = search_dev_impl(h, q_dev, nq, (int)k, nullptr, nullptr, (uint64_t *)c->keys.p, id_base, false, s);
    std::string local_err;
    if (rc) {
        // A rank that fails locally still enters the collective -- with "no rows" for keys -- so that its peers do not
        // hang in ncclAllGather; it returns its error afterwards.  The peers' result then lacks this shard and they
        // cannot know: callers must treat a failure on ANY rank as a failure of the search (exchange the return codes).
        local_err = g_err;
        hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((nkeys + 255) / 256)), dim3(256), 0, s, (int64_t)nkeys, h->metric,
                           (uint64_t *)c->keys.p, (float *)nullptr, (int64_t *)nullptr);
    }
    RCCL_TRY(g_rccl.AllGather(c->keys.p, c->gathered.p, nkeys, /* ncclUint64 */ 5, c->comm, s));
    if (rc) {
        (void)hipEventRecord(c->done, s);
        return set_err(rc, local_err);
    }
    SelectParams sp = {};
    sp.in = (const uint64_t *)c->gathered.p; sp.lm_lists = c->world; sp.lm_k = (int)k;
    sp.nq = nq; sp.k = (int)k; sp.metric = h->metric;
    sp.D = D_dev; sp.I = I_dev;
    rc = launch_select(sp, s);
    (void)hipEventRecord(c->done, s);
    if (rc) return rc;
    if (!stream) {
        if (c->world == 1) {
            HIP_TRY(hipStreamSynchronize(s));
        } else {
            // bounded: a peer that never enters the all-gather would hold hipStreamSynchronize for ever
            const double wait_s = comm_timeout_s();
            const auto t0 = std::chrono::steady_clock::now();
            int spins = 0;
            for (;;) {
                const hipError_t q = hipStreamQuery(s);
                if (q == hipSuccess) break;
                if (q != hipErrorNotReady) return set_err(KNN_ERR_HIP, std::string("sharded_search: ") + hipGetErrorString(q));
                if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > wait_s) {
                    char msg[256];
                    snprintf(msg, sizeof msg, "sharded_search: rank %d of %d: the search (local scan, ncclAllGather, selection) did not complete within "
                                              "%.0f s (KNN355_COMM_TIMEOUT_S) -- a peer never entered the all-gather; the communicator is unusable", c->rank, c->world, wait_s);
                    return set_err(KNN_ERR_TIMEOUT, msg);
                }
                if (++spins < 2000) std::this_thread::yield(); // (a healthy step takes a millisecond: stay close for the first ones)
                else std::this_thread::sleep_for(std::chrono::microseconds(200));
            }
        }
    }
    return 0;
}

