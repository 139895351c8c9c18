// eval.inc -- consumers of the (hits, scores) arrays, SURVEY.md section 8(f) N4 (included by knn355_lib.hip).
//
// The reference post-processes search results with per-row Python loops
// (pfam/proteins.py:85-122 remove_self_hit; seqvec_search/main.py:64-82 evaluate;
// pfam/proteins_shared.py:139-157 compute_auc1; cath/cath.py:76-84 compute_is_correct;
// seqvec_search/tp_cumulative.py:15-34).  At 200k queries x 1000 hits these loops dominate the
// wall time after the search.  Here each is one pass of integer work over hits[nq][k]: one wave
// per row, coalesced reads of the row, gathers into small label tables.
#include <errno.h>
#include <stdlib.h>

// ---- device helpers shared by the consumers (and by range.inc's epilogue) ---------------------
// number of set bits of the ballot m below this lane
__device__ __forceinline__ uint32_t ballot_rank(uint64_t m)
{
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// workgroup of 256: exclusive position of this thread among the threads with `flag`, and their number in *total.
// s_wcnt is an LDS array [2][4] and par the set to write (0 at first): a call writes one set and flips par, so one
// barrier per call is enough
__device__ __forceinline__ int wg_compact(bool flag, int (*s_wcnt)[4], int &par, int *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t m = __ballot(flag);
    if (lane == 0) s_wcnt[par][wave] = __builtin_popcountll(m);
    __syncthreads();
    int pos = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int c = s_wcnt[par][w];
        pos += w < wave ? c : 0;
        tot += c;
    }
    par ^= 1;
    *total = tot;
    return pos + (int)ballot_rank(m);
}

// workgroup of 256 over the LDS values s_val[0 .. n) in rank order: rank i survives when its value is not `none` and no
// earlier rank holds it (a quadratic scan, every lane reading the same word: a broadcast); survivor number `at` gets
// emit(at, i, value) while at < k_out, and the walk stops once k_out are out.  Returns min(survivors seen, k_out)
template <typename T, typename Emit>
__device__ __forceinline__ int wg_dedup_compact(const T *s_val, int n, int k_out, T none, int (*s_wcnt)[4], int &par, Emit emit)
{
    const int tid = threadIdx.x;
    int emitted = 0;
    for (int c0 = 0; c0 < n && emitted < k_out; c0 += 256) {
        const int i = c0 + tid;
        const T v = i < n ? s_val[i] : none;
        bool keep = v != none;
        for (int j = 0; keep && j < i; j++) keep = s_val[j] != v;
        int tot;
        const int at = emitted + wg_compact(keep, s_wcnt, par, &tot);
        if (keep && at < k_out) emit(at, i, v);
        emitted += tot;
    }
    return min(emitted, k_out);
}

// first i in [lo, hi) for which less(i) is false (less: "element i is below the key", true on a prefix); hi when none
template <typename I, typename Less>
__device__ __forceinline__ I lower_bound_dev(I lo, I hi, Less less)
{
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if (less(mid)) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// one wave per row, four rows per block of 256 threads: this thread's lane and its wave's row; false (for the whole
// wave) past the last row
__device__ __forceinline__ bool wave_row(int64_t nq, int &lane, int64_t &r)
{
    lane = threadIdx.x & 63;
    r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    return r < nq;
}

// the row's lead (lowest first_bad of the lanes) and tp (sum of their cnt), stored by lane 0
__device__ __forceinline__ void wave_store_lead_tp(int lane, int first_bad, int cnt, int32_t *lead, int32_t *tp)
{
    for (int off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        first_bad = min(first_bad, __shfl_xor(first_bad, off, 64));
    }
    if (lane == 0) {
        *lead = first_bad;
        *tp = cnt;
    }
}

// out row = in row with the element at `index` removed; index = position of the self id
// (0 when the search put it first), or k-1 when the row does not contain it (counted missing)
__global__ void remove_self_hit_kernel(const int64_t *__restrict__ hits, const float *__restrict__ scores, int64_t nq, int k,
                                       const int64_t *__restrict__ self_ids, int64_t *__restrict__ hits_out,
                                       float *__restrict__ scores_out, int32_t *__restrict__ missing)
{
    int lane;
    int64_t r;
    if (!wave_row(nq, lane, r)) return;
    const int64_t *h = hits + r * k;
    const float *s = scores + r * k;
    const int64_t self = self_ids[r];
    int first = k; // first position holding the self id
    for (int j = lane; j < k; j += 64)
        if (h[j] == self) { first = j; break; }
    for (int off = 32; off >= 1; off >>= 1) first = min(first, __shfl_xor(first, off, 64));
    const bool found = first < k;
    const int index = found ? first : k - 1;
    for (int j = lane; j < k - 1; j += 64) {
        const int src = j < index ? j : j + 1;
        hits_out[r * (k - 1) + j] = h[src];
        scores_out[r * (k - 1) + j] = s[src];
    }
    if (lane == 0) missing[r] = found ? 0 : 1;
}

// single-label evaluation (seqvec_search/main.py:64-82): lead = number of leading hits whose
// label equals the query's, tp = number of such hits anywhere; hit -1 never matches
__global__ void label_eval_kernel(const int64_t *__restrict__ hits, int64_t nq, int k, const int32_t *__restrict__ labels_q,
                                  const int32_t *__restrict__ labels_db, int64_t nb, uint8_t *__restrict__ is_correct,
                                  int32_t *__restrict__ lead, int32_t *__restrict__ tp)
{
    int lane;
    int64_t r;
    if (!wave_row(nq, lane, r)) return;
    const int32_t lq = labels_q[r];
    int cnt = 0, first_bad = k;
    for (int j = lane; j < k; j += 64) {
        const int64_t hid = hits[r * k + j];
        const bool ok = hid >= 0 && hid < nb && labels_db[hid] == lq;
        if (is_correct) is_correct[r * k + j] = ok ? 1 : 0;
        cnt += ok ? 1 : 0;
        if (!ok) first_bad = min(first_bad, j);
    }
    wave_store_lead_tp(lane, first_bad, cnt, lead + r, tp + r);
}

// set-membership evaluation (pfam/proteins_shared.py:139-157): query r is homologous to the
// sorted target rows members[offsets[r] .. offsets[r+1]).  MATRIX: the per-hit membership bytes
// (pfam/proteins.py:201-207 compute_correctness_array) instead of the leading run and the count
template <bool MATRIX>
__global__ void set_eval_kernel(const int64_t *__restrict__ hits, int64_t nq, int k, const int64_t *__restrict__ offsets,
                                const int64_t *__restrict__ members, int32_t *__restrict__ lead, int32_t *__restrict__ tp,
                                uint8_t *__restrict__ is_correct)
{
    int lane;
    int64_t r;
    if (!wave_row(nq, lane, r)) return;
    const int64_t lo0 = offsets[r], hi0 = offsets[r + 1];
    int cnt = 0, first_bad = k;
    for (int j = lane; j < k; j += 64) {
        const int64_t hid = hits[r * k + j];
        const int64_t lo = lower_bound_dev(lo0, hi0, [&](int64_t i) { return members[i] < hid; });
        const bool ok = lo < hi0 && members[lo] == hid;
        if (MATRIX) {
            is_correct[r * k + j] = ok ? 1 : 0;
            continue;
        }
        cnt += ok ? 1 : 0;
        if (!ok) first_bad = min(first_bad, j);
    }
    if (MATRIX) return;
    wave_store_lead_tp(lane, first_bad, cnt, lead + r, tp + r);
}

// cath/cath.py:76-84: out[q][l][j] = mapping[query_rows[q]][l] == mapping[hits[q][j]][l]
__global__ void levels_eval_kernel(const int64_t *__restrict__ hits, int64_t nq, int k, const int64_t *__restrict__ query_rows,
                                   const int32_t *__restrict__ mapping, int64_t n, int nlevels, uint8_t *__restrict__ out)
{
    int lane;
    int64_t r;
    if (!wave_row(nq, lane, r)) return;
    const int64_t qrow = query_rows[r];
    for (int j = lane; j < k; j += 64) {
        const int64_t hid = hits[r * k + j];
        for (int l = 0; l < nlevels; l++) {
            const bool ok = hid >= 0 && hid < n && mapping[hid * nlevels + l] == mapping[qrow * nlevels + l];
            out[(r * nlevels + l) * k + j] = ok ? 1 : 0;
        }
    }
}

// ---- host wrappers: host buffers in and out, rows processed in slabs -------------------------
// (EvalBufs, EVAL_ALLOC, EVAL_TRY: host_core.inc)
// The slab walker: the columns that travel between the host and the device.  A column is declared once -- host pointer,
// bytes per row, input or output -- which allocates `cap` rows of it through EvalBufs and registers its copy; upload and
// download then move the rows [r0, r0 + m) of every input and of every output column (synchronous copies on the null
// stream, in the order of the declarations).  A null host pointer, an optional column that the caller left out, gives
// a null device pointer: no allocation and no copy.  A whole-call table or accumulator is a column of a walker of one
// row (cap 1, the row being the table): upload(0, 1) once in front of the slabs, download(0, 1) once behind them.
// ready() after the declarations reports a failed allocation.
struct EvalCols {
    struct Col {
        const char *src; // host source of an input, or null
        char *dst;       // host target of an output, or null
        char *dev;
        size_t row;
    };
    EvalBufs &bufs;
    const int64_t cap;
    std::vector<Col> cols;
    EvalCols(EvalBufs &b, int64_t cap_rows) : bufs(b), cap(cap_rows) {}
    void *add(const void *src, void *dst, size_t row)
    {
        if (!src && !dst) return nullptr;
        char *d = (char *)bufs.get((size_t)cap * row);
        cols.push_back({(const char *)src, (char *)dst, d, row});
        return d;
    }
    template <typename T> T *in(const T *host, size_t row_bytes) { return (T *)add(host, nullptr, row_bytes); }
    template <typename T> T *out(T *host, size_t row_bytes) { return (T *)add(nullptr, host, row_bytes); }
    int ready() const { return bufs.oom ? set_err(KNN_ERR_HIP, "eval: out of device memory") : 0; }
    int upload(int64_t r0, int64_t m) const
    {
        for (const Col &c : cols)
            if (c.src && m * c.row) HIP_TRY(hipMemcpy(c.dev, c.src + (size_t)r0 * c.row, (size_t)m * c.row, hipMemcpyHostToDevice));
        return 0;
    }
    int download(int64_t r0, int64_t m) const
    {
        for (const Col &c : cols)
            if (c.dst && m * c.row) HIP_TRY(hipMemcpy(c.dst + (size_t)r0 * c.row, c.dev, (size_t)m * c.row, hipMemcpyDeviceToHost));
        return 0;
    }
};

// offs[0 .. n] start at or above 0 and never decrease; limit >= 0: and end at or below limit (rows)
static int eval_check_offsets(const std::string &who, const char *noun, const int64_t *offs, int64_t n, int64_t limit = -1)
{
    if (offs[0] < 0) return set_err(KNN_ERR_INVALID, who + ": negative " + noun + " offset");
    for (int64_t i = 0; i < n; i++)
        if (offs[i + 1] < offs[i]) return set_err(KNN_ERR_INVALID, who + ": " + noun + " offsets decrease");
    if (limit >= 0 && offs[n] > limit) return set_err(KNN_ERR_INVALID, who + ": " + noun + " offsets past the last row");
    return 0;
}

// rows per slab: 256 MiB of hits.  KNN355_EVAL_SLAB_ROWS (read on every call; a positive decimal integer, anything else
// is ignored) replaces the count, so that a test crosses slab boundaries with a handful of rows
static int64_t eval_slab_rows(int64_t k)
{
    const char *e = getenv("KNN355_EVAL_SLAB_ROWS");
    if (e && *e >= '0' && *e <= '9') {
        char *end = nullptr;
        errno = 0;
        const long long v = strtoll(e, &end, 10);
        if (errno == 0 && *end == '\0' && v > 0) return (int64_t)v;
    }
    return std::max<int64_t>(1, (int64_t)(256ull << 20) / (k * 8));
}
// the kernels take k as int
static bool eval_k_too_large(int64_t k) { return k > (int64_t)INT32_MAX; }

extern "C" int knn_eval_remove_self_hit(const int64_t *hits, const float *scores, int64_t nq, int64_t k, const int64_t *self_ids,
                                        int64_t *hits_out, float *scores_out, int32_t *missing_out)
{
    if (nq < 0 || k < 2) return set_err(KNN_ERR_INVALID, "remove_self_hit: need k >= 2");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "remove_self_hit: k > INT32_MAX");
    if (nq == 0) return 0;
    if (!hits || !scores || !self_ids || !hits_out || !scores_out || !missing_out) return set_err(KNN_ERR_INVALID, "remove_self_hit: null pointer");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    EvalBufs bufs;
    const int64_t slab = std::min(nq, eval_slab_rows(k));
    EvalCols w(bufs, slab);
    const int64_t *d_h = w.in(hits, (size_t)k * 8);
    const float *d_s = w.in(scores, (size_t)k * 4);
    const int64_t *d_self = w.in(self_ids, 8);
    int64_t *d_ho = w.out(hits_out, (size_t)(k - 1) * 8);
    float *d_so = w.out(scores_out, (size_t)(k - 1) * 4);
    int32_t *d_m = w.out(missing_out, 4);
    EVAL_TRY(w.ready());
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(w.upload(r0, m));
        hipLaunchKernelGGL(remove_self_hit_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, d_s, m, (int)k, d_self, d_ho, d_so, d_m);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(w.download(r0, m));
    }
    return 0;
}

extern "C" int knn_eval_labels(const int64_t *hits, int64_t nq, int64_t k, const int32_t *labels_q, const int32_t *labels_db,
                               int64_t nb, uint8_t *is_correct_out, int32_t *lead_out, int32_t *tp_out)
{
    if (nq < 0 || k < 1 || nb < 0) return set_err(KNN_ERR_INVALID, "eval_labels: bad shape");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "eval_labels: k > INT32_MAX");
    if (nq == 0) return 0;
    if (!hits || !labels_q || (!labels_db && nb > 0) || !lead_out || !tp_out) return set_err(KNN_ERR_INVALID, "eval_labels: null pointer");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    EvalBufs bufs;
    const int64_t slab = std::min(nq, eval_slab_rows(k));
    EvalCols tab(bufs, 1), w(bufs, slab);
    const int32_t *d_ldb = tab.in(labels_db, (size_t)nb * 4);
    const int64_t *d_h = w.in(hits, (size_t)k * 8);
    const int32_t *d_lq = w.in(labels_q, 4);
    uint8_t *d_ic = w.out(is_correct_out, (size_t)k);
    int32_t *d_lead = w.out(lead_out, 4);
    int32_t *d_tp = w.out(tp_out, 4);
    EVAL_TRY(w.ready());
    EVAL_TRY(tab.upload(0, 1));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(w.upload(r0, m));
        hipLaunchKernelGGL(label_eval_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, m, (int)k, d_lq, d_ldb, nb, d_ic, d_lead, d_tp);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(w.download(r0, m));
    }
    return 0;
}

// knn_eval_sets (lead_out, tp_out) and knn_eval_sets_matrix (is_correct_out): one set of checks, one slab walk
static int eval_sets_run(const int64_t *hits, int64_t nq, int64_t k, const int64_t *set_offsets, const int64_t *set_members,
                         int32_t *lead_out, int32_t *tp_out, uint8_t *is_correct_out, bool matrix)
{
    if (nq < 0 || k < 1) return set_err(KNN_ERR_INVALID, "eval_sets: bad shape");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "eval_sets: k > INT32_MAX");
    if (nq == 0) return 0;
    if (!hits || !set_offsets || (matrix ? !is_correct_out : (!lead_out || !tp_out))) return set_err(KNN_ERR_INVALID, "eval_sets: null pointer");
    // the kernel binary-searches set_members[set_offsets[r] .. set_offsets[r+1]) without further checks
    EVAL_TRY(eval_check_offsets("eval_sets", "set", set_offsets, nq));
    const int64_t nmem = set_offsets[nq];
    if (nmem > 0 && !set_members) return set_err(KNN_ERR_INVALID, "eval_sets: null pointer");
    for (int64_t r = 0; r < nq; r++)
        for (int64_t i = set_offsets[r] + 1; i < set_offsets[r + 1]; i++)
            if (set_members[i] < set_members[i - 1]) return set_err(KNN_ERR_INVALID, "eval_sets: set members not sorted");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    EvalBufs bufs;
    const int64_t slab = std::min(nq, eval_slab_rows(k));
    EvalCols tab(bufs, 1), w(bufs, slab);
    const int64_t *d_off = tab.in(set_offsets, (size_t)(nq + 1) * 8);
    const int64_t *d_mem = tab.in(set_members, (size_t)nmem * 8);
    const int64_t *d_h = w.in(hits, (size_t)k * 8);
    int32_t *d_lead = w.out(lead_out, 4); // (the matrix build has is_correct_out alone, the other build lead_out and tp_out)
    int32_t *d_tp = w.out(tp_out, 4);
    uint8_t *d_ic = w.out(is_correct_out, (size_t)k);
    EVAL_TRY(w.ready());
    EVAL_TRY(tab.upload(0, 1));
    const auto kern = matrix ? set_eval_kernel<true> : set_eval_kernel<false>;
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(w.upload(r0, m));
        hipLaunchKernelGGL(kern, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, m, (int)k, d_off + r0, d_mem, d_lead, d_tp, d_ic);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(w.download(r0, m));
    }
    return 0;
}

extern "C" int knn_eval_sets(const int64_t *hits, int64_t nq, int64_t k, const int64_t *set_offsets, const int64_t *set_members,
                             int32_t *lead_out, int32_t *tp_out)
{
    return eval_sets_run(hits, nq, k, set_offsets, set_members, lead_out, tp_out, nullptr, false);
}

extern "C" int knn_eval_sets_matrix(const int64_t *hits, int64_t nq, int64_t k, const int64_t *set_offsets,
                                    const int64_t *set_members, uint8_t *is_correct_out)
{
    return eval_sets_run(hits, nq, k, set_offsets, set_members, nullptr, nullptr, is_correct_out, true);
}

extern "C" int knn_eval_levels(const int64_t *hits, int64_t nq, int64_t k, const int64_t *query_rows, const int32_t *mapping,
                               int64_t n, int32_t nlevels, uint8_t *out)
{
    if (nq < 0 || k < 1 || n < 1 || nlevels < 1) return set_err(KNN_ERR_INVALID, "eval_levels: bad shape");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "eval_levels: k > INT32_MAX");
    if (nq == 0) return 0;
    if (!hits || !query_rows || !mapping || !out) return set_err(KNN_ERR_INVALID, "eval_levels: null pointer");
    for (int64_t i = 0; i < nq; i++)
        if (query_rows[i] < 0 || query_rows[i] >= n) return set_err(KNN_ERR_INVALID, "eval_levels: query row out of range");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    EvalBufs bufs;
    const int64_t slab = std::min(nq, eval_slab_rows(k));
    EvalCols tab(bufs, 1), w(bufs, slab);
    const int32_t *d_map = tab.in(mapping, (size_t)n * nlevels * 4);
    const int64_t *d_h = w.in(hits, (size_t)k * 8);
    const int64_t *d_q = w.in(query_rows, 8);
    uint8_t *d_out = w.out(out, (size_t)nlevels * k);
    EVAL_TRY(w.ready());
    EVAL_TRY(tab.upload(0, 1));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(w.upload(r0, m));
        hipLaunchKernelGGL(levels_eval_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, m, (int)k, d_q, d_map, n, (int)nlevels, d_out);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(w.download(r0, m));
    }
    return 0;
}

// ---- MMseqs2 prefilter database writer: SURVEY section 8(f) N3 -------------------------------
// seqvec_search/mmseqs/_write_prefilter_db.py:52-97: per query one record
//   "<target mmseqs id>\t<int(score*100)>\t0\n" per hit (hit == -1 skipped), then a NUL byte;
// index file lines "<query mmseqs id>\t<offset>\t<length>\n".  Pure host work (text
// formatting + file output); rows are formatted in parallel and written in order.
extern "C" int knn_write_prefilter_db(const char *data_path, const char *index_path, const int64_t *hits, const float *scores,
                                      int64_t nq, int64_t k, const int64_t *queries, const int64_t *test_map, int64_t n_test,
                                      const int64_t *train_map, int64_t n_train, int32_t clip)
{
    if (!data_path || !index_path || nq < 0 || k < 0) return set_err(KNN_ERR_INVALID, "write_prefilter_db: bad arguments");
    if (nq > 0 && (!hits || !scores || !queries || !test_map || !train_map)) return set_err(KNN_ERR_INVALID, "write_prefilter_db: null pointer");
    FILE *fd = fopen(data_path, "wb");
    FILE *fi = fopen(index_path, "wb");
    if (!fd || !fi) {
        if (fd) fclose(fd);
        if (fi) fclose(fi);
        return set_err(KNN_ERR_IO, std::string("write_prefilter_db: cannot open ") + (fd ? index_path : data_path));
    }
    const int64_t BLOCK = 4096;
    int rc = 0;
    int64_t offset = 0;
    for (int64_t b0 = 0; b0 < nq && rc == 0; b0 += BLOCK) {
        const int64_t m = std::min(BLOCK, nq - b0);
        std::vector<std::string> recs((size_t)m);
        int bad = 0;
#pragma omp parallel for schedule(dynamic, 64) num_threads(hnsw_threads())
        for (int64_t i = 0; i < m; i++) {
            std::string &r = recs[(size_t)i];
            r.reserve((size_t)k * 16 + 1);
            char buf[96];
            for (int64_t j = 0; j < k; j++) {
                const int64_t hit = hits[(b0 + i) * k + j];
                if (hit == -1) continue;
                if (hit < 0 || hit >= n_train) { bad = 1; continue; }
                const float s = scores[(b0 + i) * k + j];
                // clip == 1: numpy.clip(scores, -(10**30), 10**30) * 100 as the reference's pinned numpy
                // 1.22 evaluates it (value-based casting: the 10**30 bounds lift the arithmetic to
                // double); clip == 2: the same expression under numpy >= 2 (NEP 50: stays float32);
                // clip == 0: scores * 100 in float32.  int() truncates toward zero.
                double v;
                if (clip == 1) {
                    double c = (double)s;
                    if (c > 1e30) c = 1e30;
                    if (c < -1e30) c = -1e30;
                    v = c * 100.0;
                } else if (clip == 2) {
                    float c = s;
                    if (c > 1e30f) c = 1e30f;
                    if (c < -1e30f) c = -1e30f;
                    v = (double)(c * 100.0f);
                } else {
                    v = (double)(s * 100.0f);
                }
                v = v < 0 ? ceil(v) : floor(v);
                int n;
                if (fabs(v) < 9.0e18) n = snprintf(buf, sizeof buf, "%lld\t%lld\t0\n", (long long)train_map[hit], (long long)v);
                else n = snprintf(buf, sizeof buf, "%lld\t%.0f\t0\n", (long long)train_map[hit], v);
                r.append(buf, (size_t)n);
            }
            r.push_back('\0');
        }
        if (bad) { rc = set_err(KNN_ERR_INVALID, "write_prefilter_db: hit id outside the train id map"); break; }
        for (int64_t i = 0; i < m; i++) {
            const std::string &r = recs[(size_t)i];
            const int64_t q = queries[b0 + i];
            if (q < 0 || q >= n_test) { rc = set_err(KNN_ERR_INVALID, "write_prefilter_db: query id outside the test id map"); break; }
            if (fwrite(r.data(), 1, r.size(), fd) != r.size()) { rc = set_err(KNN_ERR_IO, "write_prefilter_db: short write"); break; }
            fprintf(fi, "%lld\t%lld\t%lld\n", (long long)test_map[q], (long long)offset, (long long)r.size());
            offset += (int64_t)r.size();
        }
    }
    if (fclose(fd) != 0 && rc == 0) rc = set_err(KNN_ERR_IO, "write_prefilter_db: close failed");
    if (fclose(fi) != 0 && rc == 0) rc = set_err(KNN_ERR_IO, "write_prefilter_db: close failed");
    return rc;
}
