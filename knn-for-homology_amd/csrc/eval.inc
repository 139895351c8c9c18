// eval.inc -- consumers of the (hits, scores) arrays, SURVEY.md section 8(f) N4 (included by knn355.hip).
//
// The reference post-processes search results with per-row Python loops
// (pfam/proteins.py:85-122 remove_self_hit; seqvec_search/main.py:64-82 evaluate;
// pfam/proteins_shared.py:139-157 compute_auc1; cath/cath.py:76-84 compute_is_correct;
// seqvec_search/tp_cumulative.py:15-34).  At 200k queries x 1000 hits these loops dominate the
// wall time after the search.  Here each is one pass of integer work over hits[nq][k]: one wave
// per row, coalesced reads of the row, gathers into small label tables.
#include <errno.h>
#include <stdlib.h>

// out row = in row with the element at `index` removed; index = position of the self id
// (0 when the search put it first), or k-1 when the row does not contain it (counted missing)
__global__ void remove_self_hit_kernel(const int64_t *__restrict__ hits, const float *__restrict__ scores, int64_t nq, int k,
                                       const int64_t *__restrict__ self_ids, int64_t *__restrict__ hits_out,
                                       float *__restrict__ scores_out, int32_t *__restrict__ missing)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= nq) return;
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
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= nq) return;
    const int32_t lq = labels_q[r];
    int cnt = 0, first_bad = k;
    for (int j = lane; j < k; j += 64) {
        const int64_t hid = hits[r * k + j];
        const bool ok = hid >= 0 && hid < nb && labels_db[hid] == lq;
        if (is_correct) is_correct[r * k + j] = ok ? 1 : 0;
        cnt += ok ? 1 : 0;
        if (!ok) first_bad = min(first_bad, j);
    }
    for (int off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        first_bad = min(first_bad, __shfl_xor(first_bad, off, 64));
    }
    if (lane == 0) {
        lead[r] = first_bad;
        tp[r] = cnt;
    }
}

// set-membership evaluation (pfam/proteins_shared.py:139-157): query r is homologous to the
// sorted target rows members[offsets[r] .. offsets[r+1]).  MATRIX: the per-hit membership bytes
// (pfam/proteins.py:201-207 compute_correctness_array) instead of the leading run and the count
template <bool MATRIX>
__global__ void set_eval_kernel(const int64_t *__restrict__ hits, int64_t nq, int k, const int64_t *__restrict__ offsets,
                                const int64_t *__restrict__ members, int32_t *__restrict__ lead, int32_t *__restrict__ tp,
                                uint8_t *__restrict__ is_correct)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= nq) return;
    const int64_t lo0 = offsets[r], hi0 = offsets[r + 1];
    int cnt = 0, first_bad = k;
    for (int j = lane; j < k; j += 64) {
        const int64_t hid = hits[r * k + j];
        int64_t lo = lo0, hi = hi0;
        while (lo < hi) {
            const int64_t mid = (lo + hi) >> 1;
            if (members[mid] < hid) lo = mid + 1; else hi = mid;
        }
        const bool ok = lo < hi0 && members[lo] == hid;
        if (MATRIX) {
            is_correct[r * k + j] = ok ? 1 : 0;
            continue;
        }
        cnt += ok ? 1 : 0;
        if (!ok) first_bad = min(first_bad, j);
    }
    if (MATRIX) return;
    for (int off = 32; off >= 1; off >>= 1) {
        cnt += __shfl_xor(cnt, off, 64);
        first_bad = min(first_bad, __shfl_xor(first_bad, off, 64));
    }
    if (lane == 0) {
        lead[r] = first_bad;
        tp[r] = cnt;
    }
}

// cath/cath.py:76-84: out[q][l][j] = mapping[query_rows[q]][l] == mapping[hits[q][j]][l]
__global__ void levels_eval_kernel(const int64_t *__restrict__ hits, int64_t nq, int k, const int64_t *__restrict__ query_rows,
                                   const int32_t *__restrict__ mapping, int64_t n, int nlevels, uint8_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (r >= nq) return;
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
struct EvalBufs {
    std::vector<std::pair<void *, size_t>> dev;
    ~EvalBufs() { for (auto &b : dev) if (b.first) (void)hipFree(b.first); }
    void *get(size_t bytes)
    {
        void *p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(bytes, 16)) != hipSuccess) return nullptr;
        dev.push_back({p, bytes});
        return p;
    }
};
#define EVAL_ALLOC(var, type, bytes)                                                    \
    type var = (type)bufs.get(bytes);                                                   \
    if (!var) return set_err(KNN_ERR_HIP, "eval: out of device memory")

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
    EVAL_ALLOC(d_h, int64_t *, (size_t)slab * k * 8);
    EVAL_ALLOC(d_s, float *, (size_t)slab * k * 4);
    EVAL_ALLOC(d_self, int64_t *, (size_t)slab * 8);
    EVAL_ALLOC(d_ho, int64_t *, (size_t)slab * (k - 1) * 8);
    EVAL_ALLOC(d_so, float *, (size_t)slab * (k - 1) * 4);
    EVAL_ALLOC(d_m, int32_t *, (size_t)slab * 4);
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        HIP_TRY(hipMemcpy(d_h, hits + r0 * k, (size_t)m * k * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_s, scores + r0 * k, (size_t)m * k * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_self, self_ids + r0, (size_t)m * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(remove_self_hit_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, d_s, m, (int)k, d_self, d_ho, d_so, d_m);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(hits_out + r0 * (k - 1), d_ho, (size_t)m * (k - 1) * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(scores_out + r0 * (k - 1), d_so, (size_t)m * (k - 1) * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(missing_out + r0, d_m, (size_t)m * 4, hipMemcpyDeviceToHost));
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
    EVAL_ALLOC(d_h, int64_t *, (size_t)slab * k * 8);
    EVAL_ALLOC(d_lq, int32_t *, (size_t)slab * 4);
    EVAL_ALLOC(d_ldb, int32_t *, (size_t)nb * 4);
    EVAL_ALLOC(d_ic, uint8_t *, (size_t)slab * k);
    EVAL_ALLOC(d_lead, int32_t *, (size_t)slab * 4);
    EVAL_ALLOC(d_tp, int32_t *, (size_t)slab * 4);
    if (nb) HIP_TRY(hipMemcpy(d_ldb, labels_db, (size_t)nb * 4, hipMemcpyHostToDevice));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        HIP_TRY(hipMemcpy(d_h, hits + r0 * k, (size_t)m * k * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_lq, labels_q + r0, (size_t)m * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(label_eval_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, m, (int)k, d_lq, d_ldb, nb,
                           is_correct_out ? d_ic : (uint8_t *)nullptr, d_lead, d_tp);
        HIP_TRY(hipGetLastError());
        if (is_correct_out) HIP_TRY(hipMemcpy(is_correct_out + r0 * k, d_ic, (size_t)m * k, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(lead_out + r0, d_lead, (size_t)m * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(tp_out + r0, d_tp, (size_t)m * 4, hipMemcpyDeviceToHost));
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
    if (set_offsets[0] < 0) return set_err(KNN_ERR_INVALID, "eval_sets: negative set offset");
    for (int64_t r = 0; r < nq; r++)
        if (set_offsets[r + 1] < set_offsets[r]) return set_err(KNN_ERR_INVALID, "eval_sets: set offsets decrease");
    const int64_t nmem = set_offsets[nq];
    if (nmem > 0 && !set_members) return set_err(KNN_ERR_INVALID, "eval_sets: null pointer");
    for (int64_t r = 0; r < nq; r++)
        for (int64_t i = set_offsets[r] + 1; i < set_offsets[r + 1]; i++)
            if (set_members[i] < set_members[i - 1]) return set_err(KNN_ERR_INVALID, "eval_sets: set members not sorted");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    EvalBufs bufs;
    const int64_t slab = std::min(nq, eval_slab_rows(k));
    EVAL_ALLOC(d_h, int64_t *, (size_t)slab * k * 8);
    EVAL_ALLOC(d_off, int64_t *, (size_t)(nq + 1) * 8);
    EVAL_ALLOC(d_mem, int64_t *, (size_t)nmem * 8);
    EVAL_ALLOC(d_lead, int32_t *, matrix ? 0 : (size_t)slab * 4);
    EVAL_ALLOC(d_tp, int32_t *, matrix ? 0 : (size_t)slab * 4);
    EVAL_ALLOC(d_ic, uint8_t *, matrix ? (size_t)slab * k : 0);
    HIP_TRY(hipMemcpy(d_off, set_offsets, (size_t)(nq + 1) * 8, hipMemcpyHostToDevice));
    if (nmem) HIP_TRY(hipMemcpy(d_mem, set_members, (size_t)nmem * 8, hipMemcpyHostToDevice));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        HIP_TRY(hipMemcpy(d_h, hits + r0 * k, (size_t)m * k * 8, hipMemcpyHostToDevice));
        if (matrix) {
            hipLaunchKernelGGL(set_eval_kernel<true>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, m, (int)k, d_off + r0, d_mem,
                               d_lead, d_tp, d_ic);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpy(is_correct_out + r0 * k, d_ic, (size_t)m * k, hipMemcpyDeviceToHost));
            continue;
        }
        hipLaunchKernelGGL(set_eval_kernel<false>, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, m, (int)k, d_off + r0, d_mem,
                           d_lead, d_tp, d_ic);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(lead_out + r0, d_lead, (size_t)m * 4, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(tp_out + r0, d_tp, (size_t)m * 4, hipMemcpyDeviceToHost));
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
    EVAL_ALLOC(d_h, int64_t *, (size_t)slab * k * 8);
    EVAL_ALLOC(d_q, int64_t *, (size_t)slab * 8);
    EVAL_ALLOC(d_map, int32_t *, (size_t)n * nlevels * 4);
    EVAL_ALLOC(d_out, uint8_t *, (size_t)slab * nlevels * k);
    HIP_TRY(hipMemcpy(d_map, mapping, (size_t)n * nlevels * 4, hipMemcpyHostToDevice));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        HIP_TRY(hipMemcpy(d_h, hits + r0 * k, (size_t)m * k * 8, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_q, query_rows + r0, (size_t)m * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(levels_eval_kernel, dim3((unsigned)((m + 3) / 4)), dim3(256), 0, 0, d_h, m, (int)k, d_q, d_map, n, (int)nlevels, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(out + (size_t)r0 * nlevels * k, d_out, (size_t)m * nlevels * k, hipMemcpyDeviceToHost));
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
