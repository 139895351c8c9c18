// fuse.inc -- the two hit-list fusions of the reference's results script (included by knn355_lib.hip behind pr_curve.inc).
//
// Between a search and the evaluation passes, pfam/proteins.py builds two more hit arrays per query in Python loops under
// tqdm: "combined" (lines 216-240: the MMseqs2 hits with E < 0.1, filled up with the k-NN hits that are not among them)
// and "both aligned" (lines 340-372: two lists concatenated, sorted by e-value, every hit id already seen dropped, cut to
// the width and padded).  Here both are one workgroup of 256 threads per query row over two lists A [ka] and B [kb] of
// (int64 id, float64 score); the contract is above knn_eval_fuse in include/knn355.h.  Scores are float64 because the
// reference's e-values are: below 1.4e-45 a float32 holds 0, and those are the strong homologues whose order decides AUC1.
// The kernel never does arithmetic on a score: it moves the 64 bits and compares integer images of them, so sub-normal
// doubles order by their bits whatever the float units' denormal mode.
//
//   sorted union (KNN_FUSE_SORTED_UNION)
//     stage 1  keys.  Entry p (A's column p, or B's column p - ka) becomes the pair (order word, p): the order word is
//              the monotone 64-bit image of the double (sign bit set for positive, all bits flipped for negative), taken
//              from +0.0 for either zero, complemented when larger is better, all ones for every NaN.  An entry that does
//              not exist (id < 0, or keep_a zero) becomes (all ones, 0xFFFF): behind every NaN.  The double's image
//              fills the word, so the position cannot ride in its low bits as it does in assemble.inc:
//              wg_bitonic_sort_pairs sorts the pairs lexicographically over next_pow2(ka + kb) slots.
//     stage 2  the id of every rank goes to LDS (-1 for a slot that holds no entry: existing ids are never negative).
//     stage 3  rank i is a repeat when an earlier rank holds its id: a quadratic scan of the LDS ids, every lane reading
//              the same word (a broadcast), at most 4096 compares per entry and 16 entries per thread.  Survivors are
//              compacted in rank order by ballot and prefix across the four waves; the walk stops at k_out (stage 3 is
//              eval.inc's wg_dedup_compact, the compaction of the prefix mode its wg_compact).
//   prefix, then fill (KNN_FUSE_PREFIX_FILL)
//     no sort.  A's existing entries are compacted in column order into the output and their ids into LDS; then B's
//     entries whose id a linear (broadcast) scan does not find there are compacted behind them.
//   The rest of the row is padding and filled_out gets the number of outputs.

struct FuseParams {
    const int64_t *ha, *hb;   // the slab's rows [rows][ka], [rows][kb]
    const uint64_t *sa, *sb;  // scores as their bits
    const uint8_t *keep;      // [rows][ka] or null
    int ka, kb, k_out, mode, ascending;
    int P, Pid;               // slots of the sort, slots of the id array
    int64_t *ho;              // [rows][k_out]
    uint64_t *so;
    int32_t *src;             // or null
    int32_t *filled;          // [rows]
};

#define FUSE_NO_POS 0xFFFFu

__device__ __forceinline__ uint64_t fuse_order_word(uint64_t u, int ascending)
{
    const uint64_t mag = u & 0x7FFFFFFFFFFFFFFFull;
    if (mag > 0x7FF0000000000000ull) return KEY_PAD; // NaN: behind +-inf, by position among themselves
    if (mag == 0) u = 0;                              // -0.0 becomes +0.0, the two zeros tie
    const uint64_t o = (u >> 63) ? ~u : (u | 0x8000000000000000ull);
    return ascending ? o : ~o; // (o = 0 would need u = all ones, a NaN: no other score's word is all ones)
}

__global__ __launch_bounds__(256) void fuse_kernel(FuseParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int(*s_wcnt)[4] = (int(*)[4])smem;                // [2][4]
    int64_t *s_id = (int64_t *)(smem + 32);           // [Pid]
    uint64_t *s_key = (uint64_t *)(s_id + p.Pid);     // [P]   (sorted union only)
    uint16_t *s_pos = (uint16_t *)(s_key + p.P);      // [P]
    const int tid = threadIdx.x;
    const size_t q = blockIdx.x;
    const int ka = p.ka, kb = p.kb, k_out = p.k_out, n = ka + kb;
    const int64_t *ha = p.ha + q * ka, *hb = p.hb + q * kb;
    const uint64_t *sa = p.sa + q * ka, *sb = p.sb + q * kb;
    const uint8_t *keep = p.keep ? p.keep + q * ka : nullptr;
    int64_t *ho = p.ho + q * k_out;
    uint64_t *so = p.so + q * k_out;
    int32_t *src = p.src ? p.src + q * k_out : nullptr;
    int par = 0;

    auto emit = [&](int at, int64_t id, uint64_t bits, int pos) {
        ho[at] = id;
        so[at] = bits;
        if (src) src[at] = pos;
    };

    int emitted = 0;
    if (p.mode == KNN_FUSE_SORTED_UNION) {
        // ---- stage 1 ----
        for (int i = tid; i < p.P; i += 256) {
            uint64_t key = KEY_PAD;
            uint16_t pos = FUSE_NO_POS;
            if (i < n) {
                const bool in_a = i < ka;
                const int64_t h = in_a ? ha[i] : hb[i - ka];
                if (h >= 0 && (!in_a || !keep || keep[i])) {
                    key = fuse_order_word(in_a ? sa[i] : sb[i - ka], p.ascending);
                    pos = (uint16_t)i;
                }
            }
            s_key[i] = key;
            s_pos[i] = pos;
        }
        __syncthreads();
        wg_bitonic_sort_pairs(s_key, s_pos, p.P, tid, 256);
        // ---- stage 2 ----
        for (int i = tid; i < n; i += 256) {
            const int pos = s_pos[i];
            s_id[i] = pos == FUSE_NO_POS ? -1 : pos < ka ? ha[pos] : hb[pos - ka];
        }
        __syncthreads();
        // ---- stage 3 ----
        emitted = wg_dedup_compact(s_id, n, k_out, (int64_t)-1, s_wcnt, par, [&](int at, int i, int64_t id) {
            const int pos = s_pos[i];
            emit(at, id, pos < ka ? sa[pos] : sb[pos - ka], pos);
        });
    } else {
        for (int c0 = 0; c0 < ka; c0 += 256) {
            const int i = c0 + tid;
            const int64_t h = i < ka ? ha[i] : -1;
            const bool ok = h >= 0 && (!keep || keep[i]);
            int tot;
            const int at = emitted + wg_compact(ok, s_wcnt, par, &tot);
            if (ok) {
                s_id[at] = h; // (at < ka <= Pid)
                if (at < k_out) emit(at, h, sa[i], i);
            }
            emitted += tot;
        }
        __syncthreads();
        const int na = emitted;
        for (int c0 = 0; c0 < kb && emitted < k_out; c0 += 256) {
            const int i = c0 + tid;
            const int64_t h = i < kb ? hb[i] : -1;
            bool ok = h >= 0;
            for (int j = 0; ok && j < na; j++) ok = s_id[j] != h;
            int tot;
            const int at = emitted + wg_compact(ok, s_wcnt, par, &tot);
            if (ok && at < k_out) emit(at, h, sb[i], ka + i);
            emitted += tot;
        }
        emitted = min(emitted, k_out);
    }
    const double padv = p.ascending ? DBL_MAX : -DBL_MAX;
    for (int i = emitted + tid; i < k_out; i += 256) emit(i, -1, (uint64_t)__double_as_longlong(padv), -1);
    if (tid == 0) p.filled[q] = emitted;
}

extern "C" int knn_eval_fuse(const int64_t *hits_a, const double *scores_a, const uint8_t *keep_a, int64_t ka,
                             const int64_t *hits_b, const double *scores_b, int64_t kb, int64_t nq, int32_t mode,
                             int32_t ascending, int32_t k_out, int64_t *hits_out, double *scores_out, int32_t *source_out,
                             int32_t *filled_out)
{
    if (nq < 0) return set_err(KNN_ERR_INVALID, "fuse: negative nq");
    if (ka < 1 || ka > KNN_MAX_K) return set_err(KNN_ERR_INVALID, "fuse: ka outside [1, KNN_MAX_K]");
    if (kb < 1 || kb > KNN_MAX_K) return set_err(KNN_ERR_INVALID, "fuse: kb outside [1, KNN_MAX_K]");
    if (k_out < 1 || k_out > ka + kb) return set_err(KNN_ERR_INVALID, "fuse: k_out outside [1, ka + kb]");
    if (mode != KNN_FUSE_PREFIX_FILL && mode != KNN_FUSE_SORTED_UNION) return set_err(KNN_ERR_INVALID, "fuse: unknown mode");
    if (nq == 0) return 0;
    if (!hits_a || !scores_a || !hits_b || !scores_b || !hits_out || !scores_out || !filled_out)
        return set_err(KNN_ERR_INVALID, "fuse: null pointer");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    const int n = (int)(ka + kb);
    const int64_t slab = std::min(nq, eval_slab_rows(n));
    const int P = mode == KNN_FUSE_SORTED_UNION ? next_pow2_host(n) : 0;
    const int Pid = mode == KNN_FUSE_SORTED_UNION ? P : next_pow2_host((int)ka);
    const size_t lds = 32 + (size_t)Pid * 8 + (size_t)P * (8 + 2); // 72 KB + 32 at ka + kb = 4096
    HIP_TRY(hipFuncSetAttribute((const void *)fuse_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    EvalBufs bufs;
    EvalCols w(bufs, slab);
    const FuseParams p = {w.in(hits_a, (size_t)ka * 8),
                          w.in(hits_b, (size_t)kb * 8),
                          (const uint64_t *)w.in(scores_a, (size_t)ka * 8),
                          (const uint64_t *)w.in(scores_b, (size_t)kb * 8),
                          w.in(keep_a, (size_t)ka),
                          (int)ka, (int)kb, k_out, mode, ascending ? 1 : 0, P, Pid,
                          w.out(hits_out, (size_t)k_out * 8),
                          (uint64_t *)w.out(scores_out, (size_t)k_out * 8),
                          w.out(source_out, (size_t)k_out * 4),
                          w.out(filled_out, 4)};
    EVAL_TRY(w.ready());
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(w.upload(r0, m));
        hipLaunchKernelGGL(fuse_kernel, dim3((unsigned)m), dim3(256), lds, 0, p);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(w.download(r0, m));
    }
    return 0;
}
