// assemble.inc -- protein-level hits from slice searches (included by knn355_lib.hip behind eval.inc).
//
// The reference searches fixed-length windows ("slices") of proteins (pfam/slices/slices_search.py) and then assembles
// the slice hits per protein in a Python loop under tqdm (pfam/slices/slices.py:256-291 assemble): the k hits of every
// slice of a protein are concatenated, sorted by score, cut at k, and walked once, ignoring every hit whose protein
// was already picked.  Here that is one workgroup per query group (protein); the contract is above knn_eval_assemble
// in include/knn355.h.
//
//   stage 1  selection.  The group's entries are streamed 256 at a time.  Entry p becomes the 64-bit key
//            (order word of its score << 32 | p): the order word is f2ord of the score (negated when larger is
//            better) with -0.0 folded into +0.0 and every NaN mapped to 0xFFFFFFFF, so one unsigned compare gives the
//            contract's whole order, position tie-break included, and the keys of a group are distinct.  Keys below
//            the running bound T (the depth-th best so far; KEY_PAD until depth keys have been seen) are appended to
//            an LDS buffer of N = max(2 * next_pow2(depth), 1024) keys by ballot and prefix count; when the next 256
//            would not fit, the workgroup sorts the buffer (wg_bitonic_sort), keeps the first depth and tightens T.
//            Nothing assumes that the k hits of a row arrive sorted.
//   stage 2  lookup and de-duplication.  For the <= depth selected keys in rank order the hit's group is looked up
//            (row_group; a hit outside [0, nb), a negative group and the query's own group become "no group"), then
//            rank i is a duplicate when an earlier rank holds its group: a quadratic scan of the LDS array, every lane
//            reading the same word (a broadcast).  depth <= 2048 bounds it at 8 k compares per thread; the reference's
//            depth of 100..1000 is far below that, and the alternative (a second sort by (group, rank), marking heads,
//            and a scatter back to rank order) costs more than the scan up to that depth.
//   stage 3  compaction.  Survivors are written in rank order (eval.inc's wg_dedup_compact does the scan of stage 2 and
//            this walk: ballot per wave, the waves' counts through LDS, prefix); the walk stops at k_out and the rest of
//            the row is padding.

struct AssembleParams {
    const int64_t *hits;        // the slab's rows [rows][k]
    const float *scores;
    const int64_t *offs;        // [groups of the slab + 1] row offsets (absolute)
    int64_t row0;               // absolute number of the slab's first row
    const int32_t *row_group;   // [nb]
    int64_t nb;
    const int32_t *self_group;  // [groups of the slab] or null
    int k, depth, k_out, ascending;
    int N;                      // keys in the LDS buffer
    int64_t *groups_out;        // [groups of the slab][k_out]
    float *scores_out;
    int64_t *qrow_out, *hit_out; // or null
};

__device__ __forceinline__ uint64_t assemble_key(float s, uint32_t pos, int ascending)
{
    uint32_t o = 0xFFFFFFFFu; // NaN: behind +inf (0xFF800000), by position among themselves
    if (s == s) o = f2ord((ascending ? s : -s) + 0.0f); // (+ 0.0f: -0.0 becomes +0.0, the two zeros tie)
    return ((uint64_t)o << 32) | pos;
}

__global__ __launch_bounds__(256) void assemble_kernel(AssembleParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t *sb = (uint64_t *)smem;          // [N] keys
    int32_t *s_grp = (int32_t *)(sb + p.N);   // [depth] group of rank i, -1 = none
    __shared__ int s_wcnt[2][4];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t r_lo = p.offs[g], r_hi = p.offs[g + 1];
    const int n = (int)((r_hi - r_lo) * p.k); // (the host refuses groups of 2^31 entries or more)
    const int64_t base = (r_lo - p.row0) * p.k;
    const float *sc = p.scores + base;
    const int64_t *hh = p.hits + base;
    const int depth = p.depth, k_out = p.k_out, N = p.N;
    int fill = 0, par = 0;
    uint64_t T = KEY_PAD;

    // sorts the fill keys of the buffer and keeps the best depth of them (callers put a barrier in front)
    auto cut = [&]() {
        int P = 64;
        while (P < fill) P <<= 1; // (fill <= N, a power of two)
        for (int i = fill + tid; i < P; i += 256) sb[i] = KEY_PAD;
        __syncthreads();
        wg_bitonic_sort(sb, P, tid, 256);
        if (fill >= depth) {
            fill = depth;
            T = sb[depth - 1];
        }
    };

    // ---- stage 1 ----
    for (int b0 = 0; b0 < n; b0 += 256) {
        if (fill + 256 > N) { // (uniform; after a cut fill <= depth <= N - 256)
            __syncthreads();
            cut();
        }
        const int idx = b0 + tid;
        const uint64_t key = idx < n ? assemble_key(sc[idx], (uint32_t)idx, p.ascending) : KEY_PAD;
        const bool pass = key < T;
        int tot;
        const int pos = fill + wg_compact(pass, s_wcnt, par, &tot);
        if (pass) sb[pos] = key;
        fill += tot;
    }
    __syncthreads();
    cut();
    const int m = min(fill, depth);

    // ---- stage 2 ----
    const int32_t self = p.self_group ? p.self_group[g] : -1;
    for (int i = tid; i < m; i += 256) {
        const int64_t hit = hh[(uint32_t)sb[i]];
        int32_t gv = -1;
        if (hit >= 0 && hit < p.nb) gv = p.row_group[hit];
        if (gv < 0 || gv == self) gv = -1;
        s_grp[i] = gv;
    }
    __syncthreads();

    // ---- stage 3 ----
    const int emitted = wg_dedup_compact(s_grp, m, k_out, (int32_t)-1, s_wcnt, par, [&](int pos, int i, int32_t gv) {
        const uint32_t pp = (uint32_t)sb[i];
        const size_t o = (size_t)g * k_out + pos;
        p.groups_out[o] = gv;
        p.scores_out[o] = sc[pp];
        if (p.qrow_out) p.qrow_out[o] = r_lo + pp / (uint32_t)p.k;
        if (p.hit_out) p.hit_out[o] = hh[pp];
    });
    for (int i = emitted + tid; i < k_out; i += 256) {
        const size_t o = (size_t)g * k_out + i;
        p.groups_out[o] = -1;
        p.scores_out[o] = p.ascending ? FLT_MAX : -FLT_MAX;
        if (p.qrow_out) p.qrow_out[o] = -1;
        if (p.hit_out) p.hit_out[o] = -1;
    }
}

extern "C" int knn_eval_assemble(const int64_t *hits, const float *scores, int64_t ns, int64_t k, const int64_t *group_offsets,
                                 int64_t ng, const int32_t *row_group, int64_t nb, const int32_t *self_group, int32_t depth,
                                 int32_t k_out, int32_t ascending, int64_t *groups_out, float *scores_out, int64_t *qrow_out,
                                 int64_t *hit_out)
{
    if (ns < 0 || ng < 0 || nb < 0) return set_err(KNN_ERR_INVALID, "assemble: negative ns, ng or nb");
    if (k < 1) return set_err(KNN_ERR_INVALID, "assemble: need k >= 1");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "assemble: k > INT32_MAX");
    if (depth < 1 || depth > KNN_MAX_K) return set_err(KNN_ERR_INVALID, "assemble: depth outside [1, KNN_MAX_K]");
    if (k_out < 1 || k_out > depth) return set_err(KNN_ERR_INVALID, "assemble: k_out outside [1, depth]");
    if (ng == 0) return 0;
    if (!group_offsets || !groups_out || !scores_out || (ns > 0 && (!hits || !scores)) || (nb > 0 && !row_group))
        return set_err(KNN_ERR_INVALID, "assemble: null pointer");
    EVAL_TRY(eval_check_offsets("assemble", "group", group_offsets, ng, ns));
    for (int64_t g = 0; g < ng; g++)
        if (group_offsets[g + 1] - group_offsets[g] > (((int64_t)1 << 31) - 1) / k)
            return set_err(KNN_ERR_INVALID, "assemble: a group of 2^31 entries or more");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    // slabs of whole groups: as many as fit the slab's rows (one at least, however large) and 256 MiB of group ids
    const int64_t slab_rows = eval_slab_rows(k);
    const int64_t gcap = std::max<int64_t>(1, (int64_t)(256ull << 20) / ((int64_t)k_out * 8));
    std::vector<int64_t> cuts(1, 0);
    int64_t max_rows = 0, max_groups = 0;
    for (int64_t g0 = 0; g0 < ng;) {
        int64_t g1 = g0 + 1;
        while (g1 < ng && g1 - g0 < gcap && group_offsets[g1 + 1] - group_offsets[g0] <= slab_rows) g1++;
        max_rows = std::max(max_rows, group_offsets[g1] - group_offsets[g0]);
        max_groups = std::max(max_groups, g1 - g0);
        cuts.push_back(g1);
        g0 = g1;
    }
    const int N = std::max(2 * std::max(64, next_pow2_host(depth)), 1024);
    const size_t lds = (size_t)N * 8 + (size_t)depth * 4;
    EvalBufs bufs;
    // the inputs advance by rows and the outputs (and self_group) by groups: one walker each
    EvalCols tab(bufs, 1), rows(bufs, max_rows), grp(bufs, max_groups);
    const int64_t *d_off = tab.in(group_offsets, (size_t)(ng + 1) * 8);
    const int32_t *d_rg = tab.in(row_group, (size_t)nb * 4);
    const int64_t *d_h = rows.in(hits, (size_t)k * 8);
    const float *d_s = rows.in(scores, (size_t)k * 4);
    const int32_t *d_self = grp.in(self_group, 4);
    int64_t *d_go = grp.out(groups_out, (size_t)k_out * 8);
    float *d_so = grp.out(scores_out, (size_t)k_out * 4);
    int64_t *d_qo = grp.out(qrow_out, (size_t)k_out * 8);
    int64_t *d_ho = grp.out(hit_out, (size_t)k_out * 8);
    EVAL_TRY(grp.ready());
    EVAL_TRY(tab.upload(0, 1));
    for (size_t c = 0; c + 1 < cuts.size(); c++) {
        const int64_t g0 = cuts[c], m = cuts[c + 1] - g0;
        const int64_t row0 = group_offsets[g0];
        EVAL_TRY(rows.upload(row0, group_offsets[g0 + m] - row0));
        EVAL_TRY(grp.upload(g0, m));
        const AssembleParams p = {d_h, d_s, d_off + g0, row0, d_rg, nb, d_self, (int)k, depth, k_out, ascending ? 1 : 0, N, d_go, d_so, d_qo, d_ho};
        hipLaunchKernelGGL(assemble_kernel, dim3((unsigned)m), dim3(256), lds, 0, p);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(grp.download(g0, m));
    }
    return 0;
}
