// pr_curve.inc -- the precision-recall threshold sweep over (is_correct, scores) (included by knn355_lib.hip behind
// assemble.inc).
//
// The reference computes its precision-recall curves in a Python loop over every query, once per threshold
// (pfam/proteins.py:626-648: 301 thresholds x 200 k queries, five times over).  Here a query costs one pass over its
// cells whatever the number of thresholds; the contract is above knn_eval_pr_curve in include/knn355.h.
//
//   pr_curve_kernel  one workgroup of 256 threads per block of 256 consecutive queries, one query at a time:
//     histogram  the threads stride over the query's `limit` cells (coalesced loads of the score row and the byte row);
//                a cell's bucket is c = #{i : thr[i] < (double)score}, one binary search over the thresholds in LDS (a
//                NaN compares false everywhere: c = 0); the cell is selected at the thresholds j < c, so c >= 1 adds
//                (1 << 32 | correct) to bin c - 1 of one LDS histogram of 64-bit words (ds_add_u64: selected cells in the
//                high half, correct ones in the low half; both stay below 2^31 because limit <= INT32_MAX)
//     scan       n(j) and tp(j) are the suffix sum of the bins j .. nthr - 1.  The bins go through the workgroup 256 at
//                a time from the top: a shuffle scan inside each wave, the four wave totals through LDS (two sets in
//                turn, so one barrier per 256 bins), a carry for the bins of the passes before.  The thread that reads
//                a bin clears it for the next query in front of that barrier.
//     terms      pass m leaves thread t with n and tp of threshold 256 m + t: it forms P and R and adds them to
//                register accumulators (TPT = thresholds per thread: doubles for the two sums, int64 for the three
//                counts).  Queries are taken in row order, so every accumulator gets its terms in row order.
//   At the end the block's P and R sums go to [block][nthr] arrays and the counts to global memory by atomicAdd (integer
//   sums do not depend on the order).
//   pr_fold_kernel   one workgroup, thread per threshold: adds a slab's block sums to the running sums in block order.

struct PrCurveParams {
    const uint8_t *is_correct; // the slab's rows [rows][k]
    const float *scores;
    const int64_t *totals;     // [rows]
    const double *thr;         // [nthr]
    int64_t rows;
    int k, limit, nthr;
    double *block_p, *block_r;  // [blocks of the slab][nthr]
    unsigned long long *counts; // [3][nthr]: selected, tp, empty
};

template <int TPT>
__global__ __launch_bounds__(256) void pr_curve_kernel(PrCurveParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double *s_thr = (double *)smem;                                   // [nthr]
    unsigned long long *s_h = (unsigned long long *)(s_thr + p.nthr); // [nthr] selected << 32 | correct
    __shared__ unsigned long long s_wtot[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nthr = p.nthr, limit = p.limit;
    for (int i = tid; i < nthr; i += 256) {
        s_thr[i] = p.thr[i];
        s_h[i] = 0;
    }
    __syncthreads();
    double acc_p[TPT], acc_r[TPT];
    unsigned long long acc_n[TPT], acc_tp[TPT], acc_e[TPT];
#pragma unroll
    for (int m = 0; m < TPT; m++) {
        acc_p[m] = 0.0;
        acc_r[m] = 0.0;
        acc_n[m] = acc_tp[m] = acc_e[m] = 0;
    }
    const int64_t r0 = (int64_t)blockIdx.x * 256, r1 = min(r0 + 256, p.rows);
    int par = 0;
    for (int64_t r = r0; r < r1; r++) {
        const float *sc = p.scores + r * p.k;
        const uint8_t *ic = p.is_correct + r * p.k;
        for (int c = tid; c < limit; c += 256) {
            const double v = (double)sc[c];
            const int lo = lower_bound_dev(0, nthr, [&](int i) { return s_thr[i] < v; });
            if (lo) atomicAdd(&s_h[lo - 1], (1ull << 32) | (ic[c] ? 1ull : 0ull));
        }
        const double total = (double)p.totals[r];
        __syncthreads();
        unsigned long long carry = 0; // the bins of the passes before (the same in every thread)
#pragma unroll
        for (int m = TPT - 1; m >= 0; m--) {
            if (m * 256 >= nthr) continue; // (uniform)
            const int j = m * 256 + tid;
            unsigned long long v = 0;
            if (j < nthr) {
                v = s_h[j];
                s_h[j] = 0;
            }
            for (int off = 1; off < 64; off <<= 1) {
                const unsigned long long u = __shfl_down(v, off, 64);
                if (lane + off < 64) v += u;
            }
            if (lane == 0) s_wtot[par][wave] = v;
            __syncthreads();
            unsigned long long above = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 4; w++) {
                const unsigned long long t = s_wtot[par][w];
                above += w > wave ? t : 0;
                all += t;
            }
            par ^= 1; // the next pass writes the other set: one barrier per pass is enough
            v += above + carry;
            carry += all;
            if (j < nthr) {
                const uint32_t n = (uint32_t)(v >> 32), tp = (uint32_t)v;
                acc_p[m] += n ? (double)tp / (double)n : 1.0;
                acc_r[m] += (double)tp / total;
                acc_n[m] += n;
                acc_tp[m] += tp;
                acc_e[m] += n ? 0 : 1;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < TPT; m++) {
        const int j = m * 256 + tid;
        if (j < nthr) {
            p.block_p[(size_t)blockIdx.x * nthr + j] = acc_p[m];
            p.block_r[(size_t)blockIdx.x * nthr + j] = acc_r[m];
            atomicAdd(&p.counts[j], acc_n[m]);
            atomicAdd(&p.counts[(size_t)nthr + j], acc_tp[m]);
            atomicAdd(&p.counts[2 * (size_t)nthr + j], acc_e[m]);
        }
    }
}

// sums[0][j] += block_p[0][j], then block_p[1][j], ...: the running S of the contract; sums[1] likewise from block_r
__global__ __launch_bounds__(256) void pr_fold_kernel(const double *__restrict__ block_p, const double *__restrict__ block_r,
                                                      int64_t blocks, int nthr, double *__restrict__ sums)
{
    for (int j = threadIdx.x; j < nthr; j += 256) {
        double sp = sums[j], sr = sums[nthr + j];
        for (int64_t b = 0; b < blocks; b++) {
            sp += block_p[b * nthr + j];
            sr += block_r[b * nthr + j];
        }
        sums[j] = sp;
        sums[nthr + j] = sr;
    }
}

template <int TPT>
static int pr_curve_launch(const PrCurveParams &p, int64_t blocks, size_t lds)
{
    HIP_TRY(hipFuncSetAttribute((const void *)pr_curve_kernel<TPT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(pr_curve_kernel<TPT>, dim3((unsigned)blocks), dim3(256), lds, 0, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int knn_eval_pr_curve(const uint8_t *is_correct, const float *scores, int64_t nq, int64_t k, int64_t limit,
                                 const int64_t *totals, const double *thresholds, int32_t nthr, double *precision_out,
                                 double *recall_out, int64_t *selected_out, int64_t *tp_out, int64_t *empty_out)
{
    if (nq < 1) return set_err(KNN_ERR_INVALID, "pr_curve: need nq >= 1");
    if (k < 1) return set_err(KNN_ERR_INVALID, "pr_curve: need k >= 1");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "pr_curve: k > INT32_MAX");
    if (limit < 1 || limit > k) return set_err(KNN_ERR_INVALID, "pr_curve: limit outside [1, k]");
    if (nthr < 1 || nthr > 4096) return set_err(KNN_ERR_INVALID, "pr_curve: nthr outside [1, 4096]");
    if (!is_correct || !scores || !totals || !thresholds || !precision_out || !recall_out)
        return set_err(KNN_ERR_INVALID, "pr_curve: null pointer");
    for (int64_t q = 0; q < nq; q++)
        if (totals[q] < 1) return set_err(KNN_ERR_INVALID, "pr_curve: a total below 1");
    for (int32_t j = 0; j < nthr; j++) {
        if (thresholds[j] != thresholds[j]) return set_err(KNN_ERR_INVALID, "pr_curve: NaN threshold");
        if (j && thresholds[j] < thresholds[j - 1]) return set_err(KNN_ERR_INVALID, "pr_curve: thresholds decrease");
    }
    int rc = ensure_device(g_device);
    if (rc) return rc;
    // whole blocks of 256 rows per slab: a block never straddles two slabs
    int64_t slab = eval_slab_rows(k);
    slab = slab > INT64_MAX - 255 ? INT64_MAX / 256 * 256 : (slab + 255) / 256 * 256;
    slab = std::min(slab, (nq + 255) / 256 * 256);
    const int64_t rows_cap = std::min(slab, nq), blocks_cap = slab / 256;
    const size_t lds = (size_t)nthr * 16;
    EvalBufs bufs;
    std::vector<double> sums((size_t)nthr * 2);
    std::vector<int64_t> cnt((size_t)nthr * 3);
    EvalCols tab(bufs, 1), w(bufs, rows_cap);
    const double *d_thr = tab.in(thresholds, (size_t)nthr * 8);
    double *d_sums = tab.out(sums.data(), sums.size() * 8);
    unsigned long long *d_cnt = (unsigned long long *)tab.out(cnt.data(), cnt.size() * 8);
    const uint8_t *d_ic = w.in(is_correct, (size_t)k);
    const float *d_sc = w.in(scores, (size_t)k * 4);
    const int64_t *d_tot = w.in(totals, 8);
    EVAL_ALLOC(d_bp, double *, (size_t)blocks_cap * nthr * 8);
    EVAL_ALLOC(d_br, double *, (size_t)blocks_cap * nthr * 8);
    EVAL_TRY(w.ready());
    EVAL_TRY(tab.upload(0, 1));
    HIP_TRY(hipMemset(d_sums, 0, sums.size() * 8)); // (all bits zero: +0.0)
    HIP_TRY(hipMemset(d_cnt, 0, cnt.size() * 8));
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0), blocks = (m + 255) / 256;
        EVAL_TRY(w.upload(r0, m));
        const PrCurveParams p = {d_ic, d_sc, d_tot, d_thr, m, (int)k, (int)limit, nthr, d_bp, d_br, d_cnt};
        if (nthr <= 256) rc = pr_curve_launch<1>(p, blocks, lds);
        else if (nthr <= 512) rc = pr_curve_launch<2>(p, blocks, lds);
        else if (nthr <= 1024) rc = pr_curve_launch<4>(p, blocks, lds);
        else if (nthr <= 2048) rc = pr_curve_launch<8>(p, blocks, lds);
        else rc = pr_curve_launch<16>(p, blocks, lds);
        if (rc) return rc;
        hipLaunchKernelGGL(pr_fold_kernel, dim3(1), dim3(256), 0, 0, d_bp, d_br, blocks, (int)nthr, d_sums);
        HIP_TRY(hipGetLastError());
    }
    EVAL_TRY(tab.download(0, 1));
    for (int32_t j = 0; j < nthr; j++) {
        precision_out[j] = sums[(size_t)j] / (double)nq;
        recall_out[j] = sums[(size_t)nthr + j] / (double)nq;
        if (selected_out) selected_out[j] = cnt[(size_t)j];
        if (tp_out) tp_out[j] = cnt[(size_t)nthr + j];
        if (empty_out) empty_out[j] = cnt[2 * (size_t)nthr + j];
    }
    return 0;
}
