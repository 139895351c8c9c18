// bootstrap.inc -- the bootstrap of the CATH accuracy table (included by knn355_lib.hip behind pr_curve.inc).
//
// The reference resamples the evaluable queries 500 times per method and rebuilds, per resample, a Counter of
// superfamilies and a Python list of 1 / count (cath/cath.py:404-438, once per method from :441-458).  Here a
// (replicate, method) pair costs one pass over the resample's ids; the contract is above knn_eval_bootstrap in
// include/knn355.h.
//
//   bootstrap_kernel  one workgroup of 256 threads per (replicate, method):
//     histogram  two uint32 arrays of nfam words in dynamic LDS, count and corr, zeroed by the workgroup.  The threads
//                stride over the n samples: one id from the replicate's row (coalesced), then family[id] and the method's
//                is_correct[id] (gathers out of tables that stay in L2), one LDS integer add on count[f] and one on
//                corr[f] when the sample is correct.  Integer adds commute: nothing depends on the order of the threads.
//                count is recomputed for every method, which is cheaper than a second launch and a global table.
//     reduction  wave w takes the blocks w, w + 4, ... of 256 consecutive codes, 64 codes at a time: every lane forms the
//                term of its code (one IEEE division; +0.0 for an absent family), a ballot counts the present ones, and
//                the 64 terms are added to the block's sum lane by lane, that is in code order.  Every term is >= +0.0,
//                so the +0.0 of an absent family leaves the sum's bits as they are (x + +0.0 == x for x >= +0.0, +0.0
//                included): the sum is the one over the present families only.  64 codes with no present family are
//                skipped.  Thread 0 then adds the block sums in block order and writes the outputs.
//   LDS: 8 * nfam bytes, 128 KiB at the cap of 16384 families (of the CU's 160 KiB); CATH's few thousand families leave
//   room for several workgroups per CU.

struct BootstrapParams {
    const uint8_t *is_correct; // [nm][n]
    const int32_t *family;     // [n]
    const int32_t *sample_ids; // the slab's replicates [rows][n]
    int64_t nb, b0, m0;        // replicates of the call; the slab's first replicate; the launch's first method
    int n, nfam;
    long long *correct; // [nm][nb]
    int32_t *present;   // [nb]
    double *normalized, *raw; // [nm][nb]
};

#define BOOTSTRAP_MAX_BLOCKS (KNN_BOOTSTRAP_MAX_FAMILIES / 256)

__global__ __launch_bounds__(256) void bootstrap_kernel(BootstrapParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint32_t *s_count = (uint32_t *)smem; // [nfam]
    uint32_t *s_corr = s_count + p.nfam;  // [nfam]
    __shared__ double s_bsum[BOOTSTRAP_MAX_BLOCKS];
    __shared__ uint32_t s_bpresent[BOOTSTRAP_MAX_BLOCKS], s_bcorrect[BOOTSTRAP_MAX_BLOCKS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = p.n, nfam = p.nfam;
    const int64_t m = p.m0 + blockIdx.y, b = p.b0 + blockIdx.x;
    for (int i = tid; i < 2 * nfam; i += 256) s_count[i] = 0;
    __syncthreads();
    const int32_t *ids = p.sample_ids + (int64_t)blockIdx.x * n;
    const uint8_t *ic = p.is_correct + m * n;
    for (int i = tid; i < n; i += 256) {
        const int32_t id = ids[i];
        const int32_t f = p.family[id];
        atomicAdd(&s_count[f], 1u);
        if (ic[id]) atomicAdd(&s_corr[f], 1u);
    }
    __syncthreads();
    const int nblk = (nfam + 255) >> 8;
    for (int blk = wave; blk < nblk; blk += 4) {
        double s = 0.0;
        uint32_t present = 0, correct = 0;
        for (int c = 0; c < 4; c++) {
            const int f = blk * 256 + c * 64 + lane;
            const uint32_t cnt = f < nfam ? s_count[f] : 0, cr = f < nfam ? s_corr[f] : 0;
            const unsigned long long mask = __ballot(cnt != 0);
            if (!mask) continue; // (uniform)
            present += (uint32_t)__popcll(mask);
            correct += cr;
            const double t = cnt ? (double)cr / (double)cnt : 0.0;
#pragma unroll
            for (int l = 0; l < 64; l++) s += __shfl(t, l, 64);
        }
        for (int off = 32; off; off >>= 1) correct += __shfl_xor(correct, off, 64);
        if (lane == 0) {
            s_bsum[blk] = s;
            s_bpresent[blk] = present;
            s_bcorrect[blk] = correct;
        }
    }
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        long long correct = 0;
        int32_t present = 0;
        for (int blk = 0; blk < nblk; blk++) {
            s += s_bsum[blk];
            correct += s_bcorrect[blk];
            present += (int32_t)s_bpresent[blk];
        }
        const int64_t o = m * p.nb + b;
        p.correct[o] = correct;
        p.raw[o] = (double)correct / (double)n;
        p.normalized[o] = s / (double)present; // (n >= 1: one family at least is present)
        if (m == 0) p.present[b] = present;
    }
}

extern "C" int knn_eval_bootstrap(const uint8_t *is_correct, int64_t nm, int64_t n, const int32_t *family, int32_t nfam,
                                  const int32_t *sample_ids, int64_t nb, int64_t *correct_out, int32_t *present_out,
                                  double *normalized_out, double *raw_out)
{
    if (nm < 0) return set_err(KNN_ERR_INVALID, "bootstrap: nm < 0");
    if (nb < 0) return set_err(KNN_ERR_INVALID, "bootstrap: nb < 0");
    if (n < 0) return set_err(KNN_ERR_INVALID, "bootstrap: n < 0");
    if (nm == 0 || nb == 0) return 0;
    if (n < 1) return set_err(KNN_ERR_INVALID, "bootstrap: need n >= 1");
    if (n > (int64_t)INT32_MAX) return set_err(KNN_ERR_INVALID, "bootstrap: n > INT32_MAX");
    if (nfam < 1 || nfam > KNN_BOOTSTRAP_MAX_FAMILIES)
        return set_err(KNN_ERR_INVALID, "bootstrap: nfam outside [1, KNN_BOOTSTRAP_MAX_FAMILIES]");
    if (!is_correct || !family || !sample_ids || !correct_out || !present_out || !normalized_out || !raw_out)
        return set_err(KNN_ERR_INVALID, "bootstrap: null pointer");
    for (int64_t i = 0; i < n; i++)
        if (family[i] < 0 || family[i] >= nfam) return set_err(KNN_ERR_INVALID, "bootstrap: a family value outside [0, nfam)");
    for (int64_t b = 0; b < nb; b++) {
        const int32_t *row = sample_ids + b * n;
        bool bad = false;
        for (int64_t i = 0; i < n; i++) bad |= row[i] < 0 || row[i] >= n;
        if (bad) return set_err(KNN_ERR_INVALID, "bootstrap: a sample_ids value outside [0, n)");
    }
    int rc = ensure_device(g_device);
    if (rc) return rc;
    // a row of n int32 ids is (n + 1) / 2 words of 8 bytes: the 256 MiB rule of the other entries, in their unit; at most
    // 2^20 replicates per launch (grid.x * 256 threads stays far below 2^32)
    const int64_t slab = std::min<int64_t>(std::min(nb, eval_slab_rows((n + 1) / 2)), (int64_t)1 << 20);
    const size_t lds = (size_t)nfam * 8;
    EvalBufs bufs;
    EvalCols tab(bufs, 1), w(bufs, slab);
    const uint8_t *d_ic = tab.in(is_correct, (size_t)nm * n);
    const int32_t *d_fam = tab.in(family, (size_t)n * 4);
    long long *d_cor = (long long *)tab.out(correct_out, (size_t)nm * nb * 8);
    int32_t *d_pre = tab.out(present_out, (size_t)nb * 4);
    double *d_nor = tab.out(normalized_out, (size_t)nm * nb * 8);
    double *d_raw = tab.out(raw_out, (size_t)nm * nb * 8);
    const int32_t *d_ids = w.in(sample_ids, (size_t)n * 4);
    EVAL_TRY(w.ready());
    EVAL_TRY(tab.upload(0, 1));
    HIP_TRY(hipFuncSetAttribute((const void *)bootstrap_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    for (int64_t b0 = 0; b0 < nb; b0 += slab) {
        const int64_t rows = std::min(slab, nb - b0);
        EVAL_TRY(w.upload(b0, rows));
        for (int64_t m0 = 0; m0 < nm; m0 += 65535) { // (grid.y holds 65535 at most)
            const BootstrapParams p = {d_ic, d_fam, d_ids, nb, b0, m0, (int)n, nfam, d_cor, d_pre, d_nor, d_raw};
            hipLaunchKernelGGL(bootstrap_kernel, dim3((unsigned)rows, (unsigned)std::min<int64_t>(nm - m0, 65535)), dim3(256), lds, 0, p);
            HIP_TRY(hipGetLastError());
        }
    }
    EVAL_TRY(tab.download(0, 1));
    return 0;
}
