// refine.inc -- faiss.IndexRefineFlat on MI355X: exact re-scoring of a base index's candidates (included by knn355_lib.hip).
//
// FAISS 1.7.2's IndexRefineFlat (not in the reference tree; published behaviour restated): search the base index for
// k * k_factor labels per query, IndexFlat::compute_distance_subset scores exactly those rows against the stored fp32
// vectors (fvec_inner_product / fvec_L2sqr per pair), reorder_2_heaps keeps the best k.  The reference uses its LSH index
// as such a shortlist (seqvec_search/main.py:132, pfam/search.py:27-51).
//
//   refine_rescore_kernel  one workgroup per (query, slice of up to 256 candidates): the slice's rows are gathered into
//                          LDS in slabs of 32 floats, then every lane runs the contract's fp32 chain of ITS candidate
//                          out of LDS.  Output: packed keys [nq][kb] for select_topk_kernel.
//
// Arithmetic, per (query, candidate): one sequential chain over k in blocks of 8, order 0,4,1,5,2,6,3,7 (the order of
// pair_distance_kernel and of the oracle).  Inner product: acc = fmaf(q, y, acc), key value -acc + 0.0f.  L2: t = q - y,
// acc = fmaf(t, t, acc) at every batch size (fvec_L2sqr: FAISS never takes the norm formula for a subset).
//
// Memory: a gather of nq * kb rows of dp * 4 bytes.  A slab is 128 bytes of each of the 256 rows: eight lanes fetch one
// row's piece as one full 128-byte line (16 bytes per lane), eight such loads per lane cover the slice, and they stay in
// flight in registers while the chain of the previous slab runs out of the other LDS buffer (plain loads + ds_write_b128:
// a direct-to-LDS load writes 1 KiB contiguously per wave instruction, which a padded 144-byte row cannot take).  The
// query's 128 bytes of the slab ride along as row 256, so d is not bounded by the LDS.  Row pitch 36 dwords: the 16 lanes
// of a ds_read_b128 group read the same k of 16 different rows at 36 r + k, and 36 r mod 64 = 4 (9 r mod 16) is a
// different 16-byte slot for each of 16 consecutive rows (every group's rows are distinct mod 16): no bank conflict; the
// ds_write_b128 groups (8 lanes = one row's 128 bytes) touch 32 different banks.  Two buffers of 257 x 144 bytes + the
// slice's labels = 76 KB: two workgroups per CU, 64 KB of row fetches in flight per CU.

struct RefineParams {
    const float *xb; // [nb][dp] the flat index's rows
    int64_t nb;
    int dp;
    const float *xq;       // [nq][dp]
    const int64_t *labels; // [nq][kb], -1: no candidate
    int kb;
    uint64_t *keys; // [nq][kb]
};

static constexpr int RF_ROWS = 256, RF_KS = 32, RF_PITCH = 36; // rows per slice, floats per slab, LDS row pitch in floats
static constexpr size_t RF_LDS = (size_t)2 * (RF_ROWS + 1) * RF_PITCH * 4 + RF_ROWS * 8;

template <bool L2>
__global__ __launch_bounds__(256, 2) void refine_rescore_kernel(RefineParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float *stage = (float *)smem;                                                  // [2][257][36]
    int64_t *s_row = (int64_t *)(smem + (size_t)2 * (RF_ROWS + 1) * RF_PITCH * 4); // [256] the slice's row ids
    const int tid = threadIdx.x;
    const int nsl = (p.kb + RF_ROWS - 1) / RF_ROWS;
    const int64_t q = blockIdx.x / nsl;
    const int j = (blockIdx.x % nsl) * RF_ROWS + tid; // this lane's candidate
    int64_t lab = -1;
    if (j < p.kb) lab = p.labels[(size_t)q * p.kb + j];
    if (lab < 0 || lab >= p.nb) lab = -1; // (the host entries check their labels: nothing is ever read out of bounds)
    s_row[tid] = lab;
    __syncthreads();
    // fetch pass i: row i * 32 + tid / 8, 16-byte piece tid % 8 of the slab.  A slot without a candidate reads row 0 (a
    // line every such slot shares: L2 hits); its key is KEY_PAD whatever the chain gives.
    const int piece = tid & 7, r0 = tid >> 3;
    const float *src[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int64_t r = s_row[i * 32 + r0];
        src[i] = p.xb + (size_t)(r < 0 ? 0 : r) * p.dp + piece * 4;
    }
    const float *qsrc = p.xq + (size_t)q * p.dp + piece * 4;
    f32x4 v[8], vq;
    const int KT = p.dp / RF_KS;
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = *(const f32x4 *)src[i];
    vq = *(const f32x4 *)qsrc;
    float acc = 0.0f;
    for (int ks = 0; ks < KT; ks++) {
        float *buf = stage + (ks & 1) * (RF_ROWS + 1) * RF_PITCH;
#pragma unroll
        for (int i = 0; i < 8; i++) *(f32x4 *)(buf + (i * 32 + r0) * RF_PITCH + piece * 4) = v[i];
        if (tid < 8) *(f32x4 *)(buf + RF_ROWS * RF_PITCH + piece * 4) = vq;
        // one barrier per slab: the buffer written here was last read two slabs ago, in front of the previous barrier
        __syncthreads();
        if (ks + 1 < KT) {
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = *(const f32x4 *)(src[i] + (ks + 1) * RF_KS);
            vq = *(const f32x4 *)(qsrc + (ks + 1) * RF_KS);
        }
        const float *y = buf + tid * RF_PITCH, *qq = buf + RF_ROWS * RF_PITCH;
#pragma unroll
        for (int k0 = 0; k0 < RF_KS; k0 += 8) {
            const f32x4 q0 = *(const f32x4 *)(qq + k0), q1 = *(const f32x4 *)(qq + k0 + 4);
            const f32x4 y0 = *(const f32x4 *)(y + k0), y1 = *(const f32x4 *)(y + k0 + 4);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                if (L2) {
                    const float t0 = q0[m] - y0[m];
                    acc = __builtin_fmaf(t0, t0, acc);
                    const float t1 = q1[m] - y1[m];
                    acc = __builtin_fmaf(t1, t1, acc);
                } else {
                    acc = __builtin_fmaf(q0[m], y0[m], acc);
                    acc = __builtin_fmaf(q1[m], y1[m], acc);
                }
            }
        }
    }
    if (j < p.kb) {
        uint64_t key = KEY_PAD;
        const float val = L2 ? acc + 0.0f : -acc + 0.0f;
        if (lab >= 0 && val < INFINITY) key = ((uint64_t)f2ord(val) << 32) | (uint32_t)lab; // (NaN / "worse than everything" never becomes a hit)
        p.keys[(size_t)q * p.kb + j] = key;
    }
}

// ---- host -------------------------------------------------------------------------------
// the phases of knn_index_s::refine_ms: the rescore launch and the selection of every batch (refine_batch)
enum { REFINE_RESCORE, REFINE_SELECT, REFINE_PHASES };

// after the stream has drained: the clock of a call's refine_batches into flat->refine_ms
static int refine_commit_ms(const PhaseClock &clock, knn_index_s *flat)
{
    float ms[REFINE_PHASES];
    EVAL_TRY(clock.read(ms, REFINE_PHASES));
    memcpy(flat->refine_ms, ms, sizeof ms);
    return 0;
}

// the candidates labels_dev [m][kb] of the padded queries xq_dev [m][dp] (both on the device) -> the best k of each
// query in D_dev / I_dev [m][k], on stream s.  The caller holds flat->mu and has checked the labels' range or got them
// from a search over the same number of rows.
static int refine_batch(knn_index_s *flat, const float *xq_dev, const int64_t *labels_dev, int64_t m, int kb, int k, float *D_dev,
                        int64_t *I_dev, hipStream_t s, PhaseClock &clock)
{
    RefineParams p;
    if (!(p.keys = scratch<uint64_t>(flat, flat->ws_rfkeys, (size_t)m * kb, s, "refine: out of device memory"))) return KNN_ERR_HIP;
    p.xb = flat->xb; p.nb = flat->ntotal; p.dp = flat->dp;
    p.xq = xq_dev; p.labels = labels_dev; p.kb = kb;
    const unsigned grid = (unsigned)(m * ((kb + RF_ROWS - 1) / RF_ROWS));
    void (*kern)(RefineParams) = flat->metric == KNN_METRIC_L2 ? refine_rescore_kernel<true> : refine_rescore_kernel<false>;
    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)RF_LDS));
    EVAL_TRY(clock.open(REFINE_RESCORE, s));
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), RF_LDS, s, p);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(clock.next(REFINE_SELECT, s));
    SelectParams sp = {};
    sp.in = p.keys; sp.in_stride = kb; sp.n_fixed = kb; sp.cap = kb;
    sp.nq = m; sp.k = k; sp.metric = flat->metric;
    sp.D = D_dev; sp.I = I_dev;
    EVAL_TRY(launch_select(sp, s));
    return clock.close(s);
}

static int refine_check_shape(int64_t nq, int64_t kb, int64_t k, const char *who)
{
    if (nq < 0 || k < 1 || kb < k) return set_err(KNN_ERR_INVALID, std::string(who) + ": need nq >= 0 and 1 <= k <= kb");
    if (kb > KNN_MAX_K) return set_err(KNN_ERR_UNSUPPORTED, std::string(who) + ": more than 2048 candidates per query are not supported");
    return 0;
}

static int refine_check_flat(knn_index_s *flat, const char *who)
{
    if (flat->approx16) return set_err(KNN_ERR_UNSUPPORTED, std::string(who) + ": not for an approximate (bf16) index");
    if (view_is_stale(flat)) return set_err(KNN_ERR_INVALID, std::string(who) + KNN_STALE_VIEW_MSG);
    return 0;
}

// IndexFlat::compute_distance_subset + reorder_2_heaps (IndexRefineFlat::search behind the base index's search)
extern "C" int knn_flat_refine(knn_handle h, const float *q_host, int64_t nq, const int64_t *labels_host, int64_t kb, int64_t k, float *D_host,
                               int64_t *I_host)
{
    if (!h) return set_err(KNN_ERR_INVALID, "flat_refine: null handle");
    int rc = refine_check_shape(nq, kb, k, "flat_refine");
    if (rc) return rc;
    if (nq == 0) return 0;
    if (!q_host || !labels_host || !D_host || !I_host) return set_err(KNN_ERR_INVALID, "flat_refine: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    if ((rc = refine_check_flat(h, "flat_refine"))) return rc;
    for (int64_t i = 0; i < nq * kb; i++)
        if (labels_host[i] < -1 || labels_host[i] >= h->ntotal)
            return set_err(KNN_ERR_INVALID, "flat_refine: label " + std::to_string(labels_host[i]) + " of query " + std::to_string(i / kb) +
                                                " is outside the index (" + std::to_string(h->ntotal) + " rows)");
    if (h->ntotal == 0) {
        fill_empty_host(D_host, I_host, nq * k, h->metric);
        return 0;
    }
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int64_t QB = 16384;
    const int64_t mb = std::min(QB, nq);
    const char *oom = "flat_refine: out of device memory";
    float *q_dev, *qp_dev = nullptr, *D_dev; // (qp_dev: the padded copy, where one is needed)
    int64_t *lab_dev, *I_dev;
    if (!(q_dev = scratch<float>(h, h->ws_rfq, (size_t)mb * h->d, s, oom)) || (h->dp != h->d && !(qp_dev = scratch<float>(h, h->ws_rfqp, (size_t)mb * h->dp, s, oom))) ||
        !(lab_dev = scratch<int64_t>(h, h->ws_rfI, (size_t)mb * kb, s, oom)) || !(D_dev = scratch<float>(h, h->ws_rfD, (size_t)mb * k, s, oom)) ||
        !(I_dev = scratch<int64_t>(h, h->ws_rfI2, (size_t)mb * k, s, oom)))
        return KNN_ERR_HIP;
    PhaseClock clock;
    for (int64_t b0 = 0; b0 < nq; b0 += QB) {
        const int64_t m = std::min(QB, nq - b0);
        HIP_TRY(hipMemcpyAsync(q_dev, q_host + b0 * h->d, (size_t)m * h->d * 4, hipMemcpyHostToDevice, s));
        if (h->dp != h->d && (rc = pad_rows_dev(q_dev, m, h->d, qp_dev, h->dp, s))) return rc;
        HIP_TRY(hipMemcpyAsync(lab_dev, labels_host + b0 * kb, (size_t)m * kb * 8, hipMemcpyHostToDevice, s));
        rc = refine_batch(h, qp_dev ? qp_dev : q_dev, lab_dev, m, (int)kb, (int)k, D_dev, I_dev, s, clock);
        if (rc) {
            (void)hipStreamSynchronize(s); // (nothing of this batch is left running behind the error)
            return rc;
        }
        HIP_TRY(hipMemcpyAsync(D_host + b0 * k, D_dev, (size_t)m * k * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(I_host + b0 * k, I_dev, (size_t)m * k * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return refine_commit_ms(clock, h);
}

// measurement (tools/refine_probe.py): HIP-event milliseconds of the last successful knn_flat_refine /
// knn_lsh_search_refine on this flat handle, summed over its batches
extern "C" int knn_last_refine_ms(knn_handle h, float *rescore_ms, float *select_ms)
{
    if (!h || !rescore_ms || !select_ms) return set_err(KNN_ERR_INVALID, "last_refine_ms: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    *rescore_ms = h->refine_ms[0];
    *select_ms = h->refine_ms[1];
    return 0;
}
