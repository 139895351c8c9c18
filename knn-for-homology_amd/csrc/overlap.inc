// overlap.inc -- two hit lists compared as sets of ids, query by query (included by knn355_lib.hip behind fuse.inc).
//
// pfam/pfam.py counts, per query, how the true-positive ids of two searches overlap ("TP Set overlap", lines 349-370) and
// how many distinct ids the two lists return together before their first wrong hit (auc1s_optimal, lines 602-625), in
// Python loops over `set` objects.  Here both are one workgroup of 256 threads per query row over two lists A [ka] and
// B [kb] of (int64 id, uint8 flag); the contract is above knn_eval_overlap in include/knn355.h.  Integers only: no float
// instruction, no atomic, and no loop whose length depends on the data except the early end of stage 3.
//
//   stage 1  slots.  Entry p (A's column p, or B's column p - ka) fills slot p of next_pow2(ka + kb): the key is the id
//            as uint64 (an existing id is below 2^63, so KEY_PAD marks a slot without an entry), the payload holds
//            OV_TA / OV_TB when the entry's flag is non-zero.  In the same read every thread keeps the lowest column
//            of each list that exists with a zero flag; a minimum over the workgroup gives the two lead lengths.
//   stage 2  the slots of existing entries in front of their list's lead length get OV_LA / OV_LB (before the sort:
//            slot p still is position p).
//   stage 3  wg_bitonic_sort_pairs: equal ids become neighbours.  Then the payloads of a run of equal keys are OR-ed
//            towards its head by doubling: step d gives slot i the payload of slot i + d when their keys are equal
//            (the run is contiguous, so everything between them is the same id); after the steps 1, 2, .. d a slot
//            holds the OR of [i, i + 2d) of its run.  The steps end at d >= ka + kb, or as soon as no slot of the row
//            finds its key at distance d: no run is longer than d then, and the steps before have covered it.  At
//            most 12 steps, 2 on rows whose ids repeat once.
//   stage 4  a slot is a run head when it holds an entry and its left neighbour another key.  Every thread counts its
//            heads into the six classes (TA only, both, TB only; LA only, both, LB only); the counts are added across
//            the wave by shuffles and across the four waves through LDS.
//
// LDS: 128 bytes of counters, 8 P bytes of keys, 2 P of payloads: 40 KB + 128 at ka + kb = 4096.

struct OverlapParams {
    const int64_t *ha, *hb; // the slab's rows [rows][ka], [rows][kb]
    const uint8_t *ca, *cb; // their flags
    int ka, kb, P;          // P: slots of the sort
    int32_t *tp, *lead;     // [rows][3] each, or null
};

#define OV_TA 1u
#define OV_TB 2u
#define OV_LA 4u
#define OV_LB 8u

__global__ __launch_bounds__(256) void overlap_kernel(OverlapParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    int(*s_wcnt)[4] = (int(*)[4])smem;          // [2][4]
    int(*s_red)[6] = (int(*)[6])(smem + 32);    // [4][6]
    uint64_t *s_key = (uint64_t *)(smem + 128); // [P]
    uint16_t *s_pay = (uint16_t *)(s_key + p.P); // [P]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t q = blockIdx.x;
    const int ka = p.ka, kb = p.kb, n = ka + kb, P = p.P;
    const int64_t *ha = p.ha + q * ka, *hb = p.hb + q * kb;
    const uint8_t *ca = p.ca + q * ka, *cb = p.cb + q * kb;
    int par = 0;

    // ---- stage 1 ----
    int bad_a = ka, bad_b = kb; // this thread's columns ascend: the first one found is its lowest
    for (int i = tid; i < P; i += 256) {
        uint64_t key = KEY_PAD;
        uint16_t pay = 0;
        if (i < n) {
            const bool in_a = i < ka;
            const int col = in_a ? i : i - ka;
            const int64_t h = in_a ? ha[col] : hb[col];
            if (h >= 0) {
                key = (uint64_t)h;
                if ((in_a ? ca[col] : cb[col]) != 0) pay = in_a ? OV_TA : OV_TB;
                else if (in_a) bad_a = min(bad_a, col);
                else bad_b = min(bad_b, col);
            }
        }
        s_key[i] = key;
        s_pay[i] = pay;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        bad_a = min(bad_a, __shfl_xor(bad_a, off, 64));
        bad_b = min(bad_b, __shfl_xor(bad_b, off, 64));
    }
    if (lane == 0) {
        s_red[wave][0] = bad_a;
        s_red[wave][1] = bad_b;
    }
    __syncthreads();
    const int lead_a = min(min(s_red[0][0], s_red[1][0]), min(s_red[2][0], s_red[3][0]));
    const int lead_b = min(min(s_red[0][1], s_red[1][1]), min(s_red[2][1], s_red[3][1]));
    // ---- stage 2 ---- (every slot in front of a lead length that holds an entry has its flag set)
    for (int i = tid; i < n; i += 256)
        if (s_key[i] != KEY_PAD) {
            if (i < lead_a) s_pay[i] |= OV_LA;
            else if (i >= ka && i - ka < lead_b) s_pay[i] |= OV_LB;
        }
    __syncthreads();
    // ---- stage 3 ----
    wg_bitonic_sort_pairs(s_key, s_pay, P, tid, 256);
    for (int d = 1; d < n; d <<= 1) {
        uint16_t add[KNN_MAX_K * 2 / 256];
        bool found = false;
#pragma unroll
        for (int t = 0; t < KNN_MAX_K * 2 / 256; t++) {
            const int i = tid + 256 * t;
            add[t] = 0;
            if (i + d < P) {
                const uint64_t key = s_key[i];
                if (key != KEY_PAD && s_key[i + d] == key) {
                    add[t] = s_pay[i + d];
                    found = true;
                }
            }
        }
        int tot;
        (void)wg_compact(found, s_wcnt, par, &tot); // its barrier: every read of this step is done
        if (tot == 0) break;                        // (the same for every thread)
#pragma unroll
        for (int t = 0; t < KNN_MAX_K * 2 / 256; t++)
            if (add[t]) s_pay[tid + 256 * t] |= add[t];
        __syncthreads();
    }
    // ---- stage 4 ----
    int cnt[6] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < P; i += 256) {
        const uint64_t key = s_key[i];
        if (key == KEY_PAD || (i > 0 && s_key[i - 1] == key)) continue;
        const unsigned v = s_pay[i], t = v & 3u, l = v >> 2;
        cnt[0] += t == 1u;
        cnt[1] += t == 3u;
        cnt[2] += t == 2u;
        cnt[3] += l == 1u;
        cnt[4] += l == 3u;
        cnt[5] += l == 2u;
    }
#pragma unroll
    for (int c = 0; c < 6; c++) { // (s_red was last read in front of the sort's barriers)
        for (int off = 32; off >= 1; off >>= 1) cnt[c] += __shfl_xor(cnt[c], off, 64);
        if (lane == 0) s_red[wave][c] = cnt[c];
    }
    __syncthreads();
    if (tid < 6) {
        const int v = s_red[0][tid] + s_red[1][tid] + s_red[2][tid] + s_red[3][tid];
        if (tid < 3) {
            if (p.tp) p.tp[q * 3 + tid] = v;
        } else if (p.lead) {
            p.lead[q * 3 + tid - 3] = v;
        }
    }
}

// the phases of this thread's last successful knn_eval_overlap
enum { OVERLAP_UP, OVERLAP_KERNEL, OVERLAP_DOWN, OVERLAP_PHASES };
static thread_local float g_overlap_ms[OVERLAP_PHASES] = {0, 0, 0};

extern "C" int knn_eval_overlap(const int64_t *hits_a, const uint8_t *correct_a, int64_t ka, const int64_t *hits_b,
                                const uint8_t *correct_b, int64_t kb, int64_t nq, int32_t *tp_out, int32_t *lead_out)
{
    if (nq < 0) return set_err(KNN_ERR_INVALID, "overlap: negative nq");
    if (ka < 1 || ka > KNN_MAX_K) return set_err(KNN_ERR_INVALID, "overlap: ka outside [1, KNN_MAX_K]");
    if (kb < 1 || kb > KNN_MAX_K) return set_err(KNN_ERR_INVALID, "overlap: kb outside [1, KNN_MAX_K]");
    if (nq == 0) return 0;
    if (!hits_a) return set_err(KNN_ERR_INVALID, "overlap: null hits_a");
    if (!correct_a) return set_err(KNN_ERR_INVALID, "overlap: null correct_a");
    if (!hits_b) return set_err(KNN_ERR_INVALID, "overlap: null hits_b");
    if (!correct_b) return set_err(KNN_ERR_INVALID, "overlap: null correct_b");
    if (!tp_out && !lead_out) return set_err(KNN_ERR_INVALID, "overlap: tp_out and lead_out are both null");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    const int n = (int)(ka + kb);
    const int64_t slab = std::min(nq, eval_slab_rows(n));
    const int P = next_pow2_host(n);
    const size_t lds = 128 + (size_t)P * (8 + 2);
    HIP_TRY(hipFuncSetAttribute((const void *)overlap_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HostCall call;
    EvalBufs &bufs = call.bufs;
    PhaseClock &clock = call.clock;
    EvalCols w(bufs, slab);
    const OverlapParams p = {w.in(hits_a, (size_t)ka * 8),
                             w.in(hits_b, (size_t)kb * 8),
                             w.in(correct_a, (size_t)ka),
                             w.in(correct_b, (size_t)kb),
                             (int)ka, (int)kb, P,
                             w.out(tp_out, 12),
                             w.out(lead_out, 12)};
    EVAL_TRY(w.ready());
    for (int64_t r0 = 0; r0 < nq; r0 += slab) {
        const int64_t m = std::min(slab, nq - r0);
        EVAL_TRY(clock.next(OVERLAP_UP, call.s));
        EVAL_TRY(w.upload(r0, m));
        EVAL_TRY(clock.next(OVERLAP_KERNEL, call.s));
        hipLaunchKernelGGL(overlap_kernel, dim3((unsigned)m), dim3(256), lds, call.s, p);
        HIP_TRY(hipGetLastError());
        EVAL_TRY(clock.next(OVERLAP_DOWN, call.s));
        EVAL_TRY(w.download(r0, m));
    }
    EVAL_TRY(clock.close(call.s));
    EVAL_TRY(call.finish("overlap", 0));
    float ms[OVERLAP_PHASES];
    EVAL_TRY(clock.read(ms, OVERLAP_PHASES));
    memcpy(g_overlap_ms, ms, sizeof ms);
    return 0;
}

extern "C" int knn_eval_overlap_last_ms(float *ms)
{
    if (!ms) return set_err(KNN_ERR_INVALID, "overlap_last_ms: null pointer");
    for (int i = 0; i < OVERLAP_PHASES; i++) ms[i] = g_overlap_ms[i];
    return 0;
}
