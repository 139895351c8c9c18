// range.inc -- IndexFlat.range_search on MI355X (included by knn355_lib.hip).
//
// FAISS's other flat-index query (IndexFlat::range_search; published behaviour of FAISS 1.7.2's utils/distances.cpp
// range_search_inner_product / range_search_L2sqr and python/class_wrappers.py, restated -- FAISS is not part of the
// reference tree): every database row whose score beats a radius.  Inner product keeps score > radius, squared L2
// keeps score < radius; both comparisons are strict.  Results come query by query in ascending row order (the order
// FAISS's exhaustive scan appends in), with no cap per query.  Scores are the bits `search` returns for the same
// (query, row) pair: the same chain order, the same small-batch L2 rule (fewer than 20 queries in the batch: the sum of
// squared differences; otherwise the norm formula clamped at 0).
//
//   range_scan_kernel    one (query tile, chunk of rows) per workgroup.  A distance tile on v_mfma_f32_32x32x2_f32 fed
//                        exactly as flat_scan_kernel feeds it (LDS-DMA staging, the same swizzle and fragments), or,
//                        for squared L2 with fewer than 20 queries, one fp32 difference chain per (query, row).  The
//                        epilogue parks the tile's scores in LDS, then one wave per query walks the tile's rows in
//                        order: compare with the radius, ballot, prefix count, store.  Survivors of a workgroup are
//                        therefore in ascending row order, and so is a query's result once the chunks' runs are
//                        concatenated chunk by chunk (chunks are contiguous and ascending).
//   range_gather_kernel  copies the chunks' runs out of their staging segments into one contiguous result
//   range_pick_kernel    gathers the queries of an overflow redo (rows and norms) into a compact batch
//
// Host plan (knn_flat_range_search): queries in blocks; per block one scan in which every (query, chunk) run goes to a
// staging segment of fixed capacity and its exact count is always recorded; the host reads the counts (the result
// size must be known before the arrays exist), works out the offsets (query-major, chunk-minor exclusive scan) and the
// limits, copies the segments into place, and rescans the queries whose runs overflowed ONCE, writing straight to their
// final offsets with exact capacities.

struct RangeParams {
    const float *xb;      // [nb][dp] database rows, zero padded
    const float *yn;      // [nb] squared norms (L2, norm formula)
    const float *xq;      // [nq][dp] queries, zero padded
    const float *xn;      // [nq] squared norms (L2, norm formula)
    int64_t nb, nq;
    int dp;               // multiple of 32
    float vthr;           // keep "smaller is better" scores v < vthr (IP: v = -score, vthr = -radius)
    int nqtiles, nchunks;
    int tiles_base, tiles_rem; // chunk c walks tiles_base (+1 if c < tiles_rem) database tiles
    int nt_rows;          // one query tile: database rows are read once (non-temporal staging loads)
    int64_t segcap;       // > 0: run (q, c) goes to segment (q * nchunks + c) * segcap, at most segcap entries
    const uint64_t *offs; // segcap == 0: run (q, c) goes to offs[q * nchunks + c] ...
    const uint32_t *expect; // ... at most expect[q * nchunks + c] entries (its count in the first pass)
    uint32_t *cnt;        // [nq][nchunks] exact survivors of every (query, chunk)
    float *outD;          // scores as `search` returns them (IP: the inner product, L2: the squared distance)
    int64_t *outI;
};

template <int WM, int WN, int TM, int TN, bool L2, bool DIFF>
__global__ __launch_bounds__(256, 2) void range_scan_kernel(RangeParams p)
{
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(!DIFF || (L2 && WN == 1 && TN == 1 && WM * TM == 8), "the difference build: 256 rows x 32 queries, squared L2");
    constexpr int DT = WM * TM * 32;      // database rows per tile
    constexpr int QT = WN * TN * 32;      // queries per workgroup
    constexpr int ROWS = DT + QT;         // staged rows per K step
    constexpr int NGRP = ROWS / 8;        // staging instructions per K step (8 rows each) ...
    constexpr int NI = (NGRP + 3) / 4;    // ... per wave
    static_assert(ROWS % 8 == 0, "staging split");
    constexpr int STAGE_BYTES = ROWS * 128;
    constexpr int SS = DT + 1;            // row stride of the parked score tile (odd: a column store hits 32 banks)
    constexpr int MAIN = 2 * STAGE_BYTES > QT * SS * 4 ? 2 * STAGE_BYTES : QT * SS * 4;
    constexpr int DNQ = 20;               // chains of the difference build (it serves batches of fewer than 20 queries)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *stage0 = smem;
    char *stage1 = smem + STAGE_BYTES;
    float *sT = (float *)smem;            // [QT][SS] behind the K loop: the tile's scores, query-major
    float *s_yn = (float *)(smem + MAIN); // [DT] squared norms of the tile's rows
    uint32_t *s_cnt = (uint32_t *)(s_yn + DT); // [QT] survivors so far in this chunk

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;

    const int qtile = blockIdx.x % p.nqtiles, chunk = blockIdx.x / p.nqtiles;
    const int64_t c_lo = ((int64_t)chunk * p.tiles_base + min(chunk, p.tiles_rem)) * DT;
    const int64_t c_hi = min(p.nb, c_lo + (int64_t)(p.tiles_base + (chunk < p.tiles_rem ? 1 : 0)) * DT);
    const int64_t q0 = (int64_t)qtile * QT;
    const int nqv = (int)min((int64_t)QT, p.nq - q0);
    const int KT = p.dp / 32;
    for (int i = tid; i < QT; i += 256) s_cnt[i] = 0;

    // per-lane staging bookkeeping (flat_scan_kernel's): instruction ii covers combined rows 8 ii .. 8 ii + 7
    const float *srcp[NI];
    int lds_off[NI];
    bool is_db[NI];
    int rloc[NI];
#pragma unroll
    for (int n = 0; n < NI; n++) {
        int ii = wave + 4 * n;
        if (ii >= NGRP) ii -= 4; // (the same rows once more, to the same place: harmless)
        const int row_local = 8 * ii + (lane >> 3);
        const int sp = lane & 7;
        lds_off[n] = ii * 1024;
        if (row_local < DT) {
            is_db[n] = true;
            rloc[n] = row_local;
            srcp[n] = p.xb + 4 * (sp ^ ((row_local >> 1) & 7));
        } else {
            is_db[n] = false;
            const int rq = row_local - DT;
            rloc[n] = rq;
            srcp[n] = p.xq + min(q0 + rq, p.nq - 1) * p.dp + 4 * (sp ^ ((rq >> 1) & 7));
        }
    }
    const int swz = (li >> 1) & 7;
    float xnq[TN];
#pragma unroll
    for (int b = 0; b < TN; b++) {
        xnq[b] = 0.0f;
        if constexpr (L2 && !DIFF) xnq[b] = p.xn[min(q0 + (wn * TN + b) * 32 + li, p.nq - 1)];
    }
    __syncthreads();

    for (int64_t row0 = c_lo; row0 < c_hi; row0 += DT) {
        const float *tsrc[NI];
#pragma unroll
        for (int n = 0; n < NI; n++) tsrc[n] = is_db[n] ? srcp[n] + min(row0 + rloc[n], p.nb - 1) * p.dp : srcp[n];
        if constexpr (L2 && !DIFF) {
            if (tid < DT) s_yn[tid] = p.yn[min(row0 + tid, p.nb - 1)]; // (read behind the K loop's barriers)
        }
        f32x16 acc[TM][TN];
#pragma unroll
        for (int a = 0; a < TM; a++)
#pragma unroll
            for (int b = 0; b < TN; b++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
        float dacc[DIFF ? DNQ : 1];
#pragma unroll
        for (int j = 0; j < (DIFF ? DNQ : 1); j++) dacc[j] = 0.0f;

        auto stage = [&](int koff, char *dst) {
#pragma unroll
            for (int n = 0; n < NI; n++) {
                if (p.nt_rows && n < DT / 32) stage_issue<true>(tsrc[n] + koff, dst + lds_off[n]); // (instructions n < DT / 32 stage rows)
                else stage_issue<false>(tsrc[n] + koff, dst + lds_off[n]);
            }
        };
        stage(0, stage0);
        for (int kt = 0; kt < KT; kt++) {
            const char *cur = (kt & 1) ? stage1 : stage0;
            char *nxt = (kt & 1) ? stage0 : stage1;
            // this wave's part of stage kt has landed (explicit: nothing else orders a ds_read behind an LDS-DMA), then
            // everyone's has, and everyone is through with buffer nxt
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (kt + 1 < KT) stage((kt + 1) * 32, nxt);
            const char *A = cur;
            const char *B = cur + DT * 128;
            if constexpr (DIFF) {
                // thread = row tid of the tile; one chain per query, k in the dot product's order (0,4,1,5,2,6,3,7 per
                // block of 8): the 16-byte slots 2t and 2t + 1 hold k = 8t .. 8t + 3 and 8t + 4 .. 8t + 7
                const int fy = (tid >> 1) & 7;
                f32x4 y[8];
#pragma unroll
                for (int sl = 0; sl < 8; sl++) y[sl] = *(const f32x4 *)(A + tid * 128 + ((sl ^ fy) * 16));
#pragma unroll
                for (int j = 0; j < DNQ; j++) {
                    const char *qrow = B + j * 128; // (queries past the last one repeat it: their scores are never looked at)
                    const int fq = (j >> 1) & 7;
#pragma unroll
                    for (int t = 0; t < 4; t++) {
                        const f32x4 qa = *(const f32x4 *)(qrow + (((2 * t) ^ fq) * 16));
                        const f32x4 qb = *(const f32x4 *)(qrow + (((2 * t + 1) ^ fq) * 16));
#pragma unroll
                        for (int m = 0; m < 4; m++) {
                            const float d0 = qa[m] - y[2 * t][m];
                            dacc[j] = __builtin_fmaf(d0, d0, dacc[j]);
                            const float d1 = qb[m] - y[2 * t + 1][m];
                            dacc[j] = __builtin_fmaf(d1, d1, dacc[j]);
                        }
                    }
                }
            } else {
                // flat_scan_kernel's fragments: lane (i, h) reads slot 2t + h of its row, element m feeds k = h of the m-th
                // instruction -- each accumulator visits k = 8t + m, 8t + 4 + m for m = 0..3
#pragma unroll
                for (int t = 0; t < 4; t++) {
                    const int slot = ((2 * t + lh) ^ swz) * 16;
                    f32x4 af[TM], bf[TN];
#pragma unroll
                    for (int a = 0; a < TM; a++) af[a] = *(const f32x4 *)(A + ((wm * TM + a) * 32 + li) * 128 + slot);
#pragma unroll
                    for (int b = 0; b < TN; b++) bf[b] = *(const f32x4 *)(B + ((wn * TN + b) * 32 + li) * 128 + slot);
#pragma unroll
                    for (int m = 0; m < 4; m++)
#pragma unroll
                        for (int a = 0; a < TM; a++)
#pragma unroll
                            for (int b = 0; b < TN; b++)
                                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a][m], bf[b][m], acc[a][b], 0, 0, 0);
                }
            }
        }
        __syncthreads(); // every wave has read its last fragments: the score tile takes the staging buffers' place
        // park the scores ("smaller is better", canonical +0): sT[query][row]
        if constexpr (DIFF) {
#pragma unroll
            for (int j = 0; j < DNQ; j++) sT[j * SS + tid] = dacc[j] + 0.0f;
        } else {
#pragma unroll
            for (int a = 0; a < TM; a++)
#pragma unroll
                for (int b = 0; b < TN; b++)
#pragma unroll
                    for (int s = 0; s < 16; s++) {
                        const int r = (wm * TM + a) * 32 + 4 * lh + (s & 3) + 8 * (s >> 2);
                        const float ip = acc[a][b][s];
                        float v;
                        if constexpr (L2) {
                            v = __builtin_fmaf(-2.0f, ip, xnq[b] + s_yn[r]);
                            v = v < 0.0f ? 0.0f : v;
                        } else {
                            v = -ip;
                        }
                        sT[((wn * TN + b) * 32 + li) * SS + r] = v + 0.0f;
                    }
        }
        __syncthreads();
        // one wave per query: the tile's rows in order, 64 at a time -- compare, ballot, prefix count, store
        for (int ql = wave; ql < nqv; ql += 4) {
            uint32_t cnt = __builtin_amdgcn_readfirstlane(s_cnt[ql]);
            const int64_t cidx = (q0 + ql) * p.nchunks + chunk;
            int64_t base, lim;
            if (p.segcap > 0) {
                base = cidx * p.segcap;
                lim = p.segcap;
            } else {
                base = (int64_t)p.offs[cidx];
                lim = p.expect[cidx];
            }
#pragma unroll
            for (int r0 = 0; r0 < DT; r0 += 64) {
                const int r = r0 + lane;
                const float v = sT[ql * SS + r];
                const bool pass = row0 + r < c_hi && v < p.vthr;
                const uint64_t m = __ballot(pass);
                if (m == 0ull) continue;
                const uint32_t pre = ballot_rank(m); // (eval.inc)
                const int64_t pos = (int64_t)cnt + pre;
                if (pass && pos < lim) {
                    p.outD[base + pos] = L2 ? v : -v;
                    p.outI[base + pos] = row0 + r;
                }
                cnt += (uint32_t)__builtin_popcountll(m);
            }
            if (lane == 0) s_cnt[ql] = cnt;
        }
        __syncthreads(); // (the next tile stages into the score tile's bytes)
    }
    for (int ql = tid; ql < nqv; ql += 256) p.cnt[(q0 + ql) * p.nchunks + chunk] = s_cnt[ql];
}

// out[offs[i] ..] <- the first min(cnt, segcap) entries of segment pair0 + i; one workgroup per (query, chunk)
__global__ __launch_bounds__(256) void range_gather_kernel(const float *__restrict__ segD, const int64_t *__restrict__ segI,
                                                           const uint32_t *__restrict__ cnt, int64_t segcap, int64_t pair0,
                                                           const uint64_t *__restrict__ offs, float *__restrict__ outD,
                                                           int64_t *__restrict__ outI)
{
    const int64_t pi = pair0 + blockIdx.x;
    const int64_t n = min((int64_t)cnt[pi], segcap);
    const uint64_t o = offs[blockIdx.x];
    for (int64_t i = threadIdx.x; i < n; i += blockDim.x) {
        outD[o + i] = segD[pi * segcap + i];
        outI[o + i] = segI[pi * segcap + i];
    }
}

// dst[j] <- src[idx[j]] ([dp] rows), dstn[j] <- srcn[idx[j]] (if srcn): the queries of an overflow redo
__global__ __launch_bounds__(256) void range_pick_kernel(const float *__restrict__ src, const float *__restrict__ srcn, int dp,
                                                         const int64_t *__restrict__ idx, float *__restrict__ dst, float *__restrict__ dstn)
{
    const int64_t j = blockIdx.x, q = idx[j];
    for (int c = threadIdx.x; c < dp; c += blockDim.x) dst[j * dp + c] = src[q * dp + c];
    if (srcn && threadIdx.x == 0) dstn[j] = srcn[q];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static const int64_t KNN_RANGE_QB = 16384;                   // queries per block at most
static const size_t KNN_RANGE_OUT_BYTES = (size_t)192 << 20;   // contiguous results on the device per copy-out (at least one query's)

// one launch of a block's plan (plan_range, plan.h)
static int range_launch(knn_index_s *h, const RangeParams &p, const RangePlan &pl, hipStream_t s)
{
    const bool l2 = h->metric == KNN_METRIC_L2;
    void (*kern)(RangeParams) = nullptr;
    if (pl.diff) kern = range_scan_kernel<4, 1, 2, 1, true, true>;
    else if (pl.qt == 128) kern = l2 ? range_scan_kernel<2, 2, 2, 2, true, false> : range_scan_kernel<2, 2, 2, 2, false, false>;
    else kern = l2 ? range_scan_kernel<4, 1, 2, 1, true, false> : range_scan_kernel<4, 1, 2, 1, false, false>;
    const int rc = open_timed_launch(h, s);
    if (rc) return rc;
    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds));
    hipLaunchKernelGGL(kern, dim3(pl.grid), dim3(256), pl.lds, s, p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(h->ev1, s));
    h->last_kernel = pl.name; h->last_qt = pl.qt; h->last_dt = pl.dt; h->last_chunks = pl.nchunks; h->last_grid = pl.grid;
    return 0;
}

// elapsed time of the most recent launch (its stream has been synchronised)
static float range_launch_ms(knn_index_s *h)
{
    float ms = 0.f;
    return (h->ev0 && hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) ? ms : 0.f;
}

// Range search of nq queries: uploaded rows [nq][d] (q_host) or the index's own rows [self_row0, self_row0 + nq).
// Fills lims[nq + 1]; the results stay in h->range_D / h->range_I for knn_flat_range_fetch.  Caller holds h->mu.
static int range_search_impl(knn_index_s *h, const float *q_host, int64_t self_row0, int64_t nq, float radius, uint64_t *lims)
{
    BatchScope scope(h, nq);
    h->range_D.clear();
    h->range_I.clear();
    h->range_qblocks = 0;
    h->range_redos = 0;
    h->range_redo_queries = 0;
    h->last_ms = 0.f;
    lims[0] = 0;
    for (int64_t i = 1; i <= nq; i++) lims[i] = 0;
    if (nq == 0 || h->ntotal == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const bool l2 = h->metric == KNN_METRIC_L2;
    const PlanCtx c = plan_ctx(h);
    const int dp = h->dp;
    RangeParams p;
    memset(&p, 0, sizeof(p));
    p.xb = h->xb;
    p.yn = h->yn;
    p.nb = h->ntotal;
    p.dp = dp;
    p.vthr = l2 ? radius : -radius; // (a NaN radius stays NaN: nothing compares below it)
    std::vector<uint32_t> cnt;
    std::vector<uint64_t> offs;
    std::vector<int64_t> over;
    uint64_t done = 0; // results of the blocks before this one
    const char *oom = "range_search: out of device memory";
    for (int64_t b0 = 0; b0 < nq; b0 += KNN_RANGE_QB) {
        const int64_t m = std::min(KNN_RANGE_QB, nq - b0);
        h->range_qblocks++;
        const RangePlan pl = plan_range(c, m);
        // the block's queries on the device, zero padded to dp, and their squared norms
        const float *xq, *xn = nullptr;
        if (q_host) {
            float *rq, *rqn;
            if (!(rq = scratch<float>(h, h->ws_rq, (size_t)m * h->d, s, oom)) || !(rqn = scratch<float>(h, h->ws_rqn, (size_t)m, s, oom))) return KNN_ERR_HIP;
            HIP_TRY(hipMemcpyAsync(rq, q_host + b0 * h->d, (size_t)m * h->d * 4, hipMemcpyHostToDevice, s));
            xq = rq;
            if (dp != h->d) {
                float *padded = scratch<float>(h, h->ws_q, (size_t)m * dp, s, oom);
                if (!padded) return KNN_ERR_HIP;
                int rc = pad_rows_dev(xq, m, h->d, padded, dp, s);
                if (rc) return rc;
                xq = padded;
            }
            if (l2 && !pl.diff) {
                int rc = norms_dev_impl(xq, m, h->d, dp, rqn, s);
                if (rc) return rc;
                xn = rqn;
            }
        } else {
            xq = h->xb + (size_t)(self_row0 + b0) * dp;
            if (l2 && !pl.diff) xn = h->yn + self_row0 + b0; // (the stored norms: the same chain as norm_rows_kernel over these rows)
        }
        const int64_t pairs = m * pl.nchunks, segcap = range_segcap(pl, m);
        float *segD;
        int64_t *segI;
        uint32_t *cnt_dev;
        if (!(segD = scratch<float>(h, h->ws_rsegD, (size_t)pairs * segcap, s, oom)) || !(segI = scratch<int64_t>(h, h->ws_rsegI, (size_t)pairs * segcap, s, oom)) ||
            !(cnt_dev = scratch<uint32_t>(h, h->ws_rcnt, (size_t)pairs * 2, s, oom)))
            return KNN_ERR_HIP;
        uint32_t *cnt2_dev = cnt_dev + pairs;
        p.xq = xq;
        p.xn = xn;
        p.nq = m;
        p.nqtiles = pl.nqtiles;
        p.nchunks = pl.nchunks;
        p.tiles_base = pl.tiles_base;
        p.tiles_rem = pl.tiles_rem;
        p.nt_rows = pl.nqtiles == 1;
        p.segcap = segcap;
        p.offs = nullptr;
        p.expect = nullptr;
        p.cnt = cnt_dev;
        p.outD = segD;
        p.outI = segI;
        int rc = range_launch(h, p, pl, s);
        if (rc) return rc;
        cnt.resize((size_t)pairs);
        HIP_TRY(hipMemcpyAsync(cnt.data(), cnt_dev, (size_t)pairs * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        h->last_ms += range_launch_ms(h);
        // lims of the block; a query overflowed if any of its runs did
        for (int64_t q = 0; q < m; q++) {
            uint64_t t = 0;
            for (int c = 0; c < pl.nchunks; c++) t += cnt[(size_t)q * pl.nchunks + c];
            lims[b0 + q + 1] = lims[b0 + q] + t;
        }
        const uint64_t block_total = lims[b0 + m] - done;
        h->range_D.resize((size_t)(done + block_total));
        h->range_I.resize((size_t)(done + block_total));
        // copy-out in runs of whole queries that fit the output buffer (one query at least: ntotal entries at most)
        const size_t out_cap = std::max<size_t>(KNN_RANGE_OUT_BYTES / 12, (size_t)h->ntotal);
        float *outD;
        int64_t *outI, *sel;
        uint64_t *offs_dev;
        if (!(outD = scratch<float>(h, h->ws_routD, out_cap, s, oom)) || !(outI = scratch<int64_t>(h, h->ws_routI, out_cap, s, oom)) ||
            !(offs_dev = scratch<uint64_t>(h, h->ws_roff, (size_t)pairs * 2, s, oom)) || !(sel = scratch<int64_t>(h, h->ws_rsel, (size_t)m, s, oom)))
            return KNN_ERR_HIP;
        for (int64_t qa = 0; qa < m;) {
            int64_t qb = qa + 1;
            while (qb < m && lims[b0 + qb + 1] - lims[b0 + qa] <= out_cap) qb++;
            const uint64_t run0 = lims[b0 + qa], run_n = lims[b0 + qb] - run0;
            if (run_n == 0) {
                qa = qb;
                continue;
            }
            offs.resize((size_t)(qb - qa) * pl.nchunks);
            over.clear();
            uint64_t o = 0;
            for (int64_t q = qa; q < qb; q++) {
                bool ov = false;
                for (int c = 0; c < pl.nchunks; c++) {
                    const uint32_t n = cnt[(size_t)q * pl.nchunks + c];
                    offs[(size_t)(q - qa) * pl.nchunks + c] = o;
                    o += n;
                    ov |= (int64_t)n > segcap;
                }
                if (ov) over.push_back(q);
            }
            HIP_TRY(hipMemcpyAsync(offs_dev, offs.data(), offs.size() * 8, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(range_gather_kernel, dim3((unsigned)((qb - qa) * pl.nchunks)), dim3(64), 0, s, (const float *)segD,
                               (const int64_t *)segI, (const uint32_t *)cnt_dev, segcap, qa * pl.nchunks, (const uint64_t *)offs_dev, outD, outI);
            HIP_TRY(hipGetLastError());
            if (!over.empty()) {
                // ONE rescan of the queries whose runs overflowed, same tile and chunks, straight to their final offsets with
                // the exact capacities of the first pass
                const int64_t no = (int64_t)over.size();
                h->range_redos++;
                h->range_redo_queries += no;
                std::vector<uint64_t> offs2((size_t)no * pl.nchunks);
                std::vector<uint32_t> exp2((size_t)no * pl.nchunks);
                for (int64_t j = 0; j < no; j++)
                    for (int c = 0; c < pl.nchunks; c++) {
                        offs2[(size_t)j * pl.nchunks + c] = offs[(size_t)(over[j] - qa) * pl.nchunks + c];
                        exp2[(size_t)j * pl.nchunks + c] = cnt[(size_t)over[j] * pl.nchunks + c];
                    }
                float *q2;
                uint32_t *expect;
                if (!(q2 = scratch<float>(h, h->ws_rq2, (size_t)no * dp + (size_t)no, s, oom)) || !(expect = scratch<uint32_t>(h, h->ws_rexp, (size_t)no * pl.nchunks, s, oom)))
                    return KNN_ERR_HIP;
                uint64_t *offs2_dev = offs_dev + offs.size();
                HIP_TRY(hipMemcpyAsync(offs2_dev, offs2.data(), offs2.size() * 8, hipMemcpyHostToDevice, s));
                HIP_TRY(hipMemcpyAsync(expect, exp2.data(), exp2.size() * 4, hipMemcpyHostToDevice, s));
                HIP_TRY(hipMemcpyAsync(sel, over.data(), (size_t)no * 8, hipMemcpyHostToDevice, s));
                float *qn2 = q2 + (size_t)no * dp;
                hipLaunchKernelGGL(range_pick_kernel, dim3((unsigned)no), dim3(256), 0, s, xq, xn, dp, (const int64_t *)sel, q2,
                                   xn ? qn2 : nullptr);
                HIP_TRY(hipGetLastError());
                RangeParams p2 = p;
                RangePlan pl2 = pl;
                pl2.nqtiles = (int)((no + pl.qt - 1) / pl.qt);
                pl2.grid = pl2.nqtiles * pl.nchunks;
                p2.xq = q2;
                p2.xn = xn ? qn2 : nullptr;
                p2.nq = no;
                p2.nqtiles = pl2.nqtiles;
                p2.nt_rows = pl2.nqtiles == 1;
                p2.segcap = 0;
                p2.offs = offs2_dev;
                p2.expect = expect;
                p2.cnt = cnt2_dev;
                p2.outD = outD;
                p2.outI = outI;
                rc = range_launch(h, p2, pl2, s);
                if (rc) return rc;
                std::vector<uint32_t> cnt2((size_t)no * pl.nchunks);
                HIP_TRY(hipMemcpyAsync(cnt2.data(), cnt2_dev, cnt2.size() * 4, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                h->last_ms += range_launch_ms(h);
                if (cnt2 != exp2) return set_err(KNN_ERR_HIP, "range_search: the overflow rescan counted differently from the first pass");
            }
            HIP_TRY(hipMemcpyAsync(h->range_D.data() + run0, outD, run_n * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(h->range_I.data() + run0, outI, run_n * 8, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            qa = qb;
        }
        done += block_total;
    }
    if (h->done) (void)hipEventRecord(h->done, s);
    return 0;
}

static int check_range_args(knn_index_s *h, const void *q, int64_t nq, const uint64_t *lims)
{
    if (!h) return set_err(KNN_ERR_INVALID, "range_search: null handle");
    if (nq < 0) return set_err(KNN_ERR_INVALID, "range_search: negative nq");
    if (!lims || (nq > 0 && !q)) return set_err(KNN_ERR_INVALID, "range_search: null pointer");
    if (view_is_stale(h)) return set_err(KNN_ERR_INVALID, "range_search" KNN_STALE_VIEW_MSG);
    if (h->approx16) return set_err(KNN_ERR_UNSUPPORTED, "range_search: not for an approximate (bf16) index"); // (the range scan has no bf16 build)
    return 0;
}

extern "C" int knn_flat_range_search(knn_handle h, const float *q_host, int64_t nq, float radius, uint64_t *lims_host)
{
    int rc = check_range_args(h, q_host, nq, lims_host);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    return range_search_impl(h, q_host, 0, nq, radius, lims_host);
}

extern "C" int knn_flat_range_search_self(knn_handle h, int64_t row0, int64_t nrows, float radius, uint64_t *lims_host)
{
    int rc = check_range_args(h, lims_host, nrows, lims_host);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (row0 < 0 || row0 + nrows > h->ntotal) return set_err(KNN_ERR_INVALID, "range_search_self: row range out of bounds");
    return range_search_impl(h, nullptr, row0, nrows, radius, lims_host);
}

extern "C" int knn_flat_range_fetch(knn_handle h, float *D_host, int64_t *I_host)
{
    if (!h) return set_err(KNN_ERR_INVALID, "range_fetch: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    const size_t n = h->range_D.size();
    if (n && (!D_host || !I_host)) return set_err(KNN_ERR_INVALID, "range_fetch: null pointer");
    if (n) {
        memcpy(D_host, h->range_D.data(), n * 4);
        memcpy(I_host, h->range_I.data(), n * 8);
    }
    std::vector<float>().swap(h->range_D);
    std::vector<int64_t>().swap(h->range_I);
    return 0;
}

extern "C" int knn_last_range_info(knn_handle h, int64_t *query_blocks, int64_t *redos, int64_t *redo_queries)
{
    if (!h) return set_err(KNN_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (query_blocks) *query_blocks = h->range_qblocks;
    if (redos) *redos = h->range_redos;
    if (redo_queries) *redo_queries = h->range_redo_queries;
    return 0;
}
