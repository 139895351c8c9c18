// flat_search.inc -- the flat search's host side (included by knn355_lib.hip behind flat_index.inc): launch_select, the
// choice of a flat_scan_kernel build for a plan of plan.h, search_view and its callers, the device entries,
// knn_merge_keys_dev, the symmetric self-search, host_search and the host entries.

// one workgroup per query: best k of its candidate keys (see select_topk_kernel).  tmp: scratch for the segment
// pass of arrays longer than one workgroup's registers hold.
static const int KNN_SELECT_SEG = 32768;
static int launch_select(SelectParams sp, hipStream_t s, DevBuf *tmp = nullptr)
{
    if (sp.nq <= 0) return 0;
    // (an array whose CAPACITY is larger but which is expected to hold far fewer keys -- the compact arrays of an
    // exactly seeded scan are sized for the worst case of every chunk -- goes straight to the one-launch selection:
    // 32768 keys fit its registers, a longer array is re-read from L2 on every probe)
    const bool expect_short = sp.n_expect > 0 && sp.n_expect <= 24576;
    if (tmp && sp.lm_lists == 0 && sp.cnt && sp.cap > KNN_SELECT_SEG && !expect_short) {
        // Arrays of up to `cap` > 32768 keys (a seed sample of a 10 M-row database hands on 39 k scores per
        // query): workgroup (q, s) reduces segment s of query q to its kk = kmax best keys in registers, then
        // one more launch selects among the nseg * kk survivors -- two launches instead of re-reading the
        // array from L2 on every probe.
        const int kk = sp.k + std::max(sp.k >> 2, 32);
        const int nseg = (sp.cap + KNN_SELECT_SEG - 1) / KNN_SELECT_SEG;
        uint64_t *part = scratch_device_wide<uint64_t>(*tmp, (size_t)sp.nq * nseg * kk);
        if (!part) return KNN_ERR_HIP;
        SelectParams a = {};
        a.in = sp.in; a.in_stride = sp.in_stride; a.cnt = sp.cnt; a.cap = sp.cap;
        a.seg_len = KNN_SELECT_SEG; a.nseg = nseg;
        a.nq = sp.nq; a.k = kk; a.metric = sp.metric;
        a.out_keys = part; a.out_stride = kk; a.out_fill = 0;
        a.gate = sp.gate; a.gate_n = sp.gate_n;
        const size_t lds = (size_t)next_pow2_host(kk + std::max(kk >> 2, 32)) * 8;
        hipLaunchKernelGGL((select_topk_kernel<32, 1024, false>), dim3((unsigned)sp.nq, (unsigned)nseg), dim3(1024), lds, s, a);
        HIP_TRY(hipGetLastError());
        sp.in = part;
        sp.in_stride = (int64_t)nseg * kk;
        sp.cnt = nullptr;
        sp.n_fixed = nseg * kk;
        sp.cap = nseg * kk;
        sp.n_expect = 0;
    }
    const bool seed = sp.seed_cnt != nullptr;
    const int kmax = sp.k + std::max(sp.k >> 2, 32);
    const size_t lds = seed ? 0 : (size_t)next_pow2_host(kmax) * 8;
    const int nmax = sp.lm_lists > 0 ? sp.lm_lists * sp.lm_k : (sp.cnt ? sp.cap : sp.n_fixed);
    void (*kern)(SelectParams);
    int nt = 256;
    // Many queries with short candidate arrays (the batch regime): ONE WAVE per query -- four times the queries
    // in flight per CU, and the kernel is bound by the latency of its dependent loads, not by arithmetic
    // (14433 queries x ~1400 keys: 265 us with a workgroup per query).  Few queries with long arrays (the
    // streaming regime): a workgroup per query, up to 32768 keys in registers.  Arrays longer than the
    // registers of the chosen build hold are re-read from L2 on every probe.
    const int nexp = sp.n_expect > 0 ? std::min(sp.n_expect, nmax) : nmax;
    if (sp.nq >= 512 && nexp <= 64 * 32) {
        nt = 64;
        if (seed) kern = nexp <= 64 * 8 ? select_topk_kernel<8, 64, true> : select_topk_kernel<32, 64, true>;
        else kern = nexp <= 64 * 8 ? select_topk_kernel<8, 64, false> : select_topk_kernel<32, 64, false>;
    } else if (seed) {
        if (nmax <= 256 * 4) kern = select_topk_kernel<4, 256, true>;
        else if (nmax <= 256 * 16) kern = select_topk_kernel<16, 256, true>;
        else if (nmax <= 256 * 32) kern = select_topk_kernel<32, 256, true>;
        else { kern = select_topk_kernel<32, 1024, true>; nt = 1024; }
    } else {
        // (by the EXPECTED count when the arrays carry their own: the compact arrays of a seeded scan are sized for the worst
        // case of every chunk -- 64 k slots per query on a 1.25 M-row shard -- and hold 1-2 k keys; the 1024-thread build
        // took 32-36 us for them, its probes are workgroup-wide reductions over 16 waves)
        const int nsel = sp.cnt ? nexp : nmax;
        if (nsel <= 256 * 4) kern = select_topk_kernel<4, 256, false>;
        else if (nsel <= 256 * 16) kern = select_topk_kernel<16, 256, false>;
        else if (nsel <= 256 * 32) kern = select_topk_kernel<32, 256, false>;
        else { kern = select_topk_kernel<32, 1024, false>; nt = 1024; }
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)sp.nq), dim3(nt), lds, s, sp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Which pass of a prefiltered search (search_view_s16) a search_view call enqueues, and what that pass reads.  The default is
// a plain search.
struct S16Pass {
    int mode = 0;                    // 0 plain, 1 the 16-bit pass, 2 the gated fp32 fallback
    const int *qexp = nullptr;       // 1: the fp16 queries' exponents
    const uint32_t *gate = nullptr;  // 2: the per-query fallback flags [gate_n] (ScanParams::gate)
    int gate_n = 0;
    uint32_t *gate_count = nullptr;  // 2: counts the fallbacks taken (SelectParams::gate_count)
};

typedef void (*ScanKernel)(ScanParams);

// a scan build's opt-in to lds bytes of dynamic LDS: once in front of the launch(es) of a search
static int scan_lds_opt_in(ScanKernel kern, size_t lds)
{
    HIP_TRY(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    return 0;
}

// one scan launch: grid workgroups of 256 threads with lds bytes of dynamic LDS
static int launch_scan(ScanKernel kern, const ScanParams &p, int grid, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL(kern, dim3(grid), dim3(256), lds, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// the builds of one wave layout: fp32 or bf16 rows; one query tile (rows are read once, non-temporal staging loads) or several
template <int WM, int WN, int TM, int TN>
static ScanKernel scan_build(bool l2, bool approx16, bool one_qtile)
{
    if (approx16) {
        if (one_qtile) return l2 ? flat_scan_kernel<WM, WN, TM, TN, true, true, false, true> : flat_scan_kernel<WM, WN, TM, TN, false, true, false, true>;
        return l2 ? flat_scan_kernel<WM, WN, TM, TN, true, false, false, true> : flat_scan_kernel<WM, WN, TM, TN, false, false, false, true>;
    }
    if (one_qtile) return l2 ? flat_scan_kernel<WM, WN, TM, TN, true, true> : flat_scan_kernel<WM, WN, TM, TN, false, true>;
    return l2 ? flat_scan_kernel<WM, WN, TM, TN, true, false> : flat_scan_kernel<WM, WN, TM, TN, false, false>;
}

// The flat_scan_kernel build that serves a launch: query tile qt, squared L2 or inner product, bf16 rows, one query tile or
// several, the width of the difference build (0: none), the pass of a prefiltered search (S16Pass::mode).  nullptr with the
// error set when no build serves the combination (scan_kernel_illegal, plan.h).
static ScanKernel pick_scan_kernel(int qt, bool l2, bool approx16, bool one_qtile, int diff_width, int pass_mode, int s16_fmt = 16)
{
    if (const char *why = scan_kernel_illegal(qt, l2, approx16, one_qtile, pass_mode)) {
        set_err(KNN_ERR_INVALID, why);
        return nullptr;
    }
    switch (qt) {
    case 256: return l2 ? flat_scan_kernel<2, 2, 4, 4, true, false> : flat_scan_kernel<2, 2, 4, 4, false, false>;
    case 128: return scan_build<2, 2, 2, 2>(l2, approx16, one_qtile);
    // (16-query blocks, three per wave)
    case 96: return l2 ? flat_scan_kernel<2, 2, 2, 1, true, true, false, false, 0, 3> : flat_scan_kernel<2, 2, 2, 1, false, true, false, false, 0, 3>;
    case 48: return l2 ? flat_scan_kernel<4, 1, 2, 1, true, true, false, false, 0, 3> : flat_scan_kernel<4, 1, 2, 1, false, true, false, false, 0, 3>;
    case 64: return scan_build<2, 2, 2, 1>(l2, approx16, one_qtile);
    }
    if (pass_mode == 1 && s16_fmt == 12) return flat_scan_kernel<4, 1, 2, 1, false, true, false, false, 0, 0, true, true>; // ... on the 12-bit row copies
    if (pass_mode == 1) return flat_scan_kernel<4, 1, 2, 1, false, true, false, false, 0, 0, true>; // the 16-bit pass of a prefiltered search (search_view_s16)
    // (difference builds for up to 8, 12, 16 and 19 queries: the vector work of a K step grows with the build's width -- up to 8
    // queries scan at the speed of their HBM traffic)
    switch (diff_width) {
    case 0: break;
    case 8: return flat_scan_kernel<4, 1, 2, 1, true, true, false, false, 8>;
    case 12: return flat_scan_kernel<4, 1, 2, 1, true, true, false, false, 12>;
    case 16: return flat_scan_kernel<4, 1, 2, 1, true, true, false, false, 16>;
    default: return flat_scan_kernel<4, 1, 2, 1, true, true, false, false, 20>;
    }
    return scan_build<4, 1, 2, 1>(l2, approx16, one_qtile);
}

// the build of a symmetric launch (SymPlan): square tiles of ts = 128 or 256 rows
static ScanKernel pick_sym_kernel(int ts, bool l2)
{
    if (ts == 128) return l2 ? flat_scan_kernel<2, 2, 2, 2, true, false, true> : flat_scan_kernel<2, 2, 2, 2, false, false, true>;
    return l2 ? flat_scan_kernel<2, 2, 4, 4, true, false, true> : flat_scan_kernel<2, 2, 4, 4, false, false, true>;
}

// opens a timed launch on s: the next pair of the ring of timing events becomes ev0 / ev1, ev0 is recorded; the caller records
// ev1 behind its launch(es)
static int open_timed_launch(knn_index_s *h, hipStream_t s)
{
    const int slot = (int)(h->nlaunches % knn_index_s::RING);
    if (!h->ring0[slot]) {
        HIP_TRY(hipEventCreate(&h->ring0[slot]));
        HIP_TRY(hipEventCreate(&h->ring1[slot]));
    }
    h->ev0 = h->ring0[slot];
    h->ev1 = h->ring1[slot];
    h->nlaunches++;
    HIP_TRY(hipEventRecord(h->ev0, s));
    return 0;
}

// the words the two workgroups of a CU take turns with (ScanParams::cu_turn), all zero
static int zeroed_turn_words(knn_index_s *h, hipStream_t s, uint32_t **words)
{
    if (!(*words = scratch<uint32_t>(h, h->ws_turn, 2048, s))) return KNN_ERR_HIP;
    if (h->turn_zeroed != *words) { // (once per allocation: a fill in front of every launch was 10 us of idle GPU per CATH-sized search)
        HIP_TRY(hipMemsetAsync(*words, 0, 2048 * 4, s));
        h->turn_zeroed = *words;
    }
    return 0;
}

// where the result of a (view) search goes
struct SearchOut {
    uint64_t *keys = nullptr; // sorted keys, k per query
    int64_t keys_stride = 0;
    int keys_fill = 0;
    float *D = nullptr;
    int64_t *I = nullptr;
    // seeding the enclosing search (see SelectParams)
    uint32_t *seed_cnt = nullptr, *seed_gthr = nullptr, *seed_qthr = nullptr;
    int seed_j = 0, seed_stat = 0;
    int64_t seed_nslots = 0;
};

// ---- the exact 16-bit prefilter (DESIGN 4.9) ----------------------------------------------------------------------------
static int search_view(knn_index_s *h, const float *q_dev, const float *xn, int64_t nq, int k, uint32_t id_base, int row_mul,
                       int vshift, int level, const SearchOut &out, bool allow_stat, hipStream_t s, int *reset_flag = nullptr,
                       const S16Pass &pass = S16Pass());

// what the planner (plan.h) reads from a handle
static PlanCtx plan_ctx(const knn_index_s *h)
{
    PlanCtx c;
    c.metric = h->metric; c.approx16 = h->approx16;
    c.flags = h->flags; c.force_qt = h->force_qt; c.force_chunks = h->force_chunks;
    c.num_cus = h->num_cus; c.batch_nq = h->batch_nq; c.pub_rounds_force = h->pub_rounds_force; c.ntotal = h->ntotal;
    c.s16_fmt = h->s16_fmt;
    return c;
}

// One prefiltered search, ten launches on the caller's stream, no host wait:
//   scan16_queries_kernel   fp16 queries, exponents, bounds B_q, the per-query fallback flags
//   16-bit pass             the streaming scan machinery on the fp16 (or 12-bit) copies with k' = s16_kprime(k, format): the exact
//                           top-k' of the approximate scores (state reset, flat_scan_q32_d256_f16x / _x12, selection in two launches)
//   rescore16_kernel        the window check and the exact scores of the rows inside the window: a grid of (query, 16 of its
//                           k' keys), every row fetched by a whole workgroup with coalesced 16-byte loads
//   selection               the exact top-k of those -> D / I or keys, exactly as the fp32 search writes them
//   gated fp32 search       state reset, scan, selection of the plain search, each returning at once unless some query's
//                           flag is set -- then it overwrites the output with the plain search's bits
static int search_view_s16(knn_index_s *h, const float *q_dev, const float *xn, int64_t nq, int k, uint32_t id_base, int vshift,
                           const SearchOut &out, hipStream_t s, int *reset_flag)
{
    const int kp = s16_kprime(k, h->s16_fmt);
    _Float16 *q16;
    int *qexp; // [4][nq]: exponents, bounds B_q, the two fallback flags
    uint64_t *akeys, *okeys;
    if (!(q16 = scratch<_Float16>(h, h->ws_q16x, (size_t)nq * h->dp16, s)) || !(qexp = scratch<int>(h, h->ws_s16q, (size_t)nq * 4, s)) ||
        !(akeys = scratch<uint64_t>(h, h->ws_s16ak, (size_t)nq * kp, s)) || !(okeys = scratch<uint64_t>(h, h->ws_s16ok, (size_t)nq * kp, s)))
        return KNN_ERR_HIP;
    uint32_t *sstat = (uint32_t *)h->ws_s16stat.p;
    if (!sstat) {
        if (!(sstat = scratch_device_wide<uint32_t>(h->ws_s16stat, 4))) return KNN_ERR_HIP;
        HIP_TRY(hipMemsetAsync(sstat, 0, 16, s));
    }
    float *Bq = (float *)(qexp + nq);
    uint32_t *pfail = (uint32_t *)(Bq + nq), *rfail = pfail + nq;
    hipLaunchKernelGGL(scan16_queries_kernel, dim3((unsigned)nq), dim3(64), 0, s, q_dev, h->dp, h->dp16, q16, qexp, Bq, pfail, h->s16_stat, sstat,
                       h->s16_pieces == 0 ? 1 : 0);
    HIP_TRY(hipGetLastError());
    SearchOut ao;
    ao.keys = akeys; ao.keys_stride = kp; ao.keys_fill = 0;
    S16Pass f16;
    f16.mode = 1;
    f16.qexp = qexp;
    int rc = search_view(h, (const float *)q16, nullptr, nq, kp, id_base, 1, vshift, 0, ao, false, s, reset_flag, f16);
    if (rc) return rc;
    const size_t rlds = rescore16_lds(h->dp);
    HIP_TRY(hipFuncSetAttribute((const void *)rescore16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)rlds)); // (above 64 KB from dp = 1024 on)
    hipLaunchKernelGGL(rescore16_kernel, dim3((unsigned)nq, (unsigned)((kp + RS16_ROWS - 1) / RS16_ROWS)), dim3(256), rlds, s, akeys,
                       kp, k, Bq, pfail, rfail, h->xb, h->dp, q_dev, id_base, okeys, sstat);
    HIP_TRY(hipGetLastError());
    SelectParams sp = {};
    sp.in = okeys; sp.in_stride = kp; sp.n_fixed = kp; sp.cap = kp; sp.n_expect = kp;
    sp.nq = nq; sp.k = k; sp.metric = h->metric;
    sp.out_keys = out.keys; sp.out_stride = out.keys ? out.keys_stride : 0; sp.out_fill = out.keys_fill;
    sp.D = out.D; sp.I = out.I;
    rc = launch_select(sp, s);
    if (rc) return rc;
    S16Pass gated;
    gated.mode = 2;
    gated.gate = rfail;
    gated.gate_n = (int)nq;
    gated.gate_count = sstat + 1;
    rc = search_view(h, q_dev, xn, nq, k, id_base, 1, vshift, 0, out, false, s, nullptr, gated);
    h->last_s16_used = true;
    h->last_s16_fmt = h->s16_fmt;
    h->s16_pieces++;
    return rc;
}

// Exact top-k of the block-strided view (view_row) with stride row_mul / block shift vshift for
// queries [nq][dp] on the device.  allow_stat: the caller checks h->ws_flag afterwards.  pass: the pass of a prefiltered
// search this is (search_view_s16), handed on unchanged to the seed sample's search.
static int search_view(knn_index_s *h, const float *q_dev, const float *xn, int64_t nq, int k, uint32_t id_base, int row_mul,
                       int vshift, int level, const SearchOut &out, bool allow_stat, hipStream_t s, int *reset_flag, const S16Pass &pass)
{
    const int64_t nb = view_rows(h->ntotal, row_mul, vshift);
    const PlanCtx c = plan_ctx(h);
    if (h->scan16 == 1 && h->s16_ok->load() && h->s16_rows && !out.seed_cnt && s16_eligible(c, pass.mode, nb, nq, k, row_mul, level, h->dp, h->s16_fmt))
        return search_view_s16(h, q_dev, xn, nq, k, id_base, vshift, out, s, reset_flag);
    if (level >= knn_index_s::MAX_LEVELS) return set_err(KNN_ERR_INVALID, "search: seed recursion too deep");
    const SearchPlan plan = plan_search(c, nb, nq, k, level, row_mul, allow_stat, pass.mode);
    const ScanPlan &pl = plan.pl;
    const int sstride = plan.sstride, svshift = plan.svshift < 0 ? vshift : plan.svshift, seed_stat = plan.seed_stat;
    const int pub_rounds = plan.pub_rounds, pub_m = plan.pub_m, qcap = plan.qcap;
    LevelBufs &lb = h->ws_level[level];
    uint64_t reset_sig = 0; // != 0: this search's final selection resets the level's state for a successor of the same shape
    const size_t nslots = (size_t)pl.nqtiles * pl.qt;
    uint64_t *qlist;
    uint32_t *qcnt, *gthr, *qthr;
    if (!(qlist = scratch<uint64_t>(h, lb.qlist, (size_t)nq * qcap, s)) || !(qcnt = scratch<uint32_t>(h, lb.qcnt, (size_t)nq, s)) ||
        !(gthr = scratch<uint32_t>(h, lb.gthr, nslots, s)) || !(qthr = scratch<uint32_t>(h, lb.qthr, (size_t)nq, s)))
        return KNN_ERR_HIP;
    int rc;
    if (sstride) {
        lb.clean_sig = 0;
        // the sample's sorted top-k opens every query's candidate array; its seed_j-th score is the
        // running threshold the main pass starts from
        SearchOut so;
        so.keys = qlist; so.keys_stride = qcap; so.keys_fill = 0;
        so.seed_cnt = qcnt; so.seed_gthr = gthr; so.seed_qthr = qthr; so.seed_j = plan.seed_j; so.seed_stat = seed_stat;
        so.seed_nslots = (int64_t)nslots;
        rc = search_view(h, q_dev, xn, nq, plan.k_sample, id_base, row_mul * sstride, svshift, level + 1, so, false, s, reset_flag, pass);
        if (rc) return rc;
    } else {
        const int64_t nn = std::max<int64_t>((int64_t)nslots, nq);
        uint64_t *pub = nullptr;
        uint32_t *arrive = nullptr;
        const int64_t npub = (int64_t)nslots * pub_rounds * pl.nchunks * pub_m;
        if (pub_rounds) {
            if (!(pub = scratch<uint64_t>(h, lb.pub, (size_t)npub, s)) || !(arrive = scratch<uint32_t>(h, lb.arrive, (size_t)pl.nqtiles, s))) return KNN_ERR_HIP;
        }
        // (the first launch of a search: it also clears the verification flag)
        if (pl.npairs && !scratch<uint32_t>(h, lb.pair_ctr, (size_t)pl.npairs + 1, s)) return KNN_ERR_HIP;
        // A streaming search whose predecessor on this handle had exactly this shape finds the state already reset: that
        // search's final selection did it (SelectParams::rs_*) -- one launch and a ~10 us launch gap less per step.
        if (pub_rounds && pl.npairs && !(h->flags & KNN_TUNE_ALWAYS_RESET) && !pass.mode) { // (not inside a prefiltered search: its two passes differ in shape)
            uint64_t sig = 0x9E3779B97F4A7C15ull;
            const uint64_t parts[] = {(uint64_t)nslots, (uint64_t)nq, (uint64_t)npub, (uint64_t)pl.nqtiles, (uint64_t)pl.npairs, (uint64_t)(uintptr_t)gthr,
                                      (uint64_t)(uintptr_t)qcnt, (uint64_t)(uintptr_t)qthr, (uint64_t)(uintptr_t)pub, (uint64_t)(uintptr_t)arrive,
                                      (uint64_t)(uintptr_t)lb.pair_ctr.p, (uint64_t)(uintptr_t)h->ws_flag.p};
            for (uint64_t v : parts) sig = (sig ^ v) * 0x100000001B3ull;
            reset_sig = sig ? sig : 1;
        }
        if (!(reset_sig && lb.clean_sig == reset_sig)) {
            hipLaunchKernelGGL(init_level_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s, gthr, (int64_t)nslots, qcnt, qthr, nq,
                               reset_flag, pub, npub, arrive, (int64_t)pl.nqtiles, pl.npairs ? (uint32_t *)lb.pair_ctr.p : nullptr, (int64_t)pl.npairs,
                               pass.gate, pass.gate_n);
            HIP_TRY(hipGetLastError());
        }
        lb.clean_sig = 0; // (until this search's own selection has been enqueued)
    }
    if (pl.npairs && sstride) { // (the sample's own search initialised this level: the pairs' ticket counters are left)
        uint32_t *ctr = scratch<uint32_t>(h, lb.pair_ctr, (size_t)pl.npairs + 1, s);
        if (!ctr) return KNN_ERR_HIP;
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)ctr, 2, (size_t)pl.npairs, s));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(ctr + pl.npairs), 0, 1, s));
    }
    ScanParams p = {};
    if (!(p.lists = scratch<uint64_t>(h, h->ws_lists, (size_t)pl.grid * pl.qt * pl.cap, s, "search: out of device memory (candidate lists)"))) return KNN_ERR_HIP;
    p.xb = h->xb; p.yn = h->yn; p.xq = q_dev; p.xn = xn;
    p.nb = nb; p.nq = nq; p.dp = h->dp; p.k = k; p.cap = pl.cap;
    if (h->approx16) { // bf16 rows and queries: a row is dp / 2 four-byte units
        p.xb = (const float *)h->xb16.p;
        p.dp = h->dp / 2;
    }
    if (pass.mode == 1) { // the 16-bit pass: fp16 rows and queries (q_dev), a row is dp16 / 2 four-byte units
        // (the 12-bit build addresses whole tiles of consecutive rows: plan_search gives its pass no sample, and nothing else strides it)
        if (h->s16_fmt == 12 && (row_mul != 1 || sstride)) return set_err(KNN_ERR_INVALID, "search: the 12-bit row copies cannot serve a strided view");
        p.xb = (const float *)h->s16_rows;
        p.dp = h->dp16 / 2;
        p.xexp = h->s16_exp;
        p.qexp = pass.qexp;
    }
    p.gate = pass.gate; // (a gated fallback)
    p.gate_n = pass.gate_n;
    p.nqtiles = pl.nqtiles; p.nchunks = pl.nchunks; p.tiles_base = pl.tiles_base; p.tiles_rem = pl.tiles_rem;
    p.gthr = gthr;
    p.qlist = qlist; p.qcnt = qcnt; p.qcap = qcap;
    p.id_base = id_base;
    p.row_mul = row_mul;
    p.vshift = sstride ? svshift : vshift;
    p.skip_mask = sstride ? sstride - 1 : -1;
    p.kslot = plan.kslot;
    p.sparse_epi = plan.sparse_epi;
    p.pub = pub_rounds ? (uint64_t *)lb.pub.p : nullptr;
    p.arrive = pub_rounds ? (uint32_t *)lb.arrive.p : nullptr;
    p.pub_rounds = pub_rounds;
    p.pub_n = pub_rounds * pl.nchunks * pub_m;
    p.pub_m = pub_m;
    p.pair_ctr = pl.npairs ? (uint32_t *)lb.pair_ctr.p : nullptr;
    p.npairs = pl.npairs;
    if (pl.diff) {
        const int dnq = diff_build_width(nq); // (the build pick_scan_kernel picks)
        float *qdiff = scratch<float>(h, h->ws_qdiff, (size_t)dnq * h->dp, s);
        if (!qdiff) return KNN_ERR_HIP;
        const int64_t tot = (int64_t)dnq * h->dp;
        hipLaunchKernelGGL(diff_interleave_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, q_dev, nq, h->dp, dnq, qdiff);
        HIP_TRY(hipGetLastError());
        p.xq_diff = qdiff;
    }
    if (plan.cu_turn && (rc = zeroed_turn_words(h, s, &p.cu_turn))) return rc;
    p.pool_tiles = plan.pool_tiles;
    if (pub_rounds && !(p.defer = scratch<float>(h, h->ws_defer, (size_t)pl.grid * pl.qt * pl.dt, s))) return KNN_ERR_HIP;
    const bool top = level == 0 && pass.mode != 2; // (a gated fallback leaves the introspection to the 16-bit pass)
#ifdef KNN355_TRACE
    if (level == (getenv("KNN355_TRACE_LEVEL") ? atoi(getenv("KNN355_TRACE_LEVEL")) : 0)) { // (developer build: which seed level's launch is stamped)
        if (!(p.trace = scratch_device_wide<unsigned long long>(g_trace_buf, (size_t)pl.grid * 128, "trace: out of device memory"))) return KNN_ERR_HIP;
        HIP_TRY(hipMemsetAsync(p.trace, 0, (size_t)pl.grid * 128 * 8, s));
        p.ablate = getenv("KNN355_ABLATE") ? atoi(getenv("KNN355_ABLATE")) : 0;
        g_trace_grid = pl.grid;
    }
#endif
    if (top && (rc = open_timed_launch(h, s))) return rc;
    const ScanKernel kern = pick_scan_kernel(pl.qt, h->metric == KNN_METRIC_L2, h->approx16, pl.nqtiles == 1, pl.diff ? diff_build_width(nq) : 0, pass.mode, h->s16_fmt);
    if (!kern) return KNN_ERR_INVALID;
    rc = scan_lds_opt_in(kern, pl.lds);
    if (!rc) rc = launch_scan(kern, p, pl.grid, pl.lds, s);
    if (rc) return rc;
    if (top) {
        HIP_TRY(hipEventRecord(h->ev1, s));
        h->last_kernel = pass.mode == 1 ? std::string(pl.name) + (h->s16_fmt == 12 ? "_x12" : "_f16x") : std::string(pl.name); h->last_qt = pl.qt; h->last_dt = pl.dt; h->last_chunks = pl.nchunks; h->last_grid = pl.grid;
        h->last_seed_stride = pub_rounds ? -pub_rounds * pub_m : sstride; // (negative: tile-minimum seed, keys per workgroup and query)
        h->last_seed_stat = seed_stat ? plan.seed_j : 0;
        h->last_sample_rows = sstride ? view_rows(nb, sstride, p.vshift) : 0;
    }
    // final selection: every query's candidates (seed list + the chunks' survivors) -> sorted top-k
    SelectParams sp = {};
    sp.in = qlist; sp.in_stride = qcap; sp.cnt = qcnt; sp.cap = qcap;
    sp.n_expect = select_expect_n(plan, nb, k, sstride ? view_rows(nb, sstride, p.vshift) : 0);
    sp.nq = nq; sp.k = k; sp.metric = h->metric;
    sp.out_keys = out.keys; sp.out_stride = out.keys ? out.keys_stride : 0; sp.out_fill = out.keys_fill;
    sp.D = out.D; sp.I = out.I;
    sp.seed_cnt = out.seed_cnt; sp.seed_gthr = out.seed_gthr; sp.seed_qthr = out.seed_qthr; sp.seed_j = out.seed_j; sp.seed_stat = out.seed_stat;
    sp.seed_nslots = out.seed_nslots;
    sp.qthr = qthr; sp.fail = (int *)h->ws_flag.p;
    sp.gate = pass.gate; sp.gate_n = pass.gate_n; sp.gate_count = pass.gate_count;
    if (reset_sig && out.seed_cnt == nullptr) {
        sp.rs_gthr = gthr; sp.rs_qcnt = qcnt; sp.rs_qthr = qthr; sp.rs_nslots = (int)nslots;
        sp.rs_pub = (uint64_t *)lb.pub.p; sp.rs_pub_n = pub_rounds * pl.nchunks * pub_m;
        sp.rs_arrive = (uint32_t *)lb.arrive.p; sp.rs_narrive = pl.nqtiles;
        sp.rs_pair = (uint32_t *)lb.pair_ctr.p; sp.rs_npairs = pl.npairs;
    }
    rc = launch_select(sp, s, &h->ws_tmp);
    if (!rc && sp.rs_gthr) lb.clean_sig = reset_sig;
    if (level == 0 && h->done) (void)hipEventRecord(h->done, s); // (everything this search enqueued: see DevBuf::ensure)
    return rc;
}

// queries [nq][dp] already on device (padded); writes sorted keys [nq][k] and/or D/I.
// allow_stat: the caller reads the fail flag once the stream has drained (wait_search) and repeats
// the search with allow_stat = false if it is set.
// The batch a caller handed over, for as long as the search works through it in pieces (the outermost scope wins).
struct BatchScope {
    knn_index_s *h;
    int64_t prev;
    BatchScope(knn_index_s *h_, int64_t nq) : h(h_), prev(h_->batch_nq)
    {
        if (!prev) h->batch_nq = h->batch_hint > 0 ? std::max(nq, h->batch_hint) : nq;
    }
    ~BatchScope() { h->batch_nq = prev; }
};

static int search_keys_impl(knn_index_s *h, const float *q_dev, int64_t nq, int k, uint32_t id_base,
                            uint64_t *keys_out, float *D_out, int64_t *I_out, bool allow_stat, hipStream_t s)
{
    BatchScope scope(h, nq);
    h->last_s16_used = false;
    h->s16_pieces = 0;
    const float *xn = nullptr;
    if (h->metric == KNN_METRIC_L2) {
        float *qn = scratch<float>(h, h->ws_qn, (size_t)nq, s);
        if (!qn) return KNN_ERR_HIP;
        int rc = norms_dev_impl(q_dev, nq, h->d, h->dp, qn, s);
        if (rc) return rc;
        xn = qn;
    }
    int *flag = scratch<int>(h, h->ws_flag, 16, s);
    if (!flag) return KNN_ERR_HIP;
    if (h->approx16) {
        // the scan reads bf16 queries (the fp32 ones above gave the exact norms)
        __bf16 *q16 = scratch<__bf16>(h, h->ws_q16, (size_t)nq * h->dp, s);
        if (!q16) return KNN_ERR_HIP;
        const int64_t total = nq * h->dp;
        hipLaunchKernelGGL(to_bf16_kernel, dim3((unsigned)std::min<int64_t>((total / 4 + 255) / 256, 65535)), dim3(256), 0, s, q_dev, total, q16);
        HIP_TRY(hipGetLastError());
        q_dev = (const float *)q16;
    }
    const std::vector<Piece> pieces = plan_pieces(plan_ctx(h), nq, k, allow_stat);
    for (size_t b = 0; b < pieces.size(); b++) {
        const int64_t q0 = pieces[b].q0, m = pieces[b].m;
        SearchOut out;
        out.keys = keys_out ? keys_out + q0 * k : nullptr; out.keys_stride = k; out.keys_fill = 0;
        out.D = D_out ? D_out + q0 * k : nullptr; out.I = I_out ? I_out + q0 * k : nullptr;
        int rc = search_view(h, q_dev + q0 * (h->approx16 ? h->dp / 2 : h->dp), xn ? xn + q0 : nullptr, m, k, id_base, 1, 3, 0, out, allow_stat, s,
                             b == 0 ? flag : nullptr);
        if (rc) return rc;
    }
    return 0;
}

static int check_search_args(knn_index_s *h, const void *q, int64_t nq, int64_t k, const void *D, const void *I)
{
    if (!h) return set_err(KNN_ERR_INVALID, "search: null handle");
    if (nq < 0) return set_err(KNN_ERR_INVALID, "search: negative nq");
    if (k < 1) return set_err(KNN_ERR_INVALID, "search: k must be >= 1");
    if (k > KNN_MAX_K) return set_err(KNN_ERR_UNSUPPORTED, "search: k > 2048 is not supported by the fused top-k");
    if (nq > 0 && (!q || !D || !I)) return set_err(KNN_ERR_INVALID, "search: null pointer");
    if (view_is_stale(h)) return set_err(KNN_ERR_INVALID, "search" KNN_STALE_VIEW_MSG);
    return 0;
}

// index with no rows: every slot is unfilled
__global__ void fill_empty_kernel(int64_t total, int metric, uint64_t *__restrict__ keys, float *__restrict__ D, int64_t *__restrict__ I)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    if (keys) keys[i] = KEY_PAD;
    if (D) {
        D[i] = metric == KNN_METRIC_INNER_PRODUCT ? -FLT_MAX : FLT_MAX;
        I[i] = -1;
    }
}
// the same for results in host memory: D[n], I[n]
static void fill_empty_host(float *D, int64_t *I, int64_t n, int metric)
{
    const float pad = metric == KNN_METRIC_INNER_PRODUCT ? -FLT_MAX : FLT_MAX;
    for (int64_t i = 0; i < n; i++) {
        D[i] = pad;
        I[i] = -1;
    }
}

// q_dev: [nq][d] contiguous on device. D_dev/I_dev on device.
static int search_dev_impl(knn_index_s *h, const float *q_dev, int64_t nq, int k, float *D_dev, int64_t *I_dev,
                           uint64_t *keys_dev, uint32_t id_base, bool allow_stat, hipStream_t s)
{
    if (nq == 0) return 0;
    // packed keys carry id_base + row in 32 bits: a shard whose ids would wrap is refused before anything is launched (a
    // wrapped id collides with or sorts in front of another shard's, and the merge takes keys to be distinct)
    if (keys_dev && (uint64_t)id_base + (uint64_t)h->ntotal > (1ull << 32))
        return set_err(KNN_ERR_INVALID, "search_keys: id_base " + std::to_string(id_base) + " + ntotal " + std::to_string(h->ntotal) +
                                            " exceeds 2^32: ids are 32 bits wide in the packed keys");
    const int64_t total = nq * k;
    if (h->ntotal == 0) {
        hipLaunchKernelGGL(fill_empty_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, total, h->metric, keys_dev, D_dev, I_dev);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    const float *qp = q_dev;
    if (h->dp != h->d) {
        float *padded = scratch<float>(h, h->ws_q, (size_t)nq * h->dp, s);
        if (!padded) return KNN_ERR_HIP;
        int rc = pad_rows_dev(q_dev, nq, h->d, padded, h->dp, s);
        if (rc) return rc;
        qp = padded;
    }
    return search_keys_impl(h, qp, nq, k, id_base, keys_dev, D_dev, I_dev, allow_stat, s);
}

// waits for the search on s; then: did a statistically seeded search fail its verification?
static int wait_search(knn_index_s *h, hipStream_t s, bool *failed)
{
    *failed = false;
    HIP_TRY(hipStreamSynchronize(s));
    if (!h->ws_flag.p || h->ntotal == 0) return 0;
    int flag = 0;
    HIP_TRY(hipMemcpy(&flag, h->ws_flag.p, 4, hipMemcpyDeviceToHost));
    *failed = flag != 0;
    if (flag) {
        h->stat_redo++;
        // read = cleared: a search whose predecessor left the level's state reset (LevelBufs::clean_sig) skips the launch
        // that clears the flag, and a repeat that returns early with an error never reaches its own (ADVICE r3)
        // (on the handle's stream, like every other access to the flag: a NULL-stream memset is not ordered against a
        // non-blocking stream, and completing late it could erase the flag of the repeat search -- ADVICE r4)
        HIP_TRY(hipMemsetAsync(h->ws_flag.p, 0, 4, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return 0;
}

extern "C" int knn_flat_search_dev(knn_handle h, const float *q_dev, int64_t nq, int64_t k, float *D_dev,
                                   int64_t *I_dev, void *stream)
{
    int rc = check_search_args(h, q_dev, nq, k, D_dev, I_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    h->last_ms = -1.f;
    // a caller's stream means "enqueue and return": no way to look at the verification flag, so
    // only the synchronous form may use the statistical seed
    const bool sync = stream == nullptr;
    rc = search_dev_impl(h, q_dev, nq, (int)k, D_dev, I_dev, nullptr, 0, sync, s);
    if (rc) return rc;
    if (sync) {
        bool failed = false;
        rc = wait_search(h, s, &failed);
        if (rc) return rc;
        if (failed) {
            rc = search_dev_impl(h, q_dev, nq, (int)k, D_dev, I_dev, nullptr, 0, false, s);
            if (rc) return rc;
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    return 0;
}

extern "C" int knn_flat_search_keys_dev(knn_handle h, const float *q_dev, int64_t nq, int64_t k, uint32_t id_base,
                                        uint64_t *keys_dev, void *stream)
{
    int rc = check_search_args(h, q_dev, nq, k, keys_dev, keys_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    h->last_ms = -1.f;
    rc = search_dev_impl(h, q_dev, nq, (int)k, nullptr, nullptr, keys_dev, id_base, false, s);
    if (rc) return rc;
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

extern "C" int knn_merge_keys_dev(knn_handle h, const uint64_t *keys_dev, int32_t nlists, int64_t nq, int64_t k,
                                  float *D_dev, int64_t *I_dev, void *stream)
{
    if (!h) return set_err(KNN_ERR_INVALID, "merge_keys: null handle");
    if (nlists < 1 || nq < 0 || k < 1 || k > KNN_MAX_K) return set_err(KNN_ERR_INVALID, "merge_keys: bad shape");
    if (nq == 0) return 0;
    if (!keys_dev || !D_dev || !I_dev) return set_err(KNN_ERR_INVALID, "merge_keys: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = stream ? (hipStream_t)stream : h->stream;
    // one launch whatever nlists * k is, no scratch memory: the selection reads the all-gather buffer in place
    SelectParams sp = {};
    sp.in = keys_dev; sp.lm_lists = nlists; sp.lm_k = (int)k;
    sp.nq = nq; sp.k = (int)k; sp.metric = h->metric;
    sp.D = D_dev; sp.I = I_dev;
    int rc = launch_select(sp, s);
    if (rc) return rc;
    if (!stream) HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

// Symmetric all-vs-all: index.search(x, k) for x = ALL rows of the index (cath/search.py:22-24,
// pfam/proteins_search.py:37,49, pfam/slices/slices_search.py:22-28 -- every flat search of the reference is one).
// Only the score tiles on and above the diagonal are multiplied (flat_scan_kernel<..., SYM>); needs the statistical
// seed (the rows of a database tile have no candidate list of their own in that kernel, only their compact arrays)
// and k <= 1536.  Returns 1 when it ran (D_dev / I_dev hold all n x k results, the verification flag is still to be
// read by the caller), 0 when the plain path should be used, < 0 on error.
//
// D_host / I_host / d2h given and the result large: the query tiles are served in sp.groups launches of consecutive tiles, each
// followed by the final selection of ITS rows -- a row's candidates are complete once every query tile up to its own has been
// served (tile (I, J), J >= I, scores rows I against J and J against I) -- and by their download on the copy stream d2h, which
// then overlaps the launches of the later groups (Pfam-sized k = 1000: 2.4 GB of results, 0.15 s behind a 0.38 s search;
// CATH-sized k = 301: 52 MB, 1.3 ms on the wire behind a 2.5 ms search, in four groups).
// Returns 2 then (the caller waits for d2h and checks the verification flag), 1 when the results are in D_dev / I_dev only.
// Every decision is plan_self_symmetric's and sym_work_table's (plan.h).
static int self_search_symmetric(knn_index_s *h, int k, float *D_dev, int64_t *I_dev, hipStream_t s, float *D_host = nullptr,
                                 int64_t *I_host = nullptr, hipStream_t d2h = nullptr)
{
    const int64_t n = h->ntotal;
    SymPlan sp;
    if (!plan_self_symmetric(plan_ctx(h), k, D_host && I_host && d2h, sp)) return 0;
    const int qcap = sp.qcap, groups = sp.groups;
    const size_t nslots = (size_t)sp.tiles * sp.ts;
    LevelBufs &lb = h->ws_level[0];
    lb.clean_sig = 0; // (this search leaves the level's state in its own shape)
    const char *oom = "search_self: out of device memory";
    uint64_t *qlist;
    uint32_t *qcnt, *gthr, *qthr;
    int *flag;
    if (!(qlist = scratch_device_wide<uint64_t>(lb.qlist, (size_t)n * qcap, oom)) || !(qcnt = scratch_device_wide<uint32_t>(lb.qcnt, (size_t)n, oom)) ||
        !(gthr = scratch_device_wide<uint32_t>(lb.gthr, nslots, oom)) || !(qthr = scratch_device_wide<uint32_t>(lb.qthr, (size_t)n, oom)) ||
        !(flag = scratch_device_wide<int>(h->ws_flag, 16, oom)))
        return KNN_ERR_HIP;
    const float *xn = h->metric == KNN_METRIC_L2 ? h->yn : nullptr; // the queries are the rows: their norms are the row norms
    // 0. the work table.  It depends on (tiles, groups, CUs) only: it stays on the device between searches (uploading it between
    //    the sample pass and the main launch cost a host round trip -- 35 us of idle GPU -- per search).
    if (h->sym_tiles != sp.tiles || h->sym_ts != sp.ts || h->sym_groups != groups || !h->ws_sym.p) {
        const SymTable t = sym_work_table(sp.tiles, groups, sp.slots);
        h->sym_tiles = -1;
        if (!scratch<SymItem>(h, h->ws_sym, t.items.size(), s, oom)) return KNN_ERR_HIP;
        HIP_TRY(hipMemcpyAsync(h->ws_sym.p, t.items.data(), t.items.size() * sizeof(SymItem), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s)); // (the table is a local vector)
        h->sym_tiles = sp.tiles;
        h->sym_ts = sp.ts;
        h->sym_groups = groups;
        h->sym_run = t.first_run;
        h->sym_items = (int64_t)t.items.size();
        h->sym_gstart = t.gstart;
    }
    const size_t nitems = (size_t)h->sym_items;
    // 1. the sample pass (every row is a query, the strided sample is the database): thresholds + the sample's own candidates
    SearchOut so;
    so.keys = qlist; so.keys_stride = qcap; so.keys_fill = 0;
    so.seed_cnt = qcnt; so.seed_gthr = gthr; so.seed_qthr = qthr; so.seed_j = sp.j; so.seed_stat = 1; so.seed_nslots = (int64_t)nslots;
    int rc = search_view(h, h->xb, xn, n, sp.k_sample, 0, sp.st, 0, 1, so, false, s, flag);
    if (rc) return rc;
    ScanParams p = {};
    p.lists = scratch_device_wide<uint64_t>(h->ws_lists, (size_t)std::min<int64_t>((int64_t)nitems, sp.max_wgs) * sp.ts * sp.pl.cap,
                                            "search_self: out of device memory (candidate lists)");
    if (!p.lists) return KNN_ERR_HIP;
    p.xb = h->xb; p.yn = h->yn; p.xq = h->xb; p.xn = xn;
    p.nb = n; p.nq = n; p.dp = h->dp; p.k = k; p.cap = sp.pl.cap;
    p.nqtiles = sp.tiles; p.nchunks = 1; p.tiles_base = 0; p.tiles_rem = 0;
    p.gthr = gthr;
    p.qlist = qlist; p.qcnt = qcnt; p.qcap = qcap;
    p.id_base = 0; p.row_mul = 1; p.vshift = 0; p.skip_mask = sp.st - 1;
    p.kslot = knn_kslot(k);
    p.fail = flag;
    if (sp.cu_turn && (rc = zeroed_turn_words(h, s, &p.cu_turn))) return rc;
    const ScanKernel kern = pick_sym_kernel(sp.ts, h->metric == KNN_METRIC_L2);
    rc = scan_lds_opt_in(kern, sp.lds);
    if (!rc) rc = open_timed_launch(h, s);
    if (rc) return rc;
#ifdef KNN355_TRACE
    if (!(p.trace = scratch_device_wide<unsigned long long>(g_trace_buf, nitems * 128, "trace: out of device memory"))) return KNN_ERR_HIP;
    HIP_TRY(hipMemsetAsync(p.trace, 0, (size_t)nitems * 128 * 8, s));
    p.ablate = getenv("KNN355_ABLATE") ? atoi(getenv("KNN355_ABLATE")) : 0;
    g_trace_grid = (int)std::min<size_t>(nitems, (size_t)sp.max_wgs);
#endif
    // 2 + 3. the launches, each followed by the final selection of the rows it completes (verified against the sample's bound)
    EventList gev; // with several groups: one behind each group's selection
    for (int g = 0; g < groups; g++) {
        const size_t g0 = (size_t)h->sym_gstart[(size_t)g], g1 = (size_t)h->sym_gstart[(size_t)g + 1];
        for (size_t i0 = g0; i0 < g1; i0 += (size_t)sp.max_wgs) {
            const size_t cnt = std::min<size_t>((size_t)sp.max_wgs, g1 - i0);
            p.sym_items = (const SymItem *)h->ws_sym.p + i0;
            rc = launch_scan(kern, p, (int)cnt, sp.lds, s);
            if (rc) return rc;
        }
        if (g == groups - 1) HIP_TRY(hipEventRecord(h->ev1, s));
        const int64_t r0 = sym_group_row0(sp, n, g), r1 = sym_group_row0(sp, n, g + 1);
        SelectParams sel = {};
        sel.in = qlist + (size_t)r0 * qcap; sel.in_stride = qcap; sel.cnt = qcnt + r0; sel.cap = qcap;
        sel.n_expect = sp.n_expect;
        sel.nq = r1 - r0; sel.k = k; sel.metric = h->metric;
        sel.D = D_dev + (size_t)r0 * k; sel.I = I_dev + (size_t)r0 * k;
        sel.qthr = qthr + r0; sel.fail = flag;
        rc = launch_select(sel, s, &h->ws_tmp);
        if (rc) return rc;
        if (groups > 1 && (rc = gev.mark(s, hipEventDisableTiming))) return rc;
    }
    h->last_kernel = sp.name; h->last_qt = sp.ts; h->last_dt = sp.ts; h->last_chunks = h->sym_run; h->last_grid = (int)nitems;
    h->last_seed_stride = sp.st; h->last_seed_stat = sp.j; h->last_sample_rows = sp.S;
    if (h->done) (void)hipEventRecord(h->done, s); // (everything this search enqueued on the handle's buffers: see DevBuf::ensure)
    h->sym_searches++;
    if (groups == 1) return 1;
    // the downloads, group by group behind their selections (everything above is enqueued: a copy into pageable memory may
    // block this thread as long as it likes)
    hipError_t e = hipSuccess;
    for (int g = 0; g < groups; g++) {
        const int64_t r0 = sym_group_row0(sp, n, g), r1 = sym_group_row0(sp, n, g + 1);
        if (e == hipSuccess) e = hipStreamWaitEvent(d2h, gev.ev[(size_t)g], 0);
        if (e == hipSuccess && r1 > r0) e = hipMemcpyAsync(D_host + (size_t)r0 * k, D_dev + (size_t)r0 * k, (size_t)(r1 - r0) * k * 4, hipMemcpyDeviceToHost, d2h);
        if (e == hipSuccess && r1 > r0) e = hipMemcpyAsync(I_host + (size_t)r0 * k, I_dev + (size_t)r0 * k, (size_t)(r1 - r0) * k * 8, hipMemcpyDeviceToHost, d2h);
    }
    // (always: a copy already queued writes into the caller's arrays)
    const hipError_t es = hipStreamSynchronize(d2h);
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return set_err(KNN_ERR_HIP, hipGetErrorString(e));
    return 2;
}

// Search with results (and, unless q_host is null, queries) in host memory.  q_host == nullptr:
// the queries are the index's own rows [self_row0, self_row0 + nq) -- already on the device and
// padded, nothing to upload.  Caller holds h->mu.
static int host_search(knn_index_s *h, const float *q_host, int64_t self_row0, int64_t nq, int64_t k, float *D_host,
                       int64_t *I_host)
{
    int rc = 0;
    BatchScope scope(h, nq);
    HIP_TRY(hipSetDevice(h->device));
    // Query batches bound the device workspace; 16384 queries keep >= 128 query tiles in flight.
    // Batches are pipelined: while batch b is scanned, a helper thread downloads the results of
    // batch b-1 (pageable host memory: the copy blocks its caller) and this thread uploads the
    // queries of batch b+1, each on its own stream with its own staging buffers.
    int64_t QB = 16384;
    // A single batch with a large result (CATH20-sized all-vs-all with 300 hits: 52 MB, a millisecond on
    // the wire) is split in two so that half of its download overlaps the scan; small results are not
    // worth the extra launches and the extra streams of the pipelined path.
    // (two halves: measured 5.1-5.2 ms for the CATH-sized k=301 search_self against 5.4 in one piece and 5.4 in four --
    // every piece pays its own sample pass and selections)
    if (nq <= QB && (size_t)nq * k * 12 >= ((size_t)24 << 20) && nq >= 4096)
        QB = std::max<int64_t>(2048, ((nq + 1) / 2 + 127) / 128 * 128);
    const int64_t bq = std::min(nq, QB);
    const int64_t nbatches = (nq + QB - 1) / QB;
    DevBuf *qbuf[2] = {&h->ws_tmp2, &h->ws_tmp3}, *dbuf[2] = {&h->ws_D, &h->ws_D1}, *ibuf[2] = {&h->ws_I, &h->ws_I1};
    const int nslots = nbatches > 1 ? 2 : 1;
    for (int i = 0; i < nslots; i++)
        if ((q_host && !scratch_device_wide<float>(*qbuf[i], (size_t)bq * h->d)) || !scratch_device_wide<float>(*dbuf[i], (size_t)bq * k) ||
            !scratch_device_wide<int64_t>(*ibuf[i], (size_t)bq * k))
            return KNN_ERR_HIP;
    if (!h->flag_host) HIP_TRY(hipHostMalloc((void **)&h->flag_host, 64, hipHostMallocDefault));
    // one batch of queries on the device: uploaded rows ([m][d]) or the index's own rows ([m][dp]).
    // The verification flag of a statistically seeded batch travels to flag_host[slot] behind it.
    auto scan = [&](int slot, int64_t b0, int64_t m, bool allow_stat) -> int {
        int r;
        if (q_host)
            r = search_dev_impl(h, (const float *)qbuf[slot]->p, m, (int)k, (float *)dbuf[slot]->p, (int64_t *)ibuf[slot]->p, nullptr, 0, allow_stat, h->stream);
        else
            r = search_keys_impl(h, h->xb + (size_t)(self_row0 + b0) * h->dp, m, (int)k, 0, nullptr, (float *)dbuf[slot]->p,
                                 (int64_t *)ibuf[slot]->p, allow_stat, h->stream);
        if (r) return r;
        h->flag_host[slot] = 0;
        if (allow_stat && h->ntotal > 0) HIP_TRY(hipMemcpyAsync(&h->flag_host[slot], h->ws_flag.p, 4, hipMemcpyDeviceToHost, h->stream));
        return 0;
    };
    // plain form: one batch at a time on the handle's stream (nothing to overlap with, or the
    // device's copy streams are taken)
    auto plain = [&](int64_t b0, int64_t m, bool allow_stat) -> int {
        if (q_host) HIP_TRY(hipMemcpyAsync(qbuf[0]->p, q_host + b0 * h->d, (size_t)m * h->d * 4, hipMemcpyHostToDevice, h->stream));
        int r = scan(0, b0, m, allow_stat);
        if (r) return r;
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (h->flag_host[0]) { // the statistical threshold was too tight for some query: once more without it
            h->stat_redo++;
            r = scan(0, b0, m, false);
            if (r) return r;
        }
        HIP_TRY(hipMemcpyAsync(D_host + b0 * k, dbuf[0]->p, (size_t)m * k * 4, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(I_host + b0 * k, ibuf[0]->p, (size_t)m * k * 8, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        float ms = 0.f;
        if (h->ntotal > 0 && h->ev0 && hipEventElapsedTime(&ms, h->ev0, h->ev1) == hipSuccess) h->last_ms += ms;
        return 0;
    };
    PipeLease lease;
    rc = lease_pipes(h->device, nbatches > 1, lease);
    if (rc) return rc;
    if (!lease.cp) {
        h->last_ms = 0.f;
        for (int64_t b0 = 0; b0 < nq; b0 += QB) {
            rc = plain(b0, std::min(QB, nq - b0), true);
            if (rc) return rc;
        }
        return 0;
    }
    CopyPipes &cp = *lease.cp;
    struct Download {
        std::thread th;
        hipError_t err = hipSuccess;
        hipEvent_t t0 = nullptr, t1 = nullptr; // scan events of the batch
        int64_t batch = -1;
        bool failed = false;
    } dl[2];
    float ms_total = 0.f;
    hipError_t dl_err = hipSuccess;
    std::vector<int64_t> redo; // batches whose statistical threshold failed its verification
    auto join = [&](int slot) {
        if (!dl[slot].th.joinable()) return;
        dl[slot].th.join();
        if (dl[slot].err != hipSuccess) dl_err = dl[slot].err;
        if (dl[slot].failed) redo.push_back(dl[slot].batch);
        float ms = 0.f;
        if (dl[slot].t0 && hipEventElapsedTime(&ms, dl[slot].t0, dl[slot].t1) == hipSuccess) ms_total += ms;
    };
    auto upload = [&](int64_t b) -> hipError_t {
        if (!q_host) return hipSuccess;
        const int slot = (int)(b & 1);
        const int64_t b0 = b * QB, m = std::min(QB, nq - b0);
        hipError_t e = hipMemcpyAsync(qbuf[slot]->p, q_host + b0 * h->d, (size_t)m * h->d * 4, hipMemcpyHostToDevice, cp.h2d);
        if (e == hipSuccess) e = hipEventRecord(cp.ev_query[slot], cp.h2d);
        return e;
    };
    hipError_t e = upload(0);
    for (int64_t b = 0; b < nbatches && e == hipSuccess && rc == 0; b++) {
        const int slot = (int)(b & 1);
        const int64_t b0 = b * QB, m = std::min(QB, nq - b0);
        if (q_host) e = hipStreamWaitEvent(h->stream, cp.ev_query[slot], 0);
        if (e != hipSuccess) break;
        rc = scan(slot, b0, m, true);
        if (rc) break;
        e = hipEventRecord(cp.ev_batch[slot], h->stream);
        if (e != hipSuccess) break;
        dl[slot].t0 = h->ntotal > 0 ? h->ev0 : nullptr;
        dl[slot].t1 = h->ev1;
        dl[slot].err = hipSuccess;
        dl[slot].batch = b;
        dl[slot].failed = false;
        CopyPipes *cpp = &cp;
        dl[slot].th = std::thread([=, &dl]() {
            hipError_t r = hipSetDevice(h->device);
            if (r == hipSuccess) r = hipEventSynchronize(cpp->ev_batch[slot]);
            if (r == hipSuccess && h->flag_host[slot]) {
                dl[slot].failed = true; // repeated below, after the pipeline has drained
                dl[slot].err = hipSuccess;
                return;
            }
            if (r == hipSuccess) r = hipMemcpyAsync(D_host + b0 * k, dbuf[slot]->p, (size_t)m * k * 4, hipMemcpyDeviceToHost, cpp->d2h);
            if (r == hipSuccess) r = hipMemcpyAsync(I_host + b0 * k, ibuf[slot]->p, (size_t)m * k * 8, hipMemcpyDeviceToHost, cpp->d2h);
            if (r == hipSuccess) r = hipStreamSynchronize(cpp->d2h);
            dl[slot].err = r;
        });
        if (b + 1 < nbatches) {
            // the other slot's buffers: its scan (batch b-1) must be over and downloaded
            join(slot ^ 1);
            e = upload(b + 1);
        }
    }
    join(0);
    join(1);
    if (rc) return rc;
    if (e != hipSuccess) return set_err(KNN_ERR_HIP, std::string("search: ") + hipGetErrorString(e));
    if (dl_err != hipSuccess) return set_err(KNN_ERR_HIP, std::string("search: result download failed: ") + hipGetErrorString(dl_err));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->last_ms = ms_total;
    for (int64_t b : redo) {
        h->stat_redo++;
        const int64_t b0 = b * QB;
        rc = plain(b0, std::min(QB, nq - b0), false);
        if (rc) return rc;
    }
    return 0;
}

extern "C" int knn_flat_search(knn_handle h, const float *q_host, int64_t nq, int64_t k, float *D_host,
                               int64_t *I_host)
{
    int rc = check_search_args(h, q_host, nq, k, D_host, I_host);
    if (rc) return rc;
    if (nq == 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    return host_search(h, q_host, 0, nq, k, D_host, I_host);
}

extern "C" int knn_flat_search_self(knn_handle h, int64_t row0, int64_t nrows, int64_t k, float *D_host, int64_t *I_host)
{
    if (!h) return set_err(KNN_ERR_INVALID, "search_self: null handle");
    if (nrows == 0) return 0;
    int rc = check_search_args(h, D_host, nrows, k, D_host, I_host);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    if (row0 < 0 || nrows < 0 || row0 + nrows > h->ntotal) return set_err(KNN_ERR_INVALID, "search_self: row range out of bounds");
    if (row0 == 0 && nrows == h->ntotal && (size_t)nrows * k * 12 <= ((size_t)16 << 30) && self_search_symmetric_eligible(plan_ctx(h), (int)k)) {
        // every row against every row: half the score tiles suffice (self_search_symmetric)
        HIP_TRY(hipSetDevice(h->device));
        float *D_dev;
        int64_t *I_dev;
        if (!(D_dev = scratch_device_wide<float>(h->ws_D, (size_t)nrows * k, "search_self: out of device memory")) ||
            !(I_dev = scratch_device_wide<int64_t>(h->ws_I, (size_t)nrows * k, "search_self: out of device memory")))
            return KNN_ERR_HIP;
        h->last_ms = -1.f;
        // (a large result leaves in pieces while the later query tiles are still being served: the copy stream of the device,
        // if no other host search of this process is using it)
        static const bool stream_off = getenv("KNN355_SELF_STREAM") && atoi(getenv("KNN355_SELF_STREAM")) == 0; // (A/B: the result in one piece behind the search)
        {
            PipeLease lease;
            rc = lease_pipes(h->device, !stream_off && (size_t)nrows * k * 12 >= ((size_t)dev_knob("KNN355_SELF_STREAM_MIN_MB", 32) << 20), lease);
            if (rc) return rc;
            rc = self_search_symmetric(h, (int)k, D_dev, I_dev, h->stream, D_host, I_host, lease.cp ? lease.cp->d2h : nullptr);
        }
        if (rc < 0) return rc;
        // (0: the plan left the search to the plain path after all, which also repeats a search whose verification failed: a
        // threshold estimate was too tight or a candidate array overflowed)
        bool failed = true;
        if (rc > 0) {
            const bool downloaded = rc == 2; // (the rows went out behind their groups' selections)
            rc = wait_search(h, h->stream, &failed);
            if (rc) return rc;
            if (!failed && !downloaded) {
                HIP_TRY(hipMemcpyAsync(D_host, D_dev, (size_t)nrows * k * 4, hipMemcpyDeviceToHost, h->stream));
                HIP_TRY(hipMemcpyAsync(I_host, I_dev, (size_t)nrows * k * 8, hipMemcpyDeviceToHost, h->stream));
                HIP_TRY(hipStreamSynchronize(h->stream));
            }
        }
        // the results' staging stays with the handle for the next search unless it is gigabytes, or host_search follows: that
        // works in batches and takes what it needs
        if (failed || (size_t)nrows * k * 12 > ((size_t)1 << 30)) {
            h->ws_D.release();
            h->ws_I.release();
        }
        if (!failed) return 0;
    }
    return host_search(h, nullptr, row0, nrows, k, D_host, I_host);
}

// the same with the results left on the device (D_dev [ntotal][k], I_dev [ntotal][k]); synchronous
extern "C" int knn_flat_search_self_dev(knn_handle h, int64_t k, float *D_dev, int64_t *I_dev)
{
    if (!h) return set_err(KNN_ERR_INVALID, "search_self: null handle");
    if (h->ntotal == 0) return 0;
    int rc = check_search_args(h, D_dev, h->ntotal, k, D_dev, I_dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    hipStream_t s = h->stream;
    h->last_ms = -1.f;
    rc = self_search_symmetric(h, (int)k, D_dev, I_dev, s);
    if (rc < 0) return rc;
    if (rc == 1) {
        bool failed = false;
        rc = wait_search(h, s, &failed);
        if (rc) return rc;
        if (!failed) return 0;
    }
    const int64_t QB = 16384;
    BatchScope scope(h, h->ntotal);
    for (int64_t b0 = 0; b0 < h->ntotal; b0 += QB) {
        const int64_t m = std::min(QB, h->ntotal - b0);
        for (int attempt = 0; attempt < 2; attempt++) { // (statistical seed first, plain if its verification fails)
            rc = search_keys_impl(h, h->xb + (size_t)b0 * h->dp, m, (int)k, 0, nullptr, D_dev + b0 * k, I_dev + b0 * k, attempt == 0, s);
            if (rc) return rc;
            bool failed = false;
            rc = wait_search(h, s, &failed);
            if (rc) return rc;
            if (!failed) break;
        }
    }
    return 0;
}

extern "C" int knn_flat_normalize_rows(knn_handle h)
{
    if (!h) return set_err(KNN_ERR_INVALID, "normalize_rows: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->is_view) return set_err(KNN_ERR_INVALID, "normalize_rows: a view is read-only");
    if (h->ntotal == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    int rc = normalize_dev_impl(h->xb, h->ntotal, h->d, h->dp, h->stream);
    if (rc) return rc;
    rc = norms_dev_impl(h->xb, h->ntotal, h->d, h->dp, h->yn, h->stream);
    if (rc) return rc;
    rc = approx16_sync_rows(h, 0, h->ntotal, h->stream);
    if (rc) return rc;
    rc = scan16_sync_rows(h, 0, h->ntotal, h->stream); // (the rows changed: copies and statistics from scratch)
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return 0;
}

