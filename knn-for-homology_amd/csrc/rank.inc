// rank.inc -- one stable order over every hit of a result set (included by knn355_lib.hip behind pr_curve.inc).
//
// The reference's dataset-wide curves order the whole result set at once on the host: pfam/pfam.py:561-598 (argsort of the
// flattened scores, the running sum of `correct` in that order, searchsorted at 10 000 recall levels), the cumulative
// curves is_correct[argsort(key)].cumsum() (cath/cath.py:656-675, 738-771; pfam/pfam.py:166-177, 213-236) and
// numpy.quantile over every score (pfam/proteins.py:626-648).  All three are one primitive: a stable sort of the
// flattened scores[:, :limit] that carries the `correct` flag, and look-ups into the sorted sequence.  The contract is
// above knn_eval_rank in include/knn355.h; the sizes are plan_rank's (plan.h).
//
// The sort is a least-significant-digit radix sort, 8 bits per pass, on (key, payload) pairs that stay resident:
//   key      the order-preserving unsigned image of the score (rank_image: -0.0 -> +0.0, every NaN -> all ones,
//            `descending` complements the image of everything but NaN); 32 bits for float32, 64 for float64
//   payload  flat position p = row * limit + column in bits 1..31, the `correct` flag in bit 0 (N <= 2^31 - 1)
//   rank_hist_kernel     one read of the scores: the digit histogram of every pass at once.  A pass in which one bin
//                        holds all N keys moves nothing and is skipped (the host reads the histograms back).
//   per pass, for tiles of RANK_TILE = 2048 consecutive elements, one workgroup of 256 threads per tile:
//   rank_count_kernel    the tile's digit counts into table[digit][tile]
//   the scan below       the exclusive scan of the table in digit-major order: where each tile's run of each digit starts
//   rank_scatter_kernel  wave w of the tile takes elements [512 w, 512 w + 512) in 8 rounds of 64.  In a round a lane
//                        finds the lanes of its wave with the same digit by bit matching (8 ballots); its rank is the
//                        wave's running count of the digit in LDS plus the matching lanes below it, and the highest
//                        matching lane adds the group to the running count (a wave's counts are its own: the rounds are
//                        ordered inside the wave, without workgroup barriers).  The four waves' counts are then scanned
//                        through LDS on top of the table's entry, and every element goes to base + rank: the order of
//                        equal digits is the order of the input, so the whole sort is stable.
//   The first pass that runs builds keys and payloads from the scores and flags themselves (the strided read of
//   scores[:, :limit] is fused into it); later passes ping-pong between two pairs of buffers.  With limit <= k / 2 the
//   host packs the first `limit` columns before the upload, so that at most twice the bytes needed ever travel.
// The scan (rank_scan_*_kernel) is two-level over blocks of RANK_SCAN_BLOCK = 1024 entries: block sums, one workgroup
// that scans the block sums RANK_SCAN_TOP = 256 at a time with a carry, then each block scans its entries on top of its
// sum.  The same three kernels give C(r), the inclusive running count of bit 0 of the sorted payloads.
// No workgroup waits on another one: every dependency is a kernel boundary.  Atomics are atomicAdd on LDS and, in
// rank_hist_kernel, on global memory.

template <typename K> struct RankFloat { typedef float F; };
template <> struct RankFloat<uint64_t> { typedef double F; };

template <typename K>
__device__ __forceinline__ K rank_image(typename RankFloat<K>::F v, int desc)
{
    const K top = (K)1 << (8 * sizeof(K) - 1), all = ~(K)0;
    if (v != v) return all; // every NaN: last, ascending or descending
    K u;
    __builtin_memcpy(&u, &v, sizeof(u));
    if (u == top) u = 0; // -0.0 == +0.0
    const K img = (u & top) ? ~u : (u | top);
    return desc ? ~img : img; // (img is never 0 for a non-NaN, so ~img is never all ones)
}

template <typename K> struct RankSrc {
    const typename RankFloat<K>::F *scores; // the device copy, [rows][k]: k is its row stride (RankPlan::dev_k)
    const uint8_t *correct;                 // likewise, or null
    uint32_t k, limit;
    int desc;
};

template <typename K>
__device__ __forceinline__ size_t rank_cell(const RankSrc<K> &s, uint32_t p)
{
    const uint32_t row = p / s.limit, col = p - row * s.limit;
    return (size_t)row * s.k + col;
}

template <typename K>
__device__ __forceinline__ void rank_build(const RankSrc<K> &s, uint32_t p, K &key, uint32_t &pay)
{
    const size_t cell = rank_cell(s, p);
    key = rank_image<K>(s.scores[cell], s.desc);
    pay = (p << 1) | ((s.correct && s.correct[cell]) ? 1u : 0u);
}

template <typename K>
__global__ __launch_bounds__(256) void rank_hist_kernel(RankSrc<K> src, uint32_t n, unsigned int *hist /* [sizeof(K)][256] */)
{
    constexpr int P = (int)sizeof(K);
    __shared__ unsigned int s_h[P * 256];
    const int tid = threadIdx.x;
    for (int i = tid; i < P * 256; i += 256) s_h[i] = 0;
    __syncthreads();
    for (uint64_t p = (uint64_t)blockIdx.x * 256 + tid; p < n; p += (uint64_t)gridDim.x * 256) {
        K key;
        uint32_t pay;
        rank_build(src, (uint32_t)p, key, pay);
#pragma unroll
        for (int b = 0; b < P; b++) atomicAdd(&s_h[b * 256 + (int)((key >> (8 * b)) & 255)], 1u);
    }
    __syncthreads();
    for (int i = tid; i < P * 256; i += 256)
        if (s_h[i]) atomicAdd(&hist[i], s_h[i]);
}

template <typename K, bool FIRST>
__global__ __launch_bounds__(256) void rank_count_kernel(RankSrc<K> src, const K *__restrict__ kin, uint32_t n, uint32_t ntiles, int shift,
                                                         uint32_t *__restrict__ table)
{
    __shared__ unsigned int s_h[256];
    const int tid = threadIdx.x;
    s_h[tid] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)RANK_TILE;
#pragma unroll
    for (int j = 0; j < RANK_TILE / 256; j++) {
        const uint32_t p = base + j * 256 + tid;
        if (p < n) {
            K key;
            uint32_t pay;
            if (FIRST) rank_build(src, p, key, pay);
            else key = kin[p];
            atomicAdd(&s_h[(int)((key >> shift) & 255)], 1u);
        }
    }
    __syncthreads();
    table[(size_t)tid * ntiles + blockIdx.x] = s_h[tid];
}

template <typename K, bool FIRST>
__global__ __launch_bounds__(256) void rank_scatter_kernel(RankSrc<K> src, const K *__restrict__ kin, const uint32_t *__restrict__ pin,
                                                           K *__restrict__ kout, uint32_t *__restrict__ pout,
                                                           const uint32_t *__restrict__ table, uint32_t n, uint32_t ntiles, int shift)
{
    constexpr int ROUNDS = RANK_TILE / 256; // rounds of 64 elements per wave
    __shared__ uint32_t s_cnt[4][256];      // per wave: the digit's count so far; in the end, where its run starts
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < 4 * 256; i += 256) (&s_cnt[0][0])[i] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)RANK_TILE + wave * (ROUNDS * 64);
    K key[ROUNDS];
    uint32_t pay[ROUNDS], rank[ROUNDS];
#pragma unroll
    for (int j = 0; j < ROUNDS; j++) {
        const uint32_t p = base + j * 64 + lane;
        const bool valid = p < n;
        key[j] = 0;
        pay[j] = 0;
        if (valid) {
            if (FIRST) rank_build(src, p, key[j], pay[j]);
            else {
                key[j] = kin[p];
                pay[j] = pin[p];
            }
        }
        const int d = (int)((key[j] >> shift) & 255);
        uint64_t same = __ballot(valid); // the valid lanes of this wave with this lane's digit
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const uint64_t m = __ballot((d >> b) & 1);
            same &= ((d >> b) & 1) ? m : ~m;
        }
        // s_cnt[wave] belongs to this wave alone, and a wave's LDS accesses complete in program order: the read below comes
        // behind the previous round's update and in front of this round's without a workgroup barrier.  The fences keep the
        // compiler from moving either across the other lanes' accesses.
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t before = s_cnt[wave][d];
        rank[j] = before + ballot_rank(same);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (valid && (same >> lane) == 1) s_cnt[wave][d] = before + (uint32_t)__builtin_popcountll(same); // (the highest lane of the group)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads(); // the four waves' counts are complete
    {
        uint32_t run = table[(size_t)tid * ntiles + blockIdx.x]; // thread = digit
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t c = s_cnt[w][tid];
            s_cnt[w][tid] = run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < ROUNDS; j++) {
        const uint32_t p = base + j * 64 + lane;
        if (p < n) {
            const uint32_t dst = s_cnt[wave][(int)((key[j] >> shift) & 255)] + rank[j];
            if (dst < n) { // (always, when the table is this input's: a store never leaves the buffers)
                kout[dst] = key[j];
                pout[dst] = pay[j];
            }
        }
    }
}

// workgroup of 256: the sum of v over the threads below this one, and the sum over all of them in *total.  s_w is an LDS
// array [2][4] and par the set to write (0 at first): one barrier per call, as wg_compact
__device__ __forceinline__ uint32_t rank_wg_exscan(uint32_t v, uint32_t (*s_w)[4], int &par, uint32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = __shfl_up(inc, off, 64);
        if (lane >= off) inc += u;
    }
    if (lane == 63) s_w[par][wave] = inc;
    __syncthreads();
    uint32_t below = 0, all = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint32_t t = s_w[par][w];
        below += w < wave ? t : 0;
        all += t;
    }
    par ^= 1;
    *total = all;
    return below + inc - v;
}

// FLAGS: an entry is bit `bit` of the word (bit 0 of the sorted payloads; a column of windows.inc's masks), else the word
// itself (the count table)
template <bool FLAGS>
__global__ __launch_bounds__(256) void rank_scan_reduce_kernel(const uint32_t *__restrict__ src, uint64_t m, int bit, uint32_t *__restrict__ partial)
{
    __shared__ uint32_t s_w[2][4];
    const uint64_t i0 = (uint64_t)blockIdx.x * RANK_SCAN_BLOCK + (uint64_t)threadIdx.x * (RANK_SCAN_BLOCK / 256);
    uint32_t s = 0;
#pragma unroll
    for (int u = 0; u < RANK_SCAN_BLOCK / 256; u++)
        if (i0 + u < m) s += FLAGS ? ((src[i0 + u] >> bit) & 1u) : src[i0 + u];
    int par = 0;
    uint32_t total;
    (void)rank_wg_exscan(s, s_w, par, &total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup: partial[0 .. nb) becomes its own exclusive scan
__global__ __launch_bounds__(256) void rank_scan_top_kernel(uint32_t *partial, uint32_t nb)
{
    __shared__ uint32_t s_w[2][4];
    int par = 0;
    uint32_t carry = 0;
    for (uint32_t c0 = 0; c0 < nb; c0 += RANK_SCAN_TOP) {
        const uint32_t i = c0 + threadIdx.x;
        const uint32_t v = i < nb ? partial[i] : 0;
        uint32_t total;
        const uint32_t ex = rank_wg_exscan(v, s_w, par, &total);
        if (i < nb) partial[i] = ex + carry;
        carry += total;
    }
}

// FLAGS: dst[i] = the inclusive running count of the flags; else dst[i] = the exclusive running sum (dst may be src)
template <bool FLAGS>
__global__ __launch_bounds__(256) void rank_scan_apply_kernel(const uint32_t *src, uint64_t m, int bit, const uint32_t *__restrict__ partial, uint32_t *dst)
{
    __shared__ uint32_t s_w[2][4];
    const uint64_t i0 = (uint64_t)blockIdx.x * RANK_SCAN_BLOCK + (uint64_t)threadIdx.x * (RANK_SCAN_BLOCK / 256);
    uint32_t v[RANK_SCAN_BLOCK / 256], s = 0;
#pragma unroll
    for (int u = 0; u < RANK_SCAN_BLOCK / 256; u++) {
        v[u] = 0;
        if (i0 + u < m) v[u] = FLAGS ? ((src[i0 + u] >> bit) & 1u) : src[i0 + u];
        s += v[u];
    }
    int par = 0;
    uint32_t total;
    uint32_t run = rank_wg_exscan(s, s_w, par, &total) + partial[blockIdx.x];
#pragma unroll
    for (int u = 0; u < RANK_SCAN_BLOCK / 256; u++) {
        if (FLAGS) run += v[u];
        if (i0 + u < m) dst[i0 + u] = run;
        if (!FLAGS) run += v[u];
    }
}

__global__ __launch_bounds__(256) void rank_order_kernel(const uint32_t *__restrict__ pay, uint32_t n, int64_t *__restrict__ order)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) order[i] = (int64_t)(pay[i] >> 1);
}

__global__ __launch_bounds__(256) void rank_widen_kernel(const uint32_t *__restrict__ c, uint32_t n, int64_t *__restrict__ cum)
{
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) cum[i] = (int64_t)c[i];
}

// idx[j] = the first r with C(r) >= targets[j] (0 for a target <= 0, n when no r has it); cum_at[j] = C(min(idx[j], n - 1))
__global__ __launch_bounds__(256) void rank_targets_kernel(const uint32_t *__restrict__ c, uint32_t n, const int64_t *__restrict__ targets, int64_t nt,
                                                           int64_t *__restrict__ idx, int64_t *__restrict__ cum_at)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nt) return;
    const int64_t t = targets[j];
    const int64_t lo = t <= 0 ? 0 : lower_bound_dev((int64_t)0, (int64_t)n, [&](int64_t i) { return (int64_t)c[i] < t; });
    idx[j] = lo;
    cum_at[j] = (int64_t)c[lo < (int64_t)n ? lo : (int64_t)n - 1];
}

// out[j] = the score, bits untouched, of the element of rank ranks[j] (the host has checked 0 <= ranks[j] < n)
template <typename K>
__global__ __launch_bounds__(256) void rank_gather_kernel(RankSrc<K> src, const uint32_t *__restrict__ pay, const int64_t *__restrict__ ranks, int64_t nr,
                                                          typename RankFloat<K>::F *__restrict__ out)
{
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= nr) return;
    out[j] = src.scores[rank_cell(src, pay[ranks[j]] >> 1)];
}

// ---- host -------------------------------------------------------------------------------
// measurement (tools/bench_rank.py): how this thread's last successful knn_eval_rank ran
// host clock: allocations, packing; HIP events (the clock's phases): upload, sort, scan of the flags, look-ups and downloads
enum { RANK_ALLOC, RANK_PACK, RANK_UP, RANK_SORT, RANK_SCAN, RANK_LOOKUPS, RANK_PHASES };
static thread_local struct {
    int32_t passes_run, passes_skipped;
    int64_t tiles;
    float ms[RANK_PHASES];
} g_rank_info = {0, 0, 0, {0, 0, 0, 0, 0, 0}};

// table[0 .. m) becomes its exclusive scan (FLAGS = false, dst = src), or dst[i] = the running count of bit `bit` of src
// (FLAGS = true: C(i) from bit 0 of the payloads)
template <bool FLAGS>
static int rank_scan(const uint32_t *src, uint64_t m, uint32_t *partial, uint32_t *dst, int bit = 0)
{
    const uint32_t nb = (uint32_t)((m + RANK_SCAN_BLOCK - 1) / RANK_SCAN_BLOCK);
    hipLaunchKernelGGL(rank_scan_reduce_kernel<FLAGS>, dim3(nb), dim3(256), 0, 0, src, m, bit, partial);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rank_scan_top_kernel, dim3(1), dim3(256), 0, 0, partial, nb);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(rank_scan_apply_kernel<FLAGS>, dim3(nb), dim3(256), 0, 0, src, m, bit, (const uint32_t *)partial, dst);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <typename K, bool FIRST>
static int rank_pass(const RankSrc<K> &src, const K *kin, const uint32_t *pin, K *kout, uint32_t *pout, uint32_t *table, uint32_t *partial,
                     const RankPlan &pl, int shift)
{
    const uint32_t n = (uint32_t)pl.n, ntiles = (uint32_t)pl.ntiles;
    hipLaunchKernelGGL((rank_count_kernel<K, FIRST>), dim3(ntiles), dim3(256), 0, 0, src, kin, n, ntiles, shift, table);
    HIP_TRY(hipGetLastError());
    EVAL_TRY(rank_scan<false>(table, (uint64_t)pl.table_entries, partial, table));
    hipLaunchKernelGGL((rank_scatter_kernel<K, FIRST>), dim3(ntiles), dim3(256), 0, 0, src, kin, pin, kout, pout, (const uint32_t *)table, n, ntiles,
                       shift);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The order itself, shared by knn_eval_rank and knn_eval_windows (windows.inc): the buffers of a RankPlan that the sort
// needs, and what the sort leaves in them.
template <typename K> struct RankSorted {
    typename RankFloat<K>::F *d_scores = nullptr;
    uint8_t *d_correct = nullptr;
    K *d_k0 = nullptr, *d_k1 = nullptr;
    uint32_t *d_p0 = nullptr, *d_p1 = nullptr, *d_table = nullptr, *d_partial = nullptr;
    unsigned int *d_hist = nullptr;
    RankSrc<K> src;                // the device copy of the input
    const K *keys = nullptr;       // the sorted keys (order-preserving images)
    const uint32_t *pay = nullptr; // the sorted payloads
    int nrun = 0;                  // passes run
    std::chrono::steady_clock::time_point t_pack, t_up;
};

// scores, correct, two key and two payload buffers, table, block sums, histograms: by the plan's own sizes
template <typename K>
static int rank_alloc(EvalBufs &bufs, const RankPlan &pl, RankSorted<K> &rs)
{
    typedef typename RankFloat<K>::F F;
    EVAL_ALLOC(d_scores, F *, pl.scores_bytes);
    uint8_t *d_correct = nullptr;
    if (pl.correct_bytes) {
        d_correct = (uint8_t *)bufs.get(pl.correct_bytes);
        if (!d_correct) return set_err(KNN_ERR_HIP, "eval: out of device memory");
    }
    EVAL_ALLOC(d_k0, K *, pl.keys_bytes);
    EVAL_ALLOC(d_k1, K *, pl.keys_bytes);
    EVAL_ALLOC(d_p0, uint32_t *, pl.pay_bytes);
    EVAL_ALLOC(d_p1, uint32_t *, pl.pay_bytes);
    EVAL_ALLOC(d_table, uint32_t *, pl.table_bytes);
    EVAL_ALLOC(d_partial, uint32_t *, pl.partial_bytes);
    EVAL_ALLOC(d_hist, unsigned int *, pl.hist_bytes);
    rs.d_scores = d_scores;
    rs.d_correct = d_correct;
    rs.d_k0 = d_k0;
    rs.d_k1 = d_k1;
    rs.d_p0 = d_p0;
    rs.d_p1 = d_p1;
    rs.d_table = d_table;
    rs.d_partial = d_partial;
    rs.d_hist = d_hist;
    return 0;
}

// packs, uploads and sorts.  On the clock the upload is an interval of up_phase (it ends whatever interval the caller has
// open), the sort one of sort_phase, and the event behind the sort starts one of then_phase
template <typename K>
static int rank_sort(const void *scores, int64_t rows, int64_t k, int64_t limit, const uint8_t *correct, int desc, const RankPlan &pl, PhaseClock &clock,
                     int up_phase, int sort_phase, int then_phase, RankSorted<K> &rs)
{
    typedef typename RankFloat<K>::F F;
    constexpr int P = (int)sizeof(K);
    const uint32_t n = (uint32_t)pl.n;
    F *d_scores = rs.d_scores;
    uint8_t *d_correct = rs.d_correct;
    uint32_t *d_table = rs.d_table, *d_partial = rs.d_partial;
    unsigned int *d_hist = rs.d_hist;
    rs.t_pack = std::chrono::steady_clock::now();
    // limit <= k / 2: the first `limit` columns of every row, packed on the host, are all that travels
    const F *up_scores = (const F *)scores;
    const uint8_t *up_correct = correct;
    std::vector<F> packed_scores;
    std::vector<uint8_t> packed_correct;
    if (pl.pack) {
        packed_scores.resize((size_t)pl.n);
        if (correct) packed_correct.resize((size_t)pl.n);
#pragma omp parallel for schedule(static)
        for (int64_t r = 0; r < rows; r++) {
            memcpy(packed_scores.data() + (size_t)r * limit, (const F *)scores + (size_t)r * k, (size_t)limit * sizeof(F));
            if (correct) memcpy(packed_correct.data() + (size_t)r * limit, correct + (size_t)r * k, (size_t)limit);
        }
        up_scores = packed_scores.data();
        if (correct) up_correct = packed_correct.data();
    }
    rs.t_up = std::chrono::steady_clock::now();
    EVAL_TRY(clock.next(up_phase, nullptr));
    HIP_TRY(hipMemcpy(d_scores, up_scores, pl.scores_bytes, hipMemcpyHostToDevice));
    if (correct) HIP_TRY(hipMemcpy(d_correct, up_correct, pl.correct_bytes, hipMemcpyHostToDevice));
    EVAL_TRY(clock.next(sort_phase, nullptr));
    const RankSrc<K> src = {d_scores, d_correct, (uint32_t)pl.dev_k, (uint32_t)limit, desc};
    // ---- the sort
    HIP_TRY(hipMemset(d_hist, 0, pl.hist_bytes));
    hipLaunchKernelGGL(rank_hist_kernel<K>, dim3((unsigned)std::min<int64_t>(RANK_HIST_GRID, (pl.n + 255) / 256)), dim3(256), 0, 0, src, n, d_hist);
    HIP_TRY(hipGetLastError());
    std::vector<unsigned int> hist((size_t)P * 256);
    HIP_TRY(hipMemcpy(hist.data(), d_hist, hist.size() * 4, hipMemcpyDeviceToHost));
    bool run[P];
    int nrun = 0;
    for (int b = 0; b < P; b++) {
        run[b] = true;
        for (int d = 0; d < 256; d++)
            if (hist[(size_t)b * 256 + d] == n) run[b] = false; // one digit everywhere: the pass would move nothing
        nrun += run[b] ? 1 : 0;
    }
    if (!nrun) { // (all keys equal) one pass still builds the keys and payloads
        run[0] = true;
        nrun = 1;
    }
    K *kin = nullptr, *kout = rs.d_k0, *kspare = rs.d_k1;
    uint32_t *pin = nullptr, *pout = rs.d_p0, *pspare = rs.d_p1;
    bool first = true;
    for (int b = 0; b < P; b++) {
        if (!run[b]) continue;
        if (first) EVAL_TRY((rank_pass<K, true>(src, kin, pin, kout, pout, d_table, d_partial, pl, 8 * b)));
        else EVAL_TRY((rank_pass<K, false>(src, kin, pin, kout, pout, d_table, d_partial, pl, 8 * b)));
        first = false;
        kin = kout;
        pin = pout;
        std::swap(kout, kspare);
        std::swap(pout, pspare);
    }
    rs.src = src;
    rs.keys = kin;
    rs.pay = pin;
    rs.nrun = nrun;
    EVAL_TRY(clock.next(then_phase, nullptr));
    return 0;
}

template <typename K>
static int rank_run(const void *scores, int64_t rows, int64_t k, int64_t limit, const uint8_t *correct, int desc, const RankPlan &pl,
                    int64_t *order_out, int64_t *cum_out, const int64_t *targets, int64_t nt, int64_t *idx_out, int64_t *cum_at_out,
                    const int64_t *ranks, int64_t nr, void *sorted_at_out)
{
    typedef typename RankFloat<K>::F F;
    constexpr int P = (int)sizeof(K);
    const uint32_t n = (uint32_t)pl.n;
    const bool want_c = pl.cum_bytes != 0;
    // every buffer of the plan, by the plan's own sizes (plan_rank; plan_check walks them)
    const auto t_alloc = std::chrono::steady_clock::now();
    EvalBufs bufs;
    PhaseClock clock;
    RankSorted<K> rs;
    EVAL_TRY(rank_alloc<K>(bufs, pl, rs));
    uint32_t *d_c = nullptr;
    if (want_c) {
        d_c = (uint32_t *)bufs.get(pl.cum_bytes);
        if (!d_c) return set_err(KNN_ERR_HIP, "eval: out of device memory");
    }
    int64_t *d_wide = nullptr; // order, then cum: one buffer
    if (pl.wide_bytes) {
        d_wide = (int64_t *)bufs.get(pl.wide_bytes);
        if (!d_wide) return set_err(KNN_ERR_HIP, "eval: out of device memory");
    }
    size_t allocated = 0;
    for (const auto &b : bufs.dev) allocated += b.second;
    if (allocated != pl.resident_bytes) return set_err(KNN_ERR_INVALID, "rank: the buffers are not the plan's");
    EVAL_TRY(rank_sort<K>(scores, rows, k, limit, correct, desc, pl, clock, RANK_UP, RANK_SORT, RANK_SCAN, rs));
    const auto t_pack = rs.t_pack, t_up = rs.t_up;
    const RankSrc<K> src = rs.src;
    uint32_t *d_partial = rs.d_partial;
    const uint32_t *d_pay = rs.pay; // the sorted payloads
    const int nrun = rs.nrun;
    // ---- C(r)
    if (want_c) EVAL_TRY(rank_scan<true>(d_pay, (uint64_t)n, d_partial, d_c));
    EVAL_TRY(clock.next(RANK_LOOKUPS, nullptr));
    // ---- look-ups
    const unsigned wide_grid = (unsigned)std::min<int64_t>(65536, (pl.n + 255) / 256);
    if (order_out) {
        hipLaunchKernelGGL(rank_order_kernel, dim3(wide_grid), dim3(256), 0, 0, d_pay, n, d_wide);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(order_out, d_wide, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    if (cum_out) {
        hipLaunchKernelGGL(rank_widen_kernel, dim3(wide_grid), dim3(256), 0, 0, (const uint32_t *)d_c, n, d_wide);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(cum_out, d_wide, (size_t)n * 8, hipMemcpyDeviceToHost));
    }
    if (nt > 0) {
        EVAL_ALLOC(d_t, int64_t *, (size_t)nt * 8);
        EVAL_ALLOC(d_idx, int64_t *, (size_t)nt * 8);
        EVAL_ALLOC(d_at, int64_t *, (size_t)nt * 8);
        HIP_TRY(hipMemcpy(d_t, targets, (size_t)nt * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(rank_targets_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, 0, (const uint32_t *)d_c, n, (const int64_t *)d_t, nt,
                           d_idx, d_at);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(idx_out, d_idx, (size_t)nt * 8, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(cum_at_out, d_at, (size_t)nt * 8, hipMemcpyDeviceToHost));
    }
    if (nr > 0) {
        EVAL_ALLOC(d_r, int64_t *, (size_t)nr * 8);
        EVAL_ALLOC(d_at, F *, (size_t)nr * sizeof(F));
        HIP_TRY(hipMemcpy(d_r, ranks, (size_t)nr * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(rank_gather_kernel<K>, dim3((unsigned)((nr + 255) / 256)), dim3(256), 0, 0, src, d_pay, (const int64_t *)d_r, nr, d_at);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpy(sorted_at_out, d_at, (size_t)nr * sizeof(F), hipMemcpyDeviceToHost));
    }
    EVAL_TRY(clock.close(nullptr));
    HIP_TRY(hipDeviceSynchronize());
    float ms[RANK_PHASES];
    EVAL_TRY(clock.read(ms, RANK_PHASES));
    ms[RANK_ALLOC] = std::chrono::duration<float, std::milli>(t_pack - t_alloc).count();
    ms[RANK_PACK] = std::chrono::duration<float, std::milli>(t_up - t_pack).count();
    memcpy(g_rank_info.ms, ms, sizeof ms);
    g_rank_info.passes_run = nrun;
    g_rank_info.passes_skipped = P - nrun;
    g_rank_info.tiles = pl.ntiles;
    return 0;
}

extern "C" int knn_eval_rank(const void *scores, int32_t key_type, int64_t rows, int64_t k, int64_t limit, const uint8_t *correct,
                             int32_t descending, int64_t *order_out, int64_t *cum_out, const int64_t *targets, int64_t nt, int64_t *idx_out,
                             int64_t *cum_at_out, const int64_t *ranks, int64_t nr, void *sorted_at_out)
{
    if (key_type != KNN_RANK_F32 && key_type != KNN_RANK_F64) return set_err(KNN_ERR_INVALID, "rank: unknown key type");
    if (rows < 1) return set_err(KNN_ERR_INVALID, "rank: need rows >= 1");
    if (k < 1) return set_err(KNN_ERR_INVALID, "rank: need k >= 1");
    if (eval_k_too_large(k)) return set_err(KNN_ERR_INVALID, "rank: k > INT32_MAX");
    if (limit < 1 || limit > k) return set_err(KNN_ERR_INVALID, "rank: limit outside [1, k]");
    RankPlan pl;
    if (!plan_rank(rows, k, limit, key_type == KNN_RANK_F64 ? 8 : 4, correct != nullptr, correct && (cum_out || nt > 0), order_out || cum_out, &pl))
        return set_err(KNN_ERR_INVALID, "rank: rows * limit > 2^31 - 1, or rows * k too large");
    if (nt < 0 || nt > INT32_MAX) return set_err(KNN_ERR_INVALID, "rank: nt outside [0, INT32_MAX]");
    if (nr < 0 || nr > INT32_MAX) return set_err(KNN_ERR_INVALID, "rank: nr outside [0, INT32_MAX]");
    if (!scores) return set_err(KNN_ERR_INVALID, "rank: null pointer");
    if (nt > 0 && (!targets || !idx_out || !cum_at_out)) return set_err(KNN_ERR_INVALID, "rank: null pointer");
    if (nr > 0 && (!ranks || !sorted_at_out)) return set_err(KNN_ERR_INVALID, "rank: null pointer");
    if ((cum_out || nt > 0) && !correct) return set_err(KNN_ERR_INVALID, "rank: cum and targets need correct");
    for (int64_t j = 0; j < nr; j++)
        if (ranks[j] < 0 || ranks[j] >= pl.n) return set_err(KNN_ERR_INVALID, "rank: a rank outside [0, N)");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    if (key_type == KNN_RANK_F64)
        return rank_run<uint64_t>(scores, rows, k, limit, correct, descending != 0, pl, order_out, cum_out, targets, nt, idx_out, cum_at_out, ranks, nr,
                                  sorted_at_out);
    return rank_run<uint32_t>(scores, rows, k, limit, correct, descending != 0, pl, order_out, cum_out, targets, nt, idx_out, cum_at_out, ranks, nr,
                              sorted_at_out);
}

extern "C" int knn_last_rank_info(int32_t *passes_run, int32_t *passes_skipped, int64_t *tiles, float *ms)
{
    if (!passes_run || !passes_skipped || !tiles || !ms) return set_err(KNN_ERR_INVALID, "last_rank_info: null pointer");
    *passes_run = g_rank_info.passes_run;
    *passes_skipped = g_rank_info.passes_skipped;
    *tiles = g_rank_info.tiles;
    for (int i = 0; i < RANK_PHASES; i++) ms[i] = g_rank_info.ms[i];
    return 0;
}
