// lsh.inc -- faiss.IndexLSH on MI355X (included by knn355_lib.hip).
//
// Reference call sites: seqvec_search/create_index.py:41-45 (IndexLSH(d, param), train, add),
// pfam/search.py:27-37 (1024 bits, search k = 1000), pfam/proteins_search.py:25-26 (2048 bits).
// FAISS 1.7.2's IndexLSH (not in the reference tree; published behaviour restated): rows are
// multiplied by a fixed random orthonormal matrix (nbits x d), bit j of the code is
// (x . a_j >= 0), codes are compared by Hamming distance, search returns the k smallest
// distances as float32 (ties: lower id first here).  FAISS draws its matrix from its own RNG,
// so codes are not bit-compatible with FAISS; the matrix is supplied by the caller.
//
// IndexLSH(d, nbits, rotate_data, train_thresholds = true) (FAISS 1.7.2 IndexLSH::train, restated from the published
// source as well): train() projects the training rows without thresholds and takes, per bit, the median of that
// bit's projections -- s[n/2] of the sorted column for odd n, (s[n/2 - 1] + s[n/2]) / 2 in float for even n; bit j of
// a code is then (x . a_j - t_j >= 0).
//
//   lsh_encode_kernel    MFMA projection of 128 rows x 128 bits per workgroup, bits (acc - threshold >= 0) packed
//                        with one ballot per accumulator register
//   lsh_project_kernel   the same projection (lsh_project_tile: one K loop for both), accumulators stored
//                        transposed as P[bit][row] for the training
//   lsh_median_kernel    one workgroup per bit: exact order statistics n/2 - 1 and n/2 of a column of P by an
//                        MSB-first radix select over the order-preserving uint32 image of the floats
//   hamming_scan_kernel  one thread per database row: XOR + popcount against 32 query codes held
//                        in LDS, same candidate lists / thresholds / wave_select as the flat scan

// the phases of knn_lsh_train: the slabs' uploads, their projections, the median selection
enum { LSH_TRAIN_UP, LSH_TRAIN_PROJECT, LSH_TRAIN_SELECT, LSH_TRAIN_PHASES };
struct knn_lsh_s {
    int d = 0, dp = 0, nbits = 0, W = 0; // W: 64-bit words per code (nbits padded up to 128 * 2^i)
    int device = 0;
    int64_t ntotal = 0, cap_rows = 0;
    float *rot = nullptr;      // [W*64][dp] rotation rows (zero rows pad the tail)
    float *thr = nullptr;      // [W*64] per-bit thresholds (zeros pad the tail: padding bits stay 1), or null: none
    float train_ms[LSH_TRAIN_PHASES] = {0, 0, 0}; // of the last successful knn_lsh_train (HIP events)
    uint64_t *codes = nullptr; // [cap_rows][W]
    hipStream_t stream = nullptr;
    std::mutex mu;
    DevBuf ws_x, ws_xp, ws_q, ws_lists, ws_gthr, ws_qlist, ws_qcnt, ws_D, ws_I, ws_D2, ws_I2, ws_cD, ws_cI; // (ws_D2 / ws_I2: second result set of a search of several batches; ws_cD / ws_cI: the Hamming hits a refined search re-scores)
};

struct LshEncodeParams {
    const float *x;   // [n][dp]
    const float *rot; // [W*64][dp]
    int64_t n;
    int dp, W;
    int nbits;         // code bits that exist; the bits from there up to W*64 are padding (lsh_encode_kernel)
    uint32_t *codes32; // [n][2W]                       (lsh_encode_kernel)
    const float *thr;  // [W*64] thresholds, or null     (lsh_encode_kernel)
    float *proj;       // [W*64][ldp], whole 128-row tiles (lsh_project_kernel)
    int64_t ldp;
};

// The projection of one 128-row x 128-bit tile: the K loop shared by lsh_encode_kernel and lsh_project_kernel, so that
// the training sees the very accumulators the encoder compares (same staging, same swizzle, same MFMA order).
// acc[a][b]: lane = bit (bit0 + (wn * 2 + b) * 32 + li), register r = row (row0 + (wm * 2 + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh)
__device__ __forceinline__ void lsh_project_tile(const LshEncodeParams &p, const int64_t row0, const int bit0, char *smem, f32x16 (&acc)[2][2])
{
    constexpr int NR = 256; // 128 data rows + 128 rotation rows per K step
    constexpr int STAGE_BYTES = NR * 128;
    char *stage0 = smem, *stage1 = smem + STAGE_BYTES;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const float *srcp[8];
    int lds_off[8];
#pragma unroll
    for (int nn = 0; nn < 8; nn++) {
        const int ii = wave + 4 * nn;
        const int row_local = 8 * ii + (lane >> 3);
        const int sp = lane & 7;
        lds_off[nn] = ii * 1024;
        if (row_local < 128) {
            const int s = sp ^ ((row_local >> 1) & 7);
            srcp[nn] = p.x + (size_t)min(row0 + row_local, p.n - 1) * p.dp + 4 * s;
        } else {
            const int rb = row_local - 128;
            const int s = sp ^ ((rb >> 1) & 7);
            srcp[nn] = p.rot + (size_t)(bit0 + rb) * p.dp + 4 * s;
        }
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
    const int KT = p.dp / 32;
    const int swz = (li >> 1) & 7;
#pragma unroll
    for (int nn = 0; nn < 8; nn++)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)srcp[nn],
                                         (__attribute__((address_space(3))) void *)(stage0 + lds_off[nn]), 16, 0, 0);
    for (int kt = 0; kt < KT; kt++) {
        char *cur = (kt & 1) ? stage1 : stage0;
        char *nxt = (kt & 1) ? stage0 : stage1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (this wave's staging instructions have landed -- explicit: see flat_scan_kernel's K loop)
        __syncthreads();
        if (kt + 1 < KT) {
#pragma unroll
            for (int nn = 0; nn < 8; nn++)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(srcp[nn] + (kt + 1) * 32),
                                                 (__attribute__((address_space(3))) void *)(nxt + lds_off[nn]), 16, 0, 0);
        }
        const char *A = cur, *B = cur + 128 * 128;
#pragma unroll
        for (int t = 0; t < 4; t++) {
            f32x4 af[2], bf[2];
            const int slot = ((2 * t + lh) ^ swz) * 16;
#pragma unroll
            for (int a = 0; a < 2; a++) af[a] = *(const f32x4 *)(A + ((wm * 2 + a) * 32 + li) * 128 + slot);
#pragma unroll
            for (int b = 0; b < 2; b++) bf[b] = *(const f32x4 *)(B + ((wn * 2 + b) * 32 + li) * 128 + slot);
#pragma unroll
            for (int m = 0; m < 4; m++)
#pragma unroll
                for (int a = 0; a < 2; a++)
#pragma unroll
                    for (int b = 0; b < 2; b++)
                        acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[a][m], bf[b][m], acc[a][b], 0, 0, 0);
        }
    }
}

__global__ __launch_bounds__(256, 2) void lsh_encode_kernel(LshEncodeParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int nbt = p.W / 2; // 128-bit column tiles
    const int64_t row0 = (int64_t)(blockIdx.x / nbt) * 128;
    const int bit0 = (blockIdx.x % nbt) * 128;
    f32x16 acc[2][2];
    lsh_project_tile(p, row0, bit0, smem, acc);
    // code bits: lane = bit (column), register = row; one ballot packs 32 bits of two rows.  FAISS subtracts the threshold
    // and tests the sign (x - t >= 0), and so does this: x >= t is the same predicate for FINITE operands as long as
    // denormals are kept (the fp32 default on gfx950, and the build passes no flush flag), but not when x and t are the same
    // infinity -- inf - inf is a NaN, bit 0, while inf >= inf holds -- and a threshold of +-inf is what training gives a
    // column whose middle is infinite.  Without thresholds the operand is 0.0f (x - 0 is x, NaN included: bit 0).
    // A padding bit (>= nbits) is 1 whatever the row holds: its rotation row is zero, so an ordinary row's 0 >= 0 sets it, a
    // row with a NaN or an infinity would get 0 * inf = NaN there, and two rows' Hamming distance would count bits that do
    // not exist (knn_lsh_add_codes fills the padding with ones too).
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            const int word = (bit0 >> 5) + wn * 2 + b;
            const float t = p.thr ? p.thr[word * 32 + li] : 0.0f;
            const uint64_t padm = __ballot(word * 32 + li >= p.nbits); // (once per word: a scalar OR per ballot below, nothing per lane)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const uint64_t m = __ballot(acc[a][b][r] - t >= 0.0f) | padm;
                const int64_t row = row0 + (wm * 2 + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (li == 0 && row < p.n) p.codes32[(size_t)row * (2 * p.W) + word] = lh ? (uint32_t)(m >> 32) : (uint32_t)m;
            }
        }
}

// The training's projection: the accumulators of lsh_project_tile stored transposed, P[bit][row], so that each bit's
// column is contiguous for lsh_median_kernel.  A lane holds rows 8g + 4 lh ... + 3 of its bit in registers 4g ... 4g + 3:
// one 16-byte store each (ldp and the slab offsets are multiples of 128 rows).  Whole tiles are stored: the rows of a
// partial tile beyond n repeat row n - 1 (the staging clamps) and land in the padding of P up to ldp, or in the next
// slab's rows, which that slab's launch -- later on the same stream -- overwrites.
__global__ __launch_bounds__(256, 2) void lsh_project_kernel(LshEncodeParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int li = lane & 31, lh = lane >> 5;
    const int nbt = p.W / 2;
    const int64_t row0 = (int64_t)(blockIdx.x / nbt) * 128;
    const int bit0 = (blockIdx.x % nbt) * 128;
    f32x16 acc[2][2];
    lsh_project_tile(p, row0, bit0, smem, acc);
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) {
            float *col = p.proj + (size_t)(bit0 + (wn * 2 + b) * 32 + li) * p.ldp + row0 + (wm * 2 + a) * 32 + 4 * lh;
#pragma unroll
            for (int g = 0; g < 4; g++) {
                f32x4 v;
#pragma unroll
                for (int i = 0; i < 4; i++) v[i] = acc[a][b][4 * g + i];
                *(f32x4 *)(col + 8 * g) = v;
            }
        }
}

// ---- per-bit medians ---------------------------------------------------------------------------------------------------
// One workgroup per bit column of P.  Keys: the float's bits with -0.0 mapped to +0.0 first (std::sort treats the two as
// equal; the canonical one defines the threshold's bits), then the usual order-preserving image (negative: all bits
// flipped, else the sign bit set).  Three digit passes (11 + 11 + 10 bits, MSB first) narrow the key of rank n/2: a pass
// histograms the digit of every key that carries the prefix found so far (LDS integer atomics: counts, so the result does
// not depend on their order), a workgroup scan finds the digit's bin and the rank inside it.  Ties need no special case:
// the third pass ends on the key itself, with the number of keys below it.  For even n the rank n/2 - 1 is the same key
// when fewer than n/2 keys lie below it, else the largest key below it (one more pass over the column, which by then
// sits in L2).  status[bit]: 1 a NaN projection, 2 a NaN threshold (+inf and -inf around the middle).
struct LshMedianParams {
    const float *proj; // [nbits][ldp]
    int64_t n, ldp;
    float *thr;      // [nbits]
    int32_t *status; // [nbits]
};

__device__ __forceinline__ uint32_t lsh_float_key(float v)
{
    uint32_t u = __float_as_uint(v);
    if (u == 0x80000000u) u = 0; // -0.0 -> +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float lsh_key_float(uint32_t key)
{
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

// f(key) for every key of the column: 16-byte loads (columns start on 512-byte boundaries), then the tail
template <typename F>
__device__ __forceinline__ void lsh_column_keys(const float *col, int64_t n, int tid, F f)
{
    const int64_t n4 = n >> 2;
    for (int64_t i = tid; i < n4; i += 256) {
        const f32x4 v = *(const f32x4 *)(col + 4 * i);
#pragma unroll
        for (int j = 0; j < 4; j++) f(lsh_float_key(v[j]));
    }
    const int64_t i = 4 * n4 + tid;
    if (i < n) f(lsh_float_key(col[i]));
}

// the bin that holds rank `rank` of hist[0 .. 2047], the rank inside that bin, and the count below the bin -> s_sel[0..2]
__device__ __forceinline__ void lsh_find_bin(const uint32_t *hist, uint32_t rank, uint32_t *s_wave, uint32_t *s_sel, int tid)
{
    uint32_t c[8], part = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) { c[j] = hist[tid * 8 + j]; part += c[j]; }
    const int lane = tid & 63, wave = tid >> 6;
    uint32_t incl = part;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; w++) base += s_wave[w];
    uint32_t lo = base + incl - part; // keys in the bins before this thread's
    if (rank >= lo && rank < lo + part) { // exactly one thread: the counts of all bins sum to more than rank
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (rank < lo + c[j]) { s_sel[0] = tid * 8 + j; s_sel[1] = rank - lo; s_sel[2] = lo; break; }
            lo += c[j];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void lsh_median_kernel(LshMedianParams p)
{
    __shared__ uint32_t s_hist[2048];
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_sel[3];
    __shared__ uint32_t s_flag, s_max;
    const int tid = threadIdx.x;
    const int bit = blockIdx.x;
    const float *col = p.proj + (size_t)bit * p.ldp;
    const int64_t n = p.n;
    uint32_t rank = (uint32_t)(n >> 1); // (n < 2^31: knn_lsh_train checks)
    uint32_t below = 0;                 // keys below the prefix found so far
    uint32_t prefix = 0;
    if (tid == 0) { s_flag = 0; s_max = 0; }
    // pass 1: bits 31..21 (and the NaN check), pass 2: bits 20..10, pass 3: bits 9..0
#pragma unroll 1
    for (int pass = 0; pass < 3; pass++) {
        for (int i = tid; i < 2048; i += 256) s_hist[i] = 0;
        __syncthreads();
        if (pass == 0) {
            bool nan = false;
            lsh_column_keys(col, n, tid, [&](uint32_t key) {
                // NaN images: above +inf's (0xFF800000) or below -inf's (0x007FFFFF)
                nan |= key > 0xFF800000u || key < 0x007FFFFFu;
                atomicAdd(&s_hist[key >> 21], 1u);
            });
            if (nan) s_flag = 1;
        } else if (pass == 1) {
            lsh_column_keys(col, n, tid, [&](uint32_t key) {
                if ((key >> 21) == prefix) atomicAdd(&s_hist[(key >> 10) & 0x7FFu], 1u);
            });
        } else {
            lsh_column_keys(col, n, tid, [&](uint32_t key) {
                if ((key >> 10) == prefix) atomicAdd(&s_hist[key & 0x3FFu], 1u);
            });
        }
        __syncthreads();
        lsh_find_bin(s_hist, rank, s_wave, s_sel, tid);
        prefix = (prefix << (pass == 2 ? 10 : 11)) | s_sel[0];
        rank = s_sel[1];
        below += s_sel[2];
        __syncthreads();
    }
    const uint32_t key_hi = prefix; // the key of rank n/2; `below` keys are smaller
    uint32_t key_lo = key_hi;
    if (!(n & 1) && below == (uint32_t)(n >> 1)) { // rank n/2 - 1 is the largest key below it
        uint32_t best = 0;
        lsh_column_keys(col, n, tid, [&](uint32_t key) {
            if (key < key_hi && key > best) best = key;
        });
        atomicMax(&s_max, best);
        __syncthreads();
        key_lo = s_max;
    }
    if (tid == 0) {
        float t = lsh_key_float(key_hi);
        if (!(n & 1)) t = (lsh_key_float(key_lo) + t) / 2;
        p.thr[bit] = t;
        p.status[bit] = s_flag ? 1 : (t != t ? 2 : 0);
    }
}

struct HammingParams {
    const uint64_t *codes;  // [nb][W]
    const uint64_t *qcodes; // [nq][W]
    int64_t nb, nq;
    int W, k, cap, kslot;
    int nqtiles, nchunks;
    int64_t chunk_rows;
    uint64_t *lists;
    uint32_t *gthr;
    uint64_t *qlist; // [nq][qcap] compact candidate arrays (the chunks' survivors)
    uint32_t *qcnt;  // [nq]
    int qcap;
};

template <int W>
__global__ __launch_bounds__(256, 2) void hamming_scan_kernel(HammingParams p)
{
    constexpr int QT = 32, DT = 256;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lds_main = max(max(QT * W * 8 + QT * 4, p.cap * 8), 4096);
    uint64_t *s_q = (uint64_t *)smem;             // [QT][W]
    float *s_teff = (float *)(smem + QT * W * 8); // [QT] thresholds of this tile
    const int tid = threadIdx.x;
    const int qtile = blockIdx.x % p.nqtiles, chunk = blockIdx.x / p.nqtiles;
    const int64_t q0 = (int64_t)qtile * QT;
    const int64_t c_lo = (int64_t)chunk * p.chunk_rows, c_hi = min(p.nb, c_lo + p.chunk_rows);
    ListCtx L;
    L.s_thr = (float *)(smem + lds_main);
    L.s_cnt = (int *)(L.s_thr + QT);
    L.s_need = L.s_cnt + QT;
    int *s_base = L.s_need + 4;
    L.lists = p.lists + (size_t)blockIdx.x * QT * p.cap;
    L.gthr = p.gthr + (size_t)qtile * QT;
    L.cap = p.cap;
    L.k = p.k;
    L.kslot = p.kslot;
    L.init(tid, QT);
    const int nqv = (int)min((int64_t)QT, p.nq - q0);
    for (int64_t row0 = c_lo; row0 < c_hi; row0 += DT) {
        // (re)load the query codes: the compaction fallback may have used this LDS
        for (int i = tid; i < QT * W; i += 256) {
            const int ql = i / W;
            s_q[i] = p.qcodes[(size_t)min(q0 + ql, p.nq - 1) * W + (i - ql * W)];
        }
        __syncthreads();
        if (tid < QT) s_teff[tid] = L.threshold(tid);
        __syncthreads();
        const int64_t row = row0 + tid;
        if (row < c_hi) {
            uint64_t c[W];
            const uint64_t *src = p.codes + (size_t)row * W;
#pragma unroll
            for (int w = 0; w < W; w += 2) {
                const ulonglong2 v = *(const ulonglong2 *)(src + w);
                c[w] = v.x;
                c[w + 1] = v.y;
            }
            for (int ql = 0; ql < nqv; ql++) {
                int dist = 0;
#pragma unroll
                for (int w = 0; w < W; w++) dist += __popcll(c[w] ^ s_q[ql * W + w]);
                const float v = (float)dist;
                if (v <= s_teff[ql]) L.append(ql, v, (uint32_t)row, DT);
            }
        }
        __syncthreads();
        const bool last_tile = row0 + DT >= c_hi;
        if (*L.s_need || last_tile) lists_compact<QT>(L, smem, DT, last_tile, tid);
    }
    lists_flush<QT>(L, s_base, q0, p.nq, p.qlist, p.qcnt, p.qcap, tid);
}

// ---- host -------------------------------------------------------------------------------
extern "C" int knn_lsh_create(int32_t d, int32_t nbits, const float *rotation_host, knn_lsh_s **out)
{
    if (!out || !rotation_host) return set_err(KNN_ERR_INVALID, "lsh_create: null pointer");
    if (d <= 0 || nbits <= 0 || nbits > 2048) return set_err(KNN_ERR_INVALID, "lsh_create: need d > 0 and 0 < nbits <= 2048");
    int rc = ensure_device(g_device);
    if (rc) return rc;
    knn_lsh_s *h = new knn_lsh_s();
    h->d = d;
    h->dp = round_up(d, 32);
    h->nbits = nbits;
    h->W = 2;
    while (h->W * 64 < nbits) h->W *= 2; // 128, 256, 512, 1024 or 2048 code bits; the tail is constant padding
    h->device = g_device;
    const size_t rot_rows = (size_t)h->W * 64;
    std::vector<float> padded(rot_rows * h->dp, 0.0f);
    for (int b = 0; b < nbits; b++) memcpy(&padded[(size_t)b * h->dp], rotation_host + (size_t)b * d, (size_t)d * 4);
    if (hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&h->rot, padded.size() * 4) != hipSuccess ||
        hipMemcpy(h->rot, padded.data(), padded.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        delete h;
        return set_err(KNN_ERR_HIP, "lsh_create: device allocation failed");
    }
    *out = h;
    return 0;
}

extern "C" void knn_lsh_free(knn_lsh_s *h)
{
    if (!h) return;
    if (hipSetDevice(h->device) == hipSuccess) {
        if (h->rot) (void)hipFree(h->rot);
        if (h->thr) (void)hipFree(h->thr);
        if (h->codes) (void)hipFree(h->codes);
        DevBuf *bufs[] = {&h->ws_x, &h->ws_xp, &h->ws_q, &h->ws_lists, &h->ws_gthr, &h->ws_qlist, &h->ws_qcnt, &h->ws_D, &h->ws_I, &h->ws_D2, &h->ws_I2, &h->ws_cD, &h->ws_cI};
        for (auto b : bufs) b->release();
        if (h->stream) (void)hipStreamDestroy(h->stream);
    }
    delete h;
}

extern "C" int64_t knn_lsh_ntotal(knn_lsh_s *h) { return h ? h->ntotal : -1; }
extern "C" int32_t knn_lsh_code_words(knn_lsh_s *h) { return h ? h->W : -1; }

// encodes n host rows into dst_codes (device, [n][W]) in slabs -- or, with proj given (the training), stores their
// projections into proj[W*64][ldp] instead.  With a clock (the training's; null: no event is recorded) every slab's upload
// is an LSH_TRAIN_UP interval and its kernel an LSH_TRAIN_PROJECT one.
// A slab is a whole number of 128-row tiles, so that every slab's rows start on a tile of proj.
// (xp_out: where the LAST slab's rows, zero padded to dp, stay on the device until the handle's next call)
static int64_t lsh_slab_rows(const knn_lsh_s *h) { return std::max<int64_t>(128, (int64_t)(256ull << 20) / ((int64_t)h->dp * 4) / 128 * 128); }
static int lsh_encode_host_rows(knn_lsh_s *h, const float *x_host, int64_t n, uint64_t *dst_codes, float *proj = nullptr, int64_t ldp = 0,
                                PhaseClock *clock = nullptr, const float **xp_out = nullptr)
{
    const int64_t slab = lsh_slab_rows(h);
    if (h->ws_x.ensure((size_t)std::min(n, slab) * h->d * 4) || h->ws_xp.ensure((size_t)std::min(n, slab) * h->dp * 4))
        return set_err(KNN_ERR_HIP, "lsh: out of device memory");
    hipStream_t s = h->stream;
    for (int64_t i0 = 0; i0 < n; i0 += slab) {
        const int64_t m = std::min(slab, n - i0);
        if (clock) EVAL_TRY(clock->open(LSH_TRAIN_UP, s));
        HIP_TRY(hipMemcpyAsync(h->ws_x.p, x_host + i0 * h->d, (size_t)m * h->d * 4, hipMemcpyHostToDevice, s));
        if (clock) EVAL_TRY(clock->next(LSH_TRAIN_PROJECT, s));
        const float *xp = (const float *)h->ws_x.p;
        if (h->dp != h->d) {
            int rc = pad_rows_dev((const float *)h->ws_x.p, m, h->d, (float *)h->ws_xp.p, h->dp, s);
            if (rc) return rc;
            xp = (const float *)h->ws_xp.p;
        }
        if (xp_out) *xp_out = xp;
        LshEncodeParams p;
        p.x = xp; p.rot = h->rot; p.n = m; p.dp = h->dp; p.W = h->W; p.nbits = h->nbits;
        p.codes32 = proj ? nullptr : (uint32_t *)(dst_codes + (size_t)i0 * h->W);
        p.thr = h->thr;
        p.proj = proj ? proj + i0 : nullptr;
        p.ldp = ldp;
        const unsigned grid = (unsigned)(((m + 127) / 128) * (h->W / 2));
        const size_t lds = 2 * 256 * 128;
        if (proj) {
            HIP_TRY(hipFuncSetAttribute((const void *)lsh_project_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(lsh_project_kernel, dim3(grid), dim3(256), lds, s, p);
        } else {
            HIP_TRY(hipFuncSetAttribute((const void *)lsh_encode_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(lsh_encode_kernel, dim3(grid), dim3(256), lds, s, p);
        }
        HIP_TRY(hipGetLastError());
        if (clock) EVAL_TRY(clock->close(s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return 0;
}

// installs thr_host[nbits] as the handle's thresholds (the tail up to W*64 is 0 and never decides anything: the encoder
// sets the padding bits to 1 by their index), null: none
static int lsh_install_thresholds(knn_lsh_s *h, const float *thr_host)
{
    if (!thr_host) {
        if (h->thr) {
            HIP_TRY(hipStreamSynchronize(h->stream));
            (void)hipFree(h->thr);
        }
        h->thr = nullptr;
        return 0;
    }
    std::vector<float> padded((size_t)h->W * 64, 0.0f);
    memcpy(padded.data(), thr_host, (size_t)h->nbits * 4);
    if (!h->thr) HIP_TRY(hipMalloc((void **)&h->thr, padded.size() * 4));
    HIP_TRY(hipMemcpy(h->thr, padded.data(), padded.size() * 4, hipMemcpyHostToDevice));
    return 0;
}

// IndexLSH::train with train_thresholds (seqvec_search/create_index.py:43, pfam/search.py:35, pfam/proteins_search.py:87
// call train before add): per-bit medians of the training rows' projections, installed as the thresholds
extern "C" int knn_lsh_train(knn_lsh_s *h, const float *x_host, int64_t n)
{
    if (!h || !x_host) return set_err(KNN_ERR_INVALID, "lsh_train: null pointer");
    if (n < 1) return set_err(KNN_ERR_INVALID, "lsh_train: need at least one training row");
    if (n >= (1ll << 31)) return set_err(KNN_ERR_UNSUPPORTED, "lsh_train: more than 2^31 - 1 training rows");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->ntotal) return set_err(KNN_ERR_INVALID, "lsh_train: the index already holds rows (their codes would go stale)");
    HIP_TRY(hipSetDevice(h->device));
    const int64_t ldp = (n + 127) / 128 * 128;
    const size_t need = (size_t)h->W * 64 * ldp * 4;
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    if (need > free_b / 2)
        return set_err(KNN_ERR_UNSUPPORTED, "lsh_train: the projections of the training rows take " + std::to_string(need) +
                                                " bytes, more than half of the " + std::to_string(free_b) +
                                                " bytes free on the device: train on a sample of the rows");
    EvalBufs bufs;
    PhaseClock clock;
    float *d_P = (float *)bufs.get(need), *d_thr = (float *)bufs.get((size_t)h->nbits * 4);
    int32_t *d_status = (int32_t *)bufs.get((size_t)h->nbits * 4);
    if (bufs.oom) return set_err(KNN_ERR_HIP, "lsh_train: out of device memory");
    // the projections are taken without thresholds whatever the handle holds: lsh_project_kernel does not read them
    int rc = lsh_encode_host_rows(h, x_host, n, nullptr, d_P, ldp, &clock);
    if (rc) return rc;
    hipStream_t s = h->stream;
    LshMedianParams mp;
    mp.proj = d_P; mp.n = n; mp.ldp = ldp; mp.thr = d_thr; mp.status = d_status;
    EVAL_TRY(clock.open(LSH_TRAIN_SELECT, s));
    hipLaunchKernelGGL(lsh_median_kernel, dim3(h->nbits), dim3(256), 0, s, mp); // (the padding columns are skipped)
    HIP_TRY(hipGetLastError());
    EVAL_TRY(clock.close(s));
    std::vector<float> thr((size_t)h->nbits);
    std::vector<int32_t> status((size_t)h->nbits);
    HIP_TRY(hipMemcpyAsync(thr.data(), d_thr, thr.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(status.data(), d_status, status.size() * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    float ms[LSH_TRAIN_PHASES];
    EVAL_TRY(clock.read(ms, LSH_TRAIN_PHASES));
    for (int b = 0; b < h->nbits; b++)
        if (status[b])
            return set_err(KNN_ERR_INVALID, std::string("lsh_train: ") + (status[b] == 1 ? "a projection onto bit " : "the median (+inf and -inf around the middle) of bit ") +
                                                std::to_string(b) + " is NaN");
    rc = lsh_install_thresholds(h, thr.data());
    if (rc) return rc;
    memcpy(h->train_ms, ms, sizeof ms);
    return 0;
}

// IndexLSH::thresholds of an index file (read_index), or of another index; NULL removes them
extern "C" int knn_lsh_set_thresholds(knn_lsh_s *h, const float *thr_host)
{
    if (!h) return set_err(KNN_ERR_INVALID, "lsh_set_thresholds: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    if (h->ntotal) return set_err(KNN_ERR_INVALID, "lsh_set_thresholds: the index already holds rows (their codes would go stale)");
    if (thr_host)
        for (int b = 0; b < h->nbits; b++)
            if (thr_host[b] != thr_host[b]) return set_err(KNN_ERR_INVALID, "lsh_set_thresholds: the threshold of bit " + std::to_string(b) + " is NaN");
    HIP_TRY(hipSetDevice(h->device));
    return lsh_install_thresholds(h, thr_host);
}

extern "C" int knn_lsh_get_thresholds(knn_lsh_s *h, float *out_host)
{
    if (!h || !out_host) return set_err(KNN_ERR_INVALID, "lsh_get_thresholds: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (!h->thr) return set_err(KNN_ERR_INVALID, "lsh_get_thresholds: the index has no thresholds");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy(out_host, h->thr, (size_t)h->nbits * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int knn_lsh_last_train_ms(knn_lsh_s *h, float *upload_ms, float *project_ms, float *select_ms)
{
    if (!h || !upload_ms || !project_ms || !select_ms) return set_err(KNN_ERR_INVALID, "lsh_last_train_ms: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    *upload_ms = h->train_ms[0];
    *project_ms = h->train_ms[1];
    *select_ms = h->train_ms[2];
    return 0;
}

extern "C" int knn_lsh_add(knn_lsh_s *h, const float *x_host, int64_t n)
{
    if (!h) return set_err(KNN_ERR_INVALID, "lsh_add: null handle");
    if (n < 0) return set_err(KNN_ERR_INVALID, "lsh_add: negative n");
    if (n == 0) return 0;
    if (!x_host) return set_err(KNN_ERR_INVALID, "lsh_add: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    if (h->ntotal + n > h->cap_rows) {
        int64_t ncap = std::max<int64_t>(h->ntotal + n, h->cap_rows + h->cap_rows / 2);
        uint64_t *nc = nullptr;
        HIP_TRY(hipMalloc((void **)&nc, (size_t)ncap * h->W * 8));
        if (h->ntotal) HIP_TRY(hipMemcpy(nc, h->codes, (size_t)h->ntotal * h->W * 8, hipMemcpyDeviceToDevice));
        if (h->codes) (void)hipFree(h->codes);
        h->codes = nc;
        h->cap_rows = ncap;
    }
    int rc = lsh_encode_host_rows(h, x_host, n, h->codes + (size_t)h->ntotal * h->W);
    if (rc) return rc;
    h->ntotal += n;
    return 0;
}

// codes in FAISS byte order: [n][bytes_per_vec], bit i of a row = byte i>>3, bit i&7.  The device codes carry 1 bits from
// nbits up (the encoder sets them by their index, whatever the row holds); FAISS's codes have zeros there, so they are
// cleared on the way out.
extern "C" int knn_lsh_get_codes(knn_lsh_s *h, uint8_t *out_host, int32_t bytes_per_vec)
{
    if (!h || !out_host) return set_err(KNN_ERR_INVALID, "lsh_get_codes: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    if (bytes_per_vec <= 0 || bytes_per_vec > h->W * 8) return set_err(KNN_ERR_INVALID, "lsh_get_codes: bad bytes_per_vec");
    if (h->ntotal == 0) return 0;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemcpy2D(out_host, (size_t)bytes_per_vec, h->codes, (size_t)h->W * 8, (size_t)bytes_per_vec, (size_t)h->ntotal, hipMemcpyDeviceToHost));
    if ((int64_t)bytes_per_vec * 8 > h->nbits) {
        const int b0 = h->nbits >> 3; // (< bytes_per_vec)
        const uint8_t keep = (uint8_t)((1u << (h->nbits & 7)) - 1);
        for (int64_t i = 0; i < h->ntotal; i++) {
            uint8_t *row = out_host + (size_t)i * bytes_per_vec;
            row[b0] &= keep;
            memset(row + b0 + 1, 0, (size_t)(bytes_per_vec - b0 - 1));
        }
    }
    return 0;
}

// appends precomputed codes (read_index)
extern "C" int knn_lsh_add_codes(knn_lsh_s *h, const uint8_t *codes_host, int64_t n, int32_t bytes_per_vec)
{
    if (!h || (!codes_host && n > 0)) return set_err(KNN_ERR_INVALID, "lsh_add_codes: null pointer");
    if (n <= 0) return 0;
    std::lock_guard<std::mutex> lk(h->mu);
    if (bytes_per_vec != (h->nbits + 7) / 8) return set_err(KNN_ERR_INVALID, "lsh_add_codes: bytes_per_vec does not match nbits");
    HIP_TRY(hipSetDevice(h->device));
    if (h->ntotal + n > h->cap_rows) {
        int64_t ncap = h->ntotal + n;
        uint64_t *nc = nullptr;
        HIP_TRY(hipMalloc((void **)&nc, (size_t)ncap * h->W * 8));
        if (h->ntotal) HIP_TRY(hipMemcpy(nc, h->codes, (size_t)h->ntotal * h->W * 8, hipMemcpyDeviceToDevice));
        if (h->codes) (void)hipFree(h->codes);
        h->codes = nc;
        h->cap_rows = ncap;
    }
    // padding bits are 1 in codes produced by the encoder: keep that convention
    std::vector<uint8_t> tmp((size_t)n * h->W * 8, 0xFF);
    for (int64_t i = 0; i < n; i++) {
        memcpy(&tmp[(size_t)i * h->W * 8], codes_host + (size_t)i * bytes_per_vec, (size_t)bytes_per_vec);
        if (h->nbits & 7) tmp[(size_t)i * h->W * 8 + bytes_per_vec - 1] |= (uint8_t)(0xFF << (h->nbits & 7));
    }
    HIP_TRY(hipMemcpy(h->codes + (size_t)h->ntotal * h->W, tmp.data(), tmp.size(), hipMemcpyHostToDevice));
    h->ntotal += n;
    return 0;
}

template <int W>
static int launch_hamming(const HammingParams &p, int grid, size_t lds, hipStream_t s)
{
    HIP_TRY(hipFuncSetAttribute((const void *)hamming_scan_kernel<W>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(hamming_scan_kernel<W>, dim3(grid), dim3(256), lds, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The batch loop of knn_lsh_search and knn_lsh_search_refine (the caller holds the locks and has checked the shapes): the
// kb smallest Hamming distances of every query, selected on the device.  flat == null: those are the result (k == kb).
// flat given: the batch's kb ids stay on the device, refine_batch scores them against flat's rows with the batch's fp32
// queries -- still on the device from the encode step -- and its best k are the result.  Either way only [m][k] goes down.
static int lsh_search_batches(knn_lsh_s *h, knn_index_s *flat, const float *q_host, int64_t nq, int64_t kb, int64_t k, float *D_host,
                              int64_t *I_host, PhaseClock &refine_clock)
{
    hipStream_t s = h->stream;
    const int QT = 32, DT = 256;
    // (a refined batch keeps its queries on the device: no more of them than one slab of the encoder uploads at a time)
    const int64_t QB = flat ? std::min<int64_t>(16384, lsh_slab_rows(h)) : 16384;
    const int W = h->W;
    // Several batches (pfam/search.py searches every row, k = 1000): two sets of result buffers, and the results of batch
    // b - 1 go down on the device's copy stream while batch b is scanned (ResultPipe)
    const int64_t nbatches = (nq + QB - 1) / QB;
    PipeLease lease;
    int rc = lease_pipes(h->device, nbatches > 1, lease);
    if (rc) return rc;
    const ResultPipe rp{lease.cp, s, "lsh_search: "};
    DevBuf *dD[2] = {&h->ws_D, &h->ws_D2}, *dI[2] = {&h->ws_I, &h->ws_I2};
    // batch bi: queries encoded, scanned, selected (and refined) into the result buffers of `slot`
    auto scan = [&](int64_t bi, int slot) -> int {
        const int64_t b0 = bi * QB, m = std::min(QB, nq - b0);
        if (h->ws_q.ensure((size_t)m * W * 8)) return set_err(KNN_ERR_HIP, "lsh_search: out of device memory");
        const float *xq_dev = nullptr;
        int rc = lsh_encode_host_rows(h, q_host + b0 * h->d, m, (uint64_t *)h->ws_q.p, nullptr, 0, nullptr, &xq_dev);
        if (rc) return rc;
        HammingParams p;
        p.codes = h->codes; p.qcodes = (const uint64_t *)h->ws_q.p; p.nb = h->ntotal; p.nq = m; p.W = W; p.k = (int)kb;
        p.cap = std::max(512, next_pow2_host(2 * (int)kb + DT));
        if (kb <= KNN_REGISTER_SELECT_MAX_K) p.cap = std::min(p.cap, 2048);
        else if (kb <= KNN_WAVE_SELECT_MAX_K) p.cap = std::min(p.cap, 4096);
        p.kslot = knn_kslot((int)kb);
        p.nqtiles = (int)((m + QT - 1) / QT);
        const int64_t ntiles = (h->ntotal + DT - 1) / DT;
        int64_t want = std::max<int64_t>(1, (1024 + p.nqtiles - 1) / p.nqtiles);
        const int64_t min_tiles = std::max<int64_t>(2, (4 * kb + DT - 1) / DT);
        want = std::max<int64_t>(1, std::min(want, std::max<int64_t>(1, ntiles / min_tiles)));
        const size_t per_wg = (size_t)QT * p.cap * 8;
        want = std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)((2ull << 30) / per_wg) / p.nqtiles));
        const int64_t tiles_per = (ntiles + want - 1) / want;
        p.chunk_rows = tiles_per * DT;
        p.nchunks = (int)((h->ntotal + p.chunk_rows - 1) / p.chunk_rows);
        const int grid = p.nqtiles * p.nchunks;
        p.qcap = p.nchunks * p.kslot;
        if (h->ws_lists.ensure((size_t)grid * per_wg) || h->ws_gthr.ensure((size_t)p.nqtiles * QT * 4) ||
            h->ws_qlist.ensure((size_t)m * p.qcap * 8) || h->ws_qcnt.ensure((size_t)m * 4) || dD[slot]->ensure((size_t)std::min(QB, nq) * k * 4) ||
            dI[slot]->ensure((size_t)std::min(QB, nq) * k * 8) ||
            (flat && (h->ws_cD.ensure((size_t)m * kb * 4) || h->ws_cI.ensure((size_t)m * kb * 8))))
            return set_err(KNN_ERR_HIP, "lsh_search: out of device memory");
        HIP_TRY(hipMemsetAsync(h->ws_gthr.p, 0xFF, (size_t)p.nqtiles * QT * 4, s));
        HIP_TRY(hipMemsetAsync(h->ws_qcnt.p, 0, (size_t)m * 4, s));
        p.lists = (uint64_t *)h->ws_lists.p; p.gthr = (uint32_t *)h->ws_gthr.p;
        p.qlist = (uint64_t *)h->ws_qlist.p; p.qcnt = (uint32_t *)h->ws_qcnt.p;
        const size_t lds = std::max(std::max((size_t)QT * W * 8 + QT * 4, (size_t)p.cap * 8), (size_t)4096) + QT * 12 + 16;
        switch (W) {
        case 2: rc = launch_hamming<2>(p, grid, lds, s); break;
        case 4: rc = launch_hamming<4>(p, grid, lds, s); break;
        case 8: rc = launch_hamming<8>(p, grid, lds, s); break;
        case 16: rc = launch_hamming<16>(p, grid, lds, s); break;
        case 32: rc = launch_hamming<32>(p, grid, lds, s); break;
        default: return set_err(KNN_ERR_UNSUPPORTED, "lsh_search: unsupported code width");
        }
        if (rc) return rc;
        // the chunks' survivors -> the k smallest Hamming distances per query, ties by lower id (the keys
        // carry the distance as a float: METRIC_L2 formatting)
        SelectParams sp = {};
        sp.in = p.qlist; sp.in_stride = p.qcap; sp.cnt = p.qcnt; sp.cap = p.qcap;
        sp.nq = m; sp.k = (int)kb; sp.metric = KNN_METRIC_L2;
        sp.D = (float *)(flat ? h->ws_cD.p : dD[slot]->p); sp.I = (int64_t *)(flat ? h->ws_cI.p : dI[slot]->p);
        rc = launch_select(sp, s);
        if (rc) return rc;
        if (flat) { // exact scores of the kb hits, the best k of them into this batch's result buffers
            rc = refine_batch(flat, xq_dev, (const int64_t *)h->ws_cI.p, m, (int)kb, (int)k, (float *)dD[slot]->p, (int64_t *)dI[slot]->p, s, refine_clock);
            if (rc) return rc;
        }
        return 0;
    };
    auto copy = [&](int64_t bi, int slot, hipStream_t on) -> hipError_t {
        const int64_t b0 = bi * QB, m = std::min(QB, nq - b0);
        hipError_t r = hipMemcpyAsync(D_host + b0 * k, dD[slot]->p, (size_t)m * k * 4, hipMemcpyDeviceToHost, on);
        if (r == hipSuccess) r = hipMemcpyAsync(I_host + b0 * k, dI[slot]->p, (size_t)m * k * 8, hipMemcpyDeviceToHost, on);
        return r;
    };
    for (int64_t bi = 0; bi < nbatches && !rc; bi++) {
        rc = rp.before(bi);
        if (!rc) rc = scan(bi, rp.slot(bi));
        if (!rc) rc = rp.after(bi, copy);
    }
    return rp.finish(rc, nbatches, copy);
}

extern "C" int knn_lsh_search(knn_lsh_s *h, const float *q_host, int64_t nq, int64_t k, float *D_host, int64_t *I_host)
{
    if (!h) return set_err(KNN_ERR_INVALID, "lsh_search: null handle");
    if (nq < 0 || k < 1) return set_err(KNN_ERR_INVALID, "lsh_search: bad shape");
    if (k > KNN_MAX_K) return set_err(KNN_ERR_UNSUPPORTED, "lsh_search: k > 2048 is not supported");
    if (nq == 0) return 0;
    if (!q_host || !D_host || !I_host) return set_err(KNN_ERR_INVALID, "lsh_search: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    HIP_TRY(hipSetDevice(h->device));
    if (h->ntotal == 0) {
        fill_empty_host(D_host, I_host, nq * k, KNN_METRIC_L2); // (Hamming distances: smaller is better)
        return 0;
    }
    PhaseClock none; // (nothing is refined: it stays empty)
    return lsh_search_batches(h, nullptr, q_host, nq, k, k, D_host, I_host, none);
}

// IndexRefineFlat(IndexLSH).search: IndexLSH::search for kb labels, IndexFlat::compute_distance_subset, reorder_2_heaps --
// with the labels never leaving the device.  Locks: the LSH handle's, then the flat handle's.
extern "C" int knn_lsh_search_refine(knn_lsh_s *h, knn_handle flat, const float *q_host, int64_t nq, int64_t kb, int64_t k, float *D_host,
                                     int64_t *I_host)
{
    if (!h || !flat) return set_err(KNN_ERR_INVALID, "lsh_search_refine: null handle");
    int rc = refine_check_shape(nq, kb, k, "lsh_search_refine");
    if (rc) return rc;
    if (nq == 0) return 0;
    if (!q_host || !D_host || !I_host) return set_err(KNN_ERR_INVALID, "lsh_search_refine: null pointer");
    std::lock_guard<std::mutex> lk(h->mu);
    std::lock_guard<std::mutex> lkf(flat->mu);
    if ((rc = refine_check_flat(flat, "lsh_search_refine"))) return rc;
    if (flat->device != h->device || flat->d != h->d || flat->ntotal != h->ntotal)
        return set_err(KNN_ERR_INVALID, "lsh_search_refine: the base index (device " + std::to_string(h->device) + ", d " + std::to_string(h->d) + ", " +
                                            std::to_string(h->ntotal) + " rows) and the refine index (device " + std::to_string(flat->device) + ", d " +
                                            std::to_string(flat->d) + ", " + std::to_string(flat->ntotal) + " rows) do not hold the same rows");
    HIP_TRY(hipSetDevice(h->device));
    if (h->ntotal == 0) {
        fill_empty_host(D_host, I_host, nq * k, flat->metric);
        return 0;
    }
    HIP_TRY(hipStreamSynchronize(flat->stream)); // (the rows are read on the LSH handle's stream: whatever the flat handle's own stream still does to them first)
    PhaseClock clock;
    rc = lsh_search_batches(h, flat, q_host, nq, kb, k, D_host, I_host, clock);
    if (rc) return rc;
    return refine_commit_ms(clock, flat);
}

// IndexLSH::reset: the handle keeps its rotation, thresholds and the codes' allocation
extern "C" int knn_lsh_reset(knn_lsh_s *h)
{
    if (!h) return set_err(KNN_ERR_INVALID, "lsh_reset: null handle");
    std::lock_guard<std::mutex> lk(h->mu);
    h->ntotal = 0;
    return 0;
}
