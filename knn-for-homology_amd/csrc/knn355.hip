// knn355.hip -- MI355X (gfx950 / CDNA4) flat kNN: distance + fused top-k.
//
// Stands in for faiss-cpu 1.7.2's IndexFlat / normalize_L2 as called by the
// reference (cath/search.py:13-26, seqvec_search/main.py:22-50,
// pfam/proteins_search.py:21-50, pfam/search.py:42-53,
// pfam/slices/slices_search.py:15-31).  C ABI: include/knn355.h.
//
// Arithmetic contract (bit-exact with oracle/knn_oracle.c):
//   dot(x,y)  one fp32 fma chain per (query,row) pair, k visited per 8-block in
//             the order 0,4,1,5,2,6,3,7 -- exactly what v_mfma_f32_32x32x2_f32
//             produces when lane (i,h) feeds floats 8t+4h+m for m = 0..3
//   nrm(x)    dot(x, x): the same chain, so L2(x, x) == 0 exactly
//   L2        max(0, fma(-2, dot, nrm(x)+nrm(y)))
//   ties      lower row id first (packed 64-bit keys: score bits << 32 | row)
//
// Kernel plan (DESIGN.md has the long form):
//   flat_scan_kernel     one workgroup = QT queries x one chunk of database rows.  Per
//                        32-float K step both operands are staged into LDS with
//                        global_load_lds_dwordx4 (full 128-B lines, XOR-swizzled on the
//                        source address), fragments come back with ds_read_b128, fp32 MFMA
//                        accumulates the QT x DT score tile; the epilogue compares every
//                        score with a running per-query threshold and appends the survivors
//                        as packed keys; lists are cut back by wave_select (one wave per
//                        query, registers only).
//   merge_select_kernel  one wave per (query, group of lists): exact top-k of <= 4096 keys,
//                        last round sorts and writes D / I.
//   hnsw.inc / lsh.inc / eval.inc   IndexHNSWFlat, IndexLSH, consumers of (hits, scores).
//   assemble.inc                    protein-level hits from slice searches (knn_eval_assemble).
//   slices_eval.inc                 slice-level correctness and AUC1 of slice searches (knn_eval_slice_annotate, knn_eval_slices).
//   pr_curve.inc                    the precision-recall threshold sweep over (is_correct, scores) (knn_eval_pr_curve).
//   buckets.inc                     accuracy per score bucket and the accuracy-over-hits curve (knn_eval_bucket_counts, knn_eval_hit_curve).
//   fuse.inc                        the two hit-list fusions of the results scripts: prefix-then-fill, sorted union (knn_eval_fuse).
//   overlap.inc                     two hit lists compared as sets of ids: true-positive overlap, leading-run union (knn_eval_overlap).
//   pca.inc                         mean, covariance (fp32 MFMA) and projection behind decomposition.PCA (knn_pca_moments, knn_pca_project).
//   kde.inc                         1-D Gaussian kernel density estimates behind density.gaussian_kde (knn_kde_stats, knn_kde_eval).
//   range.inc / refine.inc          IndexFlat.range_search, IndexRefineFlat (exact re-scoring of a shortlist).
//
// This file is the device code of the flat search and nothing else: bench.py and tools/summarize_profiles.py pin it by
// SHA-256, and the measured HBM traffic of profiles/pmc_traffic.json is quoted only while the hash stands.  Host code
// belongs in host_core.inc, flat_index.inc, flat_search.inc, flat_info.inc and comm.inc, a feature in an .inc file of its
// own, and every #include of them in knn355_lib.hip (the translation unit the Makefile builds) -- not here.
#include <hip/hip_runtime.h>
#include <thread>
#include <type_traits>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <float.h>
#include <math.h>
#include <algorithm>
#include <mutex>
#include <condition_variable>
#include <chrono>
#include <memory>
#include <atomic>
#include <string>
#include <vector>

#include "../../include/knn355.h"
#include "plan.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef const __attribute__((address_space(1))) f32x4 *gptr4; // explicit global (not flat) loads
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

#define KEY_PAD 0xFFFFFFFFFFFFFFFFull
#define KEY_WORD_INF 0xFF800000u // f2ord(+inf): the first score word that is no score (select_topk_kernel's load)
#ifndef KNN355_DIFF_SCALAR_Q
#define KNN355_DIFF_SCALAR_Q 1 // difference builds read their query fragments with scalar loads (0: broadcast LDS reads, round-4 first form)
#endif
#ifndef KNN355_DIFF_SCALAR_PAIRS
#define KNN355_DIFF_SCALAR_PAIRS 3 // ... the first three query pairs of a thread's half (all of them up to 12 queries), the others through the LDS
#endif
#ifndef KNN355_EPI_PRIO
#define KNN355_EPI_PRIO 0 // issue priority of a wave behind its K loop (two workgroups per CU).  Measured with 2 against 0 on one box: CATH-sized
                          // symmetric kernel 2.21-2.22 vs 2.25 ms, 10 M-row step 6.874 vs 6.886 ms, shard step 0.916 vs 0.914 ms -- nothing: off
#endif
#ifndef KNN355_STREAM_DMA_FIRST
#define KNN355_STREAM_DMA_FIRST 1 // streaming launches issue a K step's staging instructions in front of its first MFMA (flat_scan_kernel)
#endif

// ---------------------------------------------------------------------------
// device helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t f2ord(float f)
{
    uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ord2f(uint32_t o)
{
    uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    return __uint_as_float(u);
}

// nrm(x) = dot(x, x) in the contract's chain order: one lane walks one row.
// T: float, or _Float16 rows converted to float (exactly) as they are read (pool.inc).
template <bool ALIGNED, typename T = float>
__device__ __forceinline__ float lane_norm_row(const T *__restrict__ r, int d)
{
    float acc = 0.0f;
    int k0 = 0;
    for (; k0 + 8 <= d; k0 += 8) {
        float a[8];
        if constexpr (ALIGNED && sizeof(T) == 4) {
            f32x4 lo = *(const f32x4 *)(r + k0), hi = *(const f32x4 *)(r + k0 + 4);
#pragma unroll
            for (int m = 0; m < 4; m++) { a[m] = lo[m]; a[4 + m] = hi[m]; }
        } else if constexpr (ALIGNED) {
            f16x4 lo = *(const f16x4 *)(r + k0), hi = *(const f16x4 *)(r + k0 + 4);
#pragma unroll
            for (int m = 0; m < 4; m++) { a[m] = (float)lo[m]; a[4 + m] = (float)hi[m]; }
        } else {
#pragma unroll
            for (int m = 0; m < 8; m++) a[m] = r[k0 + m];
        }
#pragma unroll
        for (int m = 0; m < 4; m++) {
            acc = __builtin_fmaf(a[m], a[m], acc);
            acc = __builtin_fmaf(a[4 + m], a[4 + m], acc);
        }
    }
    if (k0 < d) {
        float a[8];
#pragma unroll
        for (int m = 0; m < 8; m++) a[m] = (k0 + m < d) ? r[k0 + m] : 0.0f;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            acc = __builtin_fmaf(a[m], a[m], acc);
            acc = __builtin_fmaf(a[4 + m], a[4 + m], acc);
        }
    }
    return acc;
}

// one lane per row; 64-thread blocks
template <bool ALIGNED>
__global__ __launch_bounds__(64) void norm_rows_kernel(const float *__restrict__ x, int64_t n, int d, int64_t stride,
                                                        float *__restrict__ out)
{
    int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= n) return;
    out[row] = lane_norm_row<ALIGNED>(x + row * stride, d);
}

// faiss.normalize_L2: each lane computes the norm of its own row, then the wave
// rescales the block's 64 rows one after the other with coalesced accesses.
template <bool ALIGNED>
__global__ __launch_bounds__(64) void normalize_rows_kernel(float *__restrict__ x, int64_t n, int d, int64_t stride)
{
    const int lane = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * 64;
    const int64_t row = row0 + lane;
    float inv = -1.0f; // < 0 == leave the row alone (0 is a factor like any other: a row whose norm overflows is multiplied by 1 / sqrt(inf) = 0, as fvec_renorm_L2 does)
    if (row < n) {
        float nr = lane_norm_row<ALIGNED>(x + row * stride, d);
        if (nr > 0.0f) inv = (float)(1.0 / (double)sqrtf(nr));
    }
    const int nrows = (int)min((int64_t)64, n - row0);
    for (int r = 0; r < nrows; r++) {
        const float s = __shfl(inv, r, 64);
        if (s < 0.0f) continue;
        float *p = x + (row0 + r) * stride;
        if constexpr (ALIGNED) {
            for (int e = 4 * lane; e < d; e += 256) {
                if (e + 3 < d) {
                    f32x4 v = *(f32x4 *)(p + e);
                    v[0] *= s; v[1] *= s; v[2] *= s; v[3] *= s;
                    *(f32x4 *)(p + e) = v;
                } else {
                    for (int c = 0; c < 3; c++)
                        if (e + c < d) p[e + c] *= s;
                }
            }
        } else {
            for (int e = lane; e < d; e += 64) p[e] *= s;
        }
    }
}

// dst[n][dp] <- src[n][d], zero padded
__global__ void pad_rows_kernel(const float *__restrict__ src, int64_t n, int d,
                                float *__restrict__ dst, int dp)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t total = n * dp;
    for (; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t r = i / dp;
        int c = (int)(i - r * dp);
        dst[i] = c < d ? src[r * d + c] : 0.0f;
    }
}

// dst[n][dp] (bf16) <- src[n][dp] (fp32), round to nearest even: the operand copies of an approximate (bf16) index
__global__ void to_bf16_kernel(const float *__restrict__ src, int64_t total, __bf16 *__restrict__ dst)
{
    int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    for (; i < total; i += (int64_t)gridDim.x * blockDim.x * 4) {
        const f32x4 v = *(const f32x4 *)(src + i); // (total is a multiple of 64)
        dst[i] = (__bf16)v[0];
        dst[i + 1] = (__bf16)v[1];
        dst[i + 2] = (__bf16)v[2];
        dst[i + 3] = (__bf16)v[3];
    }
}

// The queries of a difference-build scan (fewer than 20 of them), interleaved by pairs so that one 16-byte LDS read hands a
// lane two consecutive k of BOTH queries of a pair as two aligned register pairs (flat_scan_kernel<..., DNQ>):
//   out[2p    ][32 s + i] = query (2p + (i & 1)) [32 s + i / 2]        (k = 0..15 of K step s)
//   out[2p + 1][32 s + i] = query (2p + (i & 1)) [32 s + 16 + i / 2]   (k = 16..31)
// for p < dnq / 2; queries past the last one repeat it (their scores are never looked at).
__global__ void diff_interleave_kernel(const float *__restrict__ xq, int64_t nq, int dp, int dnq, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)dnq * dp) return;
    const int row = (int)(i / dp), col = (int)(i - (int64_t)row * dp);
    const int pr = row >> 1, half = row & 1, step = col >> 5, w = col & 31;
    const int64_t q = min((int64_t)(2 * pr + (w & 1)), nq - 1);
    out[i] = xq[q * dp + 32 * step + 16 * half + (w >> 1)];
}

// ---------------------------------------------------------------------------
// workgroup-wide bitonic sort of P (power of two) u64 keys in LDS, ascending
// ---------------------------------------------------------------------------
__device__ __forceinline__ void wg_bitonic_sort(uint64_t *sb, int P, int tid, int nthreads)
{
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (P >> 1); i += nthreads) {
                int a = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                int b = a + j;
                bool up = (a & k2) == 0;
                uint64_t x = sb[a], y = sb[b];
                if ((x > y) == up) { sb[a] = y; sb[b] = x; }
            }
            __syncthreads();
        }
    }
}

// The same network over (word, tag) PAIRS compared lexicographically, for keys that fill all 64 bits of the word and
// leave no room to pack a position behind them (fuse.inc: the order word of a double).  P <= 65536 tags.
__device__ __forceinline__ void wg_bitonic_sort_pairs(uint64_t *sk, uint16_t *st, int P, int tid, int nthreads)
{
    for (int k2 = 2; k2 <= P; k2 <<= 1) {
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < (P >> 1); i += nthreads) {
                int a = ((i & ~(j - 1)) << 1) | (i & (j - 1));
                int b = a + j;
                bool up = (a & k2) == 0;
                uint64_t x = sk[a], y = sk[b];
                uint16_t tx = st[a], ty = st[b];
                bool gt = x > y || (x == y && tx > ty);
                if (gt == up && (x != y || tx != ty)) { sk[a] = y; sk[b] = x; st[a] = ty; st[b] = tx; }
            }
            __syncthreads();
        }
    }
}

// One wave, P = 64 E keys (E = 1, 2, 4, 8, 16): the same sort in registers.  Lane l holds elements l E .. l E + E - 1, so a
// compare-exchange at distance j < E stays inside the lane (register indices and, for k2 <= E, directions known at compile
// time) and one at distance j >= E meets lane l ^ (j / E) in the same register: two cross-lane moves per key instead of two
// LDS reads, two LDS writes and a barrier per pair.  (The LDS sort of 512 keys costs a wave 720 eight-byte LDS operations;
// with 56 one-wave selections per CU -- a CATH-sized all-vs-all -- that was 67 us of a 219 us kernel on the LDS pipe alone.)
// value of lane (l ^ M) without the LDS crossbar where the vector pipe can do it: DPP inside a row of 16 lanes (quad
// permutations for 1 and 2; 4 = "mirror the half row" (l ^ 7) then "reverse the quad" (l ^ 3); 8 = rotate the row by 8),
// v_permlane16_swap / v_permlane32_swap (gfx950) across rows and wave halves
template <int M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v, int lane)
{
    if constexpr (M == 1) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0xB1, 0xF, 0xF, true);
    else if constexpr (M == 2) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x4E, 0xF, 0xF, true);
    else if constexpr (M == 4) return (uint32_t)__builtin_amdgcn_mov_dpp(__builtin_amdgcn_mov_dpp((int)v, 0x141, 0xF, 0xF, true), 0x1B, 0xF, 0xF, true);
    else if constexpr (M == 8) return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, 0x128, 0xF, 0xF, true);
    else if constexpr (M == 16) {
        const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false); // r[0]: odd rows <- the even rows below them; r[1]: even rows <- the odd rows above
        return (lane & 16) ? r[0] : r[1];
    } else {
        static_assert(M == 32, "lane distance");
        const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false);
        return (lane & 32) ? r[0] : r[1];
    }
}

// one stage of the network: compare-exchange at distance J inside runs of K2 (element index = lane E + register)
template <int E, int K2, int J>
__device__ __forceinline__ void bitonic_stage_regs(uint64_t (&v)[E], int lane)
{
    if constexpr (J >= E) {
        // (K2 >= 2 J >= 2 E here: the direction depends on the lane only; the last merge, K2 = 64 E, ascends everywhere)
        const bool up = K2 >= 64 * E || (lane & (K2 / E)) == 0;
        const bool keep_min = ((lane & (J / E)) == 0) == up;
#pragma unroll
        for (int r = 0; r < E; r++) {
            const uint32_t ohi = lane_xor<J / E>((uint32_t)(v[r] >> 32), lane);
            const uint32_t olo = lane_xor<J / E>((uint32_t)v[r], lane);
            const uint64_t o = ((uint64_t)ohi << 32) | olo;
            v[r] = ((o < v[r]) == keep_min) ? o : v[r];
        }
    } else {
#pragma unroll
        for (int r = 0; r < E; r++) {
            if ((r & J) == 0) {
                const uint64_t a = v[r], b = v[r | J];
                bool up; // bit K2 of the element index is a bit of the register index when K2 < E, of the lane otherwise
                if (K2 < E) up = (r & K2) == 0;
                else up = K2 >= 64 * E || (lane & (K2 / E)) == 0;
                const bool sw = (a > b) == up;
                v[r] = sw ? b : a;
                v[r | J] = sw ? a : b;
            }
        }
    }
    if constexpr (J > 1) bitonic_stage_regs<E, K2, J / 2>(v, lane);
    else if constexpr (K2 < 64 * E) bitonic_stage_regs<E, 2 * K2, K2>(v, lane);
}

template <int E>
__device__ __forceinline__ void wave_bitonic_sort_regs(uint64_t *sb, int lane)
{
    uint64_t v[E];
#pragma unroll
    for (int r = 0; r < E; r++) v[r] = sb[lane * E + r];
    bitonic_stage_regs<E, 2, 1>(v, lane);
#pragma unroll
    for (int r = 0; r < E; r++) sb[lane * E + r] = v[r];
}

__device__ __forceinline__ int next_pow2_dev(int n)
{
    int p = 64;
    while (p < n) p <<= 1;
    return p;
}

// ---------------------------------------------------------------------------
// wave-wide selection over one candidate list (n <= 64*R packed keys in global
// memory, pulled into registers).  Keeps the best keys -- exactly k when
// kmax == k, otherwise any count in [k, kmax] -- and writes them packed to dst
// (dst may alias lst).  No LDS, no barriers: four waves of a workgroup select
// for four different queries at once.
//   *thr_ord receives T with count(hi <= T) >= k, a valid admission threshold.
//   dst may be NULL: only T is wanted (the tile-minimum seed of the scan kernel).
// Method: MSB-first binary search on the 32-bit score word ("largest P with
// count(hi < P) <= k-1"), each probe one v_cmp + s_bcnt1 per register, started
// below the bits all keys share and stopped as soon as a probe leaves between k
// and kmax survivors; ties that straddle the cut are broken on the id word.
// ---------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum(int x)
{
    // DPP butterfly inside each row of 16 lanes, then row broadcasts; lane 63 ends with the total
    x += __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);  // quad_perm:[1,0,3,2]
    x += __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);  // quad_perm:[2,3,0,1]
    x += __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, false); // row_half_mirror
    x += __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, false); // row_mirror
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1,3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2,3
    return __builtin_amdgcn_readlane(x, 63);
}

typedef const __attribute__((address_space(1))) uint64_t *gptr_u64; // explicit global (not flat) loads
struct LoadContig {
    const uint64_t *p;
    __device__ __forceinline__ uint64_t operator()(int idx) const { return ((gptr_u64)p)[idx]; }
};
// keys other workgroups of the SAME launch are still publishing (agent scope: served from memory, never from a
// stale line of this XCD's L2)
struct LoadAgent {
    const uint64_t *p;
    __device__ __forceinline__ uint64_t operator()(int idx) const { return __hip_atomic_load(p + idx, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// element idx of the concatenation of lists l0.. of query q inside a [list][query][k] buffer
struct LoadListMajor {
    const uint64_t *base;
    int64_t nq, q;
    int k, l0;
    __device__ __forceinline__ uint64_t operator()(int idx) const
    {
        const int l = idx / k, j = idx - l * k;
        return ((gptr_u64)base)[((size_t)(l0 + l) * nq + q) * k + j];
    }
};

// min / max over the wave and inclusive prefix sum, all with DPP row operations (no LDS
// crossbar round trips): butterfly inside rows of 16 lanes, then row broadcasts
#define DPP_U32(x, ctrl, rmask) ((uint32_t)__builtin_amdgcn_update_dpp((int)(x), (int)(x), ctrl, rmask, 0xF, false))
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t x)
{
    x = min(x, DPP_U32(x, 0xB1, 0xF));
    x = min(x, DPP_U32(x, 0x4E, 0xF));
    x = min(x, DPP_U32(x, 0x141, 0xF));
    x = min(x, DPP_U32(x, 0x140, 0xF));
    x = min(x, DPP_U32(x, 0x142, 0xA));
    x = min(x, DPP_U32(x, 0x143, 0xC));
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t x)
{
    x = max(x, DPP_U32(x, 0xB1, 0xF));
    x = max(x, DPP_U32(x, 0x4E, 0xF));
    x = max(x, DPP_U32(x, 0x141, 0xF));
    x = max(x, DPP_U32(x, 0x140, 0xF));
    x = max(x, DPP_U32(x, 0x142, 0xA));
    x = max(x, DPP_U32(x, 0x143, 0xC));
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}
__device__ __forceinline__ int wave_inclusive_scan(int x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false); // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false); // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false); // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false); // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false); // row_bcast:15 -> rows 1,3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false); // row_bcast:31 -> rows 2,3
    return x;
}

template <int R, typename LD>
__device__ __attribute__((noinline)) int wave_select(LD load, int n, int k, int kmax, int lane, uint32_t *thr_ord, uint64_t *dst)
{
    static_assert(R <= 64, "at most 4096 keys per wave");
    // wave-uniform by contract; arguments of a non-inlined function arrive in VGPRs and the
    // compiler would otherwise run the search loop on lane masks
    n = __builtin_amdgcn_readfirstlane(n);
    k = __builtin_amdgcn_readfirstlane(k);
    kmax = __builtin_amdgcn_readfirstlane(kmax);
    uint32_t hi[R], lo[R];
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int idx = r * 64 + lane;
        const bool valid = idx < n;
        uint64_t key = load(valid ? idx : n - 1); // unconditional: loads go out back to back
        if (!valid) key = KEY_PAD;
        hi[r] = (uint32_t)(key >> 32);
        lo[r] = (uint32_t)key;
        mn = min(mn, hi[r]);              // padding reads as the largest word
        mx = max(mx, valid ? hi[r] : 0u);
        // groups of 16 loads: keeps the address registers of at most 16 loads alive at a time
        if ((r & 15) == 15) __builtin_amdgcn_sched_barrier(0);
    }
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    // per-lane partial counts, one DPP reduction per probe.  The compare/add-carry pair is
    // spelled out: left to the scheduler, R compares are hoisted together and their R lane
    // masks spill out of the SGPR file.
    auto count_lt = [&](uint32_t X) {
        int c = 0;
#pragma unroll
        for (int r = 0; r < R; r++)
            asm volatile("v_cmp_lt_u32_e32 vcc, %1, %2\n\tv_addc_co_u32_e32 %0, vcc, 0, %0, vcc" : "+v"(c) : "v"(hi[r]), "v"(X) : "vcc");
        return wave_sum(c);
    };
    uint32_t T = mx;
    int cnt = n;
    if (mx == 0xFFFFFFFFu && mn != mx) {
        // padded input (merge of per-chunk lists, mostly padding after a seeded scan): if no
        // more than kmax real keys exist they all survive and there is nothing to search;
        // otherwise search only the bit range of the real keys
        const int real = count_lt(0xFFFFFFFFu);
        if (real <= kmax) {
            mn = mx; // skip the search: T = 0xFFFFFFFF keeps every real key
        } else {
            uint32_t mr = 0u;
#pragma unroll
            for (int r = 0; r < R; r++) mr = max(mr, hi[r] == 0xFFFFFFFFu ? 0u : hi[r]);
            mx = wave_max_u32(mr);
            T = mx;
            cnt = real;
        }
    }
    if (mn != mx && cnt > kmax) {
        // Bracket search on the score word for an X with k <= #(keys < X) <= kmax.  f(X) = #(keys < X)
        // is monotone, f(mn) = 0 < k and f(mx + 1) = cnt > kmax.  Probes alternate between linear
        // interpolation of the target rank inside the bracket (scores between mn and mx are close
        // to evenly spread in the order-preserving integer image, so 3-5 probes usually do where
        // an MSB-first bit search spends 15-25, most of them on the empty leading bits) and
        // bisection (so the bracket at least halves every second probe).  A bracket of width one
        // means the k-th key ties with its neighbours on the score word: T is that word exactly and
        // the id tie-break below finishes the job.
        uint32_t lo_x = mn, hi_x = mx + 1u; // mx < 0xFFFFFFFF here (padding was split off above)
        int f_lo = 0, f_hi = cnt;
        const float target = 0.5f * (float)(k + kmax);
        bool interpolate = true, done = false;
        while (hi_x - lo_x > 1u) {
            uint32_t X;
            if (interpolate)
                X = lo_x + (uint32_t)((float)(hi_x - lo_x) * ((target - (float)f_lo) / (float)(f_hi - f_lo)));
            else
                X = lo_x + ((hi_x - lo_x) >> 1);
            X = max(lo_x + 1u, min(X, hi_x - 1u));
            interpolate = !interpolate;
            const int c = count_lt(X);
            if (c < k) {
                lo_x = X;
                f_lo = c;
            } else if (c > kmax) {
                hi_x = X;
                f_hi = c;
            } else {
                T = X - 1u;
                cnt = c;
                done = true;
                break;
            }
        }
        if (!done) { // lo_x is the exact k-th smallest score word
            T = lo_x;
            cnt = f_hi;
        }
    }
    uint32_t Q = 0xFFFFFFFFu;
    const uint32_t Tlt = T; // keys with hi < Tlt are kept unconditionally, hi == T only with lo <= Q
    if (cnt > kmax && T != 0xFFFFFFFFu) { // (padding keys are interchangeable: the bounded store below trims them)
        // more keys tie at T than may be kept: lowest ids win (rare: exact duplicates)
        const int need = k - count_lt(T);
        Q = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t Qt = Q | (1u << bit);
            int c = 0;
#pragma unroll
            for (int r = 0; r < R; r++)
                c += (hi[r] == T && lo[r] < Qt) ? 1 : 0;
            if (wave_sum(c) <= need - 1) Q = Qt;
        }
    }
    // survivors: lane-major packing (order inside a list is irrelevant).  When the cut falls
    // into the padding (fewer than k real keys) only real keys survive; the caller pads.
    int total;
    if (Q == 0xFFFFFFFFu) {
        // common case, no tie-break: keep hi < Tk
        const uint32_t Tk = T == 0xFFFFFFFFu ? T : T + 1u;
        int mine = 0;
#pragma unroll
        for (int r = 0; r < R; r++)
            asm volatile("v_cmp_lt_u32_e32 vcc, %1, %2\n\tv_addc_co_u32_e32 %0, vcc, 0, %0, vcc" : "+v"(mine) : "v"(hi[r]), "v"(Tk) : "vcc");
        const int incl = wave_inclusive_scan(mine);
        int pos = incl - mine;
        total = __builtin_amdgcn_readlane(incl, 63);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (hi[r] < Tk) {
                if (pos < kmax && dst) dst[pos] = ((uint64_t)hi[r] << 32) | lo[r];
                pos++;
            }
        }
    } else {
        int mine = 0;
#pragma unroll
        for (int r = 0; r < R; r++) mine += (hi[r] < Tlt || (hi[r] == T && lo[r] <= Q)) ? 1 : 0;
        const int incl = wave_inclusive_scan(mine);
        int pos = incl - mine;
        total = __builtin_amdgcn_readlane(incl, 63);
#pragma unroll
        for (int r = 0; r < R; r++) {
            if (hi[r] < Tlt || (hi[r] == T && lo[r] <= Q)) {
                if (pos < kmax && dst) dst[pos] = ((uint64_t)hi[r] << 32) | lo[r];
                pos++;
            }
        }
    }
    *thr_ord = T;
    return min(total, kmax);
}

template <typename LD>
__device__ __forceinline__ int wave_select_dispatch(int R, LD load, int n, int k, int kmax, int lane,
                                                    uint32_t *thr_ord, uint64_t *dst)
{
    if (R <= 8) return wave_select<8, LD>(load, n, k, kmax, lane, thr_ord, dst);
    if (R <= 16) return wave_select<16, LD>(load, n, k, kmax, lane, thr_ord, dst);
    return wave_select<32, LD>(load, n, k, kmax, lane, thr_ord, dst); // callers guarantee n <= 2048
}

// The merge kernel may also use 64 keys per lane (4096 keys): it is its own kernel, so the
// 250 registers of that variant do not cost the scan kernels their second wave per SIMD
// (a non-inlined callee's registers count for every kernel that can reach it).
template <int RMAX, typename LD>
__device__ __forceinline__ int wave_select_dispatch_max(int R, LD load, int n, int k, int kmax, int lane,
                                                        uint32_t *thr_ord, uint64_t *dst)
{
    if constexpr (RMAX <= 16) {
        if (R <= 8) return wave_select<8, LD>(load, n, k, kmax, lane, thr_ord, dst);
        return wave_select<16, LD>(load, n, k, kmax, lane, thr_ord, dst);
    } else if constexpr (RMAX <= 32) {
        return wave_select_dispatch(R, load, n, k, kmax, lane, thr_ord, dst);
    } else {
        if (R <= 32) return wave_select_dispatch(R, load, n, k, kmax, lane, thr_ord, dst);
        return wave_select<64, LD>(load, n, k, kmax, lane, thr_ord, dst);
    }
}

// Keeps the keys of a list whose score word is <= T (packed to the front, in place), one wave, registers only.
// Used at the end of a chunk of a tile-minimum-seeded scan: the first tiles were appended before any bound existed,
// by now the shared threshold is tight and a compare does what a selection would.
template <int R>
__device__ __attribute__((noinline)) int wave_filter(uint64_t *lst, int n, uint32_t T, int lane)
{
    n = __builtin_amdgcn_readfirstlane(n);
    T = __builtin_amdgcn_readfirstlane(T);
    uint64_t key[R];
    int mine = 0;
#pragma unroll
    for (int r = 0; r < R; r++) {
        const int idx = r * 64 + lane;
        key[r] = idx < n ? ((gptr_u64)lst)[idx] : KEY_PAD;
        if ((r & 15) == 15) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int r = 0; r < R; r++) mine += (key[r] != KEY_PAD && (uint32_t)(key[r] >> 32) <= T) ? 1 : 0;
    const int incl = wave_inclusive_scan(mine);
    int pos = incl - mine;
#pragma unroll
    for (int r = 0; r < R; r++)
        if (key[r] != KEY_PAD && (uint32_t)(key[r] >> 32) <= T) lst[pos++] = key[r];
    return __builtin_amdgcn_readlane(incl, 63);
}
__device__ __forceinline__ int wave_filter_dispatch(int R, uint64_t *lst, int n, uint32_t T, int lane)
{
    if (R <= 8) return wave_filter<8>(lst, n, T, lane);
    if (R <= 16) return wave_filter<16>(lst, n, T, lane);
    return wave_filter<32>(lst, n, T, lane);
}

// The same selection for arrays too long for one wave's registers (up to 4096 keys: lists of a search with k in
// (1536, 2048], 4096 published keys): nothing is cached, every probe re-reads the array (64-bit loads, coalesced, L2
// hits; eight in flight per lane).  A handful of probes of <= 64 loads per lane against a workgroup-wide LDS sort of
// 4096 keys (78 barrier-separated stages) that kept all four waves on one query.  Same contract as wave_select:
// keeps k .. kmax keys (the k best among them), packed to the front of dst, unsorted; dst may be the array itself --
// the packing of iteration r writes below index 64 (r + 1), all of which has been read by then.
template <typename LD>
__device__ __attribute__((noinline)) int wave_select_mem(LD load, int n, int k, int kmax, int lane, uint32_t *thr_ord, uint64_t *dst)
{
    n = __builtin_amdgcn_readfirstlane(n);
    k = __builtin_amdgcn_readfirstlane(k);
    kmax = __builtin_amdgcn_readfirstlane(kmax);
    const int iters = (n + 63) >> 6;
    // fn(key, valid) for every key of this lane, eight loads in flight
    auto for_each = [&](auto &&fn) {
        int r = 0;
        for (; r + 8 <= iters; r += 8) {
            uint64_t v[8];
#pragma unroll
            for (int u = 0; u < 8; u++) {
                const int idx = (r + u) * 64 + lane;
                v[u] = load(idx < n ? idx : n - 1);
                if (idx >= n) v[u] = KEY_PAD;
            }
#pragma unroll
            for (int u = 0; u < 8; u++) fn(v[u]);
        }
        for (; r < iters; r++) {
            const int idx = r * 64 + lane;
            uint64_t v = load(idx < n ? idx : n - 1);
            if (idx >= n) v = KEY_PAD;
            fn(v);
        }
    };
    uint32_t mn = 0xFFFFFFFFu, mx = 0u;
    int real = 0;
    for_each([&](uint64_t key) {
        const uint32_t hi = (uint32_t)(key >> 32);
        mn = min(mn, hi);
        if (hi != 0xFFFFFFFFu) {
            mx = max(mx, hi);
            real++;
        }
    });
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    real = wave_sum(real); // keys whose score word is not the padding word
    auto count_lt = [&](uint32_t X) {
        int c = 0;
        for_each([&](uint64_t key) { c += (uint32_t)(key >> 32) < X ? 1 : 0; });
        return wave_sum(c);
    };
    uint32_t T = 0xFFFFFFFFu; // keep every key with score word <= T (0xFFFFFFFF: every real key)
    int cnt = real;
    if (real > kmax && mn != mx) {
        uint32_t lo_x = mn, hi_x = mx + 1u;
        int f_lo = 0, f_hi = real;
        const float target = 0.5f * (float)(k + kmax);
        bool interpolate = true, done = false;
        while (hi_x - lo_x > 1u) {
            uint32_t X;
            if (interpolate)
                X = lo_x + (uint32_t)((float)(hi_x - lo_x) * ((target - (float)f_lo) / (float)(f_hi - f_lo)));
            else
                X = lo_x + ((hi_x - lo_x) >> 1);
            X = max(lo_x + 1u, min(X, hi_x - 1u));
            interpolate = !interpolate;
            const int c = count_lt(X);
            if (c < k) {
                lo_x = X;
                f_lo = c;
            } else if (c > kmax) {
                hi_x = X;
                f_hi = c;
            } else {
                T = X - 1u;
                cnt = c;
                done = true;
                break;
            }
        }
        if (!done) { // lo_x is the exact k-th smallest score word
            T = lo_x;
            cnt = f_hi;
        }
    } else if (real > kmax) {
        T = mn; // every real key carries the same score word: the id tie-break below decides
    }
    uint32_t Q = 0xFFFFFFFFu;
    if (cnt > kmax && T != 0xFFFFFFFFu) {
        // more keys tie at T than may be kept: lowest ids win
        const int need = k - count_lt(T);
        Q = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const uint32_t Qt = Q | (1u << bit);
            int c = 0;
            for_each([&](uint64_t key) { c += ((uint32_t)(key >> 32) == T && (uint32_t)key < Qt) ? 1 : 0; });
            if (wave_sum(c) <= need - 1) Q = Qt;
        }
    }
    // survivors, 64 keys per step, packed in place with a ballot (see above for why dst may alias the array)
    int base = 0;
    for (int r = 0; r < iters; r++) {
        const int idx = r * 64 + lane;
        uint64_t key = load(idx < n ? idx : n - 1);
        if (idx >= n) key = KEY_PAD;
        const uint32_t hi = (uint32_t)(key >> 32);
        const bool keep = hi != 0xFFFFFFFFu && (hi < T || (hi == T && (uint32_t)key <= Q));
        const unsigned long long m = __ballot(keep);
        const int pos = base + __popcll(m & ((1ull << lane) - 1ull));
        if (keep && pos < kmax && dst) dst[pos] = key;
        base += __popcll(m);
    }
    *thr_ord = T;
    return min(base, kmax);
}

// ... and the threshold filter for such an array: keeps the keys with score word <= T, packed in place
__device__ __attribute__((noinline)) int wave_filter_mem(uint64_t *lst, int n, uint32_t T, int lane)
{
    n = __builtin_amdgcn_readfirstlane(n);
    T = __builtin_amdgcn_readfirstlane(T);
    int base = 0;
    for (int r = 0; r < (n + 63) >> 6; r++) {
        const int idx = r * 64 + lane;
        const uint64_t key = idx < n ? ((gptr_u64)lst)[idx] : KEY_PAD;
        const bool keep = key != KEY_PAD && (uint32_t)(key >> 32) <= T;
        const unsigned long long m = __ballot(keep);
        if (keep) lst[base + __popcll(m & ((1ull << lane) - 1ull))] = key;
        base += __popcll(m);
    }
    return base;
}

// The bound of a tile-minimum seed: the k-th smallest of the keys published so far (one call site in the scan kernel:
// a second one -- the memory-probing variant next to the register variant -- cost a 1.25 M-row launch 70 us)
__device__ __attribute__((noinline)) void published_bound(const uint64_t *pub, int n, int k, int kmax, int lane, uint32_t *thr_ord)
{
    n = __builtin_amdgcn_readfirstlane(n);
    if (n <= 2048) wave_select_dispatch((n + 63) >> 6, LoadAgent{pub}, n, k, kmax, lane, thr_ord, (uint64_t *)nullptr);
    else wave_select_mem(LoadAgent{pub}, n, k, kmax, lane, thr_ord, (uint64_t *)nullptr);
}

// ---------------------------------------------------------------------------
// scan kernel
// ---------------------------------------------------------------------------
struct ScanParams {
    const float *xb;   // [nb][dp] database rows, zero padded to dp
    const float *yn;   // [nb] squared norms (L2 only)
    const float *xq;   // [nq][dp] queries
    const float *xn;   // [nq] squared norms (L2 only)
    const float *xq_diff; // difference builds: [DNQ][dp] the queries interleaved by pairs (diff_interleave_kernel)
    int64_t nb, nq;
    int dp;            // multiple of 32
    int k;
    int cap;           // candidate list capacity per (workgroup, query); power of two
    int nqtiles, nchunks;
    int tiles_base, tiles_rem; // chunk c walks tiles_base (+1 if c < tiles_rem) database tiles: a balanced split
    uint64_t *lists;   // [grid][QT][cap]
    uint32_t *gthr;    // [nqtiles*QT] shared running thresholds (order-mapped floats)
    uint64_t *qlist;   // [nq][qcap] compact candidate arrays: the chunks' survivors, appended as they finish
    uint32_t *qcnt;    // [nq] fill of each array
    int qcap;
    uint32_t id_base;
    int row_mul;       // this launch scans a block-strided view of the database, see view_row()
    int vshift;        // log2 of the view's block size (3: blocks of 8 rows, 0: single rows)
    int skip_mask;     // >= 0: rows whose block b has (b & skip_mask) == 0 belong to the seed sample, skip them
    int kslot;         // most keys a chunk hands on per query: k + k/4
    const struct SymItem *sym_items; // symmetric all-vs-all launch: the work of each workgroup (plan.h; see flat_scan_kernel)
    int *fail;         // symmetric launch: set when a candidate array overflows
    // tile-minimum seed (streaming regime, see flat_scan_kernel): after each of its first pub_rounds tiles a workgroup
    // publishes every query's best key of that tile; the k-th smallest published key bounds the global k-th
    uint64_t *pub;     // [nqtiles*QT][pub_n], pub_n = pub_rounds * nchunks, KEY_PAD = not published yet; NULL: off
    uint32_t *arrive;  // [nqtiles] publications so far
    int pub_n, pub_rounds;
    int pub_m;         // keys a workgroup publishes per query and round: 1 (the tile's best) or WM (each wave's best of its own rows)
    float *defer;      // [grid][QT * DT] the parked scores of every workgroup's first tile
    // paired workgroups (one-query-tile launches): workgroups w and w + npairs share ONE range of tiles, w walks it from
    // the front, w + npairs from the back; every tile is claimed with a ticket (see flat_scan_kernel)
    uint32_t *pair_ctr; // [npairs] tickets handed out so far (starts at 2: the first tile of either side); NULL: off
                        // pair_ctr[npairs]: tickets of the pool
    int npairs;
    int pool_tiles;     // the last pool_tiles tiles of every pair's range belong to a pool shared by ALL workgroups
    uint32_t *cu_turn;  // [2048] batch launches: one word per CU -- the two resident workgroups take turns in their K loops; NULL: off
    // 16-bit prefilter (F16X build, see flat_scan_kernel): per-row / per-query power-of-two exponents of the fp16 copies
    const int8_t *xexp;
    const int *qexp;
    // gated launch (the fp32 fallback behind a 16-bit prefiltered search): the kernel returns at once unless one of
    // gate[0 .. gate_n) is set; NULL: always runs
    const uint32_t *gate;
    int gate_n;
    int sparse_epi;     // 128 x 128 batch builds: filter the tiles through the sparse epilogue (thresholds that let a percent of the
                        // scores pass: statistical seed, no seed) instead of filter_tile (exactly seeded scans: almost nothing passes,
                        // its wave-wide early-outs cost next to nothing; the sparse epilogue's fixed 2 us per tile cost a 10 M-row
                        // scan of 1024 queries 4 %)
#ifdef KNN355_TRACE
    int ablate;                // developer build: 1 = skip the filter, 2 = masks only (no reservations / stores), 4 = wait for the accumulators before the stamp
    unsigned long long *trace; // developer build: [grid][128] wall-clock stamps (100 MHz) of each workgroup's progress (64.. : inside the epilogue)
#endif
};
#ifdef KNN355_TRACE
#define KNN_TRACE(slot) do { if (threadIdx.x == 0 && p.trace && (slot) < 128) p.trace[(size_t)blockIdx.x * 128 + (slot)] = wall_clock64(); } while (0)
#define KNN_TRACE_AT(cond, slot) do { if (cond) KNN_TRACE(slot); } while (0)
#define KNN_TRACE_COUNT(cond, slot) do { if (threadIdx.x == 0 && p.trace && (cond)) p.trace[(size_t)blockIdx.x * 128 + (slot)] += 1; } while (0)
#else
#define KNN_TRACE(slot) do { } while (0)
#define KNN_TRACE_AT(cond, slot) do { } while (0)
#define KNN_TRACE_COUNT(cond, slot) do { } while (0)
#endif

// Views: view row r of a launch with stride row_mul and block size B = 1 << vshift is database row
// (r / B) * B * row_mul + r % B -- blocks of B consecutive rows, every row_mul-th block (row_mul = 1:
// the database itself).  Seed samples of the streaming regime use blocks of 8 rows, because one
// staging instruction fetches 8 rows: 8 rows 32 KB apart in one page instead of 8 pages (a
// row-strided sample of a 41 GB database ran at 1.9 TB/s, bound by address translation); the
// statistical samples of the batch regime use single rows (a stratified sample of a database
// whose families sit next to each other).
__host__ __device__ __forceinline__ int64_t view_row(int64_t r, int row_mul, int vshift)
{
    return ((r >> vshift) * row_mul << vshift) + (r & (((int64_t)1 << vshift) - 1));
}

// ---- per-workgroup candidate lists shared by the scan kernels -------------------------
// s_thr / s_cnt / s_need live in LDS, the lists themselves in global memory (L2).
struct ListCtx {
    float *s_thr;     // [QT] local admission threshold (value of the loosest kept key)
    int *s_cnt;       // [QT] list fill
    int *s_need;      // some list could overflow on the next tile
    uint64_t *lists;  // [QT][cap] this workgroup's lists
    uint32_t *gthr;   // [QT] shared running thresholds of these queries
    int cap, k;
    int kslot;        // size of this workgroup's output slot per query (k + k/4)
    bool prefilter;   // end of chunk: drop what the shared threshold has overtaken before any selection

    __device__ __forceinline__ void init(int tid, int QT, int nthreads = 256)
    {
        for (int i = tid; i < QT; i += nthreads) {
            s_thr[i] = INFINITY;
            s_cnt[i] = 0;
        }
        if (tid == 0) *s_need = 0;
        prefilter = false;
    }
    __device__ __forceinline__ float threshold(int ql) const
    {
        const uint32_t g = __hip_atomic_load(&gthr[ql], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return fminf(s_thr[ql], ord2f(g));
    }
    // v: "smaller is better" score of row `id` for local query ql (caller checked v <= threshold)
    __device__ __forceinline__ void append(int ql, float v, uint32_t id, int tile_rows)
    {
        v = v + 0.0f;
        const int slot = atomicAdd(&s_cnt[ql], 1);
        if (slot < cap) lists[(size_t)ql * cap + slot] = ((uint64_t)f2ord(v) << 32) | id;
        if (slot + 1 > cap - tile_rows) *s_need = 1;
    }
};

// Called by all threads after a tile's appends (and a barrier).  Lists that could overflow on the
// next tile are cut back to the best [k, min(1.25k, cap - tile)] keys; with `final` set (end of the
// chunk) every list longer than kslot is cut to at most kslot keys instead.  Cuts happen in place
// (survivors packed to the front of the list, unsorted); exactness is the final selection's job.
template <int QT, int NT = 256>
__device__ __forceinline__ void lists_compact(ListCtx &L, char *smem, int tile_rows, bool final, int tid)
{
    const int lane = tid & 63, wave = tid >> 6;
    const int R = L.cap >> 6;
    if (R <= 64) {
        // one wave per query: one query in flight per wave of the workgroup.  Lists of up to 2048 keys are selected in
        // registers, the 4096-key lists of k in (1536, 2048] by probing the list in memory (wave_select_mem)
        auto select = [&](uint64_t *lst, int n, int kmax, uint32_t *T) -> int {
            if (R <= 32) return wave_select_dispatch(R, LoadContig{lst}, n, L.k, kmax, lane, T, lst);
            return wave_select_mem(LoadContig{lst}, n, L.k, kmax, lane, T, lst);
        };
        for (int ql = wave; ql < QT; ql += NT / 64) {
            const int n = __builtin_amdgcn_readfirstlane(min(L.s_cnt[ql], L.cap));
            uint64_t *lst = L.lists + (size_t)ql * L.cap;
            uint32_t T = 0;
            int kmax;
            if (!final) {
                if (n <= L.cap - tile_rows) continue;
                // at most cap - tile_rows keys may stay: the next tile can append tile_rows more
                // (k in (1433, 1536] with 256-row tiles: 1.25 k alone would leave too little room)
                kmax = min(L.k + (L.k >> 2), L.cap - tile_rows);
            } else {
                if (n <= L.kslot) {
                    if (lane == 0) L.s_cnt[ql] = n;
                    continue;
                }
                kmax = L.kslot;
                if (L.prefilter) {
                    const int m = R <= 32 ? wave_filter_dispatch(R, lst, n, f2ord(L.threshold(ql)), lane)
                                          : wave_filter_mem(lst, n, f2ord(L.threshold(ql)), lane);
                    if (m <= L.kslot) {
                        if (lane == 0) L.s_cnt[ql] = m;
                        continue;
                    }
                    const int cnt2 = select(lst, m, kmax, &T);
                    if (lane == 0) {
                        L.s_cnt[ql] = cnt2;
                        if (T != 0xFFFFFFFFu) { // (0xFFFFFFFF: the list held no more than kmax real keys beside its KEY_PAD entries -- no bound, and ord2f of it is a NaN)
                            L.s_thr[ql] = ord2f(T);
                            atomicMin(&L.gthr[ql], T);
                        }
                    }
                    continue;
                }
            }
            const int cnt = select(lst, n, kmax, &T);
            if (lane == 0) {
                L.s_cnt[ql] = cnt;
                if (T != 0xFFFFFFFFu) { // (see above: a cut that fell into the padding gives no bound)
                    L.s_thr[ql] = ord2f(T);
                    atomicMin(&L.gthr[ql], T);
                }
            }
        }
        __syncthreads();
    } else {
        // lists longer than 4096 keys (no plan makes them: k <= 2048): whole-workgroup LDS sort
        uint64_t *sb = (uint64_t *)smem;
        for (int ql = 0; ql < QT; ql++) {
            const int n = min(L.s_cnt[ql], L.cap);
            if (!final && n <= L.cap - tile_rows) continue;
            if (final && n <= L.kslot) {
                if (tid == 0) L.s_cnt[ql] = n; // (readers clamp with cap themselves: old or new value, same n)
                continue;
            }
            uint64_t *lst = L.lists + (size_t)ql * L.cap;
            const int P = next_pow2_dev(n > 0 ? n : 1);
            for (int i = tid; i < P; i += NT) sb[i] = i < n ? lst[i] : KEY_PAD;
            __syncthreads();
            wg_bitonic_sort(sb, P, tid, NT);
            const int keep = min(n, L.k);
            for (int i = tid; i < keep; i += NT) lst[i] = sb[i];
            if (tid == 0) {
                L.s_cnt[ql] = keep;
                if (n >= L.k) {
                    const uint32_t o = (uint32_t)(sb[L.k - 1] >> 32);
                    if (o != 0xFFFFFFFFu) { // (a list may hold KEY_PAD entries -- rows that are not there: fewer than k real keys, no bound)
                        L.s_thr[ql] = ord2f(o);
                        atomicMin(&L.gthr[ql], o);
                    }
                }
            }
            __syncthreads();
        }
    }
    if (tid == 0) *L.s_need = 0;
    __syncthreads();
}

// End of a chunk (after lists_compact(final)): every query's survivors are appended to its compact
// candidate array qlist[q][0 .. qcap) behind whatever other chunks (and the seed sample) have put
// there: one atomic add per (workgroup, query) reserves the slots, then the keys are copied, one
// wave per query.  qcap = (lists per query) x kslot: the reservations can never run past it.
template <int QT, int NT = 256>
__device__ __forceinline__ void lists_flush(ListCtx &L, int *s_base, int64_t q0, int64_t nq, uint64_t *qlist, uint32_t *qcnt,
                                            int qcap, int tid, int *fail = nullptr)
{
    const int lane = tid & 63, wave = tid >> 6;
    const int nqv = (int)min((int64_t)QT, nq - q0);
    for (int ql = tid; ql < nqv; ql += NT) {
        const int n = L.s_cnt[ql];
        s_base[ql] = n > 0 ? (int)atomicAdd(&qcnt[q0 + ql], (uint32_t)n) : 0;
    }
    __syncthreads();
    // four queries per step and wave: their loads go out together (one query at a time, a 128-query workgroup spent 57 us
    // here waiting for 64 dependent round trips to L2 -- 3 % of a CATH-sized symmetric launch with its short runs)
    constexpr int NW = NT / 64, U = 4;
    for (int ql0 = wave; ql0 < nqv; ql0 += NW * U) {
        uint64_t v[U][2];
        int n[U], base[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int ql = ql0 + u * NW;
            n[u] = ql < nqv ? L.s_cnt[ql] : 0;
            base[u] = ql < nqv ? s_base[ql] : 0;
            const uint64_t *lst = L.lists + (size_t)(ql < nqv ? ql : 0) * L.cap;
#pragma unroll
            for (int j = 0; j < 2; j++) v[u][j] = lane + 64 * j < n[u] ? ((gptr_u64)lst)[lane + 64 * j] : KEY_PAD;
        }
#pragma unroll
        for (int u = 0; u < U; u++) {
            const int ql = ql0 + u * NW;
            if (ql >= nqv) continue;
            const uint64_t *lst = L.lists + (size_t)ql * L.cap;
            uint64_t *dst = qlist + (size_t)(q0 + ql) * qcap + base[u];
#pragma unroll
            for (int j = 0; j < 2; j++)
                if (lane + 64 * j < n[u] && base[u] + lane + 64 * j < qcap) dst[lane + 64 * j] = v[u][j];
            for (int i = lane + 128; i < n[u]; i += 64)
                if (base[u] + i < qcap) dst[i] = lst[i];
            // (only a symmetric launch sizes the arrays by expectation: an overflow there repeats the search the plain way)
            if (fail && lane == 0 && base[u] + n[u] > qcap) *fail = 1;
        }
    }
}

// one staging instruction: 64 lanes x 16 B straight from global memory into LDS (LDS-DMA, no VGPR
// round trip).  NT (aux bit 1 = non-temporal): for data that is read once.
template <bool NT = false>
__device__ __forceinline__ void stage_issue(const float *src, char *lds_wave_base)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src,
                                     (__attribute__((address_space(3))) void *)lds_wave_base, 16, 0, NT ? 2 : 0);
}

// scheduling pattern "one MFMA, one LDS read", N times: a sub-step's fragment reads go out one per MFMA -- four waves that
// issue eight ds_read_b128 each in one burst keep the LDS array busy for two MFMA times (one wave per SIMD: 3.5 % of the
// 256 x 256 tile's K loop, measured by ablation)
template <int N>
__device__ __forceinline__ void sched_reads()
{
    if constexpr (N > 0) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        sched_reads<N - 1>();
    }
}

// scheduling pattern "PER MFMAs, one vector-memory instruction", N times
template <int N, int PER>
__device__ __forceinline__ void sched_spread()
{
    if constexpr (N > 0) {
        __builtin_amdgcn_sched_group_barrier(0x008, PER, 0);
        __builtin_amdgcn_sched_group_barrier(0x010, 1, 0);
        sched_spread<N - 1, PER>();
    }
}

// Pass 1 of flat_scan_kernel's sparse epilogue: ONE asm statement for four scores, put together from pieces.  A head leaves
// the values in t0..t3 (accumulators in AGPRs or VGPRs, squared L2 or inner product); a bound leaves the compare masks in
// m0..m3 (THR: the query's threshold; ROW, the second direction: each row's own, -inf for a lane whose query is no candidate);
// the tail is every build's: slot address and pointer bump, score number, store.  The operand lists follow the pieces (in_l2
// and out_bound may be empty), so a build names only what its text uses.  All of them name locals of pass1.
#define KNN_P1_HEAD_AGPR_L2 "v_accvgpr_read_b32 %[t0], %[a0]\n\t" "v_accvgpr_read_b32 %[t1], %[a1]\n\t" "v_accvgpr_read_b32 %[t2], %[a2]\n\t" "v_accvgpr_read_b32 %[t3], %[a3]\n\t" \
    "v_fma_f32 %[t0], %[t0], -2.0, %[s0]\n\t" "v_fma_f32 %[t1], %[t1], -2.0, %[s1]\n\t" "v_fma_f32 %[t2], %[t2], -2.0, %[s2]\n\t" "v_fma_f32 %[t3], %[t3], -2.0, %[s3]\n\t"
#define KNN_P1_HEAD_AGPR_IP "v_accvgpr_read_b32 %[t0], %[a0]\n\t" "v_accvgpr_read_b32 %[t1], %[a1]\n\t" "v_accvgpr_read_b32 %[t2], %[a2]\n\t" "v_accvgpr_read_b32 %[t3], %[a3]\n\t" \
    "v_xor_b32_e32 %[t0], 0x80000000, %[t0]\n\t" "v_xor_b32_e32 %[t1], 0x80000000, %[t1]\n\t" "v_xor_b32_e32 %[t2], 0x80000000, %[t2]\n\t" "v_xor_b32_e32 %[t3], 0x80000000, %[t3]\n\t"
#define KNN_P1_HEAD_VGPR_L2 "v_fma_f32 %[t0], %[a0], -2.0, %[s0]\n\t" "v_fma_f32 %[t1], %[a1], -2.0, %[s1]\n\t" "v_fma_f32 %[t2], %[a2], -2.0, %[s2]\n\t" "v_fma_f32 %[t3], %[a3], -2.0, %[s3]\n\t" // (the 128 x 128 tile's accumulators are VGPRs: read in place)
#define KNN_P1_HEAD_VGPR_IP "v_xor_b32_e32 %[t0], 0x80000000, %[a0]\n\t" "v_xor_b32_e32 %[t1], 0x80000000, %[a1]\n\t" "v_xor_b32_e32 %[t2], 0x80000000, %[a2]\n\t" "v_xor_b32_e32 %[t3], 0x80000000, %[a3]\n\t"
#define KNN_P1_BOUND_THR "v_cmp_le_f32_e64 %[m0], %[t0], %[thr]\n\t" "v_cmp_le_f32_e64 %[m1], %[t1], %[thr]\n\t" "v_cmp_le_f32_e64 %[m2], %[t2], %[thr]\n\t" "v_cmp_le_f32_e64 %[m3], %[t3], %[thr]\n\t"
#define KNN_P1_BOUND_ROW "v_cndmask_b32_e64 %[e0], %[ninf], %[h0], %[cok]\n\t" "v_cndmask_b32_e64 %[e1], %[ninf], %[h1], %[cok]\n\t" "v_cndmask_b32_e64 %[e2], %[ninf], %[h2], %[cok]\n\t" "v_cndmask_b32_e64 %[e3], %[ninf], %[h3], %[cok]\n\t" \
    "v_cmp_le_f32_e64 %[m0], %[t0], %[e0]\n\t" "v_cmp_le_f32_e64 %[m1], %[t1], %[e1]\n\t" "v_cmp_le_f32_e64 %[m2], %[t2], %[e2]\n\t" "v_cmp_le_f32_e64 %[m3], %[t3], %[e3]\n\t"
#define KNN_P1_TAIL "v_min_u32_e32 %[ad0], %[w], %[dump]\n\t" "v_cndmask_b32_e64 %[u], 0, %[step], %[m0]\n\t" "v_add_u32_e32 %[w], %[w], %[u]\n\t" \
    "v_min_u32_e32 %[ad1], %[w], %[dump]\n\t" "v_cndmask_b32_e64 %[u], 0, %[step], %[m1]\n\t" "v_add_u32_e32 %[w], %[w], %[u]\n\t" \
    "v_min_u32_e32 %[ad2], %[w], %[dump]\n\t" "v_cndmask_b32_e64 %[u], 0, %[step], %[m2]\n\t" "v_add_u32_e32 %[w], %[w], %[u]\n\t" \
    "v_min_u32_e32 %[ad3], %[w], %[dump]\n\t" "v_cndmask_b32_e64 %[u], 0, %[step], %[m3]\n\t" "v_add_u32_e32 %[w], %[w], %[u]\n\t" \
    "v_mov_b32_e32 %[i0], %[idx0]\n\t" "v_mov_b32_e32 %[i1], %[idx1]\n\t" "v_mov_b32_e32 %[i2], %[idx2]\n\t" "v_mov_b32_e32 %[i3], %[idx3]\n\t" \
    "ds_write2_b32 %[ad0], %[t0], %[i0] offset1:1\n\t" "ds_write2_b32 %[ad1], %[t1], %[i1] offset1:1\n\t" "ds_write2_b32 %[ad2], %[t2], %[i2] offset1:1\n\t" "ds_write2_b32 %[ad3], %[t3], %[i3] offset1:1"
#define KNN_P1_OUT_ROW , [e0] "=&v"(e[0]), [e1] "=&v"(e[1]), [e2] "=&v"(e[2]), [e3] "=&v"(e[3])
#define KNN_P1_IN_L2 , [s0] "v"(s0), [s1] "v"(s1), [s2] "v"(s2), [s3] "v"(s3)
#define KNN_P1_IN_THR , [thr] "v"(thr[b])
#define KNN_P1_IN_ROW , [h0] "v"(t2l[sc - c + 0]), [h1] "v"(t2l[sc - c + 1]), [h2] "v"(t2l[sc - c + 2]), [h3] "v"(t2l[sc - c + 3]), [ninf] "v"(ninf), [cok] "s"(cokm[b])
#define KNN_PASS1(head, bound, out_bound, acc_reg, in_l2, in_bound) asm volatile(head bound KNN_P1_TAIL \
    : [t0] "=&v"(t[0]), [t1] "=&v"(t[1]), [t2] "=&v"(t[2]), [t3] "=&v"(t[3]), [ad0] "=&v"(ad[0]), [ad1] "=&v"(ad[1]), [ad2] "=&v"(ad[2]), [ad3] "=&v"(ad[3]), [i0] "=&v"(ix[0]), [i1] "=&v"(ix[1]), [i2] "=&v"(ix[2]), [i3] "=&v"(ix[3]), [m0] "=&s"(mk[0]), [m1] "=&s"(mk[1]), [m2] "=&s"(mk[2]), [m3] "=&s"(mk[3]), [u] "=&v"(u), [w] "+v"(w) out_bound \
    : [a0] acc_reg(a0), [a1] acc_reg(a1), [a2] acc_reg(a2), [a3] acc_reg(a3) in_l2 in_bound, [dump] "v"(dump), [step] "v"(step), [idx0] "n"((sc + 0) | (b << 8)), [idx1] "n"((sc + 1) | (b << 8)), [idx2] "n"((sc + 2) | (b << 8)), [idx3] "n"((sc + 3) | (b << 8)) : "memory")

// WM x WN waves; each wave owns TM x TN MFMA tiles of 32(db rows) x 32(queries)
// NTDB: the launch has ONE query tile, so every database row is read by exactly one workgroup:
// its staging loads are non-temporal and do not displace the queries (re-read by every workgroup
// each K step) from L2 / Infinity Cache -- 10 M x 32 queries +4 %.  With several query tiles the
// workgroups of a chunk share the rows through L2 and non-temporal loads cost 3 %.
// SYM: all-vs-all with the index's own rows as queries.  dot(x, y) = dot(y, x) bit for bit (the chain multiplies the same
// pairs in the same order) and nrm(x) + nrm(y) commutes, so the score tile of (query tile I, database tile J) also holds
// the scores of (query tile J, database tile I): only the tiles on and above the diagonal are multiplied -- half the
// MFMA work.  Every off-diagonal tile is filtered twice: lane-wise for the queries of tile I (the resident tile, as
// always), and row-wise for the rows of tile J taken as queries, whose survivors go straight to those queries' compact
// arrays (they have no workgroup-local list here: the statistical seed keeps them few, an overflow raises the
// verification flag and the search is redone the plain way).
// BF16: the operands are bf16 copies of the rows (an index made approximate on purpose: the coarse entry scan of the
// HNSW index, where only the neighbourhood matters and every returned distance is re-scored exactly afterwards).
// A staged 128-byte row segment then holds 64 values instead of 32, the same 16-byte fragment feeds ONE
// v_mfma_f32_32x32x16_bf16 instead of four fp32 MFMAs (1/16 of the matrix time), and everything else -- staging,
// swizzle, lists, thresholds, selection -- is shared.  p.dp counts 4-byte units of a row here (d / 2).
// DNQ > 0 ("DIFF"): FAISS's squared L2 for batches of fewer than 20 queries (distance_compute_blas_threshold [ext]; reachable
// through seqvec_search/main.py:22-45 with metric=METRIC_L2 and a handful of queries): the sum of (x - y)^2 itself, not
// |x|^2 + |y|^2 - 2<x,y>.  Contract: ONE fp32 chain per (query, row), acc = fma(t, t, acc) with t = x[k] - y[k], k in the
// same order as the dot product (0,4,1,5,2,6,3,7 per block of 8).  No matrix instruction computes that: the 32-query
// tile's staging, lists, thresholds, seeding and selection are kept and the K step's MFMAs are replaced by vector
// subtract / fma chains -- thread = two rows of the 256-row tile (their 32 floats of the K step in registers), one chain per
// (query, row), the queries' floats read from LDS as broadcasts.  Behind the K loop the scores are transposed through the
// staging buffers into the accumulator layout the MFMA would have left (lane (i, h) = query i, registers = 32 rows), so the
// filter, the tile-minimum seed and everything else are shared.  The chains of the two queries of a PAIR against one row
// share packed fp32 instructions (v_pk_add_f32 / v_pk_fma_f32; round 4 -- round 3 packed two rows of one query: 12.2 ms per
// 10 M x 1024 rows for 13-19 queries, bound by LDS bank conflicts; scalar chains: 19.4; the MFMA scan with the norm formula:
// 7.0-7.4 ms); builds for up to 12 and up to 4 queries (a single query: its HBM time).
// Q16 > 0: the wave's query columns are Q16 blocks of SIXTEEN (v_mfma_f32_16x16x4_f32 -- the same k-ordered fma chain, bit for
// bit: tools/micro/mfma16.hip; lane (i, g = lane / 16) feeds k = g of each instruction: floats 8t + {0, 4, 1, 5}[g] and
// 8t + {2, 6, 3, 7}[g] per block of 8) instead of TN blocks of 32: a 48-query tile (4 x 1 waves, 33..48 queries) and a
// 96-query tile (2 x 2 waves, 65..96 queries) pay for 48 / 96 columns of matrix work, not 64 / 128.  One-query-tile launches
// only (plain fp32).
// TM x TN = 4 x 4 ("BIG", round 5): a 256 x 256 tile on four waves, ONE workgroup per CU, one wave per SIMD with up to 512
// registers -- 256 of them the wave's 128 x 128 accumulators (AGPRs), 128 KB of LDS for the two staging buffers.  Half the
// staged bytes per flop of the 128 x 128 tile, a quarter of the K-step barriers and first-fragment waits per flop; nothing
// else on the CU fills the epilogue's gaps, so this build is for long chunks only (make_plan).
// F16X: the exact 16-bit prefilter.  The operands are fp16 copies of rows and queries, each scaled by a power
// of two of its own (xexp / qexp), staged and multiplied like the BF16 build (v_mfma_f32_32x32x16_f16), but with everything
// of the fp32 streaming build kept: paired walk, pool, tile-minimum seed, parked first tile.  Behind the K loop one ldexp per
// accumulator register turns the scaled dot products into approximate scores; from there on the build is the fp32 one, run
// with k' > k.  Its output is the exact top-k' of the APPROXIMATE scores, which the re-scoring tail checks against the
// error bound and scores exactly (rescore16_kernel).  Inner product, one 32-query tile per launch.
template <int WM, int WN, int TM, int TN, bool L2, bool NTDB = false, bool SYM = false, bool BF16 = false, int DNQ = 0, int Q16 = 0, bool F16X = false, bool X12 = false>
__global__ __launch_bounds__(256, (TM * TN >= 16 ? 1 : 2)) void flat_scan_kernel(ScanParams p)
{
    if (p.gate) { // (a gated fallback launch: uniform over the workgroup, in front of every barrier)
        uint32_t any = 0;
        for (int i = 0; i < p.gate_n; i++) any |= p.gate[i];
        if (!any) return;
    }
    constexpr bool DIFF = DNQ > 0; // the difference build, for batches of up to DNQ queries (8, 12, 16 or 20)
    static_assert(!F16X || (NTDB && !L2 && !SYM && !BF16 && DNQ == 0 && Q16 == 0 && TN == 1), "the 16-bit prefilter: one query tile, inner product");
    static_assert(!X12 || (F16X && WM == 4 && TM == 2), "the 12-bit row copies: the prefilter's 256-row tile");
    constexpr bool H16 = BF16 || F16X; // 16-bit operands: a staged 128-byte segment holds 64 values
    static_assert(WM * WN == 4, "4 waves per workgroup");
    static_assert(!DIFF || (L2 && !SYM && !BF16 && WN == 1 && TN == 1), "the difference build: one 32-query tile, squared L2");
    constexpr bool M16 = Q16 > 0;
    static_assert(!M16 || (NTDB && !SYM && !BF16 && DNQ == 0 && TN == 1), "16-query blocks: plain fp32, one query tile per launch");
    constexpr int DT = WM * TM * 32;        // database rows per tile
    constexpr int QT = WN * (M16 ? Q16 * 16 : TN * 32); // queries per workgroup
    constexpr int NB = M16 ? Q16 : TN;      // query blocks of a wave (of 16 / 32 queries)
    constexpr int NS = TM * (M16 ? 8 : 16); // scores of one query block a lane holds per tile
    constexpr bool BIGT = TM * TN >= 16;    // the 256 x 256 tile: one workgroup per CU, accumulators in AGPRs, late-barrier K loop
    // the batch builds (several query tiles per launch, plain fp32): the 128 x 128 and the 256 x 256 tile filter their scores
    // through the sparse epilogue
    constexpr bool SPARSE = !NTDB && !BF16 && DNQ == 0 && Q16 == 0 && WM == 2 && WN == 2 && TM == TN && (TM == 2 || TM == 4);
    constexpr int ROWS = DT + QT;           // staged rows per K step
    // (X12: a K step of a tile is 16 KB of high bytes + 8 KB of low nibbles, already in LDS order, + 4 KB of fp16 queries)
    constexpr int X12_DB = 24;              // X12: staging instructions of a K step that fetch rows (1 KB each)
    constexpr int NGRP = X12 ? X12_DB + QT / 8 : ROWS / 8; // staging instructions per K step (8 rows each) ...
    constexpr int NI = (NGRP + 3) / 4;      // ... per wave; a wave short of one (304 rows: 38 over 4 waves) repeats its previous one
    static_assert(ROWS % 8 == 0, "staging split");
    static_assert(!X12 || NGRP % 4 == 0, "X12: every wave issues whole rounds, the last of them the queries'");
    constexpr int NDBI = X12 ? X12_DB / 4 : DT / 32; // a wave's first NDBI staging instructions fetch rows, the rest queries
    constexpr int KOFF_DB = X12 ? X12_DB * 256 : 32; // floats from one K step of a lane's row source to the next
    constexpr int B_OFF = X12 ? X12_DB * 1024 : DT * 128; // the staged queries behind the staged rows
    constexpr int STAGE_BYTES = ROWS * 128; // 32 floats per row
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *stage0 = smem;
    char *stage1 = smem + STAGE_BYTES;
    // (the symmetric 128 x 128 build's sparse epilogue keeps 36 slots of 2 KB: 8 KB more than the two staging buffers)
    const int lds_main = max(max(2 * STAGE_BYTES, p.cap * 8), SYM && TM * TN == 4 ? 73728 : 0);

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6); // (scalar: the LDS targets of the staging instructions are then SGPR arithmetic, no v_readfirstlane per instruction)
    const int wm = wave / WN, wn = wave % WN;
    const int li = lane & 31, lh = lane >> 5;
    const int lq = M16 ? (lane & 15) : li, lg = M16 ? (lane >> 4) : lh; // this lane's query of a block / its row group (accumulator layout)

    int qtile, chunk;
    int64_t c_lo, c_hi;
    if constexpr (SYM) {
        static_assert(DT == QT, "square tiles");
        const SymItem it = p.sym_items[blockIdx.x];
        qtile = it.qtile;
        chunk = 0;
        c_lo = (int64_t)it.jt0 * DT;
        c_hi = min(p.nb, c_lo + (int64_t)it.jcount * DT);
    } else {
        qtile = blockIdx.x % p.nqtiles;
        chunk = blockIdx.x / p.nqtiles;
        if (NTDB && p.pair_ctr) chunk = blockIdx.x % p.npairs; // (one query tile: blockIdx.x is the workgroup of the pair)
        c_lo = ((int64_t)chunk * p.tiles_base + min(chunk, p.tiles_rem)) * DT;
        c_hi = min(p.nb, c_lo + (int64_t)(p.tiles_base + (chunk < p.tiles_rem ? 1 : 0)) * DT);
    }
    // Paired walk (NTDB launches = one query tile = the HBM-bound streaming regime).  Two workgroups per CU is what the
    // LDS holds, and the two residents of a CU do not progress alike: the older one wins the arbitration and finished its
    // 10 tiles of a 1.25 M-row shard one tile time before the younger one, which then ran its last tile alone (per-
    // workgroup stamps: every CU's later workgroup ended at 1000 us, its earlier one at 907; 23 CUs had one workgroup and
    // idled from 600 us on).  So a launch has exactly 2 x CUs workgroups, workgroups w and w + npairs (dispatched one
    // round apart: an older and a younger resident) share ONE range of tiles, w takes tiles from the front, w + npairs
    // from the back, and each tile is claimed with a ticket from the pair's counter: both stay busy until the range is
    // used up, whatever their speeds.  Each side still walks contiguous rows (translations and DRAM pages stay warm --
    // pulling single tiles from one global counter cost 2.5-10 %).  The ticket of the NEXT tile is drawn at the start of
    // the current one: its latency hides behind the K loop.
    const bool paired = NTDB && !SYM && p.pair_ctr != nullptr;
    const int side = paired ? (int)(blockIdx.x / p.npairs) : 0;
    const int ntl = (int)((c_hi - c_lo + DT - 1) / DT); // tiles of this chunk / of the pair's range
    // The pool: pairs do not progress alike either (per-XCD means of the workgroups' lives differed by 4 %, the slowest CU
    // ended 6 % after the median one): the last pool_tiles tiles of every pair's range are nobody's -- a workgroup whose
    // pair has used up its own tiles draws them, any pair's, from one global counter until they are gone.
    const int n_own = paired ? ntl - p.pool_tiles : ntl;
    const int tile_first = (int)(c_lo / DT);
    int *s_next = nullptr;
    const int64_t q0 = (int64_t)qtile * QT;
    const int KT = p.dp / 32;
    ListCtx L;
    L.s_thr = (float *)(smem + lds_main);
    L.s_cnt = (int *)(L.s_thr + QT);
    L.s_need = L.s_cnt + QT;
    s_next = L.s_need + 1;                 // the ticket drawn for this workgroup's next tile (paired walk)
    int *s_base = L.s_need + 4;            // [QT] first slot of each query's survivors in its compact array
    float *s_yn = (float *)(s_base + QT);  // [DT] squared norms of the current tile's rows (L2 only)
    float *s_thr2 = s_yn + DT;             // SYM: [DT] thresholds of the tile's rows taken as queries
    int *s_cnt2 = (int *)(s_thr2 + DT);    // SYM: [WN][DT] survivors per row found by the waves of each query half
    int *s_base2 = s_cnt2 + WN * DT;       // SYM: [DT] first slot reserved in each row's compact array
    L.lists = p.lists + (size_t)blockIdx.x * QT * p.cap;
    L.gthr = p.gthr + (size_t)qtile * QT;
    L.cap = p.cap;
    L.k = p.k;
    L.kslot = p.kslot;
    L.init(tid, QT);
    // Tile-minimum seed (plain fp32 launches of the streaming regime; the host turns it on when the launch has a few
    // times k chunks).  No sample pass in front of the launch: every workgroup filters its first tile against nothing,
    // publishes each query's BEST key of that tile, and the k-th smallest of all keys published so far -- keys of k
    // different rows -- is an upper bound of the global k-th: one wave of the publishing workgroup works it out for one
    // query (wave_select over <= 2048 published keys) and lowers the shared threshold.  With c chunks of DT-row tiles
    // the bound sits near the k / (c DT) quantile (1.25 M rows, k = 100: ~1100 candidates per query for the whole
    // launch; the sample pass it replaces cost 90 us in front of a 0.85 ms scan and admitted 12 k).  A publication that
    // a reader does not see yet reads as KEY_PAD: the bound is then looser, never wrong.
    constexpr bool CAN_PUB = !SYM && !BF16 && QT <= 64;
    uint64_t *s_pub = (uint64_t *)s_thr2; // [QT] (a plain launch has no s_thr2)
    const bool pub_on = CAN_PUB && p.pub != nullptr;
    L.prefilter = pub_on;
    if (pub_on && tid < QT) s_pub[tid] = KEY_PAD;
    __syncthreads();
    // per-lane staging bookkeeping: instruction ii covers combined rows 8*ii..8*ii+7
    const float *srcp[NI];
    int lds_off[NI];
    bool is_db[NI];
    int rloc[NI];
#pragma unroll
    for (int n = 0; n < NI; n++) {
        int ii = wave + 4 * n;
        if (ii >= NGRP) ii -= 4; // (the same rows once more, to the same place: harmless)
        int row_local = X12 ? (ii < X12_DB ? 0 : DT + 8 * (ii - X12_DB) + (lane >> 3)) : 8 * ii + (lane >> 3);
        int sp = lane & 7;
        lds_off[n] = ii * 1024;
        if (X12 && ii < X12_DB) { // 1 KB of the tile's K step as it lies in memory: lane l's 16 bytes go to LDS bytes 16 l ..
            is_db[n] = true;
            rloc[n] = 0;
            srcp[n] = p.xb + ii * 256 + lane * 4; // tile and K step added per tile
        } else if (row_local < DT) {
            is_db[n] = true;
            rloc[n] = row_local;
            int s = sp ^ ((row_local >> 1) & 7);
            srcp[n] = p.xb + 4 * s; // row added per tile
        } else {
            is_db[n] = false;
            int rq = row_local - DT;
            rloc[n] = rq;
            int s = sp ^ ((rq >> 1) & 7);
            if constexpr (DNQ > 0) { // the difference build stages the queries interleaved by pairs: DNQ rows of diff_interleave_kernel's matrix
                srcp[n] = p.xq_diff + (int64_t)min(rq, DNQ - 1) * p.dp + 4 * s;
            } else {
                int64_t q = min(q0 + rq, p.nq - 1);
                srcp[n] = p.xq + q * p.dp + 4 * s;
            }
        }
    }
    const int swz = (li >> 1) & 7;

    uint32_t *my_turn = nullptr;
    if constexpr (!NTDB && !BF16) {
        if (p.cu_turn) { // this CU's word: XCC_ID (hwreg 20) and HW_ID (hwreg 4: cu_id [11:8], sh_id [12], se_id [15:13])
            const uint32_t hw = (uint32_t)__builtin_amdgcn_s_getreg(0xF804), xcc = (uint32_t)__builtin_amdgcn_s_getreg(0xF814) & 7u;
            my_turn = p.cu_turn + ((xcc << 8) | (((hw >> 13) & 7u) << 5) | (((hw >> 12) & 1u) << 4) | ((hw >> 8) & 15u));
        }
    }
    // (256 x 256 builds) what the sparse epilogue needs per query block and never changes: the queries' norms, and which lanes'
    // queries may be candidates of the symmetric launch's second direction (real rows the sample pass has not handed on)
    float big_xnq[NB];
    uint64_t big_cokm[NB];
    if constexpr (SPARSE) {
#pragma unroll
        for (int b = 0; b < NB; b++) {
            const int64_t q = q0 + (M16 ? 0 : (wn * TN + b) * 32 + li);
            const bool qok = q < p.nq;
            big_xnq[b] = 0.0f;
            if constexpr (L2) big_xnq[b] = p.xn[qok ? q : 0];
            big_cokm[b] = __ballot(qok && !(p.skip_mask >= 0 && ((int)(q >> p.vshift) & p.skip_mask) == 0));
        }
    }
    int f16_qe[NB]; // (F16X) the exponent of this lane's query of each query block
#pragma unroll
    for (int b = 0; b < NB; b++) f16_qe[b] = F16X ? p.qexp[min(q0 + (wn * TN + b) * 32 + li, p.nq - 1)] : 0;
    int tile_idx = 0; // tiles this workgroup has walked
    // the tile being walked / the one after it, as tile numbers of the view (-1: none)
    int cur_tile = paired ? (side == 0 ? tile_first : tile_first + n_own - 1) : tile_first;
    if (paired ? side >= n_own : ntl <= 0) cur_tile = -1;
    int own_walked = 0;     // (thread 0) tiles drawn from the pair's own range, the first one included
    bool in_pool = false;   // (thread 0) the pair's own tiles are gone
    KNN_TRACE(0);
#ifdef KNN355_TRACE
    if (threadIdx.x == 0 && p.trace) // where this workgroup runs: HW_ID (hwreg 4) and XCC_ID (hwreg 20)
        p.trace[(size_t)blockIdx.x * 128 + 62] = ((unsigned long long)__builtin_amdgcn_s_getreg(0xF814) << 32) | (unsigned)__builtin_amdgcn_s_getreg(0xF804);
#endif
    int64_t first_row0 = c_lo;
    const float *tsrc[NI]; // this lane's source of each of its staging instructions for the tile being walked (first K step)
    bool staged0 = false;  // (256 x 256 builds) K step 0 of the tile about to start is already on its way into buffer 0
    while (cur_tile >= 0) {
        const int64_t row0 = (int64_t)cur_tile * DT;
        if (tile_idx == 0) first_row0 = row0;
        int next_tile = cur_tile + 1 < tile_first + ntl ? cur_tile + 1 : -1; // (unpaired: the chunk in order)
        if (paired && tid == 0) {
            next_tile = -1;
            if (!in_pool) {
                own_walked++;
                const int t = (int)__hip_atomic_fetch_add(&p.pair_ctr[chunk], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (t < n_own) next_tile = side == 0 ? tile_first + own_walked : tile_first + n_own - 1 - own_walked;
                else in_pool = true;
            }
            if (in_pool && p.pool_tiles > 0) {
                const int g = (int)__hip_atomic_fetch_add(&p.pair_ctr[p.npairs], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (g < p.npairs * p.pool_tiles) {
                    // pool tile g: the (g / npairs)-th reserved tile of pair g % npairs
                    const int pj = g % p.npairs, pi = g / p.npairs;
                    next_tile = pj * p.tiles_base + min(pj, p.tiles_rem) + (p.tiles_base + (pj < p.tiles_rem ? 1 : 0)) - p.pool_tiles + pi;
                }
            }
        }
        f32x16 acc[M16 ? 1 : TM][M16 ? 1 : TN];
        f32x4 acc16[M16 ? 2 * TM : 1][M16 ? Q16 : 1]; // 16-query blocks: [row tile of 16][query block], lane (q = lane & 15, g = lane / 16): rows 4 g + r
#pragma unroll
        for (int a = 0; a < (M16 ? 1 : TM); a++)
#pragma unroll
            for (int b = 0; b < (M16 ? 1 : TN); b++)
#pragma unroll
                for (int r = 0; r < 16; r++) acc[a][b][r] = 0.0f;
#pragma unroll
        for (int a = 0; a < (M16 ? 2 * TM : 1); a++)
#pragma unroll
            for (int b = 0; b < (M16 ? Q16 : 1); b++) acc16[a][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // score s (0 .. NS) of query block b in this lane: its accumulator register, and its row inside the tile
        auto accv = [&](int b, int s) -> float {
            if constexpr (M16) return acc16[s >> 2][b][s & 3];
            else return acc[s >> 4][b][s & 15];
        };
        auto rowl = [&](int s) -> int {
            if constexpr (M16) return (wm * TM * 2 + (s >> 2)) * 16 + 4 * lg + (s & 3);
            else return (wm * TM + (s >> 4)) * 32 + 4 * lh + (s & 3) + 8 * ((s & 15) >> 2);
        };
        auto qloc = [&](int b) -> int { return M16 ? (wn * Q16 + b) * 16 + lq : (wn * TN + b) * 32 + li; };
        constexpr int DIFF_NQ = DIFF ? DNQ : 1; // (the difference build serves batches of fewer than 20 queries: one chain per query)
        f32x2 dacc2[(DIFF_NQ + 1) / 2];        // ... as one chain per query and row; a thread holds two rows x half the query pairs: [row][pair] (see compute)
#pragma unroll
        for (int qi = 0; qi < (DIFF_NQ + 1) / 2; qi++) dacc2[qi] = f32x2{0.0f, 0.0f};

        if (!staged0) { // (256 x 256 builds: the previous tile's epilogue has worked these out already -- and staged the first K step)
#pragma unroll
            for (int n = 0; n < NI; n++) {
                if (X12 && is_db[n]) { // (tiles past the end of a view are whole in memory: rows that are not there are dropped behind the K loop)
                    tsrc[n] = srcp[n] + (int64_t)cur_tile * KT * KOFF_DB;
                } else if (is_db[n]) {
                    int64_t r = view_row(min(row0 + rloc[n], p.nb - 1), p.row_mul, p.vshift);
                    tsrc[n] = srcp[n] + r * p.dp;
                } else {
                    tsrc[n] = srcp[n];
                }
            }
        }
        if constexpr (L2) {
            // the tile's squared norms: one coalesced load per thread now, LDS reads in the epilogue
            // (visible after the K loop's barriers) instead of 16 * TM * TN scattered global loads
            // per lane at the end of the tile
            if (tid < DT) s_yn[tid] = p.yn[view_row(min(row0 + tid, p.nb - 1), p.row_mul, p.vshift)];
        }
        if constexpr (F16X) { // the rows' exponents, in the slot of the norms (inner product: unused)
            if (tid < DT) ((int *)s_yn)[tid] = (int)p.xexp[view_row(min(row0 + tid, p.nb - 1), p.row_mul, p.vshift)];
        }
        const bool off_diag = SYM && row0 != q0; // (square tiles: the diagonal tile starts at the query tile's first row)
        // (256 x 256 builds) the queries' thresholds as they stand NOW: an agent-scope load is a round trip to memory, four of
        // them one after the other were 8 of the epilogue's 10 us; read in front of the K loop they cost nothing, and a bound
        // one tile old only admits a few candidates more (thresholds only ever tighten)
        float big_thr[NB];
        if constexpr (SPARSE) {
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const int ql = M16 ? 0 : (wn * TN + b) * 32 + li;
                big_thr[b] = q0 + ql < p.nq ? L.threshold(ql) : -INFINITY; // (a query past the end admits nothing)
            }
        }
        if constexpr (SYM) {
            if (tid < DT) // rows past the end are nobody's query: nothing beats -inf
                s_thr2[tid] = row0 + tid < p.nb ? ord2f(__hip_atomic_load(&p.gthr[row0 + tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) : -INFINITY;
            if constexpr (SPARSE) { // (the sparse epilogue's per-row counters and its "this tile is dense" flag; visible behind the K loop's barriers)
                if (tid < DT) s_cnt2[tid] = 0;
                if (tid == 0) L.s_need[2] = 0;
            }
        }
        // One K step of MFMA work from buffer `cur`.  `dma(n)` (n < NI) issues this wave's n-th
        // staging instruction of the NEXT K step; the NI of them are spread between the MFMAs so
        // that their issue cost (60-180 cycles each) is paid while the matrix pipe is busy, not
        // in front of it.  ND = 0: nothing to stage.
        int diff_koff = 0; // (difference builds) first float of the K step being multiplied
        auto compute = [&](const char *cur, auto &&dma, auto nd_tag) {
            constexpr int ND = decltype(nd_tag)::value;
            const char *A = cur;
            const char *B = cur + B_OFF;
            if constexpr (DIFF) {
#pragma unroll
                for (int n = 0; n < ND; n++) dma(n); // (the next K step's staging goes out first: the chains below take microseconds)
                // thread = TWO rows (r0, r0 + 128) and half of the query PAIRS; the two halves of a packed fp32 instruction are
                // the two queries of a pair: (qa[k] - y[k], qb[k] - y[k]), squared and added into the pair's two chains
                // (v_pk_add_f32 / v_pk_fma_f32).  The queries are staged INTERLEAVED by pairs (diff_interleave_kernel: staged
                // row 2p holds qa[k], qb[k] for k = 0..15 of the K step, row 2p + 1 for k = 16..31), so one ds_read_b128 (a
                // broadcast: every lane reads the same address) delivers two k of both queries as two aligned register pairs,
                // and the row's own floats come as plain ds_read_b128 fragments (consecutive lanes = consecutive rows: no bank
                // conflict), broadcast into both halves by op_sel.  Round 3 packed two ROWS per instruction instead: their
                // floats needed 32 ds_read2_b32 per K step that hit 8 of the 32 banks (4-way conflicts), every wave re-read
                // every query float, and the K step was bound by the LDS (12.2 ms per 10 M rows x 19 queries).
                //   Chains: 2 rows x NPH pairs per thread, all independent, interleaved instruction by instruction; the query
                // fragments of the half-block after next are requested while this one is computed.  Every chain visits
                // k = 8t + m, 8t + 4 + m (m = 0..3, t = 0..3): the dot product's order.
                constexpr int NPH = DIFF_NQ / 4;
                const int r0 = (wave & 1) * 64 + lane, qh = wave >> 1;
                const int fy = (lane >> 1) & 7; // (r0 >> 1) & 7 -- the same for r0 + 128
                f32x4 y0[8], y1[8];
#pragma unroll
                for (int sl = 0; sl < 8; sl++) {
                    y0[sl] = *(const f32x4 *)(A + r0 * 128 + ((sl ^ fy) * 16));
                    y1[sl] = *(const f32x4 *)(A + (r0 + 128) * 128 + ((sl ^ fy) * 16));
                }
                f32x4 qv[2][NPH][2];
                // half-block hb (8 per K step): block t = hb / 2 (8 k), its half u = hb % 2: k = 8t + 2u, 8t + 4 + 2u, 8t + 2u + 1,
                // 8t + 4 + 2u + 1 -- 16-byte slots 4 (t & 1) + u and 4 (t & 1) + 2 + u of staged row 2p + t / 2
                auto loadq = [&](int hb) {
                    const int t = hb >> 1, u = hb & 1;
                    // the first SQ query pairs of this thread's half come by SCALAR loads from the interleaved query matrix (the
                    // address is the same for every lane; constant address space + an address made of scalars only: s_load_dwordx4
                    // -- through a flat pointer the compiler takes vector loads and spills): they never touch the LDS pipe, which the
                    // broadcast reads of the wider builds had saturated.  Three pairs at most: with every pair in scalar registers
                    // the 16- / 20-query builds spill THOSE (9.7 / 12.5 ms per 10 M rows against 8.9 / 10.4 through the LDS)
                    // (not in the 8-query build: it runs at the HBM rate either way, and with the lighter LDS load the chip settled on a
                    // lower clock -- 6.60 against 6.31 ms per 10 M rows in steady state, three alternating runs on one box)
                    constexpr int SQ = KNN355_DIFF_SCALAR_Q && NPH >= 3 ? (NPH < KNN355_DIFF_SCALAR_PAIRS ? NPH : KNN355_DIFF_SCALAR_PAIRS) : 0;
                    typedef const __attribute__((address_space(4))) f32x4 *cq4;
#pragma unroll
                    for (int j = 0; j < SQ; j++) {
                        const int pr = qh * NPH + j;
                        const float *qg = p.xq_diff + (int64_t)(2 * pr + (t >> 1)) * p.dp + diff_koff + 4 * (4 * (t & 1) + u);
                        qv[hb & 1][j][0] = *(cq4)qg;
                        qv[hb & 1][j][1] = *(cq4)(qg + 8);
                    }
#pragma unroll
                    for (int j = SQ; j < NPH; j++) {
                        const int pr = qh * NPH + j;
                        const char *qrow = B + (2 * pr + (t >> 1)) * 128;
                        const int fq = pr & 7; // ((2 pr) >> 1) & 7 -- the same for 2 pr + 1
                        qv[hb & 1][j][0] = *(const f32x4 *)(qrow + (((4 * (t & 1) + u) ^ fq) * 16));
                        qv[hb & 1][j][1] = *(const f32x4 *)(qrow + (((4 * (t & 1) + 2 + u) ^ fq) * 16));
                    }
                };
                auto chains = [&](int hb) {
                    const int t = hb >> 1, u = hb & 1;
#pragma unroll
                    for (int e = 0; e < 2; e++) {       // first / second k of the slots
#pragma unroll
                        for (int ab = 0; ab < 2; ab++) { // slot 4 (t & 1) + u (k = 8t + ..), then slot .. + 2 (k = 8t + 4 + ..)
                            const float ya = y0[2 * t + ab][2 * u + e], yb = y1[2 * t + ab][2 * u + e];
#pragma unroll
                            for (int j = 0; j < NPH; j++) {
                                const f32x4 v = qv[hb & 1][j][ab];
                                const f32x2 qp = e == 0 ? f32x2{v[0], v[1]} : f32x2{v[2], v[3]};
                                const f32x2 ta = qp - f32x2{ya, ya};
                                dacc2[j] = __builtin_elementwise_fma(ta, ta, dacc2[j]);
                                const f32x2 tb = qp - f32x2{yb, yb};
                                dacc2[NPH + j] = __builtin_elementwise_fma(tb, tb, dacc2[NPH + j]);
                            }
                        }
                    }
                };
                loadq(0);
                loadq(1);
#pragma unroll
                for (int hb = 0; hb < 8; hb++) {
                    chains(hb);
                    if (hb + 2 < 8) loadq(hb + 2);
                    __builtin_amdgcn_sched_barrier(0);
                }
                return;
            }
            if constexpr (M16) {
                // 16 x 16 x 4 tiles: a wave's 64 rows are RT = 2 TM row tiles, its queries Q16 blocks.  Lane (i = lane & 15,
                // g = lane / 16) feeds k = g of every instruction, and the chain must visit k = 0,4,1,5 | 2,6,3,7 of each
                // block of 8: the lane reads the 16-byte slot 2t + (g & 1) of its row (floats 8t + 4 (g & 1) ..) and hands
                // element g / 2 to the block's first instruction, element g / 2 + 2 to its second.
                constexpr int RT = 2 * TM;
                const int g = lane >> 4, swz16 = ((lane & 15) >> 1) & 7;
                const bool upper = (g >> 1) != 0;
                f32x4 af16[2][RT], bf16[2][Q16];
                auto frag16 = [&](int t) {
                    const int slot = ((2 * t + (g & 1)) ^ swz16) * 16;
#pragma unroll
                    for (int a = 0; a < RT; a++)
                        af16[t & 1][a] = *(const f32x4 *)(A + ((wm * RT + a) * 16 + (lane & 15)) * 128 + slot);
#pragma unroll
                    for (int b = 0; b < Q16; b++)
                        bf16[t & 1][b] = *(const f32x4 *)(B + ((wn * Q16 + b) * 16 + (lane & 15)) * 128 + slot);
                };
                constexpr int M = 2 * RT * Q16; // MFMAs per sub-step
                frag16(0);
                __builtin_amdgcn_sched_group_barrier(0x100, RT + Q16, 0);
                auto substep16 = [&](auto t_tag) {
                    constexpr int t = decltype(t_tag)::value;
                    if constexpr (t < 3) frag16(t + 1);
#pragma unroll
                    for (int half = 0; half < 2; half++) {
                        float av[RT], bv[Q16];
                        // (one v_cndmask per operand.  The empty asm keeps the two candidates opaque: left alone, the compiler
                        // folds a fragment's two selects into ONE extraction with a four-way dynamic index and spends three
                        // v_cndmask on each)
                        auto pick = [&](const f32x4 &v) -> float {
                            float lo = v[2 * half], hi = v[2 * half + 1];
                            asm("" : "+v"(lo), "+v"(hi));
                            return upper ? hi : lo;
                        };
#pragma unroll
                        for (int a = 0; a < RT; a++) av[a] = pick(af16[t & 1][a]);
#pragma unroll
                        for (int b = 0; b < Q16; b++) bv[b] = pick(bf16[t & 1][b]);
#pragma unroll
                        for (int a = 0; a < RT; a++)
#pragma unroll
                            for (int b = 0; b < Q16; b++)
                                acc16[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[a], bv[b], acc16[a][b], 0, 0, 0);
                    }
                    constexpr int TD = 2;
                    constexpr int n0 = t < TD ? ND * t / TD : ND, n1 = t < TD ? ND * (t + 1) / TD : ND; // (spread over the first half: see the 32 x 32 x 2 path)
#pragma unroll
                    for (int n = n0; n < n1; n++) dma(n);
                    if constexpr (t < 3) __builtin_amdgcn_sched_group_barrier(0x100, RT + Q16, 0);
                    constexpr int nd = n1 - n0, per = M / (nd + 1);
                    static_assert(per >= 1, "more staging instructions than MFMAs in a sub-step");
                    sched_spread<nd, per>();
                    __builtin_amdgcn_sched_group_barrier(0x008, M - nd * per, 0);
                };
                substep16(std::integral_constant<int, 0>{});
                substep16(std::integral_constant<int, 1>{});
                substep16(std::integral_constant<int, 2>{});
                substep16(std::integral_constant<int, 3>{});
                return;
            }
            if constexpr (X12) {
                // 12-bit row copies: n = 16 (hb - 128) + lo, |n| <= 2047, as a byte hb and a nibble lo per value.  A
                // K step of a row tile lies in memory as it lies here: [row tile of 32][half][lane][16 B] high bytes, then
                // [row tile of 32][lane][16 B] nibbles -- lane (li, lh) finds the 32 + 16 bytes of its row's values
                // k = 16 t + 8 lh + j (t = 0..3: the four MFMAs of the K step, j = 0..7) with three ds_read_b128, consecutive
                // lanes 16 bytes apart.  High bytes: byte 8 (t & 1) + j of half t / 2; nibbles: byte 4 t + (j & 3), low nibble
                // j < 4.  The fp16 fragment is rebuilt exactly: 0x6400 | b is 1024 + b, so with A = 1024 + hb and L = 1024 + lo
                // fma(A - 1216, 16, L) = 16 (hb - 192) + 1024 + lo = n -- the difference is exact (|hb - 192| <= 192), the fma
                // rounds once and n is an fp16 number.  Per 8 values: 3 mask / shift, 8 byte permutes, 4 packed subtracts, 4 packed fma.
                typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
                u32x4 hi[TM][2], lo[TM];
                f32x4 bq[4][TN];
#pragma unroll
                for (int a = 0; a < TM; a++) {
                    hi[a][0] = *(const u32x4 *)(A + ((wm * TM + a) * 2 + 0) * 1024 + lane * 16);
                    hi[a][1] = *(const u32x4 *)(A + ((wm * TM + a) * 2 + 1) * 1024 + lane * 16);
                    lo[a] = *(const u32x4 *)(A + DT * 64 + (wm * TM + a) * 1024 + lane * 16);
                }
#pragma unroll
                for (int t = 0; t < 4; t++)
#pragma unroll
                    for (int b = 0; b < TN; b++) bq[t][b] = *(const f32x4 *)(B + ((wn * TN + b) * 32 + li) * 128 + (((2 * t + lh) ^ swz) * 16));
#pragma unroll
                for (int n = 0; n < ND; n++) dma(n); // (the next K step's staging first: the longest lead the double buffer allows)
                const f16x2 bias = {(_Float16)1216.0f, (_Float16)1216.0f}, sixteen = {(_Float16)16.0f, (_Float16)16.0f};
                auto pair = [&](uint32_t hw, uint32_t lw, uint32_t sel) -> uint32_t {
                    const f16x2 ah = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, hw, sel)) - bias;
                    const f16x2 al = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, lw, sel));
                    return __builtin_bit_cast(uint32_t, __builtin_elementwise_fma(ah, sixteen, al));
                };
#pragma unroll
                for (int t = 0; t < 4; t++) {
#pragma unroll
                    for (int a = 0; a < TM; a++) {
                        const uint32_t h0 = hi[a][t >> 1][2 * (t & 1)], h1 = hi[a][t >> 1][2 * (t & 1) + 1];
                        const uint32_t l0 = lo[a][t] & 0x0F0F0F0Fu, l1 = (lo[a][t] >> 4) & 0x0F0F0F0Fu;
                        // (selector bytes 0..3: the data word's bytes, 4: the constant's 0x64)
                        const u32x4 fr = {pair(h0, l0, 0x04010400u), pair(h0, l0, 0x04030402u), pair(h1, l1, 0x04010400u), pair(h1, l1, 0x04030402u)};
#pragma unroll
                        for (int b = 0; b < TN; b++)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, fr), __builtin_bit_cast(f16x8, bq[t][b]), acc[a][b], 0, 0, 0);
                    }
                }
                return;
            }
            // fragments of sub-step t+1 are requested before the MFMAs of sub-step t are issued,
            // so the LDS latency hides behind the matrix pipe (two register sets, fully unrolled)
            f32x4 af[2][TM], bf[2][TN];
            auto frag = [&](int t) {
                const int slot = ((2 * t + lh) ^ swz) * 16;
#pragma unroll
                for (int a = 0; a < TM; a++)
                    af[t & 1][a] = *(const f32x4 *)(A + ((wm * TM + a) * 32 + li) * 128 + slot);
#pragma unroll
                for (int b = 0; b < TN; b++)
                    bf[t & 1][b] = *(const f32x4 *)(B + ((wn * TN + b) * 32 + li) * 128 + slot);
            };
            constexpr int M = H16 ? TM * TN : 4 * TM * TN; // MFMAs per sub-step
            frag(0);
            if constexpr (!H16) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
            auto substep = [&](auto t_tag) {
                constexpr int t = decltype(t_tag)::value;
                if constexpr (t < 3) frag(t + 1);
                if constexpr (F16X) {
#pragma unroll
                    for (int a = 0; a < TM; a++)
#pragma unroll
                        for (int b = 0; b < TN; b++)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, af[t & 1][a]),
                                                                               __builtin_bit_cast(f16x8, bf[t & 1][b]), acc[a][b], 0, 0, 0);
                } else if constexpr (BF16) {
#pragma unroll
                    for (int a = 0; a < TM; a++)
#pragma unroll
                        for (int b = 0; b < TN; b++)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[t & 1][a]),
                                                                                __builtin_bit_cast(bf16x8, bf[t & 1][b]), acc[a][b], 0, 0, 0);
                } else {
#pragma unroll
                    for (int m = 0; m < 4; m++)
#pragma unroll
                        for (int a = 0; a < TM; a++)
#pragma unroll
                            for (int b = 0; b < TN; b++)
                                acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[t & 1][a][m], bf[t & 1][b][m], acc[a][b], 0, 0, 0);
                }
                // staging instructions [n0, n1) of the next K step belong to this sub-step; all of
                // them go out in the first TD sub-steps of the K step so that the rest covers
                // their latency before the next barrier's vmcnt(0)
                constexpr int TD = NTDB ? 2 : 3; // (batch launches hit L2: spread wide, +1 %)
                // Streaming launches (one query tile, rows straight from HBM): EVERY staging instruction of the next K step goes
                // out in front of this K step's first MFMA -- the longest lead the double buffer allows.  (Rounds 2-3 spread them
                // over the first half of the K step so that their issue cost hid behind MFMAs: 1.2-3 % slower once the epilogue and
                // the walk were what they are now -- 10 M x 32 queries 7.39 -> 7.30 ms, 1.25 M rows 0.972 -> 0.945 ms, same box.)
                // (the 32- and 64-query builds only: the 128-query one-tile launch is bound by the matrix pipe and lost 2 % with it,
                // the builds on 16-query blocks 0.5 %)
                constexpr bool FIRST = NTDB && QT <= 64 && KNN355_STREAM_DMA_FIRST;
                if constexpr (FIRST && t == 0) {
#pragma unroll
                    for (int n = 0; n < ND; n++) dma(n);
                    __builtin_amdgcn_sched_group_barrier(0x010, ND, 0);
                }
                constexpr int n0 = FIRST ? ND : (t < TD ? ND * t / TD : ND), n1 = FIRST ? ND : (t < TD ? ND * (t + 1) / TD : ND);
#pragma unroll
                for (int n = n0; n < n1; n++) dma(n);
                // pin the order: LDS reads of t+1, then the MFMAs of t with the staging
                // instructions spread between them (left alone, the scheduler sinks the reads
                // behind the MFMAs to save registers and the wait is exposed)
                if constexpr (!H16) { // (the 16-bit builds are bound by staging, not by the matrix pipe: the compiler's order will do)
                    if constexpr (t < 3) __builtin_amdgcn_sched_group_barrier(0x100, TM + TN, 0);
                    constexpr int nd = n1 - n0, per = M / (nd + 1);
                    static_assert(per >= 1, "more staging instructions than MFMAs in a sub-step");
                    sched_spread<nd, per>();
                    __builtin_amdgcn_sched_group_barrier(0x008, M - nd * per, 0);
                }
            };
            substep(std::integral_constant<int, 0>{});
            substep(std::integral_constant<int, 1>{});
            substep(std::integral_constant<int, 2>{});
            substep(std::integral_constant<int, 3>{});
        };
        auto no_dma = [](int) {};
        using nd_none = std::integral_constant<int, 0>;
        using nd_all = std::integral_constant<int, NI>;
        if constexpr (BIGT) {
            // ---- the 256 x 256 tile's K loop: ONE wave per SIMD, so nothing but this wave's own instruction order hides a
            // latency.  One barrier per K step, in front of the step's LAST sub-step ("late barrier"):
            //   sub-step 0, 1   MFMAs; the staging instructions of K step kt + 1 (groups A, B) between them
            //   sub-step 2      MFMAs only -- the staged bytes have a whole sub-step (4096 matrix cycles) to land --, then
            //                   vmcnt(0) + barrier: stage kt + 1 is in LDS for everyone, and everyone has read stage kt for the
            //                   last time (the fragments of sub-step 3 were requested at the start of sub-step 2)
            //   sub-step 3      MFMAs from registers; the FIRST fragments of K step kt + 1 are requested behind the first MFMA
            //                   (64 MFMAs cover their latency: the next K step starts without a wait), and group C of K step
            //                   kt + 2 is staged into the buffer stage kt has just left
            // Every sub-step issues one MFMA, then the fragment reads of the next sub-step: the compiler waits lgkmcnt(0) in front
            // of a sub-step's first MFMA, and with the reads behind that MFMA the wait only ever covers reads a sub-step old.
            constexpr int MS = 4 * TM * TN;                        // MFMAs per sub-step
            // staging instructions per group: half of K step kt + 1's in sub-step 3 of step kt - 1 (C), half in sub-step 0 of step kt
            // (A), none in sub-step 1 (B) -- two whole sub-steps (3.7 us) for the bytes to land before the wait in front of the
            // barrier.  (Thirds, the last of them with one sub-step of lead: fine while the rows come from L2 / the Infinity Cache
            // -- a Pfam-sized index -- and 5 % slower than the 128 x 128 tile on a 10 M-row index, whose rows come from HBM.)
            constexpr int NA = NI / 2, NBg = 0, NC = NI - NA - NBg;
#ifdef KNN355_TRACE
            // (developer build: K loop without its staging instructions / its barrier / its fragment reads -- wrong scores, right time)
            const bool stage_on = !(p.ablate & 16), barrier_on = !(p.ablate & 32), reads_on = !(p.ablate & 128);
#else
            constexpr bool stage_on = true, barrier_on = true, reads_on = true;
#endif
            f32x4 fa[2][TM], fb[2][TN];
            auto rd = [&](const char *buf, int t, int set) {
                if (!reads_on) return;
                const int slot = ((2 * t + lh) ^ swz) * 16;
#pragma unroll
                for (int a = 0; a < TM; a++) fa[set][a] = *(const f32x4 *)(buf + ((wm * TM + a) * 32 + li) * 128 + slot);
#pragma unroll
                for (int b = 0; b < TN; b++) fb[set][b] = *(const f32x4 *)(buf + DT * 128 + ((wn * TN + b) * 32 + li) * 128 + slot);
            };
            auto mfmas = [&](int set) {
#pragma unroll
                for (int m = 0; m < 4; m++)
#pragma unroll
                    for (int a = 0; a < TM; a++)
#pragma unroll
                        for (int b = 0; b < TN; b++)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[set][a][m], fb[set][b][m], acc[a][b], 0, 0, 0);
            };
            auto kstep = [&](int kt, auto h1_tag, auto h2_tag) {
                constexpr bool H1 = decltype(h1_tag)::value, H2 = decltype(h2_tag)::value; // K steps kt + 1 / kt + 2 exist
                char *cur = (kt & 1) ? stage1 : stage0;
                char *nxt = (kt & 1) ? stage0 : stage1;
                const int k1 = (kt + 1) * 32, k2 = (kt + 2) * 32;
                // sub-step 0 (set 0), fragments of sub-step 1 -> set 1, group A
                mfmas(0);
                rd(cur, 1, 1);
                if constexpr (H1) {
#pragma unroll
                    for (int n = 0; n < NA; n++) if (stage_on) stage_issue<false>(tsrc[n] + k1, nxt + lds_off[n]);
                }
                sched_reads<TM + TN>();
                sched_spread<(H1 ? NA : 0), (MS - (TM + TN)) / (NA + 1)>();
                __builtin_amdgcn_sched_group_barrier(0x008, MS - (TM + TN) - (H1 ? NA : 0) * ((MS - (TM + TN)) / (NA + 1)), 0);
                // sub-step 1 (set 1), fragments of sub-step 2 -> set 0, group B
                mfmas(1);
                rd(cur, 2, 0);
                if constexpr (H1) {
#pragma unroll
                    for (int n = NA; n < NA + NBg; n++) if (stage_on) stage_issue<false>(tsrc[n] + k1, nxt + lds_off[n]);
                }
                sched_reads<TM + TN>();
                sched_spread<(H1 ? NBg : 0), (MS - (TM + TN)) / (NBg + 1)>();
                __builtin_amdgcn_sched_group_barrier(0x008, MS - (TM + TN) - (H1 ? NBg : 0) * ((MS - (TM + TN)) / (NBg + 1)), 0);
                // sub-step 2 (set 0), fragments of sub-step 3 -> set 1, nothing staged; then the K step's one barrier
                mfmas(0);
                rd(cur, 3, 1);
                sched_reads<TM + TN>();
                __builtin_amdgcn_sched_group_barrier(0x008, MS - (TM + TN), 0);
                __builtin_amdgcn_sched_barrier(0); // (the wait and the barrier stay BEHIND this sub-step's MFMAs: they are the bytes' time to land)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // this wave's part of stage kt + 1 has landed (see the generic loop)
                if (barrier_on) __syncthreads();
                // sub-step 3 (set 1), first fragments of K step kt + 1 -> set 0, group C of K step kt + 2 into the buffer just left
                // (pinned by hand, one fragment read behind each of the first MFMAs and group C in NC pieces between the later ones:
                // a sched_group_barrier pipeline in the region behind the barrier came out as one burst of NC staging
                // instructions -- ISA checked)
                constexpr int PER = MS / (NC + 1);
                const int slot0 = (lh ^ swz) * 16; // (the first fragments of a K step: 16-byte slot 2 * 0 + lh)
#pragma unroll
                for (int i = 0; i < MS; i++) {
                    const int m = i / (TM * TN), a = (i / TN) % TM, b = i % TN;
                    acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[1][a][m], fb[1][b][m], acc[a][b], 0, 0, 0);
                    bool pinned = false;
                    if (H1 && i < TM + TN && reads_on) { // one fragment read behind each of the first MFMAs
                        if (i < TM) fa[0][i] = *(const f32x4 *)(nxt + ((wm * TM + i) * 32 + li) * 128 + slot0);
                        else fb[0][i - TM] = *(const f32x4 *)(nxt + DT * 128 + ((wn * TN + (i - TM)) * 32 + li) * 128 + slot0);
                        pinned = true;
                    }
                    if (H2 && (i + 1) % PER == 0 && (i + 1) / PER <= NC) {
                        const int n = NA + NBg + (i + 1) / PER - 1;
                        if (stage_on) stage_issue<false>(tsrc[n] + k2, cur + lds_off[n]);
                        pinned = true;
                    }
                    if (pinned) __builtin_amdgcn_sched_barrier(0);
                }
            };
            // prologue: stage K step 0, wait, barrier; group C of K step 1; the first fragments (the one exposed read of the tile)
            if (!staged0) {
#pragma unroll
                for (int n = 0; n < NI; n++) stage_issue<false>(tsrc[n], stage0 + lds_off[n]);
            }
            staged0 = false;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (KT > 1) {
#pragma unroll
                for (int n = NA + NBg; n < NI; n++) stage_issue<false>(tsrc[n] + 32, stage1 + lds_off[n]);
            }
            rd(stage0, 0, 0);
            using yes = std::true_type;
            using no = std::false_type;
            int kt = 0;
            for (; kt + 2 < KT; kt++) kstep(kt, yes{}, yes{});
            if (kt + 1 < KT) {
                kstep(kt, yes{}, no{});
                kt++;
            }
            kstep(kt, no{}, no{});
        } else {
            // prologue: stage K step 0 into buffer 0
#pragma unroll
            for (int n = 0; n < NI; n++) {
                if (NTDB && n < NDBI) stage_issue<true>(tsrc[n], stage0 + lds_off[n]); // rows, not queries
                else stage_issue<false>(tsrc[n], stage0 + lds_off[n]);
            }
            // Batch launches: the two workgroups of a CU take TURNS in their K loops.  Per-workgroup stamps showed a K loop
            // running alone (its neighbour in the epilogue) at 94-97 % of the matrix pipe's rate, and two K loops side by side
            // at 73-84 % together -- every wave's K-step barrier then also waits for the neighbour's waves on the other three
            // SIMDs.  One word per CU (found through HW_ID / XCC_ID), taken by thread 0 before the K loop and given back behind
            // it; the neighbour filters its previous tile meanwhile and waits out the rest.  (The word is cleared in front of
            // every launch; a workgroup alone on its CU never waits.)  Measured: +0.7 % on Pfam-sized launches, +1 % on CATH-sized
            // ones -- a K loop on its own reaches ~85 % of the pipe as well (one wave per SIMD: nothing fills its barrier bubbles).
            if constexpr (!NTDB && !BF16) {
                if (p.cu_turn) {
                    if (tid == 0) {
                        // (bounded: a turn that never comes -- it cannot, every holder gives the word back behind its K loop -- costs
                        // a few milliseconds, not the launch)
                        for (int it = 0; it < 8192; it++) {
                            if (__hip_atomic_exchange(my_turn, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) break;
                            __builtin_amdgcn_s_sleep(32);
                        }
                    }
                    // (no barrier of its own: the K loop's first barrier holds the other waves until thread 0 is through)
                }
            }
            for (int kt = 0; kt + 1 < KT; kt++) {
                char *cur = (kt & 1) ? stage1 : stage0;
                char *nxt = (kt & 1) ? stage0 : stage1;
                diff_koff = kt * 32;
                // Stage kt has landed in LDS for EVERY wave's reads: this wave's staging instructions are waited for HERE,
                // explicitly, then the barrier.  (Nothing else orders a ds_read behind a pending LDS-DMA: until round 4 the wait
                // was the compiler's -- it puts a vmcnt(0) in front of LDS reads it cannot tell apart from a pending DMA's target
                // -- and one instantiation lost it when the address arithmetic of the staging instructions changed: wrong scores
                // from the third K step on.  Inline asm: the waitcnt pass cannot drop it.)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads(); // buffer nxt is free
                const int koff = (kt + 1) * 32, koff_db = (kt + 1) * KOFF_DB;
                compute(cur, [&](int n) {
                    if (NTDB && n < NDBI) stage_issue<true>(tsrc[n] + koff_db, nxt + lds_off[n]);
                    else stage_issue<false>(tsrc[n] + koff, nxt + lds_off[n]);
                }, nd_all{});
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (see above)
            __syncthreads();
            diff_koff = (KT - 1) * 32;
            compute(((KT - 1) & 1) ? stage1 : stage0, no_dma, nd_none{});
            if constexpr (!NTDB && !BF16) {
                if (p.cu_turn && tid == 0) __hip_atomic_store(my_turn, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if constexpr (DIFF) {
            // the scores change hands: from "thread = row, register = query" to the accumulator layout the MFMA leaves behind
            // (lane (i, h) = query i, registers = 32 rows), through the staging buffers -- everything behind the K loop is shared
            static_assert(DT == 256 && QT == 32, "thread = row");
            float *sT = (float *)smem; // [DIFF_NQ][DT]
            __syncthreads();           // (every wave has read its last fragments)
            {
                constexpr int NPH = DIFF_NQ / 4;
                const int r0 = (wave & 1) * 64 + lane, qh = wave >> 1;
#pragma unroll
                for (int j = 0; j < NPH; j++) {
                    const int pr = qh * NPH + j; // queries 2 pr, 2 pr + 1
                    sT[(2 * pr) * DT + r0] = dacc2[j][0];
                    sT[(2 * pr + 1) * DT + r0] = dacc2[j][1];
                    sT[(2 * pr) * DT + r0 + 128] = dacc2[NPH + j][0];
                    sT[(2 * pr + 1) * DT + r0 + 128] = dacc2[NPH + j][1];
                }
            }
            __syncthreads();
#pragma unroll
            for (int a = 0; a < TM; a++)
#pragma unroll
                for (int r = 0; r < 16; r++)
                    acc[a][0][r] = li < DIFF_NQ ? sT[li * DT + (wm * TM + a) * 32 + 4 * lh + (r & 3) + 8 * (r >> 2)] : INFINITY;
            __syncthreads();           // (the next tile's prologue stages into these buffers)
        }
        if constexpr (F16X) {
            // acc = <q~, x~> of the scaled fp16 copies; the approximate score is acc * 2^(e_q + e_x) -- exact unless it
            // falls below the normal range (then off by < 2^-149, which the bound carries)
#pragma unroll
            for (int a = 0; a < TM; a++)
#pragma unroll
                for (int b = 0; b < TN; b++)
#pragma unroll
                    for (int r = 0; r < 16; r++)
                        acc[a][b][r] = __builtin_ldexpf(acc[a][b][r], f16_qe[b] + ((const int *)s_yn)[rowl(a * 16 + r)]);
        }
        KNN_TRACE(1 + 2 * tile_idx);
        // Two workgroups per CU: behind its K loop a wave's instructions run beside the MFMAs of the OTHER workgroup's wave on
        // the same SIMD.  Straight-line vector code gets through at its own rate (the sparse epilogue's pass 1: 1.6 us for 64
        // scores, alone on the CU or not); anything that WAITS -- an LDS round trip, an atomic's return, a barrier -- takes three
        // to five times what it takes with the CU to itself (per-workgroup stamps of a CATH-sized symmetric tile: epilogue 57 us
        // with two workgroups per CU, 17.5 us with one).  Raising the wave's issue priority here (s_setprio, compile-time knob)
        // changes nothing measurable.
        if constexpr (!BIGT && KNN355_EPI_PRIO > 0) __builtin_amdgcn_s_setprio(KNN355_EPI_PRIO);
        if (paired && tid == 0) *s_next = next_tile; // (read by everyone behind the barrier that ends the epilogue)

        // score s of query block b in this lane (see accv / rowl) -- "smaller is better"
        auto score_of = [&](int b, int s, float xnq) -> float {
            if constexpr (DIFF) {
                return accv(b, s);
            } else if constexpr (L2) {
                const float ynr = s_yn[rowl(s)];
                const float v = __builtin_fmaf(-2.0f, accv(b, s), xnq + ynr);
                return v < 0.0f ? 0.0f : v;
            } else {
                return -accv(b, s);
            }
        };
        // Threshold filter + append of one tile's scores.  passes(b, sc, thr, xnq): does score sc of query block b beat thr;
        // value(b, sc, xnq): the score -- from the accumulators, or read back from the parked first tile.
        //   This code runs beside the OTHER resident workgroup's K loop, whose MFMAs own the SIMD's issue port: per-workgroup
        // stamps of a CATH-sized search showed the filter of round 2 (~45 vector instructions per score: row numbers, view
        // and sample-mask arithmetic in 64 bits, the key, then a divergent append with its own LDS round trip) taking 15-60 us
        // per tile behind a 70-110 us K loop -- about one vector instruction per MFMA of the neighbour.  So: per score ONE
        // compare and a mask bit; everything else only for blocks of 8 scores in which some lane of the wave has a survivor,
        // with the 8 slot reservations (one LDS atomic per score from every lane, adding 0 where the score failed: no
        // divergence) in flight together.  Rows that are not really there (past the end in the last tile, rows of the seed
        // sample) are found only among the survivors and stored as KEY_PAD: every reader of a list drops those.
        auto filter_tile = [&](int64_t trow0, auto &&passes, auto &&value) {
            const bool ragged = trow0 + DT > p.nb, sampled = p.skip_mask >= 0, plain_rows = p.row_mul == 1;
#pragma unroll
            for (int b = 0; b < NB; b++) {
                const int ql = qloc(b);
                const int64_t q = q0 + ql;
                const bool qok = q < p.nq;
                const float thr = qok ? L.threshold(ql) : -INFINITY; // (a query past the end admits nothing)
                float xnq = 0.0f;
                if constexpr (L2) xnq = p.xn[qok ? q : 0];
                uint64_t *lst = L.lists + (size_t)ql * L.cap;
                {
#pragma unroll
                    for (int s8 = 0; s8 < NS / 8; s8++) {
                        uint32_t passm = 0;
#pragma unroll
                        for (int r8 = 0; r8 < 8; r8++) passm |= (passes(b, s8 * 8 + r8, thr, xnq) ? 1u : 0u) << r8;
                        if (__ballot(passm != 0u) == 0ull) continue;
#ifdef KNN355_TRACE
                        if (p.ablate & 2) continue;
#endif
                        int slot[8];
#pragma unroll
                        for (int r8 = 0; r8 < 8; r8++) slot[r8] = atomicAdd(&L.s_cnt[ql], (int)((passm >> r8) & 1u));
                        bool near_full = false;
#pragma unroll
                        for (int r8 = 0; r8 < 8; r8++) {
                            if ((passm >> r8) & 1u) {
                                const int sc = s8 * 8 + r8;
                                const int64_t row = trow0 + rowl(sc);
                                const float vv = value(b, sc, xnq) + 0.0f;
                                const uint32_t id = p.id_base + (plain_rows ? (uint32_t)row : (uint32_t)view_row(row, p.row_mul, p.vshift));
                                const bool gone = (ragged && row >= p.nb) || (sampled && ((int)(row >> p.vshift) & p.skip_mask) == 0);
                                if (slot[r8] < L.cap) lst[slot[r8]] = gone ? KEY_PAD : (((uint64_t)f2ord(vv) << 32) | id);
                                near_full |= slot[r8] + 1 > L.cap - DT;
                            }
                        }
                        if (near_full) *L.s_need = 1;
                    }
                }
            }
        };
        // (squared L2: max(0, x) <= thr is x <= thr for every thr >= 0, and a threshold is a score or +inf)
        auto passes_acc = [&](int b, int sc, float thr, float xnq) -> bool {
            if constexpr (DIFF) {
                return accv(b, sc) <= thr;
            } else if constexpr (L2) {
                const float ynr = s_yn[rowl(sc)];
                return __builtin_fmaf(-2.0f, accv(b, sc), xnq + ynr) <= thr;
            } else {
                return -accv(b, sc) <= thr;
            }
        };
        constexpr int NV4 = NB * NS / 4; // 16-byte pieces of a lane's scores of one tile
        bool deferred = false;
        if constexpr (CAN_PUB) {
            if (pub_on && tile_idx < p.pub_rounds) {
                // ---- tile-minimum seed: publish this tile's best key per query BEFORE the tile is filtered ----
                // lane minimum over its 16 TM TN scores, the other lane half, then the waves through LDS.  The FIRST tile
                // has nothing to filter with yet (unfiltered it would append all of its 256 x QT scores: 32 MB of list
                // writes per launch on a 1.25 M-row shard, +110 us; waiting for the bound costs every workgroup the spread
                // of the arrivals): its scores are parked in global memory (32 KB per workgroup, one coalesced store per
                // 4 accumulator registers) and filtered behind the second tile, when the bound has long been there.
                float4 *park = (float4 *)p.defer + (size_t)blockIdx.x * NV4 * 256 + tid;
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    const int ql = qloc(b);
                    const int64_t q = q0 + ql;
                    float xnq = 0.0f;
                    if constexpr (L2) xnq = p.xn[q < p.nq ? q : 0];
                    uint64_t best = KEY_PAD;
#pragma unroll
                    for (int s4 = 0; s4 < NS / 4; s4++) {
                        float vs[4];
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const int64_t row = row0 + rowl(4 * s4 + e);
                            const float v = score_of(b, 4 * s4 + e, xnq) + 0.0f;
                            vs[e] = v;
                            // (a key that is published must be one the filter would append: a real row of this chunk, finite)
                            if (v < INFINITY && row < p.nb && !(p.skip_mask >= 0 && ((int)(row >> p.vshift) & p.skip_mask) == 0)) {
                                const uint64_t key = ((uint64_t)f2ord(v) << 32) | (p.id_base + (uint32_t)view_row(row, p.row_mul, p.vshift));
                                best = key < best ? key : best;
                            }
                        }
                        if (tile_idx == 0) park[(size_t)(b * (NS / 4) + s4) * 256] = make_float4(vs[0], vs[1], vs[2], vs[3]);
                    }
                    // the other lanes that hold scores of this query: the other lane half (32-query blocks), the three other
                    // lane quarters (16-query blocks)
#pragma unroll
                    for (int off = M16 ? 16 : 32; off < 64; off <<= 1) {
                        const uint32_t ohi = (uint32_t)__shfl_xor((int)(uint32_t)(best >> 32), off);
                        const uint32_t olo = (uint32_t)__shfl_xor((int)(uint32_t)best, off);
                        const uint64_t other = ((uint64_t)ohi << 32) | olo;
                        best = other < best ? other : best;
                    }
                    if (p.pub_m > 1) {
                        // every wave publishes the best key of ITS rows (WM keys of WM different rows per workgroup and query):
                        // enough publications for a k beyond the number of workgroups
                        if (lg == 0 && q < p.nq)
                            __hip_atomic_store(&p.pub[(size_t)q * p.pub_n + ((size_t)tile_idx * p.nchunks + (paired ? (int)blockIdx.x : chunk)) * WM + wm], best,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    } else if (lg == 0 && q < p.nq) {
                        atomicMin((unsigned long long *)&s_pub[ql], (unsigned long long)best);
                    }
                }
                deferred = tile_idx == 0;
                __syncthreads();
                if (wave == 0) {
                    if (lane < QT && p.pub_m == 1) {
                        if (q0 + lane < p.nq)
                            __hip_atomic_store(&p.pub[(size_t)(q0 + lane) * p.pub_n + (size_t)tile_idx * p.nchunks + (paired ? (int)blockIdx.x : chunk)], s_pub[lane],
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        s_pub[lane] = KEY_PAD; // (the next round's minima land after the next K loop's barriers)
                    }
                    // No fence, relaxed counter: a release at agent scope writes back this XCD's whole L2 and an acquire
                    // invalidates it (measured: +120 us per launch).  Nothing here needs the order: a publication a reader
                    // misses reads as KEY_PAD.
                    int a = 0;
                    if (lane == 0) a = (int)__hip_atomic_fetch_add(&p.arrive[qtile], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    a = __builtin_amdgcn_readfirstlane(a);
                    // arrivals take the queries in turn: from the (k + QT)-th on every query has a bound, the last QT
                    // arrivals of a round see (almost) every publication
                    const int ql = a % QT;
                    if (q0 + ql < p.nq && (a + 1) * p.pub_m >= p.k) {
                        uint32_t T = 0xFFFFFFFFu;
                        const int kmax = p.k + max(p.k >> 2, 32);
                        published_bound(p.pub + (size_t)(q0 + ql) * p.pub_n, p.pub_n, p.k, kmax, lane, &T);
                        if (lane == 0 && T != 0xFFFFFFFFu) atomicMin(&L.gthr[ql], T);
                    }
                }
            }
        }

        // ---- the 256 x 256 tile's epilogue ("sparse"): ONE workgroup per CU, so nothing runs beside it -- what filter_tile
        // spends per tile (60-120 us of a 240 us K loop, measured: nearly every block of 8 scores has a survivor in SOME lane,
        // and the wave then walks eight divergent appends) is all exposed.  A lane's 256 scores hold one to three survivors at
        // the densities a warmed-up or seeded threshold leaves (0.3-1.5 %), at random places, and registers cannot be indexed
        // by a lane-varying number.  So:
        //   pass 1  straight-line, eight vector instructions per score (inline asm: left to the compiler the accumulators were
        //           copied out of their AGPRs wholesale and spilled): value, ONE compare, a store of (value, score number) into
        //           the lane's next slot of the (idle) staging buffers -- [slot][thread] x 8 bytes -- by EVERY lane, and a
        //           pointer bump where the compare passed (a failed score's entry is overwritten by the lane's next survivor;
        //           first form, with the store under the compare's exec mask: 11.6 us per tile, the wave waiting on every
        //           vector-to-scalar hand-over); a lane that runs out of slots writes into a dump slot and keeps counting;
        //   pass 2  a wave-wide loop over the slots in use (as many rounds as the busiest lane has survivors): each lane reads
        //           its entry back, works out row and key, reserves a place in the query's list (LDS atomic) and stores.
        // A wave with a lane that ran out of slots (the first tiles of an unseeded chunk, tiles full of near-duplicates) filters
        // the tile the dense way instead.  The symmetric launch's second direction (row R of this tile as a query, the resident
        // tile's rows its candidates) goes the same way with a second compare per score; its survivors are ranked per row in
        // LDS (the atomic's return), one global atomic per row reserves the places, then the keys are stored; a lane out of
        // slots hands the whole tile's second direction to the dense code below.
        bool dir2_dense = SYM && off_diag; // the second direction is (still) the dense code's
        auto sparse_epilogue = [&](int64_t trow0, bool second, auto *dense2) { // (generic: only the 256 x 256 builds instantiate it)
            // Slots per lane and tile (+ a dump slot).  256 x 256 tile: inside staging buffer 1 (buffer 0 is taking the next tile's
            // first K step meanwhile); 128 x 128 tile: both of its 32-KB staging buffers are idle during the epilogue, the
            // symmetric build adds 8 KB (lds_main).  The symmetric launch's two directions use the SAME slots, one after the
            // other: their survivor counts per lane have different tails (squared L2 on raw embeddings has hubs -- a candidate
            // of small norm beats the bound of every row: CATH-sized k = 301, a lane's largest count in a launch: first direction
            // 15, second 27 of its 64 scores, the mean 4.7), and half the slots each sent the second direction of nearly every
            // tile the dense way.
            constexpr int C = BIGT ? 31 : (SYM ? 35 : 30);
            constexpr int OFF1 = BIGT ? STAGE_BYTES : 0;
            static_assert(OFF1 + (C + 1) * 2048 <= (SYM && !BIGT ? 73728 : 2 * STAGE_BYTES), "the lanes' slots fit the staging buffer(s)");
            static_assert(NS % 16 == 0 && NS <= 64 && NB <= 4, "score numbers are sc | block << 8");
            const bool ragged = trow0 + DT > p.nb, sampled = p.skip_mask >= 0, plain_rows = p.row_mul == 1;
            const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) char *)smem);
            int *s_dense = L.s_need + 2;
            const float *thr = big_thr, *xnq = big_xnq;
            const uint64_t *cokm = big_cokm;
            KNN_TRACE_AT(tile_idx == 5, 124);
            const uint32_t w_0 = lds0 + OFF1 + tid * 8;              // LDS address of this lane's first slot
            const uint32_t dump = w_0 + C * 2048, step = 2048;
            const float ninf = -INFINITY;
            uint32_t w = w_0;                                        // ... of its next slot (counts on past the last)
            auto slot_at = [&](int j) -> char * { return smem + OFF1 + (j * 256 + tid) * 8; }; // this lane's slot j (j <= C), as a pointer
            uint32_t nblk[NB] = {};                                  // first direction: 2048 x this lane's survivors of each query block
            KNN_TRACE_AT(tile_idx == 5, 125);
            if constexpr (BIGT) asm volatile("s_nop 15\n\ts_nop 15" ::: "memory"); // (the K loop's last MFMAs -> v_accvgpr_read inside the statements below)
            // Pass 1 of one direction.  Four scores per statement: their value / compare chains are independent and issue back to
            // back (a chain on its own waits out every instruction's latency), only the pointer bumps are serial.  No exec mask, no
            // scalar instruction: EVERY lane stores (value, score number) into its next slot -- a score that fails is overwritten
            // by the lane's next survivor, which lands in the same slot -- and only a survivor moves the pointer on.
            auto pass1 = [&](auto dir_tag) {
                constexpr int DIR = decltype(dir_tag)::value;
                (void)&ninf; (void)&cokm; (void)&thr; (void)&nblk; // (named here: captures that only a discarded branch uses are not made)
#pragma unroll
                for (int c = 0; c < NS; c += 16) {
                    // the norms / second-direction thresholds of this chunk's 16 rows: four consecutive rows per 16-byte LDS read
                    // (all 64 rows of the 256-row tile at once cost 128 registers in the symmetric L2 build: spills between the statements)
                    float ynl[16], t2l[16];
#pragma unroll
                    for (int i = 0; i < 16; i += 4) {
                        f32x4 y4 = {0.0f, 0.0f, 0.0f, 0.0f}, h4 = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
                        if constexpr (L2) y4 = *(const f32x4 *)&s_yn[rowl(c + i)];
                        if constexpr (DIR == 2) h4 = *(const f32x4 *)&s_thr2[rowl(c + i)];
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            ynl[i + e] = y4[e];
                            t2l[i + e] = h4[e];
                        }
                    }
#pragma unroll
                    for (int b = 0; b < NB; b++) {
                        const uint32_t w_b = w; // (this lane's survivors of query block b: what the 16 scores below add to the pointer)
#pragma unroll
                        for (int sc = c; sc < c + 16; sc += 4) {
                            uint32_t t[4], ad[4], ix[4], e[4], u;
                            uint64_t mk[4];
                            (void)e; (void)t2l;
                            const float a0 = accv(b, sc), a1 = accv(b, sc + 1), a2 = accv(b, sc + 2), a3 = accv(b, sc + 3);
                            const float s0 = xnq[b] + ynl[sc - c], s1 = xnq[b] + ynl[sc - c + 1], s2 = xnq[b] + ynl[sc - c + 2], s3 = xnq[b] + ynl[sc - c + 3];
                            (void)s0; (void)s1; (void)s2; (void)s3;
                            // (the second direction: the same values decide for rows rowl(sc ..) as queries; a lane whose own query is no candidate --
                            // past the end, or a row of the sample -- compares against -inf)
                            if constexpr (DIR == 1 && BIGT && L2) KNN_PASS1(KNN_P1_HEAD_AGPR_L2, KNN_P1_BOUND_THR, , "a", KNN_P1_IN_L2, KNN_P1_IN_THR);
                            else if constexpr (DIR == 1 && BIGT) KNN_PASS1(KNN_P1_HEAD_AGPR_IP, KNN_P1_BOUND_THR, , "a", , KNN_P1_IN_THR);
                            else if constexpr (DIR == 1 && L2) KNN_PASS1(KNN_P1_HEAD_VGPR_L2, KNN_P1_BOUND_THR, , "v", KNN_P1_IN_L2, KNN_P1_IN_THR);
                            else if constexpr (DIR == 1) KNN_PASS1(KNN_P1_HEAD_VGPR_IP, KNN_P1_BOUND_THR, , "v", , KNN_P1_IN_THR);
                            else if constexpr (BIGT && L2) KNN_PASS1(KNN_P1_HEAD_AGPR_L2, KNN_P1_BOUND_ROW, KNN_P1_OUT_ROW, "a", KNN_P1_IN_L2, KNN_P1_IN_ROW);
                            else if constexpr (BIGT) KNN_PASS1(KNN_P1_HEAD_AGPR_IP, KNN_P1_BOUND_ROW, KNN_P1_OUT_ROW, "a", , KNN_P1_IN_ROW);
                            else if constexpr (L2) KNN_PASS1(KNN_P1_HEAD_VGPR_L2, KNN_P1_BOUND_ROW, KNN_P1_OUT_ROW, "v", KNN_P1_IN_L2, KNN_P1_IN_ROW);
                            else KNN_PASS1(KNN_P1_HEAD_VGPR_IP, KNN_P1_BOUND_ROW, KNN_P1_OUT_ROW, "v", , KNN_P1_IN_ROW);
                        }
                        if constexpr (DIR == 1) nblk[b] += w - w_b;
                    }
                }
            };
            pass1(std::integral_constant<int, 1>{});
            const uint32_t w1 = w, w1_0 = w_0;
            KNN_TRACE_AT(tile_idx == 5, 126);
            const int n1 = (int)((w1 - w1_0) >> 11);
            // ---- first direction: this wave's survivors -> the queries' lists
            KNN_TRACE_COUNT(__ballot(n1 > C) != 0ull, 60); // (developer build: tiles wave 0 filtered the dense way; slot 59: tiles whose second direction went dense; 58: the wave's largest n1)
#ifdef KNN355_TRACE
            if (p.trace) { // (developer build: the workgroup's largest per-lane survivor counts, first / second direction)
                atomicMax((unsigned long long *)&p.trace[(size_t)blockIdx.x * 128 + 58], (unsigned long long)n1);
            }
#endif
            if (__ballot(n1 > C) != 0ull) {
                filter_tile(trow0, passes_acc, score_of); // (a lane ran out of slots: the dense way, from the accumulators)
            } else {
                // One reservation per lane and query block (LDS atomics) and the lane's first U1 entries, all requested together and
                // waited for ONCE, then stores only; a lane with more entries goes round again.  (Beside the other workgroup's K loop
                // a wave that waits gets back in slowly -- per-workgroup stamps of a CATH-sized symmetric tile: pass 1, straight-line,
                // 1.6 us; this pass with four entries per round and the reservations in front, five waits: 10 us -- so what counts here
                // is the number of waits, not of instructions.)
                constexpr int U1 = 8;
                bool near_full = false;
                int base[NB], run[NB];
                uint2 e[U1];
#pragma unroll
                for (int u = 0; u < U1; u++) e[u] = *(const uint2 *)slot_at(min(u, C));
#pragma unroll
                for (int b = 0; b < NB; b++) {
                    const int cnt = (int)(nblk[b] >> 11);
                    base[b] = atomicAdd(&L.s_cnt[qloc(b)], cnt);
                    run[b] = 0;
                    near_full |= cnt > 0 && base[b] + cnt > L.cap - DT;
                }
                for (int j0 = 0;;) {
#pragma unroll
                    for (int u = 0; u < U1; u++) {
                        if (j0 + u < n1) {
                            const int b = (int)((e[u].y >> 8) & 3u);
                            // (b is a runtime number: the block's base and running count picked out of NB registers each)
                            int slot = base[0] + run[0];
#pragma unroll
                            for (int bb = 1; bb < NB; bb++) slot = b == bb ? base[bb] + run[bb] : slot;
#pragma unroll
                            for (int bb = 0; bb < NB; bb++) run[bb] += b == bb;
                            const int ql = (wn * TN + b) * 32 + li;
                            float vv = __uint_as_float(e[u].x);
                            if constexpr (L2) vv = vv < 0.0f ? 0.0f : vv;
                            vv += 0.0f;
                            const int64_t row = trow0 + rowl((int)(e[u].y & 255u));
                            const uint32_t id = p.id_base + (plain_rows ? (uint32_t)row : (uint32_t)view_row(row, p.row_mul, p.vshift));
                            const bool gone = (ragged && row >= p.nb) || (sampled && ((int)(row >> p.vshift) & p.skip_mask) == 0);
                            if (slot < L.cap) L.lists[(size_t)ql * L.cap + slot] = gone ? KEY_PAD : (((uint64_t)f2ord(vv) << 32) | id);
                        }
                    }
                    j0 += U1;
                    if (__ballot(j0 < n1) == 0ull) break;
#pragma unroll
                    for (int u = 0; u < U1; u++) e[u] = *(const uint2 *)slot_at(min(j0 + u, C));
                }
                if (near_full) *L.s_need = 1;
            }
            KNN_TRACE_AT(tile_idx == 5, 127);
            // ---- second direction (symmetric launch, off the diagonal): the rows of this tile as queries
            if constexpr (SYM) {
                if (!second) return; // (workgroup-uniform: the diagonal tile)
                // pass 1 again, with the rows' bounds, into the same slots (this lane's own: the first direction is through with them)
                w = w_0;
                pass1(std::integral_constant<int, 2>{});
                const int n2 = (int)((w - w_0) >> 11);
                if (n2 > C) *s_dense = 1;
                __syncthreads();
                const bool dense = *s_dense != 0;
                KNN_TRACE_AT(tile_idx == 5, 120);
                KNN_TRACE_COUNT(dense, 59);
#ifdef KNN355_TRACE
                if (p.trace) atomicMax((unsigned long long *)&p.trace[(size_t)blockIdx.x * 128 + 57], (unsigned long long)n2);
#endif
                *dense2 = dense;
                if (dense) return; // (the flag is cleared at the start of the next tile)
                // Ranks inside each row's survivors of this tile (LDS atomics), one global reservation per row, then the stores.
                // A lane's first U2 entries stay in REGISTERS from the rank phase to the stores, a lane with more takes the rest
                // through its LDS slots, four at a time.  (First form: every entry read from LDS in both phases, four entries per
                // round in the rank phase and one in the store phase -- 24 + 16 us of a CATH-sized symmetric tile's 59-us epilogue:
                // a dozen waits and a few dozen, beside the other workgroup's K loop.)
                constexpr int U2 = 16;
                uint2 g[U2];
                int rk[U2];
#pragma unroll
                for (int u = 0; u < U2; u++) g[u] = *(const uint2 *)slot_at(min(u, C));
#pragma unroll
                for (int u = 0; u < U2; u++) rk[u] = atomicAdd(&s_cnt2[rowl((int)(g[u].y & 63u))], u < n2 ? 1 : 0);
                for (int j0 = U2; j0 < n2; j0 += 4) { // (the entries past the registers: rank written back into the slot)
                    uint32_t *yp[4], y[4];
                    int r4[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        yp[u] = (uint32_t *)(slot_at(min(j0 + u, C)) + 4);
                        y[u] = *yp[u];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) r4[u] = atomicAdd(&s_cnt2[rowl((int)(y[u] & 63u))], j0 + u < n2 ? 1 : 0);
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (j0 + u < n2) *yp[u] = y[u] | ((unsigned)r4[u] << 16);
                }
                __syncthreads();
                KNN_TRACE_AT(tile_idx == 5, 121);
                if (tid < DT) {
                    const int c = s_cnt2[tid];
#ifdef KNN355_TRACE
                    if (p.ablate & 64) s_base2[tid] = 0; // (developer build: without the global reservation -- wrong places, right time)
                    else
#endif
                    s_base2[tid] = c > 0 ? (int)atomicAdd(&p.qcnt[trow0 + tid], (uint32_t)c) : 0;
                    s_cnt2[tid] = 0; // (for the next tile)
                }
                __syncthreads();
                KNN_TRACE_AT(tile_idx == 5, 122);
                auto put = [&](float value, int sc, int b, int at_in_row) { // (b is a runtime number: the lane's query of block b, spelled out)
                    const int rl = rowl(sc);
                    float vv = value;
                    if constexpr (L2) vv = vv < 0.0f ? 0.0f : vv;
                    const uint32_t id = p.id_base + (uint32_t)(q0 + (wn * TN + b) * 32 + li);
                    if (at_in_row < p.qcap) p.qlist[(size_t)(trow0 + rl) * p.qcap + at_in_row] = ((uint64_t)f2ord(vv + 0.0f) << 32) | id;
                    else *p.fail = 1;
                };
                int bs[U2];
#pragma unroll
                for (int u = 0; u < U2; u++) bs[u] = s_base2[rowl((int)(g[u].y & 63u))];
#ifdef KNN355_TRACE
                if (p.ablate & 256) return; // (developer build: without the stores)
#endif
#pragma unroll
                for (int u = 0; u < U2; u++)
                    if (u < n2) put(__uint_as_float(g[u].x), (int)(g[u].y & 255u), (int)((g[u].y >> 8) & 3u), bs[u] + rk[u]);
                for (int j = U2; j < n2; j++) {
                    const uint2 e = *(const uint2 *)slot_at(j);
                    const int sc = (int)(e.y & 255u);
                    put(__uint_as_float(e.x), sc, (int)((e.y >> 8) & 3u), s_base2[rowl(sc)] + (int)(e.y >> 16));
                }
            }
        };

        // ---- epilogue: threshold filter + append ----
#ifdef KNN355_TRACE
        if (p.ablate & 4) { // all MFMA results of this wave have landed before the "K loop ended" stamp is taken
            float sink = 0.0f;
#pragma unroll
            for (int b = 0; b < NB; b++) sink += accv(b, NS - 1) + accv(b, NS / 2 - 1);
            if (sink == 12345.678f) KNN_TRACE(61);
            KNN_TRACE(1 + 2 * tile_idx);
        }
        if (!(p.ablate & 1))
#endif
        {
            if (SPARSE && (BIGT || SYM || p.sparse_epi)) {
                // The next tile's first K step goes out NOW, into buffer 0: behind the K loop's last barrier no wave reads a
                // staging buffer any more (the last sub-step runs from registers), the epilogue below keeps its slots in
                // buffer 1, and its ~8 us cover the bytes' way from L2 / HBM -- the tile prologue found them exposed (2-3 us
                // per tile with nothing else on the CU).
                if constexpr (!BIGT) __syncthreads(); // (the generic K loop's last step reads its fragments from LDS: every wave is through before the slots below are written)
                if (BIGT && next_tile >= 0) {
                    const int64_t nrow0 = (int64_t)next_tile * DT;
#pragma unroll
                    for (int n = 0; n < NI; n++) {
                        tsrc[n] = is_db[n] ? srcp[n] + view_row(min(nrow0 + rloc[n], p.nb - 1), p.row_mul, p.vshift) * p.dp : srcp[n];
                        stage_issue<false>(tsrc[n], stage0 + lds_off[n]);
                    }
                    staged0 = true;
                }
                if constexpr (SPARSE) sparse_epilogue(row0, off_diag, &dir2_dense);
            } else if (!deferred) filter_tile(row0, passes_acc, score_of);
        }
        KNN_TRACE(64 + 2 * tile_idx);
        if constexpr (CAN_PUB) {
            if (pub_on && (tile_idx == 1 || (deferred && (paired ? *s_next : next_tile) < 0))) {
                // the parked first tile (every lane reads back what it stored itself); a chunk of a single tile filters
                // it on the spot
                const float4 *park = (const float4 *)p.defer + (size_t)blockIdx.x * NV4 * 256 + tid;
                float4 pv[NV4];
#pragma unroll
                for (int j = 0; j < NV4; j++) pv[j] = park[(size_t)j * 256];
                auto parked = [&](int b, int sc, float) -> float {
                    const float4 w = pv[b * (NS / 4) + (sc >> 2)];
                    return (sc & 3) == 0 ? w.x : ((sc & 3) == 1 ? w.y : ((sc & 3) == 2 ? w.z : w.w));
                };
                filter_tile(first_row0, [&](int b, int sc, float thr, float) -> bool { return parked(b, sc, 0.0f) <= thr; }, parked);
            }
        }
        if constexpr (SYM) {
#ifdef KNN355_TRACE
            if (dir2_dense && !(p.ablate & 8)) {
#else
            if (dir2_dense) {
#endif
                // the same scores, read the other way round: row R of this tile is a query, the resident tile's rows
                // are its candidates.  A (register, lane half) pair of one wave is one row R and 32 candidates.
                auto score = [&](int a, int b, int r, float xnq) -> float {
                    if constexpr (L2) {
                        const float ynr = s_yn[(wm * TM + a) * 32 + 4 * lh + (r & 3) + 8 * (r >> 2)];
                        const float v = __builtin_fmaf(-2.0f, acc[a][b][r], xnq + ynr);
                        return v < 0.0f ? 0.0f : v;
                    } else {
                        return -acc[a][b][r];
                    }
                };
                float xnq[TN];
                bool cand_ok[TN];
#pragma unroll
                for (int b = 0; b < TN; b++) {
                    const int64_t q = q0 + (wn * TN + b) * 32 + li;
                    // a candidate must be a real row that the sample pass has not already handed on
                    cand_ok[b] = q < p.nq && !(p.skip_mask >= 0 && ((int)(q >> p.vshift) & p.skip_mask) == 0);
                    xnq[b] = 0.0f;
                    if constexpr (L2) xnq[b] = p.xn[q < p.nq ? q : 0];
                }
                // pass A: survivors per row (this wave's 64 rows x its 64 candidates)
#pragma unroll
                for (int a = 0; a < TM; a++) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int rl = (wm * TM + a) * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
                        const float thr2 = s_thr2[rl];
                        int c_lo2 = 0, c_hi2 = 0;
#pragma unroll
                        for (int b = 0; b < TN; b++) {
                            const float v = score(a, b, r, xnq[b]);
                            const uint64_t m = __ballot(v <= thr2 && cand_ok[b]);
                            c_lo2 += __popc((uint32_t)m);
                            c_hi2 += __popc((uint32_t)(m >> 32));
                        }
                        if (li == 0) s_cnt2[wn * DT + rl] = lh ? c_hi2 : c_lo2;
                    }
                }
                __syncthreads();
                if (tid < DT) {
                    int c = 0;
#pragma unroll
                    for (int w2 = 0; w2 < WN; w2++) c += s_cnt2[w2 * DT + tid];
                    s_base2[tid] = c > 0 ? (int)atomicAdd(&p.qcnt[row0 + tid], (uint32_t)c) : 0;
                }
                __syncthreads();
                // pass B: the keys, behind the survivors of the waves with a lower query half
#pragma unroll
                for (int a = 0; a < TM; a++) {
#pragma unroll
                    for (int r = 0; r < 16; r++) {
                        const int rl = (wm * TM + a) * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
                        const float thr2 = s_thr2[rl];
                        int pos = s_base2[rl];
                        for (int w2 = 0; w2 < wn; w2++) pos += s_cnt2[w2 * DT + rl];
                        uint64_t *dst = p.qlist + (size_t)(row0 + rl) * p.qcap;
#pragma unroll
                        for (int b = 0; b < TN; b++) {
                            const float v = score(a, b, r, xnq[b]);
                            const bool pass = v <= thr2 && cand_ok[b];
                            const uint64_t m = __ballot(pass);
                            const uint32_t mh = lh ? (uint32_t)(m >> 32) : (uint32_t)m;
                            if (pass) {
                                const int at = pos + __popc(mh & ((1u << li) - 1u));
                                const uint32_t id = p.id_base + (uint32_t)(q0 + (wn * TN + b) * 32 + li);
                                if (at < p.qcap) dst[at] = ((uint64_t)f2ord(v + 0.0f) << 32) | id;
                                else *p.fail = 1;
                            }
                            pos += __popc(mh);
                        }
                    }
                }
            }
        }
        __syncthreads();
        KNN_TRACE(65 + 2 * tile_idx);
        // ---- compaction of lists that could overflow on the next tile ----
        if (paired) next_tile = *s_next;
        const bool last_tile = next_tile < 0;
        if (*L.s_need || last_tile) lists_compact<QT>(L, smem, DT, last_tile, tid);
        KNN_TRACE(2 + 2 * tile_idx);
        if constexpr (!BIGT && KNN355_EPI_PRIO > 0) __builtin_amdgcn_s_setprio(0);
        cur_tile = next_tile;
        tile_idx++;
    }
    if constexpr (!BIGT && KNN355_EPI_PRIO > 0) __builtin_amdgcn_s_setprio(KNN355_EPI_PRIO); // (the flush is epilogue work too)
    lists_flush<QT>(L, s_base, q0, p.nq, p.qlist, p.qcnt, p.qcap, tid, SYM ? p.fail : nullptr);
    KNN_TRACE(63);
}
#undef KNN_P1_HEAD_AGPR_L2
#undef KNN_P1_HEAD_AGPR_IP
#undef KNN_P1_HEAD_VGPR_L2
#undef KNN_P1_HEAD_VGPR_IP
#undef KNN_P1_BOUND_THR
#undef KNN_P1_BOUND_ROW
#undef KNN_P1_TAIL
#undef KNN_P1_OUT_ROW
#undef KNN_P1_IN_L2
#undef KNN_P1_IN_THR
#undef KNN_P1_IN_ROW
#undef KNN_PASS1

// ---------------------------------------------------------------------------
// final selection: one workgroup per query picks the best k of that query's candidate keys,
// sorts them and emits D / I, sorted keys, or the seed of the enclosing search.
//   input   contiguous: keys in + q * in_stride, count cnt[q] (clamped to cap) or n_fixed
//           list-major: an all-gather buffer [lm_lists][nq][lm_k] (KEY_PAD = no key)
//   method  keys are distinct 64-bit numbers (score word << 32 | row id), so f(X) = #(keys < X)
//           takes every value: a bracket search on X -- probes alternate between linear
//           interpolation of the target rank and bisection -- stops at the first X with
//           k <= f(X) <= kmax (3-6 probes; heavy ties on the score word are spread by the id
//           word).  Up to 256 * R keys live in registers (one compare + add per key and probe);
//           longer arrays are re-read from L2 on every probe.  The <= kmax survivors are packed
//           into LDS and sorted by the whole workgroup.
// ---------------------------------------------------------------------------
struct SelectParams {
    const uint64_t *in;
    int64_t in_stride;
    const uint32_t *cnt;
    int n_fixed, cap;
    int n_expect;         // host's estimate of a typical count (0: cap) -- picks the build, any count is handled
    // end-of-search reset (streaming searches with the tile-minimum seed): the final selection leaves the level's state the
    // way init_level_kernel would -- the next search of the same shape needs no launch in front of its scan
    uint32_t *rs_gthr, *rs_qcnt, *rs_qthr, *rs_arrive, *rs_pair;
    uint64_t *rs_pub;
    int rs_nslots, rs_pub_n, rs_narrive, rs_npairs;
    int seg_len, nseg;    // segment pass (nseg > 0): workgroup (q, s) selects among keys [s * seg_len, (s + 1) * seg_len) of query q
                          // and writes output row q * nseg + s
    int lm_lists, lm_k;
    int64_t nq;
    int k, metric;
    uint64_t *out_keys;   // sorted keys (may be null): k per query at out_keys + q * out_stride, padded with KEY_PAD up to out_fill
    int64_t out_stride;
    int out_fill;
    float *D;             // final distances / ids (may be null)
    int64_t *I;
    // seeding the enclosing search from this (sample) result: its candidate count, its running
    // threshold = the score word of the seed_j-th key (no bound if there are fewer), and -- for a
    // statistical seed -- the same word as the bound its own result is verified against
    uint32_t *seed_cnt, *seed_gthr, *seed_qthr;
    int seed_j, seed_stat;
    int64_t seed_nslots;  // threshold slots of the enclosing search (>= nq: the last query tile is padded)
    const uint32_t *qthr; // verification: a k-th score word above qthr[q] means the statistical threshold was too tight
    int *fail;
    // gated launch (see ScanParams::gate); gate_count: counts the launches that ran (the fallbacks taken)
    const uint32_t *gate;
    int gate_n;
    uint32_t *gate_count;
};

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = __shfl_xor(x, o, 64);
        x = y < x ? y : x;
    }
    return x;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t x)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint64_t y = __shfl_xor(x, o, 64);
        x = y > x ? y : x;
    }
    return x;
}

// R keys per thread in registers, NT threads.  SEED: this is a seed sample's selection -- no sorted
// output; it hands the enclosing search the sample's rows that beat T = the sample's seed_j-th
// score (unsorted candidates, at most k of them), T itself as the running threshold and, for a
// statistical seed, as the bound the enclosing result is verified against.
template <int R, int NT, bool SEED>
__global__ __launch_bounds__(NT) void select_topk_kernel(SelectParams p)
{
    constexpr int NW = NT / 64;
    if (p.gate) { // (uniform, in front of every barrier)
        uint32_t any = 0;
        for (int i = 0; i < p.gate_n; i++) any |= p.gate[i];
        if (!any) return;
        if (p.gate_count && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(p.gate_count, 1u);
    }
    extern __shared__ __attribute__((aligned(16))) char smem[];
    uint64_t *sb = (uint64_t *)smem; // [P] survivors, sorted in place (final mode)
    __shared__ int s_red[2][NW];
    __shared__ int s_scan[NW];
    __shared__ uint64_t s_mm[2][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t q = blockIdx.x;
    const int k = p.k;
    int n = p.lm_lists > 0 ? p.lm_lists * p.lm_k : (p.cnt ? (int)min(p.cnt[q], (uint32_t)p.cap) : p.n_fixed);
    int seg_base = 0;
    int64_t orow = q; // output row
    if (p.nseg > 0) {
        seg_base = (int)blockIdx.y * p.seg_len;
        n = max(0, min(n - seg_base, p.seg_len));
        orow = q * p.nseg + blockIdx.y;
    }
    // A key whose score word is f2ord(+inf) or above is no key (a "smaller is better" value of +inf or
    // a NaN never becomes a hit).  The scan's filters admit v <= threshold with ONE compare per score, and a list's threshold
    // starts at +inf: until a list has been cut, a +inf score gets in.  It is dropped HERE, where every result leaves the
    // scan -- D / I, out_keys, the seed's candidates and bound, the segment pass and the merge of shard lists all read their
    // keys through this function -- so a starved list is padded and counted exactly as the oracle's.  (The words above
    // f2ord(+inf) are the positive NaNs and KEY_PAD's own; a NaN fails every compare of the scan and never gets this far.)
    auto load = [&](int idx) -> uint64_t {
        uint64_t v;
        if (p.lm_lists > 0) {
            const int l = idx / p.lm_k, j = idx - l * p.lm_k;
            v = ((gptr_u64)p.in)[((size_t)l * p.nq + q) * p.lm_k + j];
        } else {
            v = ((gptr_u64)p.in)[(size_t)q * p.in_stride + seg_base + idx];
        }
        return (uint32_t)(v >> 32) >= KEY_WORD_INF ? KEY_PAD : v;
    };
    const bool in_regs = n <= NT * R;
    // memory path (more keys than the registers hold): several independent loads in flight per thread
    auto for_each_mem = [&](auto &&fn) {
        constexpr int U = NT >= 1024 ? 4 : 8; // (the 1024-thread build has 128 registers per lane)
        int idx = tid;
        for (; idx + (U - 1) * NT < n; idx += U * NT) {
            uint64_t v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = load(idx + u * NT);
#pragma unroll
            for (int u = 0; u < U; u++) fn(v[u]);
        }
        for (; idx < n; idx += NT) fn(load(idx));
    };
    uint64_t key[R];
    uint64_t mn = KEY_PAD, mx = 0;
    int real = 0;
    if (in_regs) {
#pragma unroll
        for (int r = 0; r < R; r++) {
            const int idx = r * NT + tid;
            uint64_t v = KEY_PAD;
            if (r * NT < n) { // (uniform) registers past the end of a short array cost nothing
                v = load(idx < n ? idx : n - 1);
                if (idx >= n) v = KEY_PAD;
            }
            key[r] = v;
            if (v != KEY_PAD) {
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
                real++;
            }
        }
    } else {
        for_each_mem([&](uint64_t v) {
            if (v != KEY_PAD) {
                mn = v < mn ? v : mn;
                mx = v > mx ? v : mx;
                real++;
            }
        });
    }
    mn = wave_min_u64(mn);
    mx = wave_max_u64(mx);
    real = wave_sum(real);
    if (lane == 0) {
        s_mm[0][wave] = mn;
        s_mm[1][wave] = mx;
        s_scan[wave] = real;
    }
    __syncthreads();
    real = 0;
#pragma unroll
    for (int w2 = 0; w2 < NW; w2++) {
        mn = min(mn, s_mm[0][w2]);
        mx = max(mx, s_mm[1][w2]);
        real += s_scan[w2];
    }
    __syncthreads(); // s_scan is reused below

    int par = 0;
    auto count_lt = [&](uint64_t X) -> int {
        int c = 0;
        if (in_regs) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r * NT < n) c += key[r] < X ? 1 : 0; // (uniform: registers past the end hold padding)
        } else {
            for_each_mem([&](uint64_t v) { c += v < X ? 1 : 0; });
        }
        c = wave_sum(c);
        if (lane == 0) s_red[par][wave] = c;
        __syncthreads();
        c = 0;
#pragma unroll
        for (int w2 = 0; w2 < NW; w2++) c += s_red[par][w2];
        par ^= 1; // the next probe writes the other set: one barrier per probe is enough
        return c;
    };
    // X with klo <= #(keys < X) <= khi, or KEY_PAD when no more than khi real keys exist; *cnt_out = that count
    auto bracket = [&](int klo, int khi, int *cnt_out) -> uint64_t {
        if (real <= khi) {
            *cnt_out = real;
            return KEY_PAD;
        }
        uint64_t lo = mn, hi = mx + 1; // f(lo) = 0 < klo, f(hi) = real > khi
        int f_lo = 0, f_hi = real;
        const double target = 0.5 * (double)(klo + khi);
        bool interpolate = true;
        for (int it = 0; it < 200; it++) {
            const uint64_t w = hi - lo;
            if (w <= 1) break; // cannot happen while the keys are distinct
            uint64_t X;
            if (interpolate) X = lo + (uint64_t)((double)w * ((target - (double)f_lo) / (double)(f_hi - f_lo)));
            else X = lo + (w >> 1);
            X = max(lo + 1, min(X, hi - 1));
            interpolate = !interpolate;
            const int c = count_lt(X);
            if (c < klo) {
                lo = X;
                f_lo = c;
            } else if (c > khi) {
                hi = X;
                f_hi = c;
            } else {
                *cnt_out = c;
                return X;
            }
        }
        *cnt_out = f_hi; // duplicate keys (never in a well-formed input): keep the tie, the caller clamps
        return hi;
    };
    // position of this thread's first survivor in the packed output (workgroup-wide exclusive scan)
    auto survivors_base = [&](uint64_t T) -> int {
        int mine = 0;
        if (in_regs) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r * NT < n) mine += key[r] < T ? 1 : 0;
        } else {
            for_each_mem([&](uint64_t v) { mine += v < T ? 1 : 0; });
        }
        const int incl = wave_inclusive_scan(mine);
        if (lane == 63) s_scan[wave] = incl;
        __syncthreads();
        int pos = incl - mine;
        for (int w2 = 0; w2 < wave; w2++) pos += s_scan[w2];
        return pos;
    };
    auto pack = [&](uint64_t T, int pos, uint64_t *dst, int limit) {
        if (in_regs) {
#pragma unroll
            for (int r = 0; r < R; r++)
                if (r * NT < n && key[r] < T) {
                    if (pos < limit) dst[pos] = key[r];
                    pos++;
                }
        } else {
            for_each_mem([&](uint64_t v) {
                if (v < T) {
                    if (pos < limit) dst[pos] = v;
                    pos++;
                }
            });
        }
    };

    if constexpr (SEED) {
        // T = the score word of a key of rank r in [seed_j, 1.25 seed_j] (any rank >= seed_j is a bound at least as
        // safe as the seed_j-th, and a loose target converges in 3-5 probes where the exact rank takes dozens);
        // the sample hands on every row that beats T (score word <= T: ties included, the main pass admits
        // them too) -- at most kmax of them, the k best if more rows than that tie into the bound
        const int kmax = k + max(k >> 2, 32);
        int cj = 0;
        uint32_t T = 0xFFFFFFFFu;
        uint64_t Tkey = KEY_PAD;
        int cnt = real;
        if (real >= p.seed_j) {
            const uint64_t Xj = bracket(p.seed_j, p.seed_j + max(p.seed_j >> 2, 8), &cj);
            // the largest key below Xj carries the bound
            uint64_t m = 0;
            if (in_regs) {
#pragma unroll
                for (int r = 0; r < R; r++)
                    if (r * NT < n) m = (key[r] < Xj && key[r] > m) ? key[r] : m;
            } else {
                for_each_mem([&](uint64_t v) { m = (v < Xj && v > m) ? v : m; });
            }
            m = wave_max_u64(m);
            if (lane == 0) s_mm[0][wave] = m;
            __syncthreads();
#pragma unroll
            for (int w2 = 0; w2 < NW; w2++) m = max(m, s_mm[0][w2]);
            T = (uint32_t)(m >> 32);
            Tkey = T == 0xFFFFFFFFu ? KEY_PAD : ((uint64_t)(T + 1u) << 32);
            cnt = Tkey == KEY_PAD ? real : count_lt(Tkey);
            if (cnt > kmax) {
                // (heavy ties into the bound) the best k..kmax of them.  For an EXACT seed k is the caller's k and no row
                // beyond the k-th can matter.  A STATISTICAL seed searched its sample with k_sample ~ 1.25 j << the caller's
                // k: sample rows cut here are masked out of the main scan, and one of them could belong to the caller's
                // top k while the verification (k-th <= T) still passes.  Too many ties to hand on: the estimate is
                // withdrawn, the caller repeats the search without it.
                if (p.seed_stat && tid == 0 && p.fail) *p.fail = 1;
                Tkey = bracket(k, kmax, &cnt);
            }
        }
        cnt = min(cnt, kmax);
        const int pos = survivors_base(Tkey);
        pack(Tkey, pos, p.out_keys + (size_t)q * p.out_stride, kmax);
        if (tid == 0) {
            p.seed_cnt[q] = (uint32_t)cnt;
            p.seed_gthr[q] = T;
            p.seed_qthr[q] = p.seed_stat ? T : 0xFFFFFFFFu;
        }
        // threshold slots of the padding queries of the last query tile (they mirror the last query and append nothing)
        if (q == 0)
            for (int64_t i = p.nq + tid; i < p.seed_nslots; i += NT) p.seed_gthr[i] = 0xFFFFFFFFu;
        return;
    } else {
        const int kmax = k + max(k >> 2, 32);
        int cnt = real;
        const uint64_t T = bracket(k, kmax, &cnt); // survivors: keys < T (KEY_PAD: every real key)
        int P = 64;
        while (P < cnt) P <<= 1;
        const int Pcap = 1 << (32 - __builtin_clz(kmax - 1)); // what the host sized the LDS for: next_pow2(kmax)
        if (P > Pcap) P = Pcap;
        const int pos = survivors_base(T);
        pack(T, pos, sb, P);
        for (int i = cnt + tid; i < P; i += NT) sb[i] = KEY_PAD;
        __syncthreads();
        if (NT == 64 && P <= 1024) { // (one wave per query: the sort stays in registers)
            switch (P) {
            case 64: wave_bitonic_sort_regs<1>(sb, lane); break;
            case 128: wave_bitonic_sort_regs<2>(sb, lane); break;
            case 256: wave_bitonic_sort_regs<4>(sb, lane); break;
            case 512: wave_bitonic_sort_regs<8>(sb, lane); break;
            default: wave_bitonic_sort_regs<16>(sb, lane); break;
            }
            __syncthreads();
        } else {
            wg_bitonic_sort(sb, P, tid, NT);
        }
        cnt = min(cnt, P);
        const int have = min(cnt, k); // real keys among the first k
        for (int i = tid; i < max(k, p.out_fill); i += NT) {
            const uint64_t v = i < have ? sb[i] : KEY_PAD;
            if (p.out_keys) p.out_keys[(size_t)orow * p.out_stride + i] = v;
            if (p.D && i < k) {
                const size_t o = (size_t)q * k + i;
                if (v == KEY_PAD) {
                    p.D[o] = p.metric == KNN_METRIC_INNER_PRODUCT ? -FLT_MAX : FLT_MAX;
                    p.I[o] = -1;
                } else {
                    const float f = ord2f((uint32_t)(v >> 32));
                    p.D[o] = p.metric == KNN_METRIC_INNER_PRODUCT ? -f : f;
                    p.I[o] = (int64_t)(uint32_t)v;
                }
            }
        }
        if (tid == 0 && p.qthr && p.fail) {
            const uint32_t kth = cnt >= k ? (uint32_t)(sb[k - 1] >> 32) : 0xFFFFFFFFu;
            if (kth > p.qthr[q]) *p.fail = 1;
        }
        if (p.rs_gthr) { // (this query's candidates have been read: barriers above)
            if (tid == 0) {
                p.rs_qcnt[q] = 0u;
                p.rs_qthr[q] = 0xFFFFFFFFu;
                p.rs_gthr[q] = 0xFFFFFFFFu;
            }
            for (int j = tid; j < p.rs_pub_n; j += NT) p.rs_pub[(size_t)q * p.rs_pub_n + j] = KEY_PAD;
            if (q == 0) {
                for (int64_t i = p.nq + tid; i < p.rs_nslots; i += NT) p.rs_gthr[i] = 0xFFFFFFFFu;
                for (int i = tid; i < p.rs_narrive; i += NT) p.rs_arrive[i] = 0u;
                for (int i = tid; i <= p.rs_npairs; i += NT) p.rs_pair[i] = i < p.rs_npairs ? 2u : 0u;
            }
        }
    }
}

// (re)initialises a level's per-query state in one launch: running thresholds "no bound", empty candidate
// arrays, no verification bound
__global__ void init_level_kernel(uint32_t *__restrict__ gthr, int64_t nslots, uint32_t *__restrict__ qcnt,
                                  uint32_t *__restrict__ qthr, int64_t nq, int *__restrict__ flag,
                                  uint64_t *__restrict__ pub = nullptr, int64_t npub = 0, uint32_t *__restrict__ arrive = nullptr,
                                  int64_t narrive = 0, uint32_t *__restrict__ pair_ctr = nullptr, int64_t npairs = 0,
                                  const uint32_t *__restrict__ gate = nullptr, int gate_n = 0)
{
    if (gate) { // (a gated fallback launch, see ScanParams::gate)
        uint32_t any = 0;
        for (int j = 0; j < gate_n; j++) any |= gate[j];
        if (!any) return;
    }
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pair_ctr) // paired walk: tickets 0 and 1 are the two workgroups' first tiles
        for (int64_t j = i; j <= npairs; j += (int64_t)gridDim.x * blockDim.x) pair_ctr[j] = j < npairs ? 2u : 0u; // ([npairs]: the pool's)
    if (pub) { // tile-minimum seed: nothing published yet
        for (int64_t j = i; j < npub; j += (int64_t)gridDim.x * blockDim.x) pub[j] = KEY_PAD;
        if (i < narrive) arrive[i] = 0u;
    }
    if (gthr && i < nslots) gthr[i] = 0xFFFFFFFFu;
    if (qcnt && i < nq) {
        qcnt[i] = 0u;
        qthr[i] = 0xFFFFFFFFu;
    }
    if (flag && i == 0) *flag = 0;
}

// ---------------------------------------------------------------------------
// gather distances: one wave per (query, candidate) pair, same fma chain order
// ---------------------------------------------------------------------------
__global__ void pair_distance_kernel(const float *__restrict__ xb, const float *__restrict__ yn,
                                     const float *__restrict__ xq, const float *__restrict__ xn,
                                     int dp, int metric, int64_t npairs,
                                     const int32_t *__restrict__ pair_q, const int64_t *__restrict__ pair_r,
                                     float *__restrict__ out)
{
    // Each lane runs whole chains for separate pairs (the chain is sequential in k).
    int64_t pidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pidx >= npairs) return;
    const float *q = xq + (int64_t)pair_q[pidx] * dp;
    const float *y = xb + pair_r[pidx] * dp;
    float acc = 0.0f;
    for (int k0 = 0; k0 < dp; k0 += 8) {
        f32x4 q0 = *(const f32x4 *)(q + k0), q1 = *(const f32x4 *)(q + k0 + 4);
        f32x4 y0 = *(const f32x4 *)(y + k0), y1 = *(const f32x4 *)(y + k0 + 4);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            acc = __builtin_fmaf(q0[m], y0[m], acc);
            acc = __builtin_fmaf(q1[m], y1[m], acc);
        }
    }
    if (metric == KNN_METRIC_L2) {
        float t = xn[pair_q[pidx]] + yn[pair_r[pidx]];
        float v = __builtin_fmaf(-2.0f, acc, t);
        acc = v < 0.0f ? 0.0f : v;
    }
    out[pidx] = acc;
}


// ---------------------------------------------------------------------------
// exact 16-bit prefilter: fp16 copies with power-of-two scales, the error bound, the re-scoring tail
// ---------------------------------------------------------------------------
// index-wide statistics of the fp16 copies (uint32 words): R = max |x - x'|, X' = max |x'|, X = max |x| (float bits, rounded
// up), the largest row exponent (int), "a row holds a value that is not finite"
enum { S16_R = 0, S16_XP = 1, S16_X = 2, S16_EMAX = 3, S16_NONFINITE = 4, S16_NSTAT = 8 };

// a float >= v (v >= 0): a relative margin of 2^-20, rounded to float, one step up
__device__ __forceinline__ float s16_up(double v)
{
    const float f = (float)(v * (1.0 + 0x1p-20));
    return nextafterf(f, INFINITY);
}

// One wave converts one vector of n fp32 values (zeros from n to np16): y = fp16(x * 2^-e) with max|x| * 2^-e in [2^13, 2^14)
// (e >= emin), scaled values below the fp16 normal range stored as 0 -- no 16-bit subnormals.  Returns e; *nx, *nxp, *nd: the
// Euclidean norms of x, of x' = 2^e y and of x - x' (in double, every lane gets them); *bad: a value is not finite.
__device__ __forceinline__ int s16_convert(const float *__restrict__ x, int n, int np16, _Float16 *__restrict__ y, int emin, int lane,
                                           double *nx, double *nxp, double *nd, bool *bad)
{
    float mx = 0.0f;
    bool nf = false;
    for (int i = lane; i < n; i += 64) {
        const float v = x[i];
        nf |= !isfinite(v);
        mx = fmaxf(mx, fabsf(v));
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    *bad = __ballot(nf) != 0ull;
    int e = (mx > 0.0f && isfinite(mx)) ? ilogbf(mx) - 13 : 0;
    e = max(e, emin);
    double sx = 0.0, sxp = 0.0, sd = 0.0;
    for (int i = lane; i < np16; i += 64) {
        const float v = i < n ? x[i] : 0.0f;
        _Float16 h = (_Float16)ldexpf(v, -e);
        if (!(fabsf((float)h) >= 0x1p-14f)) h = (_Float16)0.0f;
        y[i] = h;
        const double xp = ldexp((double)(float)h, e), dv = (double)v;
        sx += dv * dv;
        sxp += xp * xp;
        sd += (dv - xp) * (dv - xp);
    }
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o, 64);
        sxp += __shfl_xor(sxp, o, 64);
        sd += __shfl_xor(sd, o, 64);
    }
    *nx = sqrt(sx);
    *nxp = sqrt(sxp);
    *nd = sqrt(sd);
    return e;
}

// rows [r0, r0 + n) of the index -> fp16 copies [.][dp16] + exponents; their norms go into the statistics.  One wave per row.
__global__ __launch_bounds__(256) void scan16_rows_kernel(const float *__restrict__ xb, int dp, int64_t r0, int64_t n, int dp16,
                                                          _Float16 *__restrict__ xs, int8_t *__restrict__ xexp, uint32_t *__restrict__ stat)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = r0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= r0 + n) return;
    double nx, nxp, nd;
    bool bad;
    const int e = s16_convert(xb + (size_t)r * dp, dp, dp16, xs + (size_t)r * dp16, -128, lane, &nx, &nxp, &nd, &bad);
    if (lane == 0) {
        xexp[r] = (int8_t)e; // (in [-128, 114]: ilogb of a finite float is at most 127)
        if (bad) {
            atomicOr(&stat[S16_NONFINITE], 1u);
        } else {
            atomicMax(&stat[S16_R], __float_as_uint(s16_up(nd)));
            atomicMax(&stat[S16_XP], __float_as_uint(s16_up(nxp)));
            atomicMax(&stat[S16_X], __float_as_uint(s16_up(nx)));
            atomicMax((int *)&stat[S16_EMAX], e);
        }
    }
}

// The 12-bit copies (knn_flat_set_scan16 mode 2): n = rint(x 2^-e) clamped to [-2047, 2047] with max|x| 2^-e in [2^10, 2^11)
// (e >= -128), x' = 2^e n -- integers an fp16 holds exactly, so the scan multiplies exact fp16 values as before and only R is
// larger.  Stored as u = n + 2048 = 16 hb + lo in the order the scan's LDS wants them (flat_scan_kernel, X12): per tile of 256
// rows and K step of 64 values 16 KB of bytes hb, then 8 KB of nibbles lo; 1.5 bytes per value.  One wave per row, a lane
// per 8 values (one K-step quarter of a lane half: 8 bytes + 4 bytes).  Statistics as scan16_rows_kernel's, from the actual x'.
__global__ __launch_bounds__(256) void scan12_rows_kernel(const float *__restrict__ xb, int dp, int64_t r0, int64_t n, int dp16,
                                                          uint8_t *__restrict__ xs, int8_t *__restrict__ xexp, uint32_t *__restrict__ stat)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = r0 + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= r0 + n) return;
    const float *x = xb + (size_t)r * dp;
    float mx = 0.0f;
    bool nf = false;
    for (int i = lane; i < dp; i += 64) {
        const float v = x[i];
        nf |= !isfinite(v);
        mx = fmaxf(mx, fabsf(v));
    }
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const bool bad = __ballot(nf) != 0ull;
    int e = (mx > 0.0f && isfinite(mx)) ? ilogbf(mx) - 10 : 0;
    e = max(e, -128);
    const int KT = dp16 / 64, rt = (int)(r & 255), li = rt & 31, wa = rt >> 5; // (wa: the row tile of 32 inside the tile of 256)
    uint8_t *tile = xs + (size_t)(r >> 8) * KT * 24576;
    double sx = 0.0, sxp = 0.0, sd = 0.0;
    for (int g = lane; g < dp16 / 8; g += 64) { // values 8 g .. 8 g + 7: K step g / 8, MFMA t = (g / 2) % 4, lane half g % 2
        const int ks = g >> 3, t = (g >> 1) & 3, lh = g & 1;
        uint32_t hw[2] = {0u, 0u}, lw = 0u;
        for (int j = 0; j < 8; j++) {
            const int i = 8 * g + j;
            const float v = i < dp ? x[i] : 0.0f;
            float nv = rintf(ldexpf(v, -e)); // (round to nearest even; not finite only in a row that turns the path off)
            nv = fminf(fmaxf(nv, -2047.0f), 2047.0f);
            const int ni = nv == nv ? (int)nv : 0;
            const uint32_t u = (uint32_t)(ni + 2048);
            hw[j >> 2] |= (u >> 4) << (8 * (j & 3));
            lw |= (u & 15u) << (8 * (j & 3) + 4 * (j >> 2));
            const double xp = ldexp((double)ni, e), dv = (double)v;
            sx += dv * dv;
            sxp += xp * xp;
            sd += (dv - xp) * (dv - xp);
        }
        uint8_t *ksp = tile + (size_t)ks * 24576;
        *(uint2 *)(ksp + (wa * 2 + (t >> 1)) * 1024 + (lh * 32 + li) * 16 + (t & 1) * 8) = make_uint2(hw[0], hw[1]);
        *(uint32_t *)(ksp + 16384 + wa * 1024 + (lh * 32 + li) * 16 + t * 4) = lw;
    }
    for (int o = 32; o > 0; o >>= 1) {
        sx += __shfl_xor(sx, o, 64);
        sxp += __shfl_xor(sxp, o, 64);
        sd += __shfl_xor(sd, o, 64);
    }
    if (lane == 0) {
        xexp[r] = (int8_t)e; // (in [-128, 117])
        if (bad) {
            atomicOr(&stat[S16_NONFINITE], 1u);
        } else {
            atomicMax(&stat[S16_R], __float_as_uint(s16_up(sqrt(sd))));
            atomicMax(&stat[S16_XP], __float_as_uint(s16_up(sqrt(sxp))));
            atomicMax(&stat[S16_X], __float_as_uint(s16_up(sqrt(sx))));
            atomicMax((int *)&stat[S16_EMAX], e);
        }
    }
}

// Per search: the fp16 queries + exponents, and each query's bound B_q >= |s - s~| over every row:
//   B_q = |q| R + |q - q'| X' + g(dp, u) |q| X + g(dp16, 4u) |q'| X' + (dp + 1) 2^-149,   g(n, v) = n v / (1 - n v), u = 2^-24
// (the contract's fmaf chain; the f16 MFMA's fp32 accumulation, allowed four times the error of a round-to-nearest add; the
// roundings below the normal range, where g's relative model does not hold: each of the chain's dp steps rounds a subnormal
// partial sum to a multiple of 2^-149, and so does the ldexp of the approximate score -- half of 2^-149 each, counted whole.
// The term was a flat 2^-140 for the ldexp alone: at d = 1280 a row and a query whose products are all 2^-150 give s = 0 and
// s~ = 640 * 2^-149 against a bound of 512.54 * 2^-149, tests/test_scan16_reference.py).  fail[q] = 1 sends the search
// to its fp32 fallback: a query value or the bound is not finite, an exponent sum could overflow a score, a row is not
// finite.  One wave per query.
__global__ __launch_bounds__(64) void scan16_queries_kernel(const float *__restrict__ xq, int dp, int dp16, _Float16 *__restrict__ q16,
                                                            int *__restrict__ qexp, float *__restrict__ Bq, uint32_t *__restrict__ fail,
                                                            const uint32_t *__restrict__ stat, uint32_t *__restrict__ sstat, int first)
{
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    double nq, nqp, nd;
    bool bad;
    const int e = s16_convert(xq + (size_t)q * dp, dp, dp16, q16 + (size_t)q * dp16, -100000, lane, &nq, &nqp, &nd, &bad);
    if (lane == 0) {
        const double R = __uint_as_float(stat[S16_R]), Xp = __uint_as_float(stat[S16_XP]), X = __uint_as_float(stat[S16_X]);
        const double u = 0x1p-24, g1 = dp * u / (1.0 - dp * u), g2 = dp16 * 4.0 * u / (1.0 - dp16 * 4.0 * u);
        const double B = nq * R + nd * Xp + g1 * nq * X + g2 * nqp * Xp + (dp + 1) * 0x1p-149;
        const float Bf = s16_up(B);
        qexp[q] = e;
        Bq[q] = Bf;
        fail[q] = (bad || !isfinite(Bf) || (int64_t)e + (int)stat[S16_EMAX] > 80 || stat[S16_NONFINITE]) ? 1u : 0u;
        if (q == 0 && first) sstat[0] = 0u; // (the largest window of this search -- its first prefiltered piece -- see rescore16_kernel)
    }
}

// The tail of a 16-bit prefiltered search, one workgroup per (query, slice of RS16_ROWS of its k' keys).  ak[q]: the exact
// top-kp of the approximate keys, sorted.  With t = the k-th of them and B = B_q, every row of the exact top-k has an
// approximate score <= t + 2B; all those rows are among the kp if the kp-th approximate score is above t + 2B (or the kp hold
// fewer real rows) -- otherwise fail[q] = 1 and the gated fp32 search behind this launch redoes the search.  Every slice derives
// that check from the same four words, so all slices of a query agree; slice 0 writes fail[q] and counts the query's window
// for sstat[0].  The rows inside the window are scored with the contract's chain (pair_distance_kernel's order) into exact keys
// ok[q][0 .. kp) (KEY_PAD elsewhere); their top-k is the search's result.
//   fetching  the 256 threads read a slab of RS16_SLAB floats of each of the slice's rows together, 16 contiguous bytes per
//             lane (a 4 KB row is one fully coalesced load instruction), all rows' loads in flight at once, into LDS
//   chain     lane r < RS16_ROWS then runs row r's chain out of LDS, one accumulator carried across the slabs.  The row pitch
//             is the slab + 4 floats: the 16 lanes' ds_read_b128 of one column fall on 16 different 16-byte bank slots
constexpr int RS16_ROWS = 16, RS16_SLAB = 1024;
static inline int rescore16_slab(int dp) { return dp < RS16_SLAB ? dp : RS16_SLAB; }
// dynamic LDS: the query's slab + RS16_ROWS padded row slabs (69888 bytes from dp = 1024 on: the launch opts in)
static inline size_t rescore16_lds(int dp) { return ((size_t)rescore16_slab(dp) + (size_t)RS16_ROWS * (rescore16_slab(dp) + 4)) * 4; }

__global__ __launch_bounds__(256) void rescore16_kernel(const uint64_t *__restrict__ ak, int kp, int k, const float *__restrict__ Bq,
                                                        const uint32_t *__restrict__ pfail, uint32_t *__restrict__ fail,
                                                        const float *__restrict__ xb, int dp, const float *__restrict__ xq, uint32_t id_base,
                                                        uint64_t *__restrict__ ok, uint32_t *__restrict__ sstat)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int sl0 = dp < RS16_SLAB ? dp : RS16_SLAB, pitch = sl0 + 4;
    float *sq = (float *)smem; // [sl0] the query's slab
    float *sy = sq + sl0;      // [RS16_ROWS][pitch] the rows' slabs
    __shared__ int s_cnt;
    const int tid = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int j0 = (int)blockIdx.y * RS16_ROWS;
    const uint64_t *a = ak + (size_t)q * kp;
    // the window check (uniform: every thread of every slice computes it from the same words)
    bool f = pfail[q] != 0u;
    double lim = INFINITY;
    {
        const uint64_t tk = a[k - 1], last = a[kp - 1];
        if (!f && tk != KEY_PAD) {
            lim = (double)ord2f((uint32_t)(tk >> 32)) + 2.0 * (double)Bq[q];
            if (last != KEY_PAD && !(lim < (double)ord2f((uint32_t)(last >> 32)))) f = true;
        }
    }
    auto inside = [&](uint64_t key) -> bool { return !f && key != KEY_PAD && (double)ord2f((uint32_t)(key >> 32)) <= lim; };
    if (blockIdx.y == 0) { // (uniform) the query's flag, and its window over all slices for the search's largest
        if (tid == 0) {
            fail[q] = f ? 1u : 0u;
            s_cnt = 0;
        }
        __syncthreads();
        int cnt = 0;
        for (int j = tid; j < kp; j += 256) cnt += inside(a[j]) ? 1 : 0;
        cnt = wave_sum(cnt);
        if ((tid & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
        __syncthreads();
        if (tid == 0 && !f) atomicMax(&sstat[0], (uint32_t)s_cnt);
    }
    // this slice's rows (uniform)
    uint32_t mask = 0;
    uint64_t mykey = KEY_PAD; // lane r < RS16_ROWS of every wave: key j0 + r
#pragma unroll
    for (int r = 0; r < RS16_ROWS; r++) {
        const uint64_t key = j0 + r < kp ? a[j0 + r] : KEY_PAD;
        if (inside(key)) mask |= 1u << r;
        if (r == (tid & 63)) mykey = key;
    }
    if (!mask) { // (uniform) nothing of the window in this slice
        if (tid < RS16_ROWS && j0 + tid < kp) ok[(size_t)q * kp + j0 + tid] = KEY_PAD;
        return;
    }
    const bool mine = tid < RS16_ROWS && ((mask >> tid) & 1u);
    const int c = tid * 4;
    float acc = 0.0f;
    for (int s0 = 0; s0 < dp; s0 += RS16_SLAB) {
        const int sl = dp - s0 < RS16_SLAB ? dp - s0 : RS16_SLAB; // (a multiple of 32, like dp)
        if (s0) __syncthreads(); // (the chains have read the slab before)
        if (c < sl) {
            f32x4 v[RS16_ROWS];
#pragma unroll
            for (int r = 0; r < RS16_ROWS; r++)
                if ((mask >> r) & 1u) { // (uniform)
                    const uint32_t row = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)mykey, r) - id_base;
                    v[r] = *(const f32x4 *)(xb + (size_t)row * dp + s0 + c);
                }
            *(f32x4 *)(sq + c) = *(const f32x4 *)(xq + (size_t)q * dp + s0 + c);
#pragma unroll
            for (int r = 0; r < RS16_ROWS; r++)
                if ((mask >> r) & 1u) *(f32x4 *)(sy + r * pitch + c) = v[r];
        }
        __syncthreads();
        if (mine) {
            const float *y = sy + tid * pitch;
#pragma unroll 4
            for (int k0 = 0; k0 < sl; k0 += 8) {
                const f32x4 q0 = *(const f32x4 *)(sq + k0), q1 = *(const f32x4 *)(sq + k0 + 4);
                const f32x4 y0 = *(const f32x4 *)(y + k0), y1 = *(const f32x4 *)(y + k0 + 4);
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    acc = __builtin_fmaf(q0[m], y0[m], acc);
                    acc = __builtin_fmaf(q1[m], y1[m], acc);
                }
            }
        }
    }
    if (tid < RS16_ROWS && j0 + tid < kp) {
        uint64_t out = KEY_PAD;
        if (mine) {
            const float v = -acc + 0.0f;
            out = ((uint64_t)f2ord(v) << 32) | (uint32_t)mykey;
        }
        ok[(size_t)q * kp + j0 + tid] = out;
    }
}
