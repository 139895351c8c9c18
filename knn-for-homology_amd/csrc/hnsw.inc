// hnsw.inc -- faiss.IndexHNSWFlat on MI355X (included by knn355_lib.hip).
//
// Reference call site: pfam/proteins_search.py:27-31,35-37,49
//   index = faiss.IndexHNSWFlat(d, 42, faiss.METRIC_INNER_PRODUCT); index.hnsw.efSearch = 256
//   index.train(x); index.add(x); index.search(x, 1000)
// FAISS 1.7.2 (impl/HNSW.cpp) is not in the reference tree; the published algorithm
// (Malkov & Yashunin, as FAISS implements it) is restated: exponential level assignment
// with multiplier 1/ln(M), M links per upper level and 2M at level 0, efConstruction = 40,
// greedy descent on the upper levels, best-first beam search with ef = max(efSearch, k)
// at level 0, neighbour selection by the "closer to the centre than to any kept
// neighbour" heuristic (shrink_neighbor_list), inner product handled as negated distance,
// missing results reported as id -1.
//
// Division of labour (north star): the GRAPH lives and is walked on the host; every
// distance is computed on the GPU, in the same fp32 chain order as the flat scan:
//   pair_v_kernel       batches of (query slot, row) pairs from many walkers in lock step
//   gram_shrink_kernel  one workgroup per neighbour list to prune: MFMA Gram matrix of the
//                       gathered rows in LDS + the selection heuristic, returns kept ids
// Many queries / insertions advance together, one expansion per round, so each launch
// carries 10^4..10^6 pairs (SURVEY.md 7.3 H4).  Construction is batch-synchronous and
// therefore deterministic (FAISS's OpenMP construction is not).
// Since round 2 the level-0 walk of searches and insertions is a device kernel (hnsw_beam_kernel:
// one wave per query over a device mirror of the level-0 lists), since round 4 a batch's level-0
// links are made on the device as well (hnsw_level0_links_device) and that mirror is the master
// copy of level 0; the host graph keeps the levels above 0 and follows level 0 on demand.

#include <omp.h>
#include <sched.h>
#include <hipcub/hipcub.hpp>
#include <random>
#include <queue>

#define HNSW_EMPTY 0xFFFFFFFFu
#define SHRINK_MAX_MEMBERS 128

// v(query slot a, row b): smaller is better.  IP: -dot, L2: the sum of squared differences (FAISS's HNSW distance
// computer, fvec_L2sqr [ext]; one chain in the dot product's order -- the flat search's small-batch formula)
__global__ void pair_v_kernel(const float *__restrict__ xa, const float *__restrict__ an, const float *__restrict__ xb,
                              const float *__restrict__ bn, int dp, int metric, int64_t npairs,
                              const uint32_t *__restrict__ pa, const uint32_t *__restrict__ pb,
                              float *__restrict__ out)
{
    int64_t pidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pidx >= npairs) return;
    const float *q = xa + (size_t)pa[pidx] * dp;
    const float *y = xb + (size_t)pb[pidx] * dp;
    const bool l2 = metric == KNN_METRIC_L2;
    float acc = 0.0f;
    for (int k0 = 0; k0 < dp; k0 += 8) {
        f32x4 q0 = *(const f32x4 *)(q + k0), q1 = *(const f32x4 *)(q + k0 + 4);
        f32x4 y0 = *(const f32x4 *)(y + k0), y1 = *(const f32x4 *)(y + k0 + 4);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            if (l2) {
                const float t0 = q0[m] - y0[m], t1 = q1[m] - y1[m];
                acc = __builtin_fmaf(t0, t0, acc);
                acc = __builtin_fmaf(t1, t1, acc);
            } else {
                acc = __builtin_fmaf(q0[m], y0[m], acc);
                acc = __builtin_fmaf(q1[m], y1[m], acc);
            }
        }
    }
    out[pidx] = (l2 ? acc : -acc) + 0.0f;
}

// One workgroup per group.  members[off .. off+n): member 0 is the centre, 1..n-1 the
// candidates (n <= 128).  Computes every pairwise v among the members with MFMA (rows
// gathered by id), then keeps candidates in order of increasing v(centre, cand) unless some
// already kept neighbour is closer to the candidate than the centre is.  out_ids[g][0..max_out)
struct ShrinkParams {
    const float *xb;
    const float *yn;
    int dp, metric;
    const int32_t *group_off; // [ngroups + 1] ([ngroups] when group_cnt is given)
    const int32_t *group_cnt; // [ngroups] members of each group; NULL: group_off[g + 1] - group_off[g]
    const uint32_t *members;
    const int32_t *max_out;   // [ngroups]
    uint32_t *out_ids;        // [ngroups][out_stride]
    float *out_d;             // [ngroups][out_stride] v(centre, kept)
    int32_t *out_n;           // [ngroups]
    int out_stride;
    const int32_t *ngroups;   // device-side group count (groups composed on the device: the grid is an upper bound); NULL: the grid
};

// The Gram matrix is symmetric: only the tile pairs (a <= b) of 32 x 32 tiles are multiplied, shared out to the four waves
// ([tiles per side][wave][slot] = a << 4 | b, 0xFF: none), and every value is written to both of its places -- dot(i, j) and
// dot(j, i) are the same chain of the same products.  A group of 66..96 members (a full level-0 list of 64 and a few new
// links: the typical pruning group) costs 2 tile products per wave instead of the 4 of the full 128 x 128 matrix.
__constant__ uint8_t SHRINK_PAIRS[5][4][3] = {
    {{0xFF, 0xFF, 0xFF}, {0xFF, 0xFF, 0xFF}, {0xFF, 0xFF, 0xFF}, {0xFF, 0xFF, 0xFF}},
    {{0x00, 0xFF, 0xFF}, {0xFF, 0xFF, 0xFF}, {0xFF, 0xFF, 0xFF}, {0xFF, 0xFF, 0xFF}},
    {{0x00, 0xFF, 0xFF}, {0x01, 0xFF, 0xFF}, {0x11, 0xFF, 0xFF}, {0xFF, 0xFF, 0xFF}},
    {{0x00, 0x11, 0xFF}, {0x01, 0x22, 0xFF}, {0x02, 0xFF, 0xFF}, {0x12, 0xFF, 0xFF}},
    {{0x00, 0x11, 0x22}, {0x01, 0x02, 0x03}, {0x12, 0x13, 0xFF}, {0x23, 0x33, 0xFF}},
};

// NR: rows a group may have in this launch (64, 96 or 128: the LDS a workgroup takes); a group stages and multiplies only
// the 32-row tiles its members fill (the last one padded with member 0)
template <int NR>
__global__ __launch_bounds__(256) void gram_shrink_kernel(ShrinkParams p)
{
    static_assert(NR == 64 || NR == 96 || NR == 128, "rows per group");
    constexpr int NSI = NR / 32;           // staging instructions per wave and K step at most (8 rows each)
    constexpr int MAXP = NR == 128 ? 3 : (NR == 96 ? 2 : 1); // tile pairs per wave at most
    constexpr int STAGE_BYTES = NR * 128;
    constexpr int GLD = NR + 1;
    constexpr int MAIN_BYTES = 2 * STAGE_BYTES > NR * GLD * 4 ? 2 * STAGE_BYTES : NR * GLD * 4;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char *stage0 = smem, *stage1 = smem + STAGE_BYTES;
    float *gram = (float *)smem;                        // [NR][NR+1] v values -- over the staging buffers, behind the K loop
    uint32_t *s_ids = (uint32_t *)(smem + MAIN_BYTES);  // [NR]
    float *s_key = (float *)(s_ids + NR);               // [NR] v(centre, i)
    int *s_ord = (int *)(s_key + NR);                   // [NR] candidate order
    int *s_out = s_ord + NR;                            // [NR] kept member indices

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lh = lane >> 5;
    const int g = blockIdx.x;
    if (p.ngroups && g >= *p.ngroups) return;
    const int off = p.group_off[g];
    const int n = min(p.group_cnt ? p.group_cnt[g] : p.group_off[g + 1] - off, NR);
    const int nt = max(1, (n + 31) >> 5); // 32-row tiles in use
    for (int i = tid; i < NR; i += 256) {
        s_ids[i] = p.members[off + (i < n ? i : 0)];
        s_ord[i] = 0; // "centre": skipped by the heuristic
    }
    __syncthreads();
    int pa[MAXP], pb[MAXP]; // this wave's tile pairs (-1: none)
#pragma unroll
    for (int q = 0; q < MAXP; q++) {
        const int e = __builtin_amdgcn_readfirstlane((int)SHRINK_PAIRS[nt][wave][q]);
        pa[q] = e == 0xFF ? -1 : e >> 4;
        pb[q] = e == 0xFF ? -1 : e & 15;
    }

    // staging: 32 nt rows x 128 B per K step = 4 nt instructions of 8 rows, nt per wave
    const float *srcp[NSI];
    int lds_off[NSI];
#pragma unroll
    for (int nn = 0; nn < NSI; nn++) {
        const int ii = wave + 4 * nn;
        const int row_local = 8 * ii + (lane >> 3);
        const int sp = lane & 7;
        const int s = sp ^ ((row_local >> 1) & 7);
        srcp[nn] = p.xb + (size_t)s_ids[row_local] * p.dp + 4 * s;
        lds_off[nn] = ii * 1024;
    }
    f32x16 acc[MAXP];
#pragma unroll
    for (int q = 0; q < MAXP; q++)
#pragma unroll
        for (int r = 0; r < 16; r++) acc[q][r] = 0.0f;
    const int KT = p.dp / 32;
    const int swz = (li >> 1) & 7;
#pragma unroll
    for (int nn = 0; nn < NSI; nn++)
        if (nn < nt)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)srcp[nn],
                                             (__attribute__((address_space(3))) void *)(stage0 + lds_off[nn]), 16, 0, 0);
    for (int kt = 0; kt < KT; kt++) {
        char *cur = (kt & 1) ? stage1 : stage0;
        char *nxt = (kt & 1) ? stage0 : stage1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // (this wave's staging instructions have landed -- explicit: see flat_scan_kernel's K loop)
        __syncthreads();
        if (kt + 1 < KT) {
#pragma unroll
            for (int nn = 0; nn < NSI; nn++)
                if (nn < nt)
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(srcp[nn] + (kt + 1) * 32),
                                                     (__attribute__((address_space(3))) void *)(nxt + lds_off[nn]), 16, 0, 0);
        }
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int slot = ((2 * t + lh) ^ swz) * 16;
#pragma unroll
            for (int q = 0; q < MAXP; q++) {
                if (pa[q] >= 0) {
                    const f32x4 af = *(const f32x4 *)(cur + (pa[q] * 32 + li) * 128 + slot);
                    const f32x4 bf = *(const f32x4 *)(cur + (pb[q] * 32 + li) * 128 + slot);
#pragma unroll
                    for (int m = 0; m < 4; m++) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[m], bf[m], acc[q], 0, 0, 0);
                }
            }
        }
    }
    __syncthreads(); // (every wave has read its last fragments: the staging buffers become the matrix)
    // accumulators -> v values in LDS: A rows are the MFMA "row" index, B rows the lane; both places of every value
#pragma unroll
    for (int q = 0; q < MAXP; q++) {
        if (pa[q] < 0) continue;
        const int j = pb[q] * 32 + li;
        const float nj = p.metric == KNN_METRIC_L2 ? p.yn[s_ids[j]] : 0.0f;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int i = pa[q] * 32 + 4 * lh + (r & 3) + 8 * (r >> 2);
            float v;
            if (p.metric == KNN_METRIC_L2) {
                v = __builtin_fmaf(-2.0f, acc[q][r], p.yn[s_ids[i]] + nj);
                v = v < 0.0f ? 0.0f : v;
            } else {
                v = -acc[q][r];
            }
            gram[i * GLD + j] = v + 0.0f;
            if (pa[q] != pb[q]) gram[j * GLD + i] = v + 0.0f;
        }
    }
    __syncthreads();
    // wave 0: order candidates by (v(centre, c), id), then run the heuristic
    if (wave == 0) {
        // rank of each candidate by counting (n <= 128: two candidates per lane)
        for (int c = 1 + lane; c < n; c += 64) s_key[c] = gram[c * GLD + 0]; // dot(c, centre): same chain as dot(centre, c)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        for (int c = 1 + lane; c < n; c += 64) {
            const float kc = s_key[c];
            const uint32_t idc = s_ids[c];
            int rank = 0;
            for (int o = 1; o < n; o++) {
                const float ko = s_key[o];
                rank += (ko < kc || (ko == kc && s_ids[o] < idc)) ? 1 : 0;
            }
            s_ord[rank] = c;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const int maxo = p.max_out[g];
        int nout = 0;
        for (int t = 0; t < n - 1 && nout < maxo; t++) {
            const int c = s_ord[t];
            const float dc = s_key[c];
            bool bad = false;
            for (int o = lane; o < nout; o += 64) bad |= gram[c * GLD + s_out[o]] < dc;
            // duplicates of an already kept row (same id listed twice) are dropped as well
            for (int o = lane; o < nout; o += 64) bad |= s_ids[s_out[o]] == s_ids[c];
            if (!__any(bad) && s_ids[c] != s_ids[0]) {
                if (lane == 0) s_out[nout] = c;
                nout++;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
        }
        for (int o = lane; o < nout; o += 64) {
            p.out_ids[(size_t)g * p.out_stride + o] = s_ids[s_out[o]];
            p.out_d[(size_t)g * p.out_stride + o] = s_key[s_out[o]];
        }
        if (lane == 0) p.out_n[g] = nout;
    }
}

// ---------------------------------------------------------------------------
// Level-0 beam search on the device: one WAVE per query (a persistent wave takes queries
// slot, slot + nslots, ...).  The beam W (ef keys, unsorted, in LDS) holds every candidate the
// walk still cares about; an entry's low bit says "expanded".  Per step: the best unexpanded
// entry is expanded -- its neighbour list is one coalesced 256-B row --, neighbours are
// tested against the walker's visited bitmap (global memory, one atomicOr per lane), the
// fresh ones are scored and replace the worst entries of W.  The walk ends when W has no
// unexpanded entry left (FAISS's stop rule, "closest candidate is farther than the farthest
// result", in beam form: every candidate lives in W).
// Scoring reads each 4-KB row with four fully coalesced wave loads (8 rows = 32 KB in flight
// per wave) and sums lane partials -- fp32, but not the flat scan's summation order, so the
// walk's decisions may differ from an exact walk in the last bit.  The result does not: the
// beam's ef rows are re-scored with the exact chain (pair_v_kernel) and the final selection
// sorts those keys, so every returned distance is bit-identical to the flat search's.
// ---------------------------------------------------------------------------
struct BeamParams {
    const float *xb, *yn;   // database rows [n][dp], squared norms
    const uint16_t *xb16;   // B16 builds: bf16 copies of the rows [n][dp]
    const float *xq, *qn;   // queries [nq][dp] (zero padded), squared norms (L2)
    const uint32_t *nbr0;   // [n][M0] level-0 neighbour lists, HNSW_EMPTY = no link
    const uint32_t *entry;  // [nq][nentry] nodes the level-0 walk starts from (HNSW_EMPTY = unused slot)
    uint32_t *visited;      // [nslots][vis_words] bitmaps
    uint32_t *touched;      // lazy clearing (huge graphs): [nslots][tcap] bitmap words a walk has set; null: the walker clears its whole bitmap
    int tcap;
    uint32_t *out_ids;      // [nq][ef] the beam's rows (HNSW_EMPTY padded)
    unsigned long long *stats; // [0] rows scored, [1] expansions
    int64_t nq, n, vis_words;
    int dp, metric, M0, ef, nentry;
    int expand2;            // expand the two best unexpanded entries per step
    int keep, kmin;         // rows handed on per query: all ef of the beam (keep == ef), or its best kmin..keep by the walk's own scores
};

__device__ __forceinline__ float wave_sum_f32(float x)
{
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0xB1, 0xF, 0xF, false));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x4E, 0xF, 0xF, false));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x141, 0xF, 0xF, false));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x140, 0xF, 0xF, false));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x142, 0xA, 0xF, false));
    x += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x143, 0xC, 0xF, false));
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), 63));
}

// NCH: 16-byte chunks of a row per lane (dp <= 256 * NCH); RB: rows in flight per wave while scoring (8: 32 KB per wave
// at d = 1024, ~190 registers, two workgroups per CU; 4: half the registers, four workgroups per CU -- the walk is a
// chain of dependent latencies (neighbour list, visited bits, rows, insertion), twice the walkers hide twice as much)
// B16: the walk scores bf16 copies of the rows (half the bytes of the 4-KB gathers; NCH then counts 16-byte chunks of
// 8 values).  The walk was approximate before (lane-partial sums); what is RETURNED is re-scored from the fp32 rows.
template <int NCH, int RB, bool B16 = false>
__global__ __launch_bounds__(256, RB == 8 ? 2 : 4) void hnsw_beam_kernel(BeamParams p)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int EF = p.ef;
    const int R = (EF + 63) >> 6; // beam entries per lane
    uint64_t *W = (uint64_t *)smem + (size_t)wave * (R * 64);         // [R * 64] beam (KEY_PAD = free)
    uint32_t *fresh = (uint32_t *)((uint64_t *)smem + (size_t)4 * (R * 64)) + wave * 64; // [64] ids to score
    const int64_t nslots = (int64_t)gridDim.x * 4;
    const int64_t slot = (int64_t)blockIdx.x * 4 + wave;
    uint32_t *vis = p.visited + (size_t)slot * p.vis_words;
    const int nchunks = B16 ? p.dp >> 3 : p.dp >> 2; // 16-byte chunks per row
    unsigned long long n_rows = 0, n_exp = 0;

    for (int64_t q = slot; q < p.nq; q += nslots) {
        // this walker's bitmap and beam start empty.  Ten million rows are 1.25 MB of bitmap per walker, a walk sets a
        // few thousand bits of it: with p.touched the walker remembers the words it touched and clears those when it
        // is done (the bitmaps are zero when the kernel starts and again when it ends)
        if (!p.touched) {
            for (int64_t i = 4 * (int64_t)lane; i < p.vis_words; i += 256) *(uint4 *)(vis + i) = make_uint4(0u, 0u, 0u, 0u); // (vis_words % 4 == 0)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the clearing stores have reached L2 before the first atomicOr
        }
        uint32_t *tl = p.touched ? p.touched + (size_t)slot * p.tcap : nullptr;
        int tcnt = 0; // words remembered (uniform); > tcap: the list overflowed, everything is cleared at the end
        for (int r = 0; r < R; r++) W[r * 64 + lane] = KEY_PAD;
        // the query, in the layout of a coalesced row load: chunk c = i * 64 + lane
        constexpr int QW = B16 ? 2 : 1; // query registers (of four values) per chunk
        f32x4 qv[NCH * QW];
#pragma unroll
        for (int i = 0; i < NCH; i++) {
            const int c = i * 64 + lane;
#pragma unroll
            for (int w = 0; w < QW; w++)
                qv[i * QW + w] = c < nchunks ? *(const f32x4 *)(p.xq + (size_t)q * p.dp + 4 * (c * QW + w)) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        const float qn = p.metric == KNN_METRIC_L2 ? p.qn[q] : 0.0f;
        int wcount = 0; // filled beam entries (uniform)
        uint64_t wmax = 0; // worst key of the full beam (uniform; valid once wcount == EF)
        // scores `m` rows listed in fresh[0..m) and merges them into the beam
        auto score_and_insert = [&](int m) {
            n_rows += (unsigned long long)m;
            uint64_t mykey = KEY_PAD; // lane j < m ends up with the key of fresh[j]
            for (int b0 = 0; b0 < m; b0 += RB) {
                f32x4 v[RB][NCH];
#pragma unroll
                for (int j = 0; j < RB; j++) {
                    const uint32_t row = fresh[min(b0 + j, m - 1)]; // (uniform; the tail repeats the last row)
                    const float *src = B16 ? (const float *)(p.xb16 + (size_t)row * p.dp) : p.xb + (size_t)row * p.dp;
#pragma unroll
                    for (int i = 0; i < NCH; i++) {
                        const int c = i * 64 + lane;
                        v[j][i] = c < nchunks ? *(gptr4)(src + 4 * c) : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
                }
#pragma unroll
                for (int j = 0; j < RB; j++) {
                    float part = 0.0f;
#pragma unroll
                    for (int i = 0; i < NCH; i++)
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            if constexpr (B16) {
                                const float fe = v[j][i][e]; // (bit_cast straight from the vector element compiles to element 0 for every e)
                                const uint32_t w2 = __float_as_uint(fe);
                                part = __builtin_fmaf(__builtin_bit_cast(float, w2 << 16), qv[2 * i + (e >> 1)][(2 * e) & 3], part);
                                part = __builtin_fmaf(__builtin_bit_cast(float, w2 & 0xFFFF0000u), qv[2 * i + (e >> 1)][(2 * e + 1) & 3], part);
                            } else {
                                part = __builtin_fmaf(v[j][i][e], qv[i][e], part);
                            }
                        }
                    const float dot = wave_sum_f32(part);
                    if (b0 + j < m) {
                        const uint32_t row = fresh[b0 + j];
                        float val;
                        if (p.metric == KNN_METRIC_L2) {
                            val = __builtin_fmaf(-2.0f, dot, qn + p.yn[row]);
                            val = val < 0.0f ? 0.0f : val;
                        } else {
                            val = -dot;
                        }
                        val = val + 0.0f;
                        if (lane == b0 + j) mykey = ((uint64_t)f2ord(val) << 32) | ((uint64_t)row << 1);
                    }
                }
            }
            // appends while the beam has room, then replaces the worst entry as long as a new key beats it.  `wmax`, the
            // worst key of a full beam, is carried along (it only changes when an entry is replaced, and the pass that
            // replaces it also finds the next one); new keys that do not beat it are dropped in one compare -- at the
            // end of a walk that is nearly all of them, and this loop is what the walk's time goes into.
            if (wcount >= EF && mykey != KEY_PAD && mykey >= (wmax & ~1ull)) mykey = KEY_PAD;
            while (true) {
                const uint64_t bestnew = wave_min_u64(mykey);
                if (bestnew == KEY_PAD) break;
                if (wcount < EF) {
                    if (mykey == bestnew) {
                        W[wcount] = mykey;
                        mykey = KEY_PAD;
                    }
                    wcount++;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    if (wcount == EF) { // the beam is full from here on: its worst key
                        uint64_t m2 = 0;
                        for (int r = 0; r < R; r++) {
                            const uint64_t e = W[r * 64 + lane];
                            if (r * 64 + lane < EF && e > m2) m2 = e;
                        }
                        wmax = wave_max_u64(m2);
                        if (mykey != KEY_PAD && mykey >= (wmax & ~1ull)) mykey = KEY_PAD;
                    }
                    continue;
                }
                if (bestnew >= (wmax & ~1ull)) break; // (compare without the expanded bit)
                uint64_t m2 = 0;
                for (int r = 0; r < R; r++) {
                    if (r * 64 + lane < EF) {
                        uint64_t e = W[r * 64 + lane];
                        if (e == wmax) {
                            e = bestnew;
                            W[r * 64 + lane] = e;
                        }
                        if (e > m2) m2 = e;
                    }
                }
                if (mykey == bestnew) mykey = KEY_PAD;
                wmax = wave_max_u64(m2);
                if (mykey != KEY_PAD && mykey >= (wmax & ~1ull)) mykey = KEY_PAD;
                __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            }
        };
        // entry points (distinct nodes)
        {
            uint32_t e0 = HNSW_EMPTY;
            if (lane < p.nentry) e0 = p.entry[(size_t)q * p.nentry + lane];
            const bool ok = e0 != HNSW_EMPTY;
            if (ok) atomicOr(&vis[e0 >> 5], 1u << (e0 & 31));
            const uint64_t mask = __ballot(ok);
            if (tl) {
                if (ok) tl[__popcll(mask & ((1ull << lane) - 1ull))] = e0 >> 5; // (nentry <= 64 <= tcap)
                tcnt = __popcll(mask);
            }
            if (ok) fresh[__popcll(mask & ((1ull << lane) - 1ull))] = e0;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            score_and_insert(__popcll(mask));
        }
        while (true) {
            // the TWO best unexpanded entries are expanded together: their neighbour lists, visited tests and row
            // gathers overlap instead of forming two rounds of the same chain of dependent latencies (the second one
            // would nearly always have been next; when the first one's neighbours push it out of the beam, a few rows
            // were scored for nothing)
            uint64_t best = KEY_PAD, second = KEY_PAD;
            for (int r = 0; r < R; r++) {
                const uint64_t e = W[r * 64 + lane];
                if (!(e & 1ull)) {
                    if (e < best) {
                        second = best;
                        best = e;
                    } else if (e < second) {
                        second = e;
                    }
                }
            }
            const uint64_t b1 = wave_min_u64(best);
            if (b1 == KEY_PAD) break;
            const uint64_t b2 = p.expand2 ? wave_min_u64(best == b1 ? second : best) : KEY_PAD; // (keys are distinct)
            for (int r = 0; r < R; r++) {
                const uint64_t e = W[r * 64 + lane];
                if (e == b1 || (e == b2 && b2 != KEY_PAD)) W[r * 64 + lane] = e | 1ull;
            }
            if (b1 == wmax || (b2 == wmax && b2 != KEY_PAD)) wmax |= 1ull; // (the carried worst key follows its entry's expanded bit)
            const bool two = b2 != KEY_PAD;
            n_exp += two ? 2 : 1;
            const uint32_t nodeA = (uint32_t)(b1 & 0xFFFFFFFFull) >> 1, nodeB = (uint32_t)(b2 & 0xFFFFFFFFull) >> 1;
            for (int j0 = 0; j0 < p.M0; j0 += 64) {
                uint32_t nbA = HNSW_EMPTY, nbB = HNSW_EMPTY;
                if (j0 + lane < p.M0) {
                    nbA = p.nbr0[(size_t)nodeA * p.M0 + j0 + lane];
                    if (two) nbB = p.nbr0[(size_t)nodeB * p.M0 + j0 + lane];
                }
                bool newA = false, newB = false;
                uint32_t oldA = 0xFFFFFFFFu, oldB = 0xFFFFFFFFu;
                const uint32_t bitA = 1u << (nbA & 31), bitB = 1u << (nbB & 31);
                if (nbA != HNSW_EMPTY) oldA = atomicOr(&vis[nbA >> 5], bitA);
                if (nbB != HNSW_EMPTY) oldB = atomicOr(&vis[nbB >> 5], bitB);
                if (tl) { // (only words this walk turned from zero need remembering: a word already non-zero is on the list)
                    const bool recA = nbA != HNSW_EMPTY && oldA == 0u, recB = nbB != HNSW_EMPTY && oldB == 0u;
                    const uint64_t ra = __ballot(recA), rb = __ballot(recB);
                    const uint64_t lower = (1ull << lane) - 1ull;
                    const int ia = tcnt + __popcll(ra & lower), ib = tcnt + __popcll(ra) + __popcll(rb & lower);
                    if (recA && ia < p.tcap) tl[ia] = nbA >> 5;
                    if (recB && ib < p.tcap) tl[ib] = nbB >> 5;
                    tcnt += __popcll(ra) + __popcll(rb);
                }
                newA = nbA != HNSW_EMPTY && (oldA & bitA) == 0u;
                newB = nbB != HNSW_EMPTY && (oldB & bitB) == 0u;
                const uint64_t maskA = __ballot(newA), maskB = __ballot(newB);
                const int mA = __popcll(maskA), mB = __popcll(maskB);
                if (mA + mB == 0) continue;
                const uint64_t below = (1ull << lane) - 1ull;
                if (mA + mB <= 64) {
                    if (newA) fresh[__popcll(maskA & below)] = nbA;
                    if (newB) fresh[mA + __popcll(maskB & below)] = nbB;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    score_and_insert(mA + mB);
                } else {
                    if (newA) fresh[__popcll(maskA & below)] = nbA;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    score_and_insert(mA);
                    if (newB) fresh[__popcll(maskB & below)] = nbB;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                    score_and_insert(mB);
                }
            }
        }
        // the beam's rows, in any order (exact scores and the final order come next).  A caller that wants k << ef
        // results gets the best kmin..keep rows by the walk's scores only: those differ from the exact chain in the
        // last bits, the slack (k/8 rows at least) is there for that, and re-scoring is a 4-KB gather per row.
        if (p.keep < EF && wcount > p.keep) {
            // smallest score word X with at least kmin keys below it (bisection, keys stay in LDS), then the keys below
            // X go out, at most `keep` of them (more only if dozens of rows tie on the score word)
            uint32_t lo_x = 0u, hi_x = 0xFFFFFFFFu; // count(< lo_x) < kmin <= count(< hi_x)
            while (hi_x - lo_x > 1u) {
                const uint32_t X = lo_x + ((hi_x - lo_x) >> 1);
                int c = 0;
                for (int r = 0; r < R; r++) c += (uint32_t)(W[r * 64 + lane] >> 32) < X ? 1 : 0;
                c = wave_sum(c);
                if (c >= p.kmin) hi_x = X;
                else lo_x = X;
            }
            int base = 0;
            for (int r = 0; r < R; r++) {
                const uint64_t e = W[r * 64 + lane];
                const bool take = (uint32_t)(e >> 32) < hi_x;
                const uint64_t mask = __ballot(take);
                const int at = base + __popcll(mask & ((1ull << lane) - 1ull));
                if (take && at < p.keep) p.out_ids[(size_t)q * p.keep + at] = (uint32_t)(e & 0xFFFFFFFFull) >> 1;
                base += __popcll(mask);
            }
            for (int i = min(base, p.keep) + lane; i < p.keep; i += 64) p.out_ids[(size_t)q * p.keep + i] = HNSW_EMPTY;
        } else {
            for (int i = lane; i < p.keep; i += 64) {
                const uint64_t e = i < R * 64 ? W[i] : KEY_PAD;
                p.out_ids[(size_t)q * p.keep + i] = e == KEY_PAD ? HNSW_EMPTY : ((uint32_t)(e & 0xFFFFFFFFull) >> 1);
            }
        }
        if (tl) {
            if (tcnt <= p.tcap) {
                for (int i = lane; i < tcnt; i += 64) vis[tl[i]] = 0u;
            } else {
                for (int64_t i = 4 * (int64_t)lane; i < p.vis_words; i += 256) *(uint4 *)(vis + i) = make_uint4(0u, 0u, 0u, 0u);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // cleared before the next walk's first atomicOr
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (p.stats && lane == 0) {
        atomicAdd(&p.stats[0], n_rows);
        atomicAdd(&p.stats[1], n_exp);
    }
}

// exact keys of the beam's rows: key[q][i] = (order-preserving bits of v(q, ids[q][i])) << 32 | id, the flat scan's
// fma chain (one lane per pair); empty slots -> KEY_PAD
__global__ void beam_keys_kernel(const float *__restrict__ xq, const float *__restrict__ qn, const float *__restrict__ xb,
                                 const float *__restrict__ yn, int dp, int metric, int64_t nq, int ef,
                                 const uint32_t *__restrict__ ids, uint64_t *__restrict__ keys)
{
    const int64_t pidx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pidx >= nq * ef) return;
    const uint32_t row = ids[pidx];
    if (row == HNSW_EMPTY) {
        keys[pidx] = KEY_PAD;
        return;
    }
    const int64_t qi = pidx / ef;
    const float *a = xq + (size_t)qi * dp;
    const float *y = xb + (size_t)row * dp;
    // squared L2: the sum of squared differences, as FAISS's HNSW distance computer (fvec_L2sqr [ext]) and the flat
    // search's small-batch formula -- one chain, acc = fma(t, t, acc), t = q[k] - y[k], k in the dot product's order
    const bool l2 = metric == KNN_METRIC_L2;
    float acc = 0.0f;
    for (int k0 = 0; k0 < dp; k0 += 8) {
        f32x4 q0 = *(const f32x4 *)(a + k0), q1 = *(const f32x4 *)(a + k0 + 4);
        f32x4 y0 = *(const f32x4 *)(y + k0), y1 = *(const f32x4 *)(y + k0 + 4);
#pragma unroll
        for (int m = 0; m < 4; m++) {
            if (l2) {
                const float t0 = q0[m] - y0[m], t1 = q1[m] - y1[m];
                acc = __builtin_fmaf(t0, t0, acc);
                acc = __builtin_fmaf(t1, t1, acc);
            } else {
                acc = __builtin_fmaf(q0[m], y0[m], acc);
                acc = __builtin_fmaf(q1[m], y1[m], acc);
            }
        }
    }
    const float v = l2 ? acc : -acc;
    keys[pidx] = ((uint64_t)f2ord(v + 0.0f) << 32) | row;
}

// The same keys with coalesced row reads: a wave takes 64 pairs; per block of 64 values it copies the block of each of
// its 64 rows into LDS with one 256-byte wave load per row, then every lane runs the exact chain over ITS row's block
// from LDS (the chain of a pair is sequential, so a pair stays with one lane -- only the loads are shared).  One lane
// reading its own 4-KB row 16 bytes at a time got 1.3 TB/s out of the gathers.
__global__ __launch_bounds__(256) void beam_keys_lds_kernel(const float *__restrict__ xq, const float *__restrict__ qn,
                                                            const float *__restrict__ xb, const float *__restrict__ yn, int dp,
                                                            int metric, int64_t nq, int ef, const uint32_t *__restrict__ ids,
                                                            uint64_t *__restrict__ keys)
{
    constexpr int STR = 65; // floats per staged row block (+1: lane r reads row r, conflict-free)
    __shared__ float sblk[4][64 * STR];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *sb = sblk[wave];
    const int64_t total = nq * ef;
    const int64_t p0 = ((int64_t)blockIdx.x * 4 + wave) * 64; // (wave-uniform)
    if (p0 >= total) return;
    const int64_t pidx = p0 + lane;
    const bool have = pidx < total;
    const uint32_t row = have ? ids[pidx] : HNSW_EMPTY;
    const bool valid = row != HNSW_EMPTY;
    const int64_t qi = have ? pidx / ef : 0;
    const float *a = xq + (size_t)qi * dp;
    const bool l2 = metric == KNN_METRIC_L2;
    float acc = 0.0f;
    for (int k0 = 0; k0 < dp; k0 += 64) {
        const int w = min(64, dp - k0); // (dp is a multiple of 32)
        // stage: row rr's block, one wave load each (rows of empty slots read row 0: harmless)
        // (sixteen loads in flight, then their sixteen LDS stores)
        const int lw = lane < w ? lane : 0;
#pragma unroll
        for (int r0 = 0; r0 < 64; r0 += 16) {
            float t[16];
#pragma unroll
            for (int u = 0; u < 16; u++) {
                const uint32_t r2 = (uint32_t)__builtin_amdgcn_readlane((int)(valid ? row : 0u), r0 + u);
                t[u] = xb[(size_t)r2 * dp + k0 + lw];
            }
#pragma unroll
            for (int u = 0; u < 16; u++) sb[(r0 + u) * STR + lane] = t[u];
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const float *y = sb + lane * STR;
        for (int j = 0; j < w; j += 8) {
            const f32x4 q0 = *(const f32x4 *)(a + k0 + j), q1 = *(const f32x4 *)(a + k0 + j + 4);
#pragma unroll
            for (int m = 0; m < 4; m++) {
                if (l2) { // (the sum of squared differences: see beam_keys_kernel)
                    const float t0 = q0[m] - y[j + m], t1 = q1[m] - y[j + 4 + m];
                    acc = __builtin_fmaf(t0, t0, acc);
                    acc = __builtin_fmaf(t1, t1, acc);
                } else {
                    acc = __builtin_fmaf(q0[m], y[j + m], acc);
                    acc = __builtin_fmaf(q1[m], y[j + 4 + m], acc);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if (!have) return;
    if (!valid) {
        keys[pidx] = KEY_PAD;
        return;
    }
    const float v = l2 ? acc : -acc;
    keys[pidx] = ((uint64_t)f2ord(v + 0.0f) << 32) | row;
}

// ===========================================================================
// host side
// ===========================================================================
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need)
    {
        if (need <= bytes) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        size_t want = need + need / 2;
        if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) return -1;
        bytes = want;
        return 0;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
};

struct HnswGraph {
    int M = 32;
    std::vector<double> assign_probas;
    std::vector<int> cum_nb; // cum_nb[l] = slots of levels < l
    std::vector<int> levels; // top level of node i
    std::vector<size_t> offsets;
    std::vector<uint32_t> nbrs;
    std::vector<uint8_t> cnt0; // fill of every node's level-0 list (lists are packed to the front): appending a reverse link
                               // to a 10 M-row graph then costs one cache miss for the count, not a scan of the 256-byte list
    int max_level = -1;
    int64_t entry = -1;
    std::mt19937 rng{12345};

    void init(int M_)
    {
        M = M_;
        // FAISS [ext]: HNSW::set_default_probas(int M, float levelMult) called with 1.0 / log(M): levelMult and
        // proba are FLOATs there (the vector<double> of an IHNf file holds float-rounded values), exp evaluated
        // on the promoted argument.  The level table and the per-level slot counts follow from it.
        const float mult = (float)(1.0 / log((double)M));
        int nn = 0;
        cum_nb.push_back(0);
        for (int level = 0;; level++) {
            const float proba = (float)(exp((double)(-level / mult)) * (1 - exp((double)(-1 / mult))));
            if (proba < 1e-9) break;
            assign_probas.push_back(proba);
            nn += level == 0 ? M * 2 : M;
            cum_nb.push_back(nn);
        }
        offsets.push_back(0);
    }
    int random_level()
    {
        double f = (double)rng() / ((double)rng.max() + 1.0);
        for (size_t level = 0; level < assign_probas.size(); level++) {
            if (f < assign_probas[level]) return (int)level;
            f -= assign_probas[level];
        }
        return (int)assign_probas.size() - 1;
    }
    int nb_neighbors(int level) const { return cum_nb[level + 1] - cum_nb[level]; }
    uint32_t *list(int64_t i, int level) { return nbrs.data() + offsets[i] + cum_nb[level]; }
    const uint32_t *list(int64_t i, int level) const { return nbrs.data() + offsets[i] + cum_nb[level]; }
    int64_t ntotal() const { return (int64_t)levels.size(); }
    void append_node(int level)
    {
        levels.push_back(level);
        offsets.push_back(offsets.back() + cum_nb[level + 1]);
        nbrs.resize(offsets.back(), HNSW_EMPTY);
        cnt0.push_back(0);
    }
};

// set of visited row ids (one per walker): a bitmap when the graph is small enough for
// nwalkers x ntotal / 8 bytes, otherwise an open-addressing hash set
struct VisitedSet {
    std::vector<uint32_t> tab;
    std::vector<uint64_t> bits;
    size_t used = 0;
    bool bitmap = false;
    void reset(size_t expect, size_t ntotal, bool use_bitmap)
    {
        bitmap = use_bitmap;
        if (bitmap) {
            bits.assign((ntotal + 63) / 64, 0ull);
            return;
        }
        size_t cap = 64;
        while (cap < expect * 2) cap <<= 1;
        tab.assign(cap, HNSW_EMPTY);
        used = 0;
    }
    void grow()
    {
        std::vector<uint32_t> old;
        old.swap(tab);
        tab.assign(old.size() * 2, HNSW_EMPTY);
        used = 0;
        for (uint32_t v : old)
            if (v != HNSW_EMPTY) insert(v);
    }
    // returns true if newly inserted
    bool insert(uint32_t v)
    {
        if (bitmap) {
            uint64_t &w = bits[v >> 6];
            const uint64_t m = 1ull << (v & 63);
            if (w & m) return false;
            w |= m;
            return true;
        }
        if ((used + 1) * 2 > tab.size()) grow();
        size_t mask = tab.size() - 1;
        size_t h = ((size_t)v * 0x9E3779B97F4A7C15ull >> 20) & mask;
        while (tab[h] != HNSW_EMPTY) {
            if (tab[h] == v) return false;
            h = (h + 1) & mask;
        }
        tab[h] = v;
        used++;
        return true;
    }
};

typedef std::pair<float, uint32_t> DistId; // ordered by (v, id): ties -> lower id first

// max-heap (std::less order, as std::push_heap keeps it): overwrite the maximum with e and restore the heap
static inline void heap_replace_top(std::vector<DistId> &h, const DistId &e)
{
    const size_t n = h.size();
    size_t i = 0;
    for (;;) {
        size_t c = 2 * i + 1;
        if (c >= n) break;
        if (c + 1 < n && h[c] < h[c + 1]) c++;
        if (!(e < h[c])) break;
        h[i] = h[c];
        i = c;
    }
    h[i] = e;
}

struct Walker {
    uint32_t qslot = 0;   // row of the batch's query matrix (search) or own row id (insert)
    int phase = 0;        // 0 entry distance, 1 greedy descent, 2 beam, 3 done
    int level = 0;        // level being searched
    int stop_level = 0;   // last level to beam-search
    int greedy_until = 0; // descend greedily while level > greedy_until
    uint32_t cur = 0;
    float cur_d = 0.f;
    int ef = 16;
    bool descent_only = false; // stop where the level-0 beam would start (the device runs that part): cur = its entry node
    std::vector<DistId> C; // min-heap
    std::vector<DistId> W; // max-heap
    VisitedSet vis;
    size_t prop_off = 0, prop_n = 0;
    // insertion: candidates kept per level (sorted ascending)
    std::vector<std::vector<DistId>> level_cands;
};

struct knn_hnsw_s {
    knn_index_s *flat = nullptr;
    HnswGraph g;
    int efSearch = 16, efConstruction = 40;
    int max_batch = 16384; // (rows per insertion batch at most: 2 M rows link in 2.1 s against 2.8 s with 4096, same recall)
    int expand = 8; // candidates expanded per walker per lock-step round (1 = strict best-first)
    std::mutex mu;
    // device + pinned staging
    DevBuf d_pa, d_pb, d_out, d_q, d_qn, d_goff, d_mem, d_maxo, d_oid, d_od, d_on;
    PinnedBuf h_pa, h_pb, h_out, h_goff, h_mem, h_maxo, h_oid, h_od, h_on;
    // the walk runs its walkers in two halves: while the GPU computes the distances of one half
    // the host consumes / proposes for the other (own staging buffers, stream and event each)
    DevBuf d_pa2, d_pb2, d_out2;
    PinnedBuf h_pa2, h_pb2, h_out2;
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_pairs[2] = {nullptr, nullptr};
    // level-0 neighbour lists mirrored on the device for the beam kernel ([n][M0]); rebuilt after add / import
    DevBuf d_nbr0, d_entry, d_vis, d_touched, d_beam_ids, d_beam_keys, d_D, d_I, d_stats;
    DevBuf d_D2, d_I2, d_st2;      // second set of result buffers (searches of several batches), the counters of a batch kept for its download
    size_t vis_zero_bytes = 0; // leading bytes of d_vis known to be zero (lazy clearing of the visited bitmaps)
    PinnedBuf h_entry;
    bool nbr0_dirty = true;
    // Rows are linked in a shuffled order (FAISS's hnsw_add_vertices shuffles too, "to get rid of dataset order bias": a
    // batch-synchronous build links a batch against the frozen graph only, and rows that arrive grouped by cluster -- a Pfam
    // FASTA lists its families one after the other -- would otherwise be inserted blind to their own neighbours): the linked
    // nodes are a set, not a prefix
    std::vector<uint8_t> linked;   // [ntotal] node is linked into the graph (the others wait for their batch: no links, never an entry point)
    int64_t linked_count = 0;
    int64_t mirror_count = 0;      // linked nodes the device mirror (level-0 lists, coarse index) reflects
    int shuffle = !(getenv("KNN355_HNSW_ORDER") && !strcmp(getenv("KNN355_HNSW_ORDER"), "sequential")); // (sequential: rounds 1-3, A/B)
    DevBuf d_bids, d_bq, d_bqn;    // the batch being linked: its node ids, its rows gathered ([count][dp]) and their norms
    std::vector<uint32_t> coarse_ids_host;
    DevBuf d_scatter_ids, d_scatter_rows, d_beam_out;
    PinnedBuf h_scatter_ids, h_scatter_rows, h_keys;
    knn_index_s *coarse = nullptr; // flat index over the rows of the nodes above level 0 (entry search)
    knn_index_s *coarse2 = nullptr; // ... and one over the rows of the nodes of level >= 2 (construction candidates of those levels)
    std::vector<uint32_t> coarse2_ids_host; // its rows' node ids
    int64_t ncoarse2 = 0;
    DevBuf d_coarse_ids, d_coarse_keys;
    int64_t ncoarse = 0;
    int coarse_entries = 4;        // level-0 entry points per query taken from the coarse scan (0: greedy descent on the host)
    int beam_expand2 = !(getenv("KNN355_HNSW_EXPAND1") && atoi(getenv("KNN355_HNSW_EXPAND1")) != 0);
    int beam_rows = getenv("KNN355_HNSW_BEAM_ROWS") && atoi(getenv("KNN355_HNSW_BEAM_ROWS")) == 8 ? 8 : 4; // rows in flight per walker
    bool coarse_bf16 = !(getenv("KNN355_HNSW_COARSE_FP32") && atoi(getenv("KNN355_HNSW_COARSE_FP32")) != 0);
    int device_beam = 1; // 0: walk level 0 on the host as well (the round-1 path; KNN355_HNSW_HOST_BEAM=1)
    // Construction, level 0 on the device (hnsw_level0_links_device): the device's lists are then the master copy of level 0 and
    // the host graph's level-0 lists are brought up to date when something on the host reads them (hnsw_host0_sync).
    // KNN355_HNSW_HOST_LINKS=1: the round-3 path (candidates down, host bookkeeping, dirty rows up).
    int device_links = !(getenv("KNN355_HNSW_HOST_LINKS") && atoi(getenv("KNN355_HNSW_HOST_LINKS")) != 0);
    bool host0_stale = false;      // level-0 lists are newer on the device than in g.nbrs / g.cnt0
    DevBuf d_cnt0;                 // [rows of d_nbr0] fill of every level-0 list
    DevBuf dl_mem, dl_goff, dl_gcnt, dl_maxo, dl_gnode, dl_oid, dl_od, dl_on, dl_roff, dl_key[2], dl_from[2], dl_tmp, dl_ctr;
    // stats
    int64_t stat_pairs = 0, stat_rounds = 0, stat_shrinks = 0, stat_expansions = 0;
    int64_t stat_starved = 0; // construction: points whose upper-level candidates fell back to the host walkers
    double stat_gpu_s = 0, stat_host_s = 0;
};

// host threads for the walk: the CPUs this process may run on, at most 16 (a GPU box hands
// each single-GPU job about that share of the machine; more threads only spin); KNN355_THREADS
// overrides
static int hnsw_threads()
{
    static int nt = 0;
    if (nt == 0) {
        int n = 1;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) n = CPU_COUNT(&set);
        if (const char *e2 = getenv("KNN355_THREADS")) nt = std::max(1, atoi(e2));
        else nt = std::max(1, std::min(n, 16));
    }
    return nt;
}

static double now_s()
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
}

// Lock-step walk of all walkers over the frozen graph.  xa/an: the walkers' vectors on the
// device (row = Walker::qslot).  For searches level_cands stays empty and W holds the result.
// The walkers run in two halves: while the GPU computes the distances one half asked for, the
// host consumes the other half's results and collects its next proposals (walkers are independent,
// so the split changes nothing in what each of them visits).
static int hnsw_walk(knn_hnsw_s *H, std::vector<Walker> &ws, const float *xa, const float *an, bool keep_levels)
{
    const HnswGraph &g = H->g;
    if (g.entry < 0) {
        for (auto &w : ws) w.phase = 3;
        return 0;
    }
    knn_index_s *f = H->flat;
    const int nw = (int)ws.size();
    const int nt = nw >= 128 ? hnsw_threads() : 1;
    (void)nt; // (only the host pass sees the OpenMP pragmas that use it)
    const bool use_bitmap = (size_t)nw * ((size_t)g.ntotal() / 8 + 8) <= (256ull << 20);
    std::vector<std::vector<uint32_t>> props(nw);
    const int nhalves = nw >= 512 ? 2 : 1;
    if (nhalves == 2 && !H->stream2) HIP_TRY(hipStreamCreateWithFlags(&H->stream2, hipStreamNonBlocking));
    for (auto &e : H->ev_pairs)
        if (!e) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    struct Half {
        int lo, hi;
        DevBuf *d_pa, *d_pb, *d_out;
        PinnedBuf *h_pa, *h_pb, *h_out;
        hipStream_t stream;
        hipEvent_t done;
        bool active = true;
        size_t total = 0;
    } halves[2] = {{0, nhalves == 2 ? nw / 2 : nw, &H->d_pa, &H->d_pb, &H->d_out, &H->h_pa, &H->h_pb, &H->h_out, f->stream, H->ev_pairs[0]},
                   {nw / 2, nw, &H->d_pa2, &H->d_pb2, &H->d_out2, &H->h_pa2, &H->h_pb2, &H->h_out2, H->stream2, H->ev_pairs[1]}};

    // proposals of one half, staged in its pinned buffers; returns -1 on error, 0 if the half is done
    auto propose = [&](Half &hf) -> int {
        const int lo = hf.lo, hi = hf.hi;
        double th0 = now_s();
        // 1. proposals
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt)
        for (int i = lo; i < hi; i++) {
            Walker &w = ws[i];
            std::vector<uint32_t> &pr = props[i];
            pr.clear();
            if (w.phase == 3) continue;
            if (w.phase == 0) {
                pr.push_back((uint32_t)g.entry);
            } else if (w.phase == 1) {
                const uint32_t *l = g.list(w.cur, w.level);
                const int nn = g.nb_neighbors(w.level);
                for (int j = 0; j < nn && l[j] != HNSW_EMPTY; j++) pr.push_back(l[j]);
                if (pr.empty()) { // isolated at this level: drop a level right away
                    // handled in the consume step with an empty result
                }
            } else {
                // beam: expand up to `expand` of the closest open candidates per round (fewer
                // lock-step rounds for a few extra distances); keep popping while nothing
                // unvisited showed up
                int expanded = 0;
                while (expanded < H->expand || pr.empty()) {
                    if (w.C.empty()) break;
                    expanded++;
                    std::pop_heap(w.C.begin(), w.C.end(), std::greater<DistId>());
                    DistId c = w.C.back();
                    w.C.pop_back();
                    if ((int)w.W.size() >= w.ef && c > w.W.front()) {
                        w.C.clear();
                        break;
                    }
                    const uint32_t *l = g.list(c.second, w.level);
                    const int nn = g.nb_neighbors(w.level);
                    for (int j = 0; j < nn && l[j] != HNSW_EMPTY; j++)
                        if (w.vis.insert(l[j])) pr.push_back(l[j]);
                }
            }
        }
        size_t total = 0;
        bool any_active = false;
        for (int i = lo; i < hi; i++) {
            ws[i].prop_off = total;
            ws[i].prop_n = props[i].size();
            total += props[i].size();
            if (ws[i].phase != 3) any_active = true;
        }
        hf.total = total;
        if (!any_active) {
            H->stat_host_s += now_s() - th0;
            return 0;
        }
        if (hf.h_pa->ensure(total * 4 + 64) || hf.h_pb->ensure(total * 4 + 64) || hf.h_out->ensure(total * 4 + 64)) {
            set_err(KNN_ERR_HIP, "hnsw: out of pinned host memory");
            return -1;
        }
        uint32_t *pa = (uint32_t *)hf.h_pa->p, *pb = (uint32_t *)hf.h_pb->p;
#pragma omp parallel for schedule(static) num_threads(nt)
        for (int i = lo; i < hi; i++) {
            const Walker &w = ws[i];
            for (size_t j = 0; j < w.prop_n; j++) {
                pa[w.prop_off + j] = w.qslot;
                pb[w.prop_off + j] = props[i][j];
            }
        }
        H->stat_host_s += now_s() - th0;
        return 1;
    };
    // distances of the staged pairs, asynchronously on the half's stream
    auto launch = [&](Half &hf) -> int {
        const int64_t np = (int64_t)hf.total;
        hipStream_t s = hf.stream;
        if (np > 0) {
            if (hf.d_pa->ensure((size_t)np * 4) || hf.d_pb->ensure((size_t)np * 4) || hf.d_out->ensure((size_t)np * 4))
                return set_err(KNN_ERR_HIP, "hnsw: out of device memory");
            HIP_TRY(hipMemcpyAsync(hf.d_pa->p, hf.h_pa->p, (size_t)np * 4, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(hf.d_pb->p, hf.h_pb->p, (size_t)np * 4, hipMemcpyHostToDevice, s));
            hipLaunchKernelGGL(pair_v_kernel, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, s, xa, an, f->xb, f->yn, f->dp, f->metric, np,
                               (const uint32_t *)hf.d_pa->p, (const uint32_t *)hf.d_pb->p, (float *)hf.d_out->p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(hf.h_out->p, hf.d_out->p, (size_t)np * 4, hipMemcpyDeviceToHost, s));
            H->stat_pairs += np;
        }
        HIP_TRY(hipEventRecord(hf.done, s));
        H->stat_rounds++;
        return 0;
    };
    auto consume = [&](Half &hf) {
        const int lo = hf.lo, hi = hf.hi;
        const float *out = (const float *)hf.h_out->p;
        double th0 = now_s();
        // 4. consume
#pragma omp parallel for schedule(dynamic, 16) num_threads(nt)
        for (int i = lo; i < hi; i++) {
            Walker &w = ws[i];
            if (w.phase == 3) continue;
            const float *d = out + w.prop_off;
            const std::vector<uint32_t> &pr = props[i];
            auto start_beam = [&]() {
                if (w.descent_only) {
                    w.phase = 3;
                    return;
                }
                w.phase = 2;
                w.C.clear();
                w.W.clear();
                w.vis.reset((size_t)w.ef * 8, (size_t)g.ntotal(), use_bitmap);
                w.vis.insert(w.cur);
                w.C.push_back(DistId(w.cur_d, w.cur));
                w.W.push_back(DistId(w.cur_d, w.cur));
            };
            auto after_descent_step = [&]() {
                // called when no improvement at w.level
                if (w.level > w.greedy_until) {
                    w.level--;
                    if (w.level > w.greedy_until) return; // keep descending greedily
                }
                // w.level == greedy_until: beam search starts here
                start_beam();
            };
            if (w.phase == 0) {
                w.cur = (uint32_t)g.entry;
                w.cur_d = d[0];
                w.level = g.max_level;
                if (w.level > w.greedy_until) w.phase = 1;
                else { w.level = std::min(w.level, w.greedy_until); start_beam(); }
            } else if (w.phase == 1) {
                bool improved = false;
                for (size_t j = 0; j < pr.size(); j++) {
                    if (DistId(d[j], pr[j]) < DistId(w.cur_d, w.cur)) {
                        w.cur_d = d[j];
                        w.cur = pr[j];
                        improved = true;
                    }
                }
                if (!improved) after_descent_step();
            } else {
                for (size_t j = 0; j < pr.size(); j++) {
                    DistId e(d[j], pr[j]);
                    if ((int)w.W.size() < w.ef || e < w.W.front()) {
                        w.C.push_back(e);
                        std::push_heap(w.C.begin(), w.C.end(), std::greater<DistId>());
                        if ((int)w.W.size() < w.ef) {
                            w.W.push_back(e);
                            std::push_heap(w.W.begin(), w.W.end());
                        } else {
                            heap_replace_top(w.W, e); // e < current maximum: one sift-down instead of push + pop
                        }
                    }
                }
                if (w.C.empty() && pr.empty()) {
                    // beam at this level finished
                    std::sort(w.W.begin(), w.W.end());
                    if (keep_levels) {
                        if ((int)w.level_cands.size() <= w.level) w.level_cands.resize(w.level + 1);
                        w.level_cands[w.level] = w.W;
                    }
                    if (w.level > w.stop_level) {
                        // next level down starts from the closest point found here
                        w.cur = w.W[0].second;
                        w.cur_d = w.W[0].first;
                        w.level--;
                        start_beam();
                    } else {
                        w.phase = 3;
                    }
                }
            }
        }
        H->stat_host_s += now_s() - th0;
    };

    // the walkers' vectors (xa) may have been produced on f->stream: the second stream starts after it
    if (nhalves == 2) {
        HIP_TRY(hipEventRecord(H->ev_pairs[1], f->stream));
        HIP_TRY(hipStreamWaitEvent(H->stream2, H->ev_pairs[1], 0));
    }
    for (int h = 0; h < nhalves; h++) {
        int r = propose(halves[h]);
        if (r < 0) return KNN_ERR_HIP;
        halves[h].active = r > 0;
        if (halves[h].active) {
            int rc = launch(halves[h]);
            if (rc) return rc;
        }
    }
    for (;;) {
        bool any = false;
        for (int h = 0; h < nhalves; h++) {
            Half &hf = halves[h];
            if (!hf.active) continue;
            any = true;
            double tg0 = now_s();
            HIP_TRY(hipEventSynchronize(hf.done));
            H->stat_gpu_s += now_s() - tg0; // time the host actually waited for the GPU
            consume(hf);
            int r = propose(hf);
            if (r < 0) return KNN_ERR_HIP;
            hf.active = r > 0;
            if (hf.active) {
                int rc = launch(hf);
                if (rc) return rc;
            }
        }
        if (!any) break;
    }
    if (nhalves == 2) HIP_TRY(hipStreamSynchronize(H->stream2));
    return 0;
}

// one workgroup per group; nr: the largest group's members rounded up to 64, 96 or 128
template <int NR>
static int launch_shrink_nr(const ShrinkParams &p, int grid, hipStream_t s)
{
    const size_t lds = std::max((size_t)2 * NR * 128, (size_t)NR * (NR + 1) * 4) + (size_t)NR * 16;
    HIP_TRY(hipFuncSetAttribute((const void *)gram_shrink_kernel<NR>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(gram_shrink_kernel<NR>, dim3((unsigned)grid), dim3(256), lds, s, p);
    HIP_TRY(hipGetLastError());
    return 0;
}
static int launch_shrink(const ShrinkParams &p, int grid, int max_members, hipStream_t s)
{
    if (grid <= 0) return 0;
    if (max_members <= 64) return launch_shrink_nr<64>(p, grid, s);
    if (max_members <= 96) return launch_shrink_nr<96>(p, grid, s);
    return launch_shrink_nr<128>(p, grid, s);
}

// runs the pruning heuristic on the GPU for `ngroups` groups staged in h_goff/h_mem/h_maxo (max_members: the largest group)
static int hnsw_run_shrink(knn_hnsw_s *H, int ngroups, size_t nmembers, int out_stride, int max_members = SHRINK_MAX_MEMBERS)
{
    if (ngroups == 0) return 0;
    knn_index_s *f = H->flat;
    hipStream_t s = f->stream;
    if (H->d_goff.ensure((size_t)(ngroups + 1) * 4) || H->d_mem.ensure(nmembers * 4) || H->d_maxo.ensure((size_t)ngroups * 4) ||
        H->d_oid.ensure((size_t)ngroups * out_stride * 4) || H->d_od.ensure((size_t)ngroups * out_stride * 4) ||
        H->d_on.ensure((size_t)ngroups * 4))
        return set_err(KNN_ERR_HIP, "hnsw: out of device memory");
    if (H->h_oid.ensure((size_t)ngroups * out_stride * 4) || H->h_od.ensure((size_t)ngroups * out_stride * 4) ||
        H->h_on.ensure((size_t)ngroups * 4))
        return set_err(KNN_ERR_HIP, "hnsw: out of pinned host memory");
    double t0 = now_s();
    HIP_TRY(hipMemcpyAsync(H->d_goff.p, H->h_goff.p, (size_t)(ngroups + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(H->d_mem.p, H->h_mem.p, nmembers * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(H->d_maxo.p, H->h_maxo.p, (size_t)ngroups * 4, hipMemcpyHostToDevice, s));
    ShrinkParams p;
    p.xb = f->xb; p.yn = f->yn; p.dp = f->dp; p.metric = f->metric;
    p.group_off = (const int32_t *)H->d_goff.p; p.group_cnt = nullptr; p.ngroups = nullptr; p.members = (const uint32_t *)H->d_mem.p;
    p.max_out = (const int32_t *)H->d_maxo.p; p.out_ids = (uint32_t *)H->d_oid.p; p.out_d = (float *)H->d_od.p;
    p.out_n = (int32_t *)H->d_on.p; p.out_stride = out_stride;
    int rc = launch_shrink(p, ngroups, max_members, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(H->h_oid.p, H->d_oid.p, (size_t)ngroups * out_stride * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(H->h_od.p, H->d_od.p, (size_t)ngroups * out_stride * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(H->h_on.p, H->d_on.p, (size_t)ngroups * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    H->stat_gpu_s += now_s() - t0;
    H->stat_shrinks += ngroups;
    return 0;
}

// device side of the construction (defined with the search code below)
static int hnsw_upload_graph(knn_hnsw_s *H);
static int hnsw_level0_candidates_device(knn_hnsw_s *H, const int64_t *ids, int count, std::vector<std::vector<DistId>> &cand0);
static int hnsw_upper_candidates_device(knn_hnsw_s *H, const int64_t *ids, const std::vector<int> &up, std::vector<std::vector<std::vector<DistId>>> &lc,
                                        std::vector<int> &starved);
static int hnsw_mirror_update(knn_hnsw_s *H, const int64_t *ids, int count, std::vector<uint32_t> &dirty);
static int hnsw_level0_links_device(knn_hnsw_s *H, const int64_t *ids, int count);
static int hnsw_host0_sync(knn_hnsw_s *H);

// inserts rows ids[0 .. count) (ascending; already stored in the flat index, not linked yet) into the graph
#ifdef KNN355_DEV
static double g_hnsw_prof[8] = {0};
#define HNSW_PROF(i, t0) do { g_hnsw_prof[i] += now_s() - (t0); (t0) = now_s(); } while (0)
#else
#define HNSW_PROF(i, t0) do { } while (0)
#endif
static int hnsw_insert_batch(knn_hnsw_s *H, const int64_t *ids, int count)
{
    HnswGraph &g = H->g;
    double tp = now_s();
    (void)tp;
    knn_index_s *f = H->flat;
    const int M0 = g.nb_neighbors(0);
    // Level-0 candidates come from the device once the graph has enough nodes above level 0 for a coarse entry
    // scan: the same beam kernel as the search, ef = efConstruction, entered at the exact nearest of those nodes.
    // (Entering through the greedy descent, one cluster in eight of a 10 M-row graph was linked to the wrong
    // neighbourhood: recall@100 stalled at 0.88 whatever the efSearch.)  The upper levels -- one node in M has
    // any -- are still searched by the host walkers.
    bool dev = H->device_beam && H->coarse_entries > 0 && f->dp <= 1024 && f->dp == f->d && H->efConstruction <= 1024 &&
               g.ntotal() < (1ll << 31) && !(getenv("KNN355_HNSW_HOST_BEAM") && atoi(getenv("KNN355_HNSW_HOST_BEAM")) != 0);
    if (dev && (H->nbr0_dirty || H->mirror_count != H->linked_count)) {
        // (the mirror is rebuilt from the host graph, which holds the new nodes already: they have no links yet)
        int rc = hnsw_upload_graph(H);
        if (rc) return rc;
    }
    if (dev && H->ncoarse < 64) dev = false;
    const bool dev_links = dev && H->device_links && M0 <= 255;
    if (!dev_links && H->host0_stale) { // (this batch reads and writes the host's level-0 lists)
        int rc = hnsw_host0_sync(H);
        if (rc) return rc;
    }
    HNSW_PROF(7, tp); // (re)building the device mirror
    // 1. search the frozen graph for every new point
    std::vector<std::vector<std::vector<DistId>>> lc((size_t)count); // [point][level] candidates, ascending
    int rc;
    {
        std::vector<int> widx; // points that need a host walker
        std::vector<int> up;   // points with levels above 0 whose candidates come from the device
        const bool dev_upper = dev && !(getenv("KNN355_HNSW_HOST_UPPER") && atoi(getenv("KNN355_HNSW_HOST_UPPER")) != 0);
        for (int i = 0; i < count; i++) {
            const int top = std::min(g.levels[ids[i]], g.max_level);
            if (!dev) widx.push_back(i);
            else if (top >= 1) (dev_upper ? up : widx).push_back(i);
        }
        if (!up.empty()) {
            std::vector<int> starved;
            rc = hnsw_upper_candidates_device(H, ids, up, lc, starved);
            if (rc) return rc;
            for (int i : starved) { // (the scan found too few nodes of their highest levels: host walkers, every upper level)
                lc[(size_t)i].clear();
                widx.push_back(i);
            }
            H->stat_starved += (int64_t)starved.size();
        }
        std::vector<Walker> ws(widx.size());
        for (size_t wi = 0; wi < widx.size(); wi++) {
            Walker &w = ws[wi];
            const int64_t id = ids[widx[wi]];
            w.qslot = (uint32_t)id;
            w.ef = H->efConstruction;
            w.greedy_until = std::min(g.levels[id], g.max_level);
            w.stop_level = dev ? 1 : 0;
            w.phase = 0;
        }
        if (!ws.empty()) {
            rc = hnsw_walk(H, ws, f->xb, f->yn, true);
            if (rc) return rc;
        }
        for (size_t wi = 0; wi < widx.size(); wi++) lc[widx[wi]] = std::move(ws[wi].level_cands);
    }
    HNSW_PROF(0, tp); // host walkers (upper levels)
    if (dev_links) {
        // level 0 stays on the device: candidates, selection, links, reverse links (the phases below then see the upper levels only)
        rc = hnsw_level0_links_device(H, ids, count);
        if (rc) return rc;
        tp = now_s(); // (the function keeps its own account of the phases)
    } else if (dev) {
        std::vector<std::vector<DistId>> cand0;
        rc = hnsw_level0_candidates_device(H, ids, count, cand0);
        if (rc) return rc;
        for (int i = 0; i < count; i++) {
            if (lc[i].empty()) lc[i].resize(1);
            lc[i][0] = std::move(cand0[i]);
        }
    }

    HNSW_PROF(1, tp); // level-0 candidates on the device
    // 2. forward selection: one group per (point, level) with candidates
    struct Job { int point; int level; };
    std::vector<Job> jobs;
    for (int i = 0; i < count; i++)
        for (int l = 0; l < (int)lc[i].size(); l++)
            if (!lc[i][l].empty()) jobs.push_back({i, l});
    std::vector<std::vector<DistId>> fwd(jobs.size()); // selected (v, id) per job
    if (!jobs.empty()) {
        size_t nmem = 0;
        for (auto &j : jobs) nmem += 1 + std::min<size_t>(lc[j.point][j.level].size(), SHRINK_MAX_MEMBERS - 1);
        if (H->h_goff.ensure((jobs.size() + 1) * 4) || H->h_mem.ensure(nmem * 4) || H->h_maxo.ensure(jobs.size() * 4))
            return set_err(KNN_ERR_HIP, "hnsw: out of pinned host memory");
        int32_t *goff = (int32_t *)H->h_goff.p;
        uint32_t *mem = (uint32_t *)H->h_mem.p;
        int32_t *maxo = (int32_t *)H->h_maxo.p;
        size_t o = 0, largest = 0;
        for (size_t j = 0; j < jobs.size(); j++) { // (offsets first, then the host threads fill their groups)
            goff[j] = (int32_t)o;
            const size_t nm = 1 + std::min<size_t>(lc[jobs[j].point][jobs[j].level].size(), SHRINK_MAX_MEMBERS - 1);
            largest = std::max(largest, nm);
            o += nm;
        }
        goff[jobs.size()] = (int32_t)o;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t j = 0; j < (int64_t)jobs.size(); j++) {
            size_t w = (size_t)goff[j];
            mem[w++] = (uint32_t)ids[jobs[j].point];
            const auto &cl = lc[jobs[j].point][jobs[j].level];
            const size_t take = std::min<size_t>(cl.size(), SHRINK_MAX_MEMBERS - 1);
            for (size_t c = 0; c < take; c++) mem[w++] = cl[c].second;
            maxo[j] = g.nb_neighbors(jobs[j].level);
        }
        rc = hnsw_run_shrink(H, (int)jobs.size(), o, M0, (int)largest);
        if (rc) return rc;
        const uint32_t *oid = (const uint32_t *)H->h_oid.p;
        const float *od = (const float *)H->h_od.p;
        const int32_t *on = (const int32_t *)H->h_on.p;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t j = 0; j < (int64_t)jobs.size(); j++) {
            fwd[j].reserve((size_t)on[j]);
            for (int c = 0; c < on[j]; c++) fwd[j].push_back(DistId(od[j * M0 + c], oid[j * M0 + c]));
        }
    }
    HNSW_PROF(2, tp); // forward selection (gram_shrink)
    // 3. write forward links; collect reverse link requests per (node, level)
    struct Rev { uint32_t node; int level; uint32_t from; float d; };
    std::vector<Rev> revs;
    std::vector<uint32_t> dirty; // nodes whose level-0 list changed (the device mirror follows)
    {
        std::vector<size_t> roff(jobs.size() + 1, 0);
        for (size_t j = 0; j < jobs.size(); j++) roff[j + 1] = roff[j] + fwd[j].size();
        revs.resize(roff[jobs.size()]);
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t j = 0; j < (int64_t)jobs.size(); j++) {
            const uint32_t pid = (uint32_t)ids[jobs[j].point];
            uint32_t *l = g.list(pid, jobs[j].level);
            int c = 0;
            size_t w = roff[j];
            for (auto &e : fwd[j]) {
                l[c++] = e.second;
                revs[w++] = Rev{e.second, jobs[j].level, pid, e.first};
            }
            if (jobs[j].level == 0) g.cnt0[pid] = (uint8_t)c;
        }
    }
    if (!dev_links) // (the device wrote the new nodes' rows itself)
        for (int i = 0; i < count; i++) dirty.push_back((uint32_t)ids[i]);
    auto rev_less = [](const Rev &a, const Rev &b) {
        if (a.node != b.node) return a.node < b.node;
        if (a.level != b.level) return a.level < b.level;
        if (a.d != b.d) return a.d < b.d;
        return a.from < b.from;
    };
    {
        // sorted in slices by the host threads, then merged pairwise (the order is total: the result does not depend on
        // the number of threads)
        const int nt = std::max(1, std::min<int>(hnsw_threads(), (int)(revs.size() / 65536)));
        if (nt <= 1) {
            std::sort(revs.begin(), revs.end(), rev_less);
        } else {
            std::vector<size_t> cut((size_t)nt + 1);
            for (int t = 0; t <= nt; t++) cut[t] = revs.size() * (size_t)t / nt;
#pragma omp parallel for schedule(static, 1) num_threads(nt)
            for (int t = 0; t < nt; t++) std::sort(revs.begin() + cut[t], revs.begin() + cut[t + 1], rev_less);
            for (int w = 1; w < nt; w *= 2) {
#pragma omp parallel for schedule(static, 1) num_threads(nt)
                for (int t = 0; t < nt; t += 2 * w)
                    if (t + w < nt) std::inplace_merge(revs.begin() + cut[t], revs.begin() + cut[t + w], revs.begin() + cut[std::min(nt, t + 2 * w)], rev_less);
            }
        }
    }
    HNSW_PROF(3, tp); // forward links + sorting the reverse requests
    // 4. reverse links: append where there is room, otherwise prune on the GPU
    struct Prune { uint32_t node; int level; size_t r0, r1; };
    std::vector<Prune> prunes;
    {
        // groups of requests for one (node, level): every group writes its own list, so the groups are shared out to the host
        // threads (cut at group boundaries); the per-thread results are concatenated in thread order = request order
        const int nt = std::max(1, std::min<int>(hnsw_threads(), (int)(revs.size() / 65536)));
        std::vector<size_t> cut((size_t)nt + 1, revs.size());
        cut[0] = 0;
        for (int t = 1; t < nt; t++) {
            size_t c = revs.size() * (size_t)t / nt;
            while (c < revs.size() && c > 0 && revs[c].node == revs[c - 1].node && revs[c].level == revs[c - 1].level) c++;
            cut[t] = std::max(c, cut[t - 1]);
        }
        std::vector<std::vector<Prune>> tp_prunes((size_t)nt);
        std::vector<std::vector<uint32_t>> tp_dirty((size_t)nt);
#pragma omp parallel for schedule(static, 1) num_threads(nt)
        for (int t = 0; t < nt; t++) {
            for (size_t r0 = cut[t]; r0 < cut[t + 1];) {
                size_t r1 = r0;
                while (r1 < cut[t + 1] && revs[r1].node == revs[r0].node && revs[r1].level == revs[r0].level) r1++;
                uint32_t *l = g.list(revs[r0].node, revs[r0].level);
                const int cap = g.nb_neighbors(revs[r0].level);
                int have = 0;
                if (revs[r0].level == 0) have = g.cnt0[revs[r0].node];
                else while (have < cap && l[have] != HNSW_EMPTY) have++;
                if (revs[r0].level == 0) tp_dirty[t].push_back(revs[r0].node);
                if (have + (int)(r1 - r0) <= cap) {
                    for (size_t r = r0; r < r1; r++) l[have++] = revs[r].from;
                    if (revs[r0].level == 0) g.cnt0[revs[r0].node] = (uint8_t)have;
                } else {
                    tp_prunes[t].push_back({revs[r0].node, revs[r0].level, r0, r1});
                }
                r0 = r1;
            }
        }
        for (int t = 0; t < nt; t++) {
            prunes.insert(prunes.end(), tp_prunes[t].begin(), tp_prunes[t].end());
            dirty.insert(dirty.end(), tp_dirty[t].begin(), tp_dirty[t].end());
        }
    }
    HNSW_PROF(4, tp); // reverse links appended
    if (!prunes.empty()) {
        size_t nmem = prunes.size() * (size_t)SHRINK_MAX_MEMBERS;
        if (H->h_goff.ensure((prunes.size() + 1) * 4) || H->h_mem.ensure(nmem * 4) || H->h_maxo.ensure(prunes.size() * 4))
            return set_err(KNN_ERR_HIP, "hnsw: out of pinned host memory");
        int32_t *goff = (int32_t *)H->h_goff.p;
        uint32_t *mem = (uint32_t *)H->h_mem.p;
        int32_t *maxo = (int32_t *)H->h_maxo.p;
        size_t o = 0, largest = 0;
        for (size_t j = 0; j < prunes.size(); j++) {
            goff[j] = (int32_t)o;
            largest = std::max(largest, o - (j ? (size_t)goff[j - 1] : 0));
            const uint32_t *l = g.list(prunes[j].node, prunes[j].level);
            const int cap = g.nb_neighbors(prunes[j].level);
            mem[o++] = prunes[j].node;
            int nm = 1;
            for (int c = 0; c < cap && l[c] != HNSW_EMPTY; c++, nm++) mem[o++] = l[c];
            // closest new links first (revs are sorted by distance), as many as fit
            for (size_t r = prunes[j].r0; r < prunes[j].r1 && nm < SHRINK_MAX_MEMBERS; r++, nm++) mem[o++] = revs[r].from;
            maxo[j] = cap;
        }
        goff[prunes.size()] = (int32_t)o;
        largest = std::max(largest, o - (size_t)goff[prunes.size() - 1]);
        rc = hnsw_run_shrink(H, (int)prunes.size(), o, M0, (int)largest);
        if (rc) return rc;
        const uint32_t *oid = (const uint32_t *)H->h_oid.p;
        const int32_t *on = (const int32_t *)H->h_on.p;
        for (size_t j = 0; j < prunes.size(); j++) {
            uint32_t *l = g.list(prunes[j].node, prunes[j].level);
            const int cap = g.nb_neighbors(prunes[j].level);
            for (int c = 0; c < cap; c++) l[c] = c < on[j] ? oid[j * M0 + c] : HNSW_EMPTY;
            if (prunes[j].level == 0) g.cnt0[prunes[j].node] = (uint8_t)std::min(on[j], cap);
        }
    }
    HNSW_PROF(5, tp); // reverse pruning (gram_shrink)
    // 5. entry point / max level
    for (int i = 0; i < count; i++) {
        const int64_t id = ids[i];
        if (g.levels[id] > g.max_level) {
            g.max_level = g.levels[id];
            g.entry = id;
        }
    }
    // 6. the device mirror follows (changed level-0 rows, new nodes above level 0 join the coarse index)
    if (dev) {
        rc = hnsw_mirror_update(H, ids, count, dirty);
        HNSW_PROF(6, tp); // device mirror + coarse index update
        return rc;
    }
    H->nbr0_dirty = true;
    return 0;
}
#ifdef KNN355_DEV
extern "C" void knn_dev_hnsw_profile(double *out8, int reset)
{
    for (int i = 0; i < 8; i++) {
        out8[i] = g_hnsw_prof[i];
        if (reset) g_hnsw_prof[i] = 0;
    }
}
#endif

extern "C" int knn_hnsw_create(int32_t d, int32_t M, int32_t metric, knn_hnsw_s **out)
{
    if (!out) return set_err(KNN_ERR_INVALID, "hnsw_create: null out");
    if (M < 2 || M > 63) return set_err(KNN_ERR_INVALID, "hnsw_create: M must be in [2, 63] (2M+1 rows per pruning group <= 128)");
    knn_handle flat = nullptr;
    int rc = knn_flat_create(d, metric, &flat);
    if (rc) return rc;
    knn_hnsw_s *H = new knn_hnsw_s();
    H->flat = flat;
    H->g.init(M);
    // the level-0 beam walks on bf16 copies of the rows, kept by the storage index beside the fp32 rows (+50 % memory;
    // every returned row is re-scored from the fp32 rows).  KNN355_HNSW_BEAM_FP32=1: no copies, the beam reads fp32.
    // (rows wider than the device beam serves are walked on the host: no copies for those)
    if (round_up(d, 32) <= 1024 && !(getenv("KNN355_HNSW_BEAM_FP32") && atoi(getenv("KNN355_HNSW_BEAM_FP32")) != 0)) {
        rc = flat_keep16(flat);
        if (rc) {
            knn_free(flat);
            delete H;
            return rc;
        }
    }
    *out = H;
    return 0;
}

extern "C" void knn_hnsw_free(knn_hnsw_s *H)
{
    if (!H) return;
    if (hipSetDevice(H->flat->device) == hipSuccess) {
        DevBuf *db[] = {&H->d_beam_out, &H->d_scatter_ids, &H->d_scatter_rows, &H->d_coarse_ids, &H->d_coarse_keys, &H->d_nbr0, &H->d_entry, &H->d_vis, &H->d_touched, &H->d_beam_ids, &H->d_beam_keys, &H->d_D, &H->d_I, &H->d_stats, &H->d_pa2, &H->d_pb2, &H->d_out2, &H->d_pa, &H->d_pb, &H->d_out, &H->d_q, &H->d_qn, &H->d_goff, &H->d_mem, &H->d_maxo, &H->d_oid, &H->d_od, &H->d_on,
                         &H->d_D2, &H->d_I2, &H->d_st2, &H->d_cnt0, &H->d_bids, &H->d_bq, &H->d_bqn, &H->dl_mem, &H->dl_goff, &H->dl_gcnt, &H->dl_maxo, &H->dl_gnode, &H->dl_oid, &H->dl_od, &H->dl_on, &H->dl_roff,
                         &H->dl_key[0], &H->dl_key[1], &H->dl_from[0], &H->dl_from[1], &H->dl_tmp, &H->dl_ctr};
        for (auto b : db) b->release();
        PinnedBuf *pb[] = {&H->h_scatter_ids, &H->h_scatter_rows, &H->h_keys, &H->h_entry, &H->h_pa2, &H->h_pb2, &H->h_out2, &H->h_pa, &H->h_pb, &H->h_out, &H->h_goff, &H->h_mem, &H->h_maxo, &H->h_oid, &H->h_od, &H->h_on};
        for (auto b : pb) b->release();
        if (H->stream2) (void)hipStreamDestroy(H->stream2);
        for (auto &e : H->ev_pairs)
            if (e) (void)hipEventDestroy(e);
    }
    if (H->coarse) knn_free(H->coarse);
    if (H->coarse2) knn_free(H->coarse2);
    knn_free(H->flat);
    delete H;
}

extern "C" int knn_hnsw_set_ef(knn_hnsw_s *H, int32_t efSearch, int32_t efConstruction)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_set_ef: null handle");
    std::lock_guard<std::mutex> lk(H->mu);
    if (efSearch > 0) H->efSearch = efSearch;
    // efConstruction is the width of the construction beam, as in FAISS, and is kept as given.  The closest
    // SHRINK_MAX_MEMBERS - 1 of the beam's candidates, by the walk's key, take part in the selection; above 1024 the device
    // beam is off and host walkers link the rows (hnsw_insert_batch).
    if (efConstruction > 0) H->efConstruction = efConstruction;
    return 0;
}

// walk tuning (not part of the faiss surface): candidates expanded per walker per round
// (1 = strict best-first order) and walkers per lock-step batch
extern "C" int knn_hnsw_set_walk(knn_hnsw_s *H, int32_t expand, int32_t max_batch)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_set_walk: null handle");
    std::lock_guard<std::mutex> lk(H->mu);
    if (expand > 0) H->expand = std::min(expand, 64);
    if (max_batch > 0) H->max_batch = std::min(max_batch, 1 << 16);
    return 0;
}

// entry points of the level-0 walk: n > 0 -- the n nearest nodes above level 0, found by an exact scan on the flat
// kernel (default 4); 0 -- the classic greedy descent through the upper levels
extern "C" int knn_hnsw_set_entry(knn_hnsw_s *H, int32_t coarse_entries)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_set_entry: null handle");
    if (coarse_entries < 0 || coarse_entries > 64) return set_err(KNN_ERR_INVALID, "hnsw_set_entry: 0..64 entry points");
    std::lock_guard<std::mutex> lk(H->mu);
    if ((coarse_entries > 0) != (H->coarse_entries > 0)) H->nbr0_dirty = true; // (the coarse index exists only when used)
    H->coarse_entries = coarse_entries;
    return 0;
}

extern "C" int knn_hnsw_get_params(knn_hnsw_s *H, int32_t *M, int32_t *efSearch, int32_t *efConstruction, int32_t *max_level,
                                   int64_t *entry_point)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_get_params: null handle");
    if (M) *M = H->g.M;
    if (efSearch) *efSearch = H->efSearch;
    if (efConstruction) *efConstruction = H->efConstruction;
    if (max_level) *max_level = H->g.max_level;
    if (entry_point) *entry_point = H->g.entry;
    return 0;
}

extern "C" int64_t knn_hnsw_ntotal(knn_hnsw_s *H) { return H ? H->g.ntotal() : -1; }
extern "C" knn_handle knn_hnsw_storage(knn_hnsw_s *H) { return H ? H->flat : nullptr; }

// links rows [n0, n0 + n) (already stored in the flat index) into the graph
static int hnsw_link_rows(knn_hnsw_s *H, int64_t n0, int64_t n)
{
    for (int64_t i = 0; i < n; i++) H->g.append_node(H->g.random_level());
    H->linked.resize((size_t)H->g.ntotal(), 0);
    // the device mirror holds one row per node: too small for the new total -> rebuilt at the next use
    if ((size_t)H->g.ntotal() * H->g.nb_neighbors(0) * 4 > H->d_nbr0.bytes) H->nbr0_dirty = true;
    // the order the rows are linked in: shuffled (Fisher-Yates on the standard's mt19937: the same on every platform),
    // a fixed function of (first row, count) -- the build stays deterministic
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = n0 + i;
    if (H->shuffle) {
        std::mt19937 rng((uint32_t)(789u + (uint64_t)n0 * 2654435761u));
        for (int64_t i = n - 1; i > 0; i--) std::swap(order[(size_t)i], order[(size_t)(rng() % (uint64_t)(i + 1))]);
    }
    // batches grow with the graph: a batch never exceeds a quarter of what is already linked
    int64_t pos = 0;
    while (pos < n) {
        const int64_t done = H->linked_count;
        int64_t b = std::max<int64_t>(1, std::min<int64_t>(H->max_batch, done / 4));
        // ... nor 1/32 of its add call (32 rows at least): a call that brings one family -- rows added file by file -- is
        // linked in 32 batches, the later ones see the earlier ones (recall@50 0.992 against 0.83 with whole calls as batches,
        // tools/hnsw_sorted_probe.py).  The price: a small call into a large graph (1000 rows) is 32 batches of 32 rows, each
        // a full device pipeline (~1 ms): incremental adds of a few hundred rows cost ~30 ms per call whatever they bring.
        // The insertion order is seeded by (n0, n): the graph depends on how the rows are split over add() calls.
        b = std::min(b, std::max<int64_t>(32, n / 32));
        b = std::min(b, n - pos);
        if (H->g.entry < 0) {
            // very first point: becomes the entry point, no links yet
            const int64_t id = order[(size_t)pos];
            H->g.entry = id;
            H->g.max_level = H->g.levels[id];
            H->linked[(size_t)id] = 1;
            H->linked_count++;
            pos += 1;
            H->nbr0_dirty = true;
            continue;
        }
        std::sort(order.begin() + pos, order.begin() + pos + b); // (inside a batch the order means nothing: ascending rows read better)
        int rc = hnsw_insert_batch(H, order.data() + pos, (int)b);
        if (rc) return rc;
        for (int64_t i = 0; i < b; i++) H->linked[(size_t)order[(size_t)(pos + i)]] = 1;
        H->linked_count += b;
        pos += b;
    }
    return 0;
}

extern "C" int knn_hnsw_add(knn_hnsw_s *H, const float *x_host, int64_t n)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_add: null handle");
    if (n < 0) return set_err(KNN_ERR_INVALID, "hnsw_add: negative n");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(H->mu);
    const int64_t n0 = H->g.ntotal();
    int rc = knn_flat_add(H->flat, x_host, n); // rows + norms on the device
    if (rc) return rc;
    HIP_TRY(hipSetDevice(H->flat->device));
    return hnsw_link_rows(H, n0, n);
}

// rows already on the device ([n][d] contiguous): no host copy of the database is needed to build the graph
extern "C" int knn_hnsw_add_dev(knn_hnsw_s *H, const float *x_dev, int64_t n, void *stream)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_add: null handle");
    if (n < 0) return set_err(KNN_ERR_INVALID, "hnsw_add: negative n");
    if (n == 0) return 0;
    std::lock_guard<std::mutex> lk(H->mu);
    const int64_t n0 = H->g.ntotal();
    int rc = knn_flat_add_dev(H->flat, x_dev, n, stream); // (synchronises)
    if (rc) return rc;
    HIP_TRY(hipSetDevice(H->flat->device));
    return hnsw_link_rows(H, n0, n);
}

// rows ids[0..m) of src ([.][dp]) -> dst [m][d] (contiguous, unpadded: what knn_flat_add_dev takes)
__global__ void gather_rows_kernel(const float *__restrict__ src, int dp, int d, const uint32_t *__restrict__ ids, int64_t m,
                                   float *__restrict__ dst)
{
    const int64_t r = blockIdx.x;
    if (r >= m) return;
    const float *a = src + (size_t)ids[r] * dp;
    float *b = dst + (size_t)r * d;
    for (int c = threadIdx.x; c < d; c += blockDim.x) b[c] = a[c];
}

// coarse search result (sorted keys over the coarse index's local rows) -> graph node ids
__global__ void coarse_entries_kernel(const uint64_t *__restrict__ keys, int64_t total, const uint32_t *__restrict__ coarse_ids,
                                      uint32_t *__restrict__ entry)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const uint64_t kk = keys[i];
    entry[i] = kk == KEY_PAD ? HNSW_EMPTY : coarse_ids[(uint32_t)kk];
}

// rows[i] -> nbr0[ids[i]] (64 lanes per row)
__global__ void scatter_rows_kernel(const uint32_t *__restrict__ ids, const uint32_t *__restrict__ rows, int M0, int64_t nd,
                                    uint32_t *__restrict__ nbr0)
{
    const int64_t r = blockIdx.x;
    if (r >= nd) return;
    for (int c = threadIdx.x; c < M0; c += blockDim.x) nbr0[(size_t)ids[r] * M0 + c] = rows[(size_t)r * M0 + c];
}

__global__ void scatter_bytes_kernel(const uint32_t *__restrict__ ids, const uint8_t *__restrict__ v, int64_t n, uint8_t *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[ids[i]] = v[i];
}
__global__ void gather_f32_kernel(const float *__restrict__ src, const uint32_t *__restrict__ ids, int64_t n, float *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = src[ids[i]];
}

// rows of the nodes `add` (level >= 2, linked) -> the index the construction candidates of the levels >= 2 are scanned from
static int hnsw_coarse2_append(knn_hnsw_s *H, const std::vector<uint32_t> &add)
{
    if (add.empty()) return 0;
    knn_index_s *f = H->flat;
    hipStream_t s = f->stream;
    if (!H->coarse2) {
        const int dev_before = g_device;
        g_device = f->device; // (knn_flat_create builds on the calling thread's current device)
        int rc = knn_flat_create(f->d, f->metric, &H->coarse2);
        g_device = dev_before;
        if (rc) return rc;
        if (H->coarse_bf16) {
            rc = flat_set_approx16(H->coarse2);
            if (rc) return rc;
        }
    }
    DevBuf d_ids, d_rows;
    if (d_ids.ensure(add.size() * 4) || d_rows.ensure(add.size() * (size_t)f->d * 4)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (level-2 rows)");
    HIP_TRY(hipMemcpy(d_ids.p, add.data(), add.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)add.size()), dim3(256), 0, s, f->xb, f->dp, f->d, (const uint32_t *)d_ids.p, (int64_t)add.size(),
                       (float *)d_rows.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s));
    int rc = knn_flat_add_dev(H->coarse2, (const float *)d_rows.p, (int64_t)add.size(), nullptr);
    d_ids.release();
    d_rows.release();
    if (rc) return rc;
    H->coarse2_ids_host.insert(H->coarse2_ids_host.end(), add.begin(), add.end());
    H->ncoarse2 = (int64_t)H->coarse2_ids_host.size();
    return 0;
}

// level-0 lists -> device ([n][M0] rows of 4 * M0 bytes: one coalesced load per expansion)
static int hnsw_upload_graph(knn_hnsw_s *H)
{
    if (!H->nbr0_dirty) return 0;
    if (H->host0_stale) { // (the mirror is rebuilt from the host's lists: they must be the current ones)
        int rc0 = hnsw_host0_sync(H);
        if (rc0) return rc0;
    }
    const HnswGraph &g = H->g;
    const int64_t n = g.ntotal();
    const int M0 = g.nb_neighbors(0);
#ifdef KNN355_DEV
    if (getenv("KNN355_HNSW_DEBUG")) fprintf(stderr, "hnsw_upload_graph: n=%lld linked=%lld mirror_n=%lld nbr0 bytes=%zu\n", (long long)n, (long long)H->linked_count, (long long)H->mirror_count, H->d_nbr0.bytes);
#endif
    // (room for every row the storage has reserved space for, and half as much again when it has to guess: a graph filled
    // by several add calls otherwise outgrew its mirror at every call and rebuilt it from the host -- a quarter of the
    // build time of a 2 M-row graph added in four pieces)
    const int64_t room = std::max<int64_t>(std::max<int64_t>(n + n / 2, 1), H->flat->cap_rows);
    if (H->d_nbr0.bytes < (size_t)std::max<int64_t>(n, 1) * M0 * 4 &&
        H->d_nbr0.ensure((size_t)room * M0 * 4) && H->d_nbr0.ensure((size_t)std::max<int64_t>(n, 1) * M0 * 4))
        return set_err(KNN_ERR_HIP, "hnsw: out of device memory (neighbour lists)");
    // (every row of the mirror is valid: the lists of the linked nodes, "no link" everywhere else -- nodes waiting for their
    // batch, room for rows to come.  Few linked nodes in a large table -- the first device batch of a 10 M-row add call --
    // are scattered into a cleared table instead of uploading gigabytes of empty lists)
    const int64_t rows_dev = (int64_t)(H->d_nbr0.bytes / ((size_t)M0 * 4));
    if (H->d_cnt0.bytes < (size_t)rows_dev && H->d_cnt0.ensure((size_t)rows_dev))
        return set_err(KNN_ERR_HIP, "hnsw: out of device memory (neighbour counts)");
    if ((int64_t)H->linked.size() < n) H->linked.resize((size_t)n, 0);
    const bool sparse = H->linked_count * 8 < n;
    std::vector<uint32_t> who;
    if (sparse) {
        for (int64_t i = 0; i < n; i++)
            if (H->linked[(size_t)i]) who.push_back((uint32_t)i);
        HIP_TRY(hipMemset(H->d_nbr0.p, 0xFF, (size_t)rows_dev * M0 * 4));
        HIP_TRY(hipMemset(H->d_cnt0.p, 0, (size_t)rows_dev));
    } else if (rows_dev > n) {
        HIP_TRY(hipMemset((uint32_t *)H->d_nbr0.p + (size_t)n * M0, 0xFF, (size_t)(rows_dev - n) * M0 * 4));
        HIP_TRY(hipMemset((uint8_t *)H->d_cnt0.p + n, 0, (size_t)(rows_dev - n)));
    }
    const int64_t nl = sparse ? (int64_t)who.size() : n;
    std::vector<uint32_t> flat((size_t)nl * M0);
    std::vector<uint8_t> fills((size_t)nl);
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
    for (int64_t i = 0; i < nl; i++) {
        const int64_t node = sparse ? who[(size_t)i] : i;
        memcpy(flat.data() + (size_t)i * M0, g.list(node, 0), (size_t)M0 * 4);
        fills[(size_t)i] = g.cnt0[(size_t)node];
    }
    if (nl > 0 && !sparse) {
        HIP_TRY(hipMemcpy(H->d_nbr0.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(H->d_cnt0.p, fills.data(), (size_t)nl, hipMemcpyHostToDevice));
    } else if (nl > 0) {
        DevBuf d_who, d_rows, d_fill;
        if (d_who.ensure((size_t)nl * 4) || d_rows.ensure(flat.size() * 4) || d_fill.ensure((size_t)nl)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (mirror upload)");
        HIP_TRY(hipMemcpy(d_who.p, who.data(), (size_t)nl * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_rows.p, flat.data(), flat.size() * 4, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_fill.p, fills.data(), (size_t)nl, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)nl), dim3(64), 0, H->flat->stream, (const uint32_t *)d_who.p, (const uint32_t *)d_rows.p, M0,
                           (int64_t)nl, (uint32_t *)H->d_nbr0.p);
        hipLaunchKernelGGL(scatter_bytes_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, H->flat->stream, (const uint32_t *)d_who.p, (const uint8_t *)d_fill.p,
                           (int64_t)nl, (uint8_t *)H->d_cnt0.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(H->flat->stream));
        d_who.release(); d_rows.release(); d_fill.release();
    }
    // Coarse entry index: the rows of all nodes above level 0 (one in M), copied into a flat index of their
    // own.  A search starts with an EXACT scan of these rows on the flat kernel and enters level 0 at the
    // nearest of them -- the upper levels' greedy descent (a host loop over a few hundred nodes, and a coin toss
    // when cluster centres are equidistant) is replaced by what this GPU is best at.  10 M rows: 312 k coarse
    // rows, 20 ms per 4096 queries.
    if (H->coarse) {
        knn_free(H->coarse);
        H->coarse = nullptr;
    }
    H->ncoarse = 0;
    if (H->coarse2) {
        knn_free(H->coarse2);
        H->coarse2 = nullptr;
    }
    H->coarse2_ids_host.clear();
    H->ncoarse2 = 0;
    std::vector<uint32_t> &up = H->coarse_ids_host;
    up.clear();
    for (int64_t i = 0; i < n; i++) // (nodes still waiting for their batch have no links: never an entry point)
        if (H->linked[(size_t)i] && g.levels[i] >= 1) up.push_back((uint32_t)i);
    H->mirror_count = H->linked_count;
    knn_index_s *f = H->flat;
    if ((int64_t)up.size() >= 64 && H->coarse_entries > 0) {
        if (H->d_coarse_ids.ensure(up.size() * 4)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (coarse ids)");
        HIP_TRY(hipMemcpy(H->d_coarse_ids.p, up.data(), up.size() * 4, hipMemcpyHostToDevice));
        const int dev_before = g_device;
        g_device = f->device; // (knn_flat_create builds on the calling thread's current device)
        int rc = knn_flat_create(f->d, f->metric, &H->coarse);
        g_device = dev_before;
        if (rc) return rc;
        // only the neighbourhood matters for an entry point (the beam's rows are re-scored exactly): the coarse scan
        // multiplies bf16 copies -- 1/16 of the matrix time, half the bytes
        if (H->coarse_bf16) {
            rc = flat_set_approx16(H->coarse);
            if (rc) return rc;
        }
        rc = knn_flat_reserve(H->coarse, (int64_t)up.size());
        if (rc) return rc;
        const int64_t CH = 1 << 18;
        DevBuf tmp;
        if (tmp.ensure((size_t)std::min<int64_t>(CH, (int64_t)up.size()) * f->d * 4)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (coarse rows)");
        for (int64_t i0 = 0; i0 < (int64_t)up.size(); i0 += CH) {
            const int64_t m = std::min<int64_t>(CH, (int64_t)up.size() - i0);
            hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)m), dim3(256), 0, f->stream, f->xb, f->dp, f->d,
                               (const uint32_t *)H->d_coarse_ids.p + i0, m, (float *)tmp.p);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(f->stream));
            rc = knn_flat_add_dev(H->coarse, (const float *)tmp.p, m, nullptr);
            if (rc) { tmp.release(); return rc; }
        }
        tmp.release();
        H->ncoarse = (int64_t)up.size();
        std::vector<uint32_t> up2;
        for (uint32_t node : up)
            if (g.levels[node] >= 2) up2.push_back(node);
        const size_t CH2 = 1 << 17;
        for (size_t i0 = 0; i0 < up2.size(); i0 += CH2) {
            rc = hnsw_coarse2_append(H, std::vector<uint32_t>(up2.begin() + i0, up2.begin() + std::min(up2.size(), i0 + CH2)));
            if (rc) return rc;
        }
    }
    H->nbr0_dirty = false;
    return 0;
}

// after a batch: changed level-0 lists -> device mirror, the batch's nodes above level 0 -> coarse index
static int hnsw_mirror_update(knn_hnsw_s *H, const int64_t *ids, int count, std::vector<uint32_t> &dirty)
{
    const HnswGraph &g = H->g;
    knn_index_s *f = H->flat;
    const int M0 = g.nb_neighbors(0);
    hipStream_t s = f->stream;
    std::sort(dirty.begin(), dirty.end());
    dirty.erase(std::unique(dirty.begin(), dirty.end()), dirty.end());
    const size_t nd = dirty.size();
    if (nd) {
        if (H->h_scatter_ids.ensure(nd * 4) || H->h_scatter_rows.ensure(nd * M0 * 4) || H->d_scatter_ids.ensure(nd * 4) ||
            H->d_scatter_rows.ensure(nd * M0 * 4))
            return set_err(KNN_ERR_HIP, "hnsw: out of memory (mirror update)");
        uint32_t *hi = (uint32_t *)H->h_scatter_ids.p, *hr = (uint32_t *)H->h_scatter_rows.p;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t i = 0; i < (int64_t)nd; i++) {
            hi[i] = dirty[i];
            memcpy(hr + (size_t)i * M0, g.list(dirty[i], 0), (size_t)M0 * 4);
        }
        HIP_TRY(hipMemcpyAsync(H->d_scatter_ids.p, hi, nd * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(H->d_scatter_rows.p, hr, nd * M0 * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(scatter_rows_kernel, dim3((unsigned)nd), dim3(64), 0, s, (const uint32_t *)H->d_scatter_ids.p,
                           (const uint32_t *)H->d_scatter_rows.p, M0, (int64_t)nd, (uint32_t *)H->d_nbr0.p);
        HIP_TRY(hipGetLastError());
    }
    // coarse index: append the batch's nodes above level 0
    std::vector<uint32_t> add;
    for (int i = 0; i < count; i++)
        if (g.levels[ids[i]] >= 1) add.push_back((uint32_t)ids[i]);
    if (!add.empty()) {
        std::vector<uint32_t> &up = H->coarse_ids_host;
        const size_t old = up.size();
        up.insert(up.end(), add.begin(), add.end());
        if (H->d_coarse_ids.bytes < up.size() * 4) {
            // (DevBuf::ensure does not keep contents: the whole id list goes up again, a few hundred KB)
            if (H->d_coarse_ids.ensure(up.size() * 4 + (up.size() * 4) / 2)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (coarse ids)");
            HIP_TRY(hipMemcpyAsync(H->d_coarse_ids.p, up.data(), up.size() * 4, hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(hipMemcpyAsync((uint32_t *)H->d_coarse_ids.p + old, add.data(), add.size() * 4, hipMemcpyHostToDevice, s));
        }
        DevBuf &tmp = H->d_scatter_rows; // (free again: the scatter above is ordered before on this stream)
        if (tmp.ensure(add.size() * (size_t)f->d * 4)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (coarse rows)");
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)add.size()), dim3(256), 0, s, f->xb, f->dp, f->d,
                           (const uint32_t *)H->d_coarse_ids.p + old, (int64_t)add.size(), (float *)tmp.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(s));
        int rc = knn_flat_add_dev(H->coarse, (const float *)tmp.p, (int64_t)add.size(), nullptr);
        if (rc) return rc;
        H->ncoarse = (int64_t)up.size();
        std::vector<uint32_t> add2;
        for (uint32_t node : add)
            if (g.levels[node] >= 2) add2.push_back(node);
        rc = hnsw_coarse2_append(H, add2);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(s)); // (the pinned staging buffers are reused by the next batch)
    H->mirror_count = H->linked_count + count; // (the caller marks the batch linked)
    return 0;
}

template <int NCH, int RB, bool B16 = false>
static int launch_beam(const BeamParams &bp, int grid, size_t lds, hipStream_t s)
{
    HIP_TRY(hipFuncSetAttribute((const void *)hnsw_beam_kernel<NCH, RB, B16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL((hnsw_beam_kernel<NCH, RB, B16>), dim3(grid), dim3(256), lds, s, bp);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The device pipeline shared by search and construction, for m queries already on the device (xq: [m][dp] zero
// padded, xq_raw: [m][d] as the flat index takes them, qn: squared norms): entry points from an exact scan of the
// nodes above level 0 (or, for small graphs, from the host's greedy descent), the level-0 beam of `ef` entries,
// exact re-scoring of the beam, selection of the k best -> D/I and/or sorted keys [m][k] (device pointers).
static int hnsw_beam_pipeline(knn_hnsw_s *H, const float *xq, const float *xq_raw, const float *qn, int64_t m, int ef, int k,
                              float *D_dev, int64_t *I_dev, uint64_t *keys_dev, hipStream_t s)
{
    knn_index_s *f = H->flat;
    const HnswGraph &g = H->g;
    const int64_t n = g.ntotal();
    const int M0 = g.nb_neighbors(0);
    const int R = (ef + 63) / 64;
    const size_t lds = (size_t)4 * R * 64 * 8 + 4 * 64 * 4;
    const int64_t vis_words = ((n + 31) / 32 + 3) / 4 * 4;
    const int rb = H->beam_rows;
    const int max_grid = (rb == 8 && !f->keep16 ? 2 : 4) * std::max(1, f->num_cus); // (workgroups per CU the registers allow)
    int rc;
    if (H->d_entry.ensure((size_t)m * std::max(1, H->coarse_entries) * 4) || H->d_beam_ids.ensure((size_t)m * ef * 4) ||
        H->d_beam_keys.ensure((size_t)m * ef * 8) || H->d_stats.ensure(64))
        return set_err(KNN_ERR_HIP, "hnsw: out of device memory");
    int nentry = 1;
    if (H->coarse && H->ncoarse > 0) {
        // exact nearest nodes above level 0: one scan of the coarse rows on the flat kernel
        nentry = (int)std::min<int64_t>(H->coarse_entries, H->ncoarse);
        if (H->d_coarse_keys.ensure((size_t)m * nentry * 8)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory");
        rc = knn_flat_search_keys_dev(H->coarse, xq_raw, m, nentry, 0, (uint64_t *)H->d_coarse_keys.p, (void *)s);
        if (rc) return rc;
        const int64_t tot = m * nentry;
        hipLaunchKernelGGL(coarse_entries_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, (const uint64_t *)H->d_coarse_keys.p,
                           tot, (const uint32_t *)H->d_coarse_ids.p, (uint32_t *)H->d_entry.p);
        HIP_TRY(hipGetLastError());
    } else {
        // few nodes above level 0 (small graphs): greedy descent on the host graph, GPU distances in lock step
        if (H->h_entry.ensure((size_t)m * 4)) return set_err(KNN_ERR_HIP, "hnsw: out of pinned host memory");
        uint32_t *entry = (uint32_t *)H->h_entry.p;
        if (g.max_level > 0) {
            std::vector<Walker> ws((size_t)m);
            for (int64_t i = 0; i < m; i++) {
                ws[i].qslot = (uint32_t)i;
                ws[i].greedy_until = 0;
                ws[i].stop_level = 0;
                ws[i].descent_only = true;
            }
            rc = hnsw_walk(H, ws, xq, qn, false);
            if (rc) return rc;
            for (int64_t i = 0; i < m; i++) entry[i] = ws[i].cur;
        } else {
            for (int64_t i = 0; i < m; i++) entry[i] = (uint32_t)g.entry;
        }
        HIP_TRY(hipMemcpyAsync(H->d_entry.p, entry, (size_t)m * 4, hipMemcpyHostToDevice, s));
    }
    // rows handed on to the exact re-scoring per query
    int keep = ef, kmin = ef;
    if (k < ef) {
        kmin = std::min(ef, k + std::max(k >> 3, 8));
        keep = std::min(ef, k + std::max(k >> 2, 16));
        if (keep + 8 >= ef) keep = kmin = ef;
    }
    const int grid = (int)std::min<int64_t>((m + 3) / 4, max_grid);
    // Lazy clearing pays when a bitmap (n / 128 sixteen-byte stores) is much longer than what a walk touches (about
    // ef x M0 words at most): graphs of millions of rows.  The bitmaps must then be zero between launches: they are
    // zeroed when (re)allocated or after an eager launch, and every lazy walk leaves its own zero again.
    const int tcap = 16384;
    // (KNN355_HNSW_CLEAR=lazy|eager forces one or the other: tests)
    const char *force = getenv("KNN355_HNSW_CLEAR");
    const bool lazy = force && !strcmp(force, "lazy") ? true : (force && !strcmp(force, "eager") ? false : vis_words / 4 > 2 * (int64_t)ef * M0);
    {
        const size_t need = (size_t)grid * 4 * vis_words * 4;
        const void *before = H->d_vis.p;
        const size_t before_bytes = H->d_vis.bytes;
        if (H->d_vis.ensure(need)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (visited bitmaps)");
        if (H->d_vis.p != before || H->d_vis.bytes != before_bytes) H->vis_zero_bytes = 0;
        if (lazy) {
            if (H->d_touched.ensure((size_t)grid * 4 * tcap * 4)) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (visited lists)");
            if (H->vis_zero_bytes < need) {
                HIP_TRY(hipMemsetAsync(H->d_vis.p, 0, need, s));
                H->vis_zero_bytes = need;
            }
        } else {
            H->vis_zero_bytes = 0; // (an eager launch leaves the last walks' bits behind)
        }
    }
    HIP_TRY(hipMemsetAsync(H->d_stats.p, 0, 16, s));
    BeamParams bp;
    bp.xb = f->xb; bp.yn = f->yn; bp.xq = xq; bp.qn = qn;
    bp.nbr0 = (const uint32_t *)H->d_nbr0.p; bp.entry = (const uint32_t *)H->d_entry.p;
    bp.visited = (uint32_t *)H->d_vis.p; bp.out_ids = (uint32_t *)H->d_beam_ids.p;
    bp.touched = lazy ? (uint32_t *)H->d_touched.p : nullptr; bp.tcap = tcap;
    bp.stats = (unsigned long long *)H->d_stats.p;
    bp.nq = m; bp.n = n; bp.vis_words = vis_words; bp.dp = f->dp; bp.metric = f->metric; bp.M0 = M0; bp.ef = ef; bp.nentry = nentry; bp.keep = keep; bp.kmin = kmin; bp.expand2 = H->beam_expand2;
    const bool b16 = f->keep16 && f->xb16.p != nullptr;
    bp.xb16 = (const uint16_t *)f->xb16.p;
    if (b16) {
        // (eight rows in flight again: a bf16 row is half the registers)
        if (f->dp <= 512) rc = launch_beam<1, 8, true>(bp, grid, lds, s);
        else rc = launch_beam<2, 8, true>(bp, grid, lds, s);
        if (rc) return rc;
    }
    const int nch = (f->dp + 255) / 256;
    if (b16) {
    } else if (rb == 8) {
        if (nch <= 1) rc = launch_beam<1, 8>(bp, grid, lds, s);
        else if (nch <= 2) rc = launch_beam<2, 8>(bp, grid, lds, s);
        else rc = launch_beam<4, 8>(bp, grid, lds, s);
    } else {
        if (nch <= 1) rc = launch_beam<1, 4>(bp, grid, lds, s);
        else if (nch <= 2) rc = launch_beam<2, 4>(bp, grid, lds, s);
        else rc = launch_beam<4, 4>(bp, grid, lds, s);
    }
    if (rc) return rc;
    // exact scores of the beam's rows (the flat scan's chain), then the k best of them, sorted
    const int64_t np = m * keep;
    if (getenv("KNN355_HNSW_KEYS_DIRECT"))
        hipLaunchKernelGGL(beam_keys_kernel, dim3((unsigned)((np + 63) / 64)), dim3(64), 0, s, xq, qn, f->xb, f->yn, f->dp, f->metric, m, keep,
                           (const uint32_t *)H->d_beam_ids.p, (uint64_t *)H->d_beam_keys.p);
    else
        hipLaunchKernelGGL(beam_keys_lds_kernel, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, s, xq, qn, f->xb, f->yn, f->dp, f->metric, m,
                           keep, (const uint32_t *)H->d_beam_ids.p, (uint64_t *)H->d_beam_keys.p);
    HIP_TRY(hipGetLastError());
    SelectParams sp = {};
    sp.in = (const uint64_t *)H->d_beam_keys.p; sp.in_stride = keep; sp.n_fixed = keep; sp.cap = keep;
    sp.nq = m; sp.k = k; sp.metric = f->metric;
    sp.D = D_dev; sp.I = I_dev;
    sp.out_keys = keys_dev; sp.out_stride = k; sp.out_fill = keys_dev ? k : 0;
    return launch_select(sp, s);
}

static inline float host_ord2f(uint32_t o)
{
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    memcpy(&f, &u, 4);
    return f;
}

// the batch being linked on the device: its node ids -> d_bids, its rows gathered into d_bq ([count][dp]; the device path has
// dp == d) and their norms into d_bqn -- the batch's rows are their own queries
static int hnsw_batch_queries(knn_hnsw_s *H, const int64_t *ids, int count, hipStream_t s)
{
    knn_index_s *f = H->flat;
    if (H->d_bids.ensure((size_t)count * 4) || H->d_bq.ensure((size_t)count * f->dp * 4) || H->d_bqn.ensure((size_t)count * 4) ||
        H->h_scatter_ids.ensure((size_t)count * 4))
        return set_err(KNN_ERR_HIP, "hnsw: out of memory (batch rows)");
    uint32_t *hi = (uint32_t *)H->h_scatter_ids.p;
    for (int i = 0; i < count; i++) hi[i] = (uint32_t)ids[i];
    HIP_TRY(hipMemcpyAsync(H->d_bids.p, hi, (size_t)count * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)count), dim3(256), 0, s, f->xb, f->dp, f->dp, (const uint32_t *)H->d_bids.p, (int64_t)count,
                       (float *)H->d_bq.p);
    hipLaunchKernelGGL(gather_f32_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, f->yn, (const uint32_t *)H->d_bids.p, (int64_t)count,
                       (float *)H->d_bqn.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(s)); // (the pinned id list is reused)
    return 0;
}

// construction: level-0 candidates (efConstruction best, ascending) of rows ids[0 .. count) against the frozen graph
static int hnsw_level0_candidates_device(knn_hnsw_s *H, const int64_t *ids, int count, std::vector<std::vector<DistId>> &cand0)
{
    knn_index_s *f = H->flat;
    const int efc = H->efConstruction;
    hipStream_t s = f->stream;
    if (H->d_beam_out.ensure((size_t)count * efc * 8) || H->h_keys.ensure((size_t)count * efc * 8))
        return set_err(KNN_ERR_HIP, "hnsw: out of memory (construction candidates)");
    // the new rows are their own queries: on the device, padded (dp == d here), with their norms
    int rc = hnsw_batch_queries(H, ids, count, s);
    if (rc) return rc;
    const float *xq = (const float *)H->d_bq.p;
    rc = hnsw_beam_pipeline(H, xq, xq, (const float *)H->d_bqn.p, count, efc, efc, nullptr, nullptr, (uint64_t *)H->d_beam_out.p, s);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(H->h_keys.p, H->d_beam_out.p, (size_t)count * efc * 8, hipMemcpyDeviceToHost, s));
    unsigned long long st[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(st, H->d_stats.p, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    H->stat_pairs += (int64_t)st[0];
    H->stat_expansions += (int64_t)st[1];
    const uint64_t *keys = (const uint64_t *)H->h_keys.p;
    cand0.assign((size_t)count, std::vector<DistId>());
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
    for (int i = 0; i < count; i++) {
        std::vector<DistId> &c = cand0[i];
        c.reserve(efc);
        for (int j = 0; j < efc; j++) {
            const uint64_t kk = keys[(size_t)i * efc + j];
            if (kk == KEY_PAD) break;
            c.push_back(DistId(host_ord2f((uint32_t)(kk >> 32)), (uint32_t)kk));
        }
    }
    return 0;
}

// ---------------------------------------------------------------------------
// Construction, level 0, on the device.  What hnsw_insert_batch does on the host for every level -- forward selection,
// forward links, reverse requests sorted by (node, v, from), appended where the node's list has room, pruned otherwise
// -- restated as launches over device arrays for level 0, where all but one link in M live (10 M rows: the candidates'
// download, 16 M staged groups, a host sort of 330 k requests per batch and the dirty rows' upload were 12 of 30 s).
// Same arithmetic (gram_shrink_kernel), same order of the requests, same members per pruning group: the graph is the
// one the host path builds, bit for bit (tests/test_hnsw_gpu.py::test_device_links_build_the_host_links_graph).
// The device's lists ([n][M0], packed to the front, d_cnt0 = fill) are the master copy from then on; the host graph's
// level-0 lists follow when someone reads them (hnsw_host0_sync).
// ---------------------------------------------------------------------------

// groups of the forward selection: [ids[i], the beam's candidates (sorted keys, KEY_PAD behind the last)]; fixed stride
__global__ void dl_fwd_groups_kernel(const uint64_t *__restrict__ keys, int count, int efc, int take, const uint32_t *__restrict__ ids, int M0,
                                     uint32_t *__restrict__ mem, int32_t *__restrict__ goff, int32_t *__restrict__ gcnt, int32_t *__restrict__ maxo)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int stride = take + 1;
    const int i = (int)(t / stride), j = (int)(t % stride);
    if (i >= count) return;
    if (j == 0) {
        mem[(size_t)i * stride] = ids[i];
        int nv = 0;
        while (nv < take && keys[(size_t)i * efc + nv] != KEY_PAD) nv++;
        goff[i] = i * stride;
        gcnt[i] = 1 + nv;
        maxo[i] = M0;
    } else {
        const uint64_t kk = keys[(size_t)i * efc + j - 1];
        mem[(size_t)i * stride + j] = kk == KEY_PAD ? ids[i] : (uint32_t)kk;
    }
}

// roff[0 .. count] = exclusive prefix sums of on[0 .. count) (one workgroup)
__global__ __launch_bounds__(1024) void dl_scan_kernel(const int32_t *__restrict__ on, int count, int32_t *__restrict__ roff)
{
    __shared__ int part[1024];
    const int tid = threadIdx.x;
    const int per = (count + 1023) / 1024;
    const int i0 = min(count, tid * per), i1 = min(count, i0 + per);
    int sum = 0;
    for (int i = i0; i < i1; i++) sum += on[i];
    part[tid] = sum;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) { // (Hillis-Steele, inclusive)
        const int v = tid >= o ? part[tid - o] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - sum;
    for (int i = i0; i < i1; i++) {
        roff[i] = run;
        run += on[i];
    }
    if (tid == 1023) roff[count] = part[1023];
}

// forward links of the batch's points into their (empty) lists, and one reverse request per link: key = (node, v), value = from
__global__ __launch_bounds__(256) void dl_fwd_write_kernel(const uint32_t *__restrict__ oid, const float *__restrict__ od, const int32_t *__restrict__ on,
                                                           const int32_t *__restrict__ roff, int count, const uint32_t *__restrict__ ids, int M0,
                                                           uint32_t *__restrict__ nbr0, uint8_t *__restrict__ cnt0,
                                                           uint64_t *__restrict__ rkey, uint32_t *__restrict__ rfrom)
{
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= count) return;
    const uint32_t pid = ids[i];
    const int n = on[i], base = roff[i];
    for (int c = lane; c < M0; c += 64) {
        const uint32_t id = c < n ? oid[(size_t)i * M0 + c] : HNSW_EMPTY;
        nbr0[(size_t)pid * M0 + c] = id;
        if (c < n) {
            rkey[base + c] = ((uint64_t)id << 32) | f2ord(od[(size_t)i * M0 + c]);
            rfrom[base + c] = pid;
        }
    }
    if (lane == 0) cnt0[pid] = (uint8_t)n;
}

// The reverse requests, sorted by (node, v) and, among equals, by `from` (a stable sort of requests emitted in the order of
// the points): the thread of the first request of a node's run serves the run -- appended behind the node's links when they
// all fit, otherwise the node, its links and the closest new ones (as many as a pruning group holds) become a group.
// ctr[0] groups, ctr[1] members written so far, ctr[2] the largest group.
__global__ void dl_rev_apply_kernel(const uint64_t *__restrict__ rkey, const uint32_t *__restrict__ rfrom, int nrev, int M0,
                                    uint32_t *__restrict__ nbr0, uint8_t *__restrict__ cnt0, uint32_t *__restrict__ ctr,
                                    int32_t *__restrict__ goff, int32_t *__restrict__ gcnt, int32_t *__restrict__ maxo,
                                    uint32_t *__restrict__ gnode, uint32_t *__restrict__ mem)
{
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrev) return;
    const uint32_t node = (uint32_t)(rkey[r] >> 32);
    if (r > 0 && (uint32_t)(rkey[r - 1] >> 32) == node) return;
    int r1 = r + 1;
    while (r1 < nrev && (uint32_t)(rkey[r1] >> 32) == node) r1++;
    const int have = cnt0[node], nnew = r1 - r;
    uint32_t *l = nbr0 + (size_t)node * M0;
    if (have + nnew <= M0) {
        for (int j = 0; j < nnew; j++) l[have + j] = rfrom[r + j];
        cnt0[node] = (uint8_t)(have + nnew);
        return;
    }
    const int take = min(nnew, SHRINK_MAX_MEMBERS - 1 - have);
    const int nm = 1 + have + take;
    const uint32_t g = atomicAdd(&ctr[0], 1u);
    const uint32_t mo = atomicAdd(&ctr[1], (uint32_t)nm);
    atomicMax(&ctr[2], (uint32_t)nm);
    goff[g] = (int32_t)mo;
    gcnt[g] = nm;
    maxo[g] = M0;
    gnode[g] = node;
    mem[mo] = node;
    for (int c = 0; c < have; c++) mem[mo + 1 + c] = l[c];
    for (int j = 0; j < take; j++) mem[mo + 1 + have + j] = rfrom[r + j];
}

// the pruned lists back into place
__global__ __launch_bounds__(256) void dl_prune_write_kernel(const uint32_t *__restrict__ gnode, const uint32_t *__restrict__ oid, const int32_t *__restrict__ on,
                                                             int ngroups, int M0, uint32_t *__restrict__ nbr0, uint8_t *__restrict__ cnt0)
{
    const int g = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (g >= ngroups) return;
    const uint32_t node = gnode[g];
    const int n = min(on[g], M0);
    for (int c = lane; c < M0; c += 64) nbr0[(size_t)node * M0 + c] = c < n ? oid[(size_t)g * M0 + c] : HNSW_EMPTY;
    if (lane == 0) cnt0[node] = (uint8_t)n;
}

// level-0 links of rows ids[0 .. count): candidates from the beam (left on the device), everything else as above
static int hnsw_level0_links_device(knn_hnsw_s *H, const int64_t *ids, int count)
{
    knn_index_s *f = H->flat;
    const HnswGraph &g = H->g;
    const int efc = H->efConstruction;
    const int M0 = g.nb_neighbors(0);
    hipStream_t s = f->stream;
    double tp = now_s();
    (void)tp;
    if (H->d_beam_out.ensure((size_t)count * efc * 8)) return set_err(KNN_ERR_HIP, "hnsw: out of memory (construction candidates)");
    int rc = hnsw_batch_queries(H, ids, count, s); // (the new rows are their own queries: on the device, padded, with their norms)
    if (rc) return rc;
    const float *xq = (const float *)H->d_bq.p;
    rc = hnsw_beam_pipeline(H, xq, xq, (const float *)H->d_bqn.p, count, efc, efc, nullptr, nullptr, (uint64_t *)H->d_beam_out.p, s);
    if (rc) return rc;
#ifdef KNN355_DEV
    HIP_TRY(hipStreamSynchronize(s)); // (developer build: the beam's time apart from the selection's)
    HNSW_PROF(1, tp);
#endif
    const int take = std::min(efc, SHRINK_MAX_MEMBERS - 1);
    const int stride = take + 1;
    const size_t nrev_max = (size_t)count * M0;
    if (H->dl_mem.ensure((size_t)count * stride * 4) || H->dl_goff.ensure((size_t)count * 4) ||
        H->dl_gcnt.ensure((size_t)count * 4) || H->dl_maxo.ensure((size_t)count * 4) ||
        H->dl_oid.ensure((size_t)count * M0 * 4) || H->dl_od.ensure((size_t)count * M0 * 4) ||
        H->dl_on.ensure((size_t)count * 4) || H->dl_roff.ensure((size_t)(count + 1) * 4) || H->dl_ctr.ensure(64) ||
        H->dl_key[0].ensure(nrev_max * 8) || H->dl_key[1].ensure(nrev_max * 8) || H->dl_from[0].ensure(nrev_max * 4) || H->dl_from[1].ensure(nrev_max * 4))
        return set_err(KNN_ERR_HIP, "hnsw: out of device memory (construction, level 0)");
    uint32_t *mem = (uint32_t *)H->dl_mem.p, *nbr0 = (uint32_t *)H->d_nbr0.p, *ctr = (uint32_t *)H->dl_ctr.p;
    uint8_t *cnt0 = (uint8_t *)H->d_cnt0.p;
    int32_t *goff = (int32_t *)H->dl_goff.p, *gcnt = (int32_t *)H->dl_gcnt.p, *maxo = (int32_t *)H->dl_maxo.p;
    // forward selection
    {
        const int64_t tot = (int64_t)count * stride;
        hipLaunchKernelGGL(dl_fwd_groups_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, s, (const uint64_t *)H->d_beam_out.p, count, efc, take,
                           (const uint32_t *)H->d_bids.p, M0, mem, goff, gcnt, maxo);
        HIP_TRY(hipGetLastError());
    }
    ShrinkParams p;
    p.xb = f->xb; p.yn = f->yn; p.dp = f->dp; p.metric = f->metric;
    p.group_off = goff; p.group_cnt = gcnt; p.ngroups = nullptr; p.members = mem; p.max_out = maxo;
    p.out_ids = (uint32_t *)H->dl_oid.p; p.out_d = (float *)H->dl_od.p; p.out_n = (int32_t *)H->dl_on.p; p.out_stride = M0;
    rc = launch_shrink(p, count, stride, s);
    if (rc) return rc;
    // forward links + reverse requests
    hipLaunchKernelGGL(dl_scan_kernel, dim3(1), dim3(1024), 0, s, (const int32_t *)H->dl_on.p, count, (int32_t *)H->dl_roff.p);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(dl_fwd_write_kernel, dim3((unsigned)((count + 3) / 4)), dim3(256), 0, s, (const uint32_t *)H->dl_oid.p, (const float *)H->dl_od.p,
                       (const int32_t *)H->dl_on.p, (const int32_t *)H->dl_roff.p, count, (const uint32_t *)H->d_bids.p, M0, nbr0, cnt0,
                       (uint64_t *)H->dl_key[0].p, (uint32_t *)H->dl_from[0].p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemsetAsync(ctr, 0, 16, s));
    int32_t nrev = 0;
    unsigned long long st[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&nrev, (const int32_t *)H->dl_roff.p + count, 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(st, H->d_stats.p, 16, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    H->stat_pairs += (int64_t)st[0];
    H->stat_expansions += (int64_t)st[1];
    H->stat_shrinks += count;
    HNSW_PROF(2, tp); // forward selection + forward links (device; with the beam's time in a build without KNN355_DEV)
    if (nrev > 0) {
        // (the groups of the forward selection are done with: their arrays now hold the pruning groups -- at most one per
        // request, 1 + M0 members of its own each besides the requests it takes in)
        if (H->dl_mem.ensure((size_t)nrev * (M0 + 2) * 4) || H->dl_goff.ensure((size_t)nrev * 4) || H->dl_gcnt.ensure((size_t)nrev * 4) ||
            H->dl_maxo.ensure((size_t)nrev * 4) || H->dl_gnode.ensure((size_t)nrev * 4))
            return set_err(KNN_ERR_HIP, "hnsw: out of device memory (construction, level 0)");
        mem = (uint32_t *)H->dl_mem.p;
        goff = (int32_t *)H->dl_goff.p; gcnt = (int32_t *)H->dl_gcnt.p; maxo = (int32_t *)H->dl_maxo.p;
        p.group_off = goff; p.group_cnt = gcnt; p.members = mem; p.max_out = maxo;
        // sorted by (node, v); the node's bits that are always zero are left out of the passes
        int node_bits = 1;
        while (node_bits < 32 && (1ll << node_bits) < g.ntotal()) node_bits++;
        size_t tb = 0;
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, tb, (const uint64_t *)H->dl_key[0].p, (uint64_t *)H->dl_key[1].p, (const uint32_t *)H->dl_from[0].p,
                                                   (uint32_t *)H->dl_from[1].p, (int)nrev, 0, 32 + node_bits, s));
        if (H->dl_tmp.ensure(std::max<size_t>(tb, 256))) return set_err(KNN_ERR_HIP, "hnsw: out of device memory (sort)");
        HIP_TRY(hipcub::DeviceRadixSort::SortPairs(H->dl_tmp.p, tb, (const uint64_t *)H->dl_key[0].p, (uint64_t *)H->dl_key[1].p, (const uint32_t *)H->dl_from[0].p,
                                                   (uint32_t *)H->dl_from[1].p, (int)nrev, 0, 32 + node_bits, s));
        hipLaunchKernelGGL(dl_rev_apply_kernel, dim3((unsigned)((nrev + 255) / 256)), dim3(256), 0, s, (const uint64_t *)H->dl_key[1].p, (const uint32_t *)H->dl_from[1].p,
                           (int)nrev, M0, nbr0, cnt0, ctr, goff, gcnt, maxo, (uint32_t *)H->dl_gnode.p, mem);
        HIP_TRY(hipGetLastError());
        uint32_t hc[3] = {0, 0, 0};
        HIP_TRY(hipMemcpyAsync(hc, ctr, 12, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HNSW_PROF(4, tp); // reverse requests sorted and appended (device)
        const int nprune = (int)hc[0];
        if (nprune > 0) {
            if (H->dl_oid.ensure((size_t)std::max(count, nprune) * M0 * 4) || H->dl_od.ensure((size_t)std::max(count, nprune) * M0 * 4) ||
                H->dl_on.ensure((size_t)std::max(count, nprune) * 4))
                return set_err(KNN_ERR_HIP, "hnsw: out of device memory (construction, level 0)");
            p.out_ids = (uint32_t *)H->dl_oid.p; p.out_d = (float *)H->dl_od.p; p.out_n = (int32_t *)H->dl_on.p;
            rc = launch_shrink(p, nprune, (int)hc[2], s);
            if (rc) return rc;
            hipLaunchKernelGGL(dl_prune_write_kernel, dim3((unsigned)((nprune + 3) / 4)), dim3(256), 0, s, (const uint32_t *)H->dl_gnode.p, (const uint32_t *)H->dl_oid.p,
                               (const int32_t *)H->dl_on.p, nprune, M0, nbr0, cnt0);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(s));
            H->stat_shrinks += nprune;
        }
        HNSW_PROF(5, tp); // reverse pruning (device)
    }
    H->host0_stale = true;
    return 0;
}

// the host graph's level-0 lists (and fills) brought up to date from the device's (every row of the mirror is valid)
static int hnsw_host0_sync(knn_hnsw_s *H)
{
    if (!H->host0_stale) return 0;
    HnswGraph &g = H->g;
    knn_index_s *f = H->flat;
    const int M0 = g.nb_neighbors(0);
    const int64_t n = std::min<int64_t>((int64_t)(H->d_nbr0.bytes / ((size_t)M0 * 4)), g.ntotal());
    HIP_TRY(hipSetDevice(f->device));
    const int64_t CH = 1 << 18; // 64 MB of lists per piece at M = 32
    if (n > 0 && (H->h_scatter_rows.ensure((size_t)std::min(CH, n) * M0 * 4) || H->h_scatter_ids.ensure((size_t)std::min(CH, n))))
        return set_err(KNN_ERR_HIP, "hnsw: out of pinned host memory");
    for (int64_t i0 = 0; i0 < n; i0 += CH) {
        const int64_t m = std::min(CH, n - i0);
        HIP_TRY(hipMemcpyAsync(H->h_scatter_rows.p, (const uint32_t *)H->d_nbr0.p + (size_t)i0 * M0, (size_t)m * M0 * 4, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipMemcpyAsync(H->h_scatter_ids.p, (const uint8_t *)H->d_cnt0.p + i0, (size_t)m, hipMemcpyDeviceToHost, f->stream));
        HIP_TRY(hipStreamSynchronize(f->stream));
        const uint32_t *rows = (const uint32_t *)H->h_scatter_rows.p;
        const uint8_t *cn = (const uint8_t *)H->h_scatter_ids.p;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t i = 0; i < m; i++) {
            memcpy(g.list(i0 + i, 0), rows + (size_t)i * M0, (size_t)M0 * 4);
            g.cnt0[i0 + i] = cn[i];
        }
    }
    H->host0_stale = false;
    return 0;
}

// construction: candidates of the levels ABOVE 0.  Every node above level 0 has a row in the coarse index (the flat index the
// searches take their entry points from), so the efConstruction nearest nodes of level >= 1 are ONE exact scan of it --
// no walk at all, and better than a walk's approximation.  Levels >= 2 (one point in M^2 has any): a scan with a large k,
// filtered by level.  Until round 3 these levels were walked on the host with GPU distances in lock step: a third of the
// build time (2 M rows: 2.8 of 8.0 s) went into the thousands of round trips of one point in M.
// `starved` receives the points (members of `up`) for which that large-k scan is NOT enough: on a big graph the best
// KNN_MAX_K coarse rows hold only a handful of the nodes of the highest levels (10 M rows, M = 42: ~240 k coarse rows,
// ~135 nodes of level >= 3 -- about one of them among 2048), a level's list then comes back shorter than
// min(efConstruction, nodes of that level) and a node linked from it would sit (almost) disconnected on that level --
// invisible to the searches that enter through the coarse scan, fatal for FAISS's greedy descent (knn_hnsw_set_entry(H, 0),
// IHNf files read by the real faiss).  The caller walks those points' upper levels on the host, as before round 3: one
// point in M^2 at most, a few hundred in a 10 M-row build (ADVICE r3).
static int hnsw_upper_candidates_device(knn_hnsw_s *H, const int64_t *ids, const std::vector<int> &up, std::vector<std::vector<std::vector<DistId>>> &lc,
                                        std::vector<int> &starved)
{
    knn_index_s *f = H->flat;
    const HnswGraph &g = H->g;
    const int efc = H->efConstruction;
    hipStream_t s = f->stream;
    const int64_t nu = (int64_t)up.size();
    std::vector<int> up2; // positions in `up` of the points with levels >= 2
    for (int64_t j = 0; j < nu; j++)
        if (std::min(g.levels[ids[up[j]]], g.max_level) >= 2) up2.push_back((int)j);
    const int k1 = (int)std::min<int64_t>(efc, H->ncoarse);
    // the levels >= 2 are scanned in their own index once it holds a few rows (one node in M of the coarse index: the large-k scan
    // then reaches 32 times deeper into those levels -- on a 10 M-row graph it is the level-4 nodes that run short, not the level-3 ones)
    const bool own2 = H->coarse2 && H->ncoarse2 >= 64;
    const int64_t n2 = own2 ? H->ncoarse2 : H->ncoarse;
    const int k2 = (int)std::min<int64_t>(KNN_MAX_K, n2);
    const size_t nkeys = (size_t)nu * k1 + up2.size() * (size_t)k2;
    if (H->h_scatter_ids.ensure((size_t)nu * 4) || H->d_scatter_ids.ensure((size_t)nu * 4) || H->d_q.ensure((size_t)nu * f->d * 4) ||
        H->d_beam_out.ensure(nkeys * 8) || H->h_keys.ensure(nkeys * 8))
        return set_err(KNN_ERR_HIP, "hnsw: out of memory (upper-level candidates)");
    uint32_t *uids = (uint32_t *)H->h_scatter_ids.p;
    for (int64_t j = 0; j < nu; j++) uids[j] = (uint32_t)ids[up[j]];
    HIP_TRY(hipMemcpyAsync(H->d_scatter_ids.p, uids, (size_t)nu * 4, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)nu), dim3(256), 0, s, f->xb, f->dp, f->d, (const uint32_t *)H->d_scatter_ids.p, nu,
                       (float *)H->d_q.p);
    HIP_TRY(hipGetLastError());
    uint64_t *dk = (uint64_t *)H->d_beam_out.p;
    int rc = knn_flat_search_keys_dev(H->coarse, (const float *)H->d_q.p, nu, k1, 0, dk, (void *)s);
    if (rc) return rc;
    if (!up2.empty()) {
        // their rows, gathered again behind the first block of queries
        if (H->d_scatter_rows.ensure(up2.size() * 4) || H->h_scatter_rows.ensure(up2.size() * 4) || H->d_qn.ensure(up2.size() * (size_t)f->d * 4))
            return set_err(KNN_ERR_HIP, "hnsw: out of memory (upper-level candidates)");
        uint32_t *ids2 = (uint32_t *)H->h_scatter_rows.p;
        for (size_t j = 0; j < up2.size(); j++) ids2[j] = (uint32_t)ids[up[up2[j]]];
        HIP_TRY(hipMemcpyAsync(H->d_scatter_rows.p, ids2, up2.size() * 4, hipMemcpyHostToDevice, s));
        hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)up2.size()), dim3(256), 0, s, f->xb, f->dp, f->d, (const uint32_t *)H->d_scatter_rows.p,
                           (int64_t)up2.size(), (float *)H->d_qn.p);
        HIP_TRY(hipGetLastError());
        rc = knn_flat_search_keys_dev(own2 ? H->coarse2 : H->coarse, (const float *)H->d_qn.p, (int64_t)up2.size(), k2, 0, dk + (size_t)nu * k1, (void *)s);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(H->h_keys.p, dk, nkeys * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const uint64_t *keys = (const uint64_t *)H->h_keys.p;
    const uint32_t *cid = H->coarse_ids_host.data();
    for (int64_t j = 0; j < nu; j++) {
        const int top = std::min(g.levels[ids[up[j]]], g.max_level);
        auto &mine = lc[(size_t)up[j]];
        mine.resize((size_t)top + 1);
        std::vector<DistId> &c = mine[1];
        c.reserve(k1);
        for (int i = 0; i < k1; i++) {
            const uint64_t kk = keys[(size_t)j * k1 + i];
            if (kk == KEY_PAD) break;
            c.push_back(DistId(host_ord2f((uint32_t)(kk >> 32)), cid[(uint32_t)kk]));
        }
    }
    for (size_t u = 0; u < up2.size(); u++) {
        const int64_t j = up2[u];
        const int top = std::min(g.levels[ids[up[j]]], g.max_level);
        auto &mine = lc[(size_t)up[j]];
        const uint64_t *kr = keys + (size_t)nu * k1 + u * (size_t)k2;
        for (int i = 0; i < k2; i++) {
            if (kr[i] == KEY_PAD) break;
            const uint32_t node = own2 ? H->coarse2_ids_host[(uint32_t)kr[i]] : cid[(uint32_t)kr[i]];
            const int lv = g.levels[node];
            for (int l = 2; l <= std::min(lv, top); l++)
                if ((int)mine[l].size() < efc) mine[l].push_back(DistId(host_ord2f((uint32_t)(kr[i] >> 32)), node));
        }
    }
    static const bool fallback_on = !(getenv("KNN355_HNSW_STARVED_FALLBACK") && atoi(getenv("KNN355_HNSW_STARVED_FALLBACK")) == 0); // (tests: the round-3 behaviour)
    if (fallback_on && !up2.empty() && (int64_t)k2 < n2) {
        // (the scan saw only part of its index) nodes of each level among ALL coarse rows
        std::vector<int64_t> at_least((size_t)g.max_level + 2, 0);
        for (int64_t c = 0; c < H->ncoarse; c++) at_least[(size_t)std::min(g.levels[cid[c]], g.max_level)]++;
        for (int l = g.max_level - 1; l >= 0; l--) at_least[(size_t)l] += at_least[(size_t)l + 1];
        for (size_t u = 0; u < up2.size(); u++) {
            const int64_t j = up2[u];
            auto &mine = lc[(size_t)up[j]];
            bool short_list = false;
            for (int l = 2; l < (int)mine.size(); l++)
                short_list |= (int64_t)mine[l].size() < std::min<int64_t>(efc, at_least[(size_t)l]);
            if (short_list) starved.push_back(up[j]);
        }
    }
    return 0;
}

// Search on the device: queries up, the pipeline above, results down.
static int hnsw_search_device(knn_hnsw_s *H, const float *q_host, int64_t nq, int64_t k, int ef, float *D_host, int64_t *I_host)
{
    knn_index_s *f = H->flat;
    int rc = 0;
    if (H->nbr0_dirty || H->mirror_count != H->linked_count) {
        rc = hnsw_upload_graph(H);
        if (rc) return rc;
    }
    const int64_t B = 16384;
    const int64_t mb = std::min(nq, B);
    const int64_t nbatches = (nq + B - 1) / B;
    // Several batches: two sets of result buffers, and while batch b is walked the results of batch b - 1 go down on the
    // device's copy stream (ResultPipe; the reference's run, all-vs-all k = 1000: 200 MB per batch -- an eighth of the
    // batch's time when it waited its turn on the search's own stream)
    PipeLease lease;
    rc = lease_pipes(f->device, nbatches > 1, lease);
    if (rc) return rc;
    const bool piped = lease.cp != nullptr;
    DevBuf *dD[2] = {&H->d_D, &H->d_D2}, *dI[2] = {&H->d_I, &H->d_I2};
    if (H->d_q.ensure((size_t)mb * f->dp * 4) || H->d_qn.ensure((size_t)mb * 4) || f->ws_tmp2.ensure((size_t)mb * f->d * 4) ||
        H->d_D.ensure((size_t)mb * k * 4) || H->d_I.ensure((size_t)mb * k * 8) || H->d_st2.ensure(64) ||
        (piped && (H->d_D2.ensure((size_t)mb * k * 4) || H->d_I2.ensure((size_t)mb * k * 8))))
        return set_err(KNN_ERR_HIP, "hnsw_search: out of device memory");
    hipStream_t s = f->stream;
    const ResultPipe rp{lease.cp, s, "hnsw_search: "};
    std::vector<unsigned long long> st((size_t)nbatches * 2, 0ull);
    // batch b: queries up, the pipeline above into the result buffers of `slot`, the walk's counters kept beside them
    auto walk = [&](int64_t b, int slot) -> int {
        const int64_t b0 = b * B, m = std::min(B, nq - b0);
        int r = rp.hip(hipMemcpyAsync(f->ws_tmp2.p, q_host + b0 * f->d, (size_t)m * f->d * 4, hipMemcpyHostToDevice, s));
        if (!r) r = pad_rows_dev((const float *)f->ws_tmp2.p, m, f->d, (float *)H->d_q.p, f->dp, s);
        if (!r) r = norms_dev_impl((const float *)H->d_q.p, m, f->d, f->dp, (float *)H->d_qn.p, s);
        if (!r)
            r = hnsw_beam_pipeline(H, (const float *)H->d_q.p, (const float *)f->ws_tmp2.p, (const float *)H->d_qn.p, m, ef, (int)k,
                                   (float *)dD[slot]->p, (int64_t *)dI[slot]->p, nullptr, s);
        if (!r) r = rp.hip(hipMemcpyAsync((char *)H->d_st2.p + slot * 16, H->d_stats.p, 16, hipMemcpyDeviceToDevice, s));
        return r;
    };
    // results (and the walk's counters) of batch b: device -> host, on `on`
    auto copy = [&](int64_t b, int slot, hipStream_t on) -> hipError_t {
        const int64_t b0 = b * B, m = std::min(B, nq - b0);
        hipError_t r = hipMemcpyAsync(D_host + b0 * k, dD[slot]->p, (size_t)m * k * 4, hipMemcpyDeviceToHost, on);
        if (r == hipSuccess) r = hipMemcpyAsync(I_host + b0 * k, dI[slot]->p, (size_t)m * k * 8, hipMemcpyDeviceToHost, on);
        if (r == hipSuccess) r = hipMemcpyAsync(&st[(size_t)b * 2], (const char *)H->d_st2.p + slot * 16, 16, hipMemcpyDeviceToHost, on);
        return r;
    };
    for (int64_t b = 0; b < nbatches && !rc; b++) {
        rc = rp.before(b);
        if (!rc) rc = walk(b, rp.slot(b));
        if (!rc) rc = rp.after(b, copy);
    }
    rc = rp.finish(rc, nbatches, copy);
    if (rc) return rc;
    for (int64_t b = 0; b < nbatches; b++) {
        H->stat_pairs += (int64_t)st[(size_t)b * 2];
        H->stat_rounds += 1;
        H->stat_expansions += (int64_t)st[(size_t)b * 2 + 1];
    }
    return 0;
}

extern "C" int knn_hnsw_search(knn_hnsw_s *H, const float *q_host, int64_t nq, int64_t k, float *D_host, int64_t *I_host)
{
    if (!H) return set_err(KNN_ERR_INVALID, "hnsw_search: null handle");
    if (nq < 0 || k < 1) return set_err(KNN_ERR_INVALID, "hnsw_search: bad shape");
    if (nq == 0) return 0;
    if (!q_host || !D_host || !I_host) return set_err(KNN_ERR_INVALID, "hnsw_search: null pointer");
    std::lock_guard<std::mutex> lk(H->mu);
    knn_index_s *f = H->flat;
    HIP_TRY(hipSetDevice(f->device));
    const float pad = f->metric == KNN_METRIC_INNER_PRODUCT ? -FLT_MAX : FLT_MAX;
    const int ef = (int)std::max<int64_t>(H->efSearch, k);
    if (H->g.ntotal() == 0) {
        fill_empty_host(D_host, I_host, nq * k, f->metric);
        return 0;
    }
    // the device beam serves rows of up to 1024 floats, beams of up to 1024 entries and 2^31 rows
    static const bool host_beam = getenv("KNN355_HNSW_HOST_BEAM") && atoi(getenv("KNN355_HNSW_HOST_BEAM")) != 0;
    if (H->device_beam && !host_beam && f->dp <= 1024 && ef <= 1024 && k <= KNN_MAX_K && H->g.ntotal() < (1ll << 31))
        return hnsw_search_device(H, q_host, nq, k, ef, D_host, I_host);
    if (H->host0_stale) { // (the host walkers read level 0)
        int rc0 = hnsw_host0_sync(H);
        if (rc0) return rc0;
    }
    const int64_t B = H->max_batch;
    if (H->d_q.ensure((size_t)std::min(nq, B) * f->dp * 4) || H->d_qn.ensure((size_t)std::min(nq, B) * 4) ||
        f->ws_tmp2.ensure((size_t)std::min(nq, B) * f->d * 4))
        return set_err(KNN_ERR_HIP, "hnsw_search: out of device memory");
    for (int64_t b0 = 0; b0 < nq; b0 += B) {
        const int64_t m = std::min(B, nq - b0);
        hipStream_t s = f->stream;
        HIP_TRY(hipMemcpyAsync(f->ws_tmp2.p, q_host + b0 * f->d, (size_t)m * f->d * 4, hipMemcpyHostToDevice, s));
        int rc = pad_rows_dev((const float *)f->ws_tmp2.p, m, f->d, (float *)H->d_q.p, f->dp, s);
        if (rc) return rc;
        rc = norms_dev_impl((const float *)H->d_q.p, m, f->d, f->dp, (float *)H->d_qn.p, s);
        if (rc) return rc;
        std::vector<Walker> ws((size_t)m);
        for (int64_t i = 0; i < m; i++) {
            ws[i].qslot = (uint32_t)i;
            ws[i].ef = ef;
            ws[i].greedy_until = 0;
            ws[i].stop_level = 0;
        }
        rc = hnsw_walk(H, ws, (const float *)H->d_q.p, (const float *)H->d_qn.p, false);
        if (rc) return rc;
#pragma omp parallel for schedule(static) num_threads(hnsw_threads())
        for (int64_t i = 0; i < m; i++) {
            const auto &W = ws[i].W; // sorted ascending by (v, id)
            float *Dq = D_host + (b0 + i) * k;
            int64_t *Iq = I_host + (b0 + i) * k;
            for (int64_t j = 0; j < k; j++) {
                if (j < (int64_t)W.size()) {
                    Dq[j] = f->metric == KNN_METRIC_INNER_PRODUCT ? -W[j].first : W[j].first;
                    Iq[j] = W[j].second;
                } else {
                    Dq[j] = pad;
                    Iq[j] = -1;
                }
            }
        }
    }
    return 0;
}

// graph export / import (serialisation, tests)
extern "C" int knn_hnsw_graph_sizes(knn_hnsw_s *H, int64_t *ntotal, int64_t *nslots, int32_t *nlevels_tab)
{
    if (!H) return set_err(KNN_ERR_INVALID, "null handle");
    if (ntotal) *ntotal = H->g.ntotal();
    if (nslots) *nslots = (int64_t)H->g.nbrs.size();
    if (nlevels_tab) *nlevels_tab = (int32_t)H->g.cum_nb.size();
    return 0;
}
extern "C" int knn_hnsw_graph_export(knn_hnsw_s *H, int32_t *levels, int64_t *offsets, int32_t *nbrs, int32_t *cum_nb,
                                     double *assign_probas)
{
    if (!H) return set_err(KNN_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(H->mu);
    if (H->host0_stale) {
        int rc0 = hnsw_host0_sync(H);
        if (rc0) return rc0;
    }
    const HnswGraph &g = H->g;
    for (size_t i = 0; i < g.levels.size(); i++) levels[i] = g.levels[i];
    for (size_t i = 0; i < g.offsets.size(); i++) offsets[i] = (int64_t)g.offsets[i];
    for (size_t i = 0; i < g.nbrs.size(); i++) nbrs[i] = g.nbrs[i] == HNSW_EMPTY ? -1 : (int32_t)g.nbrs[i];
    for (size_t i = 0; i < g.cum_nb.size(); i++) cum_nb[i] = g.cum_nb[i];
    if (assign_probas)
        for (size_t i = 0; i < g.assign_probas.size(); i++) assign_probas[i] = g.assign_probas[i];
    return 0;
}
// storage rows must already be in place (knn_hnsw_storage + knn_flat_add)
extern "C" int knn_hnsw_graph_import(knn_hnsw_s *H, int64_t ntotal, const int32_t *levels, const int32_t *nbrs, int64_t nslots,
                                     int32_t max_level, int64_t entry_point)
{
    if (!H) return set_err(KNN_ERR_INVALID, "null handle");
    std::lock_guard<std::mutex> lk(H->mu);
    HnswGraph &g = H->g;
    if (g.ntotal() != 0) return set_err(KNN_ERR_INVALID, "hnsw_graph_import: graph not empty");
    if (ntotal != H->flat->ntotal) return set_err(KNN_ERR_INVALID, "hnsw_graph_import: storage holds a different number of rows");
    // every refusal from here on leaves the graph empty
    auto refuse = [&](const char *why) {
        const int M = g.M;
        g = HnswGraph();
        g.init(M);
        return set_err(KNN_ERR_INVALID, why);
    };
    for (int64_t i = 0; i < ntotal; i++) {
        if (levels[i] < 0 || levels[i] + 1 >= (int)g.cum_nb.size()) return refuse("hnsw_graph_import: bad level");
        g.append_node(levels[i]);
    }
    if ((int64_t)g.nbrs.size() != nslots) return refuse("hnsw_graph_import: neighbour table size mismatch");
    for (int64_t i = 0; i < nslots; i++) {
        if (nbrs[i] >= ntotal || nbrs[i] < -1) return refuse("hnsw_graph_import: neighbour id out of range");
        g.nbrs[i] = nbrs[i] < 0 ? HNSW_EMPTY : (uint32_t)nbrs[i];
    }
    // a walk at level l >= 1 reads list(node, l) of every node it is handed there: a node named at a level it does not have
    // owns no such slots, and the read would run into the next node's (past the table's end for the last node).  Every slot
    // counts, the ones behind a hole too: construction appends to these lists.
    for (int64_t i = 0; i < ntotal; i++)
        for (int l = 1; l <= g.levels[i]; l++) {
            const uint32_t *ul = g.list(i, l);
            for (int c = 0; c < g.nb_neighbors(l); c++)
                if (ul[c] != HNSW_EMPTY && g.levels[ul[c]] < l)
                    return refuse("hnsw_graph_import: an upper-level list names a node that does not have that level");
        }
    // (an imported list may have holes: the fill is the position of the first one, as in FAISS, whose walk stops at the
    // first -1.  What lies behind it is not part of the list and is dropped here: the device beam reads a level-0 list as
    // one whole row and tells links from empty slots by value, so ids left behind a hole would be walked on the device and
    // not on the host)
    for (int64_t i = 0; i < ntotal; i++) {
        uint32_t *l = g.list(i, 0);
        const int cap = g.nb_neighbors(0);
        int have = 0;
        while (have < cap && l[have] != HNSW_EMPTY) have++;
        g.cnt0[i] = (uint8_t)have;
        for (int c = have; c < cap; c++) l[c] = HNSW_EMPTY;
    }
    // the walk starts at (entry_point, max_level): both must describe a node of this graph
    const bool empty_ok = ntotal == 0 && entry_point == -1;
    if (!empty_ok && (entry_point < 0 || entry_point >= ntotal || max_level != g.levels[entry_point]))
        return refuse("hnsw_graph_import: entry point / max level do not match the level table");
    g.max_level = ntotal ? max_level : -1;
    g.entry = entry_point;
    H->nbr0_dirty = true;
    H->linked.assign((size_t)ntotal, 1);
    H->linked_count = ntotal;
    return 0;
}

extern "C" int knn_hnsw_stats(knn_hnsw_s *H, int64_t *pairs, int64_t *rounds, int64_t *shrinks, double *gpu_s, double *host_s,
                              int32_t reset)
{
    if (!H) return set_err(KNN_ERR_INVALID, "null handle");
    if (pairs) *pairs = H->stat_pairs;
    if (rounds) *rounds = H->stat_rounds;
    if (shrinks) *shrinks = H->stat_shrinks;
    if (gpu_s) *gpu_s = H->stat_gpu_s;
    if (host_s) *host_s = H->stat_host_s;
    if (reset) { H->stat_pairs = H->stat_rounds = H->stat_shrinks = 0; H->stat_gpu_s = H->stat_host_s = 0; }
    return 0;
}
