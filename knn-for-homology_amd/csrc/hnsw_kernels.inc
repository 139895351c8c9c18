// hnsw_kernels.inc -- faiss.IndexHNSWFlat on MI355X, part 1 of 6: every kernel (included by knn355_lib.hip).
// hnsw_kernels.inc (device code) -> hnsw_graph.h (the host graph, free of HIP) -> hnsw_state.inc (the handle, the knobs)
// -> hnsw_build.inc (construction, the device pipeline) -> hnsw_search.inc -> hnsw_api.inc (the other exported entries).
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

#include <hipcub/hipcub.hpp>
#include "hnsw_graph.h" // HNSW_EMPTY

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
