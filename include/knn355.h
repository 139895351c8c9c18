/*
 * knn355.h -- C ABI of libknn355.so, the MI355X (gfx950) kNN hot path.
 *
 * The reference (konstin/knn-for-homology) has no FFI layer of its own on this
 * path: its boundary is the slice of the `faiss` Python module it calls.  Every
 * entry point below names the faiss call it stands in for and the reference
 * call sites (paths relative to the reference repository root).
 *
 * Conventions
 *   - plain C, no C++/torch types; all matrices row-major, C-contiguous float32
 *   - "host" functions take host pointers and copy (the caller keeps ownership,
 *     nothing is retained past return); "_dev" functions take device pointers
 *     on the index's device and an optional hipStream_t passed as void*
 *     (NULL = the library's own stream, synchronised before return)
 *   - return 0 on success, negative on error; knn_last_error() gives the
 *     thread-local message.  No exceptions or abort() cross the ABI.
 *   - there is NO CPU fallback: without a usable HIP device every compute
 *     entry point fails with KNN_ERR_NO_DEVICE.
 *   - calls on different handles may run concurrently; calls on one handle
 *     are serialised internally.
 */
#ifndef KNN355_H
#define KNN355_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* faiss.METRIC_INNER_PRODUCT / faiss.METRIC_L2 (cath/search.py:14,31-32;
 * seqvec_search/main.py:26) */
#define KNN_METRIC_INNER_PRODUCT 0
#define KNN_METRIC_L2 1

#define KNN_OK 0
#define KNN_ERR_INVALID (-1)
#define KNN_ERR_NO_DEVICE (-2)
#define KNN_ERR_HIP (-3)
#define KNN_ERR_UNSUPPORTED (-4)
#define KNN_ERR_IO (-5)
#define KNN_ERR_TIMEOUT (-6) /* a bounded wait of the multi-GPU path ran out (knn_comm_create, knn_sharded_search_dev) */

/* largest k the fused top-k supports (the reference uses k <= 1000:
 * pfam/proteins_search.py:49) */
#define KNN_MAX_K 2048

typedef struct knn_index_s *knn_handle;

/* ---- library ---------------------------------------------------------- */
const char *knn_last_error(void);
const char *knn_version(void);
/* number of visible HIP devices (0 if none); never initialises a context */
int knn_device_count(void);
/* freed index storage and scratch buffers are kept in a per-device pool (<= 8 GiB) for the
 * next index; knn_trim() returns them to the driver and reports the bytes released */
int64_t knn_trim(void);
/* page-locked host memory (hipHostMalloc) for result arrays: a search result is downloaded into it
 * by one DMA at PCIe line rate; into pageable memory the runtime stages the copy.  The faiss-shaped
 * facade allocates large D / I arrays here (numpy arrays over a small pool).  NULL on failure. */
void *knn_host_alloc(int64_t bytes);
void knn_host_free(void *p);
/* selects the device used by indexes created afterwards by this thread and
 * lazily creates its context (fork safe: nothing happens at load time;
 * cath/compare_seqvec_layer.py:58-64 calls search from forked workers) */
int knn_init(int device);

/* ---- faiss.normalize_L2(x) --------------------------------------------
 * in place; rows with zero norm untouched.  cath/search.py:19,
 * pfam/proteins_search.py:22, seqvec_search/main.py:31,34, pfam/search.py:18,20,
 * pfam/slices/slices_search.py:18 */
int knn_normalize_l2(float *x_host, int64_t n, int32_t d);
int knn_normalize_l2_dev(float *x_dev, int64_t n, int32_t d, void *stream);

/* ---- faiss.IndexFlat(d, metric) ----------------------------------------
 * cath/search.py:20, pfam/proteins_search.py:24, seqvec_search/main.py:35,
 * pfam/search.py:44, pfam/slices/slices_search.py:19 */
int knn_flat_create(int32_t d, int32_t metric, knn_handle *out);
/* index.add(x): appends n rows (ids = insertion order).  cath/search.py:22,
 * pfam/proteins_search.py:37, seqvec_search/main.py:39 */
int knn_flat_add(knn_handle h, const float *x_host, int64_t n);
int knn_flat_add_dev(knn_handle h, const float *x_dev, int64_t n, void *stream);
/* index.search(x, k) -> D float32 [nq,k], I int64 [nq,k], best first;
 * unfilled slots: I=-1, D=-FLT_MAX (IP) / +FLT_MAX (L2).
 * Squared L2 follows FAISS's two formulas [ext: knn_L2sqr, distance_compute_blas_threshold = 20]: a call with
 * fewer than 20 queries returns sum (x - y)^2, a larger one max(0, |x|^2 + |y|^2 - 2<x,y>).
 * cath/search.py:24, pfam/proteins_search.py:49, seqvec_search/main.py:45,
 * pfam/search.py:51, pfam/slices/slices_search.py:28 */
int knn_flat_search(knn_handle h, const float *q_host, int64_t nq, int64_t k, float *D_host,
                    int64_t *I_host);
int knn_flat_search_dev(knn_handle h, const float *q_dev, int64_t nq, int64_t k, float *D_dev,
                        int64_t *I_dev, void *stream);
/* All-vs-all without the round trips: the reference searches the very array it
 * just added (cath/search.py:22-24 index.add(embeddings); index.search(embeddings,
 * hits + 1); pfam/proteins_search.py:37,49).  knn_flat_search_self uses rows
 * [row0, row0 + nrows) of the index, already resident and padded, as the queries --
 * same results as knn_flat_search on those rows, no query upload.
 * knn_flat_normalize_rows L2-normalises the stored rows in place on the device
 * (cath/search.py:17-19 normalises a private copy before add: add the raw rows,
 * normalise them here, and the caller's array stays untouched as in the reference). */
int knn_flat_search_self(knn_handle h, int64_t row0, int64_t nrows, int64_t k, float *D_host,
                         int64_t *I_host);
/* A self-search of the WHOLE index (row0 = 0, nrows = ntotal) multiplies only the score tiles on and
 * above the diagonal: dot(x, y) = dot(y, x) bit for bit, so the tile of (query tile I, database tile J)
 * also serves (query tile J, database tile I) -- half the matrix work, the same bits.  Results of 32 MB
 * or more reach D_host / I_host in groups of query tiles (four; eight from 256 MB on) while the later
 * groups are still being multiplied: the arrays are complete when the call returns, not before.
 * knn_flat_search_self_dev: the same search with the results left on the device (synchronous). */
int knn_flat_search_self_dev(knn_handle h, int64_t k, float *D_dev, int64_t *I_dev);
int knn_flat_normalize_rows(knn_handle h);
/* A second handle on the same device-resident rows with its own stream and scratch
 * memory (read-only: add/reset/reserve/normalize_rows fail on it; it sees the rows present
 * when it was made and must be freed before its parent).  A view goes STALE when its
 * parent's storage moves: an add or reserve beyond the parent's capacity, a reset, the
 * parent being freed (an add that fits the capacity leaves it alive, with its old row
 * count; knn_flat_normalize_rows leaves it alive and it sees the new values).  Every call
 * that reads rows refuses a stale view with KNN_ERR_INVALID before anything is copied or
 * launched, the output arrays untouched: knn_flat_search / _dev / _keys_dev / _self /
 * _self_dev, knn_sharded_search_dev, knn_flat_range_search / _self, knn_flat_refine,
 * knn_lsh_search_refine (its flat handle), knn_gather_distances (an empty candidate list
 * included), knn_flat_reconstruct, knn_flat_read_rate.  A view of a view: a stale parent
 * view is refused (KNN_ERR_INVALID); a live one yields a view of the same rows that goes
 * stale together with it.  Two searches on a handle and
 * its view overlap on the GPU -- the small launches at either end of one search (seed
 * sample, merges, the multi-GPU all-gather) hide behind the other one's scan.  FAISS's
 * GPU flat index does the same with two streams; the reference's CPU path has no
 * equivalent (seqvec_search/main.py:45 index.search is one blocking call). */
int knn_flat_view(knn_handle parent, knn_handle *out);
/* per-shard result as packed sortable keys (uint64: order-preserving score
 * bits << 32 | id_base + local row), k per query, ascending = best first,
 * padded with UINT64_MAX.  This is what ranks exchange (RCCL all-gather).
 * The id is 32 bits wide: id_base + ntotal must not exceed 2^32 (the last row's id is then at
 * most 0xFFFFFFFF); a larger sum is refused with KNN_ERR_INVALID before anything is launched. */
int knn_flat_search_keys_dev(knn_handle h, const float *q_dev, int64_t nq, int64_t k,
                             uint32_t id_base, uint64_t *keys_dev, void *stream);
/* merges nlists key lists per query ([nlists][nq][k], e.g. an all-gather
 * buffer) into final D/I on h's device, in h's metric: ONE selection launch that reads the
 * buffer in place whatever nlists * k is -- no scratch memory, nothing of h is written (h
 * supplies the device and the metric only), so merges issued through different handles or
 * streams cannot interfere.  The keys of one query are distinct (every list draws its ids from
 * its own range); the result is unspecified for duplicate keys. */
int knn_merge_keys_dev(knn_handle h, const uint64_t *keys_dev, int32_t nlists, int64_t nq, int64_t k,
                       float *D_dev, int64_t *I_dev, void *stream);
/* ---- index.range_search(x, radius) (FAISS's other flat-index query) ----------
 * Every row whose score beats the radius.  FAISS is not part of the reference tree: the
 * rules below are restated from FAISS 1.7.2's utils/distances.cpp (range_search_inner_product,
 * range_search_L2sqr) and python/class_wrappers.py.
 *   - inner product keeps score > radius; squared L2 (no sqrt) keeps score < radius.  Both are
 *     strict: a score equal to the radius is excluded.  A NaN radius keeps nothing; -inf (IP) /
 *     +inf (L2) keeps every row with a finite score.
 *   - scores are the bits knn_flat_search returns for the same (query, row), including the
 *     small-batch squared-L2 rule (fewer than 20 queries in the batch -- or in the batch announced
 *     by knn_flat_set_batch -- sum (x - y)^2, otherwise max(0, |x|^2 + |y|^2 - 2<x,y>)).
 *   - the results of query i are entries lims[i] .. lims[i+1] - 1, in ascending row id (the order
 *     FAISS's exhaustive scan appends in); no cap per query other than memory.
 * knn_flat_range_search runs the search, writes lims_host[nq + 1] (size_t in FAISS's wrapper) and
 * keeps the lims[nq] results in host memory of the handle; knn_flat_range_fetch copies them to
 * D_host (float32) / I_host (int64) and releases them -- call it once behind every search (the next
 * range search on the handle replaces results not fetched).  ntotal = 0 or nq = 0: all lims 0.
 * knn_flat_range_search_self: the same search with rows [row0, row0 + nrows) of the index as the
 * queries (no upload; identical results to knn_flat_range_search on those rows).
 * Hot path: range_scan_kernel (range.inc), the flat scan's MFMA tile with a threshold-and-compact
 * epilogue; the host reads the per-(query, chunk) counts, then copies the runs into place. */
int knn_flat_range_search(knn_handle h, const float *q_host, int64_t nq, float radius, uint64_t *lims_host);
int knn_flat_range_search_self(knn_handle h, int64_t row0, int64_t nrows, float radius, uint64_t *lims_host);
int knn_flat_range_fetch(knn_handle h, float *D_host, int64_t *I_host);
/* pre-sizes the device storage for nrows rows (faiss has no equivalent; avoids
 * regrowth copies when a shard is filled by several add calls) */
int knn_flat_reserve(knn_handle h, int64_t nrows);
/* index.ntotal / index.d / index.metric_type */
int64_t knn_ntotal(knn_handle h);
int32_t knn_dim(knn_handle h);
int32_t knn_metric(knn_handle h);
int32_t knn_device_of(knn_handle h);
/* index.reset() */
int knn_reset(knn_handle h);
/* copies rows [i0, i0+n) back to the host (index.reconstruct_n; used by
 * write_index and by the HNSW builder) */
int knn_flat_reconstruct(knn_handle h, int64_t i0, int64_t n, float *out_host);
void knn_free(knn_handle h);

/* ---- several GPUs without torch: RCCL inside the library -------------------------
 * The reference has no multi-device code; the north star asks for a database
 * row-sharded over the GPUs of a node with one all-gather of the per-shard top-k.  One process
 * per GPU: rank 0 makes a unique id and hands it to the other ranks (a file, MPI, a socket --
 * the caller's business), every rank creates its communicator, and knn_sharded_search_dev runs
 * local scan -> ncclAllGather of the [nq][k] packed keys -> selection on one stream; the result
 * (global ids: id_base + local row) is the same on every rank and does not depend on the number
 * of shards.  librccl is dlopen'ed on first use.  (Python callers can use torch.distributed
 * instead: knn_for_homology_amd.sharded.)
 * One search at a time per communicator: its key / gather buffers are reused, a call on another
 * stream waits (on the GPU) for the previous call's selection.  Two searches in flight need two
 * communicators.  A rank whose local scan fails still enters the all-gather with "no rows" so
 * that its peers do not deadlock, and returns its error: a failure on ANY rank is a failure of
 * the search -- exchange the return codes before trusting a result.
 * Global ids are 32 bits wide: a rank whose id_base + ntotal exceeds 2^32 fails in exactly that way
 * (KNN_ERR_INVALID from its local scan, after the all-gather it entered with "no rows").
 * Bounded waits: knn_comm_create gives a peer KNN355_COMM_TIMEOUT_S seconds (environment; default 120) to
 * arrive, the synchronous form of knn_sharded_search_dev (stream == NULL) gives the search the same time to
 * complete; both return KNN_ERR_TIMEOUT with the rank named in knn_last_error() instead of hanging, and the
 * communicator is unusable afterwards (free it). */
typedef struct knn_comm_s *knn_comm;
int knn_comm_unique_id(uint8_t *id128);
int knn_comm_create(const uint8_t *id128, int32_t world, int32_t rank, int32_t device, knn_comm *out);
void knn_comm_free(knn_comm c);
int knn_sharded_search_dev(knn_handle h, knn_comm c, const float *q_dev, int64_t nq, int64_t k,
                           uint32_t id_base, float *D_dev, int64_t *I_dev, void *stream);

/* ---- faiss.IndexHNSWFlat(d, M, metric) ------------------------------------
 * pfam/proteins_search.py:27-31 (M = 42, inner product, hnsw.efSearch = 256),
 * .train (no-op) / .add :35-37, .search(x, 1000) :49.  The levels above 0 live on the host;
 * the level-0 lists live on the device (the host copy is brought up to date when the graph is
 * exported or walked on the host).  A search runs on the device: an exact scan of the
 * rows of all nodes above level 0 picks the entry points (knn_hnsw_set_entry; 0 = FAISS's
 * greedy descent through the upper levels, on the host), one wave per query walks level 0
 * with a beam of ef = max(efSearch, k) entries, and the beam's rows are re-scored with the
 * flat search's arithmetic: every returned distance carries the flat index's bits (squared L2:
 * the sum of squared differences at every batch size, as FAISS's HNSW distance computer --
 * the bits a flat search of fewer than 20 queries returns).
 * Construction is batch-synchronous and deterministic; the rows of an add call are linked in a
 * shuffled order (FAISS shuffles too: rows grouped by family must not be inserted blind to their
 * own neighbours).  Level-0 candidates from the same
 * device pipeline and -- since round 4 -- level-0 selection, links, reverse links and pruning
 * on the device as well (the host path's graph, bit for bit; KNN355_HNSW_HOST_LINKS=1 is that
 * path), the candidates of the levels above from exact scans of the coarse index
 * (points whose highest levels that scan cannot fill fall back to host walkers with GPU
 * distances; knn_gather_distances is that offload as a public entry).
 * Results use the flat index's layout; slots the walk could not fill hold id -1. */
typedef struct knn_hnsw_s *knn_hnsw_handle;
int knn_hnsw_create(int32_t d, int32_t M, int32_t metric, knn_hnsw_handle *out);
/* index.hnsw.efSearch / index.hnsw.efConstruction (values <= 0 leave the setting alone).  efConstruction is the
 * width of the beam that collects a new row's candidates (up to 1024 on the device, host walkers above); the
 * closest 127 of them, by the walk's key, take part in the neighbour selection */
int knn_hnsw_set_ef(knn_hnsw_handle h, int32_t efSearch, int32_t efConstruction);
/* walk tuning (not in faiss): candidates expanded per walker per lock-step round (default 8;
 * 1 = strict best-first) and walkers / inserted rows per batch (default 16384); values <= 0 keep the setting */
int knn_hnsw_set_walk(knn_hnsw_handle h, int32_t expand, int32_t max_batch);
/* where the level-0 walk of a search starts (not in faiss): coarse_entries > 0 -- at the coarse_entries
 * nearest nodes above level 0, found by an exact scan of those rows on the flat kernel (default 4);
 * 0 -- where FAISS's greedy descent through the upper levels ends */
int knn_hnsw_set_entry(knn_hnsw_handle h, int32_t coarse_entries);
int knn_hnsw_get_params(knn_hnsw_handle h, int32_t *M, int32_t *efSearch, int32_t *efConstruction,
                        int32_t *max_level, int64_t *entry_point);
int knn_hnsw_add(knn_hnsw_handle h, const float *x_host, int64_t n);
/* the same for rows already on the index's device ([n][d] contiguous): a graph over a database that
 * never existed in host memory */
int knn_hnsw_add_dev(knn_hnsw_handle h, const float *x_dev, int64_t n, void *stream);
int knn_hnsw_search(knn_hnsw_handle h, const float *q_host, int64_t nq, int64_t k, float *D_host,
                    int64_t *I_host);
int64_t knn_hnsw_ntotal(knn_hnsw_handle h);
/* the flat storage underneath (index.storage); owned by the HNSW handle */
knn_handle knn_hnsw_storage(knn_hnsw_handle h);
void knn_hnsw_free(knn_hnsw_handle h);
/* graph tables for write_index / read_index: levels[n], offsets[n+1], nbrs[nslots]
 * (-1 = empty), cum_nb[nlevels_tab] (slots below each level), assign_probas.  A list ends at its
 * first -1 (FAISS's walk stops there): what an imported level-0 list holds behind one is dropped.
 * knn_hnsw_graph_import takes the tables of a graph whose storage rows are already in place
 * (knn_hnsw_storage + knn_flat_add) into an EMPTY graph.  It returns KNN_ERR_INVALID, and leaves
 * the graph empty so that corrected tables can follow, when: a level is outside the level table;
 * nslots is not what the levels add up to; an id is outside [-1, ntotal); (entry_point, max_level)
 * is not a node and its top level; or a list at level l >= 1 names, in any slot, a node whose top
 * level is below l -- a walk at level l reads that node's level-l list, which it does not own. */
int knn_hnsw_graph_sizes(knn_hnsw_handle h, int64_t *ntotal, int64_t *nslots, int32_t *nlevels_tab);
int knn_hnsw_graph_export(knn_hnsw_handle h, int32_t *levels, int64_t *offsets, int32_t *nbrs,
                          int32_t *cum_nb, double *assign_probas);
int knn_hnsw_graph_import(knn_hnsw_handle h, int64_t ntotal, const int32_t *levels, const int32_t *nbrs,
                          int64_t nslots, int32_t max_level, int64_t entry_point);
/* work counters since the last reset: (query,row) pairs evaluated, lock-step rounds,
 * pruned neighbour lists, seconds spent on GPU round trips and on the host walk */
int knn_hnsw_stats(knn_hnsw_handle h, int64_t *pairs, int64_t *rounds, int64_t *shrinks, double *gpu_s,
                   double *host_s, int32_t reset);

/* ---- faiss.IndexLSH(d, nbits) -----------------------------------------------
 * seqvec_search/create_index.py:41-45, pfam/search.py:27-37, pfam/proteins_search.py:25-26.
 * rotation_host: [nbits][d] row-major projection rows (FAISS uses a random orthonormal
 * matrix from its own RNG; the caller supplies one).  Codes: bit j = (x . rot_j >= 0), or
 * (x . rot_j >= t_j) once thresholds are trained or set (below);
 * search returns the k smallest Hamming distances as float32, ties by lower id. */
typedef struct knn_lsh_s *knn_lsh_handle;
int knn_lsh_create(int32_t d, int32_t nbits, const float *rotation_host, knn_lsh_handle *out);
int knn_lsh_add(knn_lsh_handle h, const float *x_host, int64_t n);
int knn_lsh_search(knn_lsh_handle h, const float *q_host, int64_t nq, int64_t k, float *D_host,
                   int64_t *I_host);
int64_t knn_lsh_ntotal(knn_lsh_handle h);
int32_t knn_lsh_code_words(knn_lsh_handle h);
/* codes in FAISS byte order ([ntotal][bytes_per_vec], bit i -> byte i>>3, bit i&7; bits at and above nbits are 0) */
int knn_lsh_get_codes(knn_lsh_handle h, uint8_t *out_host, int32_t bytes_per_vec);
int knn_lsh_add_codes(knn_lsh_handle h, const uint8_t *codes_host, int64_t n, int32_t bytes_per_vec);
/* IndexLSH(d, nbits, rotate_data, train_thresholds = true).train(x) -- every reference script calls train before add
 * (seqvec_search/create_index.py:43, pfam/search.py:35, pfam/proteins_search.py:87).  FAISS 1.7.2 IndexLSH::train
 * (published behaviour restated): the threshold of bit j is the median of x . rot_j over the n training rows (sorted
 * s: s[n/2] for odd n, (s[n/2 - 1] + s[n/2]) / 2 in float for even n; -0.0 counts as +0.0), and codes become
 * bit j = (x . rot_j >= t_j) for add and search alike.  Computes and installs the thresholds.  n < 1, a NaN projection
 * or a NaN median: KNN_ERR_INVALID (the handle keeps what it had).  The n x (code bits padded to 128 * 2^i) float
 * projections stay on the device for the call: more than half of the free device memory is KNN_ERR_UNSUPPORTED.
 * FAISS lets a filled index be trained again and leaves its stale codes behind; here train and set_thresholds on a
 * handle that holds rows are KNN_ERR_INVALID. */
int knn_lsh_train(knn_lsh_handle h, const float *x_host, int64_t n);
/* IndexLSH::thresholds as read_index finds them in an "IxHe" file: thr_host [nbits]; NULL removes them (bit j =
 * (x . rot_j >= 0) again).  A NaN entry is KNN_ERR_INVALID. */
int knn_lsh_set_thresholds(knn_lsh_handle h, const float *thr_host);
/* IndexLSH::thresholds for write_index: out_host [nbits]; KNN_ERR_INVALID if the handle has none */
int knn_lsh_get_thresholds(knn_lsh_handle h, float *out_host);
/* measurement (tools/lsh_train_probe.py): HIP-event milliseconds of the last successful knn_lsh_train -- the slabs'
 * uploads, their projection kernels, the median selection */
int knn_lsh_last_train_ms(knn_lsh_handle h, float *upload_ms, float *project_ms, float *select_ms);
/* IndexLSH::reset: drops the rows; rotation and thresholds stay */
int knn_lsh_reset(knn_lsh_handle h);
void knn_lsh_free(knn_lsh_handle h);

/* ---- faiss.IndexRefineFlat(base) --------------------------------------------
 * FAISS 1.7.2 IndexRefine::search (published behaviour restated; the reference uses its LSH index as exactly such a
 * shortlist: seqvec_search/main.py:132, pfam/search.py:27-51): the base index returns kb = k * k_factor labels per
 * query, the refine index scores those rows exactly against its stored fp32 vectors and the best k come back.
 * Scores: one fp32 chain per (query, label) in the contract's k order; inner product = the bits knn_flat_search
 * returns; L2 = the sum of squared differences at EVERY nq (IndexFlat::compute_distance_subset calls fvec_L2sqr per
 * pair, never the norm formula): the bits knn_flat_search returns for fewer than 20 queries.  Results best first,
 * equal scores by ascending label, unfilled slots -1 with -FLT_MAX (IP) / +FLT_MAX (L2).  1 <= k <= kb <= KNN_MAX_K:
 * k < 1 or k > kb is KNN_ERR_INVALID, kb > KNN_MAX_K is KNN_ERR_UNSUPPORTED.  nq = 0 returns 0; an index without rows
 * fills every slot as unfilled.  One corner differs from FAISS 1.7.2: a label of -1 (the base found fewer than kb
 * rows) never competes, where FAISS leaves the base's distance in place for it. */
/* IndexFlat::compute_distance_subset + reorder_2_heaps: labels_host int64 [nq][kb] from any base index over the same
 * rows.  Metric and rows are h's.  -1 is skipped; a label < -1 or >= ntotal is KNN_ERR_INVALID, checked before
 * anything is launched (D_host / I_host stay untouched).  A label that occurs twice in a row is scored twice and may
 * be returned twice, as in FAISS (up to 32 copies of one label per row; more may displace better labels). */
int knn_flat_refine(knn_handle h, const float *q_host, int64_t nq, const int64_t *labels_host, int64_t kb, int64_t k,
                    float *D_host, int64_t *I_host);
/* IndexRefineFlat(IndexLSH).search in one call: knn_lsh_search's batches with the kb Hamming hits of each batch
 * re-scored against flat's rows on the device; only [nq][k] is downloaded.  base and flat must be on the same device
 * with the same d and the same ntotal (KNN_ERR_INVALID otherwise).  Locks both handles: base first, then flat. */
int knn_lsh_search_refine(knn_lsh_handle base, knn_handle flat, const float *q_host, int64_t nq, int64_t kb, int64_t k,
                          float *D_host, int64_t *I_host);
/* measurement (tools/refine_probe.py): HIP-event milliseconds of the last successful knn_flat_refine /
 * knn_lsh_search_refine that used this flat handle -- its rescore launches and its final selections, summed over
 * the batches */
int knn_last_refine_ms(knn_handle h, float *rescore_ms, float *select_ms);

/* ---- consumers of (hits, scores): SURVEY section 8(f) N4 --------------------------
 * Host buffers in and out.  hits are int64 [nq][k] as returned by search.  k > INT32_MAX is KNN_ERR_INVALID
 * for all of them.  Every KNN_ERR_INVALID is returned before anything is allocated or launched on the device,
 * with the output buffers untouched.  Rows go through the device in slabs of 256 MiB of hits
 * (KNN355_EVAL_SLAB_ROWS, a positive integer, sets the rows per slab instead: tests). */
/* pfam/proteins.py:85-122 remove_self_hit: drops the self id from each row (or the last
 * hit when the row does not contain it: missing_out[r] = 1); outputs are [nq][k-1] */
int knn_eval_remove_self_hit(const int64_t *hits, const float *scores, int64_t nq, int64_t k,
                             const int64_t *self_ids, int64_t *hits_out, float *scores_out,
                             int32_t *missing_out);
/* seqvec_search/main.py:64-82 evaluate: lead_out[r] = hits of the query's label before the
 * first foreign hit, tp_out[r] = hits of the query's label anywhere; a hit < 0 or >= nb matches
 * nothing (labels_db may be NULL when nb is 0); is_correct_out
 * (uint8 [nq][k], may be NULL) is the per-hit match matrix of seqvec_search/tp_cumulative.py */
int knn_eval_labels(const int64_t *hits, int64_t nq, int64_t k, const int32_t *labels_q,
                    const int32_t *labels_db, int64_t nb, uint8_t *is_correct_out, int32_t *lead_out,
                    int32_t *tp_out);
/* pfam/proteins_shared.py:139-157 compute_auc1: query r is homologous to the SORTED target
 * rows set_members[set_offsets[r] .. set_offsets[r+1]); lead_out / tp_out as for knn_eval_labels.
 * set_offsets [nq + 1]; set_members may be NULL when set_offsets[nq] is 0.  KNN_ERR_INVALID when
 * set_offsets[0] < 0, when set_offsets[r+1] < set_offsets[r] for some r, or when the members of one
 * set are not non-decreasing (all checked on the host before the device sees them) */
int knn_eval_sets(const int64_t *hits, int64_t nq, int64_t k, const int64_t *set_offsets,
                  const int64_t *set_members, int32_t *lead_out, int32_t *tp_out);
/* cath/cath.py:76-84 compute_is_correct: out uint8 [nq][nlevels][k],
 * out[q][l][j] = mapping[query_rows[q]][l] == mapping[hits[q][j]][l]; mapping int32 [n][nlevels];
 * a hit < 0 or >= n is 0 at every level; a query row outside [0, n) is KNN_ERR_INVALID */
int knn_eval_levels(const int64_t *hits, int64_t nq, int64_t k, const int64_t *query_rows,
                    const int32_t *mapping, int64_t n, int32_t nlevels, uint8_t *out);
/* pfam/slices/slices.py:256-291 assemble: protein-level hits from a search over slices (fixed-length windows of
 * proteins; pfam/slices/slices_search.py).  hits / scores are [ns][k] as the slice search returned them; the k hits
 * of a row need not be sorted.  Query group g (a protein) owns the rows [group_offsets[g], group_offsets[g+1])
 * (group_offsets [ng + 1]); row_group[h] (int32 [nb]) is the group of database slice row h.  Per group:
 *   entries   its (score, hit) pairs, entry p = (r - group_offsets[g]) * k + j for cell j of row r
 *   order     ascending = 0: a before b when score_a > score_b; equal scores by smaller p; +0.0 and -0.0 are equal;
 *             NaN scores behind every other score, by p among themselves.  ascending = 1 mirrors the comparison
 *             (smaller scores first; ties and NaNs as before).  This is numpy.argsort(-scores) (slices.py:274) with
 *             its unspecified order among equal scores fixed to the stable one, and nothing else added.
 *   depth     only the first `depth` entries of that order are looked at (the reference: depth = k, slices.py:279)
 *   walk      those entries in order: one whose hit is < 0 or >= nb keeps its place in the order (it counts toward
 *             depth) but names no group, and neither does one whose row_group value is negative; one whose group is
 *             self_group[g] (int32 [ng]; NULL: no exclusion) is skipped; one whose group was already emitted for g is
 *             skipped; every other one is emitted: its group to groups_out, its score (the input's bits) to
 *             scores_out, and, where given, its row of hits (0 .. ns - 1) to qrow_out and its hit id to hit_out.
 *             The walk stops after k_out emissions.  (The reference indexes its slice table with the raw hit, so a
 *             hit of -1 wraps to the table's last slice there: that is not reproduced.)
 *   padding   unfilled slots: group -1, score -FLT_MAX (ascending: +FLT_MAX), -1 in qrow_out / hit_out, as the flat
 *             search pads; a group without rows is all padding.
 * Outputs are [ng][k_out].  KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched:
 * ns, ng or nb < 0; k < 1 or k > INT32_MAX; depth < 1 or depth > KNN_MAX_K; k_out < 1 or k_out > depth; a null
 * required pointer (row_group may be NULL when nb is 0, hits / scores when ns is 0); group_offsets[0] < 0, decreasing
 * offsets, group_offsets[ng] > ns; a group with rows * k >= 2^31.  ng = 0 returns 0.  Slabs (see above) are cut at
 * group boundaries and always take one whole group at least; row_group is uploaded once.
 * Hot path: assemble_kernel (assemble.inc), one workgroup per group: selection of the best depth keys in LDS, group
 * lookup and de-duplication in rank order, ballot-and-prefix compaction. */
int knn_eval_assemble(const int64_t *hits, const float *scores, int64_t ns, int64_t k,
                      const int64_t *group_offsets, int64_t ng, const int32_t *row_group, int64_t nb,
                      const int32_t *self_group, int32_t depth, int32_t k_out, int32_t ascending,
                      int64_t *groups_out, float *scores_out, int64_t *qrow_out, int64_t *hit_out);
/* pfam/slices/slices.py:49-80 and :101-142 evaluate: the hits of a search over slices judged at slice level.
 *   ids       families are dense int32 codes in [0, nfam), proteins int32 ids in [0, np)
 *   domains   domain_offsets int64 [np + 1]: protein p owns the domains [domain_offsets[p], domain_offsets[p+1]);
 *             domain_family / domain_start / domain_stop int32 [nd], nd = domain_offsets[np] (all three may be NULL
 *             when nd is 0, domain_offsets when np is 0).  Within one protein domain_family does not decrease.
 *   slices    slice_protein / slice_start / slice_stop int32 [ns]; a slice with slice_protein == -1 has no domains
 *   tests     for slice s and a domain d of its protein, exactly as slices.py:57 and :65:
 *               inside        slice_start <= domain_start && domain_stop <= slice_stop
 *               intersecting  otherwise, when slice_start < domain_stop && domain_start < slice_stop
 *             matching(s) is the set of families with a domain inside, intersecting(s) the set of families with a
 *             domain intersecting; one family can be in both, through two of its domains.
 * knn_eval_slice_annotate (slices.py:49-80):
 *   match_count[s] = |matching(s)|, distinct families counted once; annotation[s] = the one family of matching(s) when
 *   match_count[s] == 1, else -1 (slices.py:76-80: has_annotation is annotation >= 0); family_sizes[f] (int64 [nfam],
 *   all of it written) = the number of slices whose matching holds f (slices.py:70-74).
 * knn_eval_slices (slices.py:101-142), hits int64 [nq][k], row q with a = query_family[q] and hit h:
 *   is_correct[q][j] = 1 when a is in matching(h); is_ignore[q][j] = 1 when a is in intersecting(h), and also when
 *   ignore_unannotated is non-zero and match_count[h] == 0 (match_count as knn_eval_slice_annotate wrote it; it may be
 *   NULL when ignore_unannotated is 0).  A hit outside [0, ns), -1 included, is neither correct nor ignored.  (The
 *   reference indexes its lists with the raw hit, so -1 reads the last slice there: that is not reproduced.)  A row
 *   with a < 0 is all zeros, its lead and tp included.
 *   lead[q] = the correct hits in front of the first hit that is neither correct nor ignored (the loop at
 *   slices.py:131-138; a hit that is both counts as correct); tp[q] = the correct hits of the row;
 *   column_correct[j] (int64 [k], may be NULL) = the rows whose hit j is correct, summed over all slabs (the script
 *   plots its cumulative sum, slices.py:226-227).
 * KNN_ERR_INVALID, with a message, before anything is allocated or launched and with the outputs untouched: a negative
 * nq, ns, np or nfam; np > INT32_MAX; k < 1 or k > INT32_MAX; a null required pointer; domain_offsets[0] < 0 or
 * decreasing offsets; a domain family outside [0, nfam) or smaller than its predecessor in the same protein; a
 * slice_protein outside [-1, np); a query_family >= nfam.  nq = 0 returns 0 before any pointer is looked at.  ns = 0
 * runs the same checks and then returns 0 without touching the device: family_sizes is zeros, and every output of
 * knn_eval_slices is zeros (no hit names a slice).  The slice and domain tables are uploaded once per call, the hits go
 * through the device in slabs (see above).
 * Hot path: slice_annotate_kernel, one thread per slice over its protein's domains in family order, integer atomics
 * into family_sizes; slice_eval_kernel, one wave per row: per hit one 16-byte slice record, a lower-bound search for a
 * in the protein's domains and the interval tests over a's run, ballots for lead and tp (slices_eval.inc). */
int knn_eval_slice_annotate(const int32_t *slice_protein, const int32_t *slice_start, const int32_t *slice_stop,
                            int64_t ns, const int64_t *domain_offsets, const int32_t *domain_family,
                            const int32_t *domain_start, const int32_t *domain_stop, int64_t np, int64_t nfam,
                            int32_t *match_count, int32_t *annotation, int64_t *family_sizes);
int knn_eval_slices(const int64_t *hits, int64_t nq, int64_t k, const int32_t *query_family,
                    const int32_t *slice_protein, const int32_t *slice_start, const int32_t *slice_stop, int64_t ns,
                    const int64_t *domain_offsets, const int32_t *domain_family, const int32_t *domain_start,
                    const int32_t *domain_stop, int64_t np, int64_t nfam, const int32_t *match_count,
                    int32_t ignore_unannotated, uint8_t *is_correct, uint8_t *is_ignore, int32_t *lead, int32_t *tp,
                    int64_t *column_correct);
/* pfam/proteins.py:201-207 compute_correctness_array: the per-hit membership matrix of knn_eval_sets' sets.
 * Arguments, argument checks, slabs and edge cases are knn_eval_sets' (members sorted per set, checked on the host;
 * nq = 0 returns 0); is_correct_out (uint8 [nq][k], required) gets 1 where hits[r][j] is a member of set r, else 0:
 * a hit that is in no set, a negative one included, gives 0. */
int knn_eval_sets_matrix(const int64_t *hits, int64_t nq, int64_t k, const int64_t *set_offsets,
                         const int64_t *set_members, uint8_t *is_correct_out);
/* pfam/proteins.py:626-648, the precision-recall sweep: mean precision and mean recall per query at each of nthr score
 * thresholds.  is_correct (uint8) and scores are [nq][k], totals [nq] (the number of homologues of each query),
 * thresholds [nthr]; every output is [nthr].
 *   cells       only columns 0 .. limit-1 of each row are read (1 <= limit <= k); a cell is correct when its
 *               is_correct byte is non-zero
 *   selection   cell (q, c) is selected at threshold j when (double)scores[q][c] > thresholds[j]: a strict comparison in
 *               double, as numpy compares a float32 array with a float64 scalar.  A NaN score is never selected; +-inf
 *               scores and thresholds follow the comparison.
 *   thresholds  non-decreasing and free of NaN; equal neighbours are legal (quantiles of tied scores).  With that,
 *               "selected at j" is j < #{i : thresholds[i] < (double)s}: one binary search per cell.
 *   per query   n = number of selected cells, tp = number of selected correct cells;
 *               P(q,j) = n ? (double)tp / (double)n : 1.0 ("no prediction, no error", proteins.py:641);
 *               R(q,j) = (double)tp / (double)totals[q]; both divisions IEEE double, correctly rounded
 *   integers    selected_out[j] = sum over q of n, tp_out[j] = sum over q of tp, empty_out[j] = number of queries with
 *               n = 0 (any of the three may be NULL)
 *   means       precision_out[j] = S_P(j) / (double)nq and recall_out[j] = S_R(j) / (double)nq, the sums taken in one
 *               stated order, so that the result is one defined double whatever the launch shape and the slab size:
 *               queries form blocks of 256 consecutive rows by global row index; a block's sum starts at +0.0 and adds
 *               its queries' terms in row order; S starts at +0.0 and adds the block sums in block order.  (No
 *               floating-point atomics, no tree whose shape depends on the grid.)
 * KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched: nq < 1 (a mean over
 * nothing); k < 1, k > INT32_MAX, limit < 1, limit > k; nthr < 1 or nthr > 4096; a null required pointer (precision_out
 * and recall_out are required); totals[q] < 1 for some q; a decreasing or NaN threshold.
 * Slabs: as above, but the rows per slab (KNN355_EVAL_SLAB_ROWS included) are rounded up to a multiple of 256, so that
 * blocks never straddle slabs; pr_fold_kernel adds a slab's block sums to the running S in block order.
 * Hot path: pr_curve_kernel (pr_curve.inc), one workgroup per block of 256 queries: per query a histogram over the
 * thresholds in LDS, a workgroup-wide suffix scan, one division per threshold into per-thread accumulators. */
int knn_eval_pr_curve(const uint8_t *is_correct, const float *scores, int64_t nq, int64_t k, int64_t limit,
                      const int64_t *totals, const double *thresholds, int32_t nthr,
                      double *precision_out, double *recall_out,
                      int64_t *selected_out, int64_t *tp_out, int64_t *empty_out);
/* pfam/proteins.py:689-729, the accuracy per score bucket: how many cells of (is_correct, scores) fall into each of nb
 * score buckets, and how many of those are correct.  All pointers are host pointers.  scores is [nq][k], float32
 * (key_type KNN_RANK_F32) or float64 (KNN_RANK_F64), is_correct uint8 [nq][k], lo and hi [nb], both outputs int64 [nb].
 *   cells       only columns 0 .. limit-1 of each row are read (1 <= limit <= k); a cell is correct when its
 *               is_correct byte is non-zero
 *   membership  a cell with score s is in bucket b iff lo[b] < (double)s && (double)s <= hi[b], both comparisons in double,
 *               as numpy compares a float32 array with the float64 scalars the reference's loop iterates over.  A NaN
 *               score is in no bucket; +-inf and -0.0 follow the comparisons.
 *   edges       two arrays, not nb + 1 edges: the reference's lower edge is linspace(0, 1 - 1/s, s)[b] and its upper edge
 *               that + 1/s, and the upper edge of a bucket and the lower edge of the next often differ in the last bit
 *               (at s = 300: 28 pairs overlap, 62 leave a gap).  A cell may therefore be in two buckets or in none, and
 *               the last upper edge may lie one ulp below 1.0.  lo and hi are each non-decreasing and free of NaN, with
 *               lo[b] <= hi[b]; equal neighbours and lo[b] == hi[b] (an empty bucket) are legal.  With that the buckets
 *               of a cell are h .. a - 1, a = #{i : lo[i] < s}, h = #{i : hi[i] < s}: two binary searches.
 *   outputs     count_out[b] = the number of member cells, correct_out[b] = the number of correct member cells (both
 *               required).  Integers only: the result does not depend on the launch shape, the slab size or the order of
 *               the atomics.
 * KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched: an unknown key_type; nq < 1;
 * k < 1, k > INT32_MAX, limit < 1, limit > k; nb < 1 or nb > 4096; a null pointer; a NaN edge; lo or hi decreasing;
 * lo[b] > hi[b] for some b.
 * Slabs: as above (KNN355_EVAL_SLAB_ROWS included), and at most 2^31 cells each; the counters stay on the device across
 * the slabs.
 * Hot path: bucket_hist_kernel (buckets.inc), one wave per row: the two searches over the edges in LDS, packed 64-bit
 * LDS atomics into two threshold histograms (KNN355_BUCKET_AGG=1: equal (a, h) pairs merged inside the wave first), integer
 * atomicAdd into global counters; the two prefix sums over nb + 1 words and their difference are host work. */
int knn_eval_bucket_counts(const void *scores, int32_t key_type, const uint8_t *is_correct, int64_t nq, int64_t k,
                           int64_t limit, const double *lo, const double *hi, int32_t nb,
                           int64_t *count_out, int64_t *correct_out);
/* pfam/proteins.py:502-507 make_accuracy_over_hit, the mean fraction of a query's homologues found after j hits, and the
 * per-query counts behind proteins.py:476-496 (recall_per_query, loss_aligning).  All pointers are host pointers.
 * is_correct is uint8 [nq][k], totals int64 [nq] (the number of homologues of each query).
 *   C(q,j)      the number of correct cells (non-zero bytes) of row q in columns 0 .. j; only columns 0 .. limit-1 are read
 *   t(q,j)      (double)C(q,j) / (double)totals[q], IEEE double, correctly rounded
 *   mean        S(j) starts at +0.0 and adds t(0,j), t(1,j), ... in row order; mean_out[j] = S(j) / (double)nq, double
 *               [limit], required.  This is the order numpy uses for mean(axis=0) of a C-ordered 2-D array, so for
 *               limit >= 2 the result has the bits of the reference's expression.  (For limit = 1 numpy collapses the
 *               array to one dimension and sums pairwise; the contract stays "row order".)
 *   rows        row_correct_out[q] = C(q, limit-1), int64 [nq], may be NULL
 *   columns     column_correct_out[j] = the sum over q of C(q,j), int64 [limit], may be NULL
 * KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched: nq < 1; k < 1, k > INT32_MAX,
 * limit < 1, limit > k; a null is_correct, totals or mean_out; totals[q] < 1 for some q.
 * Slabs: as above (KNN355_EVAL_SLAB_ROWS included), and at most 256 MiB of t each; the running S stays on the device and
 * is carried across the slabs in row order.  No floating-point atomics.
 * Hot path (buckets.inc): hit_terms_kernel, one wave per row, C by ballot and popcount over groups of 64 columns, t into
 * a [slab rows][limit] scratch, the row counts, the correct cells per column (whose prefix sum is the column sums);
 * hit_fold_kernel, one workgroup per 32 columns, carries tiles of the scratch into LDS one tile ahead while 32 threads
 * add the rows to S in order: only the adds are serial. */
int knn_eval_hit_curve(const uint8_t *is_correct, int64_t nq, int64_t k, int64_t limit, const int64_t *totals,
                       double *mean_out, int64_t *row_correct_out, int64_t *column_correct_out);
/* measurement (tools/bench_buckets.py): milliseconds by HIP events of the calling thread's last successful
 * knn_eval_bucket_counts (counts_ms[3]) and knn_eval_hit_curve (curve_ms[3]): uploads, kernels, downloads, each summed
 * over the slabs. */
int knn_eval_buckets_last_ms(float *counts_ms /* [3] */, float *curve_ms /* [3] */);
/* One stable order over every hit of a result set, with look-ups: pfam/pfam.py:561-598 (the dataset-wide precision-recall
 * curve), the cumulative curves is_correct[argsort(key)].cumsum() (cath/cath.py:656-675, 738-771; pfam/pfam.py:166-177,
 * 213-236) and the order statistics behind numpy.quantile(scores[:, :limit], ...) (pfam/proteins.py:626-648).  All
 * pointers are host pointers.  scores is [rows][k], float32 (key_type KNN_RANK_F32) or float64 (KNN_RANK_F64); correct
 * (may be NULL) is uint8 [rows][k], non-zero meaning correct.
 *   elements    the N = rows * limit cells of columns 0 .. limit-1 (1 <= limit <= k); the flat position of cell
 *               (row, column) is p = row * limit + column.  N <= 2^31 - 1.
 *   key         the order-preserving unsigned image of the score, 32 or 64 bits: -0.0 is taken as +0.0 first (numpy
 *               compares them equal); every NaN, of either sign and any payload, gets the one largest key, so NaN sorts
 *               last, as in numpy.argsort; sub-normals order by their value, +-inf by theirs.  descending != 0
 *               complements the image of every key but NaN's: NaN still sorts last, the rest in the order of
 *               numpy.argsort(-scores, kind="stable").
 *   order       ascending by key; equal keys in ascending flat position.  This is numpy.argsort(scores[:, :limit]
 *               .flatten(), kind="stable").  The reference calls numpy's default sort, whose order among equal scores is
 *               unspecified (and differs from the stable one on tied float64 input); here it is fixed.
 *   C(r)        the number of correct cells among the ranks 0 .. r of the order (inclusive)
 *   outputs     each only when asked for:
 *               order_out int64 [N] (NULL: not wanted): order_out[r] = the flat position of the element of rank r
 *               cum_out int64 [N] (NULL: not wanted): cum_out[r] = C(r)
 *               nt > 0: for each targets[j] (int64), idx_out[j] = the first r with C(r) >= targets[j] -- 0 for a target
 *               <= 0, N for a target that no r reaches -- and cum_at_out[j] = C(min(idx_out[j], N - 1))
 *               nr > 0: sorted_at_out[j] (in the scores' type) = the score of the element of rank ranks[j], its bits
 *               untouched (a -0.0 or a NaN's payload come back as they went in)
 * KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched: an unknown key_type; rows < 1;
 * k < 1 or k > INT32_MAX; limit outside [1, k]; rows * limit > 2^31 - 1; nt or nr outside [0, INT32_MAX]; a null scores;
 * nt > 0 with a null targets, idx_out or cum_at_out; nr > 0 with a null ranks or sorted_at_out; cum_out or nt > 0 without
 * correct; a rank outside [0, N).
 * The whole problem stays on the device for the call: the two arrays -- as given, or, when limit <= k / 2, their first
 * `limit` columns packed on the host -- two key and two payload buffers of N entries, 256 counts per tile of 2048
 * elements, and what the outputs asked for need; plan_rank in csrc/plan.h has every buffer's bytes and the call allocates
 * exactly those.  A failed allocation returns KNN_ERR_HIP with nothing left allocated.
 * Hot path (rank.inc): a least-significant-digit radix sort with 8-bit digits over (key, position << 1 | correct) pairs.
 * rank_hist_kernel counts the digits of every pass in one read; a pass whose digit is the same in all keys is skipped.
 * A pass is rank_count_kernel (per-tile digit counts), a two-level exclusive scan of the [256][tiles] table in
 * digit-major order, and rank_scatter_kernel (stable rank inside the tile: bit-matching ballots inside a wave, per-wave
 * digit counts through LDS).  C(r) is a two-level inclusive scan of the sorted flags; the targets are binary searches in
 * C.  No workgroup waits on another; no floating-point number is rounded (the one
 * floating-point instruction is the v != v that finds a NaN). */
#define KNN_RANK_F32 0
#define KNN_RANK_F64 1
int knn_eval_rank(const void *scores, int32_t key_type, int64_t rows, int64_t k, int64_t limit, const uint8_t *correct,
                  int32_t descending, int64_t *order_out, int64_t *cum_out,
                  const int64_t *targets, int64_t nt, int64_t *idx_out, int64_t *cum_at_out,
                  const int64_t *ranks, int64_t nr, void *sorted_at_out);
/* measurement (tools/bench_rank.py): how the calling thread's last successful knn_eval_rank ran -- the passes it ran and
 * the ones it skipped (together the bytes of a key), the tiles of a pass, and milliseconds ms[6]: on the host's clock the
 * device allocations and the packing of the columns; by HIP events the upload of the two arrays, the sort (histograms
 * and passes), the scan of the flags, the look-ups with their downloads.  The buffers are freed as the call returns:
 * that time is in no figure. */
int knn_last_rank_info(int32_t *passes_run, int32_t *passes_skipped, int64_t *tiles, float *ms /* [6] */);
/* Statistics over contiguous ranges of one stable order: the rolling means of seqvec_search/utils.py:103 (rolling_mean =
 * numpy.convolve(data, ones(W) / W, "valid"), called on arrays in the order of a key at pfam/pfam.py:247-253,
 * cath/cath.py:799-813 and 913-919), the equal-count slices of hist_evenly (cath/cath.py:863-875, pfam/pfam.py:282-297)
 * and the fixed length bins of cath/cath.py:831-857.  All pointers are host pointers.  keys is float32 (KNN_RANK_F32) or
 * float64 (KNN_RANK_F64) [n], 1 <= n <= 2^31 - 1; values (NULL when m = 0) is uint8 [m][n], 0 <= m <=
 * KNN_WINDOWS_MAX_COLS, a non-zero byte meaning set.
 *   order       knn_eval_rank's, of the n keys (rows = n, k = limit = 1): stable, -0.0 == +0.0, every NaN last,
 *               descending != 0 the order of numpy.argsort(-keys, kind="stable").  order_out int64 [n] (NULL: not wanted)
 *               receives it.
 *   C_c(r)      the number of set cells of column c among the ranks 0 .. r, an exact integer; C_c(-1) = 0.
 *   window W    (window > 0; 0: no rolling means) n - W + 1 outputs per column and for the key:
 *               value_means_out float64 [m][n - W + 1]: (C_c(i + W - 1) - C_c(i - 1)) / W, one float64 division of two
 *               exact integers, done on the device: the correctly rounded mean of the window.  (The reference's
 *               convolution adds W terms of fl(1 / W) in an order its BLAS chooses; it differs in the last bits.)
 *               key_means_out float64 [n - W + 1], with no subtraction anywhere, so that an infinity or a NaN touches
 *               only the windows that hold it: the ranked keys, float32 widened to float64 first, are cut into blocks of
 *               W consecutive ranks, block b = r / W (the last one may be short).  Per block two chains of sequential
 *               float64 additions: P[r] = the sum of the block's elements from its first rank through r, added in rank
 *               order, and S[r] = the sum from r through the block's last rank, added from the block's end backwards;
 *               a chain starts with its first element itself (not 0 + element: a -0.0 stays -0.0).  Output i is
 *               P[i + W - 1] / W when i % W == 0, else (S[i] + P[i + W - 1]) / W.  This is numpy.cumsum along the
 *               rows of the [blocks, W] reshape, forward and reversed.
 *   bins        (nbins > 0) either ranges of ranks, starts and stops int64 [nbins] with 0 <= start <= stop <= n (edges
 *               NULL), or edges in the keys' type [nbins], finite and ascending (starts and stops NULL; ascending order
 *               only): bin j holds the keys with edges[j] <= key < edges[j + 1], the last one every key >= edges[nbins -
 *               1]; NaN keys fall in no bin.  An edge goes through the same order-preserving image as the keys, so start
 *               = the first rank whose key image is not below the edge's (-0.0 and sub-normals as in the sort), stop = the
 *               next bin's start, and the last bin stops at the first NaN.  start_out and stop_out int64 [nbins] receive
 *               the ranks (for ranges: the ones given), counts_out int64 [m][nbins] the exact C_c(stop - 1) - C_c(start
 *               - 1), key_lo_out and key_hi_out (the keys' type [nbins]) the keys at ranks min(start, n - 1) and
 *               min(stop, n - 1), bits untouched.  Means and standard errors are the caller's (evaluation.even_bins).
 * KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched: an unknown key_type; n outside
 * [1, 2^31 - 1]; m outside [0, KNN_WINDOWS_MAX_COLS]; window outside [0, n]; nbins outside [0, KNN_WINDOWS_MAX_BINS];
 * neither a window nor bins; a null keys; m > 0 with a null values; a window with a null key_means_out, or with m > 0 and
 * a null value_means_out; bins with a null output (counts_out only when m > 0), with both or neither of (starts, stops)
 * and edges, with edges and descending, with an edge that is not finite or lies below the one before it, or with a range
 * outside 0 <= start <= stop <= n; starts, stops or edges with nbins = 0.
 * The whole problem stays on the device for the call; plan_windows in csrc/plan.h has every buffer's bytes, the staging
 * run of the chains, blocks per run or runs per block and the grids, and the call allocates exactly those.
 * Hot path (windows.inc): the sort of rank.inc; window_gather_kernel (payload -> position -> one uint32 mask of the m
 * value bytes, and the key as float64, in rank order); m two-level scans of the masks' bits; window_means_kernel;
 * window_chain_kernel (runs of 2048 ranked keys staged in LDS per direction, one lane per block and direction walking its
 * chain, the sum carried across runs when W exceeds one) and window_combine_kernel; window_ranges_kernel (binary
 * searches of the edges' images, C_c at the range ends, the keys at start and stop).  No workgroup waits on another, no
 * atomic, plain vector stores only. */
#define KNN_WINDOWS_MAX_COLS 32
#define KNN_WINDOWS_MAX_BINS (1 << 20)
int knn_eval_windows(const void *keys, int32_t key_type, int64_t n, const uint8_t *values, int32_t m, int32_t descending,
                     int64_t window, double *key_means_out, double *value_means_out, int64_t *order_out,
                     const int64_t *starts, const int64_t *stops, const void *edges, int64_t nbins, int64_t *start_out,
                     int64_t *stop_out, int64_t *counts_out, void *key_lo_out, void *key_hi_out);
/* measurement (tools/bench_windows.py): how the calling thread's last successful knn_eval_windows ran -- the staging run
 * of the chains in ranks, the blocks that share a run and the runs that make a block (one of the two is 1; both 0 without
 * a window), and milliseconds ms[8]: on the host's clock the device allocations; by HIP events the uploads, the sort, the
 * gather with the scans, the chains with their combination, the columns' means, the bins, the downloads. */
int knn_last_windows_info(int64_t *run, int64_t *blocks_per_run, int64_t *runs_per_block, float *ms /* [8] */);
/* Tie-averaged ranks and the two correlations of cath/cath.py:949-952 (scipy.stats.pearsonr of the cosine scores and the
 * logged E-values, scipy.stats.spearmanr of the scores and the E-values) over every hit of a result set.  All pointers are
 * host pointers.  An array is [rows][k], float32 (KNN_RANK_F32) or float64 (KNN_RANK_F64); its elements are the N = rows *
 * limit cells of columns 0 .. limit-1, flat position p = row * limit + column, as in knn_eval_rank; 2 <= N <= 2^31 - 1.
 *   knn_eval_rankdata   rank2_out int64 [N]: rank2_out[p] = twice the average rank of cell p among all N, an exact integer
 *               in [2, 2N]: in knn_eval_rank's ascending order (keys compared by their order-preserving images: -0.0 equals
 *               +0.0, +-inf order by value) every member of a run of equal keys at the 0-based ranks s .. e gets s + e + 2.
 *               rank2_out / 2 is scipy.stats.rankdata(a[:, :limit].ravel(), "average"), bit for bit.  *nan_count_out
 *               receives the number of NaN cells; when it is not 0 no rank is written (scipy's nan_policy="propagate": every
 *               statistic of such input is NaN) and the call still returns 0.
 *   knn_eval_correlate  x and y have the same shape and either type, independently.  what is a bit set:
 *               KNN_CORR_PEARSON: pearson_out float64 [5] = mean_x, mean_y, Sxx, Sxy, Syy.  Every value is widened to float64
 *               first.  mean = (the sum of the N values) / N; then, with dx = x - mean_x and dy = y - mean_y, Sxx = the sum of
 *               dx * dx, Sxy of dx * dy, Syy of dy * dy (two passes, nothing fused, as scipy does).  Every one of the five
 *               sums is taken in ONE order that is a function of N alone (plan_correlate in csrc/plan.h): tiles of 2048
 *               consecutive terms; lane j of 256 adds terms j, j + 256, ... of its tile in that order to +0.0; the lanes fold
 *               by lane[j] += lane[j + off], off = 128, 64, ..., 1; the tiles' sums, in tile order, are summed the same way,
 *               level by level, until one is left.  No floating-point atomic, nothing that depends on the grid or on the
 *               order in which workgroups finish.  An infinity or a NaN goes through this arithmetic as IEEE 754 has it
 *               (inf - inf = NaN): nothing is special-cased.  The statistic is Sxy / (sqrt(Sxx) * sqrt(Syy)), the caller's.
 *               KNN_CORR_SPEARMAN: spearman_out uint64 [6] = (lo, hi) words of the three 128-bit two's-complement sums of
 *               u * u, u * v and v * v over the doubled, centred ranks u = rank2_x - (N + 1), v = rank2_y - (N + 1): exact
 *               integers (a term is below 2^62 in magnitude, a sum below 2^93); no floating-point number is rounded on the
 *               device.  nan_count_out int64 [2] receives the NaN cells of x and of y; when either is not 0, spearman_out is
 *               left untouched.  With KNN_CORR_PEARSON alone nothing is sorted and nan_count_out (may be NULL) is left
 *               untouched: a NaN shows in the sums.
 * KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched: an unknown type; rows < 1; k < 1
 * or k > INT32_MAX; limit outside [1, k]; N outside [2, 2^31 - 1]; a null input; what outside [1, 3]; a null rank2_out or
 * nan_count_out (rankdata); KNN_CORR_PEARSON with a null pearson_out; KNN_CORR_SPEARMAN with a null spearman_out or
 * nan_count_out.
 * The whole problem stays on the device for the call; plan_correlate in csrc/plan.h has every buffer's bytes, the levels of
 * the sums and the grids, and the call allocates exactly those.  The sorts of x and of y run one after the other in the
 * same key and payload buffers.
 * Hot path (correlate.inc): the sort of rank.inc with the flat position as payload; tie_heads_kernel (rank r heads a run
 * when its key image differs from rank r - 1's), rank.inc's scan of the head flags (the run number of every rank),
 * tie_starts_kernel (every head writes its run's first rank), tie_scatter_kernel (rank2[position] = start + end + 2);
 * moment_int_kernel and moment_f64_kernel, one launch per level.  No workgroup waits on another, no atomic, plain vector
 * stores only. */
#define KNN_CORR_PEARSON 1
#define KNN_CORR_SPEARMAN 2
int knn_eval_rankdata(const void *a, int32_t key_type, int64_t rows, int64_t k, int64_t limit, int64_t *rank2_out,
                      int32_t *nan_count_out);
int knn_eval_correlate(const void *x, int32_t x_type, const void *y, int32_t y_type, int64_t rows, int64_t k, int64_t limit,
                       int32_t what, double *pearson_out /* [5] */, uint64_t *spearman_out /* [6] */,
                       int64_t *nan_count_out /* [2] */);
/* measurement (tools/bench_correlation.py): milliseconds ms[6] of the calling thread's last successful knn_eval_rankdata or
 * knn_eval_correlate: on the host's clock the device allocations; by HIP events the uploads (with the host's packing of the
 * first `limit` columns), the sorts, the ranks (heads, scan, starts, scatter, NaN count), the moments, the downloads. */
int knn_last_correlate_info(float *ms /* [6] */);
/* cath/cath.py:404-438 bootstrap_scores, the replicates behind the "+-" of the accuracy table (:441-458): per method and
 * per resample of the evaluable queries, the raw and the superfamily-normalized top-1 accuracy.  All arrays are host
 * arrays.  is_correct uint8 [nm][n]: row m is method m's verdict for each of the n evaluable queries, a non-zero byte
 * means correct; family int32 [n]: the dense code in [0, nfam) of each query's superfamily (the reference's
 * mapping_array[is_possible, 0]); sample_ids int32 [nb][n]: replicate b's resample, values in [0, n).  present_out is
 * [nb], the other three outputs are [nm][nb].
 *   counts      for replicate b and family f, count_b[f] = #{i : family[sample_ids[b][i]] == f} and corr_{m,b}[f] = the
 *               number of those i whose is_correct[m][sample_ids[b][i]] is non-zero: exact integers
 *   integers    present_out[b] = #{f : count_b[f] > 0}; correct_out[m][b] = the sum of corr_{m,b}[f] over f
 *   raw         raw_out[m][b] = (double)correct_out[m][b] / (double)n, correctly rounded: bit for bit what
 *               is_correct[sample_ids].mean() gives (cath.py:419)
 *   terms       every f with count_b[f] > 0 contributes t_f = (double)corr[f] / (double)count[f], one IEEE division; an
 *               absent family contributes nothing: there is never a 0 / 0
 *   normalized  normalized_out[m][b] = S / (double)present_out[b], S the sum of the t_f in the order knn_eval_pr_curve
 *               defines for its queries, here over family codes: codes form blocks of 256 consecutive codes; a block's
 *               sum starts at +0.0 and adds its present families in code order; S starts at +0.0 and adds the block sums
 *               in block order.  (No floating-point atomics, no tree whose shape depends on the launch.)
 *   reference   the real number is the one cath.py:413-418 computes, sum_i c_i * (1 / n_f(i)) / #families; only the
 *               order of the sum is fixed differently (the reference's is numpy's pairwise sum)
 * KNN_ERR_INVALID, with a message naming the argument, before anything is allocated or launched and with the outputs
 * untouched: nm, nb or n negative; n < 1 when nm and nb are positive (a mean over nothing); n > INT32_MAX; nfam < 1 or
 * nfam > KNN_BOOTSTRAP_MAX_FAMILIES; a null pointer (all four outputs are required); a family value outside [0, nfam);
 * a sample_ids value outside [0, n): all checked on the host.  nm = 0 or nb = 0 returns 0 before any pointer is looked
 * at.  is_correct and family are uploaded once; the replicates go through the device in slabs of 256 MiB of
 * sample_ids rows (KNN355_EVAL_SLAB_ROWS sets the replicates per slab, as above).
 * Hot path: bootstrap_kernel (bootstrap.inc), one workgroup per (replicate, method): integer histograms count and corr
 * over the family codes in LDS (8 * nfam bytes: the cap is 128 KiB), then one wave per block of 256 codes. */
#define KNN_BOOTSTRAP_MAX_FAMILIES 16384
int knn_eval_bootstrap(const uint8_t *is_correct, int64_t nm, int64_t n, const int32_t *family, int32_t nfam,
                       const int32_t *sample_ids, int64_t nb, int64_t *correct_out, int32_t *present_out,
                       double *normalized_out, double *raw_out);
/* pfam/proteins.py:216-240 ("combined") and 340-372 ("both aligned"): one output row per query from two hit lists.
 * hits_a / scores_a / keep_a are [nq][ka], hits_b / scores_b [nq][kb], hits_out / scores_out / source_out [nq][k_out],
 * filled_out [nq]; all host arrays, row-major.  Scores are float64, as the reference's e-values are
 * (seqvec_search/mmseqs/_read_results_db.py:172; a float32 holds 0 for every e-value under 1.4e-45, and float32 scores
 * upcast exactly); ids are compared as whole int64 values.
 *   entries    an entry of A exists when its hit is >= 0 and keep_a is NULL or non-zero there; an entry of B exists when
 *              its hit is >= 0.  Entries that do not exist are never emitted and never enter a set.  (The reference pads
 *              its rows with id 0, which is therefore an ordinary id here too.)
 *   positions  the position of A's column j is j, the position of B's column j is ka + j
 *   KNN_FUSE_PREFIX_FILL   the row's output is the existing A entries in column order, then the existing B entries, in
 *              column order, whose id no existing A entry of that row carries; cut at k_out.  Repeats inside A, or inside
 *              B, are kept, as the reference keeps them.  `ascending` only chooses the padding.
 *   KNN_FUSE_SORTED_UNION  the existing entries of A and B are ordered by score: ascending != 0 puts the smallest first,
 *              otherwise the largest; -0.0 and +0.0 tie; every NaN sorts behind everything else; equal scores (and the
 *              NaNs among themselves) are ordered by position.  Sub-normal scores order by their value: the comparison is
 *              made on the doubles' bits and flushes nothing.  The row is walked once in that order: an entry whose id an
 *              earlier entry of the walk carries is dropped; the walk stops at k_out outputs.  This is numpy.argsort
 *              (proteins.py:345) with its unspecified order among equal scores fixed to the stable one.
 *   outputs    filled_out[q] is the number of outputs of row q; scores_out holds the input's bits; source_out (may be
 *              NULL) holds each output's position.  The rest of the row is padded: id -1, score +DBL_MAX (ascending) or
 *              -DBL_MAX (not ascending), source -1.
 * KNN_ERR_INVALID, with a message naming the argument, before anything is allocated or launched and with the outputs
 * untouched: nq < 0; ka or kb outside [1, KNN_MAX_K]; k_out outside [1, ka + kb]; an unknown mode; a null required
 * pointer (keep_a and source_out may be NULL).  nq = 0 returns 0 before any pointer is looked at.  Rows go through the
 * device in slabs of the row count above for k = ka + kb (KNN355_EVAL_SLAB_ROWS included).
 * Hot path: fuse_kernel (fuse.inc), one workgroup per row: a bitonic sort of (order word of the double, position) pairs
 * in LDS and a repeat scan in rank order (sorted union), or a membership scan of B against A's ids in LDS (prefix, then
 * fill); ballot-and-prefix compaction either way. */
#define KNN_FUSE_PREFIX_FILL 0
#define KNN_FUSE_SORTED_UNION 1
int knn_eval_fuse(const int64_t *hits_a, const double *scores_a, const uint8_t *keep_a, int64_t ka,
                  const int64_t *hits_b, const double *scores_b, int64_t kb, int64_t nq,
                  int32_t mode, int32_t ascending, int32_t k_out,
                  int64_t *hits_out, double *scores_out, int32_t *source_out, int32_t *filled_out);
/* pfam/pfam.py:349-370 ("TP Set overlap") and 602-625 (auc1s_optimal): two hit lists compared query by query as sets of
 * ids.  hits_a / correct_a are [nq][ka], hits_b / correct_b [nq][kb], tp_out / lead_out [nq][3]; all host arrays,
 * row-major.  correct_x is uint8, a non-zero byte meaning "this hit is a true positive": the matrices of
 * knn_eval_labels and knn_eval_sets_matrix, each list with its own.  Ids are compared as whole int64 values.
 *   entries    an entry exists when its hit is >= 0 (knn_eval_fuse's rule; ragged MMseqs2 rows are padded that way).  An
 *              entry that does not exist is in no set and does not end a leading run.
 *   TP sets    TA = the distinct ids of A's existing entries whose flag is non-zero, TB the same for B from B's own
 *              flags.  An id flagged in one list and not in the other is in one set only; an id that repeats inside a
 *              list is in that list's set when any of its occurrences is flagged.
 *   leading    A's existing entries are walked in column order up to, and without, the first one whose flag is zero; LA
 *              = the distinct ids walked, LB the same for B (the reference's `for j in hits: if correct: add, else:
 *              break`).
 *   outputs    tp_out[q] = (|TA \ TB|, |TA & TB|, |TB \ TA|); lead_out[q] = the same split of LA and LB.  Either may be
 *              NULL, not both.  The sum of lead_out[q] is |LA u LB|, the numerator of the best-case AUC1.
 * The joined walk of pfam.py:629-667 is not here: it is knn_eval_fuse in KNN_FUSE_SORTED_UNION mode with k_out = ka + kb
 * and source_out, followed by a leading-run count over the fused row.
 * KNN_ERR_INVALID, with a message naming the argument, before anything is allocated or launched and with the outputs
 * untouched: nq < 0; ka or kb outside [1, KNN_MAX_K]; a null input pointer; both output pointers null.  nq = 0 returns
 * 0 before any pointer is looked at.  Rows go through the device in slabs of the row count above for k = ka + kb
 * (KNN355_EVAL_SLAB_ROWS included).
 * Hot path: overlap_kernel (overlap.inc), one workgroup per row: the two lead lengths by a workgroup minimum, (id, four
 * membership bits) pairs sorted in LDS over next_pow2(ka + kb) slots, the bits of a run of equal ids OR-ed towards its
 * head by doubling, the heads counted into the six classes.  Integers only, no atomics, plain vector stores. */
int knn_eval_overlap(const int64_t *hits_a, const uint8_t *correct_a, int64_t ka,
                     const int64_t *hits_b, const uint8_t *correct_b, int64_t kb, int64_t nq,
                     int32_t *tp_out /* [nq][3] or NULL */, int32_t *lead_out /* [nq][3] or NULL */);
/* measurement (tools/bench_overlap.py): milliseconds by HIP events of the calling thread's last successful
 * knn_eval_overlap: uploads, kernels, downloads, each summed over the slabs. */
int knn_eval_overlap_last_ms(float *ms /* [3] */);

/* ---- principal components of embedding rows ---------------------------------------
 * pfam/reverse_evaluate.py:34-44, 100-108: sklearn.decomposition.PCA(n_components=2) over the concatenated forward and
 * scrambled embeddings.  The two stateless entries below are its array-sized halves, the mean and covariance of the
 * rows and the projection of rows onto given components; the eigen-solve of the d x d covariance between them is host
 * work (decomposition.py: numpy.linalg.eigh in float64).  All pointers are host pointers; x is float32 [n][d],
 * row-major, and is never written.  d is a multiple of 4 with 4 <= d <= KNN_PCA_MAX_D.
 * "Chain" below means one fp32 fmaf per step with a single rounding, as in oracle/knn_oracle.c.
 *   groups      the rows are cut into consecutive groups of L = 4096 * ceil(n / (4096 * 256)) rows: at most 256 groups,
 *               the last may be short.  L depends on n alone, never on the device, its CU count or a tuning flag.
 *   mean        per column j, a group's sum is the float64 sum of its rows' x[r][j] in ascending row order (starting
 *               from the first row's value); the group sums are added in ascending group order in float64 (starting
 *               from the first group's) and divided by (double)n; mean[j] is that value rounded to float32
 *   centring    xc[r][j] = x[r][j] - mean[j], one fp32 subtraction, applied as rows are loaded and never stored
 *   covariance  for group g and i <= j, P_g[i][j] is the chain over the group's rows in ascending row order,
 *               acc = fmaf(xc[r][i], xc[r][j], acc), starting from +0;
 *               cov[i][j] = (the float64 sum of (double)P_g[i][j] in ascending g, starting from P_0) / (double)(n - 1);
 *               cov[j][i] is a copy of cov[i][j]
 *   projection  out[r][c] is the library's dot chain (blocks of 8 columns in the order 0,4,1,5,2,6,3,7, the last block
 *               zero padded) of xc[r][.] with components[c][.]
 * KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched: a d outside the rule above;
 * a null pointer; knn_pca_moments with n < 2; knn_pca_project with n < 0 or nc outside [1, min(d, KNN_PCA_MAX_COMPONENTS)]
 * (n = 0 returns 0 before any pointer is looked at).  Non-finite input is not refused: it gives non-finite outputs.
 * knn_pca_moments (mean float32 [d], cov float64 [d][d]) keeps the rows on the device for the call, uploaded once on
 * the copy pipeline's host-to-device stream: n * d * 4 bytes, plus groups * d * d * 4 bytes of partial sums.  A failed
 * allocation returns KNN_ERR_HIP with nothing left allocated.  knn_pca_project (out float32 [n][nc]) holds no whole
 * copy: the rows go through the device in slabs of 256 MiB (KNN355_EVAL_SLAB_ROWS sets the rows per slab, as above).
 * Hot paths (pca.inc): pca_colsum_kernel, one thread per (group, column); pca_cov_kernel, one workgroup per (pair of
 * 128-column tiles, group) on v_mfma_f32_32x32x2_f32 with a K step = two consecutive rows; pca_cov_reduce_kernel;
 * pca_project_kernel, one lane per row and one chain per (row, component).  No floating-point atomics. */
#define KNN_PCA_MAX_D 2048
#define KNN_PCA_MAX_COMPONENTS 32
int knn_pca_moments(const float *x, int64_t n, int32_t d, float *mean /* [d] */, double *cov /* [d * d] */);
int knn_pca_project(const float *x, int64_t n, int32_t d, const float *mean, const float *components /* [nc * d] */,
                    int32_t nc, float *out /* [n * nc] */);
/* measurement (tools/bench_pca.py): HIP-event milliseconds of the calling thread's last successful knn_pca_moments,
 * moments_ms[4] = upload, column sums and mean, covariance kernel, reduce, and of its last knn_pca_project, the
 * projection kernel summed over the slabs */
int knn_pca_last_ms(float *moments_ms, float *project_ms);

/* ---- mean pooling over row ranges: per-protein and per-domain embeddings ------------------
 * The step that produces the matrix an index stores: pfam/embed_pfam_seqvec.py:29-40 (embedding[start - 1 : stop]
 * .mean(axis=0) per Pfam domain), pfam/embed_t5_l2.py:68-71 (normalize_L2 on every residue row, then the mean over
 * residues), reduce_per_protein in pfam/embed_pfam_t5.py:40-43, pfam/embed_t5_fp16.py:45-47 and cath/embed.py:92-94.
 * x is the residue matrix [rows][d], float32 (dtype 0) or float16 (dtype 1), and is never written; range o is the rows
 * starts[o] .. stops[o] - 1 (0-based, stop exclusive); ranges may overlap, repeat and come in any order; out is float32
 * [n][d].  The contract, per output o and column c, with L = stops[o] - starts[o]:
 *     acc = v(starts[o], c)                       (the first row's value, not 0 + it: -0.0 survives)
 *     acc = acc + v(r, c)  for r = starts[o] + 1 .. stops[o] - 1 in ascending order: one fp32 add each, no fma, no
 *                          wider accumulator, no reordering
 *     out[o][c] = acc / (float)L                  (one correctly rounded fp32 division)
 * which is numpy's x[start:stop].mean(axis=0) on a C-contiguous float32 array with d >= 2 (tests/test_pool_reference.py
 * checks that claim against numpy itself).  Plain (flags 0): v(r, c) = x[r][c]; float16 converts to float32 exactly.
 * KNN_POOL_NORMALIZE: v(r, c) = x[r][c] * s_r rounded to fp32, s_r being knn_normalize_l2's factor of row r (the fma chain
 * in the order 0,4,1,5,2,6,3,7, s = (float)(1.0 / sqrtf(nrm)); a row whose nrm is not > 0 is used as it is; an infinite nrm
 * gives the factor 0): the result is knn_normalize_l2 followed by the plain pooling, bit for bit.  fp32 subnormals are kept.
 * KNN_ERR_INVALID, with a message, before anything is allocated or launched and with out untouched: dtype other than 0 or
 * 1; flags other than 0 or KNN_POOL_NORMALIZE; d outside [2, KNN_POOL_MAX_D]; rows < 0 or n < 0 or n > 2^31 - 1; a null
 * pointer when n > 0; row_stride < d; (host entry) a range without 0 <= start < stop <= rows or with stop - start >= 2^24.
 * n = 0 returns 0 and launches nothing.
 * knn_pool_ranges: host pointers.  x goes up in chunks (64 MiB; KNN355_POOL_CHUNK_ROWS, a positive decimal integer, sets
 * the rows per chunk) on the copy pipeline's host-to-device stream while the previous chunk is pooled; a range belongs to
 * the chunk that holds it and a range longer than a chunk is a chunk of its own, so a call never holds all of x on the
 * device.  Rows shared by ranges of different chunks go up once per chunk.
 * knn_pool_ranges_dev: device pointers on the current device, work enqueued on `stream` (NULL: the null stream).
 * row_stride is the distance between rows of x in elements; out is contiguous.  The ranges are checked on the device
 * (pool_check_kernel: the same rules) into a status word that the call reads behind its last launch, waiting for an event
 * it records there: a bad range is KNN_ERR_INVALID naming the lowest bad index; its output row is left untouched, no
 * row of x is read for it, and every other output row is written as usual.
 * Hot path (pool.inc): pool_ranges_kernel, one wave per (range, 256 columns), rows walked in order with the loads of eight
 * rows in flight; a range is never split by rows, so few long ranges are latency-bound. */
#define KNN_POOL_NORMALIZE 1
#define KNN_POOL_MAX_D (1 << 20)
int knn_pool_ranges(const void *x_host, int32_t dtype, int64_t rows, int32_t d, const int64_t *starts_host,
                    const int64_t *stops_host, int64_t n, int32_t flags, float *out_host /* [n * d] */);
int knn_pool_ranges_dev(const void *x_dev, int32_t dtype, int64_t rows, int32_t d, int64_t row_stride,
                        const int64_t *starts_dev, const int64_t *stops_dev, int64_t n, int32_t flags, float *out_dev,
                        void *stream);
/* measurement (tools/bench_pool.py): HIP-event milliseconds of the calling thread's last successful knn_pool_ranges
 * (uploads, kernels and the download, each summed over the chunks) or knn_pool_ranges_dev (kernels; the other two are 0) */
int knn_pool_last_ms(float *upload_ms, float *kernel_ms, float *download_ms);

/* ---- one-dimensional Gaussian kernel density estimates -----------------------------------
 * pfam/reverse_evaluate.py:63-70, 113-118, 139-142: DataFrame({...}).plot.density(), which pandas turns into
 * scipy.stats.gaussian_kde(column).evaluate(grid) on a 1000-point grid per column.  Two stateless entries with host
 * pointers: the statistics the bandwidth and the grid are made of, and the evaluation.  Between them the host computes
 * the factor, h = sqrt(var) * factor, inv_h = 1 / h, norm = 1 / (n * h * sqrt(2 pi)) and the grid in float64 (density.py).
 * x is float32 (dtype 0) or float64 (dtype 1) and is never written; column c of row r is x[r * row_stride + c], c < ncols,
 * so a column view of a row-major matrix is (pointer to its first element, ncols 1, row_stride = the matrix's width).
 * Every step below is one IEEE double multiply, add or subtract; nothing is fused.
 *   widening    values are widened to float64 as they are loaded (float32 to float64 is exact)
 *   groups      consecutive groups of L = 4096 * ceil(n / (4096 * 256)) rows, the PCA contract's
 *   min, max    exact (of two zeros of different sign either may be returned)
 *   mean        per column, a group's sum is the float64 sum of its rows in ascending order starting from the first
 *               row's value; the group sums are added in ascending group order starting from the first group's; the
 *               sum is divided by (double)n
 *   var         a second pass over d = x - mean, d * d, summed in the same way and divided by (double)(n - 1)
 *   term        z = (g - x_i) * inv_h;  t = (z * z) * -0.5;  term = kexp(t)
 *   kexp(t)     for t <= 0.  t < -745.0 gives exactly 0.0.  Otherwise k = rint(t * LOG2E) (ties to even),
 *               r = (t - k * LN2_HI) - k * LN2_LO, p = the degree-13 Horner polynomial in r with the coefficients
 *               (double)(1 / i!), every step p = p * r + c_i as a multiply and an add, result ldexp(p, k): exact for
 *               k >= -1021, one rounding (to nearest even) into the subnormal range below that.
 *               LOG2E = 0x1.71547652b82fep+0, LN2_HI = 0x1.62e42fee00000p-1 (low 21 bits zero: k * LN2_HI is exact),
 *               LN2_LO = 0x1.a39ef35793c76p-33.  At most 1.2 ulp from exp (tests/test_kde_reference.py measures it).
 *   sum         per (column, grid point): the rows are cut into chunks of 16 384 consecutive rows.  Inside a chunk there
 *               are 256 partial sums, partial j adding the terms of the rows i with i % 256 == j in ascending i,
 *               starting from +0.0; the 256 partials are combined by the binary tree of adjacent pairs (strides 1, 2,
 *               4, ..., 128: p[j] += p[j + stride] for j a multiple of 2 * stride); the chunk sums are added in chunk
 *               order starting from the first chunk's; out = sum * norm.  The chunk size and the 256 are constants of
 *               this contract, not functions of the device.
 * KNN_ERR_INVALID, before anything is allocated or launched and with the outputs untouched: dtype other than 0 or 1;
 * n < 2 or n > KNN_KDE_MAX_ROWS; ncols outside [1, KNN_KDE_MAX_COLS]; row_stride < ncols; m outside
 * [1, KNN_KDE_MAX_POINTS]; a null pointer; a NaN or an infinity in a used element of x or in the grid; an inv_h or a
 * norm that is not positive and finite (which is what a zero variance or a bad factor gives).
 * Both entries upload the rows as they lie on the host, from the first used element to the last ((n - 1) * row_stride +
 * ncols elements: for a column view of a wide matrix that is the matrix), once per call, on the copy pipeline's
 * host-to-device stream; knn_kde_eval holds ncols * ceil(n / 16384) * m * 8 bytes of chunk sums beside them.
 * Hot path (kde.inc): kde_eval_kernel, one workgroup of 256 threads per (16 grid points, chunk, column), 16 float64
 * accumulators per lane, float64 VALU only (no hardware transcendental, no atomics); kde_reduce_kernel. */
#define KNN_KDE_MAX_COLS 4096
#define KNN_KDE_MAX_ROWS (65535LL * 16384)
#define KNN_KDE_MAX_POINTS (1 << 24)
int knn_kde_stats(const void *x, int32_t dtype, int64_t n, int32_t ncols, int64_t row_stride, double *min /* [ncols] */,
                  double *max, double *mean, double *var /* ddof = 1 */);
int knn_kde_eval(const void *x, int32_t dtype, int64_t n, int32_t ncols, int64_t row_stride,
                 const double *grid /* [ncols * m] */, int64_t m, const double *inv_h /* [ncols] */,
                 const double *norm /* [ncols] */, double *out /* [ncols * m] */);
/* measurement (tools/bench_kde.py): HIP-event milliseconds of the calling thread's last successful knn_kde_stats,
 * stats_ms[2] = upload, kernels, and of its last knn_kde_eval, eval_ms[3] = uploads, evaluation kernel, reduce */
int knn_kde_last_ms(float *stats_ms, float *eval_ms);

/* ---- MMseqs2 prefilter database: SURVEY section 8(f) N3 ----------------------------
 * seqvec_search/mmseqs/_write_prefilter_db.py:52-97 write_prefilter_db: data file
 * ("<prefilter>.0") and index file ("<prefilter>.index"); queries[i] is the faiss row of
 * query i, *_map translate faiss rows to MMseqs2 ids.  clip: 0 = the reference's clip=False
 * (scores * 100 in float32); 1 = clip=True as the reference's pinned numpy 1.22 evaluates
 * numpy.clip(scores, -(10**30), 10**30) * 100 (in double); 2 = clip=True under numpy >= 2
 * (NEP 50: the expression stays float32). */
int knn_write_prefilter_db(const char *data_path, const char *index_path, const int64_t *hits,
                           const float *scores, int64_t nq, int64_t k, const int64_t *queries,
                           const int64_t *test_map, int64_t n_test, const int64_t *train_map,
                           int64_t n_train, int32_t clip);

/* ---- distances for explicit candidate lists (HNSW walk offload) --------
 * For query i (row of q_dev [nq,d]) and candidates cand[off[i] .. off[i+1]),
 * out[p] = <q,y> (IP) or max(0, |q|^2+|y|^2-2<q,y>) (L2), same arithmetic as
 * the flat scan.  Replaces the per-candidate distance computer inside
 * faiss.IndexHNSWFlat (pfam/proteins_search.py:30-31,49). */
int knn_gather_distances(knn_handle h, const float *q_host, int64_t nq, const int64_t *cand_ids,
                         const int64_t *cand_offsets, float *out_host);

/* ---- tuning / introspection (not part of the faiss surface) ------------ */
/* name of the scan kernel the last search on this handle dispatched, and its
 * geometry; used by bench.py for the roofline line */
int knn_last_scan_info(knn_handle h, char *name, int32_t name_len, int32_t *query_tile,
                       int32_t *db_tile, int32_t *nchunks, int32_t *grid);
/* how the last range search on this handle ran: query_blocks = blocks of queries it was split
 * into (each one scan launch), redos = rescans of queries whose per-chunk staging segment
 * overflowed (at most one per query), redo_queries = queries rescanned.  knn_last_scan_info
 * names the range kernel and its geometry. */
int knn_last_range_info(knn_handle h, int64_t *query_blocks, int64_t *redos, int64_t *redo_queries);
/* device time (ms) of the scan kernel launches of the last search, measured
 * with hipEvents on the launch stream */
float knn_last_scan_ms(knn_handle h);
/* durations (ms) of the most recent scan launches (oldest first, at most 64 and at
 * most max_n), each from a hipEvent pair recorded around the launch on the stream it
 * was launched on; -1 for a launch that has not finished.  Returns the count. */
int32_t knn_scan_times(knn_handle h, float *out_ms, int32_t max_n);
/* how the last search on this handle was seeded: seed_stride = 0 (no seed sample), the
 * stride of the sample searched first, or -r (tile-minimum seed: no sample pass, every chunk of the
 * scan publishes r keys per query -- the best key of each of its first r tiles (r = 1, 2) or, for a k beyond
 * what that supports, the best key of each wave's rows of the first tile (r = 4 with the 32-query tile, 2 with the
 * 64-query tile; 4 with the 48-query tile) -- and the k-th smallest published key is the bound); stat_rank = 0 (the sample's k-th score, a proven bound)
 * or j (statistical seed: the sample's j-th score, result verified); stat_redo = searches
 * repeated so far because a statistical threshold failed its verification; sample_rows =
 * rows scanned by the sample pass (the main scan kernel skips them) */
int knn_last_seed_info(knn_handle h, int32_t *seed_stride, int32_t *stat_rank, int64_t *stat_redo,
                       int64_t *sample_rows);
/* knn_set_tuning flags, all off by default.  Only KNN_TUNE_NORM_L2 changes what a search returns (the other formula's
 * rounding); every other combination returns the same bits. */
enum {
    KNN_TUNE_NO_POOL = 2,                /* no shared pool of tiles in a paired (one-query-tile) launch */
    KNN_TUNE_NO_PAIRS = 4,               /* never pair the workgroups of a one-query-tile launch: static chunks instead */
    KNN_TUNE_NO_SEED = 8,                /* no seeding at all (every chunk warms its thresholds up on its own) */
    KNN_TUNE_EXACT_SEED = 16,            /* force the exact seed (a sample pass of its own in front of the scan) */
    /* squared L2 by the norm formula |x|^2 + |y|^2 - 2<x,y> whatever the batch size (default: FAISS's rule -- batches of
     * fewer than 20 queries use the sum of squared differences, larger ones the norm formula) */
    KNN_TUNE_NORM_L2 = 32,
    /* always launch the state-reset kernel in front of a streaming scan (default: the previous search's final selection
     * leaves the state reset when the next search has the same shape) */
    KNN_TUNE_ALWAYS_RESET = 64,
    KNN_TUNE_STAT_SEED = 128,            /* force the statistical seed (synchronous entry points only) */
    KNN_TUNE_NO_TURNS = 256,             /* the two workgroups of a CU do not take turns in their K loops (batch launches) */
    KNN_TUNE_NO_STAT_SEED = 512,         /* never use the statistical seed */
    KNN_TUNE_NO_SYM = 1024,              /* never use the symmetric launch of a whole-index self-search */
    /* never use the tile-minimum seed (a streaming search then runs its seed sample as a launch of its own) */
    KNN_TUNE_NO_TILE_MIN_SEED = 2048,
    /* bits 12-13: publication rounds of the tile-minimum seed (0 = the library's choice), r << KNN_TUNE_PUB_ROUNDS_SHIFT */
    KNN_TUNE_PUB_ROUNDS_SHIFT = 12,
    KNN_TUNE_PUB_ROUNDS_MASK = 3 << 12,
    /* never search the remainder behind the full 128-query tiles as a piece of its own (large databases: 129 queries are one
     * 128-query launch and one streaming launch instead of two 128-query passes) */
    KNN_TUNE_NO_REMAINDER_SPLIT = 16384,
    /* plans without the 48- and 96-query tiles (33..48 queries then pay for a 64-query tile, 65..96 for 128 or two pieces) */
    KNN_TUNE_NO_Q16 = 131072,
    /* never the 256 x 256 tile (one workgroup per CU; the library's choice for synchronous searches of >= 256 queries over
     * >= 65 536 rows with long chunks, always under the statistical seed) */
    KNN_TUNE_NO_BIG_TILE = 262144,
    /* the 256 x 256 tile wherever a batch holds more than 128 queries and the index >= 1024 rows, and 256-row tiles in the
     * symmetric whole-index self-search (tests, A/B) */
    KNN_TUNE_BIG_TILE = 524288,
    KNN_TUNE_NO_SCAN16 = 1 << 20,        /* never the exact 16-bit prefilter (knn_flat_set_scan16), A/B */
    /* the exact 16-bit prefilter wherever it applies, whatever the number of rows (tests; default: from 2^18 rows on) */
    KNN_TUNE_SCAN16_ANY_NB = 1 << 21
};
/* force a scan configuration: query_tile in {0(auto),32,48,64,96,128,256} (48 and 96: the builds on 16-query MFMA blocks, one
 * query tile per launch -- honoured when the batch fits the tile, ignored otherwise); nchunks 0=auto (a forced count also turns the paired
 * walk off); flags: KNN_TUNE_* above */
int knn_set_tuning(knn_handle h, int32_t query_tile, int32_t nchunks, int32_t flags);

/* Exact 16-bit prefilter, opt-in per index, before the first add: mode 1 keeps fp16 copies of the rows (d rounded
 * up to 64 values, one power-of-two exponent per row: +50 % of the fp32 row bytes), rebuilt by every add, knn_flat_reserve,
 * growth and knn_flat_normalize_rows; views share them (copies that move make earlier views stale, as moved rows do).  Streaming searches (one 32-query tile, inner product, >= 2^18 rows) then scan
 * the copies, keep every row a rigorous error bound cannot rule out, re-score those with the fp32 chain and return the same
 * bits as the fp32 scan; a query the bound cannot serve falls back to the fp32 scan on the device.  A row that is not finite
 * turns the path off until knn_reset.  mode 0 (default) = off.  Not for HNSW indexes (KNN_ERR_UNSUPPORTED).  With
 * KNN355_SCAN16=0 in the environment modes 1 and 2 are ignored.
 *   mode 2 keeps 12-bit fixed-point copies INSTEAD of the fp16 ones (+37.5 % of the fp32 row bytes, a quarter fewer bytes per
 * scan): per row an exponent e with max|x| 2^-e in [2^10, 2^11) and n = round-to-nearest-even(x 2^-e) clamped to
 * [-2047, 2047], stored as a byte plane and a nibble plane in tiles of 256 rows.  The integers are exact in fp16, so the scan
 * multiplies exact fp16 values and the same bound holds with a larger measured copy error; the window is wider
 * (k' = min(2048, max(3k, k + 128)) instead of max(2k, k + 64)).  Everything else is mode 1's.  With KNN355_SCAN_FORMAT=16
 * in the environment mode 2 is taken as mode 1 (same-tree A/B). */
int knn_flat_set_scan16(knn_handle h, int32_t mode);
/* used = some piece of the last search took the 16-bit prefilter, candidates_max = the most rows any of its queries
 * re-scored, fallbacks =
 * prefiltered searches of this handle that fell back to the fp32 scan so far.  Waits for the device. */
int knn_last_scan16_info(knn_handle h, int32_t *used, int32_t *candidates_max, int64_t *fallbacks);
/* format = the row copies the last search's prefilter scanned: 16 (fp16), 12 (12-bit), 0 if it did not take the prefilter */
int knn_last_scan16_format(knn_handle h, int32_t *format);

/* Diagnostic entry: makes the index APPROXIMATE ON PURPOSE, as the coarse entry indexes of an HNSW index are.  Before the first
 * add AND before knn_flat_reserve (the row stride changes: an index that already has storage is refused with KNN_ERR_INVALID
 * until knn_reset), not on a view, and not together with knn_flat_set_scan16 or on the storage index of an HNSW index
 * (KNN_ERR_UNSUPPORTED).  Rows are padded to a multiple of 64 values and a bf16
 * copy of every row (round to nearest even) is kept beside the fp32 one; knn_flat_search, knn_flat_search_dev,
 * knn_flat_search_keys_dev and knn_flat_search_self / _self_dev then multiply bf16 copies of rows and queries on the bf16 MFMA
 * (exact products, fp32 accumulation in an order that is not specified) and take the squared-L2 norms from the fp32 values, with
 * the norm formula at every batch size.  knn_flat_reconstruct returns the fp32 rows, knn_flat_normalize_rows converts the copies
 * again.  Every other entry point that reads the rows refuses such a handle with KNN_ERR_UNSUPPORTED before anything is copied
 * or launched: knn_flat_view, knn_flat_refine, knn_lsh_search_refine, knn_flat_range_search / _self, knn_gather_distances,
 * knn_sharded_search_dev, knn_flat_read_rate.  It exists so that the tests can compare the bf16 builds of the scan kernel with
 * a reference of their own arithmetic; nothing else should want it. */
int knn_flat_set_approx16(knn_handle h);

/* A caller that hands one batch of queries over in pieces (its own blocks, one slice per GPU) says how large the
 * whole batch is: FAISS chooses the squared-L2 formula by the batch ITS caller passed to index.search
 * (/root/reference/seqvec_search/main.py:45; fewer than 20 queries: the sum of squared differences), so pieces of
 * fewer than 20 queries of a larger batch keep the norm formula and the pieces return the bits of the one call.
 * nq_whole = 0 (default): every call is its own batch.  The setting stays until changed; it is per handle (views made
 * with knn_flat_view have their own). */
int knn_flat_set_batch(knn_handle h, int64_t nq_whole);

/* Measurement aid (bench.py's roofline): what THIS box's HBM delivers to a plain read kernel over the index's own rows
 * -- grid-stride 16-byte loads, nothing else, the best of `reps` launches at three grid sizes.  best_ms = its duration,
 * bytes_read = ntotal x padded row bytes.  A flat scan cannot be faster than this; boxes of one pool differ by a few
 * percent, the 8 TB/s of the data sheet is not reached by any kernel. */
int knn_flat_read_rate(knn_handle h, int32_t reps, float *best_ms, int64_t *bytes_read);

/* Measurement aid (bench.py's batch roofline): what THIS box's fp32 matrix pipes sustain -- every wave issues
 * back-to-back v_mfma_f32_32x32x2_f32 on independent accumulators, operands in registers (random values), two
 * workgroups per CU, no memory traffic.  Launches run back to back for warm_ms milliseconds first (the chip settles on
 * the clock it holds under this load), then the best of eight is reported: tflops, and clock_mhz (may be NULL) = the
 * in-kernel shader clock of that launch.  The data sheet's dense fp32 MFMA peak is 157.3 TFLOP/s at 2.4 GHz. */
int knn_mfma_rate(int32_t warm_ms, float *tflops, float *clock_mhz);

/* ---- weighted mixes of embedding layers, searched and scored where they lie ---------------
 * cath/compare_seqvec_layer.py:44-56, 87-91: ratio[0] * cnn + ratio[1] * lstm1 + ratio[2] * lstm2 for every point of a
 * simplex grid, each mix through cath.search.search, of which only is_correct[:, 3, 0].mean() is kept;
 * seqvec_search/figures/layers.py:37-47 and lstm1_vs_sum.py: sums, differences and column blocks of one [N, 3072] matrix.
 * A knn_mix handle holds L = 1 .. KNN_MIX_MAX_LAYERS layers of n rows and d columns on the device; they go up once.
 * The contract of a mix with the float32 weights w, per row r and column c:
 *     out[r][c] = ((w[0] * x0[r][c] + w[1] * x1[r][c]) + w[2] * x2[r][c]) + w[3] * x3[r][c]
 * left to right over the L layers, every product and every sum rounded to float32 on its own (no fma, no wider
 * accumulator): numpy's statement on float32 arrays with float32 weights, bit for bit (numpy 1.x casts the float64 scalars
 * of the reference's grid to float32 by value; tests/layer_mix_reference.py does it by hand).  A zero weight's term is
 * computed like any other: 0 * inf is NaN, 0 * x + y follows IEEE.
 * knn_mix_set_layer copies layer i from host rows x_host + r * row_stride (row_stride >= d in floats, so that a column
 * block of a [n, L * d] matrix is a layer); knn_mix_set_layer_dev borrows rows that already lie on the device: nothing is
 * copied, the caller keeps them alive and unchanged while the handle uses them, `stream` (the one that produced them) is
 * waited for.  All layers have the same n: a layer with another n is refused while another layer is set.
 * knn_mix_into makes `flat` hold the mix: it is reset, n rows are reserved, the rows are written by mix_rows_kernel at the
 * index's padded stride and then go through what knn_flat_add_dev does behind its copy (norms, the row copies of
 * knn_flat_set_scan16 / an approximate index, views of the old rows stale); with normalize != 0 the rows are normalised as
 * by knn_flat_normalize_rows first.  Afterwards `flat` cannot be told from an index that had knn_flat_add(mix) and
 * knn_flat_normalize_rows called on it.
 * knn_mix_sweep does, for each of the G weight rows, knn_mix_into (normalised when flat's metric is the inner product, as
 * cath.search.search does), knn_flat_search_self_dev with k neighbours and mix_top1_kernel: counts_out[g][l] = the number of
 * rows q with mapping[q][l] == mapping[I[q][column]][l] (mapping: int32 [n][nlevels] on the host; a hit < 0 or >= n is
 * wrong, knn_eval_levels' rule; column 1 is the first hit behind the self hit).  Integer counting: exact, whatever the
 * order.  D_host / I_host: both NULL, and only the counts leave the device, or both given, [G][n][k] scores and ids.
 * KNN_ERR_INVALID before anything is allocated, copied or launched, outputs untouched: a null handle or pointer, a layer
 * without rows, flat's dimension other than d, flat a view or on another device, nlayers outside 1 .. KNN_MIX_MAX_LAYERS
 * (knn_mix_create), k outside 1 .. KNN_MAX_K, column outside 0 .. k - 1, nlevels outside 1 .. KNN_MIX_MAX_LEVELS, only one
 * of D_host / I_host.
 * knn_mix_last_ms: HIP-event milliseconds of the calling thread's last successful knn_mix_sweep, summed over its mixes --
 * knn_mix_into's launches, the self-search (host gaps included), the scoring kernel; after knn_mix_into the first alone. */
#define KNN_MIX_MAX_LAYERS 4
#define KNN_MIX_MAX_LEVELS 8
typedef struct knn_mix_s *knn_mix_handle;
int knn_mix_create(int32_t d, int32_t nlayers, knn_mix_handle *out);
void knn_mix_free(knn_mix_handle h);
int knn_mix_set_layer(knn_mix_handle h, int32_t i, const float *x_host, int64_t n, int64_t row_stride);
int knn_mix_set_layer_dev(knn_mix_handle h, int32_t i, const float *x_dev, int64_t n, int64_t row_stride, void *stream);
int knn_mix_into(knn_mix_handle h, const float *weights /* [nlayers] */, knn_handle flat, int32_t normalize);
int knn_mix_sweep(knn_mix_handle h, const float *weights /* [G][nlayers] */, int64_t G, knn_handle flat, int64_t k,
                  const int32_t *mapping /* [n][nlevels] */, int32_t nlevels, int64_t column,
                  int64_t *counts_out /* [G][nlevels] */, float *D_host, int64_t *I_host);
int knn_mix_last_ms(float *mix_ms, float *search_ms, float *score_ms);

#ifdef __cplusplus
}
#endif
#endif /* KNN355_H */
