// knn355_lib.hip -- the one translation unit of libknn355.so: the flat search's device code, the host side of the flat
// index in its order of definition, then one file per feature.  Nothing but #include lines lives here; a new feature adds
// its line at the end and leaves knn355.hip (the device code the benchmark pins by hash) alone.
// (hnsw_kernels.inc itself includes hnsw_graph.h first, for HNSW_EMPTY: the host graph is parsed before the kernels, and the
// hnsw_graph.h line below is a no-op kept to name the file.)
#include "knn355.hip"      // system + project headers, the arithmetic contract, every kernel of the flat search
#include "host_core.inc"   // errors, what one call owns, pools, DevBuf / scratch, knn_index_s, knn_init, normalize
#include "flat_index.inc"  // create, view, free, reset, grow, add, reconstruct
#include "flat_search.inc" // launch_select, kernel picking, search_view, the device and host search entries
#include "flat_info.inc"   // knn_last_* and tuning entries, reserve, set_scan16, the rate probes, gather_distances
#include "comm.inc"        // RCCL inside the library: knn_sharded_search_dev
#include "hnsw_kernels.inc" // IndexHNSWFlat: every kernel (pair distances, pruning, the level-0 beam, level-0 links on the device)
#include "hnsw_graph.h"     // ... the host graph, the walkers' visited set and heaps, link order and batch schedule: no HIP
#include "hnsw_state.inc"   // ... PinnedBuf, knn_hnsw_s and its buffer lists, the KNN355_HNSW_* knobs, host threads, profile
#include "hnsw_build.inc"   // ... host walkers, device mirror, the beam pipeline, candidates, a batch's links, add
#include "hnsw_search.inc"  // ... search on the device and on the host walkers
#include "hnsw_api.inc"     // ... create, free, setters, getters, graph export / import, stats
#include "refine.inc"
#include "lsh.inc"
#include "eval.inc"
#include "assemble.inc"
#include "slices_eval.inc"
#include "pr_curve.inc"
#include "buckets.inc"
#include "rank.inc"
#include "windows.inc"
#include "bootstrap.inc"
#include "pca.inc"
#include "fuse.inc"
#include "overlap.inc"
#include "range.inc"
#include "pool.inc"
#include "kde.inc"
#include "mix.inc"
#include "correlate.inc"
