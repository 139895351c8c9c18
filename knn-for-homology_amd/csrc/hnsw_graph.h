// hnsw_graph.h -- the host side of the HNSW graph that needs no GPU: the level table and the neighbour lists, the walkers'
// visited set and heaps.  Standard library only: csrc/hnsw_check.cpp compiles it without HIP (tests/test_hnsw_graph_cpu.py).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <random>
#include <utility>
#include <vector>

#define HNSW_EMPTY 0xFFFFFFFFu // "no link" in a neighbour list, "no row" in a list of ids

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

// The order an add call links its rows [n0, n0 + n) in: shuffled (Fisher-Yates on the standard's mt19937: the same on every
// platform), a fixed function of (first row, count) -- the build stays deterministic.  The insertion order is seeded by
// (n0, n): the graph depends on how the rows are split over add() calls.
static inline std::vector<int64_t> hnsw_link_order(int64_t n0, int64_t n, bool shuffle)
{
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; i++) order[(size_t)i] = n0 + i;
    if (shuffle) {
        std::mt19937 rng((uint32_t)(789u + (uint64_t)n0 * 2654435761u));
        for (int64_t i = n - 1; i > 0; i--) std::swap(order[(size_t)i], order[(size_t)(rng() % (uint64_t)(i + 1))]);
    }
    return order;
}

// Rows of the next batch of an add call of n rows, pos of them behind it, `done` nodes linked so far.  Batches grow with
// the graph: a batch never exceeds a quarter of what is already linked
// ... nor 1/32 of its add call (32 rows at least): a call that brings one family -- rows added file by file -- is
// linked in 32 batches, the later ones see the earlier ones (recall@50 0.992 against 0.83 with whole calls as batches,
// tools/hnsw_sorted_probe.py).  The price: a small call into a large graph (1000 rows) is 32 batches of 32 rows, each
// a full device pipeline (~1 ms): incremental adds of a few hundred rows cost ~30 ms per call whatever they bring.
// (The very first row of an empty graph is a batch of its own, the entry point: the caller's special case.)
static inline int64_t hnsw_batch_rows(int64_t done, int64_t n, int64_t pos, int64_t max_batch)
{
    int64_t b = std::max<int64_t>(1, std::min<int64_t>(max_batch, done / 4));
    b = std::min(b, std::max<int64_t>(32, n / 32));
    return std::min(b, n - pos);
}
