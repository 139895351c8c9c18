// hnsw_check.cpp -- the HIP-free host code of hnsw_graph.h as a stand-alone program under ASan/UBSan (make hnsw_check;
// tests/test_hnsw_graph_cpu.py compares what it prints with tests/hnsw_build_reference.py):
//   hnsw_check levels M             cum_nb of HnswGraph::init(M), one line
//   hnsw_check order n0 n shuffle   the link order of an add call, one line
//   hnsw_check batches done n max   the batch sizes of an add call of n rows onto `done` linked nodes, walked as
//                                   hnsw_link_rows walks it (the first row of an empty graph is a batch of its own)
//   hnsw_check self                 VisitedSet hash mode against bitmap mode, heap_replace_top against the standard heap calls
#include "hnsw_graph.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>

static int self_check()
{
    std::mt19937 rng(2024);
    // 2000 inserts of ids below 4096 with repeats: ~1600 distinct ids, the hash table doubles several times from 64 slots
    VisitedSet hash, bits;
    hash.reset(1, 4096, false);
    bits.reset(1, 4096, true);
    const size_t cap0 = hash.tab.size();
    for (int i = 0; i < 2000; i++) {
        const uint32_t v = rng() % 4096u;
        const bool a = hash.insert(v), b = bits.insert(v);
        if (a != b) {
            printf("visited: insert %d of id %u: hash says %d, bitmap says %d\n", i, v, (int)a, (int)b);
            return 1;
        }
    }
    if (cap0 != 64 || hash.tab.size() < 8 * cap0) {
        printf("visited: the table started at %zu slots and ended at %zu: grow() was not exercised\n", cap0, hash.tab.size());
        return 1;
    }
    // 1000 random (v, id) with tied distances (v takes 50 values) pushed through a heap of 64 entries
    std::vector<DistId> mine, ref;
    for (int i = 0; i < 1000; i++) {
        const DistId e((float)(rng() % 50u) * 0.25f, rng() % 100000u);
        if (mine.size() < 64) {
            mine.push_back(e);
            std::push_heap(mine.begin(), mine.end());
            ref.push_back(e);
            std::push_heap(ref.begin(), ref.end());
        } else if (e < mine.front()) {
            heap_replace_top(mine, e);
            std::pop_heap(ref.begin(), ref.end());
            ref.pop_back();
            ref.push_back(e);
            std::push_heap(ref.begin(), ref.end());
        }
        std::vector<DistId> a = mine, b = ref;
        std::sort(a.begin(), a.end());
        std::sort(b.begin(), b.end());
        if (a != b || !std::is_heap(mine.begin(), mine.end())) {
            printf("heap: contents differ after step %d\n", i);
            return 1;
        }
    }
    printf("self ok\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 3 && !strcmp(argv[1], "levels")) {
        HnswGraph g;
        g.init(atoi(argv[2]));
        for (int c : g.cum_nb) printf("%d ", c);
        printf("\n");
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "order")) {
        for (int64_t id : hnsw_link_order(atoll(argv[2]), atoll(argv[3]), atoi(argv[4]) != 0)) printf("%lld ", (long long)id);
        printf("\n");
        return 0;
    }
    if (argc == 5 && !strcmp(argv[1], "batches")) {
        int64_t done = atoll(argv[2]);
        const int64_t n = atoll(argv[3]), max_batch = atoll(argv[4]);
        bool have_entry = done > 0;
        for (int64_t pos = 0; pos < n;) {
            int64_t b = hnsw_batch_rows(done, n, pos, max_batch);
            if (!have_entry) b = 1; // (the entry point: no links yet)
            have_entry = true;
            printf("%lld ", (long long)b);
            pos += b;
            done += b;
        }
        printf("\n");
        return 0;
    }
    if (argc == 2 && !strcmp(argv[1], "self")) return self_check();
    fprintf(stderr, "usage: hnsw_check levels M | order n0 n shuffle | batches done n max_batch | self\n");
    return 2;
}
