"""GPU: IndexHNSWFlat (level-0 beam search and construction candidates on the device, exact coarse entry scan,
beam rows re-scored with the flat search's arithmetic).  FAISS's own HNSW graph is not
deterministic under OpenMP, so parity is stated the way the north star does: recall@k
against the exact flat search, plus bit-equality of every returned distance with the flat
kernel's distance for the same (query, row)."""
from pathlib import Path

import numpy as np
import pytest

from conftest import GOLDEN
from hnsw_reference import assert_output_contract

pytestmark = pytest.mark.gpu


def _clustered(n, d, ncent, seed):
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((ncent, d), dtype=np.float32)
    x = cent[rng.integers(0, ncent, n)] + 0.35 * rng.standard_normal((n, d), dtype=np.float32)
    return x


def _recall(I, It):
    return sum(len(np.intersect1d(a[a >= 0], b)) for a, b in zip(I, It)) / It.size


def test_fixture_exact_when_ef_exceeds_ntotal(gpu_faiss, oracle):
    """pfam-20-10 (200 rows): ef = 256 >= ntotal, so the walk visits the whole connected
    graph and must return exactly the flat result (reference setting: M = 42, inner
    product, efSearch = 256 -- pfam/proteins_search.py:30-31)."""
    x = np.load(GOLDEN / "pfam-20-10" / "train.npy")
    q = np.load(GOLDEN / "pfam-20-10" / "test.npy")
    gpu_faiss.normalize_L2(x)
    gpu_faiss.normalize_L2(q)
    idx = gpu_faiss.IndexHNSWFlat(1024, 42, gpu_faiss.METRIC_INNER_PRODUCT)
    idx.hnsw.efSearch = 256
    idx.train(x)
    idx.add(x)
    assert idx.ntotal == 200 and idx.hnsw.efSearch == 256 and idx.hnsw.M == 42
    D, I = idx.search(q, 10)
    Do, Io = oracle.flat_search(x, q, 10, 0)
    assert np.array_equal(I, Io) and np.array_equal(D.view(np.uint32), Do.view(np.uint32))
    # k > ntotal: the tail is id -1
    D, I = idx.search(q[:3], 230)
    assert (I[:, 200:] == -1).all() and (np.sort(I[:, :200], axis=1) == np.arange(200)).all()


@pytest.mark.parametrize("metric", [0, 1])
def test_recall_and_distance_bits(gpu_faiss, oracle, metric):
    n, d, nq = 20000, 256, 1000
    x = _clustered(n, d, 200, 21)
    gpu_faiss.normalize_L2(x)
    flat = gpu_faiss.IndexFlat(d, metric)
    flat.add(x)
    Dt, It = flat.search(x[:nq], 100)
    idx = gpu_faiss.IndexHNSWFlat(d, 32, metric)
    idx.add(x)
    idx.hnsw.efSearch = 256
    D, I = idx.search(x[:nq], 100)
    assert _recall(I, It) >= 0.97
    # every returned (id, distance) equals the flat kernel's value for that pair, bit for bit
    # (squared L2: the walk's rows are re-scored with the sum of squared differences whatever the batch size, as FAISS's
    # HNSW distance computer does -- the formula a flat search uses for fewer than 20 queries, as here)
    full = gpu_faiss.IndexFlat(d, metric)
    full.add(x)
    Dall, Iall = full.search(x[:16], 2048)
    for qi in range(16):
        ref = dict(zip(Iall[qi].tolist(), Dall[qi].view(np.uint32).tolist()))
        for j, v in zip(I[qi].tolist(), D[qi].view(np.uint32).tolist()):
            if j in ref:
                assert ref[j] == v
    assert_output_contract(D, I, x, x[:nq], metric, n, oracle)
    # order: best first, ties by id
    if metric == 0:
        assert (np.diff(D, axis=1) <= 0).all()
    else:
        assert (np.diff(D, axis=1) >= 0).all()
    # efSearch trades recall for work
    idx.hnsw.efSearch = 16
    _, I16 = idx.search(x[:nq], 10)
    idx.hnsw.efSearch = 128
    _, I128 = idx.search(x[:nq], 10)
    assert _recall(I128, It[:, :10]) >= _recall(I16, It[:, :10]) >= 0.8


@pytest.mark.parametrize("metric", [0, 1])
def test_entry_modes_and_host_walk_agree_in_quality(gpu_faiss, oracle, metric, monkeypatch):
    """Three ways to walk the same graph: coarse exact entry scan + device beam (default), greedy descent + device beam
    (set_entry(0)), and the host beam of round 1.  All return flat-exact distances for the rows they find and reach the
    same recall within two points; the default must not be the worst."""
    n, d, nq, k = 30000, 128, 800, 50
    x = _clustered(n, d, 300, 77)
    gpu_faiss.normalize_L2(x)
    flat = gpu_faiss.IndexFlat(d, metric)
    flat.add(x)
    Dt, It = flat.search(x[:nq], k)
    idx = gpu_faiss.IndexHNSWFlat(d, 32, metric)
    idx.add(x)
    idx.hnsw.efSearch = 128
    rec = {}
    for name, entries in (("coarse", 4), ("descent", 0)):
        idx.set_entry(entries)
        D, I = idx.search(x[:nq], k)
        rec[name] = _recall(I, It)
        # (squared L2: the HNSW index scores with the sum of squared differences -- the flat search's formula for batches of
        # fewer than 20 queries: the reference values come from searches of 10 queries each)
        Dr = np.concatenate([flat.search(x[r0:r0 + 10], k)[0] for r0 in range(0, 50, 10)]) if metric == 1 else Dt
        Ir = np.concatenate([flat.search(x[r0:r0 + 10], k)[1] for r0 in range(0, 50, 10)]) if metric == 1 else It
        ref = [dict(zip(Ir[r].tolist(), Dr[r].view(np.uint32).tolist())) for r in range(50)]
        for r in range(50):
            for j, v in zip(I[r].tolist(), D[r].view(np.uint32).tolist()):
                if j in ref[r]:
                    assert ref[r][j] == v
        assert_output_contract(D, I, x, x[:nq], metric, n, oracle)
        assert (np.diff(D, axis=1) <= 0).all() if metric == 0 else (np.diff(D, axis=1) >= 0).all()
    assert rec["coarse"] >= 0.95 and rec["coarse"] >= rec["descent"] - 0.02, rec


@pytest.mark.parametrize("d", [128, 100])
def test_bf16_coarse_scan_matches_fp32_coarse_scan_in_quality(gpu_faiss, oracle, d, monkeypatch):
    """The coarse entry scan multiplies bf16 copies of the rows above level 0 (entry points only need the neighbourhood;
    the beam's rows are re-scored in fp32).  Same graph quality and recall as the fp32 coarse scan
    (KNN355_HNSW_COARSE_FP32=1), distances still flat-exact; d = 100 exercises the padding to 64 values."""
    n, nq, k = 30000, 800, 50
    x = _clustered(n, d, 300, 5)
    gpu_faiss.normalize_L2(x)
    flat = gpu_faiss.IndexFlat(d, 0)
    flat.add(x)
    Dt, It = flat.search(x[:nq], k)
    rec = {}
    for name, env in (("bf16", "0"), ("fp32", "1")):
        monkeypatch.setenv("KNN355_HNSW_COARSE_FP32", env)
        idx = gpu_faiss.IndexHNSWFlat(d, 32, 0)
        idx.add(x)
        idx.hnsw.efSearch = 128
        D, I = idx.search(x[:nq], k)
        rec[name] = _recall(I, It)
        for r in range(50):
            ref = dict(zip(It[r].tolist(), Dt[r].view(np.uint32).tolist()))
            for j, v in zip(I[r].tolist(), D[r].view(np.uint32).tolist()):
                if j in ref:
                    assert ref[j] == v
        assert_output_contract(D, I, x, x[:nq], 0, n, oracle)
    assert rec["bf16"] >= 0.95 and abs(rec["bf16"] - rec["fp32"]) <= 0.01, rec


def test_rows_wider_than_the_device_beam_use_the_host_walk(gpu_faiss, oracle):
    """The device beam serves rows of up to 1024 floats; wider embeddings (ESM-1b: 1280) fall back to the host walk with
    GPU distance batches -- same contract (flat-exact distances, -1 padding), recall against the flat search."""
    n, d, nq, k = 4000, 1280, 200, 20
    x = _clustered(n, d, 40, 3)
    gpu_faiss.normalize_L2(x)
    flat = gpu_faiss.IndexFlat(d, 0)
    flat.add(x)
    Dt, It = flat.search(x[:nq], k)
    idx = gpu_faiss.IndexHNSWFlat(d, 16, 0)
    idx.add(x)
    idx.hnsw.efSearch = 128
    D, I = idx.search(x[:nq], k)
    assert _recall(I, It) >= 0.95 and (I[:, 0] == np.arange(nq)).mean() > 0.97
    for r in range(20):
        ref = dict(zip(It[r].tolist(), Dt[r].view(np.uint32).tolist()))
        for j, v in zip(I[r].tolist(), D[r].view(np.uint32).tolist()):
            if j in ref:
                assert ref[j] == v
    assert_output_contract(D, I, x, x[:nq], 0, n, oracle)


def test_add_dev_builds_the_same_graph(gpu_faiss):
    """knn_hnsw_add_dev (rows already on the device, no host copy of the database) links the same graph as add()."""
    import torch
    n, d = 9000, 64
    x = _clustered(n, d, 90, 12)
    a = gpu_faiss.IndexHNSWFlat(d, 16, 0)
    a.add(x)
    b = gpu_faiss.IndexHNSWFlat(d, 16, 0)
    xd = torch.from_numpy(x).to("cuda:0")
    b.add_dev(xd[:5000].contiguous())
    b.add_dev(xd[5000:].contiguous())
    c = gpu_faiss.IndexHNSWFlat(d, 16, 0)
    c.add(x[:5000])
    c.add(x[5000:])
    assert b.ntotal == n and np.array_equal(b.graph()[2], c.graph()[2]), "same rows in the same two calls: same graph"
    assert np.array_equal(b.reconstruct_n(0, n), x)
    Da, Ia = a.search(x[:200], 10)
    Db, Ib = b.search(x[:200], 10)
    assert _recall(Ib, Ia) > 0.9  # (one call vs two calls batch the insertions differently: close, not identical)


def test_graph_invariants_and_determinism(gpu_faiss):
    n, d, M = 6000, 64, 16
    x = _clustered(n, d, 50, 5)
    a = gpu_faiss.IndexHNSWFlat(d, M, 1)
    a.add(x)
    levels, offsets, nbrs, cum, probas = a.graph()
    assert levels.shape == (n,) and offsets[-1] == nbrs.size and cum[1] == 2 * M and cum[2] - cum[1] == M
    assert levels.max() == a.hnsw.max_level and levels[a.hnsw.entry_point] == levels.max()
    assert nbrs.max() < n and nbrs.min() >= -1
    # level populations fall roughly geometrically
    assert (levels >= 1).mean() < 0.15
    for i in range(0, n, 37):
        for l in range(levels[i] + 1):
            lst = nbrs[offsets[i] + cum[l]: offsets[i] + cum[l + 1]]
            used = lst[lst >= 0]
            assert (lst[len(used):] == -1).all(), "neighbour lists are packed to the front"
            assert i not in used and len(set(used.tolist())) == len(used)
            assert (levels[used] >= l).all(), "links stay inside their level"
    # the build is deterministic (batch-synchronous), two adds give the same result as one
    b = gpu_faiss.IndexHNSWFlat(d, M, 1)
    b.add(x)
    assert np.array_equal(b.graph()[2], nbrs)


@pytest.mark.parametrize("metric,M,d,n,pieces,efc", [(0, 16, 64, 60_000, 1, 40), (1, 8, 96, 40_000, 3, 40), (0, 42, 256, 30_000, 2, 40),
                                                     (1, 24, 64, 30_000, 1, 150), (0, 63, 32, 24_000, 1, 40), (1, 2, 16, 12_000, 2, 40)])
def test_device_links_build_the_host_links_graph(gpu_faiss, monkeypatch, metric, M, d, n, pieces, efc):
    """Construction keeps level 0 on the device since round 4 (candidates, forward selection, forward links, reverse requests
    sorted by (node, v, from), appended or pruned: hnsw_build.inc::hnsw_level0_links_device); KNN355_HNSW_HOST_LINKS=1 is the
    host bookkeeping of rounds 1-3.  Same arithmetic, same request order, same members per pruning group: the two graphs
    are IDENTICAL -- every list of every level -- and so are the search results.  (M = 8: small lists, almost every reverse
    request prunes; several add calls: the device's lists outlive a call and the host copy is brought up to date in between
    only when something reads it.)"""
    x = _clustered(n, d, max(40, n // 300), 31 + M)
    # exact duplicates inside one insertion batch and across batches: two points then ask the same node for a reverse link
    # at the same distance, and the order of the requests (node, v, from) decides who is appended first / pruned
    x[n - 3000:n - 2000] = x[n - 2000:n - 1000]
    x[n // 2:n // 2 + 500] = x[:500]
    cuts = [n * i // pieces for i in range(pieces + 1)]

    def build():
        idx = gpu_faiss.IndexHNSWFlat(d, M, metric)
        idx.hnsw.efConstruction = efc  # (150: more candidates than a selection group holds -- the closest 127 take part)
        for a, b in zip(cuts[:-1], cuts[1:]):
            idx.add(x[a:b])
        return idx

    monkeypatch.setenv("KNN355_HNSW_HOST_LINKS", "1")
    host = build()
    monkeypatch.delenv("KNN355_HNSW_HOST_LINKS")
    dev = build()
    q = np.ascontiguousarray(x[::97][:300])
    Dd, Id = dev.search(q, 10)      # (searched BEFORE the graph is exported: the device's lists as they are)
    gh, gd = host.graph(), dev.graph()
    assert np.array_equal(gh[0], gd[0]) and np.array_equal(gh[1], gd[1])
    diff = np.flatnonzero(gh[2] != gd[2])
    assert diff.size == 0, f"{diff.size} of {gh[2].size} slots differ, first at {diff[:5]}"
    Dh, Ih = host.search(q, 10)
    assert np.array_equal(Ih, Id) and np.array_equal(Dh.view(np.uint32), Dd.view(np.uint32))
    # and the graph that went through the export is still the one the device searches
    Dd2, Id2 = dev.search(q, 10)
    assert np.array_equal(Id2, Id)


def test_rows_grouped_by_cluster_are_linked_like_shuffled_rows(gpu_faiss, monkeypatch):
    """A Pfam FASTA lists its families one after the other, so the rows of `full_sequences.npy`
    (pfam/proteins_search.py:18-22) arrive GROUPED.  The build is batch-synchronous -- a batch is linked against the frozen
    graph only -- and until round 4 it took the rows in their own order: a family that arrived inside one batch was
    inserted blind to itself (200 k rows in clusters of 2000: recall@100 0.25 against 0.98 for the same rows shuffled).
    Rows are now linked in a shuffled order (as FAISS's hnsw_add_vertices does, "to get rid of dataset order bias"):
    grouped and shuffled rows give the same recall; KNN355_HNSW_ORDER=sequential is the old order and shows the defect."""
    n, d, per, M, k = 60_000, 64, 1000, 16, 50
    rng = np.random.default_rng(9)
    cent = rng.standard_normal((n // per, d)).astype(np.float32)
    x = cent[np.repeat(np.arange(n // per), per)] + 0.35 * rng.standard_normal((n, d)).astype(np.float32)
    gpu_faiss.normalize_L2(x)
    shuffled = np.ascontiguousarray(x[rng.permutation(n)])

    def recall_of(rows, calls=1):
        idx = gpu_faiss.IndexHNSWFlat(d, M, 0)
        for c in range(calls):
            idx.add(rows[n * c // calls:n * (c + 1) // calls])
        idx.hnsw.efSearch = 128
        flat = gpu_faiss.IndexFlat(d, 0)
        flat.add(rows)
        q = np.ascontiguousarray(rows[::29][:1500])
        _, It = flat.search(q, k)
        _, I = idx.search(q, k)
        return _recall(I, It)

    r_grouped, r_shuffled = recall_of(x), recall_of(shuffled)
    # the same rows added family by family, one `add` call each (a call is linked in eight batches at least: the later
    # ones see the earlier ones)
    r_calls = recall_of(x, calls=n // per)
    print(f"recall@{k}: one add call per cluster {r_calls:.4f}")
    assert r_calls >= r_shuffled - 0.02, (r_calls, r_shuffled)
    monkeypatch.setenv("KNN355_HNSW_ORDER", "sequential")
    r_old = recall_of(x)
    print(f"recall@{k}: grouped rows {r_grouped:.4f}, the same rows shuffled {r_shuffled:.4f}, grouped rows linked in their own order {r_old:.4f}")
    assert r_shuffled >= 0.9 and r_grouped >= r_shuffled - 0.01, (r_grouped, r_shuffled)
    assert r_old < r_grouped - 0.05, "the rows' own order should show the defect this test is about"


def test_an_index_read_from_a_file_takes_more_rows(gpu_faiss, tmp_path):
    """read_index imports the graph (every node linked, the device's lists rebuilt from the file's); rows added afterwards are
    linked into it like rows added to the index that wrote the file.  (Not the SAME graph: the level generator's state is
    not part of a FAISS file, the new nodes draw other levels -- the same quality.)"""
    n0, n1, d, M, k = 30_000, 12_000, 64, 16, 20
    x = _clustered(n0 + n1, d, 300, 41)
    a = gpu_faiss.IndexHNSWFlat(d, M, 0)
    a.add(x[:n0])
    path = str(tmp_path / "first.index")
    gpu_faiss.write_index(a, path)
    b = gpu_faiss.read_index(path)
    assert np.array_equal(a.graph()[2], b.graph()[2])
    a.add(x[n0:])
    b.add(x[n0:])
    assert a.ntotal == b.ntotal == n0 + n1
    levels, offsets, nbrs, cum, _ = b.graph()
    for i in range(n0, n0 + n1, 97):  # every new node is linked on level 0
        assert (nbrs[offsets[i]:offsets[i] + cum[1]] >= 0).sum() >= 1
    q = np.ascontiguousarray(x[::37][:800])
    a.hnsw.efSearch = b.hnsw.efSearch = 128
    flat = gpu_faiss.IndexFlat(d, 0)
    flat.add(x)
    It = flat.search(q, k)[1]
    ra, rb = _recall(a.search(q, k)[1], It), _recall(b.search(q, k)[1], It)
    assert ra >= 0.95 and rb >= ra - 0.01, (ra, rb)
    # and it can be written and read once more
    path2 = str(tmp_path / "second.index")
    gpu_faiss.write_index(b, path2)
    c = gpu_faiss.read_index(path2)
    c.hnsw.efSearch = 128
    assert np.array_equal(c.search(q, k)[1], b.search(q, k)[1])


def test_a_search_of_several_batches_equals_its_pieces(gpu_faiss):
    """IndexHNSWFlat.search walks 16384 queries at a time; with several batches the results of batch b - 1 are downloaded
    on the copy stream while batch b is walked (two sets of result buffers).  40 000 queries in one call = the same queries
    in calls of one batch each, bit for bit -- and every row finds itself."""
    n, d, M, k = 40_000, 48, 12, 30
    x = _clustered(n, d, 200, 77)
    idx = gpu_faiss.IndexHNSWFlat(d, M, 1)
    idx.add(x)
    idx.hnsw.efSearch = 64
    D, I = idx.search(x, k)
    assert (I[:, 0] == np.arange(n)).mean() > 0.98 and (D[I[:, 0] == np.arange(n), 0] == 0).all()
    for a in range(0, n, 16384):
        b = min(n, a + 16384)
        Dp, Ip = idx.search(x[a:b], k)
        assert np.array_equal(Ip, I[a:b]) and np.array_equal(Dp.view(np.uint32), D[a:b].view(np.uint32)), (a, b)


def test_upper_levels_are_linked_on_a_graph_with_many_levels(gpu_faiss):
    """construction candidates of the levels >= 2 come from one top-2048 scan of the coarse index filtered
    by level; once the coarse index outgrows 2048 rows the highest levels' nodes are too rare in that scan (here: M = 4,
    120 k rows -> ~30 k coarse rows, ~470 nodes of level >= 4, ~30 of them among 2048 < efConstruction) and the points
    of those levels must fall back to the host walkers -- or they end up with few or no links on their upper levels, which
    FAISS's greedy descent (set_entry(0), IHNf files read by the real faiss) cannot cross.  Checks every node's fill on
    every level it has, and that the descent entry still finds its way."""
    n, d, M = 120_000, 32, 4
    x = _clustered(n, d, 400, 11)
    idx = gpu_faiss.IndexHNSWFlat(d, M, 0)
    idx.add(x)
    levels, offsets, nbrs, cum, probas = idx.graph()
    assert levels.max() >= 4, "the test needs a tall graph"
    report = {}
    for l in range(1, levels.max() + 1):
        members = np.flatnonzero(levels >= l)
        if len(members) < 2:
            continue
        empty = [int(i) for i in members if nbrs[offsets[i] + cum[l]] < 0]
        fill = float(np.mean([(nbrs[offsets[i] + cum[l]: offsets[i] + cum[l + 1]] >= 0).sum() for i in members[:2000]]))
        report[l] = (len(members), len(empty), round(fill, 2))
        # (a node inserted while its level was still empty has no one to link to: at most the first of each level)
        assert len(empty) <= 1, f"level {l}: {len(empty)} of {len(members)} nodes have no link on it"
        assert fill >= min(M, len(members) - 1) * 0.5, (l, fill)
    print("level: (nodes, without links, mean links)", report)
    flat = gpu_faiss.IndexFlat(d, 0)
    flat.add(x)
    q = np.ascontiguousarray(x[::151][:600])
    _, It = flat.search(q, 10)
    idx.hnsw.efSearch = 64
    rec = {}
    for name, entries in (("coarse", 4), ("descent", 0)):
        idx.set_entry(entries)
        _, I = idx.search(q, 10)
        rec[name] = _recall(I, It)
    print("recall@10 by entry mode", rec)
    # (M = 4 is a thin graph: the descent lands in a neighbouring cluster more often than the exact coarse scan does)
    assert rec["descent"] >= 0.7 and rec["coarse"] >= 0.85, rec


def test_write_read_index_roundtrip(gpu_faiss, tmp_path):
    n, d = 3000, 96
    x = _clustered(n, d, 30, 9)
    for make in (lambda: gpu_faiss.IndexFlat(d, 0), lambda: gpu_faiss.IndexFlat(d, 1),
                 lambda: gpu_faiss.IndexHNSWFlat(d, 12, 1)):
        idx = make()
        idx.add(x)
        f = tmp_path / "i.index"
        gpu_faiss.write_index(idx, str(f))
        raw = f.read_bytes()
        assert raw[:4] in (b"IxFI", b"IxF2", b"IHNf")
        back = gpu_faiss.read_index(str(f))
        assert type(back) is type(idx) and back.ntotal == n and back.d == d and back.metric_type == idx.metric_type
        if isinstance(idx, gpu_faiss.IndexHNSWFlat):
            idx.hnsw.efSearch = back.hnsw.efSearch = 64
        D0, I0 = idx.search(x[:50], 10)
        D1, I1 = back.search(x[:50], 10)
        assert np.array_equal(I0, I1) and np.array_equal(D0, D1)
    # IndexFlat file layout: fourcc, d, ntotal, 2 dummies, is_trained, metric, count, floats
    idx = gpu_faiss.IndexFlat(d, 1)
    idx.add(x[:5])
    gpu_faiss.write_index(idx, str(f))
    raw = f.read_bytes()
    assert len(raw) == 4 + 4 + 8 * 3 + 1 + 4 + 8 + 5 * d * 4
    assert np.array_equal(np.frombuffer(raw[-5 * d * 4:], np.float32).reshape(5, d), x[:5])


def test_proteins_search_entry_point(gpu_faiss, oracle, tmp_path, capsys):
    """pfam/proteins_search.py:11-57 protocol on a fixture-sized 'full_sequences.npy'."""
    from knn_for_homology_amd.pfam import proteins_search
    x = np.load(GOLDEN / "pfam-20-dist" / "test.npy")
    np.save(tmp_path / "full_sequences.npy", x.astype(np.float16))  # the script casts to float32
    for mode in ("flat", "hnsw"):
        proteins_search.main(["prog", mode], data_dir=tmp_path, k=50)
        out = capsys.readouterr().out
        assert "full_sequences (210, 1024)" in out and "Index creation took" in out and "Search took" in out
        assert "Embeddings:" in out and "Index:" in out and "Difference:" in out
        scores = np.load(tmp_path / f"full_sequences_{mode}_scores.npy")
        hits = np.load(tmp_path / f"full_sequences_{mode}_hits.npy")
        assert scores.shape == (210, 50) and scores.dtype == np.float32 and hits.dtype == np.int64
        assert (hits[:, 0] == np.arange(210)).all(), "self hit first (pfam/proteins.py:85-122 relies on it)"
        assert (tmp_path / f"full_sequences_{mode}.index").stat().st_size > 210 * 1024 * 4
    flat_hits = np.load(tmp_path / "full_sequences_flat_hits.npy")
    assert np.array_equal(flat_hits, np.load(tmp_path / "full_sequences_hnsw_hits.npy"))
    with pytest.raises(ValueError):
        proteins_search.main(["prog", "ivf"], data_dir=tmp_path)
    # against the oracle, bit for bit: what the script saved = flat_search(normalised rows, themselves, k)
    xo = x.astype(np.float16).astype(np.float32)
    oracle.normalize_l2(xo)
    Do, Io = oracle.flat_search(xo, xo, 50, 0)
    for mode in ("flat", "hnsw"):  # (210 rows: the HNSW walk with ef >= n is exact)
        assert np.array_equal(np.load(tmp_path / f"full_sequences_{mode}_hits.npy"), Io)
        assert np.array_equal(np.load(tmp_path / f"full_sequences_{mode}_scores.npy").view(np.uint32), Do.view(np.uint32))
    # the written flat index holds the normalised rows (pfam/proteins_search.py:22 normalises before :37 add)
    back = gpu_faiss.read_index(str(tmp_path / "full_sequences_flat.index"))
    assert np.array_equal(back.reconstruct_n(0, 210), xo)


@pytest.mark.parametrize("mode", ["flat", "hnsw"])
def test_proteins_search_normalises_in_place_and_uses_k_1000(gpu_faiss, oracle, tmp_path, capsys, mode):
    """pfam/proteins_search.py:22 `faiss.normalize_L2(embeddings)` mutates the array the script holds, :49 searches with
    k = 1000: the default k on a 1 300-row input, results against the oracle bit for bit (flat) / as exact-walk recall
    (hnsw: ef = max(efSearch, k) = 1000 of 1 300 rows)."""
    from knn_for_homology_amd.pfam import proteins_search
    rng = np.random.default_rng(12)
    n, d = 1300, 64
    cent = rng.standard_normal((40, d)).astype(np.float32)
    x = (cent[rng.integers(0, 40, n)] + 0.3 * rng.standard_normal((n, d))).astype(np.float32)
    x[700] = x[3]  # a duplicate: ties go to the lower id
    held = x.copy()
    proteins_search.run(held, mode, tmp_path, npy_size=n * d * 4)
    xo = x.copy()
    oracle.normalize_l2(xo)
    assert np.array_equal(held.view(np.uint32), xo.view(np.uint32)), "the caller's array must come back normalised, oracle bits"
    Do, Io = oracle.flat_search(xo, xo, 1000, 0)
    hits = np.load(tmp_path / f"full_sequences_{mode}_hits.npy")
    scores = np.load(tmp_path / f"full_sequences_{mode}_scores.npy")
    assert hits.shape == (n, 1000) and scores.shape == (n, 1000)
    if mode == "flat":
        assert np.array_equal(hits, Io) and np.array_equal(scores.view(np.uint32), Do.view(np.uint32))
    else:
        found = hits >= 0
        recall = np.mean([len(np.intersect1d(a[a >= 0], b)) for a, b in zip(hits, Io)]) / 1000
        assert recall >= 0.97, recall
        # whatever the walk returns carries the flat search's distance bits, best first, self hit first
        rows = np.repeat(np.arange(n), 1000).reshape(n, 1000)
        want = oracle.pair_distances(xo, xo, rows[found], hits[found], 0)
        assert np.array_equal(scores[found].view(np.uint32), want.view(np.uint32))
        assert (np.diff(np.where(found, scores, -np.inf), axis=1) <= 0).all()
        assert (hits[:, 0] == np.arange(n)).all() or (hits[700, 0] == 3 and (np.delete(hits[:, 0], 700) == np.delete(np.arange(n), 700)).all())


@pytest.mark.parametrize("metric", [0, 1])
def test_quality_matches_sequential_oracle(gpu_faiss, ko, metric):
    """Batch-synchronous GPU-offloaded construction vs the sequential CPU oracle
    (oracle/hnsw_oracle.c), same M / efConstruction / efSearch: recall must not be worse by
    more than 2 points at any setting."""
    n, d, nq, M = 20000, 64, 500, 16
    x = _clustered(n, d, 300, 33)
    gpu_faiss.normalize_L2(x)
    flat = gpu_faiss.IndexFlat(d, metric)
    flat.add(x)
    _, It = flat.search(x[:nq], 10)
    ref = ko.OracleHNSW(d, M, metric)
    ref.add(x)
    idx = gpu_faiss.IndexHNSWFlat(d, M, metric)
    idx.add(x)
    for efs in (16, 64, 256):
        _, Iref = ref.search(x[:nq], 10, efs)
        idx.hnsw.efSearch = efs
        _, I = idx.search(x[:nq], 10)
        r_ref, r_gpu = _recall(Iref, It), _recall(I, It)
        assert r_gpu >= r_ref - 0.02, (efs, r_gpu, r_ref)


def test_bf16_beam_matches_fp32_beam_in_quality(gpu_faiss, oracle, monkeypatch):
    """The level-0 beam walks on bf16 copies of the rows (default) or on the fp32 rows (KNN355_HNSW_BEAM_FP32=1): same
    recall within half a point, and in both every returned distance is the flat search's value for that pair."""
    n, d, nq, k = 30000, 256, 800, 50
    x = _clustered(n, d, 300, 9)
    gpu_faiss.normalize_L2(x)
    flat = gpu_faiss.IndexFlat(d, 0)
    flat.add(x)
    Dt, It = flat.search(x[:nq], k)
    rec = {}
    for name, env in (("bf16", "0"), ("fp32", "1")):
        monkeypatch.setenv("KNN355_HNSW_BEAM_FP32", env)
        idx = gpu_faiss.IndexHNSWFlat(d, 32, 0)
        idx.add(x)
        idx.hnsw.efSearch = 128
        D, I = idx.search(x[:nq], k)
        rec[name] = _recall(I, It)
        for r in range(50):
            ref = dict(zip(It[r].tolist(), Dt[r].view(np.uint32).tolist()))
            for j, v in zip(I[r].tolist(), D[r].view(np.uint32).tolist()):
                if j in ref:
                    assert ref[j] == v
        assert_output_contract(D, I, x, x[:nq], 0, n, oracle)
    assert rec["bf16"] >= 0.95 and abs(rec["bf16"] - rec["fp32"]) <= 0.005, rec


def test_lazy_and_eager_clearing_of_the_visited_bitmaps_agree(gpu_faiss, monkeypatch):
    """Graphs of millions of rows clear only the bitmap words a walk touched (KNN355_HNSW_CLEAR=lazy forces that on a
    small graph; an overflowing list -- efSearch 1024 with 64 neighbours per node -- falls back to the full clear):
    identical results to the eager clear, search after search, and a graph built under either is the same graph."""
    n, d, nq, k = 20000, 64, 600, 20
    x = _clustered(n, d, 200, 4)
    res, graphs = {}, {}
    for mode in ("eager", "lazy"):
        monkeypatch.setenv("KNN355_HNSW_CLEAR", mode)
        idx = gpu_faiss.IndexHNSWFlat(d, 32, 1)
        idx.add(x)
        graphs[mode] = idx.graph()[2]
        out = []
        for efs in (64, 1024, 64, 256):
            idx.hnsw.efSearch = efs
            out.append(idx.search(x[:nq], k))
        res[mode] = out
    assert np.array_equal(graphs["eager"], graphs["lazy"])
    for (De, Ie), (Dl, Il) in zip(res["eager"], res["lazy"]):
        assert np.array_equal(Ie, Il) and np.array_equal(De.view(np.uint32), Dl.view(np.uint32))


# ---- the reference's own HNSW shape: IndexHNSWFlat(d, 42, IP), efSearch = 256, all-vs-all k = 1000 -----------------
# (/root/reference/pfam/proteins_search.py:27-31,49; FAISS walks with ef = max(efSearch, k) = 1000 there)
@pytest.mark.parametrize("n,d", [(20000, 128), (20000, 1024)])
def test_reference_shape_recall_against_the_sequential_oracle(gpu_faiss, ko, n, d):
    """At a size oracle/hnsw_oracle.c builds in seconds: same M / efConstruction / ef, k = 1000 = ef.  A beam of
    exactly k entries cannot hold the whole top k (the sequential oracle itself reaches 0.94 at d = 128 and 0.90 on
    the Pfam-like structure -- d = 1024, 100 rows per cluster: beyond a query's own cluster the score profile is flat,
    rank 150 scores 0.09 and rank 1000 0.06); the device path must not be worse than the oracle by more than 2 points."""
    nq, M, k = 300, 42, 1000
    x = _clustered(n, d, 200, 7)
    gpu_faiss.normalize_L2(x)
    flat = gpu_faiss.IndexFlat(d, 0)
    flat.add(x)
    Dt, It = flat.search(x[:nq], k)
    ref = ko.OracleHNSW(d, M, 0, 40)
    ref.add(x)
    _, Ir = ref.search(x[:nq], k, 1000)
    r_ref = _recall(Ir, It)
    idx = gpu_faiss.IndexHNSWFlat(d, M, gpu_faiss.METRIC_INNER_PRODUCT)
    idx.hnsw.efSearch = 256
    idx.train(x)
    idx.add(x)
    D, I = idx.search(x[:nq], k)
    r_gpu = _recall(I, It)
    print(f"recall@1000, ef = 1000: device {r_gpu:.4f}, sequential oracle {r_ref:.4f}")
    assert r_gpu >= r_ref - 0.02, (r_gpu, r_ref)
    assert (I[:, 0] == np.arange(nq)).all()
    found = I >= 0
    rows = np.repeat(np.arange(nq), k).reshape(nq, k)
    want = ko.oracle().pair_distances(x, x[:nq], rows[found], I[found], 0)
    assert np.array_equal(D[found].view(np.uint32), want.view(np.uint32)), "returned distances carry the flat search's bits"


def test_reference_shape_at_pfam_size(gpu_faiss):
    """200 k x 1024 clustered rows through the call sequence of pfam/proteins_search.py hnsw mode (normalise in place,
    IndexHNSWFlat(d, 42, IP), efSearch = 256, train, add, search(embeddings, 1000)): recall@1000 against the flat
    search, self hit first, every slot filled or -1 (remove_self_hit of pfam/proteins.py:85-122 takes the result)."""
    from knn_for_homology_amd.evaluation import remove_self_hit
    n, d, k = 200_000, 1024, 1000
    x = _clustered(n, d, 2000, 21)
    gpu_faiss.normalize_L2(x)
    idx = gpu_faiss.IndexHNSWFlat(d, 42, gpu_faiss.METRIC_INNER_PRODUCT)
    idx.hnsw.efSearch = 256
    idx.train(x)
    idx.add(x)
    D, I = idx.search(x, k)
    assert D.shape == (n, k) and I.shape == (n, k) and I.dtype == np.int64
    assert ((I >= -1) & (I < n)).all()
    filled = I >= 0
    assert filled[:, :100].all(), "a walk with ef = 1000 fills at least the first hundred slots"
    assert (np.diff(np.where(filled, D, -np.inf), axis=1) <= 0).all(), "best first, unfilled slots last"
    assert (I[:, 0] == np.arange(n)).mean() >= 0.999
    flat = gpu_faiss.IndexFlat(d, 0)
    flat.add(x)
    sample = np.arange(0, n, 97)[:2048]
    Dt, It = flat.search(x[sample], k)
    r = _recall(I[sample], It)
    r100 = _recall(I[sample][:, :100], It[:, :100])
    # the depth the reference's consumers read: pfam/proteins.py:41,246 slice [:, :300] of the saved hits
    r300 = _recall(I[sample][:, :300], It[:, :300])
    print(f"recall@1000 {r:.4f}, recall@300 of the first three hundred {r300:.4f}, recall@100 of the first hundred {r100:.4f}")
    assert r300 >= 0.93, r300
    # (ef = k on 2000 clusters of 100 rows: the ranks past the query's own cluster are decided by score differences of
    # 1e-2 among 2000 equidistant clusters; the sequential oracle loses the same ranks at the sizes it can build -- see
    # the test above and tests/probe_hnsw_reference_shape.py: 40 k rows of this structure, oracle 0.902, device 0.911)
    assert r >= 0.78 and r100 >= 0.99, (r, r100)
    # The algorithm's own figure AT THIS SIZE: oracle/hnsw_oracle.c's sequential build of these very rows
    # (same generator and seed, M = 42, efConstruction 40), walked with ef = 1000 for these 2048 queries in the build container
    # (tests/golden/make_golden.py --hnsw-refshape: 207 s of one core) -- recall@100 0.951, @300 0.878, @1000 0.744 against the
    # oracle's exact flat search.  The device must not be worse than the oracle by more than 2 points at any depth.
    g = np.load(Path(__file__).resolve().parent / "golden" / "hnsw_refshape_200k.npz")
    assert int(g["n"]) == n and int(g["d"]) == d and int(g["M"]) == 42 and np.array_equal(g["sample"], sample)
    # the fixture's ids against the device's exact search: the stored recalls are reproduced (fp32 ties aside)
    o300 = g["oracle_I_300"].astype(np.int64)
    assert abs(_recall(o300[:, :100], It[:, :100]) - float(g["recall_at_100"])) < 2e-3
    assert abs(_recall(o300, It[:, :300]) - float(g["recall_at_300"])) < 2e-3
    assert _recall(g["exact_I_1000_first256"].astype(np.int64), It[:256]) > 0.9995, "same rows, same exact neighbours"
    print(f"sequential oracle at this size: recall@100 {float(g['recall_at_100']):.4f}, @300 {float(g['recall_at_300']):.4f}, "
          f"@1000 {float(g['recall_at_1000']):.4f}; device {r100:.4f} / {r300:.4f} / {r:.4f}")
    assert r100 >= float(g["recall_at_100"]) - 0.02 and r300 >= float(g["recall_at_300"]) - 0.02 and r >= float(g["recall_at_1000"]) - 0.02
    hits, scores = remove_self_hit(I[:4096].copy(), D[:4096].copy())
    assert hits.shape == (4096, k - 1)
