"""No GPU: the host model of range_search_impl (tests/range_reference.py) against the planner itself (csrc/plan.h through
plan_check, and the recorded RANGE_EXPECT), and the conditions under which every case of
tests/test_range_redo_exact_gpu.py means something, at 256 CUs (the GPU tests assert the same at the device's count)."""
import numpy as np
import pytest

import plan_cases as pc
import range_reference as rr
from test_plan_cpu import _lines, plan_check  # noqa: F401  (the module's fixture: plan_check built for the host)

IP, L2 = rr.IP, rr.L2


def test_model_plans_what_the_table_records():
    for c in pc.RANGE_CASES:
        assert tuple(rr.plan_range(c.n, c.metric, c.nq, 256, c.batch)) == pc.RANGE_EXPECT[c.name], c.name


def _gpu_shapes():
    """(n, block's nq, metric, batch) of every block of the GPU cases"""
    out = []
    for _, nb, nq, metric in rr.CASES_A + [rr.CASE_B]:
        out.append((nb, nq, metric, nq))
    for _, nb, metric in rr.CASES_C:
        out += [(nb, rr.QB, metric, rr.QB + 5), (nb, 5, metric, rr.QB + 5)]
    for metric in (IP, L2):
        out += [(300, rr.QB, metric, rr.QB + 5), (300, 5, metric, rr.QB + 5), (300, 19, metric, 19)]        # the L2 rule across blocks
        out += [(rr.SELF_ROWS, rr.QB, metric, rr.SELF_ROWS), (rr.SELF_ROWS, 37, metric, rr.SELF_ROWS), (rr.SELF_ROWS, 5, metric, rr.QB + 5)]
        out += [(100_000, 300, metric, 300), (100_000, 7, metric, 7)]                                        # test_large_output_and_redo, the small searches
    return out


@pytest.mark.parametrize("cus", [256, 304, 104])
def test_model_plans_what_plan_check_plans(plan_check, cus):  # noqa: F811
    shapes = _gpu_shapes()
    out = _lines(plan_check, "range", "".join(f"{n} {nq} {metric} {batch} {cus}\n" for n, nq, metric, batch in shapes), len(shapes))
    for (n, nq, metric, batch), line in zip(shapes, out):
        got = (line.split()[0], *map(int, line.split()[1:]))
        assert tuple(rr.plan_range(n, metric, nq, cus, batch)) == got, (n, nq, metric, batch)


def test_chunk_bounds_tile_the_rows():
    for n, nq, metric, batch in _gpu_shapes():
        pl = rr.plan_range(n, metric, nq, 256, batch)
        lo, hi = rr.chunk_bounds(pl, n)
        assert lo[0] == 0 and hi[-1] == n and np.array_equal(lo[1:], hi[:-1]) and (hi > lo).all()
        assert pl.tiles_base * pl.nchunks + pl.tiles_rem == -(-n // pl.dt)


def test_predict_on_small_counts():
    # one block, nothing over the capacity; a count of exactly segcap is no overflow, one more is
    pl = rr.plan_range(4096, IP, 20, 256)
    assert pl.segcap == 256 and pl.nchunks == 16
    cnt = np.zeros((20, 16), np.int64)
    cnt[3, 5] = 256
    pred = rr.predict(4096, IP, 20, 256, lambda *a: cnt)
    assert pred["last_range"] == {"query_blocks": 1, "redos": 0, "redo_queries": 0} and pred["last_scan"]["grid"] == 16
    assert [(r["qa"], r["qb"], r["n"]) for r in pred["blocks"][0]["runs"]] == [(0, 20, 256)]
    # no results: the run launches nothing; no rows or no queries: no block at all
    zero = rr.predict(4096, IP, 20, 256, lambda *a: np.zeros((20, 16), np.int64))
    assert zero["last_range"]["redos"] == 0 and zero["blocks"][0]["runs"][0]["n"] == 0
    assert rr.predict(0, IP, 20, 256, None)["last_scan"] is None and rr.predict(10, IP, 0, 256, None)["last_range"]["query_blocks"] == 0
    # keep every row of 100 000 x 300 queries: 30 M results in two runs of 167 and 133 queries, every query rescanned
    for metric in (IP, L2):
        full = rr.predict(100_000, metric, 300, 256, rr.keep_all)
        assert full["last_range"] == {"query_blocks": 1, "redos": 2, "redo_queries": 300}
        assert [(r["qa"], r["qb"]) for r in full["blocks"][0]["runs"]] == [(0, 167), (167, 300)]
        assert full["last_scan"] == {"kernel": "range_scan_q128_d128", "query_tile": 128, "db_tile": 128, "nchunks": 171, "grid": 2 * 171}
        assert full["lims"][-1] == 300 * 100_000


def test_expected_is_the_oracles_range(oracle):
    """the integer expectation against the oracle's full ranking (flat_lifecycle_reference.expected_range), both L2 formulas"""
    from flat_lifecycle_reference import expected_range
    rng = np.random.default_rng(5)
    xb_i = rr.rows_of(rng.integers(-1, 12, 700), rng)
    for nq in (7, 40):
        xq_i = rr.queries_of(rng.integers(0, 12, nq), rng)
        for metric in (IP, L2):
            got = rr.expected(xb_i, xq_i, rr.RADIUS[metric], metric, slab_pairs=5000)
            want = expected_range(oracle, rr.f32(xb_i), rr.f32(xq_i), rr.RADIUS[metric], metric)
            assert got[0][-1] > 0
            for g, w in zip(got, want):
                assert g.dtype == w.dtype and np.array_equal(g.view(np.uint32 if g.dtype == np.float32 else g.dtype), w.view(np.uint32 if w.dtype == np.float32 else w.dtype))


@pytest.mark.parametrize("name,nb,nq,metric", rr.CASES_A, ids=[c[0] for c in rr.CASES_A])
def test_partial_overflow_cases_mean_something(oracle, name, nb, nq, metric):
    p = rr.banded(name, nb, nq, metric, 256)
    pred = rr.check_banded(p)
    rr.cross_check(oracle, p.xb_i, p.xq_i, p.want, metric, np.random.default_rng(1))
    pl = p.plan
    assert pl.kernel == {"wide": "range_scan_q128_d128", "narrow": "range_scan_q32_d256", "diff": "range_scan_q32_d256_diff"}[name.split("-")[0]]
    assert pl.nqtiles == {"wide": 3, "narrow": 2, "diff": 1}[name.split("-")[0]]
    assert pred["last_range"]["redo_queries"] == {"wide": 6, "narrow": 4, "diff": 4}[name.split("-")[0]]
    if name.startswith("wide"):  # one query tile in the rescan, three in the first pass: nt_rows flips
        assert pred["last_scan"]["grid"] == pl.nchunks and pl.grid == 3 * pl.nchunks


def test_two_runs_case_means_something(oracle):
    p = rr.two_runs(*rr.CASE_B, 256)
    rr.check_two_runs(p)
    rr.cross_check(oracle, p.xb_i, p.xq_i, p.want, p.metric, np.random.default_rng(2))


@pytest.mark.parametrize("name,nb,metric", rr.CASES_C, ids=[c[0] for c in rr.CASES_C])
def test_two_blocks_cases_mean_something(oracle, name, nb, metric):
    p = rr.two_blocks(name, nb, metric, 256)
    pred = rr.check_two_blocks(p)
    rr.cross_check(oracle, p.xb_i, p.xq_i, p.want, metric, np.random.default_rng(3))
    assert pred["last_range"] == {"query_blocks": 2, "redos": 1, "redo_queries": 256}


@pytest.mark.parametrize("metric", [IP, L2])
def test_self_rows_hit_in_both_blocks(oracle, metric):
    x = rr.self_rows(rr.SELF_ROWS)
    want = rr.expected(x, x, rr.RADIUS[metric], metric)
    rr.cross_check(oracle, x, x, want, metric, np.random.default_rng(4))
    per = np.diff(want[0].astype(np.int64))
    assert per[:rr.QB].min() > 0 and per[rr.QB:].min() > 0 and want[0][-1] < 2_000_000  # hits in both blocks, a small output
    assert len(np.unique((x.astype(np.int32) ** 2).sum(1))) > 4  # the stored norms differ: a wrong norm offset shows
    pred = rr.predict(len(x), metric, len(x), 256, rr.counts_from_result(want[0], want[2]))
    assert pred["last_range"] == {"query_blocks": 2, "redos": 0, "redo_queries": 0}
