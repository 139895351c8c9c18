"""No GPU: the host model of a flat index's lifecycle (tests/flat_lifecycle_reference.py) on sequences typed in by hand.
The capacities and the life of every view below follow from reading grow_index / knn_flat_reserve / free_index_buffers /
knn_flat_view, not from running them."""
import numpy as np
import pytest

from flat_lifecycle_reference import IP, L2, FlatModel, Refused, expected_range


def _rows(n, d, seed=0):
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def test_capacity_after_7_1_42_rows(oracle):
    m = FlatModel(oracle, 5, IP)
    m.add(_rows(7, 5))
    assert (m.n, m.cap) == (7, 7)          # the first add fits exactly
    m.add(_rows(1, 5))
    assert (m.n, m.cap) == (8, 10)         # max(8, 7 + 3)
    m.add(_rows(42, 5))
    assert (m.n, m.cap) == (50, 50)        # max(50, 10 + 5)
    m.add(_rows(1, 5))
    assert (m.n, m.cap) == (51, 75)        # max(51, 50 + 25)
    m.add(_rows(24, 5))
    assert (m.n, m.cap) == (75, 75)        # fits
    m.add(np.zeros((0, 5), np.float32))
    assert (m.n, m.cap) == (75, 75)


def test_view_survives_an_add_inside_a_reserve_and_dies_on_the_next_growth(oracle):
    m = FlatModel(oracle, 3, L2)
    m.add(_rows(10, 3))
    early = m.view()
    m.reserve(5)                           # nothing happens
    assert early.alive and m.cap == 10
    m.reserve(100)                         # storage moves
    assert not early.alive and m.cap == 100
    v = m.view()
    m.add(_rows(90, 3, 1))                 # fits: 100 rows in 100
    assert v.alive and v.n == 10 and m.n == 100 and m.cap == 100
    assert np.array_equal(m.rows_of(v), m.rows[:10])
    m.add(_rows(1, 3, 2))                  # growth to max(101, 150)
    assert not v.alive and m.cap == 150
    with pytest.raises(Refused):
        m.rows_of(v)
    with pytest.raises(Refused):
        m.rows_of(early)


def test_view_of_a_view_dies_with_its_parent_view(oracle):
    m = FlatModel(oracle, 3, IP)
    m.reserve(20)
    m.add(_rows(4, 3))
    b = m.view()
    m.add(_rows(4, 3, 1))                  # fits: b keeps 4 rows
    c = m.view(of=b)
    assert c.alive and c.n == 4 and m.n == 8
    m.add(_rows(13, 3, 2))                 # 21 > 20: growth
    assert not b.alive and not c.alive
    with pytest.raises(Refused):
        m.view(of=b)
    with pytest.raises(Refused):
        m.view(of=c)
    assert m.view().n == 21


def test_view_of_an_empty_index_outlives_the_first_add(oracle):
    # (no storage moves: grow_index and knn_flat_reserve bump the generation only when there were rows to give back)
    m = FlatModel(oracle, 3, IP)
    v = m.view()
    m.add(_rows(4, 3))
    assert v.alive and v.n == 0 and m.cap == 4
    m.reset()
    assert not v.alive
    w = m.view()
    m.reserve(9)
    assert w.alive and m.cap == 9
    m.reset()                              # free_index_buffers bumps whatever it holds
    assert not w.alive


def test_normalize_is_seen_through_a_live_view(oracle):
    m = FlatModel(oracle, 4, IP)
    x = _rows(6, 4) * np.float32(3.0)
    x[2] = 0.0
    m.reserve(10)
    m.add(x[:3])
    v = m.view()
    m.add(x[3:])
    m.normalize_rows()
    want = x.copy()
    oracle.normalize_l2(want)
    assert v.alive and v.n == 3
    assert np.array_equal(m.rows.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(m.rows_of(v).view(np.uint32), want[:3].view(np.uint32))
    assert not m.rows[2].any()             # a zero row stays
    n2 = (m.rows.astype(np.float64) ** 2).sum(1)
    assert np.allclose(n2[[0, 1, 3, 4, 5]], 1.0, atol=1e-6)


def test_reset_followed_by_a_refill_and_free(oracle):
    m = FlatModel(oracle, 2, L2)
    m.add(_rows(5, 2))
    m.add(_rows(5, 2, 1))
    v = m.view()
    m.reset()
    assert (m.n, m.cap) == (0, 0) and not v.alive
    x = _rows(3, 2, 2)
    m.add(x)
    assert (m.n, m.cap) == (3, 3)          # exact fit again
    assert np.array_equal(m.rows, x)
    d = m.view()
    e = m.view(of=d)
    m.free()
    assert not d.alive and not e.alive and m.freed


def test_expected_answers_on_a_hand_made_index(oracle):
    rows = np.array([[1, 0], [0, 1], [2, 0], [0, 0]], np.float32)
    xq = np.array([[1, 0]], np.float32)
    m = FlatModel(oracle, 2, IP)
    m.add(rows)
    D, I = m.search(m.rows, xq, 6)
    assert I.tolist() == [[2, 0, 1, 3, -1, -1]] and D[0, :4].tolist() == [2.0, 1.0, 0.0, 0.0]
    assert D[0, 4] == -np.finfo(np.float32).max
    lims, Dr, Ir = m.range_search(m.rows, xq, 0.5)
    assert lims.tolist() == [0, 2] and Ir.tolist() == [0, 2] and Dr.tolist() == [1.0, 2.0]
    Ds, Is = m.search_self(m.rows, 2, 2, 1)
    assert Is.tolist() == [[2], [0]] and Ds.tolist() == [[4.0], [0.0]]
    Dg = m.gather(m.rows, xq, np.array([2, 1], np.int64), np.array([0, 2], np.int64))
    assert Dg.tolist() == [2.0, 0.0]
    Df, If = m.refine(m.rows, xq, np.array([[-1, 0, 0, 3]], np.int64), 3)
    assert If.tolist() == [[0, 0, 3]] and Df.tolist() == [[1.0, 1.0, 0.0]]
    l2 = FlatModel(oracle, 2, L2)
    l2.add(rows)
    lims, Dr, Ir = expected_range(oracle, l2.rows, xq, 1.5, L2)
    assert lims.tolist() == [0, 3] and Ir.tolist() == [0, 2, 3] and Dr.tolist() == [0.0, 1.0, 1.0]
    e = FlatModel(oracle, 2, L2)
    D, I = e.search(e.rows, xq, 2)
    assert I.tolist() == [[-1, -1]] and (D == np.finfo(np.float32).max).all()
    assert e.range_search(e.rows, xq, 1.0)[0].tolist() == [0, 0]
