"""The restated summation order of the search tests (tests/searchtree_reference.py) against numpy itself, on the four
expressions the GPU tests take as truth and at every row count of their sweep; that the sweep's tables tell numpy's order
from a sequential one, from a tree split without the rounding to 8 rows and from one without the 8192-row chunks; and the
reference of the integer bound on hand-made totals.  No GPU.

numpy's expressions are the truth (they are what the reference project computes): were the restatement ever to disagree
with them, the restatement would be what is wrong."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import searchtree_reference as sr  # noqa: E402


@pytest.mark.parametrize("kind", sr.TABLES)
@pytest.mark.parametrize("n_rows", sr.SWEEP)
def test_restatement_has_the_bits_of_numpy(n_rows, kind):
    L = sr.make_table(kind, n_rows)
    cols = np.arange(sr.N_ALLELE, dtype=np.int32)
    assert np.array_equal(sr.colsum_tree(L, cols), sr.colsum_numpy(L, cols))
    for c in (1, 2):
        ids = sr.sweep_sets(n_rows, c)
        assert np.array_equal(sr.maxsum_tree(L, ids, cols), sr.maxsum_numpy(L, ids, cols)), c
    for c in (1, 2, 3, 4, 8):
        ids = sr.sweep_sets(n_rows, c)
        assert np.array_equal(sr.setvalue_tree(L, ids), sr.setvalue_numpy(L, ids)), c
        assert np.array_equal(sr.shares_tree(L, ids), sr.shares_numpy(L, ids)), c


@pytest.mark.parametrize("kind", sr.TABLES)
@pytest.mark.parametrize("n_rows", sr.SWEEP)
def test_tables_of_the_sweep_tell_the_orders_apart(n_rows, kind):
    """A kernel that summed in another order than numpy's must not get the right bits by luck: on the very tables the GPU
    sweep uses, the wrong orders give other bits wherever they are other orders at all."""
    L = sr.make_table(kind, n_rows)
    cols = np.arange(sr.N_ALLELE, dtype=np.int32)
    ids = sr.sweep_sets(n_rows, 1)
    right = sr.maxsum_tree(L, ids, cols)
    right_cols = sr.colsum_tree(L, cols)
    if n_rows >= 8:
        assert (sr.maxsum_tree(L, ids, cols, sr.sequential_sum) != right).any()
        assert (sr.colsum_tree(L, cols, sr.sequential_sum) != right_cols).any()
    else:
        assert np.array_equal(sr.maxsum_tree(L, ids, cols, sr.sequential_sum), right)
    unrounded = lambda X: sr.tree_sum(X, round8=False)  # noqa: E731
    if sr.splits_not_multiple_of_8(n_rows):
        assert (sr.maxsum_tree(L, ids, cols, unrounded) != right).any()
        assert (sr.colsum_tree(L, cols, unrounded) != right_cols).any()
    else:
        assert np.array_equal(sr.maxsum_tree(L, ids, cols, unrounded), right)
    unchunked = lambda X: sr.tree_sum(X, chunk=None)  # noqa: E731
    if n_rows > sr.CHUNK_ROWS and n_rows % sr.CHUNK_ROWS:
        assert (sr.maxsum_tree(L, ids, cols, unchunked) != right).any()
        assert (sr.colsum_tree(L, cols, unchunked) != right_cols).any()
    elif n_rows <= sr.CHUNK_ROWS:
        assert np.array_equal(sr.maxsum_tree(L, ids, cols, unchunked), right)


def test_sweep_has_every_shape_of_the_tree():
    s = set(sr.SWEEP)
    assert {1, 7, 8, 9, 127, 128, 129, 511, 512, 513, 1024, 1025, 8191, 8192, 8193, 16384, 16385, 24577} <= s
    assert set(sr.PADDED_SWEEP) <= s
    assert any(sr.splits_not_multiple_of_8(n) for n in sr.SWEEP) and not sr.splits_not_multiple_of_8(256)
    assert sr.splits_not_multiple_of_8(8192 + 128) is False and sr.splits_not_multiple_of_8(8192 + 137)


def test_leaf_and_split_by_hand():
    x = 2.0 ** -np.arange(0, 60, 3, dtype=np.float64)[:, None] * np.array([[1.0, 3.0]])      # 20 rows, two columns
    r = [x[j] + x[8 + j] for j in range(8)]
    want = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    want = (((want + x[16]) + x[17]) + x[18]) + x[19]
    assert np.array_equal(sr.leaf_sum(x), want)
    assert np.array_equal(sr.leaf_sum(x[:5]), (((x[0] + x[1]) + x[2]) + x[3]) + x[4])
    y = np.arange(1.0, 138.0)[:, None]                   # 137 rows: 64 + 73
    assert np.array_equal(sr.pairwise(y), sr.leaf_sum(y[:64]) + sr.leaf_sum(y[64:]))
    assert np.array_equal(sr.tree_sum(y, round8=False), sr.leaf_sum(y[:68]) + sr.leaf_sum(y[68:]))
    z = np.ones((8200, 1))
    assert np.array_equal(sr.tree_sum(z), sr.pairwise(z[:8192]) + sr.leaf_sum(z[8192:]))


def test_padded_layout():
    L = sr.make_table("wide", 9, 3)
    P = sr.padded(L, 3)
    assert P.shape == (3, 12) and np.array_equal(P[:, :9], L.T) and np.isnan(P[:, 9:]).all()


def bytes_table(rows):
    return np.array(rows, dtype=np.uint8)


def test_bound_reference_by_hand():
    # four alleles, three rows; previous sets {0} and {1, 2}
    miss = bytes_table([[0, 5, 9], [3, 3, 3], [1, 200, 0], [255, 255, 255]])
    ids = [[0, 0], [1, 2]]
    cols = [3, 0, 2]
    first = np.array([[1, 1, 1], [1, 0, 1]], dtype=np.uint8)
    b = sr.bound_reference(miss, ids, cols, first, top_n=2)
    assert b.M.tolist() == [[14, 14, 5], [4, 3, 4]]
    assert (b.count, b.base, b.span, b.sh0) == (5, 4, 10, 0)
    assert b.kth == 4 and b.cut == 4 and b.selection.tolist() == [3, 5]            # the tie at the cut comes whole
    assert sr.bound_reference(miss, ids, cols, first, top_n=3).selection.tolist() == [2, 3, 5]
    assert sr.bound_reference(miss, ids, cols, first, top_n=99).selection.tolist() == [0, 1, 2, 3, 5]
    none = sr.bound_reference(miss, ids, cols, np.zeros((2, 3), dtype=np.uint8), top_n=2)
    assert none.count == 0 and len(none.selection) == 0


@pytest.mark.parametrize("n_rows,sh0", [(16448, 0), (16512, 1), (32960, 2)])
def test_bound_reference_rounds_a_wide_band_up(n_rows, sh0):
    miss = np.zeros((4, n_rows), dtype=np.uint8)
    miss[1] = 255
    miss[2, ::2] = 255
    miss[2, 0] = 7
    miss[3, :5] = 1
    ids = [[1]]
    cols = [0, 1, 2, 3]
    b = sr.bound_reference(miss, ids, cols, np.ones((1, 4), dtype=np.uint8), top_n=2)
    assert b.base == 0 and b.span == 255 * n_rows and b.sh0 == sh0 and b.kth == 5
    assert b.cut == (((5 >> sh0) + 1) << sh0) - 1 and b.kth <= b.cut < b.kth + 2 ** sh0
    assert b.selection.tolist() == [0, 3] and b.must.tolist() == [0, 3]


@pytest.mark.parametrize("n_rows,sh0", [(16448, 0), (16512, 1), (32960, 2)])
def test_band_cases_have_the_width_they_are_meant_to_have(n_rows, sh0):
    """The inputs of the GPU test of wide bands: the reference reports the shift they were built for, a top_n on an odd and
    one on an even offset exist, and two candidates lie one apart."""
    miss, ids, cols, first = sr.band_case(n_rows)
    odd, even = sr.band_top_ns(miss, ids, cols, first)
    assert odd is not None and even is not None
    for top_n in (odd, even):
        b = sr.bound_reference(miss, ids, cols, first, top_n)
        assert b.base == 0 and b.span == 255 * n_rows and b.sh0 == sh0
        assert b.kth <= b.cut < b.kth + 2 ** sh0 and (b.cut + 1) % 2 ** sh0 == 0
        assert set(b.must.tolist()) <= set(b.selection.tolist())
    b = sr.bound_reference(miss, ids, cols, first, 1)
    assert b.M[0, 3] == b.M[0, 2] + 1 and b.M[2].tolist() == [0] * 12 and b.count == 25
