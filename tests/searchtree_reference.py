"""Plain references of the likelihood search tests (tests/test_search_reference_host.py, tests/test_gpu_search_edges.py,
tests/test_gpu_bound_edges.py).

1. The summation order of ``csrc/gk_search.hip`` -- numpy's ``add.reduce`` over a contiguous axis -- written with
   element-wise ``+`` on arrays only, so that the order stands in the text: ``leaf_sum`` (at most 128 rows: eight strided
   accumulators, their fixed combination, a sequential tail), ``pairwise`` (halving with the left half rounded down to a
   multiple of 8) and ``tree_sum`` (chunks of 8192 rows added in sequence).  All sum along axis 0 and keep the other axes.
   ``sequential_sum``, ``tree_sum(round8=False)`` and ``tree_sum(chunk=None)`` are WRONG orders: the host test uses them
   to show that the tables below tell the orders apart.
2. The tables the GPU tests share: ``table`` (few distinct values per row: exact ties everywhere), ``wide`` (mantissas in
   [1, 2), exponents over 2^-12 .. 2^8, negative: every addition rounds) and ``padded`` (column-major with ``ld`` beyond
   the row count, the padding rows NaN), and the four numpy expressions the GPU results are compared with.
3. The integer bound of ``csrc/gk_bound.hip``: ``bound_reference``, and a step whose totals span 255 x rows
   (``band_case``, ``band_top_ns``) for the select's shifted bands.
"""
import numpy as np

LEAF_ROWS = 128
CHUNK_ROWS = 8192

# every row count at which a kernel of gk_search.hip changes shape, with its neighbours: all-tail leaves (< 8), the
# `len & 7` tail, one leaf (128), one sub-tree (512) with lane-stack slot 3 from 511, two parked children (513 .. 1024),
# several spans (> 1024), a second chunk of 1, 7, 8, 9, 127, 128, 129 rows, two whole chunks, three chunks
SWEEP = [1, 2, 7, 8, 9, 15, 16, 17, 127, 128, 129, 135, 136, 137, 255, 256, 257, 264, 511, 512, 513, 520, 521, 1023, 1024,
         1025, 1032, 1033, 2047, 2048, 2049, 4095, 4096, 4097, 8191, 8192, 8193, 8199, 8200, 8201, 8319, 8320, 8321,
         16383, 16384, 16385, 24577]
# one row count of each regime, then a second chunk of one row behind one and behind two whole chunks
PADDED_SWEEP = [7, 9, 128, 137, 511, 520, 1023, 1033, 4097, 8193, 16385]
TABLES = ("ties", "wide")
N_ALLELE, N_SETS = 12, 5


# ---------------------------------------------------------------------------------------------------------------------
# the summation order

def sequential_sum(X):
    total = X[0]
    for i in range(1, len(X)):
        total = total + X[i]
    return total


def leaf_sum(X):
    n = len(X)
    assert 1 <= n <= LEAF_ROWS
    if n < 8:
        return sequential_sum(X)
    r = [X[j] for j in range(8)]
    i = 8
    while i + 8 <= n:
        for j in range(8):
            r[j] = r[j] + X[i + j]
        i += 8
    total = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    while i < n:
        total = total + X[i]
        i += 1
    return total


def pairwise(X, round8=True):
    n = len(X)
    if n <= LEAF_ROWS:
        return leaf_sum(X)
    n2 = n // 2
    if round8:
        n2 -= n2 % 8
    return pairwise(X[:n2], round8) + pairwise(X[n2:], round8)


def tree_sum(X, chunk=CHUNK_ROWS, round8=True):
    n = len(X)
    if chunk is None:
        return pairwise(X, round8)
    total = pairwise(X[:chunk], round8)
    for r0 in range(chunk, n, chunk):
        total = total + pairwise(X[r0:r0 + chunk], round8)
    return total


def splits_not_multiple_of_8(n, chunk=CHUNK_ROWS):
    """Does the tree of ``n`` rows halve a node whose half is no multiple of 8 (where ``round8`` matters)?"""
    def node(m):
        if m <= LEAF_ROWS:
            return False
        n2 = m // 2
        if n2 % 8:
            return True
        n2 -= n2 % 8
        return node(n2) or node(m - n2)
    return any(node(min(chunk, n - r0)) for r0 in range(0, n, chunk))


# ---------------------------------------------------------------------------------------------------------------------
# tables and the expressions of the reference project the kernels reproduce

def table(rng, n_rows, n_allele):
    # few distinct values per row -> many exact ties, like log10 of products of 0.999 / 0.001
    L = -rng.integers(0, 4, (n_rows, n_allele)).astype(np.float64) * 2.9995654882259823
    return L - rng.integers(20, 60, (n_rows, 1)) * 0.00043451177401769


def wide(rng, n_rows, n_allele):
    # every addition rounds, at a different exponent: an order of summation other than numpy's shows in the last bits
    return -(1.0 + rng.random((n_rows, n_allele))) * 2.0 ** rng.integers(-12, 9, (n_rows, n_allele)).astype(np.float64)


def make_table(kind, n_rows, n_allele=N_ALLELE):
    """The table of the row sweep: the same on the host, which judges it, and on the GPU."""
    rng = np.random.default_rng(1000003 * (TABLES.index(kind) + 1) + n_rows)
    return (table if kind == "ties" else wide)(rng, n_rows, n_allele)


def sweep_sets(n_rows, c, n_allele=N_ALLELE, n_sets=N_SETS):
    """Allele sets of the row sweep: random ids; with two or more alleles the second set is homozygous."""
    rng = np.random.default_rng(77 * n_rows + c)
    ids = np.ascontiguousarray(rng.integers(0, n_allele, (n_sets, c)), dtype=np.int32)
    if c >= 2:
        ids[1, :] = ids[1, 0]
    ids[-1, 0] = n_allele - 1
    return ids


def padded(L, pad, fill=np.nan):
    """Column-major [allele][ld] with ld = rows + pad; the padding rows hold ``fill``."""
    n_rows, n_allele = L.shape
    out = np.full((n_allele, n_rows + pad), fill, dtype=np.float64)
    out[:, :n_rows] = L.T
    return out


def colsum_numpy(L, cols):
    return L[:, cols].sum(axis=0)                        # typing_mulit_allele.py:514


def maxsum_numpy(L, ids, cols):
    prev = L[:, ids].max(axis=2)                         # allele_prob of the previous sets (569)
    return np.maximum(L[:, cols], prev.T[:, :, None]).sum(axis=1)      # 540-542


def setvalue_numpy(L, ids):
    return np.asfortranarray(L[:, ids].max(axis=2)).sum(axis=0)


def shares_numpy(L, ids):
    """Undivided shares (575-580 before the division by the row count)."""
    gathered = L[:, ids]
    owns = np.equal(gathered, gathered.max(axis=2)[:, :, None])
    return (owns / owns.sum(axis=2)[:, :, None]).sum(axis=0)


# the same four with the restated order (`order` = tree_sum or one of the wrong orders)
def colsum_tree(L, cols, order=tree_sum):
    return order(L[:, cols])


def maxsum_tree(L, ids, cols, order=tree_sum):
    prev = L[:, ids].max(axis=2)                         # rows x sets
    return order(np.maximum(L[:, None, cols], prev[:, :, None]))


def setvalue_tree(L, ids, order=tree_sum):
    return order(L[:, ids].max(axis=2))


def shares_tree(L, ids, order=tree_sum):
    gathered = L[:, ids]
    owns = np.equal(gathered, gathered.max(axis=2)[:, :, None])
    return order(owns / owns.sum(axis=2)[:, :, None])


# ---------------------------------------------------------------------------------------------------------------------
# the integer bound

class Bound:
    """What gk_bound_step must report for one call (see ``bound_reference``)."""


def bound_reference(miss, ids, cols, first, top_n):
    """``miss``: uint8 [allele][row]; ``ids``: previous sets [n_sets][c_prev]; ``cols``: candidate columns; ``first``: mask
    [n_sets][n_cols] of the candidates.  M[t][a] = sum_r min(min_j miss[ids[t][j]][r], miss[cols[a]][r]) in int64; among
    the masked candidates: count, base (smallest M), span (largest - base), sh0 = max(0, bit_length(span) - 22) with a bit
    length of 1 for span 0, kth = the min(top_n, count)-th smallest, the cut = the largest total whose reduced value
    (M - base) >> sh0 is kth's, and the selection mask & (M <= cut) as flat indices in rising order."""
    b = Bound()
    prev = miss[np.asarray(ids)].min(axis=1)                                   # [set][row] uint8
    M = np.empty((len(ids), len(cols)), dtype=np.int64)
    for j, c in enumerate(cols):
        M[:, j] = np.minimum(prev, miss[c][None, :]).sum(axis=1, dtype=np.int64)
    b.M = M
    b.flat = M.ravel()
    b.mask = np.asarray(first).ravel().astype(bool)
    b.count = int(b.mask.sum())
    if b.count == 0:
        b.base = b.span = b.sh0 = b.kth = b.cut = 0
        b.selection = np.zeros(0, dtype=np.int64)
        b.must = b.selection
        return b
    cand = np.sort(b.flat[b.mask])
    b.base = int(cand[0])
    b.span = int(cand[-1]) - b.base
    b.sh0 = max(0, (b.span.bit_length() if b.span else 1) - 22)
    b.kth = int(cand[min(top_n, b.count) - 1])
    b.cut = b.base + ((((b.kth - b.base) >> b.sh0) + 1) << b.sh0) - 1
    b.selection = np.flatnonzero(b.mask & (b.flat <= b.cut))
    b.must = np.flatnonzero(b.mask & (b.flat <= b.kth))      # what may never be dropped
    return b


def band_case(n_rows):
    """A step whose totals span 255 * n_rows: allele 0 is all 255 (and the previous set of the first set, so that
    M[0][a] is column a's sum), allele 1 all zero, the others random with rising ceilings; allele 3 is allele 2 with one
    byte one larger (two totals one apart).  -> miss [12][n_rows], ids, cols, first."""
    rng = np.random.default_rng(n_rows)
    miss = np.zeros((12, n_rows), dtype=np.uint8)
    miss[0] = 255
    for a in range(2, 12):
        miss[a] = rng.integers(0, 22 * a, n_rows)
    miss[3] = miss[2]
    miss[3, n_rows // 2] = miss[2, n_rows // 2] + 1
    ids = np.array([[0], [7], [1]], dtype=np.int32)
    cols = np.arange(12, dtype=np.int32)
    first = np.ones((3, 12), dtype=np.uint8)
    first[2, 1:] = 0                                     # previous set = the zero column: every total 0, one is kept
    return miss, ids, cols, first


def band_top_ns(miss, ids, cols, first):
    """(top_n whose kth lies an odd number above the base, one whose kth lies an even number above it, neither 0)."""
    count = int(np.asarray(first).sum())
    odd = even = None
    for top_n in range(1, count + 1):
        b = bound_reference(miss, ids, cols, first, top_n)
        off = b.kth - b.base
        if off and off % 2 and odd is None:
            odd = top_n
        if off and off % 2 == 0 and even is None:
            even = top_n
    return odd, even
