"""gk_miss_colsum / gk_bound_step straight through the C ABI against the plain reference of the bound
(tests/searchtree_reference.py: ``bound_reference``): bytes over the whole range 0 .. 255, row counts around the staged
block (128 rows) and around the split of the reads into slices, tiles of 64 sets x 64 columns from both sides, previous
sets of 1, 2 and 8 alleles, every edge of the cut (no candidate, one, top_n of 1, of the count and beyond it, all totals
equal, ties across the cut, a mask that hides the smallest), more selected than the caller has room for, and bands of
totals wide enough for the select to round the cut up.  What the library may never do is drop a candidate at or below the
top_n-th smallest total; everything here is compared exactly."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import searchtree_reference as sr  # noqa: E402

from kir_graph_amd._lib import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu

IDX_SENTINEL = -77
M_SENTINEL = 0xABCDEF01
EXTRA = 64                      # sentinel entries behind `cap` in the host arrays


def bound_step(device, miss, ids, cols, first, top_n, cap):
    """-> (hdr, idx, mm), the host arrays EXTRA entries longer than cap and pre-filled.  The table in HBM has zero rows
    behind n_rows (ldm a multiple of 64) and one more column of 255s behind the last, so that what lies behind a column is
    never zero by luck."""
    n_allele, n_rows = miss.shape
    ldm = (n_rows + 63) // 64 * 64
    table8 = np.zeros((n_allele + 1, ldm), dtype=np.uint8)
    table8[:n_allele, :n_rows] = miss
    table8[n_allele] = 255
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    first = np.ascontiguousarray(first, dtype=np.uint8)
    assert first.shape == (len(ids), len(cols))
    d_miss = device.put(table8)
    d_msum = device.alloc(n_allele, np.uint32)
    try:
        check(lib().gk_miss_colsum(device.ctx, d_miss.ptr, ldm, n_allele, d_msum.ptr))
        assert np.array_equal(d_msum.download(), miss.sum(axis=1, dtype=np.uint64).astype(np.uint32))
        hdr = np.full(4, M_SENTINEL, dtype=np.uint32)
        idx = np.full(cap + EXTRA, IDX_SENTINEL, dtype=np.int32)
        mm = np.full(cap + EXTRA, M_SENTINEL, dtype=np.uint32)
        check(lib().gk_bound_step(device.ctx, d_miss.ptr, ldm, n_rows, d_msum.ptr, ids.ctypes.data, ids.shape[0],
                                  ids.shape[1], cols.ctypes.data, len(cols), first.ctypes.data, top_n, cap,
                                  hdr.ctypes.data, idx.ctypes.data, mm.ctypes.data))
    finally:
        d_miss.free()
        d_msum.free()
    return hdr, idx, mm


def check_bound(device, miss, ids, cols, first, top_n, cap=None):
    """One call, every assertion; -> (the reference, the header)."""
    b = sr.bound_reference(miss, ids, cols, first, top_n)
    if cap is None:
        cap = len(b.selection) + 3
    hdr, idx, mm = bound_step(device, miss, ids, cols, first, top_n, cap)
    assert int(hdr[0]) == b.count
    if b.count == 0:
        assert hdr.tolist() == [0, 0, 0, 0]
        assert (idx == IDX_SENTINEL).all() and (mm == M_SENTINEL).all()
        return b, hdr
    cut = int(hdr[1])
    assert b.kth <= cut < b.kth + 2 ** b.sh0
    assert cut == b.cut
    want = np.flatnonzero(b.mask & (b.flat <= cut))
    assert int(hdr[2]) == len(want) and int(hdr[3]) == 0
    n_back = min(len(want), cap)
    got, got_m = idx[:n_back], mm[:n_back]
    if len(want) <= cap:
        order = np.argsort(got)
        assert np.array_equal(got[order], want)
        assert np.array_equal(got_m[order], b.flat[want])
        assert np.isin(b.must, got).all()
    else:       # no room for all: the first cap entries are different members of the selection with their own totals
        assert len(np.unique(got)) == cap and np.isin(got, want).all()
        assert np.array_equal(got_m, b.flat[got])
    assert (idx[n_back:] == IDX_SENTINEL).all() and (mm[n_back:] == M_SENTINEL).all()
    return b, hdr


def random_case(seed, n_rows, n_allele, n_sets, c_prev, n_cols=None, keep=0.8):
    rng = np.random.default_rng(seed)
    miss = rng.integers(0, 256, (n_allele, n_rows)).astype(np.uint8)
    cols = rng.permutation(n_allele)[:n_cols or n_allele].astype(np.int32)
    ids = rng.integers(0, n_allele, (n_sets, c_prev)).astype(np.int32)
    first = (rng.random((n_sets, len(cols))) < keep).astype(np.uint8)
    return miss, ids, cols, first


ROWS = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 2047, 2048, 2049, 4095, 4096, 4097, 4160, 8191]
# sets x columns around the 64 x 64 tile, with the alleles of a previous set; where a column is 64 bytes long (up to 64
# rows) no case has previous sets of several alleles in a power-of-two number
SHAPES = [(1, 1, 1), (63, 65, 1), (64, 64, 1), (65, 63, 2), (128, 129, 1), (129, 128, 8), (1, 129, 2), (129, 1, 1)]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_and_tiles(device, n_rows, which):
    """Row counts around 16 (a word), 64 (the stride's unit), 128 (a staged block), 2048 / 4096 (where one slice of the
    reads turns into two) with set and column counts around the tile."""
    i = ROWS.index(n_rows)
    n_sets, n_cols, c_prev = SHAPES[(i + 3 * which) % len(SHAPES)]
    n_allele = max(n_cols, 9) + 2
    miss, ids, cols, first = random_case(1000 * n_rows + which, n_rows, n_allele, n_sets, c_prev, n_cols)
    first.ravel()[0] = 1
    top_n = max(1, int(first.sum()) // 3)
    b, _ = check_bound(device, miss, ids, cols, first, top_n)
    assert b.sh0 == 0


@pytest.mark.parametrize("n_rows", [129, 4097])
@pytest.mark.parametrize("case", ["hub", "two", "eight", "repeated"])
def test_previous_sets(device, n_rows, case):
    n_allele, n_sets = 45, 70
    miss, ids, cols, first = random_case(n_rows + len(case), n_rows, n_allele, n_sets,
                                         {"hub": 1, "two": 2, "eight": 8, "repeated": 3}[case])
    if case == "hub":
        miss[3] //= 8                      # a strong allele ...
        ids[:40, 0] = 3                    # ... is the previous set of 40 sets: 40 equal rows of totals, the smallest
        first[:40] = 1
    if case == "repeated":
        ids[::2, 1] = ids[::2, 0]          # [a, a, b]
        ids[5, :] = ids[5, 0]              # [a, a, a]
    if case == "eight":
        ids[3, :] = 7                      # eight times one allele
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=60)
    if case == "hub":                      # ties of 40 sets: whichever of them the cut reaches comes whole
        taken = np.zeros(b.mask.shape, dtype=bool)
        taken[b.selection] = True
        taken = taken.reshape(n_sets, n_allele)
        assert (taken[:40] == taken[0]).all() and taken[0].any() and int(hdr[2]) >= 60


CUT_ROWS = 200


def cut_case(kind):
    rng = np.random.default_rng(len(kind) + 17)
    n_allele, n_sets = 20, 10
    miss = rng.integers(0, 256, (n_allele, CUT_ROWS)).astype(np.uint8)
    ids = rng.integers(0, n_allele, (n_sets, 1)).astype(np.int32)
    cols = np.arange(n_allele, dtype=np.int32)
    first = np.ones((n_sets, n_allele), dtype=np.uint8)
    return miss, ids, cols, first


def test_no_candidate(device):
    miss, ids, cols, first = cut_case("none")
    first[:] = 0
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=5, cap=8)
    assert b.count == 0 and hdr.tolist() == [0, 0, 0, 0]


def test_one_candidate(device):
    miss, ids, cols, first = cut_case("one")
    first[:] = 0
    first[7, 13] = 1
    for top_n in (1, 2, 600):
        b, hdr = check_bound(device, miss, ids, cols, first, top_n=top_n, cap=4)
        assert hdr.tolist() == [1, int(b.M[7, 13]), 1, 0]


@pytest.mark.parametrize("top_n", ["one", "count-1", "count", "count+1", "far"])
def test_top_n_against_the_count(device, top_n):
    miss, ids, cols, first = cut_case("count")
    first[::3, ::2] = 0
    count = int(first.sum())
    n = {"one": 1, "count-1": count - 1, "count": count, "count+1": count + 1, "far": 1 << 30}[top_n]
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=n, cap=count + 5)
    if top_n == "one":
        assert int(hdr[1]) == b.flat[b.mask].min()
    if n >= count:
        assert int(hdr[2]) == count and int(hdr[1]) == b.flat[b.mask].max()


def test_every_total_the_same(device):
    """Span 0: the shift is computed from a bit length of 1, and everybody is selected whatever top_n is."""
    miss, ids, cols, first = cut_case("same")
    miss[:] = miss[0]
    first[2, 5:9] = 0
    for top_n in (1, 50, 1000):
        b, hdr = check_bound(device, miss, ids, cols, first, top_n=top_n)
        assert b.span == 0 and int(hdr[2]) == b.count == 196


def test_tie_group_across_the_cut(device):
    """Six identical columns: every set has six equal totals; a top_n inside such a group takes all of it."""
    miss, ids, cols, first = cut_case("ties")
    miss[1:6] = miss[0]
    ids[:, 0] = np.arange(10) + 6
    b1 = sr.bound_reference(miss, ids, cols, first, 1)
    order = np.argsort(b1.flat, kind="stable")
    inside = next(k for k in range(2, 150) if b1.flat[order[k - 1]] == b1.flat[order[k]] == b1.flat[order[k - 2]])
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=inside)
    assert int(hdr[2]) > inside and (b.flat[b.selection] == b.kth).sum() >= 3


def test_mask_hides_the_smallest_totals(device):
    miss, ids, cols, first = cut_case("hidden")
    b0 = sr.bound_reference(miss, ids, cols, first, 1)
    first = (b0.M > np.median(b0.M)).astype(np.uint8)
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=10)
    assert b.base > b0.base and int(hdr[1]) > np.median(b0.M) and 10 <= int(hdr[2]) < b.count


@pytest.mark.parametrize("cap", [1, 5, 63, 64])
def test_more_selected_than_the_caller_has_room_for(device, cap):
    """hdr[2] is the true count (the caller falls back to the exact step on it); nothing is written behind cap."""
    miss, ids, cols, first = cut_case("cap")
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=65, cap=cap)
    assert int(hdr[2]) >= 65 > cap


def test_more_selected_than_room_in_a_large_step(device):
    """The shape of the existing test's skipped branch: thousands selected, room for a few hundred; many waves append."""
    miss, ids, cols, first = random_case(5, 1000, 130, 129, 1)
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=5000, cap=300)
    assert int(hdr[2]) >= 5000


@pytest.mark.parametrize("parity", ["odd", "even"])
@pytest.mark.parametrize("n_rows,sh0", [(16448, 0), (16512, 1), (32960, 2)])
def test_wide_bands_round_the_cut_up(device, n_rows, sh0, parity):
    """From a span of 2^22 on the select works on totals shifted right: the cut becomes the last total of kth's bin -- at
    least kth, less than kth + 2^sh0 -- and the selection a superset.  16 448 rows of bytes cannot span 2^22: exact."""
    miss, ids, cols, first = sr.band_case(n_rows)
    odd, even = sr.band_top_ns(miss, ids, cols, first)
    top_n = odd if parity == "odd" else even
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=top_n)
    assert b.sh0 == sh0 and b.span == 255 * n_rows and (b.kth - b.base) % 2 == (parity == "odd")
    if sh0 == 0:
        assert int(hdr[1]) == b.kth
    else:
        assert (int(hdr[1]) + 1 - b.base) % 2 ** sh0 == 0


@pytest.mark.parametrize("n_rows,sh0", [(16512, 1), (32960, 2)])
def test_wide_band_with_totals_one_apart_at_the_cut(device, n_rows, sh0):
    """kth on the lower total of a pair one apart: in a shifted band both may share a bin, and then both are selected."""
    miss, ids, cols, first = sr.band_case(n_rows)
    b1 = sr.bound_reference(miss, ids, cols, first, 1)
    lower = int(b1.M[0, 2])
    top_n = int((np.sort(b1.flat[b1.mask]) <= lower).sum())
    b, hdr = check_bound(device, miss, ids, cols, first, top_n=top_n)
    assert b.kth == lower and b.sh0 == sh0
    assert (3 in b.selection.tolist()) == (lower + 1 <= b.cut)      # 3 = the flat index of M[0][3] = lower + 1
