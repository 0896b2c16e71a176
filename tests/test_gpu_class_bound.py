"""gk_bound_step_classes -- the integer bound over the pseudo-rows of a table whose rows fall into classes
(csrc/gk_classrows.h) -- straight through the C ABI against the plain reference of the bound on the EXPANDED row table
(tests/searchtree_reference.py: ``bound_reference``).  The reference is the judge; the row route (gk_bound_step) is
compared as well.  Every table is a random compact table [column][class] expanded through ``class_of``, so rows of one
class are equal by construction.  Weights around the planes (2^k, 2^k - 1, one class of all rows, a class per row),
classes interleaved in row order, plane sizes around the staged block of 128, tiles of 64 sets x 64 columns from both
sides, previous sets of 1, 2 and 8 alleles, every edge of the cut, the 64-bit step of the finish, the argument checks and
the hook.  Everything is compared exactly."""
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


@pytest.fixture(autouse=True)
def class_route(monkeypatch):
    """The hook is read per call: every table here takes the pseudo-rows, however few rows their padding leaves to save
    (the default rule would send most of these small tables over their rows)."""
    monkeypatch.setenv("GK_TEST_HOOKS", "class_bound=on")


def expand(compact, class_of):
    """The row table [column][row] of a compact table [column][class]; rows of a class are equal."""
    compact = np.ascontiguousarray(compact, dtype=np.uint8)
    class_of = np.ascontiguousarray(class_of, dtype=np.uint32)
    miss = np.ascontiguousarray(compact[:, class_of])
    order = np.argsort(class_of, kind="stable")
    starts = np.flatnonzero(np.r_[True, np.diff(class_of[order]) != 0])
    rep = np.repeat(order[starts], np.diff(np.r_[starts, len(order)]))      # the lowest row of every row's class
    assert np.array_equal(miss[:, order], miss[:, rep])
    return miss


def run_step(device, miss, class_of, n_classes, ids, cols, first, top_n, cap, by_class=True):
    """-> (hdr, idx, mm, msum): the host arrays EXTRA entries longer than cap and pre-filled.  The table in HBM has zero rows
    behind n_rows and one more column of 255s behind the last; msum has sentinels behind the columns the call names."""
    n_allele, n_rows = miss.shape
    ldm = (n_rows + 63) // 64 * 64
    table8 = np.zeros((n_allele + 1, ldm), dtype=np.uint8)
    table8[:n_allele, :n_rows] = miss
    table8[n_allele] = 255
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    cols = np.ascontiguousarray(cols, dtype=np.int32)
    first = np.ascontiguousarray(first, dtype=np.uint8)
    assert first.shape == (len(ids), len(cols))
    n_tab = int(max(ids.max(), cols.max())) + 1
    d_miss = device.put(table8)
    d_msum = device.put(np.full(n_allele + 4, M_SENTINEL, dtype=np.uint32))
    d_cls = device.put(np.ascontiguousarray(class_of, dtype=np.uint32))
    try:
        hdr = np.full(4, M_SENTINEL, dtype=np.uint32)
        idx = np.full(cap + EXTRA, IDX_SENTINEL, dtype=np.int32)
        mm = np.full(cap + EXTRA, M_SENTINEL, dtype=np.uint32)
        if by_class:
            check(lib().gk_bound_step_classes(device.ctx, d_miss.ptr, ldm, n_rows, d_cls.ptr, n_classes, d_msum.ptr,
                                              ids.ctypes.data, ids.shape[0], ids.shape[1], cols.ctypes.data, len(cols),
                                              first.ctypes.data, top_n, cap, hdr.ctypes.data, idx.ctypes.data,
                                              mm.ctypes.data))
        else:
            check(lib().gk_miss_colsum(device.ctx, d_miss.ptr, ldm, n_tab, d_msum.ptr))
            check(lib().gk_bound_step(device.ctx, d_miss.ptr, ldm, n_rows, d_msum.ptr, ids.ctypes.data, ids.shape[0],
                                      ids.shape[1], cols.ctypes.data, len(cols), first.ctypes.data, top_n, cap,
                                      hdr.ctypes.data, idx.ctypes.data, mm.ctypes.data))
        msum = d_msum.download()
    finally:
        d_miss.free()
        d_msum.free()
        d_cls.free()
    assert np.array_equal(msum[:n_tab], miss[:n_tab].sum(axis=1, dtype=np.uint64).astype(np.uint32))
    assert (msum[n_tab:] == M_SENTINEL).all()
    return hdr, idx, mm


def sorted_pairs(idx, mm, n):
    order = np.argsort(idx[:n], kind="stable")
    return idx[:n][order], mm[:n][order]


def check_classes(device, compact, class_of, ids, cols, first, top_n, cap=None, n_classes=None):
    """One call by class, every assertion against the reference on the expanded table; then the same call on the rows:
    equal header, equal sorted (idx, m).  -> (the reference, the header)."""
    miss = expand(compact, class_of)
    if n_classes is None:
        n_classes = compact.shape[1]
    b = sr.bound_reference(miss, ids, cols, first, top_n)
    if cap is None:
        cap = len(b.selection) + 3
    hdr, idx, mm = run_step(device, miss, class_of, n_classes, ids, cols, first, top_n, cap)
    rhdr, ridx, rmm = run_step(device, miss, class_of, n_classes, ids, cols, first, top_n, cap, by_class=False)
    assert hdr.tolist() == rhdr.tolist()
    assert int(hdr[0]) == b.count
    if b.count == 0:
        assert hdr.tolist() == [0, 0, 0, 0]
        assert (idx == IDX_SENTINEL).all() and (mm == M_SENTINEL).all()
        return b, hdr
    cut = int(hdr[1])
    assert cut == b.cut
    want = np.flatnonzero(b.mask & (b.flat <= cut))
    assert int(hdr[2]) == len(want) and int(hdr[3]) == 0
    n_back = min(len(want), cap)
    got, got_m = sorted_pairs(idx, mm, n_back)
    if len(want) <= cap:
        assert np.array_equal(got, want)
        assert np.array_equal(got_m, b.flat[want])
        assert np.isin(b.must, got).all()
        rgot, rgot_m = sorted_pairs(ridx, rmm, n_back)
        assert np.array_equal(got, rgot) and np.array_equal(got_m, rgot_m)
    else:       # no room for all: the first cap entries are different members of the selection with their own totals
        assert len(np.unique(got)) == cap and np.isin(got, want).all()
        assert np.array_equal(got_m, b.flat[got])
    assert (idx[n_back:] == IDX_SENTINEL).all() and (mm[n_back:] == M_SENTINEL).all()
    return b, hdr


def classes_of_weights(weights, rng=None):
    """class_of for classes of the given weights: class by class, or (with rng) interleaved in row order."""
    class_of = np.repeat(np.arange(len(weights), dtype=np.uint32), weights)
    return class_of if rng is None else rng.permutation(class_of)


def random_step(rng, n_classes, n_allele, n_sets, c_prev, n_cols=None, keep=0.8):
    compact = rng.integers(0, 256, (n_allele, n_classes)).astype(np.uint8)
    cols = rng.permutation(n_allele)[:n_cols or n_allele].astype(np.int32)
    ids = rng.integers(0, n_allele, (n_sets, c_prev)).astype(np.int32)
    first = (rng.random((n_sets, len(cols))) < keep).astype(np.uint8)
    first.ravel()[0] = 1
    return compact, ids, cols, first


ROWS = [1, 127, 128, 129, 1025]


@pytest.mark.parametrize("kind", ["one_class", "class_per_row", "interleaved"])
@pytest.mark.parametrize("n_rows", ROWS)
def test_rows_and_classes(device, n_rows, kind):
    """One class of all rows: weights 1, 127 (seven planes), 128 (one plane), 129, 1025.  A class per row: one plane, the row
    route's table.  A dozen classes dealt to the rows at random: not contiguous."""
    rng = np.random.default_rng(31 * n_rows + len(kind))
    if kind == "one_class":
        class_of = np.zeros(n_rows, dtype=np.uint32)
    elif kind == "class_per_row":
        class_of = rng.permutation(n_rows).astype(np.uint32)
    else:
        class_of = rng.integers(0, min(n_rows, 12), n_rows).astype(np.uint32)
        class_of[rng.permutation(n_rows)[:min(n_rows, 12)]] = np.arange(min(n_rows, 12))      # every class has a row
    n_classes = int(class_of.max()) + 1
    c_prev = {"one_class": 1, "class_per_row": 2, "interleaved": 8}[kind]
    compact, ids, cols, first = random_step(rng, n_classes, 13, 9, c_prev)
    check_classes(device, compact, class_of, ids, cols, first, top_n=20)


@pytest.mark.parametrize("order", ["by_class", "interleaved"])
def test_weights_at_the_powers_of_two(device, order):
    """Weights exactly 2^k (one plane each) and 2^k - 1 (every plane below k) for k = 1 .. 12."""
    rng = np.random.default_rng(len(order))
    weights = [w for k in range(1, 13) for w in (2 ** k, 2 ** k - 1)]
    class_of = classes_of_weights(weights, rng if order == "interleaved" else None)
    compact, ids, cols, first = random_step(rng, len(weights), 11, 7, 2 if order == "by_class" else 1)
    check_classes(device, compact, class_of, ids, cols, first, top_n=15)


@pytest.mark.parametrize("ratio", [2, 3])
def test_geometric_class_sizes(device, ratio):
    rng = np.random.default_rng(ratio)
    weights = [ratio ** k for k in range(14 if ratio == 2 else 9)]
    class_of = classes_of_weights(weights, rng)
    compact, ids, cols, first = random_step(rng, len(weights), 10, 6, 3)
    check_classes(device, compact, class_of, ids, cols, first, top_n=12)


@pytest.mark.parametrize("n_share", [127, 128, 129])
def test_plane_padding(device, n_share):
    """127, 128 and 129 classes that share bit 2 (a block of a plane short of one row, full, and one row into the next), a
    few of them with bit 0 as well, and one class alone in the highest plane."""
    rng = np.random.default_rng(n_share)
    weights = [4] * n_share + [8192]
    for c in (0, 5, n_share - 1):
        weights[c] = 5
    class_of = classes_of_weights(weights, rng)
    compact, ids, cols, first = random_step(rng, len(weights), 9, 5, 2)
    check_classes(device, compact, class_of, ids, cols, first, top_n=9)


TILES = [(1, 1, 1), (1, 64, 2), (1, 65, 8), (64, 1, 2), (64, 64, 1), (64, 65, 2), (65, 1, 8), (65, 64, 2), (65, 65, 1)]


@pytest.mark.parametrize("n_sets,n_cols,c_prev", TILES)
def test_tiles(device, n_sets, n_cols, c_prev):
    rng = np.random.default_rng(1000 * n_sets + 10 * n_cols + c_prev)
    weights = rng.integers(1, 40, 37).tolist()
    class_of = classes_of_weights(weights, rng)
    compact, ids, cols, first = random_step(rng, len(weights), max(n_cols, 9) + 2, n_sets, c_prev, n_cols)
    check_classes(device, compact, class_of, ids, cols, first, top_n=max(1, int(first.sum()) // 3))


def cut_case(kind):
    rng = np.random.default_rng(len(kind) + 17)
    n_allele, n_sets = 20, 10
    weights = rng.integers(1, 30, 23).tolist()
    class_of = classes_of_weights(weights, rng)
    compact = rng.integers(0, 256, (n_allele, len(weights))).astype(np.uint8)
    ids = rng.integers(0, n_allele, (n_sets, 1)).astype(np.int32)
    cols = np.arange(n_allele, dtype=np.int32)
    first = np.ones((n_sets, n_allele), dtype=np.uint8)
    return compact, class_of, ids, cols, first


def test_no_candidate(device):
    compact, class_of, ids, cols, first = cut_case("none")
    first[:] = 0
    b, hdr = check_classes(device, compact, class_of, ids, cols, first, top_n=5, cap=8)
    assert b.count == 0 and hdr.tolist() == [0, 0, 0, 0]


def test_one_candidate(device):
    compact, class_of, ids, cols, first = cut_case("one")
    first[:] = 0
    first[7, 13] = 1
    for top_n in (1, 2, 600):
        b, hdr = check_classes(device, compact, class_of, ids, cols, first, top_n=top_n, cap=4)
        assert hdr.tolist() == [1, int(b.M[7, 13]), 1, 0]


@pytest.mark.parametrize("top_n", ["one", "count", "far"])
def test_top_n_against_the_count(device, top_n):
    compact, class_of, ids, cols, first = cut_case("count")
    first[::3, ::2] = 0
    count = int(first.sum())
    n = {"one": 1, "count": count, "far": 1 << 30}[top_n]
    b, hdr = check_classes(device, compact, class_of, ids, cols, first, top_n=n, cap=count + 5)
    if top_n == "one":
        assert int(hdr[1]) == b.flat[b.mask].min()
    else:
        assert int(hdr[2]) == count and int(hdr[1]) == b.flat[b.mask].max()


def test_every_total_the_same(device):
    compact, class_of, ids, cols, first = cut_case("same")
    compact[:] = compact[0]
    first[2, 5:9] = 0
    for top_n in (1, 1000):
        b, hdr = check_classes(device, compact, class_of, ids, cols, first, top_n=top_n)
        assert b.span == 0 and int(hdr[2]) == b.count == 196


def test_tie_group_across_the_cut(device):
    """Six identical columns: every set has six equal totals; a top_n inside such a group takes all of it."""
    compact, class_of, ids, cols, first = cut_case("ties")
    compact[1:6] = compact[0]
    ids[:, 0] = np.arange(10) + 6
    b1 = sr.bound_reference(expand(compact, class_of), ids, cols, first, 1)
    order = np.argsort(b1.flat, kind="stable")
    inside = next(k for k in range(2, 150) if b1.flat[order[k - 1]] == b1.flat[order[k]] == b1.flat[order[k - 2]])
    b, hdr = check_classes(device, compact, class_of, ids, cols, first, top_n=inside)
    assert int(hdr[2]) > inside and (b.flat[b.selection] == b.kth).sum() >= 3


def test_mask_hides_the_smallest_totals(device):
    compact, class_of, ids, cols, first = cut_case("hidden")
    b0 = sr.bound_reference(expand(compact, class_of), ids, cols, first, 1)
    first = (b0.M > np.median(b0.M)).astype(np.uint8)
    b, hdr = check_classes(device, compact, class_of, ids, cols, first, top_n=10)
    assert b.base > b0.base and int(hdr[1]) > np.median(b0.M) and 10 <= int(hdr[2]) < b.count


@pytest.mark.parametrize("cap", [1, 64])
def test_more_selected_than_the_caller_has_room_for(device, cap):
    compact, class_of, ids, cols, first = cut_case("cap")
    b, hdr = check_classes(device, compact, class_of, ids, cols, first, top_n=65, cap=cap)
    assert int(hdr[2]) >= 65 > cap


@pytest.mark.parametrize("c_prev", [1, 2])
def test_the_64_bit_step(device, c_prev):
    """8.5 M rows in two classes, three columns of 255s (one byte of 254): psum + msum - SAD passes 2^32, every weighted
    sum on the way is formed in 64 bits; the column sums by class are checked in run_step."""
    n_rows = 8_500_000
    class_of = np.zeros(n_rows, dtype=np.uint32)
    class_of[1::2] = 1
    class_of[-3:] = 1                                  # weights 4 249 999 and 4 250 001
    compact = np.full((3, 2), 255, dtype=np.uint8)
    compact[2, 1] = 254
    ids = np.array([[0, 1][:c_prev]], dtype=np.int32)
    cols = np.array([1, 2], dtype=np.int32)
    first = np.ones((1, 2), dtype=np.uint8)
    b, hdr = check_classes(device, compact, class_of, ids, cols, first, top_n=1)
    assert 2 * b.kth > 2 ** 32 and int(hdr[2]) == 1


def small_call(device, **over):
    """A valid small call with single arguments replaced; -> the return code."""
    rng = np.random.default_rng(3)
    class_of = classes_of_weights([3, 5, 1, 7])
    compact, ids, cols, first = random_step(rng, 4, 6, 3, 2)
    miss = expand(compact, class_of)
    n_rows = miss.shape[1]
    ldm = 64
    table8 = np.zeros((7, ldm), dtype=np.uint8)
    table8[:6, :n_rows] = miss
    d_miss, d_msum, d_cls = device.put(table8), device.alloc(8, np.uint32), device.put(class_of)
    hdr, idx, mm = np.zeros(4, np.uint32), np.zeros(64, np.int32), np.zeros(64, np.uint32)
    a = dict(ctx=device.ctx, miss=d_miss.ptr, ldm=ldm, n_rows=n_rows, cls=d_cls.ptr, n_classes=4, msum=d_msum.ptr,
             ids=ids.ctypes.data, n_sets=3, c_prev=2, cols=cols.ctypes.data, n_cols=len(cols), first=first.ctypes.data,
             top_n=3, cap=64, hdr=hdr.ctypes.data, idx=idx.ctypes.data, mm=mm.ctypes.data)
    a.update(over)
    try:
        return lib().gk_bound_step_classes(*a.values())
    finally:
        d_miss.free(); d_msum.free(); d_cls.free()


BAD = [dict(miss=0), dict(cls=0), dict(msum=0), dict(ids=None), dict(cols=None), dict(first=None), dict(hdr=None),
       dict(idx=None), dict(mm=None), dict(n_classes=0), dict(n_classes=17), dict(n_sets=0), dict(n_cols=0), dict(c_prev=0),
       dict(c_prev=9), dict(top_n=0), dict(cap=0), dict(ldm=63), dict(ldm=0), dict(n_rows=0),
       dict(n_rows=16_000_000, ldm=16_000_000, n_classes=4), dict(n_classes=3)]


def test_a_valid_small_call(device):
    assert small_call(device) == 0


@pytest.mark.parametrize("bad", BAD, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_argument_checks_refuse(device, bad):
    """Null pointers, the class count (0, beyond the rows, below a class that a row names), the checks of gk_bound_step,
    the 16 M row limit."""
    assert small_call(device, **bad) != 0
    assert small_call(device) == 0          # and the context is fit for the next call


def test_hook_off_takes_the_rows(device, monkeypatch):
    rng = np.random.default_rng(8)
    weights = rng.integers(1, 300, 50).tolist()
    class_of = classes_of_weights(weights, rng)
    compact, ids, cols, first = random_step(rng, len(weights), 12, 8, 2)
    miss = expand(compact, class_of)
    b = sr.bound_reference(miss, ids, cols, first, 10)
    cap = len(b.selection) + 3
    back = {}
    for form in ("on", "off"):
        monkeypatch.setenv("GK_TEST_HOOKS", f"class_bound={form}")
        hdr, idx, mm = run_step(device, miss, class_of, len(weights), ids, cols, first, 10, cap)
        back[form] = (hdr.tolist(),) + tuple(x.tolist() for x in sorted_pairs(idx, mm, int(hdr[2])))
    monkeypatch.delenv("GK_TEST_HOOKS")
    hdr, idx, mm = run_step(device, miss, class_of, len(weights), ids, cols, first, 10, cap, by_class=False)
    rows = (hdr.tolist(),) + tuple(x.tolist() for x in sorted_pairs(idx, mm, int(hdr[2])))
    assert back["on"] == back["off"] == rows
    assert back["on"][0] == [b.count, b.cut, len(b.selection), 0] and back["on"][1] == b.selection.tolist()
