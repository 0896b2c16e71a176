"""gk_maxsum / gk_setmax / gk_fraction / gk_setsum straight through the C ABI at the row counts where the summation tree
changes shape, with NaN rows behind every column, across the flush of the program cache, on both sides of every tile, batch
and staging limit, and on sets that repeat an allele -- against numpy's own expressions, bit for bit
(tests/searchtree_reference.py; tests/test_search_reference_host.py shows that the tables tell numpy's order from others)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import searchtree_reference as sr  # noqa: E402

from kir_graph_amd._lib import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu

LEAF_GROUPS = 128                      # sets per slot of setsum_leaves
LEAF_SLOTS = {2: 6, 3: 4, 4: 3}        # slots of a launch by alleles per set


class Table:
    """A table in HBM, column-major with ``pad`` NaN rows behind every column."""

    def __init__(self, device, L, pad=0):
        self.device, self.L = device, L
        self.n_rows, self.n_allele = L.shape
        self.ld = self.n_rows + pad
        self.buf = device.put(sr.padded(L, pad))

    def free(self):
        self.buf.free()

    def maxsum(self, ids, cols, n_rows=None):
        n_rows = n_rows or self.n_rows
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        if ids is None:
            out = np.full((1, len(cols)), np.nan)
            check(lib().gk_maxsum(self.device.ctx, self.buf.ptr, n_rows, self.ld, None, 1, 0, cols.ctypes.data, len(cols),
                                  out.ctypes.data))
            return out[0]
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.full((len(ids), len(cols)), np.nan)
        check(lib().gk_maxsum(self.device.ctx, self.buf.ptr, n_rows, self.ld, ids.ctypes.data, ids.shape[0], ids.shape[1],
                              cols.ctypes.data, len(cols), out.ctypes.data))
        return out

    def setmax(self, ids):
        """[row][set], the first n_rows rows of every column of the buffer."""
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        buf = self.device.alloc((len(ids), self.ld), np.float64)
        check(lib().gk_setmax(self.device.ctx, self.buf.ptr, self.n_rows, self.ld, ids.ctypes.data, ids.shape[0],
                              ids.shape[1], buf.ptr))
        got = buf.download().reshape(len(ids), self.ld)[:, :self.n_rows].T
        buf.free()
        return got

    def fraction(self, ids):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        out = np.full(ids.shape, np.nan)
        check(lib().gk_fraction(self.device.ctx, self.buf.ptr, self.n_rows, self.ld, ids.ctypes.data, ids.shape[0],
                                ids.shape[1], out.ctypes.data))
        return out

    def setsum(self, ids, n_rows=None):
        n_rows = n_rows or self.n_rows
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        value, frac = np.full(len(ids), np.nan), np.full(ids.shape, np.nan)
        check(lib().gk_setsum(self.device.ctx, self.buf.ptr, n_rows, self.ld, ids.ctypes.data, ids.shape[0],
                              ids.shape[1], value.ctypes.data, frac.ctypes.data))
        return value, frac


def use_form(monkeypatch, form):
    if form is None:
        monkeypatch.delenv("GK_TEST_HOOKS", raising=False)
    else:
        monkeypatch.setenv("GK_TEST_HOOKS", f"setsum={form}")


def launches(device, call):
    """What ``call`` returns, and {kernel: launches} of the kernels it ran."""
    device.profEnable(True)
    device.profCollect()
    try:
        got = call()
        ran = {k: v[0] for k, v in device.profCollect().items()}
    finally:
        device.profEnable(False)
    return got, ran


def check_setsum(T, monkeypatch, ids, forms=("leaves", "tiles")):
    """gk_setsum in the given forms: value and shares are numpy's."""
    want_value = sr.setvalue_numpy(T.L, ids)
    want_frac = sr.shares_numpy(T.L, ids) / T.n_rows
    for form in forms:
        use_form(monkeypatch, form)
        value, frac = T.setsum(ids)
        assert np.array_equal(value, want_value), form
        assert np.array_equal(frac, want_frac), form
    return want_value, want_frac


def every_entry(device, monkeypatch, L, pad):
    n_rows, n_allele = L.shape
    T = Table(device, L, pad)
    try:
        cols = np.arange(n_allele, dtype=np.int32)[::-1]
        assert np.array_equal(T.maxsum(None, cols), sr.colsum_numpy(L, cols))
        cols = np.arange(n_allele, dtype=np.int32)
        for c in (1, 2):
            ids = sr.sweep_sets(n_rows, c)
            assert np.array_equal(T.maxsum(ids, cols), sr.maxsum_numpy(L, ids, cols)), c
            assert np.array_equal(T.setmax(ids), L[:, ids].max(axis=2)), c
        for c in (1, 2, 3, 4, 8):
            ids = sr.sweep_sets(n_rows, c)
            assert np.array_equal(T.fraction(ids), sr.shares_numpy(L, ids) / n_rows), c
            check_setsum(T, monkeypatch, ids, ("leaves", "tiles") if 2 <= c <= 4 else ("tiles",))
    finally:
        T.free()


@pytest.mark.parametrize("kind", sr.TABLES)
@pytest.mark.parametrize("n_rows", sr.SWEEP)
def test_row_sweep(device, monkeypatch, n_rows, kind):
    every_entry(device, monkeypatch, sr.make_table(kind, n_rows), 0)


@pytest.mark.parametrize("kind", sr.TABLES)
@pytest.mark.parametrize("pad", [3, 61])
@pytest.mark.parametrize("n_rows", sr.PADDED_SWEEP)
def test_rows_behind_a_column_are_never_read(device, monkeypatch, n_rows, pad, kind):
    """ld = n_rows + pad with NaN in the padding: one row too far in a max or a sum makes an output NaN."""
    every_entry(device, monkeypatch, sr.make_table(kind, n_rows), pad)


def test_program_cache_is_flushed_and_refilled(device, monkeypatch):
    """70 row counts the context has not seen: the cache of tree programs (64) is flushed on the way; a row count from
    before the flush is built again.  The leaf-wise set sums run in between, their tickets reused from launch to launch."""
    use_form(monkeypatch, "leaves")
    counts = list(range(3301, 3301 + 70))
    L = sr.make_table("wide", counts[-1])
    T = Table(device, L)                       # ld = the largest count; every call sums the first n rows
    cols = np.arange(sr.N_ALLELE, dtype=np.int32)
    ids = sr.sweep_sets(3301, 2)
    try:
        def both(n):
            assert np.array_equal(T.maxsum(None, cols, n_rows=n), sr.colsum_numpy(L[:n], cols)), n
            value, frac = T.setsum(ids, n_rows=n)
            assert np.array_equal(value, sr.setvalue_numpy(L[:n], ids)), n
            assert np.array_equal(frac, sr.shares_numpy(L[:n], ids) / n), n
        for n in counts:
            both(n)
        both(counts[4])
        both(counts[-1])
    finally:
        T.free()


TILE_ROWS = [137, 8199]


@pytest.fixture(scope="module")
def tile_tables():
    return {n: sr.table(np.random.default_rng(5000 + n), n, 70) for n in TILE_ROWS}


@pytest.mark.parametrize("n_rows", TILE_ROWS)
@pytest.mark.parametrize("n_sets,n_cols,c_prev", [(31, 33, 1), (32, 64, 1), (33, 31, 2), (64, 65, 1), (65, 32, 2),
                                                  (32, 32, 1), (1, 65, 1), (65, 1, 1), (33, 33, 0)])
def test_maxsum_tile_edges(device, tile_tables, n_rows, n_sets, n_cols, c_prev):
    """32 sets x 32 columns per workgroup: 31, 32, 33, 64 and 65 of either."""
    L = tile_tables[n_rows]
    rng = np.random.default_rng(n_sets * 100 + n_cols)
    T = Table(device, L)
    try:
        cols = rng.permutation(70)[:n_cols].astype(np.int32)
        if c_prev == 0:                        # several sets without previous alleles: every row of the result the column sums
            out = np.full((n_sets, n_cols), np.nan)
            check(lib().gk_maxsum(device.ctx, T.buf.ptr, n_rows, T.ld, None, n_sets, 0, cols.ctypes.data, n_cols,
                                  out.ctypes.data))
            assert np.array_equal(out, np.tile(sr.colsum_numpy(L, cols), (n_sets, 1)))
            return
        ids = rng.integers(0, 70, (n_sets, c_prev)).astype(np.int32)
        assert np.array_equal(T.maxsum(ids, cols), sr.maxsum_numpy(L, ids, cols))
    finally:
        T.free()


@pytest.mark.parametrize("n_rows", TILE_ROWS)
@pytest.mark.parametrize("case", ["32", "33", "65", "duplicate", "other_list", "rank_order"])
def test_maxsum_symmetric_shortcut_and_its_refusals(device, tile_tables, n_rows, case):
    """Sets = the columns themselves: from 33 on the upper triangle is computed and mirrored.  Not when two sets name the
    same allele, and not when the columns are another list than the sets."""
    L = tile_tables[n_rows]
    rng = np.random.default_rng(len(case) + n_rows)
    n = int(case) if case.isdigit() else 40
    alleles = rng.permutation(70)[:n].astype(np.int32)
    cols = alleles.copy()
    ids = rng.permutation(alleles)
    if case == "duplicate":
        ids[7] = ids[30]
    elif case == "other_list":
        cols = rng.permutation(70)[:n].astype(np.int32)
        assert set(cols.tolist()) != set(alleles.tolist())
    elif case == "rank_order":
        ids = alleles.copy()
    T = Table(device, L)
    try:
        got = T.maxsum(ids[:, None], cols)
        assert np.array_equal(got, sr.maxsum_numpy(L, ids[:, None], cols))
        if case not in ("duplicate", "other_list"):       # the table of set pairs is symmetric, bit for bit
            inv = {int(a): j for j, a in enumerate(cols)}
            order = [inv[int(a)] for a in ids]
            assert np.array_equal(got[:, order], got[:, order].T)
    finally:
        T.free()


@pytest.mark.parametrize("n_rows", TILE_ROWS)
@pytest.mark.parametrize("c,n_sets", [(2, 128), (2, 129), (2, 256), (2, 257), (2, 640), (2, 641), (2, 768), (2, 769),
                                      (3, 512), (3, 513), (4, 384), (4, 385)])
def test_leafwise_slots_and_batches(device, monkeypatch, tile_tables, n_rows, c, n_sets):
    """1 .. 6 sets per lane group, and the set counts at which a second launch is needed."""
    L = tile_tables[n_rows][:, :40]
    rng = np.random.default_rng(n_sets * 10 + c)
    ids = rng.integers(0, 40, (n_sets, c)).astype(np.int32)
    ids[:40, 0] = 3
    ids[-1, :] = 39                            # the last set, homozygous, names the last column
    T = Table(device, L)
    try:
        use_form(monkeypatch, "leaves")
        (value, frac), ran = launches(device, lambda: T.setsum(ids))
        per_launch = LEAF_GROUPS * LEAF_SLOTS[c]
        assert ran.get("setsum_leaves") == (n_sets + per_launch - 1) // per_launch and "fraction_chunks" not in ran
        assert np.array_equal(value, sr.setvalue_numpy(L, ids))
        assert np.array_equal(frac, sr.shares_numpy(L, ids) / n_rows)
        use_form(monkeypatch, "tiles")
        (value2, frac2), ran = launches(device, lambda: T.setsum(ids))
        assert ran.get("fraction_chunks") == 1 and "setsum_leaves" not in ran
        assert np.array_equal(value2, value) and np.array_equal(frac2, frac)
    finally:
        T.free()


@pytest.mark.parametrize("n_rows", TILE_ROWS)
@pytest.mark.parametrize("n_allele", [256, 257, 505, 506])
@pytest.mark.parametrize("c", [2, 3])
def test_leafwise_column_limits(device, monkeypatch, n_rows, n_allele, c):
    """Up to 256 columns ride in registers while a block is summed, more are staged by a loop; 505 columns fill the LDS a
    workgroup may have, 506 are summed by tiles whatever the caller asks for."""
    L = sr.table(np.random.default_rng(n_rows + n_allele), n_rows, n_allele)
    rng = np.random.default_rng(n_allele + c)
    ids = rng.integers(0, n_allele, (70, c)).astype(np.int32)
    ids[0, :] = n_allele - 1
    ids[1, 0] = 0
    ids[2] = [n_allele - 1, 0, 255][:c]
    T = Table(device, L, pad=5)
    try:
        use_form(monkeypatch, "leaves")
        (value, frac), ran = launches(device, lambda: T.setsum(ids))
        if n_allele <= 505:
            assert ran.get("setsum_leaves") == 1 and "fraction_chunks" not in ran
        else:
            assert ran.get("fraction_chunks") == 1 and "setsum_leaves" not in ran
        assert np.array_equal(value, sr.setvalue_numpy(L, ids))
        assert np.array_equal(frac, sr.shares_numpy(L, ids) / n_rows)
        use_form(monkeypatch, "tiles")
        value2, frac2 = T.setsum(ids)
        assert np.array_equal(value2, value) and np.array_equal(frac2, frac)
    finally:
        T.free()


@pytest.mark.parametrize("n_rows", TILE_ROWS)
@pytest.mark.parametrize("n_sets,n_named,leafwise", [(63, 49, False), (64, 49, True), (63, 50, True), (13, 50, True),
                                                      (12, 48, False)])
def test_dense_rule_picks_the_form(device, monkeypatch, n_rows, n_sets, n_named, leafwise):
    """Without a hook: leaf by leaf from 64 sets on, or when the sets name a quarter of the columns below the largest id."""
    n_allele = 200
    L = sr.table(np.random.default_rng(n_rows + n_sets), n_rows, n_allele)
    rng = np.random.default_rng(n_sets + n_named)
    named = np.concatenate([rng.permutation(n_allele - 1)[:n_named - 1], [n_allele - 1]]).astype(np.int32)
    ids = named[rng.integers(0, n_named, (n_sets, 4))]
    ids.ravel()[:n_named] = named              # every one of them is named
    assert len(np.unique(ids)) == n_named and ids.max() == n_allele - 1
    T = Table(device, L)
    try:
        use_form(monkeypatch, None)
        (value, frac), ran = launches(device, lambda: T.setsum(ids))
        assert ("setsum_leaves" in ran) == leafwise and ("fraction_chunks" in ran) == (not leafwise)
        assert np.array_equal(value, sr.setvalue_numpy(L, ids))
        assert np.array_equal(frac, sr.shares_numpy(L, ids) / n_rows)
    finally:
        T.free()


@pytest.mark.parametrize("n_sets", [3072, 3073])
def test_set_ceiling_of_the_leafwise_form(device, monkeypatch, n_sets):
    """3072 sets are four launches of the leaf kernel; one more and the tiles take over."""
    n_rows = 137
    L = sr.table(np.random.default_rng(n_sets), n_rows, 90)
    ids = np.random.default_rng(n_sets + 1).integers(0, 90, (n_sets, 2)).astype(np.int32)
    ids[-1, :] = 89
    T = Table(device, L)
    try:
        use_form(monkeypatch, None)
        (value, frac), ran = launches(device, lambda: T.setsum(ids))
        if n_sets <= 3072:
            assert ran.get("setsum_leaves") == 4 and "fraction_chunks" not in ran
        else:
            assert ran.get("fraction_chunks") == 1 and "setsum_leaves" not in ran
        assert np.array_equal(value, sr.setvalue_numpy(L, ids))
        assert np.array_equal(frac, sr.shares_numpy(L, ids) / n_rows)
    finally:
        T.free()


@pytest.mark.parametrize("n_rows", [137, 1033, 8199])
def test_sets_that_repeat_an_allele(device, monkeypatch, n_rows):
    """Homozygous sets ([a, a]: every row a tie of the set with itself), [a, a, b], eight times one allele, a hub allele
    shared by 40 sets, and a table with two identical columns."""
    n_allele = 30
    L = sr.table(np.random.default_rng(n_rows), n_rows, n_allele)
    L[:, 11] = L[:, 4]                                   # two alleles nothing tells apart
    a = np.arange(n_allele, dtype=np.int32)
    rng = np.random.default_rng(n_rows + 1)
    T = Table(device, L, pad=3)
    try:
        homo = np.stack([a, a], axis=1)                  # every [a, a]
        value, frac = check_setsum(T, monkeypatch, homo)
        assert np.array_equal(frac, np.full(homo.shape, 0.5))
        assert np.array_equal(value, T.maxsum(None, a))      # the set's value is the column's sum
        twins = np.array([[4, 11], [11, 4], [4, 4]], dtype=np.int32)
        value, frac = check_setsum(T, monkeypatch, twins)
        assert np.array_equal(frac, np.full(twins.shape, 0.5)) and value[0] == value[1] == value[2]
        aab = np.stack([a, a, np.roll(a, 7)], axis=1)
        check_setsum(T, monkeypatch, aab)
        aabb = np.stack([a, a, np.roll(a, 7), np.roll(a, 7)], axis=1)
        check_setsum(T, monkeypatch, aabb)
        eight = np.repeat(a[:, None], 8, axis=1)
        value, frac = check_setsum(T, monkeypatch, eight, ("tiles",))
        assert np.array_equal(frac, np.full(eight.shape, 0.125))
        assert np.array_equal(T.fraction(eight), frac)
        hub = rng.integers(0, n_allele, (90, 3)).astype(np.int32)
        hub[:40, 0] = 3
        hub[40:60, 1] = hub[40:60, 0]
        check_setsum(T, monkeypatch, hub)
        # previous sets that repeat an allele, as the search sees them
        for prev in (homo, eight, twins):
            assert np.array_equal(T.maxsum(prev, a), sr.maxsum_numpy(L, prev, a))
            assert np.array_equal(T.setmax(prev), L[:, prev].max(axis=2))
        assert np.array_equal(T.maxsum(homo, a), T.maxsum(a[:, None], a))
    finally:
        T.free()


@pytest.mark.parametrize("n_rows", [1, 129, 8193])
@pytest.mark.parametrize("c", [2, 3, 4])
def test_setsum_routes_at_most_8_sets_to_the_few_form(device, monkeypatch, n_rows, c):
    """gk_setsum without a hook: 8 sets run setsum_few and nothing else, 9 sets do not run it; numpy's bits either way."""
    n_allele = 30
    L = sr.table(np.random.default_rng(n_rows * 10 + c), n_rows, n_allele)
    ids = np.random.default_rng(n_rows + c).integers(0, n_allele, (9, c)).astype(np.int32)
    ids[0, :] = n_allele - 1                   # a homozygous set on the last column
    T = Table(device, L, pad=3)
    try:
        use_form(monkeypatch, None)
        for n_sets in (8, 9):
            (value, frac), ran = launches(device, lambda: T.setsum(ids[:n_sets]))
            if n_sets <= 8:
                assert ran.get("setsum_few") == 1 and {k for k, n in ran.items() if n} == {"setsum_few"}, ran
            else:
                assert "setsum_few" not in ran and ("setsum_leaves" in ran) != ("fraction_chunks" in ran), ran
            assert np.array_equal(value, sr.setvalue_numpy(L, ids[:n_sets])), n_sets
            assert np.array_equal(frac, sr.shares_numpy(L, ids[:n_sets]) / n_rows), n_sets
    finally:
        T.free()


RING_DOUBLES = (4 << 20) // 8                  # a result of more float64 than this does not fit a slot of the result ring


@pytest.mark.parametrize("n_sets", [174762, 174763])
def test_setsum_result_on_both_sides_of_the_result_ring(device, monkeypatch, n_sets):
    """Sets of 2 alleles bring back 3 float64 each: 174 762 sets are 524 286 values, the last count that fits a slot of the
    result ring; 174 763 are 524 289, one value past 4 MB, which the ring refuses.  Asserted here: both calls succeed,
    ran the tiles once and give numpy's bits.  WHICH way a result comes back (ring slot, or pool block + queued copy) is
    not visible through the C ABI; tests/test_call_record.py asserts it on both sides of the limit.  The plan of the
    tiles stays under 4 MB on both sides (at most 879 278 int32 for 174 763 sets: tile offsets, two columns, two local
    indices and the position per set), so only the result crosses the limit."""
    n_rows, n_allele, c = 9, 40, 2
    assert (n_sets * (c + 1) > RING_DOUBLES) == (n_sets == 174763)
    n_tiles = (n_sets + 31) // 32
    plan_ints = (n_tiles + 1) + n_sets * c + n_sets * c + n_sets
    assert plan_ints * 4 < (4 << 20) and (n_sets != 174763 or plan_ints == 879278)
    L = sr.table(np.random.default_rng(n_sets), n_rows, n_allele)
    ids = np.random.default_rng(n_sets + 1).integers(0, n_allele, (n_sets, c)).astype(np.int32)
    ids[-1, :] = n_allele - 1
    T = Table(device, L, pad=3)
    try:
        use_form(monkeypatch, None)
        (value, frac), ran = launches(device, lambda: T.setsum(ids))
        assert ran.get("fraction_chunks") == 1 and "setsum_leaves" not in ran and "setsum_few" not in ran, ran
        assert np.array_equal(value, sr.setvalue_numpy(L, ids))
        assert np.array_equal(frac, sr.shares_numpy(L, ids) / n_rows)
    finally:
        T.free()
