"""GPU: the exclusive scan and the stable compaction of csrc/gk_scan.hip and the gene partition of csrc/gk_typing.hip
(part_pass / part_offsets), driven through gk_select_nonempty and gk_select_gene on tables from gk_tab_from_csr, against the
restatements of tests/select_reference.py.  Every output is compared whole and in order; every comparison is an equality.

Launch arithmetic, read from the entry points:

* gk_compact_enqueue takes the two-launch route (compact_count, compact_scatter: 1024 items per workgroup) for
  ceil(n / 1024) <= 4096 workgroups, i.e. up to n = 4096 * 1024, and flags_to_u32 + gk_scan_u32 + scatter_selected beyond.
  In compact_scatter thread t sums the counts of workgroups t, t + 256, ... before its own: the loop takes a second trip from
  workgroup 257 on, which n = 257 * 1024 + 3 has (258 workgroups, the last one holding 3 items).
* scan_rec scans tiles of 2048 words and recurses over the tile sums while there is more than one tile: one level up to
  2048 words, two up to 2048^2 = 4 194 304, three from 4 194 305 on (2049 tiles, then 2, then 1).  The compaction's fallback
  begins at n = 4096 * 1024 + 1 = 4 194 305: the same length.  Item 4 194 304 is the only one whose position needs the third
  level's offset, so the patterns that keep the last item are the ones that read it.
* build_partition scans a histogram of 256 * ceil(n / 64) words (a table from gk_tab_from_csr has 256 bins), bin-major: 512
  rows give 2048 words (one tile), 513 rows 2304 (two levels), 1 048 576 rows 2048^2 (the last two-level length), 1 048 577
  rows 4 194 560 (three levels).  The words beyond 2048^2 there are gene 255's last 256 waves."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import select_reference as sr  # noqa: E402

from kir_graph_amd._lib import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu

FILL = 0xA5
SENTINEL = np.frombuffer(bytes([FILL] * 4), dtype=np.int32)[0]      # no row number: negative
TAIL = 37

# row 0: nothing; row 1: one positive id; row 2: one negative id; row 3: one id on both sides; row 4: two positive ids
ROWS = [[[], [], [], []], [[0], [], [], []], [[], [], [], [1]], [[2], [], [2], []], [[3], [4], [], []]]
N_VAR = 5

LENGTHS = [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2048, 2049, 257 * 1024 + 3, 4096 * 1024, 4096 * 1024 + 1]
PATTERNS = ["random", "all", "none", "first", "last", "1023_1024", "lane63", "bit0", "bit1"]


def makeTable(device, off, ids, gene, nh):
    h = C.c_void_p()
    n = (len(off) - 1) // 4
    check(lib().gk_tab_from_csr(device.ctx, N_VAR, n, off.ctypes.data, ids.ctypes.data if len(ids) else None, gene.ctypes.data,
                                nh.ctypes.data, C.byref(h)))
    return h


def sentinelBuffer(device, count):
    buf = device.alloc(count, np.int32)
    check(lib().gk_memset(device.ctx, buf.ptr, FILL, buf.nbytes))
    return buf


# ------------------------------------------------------------------------------------------------ compaction
@pytest.fixture(scope="module")
def lists():
    return sr.packLists(ROWS)


@pytest.fixture(scope="module")
def table(device, lists):
    off, ids = lists
    h = makeTable(device, off, ids, np.zeros(len(ROWS), np.uint8), np.ones(len(ROWS), np.uint8))
    yield h
    lib().gk_tab_destroy(h)


def pattern(kind, n, rng):
    """(rows int32 [n], drop flags uint8 [N_VAR], number kept or None)."""
    none = np.zeros(N_VAR, dtype=np.uint8)
    if kind == "random":       # flags under which rows 0 and 1 are dead; row 3 lives on its negative id, row 4 on its second
        return rng.choice(5, n, p=[0.25, 0.25, 1 / 6, 1 / 6, 1 / 6]), np.array([1, 0, 1, 1, 0], dtype=np.uint8), None
    if kind == "all":
        return rng.integers(1, 5, n), none, n
    if kind == "none":
        return rng.integers(0, 5, n), np.full(N_VAR, 3, dtype=np.uint8), 0
    if kind == "bit0":         # rows 1 and 4 die, rows 2 and 3 live on negative ids
        return rng.integers(0, 5, n), np.full(N_VAR, 1, dtype=np.uint8), None
    if kind == "bit1":         # row 2 dies, rows 1, 3 and 4 live on positive ids
        return rng.integers(0, 5, n), np.full(N_VAR, 2, dtype=np.uint8), None
    keep = np.zeros(n, dtype=bool)
    if kind == "first":
        keep[0] = True
    elif kind == "last":
        keep[n - 1] = True
    elif kind == "1023_1024":
        keep[1023:1025] = True
    else:
        assert kind == "lane63"
        keep[63::64] = True
    rows = np.zeros(n, dtype=np.int64)
    rows[keep] = rng.integers(1, 5, int(keep.sum()))
    return rows, none, int(keep.sum())


@pytest.mark.parametrize("n", LENGTHS)
def test_compaction_keeps_the_surviving_rows_in_order(device, table, lists, n):
    off, ids = lists
    rng = np.random.default_rng(n)
    for kind in PATTERNS:
        rows, vflag, n_kept = pattern(kind, n, rng)
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        want = sr.selectRows(rows, sr.aliveRows(off, ids, vflag))
        if n_kept is not None:
            assert len(want) == n_kept, kind                      # the pattern is what its name says
        elif n >= 255:
            assert 0.3 * n < len(want) < 0.8 * n, kind
        d_rows, d_flag, out = device.put(rows), device.put(vflag), sentinelBuffer(device, n + TAIL)
        n_out = C.c_int64(-1)
        try:
            check(lib().gk_select_nonempty(device.ctx, table, d_rows.ptr, n, d_flag.ptr, out.ptr, C.byref(n_out)))
            got = out.download()
        finally:
            d_rows.free()
            d_flag.free()
            out.free()
        assert n_out.value == len(want), (kind, n_out.value, len(want))
        assert np.array_equal(got[:len(want)], want), kind
        assert (got[len(want):] == SENTINEL).all(), kind          # nothing beyond the kept part, tail included


# ------------------------------------------------------------------------------------------------ partition
ABSENT, LAST_ONLY, FULL_WAVE = 7, 9, 200
DISTINCT = np.arange(100, 164)
FORCED = [0, 255, ABSENT, LAST_ONLY, FULL_WAVE, 100, 163]
COUNTS = [1, 63, 64, 65, 256, 257, 512, 513, 1 << 20, (1 << 20) + 1]


def layouts(n):
    return ["forced", "one_gene", "distinct"] if n < 192 else ["forced"]


def genesOf(n, layout, rng):
    """(pair_gene, pair_nh): random backbones 0 .. 255 and NH in {1, 2}, then the forced cases of the layout."""
    gene = rng.integers(0, 256, n).astype(np.uint8)
    nh = rng.integers(1, 3, n).astype(np.uint8)
    gene[gene == ABSENT] = ABSENT + 1                 # a gene without rows
    gene[gene == LAST_ONLY] = LAST_ONLY + 1
    if layout == "one_gene":                          # the first wave: up to 64 rows of gene 255
        gene[:64] = 255
    elif layout == "distinct":                        # the first wave: up to 64 rows of 64 genes, 255 the last
        gene[:64] = (192 + np.arange(64))[:min(n, 64)]
    else:
        if n >= 192:
            gene[64:128] = FULL_WAVE                  # wave 1: 64 rows of one gene
            gene[128:192] = rng.permutation(DISTINCT)  # wave 2: 64 rows of 64 genes
        if n >= 3:
            gene[0], gene[1] = 0, 255
        gene[n - 1], nh[n - 1] = LAST_ONLY, 1         # a gene whose only row is the sample's last
    return gene, nh


@pytest.mark.parametrize("n", COUNTS)
def test_partition_lists_every_gene_in_row_order(device, n):
    large = n >= 1 << 20
    for layout in layouts(n):
        rng = np.random.default_rng(31 * n + len(layout))
        gene, nh = genesOf(n, layout, rng)
        if layout == "forced":
            assert not (gene == ABSENT).any() and np.flatnonzero(gene == LAST_ONLY).tolist() == [n - 1]
        if large:                                     # gene 255 has rows in its last 256 waves: the words beyond 2048^2
            assert (gene[n - 256 * 64:] == 255).any() and (gene[:64] == 255).any()
        genes = sorted(set(FORCED) | set(np.random.default_rng(n).choice(256, 16, replace=False).tolist())) if large \
            else list(range(256))
        tab = makeTable(device, np.zeros(4 * n + 1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), gene, nh)
        out = sentinelBuffer(device, n + TAIL)
        try:
            for multiple in (0, 1):
                seen = 0
                for g in genes:
                    want = sr.genePartition(gene, nh, g, multiple)
                    n_out = C.c_int64(-1)
                    check(lib().gk_select_gene(device.ctx, tab, g, multiple, out.ptr, C.byref(n_out)))
                    keep = len(want) + TAIL
                    got = out.download(keep)
                    where = (layout, multiple, g)
                    assert n_out.value == len(want), where
                    assert np.array_equal(got[:len(want)], want), where
                    assert (got[len(want):] == SENTINEL).all(), where
                    if len(want):                     # the part just written goes back to sentinels for the next gene
                        check(lib().gk_memset(device.ctx, out.ptr, FILL, 4 * len(want)))
                    seen += len(want)
                if not large:
                    assert seen == (n if multiple else int((nh == 1).sum())), (layout, multiple)
            if large:                                 # nothing was written beyond any gene's count: the whole buffer is clean
                assert (out.download() == SENTINEL).all()
        finally:
            out.free()
            lib().gk_tab_destroy(tab)
