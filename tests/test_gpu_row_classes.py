"""The row classes behind ``gk_compat_log_miss`` / ``gk_compat_log_miss_cols`` (csrc/gk_rowclass.hip: the product chains
run once per distinct kept sequence, the results are copied into place): hand-built CSR lists, drop flags and bit rows as
in tests/test_gpu_compat_edges.py, every table against tests/compat_reference.py bit for bit -- doubles as uint64, whole
buffers over a sentinel fill, the zeroed pad of the mismatch table included -- with ``GK_TEST_HOOKS=row_classes=on``, again
with ``off``, and with the hash cut to 0 and to 4 bits (rows of different sequences then meet in one slot and are told
apart by the comparison alone).  The classes themselves (``gk_row_classes``) against tests/rowclass_reference.py: equal
under the full hash, a refinement of it under a cut one, numbered by their lowest row either way."""
import copy
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compat_reference as cr  # noqa: E402
import rowclass_reference as rr  # noqa: E402
import test_gpu_compat_edges as ce  # noqa: E402

from kir_graph_amd._lib import check, lib  # noqa: E402
from kir_graph_amd.engine import LogTable  # noqa: E402

pytestmark = pytest.mark.gpu

HOOKS = {"off": "row_classes=off", "on": "row_classes=on", "on, 0 hash bits": "row_classes=on,rowclass_hashbits=0",
         "on, 4 hash bits": "row_classes=on,rowclass_hashbits=4"}
KEPT_CAP = 256          # a row that keeps more ids than this is a class of its own (kCap of gk_rowclass.hip)

_cases: dict = {}


def gene_case(name, lists, n_allele=3, keep_empty=False, filler_every=3) -> ce.Case:
    """The case of ``lists`` in the hand-built gene of rowclass_reference; built (and its reference computed) once."""
    if name not in _cases:
        off, ids, rows = rr.packed(lists, filler_every)
        _cases[name] = ce.Case(name, off, ids, rr.N_TOTAL, rows, rr.geneFlags(), rr.VBEG, rr.VEND, rr.geneBits(n_allele),
                               keep_empty=keep_empty)
    return _cases[name]


def check_classes(gpu: ce.OnDevice, exact: bool, n_want=None):
    """``gk_row_classes`` against the numpy statement: every class lies inside one class of the reference, the classes are
    numbered by their lowest row; ``exact``: they ARE the reference's (rows that keep more than KEPT_CAP ids apart)."""
    c = gpu.case
    buf = gpu.filled(gpu.n_rows, np.uint32)
    n = C.c_int64(-1)
    check(lib().gk_row_classes(gpu.dev.ctx, gpu.tab, gpu.rows.ptr, gpu.n_rows, gpu.vflag.ptr, buf.ptr, C.byref(n)))
    got = buf.download().reshape(-1)
    buf.free()
    want = rr.classOf(c.off, c.ids, c.rows, c.vflag)
    assert got.max() + 1 == n.value and len(np.unique(got)) == n.value, c.name
    assert len(set(zip(got.tolist(), want.tolist()))) == n.value, c.name          # no class spans two of the reference's
    assert (np.diff(np.unique(got, return_index=True)[1]) > 0).all(), c.name      # numbered by their lowest row
    if exact:
        assert np.array_equal(got, want), c.name
        if n_want is not None:
            assert n.value == n_want, c.name


def check_tables(device, monkeypatch, case: ce.Case, hook: str, cols=None, expect=None, classes="exact", n_classes=None):
    """The case's table from a fresh value table (products stored, patched on the expanded table) and from the warmed one,
    under ``hook``; the classes under the same hook."""
    monkeypatch.setenv("GK_TEST_HOOKS", HOOKS[hook])
    gpu = ce.OnDevice(device, case)
    logs = LogTable(device, log2_capacity=16)
    try:
        fresh = ce.settle_log_miss(gpu, logs, cols)
        ce.assert_log_table(gpu, fresh, cols)
        if expect == "patch":
            assert fresh[3] >= 1 and fresh[4] == 0, fresh[3:]
        if expect == "again":
            assert fresh[4] >= 1, fresh[3:]
        warm = ce.settle_log_miss(gpu, logs, cols)
        assert warm[3] == 0 and warm[4] == 0, warm[3:]
        ce.assert_log_table(gpu, warm, cols)
        if classes:
            check_classes(gpu, exact=(classes == "exact" and "hash bits" not in hook), n_want=n_classes)
    finally:
        logs.close()
        gpu.close()


# ------------------------------------------------------------------------------------------------- rows, tiles, classes
ROWS = [1, 2, 15, 16, 17, 33, 129, 2049]          # 2049 rows: 129 tiles, more than one pass of a grid of 8 x 16 needs
PATTERNS = ["distinct", "identical", "two", "three", "tile edge"]


@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_rows", ROWS)
def test_row_counts_and_class_layouts(device, monkeypatch, n_rows, pattern, hook):
    """All rows distinct (as many classes as rows), all identical (one class), two and three classes interleaved, a class
    whose lowest row is the last row of a tile: the tables and the classes."""
    lists, n_classes = rr.patternLists(pattern, n_rows)
    case = gene_case(f"{pattern} x {n_rows}", lists, keep_empty=bool(n_rows % 2))
    check_tables(device, monkeypatch, case, hook, expect="patch", n_classes=n_classes)


# ------------------------------------------------------------------------------------------------- what merges, what not
A, B, CC, D, E = 12, 13, 14, 15, 16
MERGE = {
    "other dropped ids between": ([[A, 200, B, CC], [], [201, D, E], []], [[A, B, 250, 251, CC], [], [D, 260, E, 270], []]),
    "another split of the mates": ([[A, B, CC], [], [D, E], []], [[A], [B, CC], [], [D, E]]),
    "a chunk of 64 dropped whole": ([[A, B] + rr.DROPPED[:64] + [CC], [], [D, E], []], [[A, B, CC], [], [D, E], []]),
    "dropped on one side only": ([[A, 100, B], [], [105, D], []], [[A], [B, 101], [D, 106], []]),
}
APART = {
    "boundary one place apart": ([[A, B, CC], [], [D, E], []], [[A, B], [], [CC, D, E], []]),
    "another order": ([[A, B, CC], [], [D], []], [[A, CC, B], [], [D], []]),
    "one id outside the span more": ([[A, B], [], [D], []], [[A, B, 2], [], [D], []]),
    "one novel id more": ([[A, B], [], [D], []], [[A, B], [], [D, 350], []]),
    "positive here, negative there": ([[A, B], [], [], []], [[A], [], [B], []]),
    "dropped as positive, kept as negative": ([[A, 100], [], [B], []], [[A], [], [100, B], []]),
}


@pytest.mark.parametrize("hook", list(HOOKS))
def test_rows_that_must_merge_and_rows_that_must_not(device, monkeypatch, hook):
    lists = []
    for k, (x, y) in enumerate(MERGE.values()):
        lists += [x, distinct_filler(k), y]
    for k, (x, y) in enumerate(APART.values()):
        lists += [x, y]
    case = gene_case("merge and apart", lists, n_allele=70)
    cls = rr.classOf(case.off, case.ids, case.rows, case.vflag)
    for k in range(len(MERGE)):
        assert cls[3 * k] == cls[3 * k + 2] != cls[3 * k + 1]
    at = 3 * len(MERGE)
    for k in range(len(APART)):
        assert cls[at + 2 * k] != cls[at + 2 * k + 1]
    check_tables(device, monkeypatch, case, hook)


def distinct_filler(k):
    return [[30 + 2 * k], [], [31 + 2 * k], []]


@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("keep_empty", [False, True])
def test_rows_that_keep_nothing_are_one_class(device, monkeypatch, keep_empty, hook):
    """Empty rows, rows of dropped ids only (a whole chunk of them), ids dropped on their side: one class, the empty value
    in every entry; a row that keeps one id among them is another."""
    nothing = [[[], [], [], []], [rr.DROPPED[:5], [], rr.DROPPED[5:9], []], [[100, 104], [], [105], [109]],
               [rr.DROPPED[:70], [], [], rr.DROPPED[70:]]]
    lists = [nothing[k % 4] for k in range(20)]
    case = gene_case(f"nothing kept {keep_empty}", lists, n_allele=5, keep_empty=keep_empty)
    assert not case.ref.nvar.any() and (case.ref.probs == (cr.HIT if keep_empty else 1.0)).all()
    check_tables(device, monkeypatch, case, hook, n_classes=1)
    lists = lists[:7] + [[[A], [], [], []]] + lists[7:]
    check_tables(device, monkeypatch, gene_case(f"nothing kept but one {keep_empty}", lists, n_allele=5, keep_empty=keep_empty),
                 hook, n_classes=2)


# ------------------------------------------------------------------------------------------------- long rows
def long_row(n, swap=None, n_pos=None):
    ids = (rr.KEEPABLE * 2)[:n]
    if swap is not None:
        ids[swap], ids[swap + 1] = ids[swap + 1], ids[swap]
    n_pos = (2 * n) // 5 if n_pos is None else n_pos
    return [ids[:n_pos // 2], ids[n_pos // 2:n_pos], ids[n_pos:n - 3], ids[n - 3:]]


@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("n_ids", [65, 128, 256, 257, 300])
def test_long_rows(device, monkeypatch, n_ids, hook):
    """Rows of 65, 128 and 300 kept ids (two, two and five rounds of the walk), equal ones, ones that differ in their last
    two ids only, in their first two, in the place of the positive / negative boundary, and the same with dropped ids
    spread over them; 256 and 257: the most a comparison holds and one more (such rows stay apart, their entries are the
    reference's all the same)."""
    base = long_row(n_ids)
    spread = copy.deepcopy(base)
    for q, lst in enumerate(spread):
        for t in range(0, len(lst), 7):
            lst.insert(t, rr.DROPPED[(t + q) % len(rr.DROPPED)])
    lists = [base, long_row(n_ids, swap=n_ids - 2), spread, long_row(n_ids, swap=0), base,
             long_row(n_ids, n_pos=(2 * n_ids) // 5 + 1), [[A], [], [], []], spread]
    case = gene_case(f"long {n_ids}", lists, n_allele=3)
    cls = rr.classOf(case.off, case.ids, case.rows, case.vflag)
    assert cls.tolist() == [0, 1, 0, 2, 0, 3, 4, 0] and case.ref.nvar[0] == n_ids
    check_tables(device, monkeypatch, case, hook, classes="exact" if n_ids <= KEPT_CAP else "inside")


# ------------------------------------------------------------------------------------------------- alleles and columns
def mixed_lists(n=40):
    return [rr.TEMPLATES[i % 3] if i % 4 else rr.distinctRow(100 + i) for i in range(n)]


@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("n_allele", [40, 100, 150, 250, 300])
def test_allele_slots_and_a_second_pass(device, monkeypatch, n_allele, hook):
    """One to four allele slots per lane, and 300 alleles: a second pass of the kernel over the same representatives."""
    check_tables(device, monkeypatch, gene_case(f"mixed, {n_allele} alleles", mixed_lists(), n_allele=n_allele), hook,
                 expect="patch")


@pytest.mark.parametrize("hook", list(HOOKS))
@pytest.mark.parametrize("n_cols", [9, 70])
def test_column_lists(device, monkeypatch, n_cols, hook):
    """``gk_compat_log_miss_cols``: 9 and 70 of 100 alleles, both ends and the neighbours of 31 / 32 and 63 / 64 among them."""
    first = [0, 99, 31, 32, 63, 64, 30, 33, 65]
    cols = sorted(list(dict.fromkeys(first + list(range(1, 99, 1))))[:n_cols])
    assert len(cols) == n_cols
    check_tables(device, monkeypatch, gene_case("mixed, 100 alleles", mixed_lists(), n_allele=100), hook, cols=cols,
                 expect="patch")


# ------------------------------------------------------------------------------------------------- numeric edges
@pytest.mark.parametrize("hook", list(HOOKS))
def test_classes_of_rows_that_underflow(device, monkeypatch, hook):
    """The long rows of the hand-built underflow gene, each of them three times: counts of 100 and more (byte 255 and bit 0
    in every member's entry), subnormal products, the +0.0 product met before its log10 is known (bit 3: the table is
    written again, through the classes again)."""
    one = ce.numericCase(cr.HEAVY_GENE)
    n = one.n_csr
    off0, total = one.off.astype(np.int64), int(one.off[-1])
    off = np.concatenate([off0, off0[1:] + total, off0[1:] + 2 * total]).astype(np.uint32)
    key = "numeric x 3"
    if key not in _cases:
        _cases[key] = ce.Case(key, off, np.tile(one.ids, 3), one.n_var_total, np.arange(3 * n), one.vflag, one.vbeg, one.vend,
                              one.bits)
    case = _cases[key]
    assert case.ref.flag0 and (case.ref.probs == 0).any()
    assert np.array_equal(case.ref.miss[:n], case.ref.miss[n:2 * n])
    assert case.ref.nvar.max() > KEPT_CAP > case.ref.nvar.min()      # the long rows stay apart, the short ones merge
    check_tables(device, monkeypatch, case, hook, expect="again", classes="inside")
    # a class of three members that mismatches most alleles more than 100 times: 120 ids that one allele in ten carries
    odd = [v for v in rr.KEEPABLE if (v - rr.VBEG) % 2]
    heavy = (odd * 2)[:120]
    spread = list(heavy)
    for t in range(0, 120, 9):
        spread.insert(t, rr.DROPPED[t % len(rr.DROPPED)])
    lists = [[heavy[:50], heavy[50:], [], [A]], [[A], [], [B], []], [heavy[:70], heavy[70:], [A], []], [[B], [], [], []],
             [spread[:30], spread[30:], [], [A]]]
    case = gene_case("heavy class", lists, n_allele=40)
    assert rr.classOf(case.off, case.ids, case.rows, case.vflag).tolist() == [0, 1, 0, 2, 0]
    assert case.ref.flag0 and (case.ref.miss8[0] == 255).any() and (case.ref.miss8[0] < 100).any()
    check_tables(device, monkeypatch, case, hook)


# ------------------------------------------------------------------------------------------------- scratch reused
@pytest.mark.parametrize("hook", list(HOOKS))
def test_two_calls_back_to_back_on_one_stream(device, monkeypatch, hook):
    """Three tables queued without a wait between them -- 129 rows in three classes, 33 distinct rows, the first again --
    so that the slots, the compact tables and the class arrays of a call are the blocks the call before has just given
    back."""
    monkeypatch.setenv("GK_TEST_HOOKS", HOOKS[hook])
    cases = [gene_case("three x 129", rr.patternLists("three", 129)[0], keep_empty=True),
             gene_case("distinct x 33", rr.patternLists("distinct", 33)[0], keep_empty=True)]
    gpus = [ce.OnDevice(device, c) for c in cases]
    logs = LogTable(device, log2_capacity=16)
    try:
        for g in gpus:                                    # the value table learns every product first
            ce.settle_log_miss(g, logs)
        out = []
        for g in (gpus[0], gpus[1], gpus[0]):
            L = g.filled((g.case.n_allele, g.n_rows), np.float64)
            miss8 = g.filled((g.case.n_allele, g.ldm), np.uint8)
            flags = g.filled(1, np.uint32)
            check(lib().gk_compat_log_miss(*g.args(), logs.handle, L.ptr, miss8.ptr, g.ldm, flags.ptr))
            out.append((g, L, miss8, flags))
        device.sync()
        for g, L, miss8, flags in out:
            ce.assert_log_table(g, (L.download(), miss8.download(), int(flags.download()[0])))
            for b in (L, miss8, flags):
                b.free()
    finally:
        logs.close()
        for g in gpus:
            g.close()


# ------------------------------------------------------------------------------------------------- the drivers
@pytest.fixture(scope="module")
def typed_sample():
    """A small sample (3 genes, 2000 pairs), its tabulation lines' oracle and the oracle's exon-first typing."""
    from kir_graph_amd import synth
    from kir_graph_amd.index import GkIndex
    from oracle import tabulate as ot, typing as oty
    sidx = synth.makeIndex(seed=2022, n_genes=3, var_range=(200, 300), allele_range=(12, 24))
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    sample = synth.makeSample(sidx, seed=1031, n_pairs=2000)
    ref = ot.tabulateLines(synth.toSamLines(sample), gidx.variants)
    cpu = oty.makeTyper("exonfirst_1", copy.deepcopy(ref), top_n=600, variant_correction=True)
    calls = cpu.typing(sample.gene_cn)
    return gidx, sample, cpu, calls


@pytest.mark.parametrize("hook", ["off", "on", "on, 4 hash bits"])
def test_exon_first_through_the_drivers(device, monkeypatch, typed_sample, hook):
    """Exon-first typing of a small sample with every table through the row classes and with none: the oracle's calls and
    every field of every copy-number step."""
    from kir_graph_amd import packed
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.kir_typing import selectKirTypingModel
    monkeypatch.setenv("GK_TEST_HOOKS", HOOKS[hook])
    gidx, sample, cpu, want_calls = typed_sample
    rec, table = packed.packSample(sample, gidx)
    dindex = DeviceIndex(device, gidx)
    tab = Tabulation(dindex, rec)
    try:
        data = SampleData(tab, gidx, None, ins_strings=table.strings)
        gpu = selectKirTypingModel("exonfirst_1", data, top_n=600, variant_correction=True)
        assert gpu.typing(sample.gene_cn) == want_calls
        for gene, steps in cpu.results.items():
            assert len(gpu._result[gene]) == len(steps), gene
            for a, b in zip(gpu._result[gene], steps):
                ce.same_step(a, b)
    finally:
        tab.close()
        dindex.close()
