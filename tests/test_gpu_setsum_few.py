"""The sums of a few allele sets by chunk-owning workgroups (csrc/gk_setsum_few.hip: ``setsum_few``) -- ``gk_setsum_few``
straight through the C ABI at the row counts where the summation tree changes shape, with NaN rows behind every column, on
sets that repeat an allele, on a wide table, back to back with the leaf form (one ticket block), and its argument checks;
then the routing of the search (``gk_sample_search``: at most 8 sets, tables of at most 8 columns) against the forms of
gk_search.hip on one library.  Every comparison is bit for bit with numpy's own expressions
(tests/searchtree_reference.py).

What the tests catch (scratch builds, this file on the GPU; see CHANGELOG.md): the ``n2 -= n2 % 8`` rounding removed, the
tail rows of a leaf skipped, the chunk sums added in reverse order."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import searchtree_reference as sr  # noqa: E402

from kir_graph_amd._lib import check, lib  # noqa: E402

pytestmark = pytest.mark.gpu

GK_ERR_ARG = -3
FIELDS = ("value", "value_sum_indv", "allele_id", "fraction")


class Table:
    """A table in HBM, column-major with ``pad`` NaN rows behind every column."""

    def __init__(self, device, L, pad=0):
        self.device, self.L = device, L
        self.n_rows, self.n_allele = L.shape
        self.ld = self.n_rows + pad
        self.buf = device.put(sr.padded(L, pad))

    def free(self):
        self.buf.free()

    def _call(self, fn, ids, n_rows):
        n_rows = n_rows or self.n_rows
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        value, frac = np.full(len(ids), np.nan), np.full(ids.shape, np.nan)
        check(fn(self.device.ctx, self.buf.ptr, n_rows, self.ld, ids.ctypes.data, ids.shape[0], ids.shape[1],
                 value.ctypes.data, frac.ctypes.data))
        return value, frac

    def few(self, ids, n_rows=None):
        return self._call(lib().gk_setsum_few, ids, n_rows)

    def setsum(self, ids, n_rows=None):
        return self._call(lib().gk_setsum, ids, n_rows)


def launches(device, call):
    """What ``call`` returns, and {kernel: launches} of the kernels it ran."""
    device.profEnable(True)
    device.profCollect()
    try:
        got = call()
        ran = {k: v[0] for k, v in device.profCollect().items() if v[0] > 0}
    finally:
        device.profEnable(False)
    return got, ran


def check_few(T, ids, n_rows=None):
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    L = T.L[:n_rows or T.n_rows]
    value, frac = T.few(ids, n_rows)
    assert np.array_equal(value, sr.setvalue_numpy(L, ids)), (L.shape, ids.shape)
    assert np.array_equal(frac, sr.shares_numpy(L, ids) / len(L)), (L.shape, ids.shape)
    if ids.shape[1] == 1:
        assert np.array_equal(value, sr.colsum_numpy(L, ids[:, 0]))
    return value, frac


def every_form(device, L, pad):
    T = Table(device, L, pad)
    try:
        for c in (1, 2, 3, 4):
            ids = sr.sweep_sets(len(L), c, n_sets=8)
            for n_sets in (1, 2, 8):
                check_few(T, np.concatenate([ids[:n_sets - 1], ids[-1:]]))       # the last set names the last column
    finally:
        T.free()


@pytest.mark.parametrize("kind", sr.TABLES)
@pytest.mark.parametrize("n_rows", sr.SWEEP)
def test_row_sweep(device, n_rows, kind):
    """All-tail leaves, the ``len & 7`` tail, one leaf, 8191 / 8192 / 8193, a second chunk of 1 .. 129 rows, three chunks."""
    every_form(device, sr.make_table(kind, n_rows), 0)


@pytest.mark.parametrize("kind", sr.TABLES)
@pytest.mark.parametrize("pad", [3, 61])
@pytest.mark.parametrize("n_rows", sr.PADDED_SWEEP)
def test_rows_behind_a_column_are_never_read(device, n_rows, pad, kind):
    """ld = n_rows + pad with NaN in the padding: one row too far in a max or a sum makes an output NaN."""
    every_form(device, sr.make_table(kind, n_rows), pad)


@pytest.mark.parametrize("kind", sr.TABLES)
@pytest.mark.parametrize("n_rows", [137, 1033, 8199])
def test_sets_that_repeat_an_allele(device, n_rows, kind):
    """[a, a] (every row a tie of the set with itself), [a, a, b], four times one allele, and two identical columns."""
    L = sr.make_table(kind, n_rows)
    L[:, 11] = L[:, 4]                                   # two alleles nothing tells apart
    a = np.arange(8, dtype=np.int32)
    T = Table(device, L, pad=3)
    try:
        single, _ = check_few(T, a[:, None])
        value, frac = check_few(T, np.stack([a, a], axis=1))
        assert np.array_equal(frac, np.full((8, 2), 0.5)) and np.array_equal(value, single)
        value, frac = check_few(T, np.array([[4, 11], [11, 4], [4, 4]]))
        assert np.array_equal(frac, np.full((3, 2), 0.5)) and value[0] == value[1] == value[2]
        check_few(T, np.stack([a, a, np.roll(a, 3)], axis=1))
        check_few(T, np.stack([a, np.roll(a, 3), a], axis=1))
        check_few(T, np.array([[4, 11, 4], [11, 4, 2]]))
        check_few(T, np.array([[4, 11, 11, 4], [2, 4, 11, 2]]))
        value, frac = check_few(T, np.repeat(a[:, None], 4, axis=1))
        assert np.array_equal(frac, np.full((8, 4), 0.25)) and np.array_equal(value, single)
    finally:
        T.free()


@pytest.mark.parametrize("pad", [0, 5])
def test_only_the_named_columns_of_a_wide_table_are_read(device, pad):
    """Sets that name columns 0, 199 and 255 of a 256-column table: every other column is NaN, so a kernel that reads a
    column nobody named (or takes the last column's offset with n_rows for ld) returns NaN or another column's sum."""
    n_rows = 8321
    rng = np.random.default_rng(256)
    L = np.full((n_rows, 256), np.nan)
    L[:, [0, 199, 255]] = sr.wide(rng, n_rows, 3)
    T = Table(device, L, pad)
    try:
        check_few(T, np.array([[255], [0], [199]]))
        check_few(T, np.array([[0, 255], [255, 199]]))
        check_few(T, np.array([[199, 0, 255]]))
        check_few(T, np.array([[255, 0, 199, 255], [0, 0, 255, 255]]))
    finally:
        T.free()


def test_tickets_are_handed_back(device, monkeypatch):
    """Calls back to back on one context at different row counts, the leaf form (the same ticket block) in between, then the
    first again: a ticket that was not put back to zero leaves the next call without its last workgroup."""
    monkeypatch.setenv("GK_TEST_HOOKS", "setsum=leaves")          # gk_setsum below: setsum_leaves + fold_leaves
    L = sr.make_table("wide", 24577)
    T = Table(device, L)
    ids = sr.sweep_sets(24577, 3, n_sets=8)
    try:
        for n_rows, n_sets in ((24577, 8), (8193, 2), (24577, 8), (8192, 1), (7, 8)):
            check_few(T, ids[:n_sets], n_rows)
            (value, frac), ran = launches(device, lambda: T.setsum(ids, n_rows))
            assert ran.get("setsum_leaves") == 1 and ran.get("fold_leaves") == 1 and "setsum_few" not in ran
            assert np.array_equal(value, sr.setvalue_numpy(L[:n_rows], ids))
            assert np.array_equal(frac, sr.shares_numpy(L[:n_rows], ids) / n_rows)
            check_few(T, ids[:, :2], n_rows)
        _, ran = launches(device, lambda: T.few(ids))
        assert ran == {"setsum_few": 1}
    finally:
        T.free()


def test_refusals(device):
    """c = 0 or 5, a negative id, ld < n_rows: GK_ERR_ARG and no launch."""
    L = sr.make_table("ties", 137)
    T = Table(device, L)
    value, frac = np.full(4, np.nan), np.full(32, np.nan)

    def call(ids, c, n_rows=137, ld=137):
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        return lib().gk_setsum_few(device.ctx, T.buf.ptr, n_rows, ld, ids.ctypes.data, 2, c, value.ctypes.data,
                                   frac.ctypes.data)
    try:
        def refused():
            assert call(np.zeros(16), 0) == GK_ERR_ARG
            assert call(np.zeros(16), 5) == GK_ERR_ARG
            assert call([1, 2, -1, 3], 2) == GK_ERR_ARG
            assert call([1, 2, 3, 4], 2, ld=136) == GK_ERR_ARG
            assert call([1, 2, 3, 4], 2, n_rows=0) == GK_ERR_ARG
        _, ran = launches(device, refused)
        assert ran == {} and np.isnan(value).all() and np.isnan(frac).all()
        assert call([1, 2, 3, 4], 2) == 0                     # the context serves the corrected call
        assert np.array_equal(value[:2], sr.setvalue_numpy(L, np.array([[1, 2], [3, 4]])))
    finally:
        T.free()


# ---------------------------------------------------------------------------------------------------------------------
# routing

@pytest.fixture(scope="module")
def one_gene(device):
    """run(searches) = the steps of candidate searches that offer ONE allele per step (exon groups of one member: the
    one-set searches of exon-first) on the table of a gene of at most 8 alleles, through ``gk_sample_search``; the fixture
    style of tests/test_gpu_exonfirst_columns.py."""
    from kir_graph_amd import _lib, packed, synth
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.index import GkIndex
    from kir_graph_amd.kir_typing import _GeneView
    from kir_graph_amd.typing_mulit_allele import sharedLogTable
    sidx = synth.makeIndex(seed=7130001, n_genes=1, var_range=(80, 120), allele_range=(6, 7), len_range=(2500, 3000))
    gene = sidx.genes[0]
    sample = synth.makeSample(sidx, seed=7130002, n_pairs=600, gene_cn={gene: 2}, err_rate=0.0, frac_multi=0.0)
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    rec, table, _, counts = packed.packText([("\n".join(synth.toSamLines(sample)) + "\n").encode()], gidx)
    tab = Tabulation(DeviceIndex(device, gidx), device.put(rec), spill=counts.get("spill"))
    data = SampleData(tab, gidx, None, ins_strings=table.strings)
    logs = sharedLogTable(device)
    prep = tab.prepared(device, False)
    assert prep is not None
    view = _GeneView(data, gene, False, tab=tab)
    assert 6 <= len(view.alleles) <= 8
    prepared = view.prepared(prep)

    def run(searches):
        full = view.model(logs, prepared, force_homo=False, top_n=10, variant_correction=True, _defer_launch=True)
        job, _ = full.geneJob(2, False)
        job.n_steps = 0
        keep, cands = [], []
        for offered in searches:
            cols = np.array(offered, dtype=np.int32)
            offs = np.arange(len(offered) + 1, dtype=np.int32)
            keep += [cols, offs]
            cands.append(_lib.GeneJob(d_rows=job.d_rows, n_rows=job.n_rows, d_mask=job.d_mask, ldm=job.ldm, vbeg=job.vbeg,
                                      vend=job.vend, words=job.words, n_allele=job.n_allele, n_steps=len(offered), top_n=10,
                                      table_of=0, n_step_cols=len(offered), step_cols=cols.ctypes.data,
                                      step_cols_off=offs.ctypes.data))
        n = 1 + len(cands)
        jobs = (_lib.GeneJob * n)(job, *cands)
        handles = (C.c_void_p * n)()
        try:
            check(lib().gk_sample_search(device.ctx, None, 0, tab.handle, prep.vflag.ptr, logs.handle, jobs, n,
                                         _lib.NUMPY_ARGSORT, _lib.NUMPY_LOG10, handles))
            full.adoptTable(jobs[0], C.c_void_p(handles[0]))
            steps = full.adoptSearches(list(handles[1:]))
            return [{f: np.array(getattr(s, f)) for f in FIELDS} for s in steps]
        finally:
            for h in handles:
                if h:
                    lib().gk_search_destroy(C.c_void_p(h))

    yield run
    tab.close()


SEARCHES = [[1, 3, 4], [0, 2, 5], [5, 5, 1], [2, 4, 4], [3, 0, 0], [4, 1, 2], [0, 0, 0], [5, 3, 2], [1, 1, 4]]


def same_steps(got, want):
    assert len(got) == len(want)
    for x, y in zip(got, want):
        for f in FIELDS:
            assert np.array_equal(x[f], y[f]), f


def test_the_search_takes_the_form_for_at_most_8_sets(device, one_gene, monkeypatch):
    """8 one-set searches on a table of at most 8 columns: the column sums and the calls of k = 2 and 3 run setsum_few and
    nothing of gk_search.hip; under the hooks they run the forms of gk_search.hip and give the same steps."""
    monkeypatch.delenv("GK_TEST_HOOKS", raising=False)
    got, ran = launches(device, lambda: one_gene(SEARCHES[:8]))
    assert ran.get("setsum_few", 0) >= 3, ran             # the column sums (again after a patch of the table), k = 2, k = 3
    assert not {"setsum_leaves", "fold_leaves", "fraction_chunks", "colsum_chunks", "combine_chunks"} & set(ran), ran
    assert len(got) == 8 * 3
    monkeypatch.setenv("GK_TEST_HOOKS", "setsum=leaves")
    want, ran = launches(device, lambda: one_gene(SEARCHES[:8]))
    assert "setsum_few" not in ran and ran.get("setsum_leaves") == 2 and ran.get("colsum_chunks", 0) >= 1, ran
    same_steps(got, want)
    monkeypatch.setenv("GK_TEST_HOOKS", "setsum=tiles")
    want, ran = launches(device, lambda: one_gene(SEARCHES[:8]))
    assert "setsum_few" not in ran and ran.get("fraction_chunks") == 2, ran
    same_steps(got, want)


def test_a_call_of_9_sets_keeps_the_leaf_form(device, one_gene, monkeypatch):
    monkeypatch.delenv("GK_TEST_HOOKS", raising=False)
    got, ran = launches(device, lambda: one_gene(SEARCHES))
    assert ran.get("setsum_leaves") == 2 and ran.get("setsum_few", 0) >= 1, ran       # the column sums alone
    monkeypatch.setenv("GK_TEST_HOOKS", "setsum=leaves")
    want, ran = launches(device, lambda: one_gene(SEARCHES))
    assert "setsum_few" not in ran, ran
    same_steps(got, want)


def test_an_exon_first_sample_types_the_same_in_both_forms(device, monkeypatch):
    """A small sample of genes with at most 8 alleles, typed exon-first with no hook and with setsum=leaves: calls, warnings
    and every step equal; setsum_few among the kernels of the first run only."""
    from kir_graph_amd import packed, synth
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.index import GkIndex
    from kir_graph_amd.kir_typing import selectKirTypingModel
    monkeypatch.setenv("GK_SEARCH", "bound")
    sidx = synth.makeIndex(seed=7180001, n_genes=3, var_range=(80, 160), allele_range=(5, 9), len_range=(2500, 4000))
    gene_cn = {g: cn for g, cn in zip(sidx.genes, (2, 3, 1))}
    sample = synth.makeSample(sidx, seed=7180002, n_pairs=1500, gene_cn=gene_cn, err_rate=0.001, frac_multi=0.05)
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    rec, table, _, counts = packed.packText([("\n".join(synth.toSamLines(sample)) + "\n").encode()], gidx)
    tab = Tabulation(DeviceIndex(device, gidx), device.put(rec), spill=counts.get("spill"))
    data = SampleData(tab, gidx, None, ins_strings=table.strings)

    def typed():
        typer = selectKirTypingModel("exonfirst_1", data, top_n=60, variant_correction=True)
        calls, warnings = typer.typing(gene_cn)
        steps = [{f: np.array(getattr(s, f)) for f in FIELDS} for g in gene_cn for s in (typer._result.get(g) or [])]
        return list(calls), list(warnings), steps

    def launches_everywhere(call):
        """``launches`` over every context of the process: a typer drives worker contexts of its own."""
        from kir_graph_amd import _lib
        devs = [d for d in _lib.Device.instances if d.ctx]
        for d in devs:
            d.profEnable(True)
            d.profCollect()
        try:
            got, ran = call(), {}
            for d in devs:
                for k, v in d.profCollect().items():
                    if v[0] > 0:
                        ran[k] = ran.get(k, 0) + v[0]
        finally:
            for d in devs:
                d.profEnable(False)
        return got, ran
    try:
        monkeypatch.delenv("GK_TEST_HOOKS", raising=False)
        typed()                                               # the contexts the typer makes exist from here on
        got, ran = launches_everywhere(typed)
        assert ran.get("setsum_few", 0) > 0, ran
        monkeypatch.setenv("GK_TEST_HOOKS", "setsum=leaves")
        want, ran = launches_everywhere(typed)
        assert "setsum_few" not in ran and ran.get("colsum_chunks", 0) > 0, ran
        assert got[:2] == want[:2] and len(got[2]) > 0
        same_steps(got[2], want[2])
    finally:
        tab.close()
