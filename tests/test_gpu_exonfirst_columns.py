"""Exon-first writes the full-model table of a gene for the CANDIDATE alleles only (``gk_gene_job.table_cols``); the
searches on it must not notice.  Every case is typed twice, each time in a fresh child process: once as shipped and once
under ``GK_TEST_HOOKS=full_tables`` (the table of every allele, the form before the column lists).  Every step of every
candidate search and the merged result are compared bit for bit (value, sum_indv, allele_id, fraction), with the calls
and the warnings; ``log_probs`` read from a restricted model must equal the all-allele table.

The cases are small random indices whose alleles share exon variant sets (``synth.makeIndex``: the exon blocks cover a
fifth of a backbone, so many alleles differ in introns only), ``exonfirst_1`` and ``exonfirst_0.9``, copy numbers 1-4.
SEEDS were fixed after running the CPU oracle over them (``python tests/test_gpu_exonfirst_columns.py scan``): at most a
quarter of the genes fall to the fall-back (no exon set) there, and the set holds genes whose candidates are one allele,
a few alleles and every allele.  The test counts what the product did and fails when more than a quarter of the genes
left the whole-sample path, or when one of the named shapes did not occur.  No seed gave a union of more than 256
alleles that is not every allele (the wide cases end with a handful of candidates or with all of them), so that shape --
a column list that needs two passes of the compatibility kernel -- is driven through the C-ABI instead.

The C-ABI cases: a candidate search that names an allele outside its table's column list is GK_ERR_ARG, and the context
serves the corrected call right after; a list of ~300 of 330 alleles gives the search results of the whole table."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METHODS = ("exonfirst_1", "exonfirst_0.9")
FIELDS = ("value", "value_sum_indv", "allele_id", "fraction")
# (seed, wide gene)
SEEDS = tuple((s, False) for s in range(7110001, 7110009)) + ((7120001, True), (7120002, True))


def makeCase(seed: int, wide: bool):
    from kir_graph_amd import synth
    rng = np.random.default_rng(seed)
    n_genes = 1 if wide else 3
    a_lo = int(rng.choice([290, 330])) if wide else int(rng.choice([12, 40, 70]))
    sidx = synth.makeIndex(seed=seed, n_genes=n_genes, var_range=(60, 400), allele_range=(a_lo, a_lo + int(rng.integers(1, 30))),
                           len_range=(2500, 6000), frac_del=0.09, frac_ins=0.03)
    gene_cn = {g: int(rng.integers(1, 5)) for g in sidx.genes}
    sample = synth.makeSample(sidx, seed=seed + 1, n_pairs=2500 if wide else int(rng.choice([1500, 4000])), gene_cn=gene_cn,
                              err_rate=float(rng.choice([0.0, 0.001])), frac_multi=0.05)
    top_n = int(rng.choice([60, 600]))
    return sidx, gene_cn, synth.toSamLines(sample), top_n


def typeCases(out_path: str) -> None:
    """Child process: every case with both thresholds -> one .npz (arrays) with a JSON record of the rest."""
    sys.path.insert(0, ROOT)
    from kir_graph_amd import _lib, packed
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.index import GkIndex
    from kir_graph_amd.kir_typing import selectKirTypingModel
    from kir_graph_amd.typing_mulit_allele import StepList
    os.environ["GK_SEARCH"] = "bound"
    dev = _lib.Device(0)
    arrays, record = {}, []
    for seed, wide in SEEDS:
        sidx, gene_cn, lines, top_n = makeCase(seed, wide)
        gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
        rec, table, _, counts = packed.packText([("\n".join(lines) + "\n").encode()], gidx)
        tab = Tabulation(DeviceIndex(dev, gidx), dev.put(rec), spill=counts.get("spill"))
        data = SampleData(tab, gidx, None, ins_strings=table.strings)
        for method in METHODS:
            typer = selectKirTypingModel(method, data, top_n=top_n, variant_correction=True)
            calls, warnings = typer.typing(gene_cn)
            genes = {}
            for gene, cn in gene_cn.items():
                result = typer._result.get(gene)
                info = dict(getattr(typer, "exon_info", {}).get(gene, {}))
                whole = isinstance(result, StepList)      # tables and searches ran in the whole-sample calls
                info["whole_sample"] = whole
                info["alleles"] = len(gidx.tables[gidx.gene_id[gene]].alleles)
                info["steps"] = len(result) if result else 0
                for k, step in enumerate(result or []):
                    for f in FIELDS:
                        arrays[f"{seed}/{method}/{gene}/{k}/{f}"] = np.asarray(getattr(step, f))
                if whole:
                    model = result._steps._typing
                    info["restricted"] = model._model._table_cols is not None
                    arrays[f"{seed}/{method}/{gene}/log_probs"] = model.log_probs
                genes[gene] = info
            record.append({"seed": seed, "method": method, "calls": list(calls), "warnings": list(warnings), "genes": genes})
        tab.close()
    np.savez(out_path, record=np.array(json.dumps(record)), **arrays)


def _child(tmp_path, name: str, hooks: str | None):
    out = str(tmp_path / f"{name}.npz")
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("GK_TEST_HOOKS", None)
    if hooks:
        env["GK_TEST_HOOKS"] = hooks
    done = subprocess.run([sys.executable, os.path.abspath(__file__), "type", out], env=env, capture_output=True, text=True,
                          timeout=900)
    assert done.returncode == 0, done.stderr[-3000:]
    got = np.load(out)
    return json.loads(str(got["record"])), got


def test_candidate_columns_give_the_results_of_the_whole_table(device, tmp_path):
    rec_r, arr_r = _child(tmp_path, "restricted", None)
    rec_f, arr_f = _child(tmp_path, "full", "full_tables")
    assert len(rec_r) == len(rec_f) == len(SEEDS) * len(METHODS)
    n_genes = n_elsewhere = n_restricted = n_single = n_every = n_few = 0
    for r, f in zip(rec_r, rec_f):
        where = (r["seed"], r["method"])
        assert (r["calls"], r["warnings"]) == (f["calls"], f["warnings"]), where
        for gene, info in r["genes"].items():
            other = f["genes"][gene]
            n_genes += 1
            assert info["steps"] == other["steps"] and info["whole_sample"] == other["whole_sample"], (where, gene)
            if not info["whole_sample"]:
                n_elsewhere += 1
                continue
            assert not other["restricted"], (where, gene)
            assert info["table_columns"] <= info["alleles"] and other["table_columns"] == info["alleles"], (where, gene)
            assert info["restricted"] == (info["table_columns"] < info["alleles"]), (where, gene)
            n_restricted += info["restricted"]
            n_single += info["table_columns"] == 1
            n_every += info["table_columns"] == info["alleles"]
            n_few += info["restricted"] and info["table_columns"] > 1
    keys = sorted(k for k in arr_r.files if k != "record")
    assert keys == sorted(k for k in arr_f.files if k != "record")
    for k in keys:
        a, b = arr_r[k], arr_f[k]
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True), k
    print(f"[exon-first columns] genes {n_genes}: restricted {n_restricted} (one column {n_single}, several columns "
          f"{n_few}), every allele a candidate {n_every}, per-gene path or fall-back {n_elsewhere}")
    assert 4 * n_elsewhere <= n_genes, (n_elsewhere, n_genes)
    assert n_restricted > 0 and n_single > 0 and n_every > 0 and n_few > 0, (n_restricted, n_single, n_every, n_few)


def _tableAndSearch(device, seed: int, allele_range, n_pairs: int):
    """(run, n_allele, close): run(table_cols, offered) = the steps of a two-copy candidate search that offers ``offered`` on a
    table job over ``table_cols`` (None: every allele) of a one-gene index, through ``gk_sample_search``."""
    import ctypes as C
    from kir_graph_amd import _lib, packed
    from kir_graph_amd._lib import GkError, check, lib
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.index import GkIndex
    from kir_graph_amd.kir_typing import _GeneView
    from kir_graph_amd.typing_mulit_allele import sharedLogTable
    from kir_graph_amd import synth
    sidx = synth.makeIndex(seed=seed, n_genes=1, var_range=(80, 120), allele_range=allele_range, len_range=(2500, 3000))
    gene = sidx.genes[0]
    sample = synth.makeSample(sidx, seed=seed + 1, n_pairs=n_pairs, gene_cn={gene: 2}, err_rate=0.0, frac_multi=0.0)
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    lines = synth.toSamLines(sample)
    rec, table, _, counts = packed.packText([("\n".join(lines) + "\n").encode()], gidx)
    tab = Tabulation(DeviceIndex(device, gidx), device.put(rec), spill=counts.get("spill"))
    data = SampleData(tab, gidx, None, ins_strings=table.strings)
    logs = sharedLogTable(device)
    prep = tab.prepared(device, False)
    assert prep is not None
    vflag = prep.vflag
    view = _GeneView(data, gene, False, tab=tab)
    n_allele = len(view.alleles)
    prepared = view.prepared(prep)

    def run(table_cols, offered):
        full = view.model(logs, prepared, force_homo=False, top_n=10, variant_correction=True, _defer_launch=True,
                          _table_cols=table_cols)
        job, _ = full.geneJob(2, False)
        job.n_steps = 0
        cols = np.array(offered, dtype=np.int32)
        offs = np.array([0, len(offered)], dtype=np.int32)
        cand = _lib.GeneJob(d_rows=job.d_rows, n_rows=job.n_rows, d_mask=job.d_mask, ldm=job.ldm, vbeg=job.vbeg, vend=job.vend,
                            words=job.words, n_allele=job.n_allele, n_steps=2, top_n=10, table_of=0, n_step_cols=1,
                            step_cols=cols.ctypes.data, step_cols_off=offs.ctypes.data)
        jobs = (_lib.GeneJob * 2)(job, cand)
        handles = (C.c_void_p * 2)()
        try:
            check(lib().gk_sample_search(device.ctx, None, 0, tab.handle, vflag.ptr, logs.handle, jobs, 2, _lib.NUMPY_ARGSORT,
                                         _lib.NUMPY_LOG10, handles))
            full.adoptTable(jobs[0], C.c_void_p(handles[0]))
            steps = full.adoptSearches([handles[1]])
            return [{f: np.array(getattr(s, f)) for f in FIELDS} for s in steps]
        finally:
            for h in handles:
                if h:
                    lib().gk_search_destroy(C.c_void_p(h))

    return run, n_allele, tab.close


def test_a_step_column_outside_the_table_columns_is_an_argument_error(device):
    """Through the C-ABI: a table job over columns {1, 3, 4} of a six-allele gene and a candidate search that offers
    allele 2 -> GK_ERR_ARG with a message; the same call with allele 3 then runs on the same context, and its result is
    the one the all-allele table gives."""
    from kir_graph_amd._lib import GkError
    run, n_allele, close = _tableAndSearch(device, 7130001, (6, 7), 600)
    assert n_allele >= 5
    listed = np.array([1, 3, 4], dtype=np.int32)
    with pytest.raises(GkError, match="not among the columns"):
        run(listed, [1, 2, 4])
    got = run(listed, [1, 3, 4])
    want = run(None, [1, 3, 4])
    assert len(got) == len(want) == 2
    for x, y in zip(got, want):
        for f in FIELDS:
            assert np.array_equal(x[f], y[f]), f
    assert set(np.unique(got[-1]["allele_id"])) <= {1, 3, 4}
    close()


def test_a_list_of_more_than_256_columns(device):
    """A column list that takes two passes of the compatibility kernel (256 alleles per pass): nine alleles in ten of a
    330-allele gene, all of them offered."""
    run, n_allele, close = _tableAndSearch(device, 7140001, (330, 331), 2500)
    listed = np.array([a for a in range(n_allele) if a % 10 != 3], dtype=np.int32)
    assert 256 < len(listed) < n_allele
    got = run(listed, listed.tolist())
    want = run(None, listed.tolist())
    assert len(got) == len(want) == 2
    for x, y in zip(got, want):
        for f in FIELDS:
            assert np.array_equal(x[f], y[f]), f
    close()


def scan() -> None:
    """CPU only: what the oracle's exon-first does with every case of SEEDS (the shapes the docstring names)."""
    sys.path.insert(0, ROOT)
    import copy
    from oracle import tabulate as ot, typing as oty
    seen = []
    Base = oty.ExonFirstModel

    class Watch(Base):
        def typing(self, cn):
            res = oty.GeneModel.typing(self, cn)
            n_allele = sum(len(m) for m in self.allele_group.values())
            ranks = oty.topRank(res, self.candidate_set_threshold) if res.value.shape[0] else []
            union = {a for i in ranks for g in res.allele_name[i] for a in self.allele_group[g]}
            seen.append({"fallback": not res.value.shape[0], "candidates": len(ranks), "union": len(union), "alleles": n_allele})
            self.result = []
            return Base.typing(self, cn)

    oty.ExonFirstModel = Watch
    for seed, wide in SEEDS:
        sidx, gene_cn, lines, top_n = makeCase(seed, wide)
        ref = ot.tabulateLines(lines, sidx.variants)
        for method in METHODS:
            seen.clear()
            try:
                oty.makeTyper(method, copy.deepcopy(ref), top_n=top_n, variant_correction=True).typing(gene_cn)
            except np.exceptions.AxisError:
                print(seed, method, "reference crash")
                continue
            print(seed, method, "alleles per gene", {g: len(a) for g, a in sidx.alleles.items()}, "cn", gene_cn, seen, flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "type":
        typeCases(sys.argv[2])
    else:
        scan()
