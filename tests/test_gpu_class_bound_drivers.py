"""The integer bound over the pseudo-rows of the row classes (csrc/gk_classrows.h) through the drivers: exon-first typing
of the small sample of tests/test_gpu_row_classes.py (3 genes, 2000 pairs; its helper restated here) in fresh child
processes under ``GK_TEST_HOOKS=row_classes=on,class_bound=on``, ``...=off`` and ``...=nomem`` (the pool refuses the
pseudo-row table: the gene then runs on its rows).  A child types the sample twice: with the fresh value table of a new
process -- the tables are patched while the class route is on -- and with the warmed one.  Every step of every search
must agree between the hooks (values, ids, fractions, the bounded steps and the calls with ``np.array_equal``), and the
calls are the oracle's.  The launch log says which rows a bound ran over: padded pseudo-rows under ``on``, the table's
rows otherwise."""
import copy
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HOOKS = {"on": "row_classes=on,class_bound=on", "off": "row_classes=on,class_bound=off",
         "nomem": "row_classes=on,class_bound=nomem"}
FIELDS = ("value", "value_sum_indv", "allele_id", "fraction")


def small_sample():
    from kir_graph_amd import synth
    from kir_graph_amd.index import GkIndex
    sidx = synth.makeIndex(seed=2022, n_genes=3, var_range=(200, 300), allele_range=(12, 24))
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    sample = synth.makeSample(sidx, seed=1031, n_pairs=2000)
    return gidx, sample


def child(out_path):
    """Types the sample twice in this (fresh) process and leaves what came out in ``out_path``."""
    from kir_graph_amd import _lib, packed
    from kir_graph_amd import typing_mulit_allele as tma
    from kir_graph_amd.engine import DeviceIndex, Tabulation
    from kir_graph_amd.hisat2 import SampleData
    from kir_graph_amd.kir_typing import selectKirTypingModel
    gidx, sample = small_sample()
    made = _lib.Device.__init__

    def logged(self, *args, **kwargs):   # every context of the process, the ones the typing makes on its way too, keeps
        made(self, *args, **kwargs)      # its launch log
        self.call_log = []
    _lib.Device.__init__ = logged
    device = _lib.Device(0)
    rec, table = packed.packSample(sample, gidx)
    dindex = DeviceIndex(device, gidx)
    tab = Tabulation(dindex, rec)
    runs = []
    try:
        data = SampleData(tab, gidx, None, ins_strings=table.strings)
        for _ in ("fresh", "warm"):
            for d in _lib.Device.instances:
                d.call_log = []
            before = dict(tma.SEARCH_STATS)
            gpu = selectKirTypingModel("exonfirst_1", data, top_n=600, variant_correction=True)
            calls = gpu.typing(sample.gene_cn)
            steps = {gene: [dict(n=int(s.n), names=[list(r) for r in s.allele_name],
                                 **{f: np.array(getattr(s, f)) for f in FIELDS}) for s in res]
                     for gene, res in gpu._result.items()}
            runs.append(dict(calls=calls, steps=steps,
                             stats={k: tma.SEARCH_STATS[k] - before[k] for k in before},
                             bound_rows=[int(e[1]) for d in _lib.Device.instances for e in d.call_log or []
                                         if e[0] == "minsum_sad"]))
    finally:
        tab.close()
        dindex.close()
        device.close()
    with open(out_path, "wb") as f:
        pickle.dump(runs, f)


@pytest.fixture(scope="module")
def typed(tmp_path_factory):
    """hook -> [fresh run, warm run] of a child process each, and the oracle's typing."""
    from oracle import tabulate as ot, typing as oty
    from kir_graph_amd import synth
    out = {}
    for name, hooks in HOOKS.items():
        path = str(tmp_path_factory.mktemp("class_bound") / f"{name}.pkl")
        env = dict(os.environ, GK_TEST_HOOKS=hooks)
        done = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, cwd=os.path.dirname(HERE),
                              capture_output=True, text=True, timeout=300)
        assert done.returncode == 0, (name, done.stdout[-2000:], done.stderr[-4000:])
        with open(path, "rb") as f:
            out[name] = pickle.load(f)
    gidx, sample = small_sample()
    ref = ot.tabulateLines(synth.toSamLines(sample), gidx.variants)
    cpu = oty.makeTyper("exonfirst_1", copy.deepcopy(ref), top_n=600, variant_correction=True)
    want_calls = cpu.typing(sample.gene_cn)
    return out, cpu, want_calls


def same_runs(a, b):
    assert a["calls"] == b["calls"]
    assert a["stats"] == b["stats"]                      # the same steps were served by the bound
    assert a["steps"].keys() == b["steps"].keys()
    for gene in a["steps"]:
        assert len(a["steps"][gene]) == len(b["steps"][gene]), gene
        for x, y in zip(a["steps"][gene], b["steps"][gene]):
            assert x["n"] == y["n"] and x["names"] == y["names"], gene
            for f in FIELDS:
                assert x[f].shape == y[f].shape and np.array_equal(x[f], y[f]), (gene, f)


@pytest.mark.parametrize("run", [0, 1], ids=["fresh value table", "warm value table"])
@pytest.mark.parametrize("hook", ["on", "nomem"])
def test_every_step_agrees_with_the_row_route(typed, hook, run):
    out, _, _ = typed
    same_runs(out[hook][run], out["off"][run])
    same_runs(out[hook][run], out[hook][1 - run])        # and a patched table gives what a table written at once gives


@pytest.mark.parametrize("hook", list(HOOKS))
def test_calls_and_steps_are_the_oracles(typed, hook):
    out, cpu, want_calls = typed
    for run in out[hook]:
        assert run["calls"] == want_calls
        assert run["stats"]["bounded"] > 0               # the sample has steps that the bound serves
        for gene, steps in cpu.results.items():
            assert len(run["steps"][gene]) == len(steps), gene
            for x, b in zip(run["steps"][gene], steps):
                assert x["n"] == b.n and x["names"] == [list(r) for r in b.allele_name]
                for f in FIELDS:
                    y = np.asarray(getattr(b, f))
                    assert x[f].shape == y.shape and not np.isnan(x[f]).any() and np.array_equal(x[f], y), (gene, f)


def test_which_rows_the_bounds_ran_over(typed):
    """Under ``on`` every bound of a table with a class record runs over padded pseudo-rows (a multiple of 128 that is not
    the table's row count); with the pool refusing the record, and under ``off``, over the rows."""
    out, _, _ = typed
    for run in (0, 1):
        rows_off = out["off"][run]["bound_rows"]
        assert rows_off and out["nomem"][run]["bound_rows"] == rows_off
        rows_on = out["on"][run]["bound_rows"]
        assert len(rows_on) == len(rows_off)
        changed = [a for a, b in zip(rows_on, rows_off) if a != b]
        assert changed and all(a % 128 == 0 for a in changed)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    child(sys.argv[1])
