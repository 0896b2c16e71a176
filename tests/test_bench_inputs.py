"""bench.py makes its samples with its own faster copy of the package's generator (bench.synth_sample) and packs them on
several threads (bench.pack_sample): both must give exactly what synth.makeSample + packed.packSample give, or the
benchmark would time other inputs than the ones it names."""
import dataclasses
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from kir_graph_amd import packed, synth  # noqa: E402
from kir_graph_amd.index import GkIndex  # noqa: E402


@pytest.fixture(scope="module")
def bench_index():
    return bench.build_index()


def _same_sample(a, b):
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        if f.name == "index":
            assert x is y
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), f.name
        else:
            assert x == y, f.name


@pytest.mark.parametrize("seed,n_pairs,threads", [(1031, 200_000, 4), (1038, 150_001, 3), (99, 3000, 8)])
def test_bench_samples_are_the_packages(bench_index, seed, n_pairs, threads):
    sidx, gidx, by_gene = bench_index
    want = synth.makeSample(sidx, seed=seed, n_pairs=n_pairs, variants_by_gene=by_gene)
    got = bench.synth_sample(sidx, seed=seed, n_pairs=n_pairs, variants_by_gene=by_gene)
    _same_sample(want, got)
    rec, table = packed.packSample(want, gidx)
    rec2, table2 = bench.pack_sample(got, gidx, threads)
    assert rec.dtype == rec2.dtype and rec.tobytes() == rec2.tobytes()
    assert table.strings == table2.strings and table.ids == table2.ids


def test_bench_samples_on_another_index():
    """Another index shape and the generator's own defaults (variants by gene made inside)."""
    sidx = synth.makeIndex(seed=7, n_genes=4, var_range=(300, 600), allele_range=(20, 40))
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    want = synth.makeSample(sidx, seed=5, n_pairs=120_000)
    got = bench.synth_sample(sidx, seed=5, n_pairs=120_000)
    _same_sample(want, got)
    assert packed.packSample(want, gidx)[0].tobytes() == bench.pack_sample(got, gidx, 2)[0].tobytes()
