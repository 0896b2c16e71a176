"""tests/compat_reference.py against the oracle's ``GeneModel.probs`` / ``.log_probs``, bit for bit (no GPU): on a synthetic
gene with and without the error correction and with both ``no_empty`` values, and on the hand-built sample whose long rows
reach subnormal products and ``+0.0`` -- whose designed mismatch counts and list orders are checked here too, so the GPU
tests that build on it stand on a sample that is what it says."""
import copy
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import compat_reference as cr  # noqa: E402

from kir_graph_amd import synth  # noqa: E402
from oracle import tabulate as ot, typing as oty  # noqa: E402


def geneTables(data, gene=None):
    """(off, ids, rows of ``gene``, vbeg, vend, bits, allele names, n_var_total) of an oracle tabulation: ordinals are the
    positions in ``data["variants"]`` (the index variants in order, then the novel ones)."""
    variants = data["variants"]
    ordinal = {str(v.id): i for i, v in enumerate(variants)}
    off, ids = cr.packLists([[[ordinal[x] for x in r[k]] for k in ("lpv", "rpv", "lnv", "rnv")] for r in data["reads"]])
    rows = [i for i, r in enumerate(data["reads"]) if (gene is None or r["backbone"] == gene) and r["multiple"] == 1]
    mine = [i for i, v in enumerate(variants) if (gene is None or v.ref == gene) and not str(v.id).startswith("nv")]
    vbeg, vend = (mine[0], mine[-1] + 1) if mine else (0, 0)
    assert mine == list(range(vbeg, vend))
    names = sorted(oty.alleleNames(variants[vbeg:vend]))
    col = {a: i for i, a in enumerate(names)}
    bits = np.zeros((vend - vbeg, len(names)), dtype=bool)
    for i in range(vbeg, vend):
        bits[i - vbeg, [col[a] for a in variants[i].allele]] = True
    return off, ids, rows, vbeg, vend, bits, names, len(variants)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def synthetic():
    sidx = synth.makeIndex(seed=78, n_genes=1, var_range=(260, 320), allele_range=(22, 28), len_range=(5000, 6000))
    sample = synth.makeSample(sidx, seed=5, n_pairs=1200, gene_cn={sidx.genes[0]: 2}, frac_multi=0.0, err_rate=0.004)
    data = ot.tabulateLines(synth.toSamLines(sample), sidx.variants)
    for i in range(0, len(data["reads"]), 17):          # some rows without any id
        for k in ("lpv", "lnv", "rpv", "rnv"):
            data["reads"][i][k] = []
    return data


@pytest.mark.parametrize("correction", [False, True])
@pytest.mark.parametrize("no_empty", [True, False])
def test_helper_equals_the_oracle_on_a_synthetic_gene(synthetic, correction, no_empty):
    data = synthetic
    off, ids, rows, vbeg, vend, bits, names, n_var = geneTables(data)
    assert any(str(v.id).startswith("nv") for v in data["variants"])        # novel ids: no allele carries them
    vflag = np.zeros(n_var, dtype=np.uint8)
    if correction:
        vflag = cr.correctionFlags(*cr.tally(off, ids, rows, vflag, n_var))
        assert (vflag & 1).any() and (vflag & 2).any() and (vflag == 0).any()
    ref = cr.compatReference(off, ids, rows, vflag, vbeg, vend, bits, keep_empty=not no_empty)
    cpu = oty.GeneModel(copy.deepcopy([data["reads"][i] for i in rows]), data["variants"], force_homo=False, top_n=50,
                        no_empty=no_empty, variant_correction=correction)
    assert [cpu.id_to_allele[i] for i in range(len(names))] == names
    keep = ref.nvar > 0 if no_empty else np.ones(len(rows), dtype=bool)
    assert 0 < keep.sum() and (no_empty or (ref.nvar == 0).any())
    same_bits(ref.probs[keep], cpu.probs)
    same_bits(ref.log[keep], cpu.log_probs)
    miss, nvar = oty.missTable(cpu.reads, cpu.variants, cpu.allele_to_id)
    assert np.array_equal(ref.miss[keep], miss) and np.array_equal(ref.nvar[keep], nvar)
    if not no_empty:
        assert (ref.probs[ref.nvar == 0] == cr.HIT).all()


@pytest.fixture(scope="module")
def underflow():
    sidx, order = cr.underflowIndex()
    return sidx, order, {w: ot.tabulateLines(cr.underflowLines(sidx, w), sidx.variants) for w in ("a", "b")}


@pytest.mark.parametrize("which", ["a", "b"])
def test_helper_equals_the_oracle_where_products_underflow(underflow, which):
    sidx, order, tabs = underflow
    data = tabs[which]
    assert not any(str(v.id).startswith("nv") for v in data["variants"])
    pos_of = {str(v.id): v.pos for v in data["variants"]}
    for gene, counts in ((cr.HEAVY_GENE, cr.HEAVY_COUNTS), (cr.CAPPED_GENE, cr.CAPPED_COUNTS)):
        off, ids, rows, vbeg, vend, bits, names, n_var = geneTables(data, gene)
        assert names == sidx.alleles[gene] and (gene != cr.HEAVY_GENE or vbeg > 0)
        zero = np.zeros(n_var, dtype=np.uint8)
        vflag = cr.correctionFlags(*cr.tally(off, ids, rows, zero, n_var))
        ref = cr.compatReference(off, ids, rows, vflag, vbeg, vend, bits, keep_empty=False)
        cpu = oty.GeneModel(copy.deepcopy([data["reads"][i] for i in rows]), [v for v in data["variants"] if v.ref == gene],
                            force_homo=False, top_n=40, variant_correction=True)
        keep = ref.nvar > 0                   # the short pairs beyond the last window list nothing: the oracle drops them
        same_bits(ref.probs[keep], cpu.probs)
        same_bits(ref.log[keep], cpu.log_probs)
        # the sample is what its generator says: the three long rows keep every id through the correction, list their
        # sites in the designed order and mismatch allele k exactly counts[k] times
        long_rows = [i for i, r in enumerate(rows) if "\theavy" in "\t" + data["reads"][r]["l_sam"]]
        assert len(long_rows) == len(cr.PLACEMENTS)
        for w, i in enumerate(long_rows):
            r = data["reads"][rows[i]]
            listed = [pos_of[x] for k in ("lpv", "rpv", "lnv", "rnv") for x in r[k]]
            known = {v.pos for v in data["variants"] if v.ref == gene}
            assert listed == [p for p in order[gene][w] if p in known]
            kept = [x for k, bit in (("lpv", 1), ("rpv", 1), ("lnv", 2), ("rnv", 2)) for x in r[k]
                    if not vflag[int(x[2:])] & bit]
            assert len(kept) == len(listed) == ref.nvar[i]
            assert ref.miss[i].tolist() == counts, (gene, w)
        if gene == cr.CAPPED_GENE:
            assert ref.miss.max() == 99 and not ref.flag0 and np.isfinite(ref.log).all()
            continue
        heavy = ref.probs[long_rows]
        m = np.array(counts)
        tiny = np.finfo(np.float64).tiny
        assert ((heavy[:, m >= 108] == 0.0) & ~np.signbit(heavy[:, m >= 108])).all()
        assert np.isneginf(ref.log[long_rows][:, m >= 108]).all()
        sub = heavy[:, (m >= 103) & (m <= 107)]
        assert ((sub > 0) & (sub < tiny)).all()
        assert (heavy[:, m <= 102] >= tiny).all()
        # the order of the factors is part of the result: the three placements round their subnormals differently
        assert len({heavy[w, m == 107].tobytes() for w in range(3)}) > 1
        assert ref.flag0 and ref.miss8[long_rows][:, m >= 100].min() == 255 and ref.miss_u8.max() == 255
        under = [i for i, r in enumerate(rows) if "\tunder" in "\t" + data["reads"][r]["l_sam"]]
        assert len(under) == (3 if which == "b" else 0)
        for i in under:
            assert ref.nvar[i] == 130 and (ref.miss[i] == 130).all() and (ref.probs[i] == 0.0).all()
        # sample a keeps finite sets, sample b has none (and the oracle still returns a call without a NaN)
        res = cpu.typing(2)
        if which == "a":
            assert np.isfinite(res.value[0]) and np.isneginf(cpu.log_probs).any()
        else:
            assert np.isneginf(res.value).all()
        assert not np.isnan(res.value).any() and not np.isnan(res.fraction).any()
        assert len(oty.selectBest(res)) == 2
