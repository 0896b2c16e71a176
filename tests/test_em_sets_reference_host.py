"""The plain reference of the candidate-set tests (tests/emsets_reference.py) against ``oracle.em.readCandidates`` -- the
restatement the goldens tie to the upstream project -- on random pairs and on every hand-built row family that the oracle
can express: ids of the gene and novel ids (an id of another gene has alleles of its own there).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import emsets_reference as er  # noqa: E402

from oracle import em as oem  # noqa: E402


def oracleSets(lists, vbeg, vend, n_total, bits):
    """bool [n][n_allele] from ``readCandidates``: variants by name, alleles by name, novel ids carried by nobody."""
    n_allele = bits.shape[1]
    names = [f"A*{a:04d}" for a in range(n_allele)]
    col = {a: i for i, a in enumerate(names)}
    alleles_of = {f"v{v}": ([names[a] for a in np.nonzero(bits[v - vbeg])[0]] if vbeg <= v < vend else [])
                  for v in range(n_total)}
    reads = [{k: [f"v{v}" for v in lst] for k, lst in zip(("lpv", "rpv", "lnv", "rnv"), row)} for row in lists]
    out = np.zeros((len(lists), n_allele), dtype=bool)
    for i, named in enumerate(oem.readCandidates(reads, alleles_of)):
        assert len(set(named)) == len(named)
        out[i, [col[a] for a in named]] = True
    return out


def referenceSets(lists, vbeg, vend, bits):
    off, ids = er.packLists(lists)
    return er.candidateSets(off, ids, np.arange(len(lists)), vbeg, vend, bits)


@pytest.mark.parametrize("words,n_allele", [(1, 21), (1, 32), (2, 53), (3, 96), (5, 149), (9, 288), (16, 501)])
def test_reference_equals_the_oracle_on_the_row_families(words, n_allele):
    g = er.Gene(words, n_allele)
    fams = [f for f in er.rowFamilies(g) if not f[2]]
    assert len(fams) > 100
    lists = [f[1] for f in fams]
    assert all(g.vbeg <= v < g.vend or v >= g.n_var for row in lists for lst in row for v in lst)
    got = referenceSets(lists, g.vbeg, g.vend, g.bits)
    want = oracleSets(lists, g.vbeg, g.vend, g.n_total, g.bits)
    for (name, _, _), a, b in zip(fams, got, want):
        assert np.array_equal(a, b), name
    # the families are not all alike: empty sets, full sets, sets of one allele, both ways of combining the mates
    sizes = got.sum(axis=1)
    assert (sizes == 0).any() and (sizes == n_allele).any() and (sizes == 1).any() and (sizes == 2).any()


def test_reference_equals_the_oracle_on_random_pairs():
    rng = np.random.default_rng(5)
    for n_allele, p in ((7, 0.5), (40, 0.8), (70, 0.9)):
        vbeg, n_span, n_novel = 0, 60, 10
        bits = rng.random((n_span, n_allele)) < p
        lists = [[rng.integers(0, n_span + n_novel, int(m)).tolist() for m in rng.integers(0, 5, 4)] for _ in range(400)]
        got = referenceSets(lists, vbeg, vbeg + n_span, bits)
        want = oracleSets(lists, vbeg, vbeg + n_span, n_span + n_novel, bits)
        assert np.array_equal(got, want)
        both = sum(1 for row in lists if row[0] and row[1])
        assert both > 100 and 0 < (got.sum(axis=1) == 0).sum() < len(lists)


def test_pack_and_distinct():
    sets = np.zeros((6, 70), dtype=bool)
    sets[0, [0, 31, 32, 69]] = True
    sets[1, 33] = True
    sets[2] = sets[0]
    sets[4, 0] = True
    sets[5, 33] = True
    packed = er.pack(sets, 3)
    assert packed.dtype == np.uint32 and packed.shape == (6, 3)
    assert packed[0].tolist() == [0x80000001, 1, 1 << 5] and packed[1].tolist() == [0, 2, 0]
    uniq, count = er.distinct(packed)
    assert uniq.tolist() == [[0, 0, 0], [0, 2, 0], [1, 0, 0], [0x80000001, 1, 32]] and count.tolist() == [1, 2, 1, 2]
    want, want_count = np.unique(packed, axis=0, return_counts=True)
    assert np.array_equal(uniq, want) and np.array_equal(count, want_count)
    none, zero = er.distinct(np.zeros((0, 3), dtype=np.uint32))
    assert none.shape == (0, 3) and len(zero) == 0
