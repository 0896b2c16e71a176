"""The prepared-sample record (engine.PreparedSample / PreparedGene) slices like the expressions it replaced.  No device."""
import numpy as np

from kir_graph_amd.engine import PreparedGene, PreparedSample, Surviving, Tabulation, _groupByGene


class _Buffer:
    """What ``DeviceSlice`` reads of its parent."""

    def __init__(self, ptr: int, dtype, dev):
        self.ptr, self.dtype, self.dev = ptr, np.dtype(dtype), dev


def _sample():
    """Five genes; gene 2 has neither rows nor surviving variants, gene 4 has rows but no surviving variant."""
    rows = _Buffer(0x7000_0000_1000, np.int32, "tabulation's context")
    vflag, cnt = _Buffer(0x7000_0000_2000, np.uint8, None), _Buffer(0x7000_0000_3000, np.uint32, None)
    off = np.array([0, 7, 19, 19, 20, 33], dtype=np.int64)
    o = np.array([3, 4, 9, 11, 12, 15, 21, 22], dtype=np.int32)
    p = np.arange(100, 108, dtype=np.uint32)
    q = np.arange(200, 208, dtype=np.uint32)
    bounds = np.array([0, 2, 6, 6, 8, 8], dtype=np.int64)
    return PreparedSample(vflag, cnt, rows, off, Surviving(o, p, q, bounds))


def test_gene_slices_equal_the_hand_written_ones():
    prep = _sample()
    for g in range(5):                   # first, last and the empty one among them
        vbeg, vend = 10 * g, 10 * g + 7
        got = prep.gene(g, vbeg, vend, "lane's context")
        # the expressions of the drivers before the record existed
        vflag, cnt, rows_all, off = prep[:4]
        o, p, q, bounds = prep[4]
        a, b = int(off[g]), int(off[g + 1])
        lo, hi = int(bounds[g]), int(bounds[g + 1])
        assert isinstance(got, PreparedGene) and len(got) == 6
        assert got.rows.ptr == rows_all.ptr + 4 * a and got.rows.dtype == np.int32 and got.rows.shape == (b - a,)
        assert got.rows.dev == "lane's context"
        assert got.n_rows == b - a == got[1]
        assert got.vflag is vflag and got.tally is cnt
        assert got.tally_gene == (g, vbeg, vend)
        for have, want in zip(got.surviving, (o[lo:hi], p[lo:hi], q[lo:hi]), strict=True):
            assert have.dtype == want.dtype and np.array_equal(have, want)
        for have, want in zip(Tabulation.survivingOfGene(prep, g), got.surviving, strict=True):
            assert np.array_equal(have, want)
    assert prep.gene(2, 0, 0).n_rows == 0 and all(len(x) == 0 for x in prep.gene(2, 0, 0).surviving)
    assert prep.gene(4, 0, 0).n_rows == 13 and all(len(x) == 0 for x in prep.gene(4, 0, 0).surviving)
    assert prep.gene(0, 0, 0).rows.dev == "tabulation's context"       # no context given: the parent's
    assert prep.gene(0, 0, 0).rows.ptr == prep.rows.ptr and prep.gene(4, 0, 0).rows.ptr == prep.rows.ptr + 4 * 20


def test_record_still_unpacks_by_position():
    prep = _sample()
    vflag, cnt, rows, off = prep[:4]
    assert (vflag, cnt, rows) == (prep.vflag, prep.cnt, prep.rows) == prep[:3] and off is prep.off and prep[0] is prep.vflag
    o, p, q, bounds = prep[4]
    assert o is prep.surviving.ordinals and p is prep.surviving.pos and q is prep.surviving.neg
    assert bounds is prep.surviving.bounds
    rows_g, n, vflag_g, tally, tally_gene, surviving = prep.gene(1, 10, 17)
    assert n == 12 and vflag_g is vflag and tally is cnt and tally_gene == (1, 10, 17) and len(surviving) == 3


def test_grouping_by_gene_is_stable_and_bounds_every_gene():
    """``_groupByGene``: ordinals keep their order inside a gene (novel ones, numbered past the index, fall behind their
    gene's index variants), a gene without any is an empty slice."""
    gene_of = np.array([0, 0, 1, 3, 3, 1, 0], dtype=np.int64)        # the last two: novel variants of genes 1 and 0
    o = np.array([1, 2, 10, 30, 31, 40, 41], dtype=np.int32)
    s = _groupByGene(gene_of, o, (o + 100).astype(np.uint32), (o + 200).astype(np.uint32), 5)
    assert s.bounds.dtype == np.int64 and s.bounds.tolist() == [0, 3, 5, 5, 7, 7]
    assert s.ordinals.tolist() == [1, 2, 41, 10, 40, 30, 31] and s.ordinals.dtype == np.int32
    assert np.array_equal(s.pos, s.ordinals.astype(np.uint32) + 100) and s.pos.dtype == np.uint32
    assert np.array_equal(s.neg, s.ordinals.astype(np.uint32) + 200) and s.neg.dtype == np.uint32
    assert [x.tolist() for x in s.ofGene(1)] == [[10, 40], [110, 140], [210, 240]]
