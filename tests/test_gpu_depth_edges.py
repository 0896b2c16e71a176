"""GPU: the plain depth (csrc/gk_depth.hip: depth_mark, one exclusive scan of csrc/gk_scan.hip, depth_finish) through gk_depth
and gk_depth_compact against the restatement of tests/select_reference.py on the marks of tests/depthboot_reference.py: every
position compared, every comparison an equality.

The -1 marks are stored as 0xFFFFFFFF, so the sum of a scan tile whose runs began in an earlier tile wraps; the scan works
over total + 1 words in tiles of 2048: one level up to 2048 words, two up to 2048^2, three from 4 194 305 on (2049 tiles,
then 2, then 1).  At 4 194 305 words the second level's second tile holds one word, the slot past the last position, which
depth_finish does not read: what the third level adds is checked where it is read, by the compaction of
tests/test_gpu_scan_edges.py at the same length; here that length checks that the two full levels below it stay right with a
third above them, gene by gene in tiles 512 apart."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import depthboot_reference as dr  # noqa: E402
import select_reference as sr  # noqa: E402

from kir_graph_amd import _lib, packed, synth  # noqa: E402
from kir_graph_amd.engine import DeviceIndex, Tabulation  # noqa: E402
from kir_graph_amd.hisat2 import pairLines  # noqa: E402

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5A5A5A5
TAIL = 16
FORMS = ("mates", "compact")
CIG_D = 2


class Sample:
    """One sample tabulated from its 128-byte records and from its compact words (as in tests/test_gpu_cn_bootstrap.py)."""

    def __init__(self, device, gidx, rec, spill=None):
        self.dev = device
        self.rec = np.ascontiguousarray(rec)
        self.wide = None if spill is None else spill[0]
        dindex = DeviceIndex(device, gidx)
        self.tabs = {"mates": Tabulation(dindex, self.rec, dev=device, spill=spill),
                     "compact": Tabulation(dindex, packed.CompactMates(self.rec, threads=2), dev=device, spill=spill)}
        self.pair_src = self.tabs["mates"].pairSrc().copy()
        self.pair_nh = self.tabs["mates"].pairNH().copy()
        assert np.array_equal(self.pair_src, self.tabs["compact"].pairSrc())
        self._want = {}

    def depth(self, form, gene_off, multiple):
        """gk_depth / gk_depth_compact into a buffer of sentinels with a tail that must survive."""
        gene_off = np.ascontiguousarray(gene_off, dtype=np.int64)
        total = int(gene_off[-1])
        out = np.full(total + TAIL, SENTINEL, dtype=np.uint32)
        tab = self.tabs[form]
        if form == "mates":
            _lib.check(_lib.lib().gk_depth(self.dev.ctx, tab.handle, tab.mates.ptr, multiple, gene_off.ctypes.data,
                                           len(gene_off) - 1, out.ctypes.data))
        else:
            _lib.check(_lib.lib().gk_depth_compact(self.dev.ctx, tab.handle, tab.mates.words.ptr, multiple, gene_off.ctypes.data,
                                                   len(gene_off) - 1, out.ctypes.data))
        assert (out[total:] == SENTINEL).all(), "written past the last position"
        return out[:total]

    def want(self, gene_off, multiple):
        key = (tuple(int(x) for x in gene_off), int(multiple))
        if key not in self._want:
            marks = dr.pairMarks(self.rec, self.pair_src, self.pair_nh, multiple, gene_off, wide=self.wide)
            self._want[key] = sr.depth(marks, int(gene_off[-1]))
            self._want[key].setflags(write=False)
        return self._want[key]

    def check(self, gene_off, multiple, where=None):
        want = self.want(gene_off, multiple)
        for form in FORMS:
            got = self.depth(form, gene_off, multiple)
            assert np.array_equal(got, want), (where, form, multiple)
        return want

    def close(self):
        for t in self.tabs.values():
            t.mates.free()
            t.close()


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


@pytest.fixture(scope="module")
def real_lens(small_case):
    sidx, gidx, _ = small_case
    return [len(sidx.backbone[g]) for g in gidx.genes]


@pytest.fixture(scope="module")
def sample(device, small_case):
    sidx, gidx, s = small_case
    rec, _ = packed.packSample(s, gidx)
    out = Sample(device, gidx, rec)
    yield out
    out.close()


@pytest.fixture(scope="module")
def wide_sample(device, small_case):
    sidx, gidx, s = small_case
    rng = np.random.default_rng(3)
    lines = synth.toSamLines(s)
    lines = synth.withManyMismatches(lines, sidx, rng.choice(s.n_pairs, size=40, replace=False).tolist(), rng)
    spill = []
    rec, _ = packed.packPairs(list(pairLines(lines)), gidx, spill=spill)
    wide = packed.spillArrays(spill)
    assert wide is not None and len(wide[1]) >= 3
    out = Sample(device, gidx, rec, spill=wide)
    yield out
    out.close()


def firstStarts(smp, n_gene):
    """Per gene the start of the first mate of a valid pair with NH == 1 that lies on it."""
    out = [None] * n_gene
    for p, nh in zip(smp.pair_src, smp.pair_nh):
        for r in smp.rec[2 * int(p):2 * int(p) + 2]:
            if nh == 1 and out[int(r["ref"])] is None:
                out[int(r["ref"])] = int(r["pos0"])
    return out


def insideDeletions(smp, n_gene):
    """Per gene a length that ends one base into a D run of two bases or more of a counted mate: the M run before it ends
    just short of the last base, the D run crosses the end, the M run after it lies beyond."""
    out = [None] * n_gene
    for p, nh in zip(smp.pair_src, smp.pair_nh):
        for r in smp.rec[2 * int(p):2 * int(p) + 2]:
            g, cur = int(r["ref"]), int(r["pos0"])
            if nh != 1 or out[g] is not None or int(r["n_cig"]) > 14:
                continue
            for c in r["cig"][:int(r["n_cig"])]:
                op, n = int(c) & 15, int(c) >> 4
                if op == CIG_D and n >= 2:
                    out[g] = cur + 1
                    break
                if op in (0, CIG_D):
                    cur += n
    return out


# ------------------------------------------------------------------------------------------------ clipping
@pytest.mark.parametrize("multiple", [0, 1])
def test_runs_are_clipped_to_the_declared_lengths(sample, wide_sample, real_lens, multiple):
    n_gene = len(real_lens)
    for name, smp in (("plain", sample), ("wide", wide_sample)):
        starts, dels = firstStarts(smp, n_gene), insideDeletions(smp, n_gene)
        assert None not in starts and None not in dels
        last_base = [s + 1 for s in starts]
        assert all(a <= b for a, b in zip(last_base, real_lens)) and all(a <= b for a, b in zip(dels, real_lens))
        for kind, lens in (("one", [1] * n_gene), ("start_of_first_read", last_base), ("inside_deletion", dels), ("real", real_lens)):
            gene_off = offsets(lens)
            want = smp.check(gene_off, multiple, (name, kind))
            if kind == "start_of_first_read":      # that read starts on the last base and is counted there
                assert (want[gene_off[1:] - 1] >= 1).all()
            if kind == "real":
                assert want.sum() > 100 * len(smp.pair_src)
    # pairs with NH > 1 change the depth, wide pairs carry depth of their own
    assert (sample.pair_nh != 1).any()
    real_off = offsets(real_lens)
    assert not np.array_equal(sample.want(real_off, 1), sample.want(real_off, 0))
    narrow = sr.depth(dr.pairMarks(wide_sample.rec, wide_sample.pair_src, wide_sample.pair_nh, 1, real_off, wide=None), int(real_off[-1]))
    assert narrow.sum() < wide_sample.want(real_off, 1).sum()


# ------------------------------------------------------------------------------------------------ scan edges
# total + 1 = 2048 (one tile), 2049 (a second tile of one word), 4096 (two tiles), 4097 (a third tile of one word); from 4095
# on a gene boundary one word before, on and one word after the tile boundary at 2048
EDGE_LENS = [[1000, 500, 500, 47], [1000, 500, 500, 48],
             [2047, 2046, 1, 1], [2048, 2045, 1, 1], [2049, 2044, 1, 1],
             [2047, 2047, 1, 1], [2048, 2046, 1, 1], [2049, 2045, 1, 1]]


@pytest.mark.parametrize("lens", EDGE_LENS, ids=lambda lens: "-".join(str(x) for x in lens))
def test_scan_edges_with_wrapped_marks(sample, wide_sample, lens):
    gene_off = offsets(lens)
    assert int(gene_off[-1]) + 1 in (2048, 2049, 4096, 4097)
    for multiple in (0, 1):
        want = sample.check(gene_off, multiple, "plain")
        assert want.max() >= 8
        if int(gene_off[-1]) >= 4095 and lens[0] >= 2048:
            # the runs open at position 2047 began in the first tile and end in the second: with the words from 2048 on
            # summing to minus that depth, the second tile's sum wraps
            assert want[2047] > 0
    wide_sample.check(gene_off, 1, "wide")


# ------------------------------------------------------------------------------------------------ three levels
def test_three_scan_levels(sample, wide_sample, real_lens):
    """total + 1 = 4 194 305 words: declared lengths far longer than the backbones, every gene's reads in first-level tiles of
    their own (512 tiles apart), gene boundaries on, before and after a tile boundary.  Mostly zero; every position counts."""
    lens = [(1 << 20) + 1, (1 << 20) - 1, (1 << 20) + 777, (1 << 20) - 777]
    gene_off = offsets(lens)
    assert int(gene_off[-1]) + 1 == 4194305 and all(a > b for a, b in zip(lens, real_lens))
    tiles = [set(range(int(a) // 2048, (int(a) + b) // 2048 + 1)) for a, b in zip(gene_off[:-1], real_lens)]
    assert all(not (tiles[i] & tiles[j]) for i in range(4) for j in range(i))
    for multiple in (0, 1):
        want = sample.check(gene_off, multiple, "plain")
        for a, b, real in zip(gene_off[:-1], gene_off[1:], real_lens):
            assert want[a:a + real].sum() > real and not want[a + real:b].any()
    wide_sample.check(gene_off, 1, "wide")
    # the same reads under their real lengths: the padding moved them, nothing else
    real_off = offsets(real_lens)
    want, short = sample.want(gene_off, 0), sample.want(real_off, 0)
    for g, real in enumerate(real_lens):
        assert np.array_equal(want[gene_off[g]:gene_off[g] + real], short[real_off[g]:real_off[g + 1]])


# ------------------------------------------------------------------------------------------------ fewer genes
@pytest.mark.parametrize("n_gene", [1, 2, 3])
def test_mates_of_genes_beyond_the_table_are_skipped(sample, wide_sample, real_lens, n_gene):
    gene_off = offsets(real_lens[:n_gene])
    full = offsets(real_lens)
    for multiple in (0, 1):
        for smp in (sample, wide_sample):
            want = smp.check(gene_off, multiple, n_gene)
            assert np.array_equal(want, smp.want(full, multiple)[:int(gene_off[-1])])       # the other genes add nothing
    assert (sample.rec["ref"] >= n_gene).any()
