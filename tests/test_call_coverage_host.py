"""Per-allele coverage of a likelihood call, host side (no GPU): the regions of a gene, the private sites of a called
allele, both texts, command-line flags and factory refusals, and the restatement of tests/callcov_reference.py against the
depth oracle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(__file__))
import callcov_reference as cr  # noqa: E402

from kir_graph_amd import main as cli, packed, synth  # noqa: E402
from kir_graph_amd.call_coverage import (CALL_COVERAGE_COLUMNS, CALL_COVERAGE_DEPTH_COLUMNS, CallCoverage,  # noqa: E402
                                         callCoverageDepthText, callCoverageText, depthRuns, privateSites, regionsOf,
                                         summarise)
from kir_graph_amd.hisat2 import pairLines  # noqa: E402
from kir_graph_amd.index import buildMask  # noqa: E402
from kir_graph_amd.msa2hisat import Variant  # noqa: E402
from oracle import depth as odepth, tabulate as ot  # noqa: E402


# ------------------------------------------------------------------------------------------------ regions
REGION_CASES = {
    "no exons": ([], 50, [("gene", 0, 50)]),
    "an exon starting at 0": ([(0, 10), (20, 30)], 50,
                              [("gene", 0, 50), ("exon1", 0, 10), ("intron1", 10, 20), ("exon2", 20, 30), ("downstream", 30, 50)]),
    "an exon ending at the length": ([(5, 10), (40, 50)], 50,
                                     [("gene", 0, 50), ("upstream", 0, 5), ("exon1", 5, 10), ("intron1", 10, 40), ("exon2", 40, 50)]),
    "an exon ending beyond the length": ([(5, 10), (40, 70)], 50,
                                         [("gene", 0, 50), ("upstream", 0, 5), ("exon1", 5, 10), ("intron1", 10, 40), ("exon2", 40, 50)]),
    "an exon wholly beyond the length": ([(5, 10), (60, 70), (80, 90)], 50,
                                         [("gene", 0, 50), ("upstream", 0, 5), ("exon1", 5, 10), ("intron1", 10, 50)]),
    "adjacent exons": ([(5, 10), (10, 20), (30, 35)], 50,
                       [("gene", 0, 50), ("upstream", 0, 5), ("exon1", 5, 10), ("exon2", 10, 20), ("intron2", 20, 30),
                        ("exon3", 30, 35), ("downstream", 35, 50)]),
    "unsorted input": ([(30, 35), (5, 10)], 50,
                       [("gene", 0, 50), ("upstream", 0, 5), ("exon1", 5, 10), ("intron1", 10, 30), ("exon2", 30, 35),
                        ("downstream", 35, 50)]),
    "an empty exon keeps its number": ([(5, 10), (20, 20), (30, 35)], 50,
                                       [("gene", 0, 50), ("upstream", 0, 5), ("exon1", 5, 10), ("intron1", 10, 20), ("intron2", 20, 30),
                                        ("exon3", 30, 35), ("downstream", 35, 50)]),
    "length 1, in an exon": ([(0, 4)], 1, [("gene", 0, 1), ("exon1", 0, 1)]),
    "length 1, before the exon": ([(3, 4)], 1, [("gene", 0, 1), ("upstream", 0, 1)]),
    "length 1, no exons": ([], 1, [("gene", 0, 1)]),
}


@pytest.mark.parametrize("case", sorted(REGION_CASES))
def test_regions(case):
    exons, length, want = REGION_CASES[case]
    got = regionsOf(exons, length)
    assert got == want
    assert got == cr.regions(exons, length)
    # after the gene the regions tile [0, length) when there is an exon at all
    if exons:
        assert got[1][1] == 0 and got[-1][2] == length and all(a[2] == b[1] for a, b in zip(got[1:], got[2:]))


def test_regions_of_a_real_shaped_gene_equal_the_restatement():
    rng = np.random.default_rng(5)
    for _ in range(50):
        length = int(rng.integers(1, 400))
        cuts = np.sort(rng.integers(0, length + 40, size=2 * int(rng.integers(0, 6))))
        exons = [(int(cuts[2 * i]), int(cuts[2 * i + 1])) for i in range(len(cuts) // 2)]
        rng.shuffle(exons)
        assert regionsOf(exons, length) == cr.regions(exons, length), (exons, length)


# ------------------------------------------------------------------------------------------------ private sites
ALLELES = [f"G*{i:03d}" for i in range(40)]                     # two words of bits


def bitRows(carriers):
    """Bit rows of variants carried by the listed allele ordinals."""
    return buildMask([Variant(pos=i, typ="single", ref="G", id=f"v{i}", val="A", allele=[ALLELES[a] for a in c])
                      for i, c in enumerate(carriers)], ALLELES)


def test_private_sites():
    #          v0     v1      v2          v3   v4       v5           v6
    mask = bitRows([[3], [35], [3, 35], [], [7], [3, 7, 35], [7, 35]])
    assert mask.shape == (7, 2)
    # one distinct called allele: none
    assert [s.tolist() for s in privateSites(mask, [3])] == [[]]
    # two: symmetric -- every site that tells them apart is private to both
    a, b = privateSites(mask, [3, 35])
    assert a.tolist() == b.tolist() == [0, 1, 6]
    a, b = privateSites(mask, [35, 3])
    assert a.tolist() == b.tolist() == [0, 1, 6]
    # three: v2 separates 3 from 7 only (35 carries it too) and is private to 7 alone -- the one that lacks it; v6 to 3
    got = [s.tolist() for s in privateSites(mask, [3, 7, 35])]
    assert got == [[0, 6], [2, 4], [1]]
    assert 2 not in got[0] and 2 not in got[2]
    for ids in ([3], [3, 35], [35, 3], [3, 7, 35], [0, 3, 7, 35]):
        assert [s.tolist() for s in privateSites(mask, ids)] == cr.privateSites(mask, ids), ids


def test_summary_counts_sites_where_they_lie():
    depth = np.zeros((6, 30), dtype=np.uint32)                    # K = 2
    depth[0, 2:20] = 3
    depth[1, 5:8] = 1
    depth[2, 2:20] = 2
    depth[3, 4:20] = 2
    depth[4, 2:6] = 1                                             # unique_0
    depth[5, 25:30] = 4                                           # unique_1
    regs = regionsOf([(5, 10), (20, 28)], 30)
    sites = [np.array([3, 5, 9, 29]), np.array([0, 27, 29, 29])]   # a site past the end was clipped to 29 by the caller
    bases, covered, n_sites, bare = summarise(depth, regs, sites)
    want = cr.summary(depth, regs, [s.tolist() for s in sites])
    for r in range(len(regs)):
        assert (bases[r].tolist(), covered[r].tolist(), n_sites[r].tolist(), bare[r].tolist()) == tuple(want[r]), regs[r]
    assert [r[0] for r in regs] == ["gene", "upstream", "exon1", "intron1", "exon2", "downstream"]
    assert bases[0].tolist() == [54, 3, 36, 32, 4, 20] and covered[0].tolist() == [18, 3, 18, 16, 4, 5]
    assert n_sites[:, 0].tolist() == [4, 1, 2, 0, 0, 1] and bare[:, 0].tolist() == [2, 0, 1, 0, 0, 1]
    assert n_sites[:, 1].tolist() == [4, 1, 0, 0, 1, 2] and bare[:, 1].tolist() == [1, 1, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the texts
def covers():
    depth = np.zeros((6, 12), dtype=np.uint32)
    depth[0, 1:9] = 5
    depth[1, 3:5] = 1
    depth[2, 1:9] = 4
    depth[3, 2:9] = [3, 3, 3, 2, 2, 2, 2]
    depth[4, 1:4] = 2
    depth[5, 6:9] = 1
    regs = regionsOf([(2, 6)], 12)
    sites = [np.array([1, 7]), np.array([7, 11])]
    bases, covered, n_sites, bare = summarise(depth, regs, sites)
    two = CallCoverage(cn=3, reads=40, length=12, alleles=[("KIR2DL1*001", 2), ("KIR2DS1*002", 1)], depth=depth, regions=regs,
                       bases=bases, covered=covered, private_sites=n_sites, private_unsupported=bare)
    d1 = np.zeros((4, 3), dtype=np.uint32)
    d1[[0, 2, 3]] = 7                                             # K = 1: best = unique = informative
    regs1 = regionsOf([], 3)
    b1, c1, s1, u1 = summarise(d1, regs1, [np.zeros(0, dtype=np.int64)])
    one = CallCoverage(cn=2, reads=9, length=3, alleles=[("KIR2DL2*003", 2)], depth=d1, regions=regs1, bases=b1, covered=c1,
                       private_sites=s1, private_unsupported=u1)
    return {"KIR2DL1S1": two, "KIR2DL2": one}


def test_coverage_file_bytes(tmp_path):
    files = cli.writeCallReport("call_coverage", str(tmp_path / "s.pv"), covers())
    assert [os.path.basename(f) for f in files] == ["s.pv.coverage.tsv"] and not (tmp_path / "s.pv.coverage.depth.tsv").exists()
    want = ("gene\tcn\treads\tregion\tstart\tend\tlength\tinformative_bases\tmismatch_bases\tmismatch_covered\tallele\tcopies\t"
            "best_bases\tunique_bases\tbest_covered\tunique_covered\tprivate_sites\tprivate_unsupported\n"
            "KIR2DL1S1\t3\t40\tgene\t0\t12\t12\t40\t2\t2\tKIR2DL1*001\t2\t32\t6\t8\t3\t2\t1\n"
            "KIR2DL1S1\t3\t40\tgene\t0\t12\t12\t40\t2\t2\tKIR2DS1*002\t1\t17\t3\t7\t3\t2\t1\n"
            "KIR2DL1S1\t3\t40\tupstream\t0\t2\t2\t5\t0\t0\tKIR2DL1*001\t2\t4\t2\t1\t1\t1\t0\n"
            "KIR2DL1S1\t3\t40\tupstream\t0\t2\t2\t5\t0\t0\tKIR2DS1*002\t1\t0\t0\t0\t0\t0\t0\n"
            "KIR2DL1S1\t3\t40\texon1\t2\t6\t4\t20\t2\t2\tKIR2DL1*001\t2\t16\t4\t4\t2\t0\t0\n"
            "KIR2DL1S1\t3\t40\texon1\t2\t6\t4\t20\t2\t2\tKIR2DS1*002\t1\t11\t0\t4\t0\t0\t0\n"
            "KIR2DL1S1\t3\t40\tdownstream\t6\t12\t6\t15\t0\t0\tKIR2DL1*001\t2\t12\t0\t3\t0\t1\t1\n"
            "KIR2DL1S1\t3\t40\tdownstream\t6\t12\t6\t15\t0\t0\tKIR2DS1*002\t1\t6\t3\t3\t3\t2\t1\n"
            "KIR2DL2\t2\t9\tgene\t0\t3\t3\t21\t0\t0\tKIR2DL2*003\t2\t21\t21\t3\t3\t0\t0\n")
    text = open(files[0]).read()
    assert text == want == callCoverageText(covers())
    assert text.split("\n")[0].split("\t") == CALL_COVERAGE_COLUMNS == cr.COLUMNS
    # integers as integers
    for line in text.split("\n")[1:-1]:
        cells = line.split("\t")
        assert len(cells) == 18 and all(c.isdigit() for i, c in enumerate(cells) if i not in (0, 3, 10)), line
    # the restatement writes the same bytes
    entries = [(g, c.cn, c.reads, c.alleles, c.regions,
                cr.summary(c.depth, c.regions, [[1, 7], [7, 11]] if g == "KIR2DL1S1" else [[]])) for g, c in covers().items()]
    assert cr.coverageText(entries) == want
    # a gene whose report could not be made is left out; nothing at all: the header alone
    assert callCoverageText({}) == "\t".join(CALL_COVERAGE_COLUMNS) + "\n"
    files = cli.writeCallReport("call_coverage", str(tmp_path / "t.pv"), {"KIR2DL2": None, "KIR3DL3": None}, call_coverage_depth=True)
    assert open(files[0]).read() == "\t".join(CALL_COVERAGE_COLUMNS) + "\n"
    assert open(files[1]).read() == "\t".join(CALL_COVERAGE_DEPTH_COLUMNS) + "\n"


def test_depth_file_runs_tile_the_gene(tmp_path):
    files = cli.writeCallReport("call_coverage", str(tmp_path / "s.pv"), covers(), call_coverage_depth=True)
    assert [os.path.basename(f) for f in files] == ["s.pv.coverage.tsv", "s.pv.coverage.depth.tsv"]
    text = open(files[1]).read()
    assert text == callCoverageDepthText(covers())
    assert text == cr.depthText([(g, c.alleles, c.depth) for g, c in covers().items()])
    lines = text.split("\n")
    assert lines[0].split("\t") == CALL_COVERAGE_DEPTH_COLUMNS == cr.DEPTH_COLUMNS == ["gene", "track", "allele", "start", "end", "depth"]
    assert lines[-1] == ""
    rows = [line.split("\t") for line in lines[1:-1]]
    assert all(len(r) == 6 and all(c.isdigit() for c in r[3:]) for r in rows)
    # tracks in the order informative, mismatch, best, unique, alleles ascending; the allele cell empty for the first two
    order = list(dict.fromkeys((r[0], r[1], r[2]) for r in rows))
    assert order == [("KIR2DL1S1", "informative", ""), ("KIR2DL1S1", "mismatch", ""), ("KIR2DL1S1", "best", "KIR2DL1*001"),
                     ("KIR2DL1S1", "best", "KIR2DS1*002"), ("KIR2DL1S1", "unique", "KIR2DL1*001"),
                     ("KIR2DL1S1", "unique", "KIR2DS1*002"), ("KIR2DL2", "informative", ""), ("KIR2DL2", "mismatch", ""),
                     ("KIR2DL2", "best", "KIR2DL2*003"), ("KIR2DL2", "unique", "KIR2DL2*003")]
    # the runs of a track tile [0, length) in ascending order, neighbours differ, and they expand to the depth
    back = cr.expandDepthText(text)                                # asserts start == the previous end, from 0
    for gene, c in covers().items():
        k = len(c.alleles)
        keys = [(gene, "informative", ""), (gene, "mismatch", "")] + [(gene, "best", a) for a, _ in c.alleles] + \
               [(gene, "unique", a) for a, _ in c.alleles]
        for t, key in enumerate(keys):
            assert np.array_equal(back[key], c.depth[t]) and len(back[key]) == c.length, key
            runs = depthRuns(c.depth[t])
            assert runs[0][0] == 0 and runs[-1][1] == c.length and all(a[1] == b[0] and a[2] != b[2] for a, b in zip(runs, runs[1:]))
        assert len(keys) == 2 + 2 * k
    assert depthRuns(np.zeros(0, dtype=np.uint32)) == [] and depthRuns(np.array([4])) == [(0, 1, 4)]


# ------------------------------------------------------------------------------------------------ arguments
def test_parser_takes_the_call_coverage_flags():
    base = ["--step-skip-extraction", "--alignment", "s.sam"]
    args = cli.createParser().parse_args(base)
    assert args.call_coverage is False and args.call_coverage_depth is False and cli.callReportArgs(args, report="call_coverage") == {}
    args = cli.createParser().parse_args(base + ["--allele-strategy", "exonfirst", "--call-coverage"])
    assert cli.callReportArgs(args, report="call_coverage") == {"call_coverage": True, "call_coverage_depth": False}
    # the depth file implies the report
    args = cli.createParser().parse_args(base + ["--call-coverage-depth"])
    assert cli.callReportArgs(args, report="call_coverage") == {"call_coverage": True, "call_coverage_depth": True}
    # it combines with the fit report and the call bootstrap
    args = cli.createParser().parse_args(base + ["--call-coverage", "--call-fit", "--call-bootstrap", "8"])
    assert cli.callReportArgs(args, report="call_coverage")["call_coverage"] and cli.callReportArgs(args, report="call_fit")["call_fit"]
    assert cli.callReportArgs(args, report="call_bootstrap")["call_bootstrap"] == 8


@pytest.mark.parametrize("extra", [["--allele-strategy", "em", "--call-coverage"],
                                   ["--allele-strategy", "report", "--call-coverage"],
                                   ["--allele-strategy", "em", "--call-coverage-depth"]])
def test_command_line_refuses_the_em_strategy(extra, monkeypatch):
    for name in ("GK_WAIT_POLICY", "GK_SAMPLE_LANES", "GK_SEARCH_SLOTS"):      # main() sets its defaults: put them back
        monkeypatch.setenv(name, os.environ.get(name, "1"))
    args = cli.createParser().parse_args(["--step-skip-extraction", "--alignment", "no_such_sample.sam"] + extra)
    with pytest.raises(ValueError, match="--call-coverage"):       # before any sample is read
        cli.main(args)


def test_factory_refusals():
    from kir_graph_amd.kir_typing import TypingWithPosNegAllele, TypingWithReport, selectKirTypingModel
    for method in ("em", "report"):
        with pytest.raises(ValueError, match="call_coverage"):
            selectKirTypingModel(method, "nothing.json", call_coverage=True, call_coverage_len={"G": 10})
    with pytest.raises(TypeError):
        TypingWithReport("nothing.json", call_coverage=True)
    # without the lengths: refused before the sample is touched
    for lengths in (None, {}):
        with pytest.raises(ValueError, match="call_coverage_len"):
            TypingWithPosNegAllele("nothing.json", call_coverage=True, call_coverage_len=lengths)
    with pytest.raises(ValueError, match="call_coverage_len"):
        selectKirTypingModel("exonfirst", "nothing.json", call_coverage=True)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_hand_built_records():
    from kir_graph_amd._lib import MATE_DTYPE
    rec = np.zeros(6, dtype=MATE_DTYPE)

    def mate(i, pos0, ref, ops):
        rec[i]["pos0"], rec[i]["ref"], rec[i]["n_cig"] = pos0, ref, len(ops)
        for j, (op, n) in enumerate(ops):
            rec[i]["cig"][j] = (n << 4) | op
    M, I, D, S = 0, 1, 2, 4
    mate(0, 2, 0, [(S, 3), (M, 4), (I, 2), (M, 1), (D, 3), (M, 2)])      # 2..6, 6..7, 10..12
    mate(1, 9, 0, [(M, 5)])                                              # 9..14 -> clipped at 13
    mate(2, 0, 0, [(M, 2)])
    mate(3, 20, 0, [(M, 5)])                                             # wholly beyond the end
    mate(4, 1, 1, [(M, 9)])                                              # another backbone: marks nothing
    mate(5, 4, 0, [(M, 3)])
    assert cr.mateRuns(rec[0]) == [(2, 6), (6, 7), (10, 12)]
    table = np.array([[0, 2, 1],           # column 0
                      [0, 5, 0],           # column 1 (not listed)
                      [0, 1, 255]])        # column 2
    # rows: pair 1 ties with m1 = 0, pair 0 is best on column 2 alone with m1 = 1, pair 2 on column 0 alone with m1 = 1
    got = cr.tracks(rec, pair_src=np.array([0, 1, 2]), rows=[1, 0, 2], table=table, cols=[0, 2], gene=0, gene_len=13)
    one = lambda *spans: np.sum([np.isin(np.arange(13), np.arange(a, b)) for a, b in spans], axis=0)      # noqa: E731
    pair0, pair1, pair2 = one((2, 7), (10, 12), (9, 13)), one((0, 2)), one((4, 7))
    assert got.shape == (6, 13)
    assert got[0].tolist() == (pair0 + pair1 + pair2).tolist()
    assert got[1].tolist() == (pair0 + pair2).tolist()
    assert got[2].tolist() == (pair1 + pair2).tolist() and got[3].tolist() == (pair1 + pair0).tolist()
    assert got[4].tolist() == pair2.tolist() and got[5].tolist() == pair0.tolist()


def test_restatement_agrees_with_the_depth_oracle(small_case):
    """Track 0 with every row listed and a table of zeros is the depth of those pairs."""
    sidx, gidx, sample = small_case
    lines = synth.toSamLines(sample)
    pairs = list(pairLines(lines))
    assert len(pairs) == len(list(ot.pairMates(lines)))
    rec, _ = packed.packPairs(pairs, gidx)
    gene_len = {g: len(sidx.backbone[g]) for g in sidx.genes}
    gname = gidx.genes[1]
    g = gidx.gene_id[gname]
    rows = [p for p, (l, r) in enumerate(ot.pairMates(lines))
            if ot.passesFilter(l) and ot.passesFilter(r) and ot.nhOf(l) == 1 and l.split("\t")[2] == gname]
    assert len(rows) > 100
    kept = [(l, r, 1) for p, (l, r) in enumerate(ot.pairMates(lines)) if p in set(rows)]
    want = odepth.depthFromPairs(kept, gene_len)
    assert want[gname].sum() > 0 and not any(want[o].any() for o in gene_len if o != gname)
    cigars = "".join(l.split("\t")[5] for pair in kept for l in pair[:2])
    assert "I" in cigars and "D" in cigars and "S" in cigars       # the walk meets every operation
    table = np.zeros((1, len(rows)), dtype=np.uint8)
    for length in (gene_len[gname], 37, 1):
        got = cr.tracks(rec, np.arange(len(pairs)), rows, table, [0], g, length)
        assert np.array_equal(got[0], want[gname][:length]) and np.array_equal(got[2], got[0]) and np.array_equal(got[3], got[0])
        assert not got[1].any()
