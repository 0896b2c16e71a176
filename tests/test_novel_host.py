"""Novel-variant discovery (kir_graph_amd/novel_discover.py) without a GPU: the list-taking helpers against the
reference's rules (novel_discover.py:48-213), allele sequences from the index, the site pileup against a Python
restatement of its rules, the grouped BAM, and the command line's flag check."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

from kir_graph_amd import novel_discover as nd
from kir_graph_amd.hisat2 import PairRead
from kir_graph_amd.msa2hisat import Variant


def _v(vid, pos, typ="single", val="A", alleles=(), ref="G*BACKBONE"):
    return Variant(pos=pos, typ=typ, ref=ref, val=val, id=vid, allele=list(alleles))


def _typ(probs, alleles):
    return SimpleNamespace(probs=np.asarray(probs, dtype=np.float64), allele_to_id={a: i for i, a in enumerate(alleles)})


def test_group_read_by_allele_keeps_duplicates_ties_and_first_appearance_order():
    alleles = ["G*001", "G*002", "G*003"]
    p, q = 0.999 * 0.001, 0.999 * 0.999
    probs = [[p, q, p],      # G*002
             [q, q, p],      # exact tie G*001 / G*002
             [q, p, p],      # G*001
             [p, p, p],      # all equal (a read with no id left scores 0.999 everywhere)
             [p, q, q]]
    reads = [PairRead(l_sam=f"r{i}") for i in range(len(probs))]
    # a homozygous call and a call the gene does not know
    got = nd.groupReadByAllele(_typ(probs, alleles), ["G*002", "X*009", "G*001", "G*002"], reads)
    assert list(got) == [("G*002", "G*002"), ("G*001", "G*002", "G*002"), ("G*001",)]
    assert [[r.l_sam for r in rs] for rs in got.values()] == [["r0", "r4"], ["r1", "r3"], ["r2"]]
    assert nd.groupReadByAllele(_typ(probs, alleles), ["X*001"], reads) == {}


def test_confusion_and_candidates_follow_the_reference_order():
    variants = {"v1": _v("v1", 10, alleles=["G*001"]), "v2": _v("v2", 20, alleles=["G*002"]),
                "v3": _v("v3", 30, alleles=["G*001", "G*002"]), "nv0": _v("nv0", 40, val="T"),
                "nv1": _v("nv1", 50, val="C")}
    reads = [PairRead(lpv=["v2", "nv1"], rpv=["v1"], lnv=["v3", "nv0"], rnv=["v2"]),
             PairRead(lpv=[], rpv=["v2"], lnv=[], rnv=["nv0", "v3"]),
             PairRead()]
    conf = nd.variantConfusionInRead(reads[0], "G*001", variants)
    assert conf == {"novel": ["nv1", "nv0"], "tp": ["v1"], "tn": ["v2"], "fp": ["v2"], "fn": ["v3"]}
    assert nd.statNovelConfusion("G*001", reads, variants) == {"total": 6, "novel": 3, "tp": 1, "tn": 1, "fp": 2, "fn": 2}
    cand = nd.extractNovelVariant("G*001", reads, variants)
    assert list(cand) == ["novel", "fp", "fn"]
    assert [(v.id, c) for v, c in cand["novel"].items()] == [("nv1", 1), ("nv0", 2)]
    assert [(v.id, c) for v, c in cand["fp"].items()] == [("v2", 2)]
    assert [(v.id, c) for v, c in cand["fn"].items()] == [("v3", 2)]


def test_allele_sequence_from_the_index():
    backbone = "ACGTACGTACGT"
    variants = [_v("a", 2, val="T", alleles=["G*001"]), _v("b", 5, "deletion", 3, alleles=["G*001", "G*002"]),
                _v("c", 9, "insertion", "GG", alleles=["G*001"]), _v("d", 2, val="A", alleles=["G*002"])]
    seq, ins = nd.alleleSequence(backbone, variants, "G*001")
    assert seq == "ACTTA---ACGT" and ins == {9: "GG"}
    assert nd.gaplessSequence(seq, ins) == "ACTTA" + "A" + "GG" + "CGT"
    seq2, ins2 = nd.alleleSequence(backbone, variants, "G*002")
    assert seq2 == "ACATA---ACGT" and ins2 == {}


def _nv(typ, v, count=5):
    return {"gene": "G*BACKBONE", "allele": "G*001", "allele_count": 1, "type": typ, "variant": v, "pos": v.pos,
            "count": count, "skip": False, "skip_reason": "", "base_ref": "", "base_alt": "", "pileup": {}}


def test_ref_alt_apply_and_names():
    backbone = "ACGTACGTACGT"
    allele_seq = "ACTTA---ACGT"
    novel = _nv("novel", _v("nv3", 0, val="G"))
    fn = _nv("fn", _v("a", 2, val="T"))
    fp_del_covered = _nv("fp", _v("x", 6, val="C"))       # a position the allele deletes: REF is "-"
    indel = _nv("novel", _v("nv4", 10, "deletion", 1))
    for nv in (novel, fn, fp_del_covered, indel):
        nd.updateBaseRefAlt(nv, backbone, allele_seq)
    assert (novel["base_ref"], novel["base_alt"]) == ("A", "G")
    assert (fn["base_ref"], fn["base_alt"]) == ("T", "G")
    assert (fp_del_covered["base_ref"], fp_del_covered["base_alt"]) == ("-", "C")
    assert (indel["base_ref"], indel["base_alt"]) == ("G", "")
    out = nd.applyNovelVariant(backbone, allele_seq, [novel, fn, fp_del_covered, indel])
    assert out == "GCGTA-C-ACGT"
    assert indel["skip"] and indel["skip_reason"] == "Not implement indel"
    kept = [nv for nv in (novel, fn, fp_del_covered, indel) if not nv["skip"]]
    assert "G*001" + "".join(f"-{nv['pos']}{nv['base_alt']}" for nv in kept) == "G*001-0G-2G-6C"


# ---- site pileup: hand-made reads against a restatement of the rules in csrc/gk_bamread.cpp
REF = "ACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTACGTAC" * 4


def _sam(name, flag, pos1, cigar, seq, qual):
    return "\t".join([name, str(flag), "G*BACKBONE", str(pos1), "60", cigar, "=", str(pos1), "0", seq, qual])


def _records():
    """(SAM line, group of its name) -- every case the rules distinguish."""
    q = "I" * 20
    low = "I" * 5 + "+" + "I" * 14        # '+' = Q10 at read offset 5
    return [
        (_sam("a1", 99, 1, "20M", REF[0:20], q), 0),
        (_sam("a1", 147, 6, "20M", REF[5:10] + "T" + REF[11:25], q), 0),     # mates overlap site 10, bases differ
        (_sam("b1", 99, 3, "20M", REF[2:20] + "GG", q), 0),
        (_sam("b1", 147, 9, "20M", REF[8:28], q), 0),                          # mates overlap, equal bases
        (_sam("c1", 99, 6, "20M", REF[5:25], low), 0),                         # base below Q13 at site 10
        (_sam("c1", 147, 40, "20M", REF[39:59], q), 0),
        (_sam("d1", 65, 2, "20M", REF[1:21], q), 0),                           # orphan: paired, not proper
        (_sam("e1", 99, 4, "5M2D13M", REF[3:8] + REF[10:23], q[:18]), 0),      # deletes site 9 and 10
        (_sam("f1", 99, 8, "20M", REF[7:27], q), 1),                           # another group
        (_sam("g1", 1123, 8, "20M", REF[7:27], q), 0),                         # duplicate
        (_sam("h1", 99, 10, "3S17M", "TTT" + REF[9:26], q), 0),
    ]


def _restate(records, sites, groups):
    """The pileup rules restated: flags, orphans, overlapping mates, Q13, last record of a name wins, one group."""
    def cover(line, pos):
        f = line.split("\t")
        p, cig, seq, qual = int(f[3]) - 1, f[5], f[9], f[10]
        import re
        ri = 0
        for n, op in re.findall(r"(\d+)([MIDNSHP=X])", cig):
            n = int(n)
            if op in "M=X":
                if p <= pos < p + n:
                    return seq[ri + pos - p], ord(qual[ri + pos - p]) - 33, False
                p += n; ri += n
            elif op in "DN":
                if p <= pos < p + n:
                    return ("*", 0, True) if op == "D" else None
                p += n
            elif op in "IS":
                ri += n
        return None
    out = []
    for (ref, pos), grp in zip(sites, groups):
        col = []
        for line, g in records:
            flag = int(line.split("\t")[1])
            if flag & (4 | 256 | 512 | 1024) or (flag & 1 and not flag & 2):
                continue
            e = cover(line, pos)
            if e is None:
                continue
            col.append([line.split("\t")[0], g, *e])
        seen = {}
        for i, e in enumerate(col):
            if e[0] not in seen:
                seen[e[0]] = i
                continue
            a, b = col[seen.pop(e[0])], e
            if not a[4] and not b[4]:
                if a[2] == b[2]:
                    a[3], b[3] = min(200, a[3] + b[3]), 0
                elif a[3] >= b[3]:
                    a[3], b[3] = int(0.8 * a[3]), 0
                else:
                    a[3], b[3] = 0, int(0.8 * b[3])
        base = {}
        for name, g, b, qv, is_del in col:
            if g != grp:
                continue
            if is_del:
                base.setdefault(name, "*")
            elif qv >= 13:
                base[name] = b
        c = dict.fromkeys("ACGTN*", 0)
        for b in base.values():
            c[b] += 1
        out.append([c[k] for k in "ACGTN*"])
    return np.array(out, dtype=np.uint32)


def test_site_pileup_against_its_rules_with_and_without_the_index(tmp_path):
    from kir_graph_amd import packed
    recs = _records()
    header = "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:G*BACKBONE\tLN:200\n"
    path = str(tmp_path / "x.bam")
    packed.writeBam(path, header + "".join(line + "\n" for line, _ in recs))
    assert os.path.exists(path + ".bai")
    bare = str(tmp_path / "bare.bam")
    with open(path, "rb") as src, open(bare, "wb") as dst:
        dst.write(src.read())
    sites = [(0, 10), (0, 9), (0, 5), (0, 45), (0, 150), (0, 12)]
    groups = [0, 0, 0, 0, 0, 1]
    names = sorted({line.split("\t")[0]: g for line, g in recs}.items())
    keys = np.array([nd.nameKey(n) for n, _ in names], dtype=np.uint64)
    key_group = np.array([g for _, g in names], dtype=np.int32)
    want = _restate(recs, sites, groups)
    with_index = nd.pileupSites(path, np.array(sites), keys, key_group, np.array(groups))
    linear = nd.pileupSites(bare, np.array(sites), keys, key_group, np.array(groups))
    assert with_index.tolist() == want.tolist()
    assert linear.tolist() == want.tolist()
    # the cases are really there: at site 10 a1's disagreeing mates count once (its T loses), b1's agreeing mates
    # once, c1's Q10 base not at all, the orphan and the duplicate never; e1 deletes site 9
    assert want[0].tolist() == [0, 0, 4, 0, 0, 0]
    assert want[1].tolist() == [0, 4, 0, 0, 0, 1]
    assert want[4].tolist() == [0] * 6                     # nothing covers the site
    assert want[5].sum() == 1                              # group 1 sees its own read only


def test_name_keys_are_fnv1a_of_the_query_name():
    from kir_graph_amd.hisat2 import PairsText
    lines = ["r1\t99\tG\t1", "read/2\t147", "x"]
    text = PairsText(("\n".join(lines) + "\n").encode(), np.array([[0, 1]]))
    got = nd.nameKeys(text, np.array([0, 1, 2]))
    assert got.tolist() == [nd.nameKey("r1"), nd.nameKey("read/2"), nd.nameKey("x")]


def test_grouped_bam_has_one_read_group_per_group_and_every_line_tagged(tmp_path):
    from kir_graph_amd import packed
    recs = [line for line, _ in _records()]
    header = "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:G*BACKBONE\tLN:200\n"
    src = str(tmp_path / "in.bam")
    packed.writeBam(src, header + "".join(r + "\n" for r in recs))
    reads = {("G*001",): [PairRead(l_sam=recs[0], r_sam=recs[1])],
             ("G*001", "G*002"): [PairRead(l_sam=recs[2], r_sam=recs[3]), PairRead(l_sam=recs[4], r_sam=recs[5])]}
    out = str(tmp_path / "out.bam")
    nd.groupReadToBam(src, out, reads)
    assert os.path.exists(out + ".bai")
    head = packed.bamHeader(out)
    assert head.endswith("@RG\tID:G*001\n@RG\tID:G*001,G*002\n")
    body = b"".join(packed.bamChunks(out)).decode().splitlines()
    body = [b for b in body if not b.startswith("@")]
    assert len(body) == 6
    tags = sorted(line.rsplit("\t", 1)[1] for line in body)
    assert tags == ["RG:Z:G*001"] * 2 + ["RG:Z:G*001,G*002"] * 4
    assert sorted(line.rsplit("\t", 1)[0] for line in body) == sorted(recs[:6])


def test_novel_discovery_without_variant_json_is_rejected_by_the_parser():
    from kir_graph_amd.main import createParser
    assert createParser().parse_args(["--novel-discovery"]).novel_discovery
    with pytest.raises(SystemExit):
        createParser().parse_args(["--novel-discovery", "--no-variant-json"])


def test_site_pileup_seeks_across_blocks_and_windows(tmp_path):
    """Thousands of pairs over 60 kb: the BAM spans many BGZF blocks and 16 kb windows of the index; sites in every
    window, three groups, random qualities, orphans, duplicates and deletions.  The .bai seek, the read-through of the
    same file without its index and the restated rules agree at every site."""
    from kir_graph_amd import packed
    rng = np.random.default_rng(5)
    ref = "".join(rng.choice(list("ACGT"), size=60000))
    recs = []
    for k in range(3000):
        name, grp = f"p{k}", int(rng.integers(0, 3))
        p1 = int(rng.integers(0, 59700))
        p2 = min(p1 + int(rng.integers(0, 120)), 59800)
        flag1, flag2 = 99, 147
        if rng.random() < 0.05:
            flag1, flag2 = 65, 129                      # orphans
        if rng.random() < 0.03:
            flag1 |= 1024                               # a duplicate mate
        for pos, flag in ((p1, flag1), (p2, flag2)):
            seq = list(ref[pos:pos + 100])
            for j in rng.integers(0, 100, size=2):
                seq[j] = "ACGT"[int(rng.integers(0, 4))]
            qual = "".join(chr(33 + int(q)) for q in rng.choice([5, 12, 13, 30, 40], size=100))
            if rng.random() < 0.1:                      # a 3-base deletion after 50 bases
                cig, seq, qual = "50M3D47M", seq[:50] + list(ref[pos + 53:pos + 100]), qual[:97]
            else:
                cig = "100M"
            recs.append((_sam(name, flag, pos + 1, cig, "".join(seq), qual), grp))
    recs.sort(key=lambda r: int(r[0].split("\t")[3]))          # the file's (stable, coordinate) order
    header = "@HD\tVN:1.0\tSO:coordinate\n@SQ\tSN:G*BACKBONE\tLN:60000\n"
    path = str(tmp_path / "big.bam")
    packed.writeBam(path, header + "".join(line + "\n" for line, _ in recs))
    assert os.path.getsize(path) > 4 * 65536                    # several BGZF blocks
    bare = str(tmp_path / "big_bare.bam")
    with open(path, "rb") as src, open(bare, "wb") as dst:
        dst.write(src.read())
    sites = [(0, int(p)) for p in np.sort(rng.integers(0, 60000, size=40))]
    groups = [int(g) for g in rng.integers(0, 3, size=len(sites))]
    assert len({p >> 14 for _, p in sites}) >= 3                # sites in several windows
    names = {line.split("\t")[0]: g for line, g in recs}
    keys = np.array([nd.nameKey(n) for n in names], dtype=np.uint64)
    key_group = np.array(list(names.values()), dtype=np.int32)
    want = _restate(recs, sites, groups)
    assert want[:, :5].sum() > 50
    got = nd.pileupSites(path, np.array(sites), keys, key_group, np.array(groups))
    assert got.tolist() == want.tolist()
    assert nd.pileupSites(bare, np.array(sites), keys, key_group, np.array(groups)).tolist() == want.tolist()


def test_indel_candidates_have_no_alt_base_and_do_not_trip_the_snv_check():
    """An insertion the allele carries (fn): in gapless coordinates the allele and the backbone have the same base
    at its position; ALT is "" as for every indel, so the candidate is filtered, not asserted on."""
    backbone = "ACGTACGTACGT"
    ins = _v("i1", 4, "insertion", "TT", alleles=["G*001"])
    dele = _v("d1", 7, "deletion", 2, alleles=["G*002"])
    allele_seq, _ = nd.alleleSequence(backbone, [ins, dele], "G*001")
    for typ, v in (("fn", ins), ("fp", dele), ("novel", _v("nv9", 3, "insertion", "A"))):
        nv = _nv(typ, v)
        nd.updateBaseRefAlt(nv, backbone, allele_seq)
        assert nv["base_alt"] == "" and nv["base_ref"] == allele_seq[v.pos]
        nv["pileup"] = {"A": 3}
        assert nv["pileup"].get(nv["base_alt"], 0) < max(nv["pileup"].values())     # "ALT depths < REF depths"
