"""Novel-variant discovery on the device (csrc/gk_novel.hip, kir_graph_amd/novel_discover.py): the restricted products
against the full table, the device assignment and confusion against the reference's list helpers, and the command
line's ``--novel-discovery`` end to end."""
import gzip
import os

import numpy as np
import pandas as pd
import pytest

from kir_graph_amd import main as cli, novel_discover as nd, packed, synth
from kir_graph_amd.engine import DeviceIndex, Tabulation
from kir_graph_amd.hisat2 import SampleData
from kir_graph_amd.index import GkIndex
from kir_graph_amd.kir_typing import _GeneView
from kir_graph_amd.typing_mulit_allele import AlleleTyping, ReadSet

pytestmark = pytest.mark.gpu


def _data(device, sidx, sample):
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    rec, table = packed.packSample(sample, gidx)
    tab = Tabulation(DeviceIndex(device, gidx), rec)
    return SampleData(tab, gidx, None, ins_strings=table.strings)


def _hostModel(data, g):
    """The reference's model of one gene: AlleleTyping(NH == 1 reads, variants, no_empty=False), corrected reads."""
    tab = data.tab
    rows, n = tab.selectGene(g, multiple=False)
    view = _GeneView(data, data.index.genes[g], False, tab=tab)
    return AlleleTyping(ReadSet(tab, rows, n), view.variants, no_empty=False, variant_correction=True, _vbeg=view.vbeg,
                        _n_span=view.n_span, _mask=view.mask, _alleles=view.alleles, _novel=view.novel)


def test_restricted_products_equal_the_full_tables_columns(device, small_case):
    from kir_graph_amd._lib import check, lib
    for sidx, sample in ((small_case[0], small_case[2]),
                         (lambda s: (s, synth.makeSample(s, seed=5, n_pairs=3000)))(
                             synth.makeIndex(seed=77, n_genes=3, var_range=(100, 200), allele_range=(40, 70))),):
        data = _data(device, sidx, sample)
        rng = np.random.default_rng(3)
        for g, t in enumerate(data.index.tables):
            typ = _hostModel(data, g)
            full = typ.probs
            if not len(full):
                continue
            cols = rng.choice(len(t.alleles), size=min(5, len(t.alleles)), replace=False)
            carry = np.zeros(max(t.vend - t.vbeg, 1), dtype=np.uint32)
            for k, c in enumerate(cols):
                carry[:t.vend - t.vbeg] |= ((t.mask[:, c >> 5] >> np.uint32(c & 31)) & np.uint32(1)) << np.uint32(k)
            d_carry = device.put(carry)
            rs = typ._readset
            probs = device.alloc((len(cols), rs.n_rows), np.float64)
            check(lib().gk_compat(device.ctx, data.tab.handle, rs.rows.ptr, rs.n_rows, rs.vflag.ptr, t.vbeg, t.vend,
                                  d_carry.ptr, 1, len(cols), 1, probs.ptr, 0, 0))
            got = probs.download().reshape(len(cols), rs.n_rows).T
            assert np.array_equal(got.view(np.uint64), np.ascontiguousarray(full[:, cols]).view(np.uint64)), g
        data.tab.close()


def _calls(rng, index, data):
    """A random call list: alleles of several genes, a duplicated (homozygous) call, a name no gene has."""
    calls = []
    for t in index.tables:
        k = int(rng.integers(1, 4))
        picks = list(rng.choice(t.alleles, size=min(k, len(t.alleles)), replace=False))
        if rng.random() < 0.5:
            picks.append(picks[0])
        calls += picks
    calls.append("KIRX*0000001")
    rng.shuffle(calls)
    return [str(c) for c in calls]


@pytest.mark.parametrize("seed", [None, 11, 12, 13])
def test_device_groups_and_counts_equal_the_reference_helpers(device, small_case, seed):
    if seed is None:
        sidx, _, sample = small_case
    else:
        sidx = synth.makeIndex(seed=seed, n_genes=3, var_range=(150, 300), allele_range=(10, 30))
        sample = synth.makeSample(sidx, seed=seed + 100, n_pairs=3000)
    data = _data(device, sidx, sample)
    rng = np.random.default_rng(seed or 1)
    calls = _calls(rng, data.index, data)
    genes = nd.NovelDiscovery(data).run(calls)
    # the genes in order of first appearance among the NH == 1 rows
    gene_of, nh = data.tab.pairGene(), data.tab.pairNH()
    order = list(dict.fromkeys(int(g) for g, h in zip(gene_of, nh) if h == 1))
    assert [gg.gene for gg in genes] == [data.index.genes[g] for g in order]
    for gg, g in zip(genes, order):
        typ = _hostModel(data, g)
        reads = typ.reads
        want = nd.groupReadByAllele(typ, calls, reads)
        assert gg.groups == list(want), gg.gene
        assert gg.sizes == [len(r) for r in want.values()], gg.gene
        for group, rs in want.items():
            if len(group) > 1:
                continue
            assert gg.totals[group] == nd.statNovelConfusion(group[0], rs, typ.variants), (gg.gene, group)
            cand = nd.extractNovelVariant(group[0], rs, typ.variants)
            want_c = [(stat, v.id, c) for stat in ("novel", "fp", "fn") for v, c in cand[stat].items()]
            assert [(s, v.id, c) for s, v, c in gg.candidates[group]] == want_c, (gg.gene, group)
    data.tab.close()


def test_command_line_novel_discovery_finds_a_planted_snv(device, tmp_path, monkeypatch):
    """One SNV of a called allele is taken out of the index: its reads then carry a novel variant there, which
    ``--novel-discovery`` lists, confirms by the pileup, applies and names; the grouped BAM tags every pair.
    The same run without the flag writes the same typing files and no ``.novel.*`` file."""
    monkeypatch.chdir(tmp_path)
    sidx = synth.makeIndex(seed=21, n_genes=15, var_range=(60, 120), allele_range=(6, 12), len_range=(2500, 4000))
    cn = {g: (1 if k == 4 else (2 if "3DL3" in g else 0)) for k, g in enumerate(sidx.genes)}
    sample = synth.makeSample(sidx, seed=70, n_pairs=6000, gene_cn=cn, err_rate=0.0)
    gene = sidx.genes[4]
    allele = sample.truth[gene][0]
    planted = next(v for v in sidx.variants if v.ref == gene and v.typ == "single" and allele in v.allele
                   and 1000 < v.pos < len(sidx.backbone[gene]) - 1000)
    folder = tmp_path / "index"
    folder.mkdir()
    prefix = str(folder / "kir_2100_withexon_ab_2dl1s1.leftalign.mut01")
    reduced = synth.SynthIndex(genes=sidx.genes, backbone=sidx.backbone,
                               variants=[v for v in sidx.variants if v is not planted], exons=sidx.exons,
                               alleles=sidx.alleles)
    reduced.write(prefix)
    reduced.writeBackbone(prefix)
    sam = tmp_path / "s0.sam.gz"
    with gzip.open(sam, "wt") as f:
        f.write("@HD\tVN:1.0\tSO:queryname\n" + "".join(f"@SQ\tSN:{g}\tLN:{len(sidx.backbone[g])}\n" for g in sidx.genes)
                + "\n".join(synth.toSamLines(sample)) + "\n")
    cn_file = tmp_path / "s0.cn.tsv"
    cn_file.write_text("gene\tcn\n" + "".join(f"{g}\t{c}\n" for g, c in cn.items()))

    def run(out, extra):
        args = cli.createParser().parse_args(
            ["--step-skip-extraction", "--index-folder", "index", "--output-folder", str(out), "--allele-strategy",
             "pv", "--alignment", str(sam), "--cn-provided", str(cn_file), "--log-level", "WARNING"] + extra)
        cli.main(args)
        return sorted(p.name for p in out.iterdir())

    on, off = tmp_path / "on", tmp_path / "off"
    names_on, names_off = run(on, ["--novel-discovery"]), run(off, [])
    novel = [n for n in names_on if ".novel." in n]
    assert not any(".novel." in n for n in names_off)
    assert sorted(set(names_on) - set(novel)) == names_off
    for n in names_off:
        if n.endswith((".tsv",)) and ".depth." not in n:
            assert (on / n).read_text().replace(str(on), "@") == (off / n).read_text().replace(str(off), "@"), n
    stem = [n for n in novel if n.endswith(".novel.variant.tsv")]
    assert len(stem) == 1
    stem = stem[0][:-len(".variant.tsv")]
    for ext in (".variant.tsv", ".tsv", ".fa", ".bam", ".bam.bai", ".txt"):
        assert stem + ext in novel, ext
    table = pd.read_csv(on / (stem + ".variant.tsv"), sep="\t")
    hit = table[(table["type"] == "novel") & (table["pos"] == planted.pos) & (table["gene"] == gene)]
    assert len(hit) == 1, table.to_string()
    row = hit.iloc[0]
    assert not row["skip"] and row["count"] >= 3 and row["variant_val"] == planted.val
    assert row["base_alt"] == planted.val and row["pileup"].startswith("Counter(")
    pile = eval(row["pileup"], {"Counter": dict})
    assert pile[planted.val] == max(pile.values())
    called = pd.read_csv(on / (stem + ".tsv"), sep="\t")["alleles"][0].split("_")
    named = [a for a in called if a.startswith(row["allele"])]
    assert named and f"-{planted.pos}{planted.val}" in named[0]
    fa = (on / (stem + ".fa")).read_text().split(">")[1:]
    rec = next(r for r in fa if r.startswith(named[0]))
    seq = "".join(rec.splitlines()[1:])
    assert f"{row['allele']}:{planted.pos}" in rec.splitlines()[0]
    # the applied base, where the gapless sequence puts that position (no indel of the allele before it here)
    before = [v for v in reduced.variants if v.ref == gene and row["allele"] in v.allele and v.pos < planted.pos
              and v.typ != "single"]
    if not before:
        assert seq[planted.pos] == planted.val
    head = packed.bamHeader(str(on / (stem + ".bam")))
    rgs = [line for line in head.splitlines() if line.startswith("@RG")]
    body = [line for line in b"".join(packed.bamChunks(str(on / (stem + ".bam")))).decode().splitlines()
            if line and not line.startswith("@")]
    assert rgs and body
    tags = {line.rsplit("\t", 1)[1] for line in body}
    assert all(t.startswith("RG:Z:") for t in tags)
    assert {t[len("RG:Z:"):] for t in tags} <= {r.split("ID:", 1)[1] for r in rgs}
    assert len(body) % 2 == 0


def _rg_name_pairs(bam):
    """(@RG ids in header order, {query name: set of RG tags of its lines}) of a BAM."""
    head = packed.bamHeader(bam)
    rgs = [line.split("ID:", 1)[1] for line in head.splitlines() if line.startswith("@RG")]
    tags: dict[str, list[str]] = {}
    for line in b"".join(packed.bamChunks(bam)).decode().splitlines():
        if line and not line.startswith("@"):
            tags.setdefault(line.split("\t", 1)[0], []).append(line.rsplit("\t", 1)[1])
    return rgs, tags


def test_discover_sample_with_indel_candidates_and_the_grouped_bam(device, tmp_path):
    """Through discoverSample on a sample in HBM: the called allele is given an insertion it lacks (its reads hold the
    insertion's id in their negative lists: fn) and loses a deletion it has (fp), and one of its SNVs leaves the index
    (novel).  Indel candidates get ALT "" and are filtered, never asserted on; the SNV is applied.  The grouped BAM has
    one @RG per device group, in order, and both lines of every pair carry the tag of the group the device gave it."""
    import dataclasses
    from kir_graph_amd.hisat2 import extractVariantFromText, saveReadsToBam
    sidx = synth.makeIndex(seed=21, n_genes=15, var_range=(60, 120), allele_range=(6, 12), len_range=(2500, 4000))
    cn = {g: (1 if k == 4 else (2 if "3DL3" in g else 0)) for k, g in enumerate(sidx.genes)}
    sample = synth.makeSample(sidx, seed=70, n_pairs=6000, gene_cn=cn, err_rate=0.0)
    gene = sidx.genes[4]
    allele = sample.truth[gene][0]
    inner = lambda v: v.ref == gene and 300 < v.pos < len(sidx.backbone[gene]) - 300      # noqa: E731
    ins = next(v for v in sidx.variants if inner(v) and v.typ == "insertion" and allele not in v.allele)
    dele = next(v for v in sidx.variants if inner(v) and v.typ == "deletion" and allele in v.allele)
    snv = next(v for v in sidx.variants if inner(v) and v.typ == "single" and allele in v.allele)
    variants = []
    for v in sidx.variants:
        if v is snv:
            continue
        if v is ins:
            v = dataclasses.replace(v, allele=v.allele + [allele])
        elif v is dele:
            v = dataclasses.replace(v, allele=[a for a in v.allele if a != allele])
        variants.append(v)
    reduced = synth.SynthIndex(genes=sidx.genes, backbone=sidx.backbone, variants=variants, exons=sidx.exons,
                               alleles=sidx.alleles)
    prefix = str(tmp_path / "idx")
    reduced.write(prefix)
    reduced.writeBackbone(prefix)
    gidx = GkIndex.load(prefix)
    sam = str(tmp_path / "s.sam")
    with open(sam, "w") as f:
        f.write("@HD\tVN:1.0\tSO:queryname\n" + "".join(f"@SQ\tSN:{g}\tLN:{len(sidx.backbone[g])}\n" for g in sidx.genes)
                + "\n".join(synth.toSamLines(sample)) + "\n")
    data = extractVariantFromText(sam, gidx, dev=device, keep_text=True)
    saveReadsToBam(data, str(tmp_path / "s.no_multi"), sam, filter_multi_mapped=True)
    calls = [allele] + [a for g in sidx.genes if g != gene for a in sample.truth.get(g, [])]
    genes = nd.NovelDiscovery(data).run(calls)
    out = str(tmp_path / "s.novel")
    rows = nd.discoverSample(data, calls, prefix, str(tmp_path / "s.no_multi.bam"), out)
    by_id = {r["variant_id"]: r for r in rows if r["gene"] == gene}
    assert ins.id in by_id and by_id[ins.id]["type"] == "fn" and by_id[ins.id]["count"] >= 3, by_id.get(ins.id)
    assert dele.id in by_id and by_id[dele.id]["type"] == "fp" and by_id[dele.id]["count"] >= 3, by_id.get(dele.id)
    r = by_id[ins.id]       # the reads have bases there: the candidate reaches the REF / ALT step
    assert r["skip"] and r["base_alt"] == "" and r["skip_reason"] == "ALT depths < REF depths", r
    r = by_id[dele.id]      # every read of the group deletes the position: no base in the pileup
    assert r["skip"] and r["base_alt"] == "" and r["skip_reason"] in ("Pileup empty", "ALT depths < REF depths"), r
    hit = [r for r in rows if r["type"] == "novel" and r["pos"] == snv.pos and r["gene"] == gene]
    assert len(hit) == 1 and not hit[0]["skip"] and hit[0]["base_alt"] == snv.val
    table = pd.read_csv(out + ".variant.tsv", sep="\t", keep_default_na=False)
    assert len(table) == len(rows)
    assert f"{allele}-{snv.pos}{snv.val}" in pd.read_csv(out + ".tsv", sep="\t")["alleles"][0].split("_")
    # the grouped BAM against the device's groups
    rgs, tags = _rg_name_pairs(out + ".bam")
    assert rgs == [",".join(g) for gg in genes for g in gg.groups]
    text, src = nd._pairsText(data)
    want: dict[str, str] = {}
    for gg in genes:
        for group, ec, size in zip(gg.groups, gg.codes, gg.sizes):
            members = gg.rows[gg.row_code == ec]
            assert len(members) == size
            for r in members:
                want[text[int(src[r])][0].split("\t", 1)[0]] = "RG:Z:" + ",".join(group)
    assert {n: sorted(t) for n, t in tags.items()} == {n: [t, t] for n, t in want.items()}
    data.tab.close()


def test_a_million_pairs_without_the_full_table_or_host_reads(device, monkeypatch):
    """1 M pairs with ``AlleleTyping.probs`` / ``.log_probs`` / ``.reads`` patched to raise: the discovery completes on
    the device, and its group sizes and totals equal a vectorised numpy restatement built from the downloaded CSR
    (products in list order, exact maxima, the corrected lists)."""
    def boom(self):
        raise AssertionError("novel discovery touched the full table or host reads")
    for name in ("probs", "log_probs", "reads"):
        monkeypatch.setattr(AlleleTyping, name, property(boom))
    sidx = synth.makeIndex(seed=31, n_genes=3, var_range=(200, 400), allele_range=(20, 40))
    sample = synth.makeSample(sidx, seed=32, n_pairs=1_000_000)
    data = _data(device, sidx, sample)
    calls = []
    for g in sidx.genes:
        t = sample.truth.get(g, [])
        calls += list(t) + list(t[:1])                  # the truth and a duplicate of its first allele
    calls.append(sidx.alleles[sidx.genes[0]][-1])
    genes = nd.NovelDiscovery(data).run(calls)
    tab, idx = data.tab, data.index
    off, ids = tab.offsets().astype(np.int64), tab.ids().astype(np.int64)
    gene_of, nh = tab.pairGene(), tab.pairNH()
    vflag = tab.prepared(tab.dev, False)[0].download()
    seen = 0
    for gg in genes:
        g = idx.gene_id[gg.gene]
        t = idx.tables[g]
        col_of = {a: i for i, a in enumerate(t.alleles)}
        entries = [a for a in calls if a in col_of]
        if not entries:
            continue
        distinct = list(dict.fromkeys(entries))
        rows = np.flatnonzero((gene_of == g) & (nh == 1))
        assert np.array_equal(rows, gg.rows)
        # the rows' kept ids, flat, in list order
        b, m, e = off[4 * rows], off[4 * rows + 2], off[4 * rows + 4]
        lens = e - b
        flat = np.repeat(b - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens) + np.arange(lens.sum())
        row_of = np.repeat(np.arange(len(rows)), lens)
        v = ids[flat]
        pos = flat < np.repeat(m, lens)
        keep = (vflag[v] & np.where(pos, 1, 2)) == 0
        v, pos, row_of = v[keep], pos[keep], row_of[keep]
        local = v - t.vbeg
        inspan = (local >= 0) & (local < t.vend - t.vbeg)
        n_kept = np.bincount(row_of, minlength=len(rows))
        starts = np.concatenate([[0], np.cumsum(n_kept)[:-1]])
        prod = np.empty((len(rows), len(distinct)))
        carries = []
        for k, a in enumerate(distinct):
            c = col_of[a]
            carry = np.zeros(len(v), dtype=bool)
            carry[inspan] = (t.mask[local[inspan], c >> 5] >> np.uint32(c & 31)) & 1 == 1
            carries.append(carry)
            factor = np.where(carry == pos, 0.999, 0.001)
            # one factor 1.0 behind the last: rows without a kept id may start there (and take 0.999 below)
            p = np.multiply.reduceat(np.append(factor, 1.0), starts)
            prod[:, k] = np.where(n_kept > 0, p, 0.999)
        is_max = prod == prod.max(axis=1)[:, None]
        dcode = (is_max * (1 << np.arange(len(distinct)))).sum(axis=1)
        sizes = {}
        for dc in np.unique(dcode):
            group = tuple(sorted(a for a in entries if dc >> distinct.index(a) & 1))
            sizes[group] = int((dcode == dc).sum())
        assert dict(zip(gg.groups, gg.sizes)) == sizes, gg.gene
        for group in gg.groups:
            if len(group) > 1:
                continue
            k = distinct.index(group[0])
            in_group = (dcode == (1 << k))[row_of]
            carry = carries[k]
            tot = {"novel": int((in_group & ~inspan).sum()),
                   "tp": int((in_group & inspan & pos & carry).sum()),
                   "tn": int((in_group & inspan & ~pos & ~carry).sum()),
                   "fp": int((in_group & inspan & pos & ~carry).sum()),
                   "fn": int((in_group & inspan & ~pos & carry).sum())}
            tot = {"total": tot["tp"] + tot["tn"] + tot["fp"] + tot["fn"], **tot}
            assert gg.totals[group] == tot, (gg.gene, group)
            seen += 1
    assert seen >= 2
    tab.close()


def test_device_groups_and_counts_equal_the_reference_fixture(device, tmp_path, monkeypatch):
    """tests/golden/t13_novel.json.gz, made by the reference's own splitReadsByAlleles / statNovelConfusion /
    extractNovelVariant (tests/golden/make_golden_novel.py): per call list, every group in order with its member reads
    by query name, and for the singleton groups the confusion totals and the (stat, id, count) lists in order."""
    import json
    from kir_graph_amd.hisat2 import extractVariantFromText
    with gzip.open(os.path.join(os.path.dirname(__file__), "golden", "t13_novel.json.gz"), "rt") as f:
        t13 = json.load(f)
    prefix = str(tmp_path / "ix")
    for ext, body in t13["index"].items():
        with open(f"{prefix}.{ext}", "w") as f:
            f.write(body)
    sam = str(tmp_path / "s.sam")
    with open(sam, "w") as f:
        f.write(t13["header"] + "\n".join(t13["lines"]) + "\n")
    from kir_graph_amd.msa2hisat import Variant
    monkeypatch.setattr(Variant, "novel_id", 0)      # the fixture's first novel id, as the generator set it
    data = extractVariantFromText(sam, GkIndex.load(prefix), dev=device, keep_text=True)
    text, src = nd._pairsText(data)
    kinds = set()
    for case in t13["cases"]:
        genes = nd.NovelDiscovery(data).run(case["calls"])
        got = []
        for gg in genes:
            for group, ec in zip(gg.groups, gg.codes):
                members = gg.rows[gg.row_code == ec]
                entry = {"gene": gg.gene, "alleles": list(group),
                         "reads": [text[int(src[r])][0].split("\t", 1)[0] for r in members]}
                if len(group) == 1:
                    entry["confusion"] = gg.totals[group]
                    entry["candidates"] = [[s, v.id, c] for s, v, c in gg.candidates[group]]
                    kinds |= {s for s, _, _ in gg.candidates[group]}
                got.append(entry)
        assert got == case["groups"], case["calls"]
    assert kinds == {"novel", "fp", "fn"}
    data.tab.close()
