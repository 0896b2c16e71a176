"""
Novel-variant discovery after typing -- drop-in for ``graphkir/novel_discover.py``.

1. assign every read of a gene to the called allele(s) that explain it best (``groupReadByAllele``);
2. count, per called allele, the variants its reads disagree with (``novel`` / ``fp`` / ``fn``);
3. keep the frequent ones (>= 3 reads) that the pileup of those reads confirms;
4. write them, the called allele with the confirmed SNVs applied, and the reads grouped by allele as a BAM.

The list-taking helpers keep the reference's names, signatures and semantics and work on ``PairRead`` lists (small
inputs, tests).  ``discoverNovel`` and the command line go through ``NovelDiscovery``, which runs on a sample that is
already in HBM: the products of the called alleles come from ``gk_compat`` restricted to those columns, the assignment
and the confusion counts from ``csrc/gk_novel.hip``; what comes back to the host is per-group totals, the counted
(allele, variant, count, first-seen key) tuples and 2 bytes of group code per read.  The pileup at the candidate sites
(``gk_bam_pileup_sites``) and the grouped BAM (``gk_bam_write_lines_tagged``) are native host code.

Allele sequences come from the HISAT2 index the typing already uses, not from pyhlamsa MSA files: ``{msa_name}_backbone.fa``
and the allele's variants in ``.snp`` / ``.link``.  The base of an allele at backbone position ``p`` is its own
``single`` variant's value at ``p``, ``-`` if one of its deletions covers ``p``, otherwise the backbone base.  These are
the coordinates of the BAM and of ``.snp`` (the gapless backbone).  Two known differences from the reference:

* MSA gap columns are absent (the reference indexes the gapped MSA row by the variant's position);
* the FASTA holds the allele's gapless sequence, its insertions included (inserted before the base at their position),
  with the applied SNVs; the reference wrote the gapped MSA row.  ``Length`` in the description is that sequence's.

One improvement: when no candidate exists at all the reference crashes (``df["variant"]`` on an empty frame); here a
header-only ``.variant.tsv`` is written.
"""
from __future__ import annotations

import ctypes as C
import sys
from collections import Counter, defaultdict
from itertools import chain
from typing import Iterable, TextIO, TypedDict

import numpy as np

from .hisat2 import PairRead
from .msa2hisat import Variant
from .utils import logger

GroupPairRead = dict[tuple[str, ...], list[PairRead]]
STATS = ("novel", "tp", "tn", "fp", "fn")
CANDIDATE_STATS = ("novel", "fp", "fn")
MAX_ENTRIES = 16
COLUMNS = ["gene", "allele", "allele_count", "type", "pos", "count", "skip", "skip_reason", "base_ref", "base_alt",
           "pileup", "variant_type", "variant_id", "variant_val"]


class NovelVariant(TypedDict):
    gene: str
    allele: str
    allele_count: int  # The i'th allele in the gene
    type: str
    variant: Variant
    pos: int
    count: int
    skip: bool
    skip_reason: str
    base_ref: str
    base_alt: str
    pileup: dict[str, int]


# ---- list-taking helpers (novel_discover.py:48-264)
def groupReadByAllele(typ, predict_alleles: list[str], reads: list[PairRead]) -> GroupPairRead:
    """Assign the reads to the called alleles with the largest product (48-70): a read's group is the sorted tuple of
    the called entries (duplicates kept) whose product equals the row maximum exactly; groups in first-appearance order."""
    allele_names, allele_ids = [], []
    for a in predict_alleles:
        if a in typ.allele_to_id:
            allele_names.append(a)
            allele_ids.append(typ.allele_to_id[a])
    if not allele_names:
        return {}
    probs = np.asarray(typ.probs)[:, allele_ids]
    is_max = np.equal(probs, probs.max(axis=1)[:, None])
    names = np.array(allele_names)
    assign: GroupPairRead = defaultdict(list)
    for read, max_id in zip(reads, is_max):
        assign[tuple(sorted(names[max_id]))].append(read)
    return assign


def variantConfusionInRead(read: PairRead, allele: str, variants: dict[str, Variant]) -> dict[str, list[str]]:
    """The read's ids against the allele (73-102): ``nv`` ids are novel; positives tp / fp, negatives fn / tn."""
    out: dict[str, list[str]] = {s: [] for s in STATS}
    for v in chain(read.lpv, read.rpv):
        if v.startswith("nv"):
            out["novel"].append(v)
        else:
            out["tp" if allele in variants[v].allele else "fp"].append(v)
    for v in chain(read.lnv, read.rnv):
        if v.startswith("nv"):
            out["novel"].append(v)
        else:
            out["fn" if allele in variants[v].allele else "tn"].append(v)
    return out


def statNovelConfusion(allele: str, reads: list[PairRead], variants: dict[str, Variant]) -> dict[str, int]:
    """Totals of ``variantConfusionInRead`` over the reads (105-122); ``total = tp + tn + fp + fn``."""
    count = {"total": 0, **{s: 0 for s in STATS}}
    for read in reads:
        for stat, vs in variantConfusionInRead(read, allele, variants).items():
            count[stat] += len(vs)
    count["total"] = count["tp"] + count["tn"] + count["fp"] + count["fn"]
    return count


def extractNovelVariant(allele: str, reads: list[PairRead], variants: dict[str, Variant]) -> dict[str, dict[Variant, int]]:
    """``{stat: {variant: reads}}`` for novel / fp / fn, variants in order of first occurrence (125-144)."""
    lists: dict[str, list[Variant]] = {s: [] for s in CANDIDATE_STATS}
    for read in reads:
        for stat, vs in variantConfusionInRead(read, allele, variants).items():
            if stat in lists:
                lists[stat] += [variants[v] for v in vs]
    return {stat: dict(Counter(vs)) for stat, vs in lists.items()}


def updateBaseRefAlt(variant: NovelVariant, backbone_seq: str, allele_seq: str) -> NovelVariant:
    """REF = the allele's base at the position; ALT = the variant's value (fp / novel) or the backbone's base (fn);
    ``""`` for indels (147-169).  An indel is never applied, and in gapless backbone coordinates its position may hold
    the same base in the allele and the backbone (an insertion the allele carries, ``fn``), so the reference's
    ``base_ref != base_alt`` check -- true in MSA coordinates -- is kept for SNVs only."""
    v = variant["variant"]
    base_ref = allele_seq[v.pos]
    if variant["type"] not in ("fp", "novel", "fn"):
        raise NotImplementedError
    if v.typ != "single":
        base_alt = ""
    else:
        base_alt = str(v.val) if variant["type"] in ("fp", "novel") else backbone_seq[v.pos]
        assert base_ref != base_alt
    variant["base_ref"] = base_ref
    variant["base_alt"] = base_alt
    return variant


def applyNovelVariant(backbone_seq: str, allele_seq: str, novel_variants: list[NovelVariant]) -> str:
    """The kept SNVs written into the allele's sequence; indels are marked skipped (172-213)."""
    for variant in novel_variants:
        if variant["skip"]:
            continue
        v = variant["variant"]
        pos = v.pos
        logger.debug(f"  Apply {v.ref}:{v.pos} {v.val} ({v.typ}) id={v.id}")
        logger.debug(f"    Reference {backbone_seq[max(pos - 5, 0):pos + 6]}")
        logger.debug(f"    Before:   {allele_seq[max(pos - 5, 0):pos + 6]}")
        if v.typ != "single":
            logger.debug("    -> Skip (Not implement indel)")
            variant["skip"] = True
            variant["skip_reason"] = "Not implement indel"
            continue
        allele_seq = allele_seq[:pos] + variant["base_alt"] + allele_seq[pos + 1:]
        logger.debug(f"    -> After: {allele_seq[max(pos - 5, 0):pos + 6]}")
    return allele_seq


def groupReadToBam(input_bam: str, output_bam: str, assign_reads: GroupPairRead) -> None:
    """The grouped reads as a BAM (216-234): the input's header, one ``@RG ID:a,b`` per group, both lines of every
    pair tagged ``RG:Z:a,b``; coordinate sorted and indexed."""
    from .hisat2 import PairsText
    lines, group = [], []
    for k, reads in enumerate(assign_reads.values()):
        for r in reads:
            lines += [r.l_sam, r.r_sam]
            group += [k, k]
    text = PairsText(("\n".join(lines) + "\n").encode() if lines else b"", np.arange(len(lines)).reshape(-1, 2))
    writeGroupedBam(input_bam, output_bam, [",".join(a) for a in assign_reads], text,
                    np.arange(len(lines), dtype=np.int64), np.asarray(group, dtype=np.int32))


def countFilterPileup(pileup_read_base: dict[str, str], reads: list[PairRead]) -> dict[str, int]:
    """Bases of the named reads only (253-264)."""
    selected = set(read.l_sam.split("\t", 1)[0] for read in reads)
    return Counter(b for name, b in pileup_read_base.items() if name in selected)


def splitReadsByAlleles(pn_typing_model, predict_alleles: list[str]
                        ) -> Iterable[tuple[str, tuple[str, ...], list[PairRead], dict[str, Variant]]]:
    """Per gene (first appearance among the NH == 1 reads), the model ``AlleleTyping(reads, variants, no_empty=False)``
    with the error correction applied to the reads, and its groups (267-277)."""
    from .kir_typing import _GeneView
    from .typing_mulit_allele import AlleleTyping, ReadSet
    data = pn_typing_model._data
    tab = data.tab
    for g, rows, n in _genesInOrder(tab, data.index):
        view = _GeneView(data, data.index.genes[g], False, tab=tab)
        typ = AlleleTyping(ReadSet(tab, rows, n), view.variants, no_empty=False, variant_correction=True,
                           _vbeg=view.vbeg, _n_span=view.n_span, _mask=view.mask, _alleles=view.alleles,
                           _novel=view.novel)
        reads = typ.reads
        assert typ.probs.shape[0] == len(reads)
        for alleles, group in groupReadByAllele(typ, predict_alleles, reads).items():
            yield view.gene, alleles, group, typ.variants


# ---- allele sequences from the index
def readBackbone(index: str) -> dict[str, str]:
    """``{index}_backbone.fa`` -> {backbone name: sequence}."""
    seqs: dict[str, list[str]] = {}
    name = None
    with open(index + "_backbone.fa") as f:
        for line in f:
            line = line.strip()
            if line.startswith(">"):
                name = line[1:].split()[0]
                seqs[name] = []
            elif name is not None and line:
                seqs[name].append(line)
    return {k: "".join(v) for k, v in seqs.items()}


def alleleSequence(backbone_seq: str, variants: list[Variant], allele: str) -> tuple[str, dict[int, str]]:
    """(the allele's base at every backbone position, its insertions by position): its own ``single`` value, ``-``
    where one of its deletions covers the position, the backbone's base elsewhere."""
    seq = list(backbone_seq)
    ins: dict[int, str] = {}
    for v in variants:
        if allele not in v.allele:
            continue
        if v.typ == "single":
            seq[v.pos] = str(v.val)
        elif v.typ == "deletion":
            for p in range(v.pos, min(v.pos + int(v.val), len(seq))):
                seq[p] = "-"
        elif v.typ == "insertion":
            ins[v.pos] = ins.get(v.pos, "") + str(v.val)
    return "".join(seq), ins


def gaplessSequence(allele_seq: str, insertions: dict[int, str]) -> str:
    """The allele as one sequence: insertions before the base at their position, deleted positions left out."""
    parts = []
    for p, b in enumerate(allele_seq):
        if p in insertions:
            parts.append(insertions[p])
        if b != "-":
            parts.append(b)
    parts += [s for p, s in sorted(insertions.items()) if p >= len(allele_seq)]
    return "".join(parts)


# ---- native host pieces
def nameKeys(text, line_idx: np.ndarray) -> np.ndarray:
    """FNV-1a 64 of the query names of the given lines of a ``PairsText`` (``gk_sam_name_keys``)."""
    from ._lib import check, lib
    idx = np.ascontiguousarray(line_idx, dtype=np.int64)
    out = np.empty(len(idx), dtype=np.uint64)
    check(lib().gk_sam_name_keys(text.blob, len(text.blob), idx.ctypes.data if len(idx) else None, len(idx),
                                 out.ctypes.data if len(idx) else None))
    return out


def nameKey(name: str) -> int:
    """FNV-1a 64 of one name (what ``gk_sam_name_keys`` computes)."""
    h = 1469598103934665603
    for b in name.encode():
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def pileupSites(bam_path: str, sites: np.ndarray, name_keys: np.ndarray, key_group: np.ndarray,
                site_group: np.ndarray) -> np.ndarray:
    """uint32 [n_sites][6] (A, C, G, T, N, *) counts of the group's reads at (reference ordinal, 0-based position)
    sites (``gk_bam_pileup_sites``; the rules are listed in csrc/gk_bamread.cpp)."""
    from ._lib import check, lib
    sites = np.ascontiguousarray(sites, dtype=np.int64).reshape(-1, 2)
    keys = np.ascontiguousarray(name_keys, dtype=np.uint64)
    kg = np.ascontiguousarray(key_group, dtype=np.int32)
    sg = np.ascontiguousarray(site_group, dtype=np.int32)
    out = np.zeros((len(sites), 6), dtype=np.uint32)
    if len(sites):
        check(lib().gk_bam_pileup_sites(bam_path.encode(), sites.ctypes.data, len(sites),
                                        keys.ctypes.data if len(keys) else None, kg.ctypes.data if len(kg) else None,
                                        len(keys), sg.ctypes.data, out.ctypes.data))
    return out


def writeGroupedBam(input_bam: str, output_bam: str, tags: list[str], text, line_idx: np.ndarray,
                    line_group: np.ndarray) -> None:
    """``gk_bam_write_lines_tagged``: the input's header + one ``@RG`` per tag, line i tagged ``RG:Z:tags[group[i]]``."""
    from ._lib import check, lib
    from .hisat2 import alignmentHeader
    assert output_bam.endswith(".bam")
    header = alignmentHeader(input_bam).encode()
    rg = "".join(f"@RG\tID:{t}\n" for t in tags).encode()
    idx = np.ascontiguousarray(line_idx, dtype=np.int64)
    grp = np.ascontiguousarray(line_group, dtype=np.int32)
    tag_arr = (C.c_char_p * max(len(tags), 1))(*[t.encode() for t in tags])
    check(lib().gk_bam_write_lines_tagged(output_bam.encode(), header, len(header), rg, len(rg), text.blob, len(text.blob),
                                          idx.ctypes.data if len(idx) else None, grp.ctypes.data if len(grp) else None,
                                          len(idx), tag_arr, len(tags), 1))


# ---- the device path
def _genesInOrder(tab, index):
    """(backbone ordinal, NH == 1 rows on the device, their count) of every backbone with reads, in order of first
    appearance (groupReads keeps the read order, kir_typing.py:15-20)."""
    out = []
    for g in range(len(index.genes)):
        rows, n = tab.selectGene(g, multiple=False)
        if n:
            out.append((int(rows.download(1)[0]), g, rows, n))
        else:
            rows.free()
    out.sort(key=lambda x: x[0])
    return [(g, rows, n) for _, g, rows, n in out]


class GeneGroups:
    """The groups of one gene: called entries, per-group rows and counts, and for every singleton group its totals and
    its candidates (stat, variant, count) in the reference's order."""

    def __init__(self, gene: str):
        self.gene = gene
        self.groups: list[tuple[str, ...]] = []       # first-appearance order
        self.codes: list[int] = []                   # entry bitmask of each group
        self.sizes: list[int] = []
        self.rows: np.ndarray = np.zeros(0, np.int32)   # the gene's rows (tabulation order) ...
        self.row_code: np.ndarray = np.zeros(0, np.uint16)   # ... and each one's group code
        self.totals: dict[tuple[str, ...], dict[str, int]] = {}
        self.candidates: dict[tuple[str, ...], list[tuple[str, Variant, int]]] = {}


class NovelDiscovery:
    """Assignment and confusion counts of every gene of a sample that is in HBM (``SampleData``), for the given calls."""

    def __init__(self, data, tab=None):
        self.data = data
        self.tab = tab or data.tab
        self.dev = self.tab.dev

    def _vflag(self, rows, n, vbeg, vend):
        """The drop flags of the error correction (typing_mulit_allele.py:302-338): the sample's prepared ones when the
        typing made them, otherwise one pass over the gene's rows."""
        prep = self.tab.prepared(self.dev, False)
        if prep is not None:
            return prep.vflag
        vflag = self.dev.alloc(max(self.tab.n_var_total, 1), np.uint8).zero()
        self.tab.errorCorrection(rows, n, vflag, span=(vbeg, vend))
        return vflag

    def run(self, predict_alleles: list[str]) -> list[GeneGroups]:
        from ._lib import check, lib
        data, tab, dev = self.data, self.tab, self.dev
        idx = data.index
        n_index = idx.n_variant if tab.dindex is None else tab.dindex.host.n_variant
        out = []
        for g, rows, n in _genesInOrder(tab, idx):
            gene = idx.genes[g]
            gg = GeneGroups(gene)
            out.append(gg)
            t = idx.tables[g]
            col_of = {a: i for i, a in enumerate(t.alleles)}
            entries = [a for a in predict_alleles if a in col_of]
            if not entries:
                continue
            if len(entries) > MAX_ENTRIES:
                raise ValueError(f"{gene}: {len(entries)} called alleles; novel discovery supports {MAX_ENTRIES} per gene")
            distinct = list(dict.fromkeys(entries))
            col_entries = np.zeros(len(distinct), dtype=np.uint32)
            entry_col = np.zeros(MAX_ENTRIES, dtype=np.int32)
            for e, a in enumerate(entries):
                k = distinct.index(a)
                col_entries[k] |= np.uint32(1 << e)
                entry_col[e] = k
            # the restricted mask: bit k of a variant's word = the k-th distinct called allele carries it
            carry = np.zeros(max(t.vend - t.vbeg, 1), dtype=np.uint32)
            for k, a in enumerate(distinct):
                c = col_of[a]
                carry[:t.vend - t.vbeg] |= ((t.mask[:, c >> 5] >> np.uint32(c & 31)) & np.uint32(1)) << np.uint32(k)
            d_carry = dev.put(carry)
            vflag = self._vflag(rows, n, t.vbeg, t.vend)
            K = len(distinct)
            probs = dev.alloc((K, n), np.float64)
            check(lib().gk_compat(dev.ctx, tab.handle, rows.ptr, n, vflag.ptr, t.vbeg, t.vend, d_carry.ptr, 1, K, 1,
                                  probs.ptr, 0, 0))
            d_code = dev.alloc(n, np.uint16)
            code = np.empty(n, dtype=np.uint16)
            count = np.empty(1 << K, dtype=np.uint32)
            first = np.empty(1 << K, dtype=np.int32)
            check(lib().gk_novel_assign(dev.ctx, probs.ptr, n, K, col_entries.ctypes.data, len(entries), d_code.ptr,
                                        code.ctypes.data, count.ctypes.data, first.ctypes.data))
            probs.free()
            gg.rows, gg.row_code = rows.download(n), code
            live = sorted((int(first[dc]), dc) for dc in np.flatnonzero(count))
            for _, dc in live:
                ec = 0
                for k in range(K):
                    if dc >> k & 1:
                        ec |= int(col_entries[k])
                gg.codes.append(ec)
                gg.groups.append(tuple(sorted(entries[e] for e in range(len(entries)) if ec >> e & 1)))
                gg.sizes.append(int(count[dc]))
            # singleton groups: their entry gets an output slot
            entry_slot = np.full(MAX_ENTRIES, -1, dtype=np.int32)
            singles = [ec for ec in gg.codes if bin(ec).count("1") == 1]
            for s, ec in enumerate(singles):
                entry_slot[ec.bit_length() - 1] = s
            if singles:
                totals = np.zeros((len(singles), 5), dtype=np.uint64)
                cap = 1 << 12
                while True:
                    slot_o, ord_o = np.empty(cap, np.int32), np.empty(cap, np.int32)
                    cnt_o, key_o = np.empty(cap, np.uint32), np.empty(cap, np.uint64)
                    n_out = C.c_int64()
                    rc = lib().gk_novel_confusion(dev.ctx, tab.handle, rows.ptr, n, d_code.ptr, vflag.ptr, t.vbeg, t.vend,
                                                  d_carry.ptr, entry_col.ctypes.data, entry_slot.ctypes.data,
                                                  len(entries), len(singles), totals.ctypes.data, cap, slot_o.ctypes.data,
                                                  ord_o.ctypes.data, cnt_o.ctypes.data, key_o.ctypes.data, C.byref(n_out))
                    if rc == -5 and n_out.value > cap:
                        cap = int(n_out.value)
                        continue
                    check(rc)
                    break
                m = int(n_out.value)
                slot_o, ord_o, cnt_o, key_o = slot_o[:m], ord_o[:m], cnt_o[:m], key_o[:m]
                local = ord_o.astype(np.int64) - t.vbeg
                in_span = (local >= 0) & (local < t.vend - t.vbeg)
                for s, ec in enumerate(singles):
                    group = gg.groups[gg.codes.index(ec)]
                    k = int(entry_col[ec.bit_length() - 1])
                    tot = {st: int(totals[s, j]) for j, st in enumerate(STATS)}
                    gg.totals[group] = {"total": tot["tp"] + tot["tn"] + tot["fp"] + tot["fn"], **tot}
                    sel = np.flatnonzero(slot_o == s)
                    has = np.zeros(len(sel), dtype=bool)
                    isp = in_span[sel]
                    has[isp] = (carry[local[sel][isp]] >> np.uint32(k)) & np.uint32(1) != 0
                    stat = np.where(~isp, 0, np.where(has, 2, 1))       # 0 novel, 1 fp, 2 fn
                    order = np.lexsort((key_o[sel], stat))
                    cands = []
                    for j in order:
                        o = int(ord_o[sel[j]])
                        v = idx.variants[o] if o < n_index else data.novel[o - n_index]
                        cands.append((CANDIDATE_STATS[int(stat[j])], v, int(cnt_o[sel[j]])))
                    gg.candidates[group] = cands
            d_code.free()
            d_carry.free()
            rows.free()
        return out


def _pairsText(data):
    """The SAM lines of the sample's pairs (``PairsText``) and the source pair of every tabulated row."""
    from .hisat2 import PairsText
    tab = data.tab
    text = data.pairs_text
    if text is None and data._reads is not None:       # a loaded hand-off: the lines are in the reads
        reads = data._reads
        blob = ("".join(f"{r.l_sam}\n{r.r_sam}\n" for r in reads)).encode()
        text = PairsText(blob, np.arange(2 * len(reads)).reshape(-1, 2))
        return text, np.arange(len(reads))
    if text is None:
        raise ValueError("novel discovery needs the SAM lines of the sample's pairs (keep_text)")
    if not isinstance(text, PairsText):
        blob = ("".join(f"{a}\n{b}\n" for a, b in text)).encode()
        text = PairsText(blob, np.arange(2 * len(text)).reshape(-1, 2))
    src = tab.pairSrc() if tab.info.d_pair_src else np.arange(tab.n_valid)
    return text, src


def discoverSample(data, predict_alleles: list[str], msa_name: str, bam_name: str, output_name: str,
                   novel_descr: TextIO | None = None, apply: bool = True, tab=None) -> list[dict]:
    """The body of ``discoverNovel`` for a sample in HBM: ``bam_name`` is the ``.no_multi.bam`` the reads are piled up
    from (and whose header the grouped BAM gets).  Writes ``{output_name}.variant.tsv`` (and with ``apply`` the
    ``.tsv``, ``.fa`` and ``.bam``); returns the rows of the variant table."""
    import io
    descr = novel_descr if novel_descr is not None else io.StringIO()
    genes = NovelDiscovery(data, tab).run(predict_alleles)
    text, src = _pairsText(data)
    pair_lines = text.pair_lines
    idx = data.index
    backbone = readBackbone(msa_name) if any(gg.totals for gg in genes) else {}
    ref_of = {name: i for i, name in enumerate(_bamRefs(bam_name))}

    # ---- candidates of every singleton group, the count filter, and ONE pileup call for all that remain
    work = []          # (gene groups, group, allele, allele_count, allele_seq, insertions, candidates)
    allele_count: dict[str, int] = defaultdict(int)
    site_list, site_group, site_of = [], [], []
    key_parts, key_grp = [], []
    for gi, gg in enumerate(genes):
        for group, ec in zip(gg.groups, gg.codes):
            if len(group) > 1:
                continue
            allele = group[0]
            allele_count[gg.gene] += 1
            t = idx.tables[idx.gene_id[gg.gene]]
            allele_seq, ins = alleleSequence(backbone[gg.gene], idx.variants[t.vbeg:t.vend], allele)
            nvs: list[NovelVariant] = []
            for stat, v, c in gg.candidates.get(group, []):
                nvs.append({"gene": gg.gene, "allele": allele, "allele_count": allele_count[gg.gene], "type": stat,
                            "variant": v, "pos": int(v.pos), "count": c, "skip": False, "skip_reason": "",
                            "base_ref": "", "base_alt": "", "pileup": {}})
            for nv in nvs:
                if nv["count"] < 3:
                    nv["skip"] = True
                    nv["skip_reason"] = "Number of variant too low"
            w = len(work)
            work.append((gg, group, ec, allele, allele_seq, ins, nvs))
            member = gg.row_code == ec
            lines = pair_lines[src[gg.rows[member]], 0]
            key_parts.append(nameKeys(text, lines))
            key_grp.append(np.full(len(lines), w, dtype=np.int32))
            for j, nv in enumerate(nvs):
                if not nv["skip"]:
                    site_list.append((ref_of.get(gg.gene, -1), nv["pos"]))
                    site_group.append(w)
                    site_of.append((w, j))
    counts = pileupSites(bam_name, np.asarray(site_list, dtype=np.int64).reshape(-1, 2),
                         np.concatenate(key_parts) if key_parts else np.zeros(0, np.uint64),
                         np.concatenate(key_grp) if key_grp else np.zeros(0, np.int32),
                         np.asarray(site_group, dtype=np.int32))
    for (w, j), c in zip(site_of, counts):
        nv = work[w][6][j]
        nv["pileup"] = Counter({b: int(n) for b, n in zip("ACGTN", c[:5]) if n})

    rows_out: list[dict] = []
    records = []       # (name, description, sequence)
    for gg, group, ec, allele, allele_seq, ins, nvs in work:
        reads_n = gg.sizes[gg.codes.index(ec)]
        nogap = gaplessSequence(allele_seq, ins)
        backbone_seq = backbone[gg.gene]
        print(f"{gg.gene} - {allele}", file=descr)
        print(f"  Length: {len(nogap)}", file=descr)
        print(f"  Avg depth: {reads_n / len(nogap) * 150 * 2}", file=descr)
        confusion = gg.totals[group]
        print("  Total reads:", reads_n, file=descr)
        print("  Total variants:", confusion["total"], file=descr)
        for stat, c in confusion.items():
            print(f"    {stat}:", c, file=descr)
        for nv in nvs:
            if not nv["skip"] and not nv["pileup"]:
                nv["skip"] = True
                nv["skip_reason"] = "Pileup empty"
        for nv in nvs:
            if nv["skip"]:
                continue
            updateBaseRefAlt(nv, backbone_seq, allele_seq)
            if nv["pileup"].get(nv["base_alt"], 0) < max(nv["pileup"].values()):
                nv["skip"] = True
                nv["skip_reason"] = "ALT depths < REF depths"
        if any(not nv["skip"] for nv in nvs):
            print("  List", file=descr)
        for nv in nvs:
            if nv["skip"]:
                continue
            v = nv["variant"]
            print(f"    {nv['type']:5s} {v.ref}:{v.pos} {v.val} ({v.typ}) id={v.id} num={nv['count']} "
                  f"bamPile={nv['pileup']}", file=descr)
        if apply:
            applied = applyNovelVariant(backbone_seq, allele_seq, nvs)
            kept = [nv for nv in nvs if not nv["skip"]]
            print("  Apply variant num:", len(kept), file=descr)
            name = allele + "".join(f"-{nv['pos']}{nv['base_alt']}" for nv in kept)
            desc = ",".join(f"{allele}:{nv['pos']}{nv['base_ref']}>{nv['base_alt']}" for nv in kept)
            records.append((name, desc, gaplessSequence(applied, ins)))
        for nv in nvs:
            row = {k: nv[k] for k in ("gene", "allele", "allele_count", "type", "pos", "count", "skip", "skip_reason",
                                      "base_ref", "base_alt")}
            row["pileup"] = repr(nv["pileup"])       # the Counter of the pileup, {} when none was taken
            v = nv["variant"]
            row.update(variant_type=v.typ, variant_id=v.id, variant_val=v.val)
            rows_out.append(row)

    import pandas as pd
    df = pd.DataFrame(rows_out, columns=COLUMNS)
    print(df, file=descr)
    df.to_csv(output_name + ".variant.tsv", index=False, sep="\t")
    if apply:
        pd.DataFrame([{"name": output_name, "alleles": "_".join(r[0] for r in records)}]).to_csv(
            output_name + ".tsv", sep="\t", index=False)
        with open(output_name + ".fa", "w") as f:
            for name, desc, seq in records:
                f.write(f">{name} {desc}\n" if desc else f">{name}\n")
                for i in range(0, len(seq), 60):
                    f.write(seq[i:i + 60] + "\n")
        # the grouped reads: every group of every gene (homozygous and shared groups too), both lines of each pair
        tags, line_idx, line_grp = [], [], []
        for gg in genes:
            for group, ec in zip(gg.groups, gg.codes):
                lines = pair_lines[src[gg.rows[gg.row_code == ec]]].reshape(-1)
                line_idx.append(lines)
                line_grp.append(np.full(len(lines), len(tags), dtype=np.int32))
                tags.append(",".join(group))
        writeGroupedBam(bam_name, output_name + ".bam", tags, text,
                        np.concatenate(line_idx) if line_idx else np.zeros(0, np.int64),
                        np.concatenate(line_grp) if line_grp else np.zeros(0, np.int32))
    return rows_out


def _bamRefs(bam_path: str) -> list[str]:
    """Reference names of a BAM, in header order (the ordinals of ``gk_bam_pileup_sites``)."""
    from .hisat2 import alignmentHeader
    names = []
    for line in alignmentHeader(bam_path).splitlines():
        if line.startswith("@SQ"):
            for f in line.split("\t"):
                if f.startswith("SN:"):
                    names.append(f[3:])
    return names


def discoverNovel(variant_name: str, msa_name: str, result_name: str, output_name: str,
                  novel_descr: TextIO = sys.stdout, apply: bool = True) -> None:
    """Find novel variants of the sample ``variant_name`` against the alleles called in ``{result_name}.tsv``
    (280-434).  ``msa_name`` is the prefix of the HISAT2 index (``{msa_name}_backbone.fa``, ``.snp``, ``.link``);
    ``{variant_name}.json`` is loaded like ``kir_typing`` loads it, and its reads are piled up from
    ``{variant_name}.no_multi.bam``.  The compact ``.npz`` hand-off is refused: it is only written instead of the
    ``.json`` (``--no-variant-json``), so there is no ``.no_multi.bam`` next to it, and it carries no SAM lines."""
    import os
    import pandas as pd
    from .kir_typing import _sample
    result = pd.read_csv(result_name + ".tsv", sep="\t")
    predict_alleles = str(result["alleles"][0]).split("_")
    logger.debug(f"[Novel] {predict_alleles}")
    if not os.path.exists(variant_name + ".json"):
        raise FileNotFoundError(
            f"{variant_name}.json not found: novel discovery needs the .variant.json hand-off and its .no_multi.bam (the "
            f"compact .npz written under --no-variant-json has neither the SAM lines nor the BAM)")
    data = _sample(variant_name + ".json", None)
    try:
        discoverSample(data, predict_alleles, msa_name, variant_name + ".no_multi.bam", output_name, novel_descr, apply)
    finally:
        data.tab.close()
