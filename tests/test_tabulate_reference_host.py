"""``tests/tabulate_reference.py`` earns its authority before it judges the kernels (no GPU): its lists, novel variants,
backbones and NH on packed records must equal ``oracle.tabulate`` on the SAM text of the same sample, and the lists the
reference project itself wrote into the T1 and T12 fixtures (wide pairs included), with and without a pileup correction."""
import gzip
import json
import os
import sys

import numpy as np
import pytest

from kir_graph_amd import packed, pileup, synth
from kir_graph_amd.hisat2 import pairLines
from kir_graph_amd.index import GkIndex
from oracle import pileup as opile, tabulate as ot

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tabulate_reference import CapacityError, hash64, keyFields, tabulateRecords  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TYP_NAME = {0: "insertion", 1: "single", 2: "deletion"}


def lists_of(got, gidx):
    names = [str(v.id) for v in gidx.variants] + [f"nv{r}" for r in range(int(got["counts"][3]))]
    off, ids = got["off"], got["ids"]
    out = []
    for i in range(int(got["counts"][1])):
        o = off[4 * i:4 * i + 5]
        out.append({"lpv": [names[v] for v in ids[o[0]:o[1]]], "rpv": [names[v] for v in ids[o[1]:o[2]]],
                    "lnv": [names[v] for v in ids[o[2]:o[3]]], "rnv": [names[v] for v in ids[o[3]:o[4]]],
                    "multiple": int(got["pair_nh"][i]), "backbone": gidx.genes[int(got["pair_gene"][i])]})
    return out


def novel_of(got, gidx, strings):
    """[(id, pos, typ, ref, val, length)] of the novel keys, in order."""
    out = []
    for rank, k in enumerate(got["novel_key"].tolist()):
        ref, pos, typ, val = keyFields(k)
        if typ == 1:
            val, length = chr(val), 1
        elif typ == 2:
            length = val
        else:
            val = strings[val]
            length = len(val)
        out.append((f"nv{rank}", pos, TYP_NAME[typ], gidx.genes[ref], val, length))
    return out


def assert_same(got, gidx, strings, want_reads, want_novel):
    mine = lists_of(got, gidx)
    assert len(mine) == len(want_reads)
    for i, (g, r) in enumerate(zip(mine, want_reads)):
        for k in ("lpv", "rpv", "lnv", "rnv", "multiple", "backbone"):
            assert g[k] == r[k], (i, k)
    assert novel_of(got, gidx, strings) == want_novel


def oracle_novel(ref):
    return [(v.id, v.pos, v.typ, v.ref, v.val, v.length) for v in ref["variants"] if str(v.id).startswith("nv")]


@pytest.mark.parametrize("seed,err_rate", [(1031, 0.001), (77, 0.01)])
def test_synthetic_samples_equal_the_oracle(small_case, seed, err_rate):
    sidx, gidx, _ = small_case
    sample = synth.makeSample(sidx, seed=seed, n_pairs=4000, err_rate=err_rate)
    rec, table = packed.packSample(sample, gidx)
    got = tabulateRecords(rec, gidx)
    ref = ot.tabulateLines(synth.toSamLines(sample), gidx.variants)
    assert got["counts"][3] > 10 and any(m.get("clipped") for m in got["mates"])
    assert_same(got, gidx, table.strings, ref["reads"], oracle_novel(ref))
    assert got["counts"][1] == len(got["pair_src"]) < got["counts"][0] and got["counts"][2] == got["off"][-1]
    assert not [m for m in got["mates"] if m["walked"] and not m["clipped"] and not m["dropped"]
                and (m["n_pos"] != m["n_events"] or m["n_neg"] > m["hi"] - m["lo"])]


@pytest.mark.parametrize("name", ["t1_tabulation.json.gz", "t12_wide.json.gz"])
def test_fixtures_of_the_reference_project(tmp_path, name):
    with gzip.open(os.path.join(GOLD, name), "rt") as f:
        case = json.load(f)
    for ext, body in case["index"].items():
        (tmp_path / f"ix.{ext}").write_text(body)
    gidx = GkIndex.load(str(tmp_path / "ix"))
    spill: list = []
    rec, table = packed.packPairs(pairLines(case["lines"]), gidx, spill=spill)
    got = tabulateRecords(rec, gidx, spill=packed.spillArrays(spill))
    if name.startswith("t12"):
        assert len(spill) >= 8
        want_novel = [(i, p, t, r, v, n) for i, t, p, v, n, r in case["novel"]]
    else:
        assert not spill and any(m.get("dropped") for m in got["mates"])      # the novel-indel rule is in T1
        want_novel = [(v[0], v[2], v[1], None, v[3], v[4]) for v in case["variants"] if v[0].startswith("nv")]
    mine = novel_of(got, gidx, table.strings)
    if not name.startswith("t12"):      # T1 lists its variants without the backbone
        mine = [(i, p, t, None, v, n) for i, p, t, _, v, n in mine]
    assert mine == want_novel and len(mine) > 1
    got_reads = lists_of(got, gidx)
    assert len(got_reads) == len(case["reads"])
    for i, (g, r) in enumerate(zip(got_reads, case["reads"])):
        for k in ("lpv", "rpv", "lnv", "rnv", "multiple", "backbone"):
            assert g[k] == r[k], (i, k)


def test_pileup_correction_equals_the_oracle():
    """The sample of test_pileup_error_correction_matches_oracle on shorter backbones (400 pairs reach the depth of 20
    the correction asks for)."""
    sidx = synth.makeIndex(seed=21, n_genes=3, len_range=(1200, 1500), var_range=(200, 300), allele_range=(10, 20))
    gidx = GkIndex.fromVariants(sidx.variants, genes=sidx.genes, exons=sidx.exons)
    sample = synth.makeSample(sidx, seed=77, n_pairs=400, err_rate=0.01)
    lines = synth.toSamLines(sample)
    by_coord = sorted(lines, key=lambda l: (l.split("\t")[2], int(l.split("\t")[3])))
    pile = opile.pileupOfLines(by_coord)
    correction = pileup.correctionFromRatios(pile, gidx)
    assert correction[0].any()
    rec, table = packed.packSample(sample, gidx)
    plain = tabulateRecords(rec, gidx)
    got = tabulateRecords(rec, gidx, correction=correction)
    assert got["counts"][3] < plain["counts"][3] and not np.array_equal(got["ids"], plain["ids"])
    ref = ot.tabulateLines(lines, gidx.variants, pileup=pile)
    assert_same(got, gidx, table.strings, ref["reads"], oracle_novel(ref))


def test_a_mate_beyond_its_format_raises(small_case):
    from kir_graph_amd._lib import CIG_D, CIG_I, CIG_M, MATE_DTYPE
    _, gidx, _ = small_case
    rec = np.zeros(2, dtype=MATE_DTYPE)
    rec["flag"], rec["n_cig"] = 3, 1
    rec["cig"][:, 0] = (100 << 4) | CIG_M
    ops = [(80 << 4) | CIG_M] + [(1 << 4) | (CIG_I if k % 2 == 0 else CIG_D) for k in range(7)]
    rec["cig"][1, :8] = ops
    rec["n_cig"][1], rec["n_mm"][1], rec["n_ins"][1] = 8, 16, 4
    rec["mm"]["ref_off"][1], rec["mm"]["base"][1] = 5 * np.arange(16), ord("A")
    with pytest.raises(CapacityError):
        tabulateRecords(rec, gidx)
    rec["n_mm"][1] = 15      # 22 events: the format's limit
    got = tabulateRecords(rec, gidx)
    assert got["mates"][1]["n_events"] == 22 and got["mates"][1]["dropped"]


def test_restated_hash():
    """Murmur3's 64-bit finaliser, low word: fixed points of the definition."""
    assert hash64(0) == 0
    assert hash64(1) == 0xB456BCFC34C2CB2C & 0xFFFFFFFF
